// Stand-alone driver of two chained RoundPrefetch workers for a
// thread-sanitizer build (tests/test_round_driver.py compiles and runs it),
// arranged as NativeScheduler::set_prefetch arranges them: a generator whose
// produce() owns all the state, and a packer whose produce() takes the
// generator's round and transforms it. Cases: in-order takes through the
// chain, draining (packer first, then the generator) while the packer is
// blocked in the generator's take(), destruction in that order while both
// work, and a generator that throws. Exits 0 when every check holds.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../gossipy_amd/csrc/round_prefetch.h"

struct Round {
    int64_t r = -1;
    std::vector<int> events;  // the generator's part
    std::vector<int> packed;  // the packer's part
};

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__,  \
                         #cond);                                           \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static void pack(Round& d)
{
    d.packed.assign(d.events.rbegin(), d.events.rend());
}

static void check_round(const Round& d, int64_t r, bool packed)
{
    CHECK(d.r == r);
    CHECK(d.events.size() == 32 && d.events[0] == (int)(r * (r + 1) / 2));
    CHECK(d.packed.size() == (packed ? 32u : 0u));
    if (packed) CHECK(d.packed[31] == d.events[0]);
}

struct Chain {
    int64_t state = 0;  // only the generator's worker touches it
    int gen_sleep_us;
    int64_t fail_at;
    std::unique_ptr<RoundPrefetch<Round>> gen, packer;  // gen outlives packer

    Chain(int64_t first, int gen_sleep_us_ = 0, int64_t fail_at_ = -1)
        : gen_sleep_us(gen_sleep_us_), fail_at(fail_at_)
    {
        state = first * (first - 1) / 2;
        gen = std::make_unique<RoundPrefetch<Round>>(
            [this](int64_t r) {
                if (r == fail_at) throw std::runtime_error("generator failed");
                if (gen_sleep_us)
                    std::this_thread::sleep_for(
                        std::chrono::microseconds(gen_sleep_us));
                state += r;  // rounds must arrive in order
                Round d;
                d.r = r;
                d.events.assign(32, (int)state);
                return d;
            },
            first);
        RoundPrefetch<Round>* g = gen.get();
        packer = std::make_unique<RoundPrefetch<Round>>(
            [g](int64_t r) {
                Round d = g->take(r);
                pack(d);
                return d;
            },
            first);
    }

    ~Chain()
    {
        packer.reset();
        gen.reset();
    }
};

int main()
{
    // in order through both stages
    {
        Chain c(3);
        for (int64_t r = 3; r < 300; ++r) check_round(c.packer->take(r), r, true);
        bool threw = false;
        try {
            c.packer->take(400);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        check_round(c.packer->take(300), 300, true);
    }

    // drain while the packer waits for a slow generator: the packer's
    // rounds come back packed, the generator's unpacked and consecutive,
    // and generation can go on from there synchronously
    for (int rep = 0; rep < 20; ++rep) {
        Chain c(0, 200);
        int64_t taken = rep % 4;
        for (int64_t r = 0; r < taken; ++r) check_round(c.packer->take(r), r, true);
        std::vector<Round> rest = c.packer->drain();
        std::vector<Round> unpacked = c.gen->drain();
        int64_t r = taken;
        for (auto& d : rest) check_round(d, r++, true);
        for (auto& d : unpacked) {
            check_round(d, r, false);
            pack(d);
            check_round(d, r++, true);
        }
        CHECK(r - taken <= 5);  // two per stage, one in the packer's hands
        // the generator's state stands right after the last round it made
        CHECK(c.state == r * (r - 1) / 2);
    }

    // destruction while both workers are busy, at various moments
    for (int rep = 0; rep < 50; ++rep) {
        Chain c(10, rep % 3 ? 50 : 0);
        for (int64_t r = 10; r < 10 + rep % 5; ++r)
            check_round(c.packer->take(r), r, true);
    }

    // a generator that throws: the rounds before it arrive, then the error
    // comes through the packer to the consumer; teardown stays clean
    {
        Chain c(0, 0, 4);
        for (int64_t r = 0; r < 4; ++r) check_round(c.packer->take(r), r, true);
        bool threw = false;
        try {
            c.packer->take(4);
        } catch (const std::runtime_error& e) {
            threw = std::string(e.what()) == "generator failed";
        }
        CHECK(threw);
    }

    std::printf("prefetch_chain_tsan OK\n");
    return 0;
}
