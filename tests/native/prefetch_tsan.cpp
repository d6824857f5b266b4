// Stand-alone driver of csrc/round_prefetch.h for a thread-sanitizer build
// (tests/test_sched_prefetch.py compiles and runs it): a fake producer, with
// in-order takes, a producer that throws, draining, and destruction while
// the worker is producing. Exits 0 when every check holds.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../gossipy_amd/csrc/round_prefetch.h"

struct Round {
    int64_t r = -1;
    std::vector<int> payload;
};

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__,  \
                         #cond);                                           \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

int main()
{
    // producer state only the worker touches, like the scheduler's
    {
        int64_t state = 0;
        std::atomic<int64_t> produced{0};
        RoundPrefetch<Round> pf(
            [&](int64_t r) {
                state += r;  // must see rounds 5, 6, 7, ... in order
                Round out;
                out.r = r;
                out.payload.assign(64, (int)state);
                ++produced;
                return out;
            },
            5);
        int64_t expect = 0;
        for (int64_t r = 5; r < 200; ++r) {
            CHECK(pf.next() == r);
            Round got = pf.take(r);
            expect += r;
            CHECK(got.r == r);
            CHECK(got.payload.size() == 64 && got.payload[63] == (int)expect);
            // never more than `depth` finished rounds plus one in the making
            CHECK(produced.load() <= (r - 5 + 1) + 3);
        }
        bool threw = false;
        try {
            pf.take(7);  // out of order
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        std::vector<Round> rest = pf.drain();
        CHECK(rest.size() <= 3);
        for (size_t i = 0; i < rest.size(); ++i)
            CHECK(rest[i].r == 200 + (int64_t)i);
    }
    // a producer that throws: finished rounds first, then the exception
    {
        RoundPrefetch<Round> pf(
            [](int64_t r) {
                if (r == 3) throw std::runtime_error("round 3 is broken");
                Round out;
                out.r = r;
                return out;
            },
            0);
        for (int64_t r = 0; r < 3; ++r) CHECK(pf.take(r).r == r);
        for (int rep = 0; rep < 2; ++rep) {
            bool threw = false;
            try {
                pf.take(3);
            } catch (const std::runtime_error&) {
                threw = true;
            }
            CHECK(threw);
        }
    }
    // destruction while the worker is in produce(), after 0, 1 or 3 takes
    for (int rep = 0; rep < 60; ++rep) {
        RoundPrefetch<Round> pf(
            [](int64_t r) {
                std::this_thread::sleep_for(std::chrono::microseconds(200));
                Round out;
                out.r = r;
                return out;
            },
            0);
        int takes = rep % 3 == 2 ? 3 : rep % 3;
        for (int64_t r = 0; r < takes; ++r) CHECK(pf.take(r).r == r);
    }
    std::puts("prefetch_tsan OK");
    return 0;
}
