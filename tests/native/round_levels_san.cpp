// Stand-alone driver of csrc/round_levels.h for an address/undefined-
// behaviour sanitizer build (tests/test_level_pack.py compiles and runs
// it). It feeds one LevelPacker a few hundred small random rounds, among
// them empty ones, a single node, rounds that only deliver carried slots,
// and every shape the packer has to refuse. For a round it packs it checks
// that every delivery and every snapshot appears exactly once, that a
// receiver's deliveries keep their order, that no row is longer than the
// cap and that no launch reads a slot it writes or that a later launch
// writes. For a round it refuses it checks that the output was left alone.
// Exits 0 when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../gossipy_amd/csrc/round_levels.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__,  \
                         #cond);                                           \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x2545F4914F6CDD1DULL;
static uint32_t rnd(uint32_t n)  // [0, n)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % (n ? n : 1));
}

struct Flat {
    std::vector<int32_t> snap_nodes, snap_slots, snap_tptr{0};
    std::vector<int32_t> recv_nodes, recv_nptr{0}, recv_tptr{0};
    std::vector<int32_t> del_slots, reply_slots, del_pids, del_owners;
    std::vector<int32_t> pull_nodes, rep_nodes;
    int64_t n_nodes = 0, n_slots = 0;
};

// A well-formed PUSH round: n_carried slots are in flight from earlier
// rounds; every tick some nodes snapshot into fresh slots and some slots in
// flight are delivered. snap_p is the chance (in 1/8) that a node snapshots
// in a tick: high values make double snapshots, which the packer refuses.
static Flat random_round(int n_nodes, int n_ticks, int n_carried, int snap_p,
                         int deliver_p, bool extras)
{
    Flat f;
    f.n_nodes = n_nodes;
    std::vector<int32_t> flying;
    int32_t next_slot = 0;
    for (int i = 0; i < n_carried; ++i) flying.push_back(next_slot++);
    for (int t = 0; t < n_ticks; ++t) {
        for (int x = 0; x < n_nodes; ++x)
            if ((int)rnd(8) < snap_p) {
                f.snap_nodes.push_back(x);
                f.snap_slots.push_back(next_slot);
                flying.push_back(next_slot++);
            }
        f.snap_tptr.push_back((int32_t)f.snap_nodes.size());
        // this tick's deliveries, grouped by receiver in order of arrival
        std::vector<int32_t> order;
        std::map<int32_t, std::vector<int32_t>> rows;
        for (size_t i = 0; i < flying.size();) {
            if ((int)rnd(8) < deliver_p && n_nodes > 0) {
                int32_t x = (int32_t)rnd((uint32_t)n_nodes);
                if (!rows.count(x)) order.push_back(x);
                rows[x].push_back(flying[i]);
                flying.erase(flying.begin() + (long)i);
            } else {
                ++i;
            }
        }
        for (int32_t x : order) {
            f.recv_nodes.push_back(x);
            for (int32_t s : rows[x]) {
                f.del_slots.push_back(s);
                f.reply_slots.push_back(-1);
                if (extras) {
                    f.del_pids.push_back(s % 4);
                    f.del_owners.push_back((s * 7) % n_nodes);
                }
            }
            f.recv_nptr.push_back((int32_t)f.del_slots.size());
        }
        f.recv_tptr.push_back((int32_t)f.recv_nodes.size());
    }
    f.n_slots = next_slot;
    return f;
}

static const char* run(LevelPacker& lp, const Flat& f, int cap,
                       PackedRound* out)
{
    return lp.pack(f.snap_nodes, f.snap_slots, f.snap_tptr, f.recv_nodes,
                   f.recv_nptr, f.recv_tptr, f.del_slots, f.reply_slots,
                   f.del_pids, f.pull_nodes, f.rep_nodes, f.del_owners,
                   f.n_nodes, f.n_slots, cap, out);
}

static PackedRound sentinel()
{
    PackedRound p;
    p.snap_nodes = {-77};
    return p;
}

static bool untouched(const PackedRound& p)
{
    return p.snap_nodes.size() == 1 && p.snap_nodes[0] == -77 &&
           p.recv_nodes.empty() && p.pull_tptr.empty();
}

static void check_packed(const Flat& f, const PackedRound& p, int cap)
{
    const size_t n_del = f.del_slots.size();
    const size_t groups = p.snap_tptr.size() - 1;
    CHECK(p.recv_tptr.size() == groups + 1);
    CHECK(p.rep_tptr.size() == groups + 1);
    CHECK(p.pull_tptr.size() == groups + 1);
    CHECK(p.rep_nodes.empty() && p.rep_slots.empty());
    CHECK(p.del_slots.size() == n_del && p.reply_slots.size() == n_del);
    CHECK(p.recv_nptr.size() == p.recv_nodes.size() + 1);
    CHECK(p.recv_nptr.back() == (int32_t)n_del);
    CHECK(p.recv_tptr.back() == (int32_t)p.recv_nodes.size());
    CHECK(p.del_pids.size() == f.del_pids.size());
    CHECK(p.del_owners.size() == f.del_owners.size());
    if (f.snap_nodes.empty() && n_del == 0) CHECK(groups == 0);
    // the one snapshot launch opens the round
    for (size_t g = 1; g <= groups; ++g)
        CHECK(p.snap_tptr[g] == (int32_t)p.snap_nodes.size());

    // every snapshot once: at the head of the round or as a reply slot
    std::vector<int> snapped((size_t)f.n_slots, 0), want((size_t)f.n_slots, 0);
    for (int32_t s : f.snap_slots) ++want[(size_t)s];
    for (int32_t s : p.snap_slots) ++snapped[(size_t)s];
    for (int32_t s : p.reply_slots)
        if (s >= 0) ++snapped[(size_t)s];
    CHECK(snapped == want);

    // what each receiver gets, in order, in the flat round ...
    std::vector<std::vector<int32_t>> flat_seq((size_t)f.n_nodes),
        pack_seq((size_t)f.n_nodes);
    for (size_t r = 0; r < f.recv_nodes.size(); ++r)
        for (int32_t d = f.recv_nptr[r]; d < f.recv_nptr[r + 1]; ++d)
            flat_seq[(size_t)f.recv_nodes[r]].push_back(f.del_slots[(size_t)d]);
    // ... and launch by launch in the packed one
    std::vector<int> write_group((size_t)f.n_slots, -1);  // -1: before all
    std::vector<int> in_launch((size_t)f.n_nodes, -1);
    for (size_t g = 0; g < groups; ++g)
        for (int32_t r = p.recv_tptr[g]; r < p.recv_tptr[g + 1]; ++r)
            for (int32_t d = p.recv_nptr[r]; d < p.recv_nptr[r + 1]; ++d)
                if (p.reply_slots[(size_t)d] >= 0)
                    write_group[(size_t)p.reply_slots[(size_t)d]] = (int)g;
    for (size_t g = 0; g < groups; ++g) {
        CHECK(g == 0 || p.recv_tptr[g + 1] > p.recv_tptr[g]);  // no idle launch
        for (int32_t r = p.recv_tptr[g]; r < p.recv_tptr[g + 1]; ++r) {
            int32_t x = p.recv_nodes[(size_t)r];
            CHECK(in_launch[(size_t)x] != (int)g);  // one row per receiver
            in_launch[(size_t)x] = (int)g;
            int32_t n = p.recv_nptr[r + 1] - p.recv_nptr[r];
            CHECK(n >= 1 && n <= cap);
            for (int32_t d = p.recv_nptr[r]; d < p.recv_nptr[r + 1]; ++d) {
                int32_t s = p.del_slots[(size_t)d];
                pack_seq[(size_t)x].push_back(s);
                // the hazard rule: its writer ran in an earlier launch
                CHECK(write_group[(size_t)s] < (int)g);
                if (!f.del_pids.empty())
                    CHECK(p.del_pids[(size_t)d] == s % 4);
                if (!f.del_owners.empty())
                    CHECK(p.del_owners[(size_t)d] == (s * 7) % f.n_nodes);
            }
        }
    }
    CHECK(flat_seq == pack_seq);  // every delivery once, order kept
}

int main()
{
    LevelPacker lp;
    int packed = 0, refused = 0, with_reply = 0;
    for (int i = 0; i < 600; ++i) {
        int n_nodes = (i % 9 == 0) ? 1 : 2 + (int)rnd(14);
        int n_ticks = (i % 11 == 0) ? 0 : 1 + (int)rnd(7);
        int n_carried = (int)rnd(6);
        int snap_p = (i % 7 == 0) ? 0 : 1 + (int)rnd(3);  // 0: carried only
        int deliver_p = (i % 13 == 0) ? 0 : 2 + (int)rnd(5);
        int cap = 1 + (int)rnd(3);
        Flat f = random_round(n_nodes, n_ticks, n_carried, snap_p, deliver_p,
                              i % 3 == 0);
        PackedRound out = sentinel();
        const char* why = run(lp, f, cap, &out);
        if (why) {
            // only a second snapshot of one state can stop a round built
            // this way
            CHECK(std::strstr(why, "two snapshots") != nullptr);
            CHECK(untouched(out));
            ++refused;
        } else {
            check_packed(f, out, cap);
            for (int32_t s : out.reply_slots) with_reply += s >= 0;
            ++packed;
        }

        // each refused shape, made from the same round
        {
            Flat g = f;
            g.pull_nodes.push_back(0);
            out = sentinel();
            CHECK(run(lp, g, cap, &out) != nullptr && untouched(out));
        }
        {
            Flat g = f;
            g.rep_nodes.push_back(0);
            out = sentinel();
            CHECK(run(lp, g, cap, &out) != nullptr && untouched(out));
        }
        if (!f.del_slots.empty()) {
            Flat g = f;  // a PUSH_PULL reply event
            g.reply_slots[rnd((uint32_t)g.reply_slots.size())] = 0;
            out = sentinel();
            CHECK(run(lp, g, cap, &out) != nullptr && untouched(out));
            // a slot read, then snapshotted in a later tick of the round
            Flat h = f;
            h.snap_nodes.push_back(0);
            h.snap_slots.push_back(h.del_slots[0]);
            h.snap_tptr.push_back((int32_t)h.snap_nodes.size());
            h.recv_tptr.push_back(h.recv_tptr.back());
            out = sentinel();
            CHECK(run(lp, h, cap, &out) != nullptr && untouched(out));
            // ids past the arrays
            Flat k = f;
            k.del_slots.back() = (int32_t)k.n_slots;
            out = sentinel();
            CHECK(run(lp, k, cap, &out) != nullptr && untouched(out));
            k = f;
            k.recv_nodes[0] = (int32_t)k.n_nodes;
            out = sentinel();
            CHECK(run(lp, k, cap, &out) != nullptr && untouched(out));
        }
        if (!f.snap_slots.empty()) {
            Flat g = f;  // a slot written twice
            g.snap_nodes.push_back(0);
            g.snap_slots.push_back(g.snap_slots[0]);
            g.snap_tptr.back() += 1;
            out = sentinel();
            CHECK(run(lp, g, cap, &out) != nullptr && untouched(out));
        }
        {
            Flat g = f;  // pointers that do not describe the arrays
            g.recv_nptr.push_back(0);
            out = sentinel();
            CHECK(run(lp, g, cap, &out) != nullptr && untouched(out));
            out = sentinel();
            CHECK(run(lp, f, 0, &out) != nullptr && untouched(out));
        }
    }
    // a node that snapshots twice between two of its deliveries, by hand
    {
        Flat f;
        f.n_nodes = 2; f.n_slots = 3;
        f.snap_nodes = {0, 1, 1}; f.snap_slots = {0, 1, 2};
        f.snap_tptr = {0, 1, 2, 3};
        f.recv_nodes = {1}; f.recv_nptr = {0, 1}; f.recv_tptr = {0, 1, 1, 1};
        f.del_slots = {0}; f.reply_slots = {-1};
        PackedRound out = sentinel();
        const char* why = run(lp, f, 1, &out);
        CHECK(why && std::strstr(why, "two snapshots") && untouched(out));
    }
    // the sample has to hold both kinds, and reply-slot snapshots
    CHECK(packed >= 200);
    CHECK(refused >= 20);
    CHECK(with_reply >= 100);
    std::printf("round_levels_san OK: %d packed, %d refused\n", packed,
                refused);
    return 0;
}
