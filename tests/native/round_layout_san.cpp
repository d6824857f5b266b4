// Stand-alone driver of csrc/round_layout.h, csrc/round_check.h and
// csrc/round_ring.h for an address/undefined-behaviour sanitizer build
// (tests/test_round_driver.py compiles and runs it). It plays the
// RoundDriver's host side: it takes a slot from the ring, grows the slot's
// buffer to what the round needs, writes the layout into it, and marks the
// slot's "event" as pending, with a fake completion predicate in place of
// HIP; and it puts good and bad rounds to the bounds check that stands
// between a schedule and the kernels. Exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gossipy_amd/csrc/round_check.h"
#include "../../gossipy_amd/csrc/round_layout.h"
#include "../../gossipy_amd/csrc/round_ring.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__,  \
                         #cond);                                           \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// a round with n_snap snapshots, n_recv receivers of two deliveries each
// and an eval draw of n_eval ids with every id drawn twice
struct FakeRound {
    std::vector<int32_t> a[ROUND_N_ARRAYS];
    std::vector<int32_t> t[ROUND_N_TPTRS];
    std::vector<int64_t> eval;
    RoundView view;

    FakeRound(int n_snap, int n_recv, int n_eval, int64_t node_lo)
    {
        for (int i = 0; i < n_snap; ++i) {
            a[RA_SNAP_NODES].push_back(i);
            a[RA_SNAP_SLOTS].push_back(100 + i);
        }
        a[RA_RECV_NPTR].push_back(0);
        for (int i = 0; i < n_recv; ++i) {
            a[RA_RECV_NODES].push_back(i);
            for (int k = 0; k < 2; ++k) {
                a[RA_DEL_SLOTS].push_back(200 + 2 * i + k);
                a[RA_REPLY_SLOTS].push_back(-1);
            }
            a[RA_RECV_NPTR].push_back((int32_t)a[RA_DEL_SLOTS].size());
        }
        a[RA_REP_NPTR].push_back(0);
        t[RT_SNAP] = {0, n_snap};
        t[RT_RECV] = {0, n_recv};
        t[RT_PULL] = {0, 0};
        t[RT_REP] = {0, 0};
        for (int i = n_eval - 1; i >= 0; --i) {
            eval.push_back(node_lo + 3 * i);
            eval.push_back(node_lo + 3 * i);
        }
        view.sent = view.failed = view.total_size = 0;
        view.n_slots = 300;
        point_view();
    }
    FakeRound(const FakeRound&) = delete;

    // after a change to a, t or eval
    void point_view()
    {
        for (int i = 0; i < ROUND_N_ARRAYS; ++i)
            view.arrays[i] = {a[i].empty() ? nullptr : a[i].data(), a[i].size()};
        for (int i = 0; i < ROUND_N_TPTRS; ++i)
            view.tptr[i] = {t[i].data(), t[i].size()};
        view.eval_nodes = eval.empty() ? nullptr : eval.data();
        view.n_eval = eval.size();
    }
};

static void check_layout(const FakeRound& fr, const RoundLayout& lay,
                         const int32_t* buf, int n_eval)
{
    size_t off = 0;
    for (int i = 0; i < ROUND_N_ARRAYS; ++i) {
        CHECK(lay.off[i] == off);
        CHECK(lay.len[i] == fr.a[i].size());
        for (size_t k = 0; k < lay.len[i]; ++k)
            CHECK(buf[off + k] == fr.a[i][k]);
        off += lay.len[i];
    }
    CHECK(lay.eval_off == off);
    CHECK(lay.n_eval == (size_t)n_eval);
    CHECK(lay.total == off + (size_t)n_eval);
    for (int i = 0; i < n_eval; ++i) CHECK(buf[off + i] == 3 * i);
}

// csrc/round_check.h over a FakeRound: the round is laid out as the driver
// does it, `corrupt` changes one thing in the buffer, in the layout's
// lengths or in the tick pointers, and the check has to name `want`
// (nullptr: the round passes).
constexpr int64_t N_LOCAL = 50, POOL_CAP = 300;

struct Laid {
    std::vector<int32_t> buf;
    RoundLayout lay;
    std::vector<int32_t> t[ROUND_N_TPTRS];
    int32_t& at(int id, size_t i) { return buf[lay.off[id] + i]; }
};

template <typename Corrupt>
static void check_bounds(int line, const FakeRound& fr, const char* want,
                         Corrupt corrupt)
{
    Laid l;
    l.buf.assign(round_layout_capacity(fr.view), -1);
    CHECK(write_round_layout(fr.view, 0, l.buf.data(), l.buf.size(), &l.lay));
    for (int i = 0; i < ROUND_N_TPTRS; ++i) l.t[i] = fr.t[i];
    corrupt(l);
    RoundSpan tptr[ROUND_N_TPTRS];
    for (int i = 0; i < ROUND_N_TPTRS; ++i)
        tptr[i] = {l.t[i].data(), l.t[i].size()};
    const char* got =
        round_bounds_error(tptr, l.lay, l.buf.data(), N_LOCAL, POOL_CAP);
    bool same = want ? (got && std::strcmp(got, want) == 0) : !got;
    if (!same) {
        std::fprintf(stderr, "bounds check line %d: got %s, want %s\n", line,
                     got ? got : "(pass)", want ? want : "(pass)");
        std::exit(1);
    }
}
#define PASSES(fr, ...) \
    check_bounds(__LINE__, fr, nullptr, [&](Laid& l) { __VA_ARGS__; })
#define REJECTS(fr, want, ...) \
    check_bounds(__LINE__, fr, want, [&](Laid& l) { __VA_ARGS__; })

static void check_round_bounds()
{
    // 3 snapshots into slots 100..102, 2 receivers (nodes 0, 1) of two
    // deliveries each from slots 200..203, eval ids {0, 3, 6, 9}, one group
    FakeRound fr(3, 2, 4, 0);
    PASSES(fr, (void)l);
    // a negative reply slot means "none" (the round's own are all -1)
    PASSES(fr, l.at(RA_REPLY_SLOTS, 1) = INT32_MIN);
    // the last valid ids
    PASSES(fr, l.at(RA_SNAP_NODES, 0) = N_LOCAL - 1;
           l.at(RA_DEL_SLOTS, 0) = POOL_CAP - 1);
    {
        // all arrays empty but the two nptr zeros, zero groups
        FakeRound empty(0, 0, 0, 0);
        for (auto& t : empty.t) t = {0};
        empty.point_view();
        CHECK(round_layout_capacity(empty.view) == 2);
        PASSES(empty, (void)l);
    }

    // node ids: one past the last, and negative
    REJECTS(fr, "snap_nodes", l.at(RA_SNAP_NODES, 2) = N_LOCAL);
    REJECTS(fr, "recv_nodes", l.at(RA_RECV_NODES, 0) = N_LOCAL);
    REJECTS(fr, "eval ids", l.buf[l.lay.eval_off + 3] = N_LOCAL);
    REJECTS(fr, "snap_nodes", l.at(RA_SNAP_NODES, 0) = -1);
    REJECTS(fr, "recv_nodes", l.at(RA_RECV_NODES, 1) = -1);
    REJECTS(fr, "eval ids", l.buf[l.lay.eval_off] = -1);
    // slot ids: one past the pool, and negative where that is no "none"
    REJECTS(fr, "snap_slots", l.at(RA_SNAP_SLOTS, 1) = POOL_CAP);
    REJECTS(fr, "del_slots", l.at(RA_DEL_SLOTS, 3) = POOL_CAP);
    REJECTS(fr, "del_slots", l.at(RA_DEL_SLOTS, 0) = -1);
    REJECTS(fr, "reply_slots", l.at(RA_REPLY_SLOTS, 2) = POOL_CAP);
    // the deliveries' CSR pointer {0, 2, 4}
    REJECTS(fr, "recv_nptr", l.at(RA_RECV_NPTR, 0) = 1);
    REJECTS(fr, "recv_nptr", l.at(RA_RECV_NPTR, 1) = 5);  // decreases
    REJECTS(fr, "recv_nptr", l.at(RA_RECV_NPTR, 2) = 5);  // past del_slots
    // lengths that have to agree
    REJECTS(fr, "recv_nptr", l.lay.len[RA_RECV_NPTR] -= 1);
    REJECTS(fr, "snap_slots", l.lay.len[RA_SNAP_SLOTS] -= 1);
    REJECTS(fr, "reply_slots", l.lay.len[RA_REPLY_SLOTS] -= 1);
    REJECTS(fr, "pull arrays in a packed round", l.lay.len[RA_PULL_NODES] = 1);
    REJECTS(fr, "pull arrays in a packed round", l.lay.len[RA_PULL_SLOTS] = 1);
    // tick pointers: length, first element, last element
    REJECTS(fr, "snap_tptr", l.t[RT_SNAP].clear());
    REJECTS(fr, "recv_tptr", l.t[RT_RECV] = {0});
    REJECTS(fr, "rep_tptr", l.t[RT_REP] = {0, 0, 0});
    REJECTS(fr, "snap_tptr", l.t[RT_SNAP] = {1, 3});
    REJECTS(fr, "snap_tptr", l.t[RT_SNAP] = {0, 4});
    REJECTS(fr, "recv_tptr", l.t[RT_RECV] = {0, 3});
    REJECTS(fr, "pull_tptr", l.t[RT_PULL] = {0, 1});

    // the same round with a reply to each receiver's first sender and
    // per-delivery ids, in two groups, so a tick pointer can also decrease
    FakeRound rp(3, 2, 0, 0);
    rp.a[RA_REP_NODES] = {7, 8};
    rp.a[RA_REP_NPTR] = {0, 1, 2};
    rp.a[RA_REP_SLOTS] = {210, 211};
    rp.a[RA_REP_REPLY_SLOTS] = {-1, -1};
    rp.a[RA_DEL_PIDS] = {0, 1, 2, 3};
    rp.a[RA_REP_PIDS] = {4, 5};
    rp.t[RT_SNAP] = {0, 3, 3};
    rp.t[RT_RECV] = {0, 1, 2};
    rp.t[RT_PULL] = {0, 0, 0};
    rp.t[RT_REP] = {0, 1, 2};
    rp.point_view();
    PASSES(rp, (void)l);
    PASSES(rp, l.at(RA_REP_REPLY_SLOTS, 0) = -7);
    REJECTS(rp, "rep_nodes", l.at(RA_REP_NODES, 1) = N_LOCAL);
    REJECTS(rp, "rep_nodes", l.at(RA_REP_NODES, 0) = -1);
    REJECTS(rp, "rep_slots", l.at(RA_REP_SLOTS, 0) = POOL_CAP);
    REJECTS(rp, "rep_reply_slots", l.at(RA_REP_REPLY_SLOTS, 1) = POOL_CAP);
    REJECTS(rp, "rep_nptr", l.at(RA_REP_NPTR, 2) = 3);
    REJECTS(rp, "rep_nptr", l.lay.len[RA_REP_NPTR] -= 1);
    REJECTS(rp, "del_pids", l.lay.len[RA_DEL_PIDS] -= 1);
    REJECTS(rp, "rep_reply_slots", l.lay.len[RA_REP_REPLY_SLOTS] -= 1);
    REJECTS(rp, "rep_pids", l.lay.len[RA_REP_PIDS] -= 1);
    REJECTS(rp, "recv_tptr", l.t[RT_RECV] = {0, 2, 1});
    REJECTS(rp, "rep_tptr", l.t[RT_REP] = {0, 1, 3});
}

struct HostSlot {
    std::vector<int32_t> buf;  // exactly the slot's capacity: ASan sees past it
    int pending_until = -1;    // the fake event completes at this time
};

int main()
{
    // the writer alone: empty round, snapshots only, too-small buffers
    {
        FakeRound empty(0, 0, 0, 0);
        CHECK(round_layout_capacity(empty.view) == 2);  // the two nptr zeros
        std::vector<int32_t> buf(2, -7);
        RoundLayout lay;
        CHECK(write_round_layout(empty.view, 0, buf.data(), buf.size(), &lay));
        check_layout(empty, lay, buf.data(), 0);
        CHECK(lay.total == 2 && buf[0] == 0 && buf[1] == 0);
        std::vector<int32_t> one(1, -7);
        CHECK(!write_round_layout(empty.view, 0, one.data(), one.size(), &lay));
        CHECK(one[0] == -7);  // a refused write touches nothing

        FakeRound snaps(5, 0, 0, 0);
        std::vector<int32_t> b2(round_layout_capacity(snaps.view));
        CHECK(b2.size() == 12);
        CHECK(write_round_layout(snaps.view, 0, b2.data(), b2.size(), &lay));
        check_layout(snaps, lay, b2.data(), 0);

        // duplicates in the draw: room for the draw as drawn is required,
        // the unique ids come out sorted and local
        FakeRound ev(1, 2, 4, 1000);
        size_t need = round_layout_capacity(ev.view);
        CHECK(need == 2 + 2 + 3 + 4 + 4 + 1 + 8);
        std::vector<int32_t> b3(need);
        CHECK(!write_round_layout(ev.view, 1000, b3.data(), need - 1, &lay));
        CHECK(write_round_layout(ev.view, 1000, b3.data(), need, &lay));
        check_layout(ev, lay, b3.data(), 4);
    }

    check_round_bounds();

    // growth rule
    CHECK(grown_capacity(0, 1) == 256);
    CHECK(grown_capacity(256, 256) == 256);
    CHECK(grown_capacity(256, 257) == 512);
    CHECK(grown_capacity(256, 5000) == 8192);

    // the ring: 100 rounds of wrap-around over 4 slots, rounds of changing
    // size (so slots grow at different times), "events" that complete
    // three rounds after they were recorded, so the fourth acquire finds
    // its slot pending now and then and has to wait
    {
        constexpr int N = 4;
        SlotRing<N> ring;
        HostSlot slots[N];
        int now = 0, waits = 0, dones = 0;
        for (int r = 0; r < 100; ++r, ++now) {
            int sizes[] = {0, 3, 40, 7, 300, 1, 1200, 2};
            int n = sizes[r % 8] * (1 + r / 40);
            FakeRound fr(n, n / 2, r % 3 ? 1 + r % 5 : 0, 0);
            int si = ring.acquire(
                [&](int i) {
                    ++dones;
                    return slots[i].pending_until <= now;
                },
                [&](int i) {
                    ++waits;
                    CHECK(slots[i].pending_until > now);
                    now = slots[i].pending_until;  // blocks until done
                });
            CHECK(si == r % N);
            HostSlot& s = slots[si];
            // never handed out while its work is pending
            CHECK(s.pending_until <= now);
            size_t need = round_layout_capacity(fr.view);
            size_t cap = grown_capacity(s.buf.size(), need);
            CHECK(cap >= need && cap >= s.buf.size());
            if (cap != s.buf.size()) s.buf.assign(cap, -1);
            RoundLayout lay;
            CHECK(write_round_layout(fr.view, 0, s.buf.data(), s.buf.size(),
                                     &lay));
            check_layout(fr, lay, s.buf.data(), r % 3 ? 1 + r % 5 : 0);
            CHECK(lay.total <= s.buf.size());
            CHECK(ring.busy(si));
            // every 7th round's work is slow: 6 time steps instead of 3
            s.pending_until = now + (r % 7 == 0 ? 6 : 3);
        }
        CHECK(dones == 100 - N);  // a never-used slot asks nobody
        CHECK(waits > 0);

        // a failed enqueue gives the slot back, and it is next again
        int si = ring.acquire([](int) { return true; }, [](int) {});
        ring.abandon(si);
        CHECK(!ring.busy(si));
        int again = ring.acquire(
            [](int) { CHECK(false); return true; }, [](int) { CHECK(false); });
        CHECK(again == si);
    }

    std::printf("round_layout_san OK\n");
    return 0;
}
