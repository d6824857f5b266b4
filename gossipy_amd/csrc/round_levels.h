// Launch packing by dependency level (plain C++: no pybind, no torch, no
// HIP), for rounds of plain deliveries: PUSH, no pull and no reply events.
//
// A tick launch lasts as long as its longest receiver row, and the launches
// of a round run one after another. The deliveries of a round form a graph:
// a delivery to x needs the previous delivery to x, and, where its slot was
// snapshotted in this round after its sender had already received, the
// sender's last delivery before that snapshot. LevelPacker puts every
// delivery into the first launch in which both are done, at most `cap` per
// receiver row, so the round's launches add up to its critical path and not
// to the sum of its longest rows.
//
// The result is a PackedRound in the executors' format: group 0 carries the
// one snapshot launch (every snapshot whose sender has not received yet in
// the round), a later snapshot rides as the reply slot of its sender's
// latest delivery, and group g holds the receiver rows of launch g.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

// the packed arrays of a round, as stream_round and the RoundDriver take them
struct PackedRound {
    std::vector<int32_t> snap_nodes, snap_slots, snap_tptr{0};
    std::vector<int32_t> recv_nodes, recv_nptr{0}, recv_tptr{0};
    std::vector<int32_t> del_slots, reply_slots, del_pids, del_owners;
    std::vector<int32_t> rep_nodes, rep_nptr{0}, rep_tptr{0};
    std::vector<int32_t> rep_slots, rep_reply_slots, rep_pids, rep_owners;
    std::vector<int32_t> pull_tptr{};
};

// Keeps its scratch between rounds (epoch-stamped, never cleared), so a
// round costs O(events). One round at a time per object.
class LevelPacker {
public:
    // Packs the round given by the scheduler's flat arrays (the ones
    // pack_round_compute takes) into *out. Returns nullptr, or, having left
    // *out alone, the reason why this round is not one for this packer:
    //   - it has a pull or a reply event;
    //   - a delivery would need two reply slots (its receiver snapshots
    //     twice before it receives again);
    //   - a slot is snapshotted after it was read or written in the round
    //     (slot reuse within a round: launch order would change what a
    //     reader sees);
    //   - the arrays do not describe a round (sizes, ids out of range).
    const char* pack(
        const std::vector<int32_t>& snap_nodes,
        const std::vector<int32_t>& snap_slots,
        const std::vector<int32_t>& snap_tptr,
        const std::vector<int32_t>& recv_nodes,
        const std::vector<int32_t>& recv_nptr,
        const std::vector<int32_t>& recv_tptr,
        const std::vector<int32_t>& del_slots,
        const std::vector<int32_t>& reply_slots,
        const std::vector<int32_t>& del_pids,
        const std::vector<int32_t>& pull_nodes,
        const std::vector<int32_t>& rep_nodes,
        const std::vector<int32_t>& del_owners,
        int64_t n_nodes, int64_t n_slots, int cap, PackedRound* out)
    {
        if (cap < 1) return "row cap below 1";
        if (!pull_nodes.empty()) return "pull events";
        if (!rep_nodes.empty()) return "reply deliveries";
        const size_t n_del = del_slots.size(), n_snap = snap_nodes.size();
        const size_t n_rows = recv_nodes.size();
        if (snap_tptr.empty() || recv_tptr.size() != snap_tptr.size() ||
            snap_slots.size() != n_snap || recv_nptr.size() != n_rows + 1 ||
            (!reply_slots.empty() && reply_slots.size() != n_del) ||
            (!del_pids.empty() && del_pids.size() != n_del) ||
            (!del_owners.empty() && del_owners.size() != n_del) ||
            n_nodes < 0 || n_slots < 0 || n_nodes > INT32_MAX ||
            n_slots > INT32_MAX)
            return "malformed round";
        if (!ptr_ok(snap_tptr, n_snap) || !ptr_ok(recv_tptr, n_rows) ||
            !ptr_ok(recv_nptr, n_del) || (size_t)snap_tptr.back() != n_snap ||
            (size_t)recv_tptr.back() != n_rows ||
            (size_t)recv_nptr.back() != n_del)
            return "malformed round";
        for (int32_t v : reply_slots)
            if (v >= 0) return "reply events";

        begin_round((size_t)n_nodes, (size_t)n_slots, n_del);
        const size_t n_ticks = snap_tptr.size() - 1;
        g0_nodes_.clear(); g0_slots_.clear(); order_.clear();

        // pass 1, in schedule order: who writes each slot, and each
        // receiver's deliveries as a list
        for (size_t t = 0; t < n_ticks; ++t) {
            for (int32_t i = snap_tptr[t]; i < snap_tptr[t + 1]; ++i) {
                int32_t x = snap_nodes[i], s = snap_slots[i];
                if (x < 0 || x >= n_nodes || s < 0 || s >= n_slots)
                    return "malformed round";
                if (slot_w_ep_[s] == ep_ || slot_r_ep_[s] == ep_)
                    return "slot reused within the round";
                slot_w_ep_[s] = ep_;
                if (node_ep_[x] != ep_) {
                    g0_nodes_.push_back(x);
                    g0_slots_.push_back(s);
                    slot_writer_[s] = -1;
                } else {
                    int32_t last = node_tail_[x];
                    if (reply_[last] >= 0) return "two snapshots of one state";
                    reply_[last] = s;
                    slot_writer_[s] = last;
                }
            }
            for (int32_t r = recv_tptr[t]; r < recv_tptr[t + 1]; ++r) {
                int32_t x = recv_nodes[r];
                if (x < 0 || x >= n_nodes) return "malformed round";
                for (int32_t d = recv_nptr[r]; d < recv_nptr[r + 1]; ++d) {
                    int32_t s = del_slots[d];
                    if (s < 0 || s >= n_slots) return "malformed round";
                    slot_r_ep_[s] = ep_;
                    dep_[d] = slot_w_ep_[s] == ep_ ? slot_writer_[s] : -1;
                    if (node_ep_[x] != ep_) {
                        node_ep_[x] = ep_;
                        node_cur_[x] = d;
                        order_.push_back(x);
                    } else {
                        next_[node_tail_[x]] = d;
                    }
                    node_tail_[x] = d;
                }
            }
        }

        // pass 2: launch after launch from a ready list. A receiver is on
        // the list of launch g exactly when its next delivery is ready for
        // g; one that waits for a writer not yet placed hangs on that
        // writer and is listed once it is placed.
        PackedRound o;
        o.snap_nodes = g0_nodes_;
        o.snap_slots = g0_slots_;
        o.recv_nodes.reserve(n_del);
        o.recv_nptr.reserve(n_del + 1);
        o.del_slots.reserve(n_del);
        o.reply_slots.reserve(n_del);
        if (!del_pids.empty()) o.del_pids.reserve(n_del);
        if (!del_owners.empty()) o.del_owners.reserve(n_del);
        size_t placed = 0;
        int32_t g = 0;
        cand_.swap(order_);
        while (!cand_.empty()) {
            ready_.clear();
            for (int32_t x : cand_) {
                int32_t d = node_cur_[x];
                int taken = 0;
                while (d >= 0 && taken < cap &&
                       (dep_[d] < 0 ||
                        (level_[dep_[d]] >= 0 && level_[dep_[d]] < g))) {
                    if (!taken) o.recv_nodes.push_back(x);
                    o.del_slots.push_back(del_slots[d]);
                    o.reply_slots.push_back(reply_[d]);
                    if (!del_pids.empty()) o.del_pids.push_back(del_pids[d]);
                    if (!del_owners.empty())
                        o.del_owners.push_back(del_owners[d]);
                    level_[d] = g;
                    for (int32_t y = waiter_[d]; y >= 0; y = wait_next_[y])
                        ready_.push_back(y);
                    ++taken; ++placed;
                    d = next_[d];
                }
                node_cur_[x] = d;
                if (taken) o.recv_nptr.push_back((int32_t)o.del_slots.size());
                if (d >= 0) {
                    int32_t w = dep_[d];
                    if (w < 0 || level_[w] >= 0) ready_.push_back(x);
                    else { wait_next_[x] = waiter_[w]; waiter_[w] = x; }
                }
            }
            o.snap_tptr.push_back((int32_t)o.snap_nodes.size());
            o.recv_tptr.push_back((int32_t)o.recv_nodes.size());
            o.rep_tptr.push_back(0);
            cand_.swap(ready_);
            ++g;
        }
        if (placed != n_del) return "dependency cycle";
        if (g == 0 && !o.snap_nodes.empty()) {  // snapshots only
            o.snap_tptr.push_back((int32_t)o.snap_nodes.size());
            o.recv_tptr.push_back(0);
            o.rep_tptr.push_back(0);
            g = 1;
        }
        o.pull_tptr.assign((size_t)g + 1, 0);
        *out = std::move(o);
        return nullptr;
    }

private:
    // {0, ..., last}: starts at 0, never decreases, stays within target
    static bool ptr_ok(const std::vector<int32_t>& p, size_t target)
    {
        if (p.empty() || p[0] != 0) return false;
        for (size_t i = 1; i < p.size(); ++i)
            if (p[i] < p[i - 1]) return false;
        return (size_t)p.back() <= target;
    }

    void begin_round(size_t n_nodes, size_t n_slots, size_t n_del)
    {
        if (++ep_ == INT32_MAX) {  // stamps wrap: forget them all
            ep_ = 1;
            node_ep_.assign(node_ep_.size(), 0);
            slot_w_ep_.assign(slot_w_ep_.size(), 0);
            slot_r_ep_.assign(slot_r_ep_.size(), 0);
        }
        if (node_ep_.size() < n_nodes) {
            node_ep_.resize(n_nodes, 0);
            node_cur_.resize(n_nodes);
            node_tail_.resize(n_nodes);
            wait_next_.resize(n_nodes);
        }
        if (slot_w_ep_.size() < n_slots) {
            slot_w_ep_.resize(n_slots, 0);
            slot_r_ep_.resize(n_slots, 0);
            slot_writer_.resize(n_slots);
        }
        next_.assign(n_del, -1);
        dep_.assign(n_del, -1);
        reply_.assign(n_del, -1);
        level_.assign(n_del, -1);
        waiter_.assign(n_del, -1);
    }

    int32_t ep_ = 0;
    // per node: stamp of the round in which it first received, its next
    // unplaced delivery and its last one so far
    std::vector<int32_t> node_ep_, node_cur_, node_tail_;
    // per slot: stamps of the round that wrote / read it, and the delivery
    // whose reply slot it is (-1: the round-start snapshot)
    std::vector<int32_t> slot_w_ep_, slot_r_ep_, slot_writer_;
    // per delivery (flat index): the receiver's next delivery, the delivery
    // that writes its slot, its reply slot, its launch, and the first of
    // the receivers that wait for it (chained through wait_next_, per node)
    std::vector<int32_t> next_, dep_, reply_, level_, waiter_;
    std::vector<int32_t> wait_next_;
    std::vector<int32_t> g0_nodes_, g0_slots_, order_, cand_, ready_;
};
