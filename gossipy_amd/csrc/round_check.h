// The bounds check between a schedule and the kernels (plain C++: no pybind,
// no torch, no HIP), over a round as write_round_layout laid it out.
#pragma once

#include <cstddef>
#include <cstdint>

#include "round_layout.h"

// Every index the kernels will follow stays inside its array: node ids
// below n_local, slot ids below pool_cap (a negative reply slot means "none"
// to the kernels), CSR pointers and tick pointers monotone and inside their
// targets. One pass over a few KB of host memory. Returns nullptr when all
// of it holds, else the name of the first offender.
static inline const char* round_bounds_error(
    const RoundSpan tptr[ROUND_N_TPTRS], const RoundLayout& lay,
    const int32_t* host, int64_t n_local, int64_t pool_cap)
{
    const char* const* an = ROUND_ARRAY_NAMES;
    const char* const* tn = ROUND_TPTR_NAMES;
    const size_t* len = lay.len;
    auto all_in = [&](int id, int64_t lo, int64_t hi) {
        const int32_t* p = host + lay.off[id];
        for (size_t i = 0; i < len[id]; ++i)
            if (p[i] < lo || p[i] >= hi) return false;
        return true;
    };
    // {0, ..., last}: starts at 0, never decreases, last <= target
    auto ptr_ok = [](const int32_t* p, size_t n, size_t target) {
        if (n == 0 || p[0] != 0) return false;
        for (size_t i = 1; i < n; ++i)
            if (p[i] < p[i - 1]) return false;
        return (size_t)p[n - 1] <= target;
    };
    auto csr_ok = [&](int id, int into) {
        return ptr_ok(host + lay.off[id], len[id], len[into]);
    };
    auto same_or_empty = [&](int id, int as) {
        return !len[id] || len[id] == len[as];
    };
    if (tptr[RT_SNAP].len < 1) return tn[RT_SNAP];
    const size_t groups = tptr[RT_SNAP].len - 1;
    auto tptr_ok = [&](int id, size_t target) {
        return tptr[id].len == groups + 1 &&
               ptr_ok(tptr[id].data, tptr[id].len, target);
    };

    if (!all_in(RA_SNAP_NODES, 0, n_local)) return an[RA_SNAP_NODES];
    if (!all_in(RA_SNAP_SLOTS, 0, pool_cap)) return an[RA_SNAP_SLOTS];
    if (len[RA_SNAP_SLOTS] != len[RA_SNAP_NODES]) return an[RA_SNAP_SLOTS];
    if (!all_in(RA_RECV_NODES, 0, n_local)) return an[RA_RECV_NODES];
    if (!all_in(RA_DEL_SLOTS, 0, pool_cap)) return an[RA_DEL_SLOTS];
    if (!all_in(RA_REPLY_SLOTS, INT32_MIN, pool_cap)) return an[RA_REPLY_SLOTS];
    if (!all_in(RA_REP_NODES, 0, n_local)) return an[RA_REP_NODES];
    if (!all_in(RA_REP_SLOTS, 0, pool_cap)) return an[RA_REP_SLOTS];
    if (!all_in(RA_REP_REPLY_SLOTS, INT32_MIN, pool_cap))
        return an[RA_REP_REPLY_SLOTS];
    if (len[RA_PULL_NODES] || len[RA_PULL_SLOTS])
        return "pull arrays in a packed round";
    if (len[RA_RECV_NPTR] != len[RA_RECV_NODES] + 1) return an[RA_RECV_NPTR];
    if (len[RA_REP_NPTR] != len[RA_REP_NODES] + 1) return an[RA_REP_NPTR];
    if (!csr_ok(RA_RECV_NPTR, RA_DEL_SLOTS)) return an[RA_RECV_NPTR];
    if (!csr_ok(RA_REP_NPTR, RA_REP_SLOTS)) return an[RA_REP_NPTR];
    if (!same_or_empty(RA_REPLY_SLOTS, RA_DEL_SLOTS)) return an[RA_REPLY_SLOTS];
    if (!same_or_empty(RA_DEL_PIDS, RA_DEL_SLOTS)) return an[RA_DEL_PIDS];
    if (!same_or_empty(RA_REP_REPLY_SLOTS, RA_REP_SLOTS))
        return an[RA_REP_REPLY_SLOTS];
    if (!same_or_empty(RA_REP_PIDS, RA_REP_SLOTS)) return an[RA_REP_PIDS];
    if (!tptr_ok(RT_SNAP, len[RA_SNAP_NODES])) return tn[RT_SNAP];
    if (!tptr_ok(RT_RECV, len[RA_RECV_NODES])) return tn[RT_RECV];
    if (!tptr_ok(RT_PULL, 0)) return tn[RT_PULL];
    if (!tptr_ok(RT_REP, len[RA_REP_NODES])) return tn[RT_REP];
    const int32_t* ids = host + lay.eval_off;
    for (size_t i = 0; i < lay.n_eval; ++i)
        if (ids[i] < 0 || ids[i] >= n_local) return "eval ids";
    return nullptr;
}
