// The one int32 layout of a round's upload (plain C++), shared by
// NativeScheduler.next_round_packed_into and the HIP extension's
// RoundDriver:
//
//   [ the ROUND_N_ARRAYS packed event arrays, in RoundArrayId order ]
//   [ the eval ids: sorted, unique, local (global id - node_lo)      ]
//
// which is np.concatenate over ROUND_ARRAY_NAMES followed by
// np.unique(eval_nodes) - node_lo.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "round_source.h"

struct RoundLayout {
    size_t off[ROUND_N_ARRAYS];  // in int32 elements
    size_t len[ROUND_N_ARRAYS];
    size_t eval_off;
    size_t n_eval;  // unique ids written
    size_t total;   // elements written: eval_off + n_eval
};

// Elements a buffer must hold for write_round_layout to accept the view
// (the eval draw counted before de-duplication; never 0, so a buffer of
// this size is never empty).
static inline size_t round_layout_capacity(const RoundView& v)
{
    size_t n = v.n_eval;
    for (int i = 0; i < ROUND_N_ARRAYS; ++i) n += v.arrays[i].len;
    return n ? n : 1;
}

// Writes the layout into buf[0 .. cap). Returns false, having written
// nothing, when cap < round_layout_capacity(v).
static inline bool write_round_layout(const RoundView& v, int64_t node_lo,
                                      int32_t* buf, size_t cap,
                                      RoundLayout* out)
{
    if (cap < round_layout_capacity(v)) return false;
    size_t off = 0;
    for (int i = 0; i < ROUND_N_ARRAYS; ++i) {
        const RoundSpan& a = v.arrays[i];
        out->off[i] = off;
        out->len[i] = a.len;
        if (a.len) std::memcpy(buf + off, a.data, a.len * sizeof(int32_t));
        off += a.len;
    }
    out->eval_off = off;
    int32_t* ids = buf + off;
    for (size_t i = 0; i < v.n_eval; ++i)
        ids[i] = (int32_t)(v.eval_nodes[i] - node_lo);
    std::sort(ids, ids + v.n_eval);
    out->n_eval = (size_t)(std::unique(ids, ids + v.n_eval) - ids);
    out->total = off + out->n_eval;
    return true;
}
