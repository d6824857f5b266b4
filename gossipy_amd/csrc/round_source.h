// C ABI between the native scheduler and a native round executor (plain
// C++: no pybind, no torch, no HIP).
//
// A RoundSource hands out one round at a time as a RoundView: pointers into
// memory the source owns. The executor (the HIP extension's RoundDriver)
// calls take(r) once per round without the GIL; nothing of the schedule
// passes through Python objects on the way.
#pragma once

#include <cstddef>
#include <cstdint>

// The packed event arrays in the order the executors' one upload lays them
// out (the `dev_names` of BatchedGossipSimulator._run_round_fast).
enum RoundArrayId {
    RA_SNAP_NODES = 0,
    RA_SNAP_SLOTS,
    RA_RECV_NODES,
    RA_RECV_NPTR,
    RA_DEL_SLOTS,
    RA_REPLY_SLOTS,
    RA_PULL_NODES,
    RA_PULL_SLOTS,
    RA_REP_NODES,
    RA_REP_NPTR,
    RA_REP_SLOTS,
    RA_DEL_PIDS,
    RA_REP_PIDS,
    RA_REP_REPLY_SLOTS,
    ROUND_N_ARRAYS
};

// The packed tick-pointer arrays ([n_groups + 1] each, read on the host).
enum RoundTptrId {
    RT_SNAP = 0,
    RT_RECV,
    RT_PULL,
    RT_REP,
    ROUND_N_TPTRS
};

struct RoundSpan {
    const int32_t* data;
    size_t len;
};

struct RoundView {
    RoundSpan arrays[ROUND_N_ARRAYS];
    RoundSpan tptr[ROUND_N_TPTRS];
    int64_t sent, failed, total_size, n_slots;
    // the round's eval draw as drawn (global ids, unsorted, duplicates
    // possible); n_eval == 0: no draw this round
    const int64_t* eval_nodes;
    size_t n_eval;
};

struct RoundSource {
    void* self;
    // Fills *out with round r and returns 0; on failure returns nonzero
    // with a message in err (NUL-terminated, at most errlen bytes) and
    // consumes nothing. Rounds are handed out in order. The view stays
    // valid until the next take() on the same source.
    int (*take)(void* self, int64_t r, RoundView* out, char* err,
                size_t errlen);
};
