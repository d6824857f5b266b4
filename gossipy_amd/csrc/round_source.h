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

// The packed event arrays of a round. This table is their definition: its
// order is the order the one upload lays them out in, and every consumer
// (the scheduler's RoundView, the executors' RoundArrays, the Python path's
// upload through the exported ROUND_ARRAY_NAMES) indexes by it.
#define ROUND_ARRAY_TABLE(X)              \
    X(RA_SNAP_NODES, "snap_nodes")        \
    X(RA_SNAP_SLOTS, "snap_slots")        \
    X(RA_RECV_NODES, "recv_nodes")        \
    X(RA_RECV_NPTR, "recv_nptr")          \
    X(RA_DEL_SLOTS, "del_slots")          \
    X(RA_REPLY_SLOTS, "reply_slots")      \
    X(RA_PULL_NODES, "pull_nodes")        \
    X(RA_PULL_SLOTS, "pull_slots")        \
    X(RA_REP_NODES, "rep_nodes")          \
    X(RA_REP_NPTR, "rep_nptr")            \
    X(RA_REP_SLOTS, "rep_slots")          \
    X(RA_DEL_PIDS, "del_pids")            \
    X(RA_REP_PIDS, "rep_pids")            \
    X(RA_REP_REPLY_SLOTS, "rep_reply_slots")

// The packed tick-pointer arrays ([n_groups + 1] each, read on the host).
#define ROUND_TPTR_TABLE(X)   \
    X(RT_SNAP, "snap_tptr")   \
    X(RT_RECV, "recv_tptr")   \
    X(RT_PULL, "pull_tptr")   \
    X(RT_REP, "rep_tptr")

#define ROUND_TABLE_ID(id, name) id,
#define ROUND_TABLE_NAME(id, name) name,
enum RoundArrayId { ROUND_ARRAY_TABLE(ROUND_TABLE_ID) ROUND_N_ARRAYS };
enum RoundTptrId { ROUND_TPTR_TABLE(ROUND_TABLE_ID) ROUND_N_TPTRS };
static const char* const ROUND_ARRAY_NAMES[ROUND_N_ARRAYS] = {
    ROUND_ARRAY_TABLE(ROUND_TABLE_NAME)};
static const char* const ROUND_TPTR_NAMES[ROUND_N_TPTRS] = {
    ROUND_TPTR_TABLE(ROUND_TABLE_NAME)};
#undef ROUND_TABLE_ID
#undef ROUND_TABLE_NAME

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
