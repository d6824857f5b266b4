// gossipy_amd CDNA4 (gfx950) kernels — the batched compute path of the
// MI355X gossip engine.
//
// Design: one kernel launch services EVERY simulated node
// active in a tick sub-phase. Workgroups map 1:1 to nodes; a node's whole
// event sequence for the sub-phase (merge -> local SGD -> reply snapshot)
// runs inside its workgroup so no cross-workgroup ordering is ever needed —
// ordering between sub-phases comes from stream order of the launches.
//
// Kernel inventory (K-numbers from SURVEY.md §2.4):
//   snapshot_kernel       — K-equivalent of ModelHandler.caching
//                           (gossipy/model/handler.py:160-176): arena row
//                           copy instead of copy.deepcopy.
//   tick_logreg_kernel    — K3+K4+K5 fused: per-receiver merge (mean of
//                           state, gossipy/model/handler.py:260-280) +
//                           minibatch SGD on CE(sigmoid(Wx+b))
//                           (gossipy/model/handler.py:235-258,
//                            gossipy/model/nn.py:162-166).
//   tick_linear_kernel    — K1/K2: Pegasos hinge SGD
//                           (gossipy/model/handler.py:416-423) and AdaLine
//                           delta rule (gossipy/model/handler.py:364-368),
//                           one wave per node, weights in registers.
//   tick_mlp_kernel       — K3/K4 generalized: fused MLP fwd/bwd/SGD
//                           (gossipy/model/nn.py:91-99).
//   tick_mlp_wide_kernel  — the same tick for models past the LDS budget
//                           (784-100-10 and up): model rows in device
//                           memory, the minibatch read from the arena.
//   tick_mlp_comp_kernel  — the MLP tick under partitioned / sampled
//                           gossip (gossipy/model/handler.py:426-525),
//                           same SGD body, templated on the merge policy.
//   tick_logreg_lim_kernel, tick_mlp_kernel<true>
//                         — the logreg / MLP ticks with the limited merge
//                           (LimitedMergeMixin._merge,
//                           gossipy/model/handler.py:690-715) in place of
//                           the mean; see lim_rule.
//   tick_pens_kernel, tick_pens_mlp_kernel
//                         — PENS step-1 events (gossipy/node.py:767-782) for
//                           logreg / the MLP: score the cached candidates on
//                           the receiver's shard (the MLP one forward-only on
//                           mlp_update's MFMA stage, mlp_forward), merge the
//                           top-m, run the local update.
//   tick_logreg_big_kernel, tick_logreg_lim_big_kernel, <BIG = true>
//                         — the logreg kernels for batches of more rows
//                           than their 128 threads (full-shard batches of
//                           large shards); picked host-side, see big_batch.
//   tick_logreg_*thin_kernel
//                         — the four logreg kernels with the pipelined
//                           update (dot_chain_pipe, col_chain_exact,
//                           dz_row_regs): a shorter dependent chain for
//                           more registers; picked host-side for launches
//                           of at most one wave per SIMD, see
//                           thin_launch_rows.
//   eval_metrics_kernel   — K13: accuracy / macro P-R-F1 / pairwise AUC of
//                           R affine or margin models (or precomputed
//                           scores) on a shared set or per-node shards.
//   eval_mlp_kernel       — K13 for the MLP family: mlp_forward over the
//                           evaluation rows, then eval_metrics_kernel's
//                           epilogue (eval_epilogue), in one launch.
//
// Models are tiny (57x2 logreg ... few-hundred-wide MLPs); per-launch work
// is launch-latency bound, so kernels are built to let ONE launch cover all
// active nodes and to keep every intermediate in LDS/registers — the D
// parameters are read from HBM once per tick and written once.

#include <torch/extension.h>
#include <pybind11/numpy.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_cooperative_groups.h>

#include <array>
#include <atomic>
#include <chrono>
#include <deque>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "round_check.h"
#include "round_layout.h"
#include "round_ring.h"
#include "round_source.h"

#define DEV_INLINE __device__ __forceinline__

constexpr int KMAX = 16;     // max classes for the logreg path
constexpr int WAVE = 64;

// CreateModelMode numbering shared with engine/backend.py (_MODE_ID)
constexpr int MODE_UPDATE = 0;
constexpr int MODE_MERGE_UPDATE = 1;
constexpr int MODE_UPDATE_MERGE = 2;
constexpr int MODE_PASS = 3;

DEV_INLINE float wave_sum(float v)
{
    for (int off = WAVE / 2; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    return __shfl(v, 0, WAVE);
}

// reduction when only the first <=8 lanes carry data (e.g. the MF rank-k
// dot, k<=8): 3 shuffle steps instead of 6, broadcast to every lane
DEV_INLINE float wave_sum8(float v)
{
    v += __shfl_down(v, 4, WAVE);
    v += __shfl_down(v, 2, WAVE);
    v += __shfl_down(v, 1, WAVE);
    return __shfl(v, 0, WAVE);
}


// ---------------------------------------------------------------------------
// snapshot: slots[slot_ids[i]] = params[nodes[i]]  (+ age)
// ---------------------------------------------------------------------------

__global__ void snapshot_kernel(
    const float* __restrict__ params,
    const int* __restrict__ ages,
    float* __restrict__ slots,
    int* __restrict__ slot_ages,
    const int* __restrict__ nodes,
    const int* __restrict__ slot_ids,
    int n, int W, int Dp, int src_off, int A)
    // W = slot width, Dp = full row width, src_off = sub-block offset
    // (MF snapshots only the item block), A = age width
{
    long total = (long)n * W;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        int row = idx / W;
        int col = idx - (long)row * W;
        int node = nodes[row];
        int slot = slot_ids[row];
        slots[(long)slot * W + col] = params[(long)node * Dp + src_off + col];
        if (col < A) slot_ages[(long)slot * A + col] = ages[(long)node * A + col];
    }
}

// ---------------------------------------------------------------------------
// logreg tick: one workgroup per active node
// ---------------------------------------------------------------------------

struct LogregArgs {
    float* params; int* ages;
    float* slots; int* slot_ages;
    const int* nodes; const int* ptr;
    const int* dslots; const int* rslots;
    const int* dmodes;  // per-delivery pass-through flag (1 = PASS), or null
    const float* X; const float* Y; const int* counts;
    int d, k, Smax, D;
    float lr, wd;
    int epochs, bs, mode, update_only;
    int lim;  // limited-merge threshold L (LIM kernels only); last member
};

// Limited merge (Danner 2023; LimitedMergeMixin._merge,
// gossipy/model/handler.py:690-715): with a the receiver's age and b the
// received model's, keep the own row when a > b + L, adopt the received row
// when b > a + L, else W = m1*W + m2*S with m1 = a/(a+b), m2 = b/(a+b) in
// fp32 ((1/2, 1/2) when a + b == 0, where the reference divides by zero).
// The age becomes max(a, b) in every branch. All fields are wave-uniform.
constexpr int LIM_KEEP = 0, LIM_ADOPT = 1, LIM_MIX = 2;

struct LimRule {
    int br;
    float m1, m2;
};

DEV_INLINE LimRule lim_rule(int a, int b, int L)
{
    LimRule r{LIM_MIX, 0.5f, 0.5f};
    if (a > b + L) {
        r.br = LIM_KEEP;
    } else if (b > a + L) {
        r.br = LIM_ADOPT;
    } else if (a + b != 0) {
        float s = (float)(a + b);
        r.m1 = (float)a / s;
        r.m2 = (float)b / s;
    }
    return r;
}

// W[e] <- rule(W[e], S[e]) over a block-strided row; S is read only when
// the rule needs it
DEV_INLINE void lim_merge_row(const LimRule& r, float* W, const float* S,
                              int D)
{
    if (r.br == LIM_KEEP) return;
    if (r.br == LIM_ADOPT) {
        for (int e = threadIdx.x; e < D; e += blockDim.x) W[e] = S[e];
    } else {
        for (int e = threadIdx.x; e < D; e += blockDim.x)
            W[e] = r.m1 * W[e] + r.m2 * S[e];
    }
}

// Latency-chain helpers. A workgroup here is a handful of waves working on
// one tiny model, so every loop below is bound by memory round trips, not
// by throughput: a read that is waited for before the next one is issued
// costs a full LDS (or HBM) latency per element. Each helper therefore
// issues a fixed block of CH reads into registers before the first use.
constexpr int CH = 8;

// dst[e] = src[e], e < n, block-strided; all of a thread's loads of a
// chunk are in flight before its first store (any address spaces)
template <int U = CH>
DEV_INLINE void copy_row(float* dst, const float* src, int n)
{
    int tid = threadIdx.x, bd = blockDim.x;
    for (int base = tid; base < n; base += U * bd) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int e = base + u * bd;
            v[u] = (e < n) ? src[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int e = base + u * bd;
            if (e < n) dst[e] = v[u];
        }
    }
}

// W[e] = f(W[e], S[e]), e < D, block-strided, S reads batched
template <typename F>
DEV_INLINE void merge_rows(float* W, const float* S, int D, F f)
{
    int tid = threadIdx.x, bd = blockDim.x;
    for (int base = tid; base < D; base += CH * bd) {
        float v[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            int e = base + u * bd;
            v[u] = (e < D) ? S[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            int e = base + u * bd;
            if (e < D) W[e] = f(W[e], v[u]);
        }
    }
}

// W[e] = f(P[e], S[e]) for e < D and xb[e] = X[e] for e < nx in one pass:
// the three HBM streams of a chunk are in flight before the first LDS write
template <typename F>
DEV_INLINE void fused_stage(float* W, const float* P, const float* S, int D,
                            float* xb, const float* X, int nx, F f)
{
    int tid = threadIdx.x, bd = blockDim.x;
    int n = max(D, nx);
    for (int base = tid; base < n; base += CH * bd) {
        float pv[CH], sv[CH], xv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            int e = base + u * bd;
            pv[u] = (e < D) ? P[e] : 0.f;
            sv[u] = (e < D) ? S[e] : 0.f;
            xv[u] = (e < nx) ? X[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            int e = base + u * bd;
            if (e < D) W[e] = f(pv[u], sv[u]);
            if (e < nx) xb[e] = xv[u];
        }
    }
}

// acc + <w, x> as ONE chain of fused multiply-adds in order e = 0..d-1
// (the arithmetic of `for e: acc += w[e] * x[e]`), with the reads of CH
// elements issued ahead of the CH dependent FMAs
DEV_INLINE float dot_chain(float acc, const float* w, const float* x, int d)
{
    int e0 = 0;
    for (; e0 + CH <= d; e0 += CH) {
        float wv[CH], xv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) { wv[u] = w[e0 + u]; xv[u] = x[e0 + u]; }
#pragma unroll
        for (int u = 0; u < CH; ++u) acc = fmaf(wv[u], xv[u], acc);
    }
    if (e0 < d) {  // tail: clamped reads, masked FMAs
        float wv[CH], xv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            int e = min(e0 + u, d - 1);
            wv[u] = w[e]; xv[u] = x[e];
        }
#pragma unroll
        for (int u = 0; u < CH; ++u)
            if (e0 + u < d) acc = fmaf(wv[u], xv[u], acc);
    }
    return acc;
}

// sum over s = 0..m-1, in that order, of p[s*ps] * q[s*qs] (q == nullptr:
// of p[s*ps]), starting from +0; reads batched as in dot_chain. m >= 1.
DEV_INLINE float col_chain(const float* p, int ps, const float* q, int qs,
                           int m)
{
    float g = 0.f;
    for (int s0 = 0; s0 < m; s0 += CH) {
        float pv[CH], qv[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            int s = min(s0 + u, m - 1);
            pv[u] = p[s * ps];
            qv[u] = q ? q[s * qs] : 0.f;
        }
        if (q) {
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if (s0 + u < m) g = fmaf(pv[u], qv[u], g);
        } else {
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if (s0 + u < m) g += pv[u];
        }
    }
    return g;
}

// dot_chain with two register sets: the
// reads of chunk n+1 are in flight under the FMAs of chunk n. d must be
// wave-uniform: the tail reads and adds exactly d % CH elements behind
// scalar branches.
DEV_INLINE float dot_chain_pipe(float acc, const float* w, const float* x, int d)
{
    float wa[CH], xa[CH], wb[CH], xb[CH];
    auto load = [&](float* wv, float* xv, int e) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < CH; ++u) { wv[u] = w[e + u]; xv[u] = x[e + u]; }
    };
    auto fma = [&](const float* wv, const float* xv) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < CH; ++u) acc = fmaf(wv[u], xv[u], acc);
    };
    int e0 = 0;
    if (CH <= d) load(wa, xa, 0);
    // set a holds chunk e0; the body has no branch, so each FMA block waits
    // only for its own set's reads. The fences pin that order: the
    // scheduler otherwise sinks each set's reads into the FMAs before it.
    for (; e0 + 3 * CH <= d; e0 += 2 * CH) {
        load(wb, xb, e0 + CH);
        __builtin_amdgcn_sched_barrier(0);
        fma(wa, xa);
        __builtin_amdgcn_sched_barrier(0);
        load(wa, xa, e0 + 2 * CH);
        __builtin_amdgcn_sched_barrier(0);
        fma(wb, xb);
        __builtin_amdgcn_sched_barrier(0);
    }
    // one or two whole chunks are left when d >= CH, the first of them in a
    if (e0 + 2 * CH <= d) {
        load(wb, xb, e0 + CH);
        fma(wa, xa);
        fma(wb, xb);
        e0 += 2 * CH;
    } else if (e0 + CH <= d) {
        fma(wa, xa);
        e0 += CH;
    }
    // one tail for every path: the d - e0 < CH elements, into set b
    int r = d - e0;
#pragma unroll
    for (int u = 0; u < CH - 1; ++u) {
        if (u >= r) break;
        wb[u] = w[e0 + u]; xb[u] = x[e0 + u];
    }
#pragma unroll
    for (int u = 0; u < CH - 1; ++u) {
        if (u >= r) break;
        acc = fmaf(wb[u], xb[u], acc);
        // a real scalar branch, not an FMA masked by a select
        asm volatile("" : "+v"(acc));
    }
    return acc;
}

// col_chain (Q false: its q == nullptr form) whose short last chunk reads
// no clamped element and adds behind no select. m >= 1 is
// the same in every thread of the block: a short last chunk reads and adds
// exactly its own elements behind scalar branches.
template <bool Q = true>  // false: no q, the sum of p alone
DEV_INLINE float col_chain_exact(const float* p, int ps, const float* q, int qs,
                           int m)
{
    m = __builtin_amdgcn_readfirstlane(m);
    float g = 0.f;
    for (int s0 = 0; s0 < m; s0 += CH) {
        float pv[CH], qv[CH];
        int r = min(CH, m - s0);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            if (u >= r) break;
            pv[u] = p[(s0 + u) * ps];
            if constexpr (Q) qv[u] = q[(s0 + u) * qs];
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            if (u >= r) break;
            if constexpr (Q) g = fmaf(pv[u], qv[u], g); else g += pv[u];
            // a real scalar branch, not an add masked by a select
            asm volatile("" : "+v"(g));
        }
    }
    return g;
}

// dLoss/dz of one sample for a compile-time class count: the K scores are
// read once, every pass runs on registers with static indices, the K
// results are written once. The operations and their order are those of the
// generic loop in logreg_update, which recomputes exp(sg - amax) where this
// keeps it.
template <int K>
DEV_INLINE void dz_row_regs(float* zs, float y, int m)
{
    float sg[K], pk[K];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) sg[kk] = zs[kk];
    float amax = -1e30f;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        sg[kk] = 1.0f / (1.0f + __expf(-sg[kk]));
        amax = fmaxf(amax, sg[kk]);
    }
    float sum = 0.f;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        pk[kk] = __expf(sg[kk] - amax);
        sum += pk[kk];
    }
    int yi = (int)y;
    float inv = 1.0f / sum;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        float g = pk[kk] * inv - (kk == yi ? 1.0f : 0.0f);
        zs[kk] = (g / m) * sg[kk] * (1.0f - sg[kk]);
    }
}

// Minibatch SGD epochs over the node's shard, on the LDS-resident model W.
// xb/dz are LDS scratch; age is a wave-uniform register; c = counts[node],
// read once by the caller.
// BIG = a batch may have more rows than the block has threads: the
// per-sample stage strides over the batch. The host picks the instantiation
// from the largest batch (big_batch), so the default one, which every shard
// of at most blockDim rows runs, keeps its one-pass stage.
// PIPE = the forward and the reductions run through dot_chain_pipe and
// col_chain_exact and a two-class dLoss/dz row through dz_row_regs: the same
// arithmetic in the same order, a shorter chain per delivery, about 40 more
// VGPRs. Only the thin instantiations of the tick kernels use it.
template <bool BIG = false, bool PIPE = false>
DEV_INLINE void logreg_update(const LogregArgs& a, int node, int c, float* W,
                              float* xb, float* dz, int& age,
                              int prestaged = 0)
{
    int tid = threadIdx.x;
    if (c == 0) return;
    int bsz = (a.bs == 0) ? c : min(a.bs, c);
    const float* Xn = a.X + (long)node * a.Smax * a.d;
    const float* Yn = a.Y + (long)node * a.Smax;
    // single-batch shards (every BASELINE config): xb stays valid across
    // epochs AND deliveries, so it is staged at most once per receiver row
    int xb_valid = prestaged;
    for (int ep = 0; ep < a.epochs; ++ep) {
        for (int s0 = 0; s0 < c; s0 += bsz) {
            int m = min(bsz, c - s0);
            // the label is consumed only in the dz stage: its HBM trip
            // hides under the staging and the forward pass
            float yv = (tid < m) ? Yn[s0 + tid] : 0.f;
            // stage the batch in LDS (coalesced: consecutive threads read
            // consecutive floats of the shard); the caller may have staged
            // the very first batch already (fused with the W load)
            if (!xb_valid) copy_row(xb, Xn + (long)s0 * a.d, m * a.d);
            xb_valid = (c <= bsz);
            __syncthreads();
            // forward: the m*k (sample, class) scores spread over the
            // block, parked in the dz area
            for (int pr = tid; pr < m * a.k; pr += blockDim.x) {
                int s = pr / a.k, kk = pr - s * a.k;
                const float* wk = W + kk * a.d;
                const float* xs = xb + s * a.d;
                float bias = W[a.k * a.d + kk];
                if constexpr (PIPE) dz[pr] = dot_chain_pipe(bias, wk, xs, a.d);
                else dz[pr] = dot_chain(bias, wk, xs, a.d);
            }
            __syncthreads();
            // dLoss/dz of sample s with label y, in place over the sample's
            // own k scores: a = sigmoid(z); p = softmax(a);
            // dz = (p - 1_y)/m * a*(1-a)
            auto dz_row = [&](int s, float y) __attribute__((always_inline)) {
                float* zs = dz + s * a.k;
                if constexpr (PIPE) {
                    if (a.k == 2) {  // the binary row stays in registers
                        dz_row_regs<2>(zs, y, m);
                        return;
                    }
                }
                float amax = -1e30f;
                for (int kk = 0; kk < a.k; ++kk) {
                    float sg = 1.0f / (1.0f + __expf(-zs[kk]));
                    zs[kk] = sg;
                    amax = fmaxf(amax, sg);
                }
                float sum = 0.f;
                for (int kk = 0; kk < a.k; ++kk) sum += __expf(zs[kk] - amax);
                int yi = (int)y;
                float inv = 1.0f / sum;
                for (int kk = 0; kk < a.k; ++kk) {
                    float sg = zs[kk];
                    float pk = __expf(sg - amax);
                    float g = pk * inv - (kk == yi ? 1.0f : 0.0f);
                    zs[kk] = (g / m) * sg * (1.0f - sg);
                }
            };
            // thread = sample; the first pass uses the prefetched label
            if (tid < m) dz_row(tid, yv);
            if constexpr (BIG) {
                for (int s = tid + blockDim.x; s < m; s += blockDim.x)
                    dz_row(s, Yn[s0 + s]);
            }
            __syncthreads();
            // SGD step (thread = parameter)
            for (int e = tid; e < a.k * a.d; e += blockDim.x) {
                int kk = e / a.d, dd = e - kk * a.d;
                float g = PIPE
                    ? col_chain_exact<true>(dz + kk, a.k, xb + dd, a.d, m)
                    : col_chain(dz + kk, a.k, xb + dd, a.d, m);
                if (a.wd != 0.f) g += a.wd * W[e];
                W[e] -= a.lr * g;
            }
            for (int e = tid; e < a.k; e += blockDim.x) {
                float g = PIPE
                    ? col_chain_exact<false>(dz + e, a.k, nullptr, 0, m)
                    : col_chain(dz + e, a.k, nullptr, 0, m);
                W[a.k * a.d + e] -= a.lr * g;
            }
            __syncthreads();
            age += 1;  // wave-uniform (gossipy/model/handler.py:258)
        }
    }
}

// LIM = limited merge: every mean merge below becomes lim_rule on the two
// ages at that point. The plain instantiation compiles to the mean-merge
// code unchanged.
template <bool LIM, bool BIG = false, bool PIPE = false>
DEV_INLINE void logreg_process_node(const LogregArgs& a, int i)
{
    int node = a.nodes[i];
    int tid = threadIdx.x;
    int c = a.counts[node];  // once per receiver row
    extern __shared__ float sm[];
    float* W = sm;                         // D
    float* W2 = W + a.D;                   // D (UPDATE_MERGE scratch)
    float* xb = W2 + a.D;                  // bsmax*d
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    float* dz = xb + bsmax * a.d;          // bsmax*k

    // Fast path for the common MERGE_UPDATE single-sequence case: fuse the
    // model load with the FIRST delivery's merge and prefetch the first
    // minibatch in the same phase — three independent HBM streams behind
    // one barrier instead of three serial chains.
    int j0 = a.update_only ? 0 : a.ptr[i];
    int j1 = a.update_only ? 0 : a.ptr[i + 1];
    if (!a.update_only && j1 > j0 && a.mode == MODE_MERGE_UPDATE &&
        !(a.dmodes && a.dmodes[j0])) {
        int slot = a.dslots[j0];
        const float* srow = a.slots + (long)slot * a.D;
        const float* prow = a.params + (long)node * a.D;
        const float* X0 = a.X + (long)node * a.Smax * a.d;
        int age0 = a.ages[node], sage0 = a.slot_ages[slot];
        int m0 = min((a.bs == 0) ? max(c, 1) : a.bs, c);
        if constexpr (LIM) {
            // both ages are needed before the fused load, not after it
            LimRule r0 = lim_rule(age0, sage0, a.lim);
            if (r0.br == LIM_KEEP) {
                fused_stage(W, prow, srow, a.D, xb, X0, m0 * a.d,
                            [](float p, float) { return p; });
            } else if (r0.br == LIM_ADOPT) {
                fused_stage(W, prow, srow, a.D, xb, X0, m0 * a.d,
                            [](float, float s) { return s; });
            } else {
                fused_stage(W, prow, srow, a.D, xb, X0, m0 * a.d,
                            [&](float p, float s) {
                                return r0.m1 * p + r0.m2 * s;
                            });
            }
        } else {
            fused_stage(W, prow, srow, a.D, xb, X0, m0 * a.d,
                        [](float p, float s) { return 0.5f * (p + s); });
        }
        __syncthreads();
        int age = max(age0, sage0);
        // xb holds batch 0 after the fused stage above; it STAYS valid for
        // later deliveries only when the shard is a single batch
        int xb_keep = (a.bs == 0) || (c <= a.bs);
        // register double-buffer: issue the NEXT delivery's slot-row loads
        // before each (long) update so the HBM latency hides under compute
        constexpr int PRE = 8;
        float pre[PRE];
        int pre_age = 0;
        int npre = min(a.D, PRE * (int)blockDim.x);
        auto issue_pre = [&](int j) {
            if (j < j1 && !(a.dmodes && a.dmodes[j])) {
                const float* srow2 = a.slots + (long)a.dslots[j] * a.D;
                for (int u = 0; u < PRE; ++u) {
                    int e = tid + u * (int)blockDim.x;
                    pre[u] = (e < a.D) ? srow2[e] : 0.f;
                }
                pre_age = a.slot_ages[a.dslots[j]];
            }
        };
        issue_pre(j0 + 1);
        logreg_update<BIG, PIPE>(a, node, c, W, xb, dz, age, /*prestaged=*/1);
        int rs0 = a.rslots ? a.rslots[j0] : -1;
        if (rs0 >= 0) {  // first delivery's PUSH_PULL reply snapshot
            copy_row(a.slots + (long)rs0 * a.D, W, a.D);
            if (tid == 0) a.slot_ages[rs0] = age;
            __syncthreads();
        }
        for (int j = j0 + 1; j < j1; ++j) {
            int slot2 = a.dslots[j];
            const float* srow2 = a.slots + (long)slot2 * a.D;
            int md = (a.dmodes && a.dmodes[j]) ? MODE_PASS : a.mode;
            if (md == MODE_MERGE_UPDATE) {
                if constexpr (LIM) {
                    // pre[] and pre_age were issued before the previous
                    // delivery's SGD; the weights need the age AFTER it
                    LimRule r = lim_rule(age, pre_age, a.lim);
                    if (r.br == LIM_ADOPT) {
                        for (int u = 0; u < PRE; ++u) {
                            int e = tid + u * (int)blockDim.x;
                            if (e < a.D) W[e] = pre[u];
                        }
                        copy_row(W + npre, srow2 + npre, a.D - npre);
                    } else if (r.br == LIM_MIX) {
                        for (int u = 0; u < PRE; ++u) {
                            int e = tid + u * (int)blockDim.x;
                            if (e < a.D) W[e] = r.m1 * W[e] + r.m2 * pre[u];
                        }
                        merge_rows(W + npre, srow2 + npre, a.D - npre,
                                   [&](float w, float s) {
                                       return r.m1 * w + r.m2 * s;
                                   });
                    }
                } else {
                    for (int u = 0; u < PRE; ++u) {
                        int e = tid + u * (int)blockDim.x;
                        if (e < a.D) W[e] = 0.5f * (W[e] + pre[u]);
                    }
                    merge_rows(W + npre, srow2 + npre, a.D - npre,
                               [](float w, float s) { return 0.5f * (w + s); });
                }
                age = max(age, pre_age);
                __syncthreads();
                issue_pre(j + 1);
                logreg_update<BIG, PIPE>(a, node, c, W, xb, dz, age, /*prestaged=*/xb_keep);
            } else {  // PASS (pass-through coin resolved to adopt)
                copy_row(W, srow2, a.D);
                age = a.slot_ages[slot2];
                __syncthreads();
                issue_pre(j + 1);
            }
            int rs2 = a.rslots ? a.rslots[j] : -1;
            if (rs2 >= 0) {
                copy_row(a.slots + (long)rs2 * a.D, W, a.D);
                if (tid == 0) a.slot_ages[rs2] = age;
                __syncthreads();
            }
        }
        __syncthreads();
        copy_row(a.params + (long)node * a.D, W, a.D);
        if (tid == 0) a.ages[node] = age;
        return;
    }

    copy_row(W, a.params + (long)node * a.D, a.D);
    __syncthreads();
    int age = a.ages[node];

    if (a.update_only) {
        logreg_update<BIG, PIPE>(a, node, c, W, xb, dz, age);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            const float* srow = a.slots + (long)slot * a.D;
            int sage = a.slot_ages[slot];
            // pass-through gossip resolves some deliveries to PASS
            // (gossipy/node.py:380-392)
            int md = (a.dmodes && a.dmodes[j]) ? MODE_PASS : a.mode;
            if (md == MODE_MERGE_UPDATE) {
                if constexpr (LIM) {
                    lim_merge_row(lim_rule(age, sage, a.lim), W, srow, a.D);
                } else {
                    merge_rows(W, srow, a.D, [](float w, float s) {
                        return 0.5f * (w + s);
                    });
                }
                age = max(age, sage);
                __syncthreads();
                logreg_update<BIG, PIPE>(a, node, c, W, xb, dz, age);
            } else if (md == MODE_UPDATE) {
                // adopt the received model, then train it
                copy_row(W, srow, a.D);
                age = sage;
                __syncthreads();
                logreg_update<BIG, PIPE>(a, node, c, W, xb, dz, age);
            } else if (md == MODE_UPDATE_MERGE) {
                logreg_update<BIG, PIPE>(a, node, c, W, xb, dz, age);
                copy_row(W2, srow, a.D);
                __syncthreads();
                int age2 = sage;
                logreg_update<BIG, PIPE>(a, node, c, W2, xb, dz, age2);
                if constexpr (LIM) {
                    // the rule sees the two post-training ages
                    lim_merge_row(lim_rule(age, age2, a.lim), W, W2, a.D);
                } else {
                    for (int e = tid; e < a.D; e += blockDim.x)
                        W[e] = 0.5f * (W[e] + W2[e]);
                }
                age = max(age, age2);
                __syncthreads();
            } else {  // PASS
                copy_row(W, srow, a.D);
                age = sage;
                __syncthreads();
            }
            // reply-delivery launches pass rslots == nullptr (replies to
            // replies are discarded, gossipy/simul.py:426)
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {  // PUSH_PULL reply snapshot (post merge+update)
                copy_row(a.slots + (long)rs * a.D, W, a.D);
                if (tid == 0) a.slot_ages[rs] = age;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    copy_row(a.params + (long)node * a.D, W, a.D);
    if (tid == 0) a.ages[node] = age;
}

__global__ void __launch_bounds__(128)
tick_logreg_kernel(LogregArgs a)
{
    logreg_process_node<false>(a, blockIdx.x);
}

__global__ void __launch_bounds__(128)
tick_logreg_lim_kernel(LogregArgs a)
{
    logreg_process_node<true>(a, blockIdx.x);
}

// the same two for batches of more rows than the block has threads
__global__ void __launch_bounds__(128)
tick_logreg_big_kernel(LogregArgs a)
{
    logreg_process_node<false, true>(a, blockIdx.x);
}

__global__ void __launch_bounds__(128)
tick_logreg_lim_big_kernel(LogregArgs a)
{
    logreg_process_node<true, true>(a, blockIdx.x);
}

// the same four for thin launches (Plan::thin_rows): the pipelined update,
// whose registers cost no occupancy while every wave has a SIMD to itself
__global__ void __launch_bounds__(128)
tick_logreg_thin_kernel(LogregArgs a)
{
    logreg_process_node<false, false, true>(a, blockIdx.x);
}

__global__ void __launch_bounds__(128)
tick_logreg_lim_thin_kernel(LogregArgs a)
{
    logreg_process_node<true, false, true>(a, blockIdx.x);
}

__global__ void __launch_bounds__(128)
tick_logreg_big_thin_kernel(LogregArgs a)
{
    logreg_process_node<false, true, true>(a, blockIdx.x);
}

__global__ void __launch_bounds__(128)
tick_logreg_lim_big_thin_kernel(LogregArgs a)
{
    logreg_process_node<true, true, true>(a, blockIdx.x);
}

// ---------------------------------------------------------------------------
// all2all weighted k-way merge (K5 weighted variant; WeightedTMH._merge,
// gossipy/model/handler.py:666-688): params[n] = w0*params[n] + sum_j
// w_j*slots[s_j]; age = max over merged. Family-agnostic (elementwise over
// D); the per-family update-only kernel runs right after it.
// ---------------------------------------------------------------------------

__global__ void wmerge_kernel(
    float* __restrict__ params,
    int* __restrict__ ages,
    const float* __restrict__ slots,
    const int* __restrict__ slot_ages,
    const int* __restrict__ nodes,
    const int* __restrict__ ptr,
    const int* __restrict__ wslots,
    const float* __restrict__ wweights,
    const float* __restrict__ selfw,
    int D)
{
    int i = blockIdx.x;
    int node = nodes[i];
    int tid = threadIdx.x;
    int lo = ptr[i], hi = ptr[i + 1];
    float w0 = selfw[i];
    for (int e = tid; e < D; e += blockDim.x) {
        float acc = w0 * params[(long)node * D + e];
        for (int j = lo; j < hi; ++j)
            acc += wweights[j] * slots[(long)wslots[j] * D + e];
        params[(long)node * D + e] = acc;
    }
    if (tid == 0) {
        int age = ages[node];
        for (int j = lo; j < hi; ++j) age = max(age, slot_ages[wslots[j]]);
        ages[node] = age;
    }
}

// ---------------------------------------------------------------------------
// partitioned logreg tick (K7/K8, PartitionedTMH semantics)
//
// Parity: gossipy/model/handler.py:455-525 + gossipy/model/sampling.py:
// 201-234. Each node keeps a per-partition age vector; a delivery merges
// ONE partition (age-weighted), and each local batch increments every
// partition age then divides each parameter's gradient by its partition's
// age. The partition cover is the reference's F-flat equal split mapped to
// arena offsets via the device-resident perm/pptr arrays (engine/models.py
// _PartitionMixin).
// ---------------------------------------------------------------------------

struct LogregPartArgs {
    float* params; int* ages;            // ages: [n_local, P]
    float* slots; int* slot_ages;        // slot_ages: [cap, P]
    const int* nodes; const int* ptr;
    const int* dslots; const int* rslots; const int* dpids;
    const float* X; const float* Y; const int* counts;
    const int* perm;   // [D]  partition-ordered -> arena offset
    const int* pptr;   // [P+1]
    const int* apart;  // [D]  arena offset -> partition id
    int P, d, k, Smax, D;
    float lr, wd;
    int epochs, bs, mode, update_only;
    //: xb holds the WHOLE shard (staged once per receiver row) instead of
    //: one re-staged minibatch slice per step per delivery — decided
    //: host-side from the LDS budget. The reference math is unchanged;
    //: the staging was the tokenized row's repeated HBM round trip.
    int stage_full;
};

// Minibatch SGD with whole-age-vector increment per batch and per-partition
// gradient rescale (gossipy/model/handler.py:503-520).
DEV_INLINE void logreg_part_update(const LogregPartArgs& a, int node, float* W,
                                   int* agev, float* xb, float* dz)
{
    int tid = threadIdx.x;
    int c = a.counts[node];
    if (c == 0) return;
    int bsz = (a.bs == 0) ? c : min(a.bs, c);
    const float* Xn = a.X + (long)node * a.Smax * a.d;
    const float* Yn = a.Y + (long)node * a.Smax;
    for (int ep = 0; ep < a.epochs; ++ep) {
        for (int s0 = 0; s0 < c; s0 += bsz) {
            int m = min(bsz, c - s0);
            float* xs = a.stage_full ? xb + (long)s0 * a.d : xb;
            if (!a.stage_full) {
                for (int e = tid; e < m * a.d; e += blockDim.x)
                    xb[e] = Xn[(long)s0 * a.d + e];
            }
            // self.n_updates += 1 happens before the step (handler.py:506)
            for (int p = tid; p < a.P; p += blockDim.x) agev[p] += 1;
            __syncthreads();
            // thread = sample, block-strided: a batch may have more rows
            // than the block has threads
            for (int s = tid; s < m; s += blockDim.x) {
                float z[KMAX];
                for (int kk = 0; kk < a.k; ++kk) {
                    float acc = W[a.k * a.d + kk];
                    const float* wrow = W + kk * a.d;
                    const float* xrow = xs + s * a.d;
                    for (int dd = 0; dd < a.d; ++dd) acc += wrow[dd] * xrow[dd];
                    z[kk] = acc;
                }
                float amax = -1e30f;
                for (int kk = 0; kk < a.k; ++kk) {
                    z[kk] = 1.0f / (1.0f + __expf(-z[kk]));
                    amax = fmaxf(amax, z[kk]);
                }
                float sum = 0.f;
                float p[KMAX];
                for (int kk = 0; kk < a.k; ++kk) {
                    p[kk] = __expf(z[kk] - amax);
                    sum += p[kk];
                }
                int yi = (int)Yn[s0 + s];
                float inv = 1.0f / sum;
                for (int kk = 0; kk < a.k; ++kk) {
                    float g = p[kk] * inv - (kk == yi ? 1.0f : 0.0f);
                    dz[s * a.k + kk] = (g / m) * z[kk] * (1.0f - z[kk]);
                }
            }
            __syncthreads();
            for (int e = tid; e < a.k * a.d; e += blockDim.x) {
                int kk = e / a.d, dd = e - kk * a.d;
                float g = 0.f;
                for (int s = 0; s < m; ++s) g += dz[s * a.k + kk] * xs[s * a.d + dd];
                g /= (float)agev[a.apart[e]];  // _adjust_gradient
                if (a.wd != 0.f) g += a.wd * W[e];
                W[e] -= a.lr * g;
            }
            for (int e = tid; e < a.k; e += blockDim.x) {
                float g = 0.f;
                for (int s = 0; s < m; ++s) g += dz[s * a.k + e];
                g /= (float)agev[a.apart[a.k * a.d + e]];
                if (a.wd != 0.f) g += a.wd * W[a.k * a.d + e];
                W[a.k * a.d + e] -= a.lr * g;
            }
            __syncthreads();
        }
    }
}

// Age-weighted merge of partition `pid` of src into W
// (handler.py:497-501; weights (0,0) -> (1,1)). src/src_ages may point to
// LDS (trained received model) or HBM (slot row).
DEV_INLINE void logreg_part_merge(const LogregPartArgs& a, float* W, int* agev,
                                  const float* src, const int* src_ages, int pid)
{
    int tid = threadIdx.x;
    int w1 = agev[pid], w2 = src_ages[pid];
    float m1, m2;
    if (w1 == 0 && w2 == 0) { m1 = 0.5f; m2 = 0.5f; }
    else {
        float s = (float)(w1 + w2);
        m1 = (float)w1 / s;
        m2 = (float)w2 / s;
    }
    __syncthreads();
    for (int e = a.pptr[pid] + tid; e < a.pptr[pid + 1]; e += blockDim.x) {
        int i = a.perm[e];
        W[i] = m1 * W[i] + m2 * src[i];
    }
    __syncthreads();
    if (tid == 0) agev[pid] = max(w1, w2);
    __syncthreads();
}

DEV_INLINE void logreg_part_process_node(const LogregPartArgs& a, int i)
{
    int node = a.nodes[i];
    int tid = threadIdx.x;
    extern __shared__ float sm[];
    float* W = sm;                         // D
    float* W2 = W + a.D;                   // D (received-model scratch)
    float* xb = W2 + a.D;                  // (stage_full ? Smax : bsmax)*d
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    int xbn = a.stage_full ? a.Smax : bsmax;
    float* dz = xb + xbn * a.d;            // bsmax*k
    int* agev = (int*)(dz + bsmax * a.k);  // P
    int* agev2 = agev + a.P;               // P

    for (int e = tid; e < a.D; e += blockDim.x)
        W[e] = a.params[(long)node * a.D + e];
    for (int p = tid; p < a.P; p += blockDim.x)
        agev[p] = a.ages[(long)node * a.P + p];
    if (a.stage_full) {
        // whole shard -> LDS once; every delivery's every minibatch step
        // slices it (the re-staging was a repeated HBM round trip on the
        // tokenized row's sequential chains)
        int c = a.counts[node];
        const float* Xn = a.X + (long)node * a.Smax * a.d;
        for (int e = tid; e < c * a.d; e += blockDim.x) xb[e] = Xn[e];
    }
    __syncthreads();

    if (a.update_only) {
        logreg_part_update(a, node, W, agev, xb, dz);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            int pid = a.dpids ? a.dpids[j] : 0;
            const float* srow = a.slots + (long)slot * a.D;
            const int* sages = a.slot_ages + (long)slot * a.P;
            if (a.mode == MODE_MERGE_UPDATE) {
                logreg_part_merge(a, W, agev, srow, sages, pid);
                logreg_part_update(a, node, W, agev, xb, dz);
            } else {
                // UPDATE: train the received model, merge its partition
                // (handler.py:481-483). UPDATE_MERGE: also self-update first
                // (handler.py:487-490). PASS is rejected host-side.
                if (a.mode == MODE_UPDATE_MERGE)
                    logreg_part_update(a, node, W, agev, xb, dz);
                for (int e = tid; e < a.D; e += blockDim.x) W2[e] = srow[e];
                for (int p = tid; p < a.P; p += blockDim.x) agev2[p] = sages[p];
                __syncthreads();
                logreg_part_update(a, node, W2, agev2, xb, dz);
                logreg_part_merge(a, W, agev, W2, agev2, pid);
            }
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)rs * a.D + e] = W[e];
                for (int p = tid; p < a.P; p += blockDim.x)
                    a.slot_ages[(long)rs * a.P + p] = agev[p];
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < a.D; e += blockDim.x)
        a.params[(long)node * a.D + e] = W[e];
    for (int p = tid; p < a.P; p += blockDim.x)
        a.ages[(long)node * a.P + p] = agev[p];
}

__global__ void __launch_bounds__(128)
tick_logreg_part_kernel(LogregPartArgs a)
{
    logreg_part_process_node(a, blockIdx.x);
}

// ---------------------------------------------------------------------------
// sampled logreg tick (K6, SamplingTMH semantics)
//
// Parity: gossipy/model/handler.py:426-452 + gossipy/model/sampling.py:
// 75-107. Each delivery averages only a seeded random coordinate subset
// (with replacement); the index sequence is splitmix64(seed + j) % D —
// bit-identical to engine/rng.py sample_indices, so the torch oracle and
// this kernel draw the same coordinates. Ages are not merged.
// ---------------------------------------------------------------------------

DEV_INLINE unsigned long long splitmix64_dev(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

struct LogregSampArgs {
    float* params; int* ages;
    float* slots; int* slot_ages;
    const int* nodes; const int* ptr;
    const int* dslots; const int* rslots; const int* dseeds;
    const float* X; const float* Y; const int* counts;
    int samp_c, d, k, Smax, D;
    float lr, wd;
    int epochs, bs, mode, update_only;
};

// W3 holds the pre-merge W (duplicate sampled indices must all read the
// ORIGINAL value — torch advanced-index assignment semantics).
DEV_INLINE void logreg_samp_merge(const LogregSampArgs& a, float* W, float* W3,
                                  const float* src, int seed)
{
    int tid = threadIdx.x;
    for (int e = tid; e < a.D; e += blockDim.x) W3[e] = W[e];
    __syncthreads();
    for (int q = tid; q < a.samp_c; q += blockDim.x) {
        int i = (int)(splitmix64_dev((unsigned long long)seed +
                                     (unsigned long long)q) %
                      (unsigned long long)a.D);
        W[i] = 0.5f * (W3[i] + src[i]);
    }
    __syncthreads();
}

template <bool BIG>  // as logreg_update's
__global__ void __launch_bounds__(128)
tick_logreg_samp_kernel(LogregSampArgs a)
{
    int i = blockIdx.x;
    int node = a.nodes[i];
    int tid = threadIdx.x;
    extern __shared__ float sm[];
    float* W = sm;                         // D
    float* W2 = W + a.D;                   // D (received-model scratch)
    float* W3 = W2 + a.D;                  // D (pre-merge snapshot)
    float* xb = W3 + a.D;                  // bsmax*d
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    float* dz = xb + bsmax * a.d;          // bsmax*k

    for (int e = tid; e < a.D; e += blockDim.x)
        W[e] = a.params[(long)node * a.D + e];
    __syncthreads();
    int age = a.ages[node];

    // reuse the plain logreg update math: wrap args in a LogregArgs view
    LogregArgs u;
    u.X = a.X; u.Y = a.Y; u.counts = a.counts;
    u.d = a.d; u.k = a.k; u.Smax = a.Smax; u.D = a.D;
    u.lr = a.lr; u.wd = a.wd; u.epochs = a.epochs; u.bs = a.bs;
    int cn = a.counts[node];

    if (a.update_only) {
        logreg_update<BIG>(u, node, cn, W, xb, dz, age);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            int seed = a.dseeds ? a.dseeds[j] : 0;
            const float* srow = a.slots + (long)slot * a.D;
            int sage = a.slot_ages[slot];
            if (a.mode == MODE_MERGE_UPDATE) {
                logreg_samp_merge(a, W, W3, srow, seed);
                logreg_update<BIG>(u, node, cn, W, xb, dz, age);
            } else {
                // UPDATE: train received, merge its sample into self
                // (handler.py:440-442); UPDATE_MERGE: self-update first
                // (handler.py:445-448)
                if (a.mode == MODE_UPDATE_MERGE)
                    logreg_update<BIG>(u, node, cn, W, xb, dz, age);
                for (int e = tid; e < a.D; e += blockDim.x) W2[e] = srow[e];
                __syncthreads();
                int age2 = sage;
                logreg_update<BIG>(u, node, cn, W2, xb, dz, age2);
                logreg_samp_merge(a, W, W3, W2, seed);
            }
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)rs * a.D + e] = W[e];
                if (tid == 0) a.slot_ages[rs] = age;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < a.D; e += blockDim.x)
        a.params[(long)node * a.D + e] = W[e];
    if (tid == 0) a.ages[node] = age;
}

// ---------------------------------------------------------------------------
// matrix-factorization tick (K9/K10, MFModelHandler semantics)
//
// Parity: gossipy/model/handler.py:528-576. Per delivery: item-block
// age-weighted merge with the reference's extra /2 (n_updates NOT merged),
// then per-rating SGD where Y[i] uses the OLD X and X uses the NEW Y[i].
// One wavefront per receiver: lanes cover the k latent dims in the rating
// loop and stride the item block in the merge.
// ---------------------------------------------------------------------------

struct MFArgs {
    float* params; int* ages;
    float* slots; int* slot_ages;
    const int* nodes; const int* ptr;
    const int* dslots; const int* rslots;
    const float* X; const float* Y; const int* counts;  // items ride X[:,:,0]
    int k, n_items, Smax, D, item_off, Wslot;
    float reg, lr;
    int update_only;
};

DEV_INLINE void mf_update(const MFArgs& a, int node, float* row, int& age)
{
    // per-rating chain is order-dependent: wave 0 runs it; other waves of
    // the (wider) block idle here and rejoin at the caller's barrier.
    //
    // The chain is the MF round's critical path (551 µs/dispatch measured
    // at 10k nodes, 83% of round GPU time), so it is register-pipelined:
    // the user factors X and both biases live in REGISTERS for the whole
    // sweep (merges never touch them — they only rewrite the item block),
    // and the NEXT rating's item row + item bias are prefetched while the
    // current rating computes. A prefetch of the item just updated is
    // patched from registers (exact — the only write between prefetch and
    // use is the current item's).
    int lane = threadIdx.x;
    if (lane >= WAVE) return;
    int c = a.counts[node];
    if (c == 0) return;
    const float* items = a.X + (long)node * a.Smax;
    const float* ratings = a.Y + (long)node * a.Smax;
    float shrink = 1.0f - a.reg * a.lr;
    int coff = a.item_off + a.n_items * a.k;
    float x = (lane < a.k) ? row[lane] : 0.f;
    float b = row[a.k];
    int item = (int)items[0];
    float* Yi = row + a.item_off + (long)item * a.k;
    float yi = (lane < a.k) ? Yi[lane] : 0.f;
    float ci = row[coff + item];
    for (int s = 0; s < c; ++s) {
        int item_n = 0;
        float* Yi_n = nullptr;
        float yi_n = 0.f, ci_n = 0.f;
        if (s + 1 < c) {  // prefetch next item row + bias
            item_n = (int)items[s + 1];
            Yi_n = row + a.item_off + (long)item_n * a.k;
            yi_n = (lane < a.k) ? Yi_n[lane] : 0.f;
            ci_n = row[coff + item_n];
        }
        float r = ratings[s];
        float part = (lane < a.k) ? x * yi : 0.f;
        // k <= 8: 3-step reduction, bit-identical to the 64-lane tree
        // (the extra lanes only ever add zeros, so the pairings match)
        float dot = (a.k <= 8) ? wave_sum8(part) : wave_sum(part);
        float err = r - dot - b - ci;
        float yi_new = shrink * yi + a.lr * err * x;
        float ci_new = ci + a.lr * err;
        if (lane < a.k) {
            Yi[lane] = yi_new;
            x = shrink * x + a.lr * err * yi_new;
        }
        if (lane == 0) row[coff + item] = ci_new;
        b += a.lr * err;
        age += 1;
        if (s + 1 < c) {
            if (item_n == item) {  // re-rated item: fix up from registers
                yi_n = yi_new;
                ci_n = ci_new;
            }
            item = item_n;
            Yi = Yi_n;
            yi = yi_n;
            ci = ci_n;
        }
    }
    if (lane < a.k) row[lane] = x;
    if (lane == 0) row[a.k] = b;
}

DEV_INLINE void mf_merge(const MFArgs& a, float* row, int age,
                         const float* srow, int sage)
{
    float den = 2.0f * (age + sage);
    float w1 = (float)age / den, w2 = (float)sage / den;
    for (int e = threadIdx.x; e < a.Wslot; e += blockDim.x)
        row[a.item_off + e] = w1 * row[a.item_off + e] + w2 * srow[e];
}

__global__ void __launch_bounds__(256)
tick_mf_kernel(MFArgs a)
{
    // 256 threads: the item-block merge/copy loops (tens of KB per row)
    // use the full block; the order-dependent rating chain runs on wave 0
    int i = blockIdx.x;
    int node = a.nodes[i];
    float* row = a.params + (long)node * a.D;
    int age = a.ages[node];
    if (a.update_only) {
        mf_update(a, node, row, age);
        __syncthreads();
    } else {
        __shared__ int age_sh;
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            mf_merge(a, row, age, a.slots + (long)slot * a.Wslot,
                     a.slot_ages[slot]);
            __syncthreads();
            mf_update(a, node, row, age);
            __syncthreads();
            // the rating chain ran on wave 0 only — rebroadcast the age so
            // a second delivery's merge weights agree across all waves
            if (threadIdx.x == 0) age_sh = age;
            __syncthreads();
            age = age_sh;
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int e = threadIdx.x; e < a.Wslot; e += blockDim.x)
                    a.slots[(long)rs * a.Wslot + e] = row[a.item_off + e];
                // thread 0 (wave 0) holds the post-update age
                if (threadIdx.x == 0) a.slot_ages[rs] = age;
                __syncthreads();
            }
        }
    }
    if (threadIdx.x == 0) a.ages[node] = age;
}

// ---------------------------------------------------------------------------
// k-means tick (K11, KMeansHandler semantics, naive matching)
//
// Parity: gossipy/model/handler.py:579-639. Per update call: every sample
// assigns to its nearest centroid; the EMA applies with torch
// indexed-assignment semantics — per centroid only the LAST assigned
// sample lands (handler.py:613-615); n_updates bumps once per call and is
// never merged. Centroids live in LDS.
// ---------------------------------------------------------------------------

struct KMeansArgs {
    float* params; int* ages;
    float* slots; int* slot_ages;
    const int* nodes; const int* ptr;
    const int* dslots; const int* rslots;
    const float* X; const int* counts;
    int k, dim, Smax, D;
    float alpha;
    int mode, update_only;
};

DEV_INLINE void kmeans_update(const KMeansArgs& a, int node, float* C,
                              int* assign, int& age)
{
    int tid = threadIdx.x;
    int c = a.counts[node];
    if (c == 0) return;
    const float* Xn = a.X + (long)node * a.Smax * a.dim;
    // assignment: thread = sample
    for (int s = tid; s < c; s += blockDim.x) {
        const float* x = Xn + (long)s * a.dim;
        float best = 1e30f;
        int bj = 0;
        for (int j = 0; j < a.k; ++j) {
            const float* cj = C + j * a.dim;
            float d2 = 0.f;
            for (int e = 0; e < a.dim; ++e) {
                float t = x[e] - cj[e];
                d2 += t * t;
            }
            if (d2 < best) { best = d2; bj = j; }
        }
        assign[s] = bj;
    }
    __syncthreads();
    // EMA, last-write-wins: thread = centroid, scan for its last sample
    for (int j = tid; j < a.k; j += blockDim.x) {
        int last = -1;
        for (int s = 0; s < c; ++s)
            if (assign[s] == j) last = s;
        if (last >= 0) {
            const float* x = Xn + (long)last * a.dim;
            float* cj = C + j * a.dim;
            for (int e = 0; e < a.dim; ++e)
                cj[e] = cj[e] * (1.0f - a.alpha) + a.alpha * x[e];
        }
    }
    __syncthreads();
    age += 1;
}

__global__ void __launch_bounds__(128)
tick_kmeans_kernel(KMeansArgs a)
{
    int i = blockIdx.x;
    int node = a.nodes[i];
    int tid = threadIdx.x;
    extern __shared__ float sm[];
    float* C = sm;                       // D = k*dim
    float* C2 = C + a.D;                 // received-model scratch
    int* assign = (int*)(C2 + a.D);      // Smax

    for (int e = tid; e < a.D; e += blockDim.x)
        C[e] = a.params[(long)node * a.D + e];
    __syncthreads();
    int age = a.ages[node];

    if (a.update_only) {
        kmeans_update(a, node, C, assign, age);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            const float* srow = a.slots + (long)slot * a.D;
            int sage = a.slot_ages[slot];
            if (a.mode == MODE_MERGE_UPDATE) {
                for (int e = tid; e < a.D; e += blockDim.x)
                    C[e] = 0.5f * (C[e] + srow[e]);
                __syncthreads();
                kmeans_update(a, node, C, assign, age);
            } else if (a.mode == MODE_UPDATE) {
                for (int e = tid; e < a.D; e += blockDim.x) C[e] = srow[e];
                age = sage;
                __syncthreads();
                kmeans_update(a, node, C, assign, age);
            } else if (a.mode == MODE_UPDATE_MERGE) {
                kmeans_update(a, node, C, assign, age);
                for (int e = tid; e < a.D; e += blockDim.x) C2[e] = srow[e];
                __syncthreads();
                int age2 = sage;
                kmeans_update(a, node, C2, assign, age2);
                for (int e = tid; e < a.D; e += blockDim.x)
                    C[e] = 0.5f * (C[e] + C2[e]);
                __syncthreads();
            } else {  // PASS
                for (int e = tid; e < a.D; e += blockDim.x) C[e] = srow[e];
                age = sage;
                __syncthreads();
            }
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)rs * a.D + e] = C[e];
                if (tid == 0) a.slot_ages[rs] = age;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < a.D; e += blockDim.x)
        a.params[(long)node * a.D + e] = C[e];
    if (tid == 0) a.ages[node] = age;
}

// ---------------------------------------------------------------------------
// pegasos / adaline tick: one WAVE per node, weights in registers
// ---------------------------------------------------------------------------

struct LinearArgs {
    float* params; int* ages;
    float* slots; int* slot_ages;
    const int* nodes; const int* ptr;
    const int* dslots; const int* rslots;
    const int* dmodes;
    const float* X; const float* Y; const int* counts;
    int d, Smax;
    float lrlam;       // pegasos lambda or adaline lr
    int is_pegasos, mode, update_only;
};

constexpr int LIN_MAX_REGS = 16;  // supports d up to 16*64 = 1024

// Per-sample sequential pass (the math is order-dependent: Pegasos' step
// size is 1/(t*lam) with t = running age). w lives in per-lane registers
// (lane L owns dims L, L+64, ...).
DEV_INLINE void linear_update(const LinearArgs& a, int node, float* w,
                              int nreg, int& age)
{
    int lane = threadIdx.x;
    int c = a.counts[node];
    const float* Xn = a.X + (long)node * a.Smax * a.d;
    const float* Yn = a.Y + (long)node * a.Smax;
    for (int s = 0; s < c; ++s) {
        const float* x = Xn + (long)s * a.d;
        float part = 0.f;
        float xr[LIN_MAX_REGS];
        for (int r = 0; r < nreg; ++r) {
            int e = lane + r * WAVE;
            xr[r] = (e < a.d) ? x[e] : 0.f;
            part += w[r] * xr[r];
        }
        float pred = wave_sum(part);
        float y = Yn[s];
        if (a.is_pegasos) {
            age += 1;
            float lr = 1.0f / (age * a.lrlam);
            float hinge = (pred * y - 1.0f < 0.f) ? 1.0f : 0.0f;
            float scale = 1.0f - lr * a.lrlam;
            float add = hinge * lr * y;
            for (int r = 0; r < nreg; ++r) w[r] = w[r] * scale + add * xr[r];
        } else {
            float err = y - pred;
            for (int r = 0; r < nreg; ++r) w[r] += a.lrlam * err * xr[r];
        }
    }
    if (!a.is_pegasos) age += c;  // AdaLine ages by sample count
}

DEV_INLINE void linear_process_node(const LinearArgs& a, int i)
{
    int node = a.nodes[i];
    int lane = threadIdx.x & (WAVE - 1);
    int nreg = (a.d + WAVE - 1) / WAVE;
    float w[LIN_MAX_REGS];
    for (int r = 0; r < nreg; ++r) {
        int e = lane + r * WAVE;
        w[r] = (e < a.d) ? a.params[(long)node * a.d + e] : 0.f;
    }
    int age = a.ages[node];

    if (a.update_only) {
        linear_update(a, node, w, nreg, age);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            const float* srow = a.slots + (long)slot * a.d;
            int sage = a.slot_ages[slot];
            int md = (a.dmodes && a.dmodes[j]) ? MODE_PASS : a.mode;
            if (md == MODE_MERGE_UPDATE) {
                for (int r = 0; r < nreg; ++r) {
                    int e = lane + r * WAVE;
                    if (e < a.d) w[r] = 0.5f * (w[r] + srow[e]);
                }
                age = max(age, sage);
                linear_update(a, node, w, nreg, age);
            } else if (md == MODE_UPDATE) {
                for (int r = 0; r < nreg; ++r) {
                    int e = lane + r * WAVE;
                    if (e < a.d) w[r] = srow[e];
                }
                age = sage;
                linear_update(a, node, w, nreg, age);
            } else if (md == MODE_UPDATE_MERGE) {
                linear_update(a, node, w, nreg, age);
                float w2[LIN_MAX_REGS];
                for (int r = 0; r < nreg; ++r) {
                    int e = lane + r * WAVE;
                    w2[r] = (e < a.d) ? srow[e] : 0.f;
                }
                int age2 = sage;
                linear_update(a, node, w2, nreg, age2);
                for (int r = 0; r < nreg; ++r) w[r] = 0.5f * (w[r] + w2[r]);
                age = max(age, age2);
            } else {  // PASS
                for (int r = 0; r < nreg; ++r) {
                    int e = lane + r * WAVE;
                    if (e < a.d) w[r] = srow[e];
                }
                age = sage;
            }
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int r = 0; r < nreg; ++r) {
                    int e = lane + r * WAVE;
                    if (e < a.d) a.slots[(long)rs * a.d + e] = w[r];
                }
                if (lane == 0) a.slot_ages[rs] = age;
            }
        }
    }
    for (int r = 0; r < nreg; ++r) {
        int e = lane + r * WAVE;
        if (e < a.d) a.params[(long)node * a.d + e] = w[r];
    }
    if (lane == 0) a.ages[node] = age;
}

__global__ void __launch_bounds__(WAVE)
tick_linear_kernel(LinearArgs a)
{
    linear_process_node(a, blockIdx.x);
}

// ---------------------------------------------------------------------------
// MLP tick: one workgroup per node, all activations in LDS
// ---------------------------------------------------------------------------

struct MlpArgs {
    float* params; int* ages;
    float* slots; int* slot_ages;
    const int* nodes; const int* ptr;
    const int* dslots; const int* rslots;
    const int* dmodes;
    const float* X; const float* Y; const int* counts;
    const int* layout;  // [n_layers][4] = (w_off, b_off, in, out)
    int n_layers, Smax, D, act_max, d_in;
    float lr, wd;
    int epochs, bs, mode, update_only;
    // tick_mlp_wide_kernel only: the device workspace and its per-block row
    // stride in floats (0 = no workspace, ws is then null)
    float* ws; long ws_row;
    int lim;  // limited-merge threshold L (LIM kernel only); last member
};

// Fused fwd+bwd+SGD over the node's shard. LDS holds the model row plus
// per-batch activations of every layer (act) and their gradients (grad).
//
// All three GEMMs (forward X·Wᵀ, input-grad G·W, weight-grad Gᵀ·X) run on
// the matrix cores via v_mfma_f32_16x16x4_f32 (exact f32 — bitwise an fmaf
// chain, so the torch oracle tolerance is unchanged). Fragment maps per
// the CDNA4 ISA: lane l supplies A[l&15][l>>4] and B[l>>4][l&15]; the
// accumulator lane l, register r holds D[(l>>4)*4 + r][l&15]. Ragged tile
// edges are zero-padded in registers (exact for f32). One 16x16 output
// tile per wave per iteration; the block's 4 waves stride the tile grid.

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// Dual-accumulator MFMA K-loop. For K <= MLP_KPAD the loop is PADDED to a
// compile-time bound and fully unrolled: every LDS load issues up front
// (independent) and the two MFMA chains run issue-bound instead of
// load-latency-bound. Out-of-range chunks contribute exact zeros, and the
// chunk->accumulator pairing (k0%8==0 -> acc, ==4 -> acc2) matches the
// dynamic loop, so the result is BIT-IDENTICAL either way. LoadA/LoadB
// take the chunk base k0 and must return 0 outside [0, Kdim).
constexpr int MLP_KPAD = 128;

template <int PAD, typename LoadA, typename LoadB>
DEV_INLINE f32x4_t mfma_kloop_padded(LoadA la, LoadB lb)
{
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    f32x4_t acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < PAD; k0 += 8) {
        float av = la(k0), bv = lb(k0);
        float av2 = la(k0 + 4), bv2 = lb(k0 + 4);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av2, bv2, acc2, 0, 0, 0);
    }
    for (int r = 0; r < 4; ++r) acc[r] += acc2[r];
    return acc;
}

template <typename LoadA, typename LoadB>
DEV_INLINE f32x4_t mfma_kloop(int Kdim, LoadA la, LoadB lb)
{
    if (Kdim <= 32) return mfma_kloop_padded<32>(la, lb);
    if (Kdim <= 64) return mfma_kloop_padded<64>(la, lb);
    if (Kdim <= MLP_KPAD) return mfma_kloop_padded<MLP_KPAD>(la, lb);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    f32x4_t acc2 = {0.f, 0.f, 0.f, 0.f};
    {
        int k0 = 0;
        for (; k0 + 8 <= Kdim; k0 += 8) {
            float av = la(k0), bv = lb(k0);
            float av2 = la(k0 + 4), bv2 = lb(k0 + 4);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(
                av2, bv2, acc2, 0, 0, 0);
        }
        for (; k0 < Kdim; k0 += 4) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                la(k0), lb(k0), acc, 0, 0, 0);
        }
    }
    for (int r = 0; r < 4; ++r) acc[r] += acc2[r];
    return acc;
}

// One layer of the forward pass on MFMA: nxt[m, out_l] = cur[m, in_l] · W_lᵀ
// + b_l, ReLU unless l is the head. A barrier follows.
DEV_INLINE void mlp_forward_layer(const MlpArgs& a, const float* W,
                                  const float* cur, float* nxt, int m, int l)
{
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int fr = lane & 15;       // A-row / B-col fragment index
    const int fk = lane >> 4;       // K fragment index (0..3)
    const int nwaves = blockDim.x >> 6;
    int w_off = a.layout[4 * l], b_off = a.layout[4 * l + 1];
    int fin = a.layout[4 * l + 2], fout = a.layout[4 * l + 3];
    int m16 = (m + 15) >> 4, o16 = (fout + 15) >> 4;
    for (int tile = wave; tile < m16 * o16; tile += nwaves) {
        int tr = (tile / o16) << 4, tc = (tile % o16) << 4;
        f32x4_t acc = mfma_kloop(
            fin,
            [&](int k0) {
                int q = k0 + fk;
                return (tr + fr < m && q < fin)
                           ? cur[(tr + fr) * fin + q] : 0.f;
            },
            [&](int k0) {
                int q = k0 + fk;
                return (tc + fr < fout && q < fin)
                           ? W[w_off + (tc + fr) * fin + q]
                           : 0.f;
            });
        for (int r = 0; r < 4; ++r) {
            int row = tr + (fk << 2) + r, col = tc + fr;
            if (row < m && col < fout) {
                float v = acc[r] + W[b_off + col];
                if (l < a.n_layers - 1) v = fmaxf(v, 0.f);  // ReLU
                nxt[row * fout + col] = v;
            }
        }
    }
    __syncthreads();
}

// Forward pass H = X · Wᵀ + b of every layer over the m rows staged at act
// (ReLU between layers, raw head), on MFMA. The activations are laid out
// layer after layer behind the input: act[l] is [m, out_l]. Returns the
// head's [m, k] activations. The caller's barrier must stand between the
// staging of the input (and of W) and this call; a barrier follows each
// layer.
// WIDE (tick_mlp_wide_kernel): the input is not staged, layer 0 reads the m
// rows at xin in the data arena and act holds the layers' outputs alone.
// Layer 0 is a call of its own so that each call sees one address space.
template <bool WIDE = false>
DEV_INLINE const float* mlp_forward(const MlpArgs& a, const float* W,
                                    float* act, int m,
                                    const float* xin = nullptr)
{
    const float* cur = act;
    float* nxt = act + m * a.d_in;
    int l = 0;
    if constexpr (WIDE) {
        mlp_forward_layer(a, W, xin, act, m, 0);
        nxt = act + m * a.layout[3];
        l = 1;
    }
    for (; l < a.n_layers; ++l) {
        mlp_forward_layer(a, W, cur, nxt, m, l);
        cur = nxt;
        nxt = nxt + m * a.layout[4 * l + 3];
    }
    return cur;
}

// PART = partitioned gossip (PartitionedTMH._local_step + _adjust_gradient,
// gossipy/model/handler.py:503-520): the age is the LDS vector agev[P],
// bumped whole before each minibatch step, and every parameter's gradient
// is divided by the age of its partition (apart: arena offset -> partition
// id) before weight decay. The plain instantiation ignores agev/apart/P and
// compiles to the scalar-age code unchanged.
// WIDE (tick_mlp_wide_kernel): W is a row in device memory, the minibatch
// is read in place from the data arena instead of being staged, act holds
// the layers' outputs alone and a.act_max is the widest of them. Every
// operand address, every K-loop and every epilogue expression is the one of
// the staged form, so the two return the same bits.
template <bool PART, bool WIDE = false>
DEV_INLINE void mlp_update(const MlpArgs& a, int node, float* W,
                           float* act, float* grad, int& age,
                           int* agev = nullptr, const int* apart = nullptr,
                           int P = 0)
{
    int tid = threadIdx.x;
    int c = a.counts[node];
    if (c == 0) return;
    int bsz = (a.bs == 0) ? c : min(a.bs, c);
    const float* Xn = a.X + (long)node * a.Smax * a.d_in;
    const float* Yn = a.Y + (long)node * a.Smax;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int fr = lane & 15;       // A-row / B-col fragment index
    const int fk = lane >> 4;       // K fragment index (0..3)
    const int nwaves = blockDim.x >> 6;
    for (int ep = 0; ep < a.epochs; ++ep) {
        for (int s0 = 0; s0 < c; s0 += bsz) {
            int m = min(bsz, c - s0);
            // activations laid out layer after layer: act[l] is [m, out_l];
            // act[-1] (the input) is staged first at act.
            const float* xin = Xn + (long)s0 * a.d_in;
            if constexpr (!WIDE) {
                float* in = act;
                for (int e = tid; e < m * a.d_in; e += blockDim.x)
                    in[e] = xin[e];
            }
            if constexpr (PART) {
                // self.n_updates += 1 happens before the step
                // (handler.py:506); first read is the dW epilogue, behind
                // the barriers below
                for (int p = tid; p < P; p += blockDim.x) agev[p] += 1;
            }
            __syncthreads();
            // ---- forward: H = X · Wᵀ + b on MFMA
            const float* cur = mlp_forward<WIDE>(a, W, act, m, xin);
            // ---- output grad: softmax-CE on the raw head
            int k = a.layout[4 * (a.n_layers - 1) + 3];
            float* gcur = grad;  // [m, k] for the head, reused per layer
            // (thread = sample, block-strided: a batch may have more rows
            // than the block has threads)
            for (int s = tid; s < m; s += blockDim.x) {
                const float* z = cur + s * k;
                float zmax = -1e30f;
                for (int kk = 0; kk < k; ++kk) zmax = fmaxf(zmax, z[kk]);
                float sum = 0.f;
                for (int kk = 0; kk < k; ++kk) sum += __expf(z[kk] - zmax);
                int yi = (int)Yn[s0 + s];
                float inv = 1.0f / sum;
                for (int kk = 0; kk < k; ++kk) {
                    float p = __expf(z[kk] - zmax) * inv;
                    gcur[s * k + kk] = (p - (kk == yi ? 1.0f : 0.0f)) / m;
                }
            }
            __syncthreads();
            // ---- backward + SGD, layer by layer (grad buffers ping-pong);
            //      both GEMMs (dX = G·W, dW = Gᵀ·X) on MFMA
            float* gnext = grad + m * a.act_max;
            for (int l = a.n_layers - 1; l >= 0; --l) {
                int w_off = a.layout[4 * l], b_off = a.layout[4 * l + 1];
                int fin = a.layout[4 * l + 2], fout = a.layout[4 * l + 3];
                // activation input of this layer
                const float* ain = act;
                for (int q = WIDE ? 1 : 0; q < l; ++q)
                    ain += m * a.layout[4 * q + 2];
                // (ain now points at act of layer l's input: layers are
                //  packed input-first, so offset = m*(d_in + hidden_0 + ...);
                //  WIDE: act starts at hidden_0, and layer 0 reads xin)
                // grad wrt input (needed before W is updated):
                // dX[m, fin] = G[m, fout] · W[fout, fin], ReLU-masked
                if (l > 0) {
                    int m16 = (m + 15) >> 4, q16 = (fin + 15) >> 4;
                    for (int tile = wave; tile < m16 * q16; tile += nwaves) {
                        int tr = (tile / q16) << 4, tc = (tile % q16) << 4;
                        f32x4_t acc = mfma_kloop(
                            fout,
                            [&](int k0) {
                                int o = k0 + fk;
                                return (tr + fr < m && o < fout)
                                           ? gcur[(tr + fr) * fout + o]
                                           : 0.f;
                            },
                            [&](int k0) {
                                int o = k0 + fk;
                                return (o < fout && tc + fr < fin)
                                           ? W[w_off + o * fin + tc + fr]
                                           : 0.f;
                            });
                        for (int r = 0; r < 4; ++r) {
                            int row = tr + (fk << 2) + r, col = tc + fr;
                            if (row < m && col < fin) {
                                float v = acc[r];
                                // ReLU mask of the layer-(l-1) activation
                                v *= (ain[row * fin + col] > 0.f) ? 1.0f : 0.0f;
                                gnext[row * fin + col] = v;
                            }
                        }
                    }
                    __syncthreads();
                }
                // weight SGD: dW[fout, fin] = Gᵀ[fout, m] · X[m, fin], X the
                // layer's input at bin
                auto dw_stage = [&](const float* bin)
                                    __attribute__((always_inline)) {
                    int o16 = (fout + 15) >> 4, q16 = (fin + 15) >> 4;
                    for (int tile = wave; tile < o16 * q16; tile += nwaves) {
                        int tr = (tile / q16) << 4, tc = (tile % q16) << 4;
                        // partition ids of this lane's four outputs: the
                        // L2 loads issue ahead of the MFMA chain, which
                        // hides their latency from the epilogue
                        int pe[4];
                        if constexpr (PART) {
                            for (int r = 0; r < 4; ++r) {
                                int row = tr + (fk << 2) + r, col = tc + fr;
                                pe[r] = (row < fout && col < fin)
                                            ? apart[w_off + row * fin + col]
                                            : 0;
                            }
                        }
                        f32x4_t acc = mfma_kloop(
                            m,
                            [&](int k0) {
                                int sidx = k0 + fk;
                                return (tr + fr < fout && sidx < m)
                                           ? gcur[sidx * fout + tr + fr]
                                           : 0.f;
                            },
                            [&](int k0) {
                                int sidx = k0 + fk;
                                return (sidx < m && tc + fr < fin)
                                           ? bin[sidx * fin + tc + fr]
                                           : 0.f;
                            });
                        for (int r = 0; r < 4; ++r) {
                            int row = tr + (fk << 2) + r, col = tc + fr;
                            if (row < fout && col < fin) {
                                float g = acc[r];
                                int e = row * fin + col;
                                if constexpr (PART)  // _adjust_gradient
                                    g /= (float)agev[pe[r]];
                                if (a.wd != 0.f) g += a.wd * W[w_off + e];
                                W[w_off + e] -= a.lr * g;
                            }
                        }
                    }
                };
                // (WIDE: one call per address space, arena rows or LDS)
                if (WIDE && l == 0) dw_stage(xin);
                else dw_stage(ain);
                for (int e = tid; e < fout; e += blockDim.x) {
                    float g = 0.f;
                    for (int s = 0; s < m; ++s) g += gcur[s * fout + e];
                    if constexpr (PART) {
                        // the rescaled flat gradient is decayed as a whole
                        // (biases included), unlike the plain step
                        g /= (float)agev[apart[b_off + e]];
                        if (a.wd != 0.f) g += a.wd * W[b_off + e];
                    }
                    W[b_off + e] -= a.lr * g;
                }
                __syncthreads();
                float* tmp = gcur; gcur = gnext; gnext = tmp;
            }
            if constexpr (!PART) age += 1;
        }
    }
}

// LIM = limited merge (lim_rule) in place of the mean merge
template <bool LIM>
__global__ void __launch_bounds__(512)
tick_mlp_kernel(MlpArgs a)
{
    int i = blockIdx.x;
    int node = a.nodes[i];
    int tid = threadIdx.x;
    extern __shared__ float sm[];
    float* W = sm;          // D
    // W2 (the second model slab) exists only for UPDATE_MERGE — dropping
    // it elsewhere takes the flagship MLP block from 94 KB to 70 KB of
    // LDS, which fits TWO workgroups per CU (4 waves/SIMD instead of 2)
    bool has_w2 = (a.mode == MODE_UPDATE_MERGE);
    float* W2 = has_w2 ? W + a.D : nullptr;
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    // act: batch input + every layer's activation; grad: 2 ping-pong buffers
    float* act = W + (has_w2 ? 2 : 1) * (size_t)a.D;
    int act_total = 0;
    // act layout computed on host side == bs*(d_in + sum(out_l)); the host
    // passes act_max = max layer width for the grad buffers
    for (int l = 0; l < a.n_layers; ++l) act_total += a.layout[4 * l + 3];
    float* grad = act + bsmax * (a.d_in + act_total);

    for (int e = tid; e < a.D; e += blockDim.x)
        W[e] = a.params[(long)node * a.D + e];
    __syncthreads();
    int age = a.ages[node];

    if (a.update_only) {
        mlp_update<false>(a, node, W, act, grad, age);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            const float* srow = a.slots + (long)slot * a.D;
            int sage = a.slot_ages[slot];
            int md = (a.dmodes && a.dmodes[j]) ? MODE_PASS : a.mode;
            if (md == MODE_MERGE_UPDATE) {
                if constexpr (LIM) {
                    lim_merge_row(lim_rule(age, sage, a.lim), W, srow, a.D);
                } else {
                    for (int e = tid; e < a.D; e += blockDim.x)
                        W[e] = 0.5f * (W[e] + srow[e]);
                }
                age = max(age, sage);
                __syncthreads();
                mlp_update<false>(a, node, W, act, grad, age);
            } else if (md == MODE_UPDATE) {
                for (int e = tid; e < a.D; e += blockDim.x) W[e] = srow[e];
                age = sage;
                __syncthreads();
                mlp_update<false>(a, node, W, act, grad, age);
            } else if (md == MODE_UPDATE_MERGE) {
                mlp_update<false>(a, node, W, act, grad, age);
                for (int e = tid; e < a.D; e += blockDim.x) W2[e] = srow[e];
                __syncthreads();
                int age2 = sage;
                mlp_update<false>(a, node, W2, act, grad, age2);
                if constexpr (LIM) {
                    lim_merge_row(lim_rule(age, age2, a.lim), W, W2, a.D);
                } else {
                    for (int e = tid; e < a.D; e += blockDim.x)
                        W[e] = 0.5f * (W[e] + W2[e]);
                }
                age = max(age, age2);
                __syncthreads();
            } else {
                for (int e = tid; e < a.D; e += blockDim.x) W[e] = srow[e];
                age = sage;
                __syncthreads();
            }
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)rs * a.D + e] = W[e];
                if (tid == 0) a.slot_ages[rs] = age;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < a.D; e += blockDim.x)
        a.params[(long)node * a.D + e] = W[e];
    if (tid == 0) a.ages[node] = age;
}

// tick_mlp_kernel for models past the LDS budget: no LDS term scales with D
// or with batch_rows * d_in. Block per receiver, the same delivery semantics
// line by line, but
//   W   is params[node] itself, worked on in place: receivers are unique
//       within a launch, so only this block touches the row;
//   W2  (UPDATE_MERGE's trained copy of the received model) is the head of
//       this block's row of the device workspace a.ws;
//   X   is read from the data arena by the GEMM stages, never staged;
//   act / grad hold the layers' outputs and two gradient buffers of the
//       widest output: in LDS, or (ACT_WS) behind W2 in the workspace row
//       when a batch's worth of them misses the LDS budget.
// mlp_update<false, true> runs the staged form's arithmetic on these
// operands, so on a shape both kernels take the results are bit-equal. A
// __syncthreads() orders one stage's global stores before the next stage's
// loads: the waves of a workgroup share one CU and its write-through L1.
template <bool LIM, bool ACT_WS>
__global__ void __launch_bounds__(512)
tick_mlp_wide_kernel(MlpArgs a)
{
    int i = blockIdx.x;
    int node = a.nodes[i];
    int tid = threadIdx.x;
    extern __shared__ float sm[];
    float* W = a.params + (long)node * a.D;
    float* wsrow = a.ws + (long)i * a.ws_row;
    bool has_w2 = (a.mode == MODE_UPDATE_MERGE);
    float* W2 = has_w2 ? wsrow : nullptr;
    float* act;
    if constexpr (ACT_WS) act = wsrow + (has_w2 ? a.D : 0);
    else act = sm;
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    int act_total = 0;
    for (int l = 0; l < a.n_layers; ++l) act_total += a.layout[4 * l + 3];
    float* grad = act + (long)bsmax * act_total;
    int age = a.ages[node];

    if (a.update_only) {
        mlp_update<false, true>(a, node, W, act, grad, age);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            const float* srow = a.slots + (long)slot * a.D;
            int sage = a.slot_ages[slot];
            int md = (a.dmodes && a.dmodes[j]) ? MODE_PASS : a.mode;
            if (md == MODE_MERGE_UPDATE) {
                if constexpr (LIM) {
                    lim_merge_row(lim_rule(age, sage, a.lim), W, srow, a.D);
                } else {
                    for (int e = tid; e < a.D; e += blockDim.x)
                        W[e] = 0.5f * (W[e] + srow[e]);
                }
                age = max(age, sage);
                __syncthreads();
                mlp_update<false, true>(a, node, W, act, grad, age);
            } else if (md == MODE_UPDATE) {
                for (int e = tid; e < a.D; e += blockDim.x) W[e] = srow[e];
                age = sage;
                __syncthreads();
                mlp_update<false, true>(a, node, W, act, grad, age);
            } else if (md == MODE_UPDATE_MERGE) {
                mlp_update<false, true>(a, node, W, act, grad, age);
                for (int e = tid; e < a.D; e += blockDim.x) W2[e] = srow[e];
                __syncthreads();
                int age2 = sage;
                mlp_update<false, true>(a, node, W2, act, grad, age2);
                if constexpr (LIM) {
                    lim_merge_row(lim_rule(age, age2, a.lim), W, W2, a.D);
                } else {
                    for (int e = tid; e < a.D; e += blockDim.x)
                        W[e] = 0.5f * (W[e] + W2[e]);
                }
                age = max(age, age2);
                __syncthreads();
            } else {
                for (int e = tid; e < a.D; e += blockDim.x) W[e] = srow[e];
                age = sage;
                __syncthreads();
            }
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)rs * a.D + e] = W[e];
                if (tid == 0) a.slot_ages[rs] = age;
                __syncthreads();
            }
        }
    }
    if (tid == 0) a.ages[node] = age;
}

// ---------------------------------------------------------------------------
// compressed MLP ticks: partitioned (PartitionedTMH) and sampled
// (SamplingTMH) delivery on the tick_mlp_kernel structure — block per
// receiver, model row LDS-resident, SGD through mlp_update's MFMA stages.
//
// Parity: delivery semantics are those of logreg_part_process_node and
// tick_logreg_samp_kernel above (gossipy/model/handler.py:426-525). PASS is
// rejected host-side for both.
// ---------------------------------------------------------------------------

struct MlpCompArgs {
    MlpArgs m;         // dmodes unused
    const int* dpids;  // per delivery: partition id (PART) / sample seed
    const int* perm;   // [D]   partition-ordered -> arena offset   (PART)
    const int* pptr;   // [P+1]                                     (PART)
    const int* apart;  // [D]   arena offset -> partition id        (PART)
    int P;             // partitions; ages / slot_ages are [*, P]   (PART)
    int samp_c;        // coordinates per sampled merge
    //: sampled: the pre-merge copy lives in the act/grad scratch (idle
    //: between SGD steps) instead of a slab of its own — decided host-side
    int w3_alias;
};

// Age-weighted merge of partition `pid` of src into W (handler.py:497-501;
// weights (0,0) -> (1/2,1/2)); that partition's age becomes the max. src /
// src_ages may point to LDS (trained received model) or HBM (slot row).
DEV_INLINE void mlp_part_merge(const MlpCompArgs& c, float* W, int* agev,
                               const float* src, const int* src_ages, int pid)
{
    int tid = threadIdx.x;
    int w1 = agev[pid], w2 = src_ages[pid];
    float m1, m2;
    if (w1 == 0 && w2 == 0) { m1 = 0.5f; m2 = 0.5f; }
    else {
        float s = (float)(w1 + w2);
        m1 = (float)w1 / s;
        m2 = (float)w2 / s;
    }
    __syncthreads();
    for (int e = c.pptr[pid] + tid; e < c.pptr[pid + 1]; e += blockDim.x) {
        int i = c.perm[e];
        W[i] = m1 * W[i] + m2 * src[i];
    }
    if (tid == 0) agev[pid] = max(w1, w2);
    __syncthreads();
}

// Sampled mean merge: W[i] = (W[i] + src[i]) / 2 over the index stream
// splitmix64(seed + q) % D, q < samp_c (engine/rng.py sample_indices). W3
// holds the pre-merge W so duplicate indices all read the ORIGINAL value
// (torch advanced-index assignment semantics); duplicates then store the
// same value, so their order does not matter.
DEV_INLINE void mlp_samp_merge(const MlpCompArgs& c, float* W, float* W3,
                               const float* src, int seed)
{
    int tid = threadIdx.x;
    int D = c.m.D;
    for (int e = tid; e < D; e += blockDim.x) W3[e] = W[e];
    __syncthreads();
    for (int q = tid; q < c.samp_c; q += blockDim.x) {
        int i = (int)(splitmix64_dev((unsigned long long)seed +
                                     (unsigned long long)q) %
                      (unsigned long long)D);
        W[i] = 0.5f * (W3[i] + src[i]);
    }
    __syncthreads();
}

template <bool PART>
__global__ void __launch_bounds__(512)
tick_mlp_comp_kernel(MlpCompArgs c)
{
    const MlpArgs& a = c.m;
    int i = blockIdx.x;
    int node = a.nodes[i];
    int tid = threadIdx.x;
    extern __shared__ float sm[];
    // LDS (host computes the same sum): W | W2 unless MERGE_UPDATE | W3 when
    // sampled and not aliased | act | 2 grad buffers | agev, agev2 (PART)
    float* W = sm;
    bool has_w2 = (a.mode != MODE_MERGE_UPDATE);
    float* W2 = has_w2 ? W + a.D : nullptr;
    float* next = W + (has_w2 ? 2 : 1) * (size_t)a.D;
    float* W3 = nullptr;
    if (!PART && !c.w3_alias) { W3 = next; next += a.D; }
    float* act = next;
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    int act_total = 0;
    for (int l = 0; l < a.n_layers; ++l) act_total += a.layout[4 * l + 3];
    float* grad = act + bsmax * (a.d_in + act_total);
    if (!PART && c.w3_alias) W3 = act;
    int* agev = (int*)(grad + 2 * bsmax * a.act_max);  // P     (PART)
    int* agev2 = agev + c.P;                            // P     (PART)
    const int P = PART ? c.P : 0;

    for (int e = tid; e < a.D; e += blockDim.x)
        W[e] = a.params[(long)node * a.D + e];
    for (int p = tid; p < P; p += blockDim.x)
        agev[p] = a.ages[(long)node * P + p];
    __syncthreads();
    int age = PART ? 0 : a.ages[node];

    if (a.update_only) {
        mlp_update<PART>(a, node, W, act, grad, age, agev, c.apart, P);
    } else {
        for (int j = a.ptr[i]; j < a.ptr[i + 1]; ++j) {
            int slot = a.dslots[j];
            int pid = c.dpids ? c.dpids[j] : 0;  // partition id / seed
            const float* srow = a.slots + (long)slot * a.D;
            if (a.mode == MODE_MERGE_UPDATE) {
                if constexpr (PART)
                    mlp_part_merge(c, W, agev, srow,
                                   a.slot_ages + (long)slot * P, pid);
                else
                    mlp_samp_merge(c, W, W3, srow, pid);
                mlp_update<PART>(a, node, W, act, grad, age, agev, c.apart, P);
            } else {
                // UPDATE: train the received model, merge its partition /
                // sample into self (handler.py:440-442, 481-483).
                // UPDATE_MERGE: self-update first (handler.py:445-448,
                // 487-490).
                if (a.mode == MODE_UPDATE_MERGE)
                    mlp_update<PART>(a, node, W, act, grad, age, agev,
                                     c.apart, P);
                for (int e = tid; e < a.D; e += blockDim.x) W2[e] = srow[e];
                for (int p = tid; p < P; p += blockDim.x)
                    agev2[p] = a.slot_ages[(long)slot * P + p];
                __syncthreads();
                // sampled: the received model's scalar age is trained and
                // dropped — ages are never merged (handler.py:431-433)
                int age2 = 0;
                mlp_update<PART>(a, node, W2, act, grad, age2, agev2,
                                 c.apart, P);
                if constexpr (PART)
                    mlp_part_merge(c, W, agev, W2, agev2, pid);
                else
                    mlp_samp_merge(c, W, W3, W2, pid);
            }
            int rs = a.rslots ? a.rslots[j] : -1;
            if (rs >= 0) {
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)rs * a.D + e] = W[e];
                if constexpr (PART) {
                    for (int p = tid; p < P; p += blockDim.x)
                        a.slot_ages[(long)rs * P + p] = agev[p];
                } else {
                    if (tid == 0) a.slot_ages[rs] = age;
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < a.D; e += blockDim.x)
        a.params[(long)node * a.D + e] = W[e];
    if constexpr (PART) {
        for (int p = tid; p < P; p += blockDim.x)
            a.ages[(long)node * P + p] = agev[p];
    } else {
        if (tid == 0) a.ages[node] = age;
    }
}

// ---------------------------------------------------------------------------
// fused evaluation metrics (K13): accuracy / macro precision / recall / F1
// (+ pairwise ROC-AUC for binary) of R node models on one shared eval set,
// in a single launch. Replaces the reference's per-node sklearn calls
// (gossipy/model/handler.py:282-334, 375-391) and the engine's previous
// ~15-small-torch-ops path. argmax/AUC are computed on raw affine scores —
// the sigmoid is monotonic, so predictions and ranks are unchanged.
// ---------------------------------------------------------------------------

struct EvalArgs {
    const float* params;  // [n_local, D]
    const int* nodes;     // [R] local row ids
    const float* X;       // [n_eval, d]
    const float* Y;       // [n_eval] class index (or +-1 when is_margin)
    float* out;           // [R, 5] acc, prec, rec, f1, auc
    int d, k, n_eval, D;
    int is_margin;        // pegasos/adaline: score = <w, x>, label +-1
    int tile;             // samples staged per LDS tile (coalesced loads)
    // per-node shard mode (local test sets): X/Y are [n_local, n_eval(,d)]
    // arenas, eval_counts[node] gives the node's row count
    const int* eval_counts;
    // precomputed-scores mode (MLP/torchmod: any family whose forward ran
    // elsewhere): [R, n_eval, k] raw scores; skips the scoring GEMM stage
    const float* scores;
};

constexpr int EVAL_KMAX = 16;

// Metrics epilogue shared by eval_metrics_kernel and eval_mlp_kernel: from
// the block's staged positive-class scores s1[n_e], binarized labels
// yb[n_e] and kk x kk confusion counts conf, write the 5-float result row
// (accuracy, macro precision / recall / F1, AUC; AUC -1 for kk > 2). cs is
// n_e floats of scratch. The caller's barrier stands between the staging
// and this call.
DEV_INLINE void eval_epilogue(float* out_row, int n_e, int kk,
                              const float* s1, float* cs, const char* yb,
                              const int* conf)
{
    int tid = threadIdx.x;
    // pairwise AUC (binary only): wins over (pos, neg) pairs, ties 0.5 —
    // the Mann-Whitney statistic (== average-rank AUC). Every partial sum
    // is a multiple of 0.5 below 2^24, so the fp32 total does not depend
    // on the summation order.
    __shared__ float auc_wins;
    __shared__ int npos_s, nneg_s;
    if (tid == 0) { auc_wins = 0.f; npos_s = 0; nneg_s = 0; }
    __syncthreads();
    if (kk == 2) {
        // compact the scores by label: positives fill cs from the front,
        // negatives from the back (one LDS atomic per wave and label)
        int lane = tid & (WAVE - 1);
        unsigned long long below = (1ull << lane) - 1ull;
        for (int i0 = 0; i0 < n_e; i0 += blockDim.x) {
            int i = i0 + tid;
            bool in = i < n_e;
            bool ps = in && yb[in ? i : 0];
            bool ng = in && !ps;
            float sc = s1[in ? i : 0];
            unsigned long long mp = __ballot(ps), mn = __ballot(ng);
            int bp = 0, bn = 0;
            if (lane == 0) {
                bp = atomicAdd(&npos_s, __popcll(mp));
                bn = atomicAdd(&nneg_s, __popcll(mn));
            }
            bp = __shfl(bp, 0, WAVE);
            bn = __shfl(bn, 0, WAVE);
            if (ps) cs[bp + __popcll(mp & below)] = sc;
            if (ng) cs[n_e - 1 - (bn + __popcll(mn & below))] = sc;
        }
        __syncthreads();
        int npos = npos_s, nneg = n_e - npos;
        int total = npos * nneg;  // <= 2^20 for n_e <= 2048
        const float* pos = cs;
        const float* neg = cs + npos;
        float wins = 0.f;
        if (total > 0) {
            // pair q = i*nneg + j; a thread walks q = tid, tid + B, ... and
            // keeps (i, j) by adding (B / nneg, B % nneg) with one carry
            int B = blockDim.x;
            int di = B / nneg, dj = B - di * nneg;
            int i = tid / nneg, j = tid - i * nneg;
            for (int q0 = tid; q0 < total; q0 += CH * B) {
                float pv[CH], nv[CH];
                bool ok[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    ok[u] = q0 + u * B < total;
                    pv[u] = pos[min(i, npos - 1)];
                    nv[u] = neg[j];
                    i += di; j += dj;
                    if (j >= nneg) { j -= nneg; i += 1; }
                }
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    float w = pv[u] > nv[u] ? 1.f
                                            : (pv[u] == nv[u] ? 0.5f : 0.f);
                    wins += ok[u] ? w : 0.f;
                }
            }
        }
        // block reduce via wave shuffles: 256 serialized LDS atomics were
        // ~1/3 of this kernel's time
        wins = wave_sum(wins);
        if (lane == 0) atomicAdd(&auc_wins, wins);
    }
    __syncthreads();

    if (tid == 0) {
        int n = n_e;
        int correct = 0;
        float prec = 0.f, rec = 0.f, f1 = 0.f;
        for (int c = 0; c < kk; ++c) {
            int tp = conf[c * kk + c];
            correct += tp;
            int pred_tot = 0, true_tot = 0;
            for (int t2 = 0; t2 < kk; ++t2) {
                pred_tot += conf[t2 * kk + c];
                true_tot += conf[c * kk + t2];
            }
            float p = pred_tot > 0 ? (float)tp / pred_tot : 0.f;
            float q = true_tot > 0 ? (float)tp / true_tot : 0.f;
            prec += p;
            rec += q;
            f1 += (p + q) > 0.f ? 2.f * p * q / (p + q) : 0.f;
        }
        float* o = out_row;
        o[0] = (float)correct / n;
        o[1] = prec / kk;
        o[2] = rec / kk;
        o[3] = f1 / kk;
        if (kk == 2) {
            int npos = npos_s, nneg = n - npos_s;
            o[4] = (npos == 0 || nneg == 0)
                       ? 0.5f
                       : auc_wins / ((float)npos * nneg);
        } else {
            o[4] = -1.f;  // AUC undefined for k > 2 (reference parity)
        }
    }
}

__global__ void __launch_bounds__(256)
eval_metrics_kernel(EvalArgs a)
{
    int r = blockIdx.x;
    int node = a.nodes ? a.nodes[r] : r;
    int tid = threadIdx.x;
    int n_e = a.n_eval;
    const float* Xb = a.X;
    const float* Yb = a.Y;
    if (a.eval_counts) {  // per-node shard mode: a.n_eval is the row stride
        Xb = a.X + (long)node * a.n_eval * a.d;
        Yb = a.Y + (long)node * a.n_eval;
        n_e = min(a.eval_counts[node], a.n_eval);
        if (n_e == 0) {
            if (tid == 0)
                for (int e = 0; e < 5; ++e) a.out[(long)r * 5 + e] = -2.f;
            return;
        }
    }
    extern __shared__ float sm[];
    float* W = sm;                       // D
    float* s1 = W + a.D;                 // n_eval: positive-class score
    float* cs = s1 + n_e;                // n_eval: s1 compacted by label
    char* yb = (char*)(cs + n_e);   // n_eval: binarized label
    int* conf = (int*)(yb + ((n_e + 15) & ~15));  // k*k confusion
    float* XT = (float*)(conf + EVAL_KMAX * EVAL_KMAX);  // tile x d
    int kk = a.is_margin ? 2 : a.k;

    copy_row(W, a.params + (long)node * a.D, a.D);
    for (int e = tid; e < kk * kk; e += blockDim.x) conf[e] = 0;
    __syncthreads();

    if (a.scores) {
        // precomputed scores: just argmax + confusion + score staging
        const float* zs = a.scores + (long)r * n_e * (a.is_margin ? 1 : a.k);
        for (int sidx = tid; sidx < n_e; sidx += blockDim.x) {
            int pred, yt;
            float sc1;
            if (a.is_margin) {
                sc1 = zs[sidx];
                pred = sc1 >= 0.f ? 1 : 0;
                yt = Yb[sidx] > 0.f ? 1 : 0;
            } else {
                const float* z = zs + (long)sidx * a.k;
                float best = -1e30f;
                int bj = 0;
                for (int j = 0; j < a.k; ++j)
                    if (z[j] > best) { best = z[j]; bj = j; }
                sc1 = a.k > 1 ? z[1] : z[0];
                pred = bj;
                yt = (int)Yb[sidx];
            }
            s1[sidx] = sc1;
            yb[sidx] = (char)(a.is_margin ? (Yb[sidx] > 0.f ? 1 : 0)
                                          : ((int)Yb[sidx] == 1 ? 1 : 0));
            atomicAdd(&conf[yt * kk + pred], 1);
        }
        __syncthreads();
    } else
    // samples staged through LDS in coalesced tiles (the old thread-per-
    // sample global gather was a stride-d access pattern and dominated
    // the kernel's 44 us)
    for (int s0 = 0; s0 < n_e; s0 += a.tile) {
        int m = min(a.tile, n_e - s0);
        copy_row<16>(XT, Xb + (long)s0 * a.d, m * a.d);
        __syncthreads();
        for (int sidx = s0 + tid; sidx < s0 + m; sidx += blockDim.x) {
            const float* x = XT + (long)(sidx - s0) * a.d;
            float yv = Yb[sidx];  // in flight under the scoring
            int pred, yt;
            float sc1;
            if (a.is_margin) {
                float acc = dot_chain(0.f, W, x, a.d);
                sc1 = acc;
                pred = acc >= 0.f ? 1 : 0;
                yt = yv > 0.f ? 1 : 0;
            } else {
                float best = -1e30f;
                int bj = 0;
                float z1 = 0.f;
                for (int j = 0; j < a.k; ++j) {
                    float acc = dot_chain(W[a.k * a.d + j],  // bias
                                          W + j * a.d, x, a.d);
                    if (acc > best) { best = acc; bj = j; }
                    if (j == 1) z1 = acc;
                }
                sc1 = z1;
                pred = bj;
                yt = (int)yv;
            }
            s1[sidx] = sc1;
            yb[sidx] = (char)(a.is_margin ? (yv > 0.f ? 1 : 0)
                                          : ((int)yv == 1 ? 1 : 0));
            atomicAdd(&conf[yt * kk + pred], 1);
        }
        __syncthreads();
    }

    eval_epilogue(a.out + (long)r * 5, n_e, kk, s1, cs, yb, conf);
}

// K13 for the MLP family: block r runs node nodes[r]'s forward on MFMA
// (mlp_forward, the chain tick_pens_mlp_kernel scores candidates with) over
// its evaluation rows, in chunks of `tile` rows staged in LDS, and ends in
// the same metrics epilogue. Two addressing modes, as EvalArgs: per-node
// shards (eval_counts set: X/Y are [n_local, n_eval(, d_in)] arenas indexed
// by the LOCAL ROW ID nodes[r], eval_counts[node] rows of them live) or one
// shared set (X is [n_eval, d_in]). Of MlpArgs only params, nodes, X, Y,
// layout, n_layers, D and d_in are read.
struct EvalMlpArgs {
    MlpArgs m;
    float* out;              // [R, 5] acc, prec, rec, f1, auc
    const int* eval_counts;  // [n_local], or null: shared set
    int n_eval;              // rows of the shared set / row stride of a shard
    int tile;                // rows forwarded per chunk (eval_mlp_tile)
};

__global__ void __launch_bounds__(256)
eval_mlp_kernel(EvalMlpArgs p)
{
    const MlpArgs& a = p.m;
    int r = blockIdx.x;
    int node = a.nodes[r];
    int tid = threadIdx.x;
    int n_e = p.n_eval;
    const float* Xb = a.X;
    const float* Yb = a.Y;
    if (p.eval_counts) {
        Xb = a.X + (long)node * p.n_eval * a.d_in;
        Yb = a.Y + (long)node * p.n_eval;
        n_e = min(p.eval_counts[node], p.n_eval);
        if (n_e <= 0) {
            if (tid == 0)
                for (int e = 0; e < 5; ++e) p.out[(long)r * 5 + e] = -2.f;
            return;
        }
    }
    extern __shared__ float sm[];
    float* W = sm;                       // D
    float* s1 = W + a.D;                 // n_e: positive-class score
    float* cs = s1 + n_e;                // n_e: s1 compacted by label
    char* yb = (char*)(cs + n_e);        // n_e: binarized label
    int* conf = (int*)(yb + ((n_e + 15) & ~15));  // k*k confusion
    // forward scratch: tile x (d_in + act_total)
    float* act = (float*)(conf + EVAL_KMAX * EVAL_KMAX);
    int k = a.layout[4 * (a.n_layers - 1) + 3];

    copy_row(W, a.params + (long)node * a.D, a.D);
    for (int e = tid; e < k * k; e += blockDim.x) conf[e] = 0;

    for (int s0 = 0; s0 < n_e; s0 += p.tile) {
        int m = min(p.tile, n_e - s0);
        copy_row<16>(act, Xb + (long)s0 * a.d_in, m * a.d_in);
        __syncthreads();
        const float* head = mlp_forward(a, W, act, m);
        // (thread = sample, block-strided); ascending scan, strict > — the
        // first maximum wins, as torch.argmax
        for (int s = tid; s < m; s += blockDim.x) {
            const float* z = head + s * k;
            float yv = Yb[s0 + s];
            float best = z[0];
            int bj = 0;
            for (int j = 1; j < k; ++j) {
                if (z[j] > best) { best = z[j]; bj = j; }
            }
            int yt = (int)yv;
            s1[s0 + s] = k > 1 ? z[1] : z[0];
            yb[s0 + s] = (char)(yt == 1 ? 1 : 0);
            // a label outside [0, k) has no confusion row
            if ((unsigned)yt < (unsigned)k) atomicAdd(&conf[yt * k + bj], 1);
        }
        // the head is read out before the next chunk overwrites act
        __syncthreads();
    }

    eval_epilogue(p.out + (long)r * 5, n_e, k, s1, cs, yb, conf);
}

// ---------------------------------------------------------------------------
// PENS step-1 event kernel (Onoszko 2021; gossipy/node.py:767-782): one
// workgroup per event — score all cached candidate models on the
// receiver's train shard (argmax accuracy; the sigmoid is monotonic so
// raw affine scores give the reference's predictions), select the top-m
// (stable in arrival order), merge them as a (m+1)-way mean with the own
// model, run the local update, and count the winning senders.
// ---------------------------------------------------------------------------

constexpr int PENS_MAX_CAND = 64;

struct PensArgs {
    float* params; int* ages;
    const float* slots; const int* slot_ages;
    const int* nodes;       // [E] event receivers (unique within a launch)
    const int* ptr;         // [E+1] candidate ranges
    const int* cslots;      // candidate slots
    const int* cowners;     // candidate senders (global node ids)
    int* counts;            // [n_local, n_total] winner counters
    const float* X; const float* Y; const int* dcounts;
    int d, k, Smax, D, m_top, n_total;
    float lr, wd;
    int epochs, bs;
};

// Top-min(m_top, n_cand) candidates by correct count, stable in arrival
// order (the first of equal counts wins): marks them in sel[] and bumps the
// receiver's winner counter of each one's sender. One thread runs it.
DEV_INLINE void pens_select(const int* correct, int* sel, int n_cand,
                            int m_top, int* counts_row, const int* owners)
{
    for (int c = 0; c < n_cand; ++c) sel[c] = 0;
    int m = min(m_top, n_cand);
    for (int pick = 0; pick < m; ++pick) {
        int best_c = -1, best_v = -1;
        for (int c = 0; c < n_cand; ++c) {
            if (!sel[c] && correct[c] > best_v) {
                best_v = correct[c];
                best_c = c;
            }
        }
        sel[best_c] = 1;
        atomicAdd(&counts_row[owners[best_c]], 1);
    }
}

template <bool BIG>  // as logreg_update's
__global__ void __launch_bounds__(128)
tick_pens_kernel(PensArgs a)
{
    int i = blockIdx.x;
    int node = a.nodes[i];
    int tid = threadIdx.x;
    int lo = a.ptr[i], hi = a.ptr[i + 1];
    int n_cand = hi - lo;
    extern __shared__ float sm[];
    float* W = sm;                      // D
    float* xb = W + a.D;                // bsmax*d (update scratch)
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    float* dz = xb + bsmax * a.d;       // bsmax*k
    __shared__ int correct[PENS_MAX_CAND];
    __shared__ int sel[PENS_MAX_CAND];

    int c_n = a.dcounts[node];
    const float* Xn = a.X + (long)node * a.Smax * a.d;
    const float* Yn = a.Y + (long)node * a.Smax;

    // --- score candidates: thread = sample, loop candidates
    for (int c = tid; c < n_cand; c += blockDim.x) correct[c] = 0;
    __syncthreads();
    for (int c = 0; c < n_cand; ++c) {
        const float* Wc = a.slots + (long)a.cslots[lo + c] * a.D;
        int my = 0;
        for (int s = tid; s < c_n; s += blockDim.x) {
            const float* x = Xn + (long)s * a.d;
            float best = -1e30f;
            int bj = 0;
            for (int j = 0; j < a.k; ++j) {
                float acc = Wc[a.k * a.d + j];
                const float* wrow = Wc + j * a.d;
                for (int e = 0; e < a.d; ++e) acc += wrow[e] * x[e];
                if (acc > best) { best = acc; bj = j; }
            }
            if (bj == (int)Yn[s]) my += 1;
        }
        if (my) atomicAdd(&correct[c], my);
    }
    __syncthreads();

    // --- stable top-m selection (thread 0; n_cand small)
    if (tid == 0)
        pens_select(correct, sel, n_cand, a.m_top,
                    a.counts + (long)node * a.n_total, a.cowners + lo);
    __syncthreads();

    // --- merge: (own + sum selected) / (m+1), age = max
    for (int e = tid; e < a.D; e += blockDim.x)
        W[e] = a.params[(long)node * a.D + e];
    __syncthreads();
    int n_sel = 0;
    int age = a.ages[node];
    for (int c = 0; c < n_cand; ++c) {
        if (!sel[c]) continue;
        n_sel += 1;
        const float* Wc = a.slots + (long)a.cslots[lo + c] * a.D;
        for (int e = tid; e < a.D; e += blockDim.x) W[e] += Wc[e];
        age = max(age, a.slot_ages[a.cslots[lo + c]]);
    }
    float inv = 1.0f / (n_sel + 1);
    for (int e = tid; e < a.D; e += blockDim.x) W[e] *= inv;
    __syncthreads();

    // --- local update
    LogregArgs u;
    u.X = a.X; u.Y = a.Y; u.counts = a.dcounts;
    u.d = a.d; u.k = a.k; u.Smax = a.Smax; u.D = a.D;
    u.lr = a.lr; u.wd = a.wd; u.epochs = a.epochs; u.bs = a.bs;
    logreg_update<BIG>(u, node, c_n, W, xb, dz, age);
    __syncthreads();
    for (int e = tid; e < a.D; e += blockDim.x)
        a.params[(long)node * a.D + e] = W[e];
    if (tid == 0) a.ages[node] = age;
}

// PENS step-1 event for the MLP family, on the tick_mlp_kernel structure:
// model row LDS-resident, activations and two grad buffers behind it. The
// ONE model slab holds each candidate in turn while it is scored (forward
// only, mlp_forward over the receiver's shard in mlp_update's minibatch
// chunks, so the act scratch is large enough), then the own row, onto
// which the selected candidates are added straight from HBM.
struct PensMlpArgs {
    MlpArgs m;              // nodes/ptr: event receivers / candidate ranges
    const int* cslots;      // candidate slots
    const int* cowners;     // candidate senders (global node ids)
    int* wins;              // [n_local, n_total] winner counters
    int m_top, n_total;
};

__global__ void __launch_bounds__(512)
tick_pens_mlp_kernel(PensMlpArgs p)
{
    const MlpArgs& a = p.m;
    int i = blockIdx.x;
    int node = a.nodes[i];
    int tid = threadIdx.x;
    int lo = a.ptr[i], hi = a.ptr[i + 1];
    int n_cand = hi - lo;
    extern __shared__ float sm[];
    float* W = sm;          // D
    int bsmax = (a.bs == 0) ? a.Smax : min(a.bs, a.Smax);
    float* act = W + a.D;
    int act_total = 0;
    for (int l = 0; l < a.n_layers; ++l) act_total += a.layout[4 * l + 3];
    float* grad = act + bsmax * (a.d_in + act_total);
    __shared__ int correct[PENS_MAX_CAND];
    __shared__ int sel[PENS_MAX_CAND];

    int c_n = a.counts[node];
    int bsz = (a.bs == 0) ? c_n : min(a.bs, c_n);
    const float* Xn = a.X + (long)node * a.Smax * a.d_in;
    const float* Yn = a.Y + (long)node * a.Smax;
    int k = a.layout[4 * (a.n_layers - 1) + 3];

    // --- score candidates in arrival order
    for (int c = tid; c < n_cand; c += blockDim.x) correct[c] = 0;
    for (int c = 0; c < n_cand; ++c) {
        const float* Wc = a.slots + (long)p.cslots[lo + c] * a.D;
        for (int e = tid; e < a.D; e += blockDim.x) W[e] = Wc[e];
        for (int s0 = 0; s0 < c_n; s0 += bsz) {
            int m = min(bsz, c_n - s0);
            for (int e = tid; e < m * a.d_in; e += blockDim.x)
                act[e] = Xn[(long)s0 * a.d_in + e];
            __syncthreads();
            const float* head = mlp_forward(a, W, act, m);
            // (thread = sample, block-strided: a chunk may have more rows
            // than the block has threads); ascending scan, strict > — the
            // first maximum wins, as torch.argmax
            int my = 0;
            for (int s = tid; s < m; s += blockDim.x) {
                const float* z = head + s * k;
                float best = z[0];
                int bj = 0;
                for (int kk = 1; kk < k; ++kk) {
                    if (z[kk] > best) { best = z[kk]; bj = kk; }
                }
                if (bj == (int)Yn[s0 + s]) my += 1;
            }
            for (int off = WAVE / 2; off > 0; off >>= 1)
                my += __shfl_down(my, off, WAVE);
            if ((tid & (WAVE - 1)) == 0 && my) atomicAdd(&correct[c], my);
            // the head is read out before the next chunk or candidate
            // overwrites act and W
            __syncthreads();
        }
    }
    __syncthreads();

    // --- stable top-m selection (thread 0; n_cand small)
    if (tid == 0)
        pens_select(correct, sel, n_cand, p.m_top,
                    p.wins + (long)node * p.n_total, p.cowners + lo);
    __syncthreads();

    // --- merge: (own + sum selected) / (n_sel+1), age = max; each thread
    //     owns its elements of W throughout, so no barrier until the end
    for (int e = tid; e < a.D; e += blockDim.x)
        W[e] = a.params[(long)node * a.D + e];
    int n_sel = 0;
    int age = a.ages[node];
    for (int c = 0; c < n_cand; ++c) {
        if (!sel[c]) continue;
        n_sel += 1;
        int slot = p.cslots[lo + c];
        const float* Wc = a.slots + (long)slot * a.D;
        for (int e = tid; e < a.D; e += blockDim.x) W[e] += Wc[e];
        age = max(age, a.slot_ages[slot]);
    }
    float inv = 1.0f / (n_sel + 1);
    for (int e = tid; e < a.D; e += blockDim.x) W[e] *= inv;
    __syncthreads();

    // --- local update
    mlp_update<false>(a, node, W, act, grad, age);
    __syncthreads();
    for (int e = tid; e < a.D; e += blockDim.x)
        a.params[(long)node * a.D + e] = W[e];
    if (tid == 0) a.ages[node] = age;
}

// ---------------------------------------------------------------------------
// cooperative whole-round kernel (logreg family): the entire round — every
// tick's snapshot and delivery batch — runs inside ONE kernel launch, with
// grid.sync() as the tick barrier. Grids here are tiny (max batch ≈ a few
// dozen blocks on 256 CUs), so cooperative residency is guaranteed and the
// launch is REJECTED (not deadlocked) if ever oversubscribed. Cuts the
// ~200 per-round launch overheads of the stream executor to one.
// ---------------------------------------------------------------------------

struct CoopRoundArgs {
    LogregArgs base;  // nodes/ptr/dslots/rslots are set per group inside
    const int* snap_nodes; const int* snap_slots; const int* snap_tptr;
    const int* recv_nodes; const int* recv_nptr; const int* recv_tptr;
    const int* del_slots; const int* reply_slots;
    const int* pull_nodes; const int* pull_slots; const int* pull_tptr;
    const int* rep_nodes; const int* rep_nptr; const int* rep_tptr;
    const int* rep_slots;
    int delta;
};

// grid barrier that degrades to a block barrier when the kernel was
// launched PLAIN with one workgroup (the single-block round path for
// tiny-batch schedules — one launch per round, no cooperative API)
DEV_INLINE void round_sync()
{
    if (gridDim.x == 1) {
        __syncthreads();
    } else {
        cooperative_groups::this_grid().sync();
    }
}

template <bool BIG>  // as logreg_update's
__global__ void __launch_bounds__(128)
coop_round_logreg_kernel(CoopRoundArgs c)
{
    LogregArgs a = c.base;
    const int nb = gridDim.x;
    const int bid = blockIdx.x;
    const int tid = threadIdx.x;
    bool dirty = false;  // writes since the last grid sync

    for (int t = 0; t < c.delta; ++t) {
        int s0 = c.snap_tptr[t], s1 = c.snap_tptr[t + 1];
        int r0 = c.recv_tptr[t], r1 = c.recv_tptr[t + 1];
        int p0 = c.pull_tptr[t], p1 = c.pull_tptr[t + 1];
        int q0 = c.rep_tptr[t], q1 = c.rep_tptr[t + 1];

        if (s1 > s0) {
            if (dirty) { round_sync(); dirty = false; }
            // block-strided row copies (the snapshot sub-phase)
            for (int i = s0 + bid; i < s1; i += nb) {
                int node = c.snap_nodes[i];
                int slot = c.snap_slots[i];
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)slot * a.D + e] =
                        a.params[(long)node * a.D + e];
                if (tid == 0) a.slot_ages[slot] = a.ages[node];
            }
            dirty = true;
        }
        if (r1 > r0) {
            if (dirty) { round_sync(); dirty = false; }
            a.nodes = c.recv_nodes;
            a.ptr = c.recv_nptr;
            a.dslots = c.del_slots;
            a.rslots = c.reply_slots;
            for (int i = r0 + bid; i < r1; i += nb) {
                logreg_process_node<false, BIG>(a, i);
                __syncthreads();
            }
            dirty = true;
        }
        if (p1 > p0) {
            if (dirty) { round_sync(); dirty = false; }
            for (int i = p0 + bid; i < p1; i += nb) {
                int node = c.pull_nodes[i];
                int slot = c.pull_slots[i];
                for (int e = tid; e < a.D; e += blockDim.x)
                    a.slots[(long)slot * a.D + e] =
                        a.params[(long)node * a.D + e];
                if (tid == 0) a.slot_ages[slot] = a.ages[node];
            }
            dirty = true;
        }
        if (q1 > q0) {
            if (dirty) { round_sync(); dirty = false; }
            a.nodes = c.rep_nodes;
            a.ptr = c.rep_nptr;
            a.dslots = c.rep_slots;
            a.rslots = nullptr;
            for (int i = q0 + bid; i < q1; i += nb) {
                logreg_process_node<false, BIG>(a, i);
                __syncthreads();
            }
            dirty = true;
        }
    }
}

// ---------------------------------------------------------------------------
// single-block round kernels (linear / partitioned): for schedules whose
// per-tick batches are tiny (async gossip, tokenized 100-node configs),
// the whole round runs as ONE plain launch of ONE workgroup —
// __syncthreads() is the tick barrier, replacing ~2 launches per tick.
// ---------------------------------------------------------------------------

struct LinRoundArgs {
    LinearArgs base;
    const int* snap_nodes; const int* snap_slots; const int* snap_tptr;
    const int* recv_nodes; const int* recv_nptr; const int* recv_tptr;
    const int* del_slots; const int* reply_slots;
    const int* pull_nodes; const int* pull_slots; const int* pull_tptr;
    const int* rep_nodes; const int* rep_nptr; const int* rep_tptr;
    const int* rep_slots;
    int delta;
};

__global__ void __launch_bounds__(WAVE)
sb_round_linear_kernel(LinRoundArgs c)
{
    LinearArgs a = c.base;
    int tid = threadIdx.x;
    for (int t = 0; t < c.delta; ++t) {
        int s0 = c.snap_tptr[t], s1 = c.snap_tptr[t + 1];
        for (int i = s0; i < s1; ++i) {
            int node = c.snap_nodes[i], slot = c.snap_slots[i];
            for (int e = tid; e < a.d; e += blockDim.x)
                a.slots[(long)slot * a.d + e] = a.params[(long)node * a.d + e];
            if (tid == 0) a.slot_ages[slot] = a.ages[node];
        }
        __syncthreads();
        int r0 = c.recv_tptr[t], r1 = c.recv_tptr[t + 1];
        if (r1 > r0) {
            a.nodes = c.recv_nodes;
            a.ptr = c.recv_nptr;
            a.dslots = c.del_slots;
            a.rslots = c.reply_slots;
            for (int i = r0; i < r1; ++i) linear_process_node(a, i);
            __syncthreads();
        }
        int p0 = c.pull_tptr[t], p1 = c.pull_tptr[t + 1];
        for (int i = p0; i < p1; ++i) {
            int node = c.pull_nodes[i], slot = c.pull_slots[i];
            for (int e = tid; e < a.d; e += blockDim.x)
                a.slots[(long)slot * a.d + e] = a.params[(long)node * a.d + e];
            if (tid == 0) a.slot_ages[slot] = a.ages[node];
        }
        if (p1 > p0) __syncthreads();
        int q0 = c.rep_tptr[t], q1 = c.rep_tptr[t + 1];
        if (q1 > q0) {
            a.nodes = c.rep_nodes;
            a.ptr = c.rep_nptr;
            a.dslots = c.rep_slots;
            a.rslots = nullptr;
            for (int i = q0; i < q1; ++i) linear_process_node(a, i);
            __syncthreads();
        }
    }
}

struct PartRoundArgs {
    LogregPartArgs base;
    const int* snap_nodes; const int* snap_slots; const int* snap_tptr;
    const int* recv_nodes; const int* recv_nptr; const int* recv_tptr;
    const int* del_slots; const int* reply_slots; const int* del_pids;
    const int* pull_nodes; const int* pull_slots; const int* pull_tptr;
    const int* rep_nodes; const int* rep_nptr; const int* rep_tptr;
    const int* rep_slots; const int* rep_pids;
    int delta;
};

__global__ void __launch_bounds__(128)
sb_round_logreg_part_kernel(PartRoundArgs c)
{
    LogregPartArgs a = c.base;
    int tid = threadIdx.x;
    for (int t = 0; t < c.delta; ++t) {
        int s0 = c.snap_tptr[t], s1 = c.snap_tptr[t + 1];
        for (int i = s0; i < s1; ++i) {
            int node = c.snap_nodes[i], slot = c.snap_slots[i];
            for (int e = tid; e < a.D; e += blockDim.x)
                a.slots[(long)slot * a.D + e] = a.params[(long)node * a.D + e];
            for (int p = tid; p < a.P; p += blockDim.x)
                a.slot_ages[(long)slot * a.P + p] = a.ages[(long)node * a.P + p];
        }
        __syncthreads();
        int r0 = c.recv_tptr[t], r1 = c.recv_tptr[t + 1];
        if (r1 > r0) {
            a.nodes = c.recv_nodes;
            a.ptr = c.recv_nptr;
            a.dslots = c.del_slots;
            a.rslots = c.reply_slots;
            a.dpids = c.del_pids;
            for (int i = r0; i < r1; ++i) {
                logreg_part_process_node(a, i);
                __syncthreads();
            }
        }
        int p0 = c.pull_tptr[t], p1 = c.pull_tptr[t + 1];
        for (int i = p0; i < p1; ++i) {
            int node = c.pull_nodes[i], slot = c.pull_slots[i];
            for (int e = tid; e < a.D; e += blockDim.x)
                a.slots[(long)slot * a.D + e] = a.params[(long)node * a.D + e];
            for (int p = tid; p < a.P; p += blockDim.x)
                a.slot_ages[(long)slot * a.P + p] = a.ages[(long)node * a.P + p];
        }
        if (p1 > p0) __syncthreads();
        int q0 = c.rep_tptr[t], q1 = c.rep_tptr[t + 1];
        if (q1 > q0) {
            a.nodes = c.rep_nodes;
            a.ptr = c.rep_nptr;
            a.dslots = c.rep_slots;
            a.rslots = nullptr;
            a.dpids = c.rep_pids;
            for (int i = q0; i < q1; ++i) {
                logreg_part_process_node(a, i);
                __syncthreads();
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

#define CHECK_DEV(t) TORCH_CHECK(t.is_cuda() && t.is_contiguous(), #t " must be contiguous on device")

static hipStream_t current_stream()
{
    return at::hip::getCurrentHIPStream().stream();
}

// device pointer of an optional int array: null when empty or undefined
static const int* iptr(const torch::Tensor& t)
{
    return (t.defined() && t.numel()) ? t.data_ptr<int>() : nullptr;
}

// Launch of a kernel held as a pointer (a plan picks it at run time):
// hipLaunchKernel is the call a `<<<>>>` launch makes underneath.
template <typename Args>
static void launch_kernel(void (*kernel)(Args), int grid, int block,
                          size_t smem, hipStream_t s, Args& a)
{
    void* kargs[] = {&a};
    hipError_t err = hipLaunchKernel((const void*)kernel, dim3(grid),
                                     dim3(block), kargs, smem, s);
    TORCH_CHECK(err == hipSuccess, "kernel launch failed: ",
                hipGetErrorString(err));
}

// What a snapshot of one row copies: W floats from column src_off of a
// Dp-wide params row, and age_w ages.
struct SnapGeom {
    int W, Dp, src_off, age_w;
};

static void launch_snap(const float* params, const int* ages, float* slots,
                        int* slot_ages, const int* nodes, const int* slot_ids,
                        int n, const SnapGeom& g, hipStream_t s)
{
    long total = (long)n * g.W;
    int block = 256;
    int grid = (int)std::min<long>((total + block - 1) / block, 2048);
    hipLaunchKernelGGL(snapshot_kernel, dim3(grid), dim3(block), 0, s,
                       params, ages, slots, slot_ages, nodes, slot_ids, n,
                       g.W, g.Dp, g.src_off, g.age_w);
}

void snapshot(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
              torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor slot_ids,
              int64_t age_width, int64_t src_off)
{
    CHECK_DEV(params); CHECK_DEV(slots); CHECK_DEV(nodes); CHECK_DEV(slot_ids);
    int n = nodes.size(0);
    if (n == 0) return;
    SnapGeom g{(int)slots.size(1), (int)params.size(1), (int)src_off,
               (int)age_width};
    launch_snap(params.data_ptr<float>(), ages.data_ptr<int>(),
                slots.data_ptr<float>(), slot_ages.data_ptr<int>(),
                nodes.data_ptr<int>(), slot_ids.data_ptr<int>(), n, g,
                current_stream());
}

void wmerge(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
            torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor ptr,
            torch::Tensor wslots, torch::Tensor wweights, torch::Tensor selfw)
{
    CHECK_DEV(params); CHECK_DEV(slots); CHECK_DEV(nodes); CHECK_DEV(ptr);
    int n = nodes.size(0);
    if (n == 0) return;
    int D = params.size(1);
    hipLaunchKernelGGL(wmerge_kernel, dim3(n), dim3(128), 0, current_stream(),
        params.data_ptr<float>(), ages.data_ptr<int>(),
        slots.data_ptr<float>(), slot_ages.data_ptr<int>(),
        nodes.data_ptr<int>(), ptr.data_ptr<int>(),
        wslots.numel() ? wslots.data_ptr<int>() : nullptr,
        wweights.numel() ? wweights.data_ptr<float>() : nullptr,
        selfw.data_ptr<float>(), D);
}

// ---------------------------------------------------------------------------
// launch plans: everything about a family's launch that depends on the spec
// alone, built by ONE function per family that both its tick_X and its
// run_round_X entry point call. A plan holds the args struct with every
// per-spec field filled and every check done, the kernel, its dynamic LDS
// and block size, and the snapshot geometry of the family's rows. The
// per-call event pointers (nodes, ptr, dslots, rslots, update_only and the
// family's per-delivery channel: dmodes / dpids / dseeds) are left to
// launch_tick and stream_round.
// ---------------------------------------------------------------------------

template <typename Args>
struct Plan {
    Args a{};
    void (*kernel)(Args) = nullptr;
    // a second instantiation for launches of at most thin_rows workgroups,
    // or null (see thin_launch_rows)
    void (*kernel_thin)(Args) = nullptr;
    int thin_rows = 0;
    size_t smem = 0;
    int threads = 0;
    SnapGeom snap{};
};

template <typename Args>
static auto plan_kernel(const Plan<Args>& L, int n)
{
    return (L.kernel_thin && n <= L.thin_rows) ? L.kernel_thin : L.kernel;
}

// the per-delivery channel of a family: a `const int*` member of its args
template <typename Args>
struct channel {
    using type = const int* Args::*;
};

// the arena, pool and data tensors every family's entry points take
struct StateTensors {
    torch::Tensor params, ages, slots, slot_ages, X, Y, counts;
};

template <typename A>
static void fill_state_x(A& a, const StateTensors& st)
{
    const torch::Tensor &params = st.params, &slots = st.slots, &X = st.X;
    CHECK_DEV(params); CHECK_DEV(slots); CHECK_DEV(X);
    a.params = params.data_ptr<float>(); a.ages = st.ages.data_ptr<int>();
    a.slots = slots.data_ptr<float>(); a.slot_ages = st.slot_ages.data_ptr<int>();
    a.X = X.data_ptr<float>(); a.counts = st.counts.data_ptr<int>();
    a.Smax = X.size(1);
}

template <typename A>
static void fill_state(A& a, const StateTensors& st)
{
    fill_state_x(a, st);
    const torch::Tensor& Y = st.Y;
    CHECK_DEV(Y);
    a.Y = Y.data_ptr<float>();
}

template <typename A>
static void fill_sgd(A& a, double lr, double wd, int64_t epochs, int64_t bs,
                     int64_t mode)
{
    a.lr = lr; a.wd = wd; a.epochs = epochs; a.bs = bs; a.mode = mode;
}

// rows of the largest minibatch (bs == 0: the whole shard)
static int batch_rows(int64_t bs, int Smax)
{
    return (bs == 0) ? Smax : std::min<int>(bs, Smax);
}

// the logreg kernels run LOGREG_THREADS threads, one per sample in the
// dLoss/dz stage; a larger batch needs the BIG instantiation, which strides
constexpr int LOGREG_THREADS = 128;
static bool big_batch(int64_t bs, int Smax)
{
    return batch_rows(bs, Smax) > LOGREG_THREADS;
}

// The largest launch whose waves each have a SIMD to themselves (4 SIMDs per
// CU): up to there a kernel's register count costs no occupancy, so the
// instantiation with the shorter dependent chain and more registers runs;
// above it the one that keeps 8 waves per SIMD.
static int thin_launch_rows(int threads)
{
    int dev = 0, cus = 0;
    hipError_t err = hipGetDevice(&dev);
    if (err == hipSuccess)
        err = hipDeviceGetAttribute(
            &cus, hipDeviceAttributeMultiprocessorCount, dev);
    TORCH_CHECK(err == hipSuccess, "device query failed: ",
                hipGetErrorString(err));
    return cus * 4 / std::max(1, threads / WAVE);
}

// merge_limit of a plan: -1 = plain mean merge, L >= 0 = limited merge.
// Ages are int32 and the rule adds L to one, so L is kept far below 2^31.
static int check_merge_limit(int64_t merge_limit)
{
    TORCH_CHECK(merge_limit >= -1 && merge_limit <= (1 << 30),
                "merge_limit must be -1 (off) or in [0, 2^30], got ",
                merge_limit);
    return (int)std::max<int64_t>(merge_limit, 0);
}

// the event fields live in the args struct itself, except that the
// compressed MLP wraps a plain MlpArgs
template <typename A> static A& events(A& a) { return a; }
static MlpArgs& events(MlpCompArgs& c) { return c.m; }

static Plan<LogregArgs> logreg_plan(
    const StateTensors& st, int64_t d, int64_t k, double lr, double wd,
    int64_t epochs, int64_t bs, int64_t mode, int64_t merge_limit = -1)
{
    Plan<LogregArgs> L;
    LogregArgs& a = L.a;
    fill_state(a, st);
    TORCH_CHECK(k <= KMAX, "n_classes > ", KMAX, " unsupported");
    a.d = d; a.k = k; a.D = st.params.size(1);
    fill_sgd(a, lr, wd, epochs, bs, mode);
    a.lim = check_merge_limit(merge_limit);
    int bsmax = batch_rows(bs, a.Smax);
    L.smem = sizeof(float) * (2 * a.D + (size_t)bsmax * a.d + (size_t)bsmax * a.k);
    TORCH_CHECK(L.smem <= 160 * 1024, "logreg LDS budget exceeded: ", L.smem);
    bool lim = merge_limit >= 0;
    if (big_batch(bs, a.Smax)) {
        L.kernel = lim ? tick_logreg_lim_big_kernel : tick_logreg_big_kernel;
        L.kernel_thin = lim ? tick_logreg_lim_big_thin_kernel
                            : tick_logreg_big_thin_kernel;
    } else {
        L.kernel = lim ? tick_logreg_lim_kernel : tick_logreg_kernel;
        L.kernel_thin = lim ? tick_logreg_lim_thin_kernel
                            : tick_logreg_thin_kernel;
    }
    L.threads = LOGREG_THREADS;
    L.thin_rows = thin_launch_rows(LOGREG_THREADS);
    L.snap = {a.D, a.D, 0, 1};
    return L;
}

static Plan<LinearArgs> linear_plan(
    const StateTensors& st, int64_t d, double lrlam, int64_t is_pegasos,
    int64_t mode)
{
    Plan<LinearArgs> L;
    LinearArgs& a = L.a;
    fill_state(a, st);
    TORCH_CHECK(d <= LIN_MAX_REGS * WAVE, "d > ", LIN_MAX_REGS * WAVE, " unsupported");
    a.d = d;
    a.lrlam = lrlam; a.is_pegasos = is_pegasos; a.mode = mode;
    L.kernel = tick_linear_kernel;
    L.threads = WAVE;
    L.snap = {a.d, a.d, 0, 1};
    return L;
}

static Plan<LogregPartArgs> logreg_part_plan(
    const StateTensors& st, torch::Tensor perm, torch::Tensor pptr,
    torch::Tensor apart, int64_t n_parts, int64_t d, int64_t k, double lr,
    double wd, int64_t epochs, int64_t bs, int64_t mode)
{
    Plan<LogregPartArgs> L;
    LogregPartArgs& a = L.a;
    fill_state(a, st);
    CHECK_DEV(perm); CHECK_DEV(pptr); CHECK_DEV(apart);
    TORCH_CHECK(k <= KMAX, "n_classes > ", KMAX, " unsupported");
    TORCH_CHECK(mode != MODE_PASS, "Mode PASS not allowed for partitioned models.");
    a.perm = perm.data_ptr<int>(); a.pptr = pptr.data_ptr<int>();
    a.apart = apart.data_ptr<int>();
    a.P = n_parts; a.d = d; a.k = k; a.D = st.params.size(1);
    fill_sgd(a, lr, wd, epochs, bs, mode);
    int bsmax = batch_rows(bs, a.Smax);
    // whole-shard staging when it fits a 64 KB block budget (keeps >=2
    // blocks/CU); otherwise per-step slices
    size_t full = sizeof(float) * (2 * a.D + (size_t)a.Smax * a.d +
                                   (size_t)bsmax * a.k) +
                  sizeof(int) * 2 * a.P;
    a.stage_full = (full <= 64 * 1024) ? 1 : 0;
    L.smem = a.stage_full
        ? full
        : sizeof(float) * (2 * a.D + (size_t)bsmax * a.d +
                           (size_t)bsmax * a.k) +
              sizeof(int) * 2 * a.P;
    TORCH_CHECK(L.smem <= 160 * 1024, "partitioned logreg LDS budget exceeded: ", L.smem);
    L.kernel = tick_logreg_part_kernel;
    L.threads = 128;
    L.snap = {a.D, a.D, 0, a.P};
    return L;
}

static Plan<LogregSampArgs> logreg_samp_plan(
    const StateTensors& st, int64_t samp_c, int64_t d, int64_t k, double lr,
    double wd, int64_t epochs, int64_t bs, int64_t mode)
{
    Plan<LogregSampArgs> L;
    LogregSampArgs& a = L.a;
    fill_state(a, st);
    TORCH_CHECK(k <= KMAX, "n_classes > ", KMAX, " unsupported");
    TORCH_CHECK(mode != MODE_PASS, "Mode PASS not allowed for sampled models.");
    a.samp_c = samp_c; a.d = d; a.k = k; a.D = st.params.size(1);
    fill_sgd(a, lr, wd, epochs, bs, mode);
    int bsmax = batch_rows(bs, a.Smax);
    L.smem = sizeof(float) * (3 * a.D + (size_t)bsmax * a.d +
                              (size_t)bsmax * a.k);
    TORCH_CHECK(L.smem <= 160 * 1024, "sampled logreg LDS budget exceeded: ", L.smem);
    L.kernel = big_batch(bs, a.Smax) ? tick_logreg_samp_kernel<true>
                                     : tick_logreg_samp_kernel<false>;
    L.threads = LOGREG_THREADS;
    L.snap = {a.D, a.D, 0, 1};
    return L;
}

static Plan<MFArgs> mf_plan(const StateTensors& st, int64_t k, int64_t n_items,
                            double reg, double lr)
{
    Plan<MFArgs> L;
    MFArgs& a = L.a;
    fill_state(a, st);
    TORCH_CHECK(k <= WAVE, "MF latent dim > ", WAVE, " unsupported");
    a.k = k; a.n_items = n_items; a.D = st.params.size(1);
    a.item_off = k + 1; a.Wslot = n_items * (k + 1);
    a.reg = reg; a.lr = lr;
    L.kernel = tick_mf_kernel;
    L.threads = 256;
    // MF snapshots carry only the item block
    L.snap = {a.Wslot, a.D, a.item_off, 1};
    return L;
}

static Plan<KMeansArgs> kmeans_plan(const StateTensors& st, int64_t k,
                                    int64_t dim, double alpha, int64_t mode)
{
    Plan<KMeansArgs> L;
    KMeansArgs& a = L.a;
    fill_state_x(a, st);
    a.k = k; a.dim = dim; a.D = st.params.size(1);
    a.alpha = alpha; a.mode = mode;
    L.smem = sizeof(float) * 2 * a.D + sizeof(int) * a.Smax;
    TORCH_CHECK(L.smem <= 160 * 1024, "kmeans LDS budget exceeded: ", L.smem);
    L.kernel = tick_kmeans_kernel;
    L.threads = 128;
    L.snap = {a.D, a.D, 0, 1};
    return L;
}

// What the plain and the compressed MLP plan share: state, layout and SGD
// fields of the MlpArgs, and the launch geometry the layer shapes imply.
struct MlpGeom {
    size_t scratch;  // floats of activations + two grad buffers
    int threads;
    // the same for tick_mlp_wide_kernel, which stages no input and computes
    // no dX of layer 0: the layers' outputs + two buffers of the widest one
    size_t wide_scratch;
    int out_max;
};

constexpr size_t LDS_BUDGET = 160 * 1024;

// floats of activations + two grad buffers for `rows` batch rows: with the
// input staged and the buffers as wide as the widest layer side (the LDS
// kernels), or without the input and by output widths alone (wide)
static size_t mlp_scratch(int64_t rows, int64_t d_in, int64_t out_sum,
                          int64_t width_max, bool wide)
{
    return (size_t)rows * ((wide ? 0 : d_in) + out_sum) +
           2 * (size_t)rows * width_max;
}

// Which kernel serves a plain MLP tick whose LDS-resident plan needs
// `lds_bytes`: tick_mlp_kernel whenever that fits, else the global-resident
// tick_mlp_wide_kernel. GOSSIPY_MLP_WIDE=1 forces the wide kernel on any
// shape (tests, A/B runs), =0 turns it off, which restores the budget error.
static bool mlp_use_wide(size_t lds_bytes)
{
    const char* v = getenv("GOSSIPY_MLP_WIDE");
    int knob = (v && *v) ? (atoi(v) != 0) : -1;
    if (knob == 1) return true;
    bool fits = lds_bytes <= LDS_BUDGET;
    TORCH_CHECK(fits || knob != 0,
        "mlp LDS budget exceeded (", lds_bytes, " B); shrink batch_size/hidden"
        " (GOSSIPY_MLP_WIDE=0 has turned the global-resident kernel off)");
    return !fits;
}

// Per-block rows of device memory for tick_mlp_wide_kernel, one buffer per
// (device, stream): grown when a plan needs more, never shrunk, and reused
// by every later plan, so a round loop allocates nothing after its first
// launch. Never freed: the process's exit must not run into a torn-down
// runtime.
static float* mlp_wide_workspace(const torch::Device& dev, size_t floats)
{
    static auto* cache =
        new std::map<std::pair<int, hipStream_t>, torch::Tensor>();
    torch::Tensor& t = (*cache)[{(int)dev.index(), current_stream()}];
    if (!t.defined() || (size_t)t.numel() < floats)
        t = torch::empty({(int64_t)floats},
                         torch::dtype(torch::kFloat32).device(dev));
    return t.data_ptr<float>();
}

static MlpGeom mlp_fill(MlpArgs& a, const StateTensors& st,
                        torch::Tensor layout, int64_t n_layers, double lr,
                        double wd, int64_t epochs, int64_t bs, int64_t mode)
{
    fill_state(a, st);
    CHECK_DEV(layout);
    TORCH_CHECK(n_layers >= 1 && layout.numel() == 4 * n_layers,
                "mlp layout must hold n_layers x (w_off, b_off, in, out)");
    a.layout = layout.data_ptr<int>();
    a.n_layers = n_layers; a.D = st.params.size(1);
    fill_sgd(a, lr, wd, epochs, bs, mode);
    auto lay = layout.cpu();
    const int* Lh = lay.data_ptr<int>();
    int act_sum = 0, act_max = Lh[2], out_max = 0;
    for (int l = 0; l < n_layers; ++l) {
        act_sum += Lh[4 * l + 3];
        out_max = std::max(out_max, Lh[4 * l + 3]);
        act_max = std::max(act_max, Lh[4 * l + 3]);
        act_max = std::max(act_max, Lh[4 * l + 2]);
    }
    a.act_max = act_max;
    a.d_in = Lh[2];
    int bsmax = batch_rows(bs, a.Smax);
    MlpGeom g;
    g.scratch = mlp_scratch(bsmax, a.d_in, act_sum, act_max, false);
    g.wide_scratch = mlp_scratch(bsmax, a.d_in, act_sum, out_max, true);
    g.out_max = out_max;
    // block size: 8 waves when any GEMM stage has >= 8 MFMA tiles (halves
    // the sequential tile passes of the widest stage — e.g. dW [100,57] is
    // 28 tiles), else the default 4 waves
    int max_tiles = 0;
    int m16 = (bsmax + 15) >> 4;
    for (int l = 0; l < n_layers; ++l) {
        int fin16 = (Lh[4 * l + 2] + 15) >> 4;
        int fout16 = (Lh[4 * l + 3] + 15) >> 4;
        max_tiles = std::max(max_tiles, m16 * fout16);   // forward
        max_tiles = std::max(max_tiles, m16 * fin16);    // dX
        max_tiles = std::max(max_tiles, fout16 * fin16); // dW
    }
    g.threads = (max_tiles >= 8) ? 512 : 256;
    return g;
}

static Plan<MlpArgs> mlp_plan(
    const StateTensors& st, torch::Tensor layout, int64_t n_layers, double lr,
    double wd, int64_t epochs, int64_t bs, int64_t mode,
    int64_t merge_limit = -1)
{
    Plan<MlpArgs> L;
    MlpArgs& a = L.a;
    MlpGeom g = mlp_fill(a, st, layout, n_layers, lr, wd, epochs, bs, mode);
    a.lim = check_merge_limit(merge_limit);
    // LDS: model (+ scratch copy W2, UPDATE_MERGE only) + activations +
    // 2 grad buffers
    size_t w_slabs = (mode == MODE_UPDATE_MERGE) ? 2 : 1;
    L.smem = sizeof(float) * (w_slabs * (size_t)a.D + g.scratch);
    bool lim = merge_limit >= 0;
    L.threads = g.threads;
    L.snap = {a.D, a.D, 0, 1};
    if (!mlp_use_wide(L.smem)) {
        L.kernel = lim ? tick_mlp_kernel<true> : tick_mlp_kernel<false>;
        return L;
    }
    // wide: the rows live in device memory; the workspace row holds W2
    // (UPDATE_MERGE only) and, when a batch's activations and gradients miss
    // the LDS budget too, those. One row per node bounds every launch, as
    // receivers are unique within one. No workspace without either.
    a.act_max = g.out_max;
    bool act_ws = sizeof(float) * g.wide_scratch > LDS_BUDGET;
    L.smem = act_ws ? 0 : sizeof(float) * g.wide_scratch;
    a.ws_row = (mode == MODE_UPDATE_MERGE ? a.D : 0) +
               (act_ws ? (long)g.wide_scratch : 0);
    size_t ws_bytes = sizeof(float) * (size_t)a.ws_row * st.params.size(0);
    TORCH_CHECK(ws_bytes <= ((size_t)1 << 34),
        "mlp wide workspace too large: ", st.params.size(0), " nodes x ",
        a.ws_row, " floats (trained copy of the received model + a batch's"
        " activations and gradients) = ", ws_bytes,
        " B > 16 GiB; shrink batch_size/hidden");
    a.ws = a.ws_row ? mlp_wide_workspace(st.params.device(),
                                         (size_t)a.ws_row * st.params.size(0))
                    : nullptr;
    if (act_ws)
        L.kernel = lim ? tick_mlp_wide_kernel<true, true>
                       : tick_mlp_wide_kernel<false, true>;
    else
        L.kernel = lim ? tick_mlp_wide_kernel<true, false>
                       : tick_mlp_wide_kernel<false, false>;
    return L;
}

// "lds" or "wide": the kernel mlp_plan picks for a plain MLP tick of layer
// widths `dims` (d_in, hidden..., n_classes) on shards of stride Smax
static std::string mlp_tick_path(std::vector<int64_t> dims, int64_t bs,
                                 int64_t Smax, int64_t mode)
{
    TORCH_CHECK(dims.size() >= 2, "dims must hold d_in and n_classes");
    int64_t D = 0, out_sum = 0, width_max = dims[0];
    for (size_t l = 0; l + 1 < dims.size(); ++l) {
        D += dims[l + 1] * dims[l] + dims[l + 1];
        out_sum += dims[l + 1];
        width_max = std::max(width_max, dims[l + 1]);
    }
    size_t w_slabs = (mode == MODE_UPDATE_MERGE) ? 2 : 1;
    size_t lds = sizeof(float) *
                 (w_slabs * (size_t)D +
                  mlp_scratch(batch_rows(bs, (int)Smax), dims[0], out_sum,
                              width_max, false));
    return mlp_use_wide(lds) ? "wide" : "lds";
}

// Partitioned (part) or sampled compressed MLP. Checks the per-mode LDS
// budget: W, +W2 unless MERGE_UPDATE, +the sampled pre-merge copy unless it
// fits the act/grad scratch, activations, two grad buffers, 2*P age ints
// when partitioned. The partition tables are read when part only.
static Plan<MlpCompArgs> mlp_comp_plan(
    bool part, const StateTensors& st, torch::Tensor layout, int64_t n_layers,
    torch::Tensor perm, torch::Tensor pptr, torch::Tensor apart,
    int64_t n_parts, int64_t samp_c, double lr, double wd, int64_t epochs,
    int64_t bs, int64_t mode)
{
    const char* what = part ? "partitioned" : "sampled";
    Plan<MlpCompArgs> L;
    MlpCompArgs& c = L.a;
    MlpArgs& a = c.m;
    TORCH_CHECK(mode != MODE_PASS, "Mode PASS not allowed for ", what,
                " models.");
    MlpGeom g = mlp_fill(a, st, layout, n_layers, lr, wd, epochs, bs, mode);
    c.P = part ? (int)n_parts : 0;
    c.samp_c = part ? 0 : (int)samp_c;
    if (part) {
        const torch::Tensor &ages = st.ages, &slot_ages = st.slot_ages;
        CHECK_DEV(perm); CHECK_DEV(pptr); CHECK_DEV(apart);
        TORCH_CHECK(n_parts >= 1, "n_parts must be positive");
        TORCH_CHECK(ages.numel() == ages.size(0) * n_parts &&
                    slot_ages.numel() == slot_ages.size(0) * n_parts,
                    "partitioned mlp: ages and slot_ages must be [*, n_parts]");
        TORCH_CHECK(perm.numel() == a.D && apart.numel() == a.D &&
                    pptr.numel() == n_parts + 1,
                    "partition tables do not match the model row");
        c.perm = perm.data_ptr<int>(); c.pptr = pptr.data_ptr<int>();
        c.apart = apart.data_ptr<int>();
    } else {
        TORCH_CHECK(samp_c >= 1, "samp_c must be positive");
    }
    size_t w_slabs = (mode == MODE_MERGE_UPDATE) ? 1 : 2;
    if (!part) {
        c.w3_alias = (g.scratch >= (size_t)a.D) ? 1 : 0;
        if (!c.w3_alias) w_slabs += 1;
    }
    L.smem = sizeof(float) * (w_slabs * (size_t)a.D + g.scratch) +
             sizeof(int) * 2 * (size_t)c.P;
    TORCH_CHECK(L.smem <= 160 * 1024, what, " mlp LDS budget exceeded (",
                L.smem, " B > 163840 B); shrink batch_size/hidden, or use"
                " MERGE_UPDATE (the other modes hold a second model slab)."
                " The global-resident wide kernel covers the plain MLP tick"
                " only");
    L.kernel = part ? tick_mlp_comp_kernel<true> : tick_mlp_comp_kernel<false>;
    L.threads = g.threads;
    // snapshots copy one age per partition
    L.snap = {a.D, a.D, 0, part ? (int)n_parts : 1};
    return L;
}

// ---------------------------------------------------------------------------
// tick entry points: one launch, one workgroup per receiving node
// ---------------------------------------------------------------------------

struct TickEvents {
    torch::Tensor nodes, recv_ptr, del_slots, reply_slots;
};

template <typename Args>
static void launch_tick(Plan<Args>& L, const TickEvents& ev, bool update_only,
                        typename channel<Args>::type chan = nullptr,
                        const torch::Tensor& chan_vals = {})
{
    const torch::Tensor &nodes = ev.nodes, &recv_ptr = ev.recv_ptr;
    int n = nodes.size(0);
    if (n == 0) return;
    CHECK_DEV(nodes); CHECK_DEV(recv_ptr);
    auto& e = events(L.a);
    e.nodes = nodes.data_ptr<int>(); e.ptr = recv_ptr.data_ptr<int>();
    e.dslots = iptr(ev.del_slots); e.rslots = iptr(ev.reply_slots);
    e.update_only = update_only;
    if (chan) L.a.*chan = iptr(chan_vals);
    launch_kernel(plan_kernel(L, n), n, L.threads, L.smem, current_stream(),
                  L.a);
}

// `merge_limit` of the logreg and MLP entry points is the limited-merge
// threshold L, -1 = off.
void tick_logreg(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
                 torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
                 torch::Tensor del_slots, torch::Tensor reply_slots,
                 torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
                 int64_t d, int64_t k, double lr, double wd, int64_t epochs,
                 int64_t bs, int64_t mode, int64_t merge_limit,
                 bool update_only, torch::Tensor dmodes)
{
    auto L = logreg_plan({params, ages, slots, slot_ages, X, Y, counts},
                         d, k, lr, wd, epochs, bs, mode, merge_limit);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only,
                &LogregArgs::dmodes, dmodes);
}

void tick_linear(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
                 torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
                 torch::Tensor del_slots, torch::Tensor reply_slots,
                 torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
                 int64_t d, double lrlam, int64_t is_pegasos, int64_t mode,
                 bool update_only, torch::Tensor dmodes)
{
    auto L = linear_plan({params, ages, slots, slot_ages, X, Y, counts},
                         d, lrlam, is_pegasos, mode);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only,
                &LinearArgs::dmodes, dmodes);
}

void tick_mlp(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
              torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
              torch::Tensor del_slots, torch::Tensor reply_slots,
              torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
              torch::Tensor layout, int64_t n_layers, double lr, double wd,
              int64_t epochs, int64_t bs, int64_t mode, int64_t merge_limit,
              bool update_only, torch::Tensor dmodes)
{
    auto L = mlp_plan({params, ages, slots, slot_ages, X, Y, counts},
                      layout, n_layers, lr, wd, epochs, bs, mode, merge_limit);
    // receivers are unique within a launch (the wide kernel's workspace has
    // one row per node)
    TORCH_CHECK(nodes.size(0) <= params.size(0), "tick_mlp: ", nodes.size(0),
                " receivers for ", params.size(0), " nodes");
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only,
                &MlpArgs::dmodes, dmodes);
}

void tick_logreg_part(
    torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
    torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
    torch::Tensor del_slots, torch::Tensor reply_slots, torch::Tensor del_pids,
    torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
    torch::Tensor perm, torch::Tensor pptr, torch::Tensor apart,
    int64_t n_parts, int64_t d, int64_t k, double lr, double wd,
    int64_t epochs, int64_t bs, int64_t mode, bool update_only)
{
    auto L = logreg_part_plan({params, ages, slots, slot_ages, X, Y, counts},
                              perm, pptr, apart, n_parts, d, k, lr, wd,
                              epochs, bs, mode);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only,
                &LogregPartArgs::dpids, del_pids);
}

void tick_logreg_samp(
    torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
    torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
    torch::Tensor del_slots, torch::Tensor reply_slots, torch::Tensor del_seeds,
    torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
    int64_t samp_c, int64_t d, int64_t k, double lr, double wd,
    int64_t epochs, int64_t bs, int64_t mode, bool update_only)
{
    auto L = logreg_samp_plan({params, ages, slots, slot_ages, X, Y, counts},
                              samp_c, d, k, lr, wd, epochs, bs, mode);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only,
                &LogregSampArgs::dseeds, del_seeds);
}

void tick_mlp_part(
    torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
    torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
    torch::Tensor del_slots, torch::Tensor reply_slots, torch::Tensor del_pids,
    torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
    torch::Tensor layout, int64_t n_layers,
    torch::Tensor perm, torch::Tensor pptr, torch::Tensor apart,
    int64_t n_parts, double lr, double wd, int64_t epochs, int64_t bs,
    int64_t mode, bool update_only)
{
    auto L = mlp_comp_plan(true, {params, ages, slots, slot_ages, X, Y, counts},
                           layout, n_layers, perm, pptr, apart, n_parts, 0,
                           lr, wd, epochs, bs, mode);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only,
                &MlpCompArgs::dpids, del_pids);
}

void tick_mlp_samp(
    torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
    torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
    torch::Tensor del_slots, torch::Tensor reply_slots, torch::Tensor del_seeds,
    torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
    torch::Tensor layout, int64_t n_layers, int64_t samp_c,
    double lr, double wd, int64_t epochs, int64_t bs, int64_t mode,
    bool update_only)
{
    auto L = mlp_comp_plan(false, {params, ages, slots, slot_ages, X, Y, counts},
                           layout, n_layers, {}, {}, {}, 0, samp_c,
                           lr, wd, epochs, bs, mode);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only,
                &MlpCompArgs::dpids, del_seeds);
}

void tick_mf(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
             torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor recv_ptr,
             torch::Tensor del_slots, torch::Tensor reply_slots,
             torch::Tensor X, torch::Tensor Y, torch::Tensor counts,
             int64_t k, int64_t n_items, double reg, double lr,
             bool update_only)
{
    auto L = mf_plan({params, ages, slots, slot_ages, X, Y, counts},
                     k, n_items, reg, lr);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only);
}

void tick_kmeans(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
                 torch::Tensor slot_ages, torch::Tensor nodes,
                 torch::Tensor recv_ptr, torch::Tensor del_slots,
                 torch::Tensor reply_slots, torch::Tensor X,
                 torch::Tensor counts, int64_t k, int64_t dim, double alpha,
                 int64_t mode, bool update_only)
{
    auto L = kmeans_plan({params, ages, slots, slot_ages, X, {}, counts},
                         k, dim, alpha, mode);
    launch_tick(L, {nodes, recv_ptr, del_slots, reply_slots}, update_only);
}

// ---------------------------------------------------------------------------
// round executors: the C++ loop over one round's ticks. All event arrays
// arrive on-device ONCE per round; tick boundary pointers stay host-side.
// Per tick this issues up to 4 stream-ordered launches (snapshot, deliver,
// pull-snapshot, reply-deliver) with zero per-tick Python involvement —
// the host cost of a 100-tick round drops from ~10 ms of Python to
// ~200 launch enqueues of a few µs each.
// ---------------------------------------------------------------------------

// One round's arrays, indexed by the table of csrc/round_source.h.
// del_pids / rep_pids carry the partition ids (partitioned) or sample seeds
// (sampled) of each delivery; the plain families ignore them.
struct RoundArrays {
    const int* dev[ROUND_N_ARRAYS];  // device pointers; nullptr: empty
    // tick pointers [delta+1]: host-side for the stream executors,
    // device-side for the whole-round kernels
    const int* tptr[ROUND_N_TPTRS];
    int delta;
};

// The one place a RoundArrays is built: the arrays lie in one device buffer
// at `base`, array i at off[i] with len[i] elements.
static RoundArrays round_arrays(const int* base, const size_t* off,
                                const size_t* len,
                                const int* const tptr[ROUND_N_TPTRS],
                                size_t tptr_len)
{
    RoundArrays r;
    for (int i = 0; i < ROUND_N_ARRAYS; ++i)
        r.dev[i] = len[i] ? base + off[i] : nullptr;
    for (int i = 0; i < ROUND_N_TPTRS; ++i) r.tptr[i] = tptr[i];
    r.delta = (int)tptr_len - 1;
    return r;
}

using TptrTensors = std::array<torch::Tensor, ROUND_N_TPTRS>;

// The one stream round loop: per tick snapshot, deliver, pull-snapshot,
// reply-deliver. `chan` names the family's per-delivery pids/seeds member
// (set from del_pids for deliveries, rep_pids for replies), or is null.
template <typename Args>
static void stream_round(Plan<Args>& L, const RoundArrays& r,
                         typename channel<Args>::type chan = nullptr)
{
    hipStream_t s = current_stream();
    auto& e = events(L.a);
    auto snap = [&](const int* nodes, const int* slot_ids, int n) {
        launch_snap(e.params, e.ages, e.slots, e.slot_ages, nodes, slot_ids,
                    n, L.snap, s);
    };
    auto deliver = [&](const int* nodes, const int* nptr, int n,
                       const int* dslots, const int* rslots, const int* pids) {
        e.nodes = nodes; e.ptr = nptr; e.dslots = dslots; e.rslots = rslots;
        if (chan) L.a.*chan = pids;
        launch_kernel(plan_kernel(L, n), n, L.threads, L.smem, s, L.a);
    };
    const int* const* a = r.dev;
    for (int t = 0; t < r.delta; ++t) {
        int s0 = r.tptr[RT_SNAP][t], s1 = r.tptr[RT_SNAP][t + 1];
        if (s1 > s0)
            snap(a[RA_SNAP_NODES] + s0, a[RA_SNAP_SLOTS] + s0, s1 - s0);
        int r0 = r.tptr[RT_RECV][t], r1 = r.tptr[RT_RECV][t + 1];
        if (r1 > r0)
            deliver(a[RA_RECV_NODES] + r0, a[RA_RECV_NPTR] + r0, r1 - r0,
                    a[RA_DEL_SLOTS], a[RA_REPLY_SLOTS], a[RA_DEL_PIDS]);
        int p0 = r.tptr[RT_PULL][t], p1 = r.tptr[RT_PULL][t + 1];
        if (p1 > p0)
            snap(a[RA_PULL_NODES] + p0, a[RA_PULL_SLOTS] + p0, p1 - p0);
        int q0 = r.tptr[RT_REP][t], q1 = r.tptr[RT_REP][t + 1];
        if (q1 > q0)
            deliver(a[RA_REP_NODES] + q0, a[RA_REP_NPTR] + q0, q1 - q0,
                    a[RA_REP_SLOTS], a[RA_REP_REPLY_SLOTS], a[RA_REP_PIDS]);
    }
}

static int sb_threshold()
{
    // measured on MI355X: the single-workgroup round is ~5% SLOWER than
    // back-to-back stream launches even at 1-3-block batches (the stream
    // front-end pipelines launches well on gfx950), so the path is
    // opt-in via GOSSIPY_SB_MAX (profiles/r01_coop_ab.txt)
    const char* v = getenv("GOSSIPY_SB_MAX");
    return v ? atoi(v) : 0;
}

// largest per-tick batch across all four event kinds (host-side tptrs)
static int max_group(const RoundArrays& r)
{
    int mx = 0;
    for (int t = 0; t < r.delta; ++t)
        for (const int* p : r.tptr) mx = std::max(mx, p[t + 1] - p[t]);
    return mx;
}

static void set_pids(PartRoundArgs& c, const RoundArrays& r)
{
    c.del_pids = r.dev[RA_DEL_PIDS]; c.rep_pids = r.dev[RA_REP_PIDS];
}
template <typename RoundArgs> static void set_pids(RoundArgs&, const RoundArrays&) {}

// Fills a whole-round kernel's args (CoopRoundArgs, LinRoundArgs and
// PartRoundArgs share their field names) from the plan's base args and the
// round's arrays. The four tick pointers must be device-resident here.
template <typename RoundArgs, typename Args>
static RoundArgs round_args(const Args& base, const RoundArrays& r)
{
    RoundArgs c;
    c.base = base;
    c.snap_nodes = r.dev[RA_SNAP_NODES]; c.snap_slots = r.dev[RA_SNAP_SLOTS];
    c.snap_tptr = r.tptr[RT_SNAP];
    c.recv_nodes = r.dev[RA_RECV_NODES]; c.recv_nptr = r.dev[RA_RECV_NPTR];
    c.recv_tptr = r.tptr[RT_RECV];
    c.del_slots = r.dev[RA_DEL_SLOTS]; c.reply_slots = r.dev[RA_REPLY_SLOTS];
    c.pull_nodes = r.dev[RA_PULL_NODES]; c.pull_slots = r.dev[RA_PULL_SLOTS];
    c.pull_tptr = r.tptr[RT_PULL];
    c.rep_nodes = r.dev[RA_REP_NODES]; c.rep_nptr = r.dev[RA_REP_NPTR];
    c.rep_tptr = r.tptr[RT_REP];
    c.rep_slots = r.dev[RA_REP_SLOTS];
    set_pids(c, r);
    c.delta = r.delta;
    return c;
}

// Single-workgroup fallback for tiny batches: the family's whole-round
// kernel launched PLAIN with one workgroup (in the coop kernel round_sync
// degrades to __syncthreads) — one launch for the round. `tptr` are the
// host tensors behind r.tptr; the kernel reads copies of them on `dev`.
// Returns false, having done nothing, when the round does not qualify.
template <typename RoundArgs, typename Args>
static bool single_block_round(void (*kernel)(RoundArgs), const Plan<Args>& L,
                               const RoundArrays& r, const TptrTensors& tptr,
                               torch::Device dev)
{
    if (!(max_group(r) <= sb_threshold() &&
          r.dev[RA_REP_REPLY_SLOTS] == nullptr))
        return false;
    TptrTensors t;
    RoundArrays on_dev = r;
    for (int i = 0; i < ROUND_N_TPTRS; ++i) {
        t[i] = tptr[i].to(dev);
        on_dev.tptr[i] = t[i].data_ptr<int>();
    }
    RoundArgs c = round_args<RoundArgs>(L.a, on_dev);
    launch_kernel(kernel, 1, L.threads, L.smem, current_stream(), c);
    // keep the uploaded tptr tensors alive past the async launch
    static thread_local std::vector<torch::Tensor> keep;
    keep.insert(keep.end(), t.begin(), t.end());
    if (keep.size() > 64) keep.erase(keep.begin(), keep.begin() + 32);
    return true;
}

// What a run_round_* body works on: round_entry (below) makes it from the
// leading parameters every run_round_* op takes,
//   params, ages, slots, slot_ages,
//   round_buf  int32 [*] on the device: the arrays in table order
//   lens       their ROUND_N_ARRAYS lengths
//   snap_tptr, recv_tptr, pull_tptr, rep_tptr  int32 [n_groups + 1]
//   X, Y, counts
// and the family's own arguments follow.
struct RoundCall {
    StateTensors st;
    RoundArrays r;
    TptrTensors tptr;  // the tensors behind r.tptr
};

// Binds `body` as a run_round_* op. The round is validated before any
// pointer is formed; a bad one raises and launches nothing. The tick
// pointers are read on the host by the stream executors and on the device by
// the cooperative kernel, so `tptr_on_dev` says where they must live.
template <typename... Family>
static auto round_entry(void (*body)(const RoundCall&, Family...),
                        bool tptr_on_dev = false)
{
    return [body, tptr_on_dev](
               torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
               torch::Tensor slot_ages, torch::Tensor round_buf,
               std::vector<int64_t> lens, torch::Tensor snap_tptr,
               torch::Tensor recv_tptr, torch::Tensor pull_tptr,
               torch::Tensor rep_tptr, torch::Tensor X, torch::Tensor Y,
               torch::Tensor counts, Family... family) {
        TORCH_CHECK(round_buf.is_cuda() && round_buf.is_contiguous() &&
                        round_buf.scalar_type() == torch::kInt32 &&
                        round_buf.dim() == 1,
                    "round_buf must be contiguous int32 [*] on device");
        TORCH_CHECK(lens.size() == (size_t)ROUND_N_ARRAYS, "lens must have ",
                    (int)ROUND_N_ARRAYS, " entries, got ", lens.size());
        size_t off[ROUND_N_ARRAYS], len[ROUND_N_ARRAYS], total = 0;
        const size_t room = (size_t)round_buf.numel();
        for (int i = 0; i < ROUND_N_ARRAYS; ++i) {
            // each length against the room left: the sum cannot wrap
            TORCH_CHECK(lens[i] >= 0 && (size_t)lens[i] <= room - total,
                        "lens[", i, "] (", ROUND_ARRAY_NAMES[i], ") = ",
                        lens[i], " is negative or runs past round_buf");
            off[i] = total;
            len[i] = (size_t)lens[i];
            total += len[i];
        }
        RoundCall c{{params, ages, slots, slot_ages, X, Y, counts},
                    {},
                    {snap_tptr, recv_tptr, pull_tptr, rep_tptr}};
        const int* tp[ROUND_N_TPTRS];
        for (int i = 0; i < ROUND_N_TPTRS; ++i) {
            const torch::Tensor& t = c.tptr[i];
            TORCH_CHECK(t.is_cuda() == tptr_on_dev && t.is_contiguous() &&
                            t.scalar_type() == torch::kInt32 &&
                            t.numel() >= 1 &&
                            t.numel() == c.tptr[0].numel(),
                        ROUND_TPTR_NAMES[i], " must be contiguous int32 on ",
                        tptr_on_dev ? "device" : "host",
                        ", non-empty and as long as ", ROUND_TPTR_NAMES[0]);
            tp[i] = t.data_ptr<int>();
        }
        c.r = round_arrays(round_buf.data_ptr<int>(), off, len, tp,
                           (size_t)snap_tptr.numel());
        body(c, family...);
    };
}

static void run_round_logreg(
    const RoundCall& c, int64_t d, int64_t k, double lr, double wd,
    int64_t epochs, int64_t bs, int64_t mode, int64_t merge_limit)
{
    auto L = logreg_plan(c.st, d, k, lr, wd, epochs, bs, mode, merge_limit);
    // the single-workgroup round kernel has no limited-merge instantiation
    if (merge_limit < 0 &&
        single_block_round(big_batch(bs, L.a.Smax)
                               ? coop_round_logreg_kernel<true>
                               : coop_round_logreg_kernel<false>,
                           L, c.r, c.tptr, c.st.params.device()))
        return;
    stream_round(L, c.r);
}

static void run_round_linear(const RoundCall& c, int64_t d, double lrlam,
                             int64_t is_pegasos, int64_t mode)
{
    auto L = linear_plan(c.st, d, lrlam, is_pegasos, mode);
    if (single_block_round(sb_round_linear_kernel, L, c.r, c.tptr,
                           c.st.params.device()))
        return;
    stream_round(L, c.r);
}

static void run_round_logreg_part(
    const RoundCall& c, torch::Tensor perm, torch::Tensor pptr,
    torch::Tensor apart, int64_t n_parts, int64_t d, int64_t k, double lr,
    double wd, int64_t epochs, int64_t bs, int64_t mode)
{
    auto L = logreg_part_plan(c.st, perm, pptr, apart, n_parts, d, k, lr, wd,
                              epochs, bs, mode);
    if (single_block_round(sb_round_logreg_part_kernel, L, c.r, c.tptr,
                           c.st.params.device()))
        return;
    stream_round(L, c.r, &LogregPartArgs::dpids);
}

static void run_round_logreg_samp(
    const RoundCall& c, int64_t samp_c, int64_t d, int64_t k, double lr,
    double wd, int64_t epochs, int64_t bs, int64_t mode)
{
    auto L = logreg_samp_plan(c.st, samp_c, d, k, lr, wd, epochs, bs, mode);
    stream_round(L, c.r, &LogregSampArgs::dseeds);
}

static void run_round_mlp(
    const RoundCall& c, torch::Tensor layout, int64_t n_layers, double lr,
    double wd, int64_t epochs, int64_t bs, int64_t mode, int64_t merge_limit)
{
    auto L = mlp_plan(c.st, layout, n_layers, lr, wd, epochs, bs, mode,
                      merge_limit);
    // receivers are unique within a launch (the wide kernel's workspace has
    // one row per node)
    for (int t = 0; t < c.r.delta; ++t)
        for (const int* p : {c.r.tptr[RT_RECV], c.r.tptr[RT_REP]})
            TORCH_CHECK(p[t + 1] - p[t] <= c.st.params.size(0),
                        "run_round_mlp: a launch of ", p[t + 1] - p[t],
                        " receivers for ", c.st.params.size(0), " nodes");
    stream_round(L, c.r);
}

static void run_round_mlp_part(
    const RoundCall& c, torch::Tensor layout, int64_t n_layers,
    torch::Tensor perm, torch::Tensor pptr, torch::Tensor apart,
    int64_t n_parts, double lr, double wd, int64_t epochs, int64_t bs,
    int64_t mode)
{
    auto L = mlp_comp_plan(true, c.st, layout, n_layers, perm, pptr, apart,
                           n_parts, 0, lr, wd, epochs, bs, mode);
    stream_round(L, c.r, &MlpCompArgs::dpids);
}

static void run_round_mlp_samp(
    const RoundCall& c, torch::Tensor layout, int64_t n_layers,
    int64_t samp_c, double lr, double wd, int64_t epochs, int64_t bs,
    int64_t mode)
{
    auto L = mlp_comp_plan(false, c.st, layout, n_layers, {}, {}, {}, 0,
                           samp_c, lr, wd, epochs, bs, mode);
    stream_round(L, c.r, &MlpCompArgs::dpids);
}

static void run_round_mf(const RoundCall& c, int64_t k, int64_t n_items,
                         double reg, double lr)
{
    auto L = mf_plan(c.st, k, n_items, reg, lr);
    stream_round(L, c.r);
}

// NOTE: unlike the stream executors, ALL arrays (tick ptrs included) are
// device-resident here (bound with tptr_on_dev).
static void run_round_coop_logreg(
    const RoundCall& rc, int64_t d, int64_t k, double lr, double wd,
    int64_t epochs, int64_t bs, int64_t mode, int64_t max_batch)
{
    auto L = logreg_plan(rc.st, d, k, lr, wd, epochs, bs, mode);
    CoopRoundArgs c = round_args<CoopRoundArgs>(L.a, rc.r);
    const void* kernel = big_batch(bs, L.a.Smax)
        ? (const void*)coop_round_logreg_kernel<true>
        : (const void*)coop_round_logreg_kernel<false>;
    int grid = std::max<int>(1, (int)max_batch);
    // stay within guaranteed cooperative residency
    int max_blocks = 0;
    hipError_t oerr = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &max_blocks, kernel, L.threads, L.smem);
    TORCH_CHECK(oerr == hipSuccess, "occupancy query failed");
    hipDeviceProp_t prop;
    (void)hipGetDeviceProperties(&prop, 0);
    int limit = max_blocks * prop.multiProcessorCount;
    TORCH_CHECK(limit > 0, "cooperative launch not supported");
    if (grid > limit) grid = limit;
    void* kargs[] = {&c};
    hipError_t err = hipLaunchCooperativeKernel(
        kernel, dim3(grid), dim3(L.threads),
        kargs, L.smem, current_stream());
    TORCH_CHECK(err == hipSuccess, "cooperative launch failed: ",
                hipGetErrorString(err));
}

// ---------------------------------------------------------------------------
// PENS and the evaluation kernels
// ---------------------------------------------------------------------------

void tick_pens(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
               torch::Tensor slot_ages, torch::Tensor nodes, torch::Tensor ptr,
               torch::Tensor cslots, torch::Tensor cowners,
               torch::Tensor counts, torch::Tensor X, torch::Tensor Y,
               torch::Tensor dcounts, int64_t d, int64_t k, int64_t m_top,
               double lr, double wd, int64_t epochs, int64_t bs)
{
    CHECK_DEV(params); CHECK_DEV(slots); CHECK_DEV(X); CHECK_DEV(counts);
    TORCH_CHECK(k <= KMAX, "n_classes > ", KMAX, " unsupported");
    int n = nodes.size(0);
    if (n == 0) return;
    PensArgs a;
    a.params = params.data_ptr<float>(); a.ages = ages.data_ptr<int>();
    a.slots = slots.data_ptr<float>(); a.slot_ages = slot_ages.data_ptr<int>();
    a.nodes = nodes.data_ptr<int>(); a.ptr = ptr.data_ptr<int>();
    a.cslots = cslots.data_ptr<int>(); a.cowners = cowners.data_ptr<int>();
    a.counts = counts.data_ptr<int>();
    a.X = X.data_ptr<float>(); a.Y = Y.data_ptr<float>();
    a.dcounts = dcounts.data_ptr<int>();
    a.d = d; a.k = k; a.Smax = X.size(1); a.D = params.size(1);
    a.m_top = m_top; a.n_total = counts.size(1);
    a.lr = lr; a.wd = wd; a.epochs = epochs; a.bs = bs;
    int bsmax = (bs == 0) ? a.Smax : std::min<int>(bs, a.Smax);
    size_t smem = sizeof(float) * (a.D + (size_t)bsmax * a.d +
                                   (size_t)bsmax * a.k);
    TORCH_CHECK(smem <= 160 * 1024, "pens LDS budget exceeded: ", smem);
    hipLaunchKernelGGL(big_batch(bs, a.Smax) ? tick_pens_kernel<true>
                                             : tick_pens_kernel<false>,
                       dim3(n), dim3(LOGREG_THREADS), smem, current_stream(),
                       a);
}

void tick_pens_mlp(torch::Tensor params, torch::Tensor ages,
                   torch::Tensor slots, torch::Tensor slot_ages,
                   torch::Tensor nodes, torch::Tensor ptr,
                   torch::Tensor cslots, torch::Tensor cowners,
                   torch::Tensor counts, torch::Tensor X, torch::Tensor Y,
                   torch::Tensor dcounts, torch::Tensor layout,
                   int64_t n_layers, int64_t m_top, double lr, double wd,
                   int64_t epochs, int64_t bs)
{
    CHECK_DEV(counts);
    int n = nodes.size(0);
    if (n == 0) return;
    CHECK_DEV(nodes); CHECK_DEV(ptr); CHECK_DEV(cslots); CHECK_DEV(cowners);
    PensMlpArgs p{};
    MlpGeom g = mlp_fill(p.m, {params, ages, slots, slot_ages, X, Y, dcounts},
                         layout, n_layers, lr, wd, epochs, bs,
                         MODE_MERGE_UPDATE);
    p.m.nodes = nodes.data_ptr<int>(); p.m.ptr = ptr.data_ptr<int>();
    p.cslots = cslots.data_ptr<int>(); p.cowners = cowners.data_ptr<int>();
    p.wins = counts.data_ptr<int>();
    p.m_top = m_top; p.n_total = counts.size(1);
    // LDS: ONE model slab + activations + 2 grad buffers, next to the
    // kernel's static correct[] / sel[]
    size_t smem = sizeof(float) * ((size_t)p.m.D + g.scratch);
    TORCH_CHECK(smem + 2 * sizeof(int) * PENS_MAX_CAND <= 160 * 1024,
        "pens mlp LDS budget exceeded (", smem,
        " B of dynamic LDS); shrink batch_size/hidden. The global-resident"
        " wide kernel covers the plain MLP tick only");
    launch_kernel(tick_pens_mlp_kernel, n, g.threads, smem, current_stream(),
                  p);
}

// Scoring-mode launch geometry from a.D, a.d and a.n_eval: sets a.tile and
// returns the dynamic LDS.
// LDS: model + scores + their label-compacted copy + binarized labels
// + confusion + one X tile.
// The tile size adapts so everything fits the 160 KB budget.
static size_t eval_tile_smem(EvalArgs& a)
{
    int n_eval = a.n_eval, d = a.d;
    size_t fixed = sizeof(float) * (a.D + 2 * (size_t)n_eval)
        + ((n_eval + 15) & ~15) * sizeof(char)
        + sizeof(int) * EVAL_KMAX * EVAL_KMAX;
    long room = (long)(160 * 1024 - fixed) / (long)(sizeof(float) * d);
    TORCH_CHECK(room >= 16, "eval LDS budget exceeded (n_eval=", n_eval,
                ", d=", d, ")");
    a.tile = (int)std::min<long>({room, (long)n_eval, 512});
    return fixed + sizeof(float) * (size_t)a.tile * d;
}

torch::Tensor eval_metrics(torch::Tensor params, torch::Tensor nodes,
                           torch::Tensor X, torch::Tensor Y, int64_t d,
                           int64_t k, bool is_margin,
                           torch::Tensor eval_counts)
{
    CHECK_DEV(params); CHECK_DEV(nodes); CHECK_DEV(X); CHECK_DEV(Y);
    TORCH_CHECK(k <= EVAL_KMAX, "n_classes > ", EVAL_KMAX, " unsupported");
    int R = nodes.size(0);
    bool per_node = eval_counts.defined() && eval_counts.numel();
    int n_eval = per_node ? (int)X.size(1) : (int)X.size(0);
    auto out = torch::empty({R, 5}, params.options());
    if (R == 0) return out;
    EvalArgs a;
    a.params = params.data_ptr<float>();
    a.nodes = nodes.data_ptr<int>();
    a.X = X.data_ptr<float>();
    a.Y = Y.data_ptr<float>();
    a.out = out.data_ptr<float>();
    a.d = d; a.k = k; a.n_eval = n_eval; a.D = params.size(1);
    a.is_margin = is_margin;
    a.scores = nullptr;
    a.eval_counts = per_node ? eval_counts.data_ptr<int>() : nullptr;
    size_t smem = eval_tile_smem(a);
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(R), dim3(256), smem,
                       current_stream(), a);
    return out;
}

torch::Tensor eval_metrics_scores(torch::Tensor scores, torch::Tensor Y,
                                  int64_t k, bool is_margin)
{
    // K13 on PRECOMPUTED raw scores [R, n_eval, k] ([R, n_eval] margin):
    // families whose forward runs elsewhere (MLP / torchmod) get the same
    // one-launch confusion + macro-PRF + pairwise-AUC epilogue instead of
    // ~40 small torch kernels and a host sync.
    CHECK_DEV(scores); CHECK_DEV(Y);
    TORCH_CHECK(k <= EVAL_KMAX, "n_classes > ", EVAL_KMAX, " unsupported");
    int R = scores.size(0);
    int n_eval = scores.size(1);
    auto out = torch::empty({R, 5}, scores.options());
    if (R == 0) return out;
    EvalArgs a;
    a.params = nullptr; a.nodes = nullptr; a.X = nullptr;
    a.Y = Y.data_ptr<float>();
    a.out = out.data_ptr<float>();
    a.d = 0; a.k = k; a.n_eval = n_eval; a.D = 0;
    a.is_margin = is_margin;
    a.tile = 1;
    a.eval_counts = nullptr;
    a.scores = scores.data_ptr<float>();
    size_t smem = sizeof(float) * 2 * (size_t)n_eval
        + ((n_eval + 15) & ~15) * sizeof(char)
        + sizeof(int) * EVAL_KMAX * EVAL_KMAX;
    TORCH_CHECK(smem <= 160 * 1024, "eval LDS budget exceeded: ", smem);
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(R), dim3(256), smem,
                       current_stream(), a);
    return out;
}

// eval_mlp_kernel's LDS next to the forward scratch: model + scores + their
// label-compacted copy + binarized labels + confusion, and the epilogue's
// three static words (rounded up to 16 B).
static size_t eval_mlp_fixed_smem(int64_t D, int64_t n_eval)
{
    return sizeof(float) * ((size_t)D + 2 * (size_t)n_eval)
        + (((size_t)n_eval + 15) & ~(size_t)15) * sizeof(char)
        + sizeof(int) * EVAL_KMAX * EVAL_KMAX + 16;
}

// Rows eval_mlp_kernel forwards per chunk: the most that fit the 160 KB LDS
// budget, at most n_eval and 512. 0 = the shape does not fit: fewer than 16
// rows of scratch, or n_eval > 2048 (the pairwise AUC is O(n_eval^2) per
// block and its pair count assumes n_eval <= 2048).
static int64_t eval_mlp_tile(int64_t D, int64_t d_in, int64_t act_total,
                             int64_t n_eval)
{
    if (D < 1 || d_in < 1 || act_total < 1 || n_eval < 1 || n_eval > 2048)
        return 0;
    int64_t left = 160 * 1024 - (int64_t)eval_mlp_fixed_smem(D, n_eval);
    int64_t room = left / (int64_t)(sizeof(float) * (d_in + act_total));
    if (left <= 0 || room < 16) return 0;
    return std::min<int64_t>({room, n_eval, 512});
}

torch::Tensor eval_mlp(torch::Tensor params, torch::Tensor nodes,
                       torch::Tensor X, torch::Tensor Y, torch::Tensor layout,
                       int64_t n_layers, torch::Tensor eval_counts)
{
    CHECK_DEV(params); CHECK_DEV(nodes); CHECK_DEV(X); CHECK_DEV(Y);
    CHECK_DEV(layout);
    TORCH_CHECK(params.scalar_type() == torch::kFloat32 &&
                    X.scalar_type() == torch::kFloat32 &&
                    Y.scalar_type() == torch::kFloat32,
                "params, X and Y must be float32");
    TORCH_CHECK(nodes.scalar_type() == torch::kInt32 &&
                    layout.scalar_type() == torch::kInt32,
                "nodes and layout must be int32");
    TORCH_CHECK(params.dim() == 2, "params must be [n_local, D]");
    TORCH_CHECK(n_layers >= 1 && layout.numel() == 4 * n_layers,
                "mlp layout must hold n_layers x (w_off, b_off, in, out)");
    bool per_node = eval_counts.defined() && eval_counts.numel();
    int64_t D = params.size(1);
    auto lay = layout.cpu();
    const int* Lh = lay.data_ptr<int>();
    int64_t d_in = Lh[2], act_total = 0;
    for (int l = 0; l < n_layers; ++l) {
        int64_t w_off = Lh[4 * l], b_off = Lh[4 * l + 1];
        int64_t fin = Lh[4 * l + 2], fout = Lh[4 * l + 3];
        TORCH_CHECK(fin >= 1 && fout >= 1 && w_off >= 0 && b_off >= 0 &&
                        w_off + fin * fout <= D && b_off + fout <= D &&
                        fin == (l ? Lh[4 * l - 1] : d_in),
                    "mlp layout does not fit a params row of ", D);
        act_total += fout;
    }
    int64_t k = Lh[4 * (n_layers - 1) + 3];
    TORCH_CHECK(k <= EVAL_KMAX, "n_classes > ", EVAL_KMAX, " unsupported");
    int64_t n_eval;
    if (per_node) {
        CHECK_DEV(eval_counts);
        TORCH_CHECK(eval_counts.scalar_type() == torch::kInt32,
                    "eval_counts must be int32");
        TORCH_CHECK(X.dim() == 3 && X.size(2) == d_in && Y.dim() == 2 &&
                        Y.size(0) == X.size(0) && Y.size(1) == X.size(1) &&
                        eval_counts.numel() == X.size(0),
                    "per-node mode: X [n_local, S, d_in], Y [n_local, S],"
                    " eval_counts [n_local]");
        n_eval = X.size(1);
    } else {
        TORCH_CHECK(X.dim() == 2 && X.size(1) == d_in &&
                        Y.numel() == X.size(0),
                    "shared-set mode: X [n, d_in], Y [n]");
        n_eval = X.size(0);
    }
    int R = nodes.size(0);
    auto out = torch::empty({R, 5}, params.options());
    if (R == 0) return out;
    int64_t tile = eval_mlp_tile(D, d_in, act_total, n_eval);
    TORCH_CHECK(tile > 0, "eval_mlp: shape does not fit (D=", D, ", d_in=",
                d_in, ", act_total=", act_total, ", n_eval=", n_eval, ")");
    EvalMlpArgs p{};
    p.m.params = params.data_ptr<float>();
    p.m.nodes = nodes.data_ptr<int>();
    p.m.X = X.data_ptr<float>();
    p.m.Y = Y.data_ptr<float>();
    p.m.layout = layout.data_ptr<int>();
    p.m.n_layers = n_layers; p.m.D = D; p.m.d_in = d_in;
    p.out = out.data_ptr<float>();
    p.eval_counts = per_node ? eval_counts.data_ptr<int>() : nullptr;
    p.n_eval = n_eval; p.tile = tile;
    // the +16 of the fixed part stands for the epilogue's static words
    size_t smem = eval_mlp_fixed_smem(D, n_eval) - 16 +
                  sizeof(float) * (size_t)tile * (d_in + act_total);
    launch_kernel(eval_mlp_kernel, R, 256, smem, current_stream(), p);
    return out;
}

// ---------------------------------------------------------------------------
// RoundDriver: one native call per round. It takes the round from the
// scheduler's RoundSource (csrc/round_source.h), writes the upload layout
// (csrc/round_layout.h) into pinned memory, issues the one H2D copy, runs
// stream_round over pointers into the device copy, and launches the round's
// evaluation with its node ids read from the same upload. Nothing of the
// schedule becomes a Python object.
//
// Ownership: the driver owns a ring of RD_RING upload slots (pinned host
// buffer + device buffer + event) and two metric stages (pinned host
// staging + event, and with eval_overlap a device buffer of gathered params
// rows + the gather's event). A slot's event is recorded after the last
// work of its round that reads the slot; the slot is rewritten, grown or
// freed only after that event completed. At most two evaluations are in
// flight and the older one is collected, which waits for its event, before
// a third is launched: that frees a stage, staging and gathered rows alike,
// before it is reused. A held round has launched nothing, so the rule holds
// across its retry; a failed step drains both side streams. The state, pool
// and eval tensors are held by reference; the pool is replaced through
// set_pool() when it grows.
//
// Two measured options, both on by default (profiles/round_driver.md):
// mapped_metrics: the eval kernel writes its [R, 5] rows straight into the
//   device-mapped staging buffer, so no D2H copy is dispatched (off: the
//   rows go to a device buffer the driver owns and are copied out);
// side_upload: the H2D copy runs on a stream of the driver's own and the
//   compute stream waits for its event, which takes the copy off the
//   kernels' chain.
// One more, off by default: it gained 2 % on the flagship line, inside that
// line's spread (profiles/round_chain.md):
// eval_overlap: a sampled evaluation's rows are gathered on the compute
//   stream by the snapshot kernel and the eval kernel runs on a third
//   stream over that copy, beside the next round's first launches (off, or
//   with no sampled ids: the eval kernel runs in the compute stream and
//   reads params).
// ---------------------------------------------------------------------------

#define RD_CHECK(expr)                                                     \
    do {                                                                   \
        hipError_t rd_err_ = (expr);                                       \
        if (rd_err_ != hipSuccess)                                         \
            throw std::runtime_error(std::string(#expr " failed: ") +      \
                                     hipGetErrorString(rd_err_));          \
    } while (0)

constexpr int RD_RING = 4;

// What the drivers of this process hold right now: pinned host buffers,
// device buffers, events, streams. Counted where each is created and
// destroyed, so a test can see that a destroyed driver released everything.
static std::atomic<int64_t> rd_live[4];
enum { RD_HOST = 0, RD_DEV, RD_EVENT, RD_STREAM };

static void rd_host_alloc(void** p, size_t bytes, unsigned flags)
{
    RD_CHECK(hipHostMalloc(p, bytes, flags));
    ++rd_live[RD_HOST];
}
static hipError_t rd_host_free(void* p)
{
    --rd_live[RD_HOST];
    return hipHostFree(p);
}
static void rd_dev_alloc(void** p, size_t bytes)
{
    RD_CHECK(hipMalloc(p, bytes));
    ++rd_live[RD_DEV];
}
static hipError_t rd_dev_free(void* p)
{
    --rd_live[RD_DEV];
    return hipFree(p);
}
static void rd_event_create(hipEvent_t* e)
{
    RD_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    ++rd_live[RD_EVENT];
}
static void rd_event_destroy(hipEvent_t e)
{
    --rd_live[RD_EVENT];
    (void)hipEventDestroy(e);
}

static py::tuple round_driver_live()
{
    return py::make_tuple(rd_live[RD_HOST].load(), rd_live[RD_DEV].load(),
                          rd_live[RD_EVENT].load(), rd_live[RD_STREAM].load());
}

class RoundDriver {
public:
    RoundDriver(torch::Tensor params, torch::Tensor ages, torch::Tensor slots,
                torch::Tensor slot_ages, torch::Tensor X, torch::Tensor Y,
                torch::Tensor counts, torch::Tensor gx, torch::Tensor gy,
                const std::string& family, py::tuple plan, py::capsule source,
                bool eval_all, bool mapped_metrics, bool side_upload,
                bool eval_overlap)
        : st_{params, ages, slots, slot_ages, X, Y, counts}, gx_(gx), gy_(gy),
          source_cap_(source), eval_all_(eval_all), mapped_(mapped_metrics),
          side_upload_(side_upload), eval_overlap_(eval_overlap)
    {
        TORCH_CHECK(std::string(source.name() ? source.name() : "") ==
                        "gossipy_amd.RoundSource",
                    "source must be NativeScheduler.round_source()");
        src_ = *static_cast<const RoundSource*>(source.get_pointer());
        CHECK_DEV(gx); CHECK_DEV(gy);
        if (family == "logreg") {
            TORCH_CHECK(plan.size() == 8,
                        "logreg plan: (d, k, lr, wd, epochs, bs, mode,"
                        " merge_limit)");
            lg_ = logreg_plan(
                st_, plan[0].cast<int64_t>(), plan[1].cast<int64_t>(),
                plan[2].cast<double>(), plan[3].cast<double>(),
                plan[4].cast<int64_t>(), plan[5].cast<int64_t>(),
                plan[6].cast<int64_t>(), plan[7].cast<int64_t>());
            ev_.d = lg_.a.d; ev_.k = lg_.a.k; ev_.is_margin = 0;
        } else if (family == "linear") {
            TORCH_CHECK(plan.size() == 4,
                        "linear plan: (d, lrlam, is_pegasos, mode)");
            linear_ = true;
            ln_ = linear_plan(st_, plan[0].cast<int64_t>(),
                              plan[1].cast<double>(), plan[2].cast<int64_t>(),
                              plan[3].cast<int64_t>());
            ev_.d = ln_.a.d; ev_.k = 1; ev_.is_margin = 1;
        } else {
            TORCH_CHECK(false, "RoundDriver: unsupported family ", family);
        }
        TORCH_CHECK(ev_.k <= EVAL_KMAX, "n_classes > ", EVAL_KMAX,
                    " unsupported");
        TORCH_CHECK(gx.dim() == 2 && gx.size(1) == ev_.d &&
                        gx.scalar_type() == torch::kFloat32,
                    "gx must be float32 [n_eval, d]");
        TORCH_CHECK(gy.dim() == 1 && gy.size(0) == gx.size(0) &&
                        gy.scalar_type() == torch::kFloat32,
                    "gy must be float32 [n_eval]");
        const SnapGeom& g = snap_geom();
        TORCH_CHECK(params.dim() == 2 && params.size(1) == g.Dp &&
                        params.scalar_type() == torch::kFloat32,
                    "params must be float32 [n, ", g.Dp, "]");
        TORCH_CHECK(ages.is_cuda() && ages.is_contiguous() &&
                        ages.scalar_type() == torch::kInt32 &&
                        ages.dim() == 1 && ages.size(0) == params.size(0),
                    "ages must be int32 [n] on device");
        check_pool(slots, slot_ages);
        ev_.params = params.data_ptr<float>();
        ev_.X = gx.data_ptr<float>();
        ev_.Y = gy.data_ptr<float>();
        ev_.n_eval = (int)gx.size(0);
        ev_.D = (int)params.size(1);
        ev_.scores = nullptr;
        ev_.eval_counts = nullptr;
        ev_smem_ = eval_tile_smem(ev_);
        n_local_ = params.size(0);
        pool_cap_ = slots.size(0);
        try {
            for (auto& s : ring_)
                rd_event_create(&s.ev);
            for (auto& m : stage_)
                rd_event_create(&m.ev);
            if (side_upload_) {
                RD_CHECK(hipStreamCreateWithFlags(&up_stream_,
                                                  hipStreamNonBlocking));
                ++rd_live[RD_STREAM];
                rd_event_create(&up_ev_);
            }
            if (eval_overlap_) {
                RD_CHECK(hipStreamCreateWithFlags(&ev_stream_,
                                                  hipStreamNonBlocking));
                ++rd_live[RD_STREAM];
                for (auto& m : stage_)
                    rd_event_create(&m.gev);
            }
        } catch (...) {
            release();
            throw;
        }
    }

    RoundDriver(const RoundDriver&) = delete;
    RoundDriver& operator=(const RoundDriver&) = delete;

    ~RoundDriver() { release(); }

    // The pool was replaced (SlotPool.ensure grew it).
    void set_pool(torch::Tensor slots, torch::Tensor slot_ages)
    {
        check_pool(slots, slot_ages);
        st_.slots = slots; st_.slot_ages = slot_ages;
        auto set = [&](auto& a) {
            a.slots = slots.data_ptr<float>();
            a.slot_ages = slot_ages.data_ptr<int>();
        };
        if (linear_) set(ln_.a); else set(lg_.a);
        pool_cap_ = slots.size(0);
    }

    // Runs round r. Returns (sent, failed, total_size, n_slots, n_eval_rows).
    // n_eval_rows == -1: the round needs n_slots pool slots and the pool is
    // smaller; nothing was enqueued and the round is held. Grow the pool,
    // call set_pool() and call step(r) again.
    py::tuple step(int64_t r)
    {
        int64_t rows = 0;
        {
            py::gil_scoped_release nogil;
            if (failed_)
                throw std::runtime_error(
                    "RoundDriver: an earlier step failed; nothing more is "
                    "enqueued");
            if (!(held_ && held_r_ == r)) {
                if (held_)
                    throw std::runtime_error(
                        "RoundDriver: round " + std::to_string(held_r_) +
                        " is held, got step(" + std::to_string(r) + ")");
                char err[256] = {0};
                auto t0 = std::chrono::steady_clock::now();
                if (src_.take(src_.self, r, &view_, err, sizeof(err)))
                    throw std::invalid_argument(err);
                take_s_ += seconds_since(t0);
                held_ = true;
                held_r_ = r;
            }
            if (view_.n_slots > pool_cap_) {
                rows = -1;
            } else {
                auto t0 = std::chrono::steady_clock::now();
                try {
                    rows = run_held();
                } catch (...) {
                    failed_ = true;
                    throw;
                }
                enqueue_s_ += seconds_since(t0);
                ++rounds_;
                held_ = false;
            }
        }
        return py::make_tuple(view_.sent, view_.failed, view_.total_size,
                              view_.n_slots, rows);
    }

    // The launch groups of the last round run (a perf-probe counter).
    int64_t last_groups() const { return last_groups_; }

    // Where step() spent its time so far, for the perf probes: seconds
    // waiting in the source's take(), seconds writing the layout and
    // enqueueing (waits for a busy ring slot or a due evaluation included),
    // and the rounds run.
    py::tuple stats() const
    {
        return py::make_tuple(take_s_, enqueue_s_, rounds_);
    }

    // Completed evaluations as (round, float32[R, 5]), oldest first. The
    // rule of the runner's _drain_eval: without `force` only what has
    // already arrived is collected, except that two in flight make the
    // older one due.
    py::list poll_eval(bool force)
    {
        {
            py::gil_scoped_release nogil;
            while (!pending_.empty()) {
                Stage& m = stage_[pending_.front()];
                if (!force && pending_.size() < 2) {
                    hipError_t q = hipEventQuery(m.ev);
                    if (q == hipErrorNotReady) break;
                    RD_CHECK(q);
                }
                collect_oldest();
            }
        }
        py::list out;
        for (auto& d : done_) {
            auto a = py::array_t<float>({(py::ssize_t)d.rows, (py::ssize_t)5});
            std::copy(d.vals.begin(), d.vals.end(), a.mutable_data());
            out.append(py::make_tuple(d.round, a));
        }
        done_.clear();
        return out;
    }

    py::list drain() { return poll_eval(true); }

private:
    struct Slot {
        int32_t* h = nullptr;
        int32_t* d = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
    };
    struct Stage {
        float* h = nullptr;      // pinned; the kernel's target when mapped
        float* h_dev = nullptr;  // its device address
        size_t cap_rows = 0;
        hipEvent_t ev = nullptr;
        float* rows_d = nullptr;  // gathered params rows [rows_cap, D]
        size_t rows_cap = 0;
        hipEvent_t gev = nullptr;  // the gather into rows_d is done
        int64_t round = 0;
        int64_t rows = 0;
    };
    struct Done {
        int64_t round, rows;
        std::vector<float> vals;
    };

    const SnapGeom& snap_geom() const { return linear_ ? ln_.snap : lg_.snap; }

    // A pool the plan's kernels can write: rows as wide as a snapshot, one
    // int32 age per slot. The snapshot kernel writes snap.W floats per slot
    // row, so any other width would run past the pool's end.
    void check_pool(const torch::Tensor& slots,
                    const torch::Tensor& slot_ages) const
    {
        const SnapGeom& g = snap_geom();
        TORCH_CHECK(slots.is_cuda() && slots.is_contiguous() &&
                        slots.scalar_type() == torch::kFloat32 &&
                        slots.dim() == 2 && slots.size(1) == g.W,
                    "pool slots must be contiguous float32 [capacity, ", g.W,
                    "] on device");
        TORCH_CHECK(g.age_w == 1 && slot_ages.is_cuda() &&
                        slot_ages.is_contiguous() &&
                        slot_ages.scalar_type() == torch::kInt32 &&
                        slot_ages.dim() == 1 &&
                        slot_ages.size(0) == slots.size(0),
                    "pool slot_ages must be contiguous int32 [capacity] on "
                    "device");
    }

    static double seconds_since(std::chrono::steady_clock::time_point t0)
    {
        return std::chrono::duration<double>(
                   std::chrono::steady_clock::now() - t0).count();
    }

    void collect_oldest()
    {
        Stage& m = stage_[pending_.front()];
        RD_CHECK(hipEventSynchronize(m.ev));
        Done d{m.round, m.rows, {}};
        d.vals.assign(m.h, m.h + m.rows * 5);
        done_.push_back(std::move(d));
        pending_.pop_front();
    }

    void grow_slot(Slot& s, size_t need)
    {
        size_t cap = grown_capacity(s.cap, need);
        if (cap == s.cap) return;
        // the slot's event has completed: nothing reads the old buffers
        if (s.h) RD_CHECK(rd_host_free(s.h));
        s.h = nullptr; s.cap = 0;
        if (s.d) RD_CHECK(rd_dev_free(s.d));
        s.d = nullptr;
        rd_host_alloc((void**)&s.h, cap * sizeof(int32_t), hipHostMallocDefault);
        rd_dev_alloc((void**)&s.d, cap * sizeof(int32_t));
        s.cap = cap;
    }

    void grow_stage(Stage& m, size_t rows)
    {
        size_t cap = grown_capacity(m.cap_rows, rows);
        if (cap == m.cap_rows) return;
        if (m.h) RD_CHECK(rd_host_free(m.h));
        m.h = nullptr; m.cap_rows = 0;
        rd_host_alloc((void**)&m.h, cap * 5 * sizeof(float), hipHostMallocMapped);
        RD_CHECK(hipHostGetDevicePointer((void**)&m.h_dev, m.h, 0));
        m.cap_rows = cap;
    }

    // The stage's gathered-rows buffer and the identity index array for
    // `rows` rows. The stage is free (see the ownership comment), so nothing
    // reads its old buffer; the identity array may still be read by the
    // other stage's gather, which the compute stream is drained of first.
    void grow_gather(Stage& m, size_t rows, hipStream_t s)
    {
        size_t cap = grown_capacity(m.rows_cap, rows);
        if (cap != m.rows_cap) {
            if (m.rows_d) RD_CHECK(rd_dev_free(m.rows_d));
            m.rows_d = nullptr; m.rows_cap = 0;
            rd_dev_alloc((void**)&m.rows_d, cap * ev_.D * sizeof(float));
            m.rows_cap = cap;
        }
        if (cap > ident_cap_) {
            RD_CHECK(hipStreamSynchronize(s));
            if (ident_d_) RD_CHECK(rd_dev_free(ident_d_));
            ident_d_ = nullptr; ident_cap_ = 0;
            rd_dev_alloc((void**)&ident_d_, cap * sizeof(int));
            std::vector<int> iota(cap);
            for (size_t i = 0; i < cap; ++i) iota[i] = (int)i;
            RD_CHECK(hipMemcpy(ident_d_, iota.data(), cap * sizeof(int),
                               hipMemcpyHostToDevice));
            ident_cap_ = cap;
        }
    }

    // enqueue the held round; returns the rows its evaluation will have
    int64_t run_held()
    {
        hipStream_t s = current_stream();
        const RoundView& v = view_;
        // the old metrics go first: a third evaluation needs their staging
        int64_t n_ids_max = (int64_t)v.n_eval;
        bool will_eval = n_ids_max > 0 || eval_all_;
        if (will_eval && pending_.size() >= 2) collect_oldest();

        int si = slots_.acquire(
            [&](int i) {
                hipError_t q = hipEventQuery(ring_[i].ev);
                if (q != hipErrorNotReady) RD_CHECK(q);
                return q == hipSuccess;
            },
            [&](int i) { RD_CHECK(hipEventSynchronize(ring_[i].ev)); });
        Slot& sl = ring_[si];
        bool recorded = false;
        try {
            grow_slot(sl, round_layout_capacity(v));
            RoundLayout lay;
            if (!write_round_layout(v, 0, sl.h, sl.cap, &lay))
                throw std::runtime_error("RoundDriver: upload slot too small");
            // a schedule that fails this is never uploaded
            if (const char* what = round_bounds_error(v.tptr, lay, sl.h,
                                                      n_local_, pool_cap_))
                throw std::runtime_error(
                    std::string("RoundDriver: schedule out of bounds: ") +
                    what);
            if (side_upload_) {
                // the copy may not overtake the compute stream's reads of
                // this device buffer four rounds ago: the slot's event has
                // completed (acquire above), so nothing is left to wait for
                RD_CHECK(hipMemcpyAsync(sl.d, sl.h,
                                        lay.total * sizeof(int32_t),
                                        hipMemcpyHostToDevice, up_stream_));
                RD_CHECK(hipEventRecord(up_ev_, up_stream_));
                RD_CHECK(hipStreamWaitEvent(s, up_ev_, 0));
            } else {
                RD_CHECK(hipMemcpyAsync(sl.d, sl.h,
                                        lay.total * sizeof(int32_t),
                                        hipMemcpyHostToDevice, s));
            }

            const int* tp[ROUND_N_TPTRS];
            for (int i = 0; i < ROUND_N_TPTRS; ++i) tp[i] = v.tptr[i].data;
            RoundArrays ra = round_arrays(sl.d, lay.off, lay.len, tp,
                                          v.tptr[RT_SNAP].len);
            last_groups_ = ra.delta;
            if (linear_) stream_round(ln_, ra); else stream_round(lg_, ra);
            RD_CHECK(hipGetLastError());

            int64_t rows = lay.n_eval ? (int64_t)lay.n_eval
                                      : (eval_all_ ? n_local_ : 0);
            if (rows) {
                int mi = stage_next_;
                Stage& m = stage_[mi];
                grow_stage(m, (size_t)rows);
                if (!mapped_ && (size_t)rows > d_out_rows_) {
                    size_t cap = grown_capacity(d_out_rows_, (size_t)rows);
                    // hipFree waits for the device: no kernel still writes it
                    if (d_out_) RD_CHECK(rd_dev_free(d_out_));
                    d_out_ = nullptr; d_out_rows_ = 0;
                    rd_dev_alloc((void**)&d_out_, cap * 5 * sizeof(float));
                    d_out_rows_ = cap;
                }
                EvalArgs a = ev_;
                a.nodes = lay.n_eval ? sl.d + lay.eval_off : nullptr;
                a.out = mapped_ ? m.h_dev : d_out_;
                hipStream_t es = s;
                if (eval_overlap_ && lay.n_eval) {
                    // sampled evaluation leaves the compute stream: its
                    // rows are gathered here, behind the round's kernels,
                    // and the eval kernel reads the copy on its own stream
                    // while the next round rewrites params
                    grow_gather(m, (size_t)rows, s);
                    launch_snap(ev_.params, nullptr, m.rows_d, nullptr,
                                a.nodes, ident_d_, (int)rows,
                                SnapGeom{ev_.D, ev_.D, 0, 0}, s);
                    RD_CHECK(hipGetLastError());
                    RD_CHECK(hipEventRecord(m.gev, s));
                    // the gather is the last reader of the upload slot
                    RD_CHECK(hipEventRecord(sl.ev, s));
                    recorded = true;
                    es = ev_stream_;
                    RD_CHECK(hipStreamWaitEvent(es, m.gev, 0));
                    a.params = m.rows_d;
                    a.nodes = nullptr;  // row i is node i
                }
                launch_kernel(eval_metrics_kernel, (int)rows, 256, ev_smem_,
                              es, a);
                if (!mapped_)
                    RD_CHECK(hipMemcpyAsync(m.h, d_out_,
                                            (size_t)rows * 5 * sizeof(float),
                                            hipMemcpyDeviceToHost, es));
                RD_CHECK(hipEventRecord(m.ev, es));
                m.round = held_r_; m.rows = rows;
                pending_.push_back(mi);
                stage_next_ ^= 1;
            }
            // after the eval launch: in-stream, it reads its ids from this
            // slot
            if (!recorded) RD_CHECK(hipEventRecord(sl.ev, s));
            recorded = true;
            return rows;
        } catch (...) {
            // a stage that was launched but not queued must not run on
            if (ev_stream_) (void)hipStreamSynchronize(ev_stream_);
            if (!recorded) {
                // what was enqueued may still read the slot: drain it
                // before the slot counts as free again
                (void)hipStreamSynchronize(s);
                if (side_upload_) (void)hipStreamSynchronize(up_stream_);
                slots_.abandon(si);
            }
            throw;
        }
    }

    void release() noexcept
    {
        for (auto& s : ring_) {
            if (s.ev) { (void)hipEventSynchronize(s.ev); rd_event_destroy(s.ev); }
            if (s.h) (void)rd_host_free(s.h);
            if (s.d) (void)rd_dev_free(s.d);
            s = Slot{};
        }
        if (ev_stream_) (void)hipStreamSynchronize(ev_stream_);
        for (auto& m : stage_) {
            if (m.ev) { (void)hipEventSynchronize(m.ev); rd_event_destroy(m.ev); }
            if (m.gev) {
                (void)hipEventSynchronize(m.gev);
                rd_event_destroy(m.gev);
            }
            if (m.h) (void)rd_host_free(m.h);
            if (m.rows_d) (void)rd_dev_free(m.rows_d);
            m = Stage{};
        }
        if (ident_d_) (void)rd_dev_free(ident_d_);
        ident_d_ = nullptr; ident_cap_ = 0;
        if (ev_stream_) {
            (void)hipStreamDestroy(ev_stream_);
            --rd_live[RD_STREAM];
        }
        ev_stream_ = nullptr;
        if (d_out_) (void)rd_dev_free(d_out_);
        d_out_ = nullptr;
        if (up_ev_) rd_event_destroy(up_ev_);
        if (up_stream_) {
            (void)hipStreamSynchronize(up_stream_);
            (void)hipStreamDestroy(up_stream_);
            --rd_live[RD_STREAM];
        }
        up_ev_ = nullptr; up_stream_ = nullptr;
    }

    StateTensors st_;
    torch::Tensor gx_, gy_;
    py::capsule source_cap_;
    RoundSource src_{};
    bool eval_all_, mapped_, side_upload_, eval_overlap_;
    bool linear_ = false;
    Plan<LogregArgs> lg_;
    Plan<LinearArgs> ln_;
    EvalArgs ev_{};
    size_t ev_smem_ = 0;
    int64_t n_local_ = 0, pool_cap_ = 0;

    RoundView view_{};
    bool held_ = false, failed_ = false;
    int64_t held_r_ = -1, last_groups_ = 0, rounds_ = 0;
    double take_s_ = 0, enqueue_s_ = 0;

    Slot ring_[RD_RING];
    SlotRing<RD_RING> slots_;
    Stage stage_[2];
    int stage_next_ = 0;
    std::deque<int> pending_;  // staging indices in flight, oldest first
    std::vector<Done> done_;   // collected, not yet handed to Python
    float* d_out_ = nullptr;
    size_t d_out_rows_ = 0;
    hipStream_t up_stream_ = nullptr;
    hipEvent_t up_ev_ = nullptr;
    hipStream_t ev_stream_ = nullptr;  // eval_overlap: the eval kernels
    int* ident_d_ = nullptr;           // 0, 1, 2, ...: the gather's slot ids
    size_t ident_cap_ = 0;
};

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    py::class_<RoundDriver>(m, "RoundDriver")
        .def(py::init<torch::Tensor, torch::Tensor, torch::Tensor,
                      torch::Tensor, torch::Tensor, torch::Tensor,
                      torch::Tensor, torch::Tensor, torch::Tensor,
                      const std::string&, py::tuple, py::capsule, bool, bool,
                      bool, bool>(),
             py::arg("params"), py::arg("ages"), py::arg("slots"),
             py::arg("slot_ages"), py::arg("X"), py::arg("Y"),
             py::arg("counts"), py::arg("gx"), py::arg("gy"),
             py::arg("family"), py::arg("plan"), py::arg("source"),
             py::arg("eval_all") = false, py::arg("mapped_metrics") = true,
             py::arg("side_upload") = true, py::arg("eval_overlap") = false)
        .def("step", &RoundDriver::step)
        .def("set_pool", &RoundDriver::set_pool)
        .def("poll_eval", &RoundDriver::poll_eval)
        .def("drain", &RoundDriver::drain)
        .def("stats", &RoundDriver::stats)
        .def_property_readonly("last_groups", &RoundDriver::last_groups);
    m.def("round_driver_live", &round_driver_live,
          "(pinned host buffers, device buffers, events, streams) held by "
          "the RoundDrivers of this process");
    m.def("snapshot", &snapshot, "batched model snapshot (arena row copy)");
    // the table of round_source.h: the order of round_buf and lens
    py::tuple arrays((size_t)ROUND_N_ARRAYS), tptrs((size_t)ROUND_N_TPTRS);
    for (int i = 0; i < ROUND_N_ARRAYS; ++i) arrays[i] = ROUND_ARRAY_NAMES[i];
    for (int i = 0; i < ROUND_N_TPTRS; ++i) tptrs[i] = ROUND_TPTR_NAMES[i];
    m.attr("ROUND_ARRAY_NAMES") = arrays;
    m.attr("ROUND_TPTR_NAMES") = tptrs;
    m.def("tick_logreg", &tick_logreg,
          "fused merge + logreg SGD tick, merge_limit after mode");
    m.def("tick_linear", &tick_linear, "fused merge + pegasos/adaline tick");
    m.def("tick_mlp", &tick_mlp,
          "fused merge + MLP SGD tick, merge_limit after mode");
    m.def("mlp_tick_path", &mlp_tick_path,
          "\"lds\" or \"wide\": the kernel tick_mlp / run_round_mlp run for"
          " (dims, batch_size, Smax, mode)");
    m.def("run_round_logreg", round_entry(run_round_logreg),
          "whole-round executor, logreg family, merge_limit after mode",
          py::call_guard<py::gil_scoped_release>());
    m.def("run_round_linear", round_entry(run_round_linear),
          "whole-round executor, pegasos/adaline family",
          py::call_guard<py::gil_scoped_release>());
    m.def("tick_logreg_part", &tick_logreg_part,
          "fused partition-merge + age-rescaled logreg SGD tick (K7/K8)");
    m.def("run_round_logreg_part", round_entry(run_round_logreg_part),
          "whole-round executor, partitioned logreg family",
          py::call_guard<py::gil_scoped_release>());
    m.def("wmerge", &wmerge, "all2all weighted k-way merge (K5 weighted)");
    m.def("tick_logreg_samp", &tick_logreg_samp,
          "fused sampled-merge + logreg SGD tick (K6)");
    m.def("tick_mf", &tick_mf,
          "fused item-block merge + per-rating MF SGD tick (K9/K10)");
    m.def("run_round_mlp", round_entry(run_round_mlp),
          "whole-round executor, MLP family, merge_limit after mode",
          py::call_guard<py::gil_scoped_release>());
    m.def("tick_mlp_part", &tick_mlp_part,
          "fused partition-merge + age-rescaled MLP SGD tick");
    m.def("tick_mlp_samp", &tick_mlp_samp,
          "fused sampled-merge + MLP SGD tick");
    m.def("run_round_mlp_part", round_entry(run_round_mlp_part),
          "whole-round executor, partitioned MLP family",
          py::call_guard<py::gil_scoped_release>());
    m.def("run_round_mlp_samp", round_entry(run_round_mlp_samp),
          "whole-round executor, sampled MLP family",
          py::call_guard<py::gil_scoped_release>());
    m.def("run_round_logreg_samp", round_entry(run_round_logreg_samp),
          "whole-round executor, sampled logreg family",
          py::call_guard<py::gil_scoped_release>());
    m.def("run_round_mf", round_entry(run_round_mf),
          "whole-round executor, MF recommender family",
          py::call_guard<py::gil_scoped_release>());
    m.def("run_round_coop_logreg", round_entry(run_round_coop_logreg, true),
          "single-launch cooperative whole-round executor (logreg)");
    m.def("tick_pens", &tick_pens,
          "PENS step-1 event: score candidates, merge top-m, count winners");
    m.def("tick_pens_mlp", &tick_pens_mlp,
          "PENS step-1 event, MLP family: MFMA forward scoring of the"
          " candidates, top-m merge, MLP SGD");
    // most candidates one PENS event may carry (tick_pens, tick_pens_mlp)
    m.attr("PENS_MAX_CAND") = PENS_MAX_CAND;
    m.def("eval_metrics", &eval_metrics,
          "fused per-node eval metrics on a shared eval set (K13)");
    m.def("eval_metrics_scores", &eval_metrics_scores,
          "K13 metrics epilogue on precomputed scores (MLP/torchmod)");
    // most classes the evaluation kernels take (eval_metrics*, eval_mlp)
    m.attr("EVAL_KMAX") = EVAL_KMAX;
    m.def("eval_mlp", &eval_mlp,
          "K13 for the MLP family: MFMA forward + metrics in one launch, on"
          " per-node shards or (empty eval_counts) one shared set");
    m.def("eval_mlp_tile", &eval_mlp_tile,
          "rows eval_mlp forwards per chunk for (D, d_in, act_total, n_eval);"
          " 0 when the shape does not fit");
    m.def("tick_kmeans", &tick_kmeans,
          "fused centroid merge + assign/EMA k-means tick (K11)");
}
