// gx_chain.hip -- colinear chains of a long query's anchors, the device half of
// DESIGN.md 23.  No counterpart in the reference.
//
//   flags     a lane per anchor: does it start a segment (its query's first
//             anchor, or qpos more than max_gap past the anchor before it)?  The
//             scan of the flags numbers the segments.
//   segments  every segment's first anchor and its query's first anchor
//   score     the recurrence, a wave a segment, in its forward form: anchor i of
//             the segment sits in lane i % 64, slot (i / 64) % R, 64 R >= max_pred.
//             At step a the owner's (f, q, t, root, depth) are final and are read
//             with a wave-uniform readlane; the owner takes the anchor 64 R
//             further on into the slot; every lane then updates the running
//             (best, pred, root, depth) of its anchors a + 1 .. a + max_pred.  a
//             ascends, so taking every tie leaves the nearest predecessor.  Rows
//             of 64 anchors are loaded a row ahead and written a row at a time.
//   best      key[root] = max(f << 32 | ~anchor): a tree's end
//   heads     at every root: is its chain reported, and how long is it
//   counts    chains before every query, the two totals
//   walk      a lane a reported chain: its record, and its members stored at
//             member_off + depth while it walks pred from the end
//
// As gx_match.hip: 256-thread workgroups, no kernel waits on another workgroup,
// every device-wide dependency is a kernel boundary.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gx_chain.h"
#include "gx_suffix.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
constexpr int kWaves = kB / 64;
constexpr unsigned kStrideGrid = 2048;   // workgroups at most; they stride over the rest
typedef unsigned long long u64;

// The workgroup's sum of v into *total: wave shuffles, LDS, one vector atomic.
__device__ inline void block_add(u64 v, u64* sh, u64* total) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += sh[q];
        if (s) atomicAdd(total, s);
    }
}

__global__ __launch_bounds__(kB) void chain_flags_kernel(const Mem* __restrict__ anchors,
                                                         const uint32_t* __restrict__ aoff, uint32_t nq, uint32_t A,
                                                         uint32_t max_gap, uint32_t* __restrict__ flags) {
    for (u64 g = (u64)blockIdx.x * kB + threadIdx.x; g <= A; g += (u64)gridDim.x * kB) {
        if (g == A) {
            flags[g] = 0;
            continue;
        }
        const uint32_t c = match_query_of(aoff, nq, (uint32_t)g);
        const bool first = c >= nq || aoff[c] == g;
        flags[g] = chain_segment_start(first, first ? 0u : anchors[g - 1].qpos, anchors[g].qpos, max_gap) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kB) void chain_segments_kernel(const uint32_t* __restrict__ aoff, uint32_t nq, uint32_t A,
                                                            const uint32_t* __restrict__ sscan,
                                                            uint32_t* __restrict__ seg_start,
                                                            uint32_t* __restrict__ seg_base) {
    for (u64 g = (u64)blockIdx.x * kB + threadIdx.x; g <= A; g += (u64)gridDim.x * kB) {
        const uint32_t s = sscan[g];
        if (g == A) {
            seg_start[s] = A;   // (s <= A: the arrays hold A + 1)
            continue;
        }
        if (sscan[g + 1] == s) continue;
        const uint32_t c = match_query_of(aoff, nq, (uint32_t)g);
        seg_start[s] = (uint32_t)g;
        seg_base[s] = c < nq ? aoff[c] : (uint32_t)g;
    }
}

// One anchor of the look-back window as its lane holds it.
struct Slot {
    uint32_t q, t, len;
    uint32_t idx;    // its number within the segment; kChainNone: no anchor
    int32_t best;
    uint32_t pred;   // within the query
    uint32_t root;   // global number
    uint32_t depth;
};

__device__ inline uint32_t lane_of(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}

// One segment on one wave: anchors [s0, s1) of the batch, their query's first
// anchor at `base`.  Returns this lane's share of the pairs evaluated.
template <int R>
__device__ inline u64 chain_segment(const Mem* __restrict__ anchors, uint32_t s0, uint32_t s1, uint32_t base,
                                    const ChainParams& p, int32_t* __restrict__ f, uint32_t* __restrict__ pred,
                                    uint32_t* __restrict__ root, uint32_t* __restrict__ depth) {
    const uint32_t lane = threadIdx.x & 63, n = s1 - s0, loc0 = s0 - base;
    const uint32_t rows = (n + 63) / 64;
    auto load = [&](uint32_t i) {   // anchor i of the segment, zeros behind its end
        Mem m;
        m.qpos = m.tpos = m.len = 0;
        if (i < n) m = anchors[s0 + i];
        return m;
    };
    auto fresh_of = [&](const Mem& m, uint32_t i) {
        Slot s;
        s.q = m.qpos;
        s.t = m.tpos;
        s.len = m.len;
        s.idx = i < n ? i : kChainNone;
        s.best = (int32_t)(p.w_match * m.len);
        s.pred = kChainNone;
        s.root = s0 + i;
        s.depth = 0;
        return s;
    };
    Slot cur[R];
#pragma unroll
    for (int r = 0; r < R; ++r) cur[r] = fresh_of(load(64u * r + lane), 64u * r + lane);
    Mem nxt = load(64u * R + lane);   // the row that follows the slots'
    u64 evals = 0;
    for (uint32_t kb = 0; kb < rows; kb += R) {
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const uint32_t k = kb + s;   // row k in slot s
            if (k >= rows) break;        // (wave-uniform)
            const uint32_t a0 = 64u * k, steps = n - a0 < 64u ? n - a0 : 64u;
            const Mem ahead = load(a0 + 64u * (R + 1) + lane);   // used a row from now
            const Slot fresh = fresh_of(nxt, a0 + 64u * R + lane);
            int32_t of = 0;
            uint32_t op = kChainNone, orr = 0, od = 0, ev = 0;
            for (uint32_t l = 0; l < steps; ++l) {
                const uint32_t a = a0 + l, aq = loc0 + a;
                // the owner's values are final
                const int32_t fa = (int32_t)lane_of((uint32_t)cur[s].best, l);
                const uint32_t qa = lane_of(cur[s].q, l), ta = lane_of(cur[s].t, l);
                const uint32_t ra = lane_of(cur[s].root, l), da = lane_of(cur[s].depth, l);
                // ... it keeps them for the row's store and takes the anchor 64 R further on
                const bool me = lane == l;
                of = me ? cur[s].best : of;
                op = me ? cur[s].pred : op;
                orr = me ? cur[s].root : orr;
                od = me ? cur[s].depth : od;
                cur[s].q = me ? fresh.q : cur[s].q;
                cur[s].t = me ? fresh.t : cur[s].t;
                cur[s].len = me ? fresh.len : cur[s].len;
                cur[s].idx = me ? fresh.idx : cur[s].idx;
                cur[s].best = me ? fresh.best : cur[s].best;
                cur[s].pred = me ? kChainNone : cur[s].pred;
                cur[s].root = me ? fresh.root : cur[s].root;
                cur[s].depth = me ? 0u : cur[s].depth;
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    Slot& b = cur[u];
                    const bool inwin = b.idx - a - 1u < p.max_pred;   // (unsigned: idx <= a and no anchor are out)
                    ev += inwin ? 1u : 0u;
                    uint32_t dq, dt;
                    const bool ok = inwin & chain_eligible(qa, ta, b.q, b.t, p.max_gap, p.max_drift, &dq, &dt);
                    const int32_t ext = chain_ext(fa, b.len, dq, dt, p.w_match, p.w_drift);
                    const bool take = ok & chain_take(ext, aq, b.best, b.pred);
                    b.best = take ? ext : b.best;
                    b.pred = take ? aq : b.pred;
                    b.root = take ? ra : b.root;
                    b.depth = take ? da + 1u : b.depth;
                }
            }
            if (lane < steps) {
                const uint32_t g = s0 + a0 + lane;
                f[g] = of;
                pred[g] = op;
                root[g] = orr;
                depth[g] = od;
            }
            evals += ev;
            nxt = ahead;
        }
    }
    return evals;
}

template <int R>
__global__ __launch_bounds__(kB) void chain_score_kernel(const Mem* __restrict__ anchors, uint32_t A,
                                                         const uint32_t* __restrict__ sscan,
                                                         const uint32_t* __restrict__ seg_start,
                                                         const uint32_t* __restrict__ seg_base, ChainParams p,
                                                         int32_t* __restrict__ f, uint32_t* __restrict__ pred,
                                                         uint32_t* __restrict__ root, uint32_t* __restrict__ depth,
                                                         u64* evals_total) {
    __shared__ u64 sh[kWaves];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kB + threadIdx.x) >> 6));
    const uint32_t nwaves = gridDim.x * kWaves, nseg = sscan[A];
    u64 evals = 0;
    for (uint32_t s = wave; s < nseg; s += nwaves) {
        const uint32_t s0 = seg_start[s], s1 = seg_start[s + 1], base = seg_base[s];
        if (s1 > A || s0 >= s1 || base > s0) {   // never: a segment table that does not fit the anchors is the driver's error
            if ((threadIdx.x & 63) == 0) atomicAdd(evals_total + 4, 1ull);
            continue;
        }
        evals += chain_segment<R>(anchors, s0, s1, base, p, f, pred, root, depth);
    }
    block_add(evals, sh, evals_total);
}

__global__ __launch_bounds__(kB) void chain_best_kernel(const int32_t* __restrict__ f, const uint32_t* __restrict__ root,
                                                        uint32_t A, u64* __restrict__ key) {
    for (u64 g = (u64)blockIdx.x * kB + threadIdx.x; g < A; g += (u64)gridDim.x * kB) {
        const uint32_t r = root[g];
        if (r < A) atomicMax(&key[r], (u64)(uint32_t)f[g] << 32 | (uint32_t)~(uint32_t)g);
    }
}

__global__ __launch_bounds__(kB) void chain_heads_kernel(const uint32_t* __restrict__ root,
                                                         const uint32_t* __restrict__ depth,
                                                         const u64* __restrict__ key, uint32_t A, int32_t min_score,
                                                         uint32_t* __restrict__ keep, uint32_t* __restrict__ mlen) {
    for (u64 g = (u64)blockIdx.x * kB + threadIdx.x; g <= A; g += (u64)gridDim.x * kB) {
        uint32_t k = 0, m = 0;
        if (g < A && root[g] == g) {
            const u64 x = key[g];
            const uint32_t e = ~(uint32_t)x;
            if (e < A && (int32_t)(x >> 32) >= min_score) {
                k = 1;
                m = depth[e] + 1u;
            }
        }
        keep[g] = k;
        mlen[g] = m;
    }
}

__global__ __launch_bounds__(kB) void chain_counts_kernel(const uint32_t* __restrict__ aoff, uint32_t nq, uint32_t A,
                                                          const uint32_t* __restrict__ sscan,
                                                          const uint32_t* __restrict__ kscan,
                                                          const uint32_t* __restrict__ mscan,
                                                          uint32_t* __restrict__ cpre, u64* __restrict__ tot) {
    const u64 c = (u64)blockIdx.x * kB + threadIdx.x;
    if (c > nq) return;
    cpre[c] = kscan[aoff[c]];
    if (c == nq) {
        tot[0] = kscan[A];
        tot[1] = mscan[A];
        tot[2] = sscan[A];
    }
}

__global__ __launch_bounds__(kB) void chain_walk_kernel(const Mem* __restrict__ anchors, uint32_t A,
                                                        const uint32_t* __restrict__ sscan,
                                                        const uint32_t* __restrict__ seg_base,
                                                        const int32_t* __restrict__ f, const uint32_t* __restrict__ pred,
                                                        const uint32_t* __restrict__ root,
                                                        const uint32_t* __restrict__ depth, const u64* __restrict__ key,
                                                        const uint32_t* __restrict__ kscan,
                                                        const uint32_t* __restrict__ mscan, Chain* __restrict__ chains,
                                                        uint32_t* __restrict__ members, u64* bad) {
    for (u64 g = (u64)blockIdx.x * kB + threadIdx.x; g < A; g += (u64)gridDim.x * kB) {
        const uint32_t k = kscan[g];
        if (root[g] != g || kscan[g + 1] == k) continue;   // not a root, or its chain is not reported
        const uint32_t e = ~(uint32_t)key[g];
        const uint32_t base = seg_base[sscan[g + 1] - 1u];
        const uint32_t moff = mscan[g], cnt = mscan[g + 1] - moff;
        if (e >= A || e < g || base > g) {   // never: likewise
            atomicAdd(bad, 1ull);
            continue;
        }
        const Mem ar = anchors[g], ae = anchors[e];
        Chain c;
        c.member_off = moff;
        c.score = f[e];
        c.n_anchors = cnt;
        c.root = (uint32_t)g - base;
        c.end = e - base;
        c.qstart = ar.qpos;
        c.tstart = ar.tpos;
        c.qend = ae.qpos + ae.len;
        c.tend = ae.tpos + ae.len;
        chains[k] = c;
        uint32_t x = e;
        for (uint32_t step = 0; step < cnt; ++step) {
            const uint32_t d = depth[x];
            if (d < cnt) members[moff + d] = x - base;
            const uint32_t pl = pred[x];
            if (pl == kChainNone || base + pl >= x) break;   // the root (pred < its anchor always)
            x = base + pl;
        }
    }
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + kB - 1) / kB); }
inline unsigned stride_grid(u64 n) { return std::max(1u, std::min(kStrideGrid, blocks_of(n))); }

}  // namespace

hipError_t launch_chain_flags(const Mem* anchors, const uint32_t* aoff, uint32_t nq, uint32_t A, uint32_t max_gap,
                              uint32_t* flags, hipStream_t st) {
    hipLaunchKernelGGL(chain_flags_kernel, dim3(stride_grid((u64)A + 1)), dim3(kB), 0, st, anchors, aoff, nq, A, max_gap,
                       flags);
    return hipGetLastError();
}

hipError_t launch_chain_segments(const uint32_t* aoff, uint32_t nq, uint32_t A, const uint32_t* sscan,
                                 uint32_t* seg_start, uint32_t* seg_base, hipStream_t st) {
    hipLaunchKernelGGL(chain_segments_kernel, dim3(stride_grid((u64)A + 1)), dim3(kB), 0, st, aoff, nq, A, sscan,
                       seg_start, seg_base);
    return hipGetLastError();
}

hipError_t launch_chain_score(const Mem* anchors, uint32_t A, const uint32_t* sscan, const uint32_t* seg_start,
                              const uint32_t* seg_base, ChainParams p, int32_t* f, uint32_t* pred, uint32_t* root,
                              uint32_t* depth, unsigned long long* evals, hipStream_t st) {
    // a wave a segment, and there are at most A segments: kWaves of them a workgroup
    const dim3 grid(stride_grid((u64)A * 64)), block(kB);
    switch (chain_slots(p.max_pred)) {
        case 1:
            hipLaunchKernelGGL(chain_score_kernel<1>, grid, block, 0, st, anchors, A, sscan, seg_start, seg_base, p, f,
                               pred, root, depth, evals);
            break;
        case 2:
            hipLaunchKernelGGL(chain_score_kernel<2>, grid, block, 0, st, anchors, A, sscan, seg_start, seg_base, p, f,
                               pred, root, depth, evals);
            break;
        default:
            hipLaunchKernelGGL(chain_score_kernel<4>, grid, block, 0, st, anchors, A, sscan, seg_start, seg_base, p, f,
                               pred, root, depth, evals);
            break;
    }
    return hipGetLastError();
}

hipError_t launch_chain_best(const int32_t* f, const uint32_t* root, uint32_t A, unsigned long long* key,
                             hipStream_t st) {
    hipLaunchKernelGGL(chain_best_kernel, dim3(stride_grid(A)), dim3(kB), 0, st, f, root, A, key);
    return hipGetLastError();
}

hipError_t launch_chain_heads(const uint32_t* root, const uint32_t* depth, const unsigned long long* key, uint32_t A,
                              int32_t min_score, uint32_t* keep, uint32_t* mlen, hipStream_t st) {
    hipLaunchKernelGGL(chain_heads_kernel, dim3(stride_grid((u64)A + 1)), dim3(kB), 0, st, root, depth, key, A,
                       min_score, keep, mlen);
    return hipGetLastError();
}

hipError_t launch_chain_counts(const uint32_t* aoff, uint32_t nq, uint32_t A, const uint32_t* sscan,
                               const uint32_t* kscan, const uint32_t* mscan, uint32_t* cpre, unsigned long long* tot,
                               hipStream_t st) {
    hipLaunchKernelGGL(chain_counts_kernel, dim3(blocks_of((u64)nq + 1)), dim3(kB), 0, st, aoff, nq, A, sscan, kscan,
                       mscan, cpre, tot);
    return hipGetLastError();
}

hipError_t launch_chain_walk(const Mem* anchors, uint32_t A, const uint32_t* sscan, const uint32_t* seg_base,
                             const int32_t* f, const uint32_t* pred, const uint32_t* root, const uint32_t* depth,
                             const unsigned long long* key, const uint32_t* kscan, const uint32_t* mscan,
                             Chain* chains, uint32_t* members, unsigned long long* bad, hipStream_t st) {
    hipLaunchKernelGGL(chain_walk_kernel, dim3(stride_grid(A)), dim3(kB), 0, st, anchors, A, sscan, seg_base, f, pred,
                       root, depth, key, kscan, mscan, chains, members, bad);
    return hipGetLastError();
}

}  // namespace gx
