// gx_chain.h -- what the chaining kernels (gx_chain.hip) and their host driver
// and solver (gx_api_chain.cpp) share: eligibility, the extension score and the
// update rule of DESIGN.md 23.1, the one place both solvers read, so that they
// answer field by field alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gx_match.h"

namespace gx {

constexpr uint32_t kChainNone = 0xFFFFFFFFu;   // GX_CHAIN_NONE
constexpr uint32_t kChainMaxPred = 256;        // GX_CHAIN_MAX_PRED

// gx_chain_params, gx_chain (include/gx.h)
struct ChainParams {
    uint32_t w_match, w_drift, max_gap, max_drift, max_pred;
    int32_t min_score;
};
struct Chain {
    uint64_t member_off;
    int32_t score;
    uint32_t n_anchors, root, end, qstart, tstart, qend, tend;
};

// w x of a weight (<= 1024) and a length or an advance (<= 2^20 wherever the
// product is used): the device's 24-bit multiply is exact there and full rate.
__host__ __device__ inline uint32_t chain_mul(uint32_t w, uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(w, x);
#else
    return w * x;
#endif
}

// Is a = (qa, ta) eligible for b = (qb, tb) as far as the positions say (the caller
// holds b - a against max_pred)?  *dq, *dt: the two advances mod 2^32, which are the
// advances where the answer is yes: positions are below 2^32 and the advances of an
// eligible pair at most 2^20.  No branch: the score kernel runs it on every lane.
__host__ __device__ inline bool chain_eligible(uint32_t qa, uint32_t ta, uint32_t qb, uint32_t tb, uint32_t max_gap,
                                               uint32_t max_drift, uint32_t* dq, uint32_t* dt) {
    const uint32_t q = qb - qa, t = tb - ta;
    const uint32_t hi = q > t ? q : t, lo = q > t ? t : q;
    *dq = q;
    *dt = t;
    return (qb > qa) & (tb > ta) & (hi <= max_gap) & (hi - lo <= max_drift);
}

// ext(a, b) of an eligible pair (of any other pair: some number).  fa + w_match
// min(..) <= w_match (sum of len) < 2^31 and w_drift |dq - dt| <= 2^30: int32 is
// exact.
__host__ __device__ inline int32_t chain_ext(int32_t fa, uint32_t len_b, uint32_t dq, uint32_t dt, uint32_t w_match,
                                             uint32_t w_drift) {
    const uint32_t hi = dq > dt ? dq : dt, lo = dq > dt ? dt : dq;
    const uint32_t m = len_b < lo ? len_b : lo;
    return (int32_t)((uint32_t)fa + chain_mul(w_match, m) - chain_mul(w_drift, hi - lo));
}

// The update rule.  best, pred: what b holds (w_match len_b and kChainNone at
// first).  The first predecessor has to beat w_match len_b strictly; among
// predecessors the larger ext wins and of equal ext the larger a (the nearest).
// A solver that visits a ascending takes every tie, one that visits a descending
// takes none: both end at the same pred.
__host__ __device__ inline bool chain_take(int32_t ext, uint32_t a, int32_t best, uint32_t pred) {
    return (ext > best) | ((ext == best) & (pred != kChainNone) & (a > pred));
}

// Does anchor g (global number, q its qpos) start a segment?  first: it is its
// query's first anchor; q_prev: the qpos of anchor g - 1 otherwise.
__host__ __device__ inline bool chain_segment_start(bool first, uint32_t q_prev, uint32_t q, uint32_t max_gap) {
    return first || q - q_prev > max_gap;   // (q >= q_prev within a query)
}

// Look-back slots a lane of the score kernel holds: 64 R >= max_pred.
inline int chain_slots(uint32_t max_pred) { return max_pred <= 64 ? 1 : max_pred <= 128 ? 2 : 4; }

// Device stages (gx_chain.hip).  anchors: A triples, aoff: nq + 1 offsets into them.
//
// flags[g] = 1 iff anchor g starts a segment, g < A; flags[A] = 0.
hipError_t launch_chain_flags(const Mem* anchors, const uint32_t* aoff, uint32_t nq, uint32_t A, uint32_t max_gap,
                              uint32_t* flags, hipStream_t st);
// sscan: the exclusive scan of flags (sscan[A] = the segments).  seg_start[s] = the
// first anchor of segment s, seg_start[segments] = A; seg_base[s] = the first anchor
// of its query.
hipError_t launch_chain_segments(const uint32_t* aoff, uint32_t nq, uint32_t A, const uint32_t* sscan,
                                 uint32_t* seg_start, uint32_t* seg_base, hipStream_t st);
// The recurrence, a wave a segment: f[g], pred[g] (within the query), root[g]
// (global number), depth[g]; evals[0] += the pairs evaluated, evals[4] += the
// segments whose bounds do not fit the anchors (never; the driver fails on it).
hipError_t launch_chain_score(const Mem* anchors, uint32_t A, const uint32_t* sscan, const uint32_t* seg_start,
                              const uint32_t* seg_base, ChainParams p, int32_t* f, uint32_t* pred, uint32_t* root,
                              uint32_t* depth, unsigned long long* evals, hipStream_t st);
// key[root[g]] = max(f[g] << 32 | ~g): key is A zeroed words.
hipError_t launch_chain_best(const int32_t* f, const uint32_t* root, uint32_t A, unsigned long long* key,
                             hipStream_t st);
// At every root g whose end e has f[e] >= min_score: keep[g] = 1 and mlen[g] =
// depth[e] + 1; 0 elsewhere and at A.
hipError_t launch_chain_heads(const uint32_t* root, const uint32_t* depth, const unsigned long long* key, uint32_t A,
                              int32_t min_score, uint32_t* keep, uint32_t* mlen, hipStream_t st);
// kscan, mscan: the exclusive scans of keep and mlen.  cpre[c] = kscan[aoff[c]] for
// c <= nq; tot[0] = kscan[A], tot[1] = mscan[A], tot[2] = sscan[A].
hipError_t launch_chain_counts(const uint32_t* aoff, uint32_t nq, uint32_t A, const uint32_t* sscan,
                               const uint32_t* kscan, const uint32_t* mscan, uint32_t* cpre, unsigned long long* tot,
                               hipStream_t st);
// Every kept root writes chains[kscan[g]] and, walking pred from its end, its
// members at mscan[g] + depth.  *bad += the chains whose end or query does not fit
// (never; the driver fails on it).
hipError_t launch_chain_walk(const Mem* anchors, uint32_t A, const uint32_t* sscan, const uint32_t* seg_base,
                             const int32_t* f, const uint32_t* pred, const uint32_t* root, const uint32_t* depth,
                             const unsigned long long* key, const uint32_t* kscan, const uint32_t* mscan,
                             Chain* chains, uint32_t* members, unsigned long long* bad, hipStream_t st);

}  // namespace gx
