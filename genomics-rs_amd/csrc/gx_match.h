// gx_match.h -- what the matching-statistics and MEM kernels (gx_match.hip)
// and their host driver (gx_api_match.cpp) share: the rules both the host index
// (ctx = NULL) and the device run, so that they answer field by field alike
// (DESIGN.md 21).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gx_search.h"

namespace gx {

// gx_match_stat, gx_mem (include/gx.h)
struct MatchStat {
    uint32_t len, lo, count, pos;
};
struct Mem {
    uint32_t qpos, tpos, len;
};

// The query of position g of the concatenated buffer: the c with
// offs[c] <= g < offs[c + 1] (g < offs[nq]; empty queries are passed over).
__host__ __device__ inline uint32_t match_query_of(const uint32_t* offs, uint32_t nq, uint32_t g) {
    uint32_t L = 0, R = nq;   // -> the first c with offs[c + 1] > g
    while (L < R) {
        const uint32_t mid = L + (R - L) / 2;
        if (offs[mid + 1] <= g) L = mid + 1; else R = mid;
    }
    return L;
}

// Matching statistics of one position: P = the query from that position, w > 0
// bytes of it to look at (bytes past w are masked by srch_cmp, so they may be
// the next query's).  srch_one gives the longest prefix that occurs; when that
// is not the whole window, its interval takes a second pair of bounds with
// m = len.  At most twice srch_one's word steps.
__host__ __device__ inline MatchStat match_stat_one(const uint8_t* t, const uint32_t* sa, uint32_t N, const uint8_t* P,
                                                    uint32_t w, uint64_t* words) {
    SrchHit h = srch_one(t, sa, N, P, w, words);
    if (h.prefix_len < w) {
        if (h.prefix_len == 0) h = srch_one(t, sa, N, P, 0, words);   // lo = 0, count = N, no compare
        else h = srch_one(t, sa, N, P, h.prefix_len, words);          // occurs whole: count > 0
    }
    MatchStat o;
    o.len = h.prefix_len;
    o.lo = h.lo;
    o.count = h.count;
    o.pos = h.lo < N && sa[h.lo] < N ? sa[h.lo] : 0;
    return o;
}

// The seed of one position: the interval of its min_len-mer, count 0 where
// fewer than L bytes of the query remain or the L-mer does not occur.
__host__ __device__ inline void match_seed_one(const uint8_t* t, const uint32_t* sa, uint32_t N, const uint8_t* P,
                                               uint32_t rem, uint32_t L, uint32_t* lo, uint32_t* cnt, uint64_t* words) {
    *lo = 0;
    *cnt = 0;
    if (rem < L) return;
    const SrchHit h = srch_one(t, sa, N, P, L, words);
    if (h.prefix_len == L) {
        *lo = h.lo;
        *cnt = h.count;
    }
}

// A candidate pair (text i, query position j, the query byte before it at
// P[-1] when j > 0) is kept iff it is left-maximal.
__host__ __device__ inline bool match_left_maximal(const uint8_t* t, uint32_t i, const uint8_t* P, uint32_t j) {
    return i == 0 || j == 0 || t[i - 1] != P[-1];
}

// The length of a kept pair: the match of t[i ..) and P[0 .. rem), the first L
// bytes known equal, extended to the right 8 bytes a step.  The query's end is
// the mask of srch_cmp, the text's end its '$'.
__host__ __device__ inline uint32_t match_extend(const uint8_t* t, uint32_t N, uint32_t i, const uint8_t* P, uint32_t rem,
                                                 uint32_t L, uint64_t* words) {
    int rel;
    return srch_cmp(t, N, i, P, rem, L, &rel, words);
}

// d_cnt of a launch: [0] word steps of the interval kernel, [1] the candidates
// (64-bit sum of cnt), [2] word steps of the emit kernel.
//
// Matching statistics: stats[g] for every position g < npos of the concatenated
// queries (kSufPad zero bytes behind them), window min(W, end of its query - g).
hipError_t launch_match_stats(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* q,
                              const uint32_t* offs, uint32_t nq, uint32_t npos, uint32_t W, MatchStat* stats,
                              unsigned long long* words, hipStream_t st);
// Seeds: lo[g], cnt[g] (cnt[npos] = 0) and qid[g] for every position;
// cnt_total[0] += word steps, cnt_total[1] += sum of cnt.
hipError_t launch_match_seeds(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* q,
                              const uint32_t* offs, uint32_t nq, uint32_t npos, uint32_t L, uint32_t* lo, uint32_t* cnt,
                              uint32_t* qid, unsigned long long* cnt_total, hipStream_t st);
// coff: the exclusive scan of cnt (coff[npos] = T).  Candidate x < T: cg[x] = its
// position g, ci[x] = SA[lo[g] + x - coff[g]], keep[x] = 1 iff left-maximal
// (keep[T] = 0).
hipError_t launch_match_keep(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* q,
                             const uint32_t* offs, const uint32_t* qid, const uint32_t* lo, const uint32_t* coff,
                             uint32_t npos, uint32_t T, uint32_t* cg, uint32_t* ci, uint32_t* keep, hipStream_t st);
// kscan: the exclusive scan of keep.  cpre[c] = coff[offs[c]], mpre[c] =
// kscan[coff[offs[c]]] for c <= nq: the candidates and MEMs before query c.
hipError_t launch_match_counts(const uint32_t* offs, uint32_t nq, const uint32_t* coff, const uint32_t* kscan,
                               uint32_t* cpre, uint32_t* mpre, hipStream_t st);
// Every kept candidate: keys[kscan[x]] = g << 32 | i, vals[kscan[x]] = its length.
hipError_t launch_match_emit(const uint8_t* text, uint32_t N, const uint8_t* q, const uint32_t* offs,
                             const uint32_t* qid, const uint32_t* cg, const uint32_t* ci, const uint32_t* kscan,
                             uint32_t T, uint32_t L, uint64_t* keys, uint32_t* vals, unsigned long long* words,
                             hipStream_t st);
// Sorted keys and lengths -> mems[k] = (g - offs[qid[g]], i, len), k < M.
hipError_t launch_match_pack(const uint64_t* keys, const uint32_t* vals, uint32_t M, const uint32_t* offs,
                             const uint32_t* qid, Mem* mems, hipStream_t st);

}  // namespace gx
