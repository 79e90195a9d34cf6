// gx_search.h -- what the search mode kernels (gx_search.hip) and their host
// driver (gx_api_search.cpp) share: the one comparison rule of both, so that
// the host index (ctx = NULL) and the device answer every pattern alike
// (DESIGN.md 18).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gx_suffix.h"

namespace gx {

constexpr uint32_t kSrchMaxPattern = 65535;   // bytes: at most 8,192 word compares per probe

// gx_search_hit (include/gx.h)
struct SrchHit {
    uint32_t lo, count, prefix_len, prefix_pos;
};

__host__ __device__ inline uint64_t srch_load8(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// P (m bytes, all above '$') against the suffix of t at i, the first h bytes
// known equal.  Returns lcp(P, t[i..]) and *rel = 0: the suffix is smaller,
// 1: it has P as a prefix, 2: it is larger.  8 bytes a step; the first
// differing byte decides, unsigned.  t holds N bytes ending in '$' and kSufPad
// zero bytes, P has kSufPad readable bytes behind it: a load never leaves
// either, and what the pattern's last word reads past m is masked.  A suffix
// shorter than P differs from it at its '$' at the latest.
__host__ __device__ inline uint32_t srch_cmp(const uint8_t* t, uint32_t N, uint32_t i, const uint8_t* P, uint32_t m,
                                             uint32_t h, int* rel, uint64_t* words) {
    *rel = 0;
    if (i >= N) return 0;   // (a corrupt array entry: not dereferenced)
    while (h < m) {
        if ((uint64_t)i + h >= N) return h;   // (never on admitted bytes: the '$' decided)
        const uint64_t pw = srch_load8(P + h), tw = srch_load8(t + i + h);
        uint64_t x = pw ^ tw;
        ++*words;
        const uint32_t rem = m - h;
        if (rem < 8) x &= (1ull << (8 * rem)) - 1ull;
        if (x) {
            const int d = __builtin_ctzll(x) >> 3;
            *rel = (uint8_t)(tw >> (8 * d)) < (uint8_t)(pw >> (8 * d)) ? 0 : 2;
            return h + (uint32_t)d;
        }
        h += 8;
    }
    *rel = 1;
    return m;
}

// The four answers for one pattern.  Two binary searches over
// SA, the second only where P occurs; each probe starts at min(l, r), the bytes
// both ends of the open interval share with P, and the ends' LCPs left by the
// first search are the two neighbour LCPs of the insertion point.
__host__ __device__ inline SrchHit srch_one(const uint8_t* t, const uint32_t* sa, uint32_t N, const uint8_t* P,
                                            uint32_t m, uint64_t* words) {
    SrchHit o;
    if (m == 0) {
        o.lo = 0;
        o.count = N;
        o.prefix_len = 0;
        o.prefix_pos = sa[0] < N ? sa[0] : 0;
        return o;
    }
    uint32_t L = 0, R = N, ll = 0, rl = 0;   // ll = lcp(P, SA[L - 1]), rl = lcp(P, SA[R]) where those exist
    while (L < R) {
        const uint32_t mid = L + (R - L) / 2;
        int rel;
        const uint32_t h = srch_cmp(t, N, sa[mid], P, m, ll < rl ? ll : rl, &rel, words);
        if (rel == 0) { L = mid + 1; ll = h; } else { R = mid; rl = h; }
    }
    o.lo = L;
    const uint32_t a = L > 0 ? ll : 0, b = L < N ? rl : 0;
    if (b == m) {   // SA[lo] has P as a prefix: the first suffix past the interval
        uint32_t L2 = L + 1, R2 = N, l2 = m, r2 = 0;
        while (L2 < R2) {
            const uint32_t mid = L2 + (R2 - L2) / 2;
            int rel;
            const uint32_t h = srch_cmp(t, N, sa[mid], P, m, l2 < r2 ? l2 : r2, &rel, words);
            if (rel != 2) { L2 = mid + 1; l2 = h; } else { R2 = mid; r2 = h; }
        }
        o.count = L2 - L;
        o.prefix_len = m;
        o.prefix_pos = sa[L];
        return o;
    }
    o.count = 0;
    o.prefix_len = a > b ? a : b;
    o.prefix_pos = 0;
    if (o.prefix_len) {
        const uint32_t k = a >= b ? L - 1 : L;
        o.prefix_pos = sa[k] < N ? sa[k] : 0;
    }
    return o;
}

// hits[p] for pattern p = pats[offs[p] .. offs[p + 1]); *words += the 8-byte
// compare steps of the launch (one atomic per workgroup).
hipError_t launch_srch_range(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* pats,
                             const uint32_t* offs, uint32_t npat, SrchHit* hits, unsigned long long* words,
                             hipStream_t st);
// q[p] = min(hits[p].count, max_hits) for p < npat, q[npat] = 0.
hipError_t launch_srch_clamp(const SrchHit* hits, uint32_t npat, uint32_t max_hits, uint32_t* q, hipStream_t st);
// offs: the exclusive scan of q (offs[npat] = the total).  positions[offs[p] + r]
// = SA[hits[p].lo + r]; nothing is written when the total exceeds cap.
hipError_t launch_srch_gather(const uint32_t* sa, uint32_t N, const SrchHit* hits, const uint32_t* offs,
                              uint32_t npat, uint32_t* positions, uint64_t cap, hipStream_t st);

}  // namespace gx
