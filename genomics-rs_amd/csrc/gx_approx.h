// gx_approx.h -- what the k-mismatch kernels (gx_approx.hip) and their host
// driver (gx_api_search.cpp) share: the piece bounds, the exact count of
// differing bytes in a word and the verify walk, so that the host index
// (ctx = NULL) and the device keep and reject every candidate alike
// (DESIGN.md 19).
#pragma once
#include "gx_search.h"

namespace gx {

constexpr uint32_t kAprxMaxK = 8;   // GX_APPROX_MAX_K

// gx_approx_hit (include/gx.h)
struct AprxHit {
    uint32_t count, best_dist, best_pos, candidates;
};

// Piece j of a pattern of m bytes cut into k1 = k + 1 pieces is
// [aprx_piece_start(m, k1, j), aprx_piece_start(m, k1, j + 1)); none is empty
// when m >= k1.
__host__ __device__ inline uint32_t aprx_piece_start(uint32_t m, uint32_t k1, uint32_t j) {
    return (uint32_t)((uint64_t)j * m / k1);
}

// 0x80 in every byte of x that is not zero, exactly: the low seven bits carry
// into bit 7 of their own byte and no further, and bit 7 itself is or-ed in.
// (The borrow trick (x - 0x01..) & ~x & 0x80.. flags a 0x01 byte above a zero
// byte as zero too; it is not used.)
__host__ __device__ inline uint64_t aprx_ne_bytes(uint64_t x) {
    const uint64_t lo7 = 0x7f7f7f7f7f7f7f7full;
    return (((x & lo7) + lo7) | x) & ~lo7;
}

// One candidate: the window w = t + c (m bytes, inside the text: 0 <= c, c + m
// <= n) against P, reached through piece j of k + 1.  Kept iff d(c) <= k and
// every piece before j has a mismatch, so that the first intact piece alone
// reports an occurrence.  8 bytes a step, the pattern's last word masked to
// the bytes it has left; leaves as soon as the distance passes k or an earlier
// piece turns out intact.  *dist = d(c) when kept.  Loads stay inside the
// kSufPad bytes behind text and patterns.
__host__ __device__ inline bool aprx_verify(const uint8_t* w, const uint8_t* P, uint32_t m, uint32_t k, uint32_t j,
                                            uint32_t* dist, uint64_t* words) {
    const uint32_t k1 = k + 1;
    uint32_t d = 0, cur = 0, cs = 0, ce = aprx_piece_start(m, k1, 1);   // piece cur = [cs, ce), undecided
    bool seen = false;                                                  // a mismatch in piece cur so far
    for (uint32_t h = 0; h < m; h += 8) {
        uint64_t x = srch_load8(P + h) ^ srch_load8(w + h);
        ++*words;
        const uint32_t rem = m - h;
        if (rem < 8) x &= (1ull << (8 * rem)) - 1ull;
        const uint64_t y = aprx_ne_bytes(x);
        d += (uint32_t)__builtin_popcountll(y);
        if (d > k) return false;
        // the pieces before j that this word touches: ce > h holds for an undecided piece
        while (cur < j && cs < h + 8) {
            const uint32_t lo = cs > h ? cs - h : 0, hi = (ce < h + 8 ? ce : h + 8) - h;   // bytes [lo, hi) of the word
            const uint64_t below_hi = hi == 8 ? ~0ull : (1ull << (8 * hi)) - 1ull;
            if (y & below_hi & ~((1ull << (8 * lo)) - 1ull)) seen = true;
            if (ce > h + 8) break;       // the piece goes on in the next word
            if (!seen) return false;     // an earlier piece is intact: its own candidate reports this start
            ++cur;
            seen = false;
            cs = ce;
            ce = aprx_piece_start(m, k1, cur + 1);
        }
    }
    *dist = d;
    return true;
}

// poffs[i] for i <= npat * k1: the start of piece i % k1 of pattern i / k1 in
// the packed patterns (poffs[npat * k1] = offs[npat]).
hipError_t launch_aprx_pieces(const uint32_t* offs, uint32_t npat, uint32_t k1, uint32_t* poffs, hipStream_t st);
// *total += the piece counts, in 64 bits.
hipError_t launch_aprx_total(const SrchHit* phits, uint32_t npieces, unsigned long long* total, hipStream_t st);
// A lane per candidate g < total = coffs[npieces] (coffs: the exclusive scan of
// the piece counts): keep[g] = 1 or 0, keep[total] = 0, dist[g], start[g], and
// best[p] = min(best[p], d << 32 | start) over pattern p's kept candidates
// (preset to all ones).  *words += the 8-byte steps of the launch.
hipError_t launch_aprx_verify(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* pats,
                              const uint32_t* offs, const uint32_t* poffs, const SrchHit* phits,
                              const uint32_t* coffs, uint32_t npieces, uint32_t k, uint32_t total, uint32_t* keep,
                              uint8_t* dist, uint32_t* start, unsigned long long* best, unsigned long long* words,
                              hipStream_t st);
// kscan: the exclusive scan of keep (total + 1 entries).  hits[p] and oq[p] =
// min(count, max_hits) for p < npat, oq[npat] = 0.
hipError_t launch_aprx_fill(const uint32_t* coffs, const uint32_t* kscan, const unsigned long long* best,
                            uint32_t npat, uint32_t k1, uint32_t max_hits, AprxHit* hits, uint32_t* oq,
                            hipStream_t st);
// ooffs: the exclusive scan of oq.  The kept candidates whose rank within their
// pattern is below max_hits go to positions[] and distances[] at ooffs[p] +
// rank; nothing is written when ooffs[npat] exceeds cap.
hipError_t launch_aprx_scatter(const uint32_t* coffs, const uint32_t* kscan, const uint32_t* ooffs, uint32_t npat,
                               uint32_t k1, uint32_t total, uint32_t max_hits, const uint32_t* start,
                               const uint8_t* dist, uint32_t* positions, uint8_t* distances, uint64_t cap,
                               hipStream_t st);

}  // namespace gx
