// gx_edit.h -- what the k-difference kernels (gx_edit.hip) and their host
// driver (gx_api_search.cpp) share: the band rows of Sellers' recurrence, what
// a candidate reports, the minimum over a run of equal ends and the start of
// an occurrence, so that the host index (ctx = NULL) and the device compute
// every end, distance and start alike.
#pragma once
#include "gx_approx.h"

namespace gx {

constexpr uint32_t kEditMaxM = 4096;         // GX_EDIT_MAX_M
constexpr uint32_t kEditInf = 0x3FFFFFFFu;   // a cell outside the band or the text (+ 1 does not wrap)

// gx_edit_hit (include/gx.h)
struct EditHit {
    uint32_t count, best_dist, best_end, candidates;
};

// At most this many candidates report one end of one pattern: 2k + 1 diagonals
// from each of k + 1 pieces.
__host__ __device__ inline uint32_t edit_run_bound(uint32_t k) { return (2 * k + 1) * (k + 1); }

// Rows 1 .. m of the unit-cost recurrence on the band of 2k + 1 diagonals, kept
// by diagonal slot: slot s of row i is the cell (i, c) with c = i + d0 - k + s,
// so the diagonal predecessor is the slot's own previous value, the vertical
// one is slot s + 1 of the row before and the horizontal one slot s - 1 of the
// same row.  K >= k fixes the slots at compile time (2K + 1 values a lane,
// indexed by constants only: registers, not scratch); slots from 2k + 1 on,
// columns below 0 and columns above lim do not exist and count as infinite.
//
// REV = false: the text forwards, column c is the byte t[c - 1], D[0][c] = 0
// (an occurrence may begin anywhere), lim = n.  REV = true: the text read
// backwards from the end e = lim, column c is the byte t[e - c], against the
// pattern read backwards, D[0][c] = c (anchored at e), d0 = 0.  Both:
// D[i][0] = i.  Column 0 is a boundary and loads nothing, a column in [1, lim]
// loads a byte in [0, lim - 1]: nothing in front of the text is read, and
// nothing behind its n bytes.
//
// Leaves with false as soon as a row's minimum passes kk (row minima never
// decrease: every cell is a cell of the row before, or the cell to its left,
// plus something).  *cells += 2k + 1 a row.  Returns true with row m in D.
template <int K, bool REV>
__host__ __device__ inline bool edit_rows(const uint8_t* t, uint32_t lim, const uint8_t* P, uint32_t m, uint32_t k,
                                          int32_t d0, uint32_t kk, uint32_t (&D)[2 * K + 1], uint64_t* cells) {
    constexpr int W = 2 * K + 1;
    const int32_t w2 = (int32_t)(2 * k + 1), base = d0 - (int32_t)k;   // row i, slot s: column i + base + s
    uint32_t tw[W];   // tw[s]: the text byte of slot s's column in the coming row
#pragma unroll
    for (int s = 0; s < W; ++s) {
        const int32_t c = base + s;   // row 0
        D[s] = (s < w2 && c >= 0 && (uint32_t)c <= lim) ? (REV ? (uint32_t)c : 0u) : kEditInf;
        const int32_t c1 = c + 1;     // row 1
        tw[s] = (c1 >= 1 && (uint32_t)c1 <= lim) ? t[REV ? lim - (uint32_t)c1 : (uint32_t)c1 - 1] : 0u;
    }
    for (uint32_t i = 1; i <= m; ++i) {
        const uint32_t pb = P[REV ? m - i : i - 1];
        uint32_t rowmin = kEditInf;
#pragma unroll
        for (int s = 0; s < W; ++s) {
            const int32_t c = (int32_t)i + base + s;
            uint32_t v = kEditInf;
            if (s < w2 && c >= 0 && (uint32_t)c <= lim) {
                if (c == 0) {
                    v = i;
                } else {
                    v = D[s] + (pb != tw[s] ? 1u : 0u);                   // diagonal: (i - 1, c - 1)
                    if (s + 1 < W) v = v < D[s + 1] + 1 ? v : D[s + 1] + 1;   // vertical: (i - 1, c)
                    if (s > 0) v = v < D[s - 1] + 1 ? v : D[s - 1] + 1;       // horizontal: (i, c - 1), already this row's
                    v = v < kEditInf ? v : kEditInf;
                }
            }
            D[s] = v;
            rowmin = v < rowmin ? v : rowmin;
        }
        *cells += (uint32_t)w2;
        if (rowmin > kk) return false;
        // the window slides by one byte
#pragma unroll
        for (int s = 0; s + 1 < W; ++s) tw[s] = tw[s + 1];
        const int32_t cn = (int32_t)i + 1 + base + (W - 1);
        tw[W - 1] = (i < m && cn >= 1 && (uint32_t)cn <= lim) ? t[REV ? lim - (uint32_t)cn : (uint32_t)cn - 1] : 0u;
    }
    return true;
}

// One candidate: piece found so that the pattern's byte 0 lies on diagonal d0
// (-k <= d0 <= n - m + k).  The ends it reports are the columns c = m + d0 - k
// + s of row m with D <= k: bit s of *mask, and the distance in nibble s of
// *nib (slot 16, which only k = 8 has, in bits 24..27 of *mask).  Returns
// their number.
template <int K>
__host__ __device__ inline uint32_t edit_band(const uint8_t* t, uint32_t n, const uint8_t* P, uint32_t m, uint32_t k,
                                              int32_t d0, uint32_t* mask, uint64_t* nib, uint64_t* cells) {
    constexpr int W = 2 * K + 1;
    uint32_t D[W];
    *mask = 0;
    *nib = 0;
    if (!edit_rows<K, false>(t, n, P, m, k, d0, k, D, cells)) return 0;
    uint32_t cnt = 0, mk = 0;
    uint64_t nb = 0;
#pragma unroll
    for (int s = 0; s < W; ++s) {
        if (D[s] <= k) {   // (slots outside the band or the text hold kEditInf)
            mk |= 1u << s;
            if (s < 16) nb |= (uint64_t)D[s] << (4 * s);
            else mk |= D[s] << 24;
            ++cnt;
        }
    }
    *mask = mk;
    *nib = nb;
    return cnt;
}

// The distance slot s reported (bit s of mask is set).
__host__ __device__ inline uint32_t edit_slot_dist(uint32_t mask, uint64_t nib, uint32_t s) {
    return s < 16 ? (uint32_t)(nib >> (4 * s)) & 15u : (mask >> 24) & 15u;
}

// b(e) for an occurrence that ends at e with distance d = E(e): the largest b
// with ed(P, s[b .. e)) = d, i.e. e minus the smallest l with D[m][l] = d in
// the anchored band of the reversed pattern against the text read backwards
// from e.  0xFFFFFFFF when no column has d (never, for a d that is E(e)).
template <int K>
__host__ __device__ inline uint32_t edit_start(const uint8_t* t, uint32_t e, const uint8_t* P, uint32_t m, uint32_t k,
                                               uint32_t d, uint64_t* cells) {
    constexpr int W = 2 * K + 1;
    uint32_t D[W];
    if (!edit_rows<K, true>(t, e, P, m, k, 0, d, D, cells)) return 0xFFFFFFFFu;
    uint32_t b = 0xFFFFFFFFu;
#pragma unroll
    for (int s = W - 1; s >= 0; --s)   // descending: the smallest column wins
        if (D[s] == d) b = e - (uint32_t)((int32_t)m - (int32_t)k + s);
    return b;
}

// The distance of the run of equal keys that begins at i (a run head): the
// minimum over the run, since a band's value is E(e) only for the candidate
// through which e's best alignment passes and larger for the others.  bound:
// edit_run_bound(k).
__host__ __device__ inline uint32_t edit_run_min(const uint64_t* keys, const uint32_t* vals, uint64_t i, uint64_t E,
                                                 uint32_t bound) {
    const uint64_t key = keys[i];
    uint32_t d = vals[i];
    for (uint32_t r = 1; r < bound && i + r < E && keys[i + r] == key; ++r) d = vals[i + r] < d ? vals[i + r] : d;
    return d;
}

// Whether the candidate's diagonal d0 = at - ps is one a window inside the text can lie on.
__host__ __device__ inline bool edit_diag_ok(int64_t d0, uint32_t n, uint32_t m, uint32_t k) {
    return d0 >= -(int64_t)k && d0 <= (int64_t)n - (int64_t)m + (int64_t)k;
}

// The band width the kernels are built for: the smallest of 1, 2, 4, 8 that holds k.
inline int edit_width_of(uint32_t k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

// The host index's calls, at the width the kernels use for k.
inline uint32_t edit_band_host(const uint8_t* t, uint32_t n, const uint8_t* P, uint32_t m, uint32_t k, int32_t d0,
                               uint32_t* mask, uint64_t* nib, uint64_t* cells) {
    switch (edit_width_of(k)) {
        case 1: return edit_band<1>(t, n, P, m, k, d0, mask, nib, cells);
        case 2: return edit_band<2>(t, n, P, m, k, d0, mask, nib, cells);
        case 4: return edit_band<4>(t, n, P, m, k, d0, mask, nib, cells);
        default: return edit_band<8>(t, n, P, m, k, d0, mask, nib, cells);
    }
}
inline uint32_t edit_start_host(const uint8_t* t, uint32_t e, const uint8_t* P, uint32_t m, uint32_t k, uint32_t d,
                                uint64_t* cells) {
    switch (edit_width_of(k)) {
        case 1: return edit_start<1>(t, e, P, m, k, d, cells);
        case 2: return edit_start<2>(t, e, P, m, k, d, cells);
        case 4: return edit_start<4>(t, e, P, m, k, d, cells);
        default: return edit_start<8>(t, e, P, m, k, d, cells);
    }
}

// A lane per candidate g < total (coffs: the exclusive scan of the piece
// counts): cnt[g] = the ends it reports, cnt[total] = 0, rep[g] / nib[g] as
// edit_band leaves them.  *ends += the reported ends and *cells += the cell
// updates of the launch, both in 64 bits.
hipError_t launch_edit_verify(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* pats,
                              const uint32_t* offs, const uint32_t* poffs, const SrchHit* phits, const uint32_t* coffs,
                              uint32_t npieces, uint32_t k, uint32_t total, uint32_t* cnt, uint32_t* rep, uint64_t* nib,
                              unsigned long long* ends, unsigned long long* cells, hipStream_t st);
// eoffs: the exclusive scan of cnt.  keys[eoffs[g] ..] = pattern << 32 | end, vals = the distance.
hipError_t launch_edit_emit(const uint32_t* sa, uint32_t N, const uint32_t* offs, const uint32_t* poffs,
                            const SrchHit* phits, const uint32_t* coffs, uint32_t npieces, uint32_t k, uint32_t total,
                            const uint32_t* eoffs, const uint32_t* rep, const uint64_t* nib, uint64_t* keys,
                            uint32_t* vals, hipStream_t st);
// Sorted keys: head[i] = 1 where a run begins (head[E] = 0), dmin[i] = the run's
// minimum there, best[p] = min(best[p], d << 32 | end) over pattern p's heads.
hipError_t launch_edit_heads(const uint64_t* keys, const uint32_t* vals, uint32_t E, uint32_t k, uint32_t* head,
                             uint32_t* dmin, unsigned long long* best, hipStream_t st);
// hscan: the exclusive scan of head (E + 1 entries).  hits[p], hbase[p] = the
// rank of pattern p's first head among all heads, oq[p] = min(count, max_hits),
// oq[npat] = 0.
hipError_t launch_edit_fill(const uint64_t* keys, const uint32_t* hscan, uint32_t E, const uint32_t* coffs,
                            const unsigned long long* best, uint32_t npat, uint32_t k1, uint32_t max_hits,
                            EditHit* hits, uint32_t* hbase, uint32_t* oq, hipStream_t st);
// ooffs: the exclusive scan of oq.  The heads whose rank within their pattern
// is below max_hits go to ends[] and distances[] at ooffs[p] + rank; nothing is
// written when ooffs[npat] exceeds cap.
hipError_t launch_edit_scatter(const uint64_t* keys, const uint32_t* dmin, const uint32_t* hscan, uint32_t E,
                               const uint32_t* hbase, const uint32_t* ooffs, uint32_t npat, uint32_t max_hits,
                               uint32_t* ends, uint8_t* distances, uint64_t cap, hipStream_t st);
// A lane per reported occurrence o < ooffs[npat] <= cap: starts[o].
hipError_t launch_edit_starts(const uint8_t* text, const uint8_t* pats, const uint32_t* offs, const uint32_t* ooffs,
                              uint32_t npat, uint32_t k, const uint32_t* ends, const uint8_t* distances,
                              uint32_t* starts, uint64_t cap, hipStream_t st);

}  // namespace gx
