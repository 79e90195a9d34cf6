// gx_extend.h -- what the banded-extension kernels (gx_extend.hip) and their
// host driver (gx_api_extend.cpp) share: the rows of the reference's affine-gap
// recurrence on the 2B + 1 diagonals |j - i| <= B and the retrace over the two
// bits a cell leaves, so that the host index (ctx = NULL) and the device give
// every hit the same record and the same runs.
#pragma once
#include "gx_edit.h"

namespace gx {

constexpr uint32_t kExtMaxBand = 15;        // GX_EXTEND_MAX_BAND
constexpr int32_t kExtMaxScore = 32767;     // GX_EXTEND_MAX_SCORE
constexpr int32_t kExtNeg = -(1 << 30);     // a plane outside the band, and the reference's negative infinity

// gx_scores narrowed (every magnitude <= kExtMaxScore)
struct ExtScores {
    int32_t sm, smm, g, h;
};

// gx_extend_hit (include/gx.h)
struct ExtHit {
    int32_t score;
    uint32_t n_steps, matches, mismatches, opening_gaps, gap_extensions, identities, cigar_len;
};

// The trace word of a row: two bits a slot (0: S, 1: I, 2: D, the plane the
// retrace takes in that cell), 32 bits where 2 (2K + 1) <= 32.
template <int K>
struct ExtWord {
    typedef uint64_t type;
};
template <>
struct ExtWord<2> {
    typedef uint32_t type;
};
template <>
struct ExtWord<4> {
    typedef uint32_t type;
};

__host__ __device__ inline int32_t ext_max(int32_t a, int32_t b) { return a > b ? a : b; }

// Rows 0 .. w of alignment_table(is_local = false) (algo.rs:191-268) for
// s1 = t[0 .. w) (index i) and s2 = P[0 .. m) (index j), on the cells with
// |j - i| <= B, kept by diagonal slot: slot s of row i is the cell (i, j) with
// j = i - B + s.  The diagonal predecessor (i - 1, j - 1) is the slot's own old
// value, the text-consuming one (i - 1, j) slot s + 1 of the old row, the
// pattern-consuming one (i, j - 1) slot s - 1 of the new row, so the row is
// updated in place, ascending.  K >= B fixes the slots at compile time (two
// values a slot, A = max(S, I) and D, indexed by constants only); slots from
// 2B + 1 on and columns outside [0, m] hold kExtNeg in both.
//
// What a later cell reads of a cell is max(S, I, D) (diagonally), max(I, S)
// and D (from the left, where D extends for g and the other two open for
// h + g) and, within the row, I and max(S, D) (from the top, the same with I
// extending): A and D across rows, two scalars within one.
//
// trace[i * stride] receives row i's word.  *cells += the cells of the table
// inside the band.  Returns max(S, I, D) of (w, m): |w - m| <= B is the
// caller's.  Loads t[0 .. w) and P[0 .. m) only.
template <int K>
__host__ __device__ inline int32_t ext_fill(const uint8_t* t, uint32_t w, const uint8_t* P, uint32_t m, uint32_t B,
                                            ExtScores sc, typename ExtWord<K>::type* trace, size_t stride,
                                            uint64_t* cells) {
    typedef typename ExtWord<K>::type Word;
    constexpr int W = 2 * K + 1;
    const int32_t w2 = (int32_t)(2 * B + 1), hg = sc.h + sc.g;
    int32_t A[W], D[W];
    uint32_t pw[W];   // pw[s]: the pattern byte of slot s's column in the coming row
    Word word = 0;
    uint32_t n = 0;
    // row 0: (0, 0) is all zero, (0, j) has I = h + j g alone (algo.rs:195-220)
#pragma unroll
    for (int s = 0; s < W; ++s) {
        const int32_t j = s - (int32_t)B;
        const bool in = s < w2 && j >= 0 && (uint32_t)j <= m;
        A[s] = in ? (j ? sc.h + j * sc.g : 0) : kExtNeg;
        D[s] = in && j == 0 ? 0 : kExtNeg;
        if (in && j) word |= (Word)1 << (2 * s);
        n += in ? 1u : 0u;
        const int32_t j1 = j + 1;   // row 1
        pw[s] = (j1 >= 1 && (uint32_t)j1 <= m) ? P[j1 - 1] : 0u;
    }
    trace[0] = word;
    for (uint32_t i = 1; i <= w; ++i) {
        const uint32_t tb = t[i - 1];
        int32_t cI = kExtNeg, cSD = kExtNeg;   // I and max(S, D) of the cell above (slot s - 1 of this row)
        word = 0;
#pragma unroll
        for (int s = 0; s < W; ++s) {
            const int32_t j = (int32_t)i - (int32_t)B + s;
            int32_t S = kExtNeg, I = kExtNeg, Dv = kExtNeg;
            uint32_t pick = 0;
            const bool in = s < w2 && j >= 0 && (uint32_t)j <= m;
            if (in) {
                if (j == 0) {
                    Dv = sc.h + (int32_t)i * sc.g;   // column 0 (algo.rs:204-211)
                    pick = 2;
                } else {
                    S = (tb == pw[s] ? sc.sm : sc.smm) + ext_max(A[s], D[s]);
                    const int32_t lA = s + 1 < W ? A[s + 1] : kExtNeg, lD = s + 1 < W ? D[s + 1] : kExtNeg;
                    Dv = ext_max(lA + hg, lD + sc.g);
                    I = ext_max(cI + sc.g, cSD + hg);
                    const int32_t M = ext_max(ext_max(S, I), Dv);
                    pick = S == M ? 0u : I == M ? 1u : 2u;   // the first of S, I, D at the maximum (algo.rs:351-400)
                }
                ++n;
            }
            A[s] = ext_max(S, I);
            D[s] = Dv;
            cI = I;
            cSD = ext_max(S, Dv);
            word |= (Word)pick << (2 * s);
        }
        trace[(size_t)i * stride] = word;
        // the window slides by one byte
#pragma unroll
        for (int s = 0; s + 1 < W; ++s) pw[s] = pw[s + 1];
        const int32_t jn = (int32_t)i + 1 - (int32_t)B + (W - 1);
        pw[W - 1] = (i < w && jn >= 1 && (uint32_t)jn <= m) ? P[jn - 1] : 0u;
    }
    *cells += n;
    // (w, m): slot m - w + B of the last row
    const int32_t se = (int32_t)m - (int32_t)w + (int32_t)B;
    int32_t score = kExtNeg;
#pragma unroll
    for (int s = 0; s < W; ++s)
        if (s == se) score = ext_max(A[s], D[s]);
    return score;
}

// retrace (algo.rs:338-422) from (w, m) over the trace words: the labels with
// the reference's shifted is_match(i, j) (s1[i] against s2[j], a missing byte
// equal only to a missing byte) and last_choice for open against extend; a
// diagonal step is an M of the CIGAR, Insert and OpenInsert (a pattern byte)
// an I, Delete and OpenDelete (a text byte) a D.  As the reference, the cell
// it starts in is labelled before it asks whether it is (0, 0): w = m = 0
// gives one Match.  Everything of *rec but the score is written.  EMIT: the
// runs go to run_end[-1], run_end[-2], ..., the walk's first run last, which
// is pattern order.  At most w + m + 1 steps, and a slot outside the band
// ends the walk: neither happens on the words ext_fill wrote.
template <class Word, bool EMIT>
__host__ __device__ inline void ext_walk(const uint8_t* t, uint32_t w, const uint8_t* P, uint32_t m, uint32_t B,
                                         const Word* trace, size_t stride, ExtHit* rec, uint32_t* run_end) {
    uint32_t i = w, j = m, last = 0;   // last: 0 Match or Mismatch, 1 Insert, 2 Delete
    uint32_t steps = 0, mt = 0, mm = 0, og = 0, ge = 0, id = 0, runs = 0, op = 3, len = 0;
    for (;;) {
        const int32_t s = (int32_t)j - (int32_t)i + (int32_t)B;
        if (s < 0 || s > (int32_t)(2 * B) || steps > w + m) break;
        const uint32_t pick = (uint32_t)(trace[(size_t)i * stride] >> (2 * s)) & 3u;
        if (pick == 0) {
            const bool a = i < w, b = j < m;
            if (a == b && (!a || t[i] == P[j])) ++mt; else ++mm;
            if (i && j && t[i - 1] == P[j - 1]) ++id;
            last = 0;
        } else if (pick == 1) {
            if (last == 1) ++ge; else ++og;
            last = 1;
        } else {
            if (last == 2) ++ge; else ++og;
            last = 2;
        }
        ++steps;
        if (pick == op) {
            ++len;
        } else {
            if (len) {
                ++runs;
                if (EMIT) *--run_end = len << 4 | op;
            }
            op = pick;
            len = 1;
        }
        // (checked_sub: an index at 0 stays there)
        if (pick != 1 && i) --i;
        if (pick != 2 && j) --j;
        if (i == 0 && j == 0) break;
    }
    if (len) {
        ++runs;
        if (EMIT) *--run_end = len << 4 | op;
    }
    rec->n_steps = steps;
    rec->matches = mt;
    rec->mismatches = mm;
    rec->opening_gaps = og;
    rec->gap_extensions = ge;
    rec->identities = id;
    rec->cigar_len = runs;
}

// The band width the kernels are built for: the smallest of 2, 4, 8, 15 that holds B.
inline int ext_width_of(uint32_t B) { return B <= 2 ? 2 : B <= 4 ? 4 : B <= 8 ? 8 : 15; }
// ... and the bytes of its trace word.
inline size_t ext_word_bytes(uint32_t B) { return B <= 4 ? 4 : 8; }

// The hits of one launch: hits [h0, h1) of the call, h0 a multiple of 64.  Wave
// v of the call (hits 64 v ..) owns the tile of 64 x rows words at word
// toff[v] - toff[h0 / 64] of trace, rows = its largest w + 1, lane l's row i at
// tile + 64 i + l; words: the words of trace.
struct ExtLaunch {
    const uint8_t* text;        // n bytes (and the index's terminator behind them)
    const uint8_t* pats;
    const uint32_t* offs;       // npat + 1
    const uint32_t* pid;        // per hit: its pattern
    const uint32_t* starts;     // per hit: b
    const uint32_t* ends;       // per hit: e
    const uint64_t* toff;       // per wave of the call, and one behind
    uint32_t h0, h1, B;
    uint64_t words;
    ExtScores sc;
};
// fill: out[h].score and the trace; *cells += the launch's cell updates.
hipError_t launch_ext_fill(const ExtLaunch& L, void* trace, ExtHit* out, unsigned long long* cells, hipStream_t st);
// walk, first pass: the rest of out[h], cnt[h - h0] = its runs, cnt[h1 - h0] = 0, *runs += their sum.
hipError_t launch_ext_walk(const ExtLaunch& L, const void* trace, ExtHit* out, uint32_t* cnt, unsigned long long* runs,
                           hipStream_t st);
// walk, second pass: cnt is its own exclusive scan now and *runs holds every
// run up to and including this launch's, so the launch's first run is run
// *runs - cnt[h1 - h0] of the call.  goffs[h] = the call's run offset of hit h;
// with cigar, a hit whose runs end at or below cap writes them.
hipError_t launch_ext_emit(const ExtLaunch& L, const void* trace, const uint32_t* cnt, const unsigned long long* runs,
                           uint64_t* goffs, uint32_t* cigar, uint64_t cap, hipStream_t st);

}  // namespace gx
