// gx_extend.hip -- banded affine-gap alignment of reported hits on the suffix
// index, the device half of gx_suffix_index_extend.  The
// recurrence and the retrace are the reference's (algo.rs:151-441), restated on
// the band in gx_extend.h; the batching has no counterpart there.
//
//   fill   a lane per hit: the rows of ext_fill with the band in registers by
//          diagonal slot, one instantiation per band width (B <= 2, 4, 8, 15),
//          a trace word a row into the wave's tile (64 lanes side by side, so
//          a row of the wave is one coalesced store), the score, and the
//          64-bit sum of the cell updates
//   walk   a lane per hit over its own trace words: the record and the number
//          of runs, and the 64-bit sum of those
//   emit   a lane per hit, behind the scan of the numbers: the hit's run offset
//          and, where asked for, the same walk again writing the runs from the
//          tail of the hit's slice backwards
//
// 256-thread workgroups, no LDS, no kernel waits on another workgroup; the sums
// are one vector atomic a wave.
#include <hip/hip_runtime.h>

#include "gx_extend.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
typedef unsigned long long u64;

// *total += the sum of v over the wave (every lane of the wave calls it).
__device__ inline void wave_add(u64 v, u64* total) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, v);
}

// Hit g of the call, h0 <= g < h1: window and pattern, and its lane's first
// word in the launch's trace.  false (never, on what the driver staged): the
// lane's rows would leave the trace.
struct Hit {
    const uint8_t *t, *P;
    uint32_t w, m;
    u64 at;
};
__device__ inline bool hit_of(const ExtLaunch& L, uint32_t g, Hit* h) {
    const uint32_t p = L.pid[g], o = L.offs[p], b = L.starts[g];
    h->t = L.text + b;
    h->w = L.ends[g] - b;
    h->P = L.pats + o;
    h->m = L.offs[p + 1] - o;
    h->at = L.toff[g >> 6] - L.toff[L.h0 >> 6] + (g & 63u);
    return h->at + 64ull * h->w < L.words;
}

template <int K>
__global__ __launch_bounds__(kB) void ext_fill_kernel(ExtLaunch L, typename ExtWord<K>::type* __restrict__ trace,
                                                      ExtHit* __restrict__ out, u64* cells_total) {
    const u64 g = (u64)L.h0 + (u64)blockIdx.x * kB + threadIdx.x;
    uint64_t cells = 0;
    if (g < L.h1) {
        Hit h;
        int32_t score = kExtNeg;
        if (hit_of(L, (uint32_t)g, &h)) score = ext_fill<K>(h.t, h.w, h.P, h.m, L.B, L.sc, trace + h.at, 64, &cells);
        out[g].score = score;
    }
    wave_add(cells, cells_total);
}

template <class Word>
__global__ __launch_bounds__(kB) void ext_walk_kernel(ExtLaunch L, const Word* __restrict__ trace,
                                                      ExtHit* __restrict__ out, uint32_t* __restrict__ cnt,
                                                      u64* runs_total) {
    const u64 g = (u64)L.h0 + (u64)blockIdx.x * kB + threadIdx.x;
    uint64_t runs = 0;
    if (g == L.h1) cnt[g - L.h0] = 0;   // the scan's last entry: the launch's runs
    if (g < L.h1) {
        Hit h;
        ExtHit r{};
        if (hit_of(L, (uint32_t)g, &h)) ext_walk<Word, false>(h.t, h.w, h.P, h.m, L.B, trace + h.at, 64, &r, nullptr);
        ExtHit* o = out + g;   // (the score is the fill's)
        o->n_steps = r.n_steps;
        o->matches = r.matches;
        o->mismatches = r.mismatches;
        o->opening_gaps = r.opening_gaps;
        o->gap_extensions = r.gap_extensions;
        o->identities = r.identities;
        o->cigar_len = r.cigar_len;
        cnt[g - L.h0] = r.cigar_len;
        runs = r.cigar_len;
    }
    wave_add(runs, runs_total);
}

template <class Word>
__global__ __launch_bounds__(kB) void ext_emit_kernel(ExtLaunch L, const Word* __restrict__ trace,
                                                      const uint32_t* __restrict__ cnt, const u64* runs_total,
                                                      uint64_t* __restrict__ goffs, uint32_t* __restrict__ cigar,
                                                      u64 cap) {
    const u64 g = (u64)L.h0 + (u64)blockIdx.x * kB + threadIdx.x;
    if (g > L.h1) return;
    const uint32_t nl = L.h1 - L.h0, l = (uint32_t)(g - L.h0);
    const u64 o = *runs_total - cnt[nl] + cnt[l];
    goffs[g] = o;   // (g = h1: the next launch's first hit, or the call's total)
    if (g == L.h1 || !cigar) return;
    const uint32_t len = cnt[l + 1] - cnt[l];
    if (o + len > cap) return;   // (the driver reports GX_ECAP)
    Hit h;
    ExtHit r;
    if (hit_of(L, (uint32_t)g, &h)) ext_walk<Word, true>(h.t, h.w, h.P, h.m, L.B, trace + h.at, 64, &r, cigar + o + len);
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + kB - 1) / kB); }

}  // namespace

hipError_t launch_ext_fill(const ExtLaunch& L, void* trace, ExtHit* out, unsigned long long* cells, hipStream_t st) {
#define GX_EXT_FILL(K)                                                                                       \
    hipLaunchKernelGGL(ext_fill_kernel<K>, dim3(blocks_of(L.h1 - L.h0)), dim3(kB), 0, st, L,                 \
                       (typename ExtWord<K>::type*)trace, out, cells)
    switch (ext_width_of(L.B)) {
        case 2: GX_EXT_FILL(2); break;
        case 4: GX_EXT_FILL(4); break;
        case 8: GX_EXT_FILL(8); break;
        default: GX_EXT_FILL(15); break;
    }
#undef GX_EXT_FILL
    return hipGetLastError();
}

hipError_t launch_ext_walk(const ExtLaunch& L, const void* trace, ExtHit* out, uint32_t* cnt, unsigned long long* runs,
                           hipStream_t st) {
    const dim3 grid(blocks_of((u64)(L.h1 - L.h0) + 1));
    if (ext_word_bytes(L.B) == 4)
        hipLaunchKernelGGL(ext_walk_kernel<uint32_t>, grid, dim3(kB), 0, st, L, (const uint32_t*)trace, out, cnt, runs);
    else
        hipLaunchKernelGGL(ext_walk_kernel<uint64_t>, grid, dim3(kB), 0, st, L, (const uint64_t*)trace, out, cnt, runs);
    return hipGetLastError();
}

hipError_t launch_ext_emit(const ExtLaunch& L, const void* trace, const uint32_t* cnt, const unsigned long long* runs,
                           uint64_t* goffs, uint32_t* cigar, uint64_t cap, hipStream_t st) {
    const dim3 grid(blocks_of((u64)(L.h1 - L.h0) + 1));
    if (ext_word_bytes(L.B) == 4)
        hipLaunchKernelGGL(ext_emit_kernel<uint32_t>, grid, dim3(kB), 0, st, L, (const uint32_t*)trace, cnt, runs, goffs,
                           cigar, (u64)cap);
    else
        hipLaunchKernelGGL(ext_emit_kernel<uint64_t>, grid, dim3(kB), 0, st, L, (const uint64_t*)trace, cnt, runs, goffs,
                           cigar, (u64)cap);
    return hipGetLastError();
}

}  // namespace gx
