// gx_edit.hip -- k-difference (edit distance) queries on the suffix index, the
// device half of the edit search.  No counterpart in the
// reference.  Pieces, seeds, their 64-bit total and the candidate offsets are
// the k-mismatch search's (gx_approx.hip, gx_search.hip); behind them:
//
//   verify   a lane per candidate (one suffix-array entry of one piece's
//            interval): Sellers' recurrence on the 2k + 1 diagonals around the
//            one the seed lies on (edit_band, gx_edit.h), the band in
//            registers, one instantiation per band width (k <= 1, 2, 4, 8);
//            what row m reports as a slot mask and a nibble per slot, their
//            number, and the 64-bit sums of reported ends and cell updates
//   emit     a lane per candidate: (pattern << 32 | end, distance) for every
//            reported end, at the scan of the numbers.  The stable radix pass
//            of gx_suffix.hip then sorts them by key
//   heads    a lane per sorted entry: run heads, the minimum distance over the
//            head's run, an atomic minimum of (distance, end) per pattern
//   fill     a lane per pattern: count, candidates, best, min(count, max_hits)
//   scatter  a lane per sorted entry: the heads below max_hits into the packed
//            arrays, ascending by end as the sort left them
//   starts   a lane per reported occurrence: the anchored band of the reversed
//            pattern against the text read backwards from the end (edit_start)
//
// As gx_approx.hip: 256-thread workgroups, no kernel waits on another
// workgroup, every device-wide dependency is a kernel boundary.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gx_edit.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
constexpr int kWaves = kB / 64;
constexpr unsigned kStrideGrid = 2048;   // workgroups of the striding kernels at most
typedef unsigned long long u64;

// The sum of v over the workgroup, in thread 0.
__device__ inline u64 block_sum(u64 v, u64* sh) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();   // (sh may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += sh[q];
    }
    return s;
}

// The first i < n with a[(i + 1) * step] > g (a[n * step] > g: the caller's).
__device__ inline uint32_t seg_of(const uint32_t* __restrict__ a, uint32_t n, uint32_t step, uint32_t g) {
    uint32_t L = 0, R = n;
    while (L < R) {
        const uint32_t mid = L + (R - L) / 2;
        if (a[(u64)(mid + 1) * step] <= g) L = mid + 1; else R = mid;
    }
    return L;
}

// Candidate g: its pattern p (offset o, m bytes) and the diagonal d0 its seed
// lies on.  false: no such piece, a corrupt array entry, or a diagonal no
// window inside the text lies on.
struct Cand {
    uint32_t p, o, m;
    int32_t d0;
};
__device__ inline bool cand_of(const uint32_t* __restrict__ sa, uint32_t N, const uint32_t* __restrict__ offs,
                               const uint32_t* __restrict__ poffs, const SrchHit* __restrict__ phits,
                               const uint32_t* __restrict__ coffs, uint32_t npieces, uint32_t k, uint32_t g, Cand* c) {
    const uint32_t k1 = k + 1, n = N - 1;
    const uint32_t piece = seg_of(coffs, npieces, 1, g);
    if (piece >= npieces) return false;
    c->p = piece / k1;
    c->o = offs[c->p];
    c->m = offs[c->p + 1] - c->o;
    const u64 r = (u64)phits[piece].lo + (g - coffs[piece]);
    if (r >= N) return false;
    const uint32_t at = sa[r];
    if (at >= N) return false;
    const int64_t d0 = (int64_t)at - (int64_t)(poffs[piece] - c->o);
    if (!edit_diag_ok(d0, n, c->m, k)) return false;
    c->d0 = (int32_t)d0;
    return true;
}

template <int K>
__global__ __launch_bounds__(kB) void edit_verify_kernel(const uint8_t* __restrict__ text,
                                                         const uint32_t* __restrict__ sa, uint32_t N,
                                                         const uint8_t* __restrict__ pats,
                                                         const uint32_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ poffs,
                                                         const SrchHit* __restrict__ phits,
                                                         const uint32_t* __restrict__ coffs, uint32_t npieces,
                                                         uint32_t k, uint32_t total, uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ rep, uint64_t* __restrict__ nib,
                                                         u64* ends_total, u64* cells_total) {
    __shared__ u64 sh[kWaves];
    uint64_t cells = 0, ends = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[total] = 0;   // the scan's last entry: the ends before dedupe
    for (u64 g64 = (u64)blockIdx.x * kB + threadIdx.x; g64 < total; g64 += (u64)gridDim.x * kB) {
        const uint32_t g = (uint32_t)g64;
        Cand c;
        uint32_t mk = 0, q = 0;
        uint64_t nb = 0;
        if (cand_of(sa, N, offs, poffs, phits, coffs, npieces, k, g, &c))
            q = edit_band<K>(text, N - 1, pats + c.o, c.m, k, c.d0, &mk, &nb, &cells);
        cnt[g] = q;
        rep[g] = mk;
        nib[g] = nb;
        ends += q;
    }
    const u64 s = block_sum(cells, sh);
    if (threadIdx.x == 0 && s) atomicAdd(cells_total, s);
    const u64 e = block_sum(ends, sh);
    if (threadIdx.x == 0 && e) atomicAdd(ends_total, e);
}

__global__ __launch_bounds__(kB) void edit_emit_kernel(const uint32_t* __restrict__ sa, uint32_t N,
                                                       const uint32_t* __restrict__ offs,
                                                       const uint32_t* __restrict__ poffs,
                                                       const SrchHit* __restrict__ phits,
                                                       const uint32_t* __restrict__ coffs, uint32_t npieces, uint32_t k,
                                                       uint32_t total, const uint32_t* __restrict__ eoffs,
                                                       const uint32_t* __restrict__ rep,
                                                       const uint64_t* __restrict__ nib, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ vals) {
    const uint32_t E = eoffs[total];
    for (u64 g64 = (u64)blockIdx.x * kB + threadIdx.x; g64 < total; g64 += (u64)gridDim.x * kB) {
        const uint32_t g = (uint32_t)g64;
        const uint32_t mk = rep[g];
        if (!(mk & 0x1FFFFu)) continue;
        Cand c;
        if (!cand_of(sa, N, offs, poffs, phits, coffs, npieces, k, g, &c)) continue;   // (never: it reported)
        const uint64_t nb = nib[g];
        u64 o = eoffs[g];
        const int32_t c0 = (int32_t)c.m + c.d0 - (int32_t)k;   // slot s of row m: the end c0 + s, in [0, n]
        for (uint32_t s = 0; s < 2 * k + 1; ++s) {
            if (!((mk >> s) & 1u)) continue;
            if (o < E) {   // (always, while eoffs is the scan of this launch's numbers)
                keys[o] = (u64)c.p << 32 | (uint32_t)(c0 + (int32_t)s);
                vals[o] = edit_slot_dist(mk, nb, s);
            }
            ++o;
        }
    }
}

__global__ __launch_bounds__(kB) void edit_heads_kernel(const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ vals, uint32_t E, uint32_t k,
                                                        uint32_t* __restrict__ head, uint32_t* __restrict__ dmin,
                                                        u64* best) {
    if (blockIdx.x == 0 && threadIdx.x == 0) head[E] = 0;   // the scan's last entry: the number of heads
    const uint32_t bound = edit_run_bound(k);
    // (the bound is the workgroup's, not the lane's: every lane of a wave reaches the shuffles below)
    for (u64 base = (u64)blockIdx.x * kB; base < E; base += (u64)gridDim.x * kB) {
        const u64 i = base + threadIdx.x;
        uint32_t p = 0xFFFFFFFFu;
        u64 bk = ~0ull;
        if (i < E) {
            const u64 key = keys[i];
            const bool h = i == 0 || keys[i - 1] != key;
            uint32_t d = 0;
            if (h) {
                d = edit_run_min(keys, vals, i, E, bound);
                p = (uint32_t)(key >> 32);
                bk = (u64)d << 32 | (uint32_t)key;
            }
            head[i] = h ? 1u : 0u;
            dmin[i] = d;
        }
        // one atomic a wave where all its heads share a pattern (a pattern with many occurrences)
        const u64 any = __ballot(bk != ~0ull);
        if (!any) continue;
        const uint32_t p0 = __shfl(p, __ffsll((long long)any) - 1, 64);
        if (__all(bk == ~0ull || p == p0)) {
            u64 v = bk;
#pragma unroll
            for (int s = 32; s; s >>= 1) {
                const u64 o = __shfl_xor(v, s, 64);
                v = o < v ? o : v;
            }
            if ((threadIdx.x & 63) == 0) atomicMin(best + p0, v);
        } else if (bk != ~0ull) {
            atomicMin(best + p, bk);
        }
    }
}

// The first i < E with keys[i] >= key.
__device__ inline uint32_t lower_key(const uint64_t* __restrict__ keys, uint32_t E, u64 key) {
    uint32_t L = 0, R = E;
    while (L < R) {
        const uint32_t mid = L + (R - L) / 2;
        if (keys[mid] < key) L = mid + 1; else R = mid;
    }
    return L;
}

__global__ __launch_bounds__(kB) void edit_fill_kernel(const uint64_t* __restrict__ keys,
                                                       const uint32_t* __restrict__ hscan, uint32_t E,
                                                       const uint32_t* __restrict__ coffs,
                                                       const u64* __restrict__ best, uint32_t npat, uint32_t k1,
                                                       uint32_t max_hits, EditHit* __restrict__ hits,
                                                       uint32_t* __restrict__ hbase, uint32_t* __restrict__ oq) {
    const u64 p = (u64)blockIdx.x * kB + threadIdx.x;
    if (p > npat) return;
    if (p == npat) {
        oq[p] = 0;
        return;
    }
    const uint32_t lo = lower_key(keys, E, p << 32), hi = lower_key(keys, E, (p + 1) << 32);
    EditHit h;
    h.count = hscan[hi] - hscan[lo];
    h.candidates = coffs[(p + 1) * k1] - coffs[p * k1];
    const u64 b = best[p];
    h.best_dist = h.count ? (uint32_t)(b >> 32) : 0xFFFFFFFFu;
    h.best_end = h.count ? (uint32_t)b : 0u;
    hits[p] = h;
    hbase[p] = hscan[lo];
    oq[p] = h.count < max_hits ? h.count : max_hits;
}

__global__ __launch_bounds__(kB) void edit_scatter_kernel(const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ dmin,
                                                          const uint32_t* __restrict__ hscan, uint32_t E,
                                                          const uint32_t* __restrict__ hbase,
                                                          const uint32_t* __restrict__ ooffs, uint32_t npat,
                                                          uint32_t max_hits, uint32_t* __restrict__ ends,
                                                          uint8_t* __restrict__ distances, u64 cap) {
    if (ooffs[npat] > cap) return;   // (the driver reports GX_ECAP)
    for (u64 i = (u64)blockIdx.x * kB + threadIdx.x; i < E; i += (u64)gridDim.x * kB) {
        const uint32_t rank_all = hscan[i];
        if (hscan[i + 1] == rank_all) continue;   // not a head
        const u64 key = keys[i];
        const uint32_t p = (uint32_t)(key >> 32);
        if (p >= npat) continue;
        const uint32_t rank = rank_all - hbase[p];
        if (rank >= max_hits) continue;
        const u64 o = (u64)ooffs[p] + rank;
        if (o >= cap) continue;   // (never: ooffs[npat] <= cap)
        ends[o] = (uint32_t)key;
        distances[o] = (uint8_t)dmin[i];
    }
}

template <int K>
__global__ __launch_bounds__(kB) void edit_starts_kernel(const uint8_t* __restrict__ text,
                                                         const uint8_t* __restrict__ pats,
                                                         const uint32_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ ooffs, uint32_t npat, uint32_t k,
                                                         const uint32_t* __restrict__ ends,
                                                         const uint8_t* __restrict__ distances,
                                                         uint32_t* __restrict__ starts, u64 cap) {
    const uint32_t tot = ooffs[npat];
    if (tot > cap) return;   // (the driver reports GX_ECAP: nothing was scattered)
    uint64_t cells = 0;      // (the verify launch's are the work measure: not summed here)
    for (u64 o64 = (u64)blockIdx.x * kB + threadIdx.x; o64 < tot; o64 += (u64)gridDim.x * kB) {
        const uint32_t o = (uint32_t)o64;
        const uint32_t p = seg_of(ooffs, npat, 1, o);
        if (p >= npat) continue;
        const uint32_t po = offs[p], m = offs[p + 1] - po;
        starts[o] = edit_start<K>(text, ends[o], pats + po, m, k, distances[o], &cells);
    }
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + kB - 1) / kB); }
inline unsigned stride_grid(u64 n) { return std::max(1u, std::min(kStrideGrid, blocks_of(n))); }

}  // namespace

hipError_t launch_edit_verify(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* pats,
                              const uint32_t* offs, const uint32_t* poffs, const SrchHit* phits, const uint32_t* coffs,
                              uint32_t npieces, uint32_t k, uint32_t total, uint32_t* cnt, uint32_t* rep, uint64_t* nib,
                              unsigned long long* ends, unsigned long long* cells, hipStream_t st) {
#define GX_EDIT_VERIFY(K)                                                                                              \
    hipLaunchKernelGGL(edit_verify_kernel<K>, dim3(stride_grid(total)), dim3(kB), 0, st, text, sa, N, pats, offs,     \
                       poffs, phits, coffs, npieces, k, total, cnt, rep, nib, ends, cells)
    switch (edit_width_of(k)) {
        case 1: GX_EDIT_VERIFY(1); break;
        case 2: GX_EDIT_VERIFY(2); break;
        case 4: GX_EDIT_VERIFY(4); break;
        default: GX_EDIT_VERIFY(8); break;
    }
#undef GX_EDIT_VERIFY
    return hipGetLastError();
}

hipError_t launch_edit_emit(const uint32_t* sa, uint32_t N, const uint32_t* offs, const uint32_t* poffs,
                            const SrchHit* phits, const uint32_t* coffs, uint32_t npieces, uint32_t k, uint32_t total,
                            const uint32_t* eoffs, const uint32_t* rep, const uint64_t* nib, uint64_t* keys,
                            uint32_t* vals, hipStream_t st) {
    hipLaunchKernelGGL(edit_emit_kernel, dim3(stride_grid(total)), dim3(kB), 0, st, sa, N, offs, poffs, phits, coffs,
                       npieces, k, total, eoffs, rep, nib, keys, vals);
    return hipGetLastError();
}

hipError_t launch_edit_heads(const uint64_t* keys, const uint32_t* vals, uint32_t E, uint32_t k, uint32_t* head,
                             uint32_t* dmin, unsigned long long* best, hipStream_t st) {
    hipLaunchKernelGGL(edit_heads_kernel, dim3(stride_grid(E)), dim3(kB), 0, st, keys, vals, E, k, head, dmin, best);
    return hipGetLastError();
}

hipError_t launch_edit_fill(const uint64_t* keys, const uint32_t* hscan, uint32_t E, const uint32_t* coffs,
                            const unsigned long long* best, uint32_t npat, uint32_t k1, uint32_t max_hits,
                            EditHit* hits, uint32_t* hbase, uint32_t* oq, hipStream_t st) {
    hipLaunchKernelGGL(edit_fill_kernel, dim3(blocks_of((u64)npat + 1)), dim3(kB), 0, st, keys, hscan, E, coffs, best,
                       npat, k1, max_hits, hits, hbase, oq);
    return hipGetLastError();
}

hipError_t launch_edit_scatter(const uint64_t* keys, const uint32_t* dmin, const uint32_t* hscan, uint32_t E,
                               const uint32_t* hbase, const uint32_t* ooffs, uint32_t npat, uint32_t max_hits,
                               uint32_t* ends, uint8_t* distances, uint64_t cap, hipStream_t st) {
    hipLaunchKernelGGL(edit_scatter_kernel, dim3(stride_grid(E)), dim3(kB), 0, st, keys, dmin, hscan, E, hbase, ooffs,
                       npat, max_hits, ends, distances, (u64)cap);
    return hipGetLastError();
}

hipError_t launch_edit_starts(const uint8_t* text, const uint8_t* pats, const uint32_t* offs, const uint32_t* ooffs,
                              uint32_t npat, uint32_t k, const uint32_t* ends, const uint8_t* distances,
                              uint32_t* starts, uint64_t cap, hipStream_t st) {
    const unsigned grid = stride_grid(cap);
#define GX_EDIT_STARTS(K)                                                                                              \
    hipLaunchKernelGGL(edit_starts_kernel<K>, dim3(grid), dim3(kB), 0, st, text, pats, offs, ooffs, npat, k, ends,    \
                       distances, starts, (u64)cap)
    switch (edit_width_of(k)) {
        case 1: GX_EDIT_STARTS(1); break;
        case 2: GX_EDIT_STARTS(2); break;
        case 4: GX_EDIT_STARTS(4); break;
        default: GX_EDIT_STARTS(8); break;
    }
#undef GX_EDIT_STARTS
    return hipGetLastError();
}

}  // namespace gx
