// gx_approx.hip -- k-mismatch queries on the suffix index, the device half of
// the approximate search.  No counterpart in the reference.
//
//   pieces   a lane per piece: where each of a pattern's k + 1 pieces starts in
//            the packed patterns.  The interval kernel of gx_search.hip then
//            runs over the pieces as its patterns: a piece in the middle of a
//            pattern is followed by the next piece's bytes, which srch_cmp
//            reads in its last word and masks, as it masks the padding behind
//            the last pattern.
//   total    the pieces' interval sizes summed in 64 bits, so that the host
//            can refuse a batch before their 32-bit scan is relied upon
//   verify   a lane per candidate (one suffix-array entry of one piece's
//            interval): the window it implies, walked 8 bytes a step
//            (aprx_verify, gx_approx.h); a keep flag, the distance, the start,
//            and an atomic minimum of (distance, start) per pattern
//   fill     a lane per pattern: count, candidates, best, min(count, max_hits)
//   scatter  a lane per candidate: the kept ones below max_hits into the packed
//            arrays, in candidate order
//
// As gx_search.hip: 256-thread workgroups, no kernel waits on another
// workgroup, every device-wide dependency is a kernel boundary.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gx_approx.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
constexpr int kWaves = kB / 64;
constexpr unsigned kStrideGrid = 2048;   // workgroups of verify and scatter at most; they stride over the rest
typedef unsigned long long u64;

// The sum of v over the workgroup, in thread 0.
__device__ inline u64 block_sum(u64 v, u64* sh) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += sh[q];
    }
    return s;
}

__global__ __launch_bounds__(kB) void aprx_pieces_kernel(const uint32_t* __restrict__ offs, uint32_t npat, uint32_t k1,
                                                         uint32_t* __restrict__ poffs) {
    const u64 i = (u64)blockIdx.x * kB + threadIdx.x;
    const u64 npieces = (u64)npat * k1;
    if (i > npieces) return;
    if (i == npieces) {
        poffs[i] = offs[npat];
        return;
    }
    const uint32_t p = (uint32_t)(i / k1), j = (uint32_t)(i % k1);
    const uint32_t o = offs[p], e = offs[p + 1];
    poffs[i] = o + aprx_piece_start(e > o ? e - o : 0, k1, j);
}

__global__ __launch_bounds__(kB) void aprx_total_kernel(const SrchHit* __restrict__ phits, uint32_t npieces,
                                                        u64* total) {
    __shared__ u64 sh[kWaves];
    const u64 i = (u64)blockIdx.x * kB + threadIdx.x;
    const u64 s = block_sum(i < npieces ? phits[i].count : 0u, sh);
    if (threadIdx.x == 0 && s) atomicAdd(total, s);
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

__global__ __launch_bounds__(kB) void aprx_verify_kernel(const uint8_t* __restrict__ text,
                                                         const uint32_t* __restrict__ sa, uint32_t N,
                                                         const uint8_t* __restrict__ pats,
                                                         const uint32_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ poffs,
                                                         const SrchHit* __restrict__ phits,
                                                         const uint32_t* __restrict__ coffs, uint32_t npieces,
                                                         uint32_t k, uint32_t total, uint32_t* __restrict__ keep,
                                                         uint8_t* __restrict__ dist, uint32_t* __restrict__ start,
                                                         u64* best, u64* words_total) {
    __shared__ u64 sh[kWaves];
    const uint32_t k1 = k + 1, n = N - 1;
    uint64_t words = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) keep[total] = 0;   // the scan's last entry: the number kept
    // (the bound is the workgroup's, not the lane's: every lane of a wave reaches the shuffles below)
    for (u64 base = (u64)blockIdx.x * kB; base < total; base += (u64)gridDim.x * kB) {
        const u64 g64 = base + threadIdx.x;
        uint32_t p = 0xFFFFFFFFu;
        u64 key = ~0ull;
        if (g64 < total) {
            const uint32_t g = (uint32_t)g64;
            const uint32_t piece = seg_of(coffs, npieces, 1, g);
            uint32_t kept = 0, d = 0, c = 0;
            if (piece < npieces) {
                p = piece / k1;
                const uint32_t j = piece - p * k1;
                const uint32_t o = offs[p], m = offs[p + 1] - o;
                const u64 r = (u64)phits[piece].lo + (g - coffs[piece]);
                const uint32_t at = r < N ? sa[r] : N;       // (a corrupt entry: rejected below)
                const uint32_t ps = poffs[piece] - o;        // the piece's start within the pattern
                // the window [at - ps, at - ps + m) must lie inside the n text bytes: never over '$'
                if (at >= ps && (u64)(at - ps) + m <= n) {
                    c = at - ps;
                    if (aprx_verify(text + c, pats + o, m, k, j, &d, &words)) {
                        kept = 1;
                        key = (u64)d << 32 | c;
                    }
                }
            }
            keep[g] = kept;
            dist[g] = (uint8_t)d;
            start[g] = c;
        }
        // one atomic a wave where all its lanes share a pattern (a pattern with many candidates)
        const uint32_t p0 = __shfl(p, 0, 64);
        if (__all(p == p0)) {
            u64 v = key;
#pragma unroll
            for (int s = 32; s; s >>= 1) {
                const u64 o = __shfl_xor(v, s, 64);
                v = o < v ? o : v;
            }
            if ((threadIdx.x & 63) == 0 && v != ~0ull) atomicMin(best + p0, v);
        } else if (key != ~0ull) {
            atomicMin(best + p, key);
        }
    }
    const u64 s = block_sum(words, sh);
    if (threadIdx.x == 0 && s) atomicAdd(words_total, s);
}

__global__ __launch_bounds__(kB) void aprx_fill_kernel(const uint32_t* __restrict__ coffs,
                                                       const uint32_t* __restrict__ kscan,
                                                       const u64* __restrict__ best, uint32_t npat, uint32_t k1,
                                                       uint32_t max_hits, AprxHit* __restrict__ hits,
                                                       uint32_t* __restrict__ oq) {
    const u64 p = (u64)blockIdx.x * kB + threadIdx.x;
    if (p > npat) return;
    if (p == npat) {
        oq[p] = 0;
        return;
    }
    const uint32_t c0 = coffs[p * k1], c1 = coffs[(p + 1) * k1];
    AprxHit h;
    h.count = kscan[c1] - kscan[c0];
    h.candidates = c1 - c0;
    const u64 b = best[p];
    h.best_dist = h.count ? (uint32_t)(b >> 32) : 0xFFFFFFFFu;
    h.best_pos = h.count ? (uint32_t)b : 0u;
    hits[p] = h;
    oq[p] = h.count < max_hits ? h.count : max_hits;
}

__global__ __launch_bounds__(kB) void aprx_scatter_kernel(const uint32_t* __restrict__ coffs,
                                                          const uint32_t* __restrict__ kscan,
                                                          const uint32_t* __restrict__ ooffs, uint32_t npat,
                                                          uint32_t k1, uint32_t total, uint32_t max_hits,
                                                          const uint32_t* __restrict__ start,
                                                          const uint8_t* __restrict__ dist,
                                                          uint32_t* __restrict__ positions,
                                                          uint8_t* __restrict__ distances, u64 cap) {
    if (ooffs[npat] > cap) return;   // (the driver reports GX_ECAP)
    for (u64 g64 = (u64)blockIdx.x * kB + threadIdx.x; g64 < total; g64 += (u64)gridDim.x * kB) {
        const uint32_t g = (uint32_t)g64;
        const uint32_t rank_all = kscan[g];
        if (kscan[g + 1] == rank_all) continue;   // not kept
        const uint32_t p = seg_of(coffs, npat, k1, g);
        if (p >= npat) continue;
        const uint32_t rank = rank_all - kscan[coffs[(u64)p * k1]];
        if (rank >= max_hits) continue;
        const u64 o = (u64)ooffs[p] + rank;
        if (o >= cap) continue;   // (never: ooffs[npat] <= cap)
        positions[o] = start[g];
        distances[o] = dist[g];
    }
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + kB - 1) / kB); }
inline unsigned stride_grid(u64 n) { return std::max(1u, std::min(kStrideGrid, blocks_of(n))); }

}  // namespace

hipError_t launch_aprx_pieces(const uint32_t* offs, uint32_t npat, uint32_t k1, uint32_t* poffs, hipStream_t st) {
    hipLaunchKernelGGL(aprx_pieces_kernel, dim3(blocks_of((u64)npat * k1 + 1)), dim3(kB), 0, st, offs, npat, k1, poffs);
    return hipGetLastError();
}

hipError_t launch_aprx_total(const SrchHit* phits, uint32_t npieces, unsigned long long* total, hipStream_t st) {
    hipLaunchKernelGGL(aprx_total_kernel, dim3(std::max(1u, blocks_of(npieces))), dim3(kB), 0, st, phits, npieces,
                       total);
    return hipGetLastError();
}

hipError_t launch_aprx_verify(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* pats,
                              const uint32_t* offs, const uint32_t* poffs, const SrchHit* phits,
                              const uint32_t* coffs, uint32_t npieces, uint32_t k, uint32_t total, uint32_t* keep,
                              uint8_t* dist, uint32_t* start, unsigned long long* best, unsigned long long* words,
                              hipStream_t st) {
    hipLaunchKernelGGL(aprx_verify_kernel, dim3(stride_grid(total)), dim3(kB), 0, st, text, sa, N, pats, offs, poffs,
                       phits, coffs, npieces, k, total, keep, dist, start, best, words);
    return hipGetLastError();
}

hipError_t launch_aprx_fill(const uint32_t* coffs, const uint32_t* kscan, const unsigned long long* best,
                            uint32_t npat, uint32_t k1, uint32_t max_hits, AprxHit* hits, uint32_t* oq,
                            hipStream_t st) {
    hipLaunchKernelGGL(aprx_fill_kernel, dim3(blocks_of((u64)npat + 1)), dim3(kB), 0, st, coffs, kscan, best, npat, k1,
                       max_hits, hits, oq);
    return hipGetLastError();
}

hipError_t launch_aprx_scatter(const uint32_t* coffs, const uint32_t* kscan, const uint32_t* ooffs, uint32_t npat,
                               uint32_t k1, uint32_t total, uint32_t max_hits, const uint32_t* start,
                               const uint8_t* dist, uint32_t* positions, uint8_t* distances, uint64_t cap,
                               hipStream_t st) {
    hipLaunchKernelGGL(aprx_scatter_kernel, dim3(stride_grid(total)), dim3(kB), 0, st, coffs, kscan, ooffs, npat, k1,
                       total, max_hits, start, dist, positions, distances, (u64)cap);
    return hipGetLastError();
}

}  // namespace gx
