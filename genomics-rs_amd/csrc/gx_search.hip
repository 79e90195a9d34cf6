// gx_search.hip -- exact-match queries on the suffix array of t = s + '$', the
// device half of search mode.  No counterpart in the reference.
//
//   range    a lane per pattern: the interval of SA whose suffixes have the
//            pattern as a prefix, by binary search, 8 bytes a compare step
//            (srch_one, gx_search.h), and the longest prefix that occurs
//   clamp    min(count, max_hits) per pattern, what the scan turns into offsets
//   gather   a lane per reported position: SA[lo + r] into the packed array,
//            the pattern found by a search over the offsets, so a pattern with
//            a million hits spreads over as many lanes as a million with one
//
// As gx_suffix.hip: 256-thread workgroups, no kernel waits on another
// workgroup, every device-wide dependency is a kernel boundary.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gx_search.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
constexpr int kWaves = kB / 64;
constexpr unsigned kGatherGrid = 2048;   // workgroups of the gather at most; they stride over the rest
typedef unsigned long long u64;

__global__ __launch_bounds__(kB) void srch_range_kernel(const uint8_t* __restrict__ text,
                                                        const uint32_t* __restrict__ sa, uint32_t N,
                                                        const uint8_t* __restrict__ pats,
                                                        const uint32_t* __restrict__ offs, uint32_t npat,
                                                        SrchHit* __restrict__ hits, u64* words_total) {
    __shared__ u64 sh[kWaves];
    const u64 p = (u64)blockIdx.x * kB + threadIdx.x;
    uint64_t words = 0;
    if (p < npat) {
        const uint32_t o = offs[p], e = offs[p + 1];
        uint32_t m = e > o ? e - o : 0;
        if (m > kSrchMaxPattern) m = kSrchMaxPattern;   // (the driver refuses these: a lane's work stays bounded)
        hits[p] = srch_one(text, sa, N, pats + o, m, &words);
    }
    u64 w = words;
#pragma unroll
    for (int d = 32; d; d >>= 1) w += __shfl_xor(w, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += sh[q];
        if (s) atomicAdd(words_total, s);
    }
}

__global__ __launch_bounds__(kB) void srch_clamp_kernel(const SrchHit* __restrict__ hits, uint32_t npat,
                                                        uint32_t max_hits, uint32_t* __restrict__ q) {
    const u64 p = (u64)blockIdx.x * kB + threadIdx.x;
    if (p > npat) return;
    uint32_t c = 0;
    if (p < npat) {
        c = hits[p].count;
        if (c > max_hits) c = max_hits;
    }
    q[p] = c;
}

__global__ __launch_bounds__(kB) void srch_gather_kernel(const uint32_t* __restrict__ sa, uint32_t N,
                                                         const SrchHit* __restrict__ hits,
                                                         const uint32_t* __restrict__ offs, uint32_t npat,
                                                         uint32_t* __restrict__ positions, u64 cap) {
    const u64 total = offs[npat];
    if (total > cap) return;   // (the driver reports GX_ECAP)
    for (u64 j = (u64)blockIdx.x * kB + threadIdx.x; j < total; j += (u64)gridDim.x * kB) {
        uint32_t L = 0, R = npat;   // -> the first p with offs[p + 1] > j (offs[npat] = total > j)
        while (L < R) {
            const uint32_t mid = L + (R - L) / 2;
            if (offs[mid + 1] <= j) L = mid + 1; else R = mid;
        }
        if (L >= npat) continue;
        const u64 k = (u64)hits[L].lo + (j - offs[L]);
        positions[j] = k < N ? sa[k] : 0u;
    }
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + kB - 1) / kB); }

}  // namespace

hipError_t launch_srch_range(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* pats,
                             const uint32_t* offs, uint32_t npat, SrchHit* hits, unsigned long long* words,
                             hipStream_t st) {
    hipLaunchKernelGGL(srch_range_kernel, dim3(blocks_of(npat)), dim3(kB), 0, st, text, sa, N, pats, offs, npat, hits,
                       words);
    return hipGetLastError();
}

hipError_t launch_srch_clamp(const SrchHit* hits, uint32_t npat, uint32_t max_hits, uint32_t* q, hipStream_t st) {
    hipLaunchKernelGGL(srch_clamp_kernel, dim3(blocks_of((u64)npat + 1)), dim3(kB), 0, st, hits, npat, max_hits, q);
    return hipGetLastError();
}

hipError_t launch_srch_gather(const uint32_t* sa, uint32_t N, const SrchHit* hits, const uint32_t* offs,
                              uint32_t npat, uint32_t* positions, uint64_t cap, hipStream_t st) {
    const unsigned grid = std::max(1u, std::min(kGatherGrid, blocks_of(cap)));
    hipLaunchKernelGGL(srch_gather_kernel, dim3(grid), dim3(kB), 0, st, sa, N, hits, offs, npat, positions, (u64)cap);
    return hipGetLastError();
}

}  // namespace gx
