// gx_match.hip -- matching statistics and maximal exact matches of long queries
// on the suffix array of t = s + '$', the device half of DESIGN.md 21.  No
// counterpart in the reference.
//
//   stats    a lane per query position of the concatenated buffer: the longest
//            prefix of its window that occurs and that prefix's interval
//            (match_stat_one, gx_match.h); the pattern is read in place
//   seeds    the same lanes with the window min_len: (lo, cnt) of the min_len-mer
//   keep     a lane per candidate pair (a bounded grid strides over them), its
//            position found by a search over the scanned counts: i = SA[lo + r],
//            kept iff left-maximal
//   counts   candidates and MEMs before every query, from the two scans
//   emit     every kept pair extended to the right from min_len, 8 bytes a step
//   pack     sorted (position << 32 | text position, length) into gx_mem
//
// As gx_search.hip: 256-thread workgroups, no kernel waits on another
// workgroup, every device-wide dependency is a kernel boundary.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gx_match.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
constexpr int kWaves = kB / 64;
constexpr unsigned kStrideGrid = 2048;   // workgroups of keep, emit and pack at most; they stride over the rest
typedef unsigned long long u64;

// The workgroup's sum of v into *total: wave shuffles, LDS, one vector atomic.
__device__ inline void block_add(u64 v, u64* sh, u64* total) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();   // (sh may still be read from a call before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += sh[q];
        if (s) atomicAdd(total, s);
    }
}

__global__ __launch_bounds__(kB) void match_stats_kernel(const uint8_t* __restrict__ text,
                                                         const uint32_t* __restrict__ sa, uint32_t N,
                                                         const uint8_t* __restrict__ q,
                                                         const uint32_t* __restrict__ offs, uint32_t nq, uint32_t npos,
                                                         uint32_t W, MatchStat* __restrict__ stats, u64* words_total) {
    __shared__ u64 sh[kWaves];
    const u64 g = (u64)blockIdx.x * kB + threadIdx.x;
    uint64_t words = 0;
    if (g < npos) {
        const uint32_t c = match_query_of(offs, nq, (uint32_t)g);
        const uint32_t e = c < nq ? offs[c + 1] : (uint32_t)g;
        uint32_t w = e > g ? e - (uint32_t)g : 0;
        if (w > W) w = W;
        stats[g] = match_stat_one(text, sa, N, q + g, w, &words);
    }
    block_add(words, sh, words_total);
}

__global__ __launch_bounds__(kB) void match_seeds_kernel(const uint8_t* __restrict__ text,
                                                         const uint32_t* __restrict__ sa, uint32_t N,
                                                         const uint8_t* __restrict__ q,
                                                         const uint32_t* __restrict__ offs, uint32_t nq, uint32_t npos,
                                                         uint32_t L, uint32_t* __restrict__ lo,
                                                         uint32_t* __restrict__ cnt, uint32_t* __restrict__ qid,
                                                         u64* cnt_total) {
    __shared__ u64 sh[kWaves];
    const u64 g = (u64)blockIdx.x * kB + threadIdx.x;
    uint64_t words = 0;
    uint32_t n = 0;
    if (g < npos) {
        const uint32_t c = match_query_of(offs, nq, (uint32_t)g);
        const uint32_t e = c < nq ? offs[c + 1] : (uint32_t)g;
        const uint32_t rem = e > g ? e - (uint32_t)g : 0;
        uint32_t l = 0;
        match_seed_one(text, sa, N, q + g, rem, L, &l, &n, &words);
        lo[g] = l;
        cnt[g] = n;
        qid[g] = c;
    } else if (g == npos) {
        cnt[g] = 0;
    }
    block_add(words, sh, cnt_total);
    block_add(n, sh, cnt_total + 1);
}

__global__ __launch_bounds__(kB) void match_keep_kernel(const uint8_t* __restrict__ text,
                                                        const uint32_t* __restrict__ sa, uint32_t N,
                                                        const uint8_t* __restrict__ q,
                                                        const uint32_t* __restrict__ offs,
                                                        const uint32_t* __restrict__ qid,
                                                        const uint32_t* __restrict__ lo,
                                                        const uint32_t* __restrict__ coff, uint32_t npos, uint32_t T,
                                                        uint32_t* __restrict__ cg, uint32_t* __restrict__ ci,
                                                        uint32_t* __restrict__ keep) {
    for (u64 x = (u64)blockIdx.x * kB + threadIdx.x; x <= T; x += (u64)gridDim.x * kB) {
        if (x == T) {
            keep[x] = 0;
            continue;
        }
        uint32_t A = 0, R = npos;   // -> the first g with coff[g + 1] > x (coff[npos] = T > x)
        while (A < R) {
            const uint32_t mid = A + (R - A) / 2;
            if (coff[mid + 1] <= x) A = mid + 1; else R = mid;
        }
        uint32_t g = A, i = 0, k = 0;
        if (g < npos) {
            const u64 at = (u64)lo[g] + (x - coff[g]);
            i = at < N ? sa[at] : N;
            if (i < N) k = match_left_maximal(text, i, q + g, g - offs[qid[g]]) ? 1u : 0u;
        } else {
            g = 0;   // (never: the scan's total is T)
        }
        cg[x] = g;
        ci[x] = i;
        keep[x] = k;
    }
}

__global__ __launch_bounds__(kB) void match_counts_kernel(const uint32_t* __restrict__ offs, uint32_t nq,
                                                          const uint32_t* __restrict__ coff,
                                                          const uint32_t* __restrict__ kscan,
                                                          uint32_t* __restrict__ cpre, uint32_t* __restrict__ mpre) {
    const u64 c = (u64)blockIdx.x * kB + threadIdx.x;
    if (c > nq) return;
    const uint32_t x = coff[offs[c]];
    cpre[c] = x;
    mpre[c] = kscan[x];
}

__global__ __launch_bounds__(kB) void match_emit_kernel(const uint8_t* __restrict__ text, uint32_t N,
                                                        const uint8_t* __restrict__ q,
                                                        const uint32_t* __restrict__ offs,
                                                        const uint32_t* __restrict__ qid,
                                                        const uint32_t* __restrict__ cg,
                                                        const uint32_t* __restrict__ ci,
                                                        const uint32_t* __restrict__ kscan, uint32_t T, uint32_t L,
                                                        uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                        u64* words_total) {
    __shared__ u64 sh[kWaves];
    uint64_t words = 0;
    const uint32_t M = kscan[T];
    for (u64 x = (u64)blockIdx.x * kB + threadIdx.x; x < T; x += (u64)gridDim.x * kB) {
        const uint32_t k = kscan[x];
        if (kscan[x + 1] == k || k >= M) continue;   // not kept
        const uint32_t g = cg[x], i = ci[x];
        const uint32_t rem = offs[qid[g] + 1] - g;
        keys[k] = (uint64_t)g << 32 | i;
        vals[k] = match_extend(text, N, i, q + g, rem, L, &words);
    }
    block_add(words, sh, words_total);
}

__global__ __launch_bounds__(kB) void match_pack_kernel(const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ vals, uint32_t M,
                                                        const uint32_t* __restrict__ offs,
                                                        const uint32_t* __restrict__ qid, Mem* __restrict__ mems) {
    for (u64 k = (u64)blockIdx.x * kB + threadIdx.x; k < M; k += (u64)gridDim.x * kB) {
        const uint32_t g = (uint32_t)(keys[k] >> 32);
        Mem o;
        o.qpos = g - offs[qid[g]];
        o.tpos = (uint32_t)keys[k];
        o.len = vals[k];
        mems[k] = o;
    }
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + kB - 1) / kB); }
inline unsigned stride_grid(u64 n) { return std::max(1u, std::min(kStrideGrid, blocks_of(n))); }

}  // namespace

hipError_t launch_match_stats(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* q,
                              const uint32_t* offs, uint32_t nq, uint32_t npos, uint32_t W, MatchStat* stats,
                              unsigned long long* words, hipStream_t st) {
    if (!npos) return hipSuccess;
    hipLaunchKernelGGL(match_stats_kernel, dim3(blocks_of(npos)), dim3(kB), 0, st, text, sa, N, q, offs, nq, npos, W,
                       stats, words);
    return hipGetLastError();
}

hipError_t launch_match_seeds(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* q,
                              const uint32_t* offs, uint32_t nq, uint32_t npos, uint32_t L, uint32_t* lo, uint32_t* cnt,
                              uint32_t* qid, unsigned long long* cnt_total, hipStream_t st) {
    hipLaunchKernelGGL(match_seeds_kernel, dim3(blocks_of((u64)npos + 1)), dim3(kB), 0, st, text, sa, N, q, offs, nq,
                       npos, L, lo, cnt, qid, cnt_total);
    return hipGetLastError();
}

hipError_t launch_match_keep(const uint8_t* text, const uint32_t* sa, uint32_t N, const uint8_t* q,
                             const uint32_t* offs, const uint32_t* qid, const uint32_t* lo, const uint32_t* coff,
                             uint32_t npos, uint32_t T, uint32_t* cg, uint32_t* ci, uint32_t* keep, hipStream_t st) {
    hipLaunchKernelGGL(match_keep_kernel, dim3(stride_grid((u64)T + 1)), dim3(kB), 0, st, text, sa, N, q, offs, qid, lo,
                       coff, npos, T, cg, ci, keep);
    return hipGetLastError();
}

hipError_t launch_match_counts(const uint32_t* offs, uint32_t nq, const uint32_t* coff, const uint32_t* kscan,
                               uint32_t* cpre, uint32_t* mpre, hipStream_t st) {
    hipLaunchKernelGGL(match_counts_kernel, dim3(blocks_of((u64)nq + 1)), dim3(kB), 0, st, offs, nq, coff, kscan, cpre,
                       mpre);
    return hipGetLastError();
}

hipError_t launch_match_emit(const uint8_t* text, uint32_t N, const uint8_t* q, const uint32_t* offs,
                             const uint32_t* qid, const uint32_t* cg, const uint32_t* ci, const uint32_t* kscan,
                             uint32_t T, uint32_t L, uint64_t* keys, uint32_t* vals, unsigned long long* words,
                             hipStream_t st) {
    hipLaunchKernelGGL(match_emit_kernel, dim3(stride_grid(T)), dim3(kB), 0, st, text, N, q, offs, qid, cg, ci, kscan, T,
                       L, keys, vals, words);
    return hipGetLastError();
}

hipError_t launch_match_pack(const uint64_t* keys, const uint32_t* vals, uint32_t M, const uint32_t* offs,
                             const uint32_t* qid, Mem* mems, hipStream_t st) {
    hipLaunchKernelGGL(match_pack_kernel, dim3(stride_grid(M)), dim3(kB), 0, st, keys, vals, M, offs, qid, mems);
    return hipGetLastError();
}

}  // namespace gx
