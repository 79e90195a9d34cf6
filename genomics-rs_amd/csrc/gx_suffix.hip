// gx_suffix.hip -- suffix array, LCP array, BWT and the suffix tree's
// statistics of t = s + '$', the device half of suffix-tree mode
// (main.rs:154-215; compute_stats, tree.rs:740-803).
//
//   keys          round 0: the first 8 bytes of every suffix, big-endian;
//                 round r: (rank[i] << 32) | rank[i + h].  The same launch
//                 reduces the OR and the AND of all keys, from which the host
//                 skips the radix passes whose digit is the same in every key.
//   radix pass    histogram ([digit][workgroup] counts), exclusive scan of
//                 that table, stable scatter: a wave ranks its items per digit
//                 with ballots, the waves' counts meet in LDS.
//   scan          reduce, scan of the partials, downsweep (uint32).
//   ranks         head flags of the sorted keys, inclusive scan, scatter to
//                 text order.
//   LCP           Kasai's order, a lane per chunk of C text positions.
//   fold          max LCP with its first position, and the count and depth sum
//                 of the tree's internal nodes from a nearest-smaller-or-equal
//                 search to the left (own block, block minima, found block).
//
// No kernel here waits on another workgroup: every device-wide dependency is
// a kernel boundary.
#include <hip/hip_runtime.h>

#include "gx_suffix.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
constexpr int kI = kSufItems;
constexpr int kT = kSufTile;
constexpr int kWaves = kB / 64;
typedef unsigned long long u64;

__device__ inline u64 load8(const uint8_t* p) {
    u64 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ inline uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// The exclusive prefix of v over the workgroup's threads; *total = the sum.  sh: kWaves words.
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < kWaves; ++q) {
        const uint32_t s = sh[q];
        if (q < w) off += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return off + inc - v;
}

enum { kOpSum, kOpMax, kOpOr, kOpAnd };
template <int Op> __device__ inline u64 op64(u64 a, u64 b) {
    if (Op == kOpSum) return a + b;
    if (Op == kOpMax) return a > b ? a : b;
    if (Op == kOpOr) return a | b;
    return a & b;
}
// The workgroup's reduction of v, valid in thread 0.  sh: kWaves words, free again on return.
template <int Op> __device__ inline u64 block_reduce64(u64 v, u64* sh) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = op64<Op>(v, __shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = sh[0];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) r = op64<Op>(r, sh[q]);
    __syncthreads();
    return r;
}

__device__ inline void masks_fold(u64 key, bool active, uint64_t* masks, u64* sh) {
    const u64 o = block_reduce64<kOpOr>(active ? key : 0ull, sh);
    const u64 a = block_reduce64<kOpAnd>(active ? key : ~0ull, sh);
    if (threadIdx.x == 0) {
        atomicOr((u64*)&masks[0], o);
        atomicAnd((u64*)&masks[1], a);
    }
}

// ---------------------------------------------------------------------------
// keys

__global__ __launch_bounds__(kB) void suf_keys0_kernel(const uint8_t* __restrict__ text, uint32_t N,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                       uint64_t* masks) {
    __shared__ u64 sh[kWaves];
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    u64 key = 0;
    if (i < N) {
        key = __builtin_bswap64(load8(text + i));   // (kSufPad zero bytes follow the text)
        keys[i] = key;
        vals[i] = i;
    }
    masks_fold(key, i < N, masks, sh);
}

__global__ __launch_bounds__(kB) void suf_keys_kernel(const uint32_t* __restrict__ rank, uint32_t N, uint32_t h,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                      uint64_t* masks) {
    __shared__ u64 sh[kWaves];
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    u64 key = 0;
    if (i < N) {
        const uint32_t lo = (i + h < N) ? rank[i + h] : 0u;   // (N <= 2^30 and h < 2^31: no wrap)
        key = ((u64)rank[i] << 32) | lo;
        keys[i] = key;
        vals[i] = i;
    }
    masks_fold(key, i < N, masks, sh);
}

// ---------------------------------------------------------------------------
// radix pass

__global__ __launch_bounds__(kB) void suf_hist_kernel(const uint64_t* __restrict__ keys, uint32_t N, int shift,
                                                      uint32_t tiles, uint32_t* __restrict__ table) {
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kT;
#pragma unroll
    for (int r = 0; r < kI; ++r) {
        const uint32_t k = base + r * kB + threadIdx.x;
        if (k < N) atomicAdd(&hist[(uint32_t)(keys[k] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

// table: the exclusive scan of the histogram table, i.e. where this
// workgroup's first item of each digit goes.  Items keep their order: rounds
// in order, waves of a round in order (their counts in wc), lanes by ballot.
__global__ __launch_bounds__(kB) void suf_scatter_kernel(const uint64_t* __restrict__ kin,
                                                         const uint32_t* __restrict__ vin,
                                                         uint64_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                         uint32_t N, int shift, uint32_t tiles,
                                                         const uint32_t* __restrict__ table) {
    __shared__ uint32_t run[256];
    __shared__ uint32_t wc[kWaves][256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    run[t] = table[(size_t)t * tiles + blockIdx.x];
#pragma unroll
    for (int q = 0; q < kWaves; ++q) wc[q][t] = 0;
    __syncthreads();
    const u64 lt = (1ull << lane) - 1ull;
    const uint32_t base = blockIdx.x * kT;
    for (int r = 0; r < kI; ++r) {
        const uint32_t k = base + r * kB + t;
        const bool active = k < N;
        u64 key = 0;
        uint32_t val = 0, d = 0;
        if (active) {
            key = kin[k];
            val = vin[k];
            d = (uint32_t)(key >> shift) & 255u;
        }
        u64 m = __ballot(active);   // -> the active lanes of this wave that hold digit d
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 bb = __ballot(active && bit);
            m &= bit ? bb : ~bb;
        }
        const uint32_t below = __popcll(m & lt);
        if (active && below == 0) wc[w][d] = __popcll(m);
        __syncthreads();
        if (active) {
            uint32_t pos = run[d] + below;
#pragma unroll
            for (int q = 0; q < kWaves; ++q)
                if (q < w) pos += wc[q][d];
            if (pos < N) {   // (always, while the table is this input's)
                kout[pos] = key;
                vout[pos] = val;
            }
        }
        __syncthreads();
        uint32_t s = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) {
            s += wc[q][t];
            wc[q][t] = 0;
        }
        run[t] += s;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// scan

__global__ __launch_bounds__(kB) void suf_scan_reduce_kernel(const uint32_t* __restrict__ data, uint32_t n,
                                                             uint32_t* __restrict__ part) {
    __shared__ u64 sh[kWaves];
    const uint32_t base = blockIdx.x * kT;
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < kI; ++r) {
        const uint32_t k = base + r * kB + threadIdx.x;
        if (k < n) s += data[k];
    }
    const u64 tot = block_reduce64<kOpSum>(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = (uint32_t)tot;
}

// One workgroup: part[0..nb) -> its exclusive prefix sums.
__global__ __launch_bounds__(kB) void suf_scan_part_kernel(uint32_t* part, uint32_t nb) {
    __shared__ uint32_t sh[kWaves];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kB) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? part[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan(v, sh, &tot);
        if (i < nb) part[i] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(kB) void suf_scan_down_kernel(uint32_t* data, uint32_t n, int inclusive,
                                                           const uint32_t* __restrict__ part) {
    __shared__ uint32_t sh[kWaves];
    const uint32_t base = blockIdx.x * kT + threadIdx.x * kI;
    uint32_t x[kI], s = 0;
#pragma unroll
    for (int q = 0; q < kI; ++q) {
        x[q] = base + q < n ? data[base + q] : 0u;
        s += x[q];
    }
    uint32_t tot;
    uint32_t ex = block_excl_scan(s, sh, &tot) + part[blockIdx.x];
#pragma unroll
    for (int q = 0; q < kI; ++q) {
        if (base + q >= n) break;
        if (inclusive) {
            ex += x[q];
            data[base + q] = ex;
        } else {
            data[base + q] = ex;
            ex += x[q];
        }
    }
}

// ---------------------------------------------------------------------------
// ranks, BWT, LCP

__global__ __launch_bounds__(kB) void suf_flags_kernel(const uint64_t* __restrict__ keys, uint32_t N,
                                                       uint32_t* __restrict__ flags) {
    const uint32_t k = blockIdx.x * kB + threadIdx.x;
    if (k < N) flags[k] = (k > 0 && keys[k] != keys[k - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(kB) void suf_rank_scatter_kernel(const uint32_t* __restrict__ vals,
                                                              const uint32_t* __restrict__ ranks, uint32_t N,
                                                              uint32_t* __restrict__ rank, uint32_t* last) {
    const uint32_t k = blockIdx.x * kB + threadIdx.x;
    if (k >= N) return;
    const uint32_t i = vals[k], r = ranks[k];
    if (i < N) rank[i] = r;
    if (k == N - 1) *last = r;
}

__global__ __launch_bounds__(kB) void suf_bwt_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ sa,
                                                     uint32_t N, uint8_t* __restrict__ bwt) {
    const uint32_t k = blockIdx.x * kB + threadIdx.x;
    if (k >= N) return;
    const uint32_t i = sa[k];
    bwt[k] = (i > 0 && i <= N) ? text[i - 1] : (uint8_t)'$';
}

// A lane owns kSufLcpChunk consecutive text positions: it starts the first
// from h = 0 and carries h - 1 to the next (LCP[rank[i + 1]] >= LCP[rank[i]] - 1).
__global__ __launch_bounds__(kB) void suf_lcp_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ sa,
                                                     const uint32_t* __restrict__ rank, uint32_t N,
                                                     uint32_t* __restrict__ lcp) {
    const u64 g = (u64)blockIdx.x * kB + threadIdx.x;
    const u64 i0 = g * kSufLcpChunk;
    uint32_t h = 0;
    for (int q = 0; q < kSufLcpChunk; ++q) {
        const u64 i = i0 + q;
        if (i >= N) return;
        const uint32_t r = rank[i];
        if (r == 0 || r >= N) {   // the lone '$': no predecessor
            if (r == 0) lcp[0] = 0;
            h = 0;
            continue;
        }
        const uint32_t j = sa[r - 1];
        if (j >= N || j == i) { h = 0; continue; }
        // '$' is unique, so the suffixes differ before either leaves the text
        const u64 far = (i > j ? i : j);
        while (far + h < N) {
            const u64 x = load8(text + i + h) ^ load8(text + j + h);
            if (x) {
                h += (uint32_t)(__builtin_ctzll(x) >> 3);
                break;
            }
            h += 8;
        }
        lcp[r] = h;
        h = h ? h - 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// statistics fold

__global__ __launch_bounds__(kB) void suf_fold_min_kernel(const uint32_t* __restrict__ lcp, uint32_t N,
                                                          uint32_t* __restrict__ bmin, uint64_t* __restrict__ pmax) {
    __shared__ u64 sh[kWaves];
    const uint32_t k = blockIdx.x * kB + threadIdx.x;
    const uint32_t v = k < N ? lcp[k] : 0u;
    // max of ~v = ~min v; max of (v << 32) | ~k = the largest v at its smallest k
    const u64 mn = block_reduce64<kOpMax>(k < N ? (u64)(~v) : 0ull, sh);
    const u64 mx = block_reduce64<kOpMax>(k < N ? (((u64)v << 32) | (uint32_t)~k) : 0ull, sh);
    if (threadIdx.x == 0) {
        bmin[blockIdx.x] = ~(uint32_t)mn;
        pmax[blockIdx.x] = mx;
    }
}

// Position k > 0 with v = LCP[k] > 0 closes an internal node of depth v iff the
// nearest k' < k with LCP[k'] <= v has LCP[k'] < v (position 0 holds 0).
__global__ __launch_bounds__(kB) void suf_fold_count_kernel(const uint32_t* __restrict__ lcp, uint32_t N,
                                                            const uint32_t* __restrict__ bmin,
                                                            uint64_t* __restrict__ pcnt, uint64_t* __restrict__ psum) {
    __shared__ uint32_t s[kB];
    __shared__ u64 sh[kWaves];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t k = b * kB + t;
    const uint32_t v = k < N ? lcp[k] : 0u;
    s[t] = v;
    __syncthreads();
    u64 cnt = 0, sum = 0;
    if (k < N && k > 0 && v > 0) {
        bool found = false;
        uint32_t pv = 0;
        for (int p = t - 1; p >= 0; --p)
            if (s[p] <= v) { pv = s[p]; found = true; break; }
        if (!found && b > 0) {
            uint32_t bb = b - 1;
            while (bb > 0 && bmin[bb] > v) --bb;
            for (int p = kB - 1; p >= 0; --p) {   // (whole blocks: bb < b <= the last block)
                const uint32_t x = lcp[(size_t)bb * kB + p];
                if (x <= v) { pv = x; found = true; break; }
            }
        }
        if (found && pv < v) { cnt = 1; sum = v; }
    }
    const u64 c = block_reduce64<kOpSum>(cnt, sh);
    const u64 d = block_reduce64<kOpSum>(sum, sh);
    if (t == 0) {
        pcnt[b] = c;
        psum[b] = d;
    }
}

// One workgroup sums the partials.
__global__ __launch_bounds__(kB) void suf_fold_final_kernel(const uint64_t* __restrict__ pcnt,
                                                            const uint64_t* __restrict__ psum,
                                                            const uint64_t* __restrict__ pmax, uint32_t nb,
                                                            const uint32_t* __restrict__ sa, uint32_t N, SufFold* out) {
    __shared__ u64 sh[kWaves];
    u64 c = 0, d = 0, m = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += kB) {
        c += pcnt[i];
        d += psum[i];
        m = pmax[i] > m ? (u64)pmax[i] : m;
    }
    c = block_reduce64<kOpSum>(c, sh);
    d = block_reduce64<kOpSum>(d, sh);
    m = block_reduce64<kOpMax>(m, sh);
    if (threadIdx.x == 0) {
        const uint32_t L = (uint32_t)(m >> 32), ks = ~(uint32_t)m;
        out->num_internal = c;
        out->depth_sum = d;
        out->max_key = m;
        out->repeat_start = (L > 0 && ks > 0 && ks < N) ? (uint64_t)sa[ks - 1] + 1 : 0;
    }
}

inline unsigned blocks_of(uint32_t n, int per) { return (unsigned)((n + (uint32_t)per - 1) / (uint32_t)per); }

}  // namespace

hipError_t launch_suf_keys0(const uint8_t* text, uint32_t N, uint64_t* keys, uint32_t* vals, uint64_t* masks,
                            hipStream_t st) {
    hipLaunchKernelGGL(suf_keys0_kernel, dim3(blocks_of(N, kB)), dim3(kB), 0, st, text, N, keys, vals, masks);
    return hipGetLastError();
}

hipError_t launch_suf_keys(const uint32_t* rank, uint32_t N, uint32_t h, uint64_t* keys, uint32_t* vals,
                           uint64_t* masks, hipStream_t st) {
    hipLaunchKernelGGL(suf_keys_kernel, dim3(blocks_of(N, kB)), dim3(kB), 0, st, rank, N, h, keys, vals, masks);
    return hipGetLastError();
}

hipError_t launch_suf_scan(uint32_t* data, uint32_t n, bool inclusive, uint32_t* tmp, hipStream_t st) {
    const unsigned nb = blocks_of(n, kT);
    hipLaunchKernelGGL(suf_scan_reduce_kernel, dim3(nb), dim3(kB), 0, st, data, n, tmp);
    hipLaunchKernelGGL(suf_scan_part_kernel, dim3(1), dim3(kB), 0, st, tmp, nb);
    hipLaunchKernelGGL(suf_scan_down_kernel, dim3(nb), dim3(kB), 0, st, data, n, inclusive ? 1 : 0, tmp);
    return hipGetLastError();
}

hipError_t launch_suf_sort_pass(const uint64_t* kin, const uint32_t* vin, uint64_t* kout, uint32_t* vout, uint32_t N,
                                int shift, uint32_t* table, uint32_t* scan_tmp, hipStream_t st) {
    const unsigned tiles = blocks_of(N, kT);
    hipLaunchKernelGGL(suf_hist_kernel, dim3(tiles), dim3(kB), 0, st, kin, N, shift, tiles, table);
    hipError_t e = launch_suf_scan(table, 256u * tiles, false, scan_tmp, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(suf_scatter_kernel, dim3(tiles), dim3(kB), 0, st, kin, vin, kout, vout, N, shift, tiles,
                       table);
    return hipGetLastError();
}

hipError_t launch_suf_ranks(const uint64_t* keys, const uint32_t* vals, uint32_t N, uint32_t* flags,
                            uint32_t* scan_tmp, uint32_t* rank, uint32_t* last, hipStream_t st) {
    hipLaunchKernelGGL(suf_flags_kernel, dim3(blocks_of(N, kB)), dim3(kB), 0, st, keys, N, flags);
    hipError_t e = launch_suf_scan(flags, N, true, scan_tmp, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(suf_rank_scatter_kernel, dim3(blocks_of(N, kB)), dim3(kB), 0, st, vals, flags, N, rank, last);
    return hipGetLastError();
}

hipError_t launch_suf_bwt(const uint8_t* text, const uint32_t* sa, uint32_t N, uint8_t* bwt, hipStream_t st) {
    hipLaunchKernelGGL(suf_bwt_kernel, dim3(blocks_of(N, kB)), dim3(kB), 0, st, text, sa, N, bwt);
    return hipGetLastError();
}

hipError_t launch_suf_lcp(const uint8_t* text, const uint32_t* sa, const uint32_t* rank, uint32_t N, uint32_t* lcp,
                          hipStream_t st) {
    const uint32_t lanes = (N + kSufLcpChunk - 1) / kSufLcpChunk;
    hipLaunchKernelGGL(suf_lcp_kernel, dim3(blocks_of(lanes, kB)), dim3(kB), 0, st, text, sa, rank, N, lcp);
    return hipGetLastError();
}

hipError_t launch_suf_fold(const uint32_t* lcp, const uint32_t* sa, uint32_t N, uint32_t* bmin, uint64_t* pcnt,
                           uint64_t* psum, uint64_t* pmax, SufFold* out, hipStream_t st) {
    const unsigned nb = blocks_of(N, kSufFoldBlock);
    hipLaunchKernelGGL(suf_fold_min_kernel, dim3(nb), dim3(kB), 0, st, lcp, N, bmin, pmax);
    hipLaunchKernelGGL(suf_fold_count_kernel, dim3(nb), dim3(kB), 0, st, lcp, N, bmin, pcnt, psum);
    hipLaunchKernelGGL(suf_fold_final_kernel, dim3(1), dim3(kB), 0, st, pcnt, psum, pmax, nb, sa, N, out);
    return hipGetLastError();
}

}  // namespace gx
