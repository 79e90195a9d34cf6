// gx_strand.hip -- the reverse items of a staged batch, written on the device
// behind (BOTH) or instead of (REV) the forward bytes the host copied, the
// device half of DESIGN.md 24.  No counterpart in the reference.
//
//   unit     an aligned 8-byte word of the output: a lane's one vector store.
//            A lane finds the item of its word's first byte by a search over
//            the offsets (it lands on a non-empty item by construction), so a
//            million short items and one item of megabytes are the same work
//            and no lane or wave loops over an item.
//   fast     the word lies inside one item: its 8 source bytes are contiguous,
//            read as two aligned words and a shift, complemented through the
//            table in LDS, stored reversed
//   edge     the word crosses items, the region's unaligned ends or the
//            kSufPad zero bytes: byte by byte, a new search at every item end,
//            and byte stores where the word is not all this launch's
//   offsets  BOTH: off'[n + p] = T + off[p], by the same strided lanes
//
// As gx_search.hip: 256-thread workgroups, a strided grid of at most
// kStrideGrid workgroups, no workgroup waits on another, vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gx_strand.h"

namespace gx {

namespace {

constexpr int kB = kSufBlock;
constexpr unsigned kStrideGrid = 2048;   // workgroups at most; they stride over the rest
typedef unsigned long long u64;

static_assert(kB == 256, "a lane per table entry");

// The last p with off[p] <= r, for r < off[n]: r lies in item p, which is not empty.
__device__ inline uint32_t strand_item_of(const uint32_t* off, uint32_t n, uint32_t r) {
    uint32_t lo = 0, hi = n;   // off[lo] <= r < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// src, dst: 8-byte aligned.  off is read at [0, n], off_out written behind it: not restrict.
__global__ __launch_bounds__(kB) void strand_rc_kernel(const uint8_t* src, const uint32_t* off, uint32_t n, uint32_t T,
                                                       uint8_t* dst, uint32_t dst_at, uint32_t* off_out) {
    __shared__ uint8_t comp[256];
    comp[threadIdx.x] = strand_comp((uint8_t)threadIdx.x);
    __syncthreads();
    const u64 tid = (u64)blockIdx.x * kB + threadIdx.x, stride = (u64)gridDim.x * kB;
    if (off_out)
        for (u64 p = tid; p < n; p += stride) off_out[p] = T + off[p + 1];
    const u64 end = (u64)dst_at + T + kSufPad;   // the first byte behind the padding
    const u64 w0 = dst_at / kStrandUnit, w1 = (end + kStrandUnit - 1) / kStrandUnit;
    for (u64 w = w0 + tid; w < w1; w += stride) {
        const u64 g0 = w * kStrandUnit;
        u64 word = 0;
        if (g0 >= dst_at && g0 + 8 <= (u64)dst_at + T) {
            const uint32_t r = (uint32_t)(g0 - dst_at);
            const uint32_t p = strand_item_of(off, n, r), e = off[p + 1];
            if (e - r >= 8) {
                // bytes r .. r + 7 of the reverse half are rc of src[s .. s + 7], s = off[p] + (e - 8 - r)
                const uint32_t s = off[p] + (e - 8 - r), sh = (s & 7u) * 8;
                const u64* a = (const u64*)(src + (s & ~7u));
                u64 v = a[0] >> sh;
                if (sh) v |= a[1] << (64 - sh);   // (its bytes below s + 8 < T only)
#pragma unroll
                for (int j = 0; j < 8; ++j) word |= (u64)comp[(v >> (8 * (7 - j))) & 0xffu] << (8 * j);
                *(u64*)(dst + g0) = word;
                continue;
            }
        }
        // the edges: every byte of the word that is this launch's, on its own
        uint32_t p = 0, b = 0, e = 0;   // the item [b, e) of the last byte looked up (none yet)
        unsigned valid = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u64 g = g0 + j;
            if (g < dst_at || g >= end) continue;
            valid |= 1u << j;
            const u64 r64 = g - dst_at;
            if (r64 >= T) continue;   // padding: 0
            const uint32_t r = (uint32_t)r64;
            if (r >= e) {
                p = strand_item_of(off, n, r);
                b = off[p];
                e = off[p + 1];
            }
            word |= (u64)comp[src[b + (e - 1 - r)]] << (8 * j);
        }
        if (valid == 0xffu) {
            *(u64*)(dst + g0) = word;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (valid >> j & 1u) dst[g0 + j] = (uint8_t)(word >> (8 * j));
        }
    }
}

inline unsigned blocks_of(u64 n) { return (unsigned)((n + kB - 1) / kB); }
inline unsigned stride_grid(u64 n) { return std::max(1u, std::min(kStrideGrid, blocks_of(n))); }

}  // namespace

hipError_t launch_strand_rc(const uint8_t* src, const uint32_t* off, uint32_t n, uint32_t T, uint8_t* dst, uint32_t dst_at,
                            uint32_t* off_out, hipStream_t st) {
    const u64 work = std::max<u64>(strand_units(T, dst_at), off_out ? n : 0);
    hipLaunchKernelGGL(strand_rc_kernel, dim3(stride_grid(work)), dim3(kB), 0, st, src, off, n, T, dst, dst_at, off_out);
    return hipGetLastError();
}

}  // namespace gx
