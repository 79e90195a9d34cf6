// gx_lcsub.hip -- longest common substring of many (a, b) sub-problems, the
// device half of compare mode (main.rs:216-379; get_lcs, tree.rs:218-281).
//
// The longest common substring of a (n bytes) and b (m bytes) is the longest
// run of equal bytes along a diagonal j - i = d of the n x m comparison grid
// (DESIGN.md 16).  Runs on different diagonals are independent:
//
//   run kernel        one lane per diagonal, rows cut into segments of H rows.
//                     A (diagonal, segment) tile is reduced to the monoid
//                     element (head run, tail run, best inside, all-equal).
//   combine kernel    one lane per diagonal stitches its segments in row
//                     order (a run may span any number of them), stores the
//                     run length carried into every segment and reduces the
//                     diagonals to L per sub-problem (vector atomic max).
//   candidate kernel  walks again only the lanes whose tile can hold the end
//                     of a run of length >= L and emits the (i, j) start of
//                     every window of length L in such a run into a bounded
//                     buffer (vector atomic counters; an overflow flag sends
//                     the sub-problem to the host solver).
//
// All three take one descriptor array and walk the flat tile list of every
// sub-problem with a persistent grid, so one level of every pair's recursion
// is three launches.  Sequences are staged once; a descriptor holds offsets.
#include <hip/hip_runtime.h>

#include "gx_lcsub.h"

namespace gx {

namespace {

constexpr int kBlock = kLcsubBlock;

// The sub-problem that owns flat index t of a prefix-summed list
// (base(k) <= t < base(k + 1)).
template <class Base>
__device__ inline int owner(int nsub, unsigned t, Base base) {
    int lo = 0, hi = nsub - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base(mid) <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline unsigned long long load8(const uint8_t* p) {
    unsigned long long v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// Rows [lo, hi) of segment [i0, i1) in which diagonal d has a cell (0 <= j < m).
__device__ inline void lane_rows(const LcsubDesc& s, int d, int i0, int i1, int* lo, int* hi) {
    *lo = max(i0, -d);
    *hi = min(i1, (int)s.m - d);
}

}  // namespace

// elem[elem_base + seg * ndiag + k]: x = head | tail << 16, y = best | all << 31
// (H <= kLcsubMaxSeg keeps the three runs below 2^15).
__global__ __launch_bounds__(kBlock) void lcsub_run_kernel(const uint8_t* __restrict__ chars,
                                                           const LcsubDesc* __restrict__ subs, int nsub,
                                                           unsigned total_tiles, int H, uint2* __restrict__ elem) {
    for (unsigned t = blockIdx.x; t < total_tiles; t += gridDim.x) {
        const int si = owner(nsub, t, [&](int k) { return subs[k].tile_base; });
        const LcsubDesc s = subs[si];
        const unsigned tl = t - s.tile_base;
        const int ndblk = (s.ndiag + kBlock - 1) / kBlock;
        const int seg = tl / ndblk;
        const int k = (tl % ndblk) * kBlock + threadIdx.x;
        if (k >= (int)s.ndiag) continue;
        const int d = k - ((int)s.n - 1);
        const int i0 = seg * H, i1 = min((int)s.n, i0 + H);
        int lo, hi;
        lane_rows(s, d, i0, i1, &lo, &hi);
        unsigned head = 0, tail = 0, best = 0, all = 0;
        if (lo < hi) {
            const uint8_t* pa = chars + s.a_off;
            const uint8_t* pb = chars + s.b_off + d;   // pb[i] = b[i + d], read for lo <= i < hi only
            bool broke = lo > i0;
            unsigned r = 0;
            auto step = [&](bool eq) {
                if (eq) {
                    ++r;
                } else {
                    if (!broke) { head = r; broke = true; }
                    best = max(best, r);
                    r = 0;
                }
            };
            int i = lo;
            for (; i + 8 <= hi; i += 8) {
                const unsigned long long x = load8(pa + i) ^ load8(pb + i);
                if (x == 0) { r += 8; continue; }
#pragma unroll
                for (int q = 0; q < 8; ++q) step(((x >> (8 * q)) & 0xffull) == 0);
            }
            for (; i < hi; ++i) step(pa[i] == pb[i]);
            best = max(best, r);
            if (hi < i1) {   // the diagonal leaves the grid inside the segment
                if (!broke) { head = r; broke = true; }
                r = 0;
            }
            tail = r;
            if (!broke) { head = r; all = 1; }
        }
        elem[s.elem_base + (size_t)seg * s.ndiag + k] = make_uint2(head | (tail << 16), best | (all << 31));
    }
}

// carry[elem_base + seg * ndiag + k] = the run length that reaches segment
// seg's first row on diagonal k; L[sub] = the longest run of the sub-problem.
__global__ __launch_bounds__(kBlock) void lcsub_combine_kernel(const LcsubDesc* __restrict__ subs, int nsub,
                                                               unsigned total_dtiles,
                                                               const uint2* __restrict__ elem,
                                                               unsigned* __restrict__ carry,
                                                               unsigned* __restrict__ L) {
    for (unsigned t = blockIdx.x; t < total_dtiles; t += gridDim.x) {
        const int si = owner(nsub, t, [&](int k) { return subs[k].dtile_base; });
        const LcsubDesc s = subs[si];
        const int k = (t - s.dtile_base) * kBlock + threadIdx.x;
        unsigned best = 0;
        if (k < (int)s.ndiag) {
            unsigned run = 0;
            for (unsigned seg = 0; seg < s.nseg; ++seg) {
                const size_t at = s.elem_base + (size_t)seg * s.ndiag + k;
                const uint2 e = elem[at];
                carry[at] = run;
                const unsigned head = e.x & 0xffffu;
                if (e.y >> 31) {
                    run += head;
                } else {
                    best = max(best, max(run + head, e.y & 0x7fffffffu));
                    run = e.x >> 16;
                }
            }
            best = max(best, run);
        }
        for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o));
        if ((threadIdx.x & 63) == 0 && best) atomicMax(&L[si], best);
    }
}

// cand[slot] = (sub, i, j, 0) for every window of length L[sub] inside a run
// that ends in the lane's tile; hdr[0] counts the slots, cnt[sub] the
// sub-problem's windows (those past `cap` are dropped and ovf[sub] is set).
__global__ __launch_bounds__(kBlock) void lcsub_cand_kernel(const uint8_t* __restrict__ chars,
                                                            const LcsubDesc* __restrict__ subs, int nsub,
                                                            unsigned total_tiles, int H,
                                                            const uint2* __restrict__ elem,
                                                            const unsigned* __restrict__ carry,
                                                            const unsigned* __restrict__ L, unsigned cap,
                                                            unsigned slots, unsigned* __restrict__ cnt,
                                                            unsigned* __restrict__ ovf, unsigned* __restrict__ hdr,
                                                            uint4* __restrict__ cand) {
    for (unsigned t = blockIdx.x; t < total_tiles; t += gridDim.x) {
        const int si = owner(nsub, t, [&](int k) { return subs[k].tile_base; });
        const LcsubDesc s = subs[si];
        const unsigned len = L[si];
        if (len == 0) continue;
        const unsigned tl = t - s.tile_base;
        const int ndblk = (s.ndiag + kBlock - 1) / kBlock;
        const int seg = tl / ndblk;
        const int k = (tl % ndblk) * kBlock + threadIdx.x;
        if (k >= (int)s.ndiag) continue;
        const size_t at = s.elem_base + (size_t)seg * s.ndiag + k;
        const uint2 e = elem[at];
        const unsigned cin = carry[at];
        if (cin + (e.x & 0xffffu) < len && (e.y & 0x7fffffffu) < len) continue;
        const int d = k - ((int)s.n - 1);
        const int i0 = seg * H, i1 = min((int)s.n, i0 + H);
        int lo, hi;
        lane_rows(s, d, i0, i1, &lo, &hi);
        if (lo >= hi) continue;
        const uint8_t* pa = chars + s.a_off;
        const uint8_t* pb = chars + s.b_off + d;
        auto emit = [&](unsigned r, int end) {   // a run of r rows ending before row `end`
            for (unsigned w = 0; w + len <= r; ++w) {
                const unsigned i = (unsigned)end - r + w;
                if (atomicAdd(&cnt[si], 1u) < cap) {
                    const unsigned slot = atomicAdd(&hdr[0], 1u);
                    if (slot < slots) cand[slot] = make_uint4((unsigned)si, i, (unsigned)((int)i + d), 0u);
                } else {
                    atomicOr(&ovf[si], 1u);
                    return;   // the host solves this sub-problem: no need to count the rest
                }
            }
        };
        unsigned r = cin;   // (0 when the diagonal enters the grid inside this segment)
        for (int i = lo; i < hi; ++i) {
            if (pa[i] == pb[i]) {
                ++r;
            } else {
                if (r >= len) emit(r, i);
                r = 0;
            }
        }
        // the run ends here only where the diagonal does; otherwise the next
        // segment's lane holds its end (its carry is this r)
        if (r >= len && hi == min((int)s.n, (int)s.m - d)) emit(r, hi);
    }
}

hipError_t launch_lcsub_run(const uint8_t* chars, const LcsubDesc* subs, int nsub, unsigned total_tiles, int H,
                            uint2* elem, int grid, hipStream_t st) {
    hipLaunchKernelGGL(lcsub_run_kernel, dim3(grid), dim3(kBlock), 0, st, chars, subs, nsub, total_tiles, H, elem);
    return hipGetLastError();
}

hipError_t launch_lcsub_combine(const LcsubDesc* subs, int nsub, unsigned total_dtiles, const uint2* elem,
                                unsigned* carry, unsigned* L, int grid, hipStream_t st) {
    hipLaunchKernelGGL(lcsub_combine_kernel, dim3(grid), dim3(kBlock), 0, st, subs, nsub, total_dtiles, elem, carry,
                       L);
    return hipGetLastError();
}

hipError_t launch_lcsub_cand(const uint8_t* chars, const LcsubDesc* subs, int nsub, unsigned total_tiles, int H,
                             const uint2* elem, const unsigned* carry, const unsigned* L, unsigned cap,
                             unsigned slots, unsigned* cnt, unsigned* ovf, unsigned* hdr, uint4* cand, int grid,
                             hipStream_t st) {
    hipLaunchKernelGGL(lcsub_cand_kernel, dim3(grid), dim3(kBlock), 0, st, chars, subs, nsub, total_tiles, H, elem,
                       carry, L, cap, slots, cnt, ovf, hdr, cand);
    return hipGetLastError();
}

}  // namespace gx
