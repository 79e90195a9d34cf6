// gx_lcsub.h -- what the compare-mode kernels (gx_lcsub.hip) and their host
// driver (gx_api_compare.cpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace gx {

constexpr int kLcsubBlock = 256;        // diagonals per tile (one lane each)
constexpr int kLcsubSeg = 1024;         // rows per segment H (gx_compare_segment_height)
constexpr int kLcsubMaxSeg = 32768;     // the tile element keeps its runs in 16 bits
constexpr unsigned kLcsubCandCap = 64;  // candidate starts kept per sub-problem
constexpr int kLcsubPad = 16;           // bytes between staged sequences

// One sub-problem: a = chars[a_off .. a_off + n), b = chars[b_off .. b_off + m),
// both non-empty.  Diagonal k (0 <= k < ndiag = n + m - 1) is j - i = k - (n - 1).
struct __attribute__((aligned(16))) LcsubDesc {
    uint32_t a_off, b_off, n, m;
    uint32_t ndiag, nseg;        // n + m - 1, ceil(n / H)
    uint32_t tile_base;          // first flat tile (tiles = nseg * ceil(ndiag / 256), segment-major)
    uint32_t dtile_base;         // first flat diagonal block (ceil(ndiag / 256) of them)
    uint64_t elem_base;          // first tile element ([seg][diagonal])
    uint64_t pad;
};
static_assert(sizeof(LcsubDesc) == 48, "LcsubDesc is copied to the device as is");

hipError_t launch_lcsub_run(const uint8_t* chars, const LcsubDesc* subs, int nsub, unsigned total_tiles, int H,
                            uint2* elem, int grid, hipStream_t st);
hipError_t launch_lcsub_combine(const LcsubDesc* subs, int nsub, unsigned total_dtiles, const uint2* elem,
                                unsigned* carry, unsigned* L, int grid, hipStream_t st);
hipError_t launch_lcsub_cand(const uint8_t* chars, const LcsubDesc* subs, int nsub, unsigned total_tiles, int H,
                             const uint2* elem, const unsigned* carry, const unsigned* L, unsigned cap,
                             unsigned slots, unsigned* cnt, unsigned* ovf, unsigned* hdr, uint4* cand, int grid,
                             hipStream_t st);

}  // namespace gx
