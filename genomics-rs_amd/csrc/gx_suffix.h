// gx_suffix.h -- what the suffix-tree mode kernels (gx_suffix.hip) and their
// host driver (gx_api_suffix.cpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace gx {

constexpr int kSufBlock = 256;                          // threads per workgroup of every kernel here
constexpr int kSufItems = 8;                            // items per thread of the sort and scan kernels
constexpr int kSufTile = kSufBlock * kSufItems;         // items per workgroup T (gx_suffix_tile)
constexpr int kSufLcpChunk = 16;                        // text positions per lane C of the LCP kernel
constexpr int kSufFoldBlock = kSufBlock;                // LCP entries per fold block B (one per lane)
constexpr int kSufPad = 16;                             // zero bytes staged behind the text (8-byte loads)

// What the fold leaves for the host (one 32-byte copy).
struct SufFold {
    uint64_t num_internal, depth_sum;
    uint64_t max_key;        // (max LCP << 32) | ~k*, k* = the first k with LCP[k] = max LCP
    uint64_t repeat_start;   // SA[k* - 1] + 1, or 0 when max LCP = 0
};

inline size_t suf_tiles(size_t n) { return (n + kSufTile - 1) / kSufTile; }

// Keys.  masks[0] |= every key, masks[1] &= every key (the caller presets 0 / ~0).
hipError_t launch_suf_keys0(const uint8_t* text, uint32_t N, uint64_t* keys, uint32_t* vals, uint64_t* masks,
                            hipStream_t st);
hipError_t launch_suf_keys(const uint32_t* rank, uint32_t N, uint32_t h, uint64_t* keys, uint32_t* vals,
                           uint64_t* masks, hipStream_t st);
// One radix pass on digit (key >> shift) & 255: table is [256][tiles] uint32,
// scan_tmp holds suf_tiles(256 * tiles) uint32.
hipError_t launch_suf_sort_pass(const uint64_t* kin, const uint32_t* vin, uint64_t* kout, uint32_t* vout, uint32_t N,
                                int shift, uint32_t* table, uint32_t* scan_tmp, hipStream_t st);
// data[0..n) -> its exclusive or inclusive prefix sums in place; tmp holds suf_tiles(n) uint32.
hipError_t launch_suf_scan(uint32_t* data, uint32_t n, bool inclusive, uint32_t* tmp, hipStream_t st);
// Sorted keys -> dense ranks in text order (rank[vals[k]]); flags is N uint32 of
// scratch, *last = the rank of the last sorted suffix.
hipError_t launch_suf_ranks(const uint64_t* keys, const uint32_t* vals, uint32_t N, uint32_t* flags,
                            uint32_t* scan_tmp, uint32_t* rank, uint32_t* last, hipStream_t st);
hipError_t launch_suf_bwt(const uint8_t* text, const uint32_t* sa, uint32_t N, uint8_t* bwt, hipStream_t st);
hipError_t launch_suf_lcp(const uint8_t* text, const uint32_t* sa, const uint32_t* rank, uint32_t N, uint32_t* lcp,
                          hipStream_t st);
// bmin, pcnt, psum, pmax: one entry per fold block (ceil(N / B)).
hipError_t launch_suf_fold(const uint32_t* lcp, const uint32_t* sa, uint32_t N, uint32_t* bmin, uint64_t* pcnt,
                           uint64_t* psum, uint64_t* pmax, SufFold* out, hipStream_t st);

}  // namespace gx
