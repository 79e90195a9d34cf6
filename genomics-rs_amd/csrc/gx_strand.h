// gx_strand.h -- both strands of search mode: the one statement
// of the complement table, the reverse complement and the item batch of a
// caller's batch, read by the host paths (gx_api_search.cpp) and by the kernel
// that writes the reverse items behind the staged forward bytes (gx_strand.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gx_suffix.h"

// (include/gx.h has the same three for callers)
#ifndef GX_STRAND_FWD
#define GX_STRAND_FWD 1u
#define GX_STRAND_REV 2u
#define GX_STRAND_BOTH 3u
#endif

namespace gx {

// The complement of an upper-case IUPAC letter; every other byte is its own.
__host__ __device__ constexpr uint8_t strand_comp_upper(uint8_t u) {
    switch (u) {
        case 'A': return 'T';
        case 'T': return 'A';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'R': return 'Y';
        case 'Y': return 'R';
        case 'K': return 'M';
        case 'M': return 'K';
        case 'B': return 'V';
        case 'V': return 'B';
        case 'D': return 'H';
        case 'H': return 'D';
        default: return u;   // S, W and N pair with themselves; U and every non-letter stay
    }
}

// The table: an involution over all 256 bytes that keeps the case of a letter,
// and so keeps every byte above '$' above it.
__host__ __device__ constexpr uint8_t strand_comp(uint8_t x) {
    return (x >= 'a' && x <= 'z') ? (uint8_t)(strand_comp_upper((uint8_t)(x - 32)) + 32) : strand_comp_upper(x);
}

// rc(P)[j] = strand_comp(P[m - 1 - j]); dst and src do not overlap.
inline void strand_rc(const uint8_t* src, size_t m, uint8_t* dst) {
    for (size_t j = 0; j < m; ++j) dst[j] = strand_comp(src[m - 1 - j]);
}

// Items of a caller's batch of n.
__host__ __device__ inline uint64_t strand_items(uint64_t n, uint32_t strands) { return strands == GX_STRAND_BOTH ? 2 * n : n; }
// ... and the caller's n of a batch of items.
inline uint64_t strand_sources(uint64_t items, uint32_t strands) { return strands == GX_STRAND_BOTH ? items / 2 : items; }

// The item offsets (items + 1) from the caller's (n + 1): FWD and REV keep them
// (rc(P_p) has P_p's length), BOTH appends off'[n + p] = T + off[p].  Closed form: no scan.
template <class In, class Out>
inline void strand_item_offsets(const In* offs, size_t n, uint32_t strands, Out* out) {
    for (size_t p = 0; p <= n; ++p) out[p] = (Out)offs[p];
    if (strands == GX_STRAND_BOTH)
        for (size_t p = 1; p <= n; ++p) out[n + p] = (Out)(offs[n] + offs[p]);
}

// The item bytes: FWD the batch; REV item p = rc(P_p); BOTH the batch, then
// the REV items behind it.  out: strand_items(T) bytes.
template <class Off>
inline void strand_item_bytes(const uint8_t* bytes, const Off* offs, size_t n, uint32_t strands, uint8_t* out) {
    const size_t T = (size_t)offs[n];
    if (strands & GX_STRAND_FWD) {
        if (T) __builtin_memcpy(out, bytes, T);
        out += T;
    }
    if (strands & GX_STRAND_REV)
        for (size_t p = 0; p < n; ++p) strand_rc(bytes + offs[p], (size_t)(offs[p + 1] - offs[p]), out + offs[p]);
}

// The kernel's work unit: an aligned 8-byte word of the output (a lane's one vector store).
constexpr uint32_t kStrandUnit = 8;

// Reverse items of the n items off[0 .. n] of src (T = off[n] bytes) into
// dst[dst_at .. dst_at + T), then kSufPad zero bytes; dst is 8-byte aligned and
// holds dst_at + T + kSufPad bytes rounded up to 8; src may be dst (BOTH:
// dst_at = T) and has T bytes rounded up to 8 readable.  off_out (NULL: none):
// off_out[p] = T + off[p + 1] for p < n, the item offsets behind off[n].
hipError_t launch_strand_rc(const uint8_t* src, const uint32_t* off, uint32_t n, uint32_t T, uint8_t* dst, uint32_t dst_at,
                            uint32_t* off_out, hipStream_t st);
// Work units (lanes' words) of that launch.
inline uint64_t strand_units(uint64_t T, uint64_t dst_at) {
    return (dst_at + T + kSufPad + kStrandUnit - 1) / kStrandUnit - dst_at / kStrandUnit;
}

}  // namespace gx
