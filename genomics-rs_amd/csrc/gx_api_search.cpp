// gx_api_search.cpp -- search mode: a suffix index that outlives the call and
// batched exact-match queries on it, and queries with at most k
// substitutions.  No counterpart in the
// reference's main.rs; it consumes the suffix array suffix-tree mode builds.
//
//   index build    text to device text + device suffix array (suffix_device_sa,
//                  gx_api_suffix.cpp); the index keeps those two buffers out of
//                  the pool and returns the rest.  Below GX_SUFFIX_HOST_BELOW
//                  the host solver's array is uploaded.  ctx = NULL: both stay
//                  on the host.
//   host search    srch_one (gx_search.h) per pattern: the checker on a
//                  CPU-only machine and the baseline
//   device search  stage patterns and offsets, interval kernel, and for
//                  positions clamp, exclusive scan and gather (gx_search.hip);
//                  the per-pattern ascending sort is the host's
//   approximate    both sides: the k + 1 pieces of every pattern through the
//                  exact search (the seeds), the seed hits summed in 64 bits and
//                  held against GX_APPROX_CAND_BUDGET, then the verify walk of
//                  gx_approx.h on every seed hit.  Device: gx_approx.hip
//   edit           k differences, both sides: the same seeds, the
//                  band of gx_edit.h on every seed hit, the reported ends sorted
//                  and each run's minimum kept, then the starts of the reported
//                  occurrences.  Device: gx_edit.hip
//   shared stages  what the three searches and the long-query calls of
//                  gx_api_match.cpp have in common: the batch
//                  checker, the prologue of the entry points, stage_batch, the
//                  seeds of both sides, the epilogue that copies exactly the total
#include "gx_api_call.h"
#include "gx_approx.h"
#include "gx_edit.h"
#include "gx_search.h"
#include "gx_strand.h"

// ---------------------------------------------------------------------------
// shared with gx_api_match.cpp (declared in gx_api.h and gx_api_call.h)

// GX_APPROX_CAND_BUDGET, read on every call: seed hits a batch may have (gx_api.h: the MEM search holds its
// candidates against it too).
uint64_t approx_budget() {
    uint64_t b = 1ull << 27;
    if (const char* e = getenv("GX_APPROX_CAND_BUDGET")) {
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && v > 0) b = v;
    }
    return std::min<uint64_t>(b, 1ull << 31);
}

// What every call of search mode refuses of a batch before a byte is staged.
int check_batch(const BatchKind& kind, const uint8_t* bytes, const uint64_t* offsets, size_t n, uint32_t strands) {
    const std::string noun = kind.noun;
    if (offsets[0] != 0) return fail(GX_EINVAL, "offsets[0] is not 0");
    for (size_t p = 0; p < n; ++p) {
        if (offsets[p + 1] < offsets[p]) return fail(GX_EINVAL, "offsets decrease at " + noun + " " + std::to_string(p));
        if (kind.item_max && offsets[p + 1] - offsets[p] > kind.item_max)
            return fail(GX_ERANGE, noun + " " + std::to_string(p) + " has " + std::to_string(offsets[p + 1] - offsets[p]) +
                                       " bytes, more than " + std::to_string(kind.item_max));
    }
    const uint64_t total = offsets[n];
    if (kind.positions) {
        // (the device's offsets and scans are 32-bit: the positions plus one, the scan's tile rounding and the padding)
        if (total + kSufTile + kSufPad >= (1ull << 32) || (uint64_t)n + 1 + kSufTile >= (1ull << 32))
            return fail(GX_ERANGE, "match: " + std::to_string(total) + " query bytes in " + std::to_string(n) +
                                       " queries, 2^32 or more with the padding and the scan's tile rounding: split the batch");
    } else {
        // (one more than the 32-bit device offsets need, for the scan's n + 1 entries and its tile rounding)
        if (total + n >= (1ull << 32) || (uint64_t)n + 1 + kSufTile >= (1ull << 32))
            return fail(GX_ERANGE, "search: pattern bytes plus patterns come to " + std::to_string(total + n) +
                                       ", 2^32 or more: split the batch or lower max_hits");
    }
    if (strands != GX_STRAND_FWD) {
        // the same conditions on the item batch's totals, here with the batch's own: before a byte is read
        const uint64_t items = strand_items(n, strands), itotal = strand_items(total, strands);
        if (kind.positions ? itotal + kSufTile + kSufPad >= (1ull << 32) || items + 1 + kSufTile >= (1ull << 32)
                           : itotal + items >= (1ull << 32) || items + 1 + kSufTile >= (1ull << 32))
            return fail(GX_ERANGE, "strands: " + std::to_string(itotal) + " item bytes in " + std::to_string(items) +
                                       " items (the batch has " + std::to_string(total) + " bytes in " + std::to_string(n) +
                                       "), 2^32 or more with what the device adds: split the batch");
    }
    if (total && !bytes) return fail(GX_EINVAL, std::string(kind.plural) + " is NULL");
    // (one flat pass the compiler vectorises; the culprit is looked for only when there is one)
    unsigned low = 0;
    for (uint64_t k = 0; k < total; ++k) low |= bytes[k] <= 0x24;
    for (size_t p = 0; low && p < n; ++p)
        for (uint64_t k = offsets[p]; k < offsets[p + 1]; ++k)
            if (bytes[k] <= 0x24)
                return fail(GX_EINVAL, noun + " " + std::to_string(p) + ": byte " + std::to_string((int)bytes[k]) +
                                           " at offset " + std::to_string(k - offsets[p]) + " is not above '$'");
    return GX_OK;
}

void narrow_batch(const gx_suffix_index* idx, const uint8_t* bytes, const uint64_t* offsets, size_t n, HostBatch& b) {
    b.offs.resize(n + 1);
    for (size_t p = 0; p <= n; ++p) b.offs[p] = (uint32_t)offsets[p];
    if (idx->ctx) return;
    // the host compares read 8 bytes at a time too: the same padding behind the bytes
    const uint64_t total = offsets[n];
    b.padded.assign(total + kSufPad, 0);
    if (total) memcpy(b.padded.data(), bytes, total);
}

int stage_batch(DevCall& call, const char* what, const uint8_t* src, size_t total_bytes, const uint32_t* offs, uint32_t n,
                StagedBatch& b) {
    uint8_t* bytes = nullptr;
    uint32_t* off = nullptr;
    GX_GET(call, bytes, total_bytes + kSufPad);
    GX_GET(call, off, (size_t)n + 1);
    GX_GET(call, b.cnt, 8);
    // (no copy of 0 bytes from a pointer that may be NULL)
    if (total_bytes) GX_TRY(call, hipMemcpyAsync(bytes, src, total_bytes, hipMemcpyHostToDevice, call.st));
    GX_TRY(call, hipMemsetAsync(bytes + total_bytes, 0, kSufPad, call.st));
    GX_TRY(call, hipMemcpyAsync(off, offs, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, call.st));
    GX_TRY(call, hipMemsetAsync(b.cnt, 0, 64, call.st));
    b.pin = (unsigned long long*)io_pinned(call.ctx, 128);
    if (!b.pin) return call.done(fail(GX_ENOMEM, std::string(what) + ": pinned staging"));
    b.bytes = bytes;
    b.off = off;
    call.ctx->strand_items = n;
    call.ctx->strand_rc_bytes = 0;
    call.ctx->strand_timed = false;
    return GX_OK;
}

// ---------------------------------------------------------------------------
// both strands: the item batch of a caller's batch, on the host
// by gx_strand.h's loops and on the device by gx_strand.hip behind the one copy

int check_strands(uint32_t strands) {
    if (strands < GX_STRAND_FWD || strands > GX_STRAND_BOTH)
        return fail(GX_EINVAL, "strands is " + std::to_string(strands) + ", not 1 (forward), 2 (reverse) or 3 (both)");
    return GX_OK;
}

void strand_batch(const gx_suffix_index* idx, const uint8_t* bytes, const uint64_t* offsets, size_t n, uint32_t strands,
                  HostBatch& b) {
    if (strands == GX_STRAND_FWD) return narrow_batch(idx, bytes, offsets, n, b);
    // (check_batch has held the item batch's totals against the 32-bit conditions)
    const uint64_t items = strand_items(n, strands), total = strand_items(offsets[n], strands);
    b.offs.resize(items + 1);
    strand_item_offsets(offsets, n, strands, b.offs.data());
    if (idx->ctx) return;
    b.padded.assign(total + kSufPad, 0);
    strand_item_bytes(bytes, offsets, n, strands, b.padded.data());
}

int stage_batch_strands(DevCall& call, const char* what, const uint8_t* src, size_t total_bytes, const uint32_t* offs,
                        uint32_t n, uint32_t strands, StagedBatch& b) {
    if (strands == GX_STRAND_FWD) return stage_batch(call, what, src, total_bytes, offs, n, b);
    gx_context* ctx = call.ctx;
    const bool both = strands == GX_STRAND_BOTH;
    const size_t at = both ? total_bytes : 0, items = (size_t)strand_items(n, strands);
    uint8_t *bytes = nullptr, *fwd = nullptr;
    uint32_t* off = nullptr;
    // (the kernel's aligned 8-byte loads may read up to 7 bytes behind the forward bytes)
    GX_GET(call, bytes, align_up(at + total_bytes + kSufPad, 8));
    if (both) fwd = bytes;
    else GX_GET(call, fwd, align_up(total_bytes, 8) + 8);
    GX_GET(call, off, items + 1);
    GX_GET(call, b.cnt, 8);
    if (total_bytes) GX_TRY(call, hipMemcpyAsync(fwd, src, total_bytes, hipMemcpyHostToDevice, call.st));
    GX_TRY(call, hipMemcpyAsync(off, offs, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, call.st));
    GX_TRY(call, hipMemsetAsync(b.cnt, 0, 64, call.st));
    // the reverse items, the padding behind them and, for both strands, the offsets behind off[n]
    GX_TRY(call, hipEventRecord(ctx->ev_rc0, call.st));
    GX_TRY(call, launch_strand_rc(fwd, off, n, (uint32_t)total_bytes, bytes, (uint32_t)at, both ? off + n + 1 : nullptr, call.st));
    GX_TRY(call, hipEventRecord(ctx->ev_rc1, call.st));
    b.pin = (unsigned long long*)io_pinned(ctx, 128);
    if (!b.pin) return call.done(fail(GX_ENOMEM, std::string(what) + ": pinned staging"));
    b.bytes = bytes;
    b.off = off;
    ctx->strand_items = items;
    ctx->strand_rc_bytes = total_bytes;
    ctx->strand_timed = true;
    return GX_OK;
}

namespace {

static_assert(sizeof(gx_search_hit) == sizeof(SrchHit), "gx_search_hit layout");

constexpr BatchKind kPatterns{"pattern", "patterns", kSrchMaxPattern, false};

// hit_offsets from hits (gx_search_hit, gx_approx_hit or gx_edit_hit); returns the total.
template <class Hit>
uint64_t offsets_of(const Hit* hits, size_t npat, uint32_t max_hits, uint64_t* hit_offsets) {
    uint64_t tot = 0;
    for (size_t p = 0; p < npat; ++p) {
        if (hit_offsets) hit_offsets[p] = tot;
        tot += std::min(hits[p].count, max_hits);
    }
    if (hit_offsets) hit_offsets[npat] = tot;
    return tot;
}

int cap_error(uint64_t total, size_t cap) {
    return fail(GX_ECAP, "search: " + std::to_string(total) + " positions needed, positions_cap is " +
                             std::to_string(cap));
}

int total_error(uint64_t total) {
    return fail(GX_ERANGE, "search: " + std::to_string(total) +
                               " reported positions, 2^32 or more: split the batch or lower max_hits");
}

// One output array of a device search: the caller's (NULL: not asked for) and the device's, bytes per entry.
struct OutCopy {
    void* dst;
    const void* src;
    size_t elem;
};

// The end of a device search, hits[] already on the host and the stream idle: hit_offsets from the hits, and
// when the first output is asked for, the refusals and the copy of exactly the total into every output that
// is.  Only now is that number known to the host, so that GX_ECAP leaves the outputs untouched and the copies
// move no more than them (a total above what the device reserved is above cap).
template <class Hit>
int finish_hits(DevCall& call, const Hit* hits, uint32_t npat, uint32_t max_hits, bool limit32, size_t cap,
                uint64_t* hit_offsets, std::initializer_list<OutCopy> out) {
    if (!out.begin()->dst) {
        if (hit_offsets) offsets_of(hits, npat, max_hits, hit_offsets);
        return call.done(GX_OK);
    }
    const uint64_t total = offsets_of(hits, npat, max_hits, hit_offsets);
    if (limit32 && total >= (1ull << 32)) return call.done(total_error(total));
    if (total > cap) return call.done(cap_error(total, cap));
    if (total) {
        for (const OutCopy& c : out)
            if (c.dst) GX_TRY(call, hipMemcpyAsync(c.dst, c.src, (size_t)total * c.elem, hipMemcpyDeviceToHost, call.st));
        GX_TRY(call, hipStreamSynchronize(call.st));
    }
    return call.done(GX_OK);   // (the stream is idle)
}

void sort_segments(uint32_t* positions, const uint64_t* hit_offsets, size_t npat) {
    for (size_t p = 0; p < npat; ++p)
        if (hit_offsets[p + 1] - hit_offsets[p] > 1) std::sort(positions + hit_offsets[p], positions + hit_offsets[p + 1]);
}

int search_host(const gx_suffix_index* idx, const uint8_t* pats, const uint32_t* offs, size_t npat, gx_search_hit* hits,
                uint32_t max_hits, uint32_t* positions, size_t cap, uint64_t* hit_offsets) {
    const uint32_t N = (uint32_t)idx->n + 1;
    uint64_t words = 0;
    for (size_t p = 0; p < npat; ++p) {
        const SrchHit h = srch_one(idx->text.data(), idx->sa.data(), N, pats + offs[p], offs[p + 1] - offs[p], &words);
        hits[p] = gx_search_hit{h.lo, h.count, h.prefix_len, h.prefix_pos};
    }
    if (!positions) {
        if (hit_offsets) offsets_of(hits, npat, max_hits, hit_offsets);
        return GX_OK;
    }
    const uint64_t total = offsets_of(hits, npat, max_hits, hit_offsets);
    if (total >= (1ull << 32)) return total_error(total);
    if (total > cap) return cap_error(total, cap);
    for (size_t p = 0; p < npat; ++p)
        memcpy(positions + hit_offsets[p], idx->sa.data() + hits[p].lo, (hit_offsets[p + 1] - hit_offsets[p]) * 4);
    sort_segments(positions, hit_offsets, npat);
    return GX_OK;
}

// pats: the caller's total_bytes pattern bytes, unpadded (the kSufPad zero bytes behind them are set on
// the device); offs, npat: the item batch of those on `strands`.  Takes ctx->mu.
int search_device(gx_suffix_index* idx, const uint8_t* pats, size_t total_bytes, const uint32_t* offs, uint32_t npat,
                  uint32_t strands, gx_search_hit* hits, uint32_t max_hits, uint32_t* positions, size_t cap, uint64_t* hit_offsets) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    hipStream_t st = call.st;
    const uint32_t N = (uint32_t)idx->n + 1;
    ctx->srch_words = 0;
    ctx->srch_ms = ctx->srch_locate_ms = 0.0;
    // 1. patterns and offsets, kSufPad zero bytes behind the patterns
    StagedBatch b;
    if (const int rc = stage_batch_strands(call, "search", pats, total_bytes, offs, (uint32_t)strand_sources(npat, strands), strands, b)) return rc;
    SrchHit* d_h = nullptr;
    GX_GET(call, d_h, npat);
    // 2. the interval kernel
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_srch_range(text, sa, N, b.bytes, b.off, npat, d_h, b.cnt, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    // what the positions can come to at most; the device's offsets are 32-bit,
    // so a batch that could reach 2^32 is summed on the host before the scan
    const uint64_t bound = (uint64_t)npat * std::min(max_hits, N);
    uint64_t dev_cap = std::min<uint64_t>(cap, bound);
    bool copied = false, located = false;
    uint32_t* d_pos = nullptr;
    if (positions && bound >= (1ull << 32)) {
        GX_TRY(call, hipMemcpyAsync(b.pin, b.cnt, 8, hipMemcpyDeviceToHost, st));
        GX_TRY(call, hipMemcpyAsync(hits, d_h, (size_t)npat * sizeof(SrchHit), hipMemcpyDeviceToHost, st));
        GX_TRY(call, hipStreamSynchronize(st));
        copied = true;
        call.elapsed(ctx->ev0, ctx->ev1, &ctx->srch_ms);
        const uint64_t total = offsets_of(hits, npat, max_hits, nullptr);
        if (total >= (1ull << 32)) {
            offsets_of(hits, npat, max_hits, hit_offsets);
            ctx->srch_words = b.pin[0];
            return call.done(total_error(total));
        }
        dev_cap = total <= cap ? total : 0;   // (the total is known here; above cap it is GX_ECAP below)
        if (dev_cap) GX_TRY(call, hipEventRecord(ctx->ev1, st));   // the locate step starts here
    }
    if (positions && dev_cap) {
        // 3. clamp, exclusive scan, gather: nothing else between ev1 and ev2
        uint32_t *q = nullptr, *tmp = nullptr;
        GX_GET(call, q, (size_t)npat + 1);
        GX_GET(call, tmp, suf_tiles((size_t)npat + 1));
        GX_GET(call, d_pos, (size_t)dev_cap);
        GX_TRY(call, launch_srch_clamp(d_h, npat, max_hits, q, st));
        GX_TRY(call, launch_suf_scan(q, npat + 1, false, tmp, st));
        GX_TRY(call, launch_srch_gather(sa, N, d_h, q, npat, d_pos, dev_cap, st));
        GX_TRY(call, hipEventRecord(ctx->ev2, st));
        located = true;
    }
    if (!copied) {
        // (behind the last event, as suffix_device's copies: the events time kernels alone)
        GX_TRY(call, hipMemcpyAsync(b.pin, b.cnt, 8, hipMemcpyDeviceToHost, st));
        GX_TRY(call, hipMemcpyAsync(hits, d_h, (size_t)npat * sizeof(SrchHit), hipMemcpyDeviceToHost, st));
    }
    GX_TRY(call, hipStreamSynchronize(st));
    if (!copied) call.elapsed(ctx->ev0, ctx->ev1, &ctx->srch_ms);
    if (located) call.elapsed(ctx->ev1, ctx->ev2, &ctx->srch_locate_ms);
    ctx->srch_words = b.pin[0];
    // 4. the positions
    const int rc = finish_hits(call, hits, npat, max_hits, true, cap, hit_offsets, {{positions, d_pos, 4}});
    if (rc == GX_OK && positions) sort_segments(positions, hit_offsets, npat);
    return rc;
}

// ---------------------------------------------------------------------------
// k mismatches: pigeonhole seeds through the exact search, then
// the verify walk of gx_approx.h on every seed hit, host and device alike

static_assert(sizeof(gx_approx_hit) == sizeof(AprxHit), "gx_approx_hit layout");
static_assert(GX_APPROX_MAX_K == kAprxMaxK, "GX_APPROX_MAX_K");

// what: "approximate search" or "edit search".
int seed_budget_error(const char* what, uint64_t total, uint64_t budget) {
    return fail(GX_ERANGE, std::string(what) + ": " + std::to_string(total) + " seed hits, more than GX_APPROX_CAND_BUDGET = " +
                               std::to_string(budget) + ": split the batch, lower k, or raise GX_APPROX_CAND_BUDGET");
}

// A budget refusal's only output: candidates per pattern from the pieces' intervals (gx_approx_hit or gx_edit_hit).
template <class Hit>
void candidates_only(const SrchHit* ph, size_t npat, uint32_t k1, Hit* hits) {
    for (size_t p = 0; p < npat; ++p) {
        uint64_t c = 0;
        for (uint32_t j = 0; j < k1; ++j) c += ph[p * k1 + j].count;
        hits[p].candidates = (uint32_t)std::min<uint64_t>(c, 0xFFFFFFFFull);
    }
}

// The seeds on the host: every piece of every pattern through the exact search, in candidate order, into ph[];
// returns their 64-bit total.  pats: padded as for search_host.
uint64_t seed_pieces_host(const gx_suffix_index* idx, const uint8_t* pats, const uint32_t* offs, size_t npat, uint32_t k1,
                          std::vector<SrchHit>& ph, uint64_t* words) {
    const uint32_t N = (uint32_t)idx->n + 1;
    ph.resize(npat * k1);
    uint64_t total = 0;
    for (size_t p = 0; p < npat; ++p) {
        const uint32_t m = offs[p + 1] - offs[p];
        for (uint32_t j = 0; j < k1; ++j) {
            const uint32_t ps = aprx_piece_start(m, k1, j), pe = aprx_piece_start(m, k1, j + 1);
            ph[p * k1 + j] = srch_one(idx->text.data(), idx->sa.data(), N, pats + offs[p] + ps, pe - ps, words);
            total += ph[p * k1 + j].count;
        }
    }
    return total;
}

// The seeds on the device, DESIGN.md 19.2 stages 1 to 4: piece offsets, the pieces' intervals, their 64-bit
// total, candidate offsets.
struct DevSeeds {
    uint32_t* poff = nullptr;   // npieces + 1 piece offsets
    SrchHit* ph = nullptr;      // the pieces' intervals
    uint32_t* coff = nullptr;   // npieces + 1 candidate offsets: relied upon only once the host has held the total
                                // against the budget (the scan is 32-bit)
    uint32_t* tmp = nullptr;    // the scan's, suf_tiles(npieces + 1) words
    uint64_t total = 0;         // seed hits, also in b.pin[1] (b.pin[0]: the seeds' word steps)
};
// Between ev0 and ev1, then the read-back of the total; *seed_ms: the kernels alone.  Returns with the stream
// idle; the budget is the caller's to hold the total against.
int seed_pieces_device(DevCall& call, const gx_suffix_index* idx, const StagedBatch& b, uint32_t npat, uint32_t k1,
                       double* seed_ms, DevSeeds& s) {
    gx_context* ctx = call.ctx;
    hipStream_t st = call.st;
    const uint32_t N = (uint32_t)idx->n + 1, npieces = npat * k1;
    GX_GET(call, s.poff, (size_t)npieces + 1);
    GX_GET(call, s.ph, npieces);
    GX_GET(call, s.coff, (size_t)npieces + 1);
    GX_GET(call, s.tmp, suf_tiles((size_t)npieces + 1));
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_aprx_pieces(b.off, npat, k1, s.poff, st));
    GX_TRY(call, launch_srch_range((const uint8_t*)idx->d_text.p, (const uint32_t*)idx->d_sa.p, N, b.bytes, s.poff, npieces,
                                   s.ph, b.cnt, st));
    GX_TRY(call, launch_aprx_total(s.ph, npieces, b.cnt + 1, st));
    GX_TRY(call, launch_srch_clamp(s.ph, npieces, 0xFFFFFFFFu, s.coff, st));
    GX_TRY(call, launch_suf_scan(s.coff, npieces + 1, false, s.tmp, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    GX_TRY(call, hipMemcpyAsync(b.pin, b.cnt, 16, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev0, ctx->ev1, seed_ms);
    s.total = b.pin[1];
    return GX_OK;
}

// A budget refusal on the device: candidates_only from the pieces' intervals, then `rc` (the refusal, already
// in gx_last_error) through done(); a failing read-back is reported in its place.
template <class Hit>
int refuse_device(DevCall& call, const DevSeeds& s, uint32_t npat, uint32_t k1, Hit* hits, int rc) {
    std::vector<SrchHit> hp((size_t)npat * k1);
    GX_TRY(call, hipMemcpyAsync(hp.data(), s.ph, hp.size() * sizeof(SrchHit), hipMemcpyDeviceToHost, call.st));
    GX_TRY(call, hipStreamSynchronize(call.st));
    candidates_only(hp.data(), npat, k1, hits);
    return call.done(rc);
}

// Each pattern's (position, distance) pairs ascending by position (positions are distinct within a pattern).
void sort_pairs(uint32_t* positions, uint8_t* distances, const uint64_t* hit_offsets, size_t npat) {
    std::vector<uint64_t> tmp;
    for (size_t p = 0; p < npat; ++p) {
        const uint64_t b = hit_offsets[p], len = hit_offsets[p + 1] - b;
        if (len < 2) continue;
        tmp.resize(len);
        for (uint64_t i = 0; i < len; ++i) tmp[i] = (uint64_t)positions[b + i] << 8 | distances[b + i];
        std::sort(tmp.begin(), tmp.end());
        for (uint64_t i = 0; i < len; ++i) {
            positions[b + i] = (uint32_t)(tmp[i] >> 8);
            distances[b + i] = (uint8_t)tmp[i];
        }
    }
}

// pats: padded as for search_host.
int approx_host(const gx_suffix_index* idx, const uint8_t* pats, const uint32_t* offs, size_t npat, uint32_t k,
                gx_approx_hit* hits, uint32_t max_hits, uint32_t* positions, uint8_t* distances, size_t cap,
                uint64_t* hit_offsets) {
    const uint32_t n = (uint32_t)idx->n, k1 = k + 1;
    const uint8_t* t = idx->text.data();
    const uint32_t* sa = idx->sa.data();
    std::vector<SrchHit> ph;
    uint64_t words = 0;
    const uint64_t total = seed_pieces_host(idx, pats, offs, npat, k1, ph, &words), budget = approx_budget();
    if (total > budget) {
        candidates_only(ph.data(), npat, k1, hits);
        return seed_budget_error("approximate search", total, budget);
    }
    std::vector<uint64_t> out;   // position << 8 | distance, the reported ones of every pattern in turn
    for (size_t p = 0; p < npat; ++p) {
        const uint32_t m = offs[p + 1] - offs[p];
        const uint8_t* P = pats + offs[p];
        gx_approx_hit h{0, 0xFFFFFFFFu, 0, 0};
        uint64_t best = ~0ull;
        for (uint32_t j = 0; j < k1; ++j) {
            const SrchHit& s = ph[p * k1 + j];
            const uint32_t ps = aprx_piece_start(m, k1, j);
            h.candidates += s.count;
            for (uint32_t r = 0; r < s.count; ++r) {
                const uint32_t at = sa[s.lo + r];
                if (at < ps || (uint64_t)(at - ps) + m > n) continue;   // the window leaves the text
                const uint32_t c = at - ps;
                uint32_t d = 0;
                if (!aprx_verify(t + c, P, m, k, j, &d, &words)) continue;
                best = std::min(best, (uint64_t)d << 32 | c);
                if (positions && h.count < max_hits) out.push_back((uint64_t)c << 8 | d);
                ++h.count;
            }
        }
        if (h.count) {
            h.best_dist = (uint32_t)(best >> 32);
            h.best_pos = (uint32_t)best;
        }
        hits[p] = h;
    }
    if (!positions) {
        if (hit_offsets) offsets_of(hits, npat, max_hits, hit_offsets);
        return GX_OK;
    }
    const uint64_t total_out = offsets_of(hits, npat, max_hits, hit_offsets);
    if (total_out > cap) return cap_error(total_out, cap);
    for (uint64_t i = 0; i < total_out; ++i) {
        positions[i] = (uint32_t)(out[i] >> 8);
        distances[i] = (uint8_t)out[i];
    }
    sort_pairs(positions, distances, hit_offsets, npat);
    return GX_OK;
}

// pats: unpadded, as for search_device.  Takes ctx->mu.
int approx_device(gx_suffix_index* idx, const uint8_t* pats, size_t total_bytes, const uint32_t* offs, uint32_t npat,
                  uint32_t strands, uint32_t k, gx_approx_hit* hits, uint32_t max_hits, uint32_t* positions, uint8_t* distances, size_t cap,
                  uint64_t* hit_offsets) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    hipStream_t st = call.st;
    const uint32_t N = (uint32_t)idx->n + 1, k1 = k + 1, npieces = npat * k1;
    ctx->aprx_cands = ctx->aprx_words = 0;
    ctx->aprx_seed_ms = ctx->aprx_verify_ms = 0.0;
    // patterns and offsets as the exact search stages them; counters: [0] seed word steps, [1] seed hits,
    // [2] verify word steps
    StagedBatch b;
    if (const int rc = stage_batch_strands(call, "approximate search", pats, total_bytes, offs, (uint32_t)strand_sources(npat, strands), strands, b)) return rc;
    DevSeeds s;
    if (const int rc = seed_pieces_device(call, idx, b, npat, k1, &ctx->aprx_seed_ms, s)) return rc;
    const uint64_t total = s.total, budget = approx_budget();
    ctx->aprx_cands = total;
    if (total > budget) return refuse_device(call, s, npat, k1, hits, seed_budget_error("approximate search", total, budget));
    // stages 5 and 6: verify, compact
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    const uint32_t T = (uint32_t)total;   // <= 2^31
    const uint64_t dev_cap =
        positions ? std::min<uint64_t>(std::min<uint64_t>(cap, total), (uint64_t)npat * std::min(max_hits, N)) : 0;
    uint32_t *keep = nullptr, *ktmp = nullptr, *start = nullptr, *oq = nullptr, *d_pos = nullptr;
    uint8_t *dist = nullptr, *d_dst = nullptr;
    unsigned long long* best = nullptr;
    AprxHit* d_hits = nullptr;
    GX_GET(call, keep, (size_t)T + 1);
    GX_GET(call, ktmp, suf_tiles((size_t)T + 1));
    GX_GET(call, dist, std::max<size_t>(T, 1));
    GX_GET(call, start, std::max<size_t>(T, 1));
    GX_GET(call, best, npat);
    GX_GET(call, d_hits, npat);
    GX_GET(call, oq, (size_t)npat + 1);
    if (dev_cap) {
        GX_GET(call, d_pos, (size_t)dev_cap);
        GX_GET(call, d_dst, (size_t)dev_cap);
    }
    GX_TRY(call, hipMemsetAsync(best, 0xFF, (size_t)npat * 8, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    GX_TRY(call, launch_aprx_verify(text, sa, N, b.bytes, b.off, s.poff, s.ph, s.coff, npieces, k, T, keep, dist, start, best,
                                    b.cnt + 2, st));
    GX_TRY(call, launch_suf_scan(keep, T + 1, false, ktmp, st));
    GX_TRY(call, launch_aprx_fill(s.coff, keep, best, npat, k1, max_hits, d_hits, oq, st));
    if (dev_cap) {
        GX_TRY(call, launch_suf_scan(oq, npat + 1, false, s.tmp, st));
        GX_TRY(call, launch_aprx_scatter(s.coff, keep, oq, npat, k1, T, max_hits, start, dist, d_pos, d_dst, dev_cap, st));
    }
    GX_TRY(call, hipEventRecord(ctx->ev2, st));
    // (behind the last event: the events time kernels alone)
    GX_TRY(call, hipMemcpyAsync(b.pin + 2, b.cnt + 2, 8, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(hits, d_hits, (size_t)npat * sizeof(AprxHit), hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev1, ctx->ev2, &ctx->aprx_verify_ms);
    ctx->aprx_words = b.pin[2];
    const int rc = finish_hits(call, hits, npat, max_hits, false, cap, hit_offsets, {{positions, d_pos, 4}, {distances, d_dst, 1}});
    if (rc == GX_OK && positions) sort_pairs(positions, distances, hit_offsets, npat);
    return rc;
}

// ---------------------------------------------------------------------------
// k differences: the same seeds, then the band of gx_edit.h on
// every seed hit, the reported (pattern, end, distance) triples sorted and the
// minimum taken over every run of equal ends, host and device alike

static_assert(sizeof(gx_edit_hit) == sizeof(EditHit), "gx_edit_hit layout");
static_assert(GX_EDIT_MAX_M == kEditMaxM, "GX_EDIT_MAX_M");

int edit_ends_error(uint64_t total, uint64_t budget) {
    return fail(GX_ERANGE, "edit search: " + std::to_string(total) +
                               " reported ends before dedupe, more than GX_APPROX_CAND_BUDGET = " + std::to_string(budget) +
                               ": split the batch, lower k, or raise GX_APPROX_CAND_BUDGET");
}

// pats: padded as for search_host.
int edit_host(const gx_suffix_index* idx, const uint8_t* pats, const uint32_t* offs, size_t npat, uint32_t k,
              gx_edit_hit* hits, uint32_t max_hits, uint32_t* ends, uint8_t* distances, uint32_t* starts, size_t cap,
              uint64_t* hit_offsets) {
    const uint32_t n = (uint32_t)idx->n, k1 = k + 1;
    const uint8_t* t = idx->text.data();
    const uint32_t* sa = idx->sa.data();
    std::vector<SrchHit> ph;
    uint64_t words = 0, cells = 0;
    const uint64_t total = seed_pieces_host(idx, pats, offs, npat, k1, ph, &words), budget = approx_budget();
    if (total > budget) {
        candidates_only(ph.data(), npat, k1, hits);
        return seed_budget_error("edit search", total, budget);
    }
    // verify: every reported (pattern << 32 | end, distance), in candidate order
    std::vector<std::pair<uint64_t, uint32_t>> rep;
    for (size_t p = 0; p < npat; ++p) {
        const uint32_t m = offs[p + 1] - offs[p];
        for (uint32_t j = 0; j < k1; ++j) {
            const SrchHit& s = ph[p * k1 + j];
            const uint32_t ps = aprx_piece_start(m, k1, j);
            for (uint32_t r = 0; r < s.count; ++r) {
                const int64_t d0 = (int64_t)sa[s.lo + r] - (int64_t)ps;
                if (!edit_diag_ok(d0, n, m, k)) continue;
                uint32_t mk = 0;
                uint64_t nb = 0;
                if (!edit_band_host(t, n, pats + offs[p], m, k, (int32_t)d0, &mk, &nb, &cells)) continue;
                for (uint32_t sl = 0; sl < 2 * k + 1; ++sl)
                    if ((mk >> sl) & 1u)
                        rep.emplace_back((uint64_t)p << 32 | (uint32_t)((int64_t)m + d0 - k + sl), edit_slot_dist(mk, nb, sl));
                if (rep.size() > budget) {
                    // (the device sums every candidate's ends before it refuses; the host stops at the first one over)
                    candidates_only(ph.data(), npat, k1, hits);
                    return edit_ends_error(rep.size(), budget);
                }
            }
        }
    }
    // dedupe: sorted by key, candidate order kept within a run; a head takes its run's minimum
    std::stable_sort(rep.begin(), rep.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    const uint64_t E = rep.size();
    std::vector<uint64_t> keys(E);
    std::vector<uint32_t> vals(E);
    for (uint64_t i = 0; i < E; ++i) {
        keys[i] = rep[i].first;
        vals[i] = rep[i].second;
    }
    rep = std::vector<std::pair<uint64_t, uint32_t>>();
    std::vector<uint64_t> out;   // end << 8 | distance, the reported ones of every pattern in turn
    const uint32_t bound = edit_run_bound(k);
    uint64_t i = 0;
    for (size_t p = 0; p < npat; ++p) {
        gx_edit_hit h{0, 0xFFFFFFFFu, 0, 0};
        for (uint32_t j = 0; j < k1; ++j) h.candidates += ph[p * k1 + j].count;
        uint64_t best = ~0ull;
        for (; i < E && (keys[i] >> 32) == p; ++i) {
            if (i && keys[i - 1] == keys[i]) continue;   // not a head
            const uint32_t d = edit_run_min(keys.data(), vals.data(), i, E, bound), e = (uint32_t)keys[i];
            best = std::min(best, (uint64_t)d << 32 | e);
            if (ends && h.count < max_hits) out.push_back((uint64_t)e << 8 | d);
            ++h.count;
        }
        if (h.count) {
            h.best_dist = (uint32_t)(best >> 32);
            h.best_end = (uint32_t)best;
        }
        hits[p] = h;
    }
    if (!ends) {
        if (hit_offsets) offsets_of(hits, npat, max_hits, hit_offsets);
        return GX_OK;
    }
    const uint64_t total_out = offsets_of(hits, npat, max_hits, hit_offsets);
    if (total_out > cap) return cap_error(total_out, cap);
    for (size_t p = 0; p < npat; ++p)
        for (uint64_t o = hit_offsets[p]; o < hit_offsets[p + 1]; ++o) {
            ends[o] = (uint32_t)(out[o] >> 8);
            distances[o] = (uint8_t)out[o];
            if (starts)
                starts[o] = edit_start_host(t, ends[o], pats + offs[p], offs[p + 1] - offs[p], k, distances[o], &cells);
        }
    return GX_OK;
}

// pats: unpadded, as for search_device.  Takes ctx->mu.
int edit_device(gx_suffix_index* idx, const uint8_t* pats, size_t total_bytes, const uint32_t* offs, uint32_t npat,
                uint32_t strands, uint32_t k, gx_edit_hit* hits, uint32_t max_hits, uint32_t* ends, uint8_t* distances, uint32_t* starts,
                size_t cap, uint64_t* hit_offsets) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    hipStream_t st = call.st;
    const uint32_t n = (uint32_t)idx->n, N = n + 1, k1 = k + 1, npieces = npat * k1;
    ctx->edit_cands = ctx->edit_ends = ctx->edit_cells = 0;
    ctx->edit_seed_ms = ctx->edit_verify_ms = ctx->edit_dedupe_ms = 0.0;
    // counters: [0] seed word steps, [1] seed hits, [2] ends before dedupe, [3] cell updates
    StagedBatch b;
    if (const int rc = stage_batch_strands(call, "edit search", pats, total_bytes, offs, (uint32_t)strand_sources(npat, strands), strands, b)) return rc;
    // pieces, seeds, their 64-bit total, candidate offsets: DESIGN.md 19.2 stages 1 to 4
    DevSeeds s;
    if (const int rc = seed_pieces_device(call, idx, b, npat, k1, &ctx->edit_seed_ms, s)) return rc;
    const uint64_t total = s.total, budget = approx_budget();
    ctx->edit_cands = total;
    if (total > budget) return refuse_device(call, s, npat, k1, hits, seed_budget_error("edit search", total, budget));
    // the band on every candidate; what it reports is summed in 64 bits and held against the budget
    // before the 32-bit scan of the numbers is relied upon
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    const uint32_t T = (uint32_t)total;   // <= 2^31
    uint32_t *ecnt = nullptr, *etmp = nullptr, *rep = nullptr;
    uint64_t* nib = nullptr;
    GX_GET(call, ecnt, (size_t)T + 1);
    GX_GET(call, etmp, suf_tiles((size_t)T + 1));
    GX_GET(call, rep, std::max<size_t>(T, 1));
    GX_GET(call, nib, std::max<size_t>(T, 1));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    GX_TRY(call, launch_edit_verify(text, sa, N, b.bytes, b.off, s.poff, s.ph, s.coff, npieces, k, T, ecnt, rep, nib, b.cnt + 2,
                                    b.cnt + 3, st));
    GX_TRY(call, hipEventRecord(ctx->ev2, st));
    GX_TRY(call, hipMemcpyAsync(b.pin + 2, b.cnt + 2, 16, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev1, ctx->ev2, &ctx->edit_verify_ms);
    ctx->edit_ends = b.pin[2];
    ctx->edit_cells = b.pin[3];
    if (b.pin[2] > budget) return refuse_device(call, s, npat, k1, hits, edit_ends_error(b.pin[2], budget));
    // dedupe: scan, emit, sort, heads, scan, fill, scan, scatter; then the starts
    const uint32_t E = (uint32_t)b.pin[2];   // <= 2^31
    const size_t tiles = suf_tiles(E), table_n = 256 * tiles;
    const uint64_t dev_cap =
        ends ? std::min<uint64_t>(std::min<uint64_t>(cap, E), (uint64_t)npat * std::min(max_hits, N)) : 0;
    uint64_t* key[2] = {nullptr, nullptr};
    uint32_t* val[2] = {nullptr, nullptr};
    uint32_t *table = nullptr, *stmp = nullptr, *head = nullptr, *hbase = nullptr, *oq = nullptr, *d_pos = nullptr,
             *d_sta = nullptr;
    uint8_t* d_dst = nullptr;
    unsigned long long* best = nullptr;
    EditHit* d_hits = nullptr;
    for (int q = 0; q < 2; ++q) {
        GX_GET(call, key[q], std::max<size_t>(E, 1));
        GX_GET(call, val[q], std::max<size_t>(E, 1));
    }
    GX_GET(call, table, std::max<size_t>(table_n, 1));
    GX_GET(call, stmp, std::max<size_t>(std::max(suf_tiles(table_n), suf_tiles((size_t)E + 1)), 1));
    GX_GET(call, head, (size_t)E + 1);
    GX_GET(call, best, npat);
    GX_GET(call, d_hits, npat);
    GX_GET(call, hbase, npat);
    GX_GET(call, oq, (size_t)npat + 1);
    if (dev_cap) {
        GX_GET(call, d_pos, (size_t)dev_cap);
        GX_GET(call, d_dst, (size_t)dev_cap);
        if (starts) GX_GET(call, d_sta, (size_t)dev_cap);
    }
    int cur = 0;
    GX_TRY(call, hipMemsetAsync(best, 0xFF, (size_t)npat * 8, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    if (E) {
        GX_TRY(call, launch_suf_scan(ecnt, T + 1, false, etmp, st));
        GX_TRY(call, launch_edit_emit(sa, N, b.off, s.poff, s.ph, s.coff, npieces, k, T, ecnt, rep, nib, key[0], val[0], st));
        // the keys are pattern << 32 | end: ends <= n, patterns < npat
        GX_TRY(call, radix_sort_pairs(key, val, E, table, stmp, radix_digits(n, npat - 1), st, &cur));
    }
    uint32_t* dmin = val[cur ^ 1];   // (the sort's other buffer is free now)
    GX_TRY(call, launch_edit_heads(key[cur], val[cur], E, k, head, dmin, best, st));
    GX_TRY(call, launch_suf_scan(head, E + 1, false, stmp, st));
    GX_TRY(call, launch_edit_fill(key[cur], head, E, s.coff, best, npat, k1, max_hits, d_hits, hbase, oq, st));
    if (dev_cap) {
        GX_TRY(call, launch_suf_scan(oq, npat + 1, false, s.tmp, st));
        GX_TRY(call, launch_edit_scatter(key[cur], dmin, head, E, hbase, oq, npat, max_hits, d_pos, d_dst, dev_cap, st));
        if (starts) GX_TRY(call, launch_edit_starts(text, b.bytes, b.off, oq, npat, k, d_pos, d_dst, d_sta, dev_cap, st));
    }
    GX_TRY(call, hipEventRecord(ctx->ev2, st));
    // (behind the last event: the events time kernels alone)
    GX_TRY(call, hipMemcpyAsync(hits, d_hits, (size_t)npat * sizeof(EditHit), hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev1, ctx->ev2, &ctx->edit_dedupe_ms);
    return finish_hits(call, hits, npat, max_hits, false, cap, hit_offsets,
                       {{ends, d_pos, 4}, {distances, d_dst, 1}, {starts, d_sta, 4}});
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI

extern "C" int gx_suffix_index_build(gx_context* ctx, const uint8_t* s, size_t n, gx_suffix_index** out) {
    if (!out) return fail(GX_EINVAL, "out is NULL");
    *out = nullptr;
    if (n && !s) return fail(GX_EINVAL, "s is NULL");
    if (n >= (1ull << 30)) return fail(GX_ERANGE, "suffix index: sequence of 2^30 bytes or more");
    for (size_t k = 0; k < n; ++k)
        if (s[k] <= 0x24)
            return fail(GX_EINVAL, "s: byte " + std::to_string((int)s[k]) + " at " + std::to_string(k) +
                                       " is not above '$' (the terminator)");
    const size_t N = n + 1;
    std::unique_ptr<gx_suffix_index> idx(new gx_suffix_index());
    idx->ctx = ctx;
    idx->n = n;
    idx->text.assign(N + kSufPad, 0);
    if (n) memcpy(idx->text.data(), s, n);
    idx->text[n] = '$';
    const bool host_sa = !ctx || n == 0 || n < suffix_host_below();
    if (host_sa) {
        std::vector<uint32_t> rank;
        suffix_host_sa(idx->text.data(), N, idx->sa, rank);
        if (!ctx) {
            *out = idx.release();
            return GX_OK;
        }
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (host_sa) {
        // (tiny texts reach the kernels too: every search on a context runs on the device)
        int rc = pool_get(ctx, N + kSufPad, &idx->d_text, st);
        if (rc == GX_OK) rc = pool_get(ctx, N * 4, &idx->d_sa, st);
        hipError_t e = hipSuccess;
        if (rc == GX_OK) e = hipMemcpyAsync(idx->d_text.p, idx->text.data(), N + kSufPad, hipMemcpyHostToDevice, st);
        if (rc == GX_OK && e == hipSuccess)
            e = hipMemcpyAsync(idx->d_sa.p, idx->sa.data(), N * 4, hipMemcpyHostToDevice, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
        if (rc == GX_OK && e != hipSuccess) rc = fail(GX_EHIP, std::string("suffix index upload: ") + hipGetErrorString(e));
        if (rc != GX_OK) {
            pool_put(ctx, idx->d_text);
            pool_put(ctx, idx->d_sa);
            return rc;
        }
    } else {
        SufDev w;
        SufInfo info;
        const int rc = suffix_device_sa(ctx, idx->text.data(), (uint32_t)N, false, false, w, info);
        if (rc != GX_OK) return rc;
        // (the stream is idle) the index keeps the text and the array, the rest goes back
        idx->d_text = w.text;
        idx->d_sa = w.v[w.cur];
        w.text = DevBuf{};
        w.v[w.cur] = DevBuf{};
        w.release(ctx);
    }
    idx->text = std::vector<uint8_t>();
    idx->sa = std::vector<uint32_t>();
    *out = idx.release();
    return GX_OK;
}

extern "C" void gx_suffix_index_free(gx_suffix_index* idx) {
    if (!idx) return;
    if (idx->ctx) {
        std::lock_guard<std::mutex> lk(idx->ctx->mu);
        pool_put(idx->ctx, idx->d_text);
        pool_put(idx->ctx, idx->d_sa);
    }
    delete idx;
}

extern "C" int gx_suffix_index_info(const gx_suffix_index* idx, uint64_t* n, int* on_device, uint64_t* device_bytes) {
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (n) *n = idx->n;
    if (on_device) *on_device = idx->ctx ? 1 : 0;
    if (device_bytes) *device_bytes = idx->ctx ? (idx->n + 1 + kSufPad) + 4 * (idx->n + 1) : 0;
    return GX_OK;
}

extern "C" int gx_suffix_index_export(const gx_suffix_index* idx, uint32_t* sa) {
    if (!idx || !sa) return fail(GX_EINVAL, "NULL argument");
    const size_t N = idx->n + 1;
    if (!idx->ctx) {
        memcpy(sa, idx->sa.data(), N * 4);
        return GX_OK;
    }
    std::lock_guard<std::mutex> lk(idx->ctx->mu);
    HIPCHK(hipSetDevice(idx->ctx->device));
    HIPCHK(hipMemcpyAsync(sa, idx->d_sa.p, N * 4, hipMemcpyDeviceToHost, idx->ctx->stream));
    HIPCHK(hipStreamSynchronize(idx->ctx->stream));
    return GX_OK;
}

namespace {

// What the three searches' entry points differ in before a pattern byte is staged.
struct SearchKind {
    const char* what;    // its name in the messages; NULL: the exact search, which has no k
    const char* out;     // its first output array
    const char* every;   // what would match were a piece empty
    uint32_t max_m;      // a pattern's most bytes where that is below the batch checker's (0: it is not)
};
constexpr SearchKind kExact{nullptr, "positions", nullptr, 0};
constexpr SearchKind kApprox{"approximate search", "positions", "window", 0};
constexpr SearchKind kEdit{"edit search", "ends", "end", kEditMaxM};

// The checks of an entry point in their order, then the item batch of the caller's batch on `strands` as the
// drivers take it.  *run: there is a pattern to search for (without one hit_offsets[0] = 0 is the whole answer).
int search_prologue(const SearchKind& kind, const gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                    size_t npat, uint32_t strands, uint32_t k, const void* hits, const void* out, const void* distances, const void* starts,
                    uint64_t* hit_offsets, HostBatch& b, bool* run) {
    *run = false;
    if (const int src = check_strands(strands)) return src;
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (npat && !hits) return fail(GX_EINVAL, "hits is NULL");
    if (out && !hit_offsets) return fail(GX_EINVAL, std::string("hit_offsets is NULL with ") + kind.out);
    if (kind.what) {
        if (out && !distances) return fail(GX_EINVAL, std::string("distances is NULL with ") + kind.out);
        if (starts && !out) return fail(GX_EINVAL, "starts without ends");
        if (k > kAprxMaxK) return fail(GX_EINVAL, "k is " + std::to_string(k) + ", more than GX_APPROX_MAX_K = 8");
    }
    const int brc = check_batch(kPatterns, patterns, offsets, npat, strands);
    if (brc != GX_OK) return brc;
    if (kind.what) {
        for (size_t p = 0; p < npat; ++p) {
            const uint64_t m = offsets[p + 1] - offsets[p];
            if (m < (uint64_t)k + 1)
                return fail(GX_EINVAL, "pattern " + std::to_string(p) + " has " + std::to_string(m) +
                                           " bytes, fewer than k + 1 = " + std::to_string(k + 1) +
                                           ": a piece would be empty and every " + kind.every + " would match");
            if (kind.max_m && m > kind.max_m)
                return fail(GX_ERANGE, "pattern " + std::to_string(p) + " has " + std::to_string(m) +
                                           " bytes, more than GX_EDIT_MAX_M = " + std::to_string(kind.max_m));
        }
        // (the pieces are the interval kernel's patterns: their count plus one, and the scan's tile rounding, in 32 bits)
        const uint64_t npieces = (uint64_t)npat * (k + 1);
        if (npieces + 1 + kSufTile >= (1ull << 32))
            return fail(GX_ERANGE, std::string(kind.what) + ": " + std::to_string(npieces) +
                                       " pieces (npat * (k + 1)), 2^32 or more with the scan's rounding: split the batch");
    }
    if (npat == 0) {
        if (hit_offsets) hit_offsets[0] = 0;
        return GX_OK;
    }
    // (the caller's batch has passed: now its item batch)
    strand_batch(idx, patterns, offsets, npat, strands, b);
    if (kind.what) {
        const uint64_t npieces = (uint64_t)(b.offs.size() - 1) * (k + 1);   // (as above, of the items)
        if (npieces + 1 + kSufTile >= (1ull << 32))
            return fail(GX_ERANGE, std::string(kind.what) + ": " + std::to_string(npieces) +
                                       " pieces (npat * (k + 1)), 2^32 or more with the scan's rounding: split the batch");
    }
    *run = true;
    return GX_OK;
}

}  // namespace

extern "C" int gx_suffix_index_search_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                              size_t npat, uint32_t strands, gx_search_hit* hits, uint32_t max_hits,
                                              uint32_t* positions, size_t positions_cap, uint64_t* hit_offsets) {
    HostBatch b;
    bool run;
    const int rc = search_prologue(kExact, idx, patterns, offsets, npat, strands, 0, hits, positions, nullptr, nullptr, hit_offsets, b, &run);
    if (!run) return rc;
    const size_t items = b.offs.size() - 1;
    if (idx->ctx)
        return search_device(idx, patterns, (size_t)offsets[npat], b.offs.data(), (uint32_t)items, strands, hits, max_hits,
                             positions, positions_cap, hit_offsets);
    return search_host(idx, b.padded.data(), b.offs.data(), items, hits, max_hits, positions, positions_cap, hit_offsets);
}

extern "C" int gx_suffix_index_search(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets, size_t npat,
                                      gx_search_hit* hits, uint32_t max_hits, uint32_t* positions, size_t positions_cap,
                                      uint64_t* hit_offsets) {
    return gx_suffix_index_search_strands(idx, patterns, offsets, npat, GX_STRAND_FWD, hits, max_hits, positions, positions_cap,
                                          hit_offsets);
}

extern "C" int gx_search_info(const gx_context* ctx, uint64_t* word_compares, double* search_ms, double* locate_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (word_compares) *word_compares = ctx->srch_words;
    if (search_ms) *search_ms = ctx->srch_ms;
    if (locate_ms) *locate_ms = ctx->srch_locate_ms;
    return GX_OK;
}

extern "C" int gx_suffix_index_search_approx_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                                     size_t npat, uint32_t strands, uint32_t k, gx_approx_hit* hits,
                                                     uint32_t max_hits, uint32_t* positions, uint8_t* distances,
                                                     size_t positions_cap, uint64_t* hit_offsets) {
    HostBatch b;
    bool run;
    const int rc = search_prologue(kApprox, idx, patterns, offsets, npat, strands, k, hits, positions, distances, nullptr, hit_offsets, b, &run);
    if (!run) return rc;
    const size_t items = b.offs.size() - 1;
    if (idx->ctx)
        return approx_device(idx, patterns, (size_t)offsets[npat], b.offs.data(), (uint32_t)items, strands, k, hits, max_hits,
                             positions, distances, positions_cap, hit_offsets);
    return approx_host(idx, b.padded.data(), b.offs.data(), items, k, hits, max_hits, positions, distances, positions_cap,
                       hit_offsets);
}

extern "C" int gx_suffix_index_search_approx(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                             size_t npat, uint32_t k, gx_approx_hit* hits, uint32_t max_hits,
                                             uint32_t* positions, uint8_t* distances, size_t positions_cap,
                                             uint64_t* hit_offsets) {
    return gx_suffix_index_search_approx_strands(idx, patterns, offsets, npat, GX_STRAND_FWD, k, hits, max_hits, positions,
                                                 distances, positions_cap, hit_offsets);
}

extern "C" int gx_approx_info(const gx_context* ctx, uint64_t* candidates, uint64_t* word_compares, double* seed_ms,
                              double* verify_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (candidates) *candidates = ctx->aprx_cands;
    if (word_compares) *word_compares = ctx->aprx_words;
    if (seed_ms) *seed_ms = ctx->aprx_seed_ms;
    if (verify_ms) *verify_ms = ctx->aprx_verify_ms;
    return GX_OK;
}

extern "C" int gx_suffix_index_search_edit_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                                   size_t npat, uint32_t strands, uint32_t k, gx_edit_hit* hits,
                                                   uint32_t max_hits, uint32_t* ends, uint8_t* distances, uint32_t* starts,
                                                   size_t positions_cap, uint64_t* hit_offsets) {
    HostBatch b;
    bool run;
    const int rc = search_prologue(kEdit, idx, patterns, offsets, npat, strands, k, hits, ends, distances, starts, hit_offsets, b, &run);
    if (!run) return rc;
    const size_t items = b.offs.size() - 1;
    if (idx->ctx)
        return edit_device(idx, patterns, (size_t)offsets[npat], b.offs.data(), (uint32_t)items, strands, k, hits, max_hits, ends,
                           distances, starts, positions_cap, hit_offsets);
    return edit_host(idx, b.padded.data(), b.offs.data(), items, k, hits, max_hits, ends, distances, starts, positions_cap,
                     hit_offsets);
}

extern "C" int gx_suffix_index_search_edit(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                           size_t npat, uint32_t k, gx_edit_hit* hits, uint32_t max_hits, uint32_t* ends,
                                           uint8_t* distances, uint32_t* starts, size_t positions_cap,
                                           uint64_t* hit_offsets) {
    return gx_suffix_index_search_edit_strands(idx, patterns, offsets, npat, GX_STRAND_FWD, k, hits, max_hits, ends, distances,
                                               starts, positions_cap, hit_offsets);
}

extern "C" int gx_edit_info(const gx_context* ctx, uint64_t* candidates, uint64_t* pre_dedupe_ends, uint64_t* cell_updates,
                            double* seed_ms, double* verify_ms, double* dedupe_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (candidates) *candidates = ctx->edit_cands;
    if (pre_dedupe_ends) *pre_dedupe_ends = ctx->edit_ends;
    if (cell_updates) *cell_updates = ctx->edit_cells;
    if (seed_ms) *seed_ms = ctx->edit_seed_ms;
    if (verify_ms) *verify_ms = ctx->edit_verify_ms;
    if (dedupe_ms) *dedupe_ms = ctx->edit_dedupe_ms;
    return GX_OK;
}

// ---------------------------------------------------------------------------
// both strands: the reverse complement as a call of its own

namespace {
constexpr BatchKind kItems{"pattern", "bytes", 0, true};
}

extern "C" int gx_revcomp(const uint8_t* src, size_t n, uint8_t* dst) {
    if (n && (!src || !dst)) return fail(GX_EINVAL, "NULL argument");
    if (n) strand_rc(src, n, dst);
    return GX_OK;
}

extern "C" int gx_revcomp_batch(gx_context* ctx, const uint8_t* bytes, const uint64_t* offsets, size_t n, uint32_t strands,
                                uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets) {
    if (const int src = check_strands(strands)) return src;
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (!out_offsets) return fail(GX_EINVAL, "out_offsets is NULL");
    const int brc = check_batch(kItems, bytes, offsets, n, strands);
    if (brc != GX_OK) return brc;
    gx_suffix_index where;   // (only its ctx is read: which side builds the bytes)
    where.ctx = ctx;
    HostBatch b;
    strand_batch(&where, bytes, offsets, n, strands, b);
    const size_t items = b.offs.size() - 1, total = b.offs[items];
    for (size_t p = 0; p <= items; ++p) out_offsets[p] = b.offs[p];
    if (!out_bytes) return GX_OK;
    if (total > out_cap)
        return fail(GX_ECAP, "revcomp: " + std::to_string(total) + " item bytes needed, out_cap is " + std::to_string(out_cap));
    // (with room for them the kSufPad zero bytes behind the items are handed out too, as staged)
    const size_t want = out_cap - total >= (size_t)kSufPad ? total + kSufPad : total;
    if (!ctx) {
        if (want) memcpy(out_bytes, b.padded.data(), want);
        return GX_OK;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    StagedBatch sb;
    if (const int rc = stage_batch_strands(call, "revcomp", bytes, (size_t)offsets[n], b.offs.data(), (uint32_t)n, strands, sb))
        return rc;
    // the offsets as the device holds them
    GX_TRY(call, hipMemcpyAsync(b.offs.data(), sb.off, (items + 1) * 4, hipMemcpyDeviceToHost, call.st));
    if (want) GX_TRY(call, hipMemcpyAsync(out_bytes, sb.bytes, want, hipMemcpyDeviceToHost, call.st));
    GX_TRY(call, hipStreamSynchronize(call.st));
    for (size_t p = 0; p <= items; ++p) out_offsets[p] = b.offs[p];
    return call.done(GX_OK);   // (the stream is idle)
}

extern "C" int gx_strand_info(const gx_context* ctx, uint64_t* items, uint64_t* rc_bytes, double* rc_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (items) *items = ctx->strand_items;
    if (rc_bytes) *rc_bytes = ctx->strand_rc_bytes;
    if (rc_ms) {
        // (every call leaves its stream idle: the two events have completed)
        float ms = 0.f;
        *rc_ms = ctx->strand_timed && hipEventElapsedTime(&ms, ctx->ev_rc0, ctx->ev_rc1) == hipSuccess ? ms : 0.0;
    }
    return GX_OK;
}
