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
#include "gx_api.h"
#include "gx_approx.h"
#include "gx_edit.h"
#include "gx_search.h"

namespace {

static_assert(sizeof(gx_search_hit) == sizeof(SrchHit), "gx_search_hit layout");

// hit_offsets from hits (gx_search_hit or gx_approx_hit); returns the total.
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
// the device).  Takes ctx->mu.
int search_device(gx_suffix_index* idx, const uint8_t* pats, size_t total_bytes, const uint32_t* offs, uint32_t npat,
                  gx_search_hit* hits, uint32_t max_hits, uint32_t* positions, size_t cap, uint64_t* hit_offsets) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t N = (uint32_t)idx->n + 1;
    ctx->srch_words = 0;
    ctx->srch_ms = ctx->srch_locate_ms = 0.0;
    DevBuf d_pat, d_off, d_hits, d_q, d_tmp, d_small, d_pos;
    auto done = [&](int rc) {
        if (rc != GX_OK) (void)hipStreamSynchronize(st);   // nothing of this call still runs on the buffers
        for (DevBuf* b : {&d_pat, &d_off, &d_hits, &d_q, &d_tmp, &d_small, &d_pos}) pool_put(ctx, *b);
        return rc;
    };
#define SR_TRY(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return done(fail(e_ == hipErrorOutOfMemory ? GX_ENOMEM : GX_EHIP,                                 \
                             std::string(#expr) + ": " + hipGetErrorString(e_)));                             \
    } while (0)
#define SR_GET(buf, bytes)                                                      \
    do {                                                                        \
        const int rc_ = pool_get(ctx, (bytes), &(buf), st);                     \
        if (rc_ != GX_OK) return done(rc_);                                     \
    } while (0)
    // 1. patterns and offsets, kSufPad zero bytes behind the patterns
    SR_GET(d_pat, total_bytes + kSufPad);
    SR_GET(d_off, ((size_t)npat + 1) * 4);
    SR_GET(d_hits, (size_t)npat * sizeof(SrchHit));
    SR_GET(d_small, 64);
    unsigned long long* d_words = (unsigned long long*)d_small.p;
    // (pageable sources: the copies have left them once the stream is synchronised below)
    if (total_bytes) SR_TRY(hipMemcpyAsync(d_pat.p, pats, total_bytes, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync((uint8_t*)d_pat.p + total_bytes, 0, kSufPad, st));
    SR_TRY(hipMemcpyAsync(d_off.p, offs, ((size_t)npat + 1) * 4, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync(d_words, 0, 8, st));
    // 2. the interval kernel
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    SrchHit* d_h = (SrchHit*)d_hits.p;
    SR_TRY(hipEventRecord(ctx->ev0, st));
    SR_TRY(launch_srch_range(text, sa, N, (const uint8_t*)d_pat.p, (const uint32_t*)d_off.p, npat, d_h, d_words, st));
    SR_TRY(hipEventRecord(ctx->ev1, st));
    unsigned long long* pin = (unsigned long long*)io_pinned(ctx, 128);
    if (!pin) return done(fail(GX_ENOMEM, "search: pinned staging"));
    // what the positions can come to at most; the device's offsets are 32-bit,
    // so a batch that could reach 2^32 is summed on the host before the scan
    const uint64_t bound = (uint64_t)npat * std::min(max_hits, N);
    uint64_t dev_cap = std::min<uint64_t>(cap, bound);
    bool copied = false, located = false;
    float ms = 0.f;
    if (positions && bound >= (1ull << 32)) {
        SR_TRY(hipMemcpyAsync(pin, d_words, 8, hipMemcpyDeviceToHost, st));
        SR_TRY(hipMemcpyAsync(hits, d_h, (size_t)npat * sizeof(SrchHit), hipMemcpyDeviceToHost, st));
        SR_TRY(hipStreamSynchronize(st));
        copied = true;
        if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->srch_ms = ms;
        const uint64_t total = offsets_of(hits, npat, max_hits, nullptr);
        if (total >= (1ull << 32)) {
            offsets_of(hits, npat, max_hits, hit_offsets);
            ctx->srch_words = pin[0];
            return done(total_error(total));
        }
        dev_cap = total <= cap ? total : 0;   // (the total is known here; above cap it is GX_ECAP below)
        if (dev_cap) SR_TRY(hipEventRecord(ctx->ev1, st));   // the locate step starts here
    }
    if (positions && dev_cap) {
        // 3. clamp, exclusive scan, gather: nothing else between ev1 and ev2
        SR_GET(d_q, ((size_t)npat + 1) * 4);
        SR_GET(d_tmp, suf_tiles((size_t)npat + 1) * 4);
        SR_GET(d_pos, (size_t)dev_cap * 4);
        uint32_t* q = (uint32_t*)d_q.p;
        SR_TRY(launch_srch_clamp(d_h, npat, max_hits, q, st));
        SR_TRY(launch_suf_scan(q, npat + 1, false, (uint32_t*)d_tmp.p, st));
        SR_TRY(launch_srch_gather(sa, N, d_h, q, npat, (uint32_t*)d_pos.p, dev_cap, st));
        SR_TRY(hipEventRecord(ctx->ev2, st));
        located = true;
    }
    if (!copied) {
        // (behind the last event, as suffix_device's copies: the events time kernels alone)
        SR_TRY(hipMemcpyAsync(pin, d_words, 8, hipMemcpyDeviceToHost, st));
        SR_TRY(hipMemcpyAsync(hits, d_h, (size_t)npat * sizeof(SrchHit), hipMemcpyDeviceToHost, st));
    }
    SR_TRY(hipStreamSynchronize(st));
    if (!copied && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->srch_ms = ms;
    if (located && hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2) == hipSuccess) ctx->srch_locate_ms = ms;
    ctx->srch_words = pin[0];
    if (!positions) {
        if (hit_offsets) offsets_of(hits, npat, max_hits, hit_offsets);
        return done(GX_OK);
    }
    // 4. the positions: only now is their number known to the host, so that
    // GX_ECAP leaves positions[] untouched and the copy moves no more than them
    const uint64_t total = offsets_of(hits, npat, max_hits, hit_offsets);
    if (total >= (1ull << 32)) return done(total_error(total));
    if (total > cap) return done(cap_error(total, cap));
    if (total) {
        SR_TRY(hipMemcpyAsync(positions, d_pos.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        SR_TRY(hipStreamSynchronize(st));
    }
    done(GX_OK);   // (the stream is idle)
#undef SR_TRY
#undef SR_GET
    sort_segments(positions, hit_offsets, npat);
    return GX_OK;
}

// What both searches refuse of a batch before a pattern byte is staged.
int check_batch(const uint8_t* patterns, const uint64_t* offsets, size_t npat) {
    if (offsets[0] != 0) return fail(GX_EINVAL, "offsets[0] is not 0");
    for (size_t p = 0; p < npat; ++p) {
        if (offsets[p + 1] < offsets[p])
            return fail(GX_EINVAL, "offsets decrease at pattern " + std::to_string(p));
        if (offsets[p + 1] - offsets[p] > kSrchMaxPattern)
            return fail(GX_ERANGE, "pattern " + std::to_string(p) + " has " + std::to_string(offsets[p + 1] - offsets[p]) +
                                       " bytes, more than 65535");
    }
    const uint64_t total_bytes = offsets[npat];
    // (one more than the 32-bit device offsets need, for the scan's npat + 1 entries and its tile rounding)
    if (total_bytes + npat >= (1ull << 32) || (uint64_t)npat + 1 + kSufTile >= (1ull << 32))
        return fail(GX_ERANGE, "search: pattern bytes plus patterns come to " + std::to_string(total_bytes + npat) +
                                   ", 2^32 or more: split the batch or lower max_hits");
    if (total_bytes && !patterns) return fail(GX_EINVAL, "patterns is NULL");
    // (one flat pass the compiler vectorises; the culprit is looked for only when there is one)
    unsigned low = 0;
    for (uint64_t k = 0; k < total_bytes; ++k) low |= patterns[k] <= 0x24;
    for (size_t p = 0; low && p < npat; ++p)
        for (uint64_t k = offsets[p]; k < offsets[p + 1]; ++k)
            if (patterns[k] <= 0x24)
                return fail(GX_EINVAL, "pattern " + std::to_string(p) + ": byte " + std::to_string((int)patterns[k]) +
                                           " at offset " + std::to_string(k - offsets[p]) + " is not above '$'");
    return GX_OK;
}

// ---------------------------------------------------------------------------
// k mismatches: pigeonhole seeds through the exact search, then
// the verify walk of gx_approx.h on every seed hit, host and device alike

static_assert(sizeof(gx_approx_hit) == sizeof(AprxHit), "gx_approx_hit layout");
static_assert(GX_APPROX_MAX_K == kAprxMaxK, "GX_APPROX_MAX_K");

}  // namespace

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

namespace {

int budget_error(uint64_t total, uint64_t budget) {
    return fail(GX_ERANGE, "approximate search: " + std::to_string(total) + " seed hits, more than GX_APPROX_CAND_BUDGET = " +
                               std::to_string(budget) + ": split the batch, lower k, or raise GX_APPROX_CAND_BUDGET");
}

// The budget refusal's only output: candidates per pattern from the pieces' intervals.
void candidates_only(const SrchHit* ph, size_t npat, uint32_t k1, gx_approx_hit* hits) {
    for (size_t p = 0; p < npat; ++p) {
        uint64_t c = 0;
        for (uint32_t j = 0; j < k1; ++j) c += ph[p * k1 + j].count;
        hits[p].candidates = (uint32_t)std::min<uint64_t>(c, 0xFFFFFFFFull);
    }
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
    const uint32_t n = (uint32_t)idx->n, N = n + 1, k1 = k + 1;
    const uint8_t* t = idx->text.data();
    const uint32_t* sa = idx->sa.data();
    // seeds: every piece through the exact search, in candidate order
    std::vector<SrchHit> ph(npat * k1);
    uint64_t words = 0, total = 0;
    for (size_t p = 0; p < npat; ++p) {
        const uint32_t m = offs[p + 1] - offs[p];
        for (uint32_t j = 0; j < k1; ++j) {
            const uint32_t ps = aprx_piece_start(m, k1, j), pe = aprx_piece_start(m, k1, j + 1);
            ph[p * k1 + j] = srch_one(t, sa, N, pats + offs[p] + ps, pe - ps, &words);
            total += ph[p * k1 + j].count;
        }
    }
    const uint64_t budget = approx_budget();
    if (total > budget) {
        candidates_only(ph.data(), npat, k1, hits);
        return budget_error(total, budget);
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
                  uint32_t k, gx_approx_hit* hits, uint32_t max_hits, uint32_t* positions, uint8_t* distances, size_t cap,
                  uint64_t* hit_offsets) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t N = (uint32_t)idx->n + 1, k1 = k + 1, npieces = npat * k1;
    ctx->aprx_cands = ctx->aprx_words = 0;
    ctx->aprx_seed_ms = ctx->aprx_verify_ms = 0.0;
    DevBuf d_pat, d_off, d_poff, d_phits, d_coff, d_tmp, d_small, d_keep, d_ktmp, d_dist, d_start, d_best, d_hits, d_oq,
        d_pos, d_dst;
    auto done = [&](int rc) {
        if (rc != GX_OK) (void)hipStreamSynchronize(st);   // nothing of this call still runs on the buffers
        for (DevBuf* b : {&d_pat, &d_off, &d_poff, &d_phits, &d_coff, &d_tmp, &d_small, &d_keep, &d_ktmp, &d_dist,
                          &d_start, &d_best, &d_hits, &d_oq, &d_pos, &d_dst})
            pool_put(ctx, *b);
        return rc;
    };
#define SR_TRY(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return done(fail(e_ == hipErrorOutOfMemory ? GX_ENOMEM : GX_EHIP,                                 \
                             std::string(#expr) + ": " + hipGetErrorString(e_)));                             \
    } while (0)
#define SR_GET(buf, bytes)                                                      \
    do {                                                                        \
        const int rc_ = pool_get(ctx, (bytes), &(buf), st);                     \
        if (rc_ != GX_OK) return done(rc_);                                     \
    } while (0)
    // patterns and offsets as the exact search stages them; the piece offsets are the device's own
    SR_GET(d_pat, total_bytes + kSufPad);
    SR_GET(d_off, ((size_t)npat + 1) * 4);
    SR_GET(d_poff, ((size_t)npieces + 1) * 4);
    SR_GET(d_phits, (size_t)npieces * sizeof(SrchHit));
    SR_GET(d_coff, ((size_t)npieces + 1) * 4);
    SR_GET(d_tmp, suf_tiles((size_t)npieces + 1) * 4);
    SR_GET(d_small, 64);
    unsigned long long* d_cnt = (unsigned long long*)d_small.p;   // [0] seed word steps, [1] seed hits, [2] verify word steps
    SR_TRY(hipMemcpyAsync(d_pat.p, pats, total_bytes, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync((uint8_t*)d_pat.p + total_bytes, 0, kSufPad, st));
    SR_TRY(hipMemcpyAsync(d_off.p, offs, ((size_t)npat + 1) * 4, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync(d_cnt, 0, 24, st));
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    const uint8_t* dp = (const uint8_t*)d_pat.p;
    const uint32_t* off = (const uint32_t*)d_off.p;
    uint32_t* poff = (uint32_t*)d_poff.p;
    SrchHit* ph = (SrchHit*)d_phits.p;
    uint32_t* coff = (uint32_t*)d_coff.p;
    // stages 1 to 4: pieces, seeds, their 64-bit total, candidate offsets.  The scan is 32-bit and is
    // relied upon only once the host has held the total against the budget.
    SR_TRY(hipEventRecord(ctx->ev0, st));
    SR_TRY(launch_aprx_pieces(off, npat, k1, poff, st));
    SR_TRY(launch_srch_range(text, sa, N, dp, poff, npieces, ph, d_cnt, st));
    SR_TRY(launch_aprx_total(ph, npieces, d_cnt + 1, st));
    SR_TRY(launch_srch_clamp(ph, npieces, 0xFFFFFFFFu, coff, st));
    SR_TRY(launch_suf_scan(coff, npieces + 1, false, (uint32_t*)d_tmp.p, st));
    SR_TRY(hipEventRecord(ctx->ev1, st));
    unsigned long long* pin = (unsigned long long*)io_pinned(ctx, 128);
    if (!pin) return done(fail(GX_ENOMEM, "approximate search: pinned staging"));
    SR_TRY(hipMemcpyAsync(pin, d_cnt, 16, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->aprx_seed_ms = ms;
    const uint64_t total = pin[1], budget = approx_budget();
    ctx->aprx_cands = total;
    if (total > budget) {
        std::vector<SrchHit> hp(npieces);
        SR_TRY(hipMemcpyAsync(hp.data(), ph, (size_t)npieces * sizeof(SrchHit), hipMemcpyDeviceToHost, st));
        SR_TRY(hipStreamSynchronize(st));
        candidates_only(hp.data(), npat, k1, hits);
        return done(budget_error(total, budget));
    }
    // stages 5 and 6: verify, compact
    const uint32_t T = (uint32_t)total;   // <= 2^31
    const uint64_t dev_cap =
        positions ? std::min<uint64_t>(std::min<uint64_t>(cap, total), (uint64_t)npat * std::min(max_hits, N)) : 0;
    SR_GET(d_keep, ((size_t)T + 1) * 4);
    SR_GET(d_ktmp, suf_tiles((size_t)T + 1) * 4);
    SR_GET(d_dist, std::max<size_t>(T, 1));
    SR_GET(d_start, std::max<size_t>(T, 1) * 4);
    SR_GET(d_best, (size_t)npat * 8);
    SR_GET(d_hits, (size_t)npat * sizeof(AprxHit));
    SR_GET(d_oq, ((size_t)npat + 1) * 4);
    if (dev_cap) {
        SR_GET(d_pos, (size_t)dev_cap * 4);
        SR_GET(d_dst, (size_t)dev_cap);
    }
    uint32_t* keep = (uint32_t*)d_keep.p;
    uint32_t* oq = (uint32_t*)d_oq.p;
    SR_TRY(hipMemsetAsync(d_best.p, 0xFF, (size_t)npat * 8, st));
    SR_TRY(hipEventRecord(ctx->ev1, st));
    SR_TRY(launch_aprx_verify(text, sa, N, dp, off, poff, ph, coff, npieces, k, T, keep, (uint8_t*)d_dist.p,
                              (uint32_t*)d_start.p, (unsigned long long*)d_best.p, d_cnt + 2, st));
    SR_TRY(launch_suf_scan(keep, T + 1, false, (uint32_t*)d_ktmp.p, st));
    SR_TRY(launch_aprx_fill(coff, keep, (const unsigned long long*)d_best.p, npat, k1, max_hits, (AprxHit*)d_hits.p, oq,
                            st));
    if (dev_cap) {
        SR_TRY(launch_suf_scan(oq, npat + 1, false, (uint32_t*)d_tmp.p, st));
        SR_TRY(launch_aprx_scatter(coff, keep, oq, npat, k1, T, max_hits, (const uint32_t*)d_start.p,
                                   (const uint8_t*)d_dist.p, (uint32_t*)d_pos.p, (uint8_t*)d_dst.p, dev_cap, st));
    }
    SR_TRY(hipEventRecord(ctx->ev2, st));
    // (behind the last event: the events time kernels alone)
    SR_TRY(hipMemcpyAsync(pin + 2, d_cnt + 2, 8, hipMemcpyDeviceToHost, st));
    SR_TRY(hipMemcpyAsync(hits, d_hits.p, (size_t)npat * sizeof(AprxHit), hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    if (hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2) == hipSuccess) ctx->aprx_verify_ms = ms;
    ctx->aprx_words = pin[2];
    if (!positions) {
        if (hit_offsets) offsets_of(hits, npat, max_hits, hit_offsets);
        return done(GX_OK);
    }
    // the positions: their number is known to the host only now, so that GX_ECAP leaves positions[] and
    // distances[] untouched and the copies move no more than them (a total above dev_cap is above cap)
    const uint64_t total_out = offsets_of(hits, npat, max_hits, hit_offsets);
    if (total_out > cap) return done(cap_error(total_out, cap));
    if (total_out) {
        SR_TRY(hipMemcpyAsync(positions, d_pos.p, (size_t)total_out * 4, hipMemcpyDeviceToHost, st));
        SR_TRY(hipMemcpyAsync(distances, d_dst.p, (size_t)total_out, hipMemcpyDeviceToHost, st));
        SR_TRY(hipStreamSynchronize(st));
    }
    done(GX_OK);   // (the stream is idle)
#undef SR_TRY
#undef SR_GET
    sort_pairs(positions, distances, hit_offsets, npat);
    return GX_OK;
}

// ---------------------------------------------------------------------------
// k differences: the same seeds, then the band of gx_edit.h on
// every seed hit, the reported (pattern, end, distance) triples sorted and the
// minimum taken over every run of equal ends, host and device alike

static_assert(sizeof(gx_edit_hit) == sizeof(EditHit), "gx_edit_hit layout");
static_assert(GX_EDIT_MAX_M == kEditMaxM, "GX_EDIT_MAX_M");

int edit_seed_error(uint64_t total, uint64_t budget) {
    return fail(GX_ERANGE, "edit search: " + std::to_string(total) + " seed hits, more than GX_APPROX_CAND_BUDGET = " +
                               std::to_string(budget) + ": split the batch, lower k, or raise GX_APPROX_CAND_BUDGET");
}

int edit_ends_error(uint64_t total, uint64_t budget) {
    return fail(GX_ERANGE, "edit search: " + std::to_string(total) +
                               " reported ends before dedupe, more than GX_APPROX_CAND_BUDGET = " + std::to_string(budget) +
                               ": split the batch, lower k, or raise GX_APPROX_CAND_BUDGET");
}

void edit_candidates_only(const SrchHit* ph, size_t npat, uint32_t k1, gx_edit_hit* hits) {
    for (size_t p = 0; p < npat; ++p) {
        uint64_t c = 0;
        for (uint32_t j = 0; j < k1; ++j) c += ph[p * k1 + j].count;
        hits[p].candidates = (uint32_t)std::min<uint64_t>(c, 0xFFFFFFFFull);
    }
}

// The radix passes that sort pattern << 32 | end: a key byte that is zero in
// every key (ends <= n, patterns < npat) is skipped, as the suffix sort's masks
// skip constant digits.
bool edit_pass_needed(int p, uint32_t n, uint32_t npat) {
    return p < 4 ? (n >> (8 * p)) != 0 : ((npat - 1) >> (8 * (p - 4))) != 0;
}

// pats: padded as for search_host.
int edit_host(const gx_suffix_index* idx, const uint8_t* pats, const uint32_t* offs, size_t npat, uint32_t k,
              gx_edit_hit* hits, uint32_t max_hits, uint32_t* ends, uint8_t* distances, uint32_t* starts, size_t cap,
              uint64_t* hit_offsets) {
    const uint32_t n = (uint32_t)idx->n, N = n + 1, k1 = k + 1;
    const uint8_t* t = idx->text.data();
    const uint32_t* sa = idx->sa.data();
    std::vector<SrchHit> ph(npat * k1);
    uint64_t words = 0, total = 0, cells = 0;
    for (size_t p = 0; p < npat; ++p) {
        const uint32_t m = offs[p + 1] - offs[p];
        for (uint32_t j = 0; j < k1; ++j) {
            const uint32_t ps = aprx_piece_start(m, k1, j), pe = aprx_piece_start(m, k1, j + 1);
            ph[p * k1 + j] = srch_one(t, sa, N, pats + offs[p] + ps, pe - ps, &words);
            total += ph[p * k1 + j].count;
        }
    }
    const uint64_t budget = approx_budget();
    if (total > budget) {
        edit_candidates_only(ph.data(), npat, k1, hits);
        return edit_seed_error(total, budget);
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
                    edit_candidates_only(ph.data(), npat, k1, hits);
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
                uint32_t k, gx_edit_hit* hits, uint32_t max_hits, uint32_t* ends, uint8_t* distances, uint32_t* starts,
                size_t cap, uint64_t* hit_offsets) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)idx->n, N = n + 1, k1 = k + 1, npieces = npat * k1;
    ctx->edit_cands = ctx->edit_ends = ctx->edit_cells = 0;
    ctx->edit_seed_ms = ctx->edit_verify_ms = ctx->edit_dedupe_ms = 0.0;
    DevBuf d_pat, d_off, d_poff, d_phits, d_coff, d_tmp, d_small, d_ecnt, d_etmp, d_rep, d_nib, d_key[2], d_val[2], d_table,
        d_stmp, d_head, d_best, d_hits, d_hbase, d_oq, d_pos, d_dst, d_sta;
    auto done = [&](int rc) {
        if (rc != GX_OK) (void)hipStreamSynchronize(st);   // nothing of this call still runs on the buffers
        for (DevBuf* b : {&d_pat, &d_off, &d_poff, &d_phits, &d_coff, &d_tmp, &d_small, &d_ecnt, &d_etmp, &d_rep, &d_nib,
                          &d_key[0], &d_key[1], &d_val[0], &d_val[1], &d_table, &d_stmp, &d_head, &d_best, &d_hits,
                          &d_hbase, &d_oq, &d_pos, &d_dst, &d_sta})
            pool_put(ctx, *b);
        return rc;
    };
#define SR_TRY(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return done(fail(e_ == hipErrorOutOfMemory ? GX_ENOMEM : GX_EHIP,                                 \
                             std::string(#expr) + ": " + hipGetErrorString(e_)));                             \
    } while (0)
#define SR_GET(buf, bytes)                                                      \
    do {                                                                        \
        const int rc_ = pool_get(ctx, (bytes), &(buf), st);                     \
        if (rc_ != GX_OK) return done(rc_);                                     \
    } while (0)
    SR_GET(d_pat, total_bytes + kSufPad);
    SR_GET(d_off, ((size_t)npat + 1) * 4);
    SR_GET(d_poff, ((size_t)npieces + 1) * 4);
    SR_GET(d_phits, (size_t)npieces * sizeof(SrchHit));
    SR_GET(d_coff, ((size_t)npieces + 1) * 4);
    SR_GET(d_tmp, suf_tiles((size_t)npieces + 1) * 4);
    SR_GET(d_small, 64);
    unsigned long long* d_cnt = (unsigned long long*)d_small.p;   // [0] seed word steps, [1] seed hits, [2] ends before dedupe, [3] cell updates
    SR_TRY(hipMemcpyAsync(d_pat.p, pats, total_bytes, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync((uint8_t*)d_pat.p + total_bytes, 0, kSufPad, st));
    SR_TRY(hipMemcpyAsync(d_off.p, offs, ((size_t)npat + 1) * 4, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync(d_cnt, 0, 32, st));
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    const uint8_t* dp = (const uint8_t*)d_pat.p;
    const uint32_t* off = (const uint32_t*)d_off.p;
    uint32_t* poff = (uint32_t*)d_poff.p;
    SrchHit* ph = (SrchHit*)d_phits.p;
    uint32_t* coff = (uint32_t*)d_coff.p;
    // pieces, seeds, their 64-bit total, candidate offsets: DESIGN.md 19.2 stages 1 to 4
    SR_TRY(hipEventRecord(ctx->ev0, st));
    SR_TRY(launch_aprx_pieces(off, npat, k1, poff, st));
    SR_TRY(launch_srch_range(text, sa, N, dp, poff, npieces, ph, d_cnt, st));
    SR_TRY(launch_aprx_total(ph, npieces, d_cnt + 1, st));
    SR_TRY(launch_srch_clamp(ph, npieces, 0xFFFFFFFFu, coff, st));
    SR_TRY(launch_suf_scan(coff, npieces + 1, false, (uint32_t*)d_tmp.p, st));
    SR_TRY(hipEventRecord(ctx->ev1, st));
    unsigned long long* pin = (unsigned long long*)io_pinned(ctx, 128);
    if (!pin) return done(fail(GX_ENOMEM, "edit search: pinned staging"));
    SR_TRY(hipMemcpyAsync(pin, d_cnt, 16, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->edit_seed_ms = ms;
    const uint64_t total = pin[1], budget = approx_budget();
    ctx->edit_cands = total;
    std::vector<SrchHit> hp;   // the refusals' only output comes from the pieces' intervals
    auto refuse = [&](int rc) {
        hp.resize(npieces);
        if (hipMemcpyAsync(hp.data(), ph, (size_t)npieces * sizeof(SrchHit), hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipStreamSynchronize(st) == hipSuccess)
            edit_candidates_only(hp.data(), npat, k1, hits);
        return done(rc);
    };
    if (total > budget) return refuse(edit_seed_error(total, budget));
    // the band on every candidate; what it reports is summed in 64 bits and held against the budget
    // before the 32-bit scan of the numbers is relied upon
    const uint32_t T = (uint32_t)total;   // <= 2^31
    SR_GET(d_ecnt, ((size_t)T + 1) * 4);
    SR_GET(d_etmp, suf_tiles((size_t)T + 1) * 4);
    SR_GET(d_rep, std::max<size_t>(T, 1) * 4);
    SR_GET(d_nib, std::max<size_t>(T, 1) * 8);
    uint32_t* ecnt = (uint32_t*)d_ecnt.p;
    SR_TRY(hipEventRecord(ctx->ev1, st));
    SR_TRY(launch_edit_verify(text, sa, N, dp, off, poff, ph, coff, npieces, k, T, ecnt, (uint32_t*)d_rep.p,
                              (uint64_t*)d_nib.p, d_cnt + 2, d_cnt + 3, st));
    SR_TRY(hipEventRecord(ctx->ev2, st));
    SR_TRY(hipMemcpyAsync(pin + 2, d_cnt + 2, 16, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    if (hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2) == hipSuccess) ctx->edit_verify_ms = ms;
    ctx->edit_ends = pin[2];
    ctx->edit_cells = pin[3];
    if (pin[2] > budget) return refuse(edit_ends_error(pin[2], budget));
    // dedupe: scan, emit, sort, heads, scan, fill, scan, scatter; then the starts
    const uint32_t E = (uint32_t)pin[2];   // <= 2^31
    const size_t tiles = suf_tiles(E), table_n = 256 * tiles;
    const uint64_t dev_cap =
        ends ? std::min<uint64_t>(std::min<uint64_t>(cap, E), (uint64_t)npat * std::min(max_hits, N)) : 0;
    for (int q = 0; q < 2; ++q) {
        SR_GET(d_key[q], std::max<size_t>(E, 1) * 8);
        SR_GET(d_val[q], std::max<size_t>(E, 1) * 4);
    }
    SR_GET(d_table, std::max<size_t>(table_n, 1) * 4);
    SR_GET(d_stmp, std::max<size_t>(std::max(suf_tiles(table_n), suf_tiles((size_t)E + 1)), 1) * 4);
    SR_GET(d_head, ((size_t)E + 1) * 4);
    SR_GET(d_best, (size_t)npat * 8);
    SR_GET(d_hits, (size_t)npat * sizeof(EditHit));
    SR_GET(d_hbase, (size_t)npat * 4);
    SR_GET(d_oq, ((size_t)npat + 1) * 4);
    if (dev_cap) {
        SR_GET(d_pos, (size_t)dev_cap * 4);
        SR_GET(d_dst, (size_t)dev_cap);
        if (starts) SR_GET(d_sta, (size_t)dev_cap * 4);
    }
    int cur = 0;
    auto K = [&](int q) { return (uint64_t*)d_key[q].p; };
    auto V = [&](int q) { return (uint32_t*)d_val[q].p; };
    uint32_t* head = (uint32_t*)d_head.p;
    uint32_t* oq = (uint32_t*)d_oq.p;
    SR_TRY(hipMemsetAsync(d_best.p, 0xFF, (size_t)npat * 8, st));
    SR_TRY(hipEventRecord(ctx->ev1, st));
    if (E) {
        SR_TRY(launch_suf_scan(ecnt, T + 1, false, (uint32_t*)d_etmp.p, st));
        SR_TRY(launch_edit_emit(sa, N, off, poff, ph, coff, npieces, k, T, ecnt, (const uint32_t*)d_rep.p,
                                (const uint64_t*)d_nib.p, K(cur), V(cur), st));
        for (int p = 0; p < 8; ++p) {
            if (!edit_pass_needed(p, n, npat)) continue;
            SR_TRY(launch_suf_sort_pass(K(cur), V(cur), K(cur ^ 1), V(cur ^ 1), E, 8 * p, (uint32_t*)d_table.p,
                                        (uint32_t*)d_stmp.p, st));
            cur ^= 1;
        }
    }
    uint32_t* dmin = V(cur ^ 1);   // (the sort's other buffer is free now)
    SR_TRY(launch_edit_heads(K(cur), V(cur), E, k, head, dmin, (unsigned long long*)d_best.p, st));
    SR_TRY(launch_suf_scan(head, E + 1, false, (uint32_t*)d_stmp.p, st));
    SR_TRY(launch_edit_fill(K(cur), head, E, coff, (const unsigned long long*)d_best.p, npat, k1, max_hits,
                            (EditHit*)d_hits.p, (uint32_t*)d_hbase.p, oq, st));
    if (dev_cap) {
        SR_TRY(launch_suf_scan(oq, npat + 1, false, (uint32_t*)d_tmp.p, st));
        SR_TRY(launch_edit_scatter(K(cur), dmin, head, E, (const uint32_t*)d_hbase.p, oq, npat, max_hits,
                                   (uint32_t*)d_pos.p, (uint8_t*)d_dst.p, dev_cap, st));
        if (starts)
            SR_TRY(launch_edit_starts(text, dp, off, oq, npat, k, (const uint32_t*)d_pos.p, (const uint8_t*)d_dst.p,
                                      (uint32_t*)d_sta.p, dev_cap, st));
    }
    SR_TRY(hipEventRecord(ctx->ev2, st));
    // (behind the last event: the events time kernels alone)
    SR_TRY(hipMemcpyAsync(hits, d_hits.p, (size_t)npat * sizeof(EditHit), hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    if (hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2) == hipSuccess) ctx->edit_dedupe_ms = ms;
    if (!ends) {
        if (hit_offsets) offsets_of(hits, npat, max_hits, hit_offsets);
        return done(GX_OK);
    }
    // the occurrences: their number is known to the host only now, so that GX_ECAP leaves the three arrays
    // untouched and the copies move no more than them (a total above dev_cap is above cap)
    const uint64_t total_out = offsets_of(hits, npat, max_hits, hit_offsets);
    if (total_out > cap) return done(cap_error(total_out, cap));
    if (total_out) {
        SR_TRY(hipMemcpyAsync(ends, d_pos.p, (size_t)total_out * 4, hipMemcpyDeviceToHost, st));
        SR_TRY(hipMemcpyAsync(distances, d_dst.p, (size_t)total_out, hipMemcpyDeviceToHost, st));
        if (starts) SR_TRY(hipMemcpyAsync(starts, d_sta.p, (size_t)total_out * 4, hipMemcpyDeviceToHost, st));
        SR_TRY(hipStreamSynchronize(st));
    }
#undef SR_TRY
#undef SR_GET
    return done(GX_OK);   // (the stream is idle)
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

extern "C" int gx_suffix_index_search(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets, size_t npat,
                                      gx_search_hit* hits, uint32_t max_hits, uint32_t* positions, size_t positions_cap,
                                      uint64_t* hit_offsets) {
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (npat && !hits) return fail(GX_EINVAL, "hits is NULL");
    if (positions && !hit_offsets) return fail(GX_EINVAL, "hit_offsets is NULL with positions");
    const int brc = check_batch(patterns, offsets, npat);
    if (brc != GX_OK) return brc;
    const uint64_t total_bytes = offsets[npat];
    if (npat == 0) {
        if (hit_offsets) hit_offsets[0] = 0;
        return GX_OK;
    }
    std::vector<uint32_t> offs(npat + 1);
    for (size_t p = 0; p <= npat; ++p) offs[p] = (uint32_t)offsets[p];
    if (idx->ctx)
        return search_device(idx, patterns, (size_t)total_bytes, offs.data(), (uint32_t)npat, hits, max_hits, positions,
                             positions_cap, hit_offsets);
    // the host compares read 8 bytes at a time too: the same padding behind the patterns
    std::vector<uint8_t> padded(total_bytes + kSufPad, 0);
    if (total_bytes) memcpy(padded.data(), patterns, total_bytes);
    return search_host(idx, padded.data(), offs.data(), npat, hits, max_hits, positions, positions_cap, hit_offsets);
}

extern "C" int gx_search_info(const gx_context* ctx, uint64_t* word_compares, double* search_ms, double* locate_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (word_compares) *word_compares = ctx->srch_words;
    if (search_ms) *search_ms = ctx->srch_ms;
    if (locate_ms) *locate_ms = ctx->srch_locate_ms;
    return GX_OK;
}

extern "C" int gx_suffix_index_search_approx(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                             size_t npat, uint32_t k, gx_approx_hit* hits, uint32_t max_hits,
                                             uint32_t* positions, uint8_t* distances, size_t positions_cap,
                                             uint64_t* hit_offsets) {
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (npat && !hits) return fail(GX_EINVAL, "hits is NULL");
    if (positions && !hit_offsets) return fail(GX_EINVAL, "hit_offsets is NULL with positions");
    if (positions && !distances) return fail(GX_EINVAL, "distances is NULL with positions");
    if (k > kAprxMaxK) return fail(GX_EINVAL, "k is " + std::to_string(k) + ", more than GX_APPROX_MAX_K = 8");
    const int brc = check_batch(patterns, offsets, npat);
    if (brc != GX_OK) return brc;
    for (size_t p = 0; p < npat; ++p)
        if (offsets[p + 1] - offsets[p] < (uint64_t)k + 1)
            return fail(GX_EINVAL, "pattern " + std::to_string(p) + " has " + std::to_string(offsets[p + 1] - offsets[p]) +
                                       " bytes, fewer than k + 1 = " + std::to_string(k + 1) +
                                       ": a piece would be empty and every window would match");
    // (the pieces are the interval kernel's patterns: their count plus one, and the scan's tile rounding, in 32 bits)
    const uint64_t npieces = (uint64_t)npat * (k + 1);
    if (npieces + 1 + kSufTile >= (1ull << 32))
        return fail(GX_ERANGE, "approximate search: " + std::to_string(npieces) +
                                   " pieces (npat * (k + 1)), 2^32 or more with the scan's rounding: split the batch");
    const uint64_t total_bytes = offsets[npat];
    if (npat == 0) {
        if (hit_offsets) hit_offsets[0] = 0;
        return GX_OK;
    }
    std::vector<uint32_t> offs(npat + 1);
    for (size_t p = 0; p <= npat; ++p) offs[p] = (uint32_t)offsets[p];
    if (idx->ctx)
        return approx_device(idx, patterns, (size_t)total_bytes, offs.data(), (uint32_t)npat, k, hits, max_hits, positions,
                             distances, positions_cap, hit_offsets);
    std::vector<uint8_t> padded(total_bytes + kSufPad, 0);
    memcpy(padded.data(), patterns, total_bytes);
    return approx_host(idx, padded.data(), offs.data(), npat, k, hits, max_hits, positions, distances, positions_cap,
                       hit_offsets);
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

extern "C" int gx_suffix_index_search_edit(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                           size_t npat, uint32_t k, gx_edit_hit* hits, uint32_t max_hits, uint32_t* ends,
                                           uint8_t* distances, uint32_t* starts, size_t positions_cap,
                                           uint64_t* hit_offsets) {
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (npat && !hits) return fail(GX_EINVAL, "hits is NULL");
    if (ends && !hit_offsets) return fail(GX_EINVAL, "hit_offsets is NULL with ends");
    if (ends && !distances) return fail(GX_EINVAL, "distances is NULL with ends");
    if (starts && !ends) return fail(GX_EINVAL, "starts without ends");
    if (k > kAprxMaxK) return fail(GX_EINVAL, "k is " + std::to_string(k) + ", more than GX_APPROX_MAX_K = 8");
    const int brc = check_batch(patterns, offsets, npat);
    if (brc != GX_OK) return brc;
    for (size_t p = 0; p < npat; ++p) {
        const uint64_t m = offsets[p + 1] - offsets[p];
        if (m < (uint64_t)k + 1)
            return fail(GX_EINVAL, "pattern " + std::to_string(p) + " has " + std::to_string(m) +
                                       " bytes, fewer than k + 1 = " + std::to_string(k + 1) +
                                       ": a piece would be empty and every end would match");
        if (m > kEditMaxM)
            return fail(GX_ERANGE, "pattern " + std::to_string(p) + " has " + std::to_string(m) +
                                       " bytes, more than GX_EDIT_MAX_M = 4096");
    }
    const uint64_t npieces = (uint64_t)npat * (k + 1);
    if (npieces + 1 + kSufTile >= (1ull << 32))
        return fail(GX_ERANGE, "edit search: " + std::to_string(npieces) +
                                   " pieces (npat * (k + 1)), 2^32 or more with the scan's rounding: split the batch");
    const uint64_t total_bytes = offsets[npat];
    if (npat == 0) {
        if (hit_offsets) hit_offsets[0] = 0;
        return GX_OK;
    }
    std::vector<uint32_t> offs(npat + 1);
    for (size_t p = 0; p <= npat; ++p) offs[p] = (uint32_t)offsets[p];
    if (idx->ctx)
        return edit_device(idx, patterns, (size_t)total_bytes, offs.data(), (uint32_t)npat, k, hits, max_hits, ends,
                           distances, starts, positions_cap, hit_offsets);
    std::vector<uint8_t> padded(total_bytes + kSufPad, 0);
    memcpy(padded.data(), patterns, total_bytes);
    return edit_host(idx, padded.data(), offs.data(), npat, k, hits, max_hits, ends, distances, starts, positions_cap,
                     hit_offsets);
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
