// gx_api_search.cpp -- search mode: a suffix index that outlives the call and
// batched exact-match queries on it.  No counterpart in the
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
#include "gx_api.h"
#include "gx_search.h"

struct gx_suffix_index {
    gx_context* ctx = nullptr;   // nullptr: a host index
    uint64_t n = 0;
    std::vector<uint8_t> text;   // host index: t and kSufPad zero bytes
    std::vector<uint32_t> sa;    // host index
    DevBuf d_text, d_sa;         // device index: held out of the pool until the index is freed
};

namespace {

static_assert(sizeof(gx_search_hit) == sizeof(SrchHit), "gx_search_hit layout");

// hit_offsets from hits; returns the total.
uint64_t offsets_of(const gx_search_hit* hits, size_t npat, uint32_t max_hits, uint64_t* hit_offsets) {
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
