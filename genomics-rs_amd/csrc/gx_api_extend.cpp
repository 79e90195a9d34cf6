// gx_api_extend.cpp -- search mode: banded affine-gap alignment and CIGARs of
// reported hits.  The recurrence and the retrace are the
// reference's alignment_table and retrace (algo.rs:151-441) on the band of
// gx_extend.h; batching them over the hits of an index has no counterpart in
// the reference's main.rs.
//
//   checks   the entry point's in their order, the batch checker of the
//            searches, then every hit against the text, its pattern and the
//            band; the same pass leaves each hit's pattern and each wave's
//            rows, which is all the chunking needs
//   host     ext_fill and ext_walk (gx_extend.h) per hit in plain loops: the
//            checker on a CPU-only machine and the device's field-by-field
//            comparison partner
//   device   patterns staged as the searches stage them, the hits' three
//            words, the tile offsets; per chunk of at most
//            GX_EXTEND_TRACE_BYTES of trace: fill, walk, the scan of the run
//            counts, emit (gx_extend.hip); then the records, the offsets and
//            exactly the total of runs
#include "gx_api_call.h"
#include "gx_extend.h"
#include "gx_strand.h"

namespace {

static_assert(sizeof(gx_extend_hit) == sizeof(ExtHit), "gx_extend_hit layout");
static_assert(GX_EXTEND_MAX_BAND == kExtMaxBand, "GX_EXTEND_MAX_BAND");
static_assert(GX_EXTEND_MAX_SCORE == kExtMaxScore, "GX_EXTEND_MAX_SCORE");

constexpr BatchKind kPatterns{"pattern", "patterns", kEditMaxM, false};

// GX_EXTEND_TRACE_BYTES, read on every call: the trace of one launch.  At most
// 2^30: a hit has at most w + m <= 15 (w + 1) runs and at least w + 1 words of
// 4 bytes, so a launch's runs stay below 2^32 (the scan of the counts is 32-bit).
uint64_t trace_budget() {
    uint64_t b = 1ull << 29;
    if (const char* e = getenv("GX_EXTEND_TRACE_BYTES")) {
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && v > 0) b = v;
    }
    return std::min<uint64_t>(b, 1ull << 30);
}

int cap_error(uint64_t total, size_t cap) {
    return fail(GX_ECAP, "extend: " + std::to_string(total) + " runs needed, cigar_cap is " + std::to_string(cap));
}

int runs_error(uint64_t total) {
    return fail(GX_ERANGE, "extend: " + std::to_string(total) + " runs, 2^32 or more: split the batch");
}

// Every hit against the text, its pattern and the band.  pid (may be NULL):
// each hit's pattern; rows (may be NULL): per wave of 64 hits its largest w + 1.
// *steps: what the runs can come to at most, a step a run and w + m steps a hit
// (one for an empty pair).
int check_hits(uint64_t n, const uint64_t* offsets, size_t npat, const uint64_t* hit_offsets, const uint32_t* starts,
               const uint32_t* ends, uint32_t band, std::vector<uint32_t>* pid, std::vector<uint32_t>* rows,
               uint64_t* steps) {
    const uint64_t nhits = hit_offsets[npat];
    uint64_t sum = 0;
    if (pid) pid->resize(nhits);
    if (rows) rows->assign((nhits + 63) / 64, 0);
    for (size_t p = 0; p < npat; ++p) {
        const uint64_t m = offsets[p + 1] - offsets[p];
        for (uint64_t h = hit_offsets[p]; h < hit_offsets[p + 1]; ++h) {
            const uint64_t b = starts[h], e = ends[h];
            if (e < b || e > n)
                return fail(GX_EINVAL, "hit " + std::to_string(h) + " of pattern " + std::to_string(p) + ": [" +
                                           std::to_string(b) + ", " + std::to_string(e) + ") is not a window of the " +
                                           std::to_string(n) + " text bytes");
            const uint64_t w = e - b, d = w > m ? w - m : m - w;
            if (d > band)
                return fail(GX_EINVAL, "hit " + std::to_string(h) + " of pattern " + std::to_string(p) + ": a window of " +
                                           std::to_string(w) + " bytes against " + std::to_string(m) +
                                           " pattern bytes leaves the band of " + std::to_string(band));
            if (pid) (*pid)[h] = (uint32_t)p;
            if (rows) (*rows)[h >> 6] = std::max((*rows)[h >> 6], (uint32_t)w + 1);
            sum += std::max<uint64_t>(w + m, 1);
        }
    }
    *steps = sum;
    return GX_OK;
}

// One hit on the host at the width the kernels use for B.  runs: room for
// w + m + 1 words, filled from its end backwards (NULL: the record only).
template <int K>
void one_host(const uint8_t* t, uint32_t w, const uint8_t* P, uint32_t m, uint32_t B, const ExtScores& sc,
              std::vector<uint64_t>& scratch, ExtHit* rec, uint32_t* runs_end, uint64_t* cells) {
    typedef typename ExtWord<K>::type Word;
    scratch.resize((size_t)w + 1);
    Word* trace = (Word*)scratch.data();
    rec->score = ext_fill<K>(t, w, P, m, B, sc, trace, 1, cells);
    if (runs_end) ext_walk<Word, true>(t, w, P, m, B, trace, 1, rec, runs_end);
    else ext_walk<Word, false>(t, w, P, m, B, trace, 1, rec, nullptr);
}

int extend_host(const gx_suffix_index* idx, const uint8_t* pats, const uint64_t* offsets, size_t npat,
                const uint64_t* hit_offsets, const uint32_t* starts, const uint32_t* ends, const ExtScores& sc, uint32_t band,
                gx_extend_hit* out, uint32_t* cigar, size_t cap, uint64_t* cigar_offsets) {
    const uint8_t* text = idx->text.data();
    std::vector<uint64_t> scratch;
    std::vector<uint32_t> one, all;   // a hit's runs, and every hit's in turn
    uint64_t cells = 0, total = 0;
    for (size_t p = 0; p < npat; ++p) {
        const uint32_t m = (uint32_t)(offsets[p + 1] - offsets[p]);
        const uint8_t* P = pats + offsets[p];
        for (uint64_t h = hit_offsets[p]; h < hit_offsets[p + 1]; ++h) {
            const uint32_t w = ends[h] - starts[h];
            ExtHit r{};
            uint32_t* re = nullptr;
            if (cigar) {
                one.resize((size_t)w + m + 1);
                re = one.data() + one.size();
            }
            switch (ext_width_of(band)) {
                case 2: one_host<2>(text + starts[h], w, P, m, band, sc, scratch, &r, re, &cells); break;
                case 4: one_host<4>(text + starts[h], w, P, m, band, sc, scratch, &r, re, &cells); break;
                case 8: one_host<8>(text + starts[h], w, P, m, band, sc, scratch, &r, re, &cells); break;
                default: one_host<15>(text + starts[h], w, P, m, band, sc, scratch, &r, re, &cells); break;
            }
            out[h] = gx_extend_hit{r.score, r.n_steps, r.matches, r.mismatches, r.opening_gaps, r.gap_extensions,
                                   r.identities, r.cigar_len};
            cigar_offsets[h] = total;
            total += r.cigar_len;
            if (cigar && total <= cap) all.insert(all.end(), re - r.cigar_len, re);
        }
    }
    cigar_offsets[hit_offsets[npat]] = total;
    if (total >= (1ull << 32)) return runs_error(total);
    if (!cigar) return GX_OK;
    if (total > cap) return cap_error(total, cap);
    if (total) memcpy(cigar, all.data(), (size_t)total * 4);
    return GX_OK;
}

// pats: the caller's pattern bytes, unpadded; offs, npat: the item batch of those on `strands`, offsets in 32 bits;
// pid, rows: as check_hits left them.  Takes ctx->mu.
int extend_device(gx_suffix_index* idx, const uint8_t* pats, size_t total_bytes, const uint32_t* offs, uint32_t npat,
                  uint32_t strands, const std::vector<uint32_t>& pid, const std::vector<uint32_t>& rows, const uint32_t* starts,
                  const uint32_t* ends, uint32_t nhits, uint64_t steps_bound, const ExtScores& sc, uint32_t band,
                  gx_extend_hit* out, uint32_t* cigar, size_t cap, uint64_t* cigar_offsets) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    hipStream_t st = call.st;
    ctx->ext_hits = nhits;
    ctx->ext_cells = ctx->ext_trace_bytes = ctx->ext_chunks = 0;
    ctx->ext_fill_ms = ctx->ext_walk_ms = 0.0;
    // tile offsets in words, and the chunks: whole waves, as many as the budget holds, one at the least
    const size_t nwaves = rows.size(), wb = ext_word_bytes(band);
    const uint64_t budget = trace_budget() / wb;
    std::vector<uint64_t> toff(nwaves + 1, 0);
    for (size_t v = 0; v < nwaves; ++v) toff[v + 1] = toff[v] + 64ull * rows[v];
    std::vector<size_t> cut{0};   // chunk c: waves [cut[c], cut[c + 1])
    uint64_t max_words = 0;
    size_t max_waves = 0;
    for (size_t v = 0; v < nwaves;) {
        size_t e = v + 1;
        while (e < nwaves && toff[e + 1] - toff[v] <= budget) ++e;
        max_words = std::max(max_words, toff[e] - toff[v]);
        max_waves = std::max(max_waves, e - v);
        cut.push_back(e);
        v = e;
    }
    // counters: [0] cell updates, [1] runs
    StagedBatch b;
    if (const int rc = stage_batch_strands(call, "extend", pats, total_bytes, offs, (uint32_t)strand_sources(npat, strands), strands, b)) return rc;
    const uint64_t dev_cap = cigar ? std::min<uint64_t>(cap, steps_bound) : 0;
    const size_t max_hits = std::min<size_t>(max_waves * 64, nhits);
    uint32_t *d_pid = nullptr, *d_sta = nullptr, *d_end = nullptr, *cnt = nullptr, *tmp = nullptr, *d_cig = nullptr;
    uint64_t *d_toff = nullptr, *d_goffs = nullptr, *trace = nullptr;
    ExtHit* d_out = nullptr;
    GX_GET(call, d_pid, nhits);
    GX_GET(call, d_sta, nhits);
    GX_GET(call, d_end, nhits);
    GX_GET(call, d_toff, nwaves + 1);
    GX_GET(call, d_out, nhits);
    GX_GET(call, d_goffs, (size_t)nhits + 1);
    GX_GET(call, cnt, max_hits + 1);
    GX_GET(call, tmp, suf_tiles(max_hits + 1));
    GX_GET(call, trace, (size_t)((max_words * wb + 7) / 8));
    if (dev_cap) GX_GET(call, d_cig, (size_t)dev_cap);
    GX_TRY(call, hipMemcpyAsync(d_pid, pid.data(), (size_t)nhits * 4, hipMemcpyHostToDevice, st));
    GX_TRY(call, hipMemcpyAsync(d_sta, starts, (size_t)nhits * 4, hipMemcpyHostToDevice, st));
    GX_TRY(call, hipMemcpyAsync(d_end, ends, (size_t)nhits * 4, hipMemcpyHostToDevice, st));
    GX_TRY(call, hipMemcpyAsync(d_toff, toff.data(), (nwaves + 1) * 8, hipMemcpyHostToDevice, st));
    ExtLaunch L;
    L.text = (const uint8_t*)idx->d_text.p;
    L.pats = b.bytes;
    L.offs = b.off;
    L.pid = d_pid;
    L.starts = d_sta;
    L.ends = d_end;
    L.toff = d_toff;
    L.B = band;
    L.sc = sc;
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        L.h0 = (uint32_t)(cut[c] * 64);
        L.h1 = (uint32_t)std::min<uint64_t>(cut[c + 1] * 64, nhits);
        L.words = toff[cut[c + 1]] - toff[cut[c]];
        GX_TRY(call, hipEventRecord(ctx->ev0, st));
        GX_TRY(call, launch_ext_fill(L, trace, d_out, b.cnt, st));
        GX_TRY(call, hipEventRecord(ctx->ev1, st));
        GX_TRY(call, launch_ext_walk(L, trace, d_out, cnt, b.cnt + 1, st));
        GX_TRY(call, launch_suf_scan(cnt, L.h1 - L.h0 + 1, false, tmp, st));
        GX_TRY(call, launch_ext_emit(L, trace, cnt, b.cnt + 1, d_goffs, d_cig, dev_cap, st));
        GX_TRY(call, hipEventRecord(ctx->ev2, st));
        // (the three events are the context's: a chunk's times are read before the next records them)
        GX_TRY(call, hipStreamSynchronize(st));
        double f = 0.0, k = 0.0;
        call.elapsed(ctx->ev0, ctx->ev1, &f);
        call.elapsed(ctx->ev1, ctx->ev2, &k);
        ctx->ext_fill_ms += f;
        ctx->ext_walk_ms += k;
    }
    ctx->ext_chunks = cut.size() - 1;
    ctx->ext_trace_bytes = max_words * wb;
    GX_TRY(call, hipMemcpyAsync(b.pin, b.cnt, 16, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(out, d_out, (size_t)nhits * sizeof(ExtHit), hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(cigar_offsets, d_goffs, ((size_t)nhits + 1) * 8, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    ctx->ext_cells = b.pin[0];
    const uint64_t total = b.pin[1];
    if (total >= (1ull << 32)) return call.done(runs_error(total));
    if (!cigar) return call.done(GX_OK);
    if (total > cap) return call.done(cap_error(total, cap));
    if (total) {
        GX_TRY(call, hipMemcpyAsync(cigar, d_cig, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        GX_TRY(call, hipStreamSynchronize(st));
    }
    return call.done(GX_OK);   // (the stream is idle)
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI

extern "C" int gx_suffix_index_extend_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                              size_t npat, uint32_t strands, const uint64_t* hit_offsets,
                                              const uint32_t* starts, const uint32_t* ends, const gx_scores* scores,
                                              uint32_t band, gx_extend_hit* out, uint32_t* cigar, size_t cigar_cap,
                                              uint64_t* cigar_offsets) {
    if (const int src = check_strands(strands)) return src;
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (!hit_offsets) return fail(GX_EINVAL, "hit_offsets is NULL");
    if (!scores) return fail(GX_EINVAL, "scores is NULL");
    if (!cigar_offsets) return fail(GX_EINVAL, "cigar_offsets is NULL");
    if (band > kExtMaxBand)
        return fail(GX_EINVAL, "band is " + std::to_string(band) + ", more than GX_EXTEND_MAX_BAND = 15");
    const int64_t sv[4] = {scores->s_match, scores->s_mismatch, scores->g, scores->h};
    const char* const sn[4] = {"s_match", "s_mismatch", "g", "h"};
    for (int q = 0; q < 4; ++q)
        if (sv[q] > kExtMaxScore || sv[q] < -kExtMaxScore)
            return fail(GX_ERANGE, std::string("extend: ") + sn[q] + " is " + std::to_string(sv[q]) +
                                       ", above GX_EXTEND_MAX_SCORE = 32767 in magnitude");
    const int brc = check_batch(kPatterns, patterns, offsets, npat, strands);
    if (brc != GX_OK) return brc;
    // from here on the patterns are the items of the caller's batch on `strands`: hit_offsets has
    // one entry per item and one more, and a hit of a reverse item is aligned against that reverse complement
    const bool dev = idx->ctx != nullptr;
    const uint8_t* caller_patterns = patterns;
    const size_t caller_bytes = (size_t)offsets[npat];
    HostBatch hb;
    std::vector<uint64_t> item_offsets;
    if (dev || strands != GX_STRAND_FWD) strand_batch(idx, patterns, offsets, npat, strands, hb);
    if (strands != GX_STRAND_FWD) {
        item_offsets.assign(hb.offs.begin(), hb.offs.end());
        offsets = item_offsets.data();
        npat = item_offsets.size() - 1;
        if (!dev) patterns = hb.padded.data();
    }
    if (hit_offsets[0] != 0) return fail(GX_EINVAL, "hit_offsets[0] is not 0");
    for (size_t p = 0; p < npat; ++p)
        if (hit_offsets[p + 1] < hit_offsets[p])
            return fail(GX_EINVAL, "hit_offsets decrease at pattern " + std::to_string(p));
    const uint64_t nhits = hit_offsets[npat];
    // (the device's scan of the run counts is 32-bit: the hits plus one and its tile rounding)
    if (nhits + 1 + kSufTile >= (1ull << 32))
        return fail(GX_ERANGE, "extend: " + std::to_string(nhits) + " hits, 2^32 or more with the scan's rounding: split the batch");
    if (nhits && !starts) return fail(GX_EINVAL, "starts is NULL");
    if (nhits && !ends) return fail(GX_EINVAL, "ends is NULL");
    if (nhits && !out) return fail(GX_EINVAL, "out is NULL");
    std::vector<uint32_t> pid, rows;
    uint64_t steps_bound = 0;
    const int hrc = check_hits(idx->n, offsets, npat, hit_offsets, starts, ends, band, dev ? &pid : nullptr,
                               dev ? &rows : nullptr, &steps_bound);
    if (hrc != GX_OK) return hrc;
    if (nhits == 0) {
        cigar_offsets[0] = 0;
        if (dev) {
            std::lock_guard<std::mutex> lk(idx->ctx->mu);
            idx->ctx->ext_hits = idx->ctx->ext_cells = idx->ctx->ext_trace_bytes = idx->ctx->ext_chunks = 0;
            idx->ctx->ext_fill_ms = idx->ctx->ext_walk_ms = 0.0;
        }
        return GX_OK;
    }
    const ExtScores sc{(int32_t)sv[0], (int32_t)sv[1], (int32_t)sv[2], (int32_t)sv[3]};
    if (!dev)
        return extend_host(idx, patterns, offsets, npat, hit_offsets, starts, ends, sc, band, out, cigar, cigar_cap, cigar_offsets);
    return extend_device(idx, caller_patterns, caller_bytes, hb.offs.data(), (uint32_t)npat, strands, pid, rows, starts, ends,
                         (uint32_t)nhits, steps_bound, sc, band, out, cigar, cigar_cap, cigar_offsets);
}

extern "C" int gx_suffix_index_extend(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets, size_t npat,
                                      const uint64_t* hit_offsets, const uint32_t* starts, const uint32_t* ends,
                                      const gx_scores* scores, uint32_t band, gx_extend_hit* out, uint32_t* cigar,
                                      size_t cigar_cap, uint64_t* cigar_offsets) {
    return gx_suffix_index_extend_strands(idx, patterns, offsets, npat, GX_STRAND_FWD, hit_offsets, starts, ends, scores, band, out,
                                          cigar, cigar_cap, cigar_offsets);
}

extern "C" int gx_extend_info(const gx_context* ctx, uint64_t* hits, uint64_t* cell_updates, uint64_t* trace_bytes,
                              uint64_t* chunks, double* fill_ms, double* walk_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (hits) *hits = ctx->ext_hits;
    if (cell_updates) *cell_updates = ctx->ext_cells;
    if (trace_bytes) *trace_bytes = ctx->ext_trace_bytes;
    if (chunks) *chunks = ctx->ext_chunks;
    if (fill_ms) *fill_ms = ctx->ext_fill_ms;
    if (walk_ms) *walk_ms = ctx->ext_walk_ms;
    return GX_OK;
}
