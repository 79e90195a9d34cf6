// gx_api_match.cpp -- search mode for long queries: matching statistics and
// maximal exact matches on the suffix index.  No counterpart in
// the reference's main.rs.
//
//   host     the shared rules of gx_match.h on one thread: a loop over the
//            query positions, then over the candidates, then one sort.  The
//            checker on a CPU-only machine and the device's field-by-field
//            comparison partner.
//   device   the queries staged once (16 zero bytes behind them), a lane per
//            position (gx_match.hip); for MEMs the seeds' 64-bit total held
//            against GX_APPROX_CAND_BUDGET before the 32-bit scan is relied
//            upon, keep, the per-query counts, and with mems[] emit, the radix
//            sort of the suffix sort on (position << 32 | text position) and
//            the copy of exactly the total.
// The batch checker, the staging and the radix sort are the ones the three
// searches use (gx_api.h, gx_api_call.h).
#include "gx_api_call.h"
#include "gx_match.h"
#include "gx_strand.h"

namespace {

static_assert(sizeof(gx_match_stat) == sizeof(MatchStat), "gx_match_stat layout");
static_assert(sizeof(gx_mem) == sizeof(Mem), "gx_mem layout");

constexpr BatchKind kQueries{"query", "queries", 0, true};

int mem_budget_error(uint64_t total, uint64_t budget) {
    return fail(GX_ERANGE, "mems: " + std::to_string(total) + " candidate pairs, more than GX_APPROX_CAND_BUDGET = " +
                               std::to_string(budget) + ": split the batch, raise min_len, or raise GX_APPROX_CAND_BUDGET");
}

int mem_cap_error(uint64_t total, size_t cap) {
    return fail(GX_ECAP, "mems: " + std::to_string(total) + " MEMs needed, mems_cap is " + std::to_string(cap));
}

void reset_info(gx_context* ctx) {
    ctx->mat_cands = ctx->mat_kept = ctx->mat_words = 0;
    ctx->mat_stats_ms = ctx->mat_seed_ms = ctx->mat_emit_ms = 0.0;
}

// q: the queries with kSufPad zero bytes behind them.
void stats_host(const gx_suffix_index* idx, const uint8_t* q, const uint32_t* offs, uint32_t nq, uint32_t W,
                gx_match_stat* stats) {
    const uint32_t N = (uint32_t)idx->n + 1;
    uint64_t words = 0;
    for (uint32_t c = 0; c < nq; ++c)
        for (uint32_t g = offs[c]; g < offs[c + 1]; ++g) {
            const MatchStat s = match_stat_one(idx->text.data(), idx->sa.data(), N, q + g, std::min(W, offs[c + 1] - g), &words);
            stats[g] = gx_match_stat{s.len, s.lo, s.count, s.pos};
        }
}

int mems_host(const gx_suffix_index* idx, const uint8_t* q, const uint32_t* offs, uint32_t nq, uint32_t L, gx_mem* mems,
              size_t cap, uint64_t* mem_offsets, uint64_t* candidates) {
    const uint32_t N = (uint32_t)idx->n + 1, npos = offs[nq];
    const uint8_t* t = idx->text.data();
    const uint32_t* sa = idx->sa.data();
    uint64_t words = 0, total = 0;
    std::vector<uint32_t> lo(npos), cnt(npos);
    std::vector<uint64_t> cand(nq, 0);
    for (uint32_t c = 0; c < nq; ++c)
        for (uint32_t g = offs[c]; g < offs[c + 1]; ++g) {
            match_seed_one(t, sa, N, q + g, offs[c + 1] - g, L, &lo[g], &cnt[g], &words);
            cand[c] += cnt[g];
            total += cnt[g];
        }
    if (candidates) std::copy(cand.begin(), cand.end(), candidates);
    const uint64_t budget = approx_budget();
    if (total > budget) return mem_budget_error(total, budget);
    // keep: the counts first, so that counts only and a capacity that is too small build nothing
    auto kept_at = [&](uint32_t c, uint32_t g, uint32_t r, uint32_t* i) {
        *i = sa[lo[g] + r];
        return *i < N && match_left_maximal(t, *i, q + g, g - offs[c]);
    };
    uint64_t kept = 0;
    for (uint32_t c = 0; c < nq; ++c) {
        mem_offsets[c] = kept;
        for (uint32_t g = offs[c]; g < offs[c + 1]; ++g)
            for (uint32_t r = 0, i; r < cnt[g]; ++r) kept += kept_at(c, g, r, &i) ? 1 : 0;
    }
    mem_offsets[nq] = kept;
    if (!mems) return GX_OK;
    if (kept > cap) return mem_cap_error(kept, cap);
    // emit: every kept pair extended to the right; then one sort
    std::vector<std::pair<uint64_t, uint32_t>> out;   // (position << 32 | text position, length)
    out.reserve(kept);
    for (uint32_t c = 0; c < nq; ++c)
        for (uint32_t g = offs[c]; g < offs[c + 1]; ++g)
            for (uint32_t r = 0, i; r < cnt[g]; ++r)
                if (kept_at(c, g, r, &i))
                    out.emplace_back((uint64_t)g << 32 | i, match_extend(t, N, i, q + g, offs[c + 1] - g, L, &words));
    std::sort(out.begin(), out.end());
    uint32_t c = 0;
    for (uint64_t k = 0; k < kept; ++k) {
        const uint32_t g = (uint32_t)(out[k].first >> 32);
        while (g >= offs[c + 1]) ++c;
        mems[k] = gx_mem{g - offs[c], (uint32_t)out[k].first, out[k].second};
    }
    return GX_OK;
}

// q: the caller's query bytes, unpadded; offs, nq: the item batch of those on `strands` (npos item bytes).  Takes ctx->mu.
int stats_device(gx_suffix_index* idx, const uint8_t* q, const uint32_t* offs, uint32_t nq, uint32_t strands, uint32_t W,
                 gx_match_stat* stats) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    hipStream_t st = call.st;
    const uint32_t N = (uint32_t)idx->n + 1, npos = offs[nq];
    reset_info(ctx);
    if (!npos) return GX_OK;
    StagedBatch b;
    if (const int rc = stage_batch_strands(call, "match", q, (size_t)strand_sources(npos, strands), offs, (uint32_t)strand_sources(nq, strands), strands, b)) return rc;
    MatchStat* d_stats = nullptr;
    GX_GET(call, d_stats, npos);
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_match_stats((const uint8_t*)idx->d_text.p, (const uint32_t*)idx->d_sa.p, N, b.bytes, b.off, nq, npos, W,
                                    d_stats, b.cnt, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    // (behind the last event: the events time the kernel alone)
    GX_TRY(call, hipMemcpyAsync(b.pin, b.cnt, 8, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(stats, d_stats, (size_t)npos * sizeof(MatchStat), hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev0, ctx->ev1, &ctx->mat_stats_ms);
    ctx->mat_words = b.pin[0];
    return call.done(GX_OK);
}

// q: unpadded.  Takes ctx->mu.
int mems_device(gx_suffix_index* idx, const uint8_t* q, const uint32_t* offs, uint32_t nq, uint32_t strands, uint32_t L,
                gx_mem* mems, size_t cap, uint64_t* mem_offsets, uint64_t* candidates) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    hipStream_t st = call.st;
    const uint32_t n = (uint32_t)idx->n, N = n + 1, npos = offs[nq];
    reset_info(ctx);
    if (!npos) {
        for (uint32_t c = 0; c <= nq; ++c) mem_offsets[c] = 0;
        if (candidates) std::fill(candidates, candidates + nq, 0);
        return GX_OK;
    }
    // counters: [0] seed word steps, [1] candidates, [2] emit word steps
    StagedBatch b;
    if (const int rc = stage_batch_strands(call, "mems", q, (size_t)strand_sources(npos, strands), offs, (uint32_t)strand_sources(nq, strands), strands, b)) return rc;
    uint32_t *lo = nullptr, *coff = nullptr, *qid = nullptr, *tmp = nullptr;
    GX_GET(call, lo, npos);
    GX_GET(call, coff, (size_t)npos + 1);
    GX_GET(call, qid, npos);
    GX_GET(call, tmp, suf_tiles((size_t)npos + 1));
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    // 1. seeds and their 64-bit total: the scan is 32-bit and is relied upon only once the host has held
    // the total against the budget
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_match_seeds(text, sa, N, b.bytes, b.off, nq, npos, L, lo, coff, qid, b.cnt, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    GX_TRY(call, hipMemcpyAsync(b.pin, b.cnt, 16, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev0, ctx->ev1, &ctx->mat_seed_ms);
    ctx->mat_words = b.pin[0];
    const uint64_t total = b.pin[1], budget = approx_budget();
    ctx->mat_cands = total;
    if (total > budget) {
        // the refusal's only output: the counts, still unscanned, summed per query
        if (candidates) {
            std::vector<uint32_t> cnt(npos);
            GX_TRY(call, hipMemcpyAsync(cnt.data(), coff, (size_t)npos * 4, hipMemcpyDeviceToHost, st));
            GX_TRY(call, hipStreamSynchronize(st));
            for (uint32_t c = 0; c < nq; ++c) {
                uint64_t s = 0;
                for (uint32_t g = offs[c]; g < offs[c + 1]; ++g) s += cnt[g];
                candidates[c] = s;
            }
        }
        return call.done(mem_budget_error(total, budget));
    }
    // 2. candidate offsets, keep, kept offsets, per-query counts
    const uint32_t T = (uint32_t)total;   // <= 2^31
    uint32_t *cg = nullptr, *ci = nullptr, *keep = nullptr, *ktmp = nullptr, *cpre = nullptr, *mpre = nullptr;
    GX_GET(call, cg, std::max<size_t>(T, 1));
    GX_GET(call, ci, std::max<size_t>(T, 1));
    GX_GET(call, keep, (size_t)T + 1);
    GX_GET(call, ktmp, suf_tiles((size_t)T + 1));
    GX_GET(call, cpre, (size_t)nq + 1);
    GX_GET(call, mpre, (size_t)nq + 1);
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    GX_TRY(call, launch_suf_scan(coff, npos + 1, false, tmp, st));
    GX_TRY(call, launch_match_keep(text, sa, N, b.bytes, b.off, qid, lo, coff, npos, T, cg, ci, keep, st));
    GX_TRY(call, launch_suf_scan(keep, T + 1, false, ktmp, st));
    GX_TRY(call, launch_match_counts(b.off, nq, coff, keep, cpre, mpre, st));
    GX_TRY(call, hipEventRecord(ctx->ev2, st));
    std::vector<uint32_t> pre(2 * ((size_t)nq + 1));
    GX_TRY(call, hipMemcpyAsync(pre.data(), cpre, ((size_t)nq + 1) * 4, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(pre.data() + nq + 1, mpre, ((size_t)nq + 1) * 4, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    double keep_ms = 0.0;
    call.elapsed(ctx->ev1, ctx->ev2, &keep_ms);
    ctx->mat_seed_ms += keep_ms;
    for (uint32_t c = 0; c <= nq; ++c) mem_offsets[c] = pre[nq + 1 + c];
    if (candidates)
        for (uint32_t c = 0; c < nq; ++c) candidates[c] = pre[c + 1] - pre[c];
    const uint32_t M = pre[2 * (size_t)nq + 1];
    ctx->mat_kept = M;
    if (!mems) return call.done(GX_OK);
    if (M > cap) return call.done(mem_cap_error(M, cap));
    if (!M) return call.done(GX_OK);
    // 3. emit, sort, pack; then exactly M triples into the caller's array
    const size_t tiles = suf_tiles(M), table_n = 256 * tiles;
    uint64_t* key[2] = {nullptr, nullptr};
    uint32_t* val[2] = {nullptr, nullptr};
    uint32_t *table = nullptr, *stmp = nullptr;
    Mem* d_mems = nullptr;
    for (int k = 0; k < 2; ++k) {
        GX_GET(call, key[k], M);
        GX_GET(call, val[k], M);
    }
    GX_GET(call, table, table_n);
    GX_GET(call, stmp, suf_tiles(table_n));
    GX_GET(call, d_mems, M);
    int cur = 0;
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    GX_TRY(call, launch_match_emit(text, N, b.bytes, b.off, qid, cg, ci, keep, T, L, key[0], val[0], b.cnt + 2, st));
    // the keys are position << 32 | text position: text positions <= n, positions < npos
    GX_TRY(call, radix_sort_pairs(key, val, M, table, stmp, radix_digits(n, npos - 1), st, &cur));
    GX_TRY(call, launch_match_pack(key[cur], val[cur], M, b.off, qid, d_mems, st));
    GX_TRY(call, hipEventRecord(ctx->ev2, st));
    // (behind the last event: the events time kernels alone)
    GX_TRY(call, hipMemcpyAsync(b.pin + 2, b.cnt + 2, 8, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(mems, d_mems, (size_t)M * sizeof(Mem), hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev1, ctx->ev2, &ctx->mat_emit_ms);
    ctx->mat_words += b.pin[2];
    return call.done(GX_OK);   // (the stream is idle)
}

// The checks the two entry points share, in their order, then the batch as the drivers take it.  len_name,
// len: max_len or min_len, refused at 0; mem_offsets: checked when the call has one (want_offsets).
int match_prologue(const gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq, uint32_t strands,
                   const char* len_name, uint32_t len, bool want_offsets, const uint64_t* mem_offsets, HostBatch& b) {
    if (const int src = check_strands(strands)) return src;
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (want_offsets && !mem_offsets) return fail(GX_EINVAL, "mem_offsets is NULL");
    if (len == 0) return fail(GX_EINVAL, std::string(len_name) + " is 0");
    const int brc = check_batch(kQueries, queries, offsets, nq, strands);
    if (brc != GX_OK) return brc;
    strand_batch(idx, queries, offsets, nq, strands, b);   // (the item batch)
    return GX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI

extern "C" int gx_suffix_index_match_stats_strands(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets,
                                                   size_t nq, uint32_t strands, uint32_t max_len, gx_match_stat* stats) {
    HostBatch b;
    const int rc = match_prologue(idx, queries, offsets, nq, strands, "max_len", max_len, false, nullptr, b);
    if (rc != GX_OK) return rc;
    if (offsets[nq] && !stats) return fail(GX_EINVAL, "stats is NULL");
    const uint32_t items = (uint32_t)(b.offs.size() - 1);
    if (idx->ctx) return stats_device(idx, queries, b.offs.data(), items, strands, max_len, stats);
    stats_host(idx, b.padded.data(), b.offs.data(), items, max_len, stats);
    return GX_OK;
}

extern "C" int gx_suffix_index_match_stats(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq,
                                           uint32_t max_len, gx_match_stat* stats) {
    return gx_suffix_index_match_stats_strands(idx, queries, offsets, nq, GX_STRAND_FWD, max_len, stats);
}

extern "C" int gx_suffix_index_mems_strands(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq,
                                            uint32_t strands, uint32_t min_len, gx_mem* mems, size_t mems_cap,
                                            uint64_t* mem_offsets, uint64_t* candidates) {
    HostBatch b;
    const int rc = match_prologue(idx, queries, offsets, nq, strands, "min_len", min_len, true, mem_offsets, b);
    if (rc != GX_OK) return rc;
    const uint32_t items = (uint32_t)(b.offs.size() - 1);
    if (idx->ctx) return mems_device(idx, queries, b.offs.data(), items, strands, min_len, mems, mems_cap, mem_offsets, candidates);
    return mems_host(idx, b.padded.data(), b.offs.data(), items, min_len, mems, mems_cap, mem_offsets, candidates);
}

extern "C" int gx_suffix_index_mems(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq,
                                    uint32_t min_len, gx_mem* mems, size_t mems_cap, uint64_t* mem_offsets,
                                    uint64_t* candidates) {
    return gx_suffix_index_mems_strands(idx, queries, offsets, nq, GX_STRAND_FWD, min_len, mems, mems_cap, mem_offsets, candidates);
}

extern "C" int gx_match_info(const gx_context* ctx, uint64_t* candidates, uint64_t* kept, uint64_t* word_compares,
                             double* stats_ms, double* seed_ms, double* emit_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (candidates) *candidates = ctx->mat_cands;
    if (kept) *kept = ctx->mat_kept;
    if (word_compares) *word_compares = ctx->mat_words;
    if (stats_ms) *stats_ms = ctx->mat_stats_ms;
    if (seed_ms) *seed_ms = ctx->mat_seed_ms;
    if (emit_ms) *emit_ms = ctx->mat_emit_ms;
    return GX_OK;
}
