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
#include "gx_api.h"
#include "gx_match.h"

namespace {

static_assert(sizeof(gx_match_stat) == sizeof(MatchStat), "gx_match_stat layout");
static_assert(sizeof(gx_mem) == sizeof(Mem), "gx_mem layout");

// What both calls refuse of a batch before a query byte is staged.
int check_queries(const uint8_t* queries, const uint64_t* offsets, size_t nq) {
    if (offsets[0] != 0) return fail(GX_EINVAL, "offsets[0] is not 0");
    for (size_t c = 0; c < nq; ++c)
        if (offsets[c + 1] < offsets[c]) return fail(GX_EINVAL, "offsets decrease at query " + std::to_string(c));
    const uint64_t total = offsets[nq];
    // (the device's offsets and scans are 32-bit: the positions plus one, the scan's tile rounding and the padding)
    if (total + kSufTile + kSufPad >= (1ull << 32) || (uint64_t)nq + 1 + kSufTile >= (1ull << 32))
        return fail(GX_ERANGE, "match: " + std::to_string(total) + " query bytes in " + std::to_string(nq) +
                                   " queries, 2^32 or more with the padding and the scan's tile rounding: split the batch");
    if (total && !queries) return fail(GX_EINVAL, "queries is NULL");
    unsigned low = 0;
    for (uint64_t k = 0; k < total; ++k) low |= queries[k] <= 0x24;
    for (size_t c = 0; low && c < nq; ++c)
        for (uint64_t k = offsets[c]; k < offsets[c + 1]; ++k)
            if (queries[k] <= 0x24)
                return fail(GX_EINVAL, "query " + std::to_string(c) + ": byte " + std::to_string((int)queries[k]) +
                                           " at offset " + std::to_string(k - offsets[c]) + " is not above '$'");
    return GX_OK;
}

int mem_budget_error(uint64_t total, uint64_t budget) {
    return fail(GX_ERANGE, "mems: " + std::to_string(total) + " candidate pairs, more than GX_APPROX_CAND_BUDGET = " +
                               std::to_string(budget) + ": split the batch, raise min_len, or raise GX_APPROX_CAND_BUDGET");
}

int mem_cap_error(uint64_t total, size_t cap) {
    return fail(GX_ECAP, "mems: " + std::to_string(total) + " MEMs needed, mems_cap is " + std::to_string(cap));
}

// The radix passes that sort position << 32 | text position: a key byte that is
// zero in every key (text positions <= n, positions < npos) is skipped.
bool mem_pass_needed(int p, uint32_t n, uint32_t npos) {
    return p < 4 ? (n >> (8 * p)) != 0 : ((npos - 1) >> (8 * (p - 4))) != 0;
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

// q: the caller's npos query bytes, unpadded.  Takes ctx->mu.
int stats_device(gx_suffix_index* idx, const uint8_t* q, const uint32_t* offs, uint32_t nq, uint32_t W,
                 gx_match_stat* stats) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t N = (uint32_t)idx->n + 1, npos = offs[nq];
    reset_info(ctx);
    if (!npos) return GX_OK;
    DevBuf d_q, d_off, d_stats, d_small;
    auto done = [&](int rc) {
        if (rc != GX_OK) (void)hipStreamSynchronize(st);   // nothing of this call still runs on the buffers
        for (DevBuf* b : {&d_q, &d_off, &d_stats, &d_small}) pool_put(ctx, *b);
        return rc;
    };
    SR_GET(d_q, (size_t)npos + kSufPad);
    SR_GET(d_off, ((size_t)nq + 1) * 4);
    SR_GET(d_stats, (size_t)npos * sizeof(MatchStat));
    SR_GET(d_small, 64);
    unsigned long long* d_cnt = (unsigned long long*)d_small.p;
    SR_TRY(hipMemcpyAsync(d_q.p, q, npos, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync((uint8_t*)d_q.p + npos, 0, kSufPad, st));
    SR_TRY(hipMemcpyAsync(d_off.p, offs, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync(d_cnt, 0, 8, st));
    SR_TRY(hipEventRecord(ctx->ev0, st));
    SR_TRY(launch_match_stats((const uint8_t*)idx->d_text.p, (const uint32_t*)idx->d_sa.p, N, (const uint8_t*)d_q.p,
                              (const uint32_t*)d_off.p, nq, npos, W, (MatchStat*)d_stats.p, d_cnt, st));
    SR_TRY(hipEventRecord(ctx->ev1, st));
    unsigned long long* pin = (unsigned long long*)io_pinned(ctx, 128);
    if (!pin) return done(fail(GX_ENOMEM, "match: pinned staging"));
    // (behind the last event: the events time the kernel alone)
    SR_TRY(hipMemcpyAsync(pin, d_cnt, 8, hipMemcpyDeviceToHost, st));
    SR_TRY(hipMemcpyAsync(stats, d_stats.p, (size_t)npos * sizeof(MatchStat), hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->mat_stats_ms = ms;
    ctx->mat_words = pin[0];
    return done(GX_OK);
}

// q: unpadded.  Takes ctx->mu.
int mems_device(gx_suffix_index* idx, const uint8_t* q, const uint32_t* offs, uint32_t nq, uint32_t L, gx_mem* mems,
                size_t cap, uint64_t* mem_offsets, uint64_t* candidates) {
    gx_context* ctx = idx->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)idx->n, N = n + 1, npos = offs[nq];
    reset_info(ctx);
    if (!npos) {
        for (uint32_t c = 0; c <= nq; ++c) mem_offsets[c] = 0;
        if (candidates) std::fill(candidates, candidates + nq, 0);
        return GX_OK;
    }
    DevBuf d_q, d_off, d_lo, d_coff, d_qid, d_tmp, d_small, d_cg, d_ci, d_keep, d_ktmp, d_cpre, d_mpre, d_key[2], d_val[2],
        d_table, d_stmp, d_mems;
    auto done = [&](int rc) {
        if (rc != GX_OK) (void)hipStreamSynchronize(st);   // nothing of this call still runs on the buffers
        for (DevBuf* b : {&d_q, &d_off, &d_lo, &d_coff, &d_qid, &d_tmp, &d_small, &d_cg, &d_ci, &d_keep, &d_ktmp, &d_cpre,
                          &d_mpre, &d_key[0], &d_key[1], &d_val[0], &d_val[1], &d_table, &d_stmp, &d_mems})
            pool_put(ctx, *b);
        return rc;
    };
    SR_GET(d_q, (size_t)npos + kSufPad);
    SR_GET(d_off, ((size_t)nq + 1) * 4);
    SR_GET(d_lo, (size_t)npos * 4);
    SR_GET(d_coff, ((size_t)npos + 1) * 4);
    SR_GET(d_qid, (size_t)npos * 4);
    SR_GET(d_tmp, suf_tiles((size_t)npos + 1) * 4);
    SR_GET(d_small, 64);
    unsigned long long* d_cnt = (unsigned long long*)d_small.p;   // [0] seed word steps, [1] candidates, [2] emit word steps
    SR_TRY(hipMemcpyAsync(d_q.p, q, npos, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync((uint8_t*)d_q.p + npos, 0, kSufPad, st));
    SR_TRY(hipMemcpyAsync(d_off.p, offs, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemsetAsync(d_cnt, 0, 24, st));
    const uint8_t* text = (const uint8_t*)idx->d_text.p;
    const uint32_t* sa = (const uint32_t*)idx->d_sa.p;
    const uint8_t* dq = (const uint8_t*)d_q.p;
    const uint32_t* off = (const uint32_t*)d_off.p;
    uint32_t* lo = (uint32_t*)d_lo.p;
    uint32_t* coff = (uint32_t*)d_coff.p;
    uint32_t* qid = (uint32_t*)d_qid.p;
    // 1. seeds and their 64-bit total: the scan is 32-bit and is relied upon only once the host has held
    // the total against the budget
    SR_TRY(hipEventRecord(ctx->ev0, st));
    SR_TRY(launch_match_seeds(text, sa, N, dq, off, nq, npos, L, lo, coff, qid, d_cnt, st));
    SR_TRY(hipEventRecord(ctx->ev1, st));
    unsigned long long* pin = (unsigned long long*)io_pinned(ctx, 128);
    if (!pin) return done(fail(GX_ENOMEM, "mems: pinned staging"));
    SR_TRY(hipMemcpyAsync(pin, d_cnt, 16, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->mat_seed_ms = ms;
    ctx->mat_words = pin[0];
    const uint64_t total = pin[1], budget = approx_budget();
    ctx->mat_cands = total;
    if (total > budget) {
        // the refusal's only output: the counts, still unscanned, summed per query
        if (candidates) {
            std::vector<uint32_t> cnt(npos);
            SR_TRY(hipMemcpyAsync(cnt.data(), coff, (size_t)npos * 4, hipMemcpyDeviceToHost, st));
            SR_TRY(hipStreamSynchronize(st));
            for (uint32_t c = 0; c < nq; ++c) {
                uint64_t s = 0;
                for (uint32_t g = offs[c]; g < offs[c + 1]; ++g) s += cnt[g];
                candidates[c] = s;
            }
        }
        return done(mem_budget_error(total, budget));
    }
    // 2. candidate offsets, keep, kept offsets, per-query counts
    const uint32_t T = (uint32_t)total;   // <= 2^31
    SR_GET(d_cg, std::max<size_t>(T, 1) * 4);
    SR_GET(d_ci, std::max<size_t>(T, 1) * 4);
    SR_GET(d_keep, ((size_t)T + 1) * 4);
    SR_GET(d_ktmp, suf_tiles((size_t)T + 1) * 4);
    SR_GET(d_cpre, ((size_t)nq + 1) * 4);
    SR_GET(d_mpre, ((size_t)nq + 1) * 4);
    uint32_t* keep = (uint32_t*)d_keep.p;
    SR_TRY(hipEventRecord(ctx->ev1, st));
    SR_TRY(launch_suf_scan(coff, npos + 1, false, (uint32_t*)d_tmp.p, st));
    SR_TRY(launch_match_keep(text, sa, N, dq, off, qid, lo, coff, npos, T, (uint32_t*)d_cg.p, (uint32_t*)d_ci.p, keep, st));
    SR_TRY(launch_suf_scan(keep, T + 1, false, (uint32_t*)d_ktmp.p, st));
    SR_TRY(launch_match_counts(off, nq, coff, keep, (uint32_t*)d_cpre.p, (uint32_t*)d_mpre.p, st));
    SR_TRY(hipEventRecord(ctx->ev2, st));
    std::vector<uint32_t> pre(2 * ((size_t)nq + 1));
    SR_TRY(hipMemcpyAsync(pre.data(), d_cpre.p, ((size_t)nq + 1) * 4, hipMemcpyDeviceToHost, st));
    SR_TRY(hipMemcpyAsync(pre.data() + nq + 1, d_mpre.p, ((size_t)nq + 1) * 4, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    if (hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2) == hipSuccess) ctx->mat_seed_ms += ms;
    for (uint32_t c = 0; c <= nq; ++c) mem_offsets[c] = pre[nq + 1 + c];
    if (candidates)
        for (uint32_t c = 0; c < nq; ++c) candidates[c] = pre[c + 1] - pre[c];
    const uint32_t M = pre[2 * (size_t)nq + 1];
    ctx->mat_kept = M;
    if (!mems) return done(GX_OK);
    if (M > cap) return done(mem_cap_error(M, cap));
    if (!M) return done(GX_OK);
    // 3. emit, sort, pack; then exactly M triples into the caller's array
    const size_t tiles = suf_tiles(M), table_n = 256 * tiles;
    for (int k = 0; k < 2; ++k) {
        SR_GET(d_key[k], (size_t)M * 8);
        SR_GET(d_val[k], (size_t)M * 4);
    }
    SR_GET(d_table, table_n * 4);
    SR_GET(d_stmp, suf_tiles(table_n) * 4);
    SR_GET(d_mems, (size_t)M * sizeof(Mem));
    int cur = 0;
    auto K = [&](int k) { return (uint64_t*)d_key[k].p; };
    auto V = [&](int k) { return (uint32_t*)d_val[k].p; };
    SR_TRY(hipEventRecord(ctx->ev1, st));
    SR_TRY(launch_match_emit(text, N, dq, off, qid, (const uint32_t*)d_cg.p, (const uint32_t*)d_ci.p, keep, T, L, K(cur),
                             V(cur), d_cnt + 2, st));
    for (int p = 0; p < 8; ++p) {
        if (!mem_pass_needed(p, n, npos)) continue;
        SR_TRY(launch_suf_sort_pass(K(cur), V(cur), K(cur ^ 1), V(cur ^ 1), M, 8 * p, (uint32_t*)d_table.p,
                                    (uint32_t*)d_stmp.p, st));
        cur ^= 1;
    }
    SR_TRY(launch_match_pack(K(cur), V(cur), M, off, qid, (Mem*)d_mems.p, st));
    SR_TRY(hipEventRecord(ctx->ev2, st));
    // (behind the last event: the events time kernels alone)
    SR_TRY(hipMemcpyAsync(pin + 2, d_cnt + 2, 8, hipMemcpyDeviceToHost, st));
    SR_TRY(hipMemcpyAsync(mems, d_mems.p, (size_t)M * sizeof(Mem), hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    if (hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2) == hipSuccess) ctx->mat_emit_ms = ms;
    ctx->mat_words += pin[2];
    return done(GX_OK);   // (the stream is idle)
}
#undef SR_TRY
#undef SR_GET

}  // namespace

// ---------------------------------------------------------------------------
// C ABI

extern "C" int gx_suffix_index_match_stats(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq,
                                           uint32_t max_len, gx_match_stat* stats) {
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (max_len == 0) return fail(GX_EINVAL, "max_len is 0");
    const int brc = check_queries(queries, offsets, nq);
    if (brc != GX_OK) return brc;
    if (offsets[nq] && !stats) return fail(GX_EINVAL, "stats is NULL");
    const uint32_t npos = (uint32_t)offsets[nq];
    std::vector<uint32_t> offs(nq + 1);
    for (size_t c = 0; c <= nq; ++c) offs[c] = (uint32_t)offsets[c];
    if (idx->ctx) return stats_device(idx, queries, offs.data(), (uint32_t)nq, max_len, stats);
    // the host compares read 8 bytes at a time too: the same padding behind the queries
    std::vector<uint8_t> padded((size_t)npos + kSufPad, 0);
    if (npos) memcpy(padded.data(), queries, npos);
    stats_host(idx, padded.data(), offs.data(), (uint32_t)nq, max_len, stats);
    return GX_OK;
}

extern "C" int gx_suffix_index_mems(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq,
                                    uint32_t min_len, gx_mem* mems, size_t mems_cap, uint64_t* mem_offsets,
                                    uint64_t* candidates) {
    if (!idx) return fail(GX_EINVAL, "idx is NULL");
    if (!offsets) return fail(GX_EINVAL, "offsets is NULL");
    if (!mem_offsets) return fail(GX_EINVAL, "mem_offsets is NULL");
    if (min_len == 0) return fail(GX_EINVAL, "min_len is 0");
    const int brc = check_queries(queries, offsets, nq);
    if (brc != GX_OK) return brc;
    const uint32_t npos = (uint32_t)offsets[nq];
    std::vector<uint32_t> offs(nq + 1);
    for (size_t c = 0; c <= nq; ++c) offs[c] = (uint32_t)offsets[c];
    if (idx->ctx) return mems_device(idx, queries, offs.data(), (uint32_t)nq, min_len, mems, mems_cap, mem_offsets, candidates);
    std::vector<uint8_t> padded((size_t)npos + kSufPad, 0);
    if (npos) memcpy(padded.data(), queries, npos);
    return mems_host(idx, padded.data(), offs.data(), (uint32_t)nq, min_len, mems, mems_cap, mem_offsets, candidates);
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
