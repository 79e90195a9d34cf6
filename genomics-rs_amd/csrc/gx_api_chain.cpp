// gx_api_chain.cpp -- search mode for long queries: the anchors of a batch of
// queries chained into colinear chains.  No counterpart in the
// reference's main.rs.
//
//   prologue  the checks, in the order of gx.h: arguments, parameters, offsets,
//             then the host's one pass over the anchors (len, ranges, order, the
//             queries' length sums).  Nothing runs after a refusal.
//   host      the rules of gx_chain.h on one thread in the backward form of the
//             recurrence: for every b, a = b - 1 down to b - max_pred.  The
//             solver of ctx = NULL and the device's field-by-field comparison
//             partner.
//   device    the anchors staged once; flags, scan, segments, score; best, heads,
//             two scans, counts; the totals read back once for the GX_ECAP
//             decision; then the walk and the copy of exactly the totals.
// The scope of the call, the staging and the scan are the ones the other search
// calls use (gx_api_call.h).
#include "gx_api_call.h"
#include "gx_chain.h"

namespace {

static_assert(sizeof(gx_chain) == sizeof(Chain) && sizeof(gx_chain) == 40, "gx_chain layout");
static_assert(sizeof(gx_chain_params) == sizeof(ChainParams), "gx_chain_params layout");
static_assert(sizeof(gx_mem) == sizeof(Mem), "gx_mem layout");
static_assert(GX_CHAIN_NONE == kChainNone && GX_CHAIN_MAX_PRED == kChainMaxPred, "gx.h and gx_chain.h");

int chains_cap_error(uint64_t total, size_t cap) {
    return fail(GX_ECAP, "chain: " + std::to_string(total) + " chains needed, chains_cap is " + std::to_string(cap));
}

int members_cap_error(uint64_t total, size_t cap) {
    return fail(GX_ECAP, "chain: " + std::to_string(total) + " members needed, members_cap is " + std::to_string(cap));
}

// A kernel met a segment or a tree that does not fit the anchors: the outputs of the call are not to be used.
int inconsistent_error(uint64_t count) {
    return fail(GX_EHIP, "chain: " + std::to_string(count) + " segments or chains do not fit the anchors (device state corrupted)");
}

int param_error(const char* name, long long v, long long lo, long long hi) {
    return fail(GX_EINVAL, std::string("chain: ") + name + " is " + std::to_string(v) + ", outside " + std::to_string(lo) +
                               " .. " + std::to_string(hi));
}

int check_params(const ChainParams& p) {
    if (p.w_match < 1 || p.w_match > GX_CHAIN_MAX_WEIGHT) return param_error("w_match", p.w_match, 1, GX_CHAIN_MAX_WEIGHT);
    if (p.w_drift > GX_CHAIN_MAX_WEIGHT) return param_error("w_drift", p.w_drift, 0, GX_CHAIN_MAX_WEIGHT);
    if (p.max_gap < 1 || p.max_gap > GX_CHAIN_MAX_GAP) return param_error("max_gap", p.max_gap, 1, GX_CHAIN_MAX_GAP);
    if (p.max_drift > GX_CHAIN_MAX_GAP) return param_error("max_drift", p.max_drift, 0, GX_CHAIN_MAX_GAP);
    if (p.max_pred < 1 || p.max_pred > GX_CHAIN_MAX_PRED) return param_error("max_pred", p.max_pred, 1, GX_CHAIN_MAX_PRED);
    if (p.min_score < 0) return param_error("min_score", p.min_score, 0, INT32_MAX);
    return GX_OK;
}

// The host's pass over the anchors.
int check_anchors(const gx_mem* an, const uint64_t* off, size_t nq, const ChainParams& p) {
    for (size_t c = 0; c < nq; ++c) {
        uint64_t sum = 0;
        for (uint64_t g = off[c]; g < off[c + 1]; ++g) {
            const gx_mem& m = an[g];
            const std::string who = "chain: query " + std::to_string(c) + " anchor " + std::to_string(g - off[c]);
            if (m.len == 0) return fail(GX_EINVAL, who + ": len is 0");
            if ((uint64_t)m.qpos + m.len >= (1ull << 32) || (uint64_t)m.tpos + m.len >= (1ull << 32))
                return fail(GX_ERANGE, who + ": (" + std::to_string(m.qpos) + ", " + std::to_string(m.tpos) + ") + " +
                                           std::to_string(m.len) + " is at or above 2^32");
            if (g > off[c]) {
                const gx_mem& b = an[g - 1];
                if (m.qpos < b.qpos || (m.qpos == b.qpos && m.tpos <= b.tpos))
                    return fail(GX_EINVAL, who + ": (" + std::to_string(m.qpos) + ", " + std::to_string(m.tpos) +
                                               ") is not above its predecessor (" + std::to_string(b.qpos) + ", " +
                                               std::to_string(b.tpos) + ")");
            }
            sum += m.len;
        }
        if (sum * p.w_match >= (1ull << 31))
            return fail(GX_ERANGE, "chain: query " + std::to_string(c) + ": w_match * sum(len) is " +
                                       std::to_string(sum * p.w_match) + ", at or above 2^31");
    }
    return GX_OK;
}

void reset_info(gx_context* ctx) {
    ctx->chn_anchors = ctx->chn_segments = ctx->chn_evals = ctx->chn_chains = 0;
    ctx->chn_score_ms = ctx->chn_chain_ms = 0.0;
}

int chain_host(const gx_mem* an, const uint64_t* off, size_t nq, const ChainParams& p, int32_t* scores, uint32_t* preds,
               gx_chain* chains, size_t chains_cap, uint32_t* members, size_t members_cap, uint64_t* chain_offsets,
               uint64_t* members_total) {
    const uint64_t A = off[nq];
    std::vector<int32_t> f(A);
    std::vector<uint32_t> pred(A), root(A), depth(A), end(A);   // (all within the query; end: at a root, its tree's end)
    uint64_t nchains = 0, nmembers = 0;
    for (size_t c = 0; c < nq; ++c) {
        const gx_mem* q = an + off[c];
        const uint32_t n = (uint32_t)(off[c + 1] - off[c]);
        int32_t* F = f.data() + off[c];
        uint32_t *P = pred.data() + off[c], *Rt = root.data() + off[c], *D = depth.data() + off[c], *E = end.data() + off[c];
        for (uint32_t b = 0; b < n; ++b) {
            int32_t best = (int32_t)(p.w_match * q[b].len);
            uint32_t pr = kChainNone;
            for (uint32_t a = b; a-- > 0 && b - a <= p.max_pred;) {
                uint32_t dq, dt;
                if (!chain_eligible(q[a].qpos, q[a].tpos, q[b].qpos, q[b].tpos, p.max_gap, p.max_drift, &dq, &dt)) continue;
                const int32_t ext = chain_ext(F[a], q[b].len, dq, dt, p.w_match, p.w_drift);
                if (chain_take(ext, a, best, pr)) {
                    best = ext;
                    pr = a;
                }
            }
            F[b] = best;
            P[b] = pr;
            Rt[b] = pr == kChainNone ? b : Rt[pr];
            D[b] = pr == kChainNone ? 0 : D[pr] + 1;
            E[b] = b;
            if (F[b] > F[E[Rt[b]]]) E[Rt[b]] = b;   // (b ascends: of equal f the smallest index stays)
        }
        chain_offsets[c] = nchains;
        for (uint32_t r = 0; r < n; ++r)
            if (Rt[r] == r && F[E[r]] >= p.min_score) {
                ++nchains;
                nmembers += D[E[r]] + 1;
            }
    }
    chain_offsets[nq] = nchains;
    *members_total = nmembers;
    if (scores) std::copy(f.begin(), f.end(), scores);
    if (preds) std::copy(pred.begin(), pred.end(), preds);
    if (!chains) return GX_OK;
    if (nchains > chains_cap) return chains_cap_error(nchains, chains_cap);
    if (nmembers > members_cap) return members_cap_error(nmembers, members_cap);
    uint64_t k = 0, moff = 0;
    for (size_t c = 0; c < nq; ++c) {
        const gx_mem* q = an + off[c];
        const uint32_t n = (uint32_t)(off[c + 1] - off[c]);
        const int32_t* F = f.data() + off[c];
        const uint32_t *P = pred.data() + off[c], *Rt = root.data() + off[c], *D = depth.data() + off[c], *E = end.data() + off[c];
        for (uint32_t r = 0; r < n; ++r) {
            if (Rt[r] != r || F[E[r]] < p.min_score) continue;
            const uint32_t e = E[r];
            gx_chain& o = chains[k++];
            o.member_off = moff;
            o.score = F[e];
            o.n_anchors = D[e] + 1;
            o.root = r;
            o.end = e;
            o.qstart = q[r].qpos;
            o.tstart = q[r].tpos;
            o.qend = q[e].qpos + q[e].len;
            o.tend = q[e].tpos + q[e].len;
            for (uint32_t x = e;; x = P[x]) {
                members[moff + D[x]] = x;
                if (P[x] == kChainNone) break;
            }
            moff += o.n_anchors;
        }
    }
    return GX_OK;
}

// offs: the anchor offsets in 32 bits.  Takes ctx->mu.
int chain_device(gx_context* ctx, const gx_mem* an, const uint32_t* offs, uint32_t nq, const ChainParams& p, int32_t* scores,
                 uint32_t* preds, gx_chain* chains, size_t chains_cap, uint32_t* members, size_t members_cap,
                 uint64_t* chain_offsets, uint64_t* members_total) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    DevCall call(ctx);
    hipStream_t st = call.st;
    const uint32_t A = offs[nq];
    reset_info(ctx);
    *members_total = 0;
    if (!A) {
        for (uint32_t c = 0; c <= nq; ++c) chain_offsets[c] = 0;
        return GX_OK;
    }
    ctx->chn_anchors = A;
    // counters: [0] pair evaluations, [1] chains, [2] members, [3] segments, [4] entries of the segment table or of
    // the forest that a kernel found not to fit the anchors (never: the call fails on one)
    StagedBatch b;
    if (const int rc = stage_batch(call, "chain", (const uint8_t*)an, (size_t)A * sizeof(Mem), offs, nq, b)) return rc;
    const Mem* d_an = (const Mem*)b.bytes;
    const size_t A1 = (size_t)A + 1;
    uint32_t *sscan = nullptr, *stmp = nullptr, *seg_start = nullptr, *seg_base = nullptr, *pred = nullptr, *root = nullptr,
             *depth = nullptr, *kscan = nullptr, *mscan = nullptr, *ktmp = nullptr, *mtmp = nullptr, *cpre = nullptr;
    int32_t* f = nullptr;
    unsigned long long* key = nullptr;
    GX_GET(call, sscan, A1);
    GX_GET(call, stmp, suf_tiles(A1));
    GX_GET(call, seg_start, A1);
    GX_GET(call, seg_base, A1);
    GX_GET(call, f, A);
    GX_GET(call, pred, A);
    GX_GET(call, root, A);
    GX_GET(call, depth, A);
    GX_GET(call, key, A);
    GX_GET(call, kscan, A1);
    GX_GET(call, mscan, A1);
    GX_GET(call, ktmp, suf_tiles(A1));
    GX_GET(call, mtmp, suf_tiles(A1));
    GX_GET(call, cpre, (size_t)nq + 1);
    // 1. segments and scores
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_chain_flags(d_an, b.off, nq, A, p.max_gap, sscan, st));
    GX_TRY(call, launch_suf_scan(sscan, A + 1, false, stmp, st));
    GX_TRY(call, launch_chain_segments(b.off, nq, A, sscan, seg_start, seg_base, st));
    GX_TRY(call, launch_chain_score(d_an, A, sscan, seg_start, seg_base, p, f, pred, root, depth, b.cnt, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    // 2. every tree's end, the reported chains, their numbers and member offsets
    GX_TRY(call, hipMemsetAsync(key, 0, (size_t)A * 8, st));
    GX_TRY(call, launch_chain_best(f, root, A, key, st));
    GX_TRY(call, launch_chain_heads(root, depth, key, A, p.min_score, kscan, mscan, st));
    GX_TRY(call, launch_suf_scan(kscan, A + 1, false, ktmp, st));
    GX_TRY(call, launch_suf_scan(mscan, A + 1, false, mtmp, st));
    GX_TRY(call, launch_chain_counts(b.off, nq, A, sscan, kscan, mscan, cpre, b.cnt + 1, st));
    GX_TRY(call, hipEventRecord(ctx->ev2, st));
    // (behind the last event: the events time kernels alone)
    std::vector<uint32_t> pre((size_t)nq + 1);
    GX_TRY(call, hipMemcpyAsync(b.pin, b.cnt, 40, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(pre.data(), cpre, ((size_t)nq + 1) * 4, hipMemcpyDeviceToHost, st));
    if (scores) GX_TRY(call, hipMemcpyAsync(scores, f, (size_t)A * 4, hipMemcpyDeviceToHost, st));
    if (preds) GX_TRY(call, hipMemcpyAsync(preds, pred, (size_t)A * 4, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    call.elapsed(ctx->ev0, ctx->ev1, &ctx->chn_score_ms);
    call.elapsed(ctx->ev1, ctx->ev2, &ctx->chn_chain_ms);
    if (b.pin[4]) return call.done(inconsistent_error(b.pin[4]));
    const uint64_t K = b.pin[1], M = b.pin[2];
    ctx->chn_evals = b.pin[0];
    ctx->chn_chains = K;
    ctx->chn_segments = b.pin[3];
    for (uint32_t c = 0; c <= nq; ++c) chain_offsets[c] = pre[c];
    *members_total = M;
    if (!chains) return call.done(GX_OK);
    if (K > chains_cap) return call.done(chains_cap_error(K, chains_cap));
    if (M > members_cap) return call.done(members_cap_error(M, members_cap));
    if (!K) return call.done(GX_OK);
    // 3. records and members; then exactly K records and M members into the caller's arrays
    Chain* d_chains = nullptr;
    uint32_t* d_members = nullptr;
    GX_GET(call, d_chains, K);
    GX_GET(call, d_members, M);
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_chain_walk(d_an, A, sscan, seg_base, f, pred, root, depth, key, kscan, mscan, d_chains, d_members,
                                   b.cnt + 4, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    // (the walk's own check first: the caller's arrays stay untouched when it failed)
    GX_TRY(call, hipMemcpyAsync(b.pin + 4, b.cnt + 4, 8, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    if (b.pin[4]) return call.done(inconsistent_error(b.pin[4]));
    GX_TRY(call, hipMemcpyAsync(chains, d_chains, (size_t)K * sizeof(Chain), hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipMemcpyAsync(members, d_members, (size_t)M * 4, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    double walk_ms = 0.0;
    call.elapsed(ctx->ev0, ctx->ev1, &walk_ms);
    ctx->chn_chain_ms += walk_ms;
    return call.done(GX_OK);   // (the stream is idle)
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI

extern "C" int gx_chain_anchors(gx_context* ctx, const gx_mem* anchors, const uint64_t* anchor_offsets, size_t nq,
                                const gx_chain_params* params, int32_t* scores, uint32_t* preds, gx_chain* chains,
                                size_t chains_cap, uint32_t* members, size_t members_cap, uint64_t* chain_offsets,
                                uint64_t* members_total) {
    if (!anchor_offsets) return fail(GX_EINVAL, "anchor_offsets is NULL");
    if (!chain_offsets) return fail(GX_EINVAL, "chain_offsets is NULL");
    if (!members_total) return fail(GX_EINVAL, "members_total is NULL");
    ChainParams p{GX_CHAIN_DEFAULT_W_MATCH,  GX_CHAIN_DEFAULT_W_DRIFT,  GX_CHAIN_DEFAULT_MAX_GAP,
                  GX_CHAIN_DEFAULT_MAX_DRIFT, GX_CHAIN_DEFAULT_MAX_PRED, GX_CHAIN_DEFAULT_MIN_SCORE};
    if (params) p = ChainParams{params->w_match, params->w_drift, params->max_gap, params->max_drift, params->max_pred, params->min_score};
    if (const int rc = check_params(p)) return rc;
    // (the device's offsets and scans are 32-bit: one more than the queries, and the scan's tile rounding;
    // held before an offset is read)
    if ((uint64_t)nq + 1 + kSufTile >= (1ull << 32))
        return fail(GX_ERANGE, "chain: " + std::to_string(nq) + " queries, 2^32 or more with the scan's tile rounding: split the batch");
    if (anchor_offsets[0] != 0) return fail(GX_EINVAL, "anchor_offsets[0] is not 0");
    for (size_t c = 0; c < nq; ++c)
        if (anchor_offsets[c + 1] < anchor_offsets[c])
            return fail(GX_EINVAL, "anchor_offsets decrease at query " + std::to_string(c));
    if (chains && !members) return fail(GX_EINVAL, "members is NULL");
    const uint64_t A = anchor_offsets[nq], budget = approx_budget();
    if (A > budget)
        return fail(GX_ERANGE, "chain: " + std::to_string(A) + " anchors, more than GX_APPROX_CAND_BUDGET = " +
                                   std::to_string(budget) + ": split the batch, raise min_len, or raise GX_APPROX_CAND_BUDGET");
    if (A && !anchors) return fail(GX_EINVAL, "anchors is NULL");
    if (const int rc = check_anchors(anchors, anchor_offsets, nq, p)) return rc;
    if (!ctx)
        return chain_host(anchors, anchor_offsets, nq, p, scores, preds, chains, chains_cap, members, members_cap,
                          chain_offsets, members_total);
    std::vector<uint32_t> offs(nq + 1);
    for (size_t c = 0; c <= nq; ++c) offs[c] = (uint32_t)anchor_offsets[c];
    return chain_device(ctx, anchors, offs.data(), (uint32_t)nq, p, scores, preds, chains, chains_cap, members, members_cap,
                        chain_offsets, members_total);
}

extern "C" int gx_chain_info(const gx_context* ctx, uint64_t* anchors, uint64_t* segments, uint64_t* pair_evals,
                             uint64_t* chains, double* score_ms, double* chain_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (anchors) *anchors = ctx->chn_anchors;
    if (segments) *segments = ctx->chn_segments;
    if (pair_evals) *pair_evals = ctx->chn_evals;
    if (chains) *chains = ctx->chn_chains;
    if (score_ms) *score_ms = ctx->chn_score_ms;
    if (chain_ms) *chain_ms = ctx->chn_chain_ms;
    return GX_OK;
}
