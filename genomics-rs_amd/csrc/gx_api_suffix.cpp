// gx_api_suffix.cpp -- suffix-tree mode (main.rs:154-215): what compute_stats
// (tree.rs:740-803) reads off the suffix tree of t = s + '$' -- the BWT, the
// node counts, the string depths and the longest repeat -- from the suffix
// array and the LCP array of t.
//
//   host solver    suffix_host: prefix doubling with std::sort, Kasai's LCP and
//                  a stack fold, no device: the checker on a CPU-only machine,
//                  the baseline, and the path below GX_SUFFIX_HOST_BELOW
//   device driver  suffix_device_sa: the same doubling with radix sorts and
//                  scans (gx_suffix.hip), text to device text + device suffix
//                  array; one synchronisation per round, for the convergence
//                  word and the next round's pass-skip masks.  The suffix
//                  index of search mode (gx_api_search.cpp) calls it too.
//                  suffix_device: what follows it here: LCP, fold, BWT, copies
//   Display        gx_format_suffix_stats (display.rs:8-38)
#include <charconv>
#include <cmath>

#include "gx_api_call.h"

namespace {

uint64_t suf_env_u64(const char* name, uint64_t dflt) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return end == e ? dflt : (uint64_t)v;
}

// Inputs shorter than this go to the host solver (GX_SUFFIX_HOST_BELOW).  On
// random ACGT a whole call costs 0.24 ms at 256 bases and 0.41 ms at 4,096 on
// the device against 0.007 and 0.26 ms on the host solver; at 16,384 the device
// wins, 0.50 against 1.34 ms (profiles/suffix_tree.json).  The
// crossing lies between 4,096 and 16,384 and was not resolved further; the
// default is its lower bracket (an input of exactly 4,096 bytes, where the
// host still wins, goes to the device).
constexpr uint64_t kSuffixHostBelowDefault = 4096;

// ---------------------------------------------------------------------------
// host solver

struct SufArrays {
    std::vector<uint32_t> sa, lcp;
};

// Kasai's LCP from SA and its inverse: O(N) byte compares.
void kasai_host(const uint8_t* t, const uint32_t* sa, const uint32_t* rank, size_t N, std::vector<uint32_t>& lcp) {
    lcp.assign(N, 0);
    size_t h = 0;
    for (size_t i = 0; i < N; ++i) {
        const uint32_t r = rank[i];
        if (!r) { h = 0; continue; }
        const size_t j = sa[r - 1];
        while (t[i + h] == t[j + h]) ++h;   // ('$' is unique: they differ inside the text)
        lcp[r] = (uint32_t)h;
        if (h) --h;
    }
}

}  // namespace

uint64_t suffix_host_below() { return suf_env_u64("GX_SUFFIX_HOST_BELOW", kSuffixHostBelowDefault); }

// t: N = n + 1 bytes ending in '$', followed by 8 zero bytes.
void suffix_host_sa(const uint8_t* t, size_t N, std::vector<uint32_t>& sa, std::vector<uint32_t>& rank) {
    struct Item {
        uint64_t key;
        uint32_t idx;
    };
    std::vector<Item> it(N);
    rank.assign(N, 0);
    for (size_t i = 0; i < N; ++i) {
        uint64_t k = 0;
        for (int q = 0; q < 8; ++q) k = (k << 8) | t[i + q];
        it[i] = Item{k, (uint32_t)i};
    }
    const auto by_key = [](const Item& a, const Item& b) { return a.key < b.key; };
    for (uint64_t h = 8;; h *= 2) {
        std::sort(it.begin(), it.end(), by_key);
        uint32_t r = 0;
        for (size_t k = 0; k < N; ++k) {
            if (k && it[k].key != it[k - 1].key) ++r;
            rank[it[k].idx] = r;
        }
        if (r == N - 1) break;
        for (size_t i = 0; i < N; ++i)
            it[i] = Item{((uint64_t)rank[i] << 32) | (i + h < N ? rank[i + h] : 0u), (uint32_t)i};
    }
    sa.resize(N);
    for (size_t k = 0; k < N; ++k) sa[k] = it[k].idx;
}

namespace {

void suffix_host(const uint8_t* t, size_t N, SufArrays& o) {
    std::vector<uint32_t> rank;
    suffix_host_sa(t, N, o.sa, rank);
    kasai_host(t, o.sa.data(), rank.data(), N, o.lcp);
}

// The fold of DESIGN.md 17.1 with a stack of strictly increasing depths.
void stats_host(const uint32_t* sa, const uint32_t* lcp, size_t N, gx_suffix_stats* st) {
    std::vector<uint32_t> stack{0};
    uint64_t cnt = 0, sum = 0, mx = 0, ks = 0;
    for (size_t k = 1; k < N; ++k) {
        const uint32_t v = lcp[k];
        while (stack.back() > v) stack.pop_back();
        if (stack.back() < v) {
            ++cnt;
            sum += v;
            stack.push_back(v);
        }
        if (v > mx) { mx = v; ks = k; }
    }
    st->num_internal = cnt;
    st->num_leaves = N;
    st->num_nodes = cnt + N + 1;
    st->string_depth_sum = sum;
    st->max_string_depth = st->longest_repeat_len = mx;
    st->longest_repeat_start = mx ? (uint64_t)sa[ks - 1] + 1 : 0;
}

void bwt_host(const uint8_t* t, const uint32_t* sa, size_t N, uint8_t* bwt) {
    for (size_t k = 0; k < N; ++k) bwt[k] = sa[k] ? t[sa[k] - 1] : (uint8_t)'$';
}

// ---------------------------------------------------------------------------
// device driver

// The LCP kernel does up to (N / C) * max LCP byte compares in one launch and
// the fold up to (N / B) * max LCP block steps: quadratic on
// unary or long-period input (A^(1 Mi): 18.8 ms; A^(256 Mi) would hold the
// device for some 20 minutes).  The doubling bounds max LCP below its last
// offset h before either runs, so when (N / C) * (h / 8) 8-byte compares
// exceed this budget the LCP and the fold are done on the host, in O(N)
// (GX_SUFFIX_LCP_BUDGET).  2^40 is about 130 times the A^(1 Mi) launch.
constexpr uint64_t kSuffixLcpBudgetDefault = 1ull << 40;

// The scope of a suffix-array construction, for GX_TRY and GX_GET as a DevCall (gx_api_call.h), over the
// buffers of a SufDev, which outlive suffix_device_sa when it succeeds: done(GX_OK) leaves them with the
// SufDev under `keep` and returns them otherwise; a failing done() waits until nothing of the call still runs
// on them and returns them.
struct SufCall {
    gx_context* ctx;
    SufDev& w;
    bool keep;
    int get(DevBuf& b, size_t bytes) { return pool_get(ctx, bytes, &b, ctx->stream); }
    int done(int rc) {
        if (rc != GX_OK) (void)hipStreamSynchronize(ctx->stream);
        if (rc != GX_OK || !keep) w.release(ctx);
        return rc;
    }
};

}  // namespace

hipError_t radix_sort_pairs(uint64_t* const key[2], uint32_t* const val[2], uint32_t count, uint32_t* table, uint32_t* tmp,
                            uint64_t digits, hipStream_t st, int* cur, unsigned* ran) {
    for (int p = 0; p < 8; ++p) {
        if (!((digits >> (8 * p)) & 0xffull)) continue;   // the same digit in every key
        const int c = *cur;
        const hipError_t e = launch_suf_sort_pass(key[c], val[c], key[c ^ 1], val[c ^ 1], count, 8 * p, table, tmp, st);
        if (e != hipSuccess) return e;
        *cur = c ^ 1;
        if (ran) *ran |= 1u << p;
    }
    return hipSuccess;
}

// Text to device text and device suffix array (gx_api.h): what suffix-tree
// mode and the suffix index (gx_api_search.cpp) share.
int suffix_device_sa(gx_context* ctx, const uint8_t* t, uint32_t N, bool with_stats, bool with_bwt, SufDev& w,
                     SufInfo& info) {
    hipStream_t st = ctx->stream;
    const size_t tiles = suf_tiles(N);
    const size_t table_n = 256 * tiles;
    const size_t tmp_n = std::max(suf_tiles(table_n), tiles);
    const size_t nfb = (N + (size_t)kSufFoldBlock - 1) / kSufFoldBlock;
    SufCall call{ctx, w, true};
    GX_GET(call, w.text, (size_t)N + kSufPad);
    for (int q = 0; q < 2; ++q) {
        GX_GET(call, w.k[q], (size_t)N * 8);
        GX_GET(call, w.v[q], (size_t)N * 4);
    }
    GX_GET(call, w.rank, (size_t)N * 4);
    GX_GET(call, w.flags, (size_t)N * 4);
    GX_GET(call, w.table, table_n * 4);
    GX_GET(call, w.tmp, tmp_n * 4);
    GX_GET(call, w.small, 64);
    if (with_stats) GX_GET(call, w.fold, nfb * 28);
    if (with_bwt) GX_GET(call, w.bwt, (size_t)N);
    // device words: [0] OR of the keys, [1] their AND, [2] the last rank, [4..8) the fold
    uint64_t* d_masks = (uint64_t*)w.small.p;
    uint32_t* d_last = (uint32_t*)(d_masks + 2);
    // pinned words: [0..2) the masks' presets, [2..5) masks and last rank as read back, [8..12) the fold
    uint64_t* pin = w.pin = (uint64_t*)io_pinned(ctx, 128);
    if (!pin) return call.done(fail(GX_ENOMEM, "suffix: pinned staging"));
    pin[0] = 0;
    pin[1] = ~0ull;
    const uint8_t* text = (const uint8_t*)w.text.p;
    uint32_t* rank = (uint32_t*)w.rank.p;
    uint32_t* flags = (uint32_t*)w.flags.p;
    int cur = 0;
    uint64_t* const K[2] = {(uint64_t*)w.k[0].p, (uint64_t*)w.k[1].p};
    uint32_t* const V[2] = {(uint32_t*)w.v[0].p, (uint32_t*)w.v[1].p};
    // (a pageable source: the copy has left `t` once the stream is synchronised below)
    GX_TRY(call, hipMemcpyAsync(w.text.p, t, (size_t)N + kSufPad, hipMemcpyHostToDevice, st));
    GX_TRY(call, hipMemcpyAsync(d_masks, pin, 16, hipMemcpyHostToDevice, st));
    GX_TRY(call, launch_suf_keys0(text, N, K[cur], V[cur], d_masks, st));
    GX_TRY(call, hipMemcpyAsync(pin + 2, d_masks, 16, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    uint64_t h = 8;   // after a round: suffixes with equal ranks agree in their first h bytes
    for (;; h *= 2) {
        if (h >= (1ull << 31)) return call.done(fail(GX_EHIP, "suffix: the doubling did not converge"));
        const uint64_t diff = pin[2] ^ pin[3];   // bits in which the keys differ
        GX_TRY(call, hipEventRecord(ctx->ev0, st));
        unsigned ran = 0;
        GX_TRY(call, radix_sort_pairs(K, V, N, (uint32_t*)w.table.p, (uint32_t*)w.tmp.p, diff, st, &cur, &ran));
        for (int p = 0; p < 8; ++p)
            if ((ran >> p) & 1u) {
                ++info.passes;
                ++info.digit_passes[p];
            }
        GX_TRY(call, hipEventRecord(ctx->ev1, st));
        GX_TRY(call, launch_suf_ranks(K[cur], V[cur], N, flags, (uint32_t*)w.tmp.p, rank, d_last, st));
        // the next round's keys and masks ride along (unused when this round was the last)
        GX_TRY(call, hipMemcpyAsync(d_masks, pin, 16, hipMemcpyHostToDevice, st));
        GX_TRY(call, launch_suf_keys(rank, N, (uint32_t)h, K[cur ^ 1], V[cur ^ 1], d_masks, st));
        GX_TRY(call, hipMemcpyAsync(pin + 2, d_masks, 24, hipMemcpyDeviceToHost, st));
        GX_TRY(call, hipStreamSynchronize(st));
        double ms = 0.0;
        DevCall::elapsed(ctx->ev0, ctx->ev1, &ms);
        info.sort_ms += ms;
        ++info.rounds;
        if ((uint32_t)pin[4] == N - 1) break;
        cur ^= 1;
    }
    w.cur = cur;
    w.h = h;
    return GX_OK;
}

namespace {

// t: N bytes ending in '$' and kSufPad zero bytes.  The caller holds ctx->mu.
int suffix_device(gx_context* ctx, const uint8_t* t, uint32_t N, gx_suffix_stats* out, uint8_t* bwt, uint32_t* sa,
                  uint32_t* lcp, SufInfo& info) {
    hipStream_t st = ctx->stream;
    const size_t nfb = (N + (size_t)kSufFoldBlock - 1) / kSufFoldBlock;
    SufDev w;
    {
        const int rc = suffix_device_sa(ctx, t, N, true, bwt != nullptr, w, info);
        if (rc != GX_OK) return rc;
    }
    SufCall call{ctx, w, false};
    DevBuf &d_fold = w.fold, &d_bwt = w.bwt;
    uint64_t* d_masks = (uint64_t*)w.small.p;
    SufFold* d_res = (SufFold*)(d_masks + 4);
    uint64_t* pin = w.pin;
    const uint8_t* text = (const uint8_t*)w.text.p;
    uint32_t* rank = (uint32_t*)w.rank.p;
    uint32_t* flags = (uint32_t*)w.flags.p;
    const uint64_t h = w.h;
    const uint32_t* d_sa = (const uint32_t*)w.v[w.cur].p;
    // all ranks differ, so max LCP < h: the bound on the LCP kernel's and the fold's work
    const uint64_t lanes = ((uint64_t)N + kSufLcpChunk - 1) / kSufLcpChunk;
    if (lanes * (h / 8) > suf_env_u64("GX_SUFFIX_LCP_BUDGET", kSuffixLcpBudgetDefault)) {
        std::vector<uint32_t> hsa(N), hrank(N), hlcp;
        GX_TRY(call, hipMemcpyAsync(hsa.data(), d_sa, (size_t)N * 4, hipMemcpyDeviceToHost, st));
        GX_TRY(call, hipStreamSynchronize(st));
        call.done(GX_OK);   // (the stream is idle)
        for (uint32_t k = 0; k < N; ++k) {
            if (hsa[k] >= N) return fail(GX_EHIP, "suffix: suffix array entry out of range");
            hrank[hsa[k]] = k;
        }
        kasai_host(t, hsa.data(), hrank.data(), N, hlcp);
        stats_host(hsa.data(), hlcp.data(), N, out);
        if (bwt) bwt_host(t, hsa.data(), N, bwt);
        if (sa) memcpy(sa, hsa.data(), (size_t)N * 4);
        if (lcp) memcpy(lcp, hlcp.data(), (size_t)N * 4);
        return GX_OK;   // (lcp_ms and fold_ms stay 0: those kernels did not run)
    }
    uint32_t* d_lcp = flags;   // (the head flags are done with)
    if (bwt) GX_TRY(call, launch_suf_bwt(text, d_sa, N, (uint8_t*)d_bwt.p, st));
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_suf_lcp(text, d_sa, rank, N, d_lcp, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    uint32_t* d_bmin = (uint32_t*)((uint8_t*)d_fold.p + nfb * 24);
    uint64_t* d_part = (uint64_t*)d_fold.p;
    GX_TRY(call, launch_suf_fold(d_lcp, d_sa, N, d_bmin, d_part, d_part + nfb, d_part + 2 * nfb, d_res, st));
    GX_TRY(call, hipEventRecord(ctx->ev2, st));
    GX_TRY(call, hipMemcpyAsync(pin + 8, d_res, sizeof(SufFold), hipMemcpyDeviceToHost, st));
    if (bwt) GX_TRY(call, hipMemcpyAsync(bwt, d_bwt.p, N, hipMemcpyDeviceToHost, st));
    if (sa) GX_TRY(call, hipMemcpyAsync(sa, d_sa, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    if (lcp) GX_TRY(call, hipMemcpyAsync(lcp, d_lcp, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    DevCall::elapsed(ctx->ev0, ctx->ev1, &info.lcp_ms);
    DevCall::elapsed(ctx->ev1, ctx->ev2, &info.fold_ms);
    SufFold f;
    memcpy(&f, pin + 8, sizeof f);
    call.done(GX_OK);   // (the stream is idle)
    out->num_internal = f.num_internal;
    out->num_leaves = N;
    out->num_nodes = f.num_internal + N + 1;
    out->string_depth_sum = f.depth_sum;
    out->max_string_depth = out->longest_repeat_len = f.max_key >> 32;
    out->longest_repeat_start = f.repeat_start;
    return GX_OK;
}

// Rust's `{}` of an f64: the shortest digits that round-trip, never an exponent.
std::string suf_f64(double v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char b[400];
    const auto r = std::to_chars(b, b + sizeof b, v, std::chars_format::fixed);
    return std::string(b, r.ptr);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI

extern "C" int gx_suffix_tree_stats(gx_context* ctx, const uint8_t* s, size_t n, gx_suffix_stats* out, uint8_t* bwt,
                                    uint32_t* sa, uint32_t* lcp) {
    if (!out) return fail(GX_EINVAL, "out is NULL");
    if (n && !s) return fail(GX_EINVAL, "s is NULL");
    if (n >= (1ull << 30)) return fail(GX_ERANGE, "suffix tree: sequence of 2^30 bytes or more");
    // bytes at or below '$' collide with the terminator (and the keys' zero padding)
    for (size_t k = 0; k < n; ++k)
        if (s[k] <= 0x24)
            return fail(GX_EINVAL, "s: byte " + std::to_string((int)s[k]) + " at " + std::to_string(k) +
                                       " is not above '$' (the reference's terminator)");
    const size_t N = n + 1;
    std::vector<uint8_t> t(N + kSufPad, 0);
    if (n) memcpy(t.data(), s, n);
    t[n] = '$';
    const bool host = !ctx || n == 0 || n < suf_env_u64("GX_SUFFIX_HOST_BELOW", kSuffixHostBelowDefault);
    SufInfo info;
    int rc = GX_OK;
    if (host) {
        SufArrays a;
        suffix_host(t.data(), N, a);
        stats_host(a.sa.data(), a.lcp.data(), N, out);
        if (bwt) bwt_host(t.data(), a.sa.data(), N, bwt);
        if (sa) memcpy(sa, a.sa.data(), N * 4);
        if (lcp) memcpy(lcp, a.lcp.data(), N * 4);
        if (!ctx) return GX_OK;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!host) {
        HIPCHK(hipSetDevice(ctx->device));
        rc = suffix_device(ctx, t.data(), (uint32_t)N, out, bwt, sa, lcp, info);
    }
    // (a call answered by the host solver leaves zeros: no kernel ran)
    ctx->suf_rounds = info.rounds;
    ctx->suf_passes = info.passes;
    for (int p = 0; p < 8; ++p) ctx->suf_digit_passes[p] = info.digit_passes[p];
    ctx->suf_sort_ms = info.sort_ms;
    ctx->suf_lcp_ms = info.lcp_ms;
    ctx->suf_fold_ms = info.fold_ms;
    return rc;
}

extern "C" int gx_suffix_info(const gx_context* ctx, uint64_t* doubling_rounds, uint64_t* sort_passes,
                              double* sort_ms, double* lcp_ms, double* fold_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (doubling_rounds) *doubling_rounds = ctx->suf_rounds;
    if (sort_passes) *sort_passes = ctx->suf_passes;
    if (sort_ms) *sort_ms = ctx->suf_sort_ms;
    if (lcp_ms) *lcp_ms = ctx->suf_lcp_ms;
    if (fold_ms) *fold_ms = ctx->suf_fold_ms;
    return GX_OK;
}

extern "C" int gx_suffix_digit_passes(const gx_context* ctx, uint64_t passes[8]) {
    if (!ctx || !passes) return fail(GX_EINVAL, "NULL argument");
    for (int p = 0; p < 8; ++p) passes[p] = ctx->suf_digit_passes[p];
    return GX_OK;
}

extern "C" int gx_suffix_tile(int* sort_items_per_wg, int* lcp_chunk, int* fold_block) {
    if (sort_items_per_wg) *sort_items_per_wg = kSufTile;
    if (lcp_chunk) *lcp_chunk = kSufLcpChunk;
    if (fold_block) *fold_block = kSufFoldBlock;
    return GX_OK;
}

extern "C" int gx_format_suffix_stats(const gx_suffix_stats* st, const uint8_t* bwt, size_t bwt_len, char* out,
                                      size_t cap, size_t* needed) {
    if (!st || (!bwt && bwt_len)) return fail(GX_EINVAL, "NULL argument");
    // display.rs:8-38: the literal starts with a newline and indents by 12
    const std::string ind = "\n            ";
    std::string f = ind + "BWT: ";
    if (bwt_len > 100) {
        f.append((const char*)bwt, 100);
        f += "... (truncated)";
    } else {
        f.append((const char*)bwt, bwt_len);
    }
    const double avg = (double)st->string_depth_sum / (double)st->num_internal;   // 0 / 0 = NaN (tree.rs:801)
    f += ind + "BWT Length: " + std::to_string(bwt_len);
    f += ind + "Internal nodes: " + std::to_string(st->num_internal);
    f += ind + "Leaves: " + std::to_string(st->num_leaves);
    f += ind + "Nodes: " + std::to_string(st->num_nodes);
    f += ind + "Average string depth: " + suf_f64(avg);
    f += ind + "Max string depth: " + std::to_string(st->max_string_depth);
    f += ind + "Longest repeat start: " + std::to_string(st->longest_repeat_start);
    f += ind + "Longest repeat length: " + std::to_string(st->longest_repeat_len);
    f += ind;
    if (needed) *needed = f.size() + 1;
    if (!out || cap < f.size() + 1) return fail(GX_ECAP, "output buffer too small");
    memcpy(out, f.c_str(), f.size() + 1);
    return GX_OK;
}
