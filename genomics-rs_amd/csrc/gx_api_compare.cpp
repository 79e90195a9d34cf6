// gx_api_compare.cpp -- compare mode (main.rs:216-379): the longest common
// substring of two strings (get_lcs, tree.rs:218-281) and the recursion that
// sums it over the pieces around each hit (main.rs:281-315).
//
//   host solver   lcs_host: a complete implementation with no device (row
//                 sweep of diagonal run lengths), for sub-problems below
//                 GX_COMPARE_HOST_CELLS cells, for sub-problems whose
//                 candidate buffer overflowed, and for calls without a context
//   tie rule      resolve: from the starts of all common substrings of length
//                 L, the smallest W and the smallest terminated suffix per
//                 string (the suffix tree's DFS order)
//   level driver  compare_core: the recursion of every pair level by level,
//                 one batch of launches (gx_lcsub.hip) per level
#include "gx_api_call.h"
#include "gx_lcsub.h"

namespace {

// ---------------------------------------------------------------------------
// tie rule

// Is the terminated suffix of s (len bytes) at p smaller than the one at q?
// The terminator is below every admitted byte, so a proper prefix is smaller.
bool suffix_less(const uint8_t* s, size_t len, size_t p, size_t q) {
    const size_t lp = len - p, lq = len - q;
    const int c = memcmp(s + p, s + q, std::min(lp, lq));
    return c ? c < 0 : lp < lq;
}

// is / js: the distinct starts in a / b of every common substring of length L
// (L > 0, both non-empty).  W = the smallest a[i : i + L]; *oi / *oj = the
// occurrence of W with the smallest terminated suffix in a / b.
void resolve(const uint8_t* a, size_t n, const uint8_t* b, size_t m, size_t L, const std::vector<uint32_t>& is,
             const std::vector<uint32_t>& js, uint64_t* oi, uint64_t* oj) {
    const uint8_t* W = a + is[0];
    for (uint32_t i : is)
        if (memcmp(a + i, W, L) < 0) W = a + i;
    bool have = false;
    size_t bi = 0, bj = 0;
    for (uint32_t i : is) {
        if (memcmp(a + i, W, L)) continue;
        if (!have || suffix_less(a, n, i, bi)) bi = i;
        have = true;
    }
    have = false;
    for (uint32_t j : js) {
        if (memcmp(b + j, W, L)) continue;
        if (!have || suffix_less(b, m, j, bj)) bj = j;
        have = true;
    }
    *oi = bi;
    *oj = bj;
}

// ---------------------------------------------------------------------------
// host solver

// One row of the run table: nw[j + 1] = b[j] == c ? old[j] + 1 : 0; returns the row's max.
#define GX_ROW_BODY                                       \
    int32_t mx = 0;                                       \
    for (int j = 0; j < m; ++j) {                         \
        const int32_t v = b[j] == c ? old[j] + 1 : 0;     \
        nw[j + 1] = v;                                    \
        mx = v > mx ? v : mx;                             \
    }                                                     \
    return mx;
int32_t row_plain(const uint8_t* __restrict__ b, int m, uint8_t c, const int32_t* __restrict__ old,
                  int32_t* __restrict__ nw) { GX_ROW_BODY }
__attribute__((target("avx2"))) int32_t row_avx2(const uint8_t* __restrict__ b, int m, uint8_t c,
                                                 const int32_t* __restrict__ old, int32_t* __restrict__ nw) {
    GX_ROW_BODY
}
#undef GX_ROW_BODY

struct HostScratch {
    std::vector<int32_t> r0, r1;
    std::vector<uint32_t> ga, gb, is, js;
};

// lcs(a, b) of the contract; n, m < 2^31.  *ncand (optional)
// = the number of (i, j) starts of common substrings of length L.
void lcs_host(const uint8_t* a, size_t n, const uint8_t* b, size_t m, uint64_t* oi, uint64_t* oj, uint64_t* oL,
              uint64_t* ncand = nullptr) {
    *oi = *oj = *oL = 0;
    if (ncand) *ncand = 0;
    if (!n || !m) return;
    static const bool avx2 = __builtin_cpu_supports("avx2");
    thread_local HostScratch sc;
    sc.r0.assign(m + 1, 0);
    sc.r1.assign(m + 1, 0);
    sc.ga.assign(n, 0);
    sc.gb.assign(m, 0);
    int32_t* old = sc.r0.data();
    int32_t* nw = sc.r1.data();
    int32_t L = 0;
    uint32_t gen = 0;
    uint64_t cands = 0;
    for (size_t i = 0; i < n; ++i) {
        const int32_t mx = avx2 ? row_avx2(b, (int)m, a[i], old, nw) : row_plain(b, (int)m, a[i], old, nw);
        if (mx > L) { L = mx; ++gen; cands = 0; }
        if (mx == L && L > 0)
            for (size_t j = 1; j <= m; ++j)
                if (nw[j] == L) {   // a run of L ends at (i, j - 1)
                    sc.ga[i + 1 - L] = gen;
                    sc.gb[j - L] = gen;
                    ++cands;
                }
        std::swap(old, nw);
    }
    if (!L) return;
    sc.is.clear();
    sc.js.clear();
    for (size_t i = 0; i < n; ++i) if (sc.ga[i] == gen) sc.is.push_back((uint32_t)i);
    for (size_t j = 0; j < m; ++j) if (sc.gb[j] == gen) sc.js.push_back((uint32_t)j);
    resolve(a, n, b, m, (size_t)L, sc.is, sc.js, oi, oj);
    *oL = (uint64_t)L;
    if (ncand) *ncand = cands;
}

// Input bytes at or below '$' collide with the reference's terminators.
int check_bytes(const uint8_t* s, size_t n, const char* what) {
    if (n && !s) return fail(GX_EINVAL, std::string(what) + " is NULL");
    for (size_t k = 0; k < n; ++k)
        if (s[k] <= 0x24)
            return fail(GX_EINVAL, std::string(what) + ": byte " + std::to_string((int)s[k]) + " at " +
                                       std::to_string(k) + " is not above '$' (the reference's terminators)");
    return GX_OK;
}

// ---------------------------------------------------------------------------
// level driver

struct Sub {
    uint32_t pair, a_off, n, b_off, m;
    bool root;
};
struct PairAcc {
    uint64_t score = 0, first = 0, calls = 0, ri = 0, rj = 0;
};

uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    return end == e ? dflt : (uint64_t)v;
}

// Below this many cells a sub-problem is solved on the host.  0: a level's
// launches are paid once for all its sub-problems, and on the ten-genome
// matrix every threshold above 0 only added host time.
constexpr uint64_t kHostCellsDefault = 0;

int seg_height() {
    const uint64_t h = env_u64("GX_COMPARE_SEG_H", kLcsubSeg);
    return (int)std::min<uint64_t>(std::max<uint64_t>(h, 8), kLcsubMaxSeg);
}

struct Cmp {
    gx_context* ctx = nullptr;        // nullptr: host solver only
    const uint8_t* hc = nullptr;      // the staged sequences (host copy, same offsets as the device's)
    DevBuf chars;
    uint64_t host_cells = kHostCellsDefault;
    unsigned cap = kLcsubCandCap;
    int H = kLcsubSeg;
    bool recurse = true;
    std::vector<PairAcc> acc;
    uint64_t n_gpu = 0, n_host = 0, n_ovf = 0, levels = 0, batches = 0, cells = 0;
    double run_ms = 0.0;
};

// One get_matches call (main.rs:267-279) answered: account it and push its children (main.rs:295-304).
void apply(Cmp& c, const Sub& s, uint64_t i, uint64_t j, uint64_t L, std::vector<Sub>& out) {
    PairAcc& p = c.acc[s.pair];
    ++p.calls;
    p.score += L;
    if (s.root) { p.first = L; p.ri = i; p.rj = j; }
    if (!L || !c.recurse) return;
    out.push_back(Sub{s.pair, s.a_off, (uint32_t)i, s.b_off, (uint32_t)j, false});
    out.push_back(Sub{s.pair, (uint32_t)(s.a_off + i + L), (uint32_t)(s.n - i - L), (uint32_t)(s.b_off + j + L),
                      (uint32_t)(s.m - j - L), false});
}

// A sub-problem and everything below it on the host.
void host_subtree(Cmp& c, const Sub& s0) {
    std::vector<Sub> stack{s0};
    while (!stack.empty()) {
        const Sub s = stack.back();
        stack.pop_back();
        uint64_t i = 0, j = 0, L = 0;
        if (s.n && s.m) {
            lcs_host(c.hc + s.a_off, s.n, c.hc + s.b_off, s.m, &i, &j, &L);
            ++c.n_host;
        }
        apply(c, s, i, j, L, stack);
    }
}

// One batch of non-empty sub-problems on the device: run, combine and
// candidate launches, then the tie rule on the candidates.  Children go to
// `next`.  Every buffer returns to the pool after the stream has drained.
int gpu_batch(Cmp& c, const Sub* subs, size_t nsub, std::vector<Sub>& next) {
    gx_context* ctx = c.ctx;
    hipStream_t st = ctx->stream;
    ++c.batches;
    std::vector<LcsubDesc> desc(nsub);
    uint64_t elems = 0, tiles = 0, dtiles = 0, cells = 0;
    for (size_t k = 0; k < nsub; ++k) {
        const Sub& s = subs[k];
        LcsubDesc& d = desc[k];
        d.a_off = s.a_off; d.b_off = s.b_off; d.n = s.n; d.m = s.m;
        d.ndiag = s.n + s.m - 1;
        d.nseg = (s.n + c.H - 1) / c.H;
        const uint64_t ndblk = (d.ndiag + kLcsubBlock - 1) / kLcsubBlock;
        d.tile_base = (uint32_t)tiles;
        d.dtile_base = (uint32_t)dtiles;
        d.elem_base = elems;
        d.pad = 0;
        tiles += ndblk * d.nseg;
        dtiles += ndblk;
        elems += (uint64_t)d.nseg * d.ndiag;
        cells += (uint64_t)s.n * s.m;
    }
    if (tiles >= (1ull << 31)) return fail(GX_ERANGE, "compare: too many tiles in one launch");
    const size_t small_words = 4 + 3 * nsub;   // hdr[4], L, cnt, ovf
    const size_t slots = nsub * (size_t)c.cap;
    DevCall call(ctx);
    LcsubDesc* d_desc = nullptr;
    uint2* d_elem = nullptr;
    unsigned *d_carry = nullptr, *d_hdr = nullptr;
    uint4* d_cand = nullptr;
    GX_GET(call, d_desc, nsub);
    GX_GET(call, d_elem, elems);
    GX_GET(call, d_carry, elems);
    GX_GET(call, d_hdr, small_words);
    GX_GET(call, d_cand, slots);
    // pinned staging: [descriptors][small words], later the candidates that were written
    const size_t off_small = align_up(nsub * sizeof(LcsubDesc), 16);
    uint8_t* pin = (uint8_t*)io_pinned(ctx, off_small + small_words * sizeof(unsigned));
    if (!pin) return call.done(fail(GX_ENOMEM, "compare: pinned staging"));
    memcpy(pin, desc.data(), nsub * sizeof(LcsubDesc));
    unsigned* d_L = d_hdr + 4;
    unsigned* d_cnt = d_L + nsub;
    unsigned* d_ovf = d_cnt + nsub;
    const int cus = fill_grid_cap(ctx->device);
    const int grid_t = (int)std::min<uint64_t>(tiles, (uint64_t)cus * 8);
    const int grid_d = (int)std::min<uint64_t>(dtiles, (uint64_t)cus * 8);
    GX_TRY(call, hipMemcpyAsync(d_desc, pin, nsub * sizeof(LcsubDesc), hipMemcpyHostToDevice, st));
    GX_TRY(call, hipMemsetAsync(d_hdr, 0, small_words * sizeof(unsigned), st));
    GX_TRY(call, hipEventRecord(ctx->ev0, st));
    GX_TRY(call, launch_lcsub_run((const uint8_t*)c.chars.p, d_desc, (int)nsub, (unsigned)tiles, c.H, d_elem, grid_t, st));
    GX_TRY(call, hipEventRecord(ctx->ev1, st));
    GX_TRY(call, launch_lcsub_combine(d_desc, (int)nsub, (unsigned)dtiles, d_elem, d_carry, d_L, grid_d, st));
    GX_TRY(call, launch_lcsub_cand((const uint8_t*)c.chars.p, d_desc, (int)nsub, (unsigned)tiles, c.H, d_elem, d_carry, d_L,
                                   c.cap, (unsigned)slots, d_cnt, d_ovf, d_hdr, d_cand, grid_t, st));
    GX_TRY(call, hipMemcpyAsync(pin + off_small, d_hdr, small_words * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    GX_TRY(call, hipStreamSynchronize(st));
    const std::vector<unsigned> small((const unsigned*)(pin + off_small),
                                      (const unsigned*)(pin + off_small) + small_words);
    const unsigned* h_small = small.data();
    const size_t ncand = std::min<size_t>(h_small[0], slots);
    const uint4* h_cand = nullptr;
    if (ncand) {
        pin = (uint8_t*)io_pinned(ctx, ncand * sizeof(uint4));   // (may move: the small words were copied out)
        if (!pin) return call.done(fail(GX_ENOMEM, "compare: pinned staging"));
        GX_TRY(call, hipMemcpyAsync(pin, d_cand, ncand * sizeof(uint4), hipMemcpyDeviceToHost, st));
        GX_TRY(call, hipStreamSynchronize(st));
        h_cand = (const uint4*)pin;
    }
    double ms = 0.0;
    call.elapsed(ctx->ev0, ctx->ev1, &ms);
    c.run_ms += ms;
    c.cells += cells;
    call.done(GX_OK);   // (the stream is idle)
    // candidates by sub-problem (they arrive in no order)
    const unsigned* h_L = h_small + 4;
    const unsigned* h_ovf = h_L + 2 * nsub;
    std::vector<size_t> first(nsub + 1, 0);
    for (size_t q = 0; q < ncand; ++q)
        if (h_cand[q].x < nsub) ++first[h_cand[q].x + 1];
    for (size_t k = 0; k < nsub; ++k) first[k + 1] += first[k];
    std::vector<uint32_t> ci(first[nsub]), cj(first[nsub]);
    {
        std::vector<size_t> at(first.begin(), first.end() - 1);
        for (size_t q = 0; q < ncand; ++q) {
            const uint4 e = h_cand[q];
            if (e.x >= nsub) continue;
            ci[at[e.x]] = e.y;
            cj[at[e.x]++] = e.z;
        }
    }
    std::vector<uint32_t> is, js;
    for (size_t k = 0; k < nsub; ++k) {
        const Sub& s = subs[k];
        const uint8_t* a = c.hc + s.a_off;
        const uint8_t* b = c.hc + s.b_off;
        uint64_t i = 0, j = 0, L = h_L[k];
        ++c.n_gpu;
        if (L && (h_ovf[k] || first[k + 1] == first[k])) {
            // more candidates than the buffer holds: the host solves it whole
            // (no candidates at all for L > 0 cannot happen; the host then decides too)
            ++c.n_ovf;
            ++c.n_host;
            lcs_host(a, s.n, b, s.m, &i, &j, &L);
        } else if (L) {
            is.assign(ci.begin() + first[k], ci.begin() + first[k + 1]);
            js.assign(cj.begin() + first[k], cj.begin() + first[k + 1]);
            for (auto* v : {&is, &js}) {
                std::sort(v->begin(), v->end());
                v->erase(std::unique(v->begin(), v->end()), v->end());
            }
            if (is.back() + L > s.n || js.back() + L > s.m) return fail(GX_EHIP, "compare: candidate out of range");
            resolve(a, s.n, b, s.m, L, is, js, &i, &j);
        }
        apply(c, s, i, j, L, next);
    }
    return GX_OK;
}

// The recursion of every pair, level by level.
int run_levels(Cmp& c, std::vector<Sub> open) {
    std::vector<Sub> next, gpu;
    while (!open.empty()) {
        next.clear();
        gpu.clear();
        for (const Sub& s : open) {
            if (!s.n || !s.m) apply(c, s, 0, 0, 0, next);
            else if (!c.ctx || (uint64_t)s.n * s.m < c.host_cells) host_subtree(c, s);
            else gpu.push_back(s);
        }
        if (!gpu.empty()) {
            ++c.levels;
            // batches bounded in tile elements (12 B each on the device) and candidate slots
            const uint64_t max_elems = 192ull << 20, max_subs = std::max<uint64_t>(1, (4ull << 20) / c.cap);
            for (size_t k0 = 0; k0 < gpu.size();) {
                uint64_t elems = 0, tiles = 0;
                size_t k1 = k0;
                while (k1 < gpu.size() && k1 - k0 < max_subs) {
                    const uint64_t nd = (uint64_t)gpu[k1].n + gpu[k1].m - 1, ns = (gpu[k1].n + c.H - 1) / c.H;
                    const uint64_t tl = ns * ((nd + kLcsubBlock - 1) / kLcsubBlock);
                    if (k1 > k0 && (elems + nd * ns > max_elems || tiles + tl >= (1ull << 30))) break;
                    elems += nd * ns;
                    tiles += tl;
                    ++k1;
                }
                const int rc = gpu_batch(c, gpu.data() + k0, k1 - k0, next);
                if (rc != GX_OK) return rc;
                k0 = k1;
            }
        }
        open.swap(next);
    }
    return GX_OK;
}

// Stages seqs (host copy, and the device's when ctx), runs the pairs
// (ia[p], ib[p]) and leaves their sums in c.acc.
int compare_core(gx_context* ctx, const uint8_t* const* seqs, const size_t* lens, size_t nseq,
                 const std::vector<std::pair<size_t, size_t>>& pairs, bool recurse, Cmp& c) {
    std::vector<size_t> off(nseq);
    size_t total = kLcsubPad;
    for (size_t k = 0; k < nseq; ++k) {
        if (lens[k] >= (1ull << 30)) return fail(GX_ERANGE, "compare: sequence of 2^30 bytes or more");
        const int rc = check_bytes(seqs[k], lens[k], "sequence");
        if (rc != GX_OK) return rc;
        off[k] = total;
        total += align_up(lens[k], kLcsubPad) + kLcsubPad;
    }
    if (total >= (1ull << 32)) return fail(GX_ERANGE, "compare: 4 GiB of sequences or more");
    std::vector<uint8_t> hc(total, 0);
    for (size_t k = 0; k < nseq; ++k)
        if (lens[k]) memcpy(hc.data() + off[k], seqs[k], lens[k]);
    c.ctx = ctx;
    c.hc = hc.data();
    c.recurse = recurse;
    c.host_cells = env_u64("GX_COMPARE_HOST_CELLS", kHostCellsDefault);
    c.cap = (unsigned)std::min<uint64_t>(std::max<uint64_t>(env_u64("GX_COMPARE_CAND_CAP", kLcsubCandCap), 1), 1u << 16);
    c.H = seg_height();
    c.acc.assign(pairs.size(), PairAcc{});
    std::vector<Sub> open;
    for (size_t p = 0; p < pairs.size(); ++p) {
        const size_t ia = pairs[p].first, ib = pairs[p].second;
        open.push_back(Sub{(uint32_t)p, (uint32_t)off[ia], (uint32_t)lens[ia], (uint32_t)off[ib], (uint32_t)lens[ib], true});
    }
    if (!ctx) return run_levels(c, std::move(open));
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    int rc = pool_get(ctx, total, &c.chars, ctx->stream);
    if (rc != GX_OK) return rc;
    // (a pageable source: the copy has left `hc` when the call returns)
    hipError_t e = hipMemcpyAsync(c.chars.p, hc.data(), total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        pool_put(ctx, c.chars);
        return fail(GX_EHIP, std::string("compare: staging: ") + hipGetErrorString(e));
    }
    rc = run_levels(c, std::move(open));
    // (gpu_batch drained the stream on both its ways out: nothing reads the sequences now)
    pool_put(ctx, c.chars);
    ctx->cmp_gpu = c.n_gpu;
    ctx->cmp_host = c.n_host;
    ctx->cmp_ovf = c.n_ovf;
    ctx->cmp_levels = c.levels;
    ctx->cmp_batches = c.batches;
    ctx->cmp_cells = c.cells;
    ctx->cmp_run_ms = c.run_ms;
    return rc;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI

extern "C" int gx_compare_segment_height(void) { return seg_height(); }

extern "C" int gx_common_substring_host(const uint8_t* a, size_t n, const uint8_t* b, size_t m, uint64_t* i,
                                        uint64_t* j, uint64_t* len) {
    if (!i || !j || !len) return fail(GX_EINVAL, "output pointer is NULL");
    if (n >= (1ull << 30) || m >= (1ull << 30)) return fail(GX_ERANGE, "compare: sequence of 2^30 bytes or more");
    int rc = check_bytes(a, n, "a");
    if (rc == GX_OK) rc = check_bytes(b, m, "b");
    if (rc != GX_OK) return rc;
    lcs_host(a, n, b, m, i, j, len);
    return GX_OK;
}

extern "C" int gx_common_substring_candidates_host(const uint8_t* a, size_t n, const uint8_t* b, size_t m,
                                                   uint64_t* len, uint64_t* n_candidates) {
    if (!len || !n_candidates) return fail(GX_EINVAL, "output pointer is NULL");
    if (n >= (1ull << 30) || m >= (1ull << 30)) return fail(GX_ERANGE, "compare: sequence of 2^30 bytes or more");
    int rc = check_bytes(a, n, "a");
    if (rc == GX_OK) rc = check_bytes(b, m, "b");
    if (rc != GX_OK) return rc;
    uint64_t i, j;
    lcs_host(a, n, b, m, &i, &j, len, n_candidates);
    return GX_OK;
}

extern "C" int gx_common_substring(gx_context* ctx, const uint8_t* a, size_t n, const uint8_t* b, size_t m,
                                   uint64_t* i, uint64_t* j, uint64_t* len) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (!i || !j || !len) return fail(GX_EINVAL, "output pointer is NULL");
    const uint8_t* seqs[2] = {a, b};
    const size_t lens[2] = {n, m};
    Cmp c;
    const int rc = compare_core(ctx, seqs, lens, 2, {{0, 1}}, false, c);
    if (rc != GX_OK) return rc;
    *i = c.acc[0].ri;
    *j = c.acc[0].rj;
    *len = c.acc[0].first;
    return GX_OK;
}

extern "C" int gx_compare_pair(gx_context* ctx, const uint8_t* a, size_t n, const uint8_t* b, size_t m,
                               gx_compare_cell* out, uint64_t* n_calls) {
    if (!out) return fail(GX_EINVAL, "out is NULL");
    const uint8_t* seqs[2] = {a, b};
    const size_t lens[2] = {n, m};
    Cmp c;
    const int rc = compare_core(ctx, seqs, lens, 2, {{0, 1}}, true, c);
    if (rc != GX_OK) return rc;
    *out = gx_compare_cell{c.acc[0].score, n, m, c.acc[0].first};
    if (n_calls) *n_calls = c.acc[0].calls;
    return GX_OK;
}

extern "C" int gx_compare_matrix(gx_context* ctx, const uint8_t* const* seqs, const size_t* lens, size_t nseq,
                                 gx_compare_cell* out) {
    if (nseq && (!seqs || !lens || !out)) return fail(GX_EINVAL, "seqs, lens or out is NULL");
    std::vector<std::pair<size_t, size_t>> pairs;
    for (size_t j = 0; j < nseq; ++j)
        for (size_t i = 0; i <= j; ++i) pairs.push_back({i, j});   // main.rs:263: i > j is skipped
    Cmp c;
    const int rc = compare_core(ctx, seqs, lens, nseq, pairs, true, c);
    if (rc != GX_OK) return rc;
    for (size_t k = 0; k < nseq * nseq; ++k) out[k] = gx_compare_cell{0, 0, 0, 0};
    for (size_t p = 0; p < pairs.size(); ++p) {
        const size_t i = pairs[p].first, j = pairs[p].second;
        out[j * nseq + i] = gx_compare_cell{c.acc[p].score, lens[i], lens[j], c.acc[p].first};
    }
    return GX_OK;
}

extern "C" int gx_compare_info(const gx_context* ctx, uint64_t* gpu_subproblems, uint64_t* host_subproblems,
                               uint64_t* overflowed, uint64_t* levels) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (gpu_subproblems) *gpu_subproblems = ctx->cmp_gpu;
    if (host_subproblems) *host_subproblems = ctx->cmp_host;
    if (overflowed) *overflowed = ctx->cmp_ovf;
    if (levels) *levels = ctx->cmp_levels;
    return GX_OK;
}

extern "C" int gx_compare_batches(const gx_context* ctx, uint64_t* batches) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (batches) *batches = ctx->cmp_batches;
    return GX_OK;
}

extern "C" int gx_compare_run_stats(const gx_context* ctx, uint64_t* byte_compares, double* run_ms) {
    if (!ctx) return fail(GX_EINVAL, "ctx is NULL");
    if (byte_compares) *byte_compares = ctx->cmp_cells;
    if (run_ms) *run_ms = ctx->cmp_run_ms;
    return GX_OK;
}
