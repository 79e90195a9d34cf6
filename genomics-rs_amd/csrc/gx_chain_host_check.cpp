// gx_chain_host_check.cpp -- the host solver of the chaining (gx_chain_anchors
// with ctx = NULL) as a stand-alone program for the host
// sanitizers (`make chain_host_check`: the host objects built with
// -fsanitize=address,undefined, the kernels' objects linked as they are; no
// device is touched).  Random anchor sets and the edge shapes -- empty batch,
// empty queries, one anchor, long diagonals, look-backs of 1 and 256, anchors
// sharing a qpos, positions next to 2^32 -- with result arrays of exactly the
// size needed, every result against the quadratic loop written out here; exit
// status 0 when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/gx.h"

namespace {

typedef std::vector<gx_mem> Query;

int failures = 0;

void expect(bool ok, const char* what, size_t c, size_t k) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "FAIL %s: query %zu item %zu\n", what, c, k);
}

// The contract on one query, in 64 bits: every a < b is looked at.
struct Want {
    std::vector<int64_t> f;
    std::vector<uint32_t> pred;
    std::vector<gx_chain> chains;           // member_off within the query
    std::vector<uint32_t> members;
};

Want solve(const Query& q, const gx_chain_params& p) {
    const size_t n = q.size();
    Want w;
    w.f.resize(n);
    w.pred.assign(n, GX_CHAIN_NONE);
    std::vector<uint32_t> root(n);
    for (size_t b = 0; b < n; ++b) {
        const int64_t own = (int64_t)p.w_match * q[b].len;
        int64_t best = own;
        uint32_t pr = GX_CHAIN_NONE;
        for (size_t a = 0; a < b; ++a) {   // ascending: of equal ext the last, the nearest, stays
            if (b - a > p.max_pred) continue;
            const int64_t dq = (int64_t)q[b].qpos - q[a].qpos, dt = (int64_t)q[b].tpos - q[a].tpos;
            const int64_t drift = dq > dt ? dq - dt : dt - dq;
            if (dq < 1 || dq > p.max_gap || dt < 1 || dt > p.max_gap || drift > p.max_drift) continue;
            const int64_t ext = w.f[a] + p.w_match * std::min<int64_t>(q[b].len, std::min(dq, dt)) - p.w_drift * drift;
            if (ext > own && ext >= best) {
                best = ext;
                pr = (uint32_t)a;
            }
        }
        w.f[b] = best;
        w.pred[b] = pr;
        root[b] = pr == GX_CHAIN_NONE ? (uint32_t)b : root[pr];
    }
    for (size_t r = 0; r < n; ++r) {
        if (w.pred[r] != GX_CHAIN_NONE) continue;
        size_t e = r;
        for (size_t x = r; x < n; ++x)
            if (root[x] == r && w.f[x] > w.f[e]) e = x;
        if (w.f[e] < p.min_score) continue;
        std::vector<uint32_t> path;
        for (uint32_t x = (uint32_t)e;; x = w.pred[x]) {
            path.push_back(x);
            if (w.pred[x] == GX_CHAIN_NONE) break;
        }
        std::reverse(path.begin(), path.end());
        gx_chain c{};
        c.member_off = w.members.size();
        c.score = (int32_t)w.f[e];
        c.n_anchors = (uint32_t)path.size();
        c.root = (uint32_t)r;
        c.end = (uint32_t)e;
        c.qstart = q[r].qpos;
        c.tstart = q[r].tpos;
        c.qend = q[e].qpos + q[e].len;
        c.tend = q[e].tpos + q[e].len;
        w.chains.push_back(c);
        w.members.insert(w.members.end(), path.begin(), path.end());
    }
    return w;
}

void check(const std::vector<Query>& queries, const gx_chain_params& p) {
    const size_t nq = queries.size();
    std::vector<gx_mem> an;
    std::vector<uint64_t> off(1, 0);
    for (const Query& q : queries) {
        an.insert(an.end(), q.begin(), q.end());
        off.push_back(an.size());
    }
    // exactly what is needed, no entry of padding: a read or a write past it is the sanitizer's to find
    std::vector<int32_t> f(an.size());
    std::vector<uint32_t> pred(an.size());
    std::vector<uint64_t> coff(nq + 1);
    uint64_t mtot = ~0ull;
    int rc = gx_chain_anchors(nullptr, an.data(), off.data(), nq, &p, f.data(), pred.data(), nullptr, 0, nullptr, 0, coff.data(), &mtot);
    std::vector<gx_chain> chains(rc == GX_OK ? coff[nq] : 0);
    std::vector<uint32_t> members(rc == GX_OK ? mtot : 0);
    if (rc == GX_OK)
        rc = gx_chain_anchors(nullptr, an.data(), off.data(), nq, &p, nullptr, nullptr, chains.data(), chains.size(),
                              members.data(), members.size(), coff.data(), &mtot);
    if (rc != GX_OK) {
        ++failures;
        fprintf(stderr, "FAIL rc %d: %s\n", rc, gx_last_error());
        return;
    }
    uint64_t moff = 0;
    for (size_t c = 0; c < nq; ++c) {
        const Want w = solve(queries[c], p);
        for (size_t b = 0; b < queries[c].size(); ++b) {
            expect(f[off[c] + b] == w.f[b], "f", c, b);
            expect(pred[off[c] + b] == w.pred[b], "pred", c, b);
        }
        expect(coff[c + 1] - coff[c] == w.chains.size(), "chain count", c, 0);
        if (coff[c + 1] - coff[c] != w.chains.size()) return;
        for (size_t k = 0; k < w.chains.size(); ++k) {
            const gx_chain &g = chains[coff[c] + k], &x = w.chains[k];
            expect(g.member_off == moff + x.member_off && g.score == x.score && g.n_anchors == x.n_anchors && g.root == x.root &&
                       g.end == x.end && g.qstart == x.qstart && g.tstart == x.tstart && g.qend == x.qend && g.tend == x.tend,
                   "chain", c, k);
        }
        expect(moff + w.members.size() <= members.size(), "members total", c, 0);
        if (moff + w.members.size() > members.size()) return;
        for (size_t k = 0; k < w.members.size(); ++k) expect(members[moff + k] == w.members[k], "member", c, k);
        moff += w.members.size();
    }
    expect(moff == mtot && moff == members.size(), "members_total", nq, 0);
}

Query random_query(std::mt19937& rng, size_t n, uint32_t span, uint32_t base, bool repeats) {
    std::vector<std::pair<uint32_t, uint32_t>> pts;
    while (pts.size() < n) {
        const uint32_t q = base + rng() % span;
        for (int r = repeats ? 1 + rng() % 4 : 1; r > 0; --r) pts.emplace_back(q, base + rng() % span);
    }
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    Query out;
    for (const auto& pt : pts) out.push_back(gx_mem{pt.first, pt.second, 1 + (uint32_t)(rng() % 30)});
    return out;
}

Query diagonal(size_t n, uint32_t step, uint32_t len) {
    Query q;
    for (size_t i = 0; i < n; ++i) q.push_back(gx_mem{(uint32_t)(step * i), (uint32_t)(step * i + 3), len});
    return q;
}

}  // namespace

int main() {
    std::mt19937 rng(23);
    const gx_chain_params defaults{GX_CHAIN_DEFAULT_W_MATCH,  GX_CHAIN_DEFAULT_W_DRIFT,  GX_CHAIN_DEFAULT_MAX_GAP,
                                   GX_CHAIN_DEFAULT_MAX_DRIFT, GX_CHAIN_DEFAULT_MAX_PRED, GX_CHAIN_DEFAULT_MIN_SCORE};
    // the edge shapes
    check({}, defaults);
    check({Query(), Query()}, defaults);
    check({Query(), diagonal(1, 10, 7), Query(), diagonal(2, 10, 7), diagonal(1000, 10, 7), Query()}, defaults);
    for (uint32_t H : {1u, 2u, 64u, 255u, 256u}) {
        gx_chain_params p = defaults;
        p.max_pred = H;
        check({diagonal(300, 10, 7), diagonal(H, 5, 9), diagonal(H + 1, 5, 9)}, p);
    }
    {   // positions next to 2^32: qpos + len = tpos + len = 2^32 - 1 at the last anchor
        const uint32_t top = 0xFFFFFFFFu;
        Query q = {gx_mem{top - 400, top - 420, 30}, gx_mem{top - 300, top - 310, 50}, gx_mem{top - 300, top - 200, 5},
                   gx_mem{top - 100, top - 100, 100}};
        check({q}, defaults);
        Query far = {gx_mem{0, top - 5, 4}, gx_mem{1, 0, 4}, gx_mem{2, top - 3, 2}};   // dt of almost -2^32 and +2^32
        check({far}, defaults);
    }
    // random anchor sets
    for (int round = 0; round < 60; ++round) {
        gx_chain_params p = defaults;
        p.w_match = 1 + rng() % 12;
        p.w_drift = rng() % 4;
        p.max_pred = round % 5 == 0 ? 256 : 1 + rng() % 130;
        const uint32_t span = 40 + rng() % 1500;
        p.max_gap = 1 + rng() % span;
        p.max_drift = rng() % (span / 2);
        p.min_score = round % 3 == 0 ? (int32_t)(rng() % 400) : 0;
        std::vector<Query> queries;
        for (int c = 0, nq = 1 + rng() % 6; c < nq; ++c)
            queries.push_back(rng() % 5 == 0 ? Query() : random_query(rng, 1 + rng() % 400, span, rng() % 1000, round % 2 == 1));
        check(queries, p);
    }
    printf(failures ? "chain_host_check: %d FAILED\n" : "chain_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
