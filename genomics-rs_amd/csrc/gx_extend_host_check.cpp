// gx_extend_host_check.cpp -- the host index of gx_suffix_index_extend
// (ctx = NULL) as a stand-alone program for the host sanitizers
// (`make extend_host_check`: the host objects built with
// -fsanitize=address,undefined, the kernels' objects linked as they are; no
// device is touched).  Hits of the host edit search and windows of its own at
// every band width and at the text's edges, every record and every run against
// the banded recurrence and retrace written out here on a full table in 64
// bits, the CIGAR array allocated at exactly the total so that a write past it
// is the sanitizer's to find; exit status 0 when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/gx.h"

namespace {

typedef std::vector<uint8_t> Bytes;

struct Want {
    gx_extend_hit rec;
    std::vector<uint32_t> runs;   // pattern order
};

// s1 = t (index i), s2 = P (index j), the cells with |j - i| <= B.
Want banded(const Bytes& t, const Bytes& P, const gx_scores& sc, int64_t B) {
    const int64_t w = (int64_t)t.size(), m = (int64_t)P.size(), NEG = -(1ll << 40);
    struct Cell { int64_t S, I, D; };
    std::vector<Cell> tab((size_t)((w + 1) * (m + 1)), Cell{NEG, NEG, NEG});
    auto at = [&](int64_t i, int64_t j) -> Cell {
        if (i < 0 || j < 0 || std::llabs(j - i) > B) return Cell{NEG, NEG, NEG};
        return tab[(size_t)(i * (m + 1) + j)];
    };
    auto mx = [](const Cell& c) { return std::max({c.S, c.I, c.D}); };
    for (int64_t i = 0; i <= w; ++i)
        for (int64_t j = 0; j <= m; ++j) {
            if (std::llabs(j - i) > B) continue;
            Cell c{NEG, NEG, NEG};
            if (i == 0 && j == 0) c = Cell{0, 0, 0};
            else if (j == 0) c.D = sc.h + i * sc.g;
            else if (i == 0) c.I = sc.h + j * sc.g;
            else {
                const Cell top = at(i, j - 1), left = at(i - 1, j), tl = at(i - 1, j - 1);
                c.I = std::max({top.I + sc.g, top.S + sc.h + sc.g, top.D + sc.h + sc.g});
                c.D = std::max({left.I + sc.h + sc.g, left.S + sc.h + sc.g, left.D + sc.g});
                c.S = (t[i - 1] == P[j - 1] ? sc.s_match : sc.s_mismatch) + mx(tl);
            }
            tab[(size_t)(i * (m + 1) + j)] = c;
        }
    Want r{};
    r.rec.score = (int32_t)mx(at(w, m));
    int64_t i = w, j = m;
    int last = 0, op = -1;
    uint32_t len = 0;
    std::vector<uint32_t> rev;
    for (;;) {
        const Cell c = at(i, j);
        const int64_t M = mx(c);
        const int pick = c.S == M ? 0 : c.I == M ? 1 : 2;
        if (pick == 0) {
            const bool a = i < w, b = j < m;
            if (a == b && (!a || t[i] == P[j])) ++r.rec.matches; else ++r.rec.mismatches;
            if (i && j && t[i - 1] == P[j - 1]) ++r.rec.identities;
        } else if (pick == last) {
            ++r.rec.gap_extensions;
        } else {
            ++r.rec.opening_gaps;
        }
        last = pick;
        ++r.rec.n_steps;
        if (pick == op) ++len;
        else {
            if (len) rev.push_back(len << 4 | (uint32_t)op);
            op = pick;
            len = 1;
        }
        if (pick != 1 && i) --i;
        if (pick != 2 && j) --j;
        if ((i == 0 && j == 0) || r.rec.n_steps > (uint64_t)(w + m)) break;
    }
    if (len) rev.push_back(len << 4 | (uint32_t)op);
    r.runs.assign(rev.rbegin(), rev.rend());
    r.rec.cigar_len = (uint32_t)r.runs.size();
    return r;
}

int failures = 0;

// Every hit of every pattern on the host index against banded().
void check(gx_suffix_index* idx, const Bytes& s, const std::vector<Bytes>& pats, const std::vector<uint64_t>& hoff,
           const std::vector<uint32_t>& starts, const std::vector<uint32_t>& ends, const gx_scores& sc, uint32_t B) {
    Bytes packed;
    std::vector<uint64_t> off(1, 0);
    for (const Bytes& P : pats) {
        packed.insert(packed.end(), P.begin(), P.end());
        off.push_back(packed.size());
    }
    if (packed.empty()) packed.push_back(0);
    const size_t npat = pats.size(), nhits = (size_t)hoff[npat];
    std::vector<gx_extend_hit> out(nhits + 1);
    std::vector<uint64_t> coff(nhits + 1);
    int rc = gx_suffix_index_extend(idx, packed.data(), off.data(), npat, hoff.data(), starts.data(), ends.data(), &sc, B,
                                    out.data(), nullptr, 0, coff.data());
    std::vector<uint32_t> cig((size_t)coff[nhits] + 1);
    if (rc == GX_OK)
        rc = gx_suffix_index_extend(idx, packed.data(), off.data(), npat, hoff.data(), starts.data(), ends.data(), &sc, B,
                                    out.data(), cig.data(), cig.size() - 1, coff.data());
    if (rc != GX_OK) {
        ++failures;
        fprintf(stderr, "FAIL rc %d: %s\n", rc, gx_last_error());
        return;
    }
    for (size_t p = 0; p < npat; ++p)
        for (uint64_t h = hoff[p]; h < hoff[p + 1]; ++h) {
            const Want want = banded(Bytes(s.begin() + starts[h], s.begin() + ends[h]), pats[p], sc, B);
            const bool rec_ok = memcmp(&out[h], &want.rec, sizeof(gx_extend_hit)) == 0;
            const bool runs_ok = coff[h + 1] - coff[h] == want.runs.size() &&
                                 std::equal(want.runs.begin(), want.runs.end(), cig.begin() + coff[h]);
            if (rec_ok && runs_ok) continue;
            ++failures;
            fprintf(stderr, "FAIL %s: hit %llu, w %u m %zu B %u\n", rec_ok ? "runs" : "record", (unsigned long long)h,
                    ends[h] - starts[h], pats[p].size(), B);
        }
}

}  // namespace

int main() {
    std::mt19937 rng(22);
    const gx_scores score_sets[] = {{1, -2, -1, -5}, {2, -1, -1, 0}, {0, -1, -3, -1}, {5, -4, -2, -10},
                                    {GX_EXTEND_MAX_SCORE, -GX_EXTEND_MAX_SCORE, -GX_EXTEND_MAX_SCORE, -GX_EXTEND_MAX_SCORE}};
    const char* alphabets[] = {"A", "AC", "ACGT"};
    for (int round = 0; round < 45; ++round) {
        const char* alpha = alphabets[round % 3];
        const size_t na = strlen(alpha), n = 40 + rng() % 160;
        const gx_scores& sc = score_sets[round % 5];
        Bytes s(n);
        for (auto& c : s) c = (uint8_t)alpha[rng() % na];
        gx_suffix_index* idx = nullptr;
        if (gx_suffix_index_build(nullptr, s.data(), n, &idx) != GX_OK) return 2;
        // the edit search's own hits at B = k and k + 2
        for (uint32_t k : {0u, 1u, 3u, 8u}) {
            std::vector<Bytes> pats;
            for (size_t m : {(size_t)k + 1, (size_t)17, (size_t)33}) {
                const size_t i = rng() % (n - m + 1);
                Bytes P(s.begin() + i, s.begin() + i + m);
                for (uint32_t e = 0; e < k && P.size() > k + 1; ++e) {
                    const size_t c = rng() % P.size();
                    if (e % 3 == 0) P[c] = (uint8_t)(P[c] == 'A' ? 'C' : 'A');
                    else if (e % 3 == 1) P.insert(P.begin() + c, (uint8_t)'G');
                    else P.erase(P.begin() + c);
                }
                pats.push_back(P);
            }
            Bytes packed;
            std::vector<uint64_t> off(1, 0);
            for (const Bytes& P : pats) {
                packed.insert(packed.end(), P.begin(), P.end());
                off.push_back(packed.size());
            }
            std::vector<gx_edit_hit> hits(pats.size());
            std::vector<uint64_t> hoff(pats.size() + 1);
            const size_t cap = pats.size() * 8;
            std::vector<uint32_t> ends(cap), starts(cap);
            Bytes dist(cap);
            if (gx_suffix_index_search_edit(idx, packed.data(), off.data(), pats.size(), k, hits.data(), 8, ends.data(),
                                            dist.data(), starts.data(), cap, hoff.data()) != GX_OK)
                return 2;
            check(idx, s, pats, hoff, starts, ends, sc, k);
            check(idx, s, pats, hoff, starts, ends, sc, std::min(k + 2, (uint32_t)GX_EXTEND_MAX_BAND));
        }
        // windows of its own at both ends of every width: unrelated pairs, w - m in {-B, 0, B}, the text's edges
        for (uint32_t B : {0u, 1u, 2u, 3u, 4u, 5u, 8u, 9u, 15u}) {
            std::vector<Bytes> pats;
            std::vector<uint64_t> hoff(1, 0);
            std::vector<uint32_t> starts, ends;
            for (size_t m : {(size_t)1, (size_t)B + 1, (size_t)31}) {
                Bytes P(m);
                for (auto& c : P) c = (uint8_t)alpha[rng() % na];
                pats.push_back(P);
                for (int d : {-(int)B, 0, (int)B}) {
                    const int64_t w = (int64_t)m + d;
                    if (w < 0 || (size_t)w > n) continue;
                    for (size_t b : {(size_t)0, (size_t)(rng() % (n - w + 1)), n - (size_t)w}) {
                        starts.push_back((uint32_t)b);
                        ends.push_back((uint32_t)(b + w));
                    }
                }
                hoff.push_back(starts.size());
            }
            check(idx, s, pats, hoff, starts, ends, sc, B);
        }
        gx_suffix_index_free(idx);
    }
    // the longest pattern at the widest band and the score limit
    Bytes s(5000);
    for (auto& c : s) c = (uint8_t)"ACGT"[rng() % 4];
    gx_suffix_index* idx = nullptr;
    if (gx_suffix_index_build(nullptr, s.data(), s.size(), &idx) != GX_OK) return 2;
    Bytes P(s.begin() + 300, s.begin() + 300 + GX_EDIT_MAX_M);
    P[9] = 'N';
    P.erase(P.begin() + 1500);
    P.push_back('A');
    check(idx, s, {P}, {0, 3}, {300, 290, 300}, {300 + GX_EDIT_MAX_M, 290 + GX_EDIT_MAX_M + 15, 300 + GX_EDIT_MAX_M - 15},
          score_sets[4], GX_EXTEND_MAX_BAND);
    gx_suffix_index_free(idx);
    printf(failures ? "extend_host_check: %d FAILED\n" : "extend_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
