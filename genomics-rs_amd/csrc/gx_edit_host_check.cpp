// gx_edit_host_check.cpp -- the host index of the edit search (ctx = NULL,
// DESIGN.md 20) as a stand-alone program for the host sanitizers
// (`make edit_host_check`: the host objects built with
// -fsanitize=address,undefined, the kernels' objects linked as they are; no
// device is touched).  Random texts over one, two and four letters and the
// shapes at the text's edges, every result against Sellers' recurrence and
// plain Levenshtein written out here; exit status 0 when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/gx.h"

namespace {

typedef std::vector<uint8_t> Bytes;

// E(e) for e = 0 .. n.
std::vector<uint32_t> sellers(const Bytes& s, const Bytes& P) {
    const size_t n = s.size(), m = P.size();
    std::vector<uint32_t> col(m + 1), E(n + 1);
    for (size_t i = 0; i <= m; ++i) col[i] = (uint32_t)i;
    E[0] = col[m];
    for (size_t c = 1; c <= n; ++c) {
        uint32_t diag = col[0];   // D[i - 1][c - 1]
        col[0] = 0;
        for (size_t i = 1; i <= m; ++i) {
            const uint32_t up = col[i - 1], left = col[i];
            col[i] = std::min({diag + (P[i - 1] != s[c - 1] ? 1u : 0u), up + 1, left + 1});
            diag = left;
        }
        E[c] = col[m];
    }
    return E;
}

uint32_t lev(const uint8_t* a, size_t la, const uint8_t* b, size_t lb) {
    std::vector<uint32_t> prev(lb + 1), cur(lb + 1);
    for (size_t j = 0; j <= lb; ++j) prev[j] = (uint32_t)j;
    for (size_t i = 1; i <= la; ++i) {
        cur[0] = (uint32_t)i;
        for (size_t j = 1; j <= lb; ++j)
            cur[j] = std::min({prev[j - 1] + (a[i - 1] != b[j - 1] ? 1u : 0u), prev[j] + 1, cur[j - 1] + 1});
        prev.swap(cur);
    }
    return prev[lb];
}

int failures = 0;

void expect(bool ok, const char* what, const Bytes& s, const Bytes& P, uint32_t k) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "FAIL %s: n %zu m %zu k %u\n", what, s.size(), P.size(), k);
}

void check(gx_suffix_index* idx, const Bytes& s, const std::vector<Bytes>& pats, uint32_t k, uint32_t max_hits) {
    Bytes packed;
    std::vector<uint64_t> off(1, 0);
    for (const Bytes& P : pats) {
        packed.insert(packed.end(), P.begin(), P.end());
        off.push_back(packed.size());
    }
    const size_t npat = pats.size();
    std::vector<gx_edit_hit> hits(npat);
    std::vector<uint64_t> hoff(npat + 1);
    std::vector<uint32_t> ends(1), starts(1);
    Bytes dist(1);
    int rc = gx_suffix_index_search_edit(idx, packed.data(), off.data(), npat, k, hits.data(), max_hits, ends.data(),
                                         dist.data(), starts.data(), 0, hoff.data());
    if (rc == GX_ECAP) {   // allocate exactly what is needed and repeat: a write past it is the sanitizer's to find
        ends.assign(hoff[npat], 0);
        starts.assign(hoff[npat], 0);
        dist.assign(hoff[npat], 0);
        rc = gx_suffix_index_search_edit(idx, packed.data(), off.data(), npat, k, hits.data(), max_hits, ends.data(),
                                         dist.data(), starts.data(), ends.size(), hoff.data());
    }
    if (rc != GX_OK) {
        ++failures;
        fprintf(stderr, "FAIL rc %d: %s\n", rc, gx_last_error());
        return;
    }
    for (size_t p = 0; p < npat; ++p) {
        const Bytes& P = pats[p];
        const std::vector<uint32_t> E = sellers(s, P);
        std::vector<uint32_t> occ;
        uint32_t best = 0xFFFFFFFFu, bend = 0;
        for (uint32_t e = 0; e < E.size(); ++e)
            if (E[e] <= k) {
                occ.push_back(e);
                if (E[e] < best) { best = E[e]; bend = e; }
            }
        expect(hits[p].count == occ.size() && hits[p].best_dist == best && hits[p].best_end == bend, "hit", s, P, k);
        const size_t q = std::min<size_t>(occ.size(), max_hits);
        expect(hoff[p + 1] - hoff[p] == q, "offsets", s, P, k);
        for (size_t r = 0; r < q && hoff[p + 1] - hoff[p] == q; ++r) {
            const uint64_t o = hoff[p] + r;
            const uint32_t e = occ[r];
            expect(ends[o] == e && dist[o] == E[e], "occurrence", s, P, k);
            if (P.size() > 64) {   // (the quadratic check below is for the short patterns; the window must still be a legal one)
                expect(starts[o] <= e && e - starts[o] + k >= P.size() && e - starts[o] <= P.size() + k, "start range", s, P, k);
                continue;
            }
            uint32_t b = e;   // the largest b with ed(P, s[b .. e)) = E(e)
            while (lev(P.data(), P.size(), s.data() + b, e - b) != E[e] && b > 0) --b;
            expect(starts[o] == b, "start", s, P, k);
        }
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20);
    const char* alphabets[] = {"A", "AC", "ACGT"};
    for (int round = 0; round < 60; ++round) {
        const char* alpha = alphabets[round % 3];
        const size_t na = strlen(alpha), n = 1 + rng() % 120;
        Bytes s(n);
        for (auto& c : s) c = (uint8_t)alpha[rng() % na];
        gx_suffix_index* idx = nullptr;
        if (gx_suffix_index_build(nullptr, s.data(), n, &idx) != GX_OK) return 2;
        for (uint32_t k = 0; k <= 8; k += (k < 3 ? 1 : 5)) {
            std::vector<Bytes> pats;
            for (size_t m : {(size_t)k + 1, (size_t)9, (size_t)17, (size_t)33}) {
                if (m < k + 1 || m > n) continue;
                for (size_t i : {(size_t)0, (size_t)(rng() % (n - m + 1)), n - m}) {
                    Bytes P(s.begin() + i, s.begin() + i + m);
                    pats.push_back(P);
                    for (uint32_t e = 0; e < k && P.size() > k + 1; ++e) {   // an edit: substitution, insertion, deletion in turn
                        const size_t c = rng() % P.size();
                        if (e % 3 == 0) P[c] = (uint8_t)(P[c] == 'A' ? 'C' : 'A');
                        else if (e % 3 == 1) P.insert(P.begin() + c, (uint8_t)'G');
                        else P.erase(P.begin() + c);
                    }
                    pats.push_back(P);
                    Bytes front(P), back(P);   // bytes the text does not have in front of position 0 and behind n
                    front.insert(front.begin(), (uint8_t)'T');
                    back.push_back((uint8_t)'T');
                    pats.push_back(front);
                    pats.push_back(back);
                }
            }
            if (pats.empty()) continue;
            check(idx, s, pats, k, 0xFFFFFFFFu);
            check(idx, s, pats, k, 2);
        }
        gx_suffix_index_free(idx);
    }
    // the longest pattern at the widest band
    Bytes s(5000);
    for (auto& c : s) c = (uint8_t)"ACGT"[rng() % 4];
    gx_suffix_index* idx = nullptr;
    if (gx_suffix_index_build(nullptr, s.data(), s.size(), &idx) != GX_OK) return 2;
    Bytes P(s.begin() + 900, s.begin() + 900 + GX_EDIT_MAX_M);
    P[7] = 'N';
    P.erase(P.begin() + 2000);
    P.push_back('A');
    check(idx, s, {P, Bytes(s.begin(), s.begin() + GX_EDIT_MAX_M), Bytes(s.end() - GX_EDIT_MAX_M, s.end())}, 8, 0xFFFFFFFFu);
    gx_suffix_index_free(idx);
    printf(failures ? "edit_host_check: %d FAILED\n" : "edit_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
