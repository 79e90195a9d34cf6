// gx_match_host_check.cpp -- the host index of matching statistics and MEMs
// (ctx = NULL) as a stand-alone program for the host sanitizers
// (`make match_host_check`: the host objects built with
// -fsanitize=address,undefined, the kernels' objects linked as they are; no
// device is touched).  A handful of texts and queries -- empty query, one byte,
// query = text, unary, queries ending at word edges -- every result against the
// quadratic loop written out here; exit status 0 when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/gx.h"

namespace {

typedef std::vector<uint8_t> Bytes;

int failures = 0;

void expect(bool ok, const char* what, size_t n, size_t c, size_t j, uint32_t L) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "FAIL %s: n %zu query %zu position %zu L %u\n", what, n, c, j, L);
}

// lcp(s[i ..), q[j ..))
uint32_t run(const Bytes& s, const Bytes& q, size_t i, size_t j) {
    uint32_t k = 0;
    while (i + k < s.size() && j + k < q.size() && s[i + k] == q[j + k]) ++k;
    return k;
}

void check(gx_suffix_index* idx, const Bytes& s, const std::vector<Bytes>& queries, uint32_t L, uint32_t W) {
    const size_t n = s.size(), N = n + 1, nq = queries.size();
    Bytes packed;
    std::vector<uint64_t> off(1, 0);
    for (const Bytes& q : queries) {
        packed.insert(packed.end(), q.begin(), q.end());
        off.push_back(packed.size());
    }
    // exactly what is needed, no byte of padding: a read or a write past it is the sanitizer's to find
    std::vector<uint32_t> sa(N);
    std::vector<gx_match_stat> st(packed.size());
    std::vector<uint64_t> moff(nq + 1), cand(nq);
    int rc = gx_suffix_index_export(idx, sa.data());
    if (rc == GX_OK) rc = gx_suffix_index_match_stats(idx, packed.data(), off.data(), nq, W, st.data());
    if (rc == GX_OK) rc = gx_suffix_index_mems(idx, packed.data(), off.data(), nq, L, nullptr, 0, moff.data(), cand.data());
    std::vector<gx_mem> mems(rc == GX_OK ? moff[nq] : 0);
    if (rc == GX_OK && !mems.empty())
        rc = gx_suffix_index_mems(idx, packed.data(), off.data(), nq, L, mems.data(), mems.size(), moff.data(), cand.data());
    if (rc != GX_OK) {
        ++failures;
        fprintf(stderr, "FAIL rc %d: %s\n", rc, gx_last_error());
        return;
    }
    for (size_t c = 0; c < nq; ++c) {
        const Bytes& q = queries[c];
        std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> want;   // (qpos, tpos, len), in the order of the contract
        uint64_t pairs = 0;
        for (size_t j = 0; j < q.size(); ++j) {
            uint32_t best = 0;
            std::vector<uint32_t> at;
            for (size_t i = 0; i < n; ++i) {
                const uint32_t r = run(s, q, i, j), rc_ = std::min(r, W);
                if (rc_ > best) { best = rc_; at.clear(); }
                if (rc_ == best && best) at.push_back((uint32_t)i);
                if (r >= L) {
                    ++pairs;
                    if (i == 0 || j == 0 || s[i - 1] != q[j - 1]) want.emplace_back((uint32_t)j, (uint32_t)i, r);
                }
            }
            const gx_match_stat& m = st[off[c] + j];
            expect(m.len == best, "len", n, c, j, W);
            if (!best) {
                expect(m.lo == 0 && m.count == N && m.pos == n, "len 0", n, c, j, W);
                continue;
            }
            expect(m.count == at.size() && (uint64_t)m.lo + m.count <= N && m.pos == sa[m.lo], "interval", n, c, j, W);
            if (m.count == at.size() && (uint64_t)m.lo + m.count <= N) {
                std::vector<uint32_t> got(sa.begin() + m.lo, sa.begin() + m.lo + m.count);
                std::sort(got.begin(), got.end());
                expect(got == at, "positions", n, c, j, W);
            }
        }
        expect(cand[c] == pairs, "candidates", n, c, 0, L);
        expect(moff[c + 1] - moff[c] == want.size(), "mem count", n, c, 0, L);
        for (size_t k = 0; k < want.size() && moff[c + 1] - moff[c] == want.size(); ++k) {
            const gx_mem& g = mems[moff[c] + k];
            expect(std::make_tuple(g.qpos, g.tpos, g.len) == want[k], "mem", n, c, k, L);
        }
    }
}

Bytes bytes_of(const char* z) { return Bytes(z, z + strlen(z)); }

}  // namespace

int main() {
    std::mt19937 rng(21);
    const char* alphabets[] = {"A", "AC", "ACGT"};
    for (int round = 0; round < 45; ++round) {
        const char* alpha = alphabets[round % 3];
        const size_t na = strlen(alpha), n = round < 3 ? (size_t)round : 1 + rng() % 150;
        Bytes s(n);
        for (auto& c : s) c = (uint8_t)alpha[rng() % na];
        gx_suffix_index* idx = nullptr;
        if (gx_suffix_index_build(nullptr, s.data(), n, &idx) != GX_OK) return 2;
        std::vector<Bytes> queries = {Bytes(), bytes_of("A"), s, bytes_of("N")};
        // queries ending at word edges: cut from the text, and the last with no byte behind it in the batch
        for (size_t m : {(size_t)7, (size_t)8, (size_t)9, (size_t)15, (size_t)16, (size_t)17, (size_t)24}) {
            if (m > n) continue;
            const size_t i = rng() % (n - m + 1);
            Bytes q(s.begin() + i, s.begin() + i + m);
            queries.push_back(q);
            q[m / 2] = (uint8_t)(q[m / 2] == 'A' ? 'C' : 'A');
            queries.push_back(q);
        }
        Bytes twice(s);
        twice.insert(twice.end(), s.begin(), s.end());
        queries.push_back(twice);   // longer than the text
        for (uint32_t L : {1u, 2u, 8u, 9u})
            for (uint32_t W : {1u, 8u, 9u, 1000u}) check(idx, s, queries, L, W);
        check(idx, s, {}, 1, 1);
        check(idx, s, {Bytes(), Bytes()}, 3, 3);
        gx_suffix_index_free(idx);
    }
    // unary: every pair is a candidate
    Bytes s(600, (uint8_t)'A');
    gx_suffix_index* idx = nullptr;
    if (gx_suffix_index_build(nullptr, s.data(), s.size(), &idx) != GX_OK) return 2;
    check(idx, s, {Bytes(20, 'A'), bytes_of("AAAAAAAAAAAAAAAAAAAC"), bytes_of("CAAAAAAAAAAAAAAAAAAA"), s}, 5, 16);
    gx_suffix_index_free(idx);
    printf(failures ? "match_host_check: %d FAILED\n" : "match_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
