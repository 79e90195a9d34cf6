// gx_strand_host_check.cpp -- the host side of both strands as a
// stand-alone program for the host sanitizers (`make strand_host_check`: the
// host objects built with -fsanitize=address,undefined, the kernels' objects
// linked as they are; no device is touched).  gx_revcomp, the host
// gx_revcomp_batch and every _strands call on a host index (ctx = NULL), over
// the edge batch of the device tests: every length of kLengths behind fillers
// of 0 to 7 bytes, no item, one empty item, empty items only, one item of
// 65,535 and one of 70,001 bytes.  Every output array has exactly the entries
// the call may write, so a read or a write past one is the sanitizer's to find;
// every result is held against the call without the suffix on the item batch
// built by the loops written out here.  Exit status 0 when all agree.
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

int failures = 0;

void expect(bool ok, const char* what, const char* batch, uint32_t strands) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "FAIL %s: batch %s strands %u: %s\n", what, batch, strands, gx_last_error());
}

// the table from its definition, not from the library's header
uint8_t comp(uint8_t x) {
    static const char* pairs = "ATCGRYKMBVDH";
    for (int k = 0; k < 12; ++k) {
        if (x == (uint8_t)pairs[k]) return (uint8_t)pairs[k ^ 1];
        if (x == (uint8_t)(pairs[k] + 32)) return (uint8_t)(pairs[k ^ 1] + 32);
    }
    return x;
}

Bytes rc(const Bytes& p) {
    Bytes o(p.size());
    for (size_t j = 0; j < p.size(); ++j) o[j] = comp(p[p.size() - 1 - j]);
    return o;
}

std::vector<Bytes> items_of(const std::vector<Bytes>& pats, uint32_t strands) {
    std::vector<Bytes> o;
    if (strands & GX_STRAND_FWD) o = pats;
    if (strands & GX_STRAND_REV)
        for (const Bytes& p : pats) o.push_back(rc(p));
    return o;
}

struct Packed {
    Bytes bytes;
    std::vector<uint64_t> off;
    explicit Packed(const std::vector<Bytes>& v) : off(1, 0) {
        for (const Bytes& p : v) {
            bytes.insert(bytes.end(), p.begin(), p.end());
            off.push_back(bytes.size());
        }
    }
    size_t n() const { return off.size() - 1; }
};

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

void check_revcomp(const char* name, const std::vector<Bytes>& pats) {
    for (const Bytes& p : pats) {
        Bytes got(p.size());
        expect(gx_revcomp(p.data(), p.size(), got.data()) == GX_OK && got == rc(p), "gx_revcomp", name, 0);
    }
    const Packed in(pats);
    for (uint32_t strands = 1; strands <= 3; ++strands) {
        const Packed want(items_of(pats, strands));
        std::vector<uint64_t> off(want.n() + 1, 0xDEAD);
        Bytes out(want.bytes.size());
        int rc_ = gx_revcomp_batch(nullptr, in.bytes.data(), in.off.data(), in.n(), strands, out.data(), out.size(), off.data());
        expect(rc_ == GX_OK && out == want.bytes && off == want.off, "gx_revcomp_batch", name, strands);
        Bytes padded(want.bytes.size() + GX_STRAND_PAD, 0xEE);
        rc_ = gx_revcomp_batch(nullptr, in.bytes.data(), in.off.data(), in.n(), strands, padded.data(), padded.size(), off.data());
        expect(rc_ == GX_OK && std::equal(want.bytes.begin(), want.bytes.end(), padded.begin()) &&
                   std::all_of(padded.begin() + want.bytes.size(), padded.end(), [](uint8_t b) { return b == 0; }),
               "gx_revcomp_batch padding", name, strands);
        if (!want.bytes.empty()) {
            Bytes small(want.bytes.size() - 1, 0xEE);
            rc_ = gx_revcomp_batch(nullptr, in.bytes.data(), in.off.data(), in.n(), strands, small.data(), small.size(), off.data());
            expect(rc_ == GX_ECAP && off == want.off && std::all_of(small.begin(), small.end(), [](uint8_t b) { return b == 0xEE; }),
                   "gx_revcomp_batch GX_ECAP", name, strands);
        }
    }
}

// The exact search, matching statistics and MEMs: any bytes above '$', any length up to 65,535.
void check_any(gx_suffix_index* idx, const char* name, const std::vector<Bytes>& pats) {
    const Packed in(pats);
    for (uint32_t strands = 1; strands <= 3; ++strands) {
        const Packed it(items_of(pats, strands));
        const size_t n = it.n();
        {
            std::vector<gx_search_hit> a(n), b(n);
            std::vector<uint64_t> ao(n + 1), bo(n + 1);
            int ra = gx_suffix_index_search_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, a.data(), 3, nullptr, 0, ao.data());
            int rb = gx_suffix_index_search(idx, it.bytes.data(), it.off.data(), n, b.data(), 3, nullptr, 0, bo.data());
            expect(ra == GX_OK && rb == GX_OK && same(a, b) && ao == bo, "search counts", name, strands);
            std::vector<uint32_t> ap(ao[n]), bp(bo[n]);
            ra = gx_suffix_index_search_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, a.data(), 3, ap.data(), ap.size(), ao.data());
            rb = gx_suffix_index_search(idx, it.bytes.data(), it.off.data(), n, b.data(), 3, bp.data(), bp.size(), bo.data());
            expect(ra == rb && same(a, b) && ao == bo && ap == bp, "search", name, strands);
        }
        {
            std::vector<gx_match_stat> a(it.bytes.size()), b(it.bytes.size());
            const int ra = gx_suffix_index_match_stats_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, 19, a.data());
            const int rb = gx_suffix_index_match_stats(idx, it.bytes.data(), it.off.data(), n, 19, b.data());
            expect(ra == GX_OK && rb == GX_OK && same(a, b), "match_stats", name, strands);
        }
        {
            std::vector<uint64_t> ao(n + 1), bo(n + 1), ac(n), bc(n);
            int ra = gx_suffix_index_mems_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, 6, nullptr, 0, ao.data(), ac.data());
            int rb = gx_suffix_index_mems(idx, it.bytes.data(), it.off.data(), n, 6, nullptr, 0, bo.data(), bc.data());
            expect(ra == GX_OK && rb == GX_OK && ao == bo && ac == bc, "mems counts", name, strands);
            std::vector<gx_mem> am(ao[n]), bm(bo[n]);
            ra = gx_suffix_index_mems_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, 6, am.data(), am.size(), ao.data(), ac.data());
            rb = gx_suffix_index_mems(idx, it.bytes.data(), it.off.data(), n, 6, bm.data(), bm.size(), bo.data(), bc.data());
            expect(ra == GX_OK && rb == GX_OK && same(am, bm) && ao == bo && ac == bc, "mems", name, strands);
        }
    }
}

// The k-mismatch and k-difference searches and the extension of what the latter reports: patterns of k + 1 to
// GX_EDIT_MAX_M bytes.
void check_k(gx_suffix_index* idx, const char* name, const std::vector<Bytes>& pats, uint32_t k) {
    const Packed in(pats);
    const gx_scores sc{1, -2, -1, -5};
    for (uint32_t strands = 1; strands <= 3; ++strands) {
        const Packed it(items_of(pats, strands));
        const size_t n = it.n();
        {
            std::vector<gx_approx_hit> a(n), b(n);
            std::vector<uint64_t> ao(n + 1), bo(n + 1);
            int ra = gx_suffix_index_search_approx_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, k, a.data(), 4, nullptr,
                                                           nullptr, 0, ao.data());
            int rb = gx_suffix_index_search_approx(idx, it.bytes.data(), it.off.data(), n, k, b.data(), 4, nullptr, nullptr, 0, bo.data());
            expect(ra == GX_OK && rb == GX_OK && same(a, b) && ao == bo, "approx counts", name, strands);
            std::vector<uint32_t> ap(ao[n] + 1), bp(bo[n] + 1);
            Bytes ad(ao[n] + 1), bd(bo[n] + 1);
            ra = gx_suffix_index_search_approx_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, k, a.data(), 4, ap.data(),
                                                       ad.data(), ao[n], ao.data());
            rb = gx_suffix_index_search_approx(idx, it.bytes.data(), it.off.data(), n, k, b.data(), 4, bp.data(), bd.data(), bo[n],
                                               bo.data());
            expect(ra == GX_OK && rb == GX_OK && same(a, b) && ao == bo && ap == bp && ad == bd, "approx", name, strands);
        }
        std::vector<gx_edit_hit> a(n), b(n);
        std::vector<uint64_t> ao(n + 1), bo(n + 1);
        int ra = gx_suffix_index_search_edit_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, k, a.data(), 4, nullptr,
                                                     nullptr, nullptr, 0, ao.data());
        int rb = gx_suffix_index_search_edit(idx, it.bytes.data(), it.off.data(), n, k, b.data(), 4, nullptr, nullptr, nullptr, 0,
                                             bo.data());
        expect(ra == GX_OK && rb == GX_OK && same(a, b) && ao == bo, "edit counts", name, strands);
        const size_t nh = ao[n];
        std::vector<uint32_t> ae(nh + 1), be(nh + 1), as(nh + 1), bs(nh + 1);
        Bytes ad(nh + 1), bd(nh + 1);
        ra = gx_suffix_index_search_edit_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, k, a.data(), 4, ae.data(),
                                                 ad.data(), as.data(), nh, ao.data());
        rb = gx_suffix_index_search_edit(idx, it.bytes.data(), it.off.data(), n, k, b.data(), 4, be.data(), bd.data(), bs.data(), nh,
                                         bo.data());
        expect(ra == GX_OK && rb == GX_OK && same(a, b) && ao == bo && ae == be && ad == bd && as == bs, "edit", name, strands);
        if (ra != GX_OK || rb != GX_OK) continue;
        std::vector<gx_extend_hit> ax(nh + 1), bx(nh + 1);
        std::vector<uint64_t> aco(nh + 1), bco(nh + 1);
        ra = gx_suffix_index_extend_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, ao.data(), as.data(), ae.data(), &sc,
                                            k, ax.data(), nullptr, 0, aco.data());
        rb = gx_suffix_index_extend(idx, it.bytes.data(), it.off.data(), n, bo.data(), bs.data(), be.data(), &sc, k, bx.data(),
                                    nullptr, 0, bco.data());
        expect(ra == GX_OK && rb == GX_OK && aco == bco, "extend counts", name, strands);
        std::vector<uint32_t> ac(aco[nh] + 1), bc(bco[nh] + 1);
        ra = gx_suffix_index_extend_strands(idx, in.bytes.data(), in.off.data(), in.n(), strands, ao.data(), as.data(), ae.data(), &sc,
                                            k, ax.data(), ac.data(), aco[nh], aco.data());
        rb = gx_suffix_index_extend(idx, it.bytes.data(), it.off.data(), n, bo.data(), bs.data(), be.data(), &sc, k, bx.data(),
                                    bc.data(), bco[nh], bco.data());
        ax.resize(nh);
        bx.resize(nh);
        expect(ra == GX_OK && rb == GX_OK && same(ax, bx) && aco == bco && ac == bc, "extend", name, strands);
    }
}

}  // namespace

int main() {
    std::mt19937 rng(24);
    const std::string alpha = std::string("ACGTRYKMBVDHSWNUacgtrykmbvdhswnu%*-.0279@[^_{~") + "\x7f\x80\xc3\xff";
    auto draw = [&](size_t m) {
        Bytes b(m);
        for (auto& c : b) c = (uint8_t)alpha[rng() % alpha.size()];
        return b;
    };
    const size_t kLengths[] = {0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257};
    const size_t nl = sizeof(kLengths) / sizeof(kLengths[0]);
    Bytes text(3000);
    for (auto& c : text) c = (uint8_t)"ACGT"[rng() % 4];
    gx_suffix_index* idx = nullptr;
    if (gx_suffix_index_build(nullptr, text.data(), text.size(), &idx) != GX_OK) return 2;
    for (size_t q = 0; q < 8; ++q) {
        std::vector<Bytes> pats = {draw(q)}, cut;
        for (size_t j = 0; j < nl; ++j) pats.push_back(draw(kLengths[(q + j) % nl]));
        // some that occur: windows of the text of the same lengths, every other one reverse-complemented, one
        // base changed in every third
        for (size_t j = 0; j < nl; ++j) {
            const size_t m = kLengths[(q + j) % nl], i = rng() % (text.size() - m);
            Bytes w(text.begin() + i, text.begin() + i + m);
            if (m > 3 && j % 3 == 0) w[m / 2] = (uint8_t)(w[m / 2] == 'A' ? 'C' : 'A');
            pats.push_back(j % 2 ? rc(w) : w);
            if (m >= 3) cut.push_back(pats.back());
        }
        const std::string name = "rotation" + std::to_string(q);
        check_revcomp(name.c_str(), pats);
        check_any(idx, name.c_str(), pats);
        for (uint32_t k : {0u, 1u, 2u}) check_k(idx, name.c_str(), cut, k);
    }
    check_revcomp("n0", {});
    check_any(idx, "n0", {});
    check_k(idx, "n0", {}, 1);
    check_revcomp("n1-m0", {Bytes()});
    check_any(idx, "n1-m0", {Bytes()});
    check_revcomp("all-empty", std::vector<Bytes>(300));
    check_any(idx, "all-empty", std::vector<Bytes>(300));
    check_revcomp("m65535", {draw(65535)});
    check_any(idx, "m65535", {draw(65535)});
    check_revcomp("m70001", {draw(70001)});
    {   // (above the exact search's pattern length: the long-query calls alone)
        const std::vector<Bytes> pats = {draw(70001)};
        const Packed in(pats);
        for (uint32_t strands = 1; strands <= 3; ++strands) {
            const Packed it(items_of(pats, strands));
            std::vector<gx_match_stat> a(it.bytes.size()), b(it.bytes.size());
            const int ra = gx_suffix_index_match_stats_strands(idx, in.bytes.data(), in.off.data(), 1, strands, 19, a.data());
            const int rb = gx_suffix_index_match_stats(idx, it.bytes.data(), it.off.data(), it.n(), 19, b.data());
            expect(ra == GX_OK && rb == GX_OK && same(a, b), "match_stats", "m70001", strands);
        }
    }
    gx_suffix_index_free(idx);
    printf(failures ? "strand_host_check: %d FAILED\n" : "strand_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
