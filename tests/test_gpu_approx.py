"""Approximate search on the GPU: gx_suffix_index_search_approx on a
device-resident index, every result compared field by field with the host
index and checked against the brute force of tests/approx_check.py, at the
sizes where gx_approx.hip and the kernels it borrows change path:

  word and piece edges  pattern lengths around 8, 16, 32, 64 and 128 and m = k + 1,
                        a substitution at every byte in turn, at the first and
                        last byte of every piece, windows at every alignment mod 8
  byte-count exactness  substituted pairs that differ in bit 0 only, in bit 7 only
                        and 0x7F / 0x80: XOR words with 0x01 bytes beside zero bytes
  distance edge         the same window at exactly k and at k + 1
  dedupe                an exact occurrence (every piece leads to it), an occurrence
                        for each single intact piece, A^5000 and (ACGT)^1250
  window legality       starts below 0, windows past n and over '$', tiny texts
  batch shapes          npat around the wave and the workgroup, pieces around the
                        scan tile, skewed candidates, counts only, GX_ECAP, the
                        budget and the 64-bit total, alternating searches, the CLI

Every device search must show candidates > 0 where seeds exist, seed_ms > 0 and
verify_ms > 0, and keep the work bound: word steps <= sum_p candidates_p
(ceil(m_p / 8) + k + 1)."""
import os
import subprocess

import numpy as np
import pytest

from approx_check import ALL_HITS, NO_DIST, brute, check_approx, same_approx
from conftest import COMPARISON, ROOT, read_fasta_records
from test_approx_host import ecap_protocol, new_errors, other, planted, wrap_case
from test_suffix_host import BYTES_219, np_rand

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "genomics-rs_amd", "gx-align")
N5 = 5000
LENGTHS = (2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 129)


def device_approx(gx, ctx, idx, pats, k, max_hits, lengths=None, seeds=True):
    """The search, with what every case asserts of approx_info."""
    r = idx.search_approx(pats, k, max_hits=max_hits)
    info = gx.approx_info(ctx)
    lengths = np.array([len(p) for p in pats] if lengths is None else lengths, np.int64)
    bound = int((r["candidates"].astype(np.int64) * ((lengths + 7) // 8 + k + 1)).sum())
    print(f"npat {len(lengths)} k {k} max_hits {max_hits}: {info}, bound {bound}")
    assert info["candidates"] == int(r["candidates"].astype(np.int64).sum()), info
    assert info["seed_ms"] > 0 and info["verify_ms"] > 0, info
    assert info["word_compares"] <= bound, (info, bound)
    if seeds:
        assert info["candidates"] > 0, info
    return r


class Text:
    """A text with its host index and its device index, shared by the cases on it."""

    def __init__(self, gx, ctx, s: bytes):
        self.gx, self.ctx, self.s = gx, ctx, s
        self.host = gx.SuffixIndex(s, host=True)
        self.dev = gx.SuffixIndex(s, ctx=ctx)

    def check(self, pats, k, max_hits=ALL_HITS, seeds=True):
        r = device_approx(self.gx, self.ctx, self.dev, pats, k, max_hits, seeds=seeds)
        check_approx(self.s, pats, k, r, max_hits)
        same_approx(r, self.host.search_approx(pats, k, max_hits=max_hits))
        return r

    def close(self):
        self.dev.close()
        self.host.close()


def segment(r, p):
    a, b = int(r["hit_offsets"][p]), int(r["hit_offsets"][p + 1])
    return dict(zip(r["positions"][a:b].tolist(), r["distances"][a:b].tolist()))


def pieces(m: int, k: int):
    return [(j * m // (k + 1), (j + 1) * m // (k + 1)) for j in range(k + 1)]


@pytest.fixture(scope="module")
def acgt(gx, ctx):
    t = Text(gx, ctx, np_rand(5001, b"ACGT", N5))
    yield t
    t.close()


@pytest.mark.parametrize("k", [0, 1, 2, 3, 8])
def test_word_and_piece_edges(acgt, k):
    """Every length with m >= k + 1, m = k + 1 itself, windows at every alignment mod 8: exact, with k and with
    k + 1 substitutions; for k = 1 a substitution at every byte in turn; for k = 2, 3 substitutions at the first
    and the last byte of every piece."""
    s, rng = acgt.s, np.random.default_rng(k)
    trip = []   # (pattern, origin, planted substitutions)
    for m in sorted(set(LENGTHS + (k + 1,))):
        if m < k + 1:
            continue
        base = 8 * int(rng.integers(1, (N5 - 140) // 8))
        for a in range(8):
            i = base + a
            trip.append((s[i:i + m], i, 0))
            for subs in (k, k + 1):
                if 0 < subs <= m:
                    trip.append((planted(s, i, m, rng.choice(m, subs, replace=False).tolist(), b"ACGT"), i, subs))
            if k == 1:
                trip += [(planted(s, i, m, [b], b"ACGT"), i, 1) for b in range(m)]
            if k in (2, 3):
                for lo, hi in pieces(m, k):
                    cols = sorted({lo, hi - 1})
                    trip.append((planted(s, i, m, cols, b"ACGT"), i, len(cols)))
                firsts = [lo for lo, _ in pieces(m, k)]
                trip.append((planted(s, i, m, firsts[:k], b"ACGT"), i, k))        # every piece but the last
                trip.append((planted(s, i, m, firsts[1:], b"ACGT"), i, k))        # every piece but the first
    pats = [t[0] for t in trip]
    r = acgt.check(pats, k)
    for p, (P, origin, subs) in enumerate(trip):
        assert segment(r, p).get(origin) == (subs if subs <= k else None), (P, origin, subs)
    acgt.check(pats[::7], k, max_hits=1)


@pytest.mark.parametrize("alpha", [b"\x40\x41", b"\x41\xc1", b"\x7f\x80", BYTES_219],
                         ids=["bit0", "bit7", "7f_80", "bytes219"])
def test_byte_count_exactness(gx, ctx, alpha):
    """Over a two-letter alphabet every XOR byte is zero or the one difference of the pair (0x01, 0x80, 0xFF): runs
    of 0x01 bytes beside zero bytes, where a borrow-based zero-byte test counts wrongly."""
    s = np_rand(len(alpha) + alpha[0], alpha, 2000)
    t = Text(gx, ctx, s)
    rng = np.random.default_rng(alpha[1])
    for k in (1, 3):
        trip = []
        for m in (8, 9, 16, 24, 33):
            for _ in range(6):
                i = int(rng.integers(0, 2000 - m))
                for subs in range(k + 2):
                    trip.append((planted(s, i, m, rng.choice(m, subs, replace=False).tolist(), alpha), i, subs))
                # a substituted byte directly above an equal one and below an equal one, in one word
                b = int(rng.integers(1, min(m, 8) - 1))
                trip.append((planted(s, i, m, [b], alpha), i, 1))
                trip.append((planted(s, i, m, [b - 1, b + 1][:k], alpha), i, min(k, 2)))
        pats = [x[0] for x in trip]
        r = t.check(pats, k)
        if len(alpha) > 2:   # (over two letters a short pattern recurs: its origin is checked by the brute force alone)
            for p, (P, origin, subs) in enumerate(trip):
                assert segment(r, p).get(origin) == (subs if subs <= k else None), (P, origin, subs)
    t.close()


def test_distance_edge(acgt):
    """One window at exactly k (reported, with that distance) and at k + 1 (not reported)."""
    s = acgt.s
    for k in (1, 2, 3, 8):
        m, i = 64, 1003
        assert brute(s, s[i:i + m], k)[0] == 1   # (unique: the edge is that window's alone)
        cols = list(range(3, 3 + 6 * (k + 1), 6))
        at_k, past_k = planted(s, i, m, cols[:k], b"ACGT"), planted(s, i, m, cols, b"ACGT")
        r = acgt.check([at_k, past_k], k)
        assert segment(r, 0) == {i: k} and segment(r, 1) == {}
        assert r["count"].tolist() == [1, 0] and r["best_dist"].tolist() == [k, NO_DIST]


def test_dedupe_pieces(acgt):
    """An exact occurrence is reached through all k + 1 pieces and reported once; for each j an occurrence
    whose only intact piece is j."""
    s, i, m = acgt.s, 2024, 48
    for k in (1, 2, 3, 8):
        assert brute(s, s[i:i + m], k)[0] == 1
        pats = [s[i:i + m]]
        for j in range(k + 1):
            pats.append(planted(s, i, m, [lo for q, (lo, hi) in enumerate(pieces(m, k)) if q != j], b"ACGT"))
        r = acgt.check(pats, k)
        assert r["count"].tolist() == [1] * (k + 2) and r["best_dist"].tolist() == [0] + [k] * (k + 1)
        assert int(r["candidates"][0]) >= k + 1
        assert r["positions"].tolist() == [i] * (k + 2)


def test_dedupe_unary(gx, ctx):
    t = Text(gx, ctx, b"A" * N5)
    r = t.check([b"A" * 20], 1)
    assert (int(r["count"][0]), int(r["candidates"][0])) == (4981, 9982)   # two pieces A^10, 4,991 hits each
    r = t.check([b"A" * 20, b"A" * 19 + b"C", b"C" + b"A" * 19, b"A" * 9 + b"CC" + b"A" * 9, b"A" * 5000, b"A" * 5001],
                1, max_hits=5)
    assert r["count"].tolist() == [4981, 4981, 4981, 0, 1, 0]
    t.check([b"A" * 20, b"A" * 10 + b"C" + b"A" * 9], 3, max_hits=ALL_HITS)
    t.close()


def test_dedupe_periodic(gx, ctx):
    t = Text(gx, ctx, b"ACGT" * 1250)
    pats = [b"ACGT" * 5, b"ACGT" * 2 + b"ACGA" + b"ACGT" * 2, b"GTAC" * 6 + b"G", b"ACGT" * 1250, b"TCGT" + b"ACGT" * 1249,
            b"ACGT" * 1249 + b"ACGG", b"CCGT" * 3]
    for k in (1, 2):
        r = t.check(pats, k, max_hits=7)
        assert r["count"].tolist()[:2] == [1246, 1246]
    t.close()


def test_window_legality(acgt):
    s, n = acgt.s, N5
    for k in (1, 2):
        pats = [b"TTTTT" + s[:5],                 # the later piece occurs at 0: the start would be negative
                s[1:6] + s[:5],                   # the same with an earlier piece that occurs too
                s[n - 5:] + b"AAAAA",             # the first piece occurs in the last bytes: start + m > n
                s[n - 7:] + s[:3],
                s[n - 15:] + b"A", s[n - 15:] + b"C", s[n - 15:] + b"G", s[n - 15:] + b"T",   # one byte over '$'
                s[n - 16:], s[:16], s[n - 16:n - 1] + bytes([other(s[n - 1], b"ACGT")]),      # the last legal window
                bytes([other(s[0], b"ACGT")]) + s[1:16]]
        r = acgt.check(pats, k)
        assert int(r["count"][8]) >= 1 and segment(r, 10).get(n - 16) == 1 and segment(r, 11).get(0) == 1
        for p in (4, 5, 6, 7):
            assert n - 15 not in segment(r, p)


@pytest.mark.parametrize("host_below", ["0", None], ids=["device_array", "host_array"])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9])
def test_tiny_texts(gx, ctx, monkeypatch, n, host_below):
    """Tiny texts reach the kernels whichever solver built the array."""
    if host_below is not None:
        monkeypatch.setenv("GX_SUFFIX_HOST_BELOW", host_below)
    s = np_rand(n + 20, b"AC", n)
    t = Text(gx, ctx, s)
    for k in (0, 1, 2):
        pats = [P for P in (b"A", b"C", b"AC", b"CA", b"ACA", s, s + b"A", s[1:] + b"C", s[:-1] + b"\xff", b"A" * 9,
                            b"C" * 17, b"%%%") if len(P) >= k + 1]
        t.check(pats, k, seeds=n > 1 or k == 0)
        t.check(pats, k, max_hits=1, seeds=n > 1 or k == 0)
    t.close()


def random_batch(s: bytes, npat: int, k: int, seed: int):
    rng = np.random.default_rng(seed)
    pats = []
    for p in range(npat):
        m = int(rng.integers(max(k + 1, 6), 24))
        i = int(rng.integers(0, len(s) - m))
        pats.append(planted(s, i, m, rng.choice(m, p % (k + 2), replace=False).tolist(), b"ACGT"))
    return pats


@pytest.mark.parametrize("npat", [1, 63, 64, 65, 256, 257])
def test_batch_edges_small(acgt, npat):
    pats = random_batch(acgt.s, npat, 2, npat)
    acgt.check(pats, 2, max_hits=4)
    acgt.check(pats, 2, max_hits=0)


def test_batch_edges_scan_tile(gx, acgt):
    """npat (k + 1) + 1 offsets just inside the scan's tile, one over and a piece count above it."""
    T = gx.suffix_tile()[0]
    assert T == 2048
    for npat, k in ((T // 2 - 1, 1), (T // 2, 1), (T // 2 + 1, 1), (T // 4 + 1, 3)):
        acgt.check(random_batch(acgt.s, npat, k, npat), k, max_hits=3)


def test_candidate_skew(gx, ctx):
    """One pattern with thousands of candidates between patterns with none and a few."""
    s = np_rand(9, b"AC", N5) + b"G" + np_rand(10, b"AC", 40) + b"T"
    t = Text(gx, ctx, s)
    pats = [b"GGGG", b"TTTT", b"GTGT", b"TGTG"] * 5 + [b"ACAC"] + [b"GGGG", b"TGGT", b"TTTG", b"GTTG"] * 5 + [b"CACG", b"ACAT"]
    r = t.check(pats, 1)
    assert int(r["candidates"][20]) > 2048 and int(r["candidates"][:20].sum()) == 0
    t.check(pats, 1, max_hits=3)
    t.close()


def test_counts_only(acgt):
    pats = random_batch(acgt.s, 100, 2, 5)
    a = acgt.check(pats, 2, max_hits=0)
    b = acgt.check(pats, 2, max_hits=7)
    for f in a:
        assert np.array_equal(a[f], b[f])


def test_ecap_on_device(gx, ctx):
    idx = gx.SuffixIndex(b"BANANA", ctx=ctx)
    ecap_protocol(gx, idx)
    info = gx.approx_info(ctx)
    assert info["candidates"] > 0 and info["verify_ms"] > 0
    idx.close()


def test_errors_and_budget_on_device(gx, ctx, monkeypatch):
    idx = gx.SuffixIndex(b"ACGTACGT", ctx=ctx)
    new_errors(gx, idx, monkeypatch)
    idx.close()


def test_wrap_case_on_device(gx, ctx, monkeypatch):
    idx = gx.SuffixIndex(b"A" * N5, ctx=ctx)
    wrap_case(gx, idx, monkeypatch)
    info = gx.approx_info(ctx)
    assert info["candidates"] == 2 * 430000 * 5000 and info["word_compares"] == 0 and info["verify_ms"] == 0, info
    r = idx.search_approx([b"AA"], 1)   # the index and the context go on working
    assert r["count"].tolist() == [4999]
    idx.close()


def test_alternating_and_two_indexes(gx, ctx, acgt):
    from search_check import Brute, check_result
    sB = np_rand(6000, b"ACGT", 6000)
    B = Text(gx, ctx, sB)
    brA, brB = Brute(acgt.s), Brute(sB)
    pa, pb = random_batch(acgt.s, 40, 2, 1), random_batch(sB, 40, 2, 2)
    exact = [acgt.s[10:30], sB[-9:], b"ACGTACG", b""]
    for _ in range(2):
        acgt.check(pa + pb, 2, max_hits=3)
        check_result(brA, exact, acgt.dev.search(exact, max_hits=ALL_HITS), ALL_HITS)
        B.check(pb + pa, 2)
        check_result(brB, exact, B.dev.search(exact, max_hits=ALL_HITS), ALL_HITS)
    B.close()


def reads_of(s: bytes, nreads: int, m: int, k: int, seed: int):
    """nreads reads of m bases cut from s, read r with r % (k + 2) substitutions."""
    rng = np.random.default_rng(seed)
    starts = rng.integers(0, len(s) - m + 1, nreads).tolist()
    return [planted(s, i, m, rng.choice(m, r % (k + 2), replace=False).tolist(), b"ACGT") for r, i in enumerate(starts)], starts


def test_covid_reads_and_cli(gx, ctx, tmp_path):
    path = os.path.join(COMPARISON, "Covid_Wuhan.fasta")
    s = read_fasta_records(path)[0][1]
    assert set(s) <= set(b"ACGT")
    pats, starts = reads_of(s, 2000, 50, 2, 11)
    dev, host = gx.SuffixIndex(s, ctx=ctx), gx.SuffixIndex(s, host=True)
    r = device_approx(gx, ctx, dev, pats, 2, 16)
    same_approx(r, host.search_approx(pats, 2, max_hits=16))
    check_approx(s, pats[:200], 2, {f: (v[:200] if len(v) == 2000 else v) for f, v in r.items()}, 0)
    for p, i in enumerate(starts):
        assert segment(r, p).get(i) == (p % 4 if p % 4 <= 2 else None), p
    dev.close()
    host.close()
    fa = tmp_path / "reads.fasta"
    fa.write_bytes(b"".join(b">read%d\n%s\n" % (q, p) for q, p in enumerate(pats)))
    tsv = tmp_path / "hits.tsv"
    subprocess.run([CLI, "search", "-f", path, "-p", str(fa), "--max-hits", "16", "-k", "2", "-o", str(tsv)], check=True,
                   timeout=120, env=dict(os.environ, GX_LOG="warn"))
    lines = tsv.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 2001
    for q, line in enumerate(lines[:-1]):
        seg = segment(r, q)
        assert line == "\t".join([f"read{q}", "50", str(r["count"][q]), str(r["best_dist"][q]), str(r["best_pos"][q]),
                                  ",".join(f"{i}:{d}" for i, d in seg.items())]), q
