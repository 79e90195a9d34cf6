"""Edit search on the GPU: gx_suffix_index_search_edit on a device-resident
index, every result checked against the brute force of tests/edit_check.py and
compared field by field with the host index, at the shapes where gx_edit.hip and
the kernels it borrows can go wrong:

  band widths     pattern lengths around 8, 16, 32, 64 and 128 and m = k + 1 for
                  k in {0, 1, 2, 3, 8} (both ends of every instantiation's k
                  range), m = 4096 at k = 8; a substitution, an insertion and a
                  deletion at every byte in turn (k = 1), at the first and last
                  byte of every piece (k = 2, 3), windows at every alignment mod 8
  distance edge   one locus at exactly k edits and at k + 1
  the minimum     inputs on which two candidates report one end with different
                  distances
  text edges      pattern bytes missing at position 0 (negative diagonals, down to
                  -k) and at n, tiny texts
  runs            A^5000 and (ACGT)^1250: every end reported by many candidates
  batch shapes    npat around the wave and the workgroup, ends before dedupe
                  around the scan tile, skewed candidates, counts only, starts
                  NULL, GX_ECAP, both budgets, the refusals, alternating searches,
                  the CLI

Every device search must show candidates equal to the hits' sum, cell updates
<= sum_p candidates_p m_p (2k + 1), and seed_ms, verify_ms and dedupe_ms above
zero where seeds exist."""
import os
import subprocess

import numpy as np
import pytest

from edit_check import ALL_HITS, band_reports, brute, check_edit, disagreements, same_edit, segment
from conftest import COMPARISON, ROOT, read_fasta_records
from test_approx_host import other
from test_edit_host import KINDS, ecap_protocol, edited, random_edits, refusals, wrap_case
from test_suffix_host import BYTES_219, np_rand

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "genomics-rs_amd", "gx-align")
N5 = 5000
LENGTHS = (2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 129)


def device_edit(gx, ctx, idx, pats, k, max_hits, starts=True, seeds=True):
    """The search, with what every case asserts of edit_info."""
    r = idx.search_edit(pats, k, max_hits=max_hits, starts=starts)
    info = gx.edit_info(ctx)
    lengths = np.array([len(p) for p in pats], np.int64)
    cand, count = r["candidates"].astype(np.int64), r["count"].astype(np.int64)
    bound = int((cand * lengths * (2 * k + 1)).sum())
    print(f"npat {len(pats)} k {k} max_hits {max_hits}: {info}, bound {bound}")
    assert info["candidates"] == int(cand.sum()), info
    assert info["cell_updates"] <= bound, (info, bound)
    # every end comes from at least one candidate and from at most (2k + 1)(k + 1); a candidate reports at most 2k + 1
    assert int(count.sum()) <= info["pre_dedupe_ends"] <= min(int(cand.sum()), int(count.sum()) * (k + 1)) * (2 * k + 1), info
    if seeds:
        assert info["candidates"] > 0 and info["cell_updates"] > 0, info
        assert info["seed_ms"] > 0 and info["verify_ms"] > 0 and info["dedupe_ms"] > 0, info
    return r


class Text:
    """A text with its host index and its device index, shared by the cases on it."""

    def __init__(self, gx, ctx, s: bytes):
        self.gx, self.ctx, self.s = gx, ctx, s
        self.host = gx.SuffixIndex(s, host=True)
        self.dev = gx.SuffixIndex(s, ctx=ctx)

    def check(self, pats, k, max_hits=ALL_HITS, starts=True, seeds=True):
        r = device_edit(self.gx, self.ctx, self.dev, pats, k, max_hits, starts=starts, seeds=seeds)
        check_edit(self.s, pats, k, r, max_hits)
        same_edit(r, self.host.search_edit(pats, k, max_hits=max_hits, starts=starts))
        return r

    def close(self):
        self.dev.close()
        self.host.close()


def pieces(m: int, k: int):
    return [(j * m // (k + 1), (j + 1) * m // (k + 1)) for j in range(k + 1)]


@pytest.fixture(scope="module")
def acgt(gx, ctx):
    t = Text(gx, ctx, np_rand(5001, b"ACGT", 1500))
    yield t
    t.close()


@pytest.fixture(scope="module")
def unary(gx, ctx):
    t = Text(gx, ctx, b"A" * N5)
    yield t
    t.close()


@pytest.mark.parametrize("k", [0, 1, 2, 3, 8])
def test_band_width_edges(acgt, k):
    """Every length with m >= k + 1, m = k + 1 itself, windows at every alignment mod 8: exact, with k and with
    k + 1 random edits; for k = 1 each kind of edit at every byte in turn; for k = 2, 3 edits at the first and the
    last byte of every piece, the kinds in turn."""
    s, rng = acgt.s, np.random.default_rng(k)
    trip = []   # (pattern, the end of the window it was cut from, planted edits)

    def add(i, m, edits):
        P = edited(s[i:i + m], edits, b"ACGT")
        if len(P) >= k + 1:
            trip.append((P, i + m, len(edits)))

    for m in sorted(set(LENGTHS + (k + 1,))):
        if m < k + 1:
            continue
        base = 8 * int(rng.integers(1, (len(s) - 140) // 8))
        for a in range(8):
            i = base + a
            add(i, m, [])
            for count in (k, k + 1):
                if 0 < count <= m:
                    add(i, m, random_edits(rng, m, count))
            if k in (2, 3):
                for q, (lo, hi) in enumerate(pieces(m, k)):
                    add(i, m, [(KINDS[(q + a + c) % 3], c) for c in sorted({lo, hi - 1})])
        if k == 1:
            for c in range(m):
                for kind in KINDS:
                    add(base + c % 8, m, [(kind, c)])
    pats = [t[0] for t in trip]
    r = acgt.check(pats, k)
    for p, (P, end, count) in enumerate(trip):
        if count <= k:
            seg = segment(r, p)
            assert end in seg and seg[end][0] <= count, (P, end, count)
    acgt.check(pats[::7], k, max_hits=1)


def test_longest_pattern(gx, ctx):
    """m = GX_EDIT_MAX_M at k = 8: 4,096 rows of 17 cells a lane, pieces of 455 bytes."""
    s = np_rand(77, b"ACGT", 6000)
    rng = np.random.default_rng(77)
    t = Text(gx, ctx, s)
    pats = [s[1000:5096], edited(s[1001:5097], random_edits(rng, 4096, 8), b"ACGT"),
            edited(s[3:4099], random_edits(rng, 4096, 9), b"ACGT")]
    pats = [P[:4096] for P in pats]
    r = t.check(pats, 8)
    assert segment(r, 0)[5096] == (0, 1000) and int(r["count"][0]) == 17
    t.close()


def test_exactly_k_and_k_plus_1(gx, ctx):
    """Substitutions at spread columns of a window over 219 letters: found with exactly k, absent with k + 1."""
    s = np_rand(40, BYTES_219, 700)
    t = Text(gx, ctx, s)
    for k in (1, 2, 3, 4, 8):
        m, i = 45, 300 + k
        cols = [c * (m // (k + 2)) + 1 for c in range(k + 1)]
        at_k = edited(s[i:i + m], [("sub", c) for c in cols[:k]], BYTES_219)
        over = edited(s[i:i + m], [("sub", c) for c in cols], BYTES_219)
        r = t.check([at_k, over], k)
        assert segment(r, 0)[i + m] == (k, i) and i + m not in segment(r, 1)
    t.close()


def test_bands_disagree(gx, ctx):
    """AAACCAA / CCAC / k = 3 (two candidates report end 6, with 1 and with 3) and 20 more inputs of that kind,
    found by the band model of edit_check.py: the dedupe must take the minimum, not a run's first."""
    assert {1, 3} <= set(band_reports(b"AAACCAA", b"CCAC", 3)[6])
    for s, P in [(b"AAACCAA", b"CCAC")] + disagreements(20, 2020):
        t = Text(gx, ctx, s)
        r = t.check([P], 3)
        rep = band_reports(s, P, 3)
        assert {e: min(v) for e, v in rep.items()} == {e: d for e, (d, _) in segment(r, 0).items()}
        t.close()


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_text_edges(gx, ctx, k):
    """The first 1 .. k pattern bytes missing at text position 0: the seeds lie on the diagonals -1 .. -k.  The last
    1 .. k missing at n: without the boundary the window would run over '$'."""
    s = np_rand(50 + k, BYTES_219, 400)
    t = Text(gx, ctx, s)
    m, n, junk = 60, len(s), bytes([other(s[0], BYTES_219)])
    pats, want = [], []
    for j in range(1, k + 1):
        pats.append(junk * j + s[:m - j])              # best: drop the j bytes, window s[0:m - j]
        want.append((m - j, j, 0))
        pats.append(s[n - (m - j):] + junk * j)        # best: drop the j bytes, window s[n - (m - j):n]
        want.append((n, j, n - (m - j)))
        pats.append(s[j:m])                            # an exact window at j: diagonals j - k .. j + k, some below 0
        want.append((m, 0, j))
    pats += [s[:m], s[n - m:], s[n - k - 1:]]
    r = t.check(pats, k)
    for p, (e, d, b) in enumerate(want):
        assert segment(r, p)[e] == (d, b), (p, e, d, b)
    t.check(pats, k, max_hits=2)
    t.close()


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9])
def test_tiny_texts(gx, ctx, n):
    s = np_rand(60 + n, b"AC", n)
    t = Text(gx, ctx, s)
    for k in (0, 1, 2):
        pats = [P for P in (s, s + b"A", b"C" + s, s[1:], s[:-1], b"A" * (k + 1), b"C" * (n + k), b"ACACACACACAC",
                            b"C" * 17, b"%%%") if len(P) >= k + 1]
        t.check(pats, k, seeds=False)
        t.check(pats, k, max_hits=1, seeds=False)
    t.close()


def test_unary_run(gx, ctx, unary):
    """A^20 in A^5000 at k = 1: every end 19 .. 5000 from 9,982 candidates, each end reported by up to 6 of them."""
    r = unary.check([b"A" * 20], 1)
    assert int(r["count"][0]) == 4982 and int(r["candidates"][0]) == 9982
    assert r["ends"].tolist() == list(range(19, N5 + 1))
    info = gx.edit_info(ctx)
    assert 4982 < info["pre_dedupe_ends"] <= 4982 * 6, info   # the run-length invariant: (2k + 1)(k + 1) = 6
    unary.check([b"A" * 20, b"A" * 9 + b"C" + b"A" * 9], 2, max_hits=5)


def test_periodic_run(gx, ctx):
    t = Text(gx, ctx, b"ACGT" * 1250)
    t.check([b"ACGT" * 5, b"ACGT" * 2 + b"ACT" + b"ACGT" * 2, b"CGTA" * 4 + b"G"], 2)
    t.check([b"ACGT" * 5, b"GTAC" * 3], 3, max_hits=7)
    t.close()


def random_batch(s: bytes, npat: int, k: int, seed: int):
    rng = np.random.default_rng(seed)
    pats = []
    for p in range(npat):
        m = int(rng.integers(max(k + 2, 8), 26))
        i = int(rng.integers(0, len(s) - m))
        pats.append(edited(s[i:i + m], random_edits(rng, m, p % (k + 2)), b"ACGT"))
    return pats


@pytest.mark.parametrize("npat", [1, 63, 64, 65, 256, 257])
def test_batch_edges_small(acgt, npat):
    pats = random_batch(acgt.s, npat, 2, npat)
    acgt.check(pats, 2, max_hits=4)
    acgt.check(pats, 2, max_hits=0)


def test_ends_around_the_scan_tile(gx, ctx, acgt):
    """Batches whose ends before dedupe come to 2,046 .. 2,052, the scan and sort tile being 2,048: the number
    the band model predicts is the number the device reports."""
    assert gx.suffix_tile()[0] == 2048
    k = 1
    pool = random_batch(acgt.s, 900, k, 4242)
    per = [sum(len(v) for v in band_reports(acgt.s, P, k).values()) for P in pool]
    for target in range(2046, 2053):
        pats, total = [], 0
        for P, q in zip(pool, per):   # in turn, whatever still fits: the patterns with one end close the gap
            if total + q <= target:
                pats.append(P)
                total += q
        assert total == target
        acgt.check(pats, k, max_hits=3)
        assert gx.edit_info(ctx)["pre_dedupe_ends"] == target


def test_candidate_skew(unary):
    """One pattern with thousands of candidates between patterns with none."""
    pats = [b"C" * 10, b"CCCCCCCCCCCC", b"A" * 20, b"C" * 12, b"GGGG"]
    r = unary.check(pats, 1, max_hits=9)
    assert r["candidates"].tolist() == [0, 0, 9982, 0, 0]
    unary.check(pats, 1, max_hits=0)


def test_counts_only_and_no_starts(acgt):
    pats = random_batch(acgt.s, 100, 2, 5)
    a = acgt.check(pats, 2, max_hits=0)
    b = acgt.check(pats, 2, max_hits=7)
    c = acgt.check(pats, 2, max_hits=7, starts=False)
    for f in a:
        assert np.array_equal(a[f], b[f])
    assert c["starts"] is None and np.array_equal(b["ends"], c["ends"]) and np.array_equal(b["distances"], c["distances"])


def test_ecap_on_device(gx, ctx):
    idx = gx.SuffixIndex(b"BANANA", ctx=ctx)
    ecap_protocol(gx, idx)
    info = gx.edit_info(ctx)
    assert info["candidates"] > 0 and info["verify_ms"] > 0
    idx.close()


def test_refusals_and_budgets_on_device(gx, ctx, monkeypatch):
    idx = gx.SuffixIndex(b"ACGTACGT", ctx=ctx)
    refusals(gx, idx, monkeypatch)
    idx.close()


def test_wrap_case_on_device(gx, ctx, monkeypatch):
    idx = gx.SuffixIndex(b"A" * N5, ctx=ctx)
    wrap_case(gx, idx, monkeypatch)
    info = gx.edit_info(ctx)
    assert info["candidates"] == 2 * 430000 * 5000 and info["cell_updates"] == 0 and info["verify_ms"] == 0, info
    r = idx.search_edit([b"AA"], 1)   # the index and the context go on working
    assert r["count"].tolist() == [N5]
    idx.close()


def test_alternating_and_two_indexes(gx, ctx, acgt):
    from approx_check import check_approx
    from search_check import Brute, check_result
    sB = np_rand(6000, b"ACGT", 2000)
    B = Text(gx, ctx, sB)
    brA, brB = Brute(acgt.s), Brute(sB)
    pa, pb = random_batch(acgt.s, 40, 2, 1), random_batch(sB, 40, 2, 2)
    exact = [acgt.s[10:30], sB[-9:], b"ACGTACG", b""]
    for _ in range(2):
        acgt.check(pa + pb, 2, max_hits=3)
        check_result(brA, exact, acgt.dev.search(exact, max_hits=ALL_HITS), ALL_HITS)
        check_approx(sB, pb, 2, B.dev.search_approx(pb, 2, max_hits=ALL_HITS), ALL_HITS)
        B.check(pb + pa, 2)
        check_result(brB, exact, B.dev.search(exact, max_hits=ALL_HITS), ALL_HITS)
        check_approx(acgt.s, pa, 1, acgt.dev.search_approx(pa, 1, max_hits=ALL_HITS), ALL_HITS)
    B.close()


def reads_of(s: bytes, nreads: int, m: int, k: int, seed: int):
    """nreads reads of about m bases cut from s, read r with r % (k + 2) edits, insertions and deletions in turn."""
    rng = np.random.default_rng(seed)
    at = rng.integers(0, len(s) - m + 1, nreads).tolist()
    reads = []
    for r, i in enumerate(at):
        cols = rng.choice(m, r % (k + 2), replace=False).tolist()
        reads.append(edited(s[i:i + m], [(("ins", "del")[(r + q) % 2], c) for q, c in enumerate(cols)], b"ACGT"))
    return reads, at


def test_covid_reads_and_cli(gx, ctx, tmp_path):
    path = os.path.join(COMPARISON, "Covid_Wuhan.fasta")
    s = read_fasta_records(path)[0][1]
    assert set(s) <= set(b"ACGT")
    pats, at = reads_of(s, 2000, 50, 2, 11)
    dev, host = gx.SuffixIndex(s, ctx=ctx), gx.SuffixIndex(s, host=True)
    r = device_edit(gx, ctx, dev, pats, 2, 16)
    same_edit(r, host.search_edit(pats, 2, max_hits=16))
    check_edit(s, pats[:100], 2, {f: r[f][:100] for f in ("count", "best_dist", "best_end", "candidates")}, 0)
    for p, i in enumerate(at):
        if p % 4 <= 2:   # the planted indels are found where the read was cut, with at most their number
            assert segment(r, p).get(i + 50, (9, 0))[0] <= p % 4, p
    dev.close()
    host.close()
    fa = tmp_path / "reads.fasta"
    fa.write_bytes(b"".join(b">read%d\n%s\n" % (q, p) for q, p in enumerate(pats)))
    tsv = tmp_path / "hits.tsv"
    subprocess.run([CLI, "search", "-f", path, "-p", str(fa), "--max-hits", "16", "-e", "2", "-o", str(tsv)], check=True,
                   timeout=120, env=dict(os.environ, GX_LOG="warn"))
    lines = tsv.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 2001
    for q, line in enumerate(lines[:-1]):
        seg = segment(r, q)
        assert line == "\t".join([f"read{q}", str(len(pats[q])), str(r["count"][q]), str(r["best_dist"][q]),
                                  str(r["best_end"][q]), ",".join(f"{b}-{e}:{d}" for e, (d, b) in seg.items())]), q
    bad = subprocess.run([CLI, "search", "-f", path, "-p", str(fa), "-e", "2", "-k", "1"], capture_output=True, timeout=60)
    assert bad.returncode == 2   # -e together with -k
