"""gx_suffix_index_extend on the GPU: every hit against the plain-Python restatement of
tests/extend_check.py and, field by field and run by run, against the host index, at the shapes where
gx_extend.hip can go wrong:

  band            B in {0, 1, 2, 3, 4, 5, 8, 9, 15}: both ends of every instantiation (B <= 2, 4, 8, 15) and
                  both trace word widths, each with w - m in {-B, 0, B}
  lengths         m in {1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65}; m = 4,096 at B = 15
  shapes          a gap run at the first and at the last column, each kind of edit at every byte of a
                  33-base read, ties on A^n and (AC)^n that the S > I > D rule breaks
  windows         b = 0 and e = n, empty windows, tiny texts
  hit counts      1, 63, 64, 65, 255, 256, 257, mixed m inside a wave (a tile takes its largest row count),
                  a pattern without a hit between patterns with some
  chunks          GX_EXTEND_TRACE_BYTES for 1, 2 and 3 launches, the boundaries inside one pattern's hits
  score edges     +-GX_EXTEND_MAX_SCORE at m = 4,096, one past it refused
  protocol        cigar = NULL, GX_ECAP, every refusal text, alternating with search_edit and mems on one
                  context, map_reads against the two calls it is made of, the CLI with and without --cigar

Every device call must show extend_info hits equal to the batch's, cell updates
<= sum (w + 1)(2B + 1), and fill_ms and walk_ms above zero."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from extend_check import check_extend, hit_runs, same_extend
from extend_error_cases import TEXT, run_case
from test_edit_host import KINDS, edited
from test_extend_host import CASES, WANT, limits, unrelated_hits
from test_suffix_host import np_rand

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "genomics-rs_amd", "gx-align")
BANDS = (0, 1, 2, 3, 4, 5, 8, 9, 15)
LENGTHS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65)
DEFAULT = (1, -2, -1, -5)


def as_hits(per_read):
    """per_read[p] = [(b, e), ...] -> the mapping extend takes."""
    flat = [w for ws in per_read for w in ws]
    off = np.zeros(len(per_read) + 1, np.uint64)
    np.cumsum([len(ws) for ws in per_read], out=off[1:])
    return {"hit_offsets": off, "starts": np.array([b for b, _ in flat], np.uint32),
            "ends": np.array([e for _, e in flat], np.uint32)}


class Text:
    """A text with its host index and its device index, shared by the cases on it."""

    def __init__(self, gx, ctx, s: bytes):
        self.gx, self.ctx, self.s = gx, ctx, s
        self.host = gx.SuffixIndex(s, host=True)
        self.dev = gx.SuffixIndex(s, ctx=ctx)

    def check(self, reads, hits, scores, B, cigars=True, chunks=None):
        gx = self.gx
        r = self.dev.extend(reads, hits, gx.Scores(*scores), band=B, cigars=cigars)
        info = gx.extend_info(self.ctx)
        w = np.asarray(hits["ends"]).astype(np.int64) - np.asarray(hits["starts"]).astype(np.int64)
        bound = int(((w + 1) * (2 * B + 1)).sum())
        print(f"hits {len(w)} B {B} scores {scores}: {info}, bound {bound}")
        assert info["hits"] == len(w) and 0 < info["cell_updates"] <= bound, (info, bound)
        assert info["fill_ms"] > 0 and info["walk_ms"] > 0 and info["trace_bytes"] > 0, info
        if chunks is not None:
            assert info["chunks"] == chunks, info
        assert check_extend(self.s, reads, hits, scores, B, r, cigars=cigars) == len(w)
        same_extend(r, self.host.extend(reads, hits, gx.Scores(*scores), band=B, cigars=cigars))
        return r

    def close(self):
        self.dev.close()
        self.host.close()


@pytest.fixture(scope="module")
def acgt(gx, ctx):
    t = Text(gx, ctx, np_rand(2201, b"ACGT", 6000))
    yield t
    t.close()


def gapped(window: bytes, m: int, where: str, seed: int) -> bytes:
    """A read of m bytes from a window of w: the |w - m| bytes are dropped from, or put into, the window as one
    run at its first column, its last column or its middle; "sub" adds a substitution."""
    w, rng = len(window), np.random.default_rng(seed)
    run = abs(w - m)
    at = {"first": 0, "last": w if w < m else w - run, "middle": min(w, m) // 2, "sub": min(w, m) // 3}[where]
    if w >= m:
        read = window[:at] + window[at + run:]
    else:
        read = window[:at] + np_rand(seed, b"ACGT", run) + window[at:]
    if where == "sub" and m:
        c = int(rng.integers(0, m))
        read = read[:c] + bytes([b"ACGT"[(b"ACGT".index(read[c]) + 1) % 4]]) + read[c + 1:]
    assert len(read) == m
    return read


@pytest.mark.parametrize("B", BANDS)
def test_bands_and_lengths(acgt, B):
    s = acgt.s
    rng = np.random.default_rng(B)
    reads, per = [], []
    for m in LENGTHS:
        for d in sorted({-B, 0, B}):
            w = m + d
            if w < 0:
                continue
            for q, where in enumerate(("first", "last", "middle", "sub", "unrelated")):
                b = int(rng.integers(0, len(s) - w + 1))
                reads.append(np_rand(100 * m + q, b"ACGT", m) if where == "unrelated" else gapped(s[b:b + w], m, where, 7 * m + q))
                per.append([(b, b + w)])
    hits = as_hits(per)
    acgt.check(reads, hits, DEFAULT, B)
    acgt.check(reads, hits, (2, -1, -1, 0), B)
    acgt.check(reads[::3], as_hits(per[::3]), (0, -1, -3, -1), B, cigars=False)


@pytest.mark.parametrize("scores", [DEFAULT, (32767, -32767, -32767, -32767), (-32767, 32767, 32767, 32767)],
                         ids=["default", "max", "max-signs-swapped"])
def test_longest_pattern_at_the_widest_band(gx, ctx, scores):
    """m = GX_EDIT_MAX_M at B = 15, w - m in {-15, 0, 15}: 4,112 rows of 31 cells a lane, and with the scores
    at the limit the values that come closest to the 32-bit sentinel."""
    s = np_rand(4096, b"ACGT", 6000)
    t = Text(gx, ctx, s)
    rng = np.random.default_rng(15)
    P = edited(s[1000:1000 + 4096], [(KINDS[q % 3], int(c)) for q, c in enumerate(rng.choice(4096, 9, replace=False))], b"ACGT")
    P = (P + s[5096:5100])[:4096]
    r = t.check([P], as_hits([[(1000, 5096), (1000, 5096 + 15), (1008, 5096 - 7), (1015, 5096)]]), scores, 15)
    assert int(r["n_steps"].max()) >= 4096
    t.close()


def test_one_past_the_score_limit_is_refused(gx, acgt):
    hits = as_hits([[(0, 8)]])
    for bad in ((32768, -2, -1, -5), (1, -2, -1, -32768)):
        with pytest.raises(gx.GxError) as e:
            acgt.dev.extend([acgt.s[:8]], hits, gx.Scores(*bad), band=0)
        assert e.value.code == 3 and "GX_EXTEND_MAX_SCORE" in str(e.value)
    acgt.check([acgt.s[:8]], hits, (32767, -2, -1, -32767), 0)


def test_every_edit_at_every_byte(gx, acgt):
    """A 33-base read with a substitution, an insertion and a deletion at every byte in turn, found by the edit
    search at k = 1 and aligned at B = 1; the exact read too."""
    s, i = acgt.s, 1234
    reads = [s[i:i + 33]] + [edited(s[i:i + 33], [(kind, c)], b"ACGT") for c in range(33) for kind in KINDS]
    found = acgt.dev.search_edit(reads, 1, max_hits=8)
    assert (np.diff(found["hit_offsets"]) > 0).all()
    r = acgt.check(reads, found, DEFAULT, 1)
    exact = [h for h in range(int(found["hit_offsets"][1])) if found["distances"][h] == 0]   # read 0 where it was cut
    assert len(exact) == 1 and gx.cigar_string(hit_runs(r, exact[0])) == "33M" and r["score"][exact[0]] == 33
    acgt.check(reads, found, (5, -4, -2, -10), 2)


@pytest.mark.parametrize("unit", [b"A", b"AC"], ids=["A^n", "(AC)^n"])
def test_ties(gx, ctx, unit):
    """Periodic texts: many paths share the maximum, and only the S > I > D order picks one."""
    s = unit * (400 // len(unit))
    t = Text(gx, ctx, s)
    reads = [unit * (20 // len(unit)), unit * (18 // len(unit)) + b"C" + unit * 4, (unit * 12)[1:], unit * 3]
    found = t.dev.search_edit(reads, 2, max_hits=12)
    assert len(found["ends"]) >= 24
    for scores in (DEFAULT, (2, -1, -1, 0), (1, -1, 0, 0)):
        t.check(reads, found, scores, 2)
    per = [[(b, b + len(P) + d) for b in (0, 7, len(s) - len(P) - 3) for d in (-3, 0, 3)] for P in reads]
    t.check(reads, as_hits(per), DEFAULT, 3)
    t.check(reads, as_hits(per), (1, -1, 0, 0), 5)
    t.close()


@pytest.mark.parametrize("n", [1, 2, 7, 8])
def test_text_edges_and_tiny_texts(gx, ctx, n):
    """Windows that begin at 0 and end at n, and the empty windows [0, 0) and [n, n)."""
    s = np_rand(80 + n, b"AC", n)
    t = Text(gx, ctx, s)
    reads = [s, s + b"A", b"C" + s, s[1:] or b"A", b"A", b"AC", b"CCA"]
    for B in (0, 1, 3):
        keep, per = [], []
        for P in reads:
            ws = [(b, e) for b, e in ((0, n), (0, 0), (n, n), (0, min(n, len(P))), (max(0, n - len(P)), n))
                  if abs((e - b) - len(P)) <= B]
            keep.append(P)
            per.append(sorted(set(ws)))
        if any(per):
            t.check(keep, as_hits(per), DEFAULT, B)
            t.check(keep, as_hits(per), (2, -1, -1, 0), B)
    t.close()


@pytest.mark.parametrize("nhits", [1, 63, 64, 65, 255, 256, 257])
def test_hit_counts(acgt, nhits):
    """Reads of 5 .. 40 bases with 0 .. 3 hits each, so that a wave holds several lengths and every fourth read
    has no hit at all."""
    s, rng = acgt.s, np.random.default_rng(nhits)
    reads, per, total = [], [], 0
    while total < nhits:
        p = len(reads)
        m, want = 5 + (7 * p) % 36, min((p + 1) % 4, nhits - total)
        b = int(rng.integers(0, len(s) - m - 2))
        reads.append(edited(s[b:b + m], [(KINDS[p % 3], int(rng.integers(0, m)))] if p % 2 else [], b"ACGT"))
        m = len(reads[-1])
        per.append([(b + q, b + q + m + (-1, 0, 1)[(p + q) % 3]) for q in range(want)])
        total += want
    reads.append(b"ACGTACGT")   # and a last read without a hit
    per.append([])
    assert any(not ws for ws in per[:-1]) or nhits == 1
    acgt.check(reads, as_hits(per), DEFAULT, 1, chunks=1)
    acgt.check(reads, as_hits(per), (1, -1, -3, -1), 4, cigars=False)


def test_chunks(gx, acgt, monkeypatch):
    """300 hits of one read, five waves of one tile size: the trace budget set to five, three and two tiles
    gives 1, 2 and 3 launches whose boundaries lie inside the read's hits; the results do not change."""
    s = acgt.s
    m = 40
    read = edited(s[500:500 + m], [("sub", 11)], b"ACGT")
    per = [[(0, 8)], [(q + 400, q + 400 + m + (-1, 0, 1)[q % 3]) for q in range(300)], [(9, 18)]]
    flat = [w for ws in per for w in ws]
    for q in range(0, len(flat), 64):   # every wave holds a window of m + 1 bytes: m + 2 rows of 64 words of 4 bytes
        assert max(e - b for b, e in flat[q:q + 64]) == m + 1
    reads = [s[0:8], read, s[9:18]]
    # (the first and the last read's single hits share the outer waves: 302 hits, tiles of m + 2 rows all the same)
    tile = 64 * (m + 2) * 4
    monkeypatch.delenv("GX_EXTEND_TRACE_BYTES", raising=False)
    whole = acgt.check(reads, as_hits(per), DEFAULT, 1, chunks=1)
    for tiles, chunks in ((5, 1), (3, 2), (2, 3), (1, 5)):
        monkeypatch.setenv("GX_EXTEND_TRACE_BYTES", str(tiles * tile))
        r = acgt.check(reads, as_hits(per), DEFAULT, 1, chunks=chunks)
        same_extend(r, whole)
        assert gx.extend_info(acgt.ctx)["trace_bytes"] == min(tiles, 5) * tile
    monkeypatch.setenv("GX_EXTEND_TRACE_BYTES", "1")   # below one tile: a wave a launch
    same_extend(acgt.check(reads, as_hits(per), DEFAULT, 1, cigars=False, chunks=5), acgt.host.extend(reads, as_hits(per), band=1, cigars=False))
    # the 8-byte words of B = 9: the same hits take twice the bytes
    monkeypatch.setenv("GX_EXTEND_TRACE_BYTES", str(3 * tile))
    acgt.check(reads, as_hits(per), DEFAULT, 9, chunks=5)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_refusal(gx, ctx, case):
    cid, over = case
    idx = gx.SuffixIndex(TEXT, ctx=ctx)
    rc, text = run_case(gx, idx, over)
    ok = run_case(gx, idx, {})   # and the index goes on working
    idx.close()
    assert (rc, text) == (WANT[cid]["rc"], WANT[cid]["text"])
    assert ok[0] == 0


def test_limits_and_ecap_on_device(gx, ctx):
    idx = gx.SuffixIndex(TEXT, ctx=ctx)
    limits(gx, idx)
    info = gx.extend_info(ctx)
    assert info["hits"] == 1 and info["fill_ms"] > 0
    idx.close()


def test_python_repeats_after_ecap_on_device(gx, acgt, monkeypatch):
    monkeypatch.setattr(gx, "_FIRST_RUNS", 2)
    reads, hits = unrelated_hits(acgt.s, 2, 78, count=70)
    r = acgt.check(reads, hits, (2, -1, -1, 0), 2)
    assert len(r["cigar"]) > 2 * 70   # (the first capacity was too small)


def test_alternating_with_the_searches(gx, ctx, acgt):
    from match_check import check_mems
    s = acgt.s
    reads = [edited(s[i:i + 30], [(KINDS[i % 3], i % 30)], b"ACGT") for i in range(100, 2100, 100)]
    long_query = [s[300:420] + b"T" + s[900:1000]]
    first = None
    for _ in range(2):
        found = acgt.dev.search_edit(reads, 2, max_hits=4)
        r = acgt.check(reads, found, DEFAULT, 2)
        check_mems(s, long_query, 20, acgt.dev.mems(long_query, 20))
        again = acgt.check(reads, found, DEFAULT, 3)
        assert np.array_equal(r["score"], again["score"])   # (every path was inside the band of 2 already)
        if first is not None:
            same_extend(r, first)
        first = r


def test_map_reads_is_its_two_calls(gx, ctx, acgt):
    s = acgt.s
    reads = [edited(s[i:i + 50], [(KINDS[i % 3], i % 50), ("sub", (i // 7) % 50)], b"ACGT") for i in range(0, 3000, 150)]
    found, ext = acgt.dev.map_reads(reads, 2, max_hits=4, scores=gx.Scores(2, -3, -1, -4))
    again = acgt.dev.search_edit(reads, 2, max_hits=4)
    for f in ("count", "best_dist", "best_end", "ends", "distances", "starts", "hit_offsets"):
        assert np.array_equal(found[f], again[f]), f
    same_extend(ext, acgt.dev.extend(reads, again, gx.Scores(2, -3, -1, -4), band=2))
    check_extend(s, reads, found, (2, -3, -1, -4), 2, ext)
    assert gx.extend_info(ctx)["hits"] == len(found["ends"]) > 0


def test_cli_with_and_without_cigar(gx, ctx, acgt, tmp_path):
    s = acgt.s
    reads = [edited(s[i:i + 40], [(KINDS[i % 3], i % 40)] if i % 200 else [], b"ACGT") for i in range(0, 4000, 100)]
    found, ext = acgt.dev.map_reads(reads, 2, max_hits=16)
    genome, fa, plain, tsv = tmp_path / "genome.fasta", tmp_path / "reads.fasta", tmp_path / "plain.tsv", tmp_path / "cigar.tsv"
    genome.write_bytes(b">g\n" + s + b"\n")
    fa.write_bytes(b"".join(b">read%d\n%s\n" % (q, p) for q, p in enumerate(reads)))
    base = [CLI, "-c", os.path.join(GOLDEN, "config.toml"), "search", "-f", str(genome), "-p", str(fa), "--max-hits", "16", "-e", "2"]
    env = dict(os.environ, GX_LOG="warn")
    subprocess.run(base + ["-o", str(plain)], check=True, timeout=120, env=env)
    subprocess.run(base + ["--cigar", "-o", str(tsv)], check=True, timeout=120, env=env)
    ho = found["hit_offsets"].astype(np.int64)
    for with_cigar, path in ((False, plain), (True, tsv)):
        lines = path.read_text().split("\n")
        assert lines[-1] == "" and len(lines) == len(reads) + 1
        for q, line in enumerate(lines[:-1]):
            trip = []
            for h in range(ho[q], ho[q + 1]):
                t = f"{found['starts'][h]}-{found['ends'][h]}:{found['distances'][h]}"
                trip.append(t + f":{ext['score'][h]}:{gx.cigar_string(hit_runs(ext, h))}" if with_cigar else t)
            assert line == "\t".join([f"read{q}", str(len(reads[q])), str(found["count"][q]), str(found["best_dist"][q]),
                                      str(found["best_end"][q]), ",".join(trip)]), (q, with_cigar)
    bad = subprocess.run(base[:-2] + ["--cigar"], capture_output=True, timeout=60)
    assert bad.returncode == 2   # --cigar without -e
    bad = subprocess.run(base[:-2] + ["-k", "1", "--cigar"], capture_output=True, timeout=60)
    assert bad.returncode == 2
