"""gx_suffix_index_extend on the host index (no device): banded affine-gap alignment and CIGARs
of reported hits.

  the checker   tests/extend_check.py with a band that holds the whole table is oracle.align(window, pattern):
                score, the four statistics, n_steps and every move
  the host      every hit of every case below against the checker, on every field and every run
  the oracle    hits of the host edit search on a 5,000-base text with up to k planted edits at B = k: wherever
                the oracle's retrace path stays inside the band the host result is the oracle's, exactly; at
                most 5 % of the hits may lie outside, so that the clause cannot go empty unnoticed
  the band      unrelated pairs at B = |w - m|: the checker's result, never above the oracle's score, and
                strictly below it at least once
  refusals      every text and the order of the checks against tests/golden/extend_error_texts.json, the
                GX_ECAP protocol, cigar = NULL
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from extend_check import (FIELDS, banded, check_extend, hit_record, hit_runs, hits_of, in_band, oracle_record,
                          oracle_runs, oracle_steps)
from extend_error_cases import TEXT, cases, run_case
from test_edit_host import edited, random_edits
from test_suffix_host import np_rand

SCORE_SETS = [(1, -2, -1, -5), (2, -1, -1, 0), (1, -1, -3, -1), (5, -4, -2, -10), (0, -3, -2, -4)]

with open(os.path.join(GOLDEN, "extend_error_texts.json")) as f:
    WANT = json.load(f)
CASES = cases()


@pytest.mark.parametrize("alpha", [b"A", b"AC", b"ACGT"], ids=["A", "AC", "ACGT"])
def test_checker_is_the_oracle_when_the_band_holds_the_table(oracle, alpha):
    rng = np.random.default_rng(len(alpha))
    for case in range(150):
        w, m = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        s1, s2 = np_rand(7000 * len(alpha) + case, alpha, w), np_rand(9000 * len(alpha) + case, alpha, m)
        if case % 3 == 0 and w > 4:   # related pairs too: s2 is s1 with a few edits
            s2 = edited(s1, random_edits(rng, w, min(3, w)), b"ACGT")
            m = len(s2)
        scores = SCORE_SETS[case % len(SCORE_SETS)]
        o = oracle.align(s1, s2, scores)
        rec, runs, steps = banded(s1, s2, scores, max(w, m))
        assert rec == oracle_record(o, s1, s2), (s1, s2, scores)
        assert steps == oracle_steps(o), (s1, s2, scores)
        assert runs == oracle_runs(o)
        assert sum(r >> 4 for r in runs) == len(steps) and all((r & 15) < 3 for r in runs)


def planted_reads(s: bytes, nreads: int, m: int, k: int, seed: int):
    """Reads of about m bases cut from s, read r with r % (k + 1) edits of every kind."""
    rng = np.random.default_rng(seed)
    reads = []
    for r in range(nreads):
        i = int(rng.integers(0, len(s) - m + 1))
        reads.append(edited(s[i:i + m], random_edits(rng, m, r % (k + 1)), b"ACGT"))
    return [P for P in reads if len(P) >= k + 1]


@pytest.fixture(scope="module")
def text5000(gx):
    s = np_rand(2200, b"ACGT", 5000)
    idx = gx.SuffixIndex(s, host=True)
    yield s, idx
    idx.close()


@pytest.mark.parametrize("k", [0, 1, 2, 3, 8])
def test_oracle_clause(gx, oracle, text5000, k):
    s, idx = text5000
    reads = planted_reads(s, 40, 48, k, 100 + k)
    found = idx.search_edit(reads, k, max_hits=16)
    inside = outside = 0
    for scores in SCORE_SETS[:4]:
        r = idx.extend(reads, found, gx.Scores(*scores), band=k)
        assert check_extend(s, reads, found, scores, k, r) == len(found["ends"]) > 0
        for h, p, b, e in hits_of(reads, found):
            o = oracle.align(s[b:e], reads[p], scores)
            assert int(r["score"][h]) <= o.score
            if not in_band(o, k):
                outside += 1
                continue
            inside += 1
            assert hit_record(r, h) == oracle_record(o, s[b:e], reads[p]), (h, p, b, e, scores)
            assert hit_runs(r, h) == oracle_runs(o), (h, p, b, e, scores)
    print(f"k {k}: {inside} hits with the oracle's path inside the band, {outside} outside")
    assert inside > 0 and outside <= 0.05 * (inside + outside)


def unrelated_hits(s: bytes, B: int, seed: int, count: int = 24):
    """Reads that have nothing to do with their windows: (reads, hits) with w - m in {-B, 0, B}."""
    rng = np.random.default_rng(seed)
    reads, starts, ends = [], [], []
    for q in range(count):
        m = int(rng.integers(max(B, 1), 33))
        w = m + (-B, 0, B)[q % 3]
        b = int(rng.integers(0, len(s) - w + 1))
        reads.append(np_rand(seed * 1000 + q, b"ACGT", m))
        starts.append(b)
        ends.append(b + w)
    hits = {"hit_offsets": np.arange(count + 1, dtype=np.uint64), "starts": np.array(starts, np.uint32),
            "ends": np.array(ends, np.uint32)}
    return reads, hits


def test_band_binds(gx, oracle, text5000):
    s, idx = text5000
    lower = 0
    for B in (0, 1, 2, 5):
        reads, hits = unrelated_hits(s, B, 300 + B)
        for scores in SCORE_SETS[:4]:
            r = idx.extend(reads, hits, gx.Scores(*scores), band=B)
            check_extend(s, reads, hits, scores, B, r)
            same = idx.extend(reads, hits, gx.Scores(*scores))   # band=None: the largest |w - m|
            assert all(np.array_equal(r[f], same[f]) for f in FIELDS)
            for h, p, b, e in hits_of(reads, hits):
                o = oracle.align(s[b:e], reads[p], scores)
                assert int(r["score"][h]) <= o.score
                lower += int(r["score"][h]) < o.score
    print(f"{lower} hits score strictly below the oracle")
    assert lower > 0


def test_shapes_by_hand(gx):
    idx = gx.SuffixIndex(b"ACGTACGTTTGACA", host=True)
    hits = {"hit_offsets": [0, 1, 2, 3, 4], "starts": [0, 0, 0, 8], "ends": [8, 8, 7, 14]}
    reads = [b"ACGTACGT", b"ACGACGT", b"ACGTTACG", b"TTGGACA"]
    r = idx.extend(reads, hits, gx.Scores(1, -2, -1, -5), band=1)
    # an exact window; a text byte the read lacks (D); a read byte the text lacks (I), twice; a gap costs h + g = -6
    assert [gx.cigar_string(hit_runs_np(r, h)) for h in range(4)] == ["8M", "3M1D4M", "3M1I4M", "2M1I4M"]
    assert r["score"].tolist() == [8, 1, 1, 0] and r["identities"].tolist() == [8, 7, 7, 6]
    assert r["opening_gaps"].tolist() == [0, 1, 1, 1] and r["n_steps"].tolist() == [8, 8, 8, 7]
    check_extend(b"ACGTACGTTTGACA", reads, {k: np.asarray(v) for k, v in hits.items()}, (1, -2, -1, -5), 1, r)
    idx.close()


def hit_runs_np(r, h):
    return r["cigar"][int(r["cigar_offsets"][h]):int(r["cigar_offsets"][h + 1])]


def test_cigar_string(gx):
    assert gx.cigar_string(np.array([57 << 4, 1 << 4 | 1, 42 << 4, 3 << 4 | 2], np.uint32)) == "57M1I42M3D"
    assert gx.cigar_string([]) == ""


def test_empty_batches_and_counts_only(gx, text5000):
    s, idx = text5000
    r = idx.extend([], {"hit_offsets": [0], "starts": [], "ends": []})
    assert r["score"].tolist() == [] and r["cigar_offsets"].tolist() == [0] and r["cigar"].tolist() == []
    reads = [s[10:40], b"GGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGG", s[100:120]]   # a read without a hit between two with one
    found = idx.search_edit(reads, 1, max_hits=4)
    assert np.diff(found["hit_offsets"]).tolist()[1] == 0
    a = idx.extend(reads, found, band=1)
    b = idx.extend(reads, found, band=1, cigars=False)
    check_extend(s, reads, found, (1, -2, -1, -5), 1, a)
    check_extend(s, reads, found, (1, -2, -1, -5), 1, b, cigars=False)
    both = idx.map_reads(reads, 1, max_hits=4)
    assert all(np.array_equal(both[0][f], found[f]) for f in ("ends", "starts", "distances", "hit_offsets"))
    assert all(np.array_equal(both[1][f], a[f]) for f in FIELDS + ("cigar", "cigar_offsets"))


def test_python_repeats_after_ecap(gx, text5000, monkeypatch):
    """A first capacity of two runs a hit is too small for unrelated pairs: the second call takes the total."""
    monkeypatch.setattr(gx, "_FIRST_RUNS", 2)
    s, idx = text5000
    reads, hits = unrelated_hits(s, 2, 77, count=12)
    r = idx.extend(reads, hits, gx.Scores(2, -1, -1, 0), band=2)
    assert len(r["cigar"]) > 2 * 12
    check_extend(s, reads, hits, (2, -1, -1, 0), 2, r)


def test_fixture_covers_every_case():
    assert sorted(WANT) == sorted(c[0] for c in CASES) and len(WANT) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_refusal(gx, case):
    cid, over = case
    idx = gx.SuffixIndex(TEXT, host=True)
    rc, text = run_case(gx, idx, over)
    idx.close()
    assert (rc, text) == (WANT[cid]["rc"], WANT[cid]["text"])


def limits(gx, idx):
    """The last admitted value beside every first refused one, and the GX_ECAP protocol.  idx: TEXT."""
    assert run_case(gx, idx, {})[0] == 0
    assert run_case(gx, idx, {"band": 15})[0] == 0
    assert run_case(gx, idx, {"scores": (32767, -32767, -32767, -32767)})[0] == 0
    assert run_case(gx, idx, {"starts": [0], "ends": [5]})[0] == 0 and run_case(gx, idx, {"starts": [4], "ends": [8]})[0] == 0
    assert run_case(gx, idx, {"hoff": [0, 0], "null": {"starts", "ends", "out", "patterns"}, "off": [0, 0]})[0] == 0
    # GX_ECAP: out[] and cigar_offsets[] complete, cigar[] untouched; then allocate and repeat
    over = dict(dict(CASES)["ecap"])
    got = {}
    assert run_case(gx, idx, over, got)[0] == 7
    rec, runs, _ = banded(TEXT[0:7], b"ACTACG", (1, -2, -1, -5), 1)
    assert {f: int(got["out"][f][0]) for f in FIELDS} == rec and got["cigar_offsets"].tolist() == [0, 3] == [0, len(runs)]
    assert (got["cigar"] == 0xDEADBEEF).all()
    over["cap"] = 3
    assert run_case(gx, idx, over, got)[0] == 0 and got["cigar"].tolist() == runs
    over["null"] = {"cigar"}   # cigar = NULL: the records and the offsets alone, whatever the capacity says
    over["cap"] = 0
    assert run_case(gx, idx, over, got)[0] == 0 and got["cigar_offsets"].tolist() == [0, 3]
    assert {f: int(got["out"][f][0]) for f in FIELDS} == rec


def test_host_limits_and_ecap(gx):
    idx = gx.SuffixIndex(TEXT, host=True)
    limits(gx, idx)
    assert gx.lib().gx_extend_info(None, None, None, None, None, None, None) == 1   # (it reports a context's last call)
    idx.close()
