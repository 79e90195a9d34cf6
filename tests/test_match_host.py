"""Matching statistics and maximal exact matches on the host index (ctx = NULL,
DESIGN.md 21): every content case of the GPU suite (tests/test_gpu_match.py
imports them from here) against the brute force of tests/match_check.py, the
error table, the GX_ECAP protocol, the candidate budget and the 64-bit candidate
total.  No GPU."""
import time

import numpy as np
import pytest

import gxamd
from match_check import brute_mems, check_mems, check_stats, same_mems, same_stats
from test_approx_host import other
from test_suffix_host import BYTES_219, np_rand

EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)
ALPHABETS = {"x40x41": b"\x40\x41", "x7fx80": b"\x7f\x80", "bytes219": BYTES_219}
BIG = 100000   # a max_len above every length here
TILE = gxamd.suffix_tile()[0]   # items per workgroup of the scans (2048)


def sep_of(alpha: bytes) -> int:
    """A query byte that is not in a two-letter alphabet (any admitted byte is in BYTES_219)."""
    return alpha[-1] + 1 if len(alpha) < 200 else 0x25


def edge_queries(s: bytes, L: int, alpha: bytes):
    """64 queries: b separator bytes, then the text from 100 + a of length L - 1, L or L + 1, then one byte
    that differs from the text's next: the planted match starts and ends at every alignment mod 8 in the text
    (a) and, the queries being staged back to back, in the query buffer."""
    sep, out = sep_of(alpha), []
    for a in range(8):
        for b in range(8):
            ln = L + (a + b) % 3 - 1
            i = 100 + a
            out.append(bytes([sep]) * b + s[i:i + ln] + bytes([other(s[i + ln], alpha)]))
    return out


def mutate(q: bytes, every: int, alpha: bytes) -> bytes:
    p = bytearray(q)
    for k in range(every // 2, len(p), every):
        p[k] = other(p[k], alpha)
    return bytes(p)


def content_cases():
    """[(id, text, queries, min_lens, max_lens)]: the smallest shapes that can go wrong."""
    out = []
    # word edges
    for name, alpha in ALPHABETS.items():
        s = np_rand(2100 + len(alpha), alpha, 400)
        for L in EDGES:
            out.append((f"edge-{name}-{L}", s, edge_queries(s, L, alpha), (L,), (L,)))
    # ends
    s = np_rand(2121, b"ACGT", 500)
    out.append(("ends", s, [s[:40] + b"N", b"N" + s[460:], s[:40], s[460:], s, s + s[:100] + b"TTTT", s[5:24], b"",
                            b"N", s[499:] + s[:1]], (20,), (64, BIG)))
    for n in (1, 2, 7, 8, 9):
        t = b"ACGTACGTA"[:n]
        out.append((f"tiny-{n}", t, [t, t + t, b"A", b"", t[1:], b"N" + t, t + b"N"], (1, 2), (1, 8, BIG)))
    out.append(("empty-text", b"", [b"ACGT", b"", b"A"], (1,), (1, 8)))
    # query boundaries: consecutive chunks of the text, so a match would run on into the next query (and its
    # last word reads into it) and back into the one before if the boundaries were ignored
    s = np_rand(2122, b"ACGT", 400)
    for B in (7, 8, 9, 63, 64, 65):
        qs = [s[100:100 + B], s[100 + B:100 + 2 * B], s[100 + 2 * B:100 + 3 * B - 3], b"", s[97 + 3 * B:110 + 3 * B]]
        out.append((f"boundary-{B}", s, qs, (4, 8), (8, 200)))
    # maximality
    s = np_rand(2123, b"ACGT", 600)
    rep = s[200:260]
    t = s[:300] + rep + s[300:450] + rep[10:] + s[450:]                  # overlapping MEMs on different diagonals
    one = s[50:90] + bytes([other(s[90], b"ACGT")]) + s[91:130]          # two MEMs on one diagonal
    out.append(("maximal", t, [one, rep, s[190:270], mutate(s[300:420], 16, b"ACGT")], (8, 20), (16, BIG)))
    out.append(("periodic", b"ACGT" * 1250, [b"ACGT" * 5 + b"A", b"GTAC" * 4 + b"GG", b"ACGA"], (4, 9), (8, 64)))
    # batch shapes: total positions around the wave and the workgroup
    s = np_rand(2124, b"ACGT", 800)
    for total in (63, 64, 65, 255, 256, 257):
        a, b = total // 3, total // 2
        qs = [mutate(s[10:10 + a], 11, b"ACGT"), s[300:300 + b], mutate(s[500:500 + total - a - b], 7, b"ACGT")]
        out.append((f"positions-{total}", s, qs, (6,), (32,)))
    # candidate and kept totals just inside, at and one over the scan tile: A^n against A at min_len 1 has n
    # candidates, all kept
    for n in (TILE - 1, TILE, TILE + 1):
        out.append((f"tile-{n}", b"A" * n, [b"C", b"A", b"CC"], (1,), (4,)))
    # one position with thousands of candidates between positions with none
    t = b"G" * 3000 + np_rand(2125, b"ACT", 400)
    out.append(("skewed", t, [b"NNNN" + b"G" * 8 + b"NNNN", b"N" * 30], (8,), (8,)))
    return out


CASES = content_cases()
IDS = [c[0] for c in CASES]


def run_case(idx, s, queries, min_lens, max_lens, sa=None):
    """Every call of a case on idx against the brute force; returns the results for a comparison partner."""
    sa = idx.sa() if sa is None else sa
    res = []
    for W in max_lens:
        r = idx.matching_stats(queries, max_len=W)
        check_stats(s, queries, W, r, sa)
        res.append(r)
    for L in min_lens:
        r = idx.mems(queries, L)
        check_mems(s, queries, L, r)
        counts = idx.mems(queries, L, max_mems=0)
        assert np.array_equal(counts["mem_offsets"], r["mem_offsets"])
        assert np.array_equal(counts["candidates"], r["candidates"]) and len(counts["qpos"]) == 0
        res.append(r)
    return res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_content(gx, case):
    _, s, queries, min_lens, max_lens = case
    idx = gx.SuffixIndex(s, host=True)
    run_case(idx, s, queries, min_lens, max_lens)
    idx.close()


def unary_counts(idx, n=5000, L=5):
    """A^n against A^20, A^19 C and C A^19 at min_len L, in closed form.  A pair of the run A^r of a query is a
    MEM iff it starts at text 0 or at the run's first byte: n - L + 1 text starts with the whole run (the last
    ones cut by the text's end), and r - L later starts in the run against text 0.  Candidates: every pair of
    an L-mer of the run and an L-mer of the text."""
    r = idx.mems([b"A" * 20, b"A" * 19 + b"C", b"C" + b"A" * 19], L)
    tstarts = n - L + 1
    assert np.diff(r["mem_offsets"].astype(np.int64)).tolist() == [tstarts + 20 - L, tstarts + 19 - L, tstarts + 19 - L]
    assert r["candidates"].tolist() == [(20 - L + 1) * tstarts, (19 - L + 1) * tstarts, (19 - L + 1) * tstarts]
    assert (r["length"][:tstarts - 15] == 20).all() and r["qpos"][:tstarts].max() == 0
    return r


def test_host_unary_closed_form(gx):
    s = b"A" * 5000
    idx = gx.SuffixIndex(s, host=True)
    r = unary_counts(idx)
    check_mems(s, [b"A" * 20, b"A" * 19 + b"C", b"C" + b"A" * 19], 5, r)
    idx.close()


def raw_mems(gx, idx, packed: bytes, off, min_len, cap, want_mems=True, want_cand=True, moff_null=False):
    buf = np.frombuffer(packed, np.uint8) if packed else np.zeros(1, np.uint8)
    off = np.asarray(off, np.uint64)
    nq = len(off) - 1
    mem = np.full(max(cap, 1) * 3, 0xDEADBEEF, np.uint32)
    moff = np.full(nq + 1, 0xABCDABCD, np.uint64)
    cand = np.full(max(nq, 1), 0xABCDABCD, np.uint64)
    rc = gx.lib().gx_suffix_index_mems(idx.ptr, buf.ctypes.data, off.ctypes.data, nq, min_len,
                                       mem.ctypes.data if want_mems else None, cap,
                                       None if moff_null else moff.ctypes.data, cand.ctypes.data if want_cand else None)
    return rc, mem, moff, cand


def raw_stats(gx, idx, packed: bytes, off, max_len, null=False):
    buf = np.frombuffer(packed, np.uint8) if packed else np.zeros(1, np.uint8)
    off = np.asarray(off, np.uint64)
    st = np.zeros(max(len(packed), 1) * 4, np.uint32)   # (a refused batch's offsets may name more)
    return gx.lib().gx_suffix_index_match_stats(idx.ptr, buf.ctypes.data, off.ctypes.data, len(off) - 1, max_len,
                                                None if null else st.ctypes.data)


def error_table(gx, idx):
    """On an index of BANANA."""
    err = lambda: gx.lib().gx_last_error()
    assert raw_stats(gx, idx, b"ANA", [0, 3], 0) == 1 and b"max_len" in err()
    assert raw_stats(gx, idx, b"ANA", [0, 3], 4, null=True) == 1
    assert raw_stats(gx, idx, b"ANA", [1, 3], 4) == 1
    assert raw_stats(gx, idx, b"ANANA", [0, 4, 2], 4) == 1 and b"offsets decrease at query 1" in err()
    assert raw_stats(gx, idx, b"ANAB$A", [0, 3, 6], 4) == 1 and b"query 1: byte 36 at offset 1" in err()
    assert raw_stats(gx, idx, b"ANA\x00", [0, 4], 4) == 1 and b"query 0: byte 0 at offset 3" in err()
    assert raw_mems(gx, idx, b"ANA", [0, 3], 0, 8)[0] == 1 and b"min_len" in err()
    assert raw_mems(gx, idx, b"ANA", [0, 3], 2, 8, moff_null=True)[0] == 1
    assert raw_mems(gx, idx, b"ANA", [1, 3], 2, 8)[0] == 1
    assert raw_mems(gx, idx, b"AN$", [0, 3], 2, 8)[0] == 1 and b"query 0: byte 36 at offset 2" in err()
    # the 32-bit device offsets: refused from the offsets alone, before a byte is read
    for f in (lambda o: raw_stats(gx, idx, b"A", o, 4), lambda o: raw_mems(gx, idx, b"A", o, 2, 8)[0]):
        assert f([0, (1 << 32) - 16]) == 3 and b"2^32" in err()
    # and the index goes on working
    rc, mem, moff, cand = raw_mems(gx, idx, b"ANA", [0, 3], 2, 8)
    assert rc == 0 and moff.tolist() == [0, 2] and mem[:6].tolist() == [0, 1, 3, 0, 3, 3] and cand.tolist() == [4]


def test_host_error_table(gx):
    idx = gx.SuffixIndex(b"BANANA", host=True)
    error_table(gx, idx)
    idx.close()


def ecap_protocol(gx, idx):
    """BANANA at min_len 2.  ANA: (0, 1, 3) and (0, 3, 3); the inner pairs extend to the left.  NAB: NA at 2
    and 4, both left-maximal at query 0 -> (0, 2, 2), (0, 4, 2); AB nowhere.  XX: nothing."""
    packed, off = b"ANA" + b"NAB" + b"XX", [0, 3, 6, 8]
    rc, mem, moff, cand = raw_mems(gx, idx, packed, off, 2, 3)
    assert rc == 7 and b"4 MEMs needed" in gx.lib().gx_last_error()
    assert moff.tolist() == [0, 2, 4, 4] and cand.tolist() == [4, 2, 0]   # complete
    assert (mem == 0xDEADBEEF).all()                                      # untouched
    rc, mem, moff, cand = raw_mems(gx, idx, packed, off, 2, int(moff[-1]))   # allocate and repeat
    assert rc == 0 and mem.tolist() == [0, 1, 3, 0, 3, 3, 0, 2, 2, 0, 4, 2] and moff.tolist() == [0, 2, 4, 4]
    assert raw_mems(gx, idx, packed, off, 2, 0)[0] == 7
    rc, mem, moff, cand = raw_mems(gx, idx, packed, off, 2, 0, want_mems=False, want_cand=False)   # counts only
    assert rc == 0 and moff.tolist() == [0, 2, 4, 4]
    r = idx.mems([b"ANA", b"NAB", b"XX"], 2, max_mems=4)
    assert r["tpos"].tolist() == [1, 3, 2, 4]
    with pytest.raises(gx.GxError) as e:
        idx.mems([b"ANA", b"NAB", b"XX"], 2, max_mems=3)
    assert e.value.code == 7


def test_host_ecap_protocol(gx):
    idx = gx.SuffixIndex(b"BANANA", host=True)
    ecap_protocol(gx, idx)
    idx.close()


def budget_case(gx, idx, s, monkeypatch):
    """idx on s = A^300 + C^300: the candidates of [A^10, C^10 A, G^5] at min_len 4 are 7 * 297, 7 * 297 and 0.
    A budget one below refuses and writes candidates[] alone; the budget itself admits."""
    packed, off = b"A" * 10 + b"C" * 10 + b"A" + b"G" * 5, [0, 10, 21, 26]
    want = [7 * 297, 7 * 297, 0]
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", str(sum(want) - 1))
    rc, mem, moff, cand = raw_mems(gx, idx, packed, off, 4, 1 << 14)
    assert rc == 3 and f"{sum(want)} candidate pairs".encode() in gx.lib().gx_last_error()
    assert cand.tolist() == want
    assert (moff == 0xABCDABCD).all() and (mem == 0xDEADBEEF).all()   # nothing else is written
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", str(sum(want)))       # read on every call
    queries = [packed[off[c]:off[c + 1]] for c in range(3)]
    r = idx.mems(queries, 4)
    check_mems(s, queries, 4, r)
    monkeypatch.delenv("GX_APPROX_CAND_BUDGET")
    check_stats(s, queries, 6, idx.matching_stats(queries, max_len=6), idx.sa())   # (no budget: no candidates)
    return r


def test_host_budget(gx, monkeypatch):
    s = b"A" * 300 + b"C" * 300
    idx = gx.SuffixIndex(s, host=True)
    budget_case(gx, idx, s, monkeypatch)
    idx.close()


WRAP_M = 860001


def wrap_case(gx, idx, monkeypatch):
    """A^5000 and the query A^860,001 at min_len 1: 4,300,005,000 candidates.  Cut to 32 bits that is 5,037,704,
    inside the default budget: the total must be held in 64 bits, before a 32-bit scan is relied upon."""
    monkeypatch.delenv("GX_APPROX_CAND_BUDGET", raising=False)
    total = WRAP_M * 5000
    assert total > 1 << 32 and total % (1 << 32) == 5037704 < 1 << 27
    q = (np.full(WRAP_M, 0x41, np.uint8), np.array([0, WRAP_M], np.uint64))
    t0 = time.perf_counter()
    with pytest.raises(gx.GxError) as e:
        idx.mems(q, 1, max_mems=0)
    dt = time.perf_counter() - t0
    print(f"wrap case refused in {dt * 1e3:.1f} ms")
    assert e.value.code == 3 and f"{total} candidate pairs" in str(e.value)
    rc, mem, moff, cand = raw_mems(gx, idx, b"A" * WRAP_M, [0, WRAP_M], 1, 16)
    assert rc == 3 and cand.tolist() == [total] and (moff == 0xABCDABCD).all()
    r = idx.mems([b"AAAC"], 3)                                   # and the index goes on working
    assert r["mem_offsets"].tolist() == [0, 4998] and r["candidates"].tolist() == [4998]
    return dt


def test_host_wrap_case(gx, monkeypatch):
    idx = gx.SuffixIndex(b"A" * 5000, host=True)
    wrap_case(gx, idx, monkeypatch)   # (refused with mem_offsets untouched: nothing of the 4.3e9 is examined)
    idx.close()


def test_host_stats_against_search(gx):
    """Where the whole window occurs, lo and count are the exact search's of that window; len is prefix_len
    everywhere."""
    s = np_rand(2130, b"ACGT", 1500)
    idx = gx.SuffixIndex(s, host=True)
    q = mutate(s[200:500], 37, b"ACGT")
    for W in (5, 12, 300):
        r = idx.matching_stats([q], max_len=W)
        wins = [q[j:j + W] for j in range(len(q))]
        h = idx.search(wins)
        assert np.array_equal(r["len"], h["prefix_len"])
        whole = r["len"] == np.array([len(w) for w in wins])
        assert whole.any() and np.array_equal(r["lo"][whole], h["lo"][whole])
        assert np.array_equal(r["count"][whole], h["count"][whole])
    idx.close()
