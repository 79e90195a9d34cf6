"""Approximate search on the host index (no device): gx_suffix_index_search_approx
with ctx = NULL against the brute force of tests/approx_check.py, on 200 random
strings over four alphabets with k = 0..3 and 0..k+1 planted substitutions,
every max_hits edge, the GX_ECAP protocol, every new error code at its first
refused value, the 64-bit candidate total (the wrap case), k = 0 against the
exact search, the empty text, and BANANA by hand."""
import time

import numpy as np
import pytest

from approx_check import ALL_HITS, NO_DIST, brute, check_approx
from test_suffix_host import BYTES_219, np_rand

ALPHABETS = [b"A", b"AC", b"ACGT", BYTES_219]


def other(c: int, alpha: bytes) -> int:
    """A byte that differs from c: the next letter of the alphabet, or one outside a unary alphabet."""
    return alpha[(alpha.index(c) + 1) % len(alpha)] if len(alpha) > 1 else c + 1


def planted(s: bytes, i: int, m: int, cols, alpha: bytes) -> bytes:
    p = bytearray(s[i:i + m])
    for c in cols:
        p[c] = other(p[c], alpha)
    return bytes(p)


def patterns_for(s: bytes, k: int, alpha: bytes, rng):
    """[(pattern, origin, planted substitutions)]: cut at the start, the middle and the very end of the text,
    with 0 .. k + 1 substitutions at random columns."""
    n, out = len(s), []
    for m in (k + 1, k + 2, 8, 9, 17, 40):
        if m > n or m < k + 1:
            continue
        for i in (0, int(rng.integers(0, n - m + 1)), n - m):
            for subs in range(0, k + 2):
                if subs > m:
                    continue
                cols = rng.choice(m, subs, replace=False).tolist()
                out.append((planted(s, i, m, cols, alpha), i, subs))
    return out


@pytest.mark.parametrize("alpha", ALPHABETS, ids=["A", "AC", "ACGT", "bytes219"])
def test_host_brute_force(gx, alpha):
    rng = np.random.default_rng(len(alpha))
    for case in range(50):
        n = int(rng.integers(1, 301))
        s = np_rand(2000 * len(alpha) + case, alpha, n)
        idx = gx.SuffixIndex(s, host=True)
        for k in range(4):
            trip = patterns_for(s, k, alpha, rng)
            if not trip:
                continue
            pats = [t[0] for t in trip]
            r = idx.search_approx(pats, k, max_hits=ALL_HITS)
            check_approx(s, pats, k, r, ALL_HITS)
            check_approx(s, pats, k, idx.search_approx(pats, k), 0)
            check_approx(s, pats, k, idx.search_approx(pats, k, max_hits=2), 2)
            for p, (P, origin, subs) in enumerate(trip):
                seg = dict(zip(r["positions"][int(r["hit_offsets"][p]):int(r["hit_offsets"][p + 1])].tolist(),
                               r["distances"][int(r["hit_offsets"][p]):int(r["hit_offsets"][p + 1])].tolist()))
                if subs <= k:
                    assert seg.get(origin) == subs, (s, P, k, origin, subs)   # found, with exactly that distance
                else:
                    assert origin not in seg, (s, P, k, origin)               # k + 1 substitutions: not at its origin
        idx.close()


def test_host_empty_text(gx):
    idx = gx.SuffixIndex(b"", host=True)
    for k in (0, 1, 3):
        pats = [b"A" * (k + 1), b"ACGTACGTAC"]
        r = idx.search_approx(pats, k, max_hits=ALL_HITS)
        check_approx(b"", pats, k, r, ALL_HITS)
        assert r["count"].tolist() == [0, 0] and r["best_dist"].tolist() == [NO_DIST] * 2
        assert r["positions"].tolist() == [] and r["hit_offsets"].tolist() == [0, 0, 0]
    assert idx.search_approx([], 2)["count"].tolist() == []
    idx.close()


def test_host_max_hits_edges(gx):
    s = np_rand(78, b"AC", 300)
    idx = gx.SuffixIndex(s, host=True)
    pats = [b"ACAC", b"CCAA", b"ACACACAC", s[10:30], b"AAAAAAAA", b"GGGG"]
    for k in (1, 2):
        count = brute(s, b"ACAC", k)[0]
        assert count > 3
        for mh in (0, 1, count - 1, count, count + 1, ALL_HITS):
            check_approx(s, pats, k, idx.search_approx(pats, k, max_hits=mh), mh)
    idx.close()


def raw_approx(gx, idx, packed: bytes, offsets, k, max_hits, cap, want_positions=True):
    """gx_suffix_index_search_approx as the C caller sees it: (rc, hits, positions, distances, hit_offsets)."""
    off = np.asarray(offsets, np.uint64)
    npat = len(off) - 1
    pk = np.frombuffer(packed, np.uint8) if len(packed) else np.zeros(1, np.uint8)
    hits = np.full(max(npat, 1), 0xABABABAB, np.uint32).repeat(4).view(gx.APPROX_HIT_DTYPE)
    pos = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    dst = np.full(max(cap, 1), 0xEE, np.uint8)
    hoff = np.full(npat + 1, 0xDEAD, np.uint64)
    rc = gx.lib().gx_suffix_index_search_approx(idx.ptr, pk.ctypes.data, off.ctypes.data, npat, k, hits.ctypes.data,
                                                max_hits, pos.ctypes.data if want_positions else None,
                                                dst.ctypes.data if want_positions else None, cap,
                                                hoff.ctypes.data if want_positions else None)
    return rc, hits[:npat], pos, dst, hoff


def ecap_protocol(gx, idx):
    """BANANA, k = 1: ANA occurs at 1 and 3 (d = 0); BNN at 0 (BAN, d = 1) and 2 (NAN: d = 2, no) -> [0];
    ANANA at 1 (d = 0); XX nowhere at k = 1 (two substitutions)."""
    packed, off = b"ANA" + b"BNN" + b"ANANA" + b"XX", [0, 3, 6, 11, 13]
    rc, hits, pos, dst, hoff = raw_approx(gx, idx, packed, off, 1, ALL_HITS, 3)
    assert rc == 7                                                   # GX_ECAP
    assert b"4 positions needed" in gx.lib().gx_last_error()
    assert hits["count"].tolist() == [2, 1, 1, 0] and hoff.tolist() == [0, 2, 3, 4, 4]   # complete
    assert hits["best_dist"].tolist() == [0, 1, 0, NO_DIST] and hits["best_pos"].tolist() == [1, 0, 1, 0]
    assert (pos == 0xDEADBEEF).all() and (dst == 0xEE).all()         # untouched
    rc, hits, pos, dst, hoff = raw_approx(gx, idx, packed, off, 1, ALL_HITS, int(hoff[-1]))   # allocate and repeat
    assert rc == 0 and pos.tolist() == [1, 3, 0, 1] and dst.tolist() == [0, 0, 1, 0] and hoff.tolist() == [0, 2, 3, 4, 4]
    rc, *_ = raw_approx(gx, idx, packed, off, 1, ALL_HITS, 0)
    assert rc == 7
    rc, hits, *_ = raw_approx(gx, idx, packed, off, 1, 0, 0, want_positions=False)   # counts only
    assert rc == 0 and hits["count"].tolist() == [2, 1, 1, 0]


def test_host_ecap_protocol(gx):
    idx = gx.SuffixIndex(b"BANANA", host=True)
    ecap_protocol(gx, idx)
    idx.close()


def test_host_python_repeats_after_ecap(gx, monkeypatch):
    monkeypatch.setattr(gx, "_FIRST_CAP", 3)
    s = b"A" * 50
    idx = gx.SuffixIndex(s, host=True)
    pats = [b"AA", b"ACA", b"CC"]
    check_approx(s, pats, 1, idx.search_approx(pats, 1, max_hits=ALL_HITS), ALL_HITS)
    idx.close()


def new_errors(gx, idx, monkeypatch):
    """Every new refusal at its first refused value, and the value before it admitted.  idx: ACGTACGT."""
    L = gx.lib()
    # k = 9: GX_EINVAL; k = 8 with m = 9 is admitted
    rc, *_ = raw_approx(gx, idx, b"ACGTACGTAC", [0, 10], 9, 0, 0, want_positions=False)
    assert rc == 1 and b"GX_APPROX_MAX_K" in L.gx_last_error()
    rc, hits, *_ = raw_approx(gx, idx, b"ACGTACGTA", [0, 9], 8, 0, 0, want_positions=False)
    assert rc == 0 and hits["count"].tolist() == [0]   # (m = 9 > n = 8: no window)
    # m = k: GX_EINVAL naming the pattern; m = k + 1 is admitted
    rc, *_ = raw_approx(gx, idx, b"ACGT" + b"ACG", [0, 4, 7], 3, 0, 0, want_positions=False)
    assert rc == 1 and b"pattern 1" in L.gx_last_error() and b"k + 1" in L.gx_last_error()
    rc, hits, *_ = raw_approx(gx, idx, b"ACGT" + b"ACGA", [0, 4, 8], 3, 0, 0, want_positions=False)
    assert rc == 0 and hits["count"].tolist() == [brute(b"ACGTACGT", P, 3)[0] for P in (b"ACGT", b"ACGA")] == [2, 3]
    # everything the exact search refuses
    rc, *_ = raw_approx(gx, idx, b"AC" + b"GT$A", [0, 2, 6], 1, 0, 0, want_positions=False)
    assert rc == 1 and b"pattern 1" in L.gx_last_error() and b"offset 2" in L.gx_last_error()
    rc, *_ = raw_approx(gx, idx, b"ACGT", [1, 2], 0, 0, 0, want_positions=False)
    assert rc == 1
    rc, *_ = raw_approx(gx, idx, b"ACGT", [0, 3, 2], 0, 0, 0, want_positions=False)
    assert rc == 1
    rc, *_ = raw_approx(gx, idx, b"A" * 65536, [0, 65536], 1, 0, 0, want_positions=False)
    assert rc == 3 and b"65535" in L.gx_last_error()
    hits = np.zeros(1, gx.APPROX_HIT_DTYPE)
    pos, dst = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    off, pk = np.array([0, 2], np.uint64), np.frombuffer(b"AC", np.uint8)
    for d, h in ((dst.ctypes.data, None), (None, off.ctypes.data)):   # positions without hit_offsets / distances
        assert L.gx_suffix_index_search_approx(idx.ptr, pk.ctypes.data, off.ctypes.data, 1, 1, hits.ctypes.data, 4,
                                               pos.ctypes.data, d, 4, h) == 1
    # the candidate budget: ACGT, k = 1: pieces AC and GT, two seed hits each on ACGTACGT, total 4
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", "3")   # total = budget + 1
    rc, hits, pos, dst, hoff = raw_approx(gx, idx, b"ACGT", [0, 4], 1, ALL_HITS, 8)
    assert rc == 3 and b"raise GX_APPROX_CAND_BUDGET" in L.gx_last_error() and b"4 seed hits" in L.gx_last_error()
    assert hits["candidates"].tolist() == [4] and hits["count"].tolist() == [0xABABABAB]   # nothing past candidates
    assert (pos == 0xDEADBEEF).all() and (dst == 0xEE).all() and (hoff == 0xDEAD).all()
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", "4")   # read on every call: total = budget is admitted
    rc, hits, pos, dst, hoff = raw_approx(gx, idx, b"ACGT", [0, 4], 1, ALL_HITS, 8)
    assert rc == 0 and hits["count"].tolist() == [2] and hits["candidates"].tolist() == [4]
    assert pos[:2].tolist() == [0, 4] and dst[:2].tolist() == [0, 0]
    monkeypatch.delenv("GX_APPROX_CAND_BUDGET")


def test_host_errors(gx, monkeypatch):
    idx = gx.SuffixIndex(b"ACGTACGT", host=True)
    new_errors(gx, idx, monkeypatch)
    assert gx.lib().gx_approx_info(None, None, None, None, None) == 1   # (it reports a context's last search)
    idx.close()


WRAP_NPAT = 430000


def wrap_case(gx, idx, monkeypatch):
    """A^5000 and 430,000 times AA at k = 1: 860,000 pieces A with 5,000 hits each, 4.3e9 candidates.  Cut to
    32 bits that is 5,032,704, inside the default budget: the total must be held in 64 bits."""
    monkeypatch.delenv("GX_APPROX_CAND_BUDGET", raising=False)
    total = 2 * WRAP_NPAT * 5000
    assert total > 1 << 32 and total % (1 << 32) == 5032704 < 1 << 27
    packed = np.full(2 * WRAP_NPAT, 0x41, np.uint8)
    off = np.arange(WRAP_NPAT + 1, dtype=np.uint64) * np.uint64(2)
    t0 = time.perf_counter()
    with pytest.raises(gx.GxError) as e:
        idx.search_approx((packed, off), 1, max_hits=4)
    dt = time.perf_counter() - t0
    print(f"wrap case refused in {dt * 1e3:.1f} ms")
    assert e.value.code == 3 and f"{total} seed hits" in str(e.value)
    return dt


def test_host_wrap_case(gx, monkeypatch):
    idx = gx.SuffixIndex(b"A" * 5000, host=True)
    assert wrap_case(gx, idx, monkeypatch) < 2.0   # the seeds alone: nothing of the 4.3e9 is verified
    idx.close()


def test_host_k0_equals_exact_search(gx):
    for alpha in (b"A", b"AC", b"ACGT"):
        s = np_rand(31 + len(alpha), alpha, 300)
        rng = np.random.default_rng(len(alpha))
        pats = [s[i:i + m] for i, m in zip(rng.integers(0, 260, 60).tolist(), rng.integers(1, 40, 60).tolist())]
        pats += [b"ACGTT", s + b"A", s, b"C", b"\xff"]
        idx = gx.SuffixIndex(s, host=True)
        for mh in (1, 3, ALL_HITS):
            a, e = idx.search_approx(pats, 0, max_hits=mh), idx.search(pats, max_hits=mh)
            assert np.array_equal(a["count"], e["count"]) and np.array_equal(a["candidates"], e["count"])
            assert np.array_equal(a["positions"], e["positions"]) and np.array_equal(a["hit_offsets"], e["hit_offsets"])
            assert not a["distances"].any()
        idx.close()


def one(idx, P, k, max_hits=ALL_HITS):
    r = idx.search_approx([P], k, max_hits=max_hits)
    return (int(r["count"][0]), int(r["best_dist"][0]), int(r["best_pos"][0]), int(r["candidates"][0]),
            list(zip(r["positions"].tolist(), r["distances"].tolist())))


def test_banana_by_hand(gx):
    # BANANA$: SA = 6 5 3 1 0 4 2
    idx = gx.SuffixIndex(b"BANANA", host=True)
    # ANANA, k = 1: pieces AN (at 3, 1 in suffix-array order) and ANA (at 3, 1).  Piece 0 leads to starts 3 (the
    # window leaves the text) and 1 (d = 0, kept); piece 1 leads to 3 - 2 = 1 (piece 0 intact there: not kept
    # again) and 1 - 2 < 0.  One occurrence from four candidates.
    assert one(idx, b"ANANA", 1) == (1, 0, 1, 4, [(1, 0)])
    # ANA, k = 1: pieces A (5, 3, 1) and NA (4, 2).  Windows: BAN 2, ANA 0, NAN 3, ANA 0.  The two exact ones
    # come through piece 0; nothing else is within 1.
    assert one(idx, b"ANA", 1) == (2, 0, 1, 5, [(1, 0), (3, 0)])
    # ANA, k = 2: pieces A, N, A.  BAN is at distance 2 with no piece intact... B/A, A/N, N/A: no.  NAN: N/A, A/N, N/A: no.
    assert one(idx, b"ANA", 2) == (2, 0, 1, 8, [(1, 0), (3, 0)])
    # BANANA with its last byte changed, its first byte changed, and both
    assert one(idx, b"BANANX", 1) == (1, 1, 0, 1, [(0, 1)])
    assert one(idx, b"XANANA", 1) == (1, 1, 0, 2, [(0, 1)])      # only piece 1 (ANA at 3, 1) is intact: starts 0 and -2
    assert one(idx, b"XANANX", 1)[:3] == (0, NO_DIST, 0)
    assert one(idx, b"XANANX", 2) == (1, 2, 0, 2, [(0, 2)])      # pieces XA, NA (at 4, 2), NX: starts 2 (leaves the text) and 0
    # NAN, k = 1: pieces N (4, 2) and AN (3, 1); windows BAN 1, ANA 3, NAN 0, ANA 3: best is the exact one at 2
    assert one(idx, b"NAN", 1) == (2, 0, 2, 4, [(0, 1), (2, 0)])
    # a window over '$' is no occurrence: NAX would match NA$ at 4
    assert one(idx, b"NAX", 1) == (1, 1, 2, 2, [(2, 1)])
    # max_hits = 1 keeps the first in candidate order: piece 0 (N at 4, 2): start 4 leaves the text, start 2 is kept
    assert one(idx, b"NAN", 1, max_hits=1) == (2, 0, 2, 4, [(2, 0)])
    idx.close()
