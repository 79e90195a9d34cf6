"""Edit search on the host index (no device): gx_suffix_index_search_edit with
ctx = NULL against the brute force of tests/edit_check.py, on 200 random
strings over four alphabets with k = 0..3 and 0..k+1 planted substitutions,
insertions and deletions, every max_hits edge, starts NULL, the GX_ECAP
protocol, every refusal at its first refused value beside the last admitted
one, both budgets, the 64-bit candidate total (the wrap case), k = 0 against
the exact search, the empty text, and three inputs by hand."""
import time

import numpy as np
import pytest

from edit_check import ALL_HITS, NO_DIST, brute, check_edit, lev, segment
from test_approx_host import WRAP_NPAT, other
from test_suffix_host import BYTES_219, np_rand

ALPHABETS = [b"A", b"AC", b"ACGT", BYTES_219]
KINDS = ("sub", "ins", "del")


def edited(P: bytes, edits, alpha: bytes) -> bytes:
    """P with the edits [(kind, column)] applied, from the last column to the first so that columns keep their
    meaning: a substitution changes the byte, an insertion puts a different byte in front of it, a deletion
    drops it."""
    p = bytearray(P)
    for kind, c in sorted(edits, key=lambda e: -e[1]):
        if kind == "sub":
            p[c] = other(p[c], alpha)
        elif kind == "ins":
            p.insert(c, other(p[c], alpha))
        else:
            del p[c]
    return bytes(p)


def random_edits(rng, m: int, count: int):
    cols = rng.choice(m, count, replace=False).tolist()
    return [(KINDS[int(rng.integers(0, 3))], c) for c in cols]


def patterns_for(s: bytes, k: int, alpha: bytes, rng):
    """[(pattern, the end of the window it was cut from, planted edits)]: windows at the start, the middle and the
    very end of the text, with 0 .. k + 1 edits at random columns."""
    n, out = len(s), []
    for m in (k + 2, k + 3, 8, 9, 17, 40):
        if m > n:
            continue
        for i in (0, int(rng.integers(0, n - m + 1)), n - m):
            for count in range(0, k + 2):
                if count > m:
                    continue
                P = edited(s[i:i + m], random_edits(rng, m, count), alpha)
                if len(P) >= k + 1:
                    out.append((P, i + m, count))
    return out


@pytest.mark.parametrize("alpha", ALPHABETS, ids=["A", "AC", "ACGT", "bytes219"])
def test_host_brute_force(gx, alpha):
    rng = np.random.default_rng(len(alpha))
    for case in range(50):
        n = int(rng.integers(1, 301))
        s = np_rand(3000 * len(alpha) + case, alpha, n)
        idx = gx.SuffixIndex(s, host=True)
        for k in range(4):
            trip = patterns_for(s, k, alpha, rng)
            if not trip:
                continue
            pats = [t[0] for t in trip]
            r = idx.search_edit(pats, k, max_hits=ALL_HITS)
            check_edit(s, pats, k, r, ALL_HITS)
            check_edit(s, pats, k, idx.search_edit(pats, k), 0)
            check_edit(s, pats, k, idx.search_edit(pats, k, max_hits=2), 2)
            for p, (P, end, count) in enumerate(trip):
                if count <= k:   # found where it was cut, with at most the planted edits
                    assert end in segment(r, p) and segment(r, p)[end][0] <= count, (s, P, k, end, count)
        idx.close()


def test_host_empty_text(gx):
    idx = gx.SuffixIndex(b"", host=True)
    for k in (0, 1, 3):
        pats = [b"A" * (k + 1), b"ACGTACGTAC"]
        r = idx.search_edit(pats, k, max_hits=ALL_HITS)
        check_edit(b"", pats, k, r, ALL_HITS)
        assert r["count"].tolist() == [0, 0] and r["best_dist"].tolist() == [NO_DIST] * 2
        assert r["ends"].tolist() == [] and r["hit_offsets"].tolist() == [0, 0, 0]
    assert idx.search_edit([], 2)["count"].tolist() == []
    idx.close()


def test_host_max_hits_edges_and_no_starts(gx):
    s = np_rand(78, b"AC", 300)
    idx = gx.SuffixIndex(s, host=True)
    pats = [b"ACAC", b"CCAA", b"ACACACAC", s[10:30], b"AAAAAAAA", b"GGGG"]
    for k in (1, 2):
        count = brute(s, b"ACAC", k)[0]
        assert count > 3
        for mh in (0, 1, count - 1, count, count + 1, ALL_HITS):
            check_edit(s, pats, k, idx.search_edit(pats, k, max_hits=mh), mh)
            r = idx.search_edit(pats, k, max_hits=mh, starts=False)
            assert mh == 0 or r["starts"] is None
            check_edit(s, pats, k, r, mh)
    idx.close()


def raw_edit(gx, idx, packed: bytes, offsets, k, max_hits, cap, want_ends=True, want_starts=True):
    """gx_suffix_index_search_edit as the C caller sees it: (rc, hits, ends, distances, starts, hit_offsets)."""
    off = np.asarray(offsets, np.uint64)
    npat = len(off) - 1
    pk = np.frombuffer(packed, np.uint8) if len(packed) else np.zeros(1, np.uint8)
    hits = np.full(max(npat, 1), 0xABABABAB, np.uint32).repeat(4).view(gx.EDIT_HIT_DTYPE)
    end = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    sta = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    dst = np.full(max(cap, 1), 0xEE, np.uint8)
    hoff = np.full(npat + 1, 0xDEAD, np.uint64)
    rc = gx.lib().gx_suffix_index_search_edit(idx.ptr, pk.ctypes.data, off.ctypes.data, npat, k, hits.ctypes.data,
                                              max_hits, end.ctypes.data if want_ends else None,
                                              dst.ctypes.data if want_ends else None,
                                              sta.ctypes.data if want_ends and want_starts else None, cap,
                                              hoff.ctypes.data if want_ends else None)
    return rc, hits[:npat], end, dst, sta, hoff


def ecap_protocol(gx, idx):
    """BANANA, k = 1.  ANNA: E = 4 3 2 2 1 2 1 -> ends 4 (ANA, start 1) and 6 (ANA, start 3); BANANA: end 5 (BANAN,
    one deletion) and 6 (exact); XX: nowhere."""
    s = b"BANANA"
    packed, off = b"ANNA" + b"BANANA" + b"XX", [0, 4, 10, 12]
    want = [brute(s, P, 1) for P in (b"ANNA", b"BANANA", b"XX")]
    assert [w[0] for w in want] == [2, 2, 0]
    rc, hits, end, dst, sta, hoff = raw_edit(gx, idx, packed, off, 1, ALL_HITS, 3)
    assert rc == 7                                                   # GX_ECAP
    assert b"4 positions needed" in gx.lib().gx_last_error()
    assert hits["count"].tolist() == [2, 2, 0] and hoff.tolist() == [0, 2, 4, 4]   # complete
    assert hits["best_dist"].tolist() == [1, 0, NO_DIST] and hits["best_end"].tolist() == [4, 6, 0]
    assert (end == 0xDEADBEEF).all() and (dst == 0xEE).all() and (sta == 0xDEADBEEF).all()   # untouched
    rc, hits, end, dst, sta, hoff = raw_edit(gx, idx, packed, off, 1, ALL_HITS, int(hoff[-1]))   # allocate and repeat
    assert rc == 0 and end.tolist() == [4, 6, 5, 6] and dst.tolist() == [1, 1, 1, 0] and sta.tolist() == [1, 3, 0, 0]
    rc, *_ = raw_edit(gx, idx, packed, off, 1, ALL_HITS, 0)
    assert rc == 7
    rc, hits, end, dst, sta, hoff = raw_edit(gx, idx, packed, off, 1, ALL_HITS, 4, want_starts=False)   # starts NULL
    assert rc == 0 and end.tolist() == [4, 6, 5, 6] and (sta == 0xDEADBEEF).all()
    rc, hits, *_ = raw_edit(gx, idx, packed, off, 1, 0, 0, want_ends=False)   # counts only
    assert rc == 0 and hits["count"].tolist() == [2, 2, 0]


def test_host_ecap_protocol(gx):
    idx = gx.SuffixIndex(b"BANANA", host=True)
    ecap_protocol(gx, idx)
    idx.close()


def test_host_python_repeats_after_ecap(gx, monkeypatch):
    monkeypatch.setattr(gx, "_FIRST_CAP", 3)
    s = b"A" * 50
    idx = gx.SuffixIndex(s, host=True)
    pats = [b"AA", b"ACA", b"CC"]
    check_edit(s, pats, 1, idx.search_edit(pats, 1, max_hits=ALL_HITS), ALL_HITS)
    idx.close()


def refusals(gx, idx, monkeypatch):
    """Every refusal at its first refused value, and the value before it admitted.  idx: ACGTACGT."""
    L, s = gx.lib(), b"ACGTACGT"
    # k = 9: GX_EINVAL; k = 8 with m = 9 is admitted
    rc, *_ = raw_edit(gx, idx, b"ACGTACGTAC", [0, 10], 9, 0, 0, want_ends=False)
    assert rc == 1 and b"GX_APPROX_MAX_K" in L.gx_last_error()
    rc, hits, *_ = raw_edit(gx, idx, b"ACGTACGTA", [0, 9], 8, 0, 0, want_ends=False)
    assert rc == 0 and hits["count"].tolist() == [brute(s, b"ACGTACGTA", 8)[0]]
    # m = k: GX_EINVAL naming the pattern; m = k + 1 is admitted
    rc, *_ = raw_edit(gx, idx, b"ACGT" + b"ACG", [0, 4, 7], 3, 0, 0, want_ends=False)
    assert rc == 1 and b"pattern 1" in L.gx_last_error() and b"k + 1" in L.gx_last_error()
    rc, hits, *_ = raw_edit(gx, idx, b"ACGT" + b"ACGA", [0, 4, 8], 3, 0, 0, want_ends=False)
    assert rc == 0 and hits["count"].tolist() == [brute(s, P, 3)[0] for P in (b"ACGT", b"ACGA")]
    # m = 4097: GX_ERANGE naming the pattern and the limit; m = 4096 is admitted
    rc, *_ = raw_edit(gx, idx, b"AC" + b"A" * 4097, [0, 2, 4099], 1, 0, 0, want_ends=False)
    assert rc == 3 and b"pattern 1" in L.gx_last_error() and b"GX_EDIT_MAX_M" in L.gx_last_error()
    rc, hits, *_ = raw_edit(gx, idx, b"AC" + b"A" * 4096, [0, 2, 4098], 1, 0, 0, want_ends=False)
    assert rc == 0 and hits["count"].tolist() == [brute(s, b"AC", 1)[0], 0]
    # everything the exact search refuses
    rc, *_ = raw_edit(gx, idx, b"AC" + b"GT$A", [0, 2, 6], 1, 0, 0, want_ends=False)
    assert rc == 1 and b"pattern 1" in L.gx_last_error() and b"offset 2" in L.gx_last_error()
    rc, *_ = raw_edit(gx, idx, b"ACGT", [1, 2], 0, 0, 0, want_ends=False)
    assert rc == 1
    rc, *_ = raw_edit(gx, idx, b"ACGT", [0, 3, 2], 0, 0, 0, want_ends=False)
    assert rc == 1
    rc, *_ = raw_edit(gx, idx, b"A" * 65536, [0, 65536], 1, 0, 0, want_ends=False)
    assert rc == 3 and b"65535" in L.gx_last_error()
    hits = np.zeros(1, gx.EDIT_HIT_DTYPE)
    end, dst = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    off, pk = np.array([0, 2], np.uint64), np.frombuffer(b"AC", np.uint8)
    for e, d, h in ((end.ctypes.data, dst.ctypes.data, None), (end.ctypes.data, None, off.ctypes.data),
                    (None, None, None)):   # ends without hit_offsets / distances; starts without ends
        assert L.gx_suffix_index_search_edit(idx.ptr, pk.ctypes.data, off.ctypes.data, 1, 1, hits.ctypes.data, 4,
                                             e, d, end.ctypes.data, 4, h) == 1
    # the seed budget: ACGT, k = 1: pieces AC and GT, two seed hits each on ACGTACGT, total 4
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", "3")   # total = budget + 1
    rc, hits, end, dst, sta, hoff = raw_edit(gx, idx, b"ACGT", [0, 4], 1, ALL_HITS, 16)
    assert rc == 3 and b"raise GX_APPROX_CAND_BUDGET" in L.gx_last_error() and b"4 seed hits" in L.gx_last_error()
    assert hits["candidates"].tolist() == [4] and hits["count"].tolist() == [0xABABABAB]   # nothing past candidates
    assert (end == 0xDEADBEEF).all() and (dst == 0xEE).all() and (sta == 0xDEADBEEF).all() and (hoff == 0xDEAD).all()
    # the budget on the ends before dedupe: every one of the 4 candidates reports its exact end and the two beside
    # it (one deletion, one insertion), except that the last window has no end beyond n: 3 + 3 + 3 + 3 - 2 = 10
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", "9")   # ends = budget + 1 (the seed hits, 4, are inside)
    rc, hits, end, dst, sta, hoff = raw_edit(gx, idx, b"ACGT", [0, 4], 1, ALL_HITS, 16)
    assert rc == 3 and b"raise GX_APPROX_CAND_BUDGET" in L.gx_last_error(), L.gx_last_error()
    assert b"10 reported ends before dedupe" in L.gx_last_error()
    assert hits["candidates"].tolist() == [4] and hits["count"].tolist() == [0xABABABAB]
    assert (end == 0xDEADBEEF).all() and (dst == 0xEE).all() and (sta == 0xDEADBEEF).all() and (hoff == 0xDEAD).all()
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", "10")   # read on every call: ends = budget is admitted
    rc, hits, end, dst, sta, hoff = raw_edit(gx, idx, b"ACGT", [0, 4], 1, ALL_HITS, 16)
    want = brute(s, b"ACGT", 1)
    assert rc == 0 and hits["count"].tolist() == [want[0]] == [5] and hits["candidates"].tolist() == [4]
    assert end[:5].tolist() == want[3].tolist() == [3, 4, 5, 7, 8] and dst[:5].tolist() == want[4].tolist()
    assert sta[:5].tolist() == want[5].tolist()
    monkeypatch.delenv("GX_APPROX_CAND_BUDGET")


def test_host_refusals(gx, monkeypatch):
    idx = gx.SuffixIndex(b"ACGTACGT", host=True)
    refusals(gx, idx, monkeypatch)
    assert gx.lib().gx_edit_info(None, None, None, None, None, None, None) == 1   # (it reports a context's last search)
    idx.close()


def wrap_case(gx, idx, monkeypatch):
    """A^5000 and 430,000 times AA at k = 1: 4.3e9 seed hits, 5,032,704 when cut to 32 bits: refused from the
    64-bit total, before anything is verified."""
    monkeypatch.delenv("GX_APPROX_CAND_BUDGET", raising=False)
    total = 2 * WRAP_NPAT * 5000
    packed = np.full(2 * WRAP_NPAT, 0x41, np.uint8)
    off = np.arange(WRAP_NPAT + 1, dtype=np.uint64) * np.uint64(2)
    t0 = time.perf_counter()
    with pytest.raises(gx.GxError) as e:
        idx.search_edit((packed, off), 1, max_hits=4)
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
        lens = np.array([len(P) for P in pats], np.uint32)
        idx = gx.SuffixIndex(s, host=True)
        e = idx.search(pats, max_hits=ALL_HITS)
        eo = e["hit_offsets"].astype(np.int64)
        for mh in (1, 3, ALL_HITS):
            a = idx.search_edit(pats, 0, max_hits=mh)
            assert np.array_equal(a["count"], e["count"]) and np.array_equal(a["candidates"], e["count"])
            assert not a["distances"].any()
            # the exact search keeps the first max_hits of the suffix-array interval, this one the smallest:
            # they are the head of every pattern's complete ascending list
            pos = np.concatenate([e["positions"][eo[p]:eo[p + 1]][:mh] for p in range(len(pats))])
            per = np.repeat(lens, np.diff(a["hit_offsets"]).astype(np.int64))
            assert np.array_equal(a["starts"], pos) and np.array_equal(a["ends"], pos + per)
        idx.close()


def one(idx, P, k, max_hits=ALL_HITS):
    """[(end, distance, start)] of one pattern."""
    r = idx.search_edit([P], k, max_hits=max_hits)
    return list(zip(r["ends"].tolist(), r["distances"].tolist(), r["starts"].tolist()))


BY_HAND = [
    # two candidates report end 6, with 1 and with 3: the minimum is the contract
    (b"AAACCAA", b"CCAC", 3, [(1, 3, 0), (2, 3, 1), (3, 3, 2), (4, 2, 2), (5, 2, 3), (6, 1, 3), (7, 1, 3)]),
    (b"BANANA", b"ANNA", 1, [(4, 1, 1), (6, 1, 3)]),
    # the first pattern byte missing at text position 0 (diagonal -1), the last missing at n
    (b"CGTAC", b"ACGTAC", 1, [(5, 1, 0)]),
    (b"ACGTA", b"ACGTAC", 1, [(5, 1, 0)]),
]


@pytest.mark.parametrize("s,P,k,want", BY_HAND)
def test_by_hand(gx, s, P, k, want):
    for e, d, b in want:   # (the table against plain Levenshtein, before the library is asked)
        assert lev(P, s[b:e]) == d and all(lev(P, s[x:e]) >= d for x in range(e + 1))
        assert all(lev(P, s[x:e]) > d for x in range(b + 1, e + 1))
    idx = gx.SuffixIndex(s, host=True)
    assert one(idx, P, k) == want
    check_edit(s, [P], k, idx.search_edit([P], k, max_hits=ALL_HITS), ALL_HITS)
    idx.close()
