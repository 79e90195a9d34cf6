"""The checker of the approximate search: a brute force that
slides the pattern over every legal window of s and counts the differing bytes.
It shares nothing with the suffix array, the pieces or the library.  No test."""
import numpy as np

ALL_HITS = 0xFFFFFFFF
NO_DIST = 0xFFFFFFFF


def distances(s: bytes, P: bytes) -> np.ndarray:
    """d(i) for every legal start i = 0 .. n - m (empty when m > n): the windows never touch '$'."""
    a, p = np.frombuffer(s, np.uint8), np.frombuffer(P, np.uint8)
    n, m = len(a), len(p)
    if m > n:
        return np.zeros(0, np.int64)
    d = np.zeros(n - m + 1, np.int64)
    for j in range(m):
        d += a[j:j + n - m + 1] != p[j]
    return d


def brute(s: bytes, P: bytes, k: int):
    """(count, best_dist, best_pos, [(pos, dist) ascending]) of P in s with at most k substitutions."""
    d = distances(s, P)
    pos = np.nonzero(d <= k)[0]
    if len(pos) == 0:
        return 0, NO_DIST, 0, []
    best = int(d[pos].min())
    return len(pos), best, int(pos[d[pos] == best][0]), [(int(i), int(d[i])) for i in pos]


def check_approx(s: bytes, patterns, k: int, r: dict, max_hits: int = 0):
    """The contract on a search_approx result r.  A pattern with count <= max_hits must report exactly the brute
    force's list; one with more reports max_hits of them, chosen by the candidate order, which the brute force
    does not know: distinct, ascending, genuine, with the right distances."""
    npat = len(patterns)
    assert all(len(r[f]) == npat for f in ("count", "best_dist", "best_pos", "candidates"))
    at = 0
    for p, P in enumerate(patterns):
        count, best, bpos, occ = brute(s, P, k)
        got = (int(r["count"][p]), int(r["best_dist"][p]), int(r["best_pos"][p]))
        assert got == (count, best, bpos), (p, P, k, got, (count, best, bpos))
        assert int(r["candidates"][p]) >= count, (p, P)   # every occurrence is a verified seed hit
        if max_hits <= 0:
            continue
        assert int(r["hit_offsets"][p]) == at, p
        q = min(count, max_hits)
        seg = list(zip(r["positions"][at:at + q].tolist(), r["distances"][at:at + q].tolist()))
        if count <= max_hits:
            assert seg == occ, (p, P, k, seg, occ)
        else:
            assert all(a[0] < b[0] for a, b in zip(seg, seg[1:])), (p, seg)   # distinct and ascending
            want = dict(occ)
            assert all(want.get(i) == d for i, d in seg), (p, P, k, seg)       # genuine, right distance
        at += q
    if max_hits > 0:
        assert int(r["hit_offsets"][npat]) == at and len(r["positions"]) == at and len(r["distances"]) == at


def same_approx(a: dict, b: dict):
    """Field by field: the device against the host index."""
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]), f
