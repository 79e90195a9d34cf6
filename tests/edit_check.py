"""The checker of the edit search: a brute force that shares
nothing with the suffix array, the pieces, the bands or the library.

  sellers       E(e) for every end: Sellers' recurrence over the whole text, one
                pattern byte a step, every text column at once in numpy
  starts_of     b(e): plain Levenshtein (the full matrix, no band) of the pattern
                against every window s[b:e] with b in [e - m - k, e]
  lev           plain Levenshtein of two byte strings, in Python (the hand cases)
  check_edit    the contract of DESIGN.md 20.1 on a search_edit result, the
                max_hits rule included
  band_reports  the band model of DESIGN.md 20.2 written out on its own: what
                every candidate reports, to find inputs where two candidates
                report one end with different distances

No test."""
import functools

import numpy as np

ALL_HITS = 0xFFFFFFFF
NO_DIST = 0xFFFFFFFF
_BIG = 1 << 30


def _relax(row: np.ndarray) -> np.ndarray:
    """row[..., c] = min over j <= c of row[..., j] + (c - j): the left-to-right + 1 minimum of a DP row."""
    ar = np.arange(row.shape[-1], dtype=np.int64)
    return np.minimum.accumulate(row - ar, axis=-1) + ar


def sellers(s: bytes, P: bytes) -> np.ndarray:
    """E(e) = min over b <= e of ed(P, s[b:e]) for e = 0 .. n."""
    a, p = np.frombuffer(s, np.uint8), np.frombuffer(P, np.uint8)
    row = np.zeros(len(a) + 1, np.int64)   # D[0][c] = 0
    for i in range(1, len(p) + 1):
        new = np.empty_like(row)
        new[0] = i                         # D[i][0] = i
        new[1:] = np.minimum(row[:-1] + (a != p[i - 1]), row[1:] + 1)
        row = _relax(new)
    return row


def lev(a: bytes, b: bytes) -> int:
    """Plain Levenshtein."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[-1]


def starts_of(s: bytes, P: bytes, k: int, ends, dists) -> np.ndarray:
    """b(e) = max{ b : ed(P, s[b:e]) = E(e) } for every e of ends (E(e) in dists), b over [e - m - k, e].
    ed(P, s[e - l:e]) for every l at once is the last row of the full Levenshtein matrix of the reversed
    pattern against the text read backwards from e; every end is a row of one numpy array."""
    a, p = np.frombuffer(s, np.uint8), np.frombuffer(P, np.uint8)[::-1]
    ends, dists = np.asarray(ends, np.int64), np.asarray(dists, np.int64)
    if len(ends) == 0:
        return np.zeros(0, np.int64)
    L = len(p) + k
    ls = np.arange(1, L + 1, dtype=np.int64)
    idx = ends[:, None] - ls[None, :]            # column l reads s[e - l]
    legal = idx >= 0
    win = np.where(legal, a[np.clip(idx, 0, max(len(a) - 1, 0))] if len(a) else 0, 0)
    row = np.broadcast_to(np.arange(L + 1, dtype=np.int64), (len(ends), L + 1)).copy()   # D[0][l] = l
    row[:, 1:][~legal] = _BIG
    for i in range(1, len(p) + 1):
        new = np.empty_like(row)
        new[:, 0] = i
        new[:, 1:] = np.minimum(row[:, :-1] + (win != p[i - 1]), row[:, 1:] + 1)
        new[:, 1:][~legal] = _BIG
        row = _relax(new)
        row[:, 1:][~legal] = _BIG
    hit = row == dists[:, None]
    assert hit.any(axis=1).all(), "an end without a window of its distance: the checker is wrong"
    return ends - hit.argmax(axis=1)             # the smallest l


@functools.lru_cache(maxsize=2048)
def brute(s: bytes, P: bytes, k: int):
    """(count, best_dist, best_end, ends, dists, starts) of P in s with at most k differences.  (Kept for the
    next call on the same input: a case is checked at several max_hits, and never changed by its readers.)"""
    E = sellers(s, P)
    ends = np.nonzero(E <= k)[0]
    if len(ends) == 0:
        return 0, NO_DIST, 0, ends, ends, ends
    d = E[ends]
    best = int(d.min())
    return len(ends), best, int(ends[d == best][0]), ends, d, starts_of(s, P, k, ends, d)


def check_edit(s: bytes, patterns, k: int, r: dict, max_hits: int = 0):
    """The contract on a search_edit result r: count, best_dist and best_end of every pattern, and with max_hits
    its min(count, max_hits) smallest ends, ascending, each with E(e) and (unless r["starts"] is None) b(e)."""
    npat = len(patterns)
    assert all(len(r[f]) == npat for f in ("count", "best_dist", "best_end", "candidates"))
    at = 0
    for p, P in enumerate(patterns):
        count, best, bend, ends, d, b = brute(s, P, k)
        got = (int(r["count"][p]), int(r["best_dist"][p]), int(r["best_end"][p]))
        assert got == (count, best, bend), (p, P, k, got, (count, best, bend))
        if max_hits <= 0:
            continue
        assert int(r["hit_offsets"][p]) == at, p
        q = min(count, max_hits)
        assert r["ends"][at:at + q].tolist() == ends[:q].tolist(), (p, P, k)
        assert r["distances"][at:at + q].tolist() == d[:q].tolist(), (p, P, k)
        if r["starts"] is not None:
            assert r["starts"][at:at + q].tolist() == b[:q].tolist(), (p, P, k)
            assert all(len(P) - k <= e - x <= len(P) + k for e, x in zip(ends[:q].tolist(), b[:q].tolist()))
        at += q
    if max_hits > 0:
        assert int(r["hit_offsets"][npat]) == at and len(r["ends"]) == at and len(r["distances"]) == at
        assert r["starts"] is None or len(r["starts"]) == at
    else:
        assert "ends" not in r


def same_edit(a: dict, b: dict):
    """Field by field: the device against the host index."""
    assert sorted(a) == sorted(b)
    for f in a:
        if a[f] is None or b[f] is None:
            assert a[f] is None and b[f] is None, f
        else:
            assert np.array_equal(a[f], b[f]), f


def segment(r: dict, p: int) -> dict:
    """{end: (distance, start)} of pattern p (start None without starts)."""
    a, b = int(r["hit_offsets"][p]), int(r["hit_offsets"][p + 1])
    st = r["starts"][a:b].tolist() if r["starts"] is not None else [None] * (b - a)
    return {e: (d, x) for e, d, x in zip(r["ends"][a:b].tolist(), r["distances"][a:b].tolist(), st)}


def band_reports(s: bytes, P: bytes, k: int) -> dict:
    """{end: [the distance every candidate that reports it gives]}: P cut into k + 1 pieces, every occurrence
    of a piece a candidate on the diagonal d0 = at - piece start, Sellers' recurrence on the cells with
    c - i in [d0 - k, d0 + k], a neighbour outside the band infinite."""
    n, m, out = len(s), len(P), {}
    for j in range(k + 1):
        ps, pe = j * m // (k + 1), (j + 1) * m // (k + 1)
        for at in range(n - (pe - ps) + 1):
            if s[at:at + pe - ps] != P[ps:pe]:
                continue
            d0 = at - ps
            if d0 < -k or d0 > n - m + k:
                continue
            D = {(0, c): 0 for c in range(max(0, d0 - k), min(n, d0 + k) + 1)}
            for i in range(1, m + 1):
                for c in range(max(0, i + d0 - k), min(n, i + d0 + k) + 1):
                    D[(i, c)] = i if c == 0 else min(D.get((i - 1, c - 1), _BIG) + (P[i - 1] != s[c - 1]),
                                                     D.get((i - 1, c), _BIG) + 1, D.get((i, c - 1), _BIG) + 1)
            for c in range(max(0, m + d0 - k), min(n, m + d0 + k) + 1):
                if D[(m, c)] <= k:
                    out.setdefault(c, []).append(D[(m, c)])
    return out


def disagreements(count: int, seed: int, k: int = 3):
    """`count` inputs (s, P) on which two candidates report one end with different distances."""
    rng, found = np.random.default_rng(seed), []
    while len(found) < count:
        n, m = int(rng.integers(5, 13)), int(rng.integers(k + 1, 8))
        s = bytes(rng.choice(np.frombuffer(b"AC", np.uint8), n).tolist())
        P = bytes(rng.choice(np.frombuffer(b"AC", np.uint8), m).tolist())
        if any(len(set(v)) > 1 for v in band_reports(s, P, k).values()) and (s, P) not in found:
            found.append((s, P))
    return found
