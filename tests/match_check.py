"""Brute force for matching statistics and maximal exact matches,
and the checks the host and the GPU tests share.  No tests here.

The brute force is the definition: the equality matrix of s and q, the run
lengths along the diagonals to the right, left-maximality from the cell up-left.
Texts and queries of a few thousand bytes at most."""
import functools

import numpy as np

STAT_FIELDS = ("len", "lo", "count", "pos")
MEM_FIELDS = ("qpos", "tpos", "length")


@functools.lru_cache(maxsize=256)
def runs(s: bytes, q: bytes):
    """(R, leftmax): R[i, j] = the longest common prefix of s[i:] and q[j:], leftmax[i, j] = the pair cannot
    be extended to the left."""
    n, m = len(s), len(q)
    a, b = np.frombuffer(s, np.uint8), np.frombuffer(q, np.uint8)
    eq = a[:, None] == b[None, :]
    R = np.zeros((n + 1, m + 1), np.int32)
    for i in range(n - 1, -1, -1):
        R[i, :m] = np.where(eq[i], R[i + 1, 1:] + 1, 0)
    leftmax = np.ones((n, m), bool)
    if n > 1 and m > 1:
        leftmax[1:, 1:] = ~eq[:-1, :-1]
    return R[:n, :m], leftmax


def brute_mems(s: bytes, q: bytes, min_len: int):
    """[(qpos, tpos, len)] ordered by qpos, then tpos; and the candidates: the pairs with R >= min_len."""
    R, leftmax = runs(s, q)
    long_enough = R >= min_len
    jj, ii = np.nonzero((long_enough & leftmax).T)   # (row-major over the transpose: by j, then i)
    return [(int(j), int(i), int(R[i, j])) for j, i in zip(jj, ii)], int(long_enough.sum())


def brute_stats(s: bytes, q: bytes, max_len: int):
    """Per position j: (len, the positions i whose match reaches len)."""
    R, _ = runs(s, q)
    Rc = np.minimum(R, max_len)
    out = []
    for j in range(len(q)):
        col = Rc[:, j] if len(s) else np.zeros(0, np.int32)
        ln = int(col.max()) if col.size else 0
        out.append((ln, np.nonzero(col >= ln)[0] if ln else None))
    return out


def check_stats(s: bytes, queries, max_len: int, r, sa):
    """r = SuffixIndex.matching_stats(queries, max_len), sa = SuffixIndex.sa() of the same index."""
    n, N = len(s), len(s) + 1
    off = r["offsets"]
    assert len(off) == len(queries) + 1 and int(off[0]) == 0
    assert all(int(off[c + 1] - off[c]) == len(q) for c, q in enumerate(queries))
    for f in STAT_FIELDS:
        assert len(r[f]) == int(off[-1]), f
    for c, q in enumerate(queries):
        b = int(off[c])
        for j, (ln, where) in enumerate(brute_stats(s, q, max_len)):
            g = b + j
            ctx_ = (c, j, q[j:j + 12])
            assert int(r["len"][g]) == ln, ctx_
            lo, cnt = int(r["lo"][g]), int(r["count"][g])
            assert lo + cnt <= N, ctx_
            assert int(r["pos"][g]) == int(sa[lo]), ctx_
            if ln == 0:
                assert (lo, cnt, int(r["pos"][g])) == (0, N, n), ctx_
            else:
                assert cnt == len(where), ctx_
                assert np.array_equal(np.sort(sa[lo:lo + cnt]), where), ctx_


def check_mems(s: bytes, queries, min_len: int, r):
    """r = SuffixIndex.mems(queries, min_len): the exact list in the specified order, and the candidates."""
    moff = r["mem_offsets"]
    assert len(moff) == len(queries) + 1 and int(moff[0]) == 0
    for c, q in enumerate(queries):
        want, cand = brute_mems(s, q, min_len)
        a, b = int(moff[c]), int(moff[c + 1])
        assert b - a == len(want), (c, b - a, len(want))
        assert int(r["candidates"][c]) == cand, (c, int(r["candidates"][c]), cand)
        if len(r["qpos"]) or not int(moff[-1]):   # (counts only: no triples to compare)
            got = list(zip(r["qpos"][a:b].tolist(), r["tpos"][a:b].tolist(), r["length"][a:b].tolist()))
            assert got == want, (c, [x for x in zip(got, want) if x[0] != x[1]][:3])


def same_stats(a, b):
    for f in STAT_FIELDS + ("offsets",):
        assert np.array_equal(a[f], b[f]), f


def same_mems(a, b):
    for f in MEM_FIELDS + ("mem_offsets", "candidates"):
        assert np.array_equal(a[f], b[f]), f


def ceil_log2(x: int) -> int:
    return max(0, (x - 1).bit_length())


def interval_word_bound(N: int, windows, searches: int = 2) -> int:
    """`searches` times the exact search's bound 2 (ceil(log2(N + 1)) + 2) (ceil(w / 8) + 1) per
    position of window w: two searches a position for the matching statistics, one for a seed."""
    lg = ceil_log2(N + 1) + 2
    return sum(searches * 2 * lg * ((int(w) + 7) // 8 + 1) for w in windows)


def seed_word_bound(N: int, lengths, min_len: int) -> int:
    """one exact search of min_len bytes at every position with min_len bytes or more of its
    query left; the other positions take no step."""
    return interval_word_bound(N, [min_len] * sum(max(0, int(m) - min_len + 1) for m in lengths), searches=1)


def emit_word_bound(lengths, min_len: int) -> int:
    """ceil((len - min_len) / 8) + 1 per MEM."""
    return sum((int(x) - min_len + 7) // 8 + 1 for x in lengths)
