"""A checker for suffix-tree mode that descends from the definitions of
DESIGN.md 17.1 and from nothing in the solvers: no sort, no doubling, no Kasai.
It takes a suffix array and an LCP array as given and verifies them against the
text directly, in time linear in N + sum(LCP), so it reaches sizes the
brute-force restatement of tests/test_suffix_host.py cannot.

Why the clauses of check_arrays suffice.  For neighbours a = SA[k-1], b = SA[k]
and l = LCP[k]: the first l bytes of the two suffixes are equal (clause "too
large") and byte l of a is below byte l of b (clause "order").  Then l is their
longest common prefix exactly and suffix a < suffix b.  With SA a permutation
the chain of N - 1 strict inequalities is the sorted order.  Both positions
a + l and b + l lie inside t (clause "bounds"), where '$' is unique, so no
clause ever reads the zero padding the solvers rely on."""
import numpy as np

DOLLAR = 0x24


def check_arrays(s: bytes, sa, lcp, bwt=None, max_work=None) -> int:
    """AssertionError unless sa, lcp (and bwt, if given) are the suffix array,
    the LCP array and the BWT of t = s + '$'.  Returns the number of byte pairs
    compared: sum(lcp) for equality plus N - 1 for the order.  sum(lcp) above
    max_work (default 128 * N) is a failure: nothing is skipped or sampled."""
    t = np.frombuffer(bytes(s) + b"$", np.uint8)
    N = t.size
    sa = np.asarray(sa)
    lcp = np.asarray(lcp)
    assert sa.shape == (N,) and lcp.shape == (N,), f"shape: sa {sa.shape}, lcp {lcp.shape}, N = {N}"
    sa = sa.astype(np.int64)
    lcp = lcp.astype(np.int64)
    assert np.array_equal(np.sort(sa), np.arange(N, dtype=np.int64)), "permutation: sa is not one of 0..N-1"
    assert lcp[0] == 0, f"lcp[0] = {lcp[0]}"
    assert (lcp >= 0).all(), "bounds: negative lcp"
    a, b, l = sa[:-1], sa[1:], lcp[1:]
    over = np.flatnonzero(np.maximum(a, b) + l >= N)
    assert over.size == 0, f"bounds: max(sa[k-1], sa[k]) + lcp[k] >= N first at k = {over[:4] + 1}"
    work = int(l.sum())
    cap = 128 * N if max_work is None else max_work
    assert work <= cap, f"max_work: sum(lcp) = {work} > {cap}"
    # not too large: the first lcp[k] bytes agree; the set of k alive at depth h shrinks as h grows
    alive = np.flatnonzero(l > 0)
    h = 0
    while alive.size:
        bad = alive[t[a[alive] + h] != t[b[alive] + h]]
        assert bad.size == 0, f"too large: suffixes sa[k-1], sa[k] differ at depth {h} < lcp[k], first at k = {bad[:4] + 1}"
        h += 1
        alive = alive[l[alive] > h]
    # the order, and not too small: the byte behind the common prefix rises strictly
    bad = np.flatnonzero(t[a + l] >= t[b + l])
    assert bad.size == 0, f"order: t[sa[k-1] + lcp[k]] >= t[sa[k] + lcp[k]] first at k = {bad[:4] + 1}"
    if bwt is not None:
        w = np.frombuffer(bwt, np.uint8) if isinstance(bwt, (bytes, bytearray)) else np.asarray(bwt)
        assert w.shape == (N,), f"shape: bwt {w.shape}, N = {N}"
        want = np.where(sa > 0, t[sa - 1], DOLLAR)   # (sa = 0 reads t[-1], which the where discards)
        bad = np.flatnonzero(w != want)
        assert bad.size == 0, f"bwt: differs from t[sa[k] - 1] first at k = {bad[:4]}"
    return work + N - 1


def fold_stats(sa, lcp) -> dict:
    """The seven gx_suffix_stats fields by the interval rule of DESIGN.md 17.1:
    k >= 1 with lcp[k] > 0 counts iff the nearest k' < k with lcp[k'] <= lcp[k]
    has lcp[k'] < lcp[k].  The stack holds the values a later k can still see,
    strictly increasing, above the sentinel lcp[0] = 0."""
    sa = np.asarray(sa)
    lcp = np.asarray(lcp)
    N = int(lcp.size)
    cnt = dsum = 0
    stack = [0]
    for v in lcp[1:].tolist():
        while stack[-1] > v:
            stack.pop()
        if stack[-1] < v:
            cnt += 1
            dsum += v
            stack.append(v)
    mx = int(lcp.max()) if N else 0
    ks = int(np.argmax(lcp)) if N else 0   # (the first position of the maximum)
    return {"num_internal": cnt, "num_leaves": N, "num_nodes": cnt + N + 1, "string_depth_sum": dsum,
            "max_string_depth": mx, "longest_repeat_len": mx, "longest_repeat_start": int(sa[ks - 1]) + 1 if mx else 0}
