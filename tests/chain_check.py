"""The chaining contract in plain numpy, the checker of tests/test_chain_host.py and
tests/test_gpu_chain.py.  It shares nothing with the library: the recurrence in its backward form (for each b,
a = b - 1 down to b - max_pred, keep strictly greater) in int64, trees from pred by a loop, ends by argmax,
members by walking; segments and pair evaluations in closed form."""
import numpy as np

NONE = 0xFFFFFFFF
DEFAULTS = {"w_match": 8, "w_drift": 1, "max_gap": 5000, "max_drift": 500, "max_pred": 64, "min_score": 0}
CHAIN_FIELDS = ("member_off", "score_chain", "n_anchors", "root", "end", "qstart", "tstart", "qend", "tend")


def pack(queries):
    """A mapping as SuffixIndex.mems returns it from a list of queries, each a list of (qpos, tpos, len)."""
    flat = [a for q in queries for a in q]
    arr = np.asarray(flat, np.int64).reshape(len(flat), 3)
    off = np.zeros(len(queries) + 1, np.uint64)
    np.cumsum([len(q) for q in queries], out=off[1:])
    return {"qpos": arr[:, 0].astype(np.uint32), "tpos": arr[:, 1].astype(np.uint32),
            "length": arr[:, 2].astype(np.uint32), "mem_offsets": off}


def solve_query(q, t, ln, P):
    """f, pred, and the chains [(root, end, members)] by root, of one query's anchors (int64 arrays)."""
    n = len(q)
    f, pred = np.zeros(n, np.int64), np.full(n, NONE, np.int64)
    wm, wd, H = P["w_match"], P["w_drift"], P["max_pred"]
    for b in range(n):
        own = wm * ln[b]
        f[b] = own
        lo = max(0, b - H)
        if lo == b:
            continue
        a = np.arange(b - 1, lo - 1, -1)   # nearest first
        dq, dt = q[b] - q[a], t[b] - t[a]
        ok = (dq >= 1) & (dq <= P["max_gap"]) & (dt >= 1) & (dt <= P["max_gap"]) & (np.abs(dq - dt) <= P["max_drift"])
        if not ok.any():
            continue
        ext = f[a] + wm * np.minimum(ln[b], np.minimum(dq, dt)) - wd * np.abs(dq - dt)
        ext = np.where(ok, ext, np.iinfo(np.int64).min)
        k = int(np.argmax(ext))   # the first of the largest: the nearest
        if ext[k] > own:
            f[b], pred[b] = ext[k], a[k]
    root = np.arange(n)
    for b in range(n):
        if pred[b] != NONE:
            root[b] = root[pred[b]]
    chains = []
    for r in np.nonzero(pred == NONE)[0]:
        tree = np.nonzero(root == r)[0]
        e = int(tree[np.argmax(f[tree])])   # the first of the largest: the smallest index
        if f[e] < P["min_score"]:
            continue
        mem = [e]
        while pred[mem[-1]] != NONE:
            mem.append(int(pred[mem[-1]]))
        chains.append((int(r), e, mem[::-1]))
    return f, pred, chains


def solve(anchors, **params):
    """What gxamd.chain_anchors returns, from the contract."""
    P = {**DEFAULTS, **params}
    off = np.asarray(anchors["mem_offsets"], np.int64)
    Q, T, L = (np.asarray(anchors[k], np.int64) for k in ("qpos", "tpos", "length"))
    score, pred = np.zeros(len(Q), np.int32), np.zeros(len(Q), np.uint32)
    rec, members, coff = [], [], np.zeros(len(off), np.uint64)
    for c in range(len(off) - 1):
        s, e = int(off[c]), int(off[c + 1])
        f, p, chains = solve_query(Q[s:e], T[s:e], L[s:e], P)
        assert (f > 0).all() and (f < 2 ** 31).all()
        score[s:e], pred[s:e] = f, p
        for r, end, mem in chains:
            rec.append((len(members), f[end], len(mem), r, end, Q[s + r], T[s + r], Q[s + end] + L[s + end],
                        T[s + end] + L[s + end]))
            members += mem
        coff[c + 1] = len(rec)
    out = {"score": score, "pred": pred, "members": np.asarray(members, np.uint32), "chain_offsets": coff,
           "members_total": len(members)}
    rec = np.asarray(rec, np.int64).reshape(len(rec), 9)
    for k, name in enumerate(CHAIN_FIELDS):
        out[name] = rec[:, k].astype(np.uint64 if name == "member_off" else np.int32 if name == "score_chain" else np.uint32)
    return out


def same(got, want, what=""):
    """Field by field."""
    for k in ("score", "pred", "members", "chain_offsets") + CHAIN_FIELDS:
        assert got[k].dtype == want[k].dtype, (what, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])
    assert got["members_total"] == want["members_total"], what


def closed_form(anchors, **params):
    """(segments, pair evaluations): a query's anchors are cut where qpos advances by more than max_gap, and a
    segment of s anchors has sum_i min(max_pred, s - 1 - i) pairs."""
    P = {**DEFAULTS, **params}
    off = np.asarray(anchors["mem_offsets"], np.int64)
    Q = np.asarray(anchors["qpos"], np.int64)
    segs = pairs = 0
    for c in range(len(off) - 1):
        q = Q[off[c]:off[c + 1]]
        if not len(q):
            continue
        cuts = np.concatenate(([0], np.nonzero(np.diff(q) > P["max_gap"])[0] + 1, [len(q)]))
        for s in np.diff(cuts):
            segs += 1
            pairs += int(np.minimum(P["max_pred"], s - 1 - np.arange(s)).sum())
    return segs, pairs
