"""Colinear chains of a long query's anchors on the host solver (gx_chain_anchors with ctx = NULL,
DESIGN.md 23): every content case against the contract in plain numpy (tests/chain_check.py), the error table
against tests/golden/chain_error_texts.json, the GX_ECAP protocol, the int32 edge and the anchor budget.  No
device.  tests/test_gpu_chain.py runs the same cases, CASES, on the device.

A case is (id, queries, params): a batch, each query a list of (qpos, tpos, len), and the parameters that
differ from the defaults."""
import json
import os

import numpy as np
import pytest

from chain_check import DEFAULTS, NONE, closed_form, pack, same, solve
from chain_error_cases import cases as error_cases
from chain_error_cases import raw_call, run_case
from conftest import GOLDEN

M20 = 1 << 20
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
PREDS = (1, 2, 63, 64, 65, 128, 129, 255, 256)
GOLDEN_TEXTS = os.path.join(GOLDEN, "chain_error_texts.json")


def diagonal(n, step=10, ln=7, q0=0, t0=3):
    """n anchors on one diagonal: dq = dt = step >= ln, so f(i) = w_match ln (i + 1)."""
    return [(q0 + step * i, t0 + step * i, ln) for i in range(n)]


def planted(H, back):
    """The only good predecessor of the last anchor `back` anchors before it, ineligible filler between: the
    filler's tpos descends from far away, so nothing reaches it and it reaches nothing."""
    return [(0, 0, 10)] + [(1 + i, 1000000 - 1000 * i, 3) for i in range(back - 1)] + [(300, 300, 10)]


def rand_query(rng, n, span, repeats=False):
    """n random anchors in a span x span square, ascending and distinct; repeats: several tpos at a qpos."""
    pts = set()
    while len(pts) < n:
        q = int(rng.integers(0, span))
        for _ in range(int(rng.integers(1, 5)) if repeats else 1):
            pts.add((q, int(rng.integers(0, span))))
    return [(q, t, int(rng.integers(1, 30))) for q, t in sorted(pts)[:n]]


def make_cases():
    rng = np.random.default_rng(23)
    out = []
    out.append(("diagonals", [diagonal(n) for n in SIZES], {}))
    for n in (64, 65, 257):   # a query of one segment alone in its batch
        out.append((f"diagonal-{n}", [diagonal(n)], {}))
    # one query, a segment of every size: the diagonals laid behind one another, max_gap + 1 apart in qpos
    q, at = [], 0
    for n in SIZES[1:]:
        q += diagonal(n, q0=at, t0=at + 3)
        at = q[-1][0] + 61
    out.append(("segments-of-every-size", [q], {"max_gap": 60}))
    for H in PREDS:
        out.append((f"planted-pred-{H}", [planted(H, H), planted(H, H + 1), planted(H, 1)], {"max_pred": H}))
        out.append((f"diagonal-pred-{H}", [diagonal(300), diagonal(H), diagonal(H + 1)], {"max_pred": H}))
    # dq and dt each at 0, 1, max_gap and max_gap + 1
    G = 50
    out.append(("gap-edges", [[(100, 100, 5), (100 + dq, 100 + dt, 5)] for dq in (0, 1, G, G + 1) for dt in (0, 1, G, G + 1)
                              if (dq, dt) != (0, 0)], {"max_gap": G, "max_drift": M20}))
    out.append(("gap-edges-max", [[(100, 100, 5), (100 + dq, 100 + dt, 5)] for dq in (1, M20, M20 + 1) for dt in (1, M20, M20 + 1)],
                {"max_gap": M20, "max_drift": M20}))
    out.append(("drift-edges", [[(0, 0, 5), (100, 130, 5)], [(0, 0, 5), (100, 131, 5)], [(0, 0, 5), (130, 100, 5)],
                                [(0, 0, 5), (131, 100, 5)], [(0, 0, 5), (100, 100, 5)]], {"max_drift": 30}))
    out.append(("drift-0", [[(0, 0, 5), (100, 100, 5)], [(0, 0, 5), (100, 101, 5)]], {"max_drift": 0}))
    out.append(("break-at-gap", [[(0, 0, 5), (50, 50, 5), (100, 100, 5)], [(0, 0, 5), (51, 51, 5), (102, 102, 5)],
                                 [(0, 0, 5), (50, 50, 5), (101, 101, 5)]], {"max_gap": 50}))
    out.append(("binding-term", [[(0, 0, 5), (20, 20, 10)], [(0, 0, 5), (6, 20, 10)], [(0, 0, 5), (20, 6, 10)]], {}))
    # ext = w_match len_b exactly: 8 + 8 * 10 - 8; and one above it
    out.append(("ext-equals-own", [[(0, 0, 1), (10, 18, 10)], [(0, 0, 1), (10, 17, 10)]], {}))
    out.append(("equal-ext-nearer-wins", [[(0, 0, 5), (0, 2, 5), (10, 11, 5)], [(0, 0, 5), (0, 2, 5), (0, 4, 5), (10, 12, 5)]], {}))
    out.append(("equal-ends-smaller-wins", [[(0, 0, 5), (10, 11, 5), (11, 10, 5)]], {}))
    out.append(("interior-maximum", [[(0, 0, 10), (20, 20, 15), (150, 160, 1)]], {}))
    out.append(("branching", [[(0, 0, 5), (10, 10, 5), (20, 21, 5), (21, 20, 5), (30, 31, 5), (31, 30, 9), (40, 39, 5)]], {}))
    for ms in (168, 169):   # f(e) of a diagonal of 3 is 8 * 7 * 3
        out.append((f"min-score-{ms}", [diagonal(3), diagonal(4), diagonal(2)], {"min_score": ms}))
    out.append(("shared-qpos", [[(10 * i, 10 * i + 1000 * j, 6) for i in range(40) for j in range(4)]], {}))
    out.append(("shared-qpos-pred-3", [[(10 * i, 10 * i + 1000 * j, 6) for i in range(40) for j in range(4)]], {"max_pred": 3}))
    for nq in (1, 64, 257):
        out.append((f"batch-{nq}", [rand_query(rng, int(rng.integers(0, 4)) * int(rng.integers(0, 12)), 200) for _ in range(nq)],
                    {"max_gap": 60, "max_drift": 25}))
    out.append(("empty-batch", [], {}))
    out.append(("empty-queries", [[], [], []], {}))
    for n in (2047, 2048, 2049):   # the scan's tile: segments and chains across a batch and within one query
        out.append((f"tile-{n}-queries", [[(5, 7, 3)] for _ in range(n)], {}))
        out.append((f"tile-{n}-segments", [[(100 * i, 100 * i, 3) for i in range(n)]], {"max_gap": 99}))
    for H, n, span in ((1, 200, 300), (5, 300, 200), (64, 700, 900), (65, 400, 700), (128, 700, 1500), (129, 600, 1300),
                       (200, 900, 2500), (256, 1300, 3000)):
        out.append((f"random-pred-{H}", [rand_query(rng, n, span), rand_query(rng, n // 3, span // 2, repeats=True)],
                    {"max_pred": H, "max_gap": span // 3, "max_drift": span // 8, "w_match": 3, "w_drift": 2}))
    out.append(("random-ties", [rand_query(rng, 500, 60, repeats=True)], {"w_drift": 0, "max_pred": 100, "max_gap": 20}))
    out.append(("weights-at-max", [rand_query(rng, 200, 400)], {"w_match": 1024, "w_drift": 1024, "max_gap": 100, "max_drift": 100}))
    return out


CASES = make_cases()
IDS = [c[0] for c in CASES]
_WANT = {}


def expected(case):
    """The checker's answer, computed once a session and shared."""
    cid, queries, params = case
    if cid not in _WANT:
        anchors = pack(queries)
        _WANT[cid] = (anchors, solve(anchors, **params))
        for k in _WANT[cid][1].values():
            if isinstance(k, np.ndarray):
                k.setflags(write=False)
    return _WANT[cid]


def test_worked_examples(gx):
    """Cases small enough to work by hand, asked of the checker and of the host solver alike."""
    for ask in (solve, lambda anchors: gx.chain_anchors(anchors, host=True)):
        worked_examples(ask)
    assert closed_form(pack([diagonal(5)]), max_pred=2) == (1, 2 + 2 + 2 + 1)
    assert closed_form(pack([[(0, 0, 5), (50, 50, 5), (101, 101, 5)], []]), max_gap=50) == (2, 1)


def worked_examples(solve):   # noqa: F811 (the solver asked, in the checker's place)
    w = solve(pack([diagonal(1000)]))
    assert w["score_chain"].tolist() == [56000] and w["n_anchors"].tolist() == [1000]
    assert w["members"].tolist() == list(range(1000)) and (w["qend"][0], w["tend"][0]) == (9997, 10000)
    w = solve(pack([[(0, 0, 1), (10, 18, 10)], [(0, 0, 1), (10, 17, 10)]]))
    assert w["pred"].tolist() == [NONE, NONE, NONE, 0] and w["score"].tolist() == [8, 80, 8, 81]
    w = solve(pack([[(0, 0, 5), (0, 2, 5), (10, 11, 5)]]))
    assert w["pred"].tolist() == [NONE, NONE, 1] and w["score"].tolist() == [40, 40, 79]
    w = solve(pack([[(0, 0, 5), (10, 11, 5), (11, 10, 5)]]))
    assert w["score"].tolist() == [40, 79, 79] and w["end"].tolist() == [1] and w["members"].tolist() == [0, 1]
    w = solve(pack([[(0, 0, 10), (20, 20, 15), (150, 160, 1)]]))
    assert w["score"].tolist() == [80, 200, 198] and w["pred"].tolist() == [NONE, 0, 1] and w["end"].tolist() == [1]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_content(gx, case):
    anchors, want = expected(case)
    same(gx.chain_anchors(anchors, host=True, **case[2]), want, case[0])


def test_planted_predecessors_are_taken_and_not(gx):
    """What the planted cases are for, said of the checker's answer and of the host solver's."""
    for H in PREDS:
        anchors, want = expected(CASES[IDS.index(f"planted-pred-{H}")])
        last = np.cumsum([H + 1, H + 2, 2]) - 1
        assert want["pred"][last].tolist() == [0, NONE, 0], H
        assert gx.chain_anchors(anchors, host=True, max_pred=H)["pred"][last].tolist() == [0, NONE, 0], H


def load_golden():
    with open(GOLDEN_TEXTS) as f:
        return json.load(f)


def error_table(gx, ctx_ptr):
    """Every refusal: code and text as recorded, chains and members untouched, and where nothing ran the other
    outputs too."""
    golden = load_golden()
    assert sorted(golden) == sorted(cid for cid, _ in error_cases())
    for cid, over in error_cases():
        fill = {}
        rc, text = run_case(gx, ctx_ptr, over, fill)
        assert (rc, text) == (golden[cid]["rc"], golden[cid]["text"]), cid
        assert (fill["chains"].view(np.uint8) == 0xAB).all() and (fill["members"].view(np.uint8) == 0xAB).all(), cid
        if rc != 7:
            for k in ("scores", "preds", "chain_offsets", "members_total"):
                assert (fill[k].view(np.uint8) == 0xAB).all(), (cid, k)
    assert raw_call(gx, ctx_ptr, pack([[(0, 0, 4), (10, 10, 4)]]))[0] == 0   # the case without overrides succeeds


def test_error_table(gx):
    error_table(gx, None)


def null_combinations(gx, ctx_ptr, case):
    """Counts only, and scores / preds NULL in each combination: what is asked for is the full call's."""
    anchors, want = expected(case)
    K, M = len(want["root"]), want["members_total"]
    for null in ((), ("scores",), ("preds",), ("scores", "preds")):
        for counts_only in (False, True):
            fill = {}
            nul = set(null) | ({"chains", "members"} if counts_only else set())
            rc, _ = raw_call(gx, ctx_ptr, anchors, case[2], nul, ccap=K, mcap=M, fill=fill)
            assert rc == 0
            assert np.array_equal(fill["chain_offsets"], want["chain_offsets"]) and int(fill["members_total"][0]) == M
            for k, name in (("scores", "score"), ("preds", "pred")):
                if k in null:
                    assert (fill[k].view(np.uint8) == 0xAB).all()
                else:
                    assert np.array_equal(fill[k], want[name])
            if counts_only:
                assert (fill["chains"].view(np.uint8) == 0xAB).all() and (fill["members"].view(np.uint8) == 0xAB).all()
            else:
                assert np.array_equal(fill["members"][:M], want["members"])
                assert np.array_equal(fill["chains"]["end"][:K], want["end"])
    rc, _ = raw_call(gx, ctx_ptr, anchors, "null", ccap=K, mcap=M)   # params = NULL: the defaults
    assert rc == 0


def test_null_combinations(gx):
    null_combinations(gx, None, CASES[IDS.index("branching")])
    null_combinations(gx, None, CASES[IDS.index("batch-64")])


def ecap_protocol(gx, ctx_ptr):
    """GX_ECAP: counts, scores and preds complete, chains and members untouched; the exact capacity succeeds."""
    case = CASES[IDS.index("batch-64")]
    anchors, want = expected(case)
    K, M = len(want["root"]), want["members_total"]
    assert K > 2 and M > K
    for ccap, mcap in ((K - 1, M), (K, M - 1), (0, 0)):
        fill = {}
        rc, text = raw_call(gx, ctx_ptr, anchors, case[2], ccap=ccap, mcap=mcap, fill=fill)
        what = f"{K} chains needed, chains_cap is {ccap}" if ccap < K else f"{M} members needed, members_cap is {mcap}"
        assert (rc, text) == (7, "chain: " + what)
        assert np.array_equal(fill["chain_offsets"], want["chain_offsets"]) and int(fill["members_total"][0]) == M
        assert np.array_equal(fill["scores"], want["score"]) and np.array_equal(fill["preds"], want["pred"])
        assert (fill["chains"].view(np.uint8) == 0xAB).all() and (fill["members"].view(np.uint8) == 0xAB).all()
    fill = {}
    assert raw_call(gx, ctx_ptr, anchors, case[2], ccap=K, mcap=M, fill=fill)[0] == 0
    assert np.array_equal(fill["members"], want["members"]) and np.array_equal(fill["chains"]["root"], want["root"])
    assert np.array_equal(fill["chains"]["member_off"], want["member_off"])


def test_ecap_protocol(gx):
    ecap_protocol(gx, None)


def int32_edge(gx, ctx, host):
    """w_match * sum(len) = 2^31 - 1 on a single diagonal is accepted and f reaches it; 2^31 is refused."""
    q = [(i * M20, i * M20, M20) for i in range(2047)] + [(2047 * M20, 2047 * M20, M20 - 1)]
    params = {"w_match": 1, "max_gap": M20, "max_drift": 0, "max_pred": 1}
    r = gx.chain_anchors(pack([q]), ctx=ctx, host=host, **params)
    assert int(r["score"][-1]) == 2 ** 31 - 1 and r["score_chain"].tolist() == [2 ** 31 - 1]
    assert r["n_anchors"].tolist() == [2048] and int(r["tend"][0]) == 2 ** 31 - 1
    assert np.array_equal(r["score"].astype(np.int64), np.minimum(np.arange(1, 2049) * M20, 2 ** 31 - 1))
    q[-1] = (2047 * M20, 2047 * M20, M20)
    with pytest.raises(gx.GxError) as e:
        gx.chain_anchors(pack([q]), ctx=ctx, host=host, **params)
    assert e.value.code == 3 and "2147483648, at or above 2^31" in str(e.value)


def test_int32_edge(gx):
    int32_edge(gx, None, True)


def budget_case(gx, ctx, host, monkeypatch):
    """The anchor budget: refused at one below the anchor count, accepted exactly at it."""
    case = CASES[IDS.index("batch-64")]
    anchors, want = expected(case)
    A = len(anchors["qpos"])
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", str(A - 1))
    with pytest.raises(gx.GxError) as e:
        gx.chain_anchors(anchors, ctx=ctx, host=host, **case[2])
    assert f"chain: {A} anchors, more than GX_APPROX_CAND_BUDGET = {A - 1}" in str(e.value)
    monkeypatch.setenv("GX_APPROX_CAND_BUDGET", str(A))
    same(gx.chain_anchors(anchors, ctx=ctx, host=host, **case[2]), want)
    monkeypatch.delenv("GX_APPROX_CAND_BUDGET")


def test_budget(gx, monkeypatch):
    budget_case(gx, None, True, monkeypatch)


def test_host_index_chain_mems(gx):
    """SuffixIndex.chain_mems on a host index: the MEMs, then their chains by the host solver."""
    rng = np.random.default_rng(5)
    s = bytes(rng.choice(list(b"ACGT"), 3000).tolist())
    q = bytearray(s[500:2500])
    for k in range(40, len(q), 97):
        q[k] = ord("A") if q[k] != ord("A") else ord("C")
    idx = gx.SuffixIndex(s, host=True)
    r = idx.chain_mems([bytes(q), b"ACGT", s[100:300]], 12, min_score=100)
    idx.close()
    same(r["chains"], solve(r["mems"], min_score=100))
    assert len(r["chains"]["root"]) >= 2 and r["chains"]["n_anchors"].max() > 5
    assert int(r["chains"]["score_chain"][-1]) == 8 * 200   # the third query is one MEM


def test_unknown_parameter_is_refused(gx):
    with pytest.raises(TypeError):
        gx.chain_anchors(pack([diagonal(2)]), host=True, max_gaps=5)
    assert gx.CHAIN_DEFAULTS == DEFAULTS and gx.CHAIN_NONE == NONE
