"""The refusals of gx_chain_anchors as data, the way tests/extend_error_cases.py holds those of
gx_suffix_index_extend: the inputs of every case and the raw caller that returns (return code,
gx_last_error()).  tests/golden/make_chain_error_texts.py records them once into
tests/golden/chain_error_texts.json; tests/test_chain_host.py (ctx = NULL) and tests/test_gpu_chain.py (a device
context) hold every later library to that file.

A case is (id, overrides).  Without overrides a call is one query of the two anchors (0, 0, 4) and (10, 10, 4),
the default parameters passed explicitly, capacities of 16 chains and 16 members and no NULL argument: it
succeeds with one chain of two members.  Overrides:
  queries        the batch, a list of queries, each a list of (qpos, tpos, len)
  off, nq        the offsets and the query count, where they are not the batch's own (a call refused before
                 an offset or an anchor is read may name more than the arrays hold)
  params         parameters that differ from the defaults
  null           arguments passed as NULL, by their names in gx.h
  ccap, mcap     the capacities
  budget         GX_APPROX_CAND_BUDGET for the call
Where two refusals apply at once the id names both, the winner first: those cases pin the order of the checks."""
import ctypes
import os

import numpy as np

from chain_check import DEFAULTS, pack

BASE = [[(0, 0, 4), (10, 10, 4)]]
M20 = 1 << 20


def _pair(first, second, **over):
    return (f"{first}-before-{second}", over)


def cases():
    big = [[(i * M20, i * M20, M20) for i in range(2048)]]   # w_match * sum(len) = 2^31 at w_match 1
    return [
        ("anchor-offsets-null", {"null": {"anchor_offsets"}}),
        ("chain-offsets-null", {"null": {"chain_offsets"}}),
        ("members-total-null", {"null": {"members_total"}}),
        ("w-match-0", {"params": {"w_match": 0}}),
        ("w-match-1025", {"params": {"w_match": 1025}}),
        ("w-drift-1025", {"params": {"w_drift": 1025}}),
        ("max-gap-0", {"params": {"max_gap": 0}}),
        ("max-gap-above", {"params": {"max_gap": M20 + 1}}),
        ("max-drift-above", {"params": {"max_drift": M20 + 1}}),
        ("max-pred-0", {"params": {"max_pred": 0}}),
        ("max-pred-257", {"params": {"max_pred": 257}}),
        ("min-score-negative", {"params": {"min_score": -1}}),
        ("queries-range", {"nq": (1 << 32) - 2049}),
        ("offsets0", {"off": [1, 2]}),
        ("offsets-decrease", {"queries": [BASE[0], [], BASE[0]], "off": [0, 2, 1, 4]}),
        ("members-null", {"null": {"members"}}),
        ("budget", {"budget": 1}),
        ("anchors-null", {"null": {"anchors"}}),
        ("len-0", {"queries": [[(0, 0, 4)], [(0, 0, 4), (5, 5, 0)]]}),
        ("qpos-range", {"queries": [[(0, 0, 4), ((1 << 32) - 4, 10, 4)]]}),
        ("tpos-range", {"queries": [[(0, 0, 4), (10, (1 << 32) - 1, 1)]]}),
        ("order-equal", {"queries": [[(0, 0, 4), (10, 10, 4), (10, 10, 5)]]}),
        ("order-qpos", {"queries": [[(5, 0, 4), (4, 10, 4)]]}),
        ("order-tpos", {"queries": [[], [(5, 9, 4), (5, 8, 4)]]}),
        ("sum-range", {"queries": [BASE[0]] + big, "params": {"w_match": 1, "max_gap": M20}}),
        ("sum-range-w", {"queries": [[(0, 0, M20), (M20, M20, M20)]], "params": {"w_match": 1024}}),
        ("ecap-chains", {"queries": [[(0, 0, 4)], [(0, 0, 4)]], "ccap": 1}),
        ("ecap-members", {"mcap": 1}),
        ("ecap-0", {"ccap": 0, "mcap": 0}),
        _pair("anchor-offsets-null", "chain-offsets-null", null={"anchor_offsets", "chain_offsets"}),
        _pair("chain-offsets-null", "members-total-null", null={"chain_offsets", "members_total"}),
        _pair("members-total-null", "w-match-0", null={"members_total"}, params={"w_match": 0}),
        _pair("w-match-0", "w-drift-1025", params={"w_match": 0, "w_drift": 1025}),
        _pair("w-drift-1025", "max-gap-0", params={"w_drift": 1025, "max_gap": 0}),
        _pair("max-gap-0", "max-drift-above", params={"max_gap": 0, "max_drift": M20 + 1}),
        _pair("max-drift-above", "max-pred-0", params={"max_drift": M20 + 1, "max_pred": 0}),
        _pair("max-pred-257", "min-score-negative", params={"max_pred": 257, "min_score": -1}),
        _pair("min-score-negative", "queries-range", params={"min_score": -1}, nq=(1 << 32) - 2049),
        _pair("queries-range", "offsets0", nq=(1 << 32) - 2049, off=[1, 2]),
        _pair("offsets0", "offsets-decrease", queries=[BASE[0], [], BASE[0]], off=[1, 2, 1, 4]),
        _pair("offsets-decrease", "members-null", queries=[BASE[0], [], BASE[0]], off=[0, 2, 1, 4], null={"members"}),
        _pair("members-null", "budget", null={"members"}, budget=1),
        _pair("budget", "anchors-null", budget=1, null={"anchors"}),
        _pair("anchors-null", "ecap", null={"anchors"}, ccap=0),
        _pair("len-0", "range", queries=[[(0, (1 << 32) - 1, 0)]]),
        _pair("range", "order", queries=[[(5, 5, 4), (4, (1 << 32) - 4, 4)]]),
        _pair("order-a1", "len-0-a2", queries=[[(5, 5, 4), (5, 5, 4), (6, 6, 0)]]),
        _pair("sum-range-q0", "len-0-q1", queries=big + [[(0, 0, 0)]], params={"w_match": 1, "max_gap": M20}),
        _pair("sum-range", "ecap", queries=big, params={"w_match": 1, "max_gap": M20}, ccap=0),
        _pair("ecap-chains", "ecap-members", ccap=0, mcap=0),
    ]


class CParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32 if k == "min_score" else ctypes.c_uint32) for k in DEFAULTS]


def c_params(params):
    """The C structure of the defaults with `params` over them (any int32 / uint32 value: the refusals' too)."""
    p = CParams()
    for k, v in {**DEFAULTS, **(params or {})}.items():
        setattr(p, k, v)
    return p


def raw_call(gx, ctx_ptr, anchors, params=None, null=(), ccap=16, mcap=16, off=None, nq=None, fill=None):
    """gx_chain_anchors as it is, on `anchors` (a mapping as chain_check.pack makes it): (return code,
    gx_last_error()).  fill: a dict that receives the output arrays as the call left them: scores, preds, chains
    (CHAIN_DTYPE), members, chain_offsets, members_total, all preset to 0xAB bytes."""
    A = len(anchors["qpos"])
    an = np.zeros(max(A, 1), gx.MEM_DTYPE)
    an["qpos"][:A], an["tpos"][:A], an["len"][:A] = anchors["qpos"], anchors["tpos"], anchors["length"]
    offs = np.asarray(off if off is not None else anchors["mem_offsets"], np.uint64)
    n = len(offs) - 1 if nq is None else nq
    p = c_params(params) if params != "null" else None
    scores = np.full(max(A, 1), 0xAB, np.uint8).repeat(4).view(np.int32)
    preds = np.full(max(A, 1), 0xAB, np.uint8).repeat(4).view(np.uint32)
    chains = np.full(40 * max(ccap, 1), 0xAB, np.uint8).view(gx.CHAIN_DTYPE)
    members = np.full(4 * max(mcap, 1), 0xAB, np.uint8).view(np.uint32)
    coff = np.full(8 * (len(offs) if nq is None else 2), 0xAB, np.uint8).view(np.uint64)
    mtot = np.full(8, 0xAB, np.uint8).view(np.uint64)
    ptr = {"anchors": an.ctypes.data, "anchor_offsets": offs.ctypes.data, "params": ctypes.byref(p) if p else None,
           "scores": scores.ctypes.data, "preds": preds.ctypes.data, "chains": chains.ctypes.data,
           "members": members.ctypes.data, "chain_offsets": coff.ctypes.data, "members_total": mtot.ctypes.data}
    a = {k: (None if k in null else v) for k, v in ptr.items()}
    lib = gx.lib()
    rc = lib.gx_chain_anchors(ctx_ptr, a["anchors"], a["anchor_offsets"], n, a["params"], a["scores"], a["preds"],
                              a["chains"], ccap, a["members"], mcap, a["chain_offsets"], a["members_total"])
    if fill is not None:
        fill.update(scores=scores[:A], preds=preds[:A], chains=chains, members=members, chain_offsets=coff,
                    members_total=mtot)
    return int(rc), lib.gx_last_error().decode()


def run_case(gx, ctx_ptr, over, fill=None):
    """(return code, gx_last_error()) of the case; ctx_ptr: None for the host solver, or a context's pointer."""
    anchors = pack(over.get("queries", BASE))
    old = os.environ.get("GX_APPROX_CAND_BUDGET")
    if "budget" in over:
        os.environ["GX_APPROX_CAND_BUDGET"] = str(over["budget"])
    try:
        return raw_call(gx, ctx_ptr, anchors, over.get("params"), over.get("null", set()), over.get("ccap", 16),
                        over.get("mcap", 16), over.get("off"), over.get("nq"), fill)
    finally:
        if "budget" in over:
            if old is None:
                del os.environ["GX_APPROX_CAND_BUDGET"]
            else:
                os.environ["GX_APPROX_CAND_BUDGET"] = old
