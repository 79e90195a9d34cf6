"""GPU parity at the edges of the score ranges that choose a fill and a plane
format (gx_api_plan.cpp w16_ok, d8_planes_ok, twin_width).

Every kernel that decodes the twin fill's 12-bit plane codes (gx_kernels.hip
w16_decode: w16_word_of / tb_w16_codes_kernel, tb_seq_kernel,
plane_sums_kernel, export_w16_kernel, local_col_kernel) runs on scores whose
x_S = S - I attains both ends of its 5-bit field, -16 (code & 31 == 16, the
sign-extension case with its borrow into x_D) and 15; tests/test_formats.py
proves on the CPU, from the oracle's planes, that the batches used here
attain them.  One step past the field the launch must fall back to byte
planes, and one step past the byte planes' range (U - 2a = 127) to int32
planes without the twin fill.  Every comparison is bit-exact against the
oracle; every plane cell is compared, not a sample."""
import functools

import numpy as np
import pytest

from test_formats import EDGE_KINDS, EDGE_SCORES, ONE_PAST_SCORES, edge_batch, edge_family
from test_gpu_twin import _steps_list

pytestmark = pytest.mark.gpu

LAUNCH = {"auto": {}, "w4_grid2": {"GX_BAND_WAVES": "4", "GX_FILL_GRID": "2"},
          "w7_grid3": {"GX_BAND_WAVES": "7", "GX_FILL_GRID": "3"}}
FOUR_KINDS = tuple(k for k in EDGE_KINDS if k != "acgtn")


@pytest.fixture(autouse=True)
def _twin_layout0(monkeypatch):
    """Small batches: the anti-diagonal layout and the twin fill are forced
    (run_fill picks them for deep queues only); no overlapped pipeline."""
    monkeypatch.setenv("GX_LAYOUT", "0")
    monkeypatch.setenv("GX_TWIN", "1")
    monkeypatch.setenv("GX_OVERLAP", "0")


@functools.lru_cache(maxsize=2)
def _reference(oracle, scores, is_local, kinds):
    """(pairs, per pair the oracle's result with whole planes, its plane
    checksums), computed once for the launches that share it."""
    pairs = edge_batch(kinds)
    full = [oracle.align(a, b, scores, is_local=is_local, want_planes=True) for a, b in pairs]
    sums = [oracle.align_lean(a, b, scores, is_local=is_local).extra["plane_sums"] for a, b in pairs]
    return pairs, full, sums


def _assert_planes(t, n, want, tag):
    """Every cell of the three planes of table t, exported 100 rows at a time
    (offsets that fall inside the 128-row strips)."""
    for which in range(3):
        got = np.concatenate([t.rows(which, r0, min(100, n + 1 - r0)) for r0 in range(0, n + 1, 100)])
        if not np.array_equal(got, want[which]):
            bad = np.argwhere(got != want[which])
            i, j = (int(x) for x in bad[0])
            raise AssertionError((tag, "plane", which, "cells differing", len(bad), "first", (i, j),
                                  "got", int(got[i, j]), "want", int(want[which][i, j])))


def _run_staged_checked(gx, ctx, oracle, scores, is_local, kinds, want_info):
    """Two pipelined passes with kept planes: fill_info, both passes' plane
    checksums, score, n_steps and alignment of every pair, every plane cell."""
    pairs, full, sums_want = _reference(oracle, scores, is_local, kinds)
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*scores), is_local, keep_planes=True, steps=2, plane_sums=True, keep=True)
    info = ctx.fill_info()
    for key, v in want_info.items():
        assert info[key] == v, (key, info)
    sums = st.plane_sums()
    assert sums.shape == (2, len(pairs), 3)
    for p, (a, b) in enumerate(pairs):
        o = full[p]
        tag = (scores, "local" if is_local else "global", p, len(a), len(b))
        for k in range(2):
            assert [int(x) for x in sums[k, p]] == sums_want[p], (tag, "pass", k)
        assert res[p].score == o.score and res[p].n_steps == len(o.choices), tag
        assert _steps_list(st.steps(p)) == o.alignment(), tag
        t = st.table(p)
        _assert_planes(t, len(a), o.planes, tag)
        t.free()
    return info


EDGE_CASES = [pytest.param(s, loc, la, id="%s-%s-%s" % ("_".join(map(str, s)), "local" if loc else "global", la))
              for s in EDGE_SCORES for loc in (False, True) for la in LAUNCH]


@pytest.mark.parametrize("scores,is_local,launch", EDGE_CASES)
def test_codes_at_field_edges(gx, ctx, oracle, monkeypatch, scores, is_local, launch):
    """Twin plane codes (1.5 B/cell) under scores that attain x_S = -16 and 15:
    the batch with ACGTN pairs (the plain match test) and the batch of <= 4
    symbols (the score tables, where the shifted scores fit them; the local
    twin of (-15, -16, 0, -15) carries K = 16)."""
    for k, v in LAUNCH[launch].items():
        monkeypatch.setenv(k, v)
    for kinds in (EDGE_KINDS, FOUR_KINDS):
        _run_staged_checked(gx, ctx, oracle, scores, is_local, kinds, {"twin": 1, "plane_bytes_per_cell": 1.5})


@pytest.mark.parametrize("scores", ONE_PAST_SCORES, ids=lambda s: "_".join(map(str, s)))
def test_codes_one_past_edge(gx, ctx, oracle, scores):
    """One step outside the 5-bit field (x_S = 16 attained; -17 proved): the
    global twin keeps byte planes, the local fill takes no twin (twin_width
    needs the codes there); exact either way."""
    _run_staged_checked(gx, ctx, oracle, scores, False, EDGE_KINDS, {"twin": 1, "plane_bytes_per_cell": 3})
    _run_staged_checked(gx, ctx, oracle, scores, True, EDGE_KINDS, {"twin": 0, "plane_bytes_per_cell": 3})


@pytest.mark.parametrize("scores", [(1, -1, 0, -42), (1, -1, 0, -43)], ids=["h42", "h43"])
def test_byte_plane_edge(gx, ctx, oracle, monkeypatch, scores):
    """(1, -1, 0, -42): U - 2a = 127, the last scores of the byte planes and a
    W = 3 twin; (1, -1, 0, -43): int32 planes, and with planes no twin fill.
    A staged batch, one table through the twin fill, and untracked tables on
    every layout, global and local: every plane cell."""
    last = scores[3] == -42
    _run_staged_checked(gx, ctx, oracle, scores, False, EDGE_KINDS,
                        {"twin": 1, "band_waves": 3, "plane_bytes_per_cell": 3} if last else
                        {"twin": 0, "plane_bytes_per_cell": 12})
    monkeypatch.setenv("GX_NO_TABLE_PRINT", "1")
    # one table filled by the twin kernel (the pair beside a copy of itself)
    monkeypatch.setenv("GX_TABLE_TWIN", "1")
    for kind in ("related", "ac"):
        a, b = edge_family(300, 260)[kind]
        cont = gx.SequenceContainer([gx.Sequence("a", a.decode()), gx.Sequence("b", b.decode())])
        t, _ = gx.alignment_table(cont, gx.Scores(*scores), False, False, ctx=ctx, max_cell=False)
        info = ctx.fill_info()
        assert (info["twin"], info["plane_bytes_per_cell"]) == ((1, 3) if last else (0, 12)), info
        assert not last or info["band_waves"] == 3, info
        o = oracle.align(a, b, scores, want_planes=True)
        for k in range(3):
            assert np.array_equal(t.plane(k), o.planes[k]), (scores, kind, k)
        al = gx.retrace(cont, t, False)
        assert _steps_list(al._steps) == o.alignment() and al.score == o.score, (scores, kind)
    # untracked tables on the per-pair formats of every layout
    monkeypatch.delenv("GX_TABLE_TWIN")
    monkeypatch.delenv("GX_TWIN")
    a, b = edge_family(129, 300)["related"]
    cont = gx.SequenceContainer([gx.Sequence("a", a.decode()), gx.Sequence("b", b.decode())])
    for is_local in (False, True):
        o = oracle.align(a, b, scores, is_local=is_local, want_planes=True)
        for lay in (0, 1, 3):
            monkeypatch.setenv("GX_LAYOUT", str(lay))
            t, _ = gx.alignment_table(cont, gx.Scores(*scores), is_local, False, ctx=ctx, max_cell=False)
            info = ctx.fill_info()
            # (fill_info reports the split column step, layout 1's local default, as 2)
            assert info["twin"] == 0 and info["layout"] in ((1, 2) if lay == 1 else (lay,)), (lay, is_local, info)
            if lay == 0:
                assert info["plane_bytes_per_cell"] == (3 if last else 12), info
            for k in range(3):
                assert np.array_equal(t.plane(k), o.planes[k]), (scores, lay, is_local, k)
            al = gx.retrace(cont, t, is_local)
            assert _steps_list(al._steps) == o.alignment() and al.score == o.score, (scores, lay, is_local)


PIPE_SHAPES = [(65, 200), (129, 300), (257, 256), (300, 130), (513, 70), (640, 641)]


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("is_local", [False, True], ids=["global", "local"])
def test_tracked_planes_pipelined(gx, ctx, oracle, monkeypatch, is_local, poison):
    """Tracked passes with kept planes on layout 3, pipelined: from the second
    pass on the reductions behind a fill (launch_finalize, launch_skew_max_col,
    the plane checksums) run on a stream of their own beside the next pass's
    fill (gx_api_fill.cpp run_fill, post_aside).  Two sets of pairs of equal
    shapes alternate pass by pass, so every buffer a pass takes last held the
    other set's data (with GX_POOL_POISON, garbage).  Every pass's results --
    score, statistics, max cell, matches_at_max -- and plane checksums, and
    each set's last alignments."""
    monkeypatch.setenv("GX_LAYOUT", "3")
    if poison:
        monkeypatch.setenv("GX_POOL_POISON", "1")
    rng = np.random.default_rng(606)
    pairs = [(bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8)),
              bytes(rng.choice(list(b"ACGT"), size=m).astype(np.uint8))) for _ in range(2) for n, m in PIPE_SHAPES]
    H, steps = len(PIPE_SHAPES), 5
    scores = (1, -2, -1, -5)
    want = [oracle.align(a, b, scores, is_local=is_local) for a, b in pairs]
    want_sums = [oracle.align_lean(a, b, scores, is_local=is_local).extra["plane_sums"] for a, b in pairs]
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*scores), is_local, keep_planes=True, max_cell=True, steps=steps, plane_sums=True,
                    alternate=True)
    info = ctx.fill_info()
    assert info["layout"] == 3 and info["twin"] == 0 and info["plane_bytes_per_cell"] == 12, info
    sums = st.plane_sums()
    passes = st.pass_results()
    assert sums.shape == (steps, len(pairs), 3) and len(passes) == steps

    def fields(r):
        return (r.score, r.matches, r.mismatches, r.gap_extensions, r.opening_gaps, r.n_steps, r.max_cell_i,
                r.max_cell_j, r.matches_at_max)

    for p, o in enumerate(want):
        o.extra["fields"] = (o.score, o.matches, o.mismatches, o.gap_extensions, o.opening_gaps, len(o.choices),
                             o.max_cell[0], o.max_cell[1], o.matches_at_max)
    for k in range(steps):
        for q in range(H):
            p = (k % 2) * H + q
            assert fields(passes[k][p]) == want[p].extra["fields"], (p, "pass", k)
            assert [int(x) for x in sums[k, p]] == want_sums[p], (p, "pass", k)
    for p, o in enumerate(want):   # each set's last pass
        assert fields(res[p]) == o.extra["fields"], (p, "last")
        assert _steps_list(st.steps(p)) == o.alignment(), (p, "last")
