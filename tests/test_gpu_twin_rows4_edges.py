"""GPU parity of the four-rows-a-lane twin fill (gx_fill_pk.hip R = 4) at every
band width and with both match tests, where its int16 halves are loaded.

tests/test_gpu_twin_rows4.py runs the default scores on small alphabets: the
score tables at the widths those scores admit, with values far from the int16
limit.  Here every R = 4 instantiation runs -- band widths 3, 4, 7, 8 and 15,
with the score tables (PLANES 30) and with the plain match test (PLANES 26:
GX_NO_SCORE_TABLE, a fifth symbol, or a negative shifted mismatch) -- on the
scores whose gap extension dominates the neighbour step, which
tests/test_twin_bound_r4.py shows (from the oracle's planes) to reach 0.787 of
the admission rule's per-strip term.  Each run asserts the band width, the rows
per lane and the match test of the launch (Context.fill_info), so a silent
fall-back to another kernel fails.  One step past each width the launch must
narrow; the plane codes' field ends (x_S = -16, 15) are decoded across 256-row
strip and band edges; twins 1,024 columns apart; 65,536 columns; and the
launch nobody forces must take four rows exactly where the rule says.

Everything is bit-exact against the oracle: every pass's plane checksums and
results, the last pass's alignments, and where stated every plane cell."""
import ctypes
import random

import numpy as np
import pytest

from conftest import CONFIG_SCORES
from test_formats import EDGE_KINDS, EDGE_SCORES, edge_batch_rows4
from test_gpu_twin_rows4 import COLS_M, ROWS_N, _dna, _lean, _run_checked, _stats, _steps_list
from test_twin_bound import _families, _neighbour_d
from test_twin_bound_r4 import HEAVY_CASES, ONE_PAST, ROWS, WIDTHS, _closed_form, widest_admitted

pytestmark = pytest.mark.gpu

HEAVY_FAMILIES = ("all_mismatch", "all_match", "gap_rows", "gap_cols", "repeat")


@pytest.fixture(autouse=True)
def _force_rows4(monkeypatch):
    monkeypatch.setenv("GX_TWIN", "1")
    monkeypatch.setenv("GX_TWIN_ROWS", "4")
    monkeypatch.setenv("GX_LAYOUT", "0")
    for k in ("GX_BAND_WAVES", "GX_FILL_GRID", "GX_NO_SCORE_TABLE"):
        monkeypatch.delenv(k, raising=False)


def _twin_gap(scores, W):
    """Column gap of the batches' unequal twin: 300 columns, or where the
    heaviest scores of a width leave less room, the widest gap the closed-form
    rule still admits at W (15: 171 columns, 8: 144, 7: 45) -- the launch then
    sits within one neighbour step of the 30,000 limit."""
    return min(300, (29999 - _closed_form(scores, W)) // _neighbour_d(scores))


def _heavy_batch(scores, W_rows, W_bound, families=HEAVY_FAMILIES):
    """Two full W_rows-strip bands of 256-row strips and a partial third, 900
    columns: the families that push the values hardest, a random pair of the
    same shape, and a random pair _twin_gap columns narrower.  twin_table
    orders by columns, then rows: the 900-column pairs of full height twin
    among themselves, gap_cols (few rows) with the narrower pair -- a twin
    unequal both ways -- and gap_rows (75 columns) with itself."""
    n, m = ROWS * W_rows * 2 + 150, 900
    fam = _families(n, m)
    rng = random.Random(n)
    pairs = [fam[f] for f in families] + [fam["random"], (_dna(rng, n), _dna(rng, m - _twin_gap(scores, W_bound)))]
    assert sum(len(b) == m for _, b in pairs) % 2 == 1
    return pairs


def _admitted_width(gx, scores, want, gaps=(0,)):
    """The widest instantiated width <= want that gx_twin_admission_rows admits
    at four rows (twin_width's choice), the same for every column gap given."""
    got = set()
    for dm in gaps:
        ws = [W for W in WIDTHS if (W <= want or W == 3) and gx.twin_admission(gx.Scores(*scores), W, dm,
                                                                                rows_per_lane=4)[0]]
        got.add(max(ws) if ws else 0)
    assert len(got) == 1, (scores, want, gaps, got)
    return got.pop()


def _assert_planes(t, n, want, tag):
    """Every cell of the three planes of table t, exported 100 rows at a time
    (offsets that fall inside the 256-row strips and their 64-row blocks)."""
    for which in range(3):
        got = np.concatenate([t.rows(which, r0, min(100, n + 1 - r0)) for r0 in range(0, n + 1, 100)])
        if not np.array_equal(got, want[which]):
            bad = np.argwhere(got != want[which])
            i, j = (int(x) for x in bad[0])
            raise AssertionError((tag, "plane", which, "cells differing", len(bad), "first", (i, j),
                                  "got", int(got[i, j]), "want", int(want[which][i, j])))


@pytest.mark.parametrize("match", ["tables", "plain"])
@pytest.mark.parametrize("scores,W", HEAVY_CASES, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_heavy_scores_every_width(gx, ctx, oracle, monkeypatch, scores, W, match):
    """Every R = 4 kernel (W in {3, 4, 7, 8, 15} x {score tables, plain match
    test}) at the heaviest scores its width admits, two passes."""
    monkeypatch.setenv("GX_BAND_WAVES", str(W))
    if match == "plain":
        monkeypatch.setenv("GX_NO_SCORE_TABLE", "1")
    pairs = _heavy_batch(scores, W, W)
    _run_checked(gx, ctx, oracle, pairs, steps=2, scores=scores, band_waves=W)
    assert ctx.fill_info()["score_table"] == (1 if match == "tables" else 0), ctx.fill_info()
    if W <= 4:   # every cell of one loaded pair's planes (checksums alone would let compensating errors through)
        st = gx.StagedPairs(pairs, ctx=ctx)
        st.run(gx.Scores(*scores), False, keep_planes=True, steps=1, keep=True)
        info = ctx.fill_info()
        assert (info["twin"], info["twin_rows"], info["band_waves"], info["plane_bytes_per_cell"]) == (1, 4, W, 1.5), info
        p = HEAVY_FAMILIES.index("repeat")                 # (attains 0.787 of the rule, tests/test_twin_bound_r4.py)
        a, b = pairs[p]
        t = st.table(p)
        _assert_planes(t, len(a), oracle.align(a, b, scores, want_planes=True).planes, (scores, W, match))
        t.free()


@pytest.mark.parametrize("scores,refused,takes", ONE_PAST, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_past_narrows(gx, ctx, oracle, monkeypatch, scores, refused, takes):
    """One step past a width's heaviest scores, asked for that width: the
    launch takes the next narrower one, still at four rows, and is exact on
    inputs that would overflow the refused width's term."""
    monkeypatch.setenv("GX_BAND_WAVES", str(refused))
    assert widest_admitted(scores, refused, _twin_gap(scores, takes)) == takes      # (the closed form, in Python)
    pairs = _heavy_batch(scores, refused, takes, ("all_mismatch", "all_match"))
    _run_checked(gx, ctx, oracle, pairs, steps=2, scores=scores, band_waves=takes)
    assert ctx.fill_info()["score_table"] == 1


def test_plain_match_five_symbols(gx, ctx, oracle):
    """The plain match test at four rows on its own terms: ACGTN pairs at the
    default scores over the row and column edges, and (1, -1, 0, -5) on ACGT,
    whose shifted mismatch score (-1) keeps the twin off its score tables."""
    rng = random.Random(26)
    cols = [1, 17, 64, 129]
    five = [(_dna(rng, n, b"ACGTN"), _dna(rng, m, b"ACGTN")) for n in ROWS_N for m in cols]
    _run_checked(gx, ctx, oracle, five, steps=2)
    assert ctx.fill_info()["score_table"] == 0, ctx.fill_info()
    four = [(_dna(rng, n), _dna(rng, m)) for n in ROWS_N for m in COLS_M[1::2]]
    _run_checked(gx, ctx, oracle, four, steps=2, scores=(1, -1, 0, -5))
    assert ctx.fill_info()["score_table"] == 0, ctx.fill_info()
    _run_checked(gx, ctx, oracle, four, steps=1)            # (and the same pairs through the tables)
    assert ctx.fill_info()["score_table"] == 1, ctx.fill_info()


_EDGE_REF = {}


def _edge_reference(oracle, scores, kinds):
    key = (scores, kinds)
    if key not in _EDGE_REF:
        pairs = edge_batch_rows4(kinds)
        _EDGE_REF[key] = (pairs, [oracle.align(a, b, scores, want_planes=True) for a, b in pairs])
    return _EDGE_REF[key]


@pytest.mark.parametrize("alphabet", ["five_symbols", "four_symbols"])
@pytest.mark.parametrize("scores", EDGE_SCORES, ids=lambda s: "_".join(map(str, s)))
def test_code_field_edges_rows4(gx, ctx, oracle, monkeypatch, scores, alphabet):
    """Scores that attain x_S = -16 and 15 (tests/test_formats.py proves it of
    this batch) at four rows, asked for 8-strip bands: (15, -1, 0, 0) and
    (-15, -16, 0, -15) are admitted up to 4, where the 1,100-row pair crosses
    a band edge.  Every plane cell of every pair, the results and alignments."""
    monkeypatch.setenv("GX_BAND_WAVES", "8")
    kinds = EDGE_KINDS if alphabet == "five_symbols" else tuple(k for k in EDGE_KINDS if k != "acgtn")
    pairs, full = _edge_reference(oracle, scores, kinds)
    W = _admitted_width(gx, scores, 8, gaps=(0, 300))     # (no two pairs of the batch lie further apart)
    assert W == (4 if scores in EDGE_SCORES[:2] else 8)
    _run_checked(gx, ctx, oracle, pairs, steps=2, scores=scores, band_waves=W)
    sm, smm, g = scores[:3]
    tables = alphabet == "four_symbols" and min(sm, smm) - 2 * g >= 0      # gx_api_fill.cpp twin_tbl
    assert ctx.fill_info()["score_table"] == (1 if tables else 0), ctx.fill_info()
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*scores), False, keep_planes=True, steps=1, keep=True)
    info = ctx.fill_info()
    assert (info["twin"], info["twin_rows"], info["band_waves"], info["plane_bytes_per_cell"]) == (1, 4, W, 1.5), info
    for p, (a, b) in enumerate(pairs):
        assert res[p].score == full[p].score, p
        t = st.table(p)
        _assert_planes(t, len(a), full[p].planes, (scores, alphabet, p, len(a), len(b)))
        t.free()


@pytest.mark.parametrize("scores", [CONFIG_SCORES, (1, -1, -5, 0)], ids=lambda s: "_".join(map(str, s)))
def test_twins_far_apart(gx, ctx, oracle, monkeypatch, scores):
    """Twins exactly 1,024 columns apart (the pairing rule's cap): the column
    gap enters the bound, 28,882 at the default scores and 8-strip bands --
    still admitted -- while (1, -1, -5, 0) is refused at 8 and 7 and takes 4."""
    monkeypatch.setenv("GX_BAND_WAVES", "8")
    W = _admitted_width(gx, scores, 8, gaps=(1024,))
    assert W == (8 if scores == CONFIG_SCORES else 4)
    if scores == CONFIG_SCORES:
        assert gx.twin_admission(gx.Scores(*scores), 8, 1024, rows_per_lane=4) == (True, 28882)
    rng = random.Random(1024)
    n = 2200
    # (twins by columns: the first two pairs together, the third with the 1,976-column one)
    pairs = [(b"A" * n, b"A" * 3000), ((b"AC" * n)[:n], (b"CA" * 3000)[:3000]), (_dna(rng, n), _dna(rng, 3000)),
             (_dna(rng, n), _dna(rng, 1976))]
    _run_checked(gx, ctx, oracle, pairs, steps=2, scores=scores, band_waves=W)


def test_column_limit_rows4(gx, ctx, oracle):
    """65,536 columns at four rows: the launch keeps no skeleton, so no int16
    column quantity is left and no column limit applies; rows either side of
    the 256-row strip edge."""
    rng = random.Random(65536)
    m = 65536
    pairs = [(_dna(rng, n), _dna(rng, mm)) for n, mm in [(260, m), (257, m - 7), (300, m - 1)]]
    _run_checked(gx, ctx, oracle, pairs)


def _check_lean(gx, ctx, oracle, pairs, distinct, rows, band_waves=None):
    """One run of a batch that repeats `distinct` pairs: fill_info, every
    pair's results and plane checksums, the first and last repeats' alignments."""
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*CONFIG_SCORES), False, keep_planes=True, steps=1, plane_sums=True)
    info = ctx.fill_info()
    assert info["twin"] == 1 and info["twin_rows"] == rows and info["plane_bytes_per_cell"] == 1.5, info
    if band_waves is not None:
        assert info["band_waves"] == band_waves, info
    sums = st.plane_sums()
    for p, (a, b) in enumerate(pairs):
        o = _lean(oracle, a, b)
        assert [int(x) for x in sums[0, p]] == o.extra["plane_sums"], p
        assert _stats(res[p]) == (o.score, o.matches, o.mismatches, o.gap_extensions, o.opening_gaps,
                                  len(o.choices)), p
        if p < distinct or p >= len(pairs) - distinct:
            assert _steps_list(st.steps(p)) == o.alignment(), p
    return info


def _cu_count(gx, device):
    """The device's CU count as fill_grid_cap reads it, from the HIP runtime
    the library is linked to (a dependency's symbols resolve through the
    library's handle); None when the runtime will not say."""
    v = ctypes.c_int(0)
    fn = gx.lib().hipDeviceGetAttribute
    fn.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int]
    rc = fn(ctypes.byref(v), 63, device)     # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    return v.value if rc == 0 and 1 <= v.value <= 4096 else None


def test_default_launch_takes_four_rows(gx, ctx, oracle, monkeypatch):
    """Nothing forced: pairs of 2,048 rows (8 strips of 256), two per CU (one
    8-strip twin band each), take four rows at 8-strip bands with the score
    tables; the same batch at 1,792 rows (7 strips) keeps two rows a lane
    (gx_api_plan.cpp twin_rows4_auto)."""
    for k in ("GX_TWIN", "GX_TWIN_ROWS", "GX_BAND_WAVES", "GX_FILL_GRID", "GX_LAYOUT"):
        monkeypatch.delenv(k, raising=False)
    cus = _cu_count(gx, ctx.device)      # (256 on an MI355X: 512 pairs)
    if cus is None:
        pytest.skip("the HIP runtime did not report the device's CU count")
    rng = random.Random(2048)
    base = [(_dna(rng, 2048), _dna(rng, 96)) for _ in range(8)]
    P = 2 * cus
    shapes = [(2048, 96)] * P
    assert gx.plan_twin_rows(gx.Scores(*CONFIG_SCORES), shapes, cus) == (4, 8)
    info = _check_lean(gx, ctx, oracle, [base[p % 8] for p in range(P)], 8, rows=4, band_waves=8)
    assert info["score_table"] == 1 and info["layout"] == 0, info
    short = [(a[:1792], b) for a, b in base]
    assert gx.plan_twin_rows(gx.Scores(*CONFIG_SCORES), [(1792, 96)] * P, cus)[0] == 2
    _check_lean(gx, ctx, oracle, [short[p % 8] for p in range(P)], 8, rows=2)
