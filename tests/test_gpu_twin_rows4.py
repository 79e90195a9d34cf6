"""GPU parity of the twin fill at four rows a lane (gx_fill_pk.hip R = 4:
256-row strips; GX_TWIN_ROWS=4 forces it, GX_TWIN=1 the twin fill itself).

The batch fill with twin plane codes gives a lane four rows instead of two, so
that every per-step cost of the band pipeline is paid once per four rows.
Strips are 256 rows, the code plane keeps [group][row-in-lane][lane] records
with four rows a group, and every decoder (plane checksums, exports, the
sequential traceback over four 64-row blocks a strip) addresses it through
gx_device.h w12_rec_off with the launch's rows per lane.

Every case is checked against the oracle for score, statistics, the alignment
(step for step) and the three plane checksums; small cases also compare the
exported planes cell for cell.  Shapes are the smallest at which the new code
can go wrong: every n mod 4, a partial last lane, the 256-row strip edge,
sub-block and lane-skew column edges, twins of unequal shape, a self-twin,
band hand-offs through HBM, moving bases, and walks across the four blocks of
a strip.  The same batches at two rows a lane must agree with both."""
import os
import random
import sys

import numpy as np
import pytest

from conftest import CONFIG_SCORES, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the related-pair recipe)

pytestmark = pytest.mark.gpu

NAMES = ["Match", "Mismatch", "Insert", "Delete", "OpenInsert", "OpenDelete"]
ROWS_N = [1, 3, 4, 5, 255, 256, 257, 511, 513]
COLS_M = [1, 15, 16, 17, 63, 64, 65, 129]


def _steps_list(steps):
    return [(NAMES[int(c)], int(i), int(j)) for c, i, j in zip(steps["choice"], steps["i"], steps["j"])]


def _dna(rng, k, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(k))


@pytest.fixture(autouse=True)
def _force_rows4(monkeypatch):
    monkeypatch.setenv("GX_TWIN", "1")
    monkeypatch.setenv("GX_TWIN_ROWS", "4")
    monkeypatch.setenv("GX_LAYOUT", "0")


_ORACLE = {}


def _lean(oracle, a, b, scores=CONFIG_SCORES):
    """The oracle's result of a pair, computed once and shared."""
    key = (a, b, scores)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.align_lean(a, b, scores)
    return _ORACLE[key]


def _stats(r):
    return (r.score, r.matches, r.mismatches, r.gap_extensions, r.opening_gaps, r.n_steps)


def _run_checked(gx, ctx, oracle, pairs, steps=1, rows=4, scores=CONFIG_SCORES, band_waves=None, groups=None):
    """A staged run with planes: every pass's plane checksums and results and
    the last pass's alignments against the oracle; returns (results, sums)."""
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*scores), False, keep_planes=True, steps=steps, plane_sums=True)
    info = ctx.fill_info()
    assert info["twin"] == 1 and info["twin_rows"] == rows and info["plane_bytes_per_cell"] == 1.5, info
    if band_waves is not None:
        assert info["band_waves"] == band_waves, info
    if groups is not None:
        assert info["groups"] == groups, info
    sums = st.plane_sums().copy()
    passes = st.pass_results()
    assert len(passes) == steps
    for p, (a, b) in enumerate(pairs):
        o = _lean(oracle, a, b, scores)
        want = (o.score, o.matches, o.mismatches, o.gap_extensions, o.opening_gaps, len(o.choices))
        for k in range(steps):
            assert [int(x) for x in sums[k, p]] == o.extra["plane_sums"], (p, len(a), len(b), k)
            assert _stats(passes[k][p]) == want, (p, len(a), len(b), k)
        assert _stats(res[p]) == want, (p, len(a), len(b))
        assert _steps_list(st.steps(p)) == o.alignment(), (p, len(a), len(b))
    return [_stats(r) for r in res], sums


def _grid_pairs():
    rng = random.Random(4)
    return [(_dna(rng, n, b"ACGT" if (n + m) % 3 else b"AC"), _dna(rng, m, b"ACGT" if (n + m) % 3 else b"AC"))
            for n in ROWS_N for m in COLS_M]


def test_rows_and_columns_grid(gx, ctx, oracle):
    """Every n in ROWS_N with every m in COLS_M in one batch: twins are formed
    by shape, so pairs of equal m and different n share a twin (n0 != n1 across
    the strip edge); and the same with one pair more (an odd count: a self-twin)."""
    pairs = _grid_pairs()
    _run_checked(gx, ctx, oracle, pairs)
    rng = random.Random(5)
    _run_checked(gx, ctx, oracle, pairs[:8] + [(_dna(rng, 300), _dna(rng, 77))])


def test_unequal_twins(gx, ctx, oracle):
    """Twins of unequal shape: rows either side of a strip edge, columns either
    side of a sub-block and of the lane skew, and an odd pair count."""
    rng = random.Random(6)
    shapes = [(255, 129), (257, 120), (513, 64), (256, 17), (511, 300), (4, 290), (300, 1)]
    pairs = [(_dna(rng, n), _dna(rng, m)) for n, m in shapes]
    _run_checked(gx, ctx, oracle, pairs, steps=2)


@pytest.mark.parametrize("n", [800, 1537])
def test_band_handoff_through_hbm(gx, ctx, oracle, monkeypatch, n):
    """3-strip bands: n = 800 is a full band and a last band of one strip, n =
    1,537 two full bands and a single-strip third; band rows pass through HBM."""
    monkeypatch.setenv("GX_BAND_WAVES", "3")
    monkeypatch.setenv("GX_FILL_GRID", "2")
    rng = random.Random(n)
    pairs = [(_dna(rng, n), _dna(rng, 333)), (_dna(rng, n - 5), _dna(rng, 300)), (_dna(rng, n), _dna(rng, 129))]
    _run_checked(gx, ctx, oracle, pairs, band_waves=3)


def test_band_width_narrowed_by_bound(gx, ctx, oracle, monkeypatch):
    """15-strip bands of 256-row strips exceed the int16 bound at the default
    scores (tests/test_twin_bound_r4.py): the launch takes the widest admitted
    width instead, 8."""
    monkeypatch.setenv("GX_BAND_WAVES", "15")
    rng = random.Random(15)
    pairs = [(_dna(rng, 600), _dna(rng, 200)), (_dna(rng, 500), _dna(rng, 210))]
    _run_checked(gx, ctx, oracle, pairs, band_waves=8)


def test_base_changes(gx, ctx, oracle):
    """An all-match pair twinned with an all-mismatch pair over 2,000 columns:
    the halves' bases move apart, and the lanes rebase four rows."""
    pairs = [(b"A" * 300, b"A" * 2000), (b"A" * 290, b"C" * 1990)]
    _run_checked(gx, ctx, oracle, pairs, steps=2)


def test_traceback_across_blocks(gx, ctx, oracle):
    """The sequential walk over the four 64-row blocks of a strip: a related
    pair at 1,000 x 1,000 (the benchmark's recipe) beside a gapped pair whose
    walk starts in the third block of its last strip (n = 256 + 2 x 64 + 30)
    and crosses blocks and the strip edge through long gaps."""
    a, b = bench.related_pair(3, 1000)
    rng = random.Random(8)
    s1 = _dna(rng, 414)
    s2 = s1[:100] + s1[170:300] + _dna(rng, 45) + s1[300:]      # a 70-row delete run and a 45-column insert run
    pairs = [(a, b), (s1, s2)]
    _run_checked(gx, ctx, oracle, pairs, steps=2)


def test_pipelined_passes(gx, ctx, oracle, monkeypatch):
    """StagedPairs.run(steps=3) on 16 pairs of 4,200 x 4,200 through the
    overlapped two-group pipeline: every pass's results and checksums."""
    monkeypatch.setenv("GX_OVERLAP", "1")
    pairs = [bench.synth_pair(k, 4200) if k % 2 else bench.related_pair(k, 4200) for k in range(16)]
    pairs = [(a[:4200], b[:4200]) for a, b in pairs]
    _run_checked(gx, ctx, oracle, pairs, steps=3, groups=2)


def test_two_rows_unchanged_and_equal(gx, ctx, oracle, monkeypatch):
    """The same batch at two rows a lane (GX_TWIN_ROWS=2): identical results
    and plane checksums (checksums do not depend on the layout), equal to the
    four-row run's and to the oracle's."""
    rng = random.Random(9)
    shapes = [(513, 129), (511, 140), (257, 65), (900, 700), (890, 650), (5, 17), (256, 64)]
    pairs = [(_dna(rng, n), _dna(rng, m)) for n, m in shapes]
    r4, s4 = _run_checked(gx, ctx, oracle, pairs, steps=2, rows=4)
    monkeypatch.setenv("GX_TWIN_ROWS", "2")
    r2, s2 = _run_checked(gx, ctx, oracle, pairs, steps=2, rows=2)
    assert r2 == r4 and np.array_equal(s2, s4)


def test_exported_planes_cell_for_cell(gx, ctx, oracle):
    """Tables of a kept four-row run (gx_staged_table): every cell of the I, D
    and S planes, exported row range by row range across the strip and block
    edges, equals the oracle's."""
    rng = random.Random(10)
    shapes = [(300, 129), (513, 65), (257, 17), (5, 300), (256, 64)]
    pairs = [(_dna(rng, n), _dna(rng, m)) for n, m in shapes]
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*CONFIG_SCORES), False, keep_planes=True, steps=1, keep=True)
    info = ctx.fill_info()
    assert info["twin"] == 1 and info["twin_rows"] == 4 and info["plane_bytes_per_cell"] == 1.5, info
    for p, (a, b) in enumerate(pairs):
        o = oracle.align(a, b, CONFIG_SCORES, want_planes=True)
        assert res[p].score == o.score, p
        t = st.table(p)
        for which in range(3):
            got = np.concatenate([t.rows(which, r0, min(100, len(a) + 1 - r0)) for r0 in range(0, len(a) + 1, 100)])
            assert np.array_equal(got, o.planes[which]), (p, which)
        t.free()
