"""CPU: the twin fill's int16 admission rule at four rows a lane (256-row
strips, gx_api_plan.cpp twin_bound / gx_twin_admission_rows) against
brute-force spreads measured with the oracle, as tests/test_twin_bound.py does
for the 128-row strips.

With four rows a lane a strip is 256 rows tall, while the base a strip holds
still lags one lane = one column per lane behind the cell (each strip adopts
the base of the block it consumes, so strip k's base column lies up to
64 (k + 1) + 16 columns right of the cell whatever the rows per lane).  Strip
k's lowest row is 256 (k + 1) rows below the band's top row, so a value of
strip k lies within D (320 (k + 1) + 16 + dm) of its base and the host admits
a band width W only when D (320 W + 16 + dm) + 2 (|a| + |smax| + |smin|) + 64 <
30,000 (D the largest neighbour difference of the shifted values, DESIGN.md
6.5).

For every instantiated band width, at the default scores (where that width is
admitted) and at the widest scores the width admits, the oracle's planes give
every cell's I'', D'', S'' and score_max''; every cell of strip k of every
256-row-strip band is compared with every base the kernel could hold for it,
and the largest spread must stay within the per-strip term of the rule.  One
step past the widest scores the launch must be refused.
"""
import numpy as np
import pytest

from conftest import CONFIG_SCORES
from test_twin_bound import _families, _neighbour_d

ROWS = 256            # rows per strip at four rows a lane
STEPS = ROWS + 64     # neighbour steps a strip adds to the bound: its rows + one column of lag per lane
WIDTHS = (3, 4, 7, 8, 15)   # gx_fill_pk.hip launch_fill_pk


def _const(scores):
    sm, smm, g, h = scores
    return 2 * (abs(h + g) + abs(max(sm, smm)) + abs(min(sm, smm))) + 64


def _closed_form(scores, W, dm=0):
    return _neighbour_d(scores) * (STEPS * W + 16 + dm) + _const(scores)


def _edge_scores(W):
    """(1, -1, 0, h) with the most negative h whose closed-form bound at W
    stays below 30,000: D = 1 - h, the widest scores W admits at four rows."""
    h = 0
    while _closed_form((1, -1, 0, h - 1), W) < 30000:
        h -= 1
    return (1, -1, 0, h)


def _max_spread_ratio(planes, g, W, dm):
    """Largest spread of strip k over its per-strip bound term, over every
    band and strip of 256 rows: max |V''(i, j) - SM''(r0, c)| / (320 (k + 1) +
    16 + dm), c over the columns whose base the strip could hold."""
    from scipy.ndimage import maximum_filter1d, minimum_filter1d
    I, D, S = (p.astype(np.int64) for p in planes)
    n1, m1 = I.shape
    ii = np.arange(n1)[:, None]
    jj = np.arange(m1)[None, :]
    shift = (ii + jj) * g
    SM = np.maximum(np.maximum(I, D), S) - shift
    worst = 0.0
    for r0 in range(0, n1 - 1, ROWS * W):
        top = SM[r0]
        for k in range(W):
            lo_r, hi_r = r0 + ROWS * k + 1, min(r0 + ROWS * (k + 1), n1 - 1)
            if lo_r > hi_r:
                break
            sl = slice(lo_r, hi_r + 1)
            vals = [I[sl, 1:] - shift[sl, 1:], D[sl, 1:] - shift[sl, 1:], S[sl, 1:] - shift[sl, 1:], SM[sl, 1:]]
            vmax = np.max(np.stack([v.max(axis=0) for v in vals]), axis=0)
            vmin = np.min(np.stack([v.min(axis=0) for v in vals]), axis=0)
            # bases over c in [j - 32, j + 64 (k + 1) + 32 + dm], clamped to [0, m]
            left, right = 32, 64 * (k + 1) + 32 + dm
            size = left + right + 1
            pad = np.concatenate([np.full(left, top[0]), top, np.full(right, top[-1])])
            wmax = maximum_filter1d(pad, size, origin=-(size // 2))[1:m1]
            wmin = minimum_filter1d(pad, size, origin=-(size // 2))[1:m1]
            spread = max(int((vmax - wmin).max()), int((wmax - vmin).max()))
            worst = max(worst, spread / (STEPS * (k + 1) + 16 + dm))
    return worst


CASES = [(CONFIG_SCORES, W) for W in WIDTHS if _closed_form(CONFIG_SCORES, W) < 30000] + \
        [(_edge_scores(W), W) for W in WIDTHS]


def test_default_scores_widths():
    """The default scores: 18,130 at W = 7 and 20,690 at W = 8, under the
    limit; 15-strip bands of 256-row strips are not (38,610)."""
    assert _closed_form(CONFIG_SCORES, 7) == 8 * (320 * 7 + 16) + 2 * (6 + 1 + 2) + 64 == 18130
    assert [W for s, W in CASES if s == CONFIG_SCORES] == [3, 4, 7, 8]
    assert _closed_form(CONFIG_SCORES, 15) >= 30000


@pytest.mark.parametrize("scores,W", CASES)
def test_admission_rule_rows4(gx, scores, W):
    """gx_twin_admission_rows(rows = 4) is the closed form, admits W, and
    agrees with the two-row export at rows = 2."""
    s = gx.Scores(*scores)
    ok, bound = gx.twin_admission(s, W, 0, rows_per_lane=4)
    assert bound == _closed_form(scores, W) and ok and bound < 30000, (scores, W, bound)
    ok_d, bound_d = gx.twin_admission(s, W, 700, rows_per_lane=4)
    assert bound_d == _closed_form(scores, W, 700) and ok_d == (bound_d < 30000)
    b2 = ctypes_bound(gx, s, W, 2)
    assert b2 == gx.twin_admission(s, W, 0)[1] == _neighbour_d(scores) * (192 * W + 16) + _const(scores)


def ctypes_bound(gx, s, W, rows):
    import ctypes
    b = ctypes.c_int64(0)
    assert gx.lib().gx_twin_admission_rows(ctypes.byref(s.c()), 0, W, 0, rows, ctypes.byref(b)) in (0, 1)
    return int(b.value)


@pytest.mark.parametrize("W", WIDTHS)
def test_launch_beyond_bound_refused(gx, W):
    """One step past the widest scores of W the four-row launch is refused at
    W (run_fill then narrows the band or keeps two rows a lane); the next
    wider instantiated width refuses the edge scores themselves; local fills
    and other row counts are never admitted."""
    sm, smm, g, h = _edge_scores(W)
    ok, bound = gx.twin_admission(gx.Scores(sm, smm, g, h - 1), W, 0, rows_per_lane=4)
    assert not ok and bound >= 30000, (W, bound)
    wider = {3: 4, 4: 7, 7: 8, 8: 15}.get(W)
    if wider:
        assert not gx.twin_admission(gx.Scores(sm, smm, g, h), wider, 0, rows_per_lane=4)[0]
    assert not gx.twin_admission(gx.Scores(*CONFIG_SCORES), 3, 0, is_local=True, rows_per_lane=4)[0]
    with pytest.raises(gx.GxError):
        gx.twin_admission(gx.Scores(*CONFIG_SCORES), 3, 0, rows_per_lane=3)


@pytest.mark.parametrize("scores,W", CASES)
@pytest.mark.parametrize("family", ["all_mismatch", "all_match", "gap_rows", "gap_cols", "repeat", "random"])
def test_spread_within_rule_rows4(oracle, scores, W, family):
    """Brute force: every state of every 256-row strip of every band stays
    within the rule's per-strip term of every base the kernel could hold."""
    n = ROWS * W * 2 + 150          # two full bands and a partial third
    m = 900
    a, b = _families(n, m)[family]
    o = oracle.align(a, b, scores, want_planes=True)
    ratio = _max_spread_ratio(o.planes, scores[2], W, 0)
    d = _neighbour_d(scores)
    assert ratio <= d, (family, scores, W, ratio, d)


def test_spread_unequal_twins_rows4(oracle):
    """A twin's shorter pair 700 columns narrower (the margin dm) at W = 8."""
    W, dm = 8, 700
    rng = np.random.default_rng(5)
    n, m = ROWS * W + 200, 900
    a = bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    b = bytes(rng.choice(list(b"AC"), size=m).tolist())
    o = oracle.align(a, b, CONFIG_SCORES, want_planes=True)
    assert _max_spread_ratio(o.planes, CONFIG_SCORES[2], W, dm) <= _neighbour_d(CONFIG_SCORES)
