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

Those (1, -1, 0, h) scores leave the bound loose by a factor of 2 to 8.
HEAVY_CASES below are the scores whose gap extension dominates D: the same
inputs must reach 0.75 D of the rule there, which is what lets the GPU runs of
tests/test_gpu_twin_rows4_edges.py load the int16 halves.  Last, the launch's
rows-per-lane rule (gx_api_plan.cpp twin_plan, through gx_plan_twin_rows) is
held at each of its thresholds against a restatement in Python.
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


# ---- scores whose gap extension dominates the neighbour step D ----
# With h = 0 and a large |g| the worst-input families attain 256 of the 325
# steps of a strip's term (its rows; 0.787 D), where the (1, -1, 0, h) edge
# scores above stay below 0.3 D: these are the scores that bring a half-word
# near its limit, each at the widest width it admits (and the
# last at W = 3 too, to load that kernel).  All satisfy w16_ok and d8_planes_ok.
HEAVY_CASES = [((0, -1, -3, 0), 15), ((1, -1, -5, 0), 8), ((1, -1, -6, 0), 7), ((1, -1, -7, 0), 4),
               ((1, -1, -7, 0), 3)]
# one step past: (scores, the width refused, the width the launch takes instead)
ONE_PAST = [((1, -1, -3, 0), 15, 8), ((1, -1, -6, 0), 8, 7), ((1, -1, -7, 0), 7, 4)]
FAMILIES = ["all_mismatch", "all_match", "gap_rows", "gap_cols", "repeat", "random"]
WIDER = {3: 4, 4: 7, 7: 8, 8: 15}


def widest_admitted(scores, want, dm=0):
    """twin_width's choice at four rows: the widest instantiated width <= want
    (3 whatever was asked) whose closed-form bound stays below 30,000; 0: none."""
    for W in sorted(WIDTHS, reverse=True):
        if (W <= want or W == 3) and _closed_form(scores, W, dm) < 30000:
            return W
    return 0


def test_heavy_cases_sit_at_their_widths():
    """The closed-form bounds the cases were chosen by, and that the plane
    formats admit them (test_formats restates w16_ok)."""
    from test_formats import _w16_ok
    assert [_closed_form(s, W) for s, W in HEAVY_CASES] == [28968, 28414, 29408, 19522, 14722]
    assert [_closed_form(s, W) for s, W, _ in ONE_PAST] == [33786, 33568, 33922]
    assert all(_w16_ok(*s) for s, _ in HEAVY_CASES) and all(_w16_ok(*s) for s, _, _ in ONE_PAST)
    assert max(1, -1) - 2 * (0 - 7) == 15     # (1, -1, -7, 0): x_S reaches the code field's own end


@pytest.mark.parametrize("scores,W", HEAVY_CASES)
def test_heavy_admission_rows4(gx, scores, W):
    """gx_twin_admission_rows(rows = 4) is the closed form and admits W; the
    next wider instantiated width refuses these scores (but for the W = 3 row,
    which repeats the W = 4 scores to run that kernel under load)."""
    s = gx.Scores(*scores)
    ok, bound = gx.twin_admission(s, W, 0, rows_per_lane=4)
    assert bound == _closed_form(scores, W) and ok and bound < 30000, (scores, W, bound)
    if W != 3:
        assert widest_admitted(scores, 15) == W
    if W in (4, 7, 8):     # (15 is the widest instantiated)
        ok_w, bound_w = gx.twin_admission(s, WIDER[W], 0, rows_per_lane=4)
        assert bound_w == _closed_form(scores, WIDER[W]) and not ok_w and bound_w >= 30000


@pytest.mark.parametrize("scores,refused,takes", ONE_PAST)
def test_one_past_narrows_on_the_host(gx, monkeypatch, scores, refused, takes):
    """One step past a width's heaviest scores the admission export refuses
    it, admits the narrower width, and the launch rule (gx_plan_twin_rows)
    asked for the refused width takes the narrower one at four rows."""
    s = gx.Scores(*scores)
    assert not gx.twin_admission(s, refused, 0, rows_per_lane=4)[0]
    assert gx.twin_admission(s, takes, 0, rows_per_lane=4)[0]
    assert widest_admitted(scores, refused) == takes
    assert all(not gx.twin_admission(s, W, 0, rows_per_lane=4)[0] for W in WIDTHS if takes < W <= refused)
    _plan_env(monkeypatch, GX_TWIN="1", GX_TWIN_ROWS="4", GX_LAYOUT="0", GX_BAND_WAVES=str(refused))
    assert gx.plan_twin_rows(s, [(ROWS * refused * 2 + 150, 900)] * 6) == (4, takes)


_RATIO = {}


def _heavy_ratio(oracle, scores, W, family):
    """The attained spread ratio of a family at n = 256 W 2 + 150, m = 900, computed once."""
    key = (scores, W, family)
    if key not in _RATIO:
        a, b = _families(ROWS * W * 2 + 150, 900)[family]
        o = oracle.align(a, b, scores, want_planes=True)
        _RATIO[key] = _max_spread_ratio(o.planes, scores[2], W, 0)
    return _RATIO[key]


@pytest.mark.parametrize("scores,W", HEAVY_CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_heavy_spread_within_rule(oracle, scores, W, family):
    """Every state of every 256-row strip stays within the rule's per-strip term."""
    d = _neighbour_d(scores)
    ratio = _heavy_ratio(oracle, scores, W, family)
    assert ratio <= d, (family, scores, W, ratio, d)


@pytest.mark.parametrize("scores,W", HEAVY_CASES)
def test_heavy_spread_loads_the_rule(oracle, scores, W):
    """... and the families reach at least 0.75 D of it: a strip's rows are
    256 of the 325 steps of its term (0.787), less a margin for the partial
    third band.  A property of the oracle and the inputs: it is what lets the
    GPU runs of these cases (tests/test_gpu_twin_rows4_edges.py) bring the
    int16 halves near the limit the rule guards."""
    d = _neighbour_d(scores)
    ratios = {f: _heavy_ratio(oracle, scores, W, f) for f in FAMILIES}
    assert max(ratios.values()) >= 0.75 * d, (scores, W, d, ratios)


# ---- the rows-per-lane rule of a launch (gx_api_plan.cpp twin_plan, gx_plan_twin_rows) ----
PLAN_ENV = ("GX_TWIN", "GX_TWIN_ROWS", "GX_BAND_WAVES", "GX_FILL_GRID", "GX_LAYOUT")
FILL_WIDTHS = (3, 4, 6, 8, 11, 15)    # gx_internal.h kFillWidths


def _plan_env(monkeypatch, **env):
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _cdiv(a, b):
    return -(-a // b)


def _queue_width(total_strips, grid_cap):
    """fill_band_waves for short pairs: the narrowest width up to 8 whose
    bands fit the grid, else 8-strip bands that queue."""
    for x in FILL_WIDTHS:
        if x <= 8 and _cdiv(total_strips, x) <= grid_cap:
            return x
    return 8


def _rows_rule(scores, shapes, grid_cap, env):
    """The documented rule for a global launch that is the twin fill with
    twin plane codes: four rows when forced (GX_TWIN_ROWS=4), or unasked when
    neither band width nor grid is given, every pair has >= 8 strips of 256
    rows and the twins' strips make >= one 8-strip band per CU; never with
    GX_TWIN_ROWS=2, without twin codes, or when no width is admitted.  The
    band width: the one asked for or min(8, the queue rule on the 256-row
    strips), narrowed to the widest admitted.  Returns (rows, W or None)."""
    from test_formats import _w16_ok
    if not _w16_ok(*scores):
        return 2, None
    strips4 = [_cdiv(n, ROWS) for n, _ in shapes]
    twin_strips4 = sum(strips4) // 2
    force = int(env.get("GX_TWIN_ROWS", "0"))
    plain = "GX_BAND_WAVES" not in env and "GX_FILL_GRID" not in env
    auto = plain and min(strips4) >= 8 and _cdiv(twin_strips4, 8) >= grid_cap
    if force == 2 or not (force == 4 or auto):
        return 2, None
    want = int(env["GX_BAND_WAVES"]) if "GX_BAND_WAVES" in env else min(8, _queue_width(twin_strips4, grid_cap))
    dm = max(m for _, m in shapes) - min(m for _, m in shapes)   # (an upper bound of any twin's gap; 0 below)
    W = widest_admitted(scores, want, dm)
    return (4, W) if W else (2, None)


SHORT = [(300, 100), (600, 100), (257, 100)]


@pytest.mark.parametrize("cap", [256, 100])
def test_plan_twin_rows_thresholds(gx, monkeypatch, cap):
    """gx_plan_twin_rows (the function run_fill calls) at each threshold of
    the rule, the expectation derived from _rows_rule, never read back."""
    s = gx.Scores(*CONFIG_SCORES)
    P = 2 * cap                         # pairs of 8 strips: P / 2 twins, one 8-strip band each
    full = [(2048, 100)] * P
    # (the big batches take the twin fill unasked: their 128-row-strip bands outnumber 0.9 x the grid)
    assert 10 * (P // 2) * _cdiv(_cdiv(1792, 128), 8) >= 9 * cap

    def check(shapes, want_rows, want_w=None, scores=CONFIG_SCORES, **env):
        _plan_env(monkeypatch, **env)
        assert _rows_rule(scores, shapes, cap, env)[0] == want_rows
        if want_w is not None:
            assert _rows_rule(scores, shapes, cap, env)[1] == want_w
        rows, W = gx.plan_twin_rows(gx.Scores(*scores), shapes, cap)
        assert rows == want_rows, (shapes[:3], len(shapes), env, rows, W)
        if want_w is not None:
            assert W == want_w, (shapes[:3], len(shapes), env, rows, W)
        return W

    check(full, 4, 8)
    assert check([(1792, 100)] * P, 2) > 0                       # 7 strips a pair (still the twin fill)
    check([(1792, 100)] + full[1:], 2)                           # one such pair among the rest
    check(full[:-2], 2)                                          # cap - 1 bands
    check(full, 2, GX_BAND_WAVES="8")
    check(full, 2, GX_FILL_GRID=str(cap))
    check(full, 2, GX_TWIN_ROWS="2")
    check(full, 4, 8, GX_TWIN_ROWS="4", GX_BAND_WAVES="8")       # forced: a given width does not matter
    # small forced launches (GX_TWIN=1 and GX_LAYOUT=0 make three short pairs a layout-0 twin fill)
    check(SHORT, 4, 3, GX_TWIN="1", GX_LAYOUT="0", GX_TWIN_ROWS="4")
    check(SHORT, 2, GX_TWIN="1", GX_LAYOUT="0")
    check(SHORT, 4, 8, GX_TWIN="1", GX_LAYOUT="0", GX_TWIN_ROWS="4", GX_BAND_WAVES="15")
    check(SHORT, 4, 7, GX_TWIN="1", GX_LAYOUT="0", GX_TWIN_ROWS="4", GX_BAND_WAVES="7")
    # (1, -1, 0, -20): x_S up to 41, outside the code field: no twin codes, so no four rows
    check(SHORT, 2, scores=(1, -1, 0, -20), GX_TWIN="1", GX_LAYOUT="0", GX_TWIN_ROWS="4")
    with pytest.raises(gx.GxError):
        gx.plan_twin_rows(s, [(0, 100)], cap)
