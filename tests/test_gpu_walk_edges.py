"""GPU parity of the two device walkers on planted paths (gx_kernels.hip
tb_chase_kernel + tb_strip_kernel with kTbWin = 32 words, tb_seq_kernel with
kSqWin = 12; both through tb_walk_block; records labelled by gx_api_walk.cpp
label_walk_records).

Every walker launch runs the whole case list of its geometry
(tests/test_walk_cases.py, where each case is shown on the CPU to reach the
branch it was planted for: word edges, the table, the scan below the window,
entries below the window, runs to column 0, moves onto column 0 and row 0,
block and strip edges, adjacent runs, the last word of a row) as one batch per
score set and mode, and every pair must equal the oracle step for step and in
score, matches, mismatches, gap extensions, gap openings and step count.  Each
test first asserts from fill_info that the launch is the one it names; staged
launches also check the plane checksums, so that a wrong fill is not blamed
on the walk.  Twins are formed by shape and an odd count leaves a self-twin."""
import pytest

from conftest import CONFIG_SCORES
from test_walk_cases import cases, dear_scores, oracle_result
from walk_model import GEOMETRIES

pytestmark = pytest.mark.gpu

NAMES = ["Match", "Mismatch", "Insert", "Delete", "OpenInsert", "OpenDelete"]

# launch -> (environment, geometry, staged with planes, what fill_info must show)
LAUNCHES = {
    "scalar_layout0": ({"GX_TWIN": "0", "GX_LAYOUT": "0"}, "lay0", False, {"layout": 0, "twin": 0}),
    "layout1_one_wave": ({"GX_LAYOUT": "1", "GX_CS2": "0"}, "lay1", False, {"layout": 1}),
    # (every case has g <= 0: the split column step takes local fills too, test_gpu_parity.py test_untracked_table_planes)
    "split_column_step": ({"GX_LAYOUT": "1", "GX_CS2": "1"}, "lay1", False, {"layout": 2}),
    "skewed_strips": ({"GX_LAYOUT": "3"}, "lay3", False, {"layout": 3}),
    "twin_int16_skeleton": ({"GX_TWIN": "1", "GX_LAYOUT": "0"}, "lay0", False, {"twin": 1, "plane_bytes_per_cell": 0}),
    "twin_byte_planes": ({"GX_TWIN": "1", "GX_LAYOUT": "0", "GX_PLANES_W16": "0"}, "lay0", True,
                         {"twin": 1, "plane_bytes_per_cell": 3}),
    "twin_codes_two_rows": ({"GX_TWIN": "1", "GX_LAYOUT": "0", "GX_TWIN_ROWS": "2"}, "seq2", True,
                            {"twin": 1, "twin_rows": 2, "plane_bytes_per_cell": 1.5}),
    "twin_codes_four_rows": ({"GX_TWIN": "1", "GX_LAYOUT": "0", "GX_TWIN_ROWS": "4"}, "seq4", True,
                             {"twin": 1, "twin_rows": 4, "plane_bytes_per_cell": 1.5}),
}
LOCAL_LAUNCHES = ["scalar_layout0", "layout1_one_wave", "split_column_step", "skewed_strips"]
POISONED = ["scalar_layout0", "twin_codes_two_rows", "twin_codes_four_rows"]


def _steps_list(steps):
    return [(NAMES[int(c)], int(i), int(j)) for c, i, j in zip(steps["choice"], steps["i"], steps["j"])]


def _stats(r):
    return (r.score, r.matches, r.mismatches, r.gap_extensions, r.opening_gaps, r.n_steps)


def _want(o):
    return (o.score, o.matches, o.mismatches, o.gap_extensions, o.opening_gaps, len(o.choices))


def _batches(geom, local):
    """A geometry's cases of one mode as launches' batches: one per score set."""
    by = {}
    for c in cases(geom):
        if c.local == local:
            by.setdefault(c.scores, []).append(c)
    assert set(by) == ({CONFIG_SCORES} if local else {CONFIG_SCORES, dear_scores(GEOMETRIES[geom])})
    return sorted(by.items())


def _shown(info, expect):
    return all(info[k] == v for k, v in expect.items())


def _run(gx, ctx, oracle, launch, batch, scores, local, steps=1):
    """One launch of a batch -> [(stats, alignment)], checked against the oracle."""
    _, _, staged, expect = LAUNCHES[launch]
    pairs = [(c.a, c.b) for c in batch]
    got = []
    if staged:
        st = gx.StagedPairs(pairs, ctx=ctx)
        res, _ = st.run(gx.Scores(*scores), local, keep_planes=True, steps=steps, plane_sums=True)
        info = ctx.fill_info()
        assert _shown(info, expect), (launch, scores, info)
        sums, passes = st.plane_sums(), st.pass_results()
        assert len(passes) == steps
        for p, c in enumerate(batch):
            o = oracle_result(oracle, c)
            for k in range(steps):
                assert [int(x) for x in sums[k, p]] == o.extra["plane_sums"], (c.name, "plane sums, pass", k)
                assert _stats(passes[k][p]) == _want(o), (c.name, "pass", k)
            got.append((_stats(res[p]), _steps_list(st.steps(p))))
    else:
        out = gx.align_batch(pairs, gx.Scores(*scores), local, ctx=ctx, max_cell=False)
        info = ctx.fill_info()
        assert _shown(info, expect), (launch, scores, info)
        got = [(_stats(r), _steps_list(s)) for s, r in out]
    for c, (stats, steps_) in zip(batch, got):
        o = oracle_result(oracle, c)
        assert stats == _want(o), c.name
        assert steps_ == o.alignment(), c.name
    return got


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_global_cases(gx, ctx, oracle, monkeypatch, launch):
    """The geometry's global cases on one walker launch: the default scores'
    batch and the dear-mismatch batch."""
    env, geom = LAUNCHES[launch][:2]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for scores, batch in _batches(geom, False):
        _run(gx, ctx, oracle, launch, batch, scores, False)


@pytest.mark.parametrize("launch", LOCAL_LAUNCHES)
def test_local_cases(gx, ctx, oracle, monkeypatch, launch):
    """The local cases (runs to column 0 along zero cells, start cells from
    the fill's last maximum) on the strip walker's launches."""
    env, geom = LAUNCHES[launch][:2]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for scores, batch in _batches(geom, True):
        _run(gx, ctx, oracle, launch, batch, scores, True)


def test_local_cases_overlapped_twin(gx, ctx, oracle, monkeypatch):
    """The local twin through the overlapped two-group pipeline, two passes:
    the sequential walker starts from the fill's last maximum on the device
    (TbDev.start_ij_dev), not from a start cell the host worked out."""
    for k, v in {"GX_TWIN": "1", "GX_LAYOUT": "0", "GX_OVERLAP": "1"}.items():
        monkeypatch.setenv(k, v)
    (scores, batch), = _batches("seq2", True)
    assert len(batch) >= 16   # (the pipeline's lower bound, gx_api_batch.cpp)
    pairs = [(c.a, c.b) for c in batch]
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*scores), True, keep_planes=True, steps=2, plane_sums=True)
    info = ctx.fill_info()
    assert info["twin"] == 1 and info["plane_bytes_per_cell"] == 1.5 and info["groups"] == 2, info
    sums, passes = st.plane_sums(), st.pass_results()
    assert len(passes) == 2
    for p, c in enumerate(batch):
        o = oracle_result(oracle, c)
        for k in range(2):
            assert [int(x) for x in sums[k, p]] == o.extra["plane_sums"], (c.name, "plane sums, pass", k)
            assert _stats(passes[k][p]) == _want(o), (c.name, "pass", k)
        assert _stats(res[p]) == _want(o), c.name
        assert _steps_list(st.steps(p)) == o.alignment(), c.name


@pytest.mark.parametrize("launch", POISONED)
def test_poisoned_pool_changes_nothing(gx, ctx, oracle, monkeypatch, launch):
    """The same launches with every pool buffer filled with 0xA5 bytes before
    its user's work (GX_POOL_POISON): the walk's scan below the window and its
    clamped prefetch read words that no path cell owns, and a result that
    depended on them would change here.  Equal to the plain run's, pair by pair."""
    env, geom = LAUNCHES[launch][:2]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for scores, batch in _batches(geom, False):
        plain = _run(gx, ctx, oracle, launch, batch, scores, False)
        monkeypatch.setenv("GX_POOL_POISON", "1")
        assert _run(gx, ctx, oracle, launch, batch, scores, False) == plain
        monkeypatch.delenv("GX_POOL_POISON")


def test_skewed_strips_table_and_retrace(gx, ctx, oracle, monkeypatch):
    """alignment_table + retrace (the table's own walk launch) on layout 3:
    the scan past a whole window, a run to column 0 past the window, and the
    delete run over two whole strips."""
    monkeypatch.setenv("GX_LAYOUT", "3")
    monkeypatch.setenv("GX_NO_TABLE_PRINT", "1")
    picked = [c for c in cases("lay3") if c.name.split(":")[1] in
              ("c_one_window_d7", "e_run_to_col0_below_window_row64_dear", "j_delete_two_strips")]
    assert len(picked) == 3
    for c in picked:
        o = oracle_result(oracle, c)
        cont = gx.SequenceContainer([gx.Sequence("a", c.a.decode()), gx.Sequence("b", c.b.decode())])
        table, _ = gx.alignment_table(cont, gx.Scores(*c.scores), c.local, False, ctx=ctx, max_cell=False)
        assert ctx.fill_info()["layout"] == 3, (c.name, ctx.fill_info())
        sums = table.plane_sums()
        aln = gx.retrace(cont, table, c.local)
        assert sums == o.extra["plane_sums"], c.name
        assert (aln.score, aln.matches, aln.mismatches, aln.gap_extensions, aln.opening_gaps, len(aln.alignment)) == \
            _want(o), c.name
        assert [(x[0].name, x[1], x[2]) for x in aln.alignment] == o.alignment(), c.name
