"""GPU parity of the rotating overlapped pipeline (gx_api_batch.cpp
pipeline_rotate, overlap_rotate_plan): a global long-pair batch split in
halves runs its fills i = 2 pass + group through three plane buffers in
rotation, each group walked on its own behind its fill; fill i reuses the
buffers of fill i - 3 once the host has collected that fill and its stream has
waited on the device for walk i - 3.  Every pass's plane checksums and results
(gx_staged_pass_results) and the last pass's alignments must equal the
oracle's, over enough passes for the three jobs, the four fill slots and the
six walk slots to wrap out of phase, with unequal groups, with launches that
share the device, and with two alternating pair sets (a walk that read a
refilled buffer then gives a wrong alignment, not an equal one).  Local
batches and GX_OVERLAP_ROTATE=0 keep the two-buffer scheme.  A batch the
overlapped schemes refuse falls back to the plain pipeline of its kind with
every pass's checksums in place, and each pipeline leaves the context's slots,
held buffers and streams fit for the next one."""
import random

import pytest

from conftest import CONFIG_SCORES
from test_gpu_twin import _steps_list

pytestmark = pytest.mark.gpu

SHAPES20 = [(1300 + 97 * k, 1100 + 61 * ((k * 7) % 20)) for k in range(20)]   # 1,300-3,143 rows, 1,100-2,259 columns
_REF = {}   # (a, b, local) -> oracle result, computed once and shared by the tests


def _pairs(seed, shapes):
    rng = random.Random(seed)
    return [(bytes(rng.choice(b"ACGT") for _ in range(n)), bytes(rng.choice(b"ACGT") for _ in range(m)))
            for n, m in shapes]


PAIRS20 = _pairs(2025, SHAPES20)
# a second set of the same shapes and other sequences (the alternating sets' other half)
PAIRS16_ALT = _pairs(4051, SHAPES20[:16])


def _ref(oracle, a, b, local=False):
    key = (a, b, local)
    if key not in _REF:
        _REF[key] = oracle.align_lean(a, b, CONFIG_SCORES, is_local=local)
    return _REF[key]


@pytest.fixture(autouse=True)
def _overlap_env(monkeypatch):
    monkeypatch.setenv("GX_TWIN", "1")      # small batches: force the twin fill
    monkeypatch.setenv("GX_LAYOUT", "0")
    monkeypatch.setenv("GX_OVERLAP", "1")   # the overlapped pipeline from 16 pairs (by default from n >= 16,384)
    monkeypatch.delenv("GX_OVERLAP_ROTATE", raising=False)
    monkeypatch.delenv("GX_OVERLAP_A", raising=False)


def _want(o):
    return (o.score, o.matches, o.mismatches, o.gap_extensions, o.opening_gaps, len(o.choices))


def _got(r):
    return (r.score, r.matches, r.mismatches, r.gap_extensions, r.opening_gaps, r.n_steps)


def _run_check(gx, ctx, oracle, pairs, K, scheme, local=False, twin=1):
    """K passes of `pairs`: every pass's checksums and results, the last pass's alignments.
    scheme 0: the plain pipeline, one launch a pass; twin: the twin fill ran (fill_info)."""
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*CONFIG_SCORES), local, keep_planes=True, steps=K, plane_sums=True)
    info = ctx.fill_info()
    # (one pass alone runs unpipelined: one launch, no scheme)
    assert info["groups"] == (2 if K >= 2 and scheme else 1) and info["twin"] == twin, info
    assert ctx.overlap_scheme() == (scheme if K >= 2 else 0)
    sums = st.plane_sums()
    passes = st.pass_results()
    assert len(passes) == K
    for p, (a, b) in enumerate(pairs):
        o = _ref(oracle, a, b, local)
        for k in range(K):
            assert [int(x) for x in sums[k, p]] == o.extra["plane_sums"], (p, len(a), len(b), k)
            assert _got(passes[k][p]) == _want(o), (p, k)
        assert _got(res[p]) == _want(o), p
        assert _steps_list(st.steps(p)) == o.alignment(), (p, len(a), len(b))


@pytest.mark.parametrize("K", [1, 2, 3, 4, 7])
def test_rotation_wrap(gx, ctx, oracle, K):
    """20 mixed shapes, K passes.  K = 7 is 14 fills: the three jobs, the four
    fill slots and the six walk slots all wrap more than once, out of phase."""
    _run_check(gx, ctx, oracle, PAIRS20, K, scheme=2)


@pytest.mark.parametrize("Q", [18, 19])
def test_unequal_groups(gx, ctx, oracle, Q):
    """18 pairs split 8 + 10 and 19 pairs 10 + 9: every job holds the two
    group sizes in turn (its buffer has the larger one's size)."""
    _run_check(gx, ctx, oracle, PAIRS20[:Q], 4, scheme=2)


def test_interleaved_launches(gx, ctx, oracle, monkeypatch):
    """Three workgroups a launch (4-wave bands): neighbouring fills share the
    device for their whole length, and the walks run beside them."""
    monkeypatch.setenv("GX_BAND_WAVES", "4")
    monkeypatch.setenv("GX_FILL_GRID", "3")
    _run_check(gx, ctx, oracle, PAIRS20, 4, scheme=2)


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_stale_buffer_alternating_sets(gx, ctx, oracle, monkeypatch, poison):
    """Two sets of 16 pairs, same shapes and different sequences, alternate
    pass by pass (GX_STAGED_ALTERNATE, the call that reaches the pipelines'
    `alt` sets: pass k runs set k % 2, and such a run is one chunk), five
    passes: every buffer, descriptor block and pinned block a fill or walk
    takes last held the other set's data, so a walk that read a buffer already
    refilled, or records of another pass, gives the other set's alignment.
    With GX_POOL_POISON every pool buffer is filled with garbage on its new
    user's stream first."""
    if poison:
        monkeypatch.setenv("GX_POOL_POISON", "1")
    H, K = 16, 5
    pairs = PAIRS20[:H] + PAIRS16_ALT
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, fill_ms = st.run(gx.Scores(*CONFIG_SCORES), False, keep_planes=True, steps=K, plane_sums=True, alternate=True)
    assert ctx.fill_info()["groups"] == 2 and ctx.overlap_scheme() == 2 and fill_ms > 0
    sums = st.plane_sums()
    passes = st.pass_results()
    assert sums.shape == (K, 2 * H, 3) and len(passes) == K
    for k in range(K):
        for q in range(H):
            p = (k % 2) * H + q
            o = _ref(oracle, *pairs[p])
            assert [int(x) for x in sums[k, p]] == o.extra["plane_sums"], (p, "pass", k)
            assert _got(passes[k][p]) == _want(o), (p, "pass", k)
            other = passes[k][(1 - k % 2) * H + q]
            assert other.score == 0 and other.n_steps == 0, (p, "pass", k, "the other set's row is empty")
    for p, (a, b) in enumerate(pairs):   # each set's last pass
        o = _ref(oracle, a, b)
        assert _got(res[p]) == _want(o), p
        assert _steps_list(st.steps(p)) == o.alignment(), p
    # the two sets differ where it matters: no pair's alignment equals its counterpart's
    assert all(_ref(oracle, *pairs[q]).alignment() != _ref(oracle, *pairs[H + q]).alignment() for q in range(H))


def test_chunked_batch(gx, ctx, oracle, monkeypatch):
    """32 pairs in two chunks of 16 (GX_CHUNK_BYTES at 0.6 of the batch's
    planned bytes, gx_api_plan.cpp pair_device_bytes at 3 B a cell): each chunk
    runs its own rotation through the buffers the other left in the pool."""
    pairs = PAIRS20[:16] + PAIRS16_ALT
    total = sum((len(a) + 128) * (len(b) + 64) * 3.25 + 64 * (len(b) + 64) * (len(a) // 64 + 2) / 8 + 65536
                for a, b in pairs)
    monkeypatch.setenv("GX_CHUNK_BYTES", str(0.6 * total))
    st = gx.StagedPairs(pairs, ctx=ctx)
    res, _ = st.run(gx.Scores(*CONFIG_SCORES), False, keep_planes=True, steps=3, plane_sums=True)
    info = ctx.fill_info()
    assert info["chunks"] == 2 and info["groups"] == 2 and ctx.overlap_scheme() == 2, info
    sums = st.plane_sums()
    passes = st.pass_results()
    for p, (a, b) in enumerate(pairs):
        o = _ref(oracle, a, b)
        for k in range(3):
            assert [int(x) for x in sums[k, p]] == o.extra["plane_sums"], (p, k)
            assert _got(passes[k][p]) == _want(o), (p, k)
        assert _got(res[p]) == _want(o), p
        assert _steps_list(st.steps(p)) == o.alignment(), p


def test_switch_keeps_two_buffer_scheme(gx, ctx, oracle, monkeypatch):
    """GX_OVERLAP_ROTATE=0: the same results from two A buffers and one B buffer."""
    monkeypatch.setenv("GX_OVERLAP_ROTATE", "0")
    _run_check(gx, ctx, oracle, PAIRS20, 3, scheme=1)


def test_local_batch_keeps_two_buffer_scheme(gx, ctx, oracle):
    """A local batch splits a fifth against four fifths: it stays on the
    two-buffer scheme, with every result against the oracle's local restatement."""
    from test_gpu_twin_local import _planted
    rng = random.Random(654)
    pairs = [_planted(rng, 1500 + 37 * k, 1200 + 53 * k, 400 + 20 * k) for k in range(16)]
    _run_check(gx, ctx, oracle, pairs, 3, scheme=1, local=True)


def _poison(monkeypatch, poison):
    if poison:
        monkeypatch.setenv("GX_POOL_POISON", "1")
    else:
        monkeypatch.delenv("GX_POOL_POISON", raising=False)


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
def test_fallback_keeps_every_pass_checksums(gx, ctx, oracle, monkeypatch, poison, local):
    """GX_OVERLAP=1 asks for the overlapped pipeline and GX_TWIN=0 keeps the
    fills off the twin fill, so the admission check refuses: a global batch
    runs the three-slot pipeline, a local one the two-slot pipeline, one
    launch a pass and no scheme.  The checksums of all four passes are in
    place: the fallback writes them from where the call's first would go."""
    monkeypatch.setenv("GX_TWIN", "0")
    _poison(monkeypatch, poison)
    _run_check(gx, ctx, oracle, PAIRS20, 4, scheme=0, local=local, twin=0)


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_pipelines_back_to_back(gx, ctx, oracle, monkeypatch, poison):
    """Rotation, the three-slot pipeline, scheme 1, a one-pass batch and the
    rotation again on one context: each leaves the slots, the held buffers and
    the streams fit for the next one."""
    _poison(monkeypatch, poison)
    _run_check(gx, ctx, oracle, PAIRS20, 4, scheme=2)
    monkeypatch.setenv("GX_OVERLAP", "0")
    _run_check(gx, ctx, oracle, PAIRS20, 5, scheme=0)
    monkeypatch.setenv("GX_OVERLAP", "1")
    monkeypatch.setenv("GX_OVERLAP_ROTATE", "0")
    _run_check(gx, ctx, oracle, PAIRS20, 3, scheme=1)
    batch = gx.align_batch(PAIRS20, gx.Scores(*CONFIG_SCORES), False, ctx=ctx, max_cell=False)
    for p, ((a, b), (steps, r)) in enumerate(zip(PAIRS20, batch)):
        o = _ref(oracle, a, b)
        assert _got(r) == _want(o), p
        assert _steps_list(steps) == o.alignment(), p
    monkeypatch.delenv("GX_OVERLAP_ROTATE")
    _run_check(gx, ctx, oracle, PAIRS20, 3, scheme=2)
