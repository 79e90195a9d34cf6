"""GPU parity of the sequential walker's table-driven block chase
(gx_kernels.hip tb_seq_window_tab / tb_chase_block in tb_seq_kernel) against
the fixed-point walk it replaces where it can (tb_walk_block, GX_TB_FAST=0):
on the same fills the two walkers' records -- end cell, first strip, every
strip's entry, count and record words (gx_walk_records) -- must be equal word
for word and every alignment equal to the oracle's, on the planted paths of
tests/test_walk_cases.py and on tests/walk_chase_cases.py (insert runs of 126
to 193 steps, runs ending at column 1 and column 0, delete runs over block and
strip edges, start rows on lanes 0 and 63, both halves of a twin, twins of
unequal length), on the two- and the four-row geometry.  The device must chase
exactly the blocks that the CPU model chases (tests/walk_chase_model.py) and
give back exactly the blocks it gives back.  A poisoned pool must change
nothing, and a rotated batch must give the oracle's results in every pass at
every walker priority, with the policy's priorities on its walks (0 beside a
queued fill, 3 on the call's last walk) and the fixed-point kernel unless the
chase is asked for."""
import random

import pytest

from conftest import CONFIG_SCORES
from test_gpu_walk_edges import LAUNCHES, _batches, _run
from test_walk_chase_model import planes_of
from walk_chase_cases import chase_cases
from walk_chase_model import chase_walk
from walk_model import GEOMETRIES

pytestmark = pytest.mark.gpu

SEQ_LAUNCHES = {"seq2": "twin_codes_two_rows", "seq4": "twin_codes_four_rows"}


def _both_walkers(gx, ctx, oracle, monkeypatch, launch, batch, scores):
    """One batch through the chase and through the fixed point alone -> the chase's records."""
    monkeypatch.setenv("GX_WALK_RECORDS", "1")
    monkeypatch.setenv("GX_TB_FAST", "1")
    got = _run(gx, ctx, oracle, launch, batch, scores, False)
    info, fast = ctx.walk_info(), ctx.walk_records()
    assert info["sequential"] == 1 and info["fast"] == 1 and info["pairs"] == len(batch), info
    monkeypatch.setenv("GX_TB_FAST", "0")
    assert _run(gx, ctx, oracle, launch, batch, scores, False) == got
    info0 = ctx.walk_info()
    assert info0["fast"] == 0 and info0["blocks_chased"] == 0, info0
    strip = lambda rs: [{k: v for k, v in r.items() if not k.startswith("blocks_")} for r in rs]
    assert strip(ctx.walk_records()) == strip(fast)
    assert [r["blocks_chased"] + r["blocks_fixed_point"] for r in fast] == \
        [r["blocks_fixed_point"] for r in ctx.walk_records()]
    monkeypatch.delenv("GX_TB_FAST")
    return fast


@pytest.mark.parametrize("geom", sorted(SEQ_LAUNCHES))
def test_planted_walk_cases(gx, ctx, oracle, monkeypatch, geom):
    """The geometry's global lists of test_walk_cases.py: word for word, and the chase did run."""
    launch = SEQ_LAUNCHES[geom]
    for k, v in LAUNCHES[launch][0].items():
        monkeypatch.setenv(k, v)
    for scores, batch in _batches(geom, False):
        fast = _both_walkers(gx, ctx, oracle, monkeypatch, launch, batch, scores)
        assert sum(r["blocks_chased"] for r in fast) > 0
        assert all(r["blocks_fixed_point"] >= 1 for r in fast)   # (every walk's first block)


@pytest.mark.parametrize("geom", sorted(SEQ_LAUNCHES))
def test_chase_cases_against_model(gx, ctx, oracle, monkeypatch, geom):
    """tests/walk_chase_cases.py: word for word, and block for block what the CPU model takes and gives back."""
    launch = SEQ_LAUNCHES[geom]
    for k, v in LAUNCHES[launch][0].items():
        monkeypatch.setenv(k, v)
    by = {}
    for c, _ in chase_cases(geom):
        by.setdefault(c.scores, []).append(c)
    halves, unequal = set(), 0
    for scores, batch in sorted(by.items()):
        fast = _both_walkers(gx, ctx, oracle, monkeypatch, launch, batch, scores)
        for c, r in zip(batch, fast):
            rep = chase_walk(planes_of(oracle, c)[0], GEOMETRIES[geom])
            assert (r["blocks_chased"], r["blocks_fixed_point"]) == (rep.chased, rep.fixed_point), (c.name, rep.blocks)
            assert r["end"] == rep.end, c.name
            halves.add(r["half"])
            # a pair in a twin's high half has a mate in the low half; if no other pair of the launch
            # has its shape, that twin holds two pairs of unequal length
            shape = (len(c.a), len(c.b))
            unequal += r["half"] == 1 and sum((len(x.a), len(x.b)) == shape for x in batch) == 1
    assert halves == {0, 1} and unequal >= 1   # both halves of a twin, twins of unequal length


@pytest.mark.parametrize("geom", sorted(SEQ_LAUNCHES))
def test_poisoned_pool_changes_nothing(gx, ctx, oracle, monkeypatch, geom):
    """GX_POOL_POISON: every pool buffer 0xA5 before its user's work.  The byte tables live in LDS and are
    written whole for every block; a byte read before it was written, or one that rested on a word no path
    cell owns, would change the records or the blocks taken."""
    launch = SEQ_LAUNCHES[geom]
    for k, v in LAUNCHES[launch][0].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GX_WALK_RECORDS", "1")
    monkeypatch.delenv("GX_TB_FAST", raising=False)
    batch = [c for c, _ in chase_cases(geom) if c.scores == CONFIG_SCORES]
    plain = _run(gx, ctx, oracle, launch, batch, CONFIG_SCORES, False)
    rec = ctx.walk_records()
    assert ctx.walk_info()["fast"] == 1   # (the policy: an unpipelined walk of at most 256 pairs)
    monkeypatch.setenv("GX_POOL_POISON", "1")
    assert _run(gx, ctx, oracle, launch, batch, CONFIG_SCORES, False) == plain
    assert ctx.walk_records() == rec


_ROT = {}


def _rot_pairs():
    if not _ROT:
        rng = random.Random(77)
        base = [(bytes(rng.choice(b"ACGT") for _ in range(4096 + 64 * k)), bytes(rng.choice(b"ACGT") for _ in range(4100 + 48 * k)))
                for k in range(4)]
        _ROT["pairs"] = [base[k % 4] for k in range(16)]
    return _ROT["pairs"]


@pytest.mark.parametrize("prio,fast", [("policy", None), ("0", None), ("1", None), ("2", None), ("3", None), ("policy", "1")])
def test_rotated_batch_at_every_priority(gx, ctx, oracle, monkeypatch, prio, fast):
    """16 pairs of 4,096+ rows through the rotated pipeline, three passes (six walks), at the policy's
    priorities and at each override: every pass's results and the last pass's alignments against the
    oracle.  The policy launches walks 0-4, each with a fill queued behind it, at priority 0 and the call's
    last walk at 3, all on the fixed-point kernel; GX_TB_FAST=1 puts the chase beside the fills."""
    from test_gpu_overlap_rotate import _run_check
    for k, v in {"GX_TWIN": "1", "GX_LAYOUT": "0", "GX_OVERLAP": "1"}.items():
        monkeypatch.setenv(k, v)
    for name, v in (("GX_TB_PRIO", None if prio == "policy" else prio), ("GX_TB_FAST", fast)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    _run_check(gx, ctx, oracle, _rot_pairs(), 3, scheme=2)
    info = ctx.walk_info()
    assert info["sequential"] == 1 and info["fast"] == (1 if fast == "1" else 0), info
    assert (info["blocks_chased"] > 0) == (fast == "1"), info
    assert info["launch_prios"][-6:] == ([0] * 5 + [3] if prio == "policy" else [int(prio)] * 6), info
