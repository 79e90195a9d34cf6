"""Planted pairs for the sequential walker's table-driven block chase
(gx_kernels.hip tb_chase_block), beside the lists of tests/test_walk_cases.py:
global pairs of a few hundred rows whose oracle path puts a gap where the
chase's byte table changes its answer.  Each case names what it expects of the
chase: "plain" (every block after the walk's first is chased; only the
walk's last block may go back to the fixed-point walk, where the path lands
on column 0) or the reason, in walk_chase_model's words, for which at least
one block must go back: "escape" or "column_below_1"; or "block1:" and what
becomes of block 1 alone (the block above a long run is entered below the
window that was fetched for it while the run's block was walked).  The recipes are
test_walk_cases.py's: a = X + Z, b = T^s + X + T^L + Z plants an insert run of
L on row |X|; the fillers on the other side plant a delete run."""
import random

from conftest import CONFIG_SCORES
from test_walk_cases import DEAR_SEQ, Case, _rand, _single
from walk_model import BLOCK, GEOMETRIES

_CASES = {}


def chase_cases(geom_name):
    """[(Case, what it expects of the chase)] of one sequential geometry, built once."""
    if geom_name in _CASES:
        return _CASES[geom_name]
    G = GEOMETRIES[geom_name]
    assert G.sequential
    out = []

    def add(name, a, b, expect, scores=CONFIG_SCORES):
        out.append((Case(f"{geom_name}:chase_{name}", a, b, scores, False, []), expect))

    # insert runs on lane 1 of block 1.  A window holds 192 steps and a diagonal row uses up to 1.5 of
    # them, so a chased block has no room for a run of 126 beside 63 diagonal rows: 46 rows of the block
    # are a delete run (no column moves), and s sets the start column's step to its word's last phase, so
    # that the block is entered 10 steps below the window's top.  Then 126 is a table byte and the whole
    # block is chased, 127 is the first escape, and the runs of 191-193 steps also leave the window's
    # low edge.
    for L in (126, 127, 128, 191, 192, 193):
        rng = random.Random(300 + L)
        X, Z1, Z2 = _rand(rng, BLOCK + 2, b"AC"), _rand(rng, 3, b"AC"), _rand(rng, 23, b"AC")
        m0 = len(X) + L + len(Z1) + len(Z2)
        lot63 = G.lot(2 * BLOCK - 1)
        s = next(s for s in range(1, 17) if (s + m0 - 1 + lot63) & 15 == 15)
        add(f"run{L}", X + Z1 + b"G" * 46 + Z2, b"T" * s + X + b"T" * L + Z1 + Z2, "block1:chase" if L < 127 else "block1:escape")
    # the same run deep in block 1 (lane 20, 43 rows above the block's entry): short of 127 steps, yet
    # past the low edge of the window fetched at the block's entry
    a, b = _single(G, 320, BLOCK + 21, 64, 3, 126)
    add("run126_past_window_edge", a, b, "escape")
    # a run that ends exactly at column 1 (row 1's diagonal move then lands on (0, 0)) ...
    a, b = _single(G, 330, 1, 100, 0, 20)
    add("run_to_col1", a, b, "column_below_1")
    # ... and one that reaches column 0: the mismatch dearer than two gaps, then deletes down column 0
    rng = random.Random(331)
    P, Y = _rand(rng, BLOCK + 21), _rand(rng, 70)
    add("run_to_col0", P + Y, b"T" * 20 + Y, "escape", scores=DEAR_SEQ)
    # delete runs across a 64-row block edge, row 128 | 129 and row 256 | 257 (strip tops of the two geometries)
    for name, k, Ld, z in (("block_edge", 50, 30, 120), ("row128", 110, 40, 150), ("row256", 240, 40, 100)):
        rng = random.Random(340 + k)
        X, Z = _rand(rng, k), _rand(rng, z)
        add(f"delete_{name}", X + b"T" * Ld + Z, X + Z, "plain")
    # start rows on lane 0 and on lane 63: the next block is entered from there
    for n in (2 * BLOCK + 1, 3 * BLOCK):
        rng = random.Random(350 + n)
        X = _rand(rng, n)
        add(f"start_row{n}", X, X[:20] + b"TTT" + X[20:], "plain")
    # a long diagonal with scattered gaps over several strips, twice: the same shape fills both halves of a twin
    for k in (0, 1):
        rng = random.Random(360 + k)
        X = _rand(rng, 700, b"ACGT")
        y = bytearray(X)
        for pos in sorted(rng.sample(range(20, 680), 12), reverse=True):
            if rng.random() < 0.5:
                del y[pos:pos + rng.randint(1, 6)]
            else:
                y[pos:pos] = _rand(rng, rng.randint(1, 6), b"ACGT")
        add(f"gapped700_{k}", X, bytes(y[:700]) if len(y) >= 700 else bytes(y), "plain")
    _CASES[geom_name] = out
    return out
