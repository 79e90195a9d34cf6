"""CPU half of the table-driven block chase (gx_kernels.hip tb_seq_window_tab,
tb_chase_block): the byte-table rule and the chase, modelled in plain Python
from the oracle's score planes (tests/walk_chase_model.py), must walk every
planted path exactly as tests/walk_model.py reads it off the oracle's own
alignment, and must take or give back each block as its case expects.  This
pins the rule -- ((1 + run - del) << 1) | del, the escape at 127 steps, at the window's
low edge and at column 0 -- without a GPU; tests/test_gpu_walk_chase.py holds
the device to the model's block counts."""
import pytest

from test_walk_cases import cases
from walk_chase_cases import chase_cases
from walk_chase_model import ESC, chase_walk, code_bits, table_byte
from walk_model import GEOMETRIES, _interior_rows, q0_of

SEQ = ["seq2", "seq4"]
_PLANES = {}


def planes_of(oracle, c):
    """The oracle's I, D, S planes and alignment of a case, computed once and shared."""
    key = (c.a, c.b, c.scores)
    if key not in _PLANES:
        o = oracle.align(c.a, c.b, c.scores, is_local=False, want_planes=True)
        _PLANES[key] = (o.planes, o.alignment())
    return _PLANES[key]


def small_walk_cases(geom):
    """The global cases of test_walk_cases.py's list that fit a model run (planes of at most 700 x 900 cells)."""
    return [c for c in cases(geom) if not c.local and len(c.a) <= 700 and len(c.b) <= 900]


@pytest.mark.parametrize("geom", SEQ)
def test_chase_walks_the_oracle_path(oracle, geom):
    """With and without the chase the model's rows are the rows of the oracle's
    alignment: entry column, insert run and move of every interior row."""
    G = GEOMETRIES[geom]
    batch = [c for c, _ in chase_cases(geom)] + small_walk_cases(geom)
    assert len(batch) >= 30
    for c in batch:
        planes, path = planes_of(oracle, c)
        want = _interior_rows(path)
        for use in (True, False):
            rep = chase_walk(planes, G, use_chase=use)
            assert rep.rows == want, (c.name, use)
        assert chase_walk(planes, G, use_chase=False).chased == 0


@pytest.mark.parametrize("geom", SEQ)
def test_blocks_taken_and_given_back(oracle, geom):
    """Plain cases are chased through every block after the first (the walk's
    last block may end on column 0); the escape cases give a block back for
    the reason they were planted for."""
    G = GEOMETRIES[geom]
    for c, expect in chase_cases(geom):
        rep = chase_walk(planes_of(oracle, c)[0], G)
        hows = [how for _, how in rep.blocks]
        assert hows[0] == "first", c.name
        if expect.startswith("block1:"):
            assert dict(rep.blocks)[1] == expect.split(":")[1], (c.name, rep.blocks)
        elif expect == "plain":
            assert rep.chased >= 1, (c.name, rep.blocks)
            assert all(h == "chase" for h in hows[1:-1]), (c.name, rep.blocks)
            assert hows[-1] in ("chase", "column_below_1") or len(hows) == 1, (c.name, rep.blocks)
        else:
            assert expect in hows, (c.name, rep.blocks)


def test_escape_starts_at_127_steps(oracle):
    """The byte at the run's entry step: 126 steps fit, ((1 + 126) << 1) | 0 = 254; 127 and 128 escape."""
    G = GEOMETRIES["seq4"]
    got = {}
    for c, _ in chase_cases("seq4"):
        tag = c.name.split("chase_")[1]
        if tag not in ("run126", "run127", "run128"):
            continue
        planes, path = planes_of(oracle, c)
        non_i, dele = code_bits(planes)
        (i, entry, run, kind), = [r for r in _interior_rows(path) if r[2] >= 100]
        assert run == int(tag[3:]) and kind == "sub", c.name
        lot = G.lot((i - 1) % G.strip_rows)
        # the window fetched for the block below's entry (the start column) on this block's lane 63
        q0 = q0_of(G, len(c.b) - 1 + G.lot(((i - 1) % G.strip_rows) | 63))
        got[tag] = table_byte(non_i, dele, i, entry, lot, q0)
    assert got == {"run126": 254, "run127": ESC, "run128": ESC}
