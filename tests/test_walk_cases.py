"""Planted traceback paths for the two device walkers (gx_kernels.hip
tb_chase_kernel + tb_strip_kernel, tb_seq_kernel; both through tb_walk_block)
and the host's labelling of their records (gx_api_walk.cpp
label_walk_records): one list of cases per walker geometry
(tests/walk_model.py GEOMETRIES), each case a pair whose oracle alignment has
a gap of a chosen length at a chosen row and column, so that the walk meets a
named word, window, block or strip edge.

This file is the CPU half.  It aligns every case with the oracle alone and
asserts, through walk_model, that the path shows the facts the case was
planted for -- the proof that the cases reach their branches.
tests/test_gpu_walk_edges.py runs the same lists on every walker launch.

Recipes (the oracle is the only judge of where a path goes):
  * a = X + Z, b = T^s + X + T^L + Z with X, Z random over ACG: one insert run
    of L on row |X| (entry column s + |X| + L), |Z| diagonal rows below it,
    and s leading columns on row 0 that set the run's phase in its 16-step
    word.  Swapping the fillers' sides gives a delete run.
  * a = P + Y, b = T^L + Y (P over ACG): local mode stops at the zero cell
    (|P|, L) only after an insert run along row |P| to column 0 (I = 0 there,
    S < 0); global mode with a mismatch dearer than two gaps takes the same
    run and then deletes down column 0.
  * dear mismatches: (1, -30, -1, -5) on the strip walkers; the sequential
    walkers run only where the twin plane codes hold the scores
    (gx_api_plan.cpp w16_ok: smm - U >= -16), so their lists use (1, -9, -1, -2),
    still dearer than two gap openings (-6).
  * a delete run directly followed by an insert run cannot be planted from
    scores alone (both corners of a gap rectangle tie and the retrace prefers
    the insert): the case ends in a 13 x 8 tail found by search whose retrace
    switches planes there, behind a common prefix that puts the junction on a
    strip edge."""
import random
from collections import namedtuple

import pytest

from conftest import CONFIG_SCORES
from walk_model import BLOCK, GEOMETRIES, q0_of, t16_of, walk

Case = namedtuple("Case", "name a b scores local facts")   # facts: [(label, predicate(Report))]

DEAR_STRIP = (1, -30, -1, -5)
DEAR_SEQ = (1, -9, -1, -2)
SWITCH_TAIL = (b"GCAGTCTCGTGTT", b"GACGCCTT")   # ... OpenDelete, Delete, OpenInsert, Insert under both dear sets


def dear_scores(geom):
    return DEAR_SEQ if geom.sequential else DEAR_STRIP


def _rand(rng, k, alphabet=b"ACG"):
    return bytes(rng.choice(alphabet) for _ in range(k))


def _lot(G, i):
    return G.lot((i - 1) % G.strip_rows)


def _row(rep, i):
    for r in rep.rows:
        if r.i == i:
            return r
    return None


def _on(i, pred):
    """A fact about the walked row i."""
    def f(rep):
        r = _row(rep, i)
        return r is not None and pred(r)
    return f


def _single(G, seed, i_run, d, s, L):
    rng = random.Random(seed)
    X, Z = _rand(rng, i_run), _rand(rng, d)
    return X + Z, b"T" * s + X + b"T" * L + Z


def _solve(G, i_run, d, pred, Ls=None):
    """The first (s, L) of a _single pair whose run row satisfies pred(q); q
    holds the row's tf, t_in and the q0 of its block (the walk's first: the
    start row lies in the run row's block)."""
    assert (i_run - 1) // BLOCK == (i_run + d - 1) // BLOCK
    lo = _lot(G, i_run)
    for L in (Ls or range(1, 1400)):
        for s in range(16):
            x = s + i_run
            q = dict(s=s, L=L, lo=lo, tf=x - 1 + lo, t_in=x + L - 1 + lo, m=x + L + d)
            q["q0"] = q0_of(G, q["m"] - 1 + _lot(G, i_run + d))
            if pred(q):
                return s, L
    raise AssertionError("no (s, L) for the case")


def _adjacent(rep, first, second):
    for u, v in zip(rep.runs, rep.runs[1:]):
        if (u.kind, v.kind) != (first, second):
            continue
        nxt = (u.i, u.j - u.length) if first == "insert" else (u.i - u.length, u.j)
        if (v.i, v.j) == nxt and u.length >= 2 and v.length >= 2:
            return True
    return False


def _build(geom_name):
    G = GEOMETRIES[geom_name]
    SR, WIN = G.strip_rows, G.win
    DEAR = dear_scores(G)
    over = 16 * WIN + 40            # a run longer than a whole window
    out = []

    def add(name, a, b, facts, scores=CONFIG_SCORES, local=False):
        out.append(Case(f"{geom_name}:{name}", a, b, scores, local, facts))

    run_row = BLOCK + 21            # lane 20 of block 1: a mid lane, lot > 0 on the skewed layouts
    below = lambda r: r.branch == "entry_below_window"

    # a. word edges: runs of 1, 15, 16, 17 entered at phases 0 and 15 (b. one word edge crossed)
    for phase in (0, 15):
        for L in (1, 15, 16, 17):
            s, _ = _solve(G, run_row, 30, lambda q: q["t_in"] & 15 == phase, Ls=[L])
            a, b = _single(G, 100 + L, run_row, 30, s, L)
            facts = [(f"run {L} entered at phase {phase}",
                      _on(run_row, lambda r, L=L, phase=phase: r.run == L and r.phase_in == phase and r.kind == "sub"))]
            if L == 1:
                facts.append((f"last insert step at phase {phase}", _on(run_row, lambda r, phase=phase: (r.tf + 1) & 15 == phase)))
            if (phase, L) in ((0, 1), (0, 15), (15, 16)):
                facts.append(("table: exactly one word edge",
                              _on(run_row, lambda r: r.branch == "table" and (r.t_in >> 4) - (r.tf >> 4) == 1)))
            if (phase, L) in ((15, 1), (15, 15)):
                facts.append(("in_word", _on(run_row, lambda r: r.branch == "in_word")))
            for local in (False, True):
                add(f"a_run{L}_phase{phase}" + ("_local" if local else ""), a, b, facts, local=local)

    # b. table: the run ends in the window's lowest word
    s, L = _solve(G, run_row, 10, lambda q: q["q0"] >= 1 and (q["tf"] >> 4) == q["q0"] and q["tf"] & 15 == 0)
    a, b = _single(G, 120, run_row, 10, s, L)
    add("b_lowest_word", a, b, [("table, run ends at the first step of word q0",
                                 _on(run_row, lambda r: r.branch == "table" and r.q0 >= 1 and r.tf == 16 * r.q0))])

    # c. scan below the window, on the block's entry row (d = 0) and after 7 diagonal rows; d. rows above it
    edge = {"one_step": lambda q: q["tf"] == 16 * q["q0"] - 1,
            "one_word": lambda q: q["tf"] < 16 * (q["q0"] - 1),
            "one_window": lambda q: q["L"] >= 2 * 16 * WIN}
    shown = {"one_step": lambda r: r.tf == 16 * r.q0 - 1,
             "one_word": lambda r: r.tf < 16 * (r.q0 - 1),
             "one_window": lambda r: r.run >= 2 * 16 * WIN}
    for d in (0, 7):
        for k, (kind, pred) in enumerate(edge.items()):
            s, L = _solve(G, run_row, d, lambda q: q["q0"] >= 1 and 16 * q["q0"] > q["lo"] and pred(q))
            a, b = _single(G, 130 + 10 * d + k, run_row, d, s, L)
            add(f"c_{kind}_d{d}", a, b,
                [(f"scan below the window ({kind})",
                  _on(run_row, lambda r, kind=kind, d=d: r.branch == "scan_below_window" and shown[kind](r) and
                      r.block_entry == (d == 0))),
                 ("rows above it in the block enter below the window",
                  lambda rep: all(below(_row(rep, i)) for i in range(BLOCK + 1, run_row)))])

    # d. a row entered below the window with a run of its own across a word edge
    rng = random.Random(150)
    X, Z1, Z2 = _rand(rng, run_row - 5), _rand(rng, 5), _rand(rng, 7)
    add("d_run_below_window", X + Z1 + Z2, X + b"T" * 20 + Z1 + b"T" * over + Z2,
        [("long run", _on(run_row, lambda r: r.run == over)),
         ("run of 20 below the window, across a word edge",
          _on(run_row - 5, lambda r: below(r) and r.run == 20 and (r.t_in >> 4) != (r.tf >> 4)))])

    # e. runs to column 0, inside the window and past its low edge: lanes 0, 63 and mid lanes; the
    # row-30 runs end in strip 0 below a start cell in strip 1 (the chase's exit at a negative landing column)
    for r0 in (1, 30, BLOCK, BLOCK + 1):
        for kind, L in (("run_to_col0", 20), ("run_to_col0_below_window", 16 * (WIN + 6))):
            rng = random.Random(160 + r0)
            P, Y = _rand(rng, r0), _rand(rng, SR + 10 if r0 == 30 else 40)
            facts = [(f"{kind} on lane {(r0 - 1) % BLOCK}",
                      _on(r0, lambda r, kind=kind, L=L: r.branch == kind and r.run == L and r.kind == "col0"))]
            if r0 == 30:
                facts.append(("the run ends in a strip above the start strip", lambda rep: rep.start[0] > SR))
            add(f"e_{kind}_row{r0}_local", P + Y, b"T" * L + Y, facts, local=True)
            add(f"e_{kind}_row{r0}_dear", P + Y, b"T" * L + Y, facts, scores=DEAR)

    # f. a diagonal move onto column 0 from lanes 0, mid and 63, in a strip above the start strip
    for r0 in sorted({SR, 30, BLOCK - 1, BLOCK}):
        rng = random.Random(170 + r0)
        Y = _rand(rng, SR + 50)
        add(f"f_col0_from_row{r0 + 1}", b"T" * r0 + Y, Y,
            [(f"diagonal move onto (., 0) from lane {r0 % BLOCK} above the start strip",
              lambda rep, r0=r0: rep.rows[-1].i == r0 + 1 and rep.rows[-1].lands_col0 and rep.rows[-1].lane == r0 % BLOCK
              and r0 // SR < (rep.start[0] - 1) // SR)])

    # g. the path reaches row 0 at columns 1, 16 and m - 1
    for ylen, c in ((40, 1), (40, 16), (1, 20)):
        rng = random.Random(180 + c)
        Y = _rand(rng, ylen)
        add(f"g_row0_at_col{c}", Y, b"T" * c + Y,
            [(f"lands on (0, {c})" + (" = (0, m - 1)" if ylen == 1 else ""),
              lambda rep, c=c, ylen=ylen: rep.rows[-1].lands_row0 and rep.rows[-1].kind == "sub" and
              rep.rows[-1].exit - 1 == c)])

    # h. start cells on lanes 0 and 63 and on a strip's first and last row
    for n in sorted({BLOCK, BLOCK + 1, SR, SR + 1}):
        rng = random.Random(190 + n)
        X = _rand(rng, n)
        for local in (False, True):
            add(f"h_start_row{n}" + ("_local" if local else ""), X, X[:20] + b"TTT" + X[20:],
                [(f"start cell on row {n}", lambda rep, n=n: rep.start[0] == n and rep.rows[0].i == n and
                  rep.rows[0].lane == (n - 1) % BLOCK and rep.rows[0].rho == (n - 1) % SR)], local=local)

    # i. insert runs on a strip's top and bottom row and on lanes 0 and 63 (short, and past the window)
    for i_run in sorted({BLOCK, BLOCK + 1, SR, SR + 1}):
        for L in (20, over):
            rng = random.Random(200 + i_run)
            X, Z = _rand(rng, i_run), _rand(rng, 30)
            facts = [(f"run {L} on lane {(i_run - 1) % BLOCK}, row {(i_run - 1) % SR} of its strip",
                      _on(i_run, lambda r, L=L: r.run == L and r.kind == "sub"))]
            if L == over and (i_run - 1) % BLOCK == BLOCK - 1:
                facts.append(("the block is entered on lane 63 and leaves its window at once",
                              _on(i_run, lambda r: r.block_entry and r.lane == BLOCK - 1 and r.branch == "scan_below_window")))
            add(f"i_run{L}_row{i_run}", X + Z, X + b"T" * L + Z, facts)

    # j. delete runs across a block edge, across a strip edge, and over two whole strips
    for name, k, Ld in (("block_edge", 50, 30), ("strip_edge", SR - 20, 40), ("two_strips", 20, 3 * SR)):
        rng = random.Random(210 + k)
        X, Z = _rand(rng, k), _rand(rng, 30)

        def shown_j(rep, name=name, k=k, Ld=Ld):
            runs = [u for u in rep.runs if u.kind == "delete" and u.length == Ld and u.i == k + Ld and u.j == k]
            if not runs:
                return False
            top, bot = k + 1, k + Ld
            if name == "block_edge":
                return (top - 1) // BLOCK != (bot - 1) // BLOCK
            if name == "strip_edge":
                return (top - 1) // SR != (bot - 1) // SR
            whole = [s for s in range((top - 1) // SR + 1, (bot - 1) // SR) if s * SR + 1 >= top and (s + 1) * SR <= bot]
            rows = [r for r in rep.rows if (r.i - 1) // SR in whole]
            return len(whole) >= 2 and len(rows) == len(whole) * SR and \
                all(r.kind == "del" and r.run == 0 and r.entry == k for r in rows)
        add(f"j_delete_{name}", X + b"T" * Ld + Z, X + Z, [(f"delete run of {Ld}: {name}", shown_j)])

    # k. adjacent runs, the junction on a strip edge
    rng = random.Random(220)
    X, Z = _rand(rng, SR - 3, b"AC"), _rand(rng, 30, b"AC")
    add("k_insert_then_delete", X + b"G" * 5 + Z, X + b"T" * 7 + Z,
        [("insert run directly followed by a delete run", lambda rep: _adjacent(rep, "insert", "delete"))], scores=DEAR)
    X = _rand(random.Random(221), SR - 9)
    add("k_delete_then_insert", X + SWITCH_TAIL[0], X + SWITCH_TAIL[1],
        [("delete run directly followed by an insert run", lambda rep: _adjacent(rep, "delete", "insert")),
         ("the junction lies on a strip edge",
          lambda rep: any(u.kind == "insert" and u.i == SR and v.kind == "delete" for v, u in zip(rep.runs, rep.runs[1:])))],
        scores=DEAR)

    # l. the start row's entry step in the row's last word, then a run longer than the window
    # (a twin launch sizes the rows for the twin's wider pair: the last word there is its mate's)
    n = SR
    rng = random.Random(230)
    X = _rand(rng, n)
    s = next(s for s in range(16)
             if ((s + n + over - 1 + _lot(G, n)) >> 4) == t16_of(G, s + n + over) - 1)
    add("l_last_word", X, b"T" * s + X + b"T" * over,
        [("start row enters in its last word and leaves the window",
          lambda rep: rep.rows[0].i == SR and rep.rows[0].last_word and rep.rows[0].run == over and
          rep.rows[0].branch == "scan_below_window")])
    return out


_CASES = {}


def cases(geom_name):
    """The planted cases of one geometry, built once."""
    if geom_name not in _CASES:
        _CASES[geom_name] = _build(geom_name)
    return _CASES[geom_name]


_ORACLE = {}


def oracle_result(oracle, case):
    """The oracle's alignment of a case, computed once a session and shared."""
    key = (case.a, case.b, case.scores, case.local)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.align_lean(case.a, case.b, case.scores, is_local=case.local)
    return _ORACLE[key]


# every fact of the issue's list (a - l) must be present in every geometry's list
REQUIRED = ["a_run1_phase0", "a_run15_phase0", "a_run16_phase0", "a_run17_phase0", "a_run1_phase15", "a_run15_phase15",
            "a_run16_phase15", "a_run17_phase15", "b_lowest_word", "c_one_step_d0", "c_one_word_d0", "c_one_window_d0",
            "c_one_step_d7", "c_one_word_d7", "c_one_window_d7", "d_run_below_window",
            "e_run_to_col0_row1_local", "e_run_to_col0_row30_local", "e_run_to_col0_row64_local",
            "e_run_to_col0_below_window_row1_local", "e_run_to_col0_below_window_row30_local",
            "e_run_to_col0_below_window_row64_local", "e_run_to_col0_row30_dear", "e_run_to_col0_row64_dear",
            "e_run_to_col0_below_window_row30_dear", "e_run_to_col0_below_window_row65_dear",
            "f_col0_from_row31", "f_col0_from_row64", "f_col0_from_row65", "g_row0_at_col1", "g_row0_at_col16",
            "g_row0_at_col20", "h_start_row64", "h_start_row65", "i_run20_row64", "i_run20_row65", "j_delete_block_edge",
            "j_delete_strip_edge", "j_delete_two_strips", "k_insert_then_delete", "k_delete_then_insert", "l_last_word"]


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_case_list_is_complete(geom):
    names = {c.name.split(":", 1)[1] for c in cases(geom)}
    assert not [r for r in REQUIRED if r not in names]
    assert len(names) == len(cases(geom))
    G = GEOMETRIES[geom]
    for c in cases(geom):
        assert len(c.a) <= 2000 and len(c.b) <= 2000, c.name
        assert not c.local or c.scores == CONFIG_SCORES, c.name
    # the local list is long enough for the overlapped pipeline (>= 16 pairs)
    assert not G.sequential or sum(c.local for c in cases(geom)) >= 16


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_planted_cases_reach_their_branches(oracle, geom):
    """Every case's facts hold on the oracle's own path, in the case's geometry."""
    G = GEOMETRIES[geom]
    failed = []
    for c in cases(geom):
        o = oracle_result(oracle, c)
        assert o.status == 0, c.name
        rep = walk(o.alignment(), G, len(c.b))
        for label, pred in c.facts:
            if not pred(rep):
                failed.append((c.name, label))
    assert not failed, failed


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_every_branch_is_reached(oracle, geom):
    """Over a geometry's list the model names every branch of tb_walk_block,
    every way out of a block, and both word-edge phases on entry and exit."""
    G = GEOMETRIES[geom]
    branches, ways, tin, tf = set(), set(), set(), set()
    for c in cases(geom):
        rep = walk(oracle_result(oracle, c).alignment(), G, len(c.b))
        for r in rep.rows:
            branches.add(r.branch)
            tin.add(r.phase_in)
            tf.add(r.phase_out)
            ways |= {k for k in ("leaves_block", "leaves_strip", "lands_col0", "lands_row0", "last_word") if getattr(r, k)}
    assert branches == {"in_word", "table", "scan_below_window", "entry_below_window", "run_to_col0",
                        "run_to_col0_below_window"}
    assert ways == {"leaves_block", "leaves_strip", "lands_col0", "lands_row0", "last_word"}
    assert tin == set(range(16)) and tf == set(range(16))
