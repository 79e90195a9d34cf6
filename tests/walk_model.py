"""Plain-Python model of the device walk's window arithmetic (gx_kernels.hip
tb_q0 / tb_rho / tb_lot and the conditions of tb_walk_block), for
test_walk_cases.py and test_gpu_walk_edges.py.  It works from an alignment
alone -- [(choice name, i, j)] in traceback order, as the oracle gives it --
and never touches the library: it says which branch of tb_walk_block the
converged walk takes on every interior row of that path under one walker
geometry, so that a planted case can be shown to reach the branch it was
planted for.

A geometry is a walker launch's strip height, the step at which a row of the
strip computes column 1 (lot), the window width in 16-step words, whether the
strips are walked one after another (tb_seq_kernel) or in parallel
(tb_chase_kernel + tb_strip_kernel), and how many steps a strip's rows hold
(gx_api_fill.cpp: T = m + 1 on layout 1, m + 64 elsewhere; t16 = ceil(T / 16)).

The window of a block, words q0 .. q0 + WIN - 1, ends at the word of the step
the block was fetched for: the block's own entry step when it is the first
block of the walk (both walkers) or of a strip (the strip walker: every strip
starts from its own entry in seg[]), and otherwise the step of the entry
column of the block BELOW on lane 63 of this block (the prefetch, q_n / qn:
the path only moves left, so that word is no lower than the real entry)."""
from collections import namedtuple

Geometry = namedtuple("Geometry", "name strip_rows lot win sequential pad")

GEOMETRIES = {
    "lay0": Geometry("lay0", 128, lambda rho: rho >> 1, 32, False, 64),
    "lay1": Geometry("lay1", 64, lambda rho: 0, 32, False, 1),
    "lay3": Geometry("lay3", 64, lambda rho: rho, 32, False, 64),
    "seq2": Geometry("seq2", 128, lambda rho: rho >> 1, 12, True, 64),
    "seq4": Geometry("seq4", 256, lambda rho: rho >> 2, 12, True, 64),
}

BLOCK = 64   # rows of a walked block (kTbRows); lane = row in block

INSERTS = ("Insert", "OpenInsert")
DELETES = ("Delete", "OpenDelete")

Row = namedtuple("Row", "i vb lane rho lot entry exit run kind t_in tf q0 block_entry branch "
                        "leaves_block leaves_strip lands_col0 lands_row0 last_word phase_in phase_out")
Run = namedtuple("Run", "kind i j length")   # the run's first step on the path (its highest i, j)
Report = namedtuple("Report", "rows runs start block_entry_lanes")


def t16_of(geom, m):
    return (m + geom.pad + 15) // 16


def q0_of(geom, t):
    return max((t >> 4) - (geom.win - 1), 0)


def runs_of(path):
    """Maximal insert / delete runs in path order."""
    def gap(c):
        return "insert" if c in INSERTS else "delete" if c in DELETES else None
    out, k = [], 0
    while k < len(path):
        c, i, j = path[k]
        kind = gap(c)
        if kind is None:
            k += 1
            continue
        e = k
        while e + 1 < len(path) and gap(path[e + 1][0]) == kind:
            e += 1
        out.append(Run(kind, i, j, e - k + 1))
        k = e + 1
    return out


def _interior_rows(path):
    """(i, entry column, insert run, kind) of the rows the device walks: from
    the start cell up to the move that leaves the interior."""
    rows = []
    k = 0
    while k < len(path):
        c, i, j = path[k]
        if i < 1 or j < 1:
            break
        entry, run = j, 0
        while k < len(path) and path[k][1] == i and path[k][2] >= 1 and path[k][0] in INSERTS:
            run += 1
            k += 1
        if k < len(path) and path[k][1] == i and path[k][2] >= 1:
            kind = "del" if path[k][0] in DELETES else "sub"
            k += 1
        else:
            kind = "col0"     # (i, entry .. 1) all insert: the walk leaves at (i, 0)
        rows.append((i, entry, run, kind))
        if kind == "col0" or (kind == "sub" and entry - run == 1) or i == 1:
            break
    return rows


def walk(path, geom, m):
    """The model's report of one alignment under one geometry (m = columns of
    the pair, for the row's last word)."""
    SR, bps = geom.strip_rows, geom.strip_rows // BLOCK
    t16 = t16_of(geom, m)
    raw = _interior_rows(path)
    rows, lanes = [], []
    prev_vb, prev_ce, q0 = None, None, 0
    for i, entry, run, kind in raw:
        vb, lane, rho = (i - 1) // BLOCK, (i - 1) % BLOCK, (i - 1) % SR
        lot = geom.lot(rho)
        block_entry = vb != prev_vb
        if block_entry:
            first = prev_vb is None or (not geom.sequential and vb // bps != prev_vb // bps)
            if first:
                q0 = q0_of(geom, entry - 1 + lot)
            else:                 # fetched for the block below's entry column, on this block's lane 63
                q0 = q0_of(geom, prev_ce - 1 + geom.lot(((vb & (bps - 1)) << 6) + BLOCK - 1))
            prev_vb, prev_ce = vb, entry
            lanes.append(lane)
        t_in = entry - 1 + lot
        ex = entry - run
        tf = lot - 1 if kind == "col0" else ex - 1 + lot
        if (t_in >> 4) - q0 < 0:
            branch = "entry_below_window"
        elif kind == "col0":
            branch = "run_to_col0_below_window" if (tf >> 4) < q0 and 16 * q0 > lot else "run_to_col0"
        elif (tf >> 4) == (t_in >> 4):
            branch = "in_word"
        elif (tf >> 4) >= q0:
            branch = "table"
        else:
            branch = "scan_below_window"
        goes_on = kind != "col0" and not (kind == "sub" and ex == 1) and i > 1
        rows.append(Row(i, vb, lane, rho, lot, entry, ex, run, kind, t_in, tf, q0, block_entry, branch,
                        lane == 0 and goes_on, rho == 0 and goes_on,
                        kind == "sub" and ex == 1, i == 1 and kind != "col0", (t_in >> 4) == t16 - 1,
                        t_in & 15, tf & 15))
    start = (path[0][1], path[0][2]) if path else (0, 0)
    return Report(rows, runs_of(path), start, lanes)
