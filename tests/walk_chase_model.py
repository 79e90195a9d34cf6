"""Plain-Python model of the sequential walker's table-driven block chase
(gx_kernels.hip tb_seq_window_tab / tb_chase_block / tb_seq_kernel), for
test_walk_chase_model.py and test_gpu_walk_chase.py.  It works from the
oracle's score planes alone and never touches the library.

The retrace's choice at a cell is its code: insert when I > S
and the delete does not beat both, delete when D > max(I, S), else a diagonal
move.  A row entered at column g takes its insert run down to the nearest
non-insert cell and then that cell's move: it leaves at g - d, d = 1 + run - del.

For every block after a walk's first the helpers write a byte per row and
window step: (d << 1) | del, or ESC when run >= 127, when no non-insert step
at or below the step lies inside the window, or when that step is left of the
row's column 1.  The walker chases a block through those bytes and gives the
block back to the fixed-point walk (the reference walker here) on an ESC byte,
an entry outside the window, or a column < 1 at the block's end (a row never
moves right, so that covers every row)."""
from collections import namedtuple

import numpy as np

from walk_model import BLOCK, q0_of

ESC = 0xFF
WIN_STEPS = 16 * 12     # kSqSteps: the sequential walker's window, in steps

ChaseReport = namedtuple("ChaseReport", "rows blocks chased fixed_point end")
# rows: [(i, entry column, insert run, kind)] as walk_model._interior_rows gives them;
# blocks: [(vb, "chase" | "first" | reason the chase gave the block back)]


def code_bits(planes):
    """(non-insert, delete) bit planes [n + 1, m + 1] of the oracle's I, D, S planes."""
    I, D, S = planes
    dele = D > np.maximum(I, S)
    ins = (I > S) & ~dele
    return ~ins, dele


def table_byte(non_i, dele, i, j, lot, q0):
    """The helpers' byte of row i at column j (a step inside the window)."""
    lo = max(1, 16 * q0 - lot + 1)          # the lowest column the byte may rest on: the window's edge, column 1
    jf = j
    while jf >= lo and not non_i[i, jf]:
        jf -= 1
    if jf < lo or j - jf >= 127:
        return ESC
    d = int(dele[i, jf])
    return ((1 + j - jf - d) << 1) | d


def chase_block(non_i, dele, geom, vb, q0, ce):
    """The chase of block vb entered at lane 63, column ce -> ([entry column per
    lane, 63 first], exit column) or the reason the block goes back to the fixed point."""
    g, entries = ce, []
    for lane in range(BLOCK - 1, -1, -1):
        i = vb * BLOCK + lane + 1
        lot = geom.lot((i - 1) % geom.strip_rows)
        off = g - 1 + lot - 16 * q0
        if not 0 <= off < WIN_STEPS:
            return "entry_outside_window"
        e = table_byte(non_i, dele, i, g, lot, q0)
        if e == ESC:
            return "escape"
        entries.append(g)
        g -= e >> 1
    if g < 1:
        return "column_below_1"
    return entries, g


def _row(non_i, dele, i, g):
    """The reference walker on one row: (run, kind, next column)."""
    jf = g
    while jf >= 1 and not non_i[i, jf]:
        jf -= 1
    if jf < 1:
        return g, "col0", 0
    d = bool(dele[i, jf])
    return g - jf, "del" if d else "sub", jf - 1 + int(d)


def chase_walk(planes, geom, use_chase=True):
    """The sequential walk of a global pair from (n, m) under one geometry."""
    non_i, dele = code_bits(planes)
    n, m = planes.shape[1] - 1, planes.shape[2] - 1
    bps = geom.strip_rows // BLOCK
    rows, blocks = [], []
    i, g = n, m
    vb = (i - 1) // BLOCK
    q0 = q0_of(geom, g - 1 + geom.lot((i - 1) % geom.strip_rows))
    first = True
    end = None
    while end is None:
        ce = g
        took = None
        if use_chase and not first:
            took = chase_block(non_i, dele, geom, vb, q0, ce)
        if took is not None and not isinstance(took, str):
            entries, g_out = took
            for lane, ge in zip(range(BLOCK - 1, -1, -1), entries):
                run, kind, _ = _row(non_i, dele, vb * BLOCK + lane + 1, ge)
                rows.append((vb * BLOCK + lane + 1, ge, run, kind))
            blocks.append((vb, "chase"))
            g, i = g_out, vb * BLOCK
            if i == 0:
                end = (0, g)
        else:
            blocks.append((vb, "first" if first else took if use_chase else "fixed_point"))
            while i > vb * BLOCK:
                run, kind, nxt = _row(non_i, dele, i, g)
                rows.append((i, g, run, kind))
                if kind == "col0":
                    end = (i, 0)
                    break
                i -= 1
                g = nxt
                if g < 1 or i == 0:
                    end = (i, g)
                    break
        first = False
        if end is None:
            vb -= 1
            # fetched for the block below's entry column, on this block's lane 63
            q0 = q0_of(geom, ce - 1 + geom.lot(((vb & (bps - 1)) << 6) + BLOCK - 1))
    chased = sum(1 for _, how in blocks if how == "chase")
    return ChaseReport(rows, blocks, chased, len(blocks) - chased, end)
