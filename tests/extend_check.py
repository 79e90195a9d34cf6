"""The contract of gx_suffix_index_extend restated in plain Python, for the tests of the host
index and of the device: the reference's alignment_table(is_local = false) and retrace (algo.rs:151-441) for
s1 = the window (index i) and s2 = the pattern (index j), on the cells with |j - i| <= B alone.  A cell outside
the band reads as the reference's negative infinity in every plane; the boundary cells (i, 0) and (0, j) inside
it are the reference's.  Python's integers do not overflow, so negative infinity is the reference's own
i64::MIN + |g + h| and nothing here depends on the product's 32-bit sentinel.

  banded(window, pattern, scores, B)   the record, the runs in pattern order, the steps in retrace order
  oracle_runs(o), oracle_record(o, ..) the same two of an oracle.align result
  in_band(o, B)                        whether the oracle's retrace path stays inside the band
  check_extend(...)                    a whole extend result against banded()
"""
import numpy as np

FIELDS = ("score", "n_steps", "matches", "mismatches", "opening_gaps", "gap_extensions", "identities", "cigar_len")
MATCH, MISMATCH, INSERT, DELETE, OPEN_INSERT, OPEN_DELETE = range(6)   # oracle.CHOICE_NAMES
OP_OF = {MATCH: 0, MISMATCH: 0, INSERT: 1, OPEN_INSERT: 1, DELETE: 2, OPEN_DELETE: 2}   # M, I, D


def runs_of(ops_in_retrace_order):
    """len << 4 | op for every run, in pattern order (the reverse of the retrace)."""
    runs = []
    for op in reversed(list(ops_in_retrace_order)):
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    return [n << 4 | op for op, n in runs]


def banded(window: bytes, pattern: bytes, scores, B: int):
    """(record dict, runs, steps): steps are (choice, i, j) as AlignedSequences.alignment has them."""
    sm, smm, g, h = scores
    w, m = len(window), len(pattern)
    assert abs(w - m) <= B
    neg = -(1 << 63) + abs(g + h)
    out = (neg, neg, neg)
    rows = []   # rows[i]: (first column, [(S, I, D), ...]) of the cells of row i inside the band and the table

    def cell(i, j):
        if i < 0 or j < 0 or abs(j - i) > B:
            return out
        lo, cells = rows[i]
        return cells[j - lo]

    for i in range(w + 1):
        lo, hi = max(0, i - B), min(m, i + B)
        cells = []
        rows.append((lo, cells))
        for j in range(lo, hi + 1):
            if i == 0 and j == 0:
                c = (0, 0, 0)
            elif j == 0:
                c = (neg, neg, h + i * g)
            elif i == 0:
                c = (neg, h + j * g, neg)
            else:
                tS, tI, tD = cell(i, j - 1)        # top: consumes a pattern byte
                lS, lI, lD = cell(i - 1, j)        # left: consumes a text byte
                I = max(tI + g, tS + h + g, tD + h + g)
                D = max(lI + h + g, lS + h + g, lD + g)
                S = (sm if window[i - 1] == pattern[j - 1] else smm) + max(cell(i - 1, j - 1))
                c = (S, I, D)
            cells.append(c)
    rec = dict.fromkeys(FIELDS, 0)
    rec["score"] = max(cell(w, m))
    i, j, last, steps = w, m, MATCH, []
    while True:
        S, I, D = cell(i, j)
        top = max(S, I, D)
        if top == S:
            a = window[i] if i < w else None       # the shifted is_match(i, j) of the retrace: a missing byte
            b = pattern[j] if j < m else None      # equals a missing byte alone
            choice = MATCH if a == b else MISMATCH
            rec["matches" if a == b else "mismatches"] += 1
            if i and j and window[i - 1] == pattern[j - 1]:
                rec["identities"] += 1
            last = choice
            ni, nj = i - 1, j - 1
        elif top == I:
            choice = INSERT if last == INSERT else OPEN_INSERT
            rec["gap_extensions" if last == INSERT else "opening_gaps"] += 1
            last = INSERT
            ni, nj = i, j - 1
        else:
            choice = DELETE if last == DELETE else OPEN_DELETE
            rec["gap_extensions" if last == DELETE else "opening_gaps"] += 1
            last = DELETE
            ni, nj = i - 1, j
        steps.append((choice, i, j))
        if ni < 0 and nj < 0:
            break
        i, j = max(ni, 0), max(nj, 0)
        if i == 0 and j == 0:
            break
        assert len(steps) <= w + m, "the retrace does not end"
    runs = runs_of(OP_OF[c] for c, _, _ in steps)
    rec["n_steps"], rec["cigar_len"] = len(steps), len(runs)
    return rec, runs, steps


def oracle_steps(o):
    return list(zip(o.choices.tolist(), o.steps_i.tolist(), o.steps_j.tolist()))


def oracle_runs(o):
    return runs_of(OP_OF[c] for c in o.choices.tolist())


def oracle_record(o, window: bytes, pattern: bytes):
    ident = sum(1 for c, i, j in oracle_steps(o) if OP_OF[c] == 0 and i and j and window[i - 1] == pattern[j - 1])
    return {"score": o.score, "n_steps": len(o.choices), "matches": o.matches, "mismatches": o.mismatches,
            "opening_gaps": o.opening_gaps, "gap_extensions": o.gap_extensions, "identities": ident,
            "cigar_len": len(oracle_runs(o))}


def in_band(o, B: int) -> bool:
    return all(abs(i - j) <= B for _, i, j in oracle_steps(o))


def hit_record(r, h: int):
    return {f: int(r[f][h]) for f in FIELDS}


def hit_runs(r, h: int):
    o = r["cigar_offsets"]
    return r["cigar"][int(o[h]):int(o[h + 1])].tolist()


def hits_of(reads, hits):
    """[(hit, read, start, end)] of a mapping with hit_offsets, starts and ends."""
    ho = np.asarray(hits["hit_offsets"]).astype(np.int64)
    return [(h, p, int(hits["starts"][h]), int(hits["ends"][h]))
            for p in range(len(reads)) for h in range(ho[p], ho[p + 1])]


def check_extend(s: bytes, reads, hits, scores, B: int, r, cigars: bool = True):
    """Every hit of the result r against banded(); returns the number of hits."""
    all_hits = hits_of(reads, hits)
    co = r["cigar_offsets"].astype(np.int64)
    assert len(co) == len(all_hits) + 1 and co[0] == 0
    for f in FIELDS:
        assert len(r[f]) == len(all_hits), f
    for h, p, b, e in all_hits:
        rec, runs, _ = banded(s[b:e], reads[p], scores, B)
        assert hit_record(r, h) == rec, (h, p, b, e, B, scores, hit_record(r, h), rec)
        assert co[h + 1] - co[h] == len(runs), (h, p, b, e)
        if cigars:
            assert hit_runs(r, h) == runs, (h, p, b, e, B, scores)
    if cigars:
        assert len(r["cigar"]) == co[-1]
    else:
        assert r["cigar"] is None
    return len(all_hits)


def same_extend(a, b):
    """Two results field by field (the device against the host index)."""
    for f in FIELDS + ("cigar_offsets",):
        assert np.array_equal(a[f], b[f]), f
    assert (a["cigar"] is None) == (b["cigar"] is None)
    if a["cigar"] is not None:
        assert np.array_equal(a["cigar"], b["cigar"])
