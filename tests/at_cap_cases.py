"""Batches that take the capped-grid kernels of search mode past their grid cap, and their expected results
(DESIGN.md 19.4, 20.4, 21.4, 23.4).  No test, and no device: tests/test_search_at_cap_host.py holds every
batch here against the host index, tests/test_gpu_search_at_cap.py against the device.

gx_approx.hip, gx_edit.hip, gx_match.hip and gx_chain.hip launch their per-item kernels on at most CAP lanes
and let them stride over the rest, so a lane takes a second item only in a batch of more than CAP items.  Such
a batch is far beyond a brute force.  It is therefore built from a *pool* of at most a few hundred distinct
patterns, queries or anchor lists, repeated in a seeded random order (no period at all, so none that divides
256, 2,048, 8,192 or 524,288).  The checkers of the small suites (approx_check, edit_check, match_check,
chain_check.solve: they share nothing with the library) answer every pool member once, and the expected result
of the whole batch is composed from those answers by indexing: per-item fields directly, flat arrays by
concatenation, offsets by cumsum, the chains' member_off rebased on the members before them (root, end, pred and
members are anchor numbers within the query and stay).  The cost is the pool's, not the batch's.

Two things the checkers do not give are modelled here, each in a few lines of its own:

  candidates     of a pattern: the occurrences of each of its k + 1 pieces in the text, counted by comparison
  first max_hits the approximate search reports of a pattern with more occurrences than max_hits the first
                 max_hits in candidate order (piece by piece, each piece's occurrences in suffix-array order,
                 an occurrence reported by its first intact piece): candidate_order, which is held against the
                 brute force's full list on every pool member
"""
import functools

import numpy as np

import approx_check
import chain_check
import edit_check
import match_check

CAP = 2048 * 256     # kStrideGrid workgroups of kSufBlock lanes: what one trip of a grid-stride loop covers
REACH = CAP + 256    # a case must pass the cap by more than one workgroup
WAVES = CAP // 64    # the waves of chain_score_kernel at the cap: a wave's second segment is number s + WAVES
ALL_HITS = 0xFFFFFFFF
PERIODS = (256, 2048, 8192, 524288)
K = 1                # the searches' k: pieces of half a pattern


def rand_bytes(seed: int, alphabet: bytes, n: int) -> bytes:
    return np.frombuffer(alphabet, np.uint8)[np.random.default_rng(seed).integers(0, len(alphabet), n)].tobytes()


def tile(flat: np.ndarray, off, ids: np.ndarray):
    """The pool's segments flat[off[i]:off[i + 1]] for i in ids, one behind the other, and their offsets."""
    off = np.asarray(off, np.int64)
    cnt = (off[1:] - off[:-1])[ids]
    out = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(cnt, out=out[1:])
    src = np.repeat(off[:-1][ids] - out[:-1], cnt) + np.arange(out[-1], dtype=np.int64)
    return flat[src], out


def flat_of(parts, dtype):
    """(flat, offsets) of a list of arrays."""
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    flat = np.concatenate([np.asarray(p, dtype) for p in parts]) if parts else np.zeros(0, dtype)
    return flat.astype(dtype), off


def aperiodic(ids: np.ndarray) -> bool:
    """No shift by a grid size maps the order onto itself (a period that divides one would)."""
    return all(P >= len(ids) or not np.array_equal(ids[P:], ids[:-P]) for P in PERIODS)


def same_fields(got: dict, want: dict, what=""):
    """Field by field and dtype by dtype; None only beside None."""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for f in want:
        if isinstance(want[f], np.ndarray):
            assert got[f].dtype == want[f].dtype, (what, f, got[f].dtype, want[f].dtype)
            if not np.array_equal(got[f], want[f]):
                bad = np.nonzero(got[f] != want[f])[0] if got[f].shape == want[f].shape else None
                raise AssertionError((what, f, got[f].shape, want[f].shape, None if bad is None else
                                      (len(bad), bad[:5], got[f][bad[:5]], want[f][bad[:5]])))
        else:
            assert got[f] == want[f], (what, f, got[f], want[f])


# ---------------------------------------------------------------------------
# patterns: the approximate and the edit search at k = 1

# 1,500 random bases, a run of 150 A, 1,500 random bases: a pattern of 8 to 11 bytes has pieces of 4 to 6 bytes
# with tens of occurrences, A^8 has two pieces of 147 consecutive candidates each
TEXT = rand_bytes(3301, b"ACGT", 1500) + b"A" * 150 + rand_bytes(3302, b"ACGT", 1500)
LOW = b"A" * 8


def pieces(m: int, k: int):
    return [(j * m // (k + 1), (j + 1) * m // (k + 1)) for j in range(k + 1)]


def occurrences(s: bytes, piece: bytes) -> np.ndarray:
    a = np.frombuffer(s, np.uint8)
    ok = np.ones(max(len(a) - len(piece) + 1, 0), bool)
    for j, b in enumerate(piece):
        ok &= a[j:j + len(ok)] == b
    return np.nonzero(ok)[0]


def piece_candidates(s: bytes, P: bytes, k: int) -> int:
    return sum(len(occurrences(s, P[a:b])) for a, b in pieces(len(P), k))


@functools.lru_cache(maxsize=4)
def suffix_rank(s: bytes) -> np.ndarray:
    """rank[i] of the suffix s[i:] among all of them ('$' below every byte: a prefix sorts first)."""
    sa = sorted(range(len(s)), key=lambda i: s[i:])
    rank = np.zeros(len(s), np.int64)
    rank[sa] = np.arange(len(s))
    return rank


def candidate_order(s: bytes, P: bytes, k: int):
    """[(position, distance)] of P's occurrences in the order the search meets them: piece by piece, a piece's
    occurrences in suffix-array order, a window taken by the first piece that is intact in it."""
    rank, n, m, out = suffix_rank(s), len(s), len(P), []
    pc = pieces(m, k)
    for j, (ps, pe) in enumerate(pc):
        at = occurrences(s, P[ps:pe])
        for a in at[np.argsort(rank[at])].tolist():
            c = a - ps
            if c < 0 or c + m > n:
                continue
            d = sum(x != y for x, y in zip(s[c:c + m], P))
            if d <= k and all(s[c + a2:c + b2] != P[a2:b2] for a2, b2 in pc[:j]):
                out.append((c, d))
    return out


def mutated(rng, P: bytes, kind: int) -> bytes:
    """P as cut (0), with one substitution (1), insertion (2) or deletion (3), or two substitutions (4)."""
    p = bytearray(P)
    for _ in range(2 if kind == 4 else 1 if kind else 0):
        c = int(rng.integers(0, len(p)))
        x = b"ACGT"[(b"ACGT".index(p[c]) + int(rng.integers(1, 4))) % 4]
        if kind in (1, 4):
            p[c] = x
        elif kind == 2:
            p.insert(c, x)
        else:
            del p[c]
    return bytes(p)


class PatternBatch:
    """A pool of patterns and the order they are repeated in.

    The pool: `short` patterns cut from TEXT with none, one or two changes (at k = 1 of 8 to 11 bytes: pieces
    of 4 to 6 bytes, tens of candidates each), `rare` patterns (at k = 1 of 16 to 20 bytes, one or two
    candidates: a piece of 8 bytes is almost unique) and `low`, a run of A.  The order: random short and rare
    patterns until the candidates before them (or what lead_by counts, the smallest of the case's reach numbers)
    pass CAP + 512, then rare, rare, low, rare, rare (whole waves of the second trip share `low`, the lanes on
    both sides of it do not share a pattern), then `tail` more random ones, then rare patterns until
    `units % 256` is not in {0, 255}, where units is what the case's last strided kernel counts (candidates, or
    ends before dedupe)."""

    def __init__(self, seed: int, short_kinds, n_short: int, n_rare: int, tail: int, units=None, lead_by=None, k: int = K,
                 short_len=(8, 12), rare_len=(16, 21), low: bytes = LOW):
        rng = np.random.default_rng(seed)
        s = TEXT
        pool = []
        for p in range(n_short):
            m = int(rng.integers(*short_len))
            i = int(rng.integers(0, len(s) - m))
            pool.append(mutated(rng, s[i:i + m], short_kinds[p % len(short_kinds)]))
        rare, tries = [], 0
        while len(rare) < n_rare:
            tries += 1
            assert tries < 100 * n_rare
            m = int(rng.integers(*rare_len))
            i = int(rng.integers(0, 1500 - m)) + (1650 if len(rare) % 2 else 0)
            # (unchanged, every one of the k + 1 pieces is a candidate: at k = 2 only changed ones have two or fewer)
            P = mutated(rng, s[i:i + m], ((0, 1) if k == 1 else (1, 4))[len(rare) % 2])
            if 1 <= piece_candidates(s, P, k) <= 2 and P not in rare:
                rare.append(P)
        self.s, self.k, self.pool = s, k, pool + rare + [low]
        self.rare = np.arange(n_short, n_short + n_rare)
        self.low = len(self.pool) - 1
        self.cand = np.array([piece_candidates(s, P, k) for P in self.pool], np.int64)
        self.units = self.cand if units is None else np.asarray(units(self), np.int64)
        per = self.cand if lead_by is None else np.asarray(lead_by(self), np.int64)
        ids = []
        total = 0
        while total < CAP + 512:
            ids.append(int(rng.integers(0, n_short + n_rare)))
            total += int(per[ids[-1]])
        r = rng.choice(self.rare, 4, replace=False).tolist()
        self.low_at = len(ids) + 2
        ids += r[:2] + [self.low] + r[2:]
        ids += rng.integers(0, n_short + n_rare, tail).tolist()
        while int(self.units[ids].sum()) % 256 in (0, 255):
            ids.append(int(rng.choice(self.rare)))
        self.ids = np.array(ids, np.int64)

    def patterns(self):
        return [self.pool[i] for i in self.ids.tolist()]


def compose_hits(fields: dict, flats: dict, counts: np.ndarray, ids: np.ndarray, max_hits: int) -> dict:
    """fields: per-pattern arrays of the pool; flats: {name: (list of the pool's full per-pattern lists, dtype)};
    the first min(count, max_hits) of each list are reported."""
    out = {f: v[ids] for f, v in fields.items()}
    if max_hits > 0:
        q = np.minimum(counts, max_hits)
        for f, (lists, dtype) in flats.items():
            flat, off = flat_of([np.asarray(x)[:n] for x, n in zip(lists, q.tolist())], dtype)
            out[f], hoff = tile(flat, off, ids)
        out["hit_offsets"] = hoff.astype(np.uint64)
    return out


@functools.lru_cache(maxsize=1)
def approx_batch():
    return PatternBatch(1901, (0, 1, 4), n_short=240, n_rare=40, tail=300)


@functools.lru_cache(maxsize=4)
def approx_expected(max_hits: int) -> dict:
    """What search_approx(approx_batch().patterns(), 1, max_hits) must return."""
    b = approx_batch()
    rows, pos, dst = [], [], []
    for P in b.pool:
        count, best, bpos, occ = approx_check.brute(b.s, P, K)
        order = candidate_order(b.s, P, K)
        assert sorted(order) == occ, P   # (the model of the candidate order finds what the brute force finds)
        rep = sorted(order[:max_hits]) if max_hits > 0 else []
        rows.append((count, best, bpos))
        pos.append([c for c, _ in rep])
        dst.append([d for _, d in rep])
    rows = np.array(rows, np.uint32)
    fields = {"count": rows[:, 0], "best_dist": rows[:, 1], "best_pos": rows[:, 2], "candidates": b.cand.astype(np.uint32)}
    return compose_hits(fields, {"positions": (pos, np.uint32), "distances": (dst, np.uint8)}, rows[:, 0].astype(np.int64),
                        b.ids, max_hits)


def band_ends(s: bytes, P: bytes, k: int) -> int:
    """The ends P's candidates report before equal ends are merged (the band model of edit_check.py)."""
    return sum(len(v) for v in edit_check.band_reports(s, P, k).values())


@functools.lru_cache(maxsize=1)
def edit_batch():
    """One batch for the three reach conditions of the edit search.  Its short patterns are mostly cut from the
    text unchanged: such a pattern is found by both pieces, reports three ends from each and keeps three."""
    return PatternBatch(2001, (0, 0, 0, 1, 2, 3), n_short=240, n_rare=40, tail=300,
                        units=lambda b: [band_ends(b.s, P, K) for P in b.pool],
                        lead_by=lambda b: [edit_check.brute(b.s, P, K)[0] for P in b.pool])


@functools.lru_cache(maxsize=1)
def edit_k2_batch():
    """A smaller batch at k = 2 that passes CAP in candidates only: the verify kernel's second instantiation.
    Patterns of 12 to 15 bytes have three pieces of 4 or 5, A^12 three pieces of 147 consecutive candidates."""
    return PatternBatch(2002, (0, 1, 2, 3, 4), n_short=200, n_rare=30, tail=300, k=2, short_len=(12, 16),
                        rare_len=(26, 33), low=b"A" * 12)


@functools.lru_cache(maxsize=8)
def edit_expected(max_hits: int, starts: bool = True, k: int = K) -> dict:
    """What search_edit(b.patterns(), k, max_hits, starts) must return of b = edit_batch() (k = 1) or
    edit_k2_batch() (k = 2)."""
    b = edit_batch() if k == K else edit_k2_batch()
    assert b.k == k
    rows, ends, dst, sta = [], [], [], []
    for P in b.pool:
        count, best, bend, e, d, st = edit_check.brute(b.s, P, k)
        rows.append((count, best, bend))
        ends.append(e)
        dst.append(d)
        sta.append(st)
    rows = np.array(rows, np.uint32)
    fields = {"count": rows[:, 0], "best_dist": rows[:, 1], "best_end": rows[:, 2], "candidates": b.cand.astype(np.uint32)}
    out = compose_hits(fields, {"ends": (ends, np.uint32), "distances": (dst, np.uint8), "starts": (sta, np.uint32)},
                       rows[:, 0].astype(np.int64), b.ids, max_hits)
    if max_hits > 0 and not starts:
        out["starts"] = None
    return out


def edit_pre_dedupe_ends() -> int:
    b = edit_batch()
    return int(b.units[b.ids].sum())


# ---------------------------------------------------------------------------
# MEMs: min_len 3 over four letters, so that a query position has tens of candidates, three in four left-maximal

MEM_TEXT = rand_bytes(2101, b"ACGT", 1500)
MEM_MIN_LEN = 3


class MemBatch:
    def __init__(self, seed: int = 2102, npool: int = 96, extra: int = 40):
        rng = np.random.default_rng(seed)
        self.s, self.pool = MEM_TEXT, []
        for c in range(npool):
            m = int(rng.integers(40, 100))
            if c % 3 == 0:   # cut from the text and changed here and there: long MEMs among the short ones
                i = int(rng.integers(0, len(self.s) - m))
                q = bytearray(self.s[i:i + m])
                for j in range(int(rng.integers(3, 17)), m, 17):
                    q[j] = b"ACGT"[(b"ACGT".index(q[j]) + 1) % 4]
                self.pool.append(bytes(q))
            else:
                self.pool.append(rand_bytes(seed + 1 + c, b"ACGT", m))
        self.pool += [b"", b"AC"]   # nothing to seed
        self.answers = [match_check.brute_mems(self.s, q, MEM_MIN_LEN) for q in self.pool]
        kept = np.array([len(a[0]) for a in self.answers], np.int64)
        ids, total = [], 0
        while total <= REACH + 1000:
            ids.append(int(rng.integers(0, len(self.pool))))
            total += int(kept[ids[-1]])
        ids += rng.integers(0, len(self.pool), extra).tolist()
        self.ids = np.array(ids, np.int64)

    def queries(self):
        return [self.pool[i] for i in self.ids.tolist()]


@functools.lru_cache(maxsize=1)
def mem_batch():
    return MemBatch()


@functools.lru_cache(maxsize=1)
def mem_expected() -> dict:
    """What mems(mem_batch().queries(), MEM_MIN_LEN) must return."""
    b = mem_batch()
    trip, off = flat_of([np.asarray(a[0], np.int64).reshape(len(a[0]), 3) for a in b.answers], np.int64)
    flat, moff = tile(trip.reshape(-1, 3), off, b.ids)
    cand = np.array([a[1] for a in b.answers], np.uint64)
    return {"qpos": flat[:, 0].astype(np.uint32), "tpos": flat[:, 1].astype(np.uint32), "length": flat[:, 2].astype(np.uint32),
            "mem_offsets": moff.astype(np.uint64), "candidates": cand[b.ids]}


# ---------------------------------------------------------------------------
# chains

SEG_SIZES = (1, 2, 63, 64, 65, 129, 257)
SEG_WEIGHTS = (0.3, 0.3, 0.1, 0.1, 0.1, 0.06, 0.04)
CHAIN_GAP = 30
CHAIN_PARAMS = {H: {"max_pred": H, "max_gap": CHAIN_GAP, "max_drift": 25, "w_match": 3, "w_drift": 2} for H in (64, 128, 256)}


def rand_segment(rng, n: int, q0: int):
    """n random anchors with many ties, ascending and distinct, no two neighbours more than CHAIN_GAP apart in
    qpos (so that they stay one segment), several tpos at some qpos."""
    while True:
        pts = set()
        while len(pts) < n:
            q = int(rng.integers(0, 2 * n))
            for _ in range(int(rng.integers(1, 4))):
                pts.add((q, int(rng.integers(0, 70))))
        pts = sorted(pts)[:n]
        if all(b[0] - a[0] <= CHAIN_GAP for a, b in zip(pts, pts[1:])):
            return [(q0 + q, t, int(rng.integers(1, 30))) for q, t in pts]


def rand_chain_query(rng, nseg: int):
    """nseg segments with sizes drawn from SEG_SIZES, each more than max_gap behind the one before."""
    out, q0 = [], int(rng.integers(0, 50))
    for n in rng.choice(SEG_SIZES, nseg, p=SEG_WEIGHTS).tolist():
        out += rand_segment(rng, n, q0)
        q0 = out[-1][0] + CHAIN_GAP + 1 + int(rng.integers(0, 4))
    return out


def segment_sizes(anchors: dict, max_gap: int) -> np.ndarray:
    """The sizes of a batch's segments in order: cut at a query's end and where qpos advances by more than
    max_gap."""
    q = np.asarray(anchors["qpos"], np.int64)
    off = np.asarray(anchors["mem_offsets"], np.int64)
    first = np.zeros(len(q) + 1, bool)
    first[off[off < len(q)]] = True
    first[1:-1] |= np.diff(q) > max_gap
    first[-1] = True
    return np.diff(np.nonzero(first)[0])


@functools.lru_cache(maxsize=1)
def chain_pool():
    """64 queries of 0 to 9 segments (one of them empty), and one of a single diagonal of 300 anchors: one chain
    from its first anchor to its last."""
    rng = np.random.default_rng(2301)
    pool = [rand_chain_query(rng, int(rng.integers(1, 10))) for _ in range(63)] + [[]]
    pool.append([(3 * i, 5 + 3 * i, 2) for i in range(300)])
    return pool


@functools.lru_cache(maxsize=4)
def chain_answers(H: int):
    """chain_check.solve on every pool member alone."""
    return [chain_check.solve(chain_check.pack([q]), **CHAIN_PARAMS[H]) for q in chain_pool()]


def compose_chains(pool, answers, ids: np.ndarray):
    """(anchors, expected result) of the pool's queries in the order ids."""
    arr, aoff = flat_of([np.asarray(q, np.int64).reshape(len(q), 3) for q in pool], np.int64)
    an, off = tile(arr.reshape(-1, 3), aoff, ids)
    anchors = {"qpos": an[:, 0].astype(np.uint32), "tpos": an[:, 1].astype(np.uint32), "length": an[:, 2].astype(np.uint32),
               "mem_offsets": off.astype(np.uint64)}
    want = {}
    for f in ("score", "pred"):
        flat, _ = flat_of([a[f] for a in answers], answers[0][f].dtype)
        want[f], _ = tile(flat, aoff, ids)
    mflat, moff = flat_of([a["members"] for a in answers], np.uint32)
    want["members"], mout = tile(mflat, moff, ids)
    want["members_total"] = int(mout[-1])
    coff = None
    for f in chain_check.CHAIN_FIELDS:
        flat, coff = flat_of([a[f] for a in answers], answers[0][f].dtype)
        want[f], cout = tile(flat, coff, ids)
    # a pool member was solved alone, so its member_off starts at 0: the batch's go on from the members before
    want["member_off"] = (want["member_off"] + np.repeat(mout[:-1], np.diff(coff)[ids]).astype(np.uint64)).astype(np.uint64)
    want["chain_offsets"] = cout.astype(np.uint64)
    return anchors, want


@functools.lru_cache(maxsize=4)
def chain_segments_batch(H: int):
    """More than WAVES + 256 segments: random queries of the pool until there are WAVES + 700."""
    rng = np.random.default_rng(2310 + H)
    pool = chain_pool()[:64]
    nseg = np.array([len(segment_sizes(chain_check.pack([q]), CHAIN_GAP)) for q in pool])
    ids, total = [], 0
    while total < WAVES + 700:
        ids.append(int(rng.integers(0, 64)))
        total += int(nseg[ids[-1]])
    ids = np.array(ids, np.int64)
    return (ids,) + compose_chains(pool, chain_answers(H)[:64], ids)


@functools.lru_cache(maxsize=1)
def chain_anchors_batch():
    """More than CAP + 256 anchors at max_pred 64, the diagonal of 300 laid across anchor number CAP."""
    rng = np.random.default_rng(2350)
    pool = chain_pool()
    size = np.array([len(q) for q in pool])
    ids, total = [], 0
    while total < CAP - 150 - 257 * 9:          # (no random query is larger than 9 segments of 257)
        ids.append(int(rng.integers(0, 64)))
        total += int(size[ids[-1]])
    small = [i for i in range(64) if 0 < size[i] <= 100]
    while total < CAP - 250:
        ids.append(small[int(rng.integers(0, len(small)))])
        total += int(size[ids[-1]])
    across = len(ids)
    ids.append(64)
    total += 300
    while total <= REACH + 1000:
        ids.append(int(rng.integers(0, 64)))
        total += int(size[ids[-1]])
    ids = np.array(ids, np.int64)
    return (ids, across) + compose_chains(pool, chain_answers(64), ids)
