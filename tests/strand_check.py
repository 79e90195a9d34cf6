"""Both strands of search mode, restated for the tests without the library's header:

  comp_table()        the complement table from its definition: IUPAC pairs in both cases, every other byte itself
  rc(b)               the reverse complement by numpy
  item_batch(...)     the item batch of a batch on "forward", "reverse" or "both": the explicit batch that a
                      stranded call must answer like the existing call
  same_as_explicit    a stranded result against the existing call's result on the item batch: every field, its
                      dtype and its values; the stranded result has "pattern" and "strand" besides
  scenario()          the seeded 20,000-base text with reads cut from it, half of them reverse-complemented,
                      with planted substitutions and indels for k in {0, 1, 2}; shared by the host and the
                      device tests, built once
  edge_batches()      the kernel's edge batches: every length of EDGE_LENGTHS at every start alignment mod 8 in
                      both halves, bytes of the whole IUPAC alphabet in both cases and non-letters above '$'
"""
import functools

import numpy as np

PAIRS = ("AT", "CG", "RY", "KM", "BV", "DH")
STRANDS = ("forward", "reverse", "both")
EDGE_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
# IUPAC in both cases, U, and non-letters above '$'
ALPHABET = np.frombuffer(b"ACGTRYKMBVDHSWNUacgtrykmbvdhswnu%*-.0279@[^_{~" + bytes([0x7F, 0x80, 0xC3, 0xFF]), np.uint8)


@functools.lru_cache(maxsize=None)
def _table_bytes() -> bytes:
    t = list(range(256))
    for a, b in PAIRS:
        for x, y in ((a, b), (b, a)):
            t[ord(x)] = ord(y)
            t[ord(x.lower())] = ord(y.lower())
    return bytes(t)


def comp_table() -> np.ndarray:
    return np.frombuffer(_table_bytes(), np.uint8)


def rc(b: bytes) -> bytes:
    return comp_table()[np.frombuffer(bytes(b), np.uint8)[::-1]].tobytes()


def item_batch(patterns, strands: str):
    """The items of `patterns` (a list of bytes) on `strands`, as a list of bytes."""
    patterns = [bytes(p) for p in patterns]
    if strands == "forward":
        return patterns
    rev = [rc(p) for p in patterns]
    return rev if strands == "reverse" else patterns + rev


def packed(items):
    """(uint8 bytes back to back, uint64 offsets) of a list of bytes."""
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), np.uint8), off


def same_as_explicit(result: dict, explicit: dict, npat: int, strands: str):
    """`result`: a stranded call's; `explicit`: the existing call's on item_batch(patterns, strands)."""
    extra = set() if strands == "forward" else {"pattern", "strand"}
    assert set(result) == set(explicit) | extra, (sorted(result), sorted(explicit))
    for key, want in explicit.items():
        got = result[key]
        if want is None or not isinstance(want, np.ndarray):
            assert got == want if want is not None else got is None, key
            continue
        assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, got.shape, want.shape)
        assert np.array_equal(got, want), key
    if extra:
        reps = 2 if strands == "both" else 1
        assert result["pattern"].dtype == np.uint32 and result["strand"].dtype == np.uint8
        assert result["pattern"].tolist() == list(range(npat)) * reps
        assert result["strand"].tolist() == ([0] * npat + [1] * npat if strands == "both" else [1] * npat)


def _other(c: int, rng) -> int:
    return int([x for x in b"ACGT" if x != c][int(rng.integers(0, 3))])


def _edit(window: bytes, rng, count: int, subs_only: bool) -> bytes:
    p = bytearray(window)
    cols = sorted(rng.choice(len(p), count, replace=False).tolist(), reverse=True)
    for c in cols:
        kind = 0 if subs_only else int(rng.integers(0, 3))
        if kind == 0:
            p[c] = _other(p[c], rng)
        elif kind == 1:
            p.insert(c, _other(p[c], rng))
        else:
            del p[c]
    return bytes(p)


class Scenario:
    """text: 20,000 seeded bases.  reads[r] with cut[r] = (start, end of its window in the text), edits[r] (how
    many were planted), subs[r] (substitutions only) and reverse[r] (the read is the reverse complement of the
    edited window: only the - strand finds it)."""

    def __init__(self, seed=2024, n=20000):
        rng = np.random.default_rng(seed)
        self.text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
        self.reads, self.cut, self.edits, self.subs, self.reverse = [], [], [], [], []
        r = 0
        for count in (0, 1, 2):
            for subs_only in (True, False):
                for m in (24, 33, 57, 64):
                    for _ in range(2):
                        i = int(rng.integers(0, n - m + 1))
                        read = _edit(self.text[i:i + m], rng, count, subs_only)
                        rev = r % 2 == 1
                        self.reads.append(rc(read) if rev else read)
                        self.cut.append((i, i + m))
                        self.edits.append(count)
                        self.subs.append(subs_only or count == 0)
                        self.reverse.append(rev)
                        r += 1
        # the long query: a forward block, then an inverted block of the text
        self.blocks = ((1000, 1300), (7000, 7300))
        (a0, a1), (b0, b1) = self.blocks
        self.query = self.text[a0:a1] + rc(self.text[b0:b1])

    def select(self, max_edits: int, subs_only: bool):
        """Indices of the reads with at most max_edits planted edits (substitutions only when asked)."""
        return [r for r in range(len(self.reads)) if self.edits[r] <= max_edits and (self.subs[r] or not subs_only)]


@functools.lru_cache(maxsize=None)
def scenario() -> Scenario:
    return Scenario()


def edge_batches():
    """[(id, [items as bytes])]: eight rotations of EDGE_LENGTHS, rotation q behind a filler of q bytes.  The
    lengths sum to 1,341 = 5 mod 8, so the totals 5 + q take every value mod 8.  One filler a rotation cannot
    give every length every start alignment in both halves at once (a reverse item starts at the total plus its
    forward start, and the filler moves both), so the list behind a filler of f bytes and in front of a tail
    of t bytes follows for every (f, t): a length's forward start takes every residue over f, and for each f
    its reverse start takes every residue over t.  That is asserted below, not assumed.  Then the degenerate
    and the long batches."""
    rng = np.random.default_rng(99)

    def draw(m):
        return ALPHABET[rng.integers(0, ALPHABET.size, m)].tobytes()

    out = []
    for q in range(8):
        lens = [q] + list(EDGE_LENGTHS[q:] + EDGE_LENGTHS[:q])
        out.append((f"rotation{q}", [draw(m) for m in lens]))
    assert sorted({sum(len(x) for x in items) % 8 for _, items in out}) == list(range(8))
    for f in range(8):
        for t in range(8):
            out.append((f"filler{f}-tail{t}", [draw(m) for m in [f] + list(EDGE_LENGTHS) + [t]]))
    seen = {}
    for _, items in out:
        total, at = sum(len(x) for x in items), len(items[0])
        for x in items[1:]:   # (not the filler)
            seen.setdefault(len(x), set()).add((at % 8, (total + at) % 8))
            at += len(x)
    for m in EDGE_LENGTHS:
        assert {a for a, _ in seen[m]} == set(range(8)) and {b for _, b in seen[m]} == set(range(8)), m
    out.append(("n0", []))
    out.append(("n1-m0", [b""]))
    out.append(("all-empty", [b""] * 300))
    out.append(("m65535", [draw(65535)]))
    out.append(("m70001", [draw(70001)]))
    out.append(("empties-between", [draw(3), b"", b"", draw(5), b"", draw(1), b""]))
    return out


def expected_items(items, strands: str):
    """(bytes, offsets) of the item batch of `items`, by this file's rule."""
    return packed(item_batch(items, strands))
