"""CPU: the host solver of compare mode (gx_common_substring_host, and
gx_compare_pair without a context) against a brute-force restatement of the
contract in DESIGN.md 16.1:

  lcs(a, b) -> (i, j, L): L = the longest common substring's length, W = the
  lexicographically smallest common substring of that length, i / j = the
  start of the smallest suffix of a + '$' / b + '!' that begins with W.
  compare_pair(a, b) -> (score, first_L, calls): the sum of L over the
  traversal that recurses on the pieces before and after each hit.

The restatement builds the O(n m) table of diagonal run lengths with numpy and
sorts the candidate substrings and terminated suffixes explicitly.  It is
pinned by the reference's own get_lcs assertions (tests/golden/
lcs_vectors.json, from tests/test_suffixtree.rs:135-237).

The restatement orders bytes as Python does (unsigned); the byte-range cases
hold the host solver to it at the edges of the admitted range (0x25, 0x7F,
0x80, 0xFF), and tests/test_gpu_compare.py runs the same cases on the kernels."""
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, read_fasta_records


def ref_lcs(a: bytes, b: bytes):
    n, m = len(a), len(b)
    if not n or not m:
        return (0, 0, 0)
    A = np.frombuffer(a, np.uint8)
    B = np.frombuffer(b, np.uint8)
    run = np.zeros((n + 1, m + 1), np.int64)
    for i in range(n):
        run[i + 1, 1:] = np.where(A[i] == B, run[i, :-1] + 1, 0)
    L = int(run.max())
    if L == 0:
        return (0, 0, 0)
    subs = sorted({a[ie - L:ie] for ie, _ in np.argwhere(run == L)})
    W = subs[0]
    i = sorted((a[k:] + b"$", k) for k in range(n - L + 1) if a[k:k + L] == W)[0][1]
    j = sorted((b[k:] + b"!", k) for k in range(m - L + 1) if b[k:k + L] == W)[0][1]
    return (i, j, L)


def ref_compare(a: bytes, b: bytes, lcs=ref_lcs):
    """(score, first_L, get_matches calls) of main.rs:281-315 on top of `lcs`."""
    first = lcs(a, b)
    stack = [(first, a, b)]
    score, calls = 0, 1
    while stack:
        (i, j, L), s1, s2 = stack.pop()
        if L > 0:
            for p, q in ((s1[:i], s2[:j]), (s1[i + L:], s2[j + L:])):
                stack.append((lcs(p, q), p, q))
                calls += 1
        score += L
    return score, first[2], calls


def vectors():
    with open(os.path.join(GOLDEN, "lcs_vectors.json")) as f:
        cases = json.load(f)["cases"]
    out = []
    for c in cases:
        if "fasta" in c:
            s = read_fasta_records(os.path.join(GOLDEN, c["fasta"]))[c["record"]][1]
            out.append((c["name"], s, s, (0, 0, len(s)), False))
        else:
            out.append((c["name"], c["a"].encode(), c["b"].encode(),
                        tuple(c["expect"]) if c["expect"] else None, True))
    return out


def tie_pairs(count=200, seed=11, lo=1, hi=40, alphabet=b"AB"):
    rng = random.Random(seed)
    return [tuple(bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(2))
            for _ in range(count)]


def periodic_pairs():
    return [(b"AB" * 20, b"AB" * 13 + b"A"), (b"BA" * 9 + b"B", b"AB" * 16), (b"ABC" * 11, b"BCA" * 7 + b"B"),
            (b"A" * 17, b"A" * 9), (b"AAB" * 8, b"ABA" * 5)]


def random_pairs(count=6, seed=5, hi=300, alphabet=b"ACGT"):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        a = bytes(rng.choice(alphabet) for _ in range(rng.randint(hi // 2, hi)))
        b = bytearray(rng.choice(alphabet) for _ in range(rng.randint(hi // 2, hi)))
        k = rng.randint(5, 40)   # a shared block, so that the recursion has depth
        p, q = rng.randrange(len(a) - k), rng.randrange(len(b) - k)
        b[q:q + k] = a[p:p + k]
        out.append((a, bytes(b)))
    return out


# The admitted byte range at its edges: the lowest admitted byte next to the
# highest, the two sides of the signed-char line, and all four together.
BYTE_ALPHABETS = (b"\x25\xff", b"\x7f\x80", b"\x25\x7f\x80\xff")

_byte_range = {}


def byte_range_cases(alphabet):
    """[(a, b, ref_lcs(a, b), ref_compare(a, b))] over `alphabet`: 100 seeded
    pairs of 1..40 bytes and the periodic shapes with their letters mapped
    onto the alphabet in rising and in falling order, each pair in both
    argument orders.  Computed once per alphabet and shared (CPU and GPU tests)."""
    if alphabet not in _byte_range:
        pairs = tie_pairs(100, seed=17, alphabet=alphabet)
        for letters in (alphabet, alphabet[::-1]):
            to = bytes.maketrans(b"ABC", bytes(letters[k % len(letters)] for k in range(3)))
            pairs += [(a.translate(to), b.translate(to)) for a, b in periodic_pairs()]
        pairs += [(b, a) for a, b in pairs]
        _byte_range[alphabet] = [(a, b, ref_lcs(a, b), ref_compare(a, b)) for a, b in pairs]
    return _byte_range[alphabet]


def test_restatement_matches_reference_fixtures():
    for name, a, b, want, small in vectors():
        if small and want is not None:
            assert ref_lcs(a, b) == want, name


def test_host_solver_on_reference_fixtures(gx):
    for name, a, b, want, small in vectors():
        got = gx.common_substring_host(a, b)
        if want is not None:
            assert got == want, name
        if small:
            assert got == ref_lcs(a, b), name


def test_host_solver_edges(gx):
    assert gx.common_substring_host(b"", b"") == (0, 0, 0)
    assert gx.common_substring_host(b"", b"ACGT") == (0, 0, 0)
    assert gx.common_substring_host(b"ACGT", b"") == (0, 0, 0)
    assert gx.common_substring_host(b"A", b"C") == (0, 0, 0)
    assert gx.common_substring_host(b"A", b"A") == (0, 0, 1)
    assert gx.common_substring_host(b"AAAA", b"AAA") == (1, 0, 3)
    for a, b in [(b"A", b"CA"), (b"CA", b"A"), (b"G", b"ACGT"), (b"AAA", b"AAAA")]:
        assert gx.common_substring_host(a, b) == ref_lcs(a, b), (a, b)


def test_host_solver_periodic(gx):
    for a, b in periodic_pairs():
        assert gx.common_substring_host(a, b) == ref_lcs(a, b), (a, b)
        assert gx.common_substring_host(b, a) == ref_lcs(b, a), (b, a)


def test_host_solver_two_letter_ties(gx):
    for a, b in tie_pairs():
        assert gx.common_substring_host(a, b) == ref_lcs(a, b), (a, b)


def test_host_solver_random_pairs(gx):
    for a, b in random_pairs():
        assert gx.common_substring_host(a, b) == ref_lcs(a, b), (a, b)


@pytest.mark.parametrize("alphabet", BYTE_ALPHABETS, ids=lambda s: s.hex())
def test_host_solver_full_byte_range(gx, alphabet):
    """The tie rule orders bytes (resolve, suffix_less: memcmp) and so does the
    restatement (Python's bytes order): both unsigned, across 0x7F / 0x80 and
    from the lowest admitted byte 0x25 to 0xFF."""
    for a, b, want_lcs, want_cmp in byte_range_cases(alphabet):
        assert gx.common_substring_host(a, b) == want_lcs, (a, b)
        assert gx.compare_pair(a, b, host=True) == want_cmp, (a, b)


def test_knob_clamps(gx, monkeypatch):
    """GX_COMPARE_SEG_H is read on every call and clamped to [8, 32768]
    (the tile element keeps its runs in 16 bits); a non-number is the default."""
    for value, want in ((0, 8), (1, 8), (7, 8), (8, 8), (9, 9), (32768, 32768), (32769, 32768), (10**12, 32768),
                        ("x", 1024)):
        monkeypatch.setenv("GX_COMPARE_SEG_H", str(value))
        assert gx.compare_segment_height() == want, value
    monkeypatch.delenv("GX_COMPARE_SEG_H")
    assert gx.compare_segment_height() == 1024


def test_host_compare_pair(gx):
    """gx_compare_pair without a context (host recursion) == the restatement's
    recursion, and == the same recursion driven from Python over
    gx_common_substring_host."""
    cases = [(a, b) for _, a, b, _, small in vectors() if small]
    cases += periodic_pairs() + tie_pairs(60, seed=3) + random_pairs(3) + [(b"", b"ACGT"), (b"ACGT", b"")]
    for a, b in cases:
        want = ref_compare(a, b)
        assert gx.compare_pair(a, b, host=True) == want, (a, b)
        assert ref_compare(a, b, lcs=gx.common_substring_host) == want, (a, b)


def test_host_compare_matrix(gx):
    seqs = [a for a, _ in random_pairs(4, seed=9, hi=120)]
    mat = gx.compare_matrix(seqs, host=True)
    for j in range(len(seqs)):
        for i in range(len(seqs)):
            if i > j:
                assert not mat[j, i].any()
            else:
                score, first, _ = ref_compare(seqs[i], seqs[j])
                assert [int(x) for x in mat[j, i]] == [score, len(seqs[i]), len(seqs[j]), first], (i, j)
                if i == j:
                    assert int(mat[j, i, 0]) == len(seqs[i])


def test_low_bytes_are_rejected(gx):
    for bad in (b"AC$GT", b"AC!GT", b"AC GT", b"AC\nGT", b"\x00"):
        for a, b in ((bad, b"ACGT"), (b"ACGT", bad)):
            with pytest.raises(gx.GxError) as e:
                gx.common_substring_host(a, b)
            assert e.value.code == 1   # GX_EINVAL
            with pytest.raises(gx.GxError) as e:
                gx.compare_pair(a, b, host=True)
            assert e.value.code == 1
    assert gx.common_substring_host(b"%%A", b"A%%") == ref_lcs(b"%%A", b"A%%")   # 0x25 is the lowest admitted byte
