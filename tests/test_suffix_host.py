"""Suffix-tree mode on the host solver (no device): gx_suffix_tree_stats with
ctx = NULL against a brute-force restatement (suffixes sorted explicitly, LCP by
direct compare, the interval rule of DESIGN.md 17.1), against the reference's
own BWT files and asserted node counts (tests/golden/suffix), the error codes,
Display for TreeStats, and the crate-shaped SuffixTree mirror.  Beyond the
brute force's reach (n > 300: every admitted byte, half a Mi of random ACGT,
mutated tandem copies, unary input) the checker of tests/suffix_check.py is
the reference; it is itself checked against the brute force and against seven
corruptions it must reject."""
import gzip
import hashlib
import json
import math
import os
import random

import numpy as np
import pytest

import oracle as oracle_mod
from conftest import COMPARISON, GOLDEN, read_fasta_records
from suffix_check import check_arrays, fold_stats

SUFFIX = os.path.join(GOLDEN, "suffix")
ALPHABETS = os.path.join(GOLDEN, "alphabets")


def load_vectors():
    with open(os.path.join(SUFFIX, "suffix_vectors.json")) as f:
        return json.load(f)["vectors"]


def vector_text(v) -> bytes:
    if "text" in v:
        return v["text"].encode()
    if "fasta" in v:
        return fasta_first(os.path.join(GOLDEN, v["fasta"]))
    p = np.fromfile(os.path.join(SUFFIX, v["acgt2"]), np.uint8)
    codes = np.stack([(p >> (2 * k)) & 3 for k in range(4)], 1).reshape(-1)[:v["n"]]
    return np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()


def read_golden(path) -> bytes:
    """A fixture's bytes; the large ones are kept gzip-compressed, otherwise as the reference wrote them."""
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        return f.read()


def fasta_first(path) -> bytes:
    return oracle_mod.fasta_parse(read_golden(path))[0][1]


def read_bwt_file(name) -> bytes:
    return read_golden(os.path.join(SUFFIX, name)).replace(b"\n", b"")


def brute(s: bytes):
    """(sa, lcp, bwt, stats dict) of s + '$' by the definitions."""
    t = s + b"$"
    N = len(t)
    sa = sorted(range(N), key=lambda i: t[i:])
    lcp = [0] * N
    for k in range(1, N):
        a, b = t[sa[k - 1]:], t[sa[k]:]
        h = 0
        while h < len(a) and h < len(b) and a[h] == b[h]:
            h += 1
        lcp[k] = h
    bwt = bytes(t[i - 1] if i else 0x24 for i in sa)
    cnt = dsum = 0
    for k in range(1, N):
        if lcp[k] == 0:
            continue
        kk = k - 1
        while lcp[kk] > lcp[k]:   # (position 0 holds 0: the sentinel)
            kk -= 1
        if lcp[kk] < lcp[k]:
            cnt += 1
            dsum += lcp[k]
    mx = max(lcp)
    ks = lcp.index(mx)
    st = {"num_internal": cnt, "num_leaves": N, "num_nodes": cnt + N + 1, "string_depth_sum": dsum,
          "max_string_depth": mx, "longest_repeat_len": mx, "longest_repeat_start": sa[ks - 1] + 1 if mx else 0}
    return sa, lcp, bwt, st


def raw_dict(raw):
    return {k: getattr(raw, k) for k, _ in raw._fields_}


def test_host_matches_brute_force(gx):
    # (brute_cases() below restates this generator: seed, lengths, alphabets; keep the two in step)
    rng = random.Random(20260117)
    lengths = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 300] + [rng.randrange(0, 301) for _ in range(189)]
    assert len(lengths) == 200
    for k, n in enumerate(lengths):
        alpha = (b"A", b"AC", b"ACGT")[k % 3]
        s = bytes(rng.choice(alpha) for _ in range(n))
        r = gx.suffix_tree_stats(s, host=True, want=("bwt", "sa", "lcp"))
        sa, lcp, bwt, st = brute(s)
        assert r["sa"].tolist() == sa, s
        assert r["lcp"].tolist() == lcp, s
        assert r["bwt"] == bwt, s
        assert raw_dict(r["raw"]) == st, s


def test_empty_input(gx):
    r = gx.suffix_tree_stats(b"", host=True)
    assert r["bwt"] == b"$"
    assert (r["raw"].num_leaves, r["raw"].num_internal, r["raw"].num_nodes) == (1, 0, 2)
    assert math.isnan(r["stats"].average_string_depth)


@pytest.mark.parametrize("v", load_vectors(), ids=lambda v: v["name"])
def test_reference_vectors(gx, v):
    s = vector_text(v)
    assert len(s) == v["n"]
    r = gx.suffix_tree_stats(s, host=True)
    for key in ("num_internal", "num_leaves", "num_nodes", "string_depth_sum", "max_string_depth",
                "longest_repeat_start"):
        assert getattr(r["raw"], key) == v[key][0], key
    assert r["raw"].longest_repeat_len == v["max_string_depth"][0]
    if v.get("bwt"):
        assert r["bwt"] == read_bwt_file(v["bwt"])
    if v.get("bwt_text"):
        assert r["bwt"] == v["bwt_text"][0].encode()
    if v.get("bwt_sha256"):
        assert hashlib.sha256(r["bwt"]).hexdigest() == v["bwt_sha256"][0]


def test_error_codes(gx):
    for bad in (b"AC$GT", b"AC GT", b"$", b" "):
        with pytest.raises(gx.GxError) as e:
            gx.suffix_tree_stats(bad, host=True)
        assert e.value.code == 1   # GX_EINVAL


BANANA_DISPLAY = ("\n"
                  "            BWT: ANNB$AA\n"
                  "            BWT Length: 7\n"
                  "            Internal nodes: 3\n"
                  "            Leaves: 7\n"
                  "            Nodes: 11\n"
                  "            Average string depth: 2\n"
                  "            Max string depth: 3\n"
                  "            Longest repeat start: 4\n"
                  "            Longest repeat length: 3\n"
                  "            ")


def test_format_stats(gx):
    r = gx.suffix_tree_stats(b"BANANA", host=True)
    assert gx.format_suffix_stats(r["raw"], r["bwt"]) == BANANA_DISPLAY
    assert str(r["stats"]) == BANANA_DISPLAY
    # the size query reports the text and its NUL; a short buffer is GX_ECAP
    import ctypes
    need = ctypes.c_size_t()
    kb, pb = gx._buf(r["bwt"])
    assert gx.lib().gx_format_suffix_stats(ctypes.byref(r["raw"]), pb, 7, None, 0, ctypes.byref(need)) == 7
    assert need.value == len(BANANA_DISPLAY) + 1
    covid = read_fasta_records(os.path.join(COMPARISON, "Covid_Wuhan.fasta"))[0][1]
    rc = gx.suffix_tree_stats(covid, host=True)
    txt = gx.format_suffix_stats(rc["raw"], rc["bwt"])
    assert "\n            Average string depth: 7.386637344224527\n" in txt
    assert "\n            BWT: " + rc["bwt"][:100].decode() + "... (truncated)\n" in txt
    assert "\n            BWT Length: 29904\n" in txt
    ra = gx.suffix_tree_stats(b"A", host=True)
    assert "\n            Average string depth: NaN\n" in gx.format_suffix_stats(ra["raw"], ra["bwt"])


@pytest.mark.parametrize("alphabet, text, internal, leaves, nodes, avg, depth, bwt", [
    ("dna.txt", "ACA", None, None, 6, None, None, None),
    ("banana.txt", "BANANA", 3, 7, 11, 2.0, 3, "ANNB$AA"),
    ("english.txt", "MISSISSIPPI", 6, 12, 19, 2.0, 4, "IPSSM$PISSII"),
])
def test_suffix_tree_mirror(gx, alphabet, text, internal, leaves, nodes, avg, depth, bwt):
    """test_tree_simple2 / 3 / 4 (tests/test_suffixtree.rs:7-48)."""
    tree = gx.SuffixTree(os.path.join(ALPHABETS, alphabet), 20, host=True)
    tree.insert_string(text, True, True)
    tree.compute_stats(0)
    assert tree.stats.num_nodes == nodes
    if internal is not None:
        assert tree.stats.num_internal == internal
        assert tree.stats.num_leaves == leaves
        assert tree.stats.average_string_depth == avg
        assert tree.stats.max_string_depth == depth
        assert tree.stats.longest_repeat_len == depth
        assert tree.stats.bwt == bwt
    assert str(tree) == "\nStats: " + str(tree.stats) + "\n"


def test_suffix_tree_mirror_alphabet(gx):
    tree = gx.SuffixTree(os.path.join(ALPHABETS, "dna.txt"), 10, host=True)
    with pytest.raises(ValueError, match="Character N not found in alphabet"):
        tree.insert_string("ACNGT", False, False)
    with pytest.raises(RuntimeError, match="Could not read alphabet file"):
        gx.SuffixTree(os.path.join(ALPHABETS, "missing.txt"), 10, host=True)


def test_suffix_tree_mirror_get_lcs(gx):
    with open(os.path.join(GOLDEN, "lcs_vectors.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 5
    for c in cases:
        if "fasta" in c:
            a = b = read_fasta_records(os.path.join(GOLDEN, c["fasta"]))[c["record"]][1].decode()
            expect = (0, 0, len(a))
            alphabet = "dna.txt"
        else:
            a, b = c["a"], c["b"]
            expect = tuple(c["expect"]) if c["expect"] else None
            alphabet = "banana.txt" if "B" in a else "dna.txt"
        tree = gx.SuffixTree(os.path.join(ALPHABETS, alphabet), 10, host=True)
        tree.insert_string(a, True, True)
        tree.insert_string(b, True, True)
        got = tree.get_lcs(0, 1)
        assert got == gx.common_substring_host(a.encode(), b.encode())
        if expect:
            assert got == expect, c["name"]


# ---------------------------------------------------------------------------
# Beyond brute's reach the reference is tests/suffix_check.py: check_arrays and
# fold_stats verify the arrays from the definitions and share nothing with the
# host solver's construction (doubling, its keys and padding, Kasai's order).

BYTES_219 = bytes(range(0x25, 0x100))   # every byte the ABI admits
SIGN_EDGE = b"\x7f\x80"                 # straddles the sign bit of a byte


def np_rand(seed, alpha: bytes, n: int) -> bytes:
    """n letters of alpha, uniform, from numpy.random.default_rng(seed)."""
    letters = np.frombuffer(alpha, np.uint8)
    return letters[np.random.default_rng(seed).integers(0, len(alpha), n)].tobytes()


def mutated_tandem_copies(seed=7, copies=48, block=4096, mutations=64) -> bytes:
    """`copies` copies of one random ACGT block, each with `mutations` positions
    (drawn without replacement) overwritten with random letters: long repeats
    between every pair of copies, so many doubling rounds, at a length whose
    ranks need three digit bytes (48 * 4,096 + 1 = 196,609 suffixes)."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    text = np.tile(letters[rng.integers(0, 4, block)], (copies, 1))
    for c in range(copies):
        text[c, rng.choice(block, mutations, replace=False)] = letters[rng.integers(0, 4, mutations)]
    return text.tobytes()


def brute_cases():
    """The 200 strings of test_host_matches_brute_force, by a copy of its
    generator (that test is left as it was): the same seed, lengths and
    alphabet rotation, drawn in the same order.  Keep the two in step."""
    rng = random.Random(20260117)
    lengths = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 300] + [rng.randrange(0, 301) for _ in range(189)]
    for k, n in enumerate(lengths):
        alpha = (b"A", b"AC", b"ACGT")[k % 3]
        yield bytes(rng.choice(alpha) for _ in range(n))


def test_checker_accepts_brute_force():
    cases = list(brute_cases())
    assert len(cases) == 200
    for s in cases:
        sa, lcp, bwt, st = brute(s)
        assert check_arrays(s, sa, lcp, bwt, max_work=len(s) ** 2 + 1) == sum(lcp) + len(s), s
        assert fold_stats(sa, lcp) == st, s


@pytest.fixture(scope="module")
def solved_3000(gx):
    s = np_rand(3000, b"ACGT", 3000)
    r = gx.suffix_tree_stats(s, host=True, want=("bwt", "sa", "lcp"))
    check_arrays(s, r["sa"], r["lcp"], r["bwt"])
    return s, r["sa"], r["lcp"], np.frombuffer(r["bwt"], np.uint8)


def corrupt_lcp_plus_one(s, sa, lcp, bwt):
    lcp[1500] += 1


def corrupt_lcp_max_minus_one(s, sa, lcp, bwt):
    lcp[np.argmax(lcp)] -= 1


def corrupt_sa_swap(s, sa, lcp, bwt):
    sa[[1500, 1501]] = sa[[1501, 1500]]


def corrupt_sa_duplicate(s, sa, lcp, bwt):
    sa[1500] = sa[700]


def corrupt_bwt_byte(s, sa, lcp, bwt):
    bwt[1500] = ord("A") if bwt[1500] != ord("A") else ord("C")


def corrupt_lcp0(s, sa, lcp, bwt):
    lcp[0] = 1


@pytest.mark.parametrize("corrupt, clause", [
    (corrupt_lcp_plus_one, "bounds|too large"), (corrupt_lcp_max_minus_one, "order"), (corrupt_sa_swap, None),
    (corrupt_sa_duplicate, "permutation"), (corrupt_bwt_byte, "bwt"), (corrupt_lcp0, r"lcp\[0\]")],
    ids=lambda v: v.__name__[8:] if callable(v) else None)
def test_checker_rejects_corruption(solved_3000, corrupt, clause):
    s, sa, lcp, bwt = solved_3000
    sa, lcp, bwt = sa.copy(), lcp.copy(), bwt.copy()
    corrupt(s, sa, lcp, bwt)
    with pytest.raises(AssertionError, match=clause):
        check_arrays(s, sa, lcp, bwt)


def test_checker_work_cap_fails(solved_3000):
    s, sa, lcp, bwt = solved_3000
    total = int(lcp.sum())
    assert check_arrays(s, sa, lcp, bwt, max_work=total) == total + len(s)
    with pytest.raises(AssertionError, match="max_work"):
        check_arrays(s, sa, lcp, bwt, max_work=total - 1)
    # the default cap, 128 * N, on an input far above it
    u = b"A" * 1000
    usa, ulcp, ubwt, _ = brute(u)
    with pytest.raises(AssertionError, match="max_work"):
        check_arrays(u, usa, ulcp, ubwt)


def host_against_checker(gx, s, max_work=None):
    r = gx.suffix_tree_stats(s, host=True, want=("bwt", "sa", "lcp"))
    check_arrays(s, r["sa"], r["lcp"], r["bwt"], max_work=max_work)
    assert raw_dict(r["raw"]) == fold_stats(r["sa"], r["lcp"])
    return r


def test_host_full_byte_range(gx):
    """Bytes up to 0xFF: round 0 keys with bit 63 set, and the unsigned order at the sign bit."""
    for alpha in (BYTES_219, SIGN_EDGE):
        s = np_rand(len(alpha), alpha, 300)
        r = gx.suffix_tree_stats(s, host=True, want=("bwt", "sa", "lcp"))
        sa, lcp, bwt, st = brute(s)   # (Python compares bytes unsigned)
        assert (r["sa"].tolist(), r["lcp"].tolist(), r["bwt"], raw_dict(r["raw"])) == (sa, lcp, bwt, st)
    host_against_checker(gx, np_rand(219, BYTES_219, 5000))
    host_against_checker(gx, np_rand(2, SIGN_EDGE, 5000))


def test_host_random_half_mi(gx):
    host_against_checker(gx, np_rand(524288, b"ACGT", 524288))


def test_host_mutated_tandem_copies(gx):
    s = mutated_tandem_copies()
    assert len(s) + 1 == 196609
    r = host_against_checker(gx, s)   # (inside the default cap: sum(lcp) / N is near 80)
    assert r["raw"].max_string_depth >= 256   # more than the offsets 8 .. 128 resolve: eight rounds or more


def test_host_unary_threshold(gx):
    s = b"A" * 4096
    r = host_against_checker(gx, s, max_work=(len(s) + 1) ** 2)
    assert r["raw"].max_string_depth == 4095


def test_tile_constants(gx):
    T, C, B = gx.suffix_tile()
    assert T > 0 and T % 64 == 0 and C > 0 and B > 0
