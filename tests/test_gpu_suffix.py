"""Suffix-tree mode on the GPU: SA, LCP, BWT and the statistics of
gx_suffix_tree_stats element by element against the host solver (itself pinned
by tests/test_suffix_host.py), at the sizes where the kernels of gx_suffix.hip
change path (T sort items per workgroup, C text positions per LCP lane, B LCP
entries per fold block), on the reference's fixtures, and through `gx-align
suffix-tree`.

The host solver and the device share their construction (the doubling's keys,
the zero padding, Kasai's order), so the second family of tests here does not
consult it: check_definition verifies the device's own arrays from the
definitions (tests/suffix_check.py).  Its sizes, with W = 256 threads per
workgroup, N = n + 1:

  rank scan's chunk edge    N in {W T, W T + 1}: 256 and 257 partials of the
                            scan over the head flags, where the one-workgroup
                            scan of the partials starts to carry between chunks
  table scan's chunk edge   N in {T T, T T + 1}: T and T + 1 tiles, 256 and 257
                            partials of the scan over the [256][tiles] histogram
                            table of every radix pass (the largest cases here)
  every admitted byte       0x25..0xFF at n = T - 1 and 5,000, {0x7F, 0x80} at
                            5,000: keys with bit 63 set, digits above 'T'
  many rounds, wide ranks   48 mutated copies of a 4,096-base block, N = 196,609:
                            seven doubling rounds or more and radix passes on
                            rank bits 16-23 (beyond round 0's one per digit)
  NULL outputs              every subset of one of (bwt, sa, lcp), and none
  sizes falling and rising  n = 4 T + 1, 65, 3 T, 1, 4 T + 1 on one context: the
                            pooled buffers larger than the call and stale

Not covered: N >= 2^24, the fourth digit byte of a rank."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from suffix_check import check_arrays, fold_stats
from test_suffix_host import (BYTES_219, SIGN_EDGE, load_vectors, mutated_tandem_copies, np_rand, raw_dict,
                              read_bwt_file, read_golden, vector_text)

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "genomics-rs_amd", "gx-align")
WANT = ("bwt", "sa", "lcp")


@pytest.fixture(autouse=True)
def device_for_every_size(monkeypatch):
    monkeypatch.setenv("GX_SUFFIX_HOST_BELOW", "0")


def tiles(gx):
    return gx.suffix_tile()


def check(gx, ctx, s: bytes):
    """Device = host solver, element by element, and the kernels ran."""
    d = gx.suffix_tree_stats(s, ctx=ctx, want=WANT)
    info = gx.suffix_info(ctx)
    h = gx.suffix_tree_stats(s, host=True, want=WANT)
    assert np.array_equal(d["sa"], h["sa"]), f"SA differs first at {np.flatnonzero(d['sa'] != h['sa'])[:4]}"
    assert np.array_equal(d["lcp"], h["lcp"]), f"LCP differs first at {np.flatnonzero(d['lcp'] != h['lcp'])[:4]}"
    assert d["bwt"] == h["bwt"]
    assert raw_dict(d["raw"]) == raw_dict(h["raw"])
    assert info["doubling_rounds"] >= 1 and info["sort_passes"] >= 1, info
    return d, info


def check_definition(gx, ctx, s: bytes, want=WANT, max_work=None):
    """The device's own SA, LCP and BWT satisfy their definitions and its
    statistics are their fold (tests/suffix_check.py), and the kernels ran,
    the LCP and fold kernels included.  The host solver is not consulted.
    `want` must name sa and lcp (there is nothing to check without them); bwt
    is checked when it is asked for."""
    assert "sa" in want and "lcp" in want, want
    d = gx.suffix_tree_stats(s, ctx=ctx, want=want)
    info = gx.suffix_info(ctx)
    assert info["doubling_rounds"] >= 1 and info["sort_passes"] >= 1, info
    assert info["lcp_ms"] > 0 and info["fold_ms"] > 0, info
    assert sum(info["digit_passes"]) == info["sort_passes"], info
    check_arrays(s, d["sa"], d["lcp"], d.get("bwt"), max_work=max_work)
    assert raw_dict(d["raw"]) == fold_stats(d["sa"], d["lcp"])
    return d, info


def scan_chunk(gx):
    """(T, W): sort and scan items per workgroup, and the partials the
    one-workgroup scan of suf_scan_part_kernel takes per chunk, which is the
    workgroup size kSufBlock.  gx_suffix_tile does not report kSufBlock itself;
    the fold block B is defined as kSufBlock (kSufFoldBlock = kSufBlock,
    gx_suffix.h), so B stands in for it and is pinned to the literal here."""
    T, _, B = tiles(gx)
    assert B == 256
    return T, 256


def rand(rng, alpha: bytes, n: int) -> bytes:
    return bytes(rng.choice(alpha) for _ in range(n))


def sizes(gx):
    """String lengths n.  The tile edges are edges of N = n + 1, the number of
    suffixes the kernels see: N in {2, 3, 63, 64, 65, T-1, T, T+1, 2T+1, 3T} (one
    short of a wave, one inactive lane in a full tile, a tile holding a single
    item, a last tile exactly full).  N = 1 is the empty string, which goes to
    the host solver: test_empty_input_with_context.  The same values taken as n
    (N one more) ride along."""
    T, _, _ = tiles(gx)
    edges = [2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T]
    return sorted({N - 1 for N in edges} | set(edges))


@pytest.mark.parametrize("alpha", [b"ACGT", b"AC"], ids=["acgt", "ac"])
def test_sizes(gx, ctx, alpha):
    rng = random.Random(len(alpha))
    for n in sizes(gx):
        check(gx, ctx, rand(rng, alpha, n))


def test_unary(gx, ctx):
    """One digit bucket in every pass, the most doubling rounds, the LCP kernel's worst case."""
    T, _, _ = tiles(gx)
    for n in (1, 64, 4096, 3 * T):
        d, info = check(gx, ctx, b"A" * n)
        assert d["raw"].max_string_depth == n - 1
        if n >= 64:
            assert info["doubling_rounds"] >= 2


def test_periodic_and_fibonacci(gx, ctx):
    check(gx, ctx, b"AB" * 2500)
    a, b = b"A", b"AB"
    while len(b) < 10000:
        a, b = b, b + a
        if len(b) in (13, 233, 2584):
            check(gx, ctx, b)
    check(gx, ctx, b)   # 10,946


def test_decreasing_lcp_run(gx, ctx):
    """A^k C: the LCP values k-1, k-2, ..., 1 follow each other, so the search to
    the left crosses more than two fold blocks."""
    _, _, B = tiles(gx)
    d, _ = check(gx, ctx, b"A" * (2 * B + 3) + b"C")
    assert d["raw"].num_internal == 2 * B + 2


def test_repeat_across_lcp_chunks(gx, ctx):
    _, C, _ = tiles(gx)
    rng = random.Random(5)
    rep = rand(rng, b"ACGT", 3 * C)
    s = rand(rng, b"ACGT", C + 5) + rep + b"G" + rand(rng, b"ACGT", 2 * C + 3) + rep + b"T" + rand(rng, b"ACGT", 7)
    d, _ = check(gx, ctx, s)
    assert d["raw"].max_string_depth >= 3 * C


def test_mutated_copies(gx, ctx):
    rng = random.Random(77)
    block = rand(rng, b"ACGT", 700)
    parts = [rand(rng, b"ACGT", 725)]
    for _ in range(3):
        m = bytearray(block)
        for p in rng.sample(range(700), 6):
            m[p] = rng.choice(b"ACGT")
        parts += [bytes(m), rand(rng, b"ACGT", 725)]
    s = b"".join(parts)
    assert len(s) == 5000
    d, _ = check(gx, ctx, s)
    assert d["raw"].max_string_depth >= 50


def test_lcp_budget_finishes_on_host(gx, ctx, monkeypatch):
    """Above GX_SUFFIX_LCP_BUDGET the device's suffix array is finished on the
    host (LCP, statistics): same results, and the LCP and fold kernels did not run."""
    T, C, _ = tiles(gx)
    s = b"A" * (3 * T)
    _, info = check(gx, ctx, s)
    assert info["lcp_ms"] > 0 and info["fold_ms"] > 0
    # the bound of this input is ceil(N / C) * (h / 8) with h >= N: one below it trips
    monkeypatch.setenv("GX_SUFFIX_LCP_BUDGET", str((len(s) // C) * (len(s) // 8) - 1))
    _, info = check(gx, ctx, s)
    assert info["lcp_ms"] == 0 and info["fold_ms"] == 0 and info["sort_passes"] >= 1, info
    check(gx, ctx, rand(random.Random(3), b"ACGT", 5000))


def test_rank_scan_chunk_edge(gx, ctx):
    """256 and 257 partials in the scan of the head flags: without the carry
    between chunks of suf_scan_part_kernel the ranks restart in the last tile."""
    T, W = scan_chunk(gx)
    for N in (W * T, W * T + 1):
        assert -(-N // T) == W + (N > W * T)
        check_definition(gx, ctx, np_rand(N, b"ACGT", N - 1))


@pytest.mark.parametrize("extra", [0, 1], ids=["tiles_T", "tiles_T_plus_1"])
def test_table_scan_chunk_edge(gx, ctx, extra):
    """T and T + 1 tiles: the [256][tiles] histogram table of a radix pass has
    256 T and 256 (T + 1) entries, 256 and 257 partials of its scan."""
    T, W = scan_chunk(gx)
    N = T * T + extra
    tiles_n = -(-N // T)
    assert tiles_n == T + extra and -(-256 * tiles_n // T) == W + extra
    check_definition(gx, ctx, np_rand(N, b"ACGT", N - 1))


@pytest.mark.parametrize("alpha, n", [(BYTES_219, None), (BYTES_219, 5000), (SIGN_EDGE, 5000)],
                         ids=["bytes219_T-1", "bytes219_5000", "7f80_5000"])
def test_full_byte_range(gx, ctx, alpha, n):
    """Every byte the ABI admits: round 0 keys with bit 63 set, radix digits up to 0xFF."""
    T, _, _ = tiles(gx)
    s = np_rand(len(alpha), alpha, T - 1 if n is None else n)
    check(gx, ctx, s)
    check_definition(gx, ctx, s)


def test_many_rounds_wide_ranks(gx, ctx):
    """digit_passes counts round 0 as well, whose keys are 8 text bytes and differ
    in every digit byte: round 0 gives exactly one pass per digit, whatever N.
    So a pass on rank bits 16-23 shows as a count of two or more in digits 2
    and 6 (the low and the high half of a rank pair), never as one.  The
    control is a short input, whose ranks fit two digit bytes; and here
    N < 2^24, so digits 3 and 7 stay at round 0's one."""
    _, small = check_definition(gx, ctx, np_rand(12, b"ACGT", 5000))
    assert small["doubling_rounds"] >= 2, small
    assert [small["digit_passes"][p] for p in (2, 3, 6, 7)] == [1, 1, 1, 1], small
    s = mutated_tandem_copies()
    assert 1 << 16 < len(s) + 1 == 196609 < 1 << 24
    d, info = check_definition(gx, ctx, s)
    assert info["doubling_rounds"] >= 7, info
    assert info["digit_passes"][2] >= 2 and info["digit_passes"][6] >= 2, info
    assert info["digit_passes"][3] == 1 and info["digit_passes"][7] == 1, info


def test_null_outputs(gx, ctx):
    """Any of bwt, sa, lcp may be NULL: the statistics and the other arrays do not change."""
    s = np_rand(11, b"ACGT", 5000)
    full, _ = check_definition(gx, ctx, s)
    stats = fold_stats(full["sa"], full["lcp"])
    for want in ((), ("sa",), ("lcp",), ("bwt",), WANT):
        d = gx.suffix_tree_stats(s, ctx=ctx, want=want)
        info = gx.suffix_info(ctx)
        assert info["sort_passes"] >= 1 and info["lcp_ms"] > 0 and info["fold_ms"] > 0, (want, info)
        assert raw_dict(d["raw"]) == stats, want
        assert sorted(k for k in d if k in WANT) == sorted(want)
        for k in want:
            assert np.array_equal(d[k], full[k]) if k != "bwt" else d[k] == full[k], (want, k)


def test_sizes_falling_and_rising(gx, ctx):
    """One context, sizes down and up again: the pooled table, scan and flag
    buffers are larger than the call needs and hold the previous call's data."""
    T, _, _ = tiles(gx)
    for k, n in enumerate((4 * T + 1, 65, 3 * T, 1, 4 * T + 1)):
        check_definition(gx, ctx, np_rand(100 + k, b"ACGT", n))


def test_empty_input_with_context(gx, ctx):
    d = gx.suffix_tree_stats(b"", ctx=ctx, want=WANT)
    assert d["bwt"] == b"$" and d["sa"].tolist() == [0] and d["lcp"].tolist() == [0]
    assert (d["raw"].num_leaves, d["raw"].num_internal, d["raw"].num_nodes) == (1, 0, 2)


def vectors(slow):
    out = []
    for v in load_vectors():
        big = v["n"] > 500000
        if big == slow:
            out.append(pytest.param(v, id=v["name"]))
    return out


def check_vector(gx, ctx, v):
    s = vector_text(v)
    d, _ = check(gx, ctx, s)
    for key in ("num_internal", "num_leaves", "num_nodes", "string_depth_sum", "max_string_depth",
                "longest_repeat_start"):
        assert getattr(d["raw"], key) == v[key][0], key
    if v.get("bwt"):
        assert d["bwt"] == read_bwt_file(v["bwt"])


@pytest.mark.parametrize("v", vectors(False))
def test_reference_vectors(gx, ctx, v):
    check_vector(gx, ctx, v)


@pytest.mark.slow
@pytest.mark.parametrize("v", vectors(True))
def test_reference_vectors_large(gx, ctx, v):
    check_vector(gx, ctx, v)


def test_mirror_on_device(gx, ctx):
    tree = gx.SuffixTree(os.path.join(ROOT, "tests", "golden", "alphabets", "banana.txt"), 10, ctx=ctx)
    tree.insert_string("BANANA", True, True)
    tree.insert_string("ABANANA", True, True)
    tree.compute_stats(0)
    assert gx.suffix_info(ctx)["doubling_rounds"] >= 1
    assert (tree.stats.num_internal, tree.stats.num_leaves, tree.stats.num_nodes) == (3, 7, 11)
    assert tree.stats.bwt == "ANNB$AA"
    assert tree.get_lcs(0, 1) == (0, 1, 6)


POISON_SCRIPT = r"""
import json, random, sys
sys.path.insert(0, sys.argv[1])
import gxamd as gx
ctx = gx.Context(0)
rng = random.Random(9)
a = bytes(rng.choice(b"ACGT") for _ in range(5000))
b = bytes(rng.choice(b"AC") for _ in range(4100))
out = []
for s in (a, a, b, a):
    r = gx.suffix_tree_stats(s, ctx=ctx, want=("bwt", "sa", "lcp"))
    h = gx.suffix_tree_stats(s, host=True, want=("bwt", "sa", "lcp"))
    out.append(bool((r["sa"] == h["sa"]).all() and (r["lcp"] == h["lcp"]).all() and r["bwt"] == h["bwt"]
                    and [getattr(r["raw"], k) for k, _ in r["raw"]._fields_]
                    == [getattr(h["raw"], k) for k, _ in h["raw"]._fields_]
                    and gx.suffix_info(ctx)["sort_passes"] > 0))
ctx.close()
print(json.dumps(out))
"""


def test_pool_poison_repeat_calls(tmp_path):
    """Calls in a row on one context with every pooled buffer filled with 0xA5
    before its new user: no buffer is read before it is written.  (The pool
    reads GX_POOL_POISON once per process, hence a process of its own.)"""
    script = tmp_path / "poison.py"
    script.write_text(POISON_SCRIPT)
    env = dict(os.environ, GX_POOL_POISON="1", GX_SUFFIX_HOST_BELOW="0")
    p = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "genomics-rs_amd")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout.strip().splitlines()[-1]) == [True, True, True, True]


def test_cli_brca2(gx, tmp_path):
    v = next(v for v in load_vectors() if v["name"] == "Human-BRCA2-cds")
    s = vector_text(v)
    out = tmp_path / "brca2_bwt.txt"
    alphabet = os.path.join(ROOT, "tests", "golden", "alphabets", "dna.txt")
    p = subprocess.run([CLI, "suffix-tree", "-f", os.path.join(GOLDEN, v["fasta"]), "-a", alphabet, "--suffix-links",
                        "--stats", "-o", str(out)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    assert out.read_bytes() == read_golden(os.path.join(GOLDEN, "suffix", v["bwt"]))
    h = gx.suffix_tree_stats(s, host=True)
    assert p.stdout == "\nStats: " + gx.format_suffix_stats(h["raw"], h["bwt"]) + "\n"
    assert "Time taken to build suffix tree:" in p.stderr
    # the default path: BWT_out/<name>_bwt.txt beside the working directory (main.rs:181-191)
    p = subprocess.run([CLI, "suffix-tree", "-f", os.path.join(GOLDEN, v["fasta"]), "--stats"], capture_output=True,
                       text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "BWT_out" / "Human-BRCA2-cds_bwt.txt").read_bytes() == out.read_bytes()


def test_cli_alphabet(tmp_path):
    """The alphabet is the file's characters and the reference's terminators (tree.rs:147)."""
    alphabet = os.path.join(ROOT, "tests", "golden", "alphabets", "dna.txt")
    for text, code in (("ACGT|AC~GT^A", 0), ("ACGNT", 101)):
        fasta = tmp_path / "a.fasta"
        fasta.write_text(">a\n" + text + "\n")
        p = subprocess.run([CLI, "suffix-tree", "-f", str(fasta), "-a", alphabet], capture_output=True, text=True,
                           timeout=300, cwd=str(tmp_path))
        assert p.returncode == code, p.stderr
        assert ("Character N not found in alphabet" in p.stderr) == (code == 101)
