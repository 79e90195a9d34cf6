"""GPU: compare mode (main.rs:216-379) on the kernels of gx_lcsub.hip --
gx_common_substring, gx_compare_pair, gx_compare_matrix and `gx-align
compare` -- against the host solver, the brute-force restatement of
tests/test_compare_host.py and tests/golden/compare_digests.json (host
solver, tests/golden/make_compare_digests.py).

Every case runs with GX_COMPARE_HOST_CELLS=0, so that each non-empty
sub-problem goes through the kernels; gx_compare_info confirms it.

The first half runs at the shipped segment height (1024 rows) on ASCII
letters.  The second half (from HEIGHTS on; DESIGN.md 16.4 lists what pins
what) varies what the first holds fixed:

  H          GX_COMPARE_SEG_H = 8, 9, 13, 64, 1000 (`*_by_height`,
             `test_long_runs_over_many_segments`, `test_run_ends_at_segment_
             boundary`) and 32768 (`test_element_fields_at_their_limits`):
             runs over up to 37 segments, segments that start off a multiple
             of 8 bytes, blocks and diagonals that end on a boundary, the
             16-bit fields of the tile element at 32768
  bytes      {0x25, 0xFF}, {0x7F, 0x80} and all four (`test_full_byte_range_*`)
  batches    gx_compare_batches: a level split by sub-problem count, by tile
             elements (`test_batches_split_*`), and the clamp of
             GX_COMPARE_CAND_CAP (`test_cand_cap_clamps`)

Their expected values are known from the construction (a planted block, a
string against itself) or come from the restatement; only inputs too long for
the restatement are held to the host solver.  None compares the kernels with
themselves alone."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import COMPARISON, CONFIG_SCORES, GOLDEN, ROOT
from test_compare_host import BYTE_ALPHABETS, byte_range_cases, periodic_pairs, ref_compare, ref_lcs, vectors

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "genomics-rs_amd", "gx-align")


@pytest.fixture(autouse=True)
def all_on_gpu(monkeypatch):
    monkeypatch.setenv("GX_COMPARE_HOST_CELLS", "0")
    monkeypatch.delenv("GX_COMPARE_CAND_CAP", raising=False)
    monkeypatch.delenv("GX_COMPARE_SEG_H", raising=False)


def on_gpu_only(gx, ctx):
    info = gx.compare_info(ctx)
    assert info["gpu_subproblems"] > 0 and info["host_subproblems"] == 0 and info["overflowed"] == 0, info
    return info


def digests():
    with open(os.path.join(GOLDEN, "compare_digests.json")) as f:
        return json.load(f)


def genomes(gx):
    cont = gx.SequenceContainer()
    for f in sorted(os.listdir(COMPARISON)):
        if f.endswith(".fasta"):
            cont.from_fasta(os.path.join(COMPARISON, f))
    return cont


def planted(rng, n, m, p, q, k, bg_a=b"AC", bg_b=b"GT", block=b"ACGT"):
    """a over {A, C}, b over {G, T}, and one common block of k random ACGT
    bytes at a[p:], b[q:] whose ends differ from the background on neither
    side: the only common substrings lie inside the block."""
    assert 0 <= p and p + k <= n and 0 <= q and q + k <= m, (n, m, p, q, k)
    a = bytearray(rng.choice(bg_a) for _ in range(n))
    b = bytearray(rng.choice(bg_b) for _ in range(m))
    blk = bytes(rng.choice(block) for _ in range(k))
    a[p:p + k] = blk
    b[q:q + k] = blk
    return bytes(a), bytes(b)


def tie_cases():
    rng = random.Random(23)
    two = [tuple(bytes(rng.choice(b"AB") for _ in range(300)) for _ in range(2)) for _ in range(3)]
    return two + periodic_pairs() + [(b"AB" * 60, b"AB" * 41 + b"A")]


def test_reference_fixtures(gx, ctx):
    for name, a, b, want, small in vectors():
        got = gx.common_substring(a, b, ctx=ctx)
        on_gpu_only(gx, ctx)
        if want is not None:
            assert got == want, name
        if small:
            assert got == ref_lcs(a, b), name


def test_edge_lengths(gx, ctx):
    H = gx.compare_segment_height()
    lens = [1, 63, 64, 65, 127, 128, 129, H - 1, H, H + 1, 2 * H + 3]
    rng = random.Random(7)
    for n in lens:
        for m in lens:
            a = bytearray(rng.choice(b"ACGT") for _ in range(n))
            b = bytearray(rng.choice(b"ACGT") for _ in range(m))
            k = min(n, m, 24)
            p, q = rng.randrange(n - k + 1), rng.randrange(m - k + 1)
            b[q:q + k] = a[p:p + k]
            a, b = bytes(a), bytes(b)
            assert gx.common_substring(a, b, ctx=ctx) == gx.common_substring_host(a, b), (n, m, p, q)
            if min(n, m) > 1:
                on_gpu_only(gx, ctx)
            else:
                # one byte against a long string: L = 1 with hundreds of equal starts, more than the
                # candidate buffer holds (the overflow case); nothing else may reach the host solver
                info = gx.compare_info(ctx)
                assert info["gpu_subproblems"] == 1 and info["host_subproblems"] == info["overflowed"], info


def test_runs_across_segments(gx, ctx):
    H = gx.compare_segment_height()
    rng = random.Random(8)
    n = 2 * H + 3
    a = bytes(rng.choice(b"ACGT") for _ in range(n))
    assert gx.common_substring(a, a, ctx=ctx) == (0, 0, n)
    on_gpu_only(gx, ctx)
    for x in (b"T", bytes(rng.choice(b"ACGT") for _ in range(H + 5))):
        assert gx.common_substring(a, x + a, ctx=ctx) == (0, len(x), n), len(x)
        assert gx.common_substring(x + a, a, ctx=ctx) == (len(x), 0, n), len(x)
    # a block that crosses a segment boundary by one byte, on either side
    # (first row before the boundary, last row after it, both, and blocks longer than a segment)
    for p, k in ((H - 1, 40), (H - 39, 40), (H - 1, 2), (2 * H - 1, 2 + H // 2), (H - 1, H + 2)):
        for q in (5, H + 7):
            a, b = planted(rng, 3 * H + 1, 2 * H + 50, p, q, k)
            got = gx.common_substring(a, b, ctx=ctx)
            on_gpu_only(gx, ctx)
            assert got == gx.common_substring_host(a, b), (p, q, k)
            if k >= 40:   # (a shorter block also matches the background by chance)
                assert got == (p, q, k), (p, q, k)


def test_runs_at_wave_and_block_edges(gx, ctx):
    """A block on the diagonals on either side of a 64-lane wave boundary and
    of a 256-lane workgroup boundary (diagonal index q - p + n - 1)."""
    rng = random.Random(9)
    n, m, k = 400, 500, 30
    for diag in (63, 64, 255, 256, 511, 512):
        p = max(0, n - 1 - diag) + 4
        q = diag - (n - 1) + p
        a, b = planted(rng, n, m, p, q, k)
        assert gx.common_substring(a, b, ctx=ctx) == (p, q, k), diag
        on_gpu_only(gx, ctx)


def test_equal_blocks_in_neighbouring_waves(gx, ctx):
    """The same block twice in each string, so that equal runs lie on
    diagonals 63 and 64 (two waves) and on two more: the suffix order decides."""
    rng = random.Random(10)
    n, m, k = 460, 500, 20
    a = bytearray(rng.choice(b"AC") for _ in range(n))
    b = bytearray(rng.choice(b"GT") for _ in range(m))
    blk = bytes(rng.choice(b"ACGT") for _ in range(k))
    for p, q in ((400, 4), (430, 35)):   # q - p + n - 1 = 63, 64
        a[p:p + k] = blk
        b[q:q + k] = blk
    a, b = bytes(a), bytes(b)
    got = gx.common_substring(a, b, ctx=ctx)
    on_gpu_only(gx, ctx)
    assert got == gx.common_substring_host(a, b) == ref_lcs(a, b)
    assert got[2] >= k


def test_ties(gx, ctx):
    for a, b in tie_cases():
        want = ref_compare(a, b)
        assert gx.compare_pair(a, b, ctx=ctx) == want, (a, b)
        on_gpu_only(gx, ctx)
        assert gx.common_substring(a, b, ctx=ctx) == ref_lcs(a, b), (a, b)


def test_candidate_overflow_goes_to_host(gx, ctx, monkeypatch):
    monkeypatch.setenv("GX_COMPARE_CAND_CAP", "1")
    overflowed = 0
    for a, b in tie_cases():
        assert gx.compare_pair(a, b, ctx=ctx) == ref_compare(a, b), (a, b)
        info = gx.compare_info(ctx)
        assert info["gpu_subproblems"] > 0 and info["host_subproblems"] == info["overflowed"], info
        overflowed += info["overflowed"]
    assert overflowed > 0


def mutated_copies(count, seed=12):
    """Prefixes of 200..500 bytes of one random ACGT base, 3..40 point changes each."""
    rng = random.Random(seed)
    base = bytes(rng.choice(b"ACGT") for _ in range(500))
    seqs = []
    for _ in range(count):
        s = bytearray(base[:rng.randint(200, 500)])
        for _ in range(rng.randint(3, 40)):
            s[rng.randrange(len(s))] = rng.choice(b"ACGT")
        seqs.append(bytes(s))
    return seqs


def test_matrix_levels_equal_pairs(gx, ctx):
    seqs = mutated_copies(6)
    mat = gx.compare_matrix(seqs, ctx=ctx)
    info = on_gpu_only(gx, ctx)
    assert info["levels"] > 1
    for j in range(6):
        for i in range(6):
            if i > j:
                assert not mat[j, i].any()
                continue
            score, first, _ = gx.compare_pair(seqs[i], seqs[j], ctx=ctx)
            assert [int(x) for x in mat[j, i]] == [score, len(seqs[i]), len(seqs[j]), first], (i, j)
            if i == j:
                assert score == len(seqs[i])
    assert (mat == gx.compare_matrix(seqs, host=True)).all()


def test_synthetic_pairs_match_digest(gx, ctx):
    for c in digests()["synthetic"]:
        got = gx.compare_pair(c["a"].encode(), c["b"].encode(), ctx=ctx)
        assert got == (c["score"], c["first_lcs"], c["calls"])
        on_gpu_only(gx, ctx)


def test_genome_matrix_matches_digest(gx, ctx, monkeypatch):
    """All 132,165 non-empty sub-problems of the 55 recursions on the kernels.  A few tiny ones hold up
    to 481 equal candidate starts (profiles/compare_candidates.json), above the shipped cap that is
    sized for the sub-problems the default configuration sends to the GPU: the cap is raised here so
    that none falls back to the host solver."""
    monkeypatch.setenv("GX_COMPARE_CAND_CAP", "1024")
    g = digests()
    cont = genomes(gx)
    assert [s.name for s in cont.sequences] == g["names"]
    mat = gx.compare_matrix([s.sequence.encode() for s in cont.sequences], ctx=ctx)
    on_gpu_only(gx, ctx)
    want = np.zeros_like(mat)
    for c in g["matrix"]:
        want[c["j"], c["i"]] = (c["score"], g["lengths"][c["i"]], g["lengths"][c["j"]], c["first_lcs"])
    assert (mat == want).all()


def test_genome_matrix_default_configuration(gx, ctx, monkeypatch):
    """The shipped configuration (no environment knob set): only sub-problems
    whose candidates overflow the shipped cap reach the host solver."""
    monkeypatch.delenv("GX_COMPARE_HOST_CELLS")
    g = digests()
    mat = gx.compare_matrix([s.sequence.encode() for s in genomes(gx).sequences], ctx=ctx)
    info = gx.compare_info(ctx)
    assert info["gpu_subproblems"] > 0 and info["host_subproblems"] == info["overflowed"], info
    for c in g["matrix"]:
        assert (int(mat[c["j"], c["i"], 0]), int(mat[c["j"], c["i"], 3])) == (c["score"], c["first_lcs"]), c


def test_genome_matrix_split_between_host_and_gpu(gx, ctx, monkeypatch):
    """Sub-problems below 65,536 cells, and everything under them, on the host
    solver; the rest on the kernels (none of those overflows the shipped cap)."""
    monkeypatch.setenv("GX_COMPARE_HOST_CELLS", "65536")
    g = digests()
    mat = gx.compare_matrix([s.sequence.encode() for s in genomes(gx).sequences], ctx=ctx)
    info = gx.compare_info(ctx)
    assert info["gpu_subproblems"] > 0 and info["host_subproblems"] > 0 and info["overflowed"] == 0, info
    for c in g["matrix"]:
        assert (int(mat[c["j"], c["i"], 0]), int(mat[c["j"], c["i"], 3])) == (c["score"], c["first_lcs"]), c


def test_cli_compare_tsv(gx, tmp_path):
    g = digests()
    K = len(g["names"])
    score = [[0] * K for _ in range(K)]
    first = [[0] * K for _ in range(K)]
    for c in g["matrix"]:
        score[c["j"]][c["i"]] = c["score"]
        first[c["j"]][c["i"]] = c["first_lcs"]

    def block(rows, corner):   # main.rs:337-378: header row first, a trailing tab per row, the row index first
        head = corner + "\t" + "".join(f"{i}\t" for i in range(K)) + "\n"
        return head + "".join(f"{j}\t" + "".join(f"{v}\t" for v in rows[j]) + "\n" for j in range(K))

    tsv = tmp_path / "similarity_matrix.tsv"
    p = subprocess.run([CLI, "compare", "-d", COMPARISON, "-o", str(tsv)], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    assert tsv.read_text() == block(score, "")
    assert p.stdout == "Similarity TSV:\n" + block(score, " ") + "\nLCS Length TSV:\n" + block(first, " ")
    assert "[FindPath] Time taken to compare:" in p.stderr


def test_align_after_compare_on_one_context(gx, ctx, oracle):
    from test_gpu_parity import assert_same
    rng = random.Random(13)
    a = bytes(rng.choice(b"ACGT") for _ in range(700))
    b = a[:300] + bytes(rng.choice(b"ACGT") for _ in range(150)) + a[350:]
    gx.compare_pair(a, b, ctx=ctx)
    on_gpu_only(gx, ctx)
    for loc in (False, True):
        steps, r = gx.align_raw(a, b, gx.Scores(*CONFIG_SCORES), loc, ctx=ctx)
        assert_same(steps, r, oracle.align(a, b, CONFIG_SCORES, is_local=loc), loc)
    assert gx.compare_pair(a, b, ctx=ctx) == gx.compare_pair(a, b, host=True)


# ---------------------------------------------------------------------------
# The tile monoid at every segment height and byte.  Expected
# values come from the construction (planted blocks, a against itself), from
# the restatement (ref_lcs / ref_compare), or, for inputs too long for it, from
# the host solver, which tests/test_compare_host.py holds to the restatement.

# 8 is the lowest height (a segment is one 8-byte load), 9 and 13 start every
# segment but the first off a multiple of 8, 64 is the wave width, 1000 a
# height near the default whose segments are no multiple of 8 rows apart.
HEIGHTS = (8, 9, 13, 64, 1000)


@pytest.fixture(params=HEIGHTS)
def H(request, gx, monkeypatch, all_on_gpu):
    monkeypatch.setenv("GX_COMPARE_SEG_H", str(request.param))
    assert gx.compare_segment_height() == request.param
    return request.param


def acgt(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def expect_planted(gx, ctx, rng, n, m, p, q, k):
    """One planted block of k >= 40 random bytes: the answer is (p, q, k) by construction."""
    assert k >= 40
    a, b = planted(rng, n, m, p, q, k)
    got = gx.common_substring(a, b, ctx=ctx)
    on_gpu_only(gx, ctx)
    assert got == (p, q, k), (n, m, p, q, k)


_tie_refs = []


def tie_refs():
    """[(a, b, ref_lcs, ref_compare)] of tie_cases(), computed once."""
    if not _tie_refs:
        _tie_refs.extend((a, b, ref_lcs(a, b), ref_compare(a, b)) for a, b in tie_cases())
    return _tie_refs


def test_edge_lengths_by_height(gx, ctx, H):
    """test_edge_lengths with the lengths around a segment of H rows, up to six segments."""
    lens = [1, 7, 8, 9, H - 1, H, H + 1, 2 * H + 3] + ([5 * H + 1] if H != 1000 else [])
    lens = list(dict.fromkeys(lens))
    rng = random.Random(70 + H)
    for n in lens:
        for m in lens:
            a = bytearray(rng.choice(b"ACGT") for _ in range(n))
            b = bytearray(rng.choice(b"ACGT") for _ in range(m))
            k = min(n, m, 24)
            p, q = rng.randrange(n - k + 1), rng.randrange(m - k + 1)
            b[q:q + k] = a[p:p + k]
            a, b = bytes(a), bytes(b)
            want = ref_lcs(a, b) if n * m <= 40_000 else gx.common_substring_host(a, b)
            assert gx.common_substring(a, b, ctx=ctx) == want, (n, m, p, q)
            if min(n, m) > 1:
                on_gpu_only(gx, ctx)
            else:
                # (as in test_edge_lengths: one byte against a long string overflows the candidate buffer)
                info = gx.compare_info(ctx)
                assert info["gpu_subproblems"] == 1 and info["host_subproblems"] == info["overflowed"], info


def test_long_runs_over_many_segments(gx, ctx, H):
    """Runs through up to 37 all-equal tiles (the combine kernel's `run += head`,
    carry[] far from the run's start) and planted blocks that begin on either
    side of a boundary and cross 2 or 11 of them.  At H = 1000 the strings
    are 5 / 6 / 3 segments long in place of 37 / 40 / 12 (at most 4e7 cells),
    and the longer block is the longest that fits b behind q = H + 7."""
    ma, mn, mm = (5, 6, 3) if H == 1000 else (37, 40, 12)
    rng = random.Random(100 + H)
    n = ma * H + 5
    a = acgt(rng, n)
    assert gx.common_substring(a, a, ctx=ctx) == (0, 0, n)
    info = on_gpu_only(gx, ctx)
    assert info["levels"] == 1 and info["batches"] == 1, info
    for lx in (1, H - 1, H, H + 3):
        x = acgt(rng, lx)
        assert gx.common_substring(a, x + a, ctx=ctx) == (0, lx, n), lx
        on_gpu_only(gx, ctx)
        assert gx.common_substring(x + a, a, ctx=ctx) == (lx, 0, n), lx
        on_gpu_only(gx, ctx)
    n, m = mn * H, mm * H + 50
    for p in (H - 1, H, H + 1, 3 * H - 1):
        for k in sorted({max(40, 2 * H + 1), max(40, min(11 * H, m - (H + 7)))}):
            for q in (5, H + 7):
                expect_planted(gx, ctx, rng, n, m, p, q, k)


def test_run_ends_at_segment_boundary(gx, ctx, H):
    """A run ends at an unequal byte or where the diagonal leaves the grid,
    and a segment boundary at the same row must neither end it twice nor lose it."""
    rng = random.Random(200 + H)
    n, m = 6 * H + 120, 4 * H + 120
    nb = -(-n // H) * H   # a whole number of segments
    for k in (40, 41, 2 * H + 43):
        c0 = -(-(k + 1) // H)
        for c in (c0, c0 + 1):
            p = c * H - k   # the block's last row is a segment's last row
            for q in (5, H + 7, m - k):   # (m - k: b ends there too, m - d == c * H)
                expect_planted(gx, ctx, rng, n, m, p, q, k)
        for c in (1, 2):   # the block's first row is a segment's first row
            for q in (5, H + 7):
                expect_planted(gx, ctx, rng, n, m, c * H, q, k)
        # the diagonal ends with a's last segment: the block at the end of a, and at the end of both
        for q in (5, m - k):
            expect_planted(gx, ctx, rng, nb, m, nb - k, q, k)


def test_ties_by_height(gx, ctx, H, monkeypatch):
    monkeypatch.setenv("GX_COMPARE_CAND_CAP", "65536")
    for a, b, want_lcs, want_cmp in tie_refs():
        assert gx.compare_pair(a, b, ctx=ctx) == want_cmp, (a, b)
        on_gpu_only(gx, ctx)
        assert gx.common_substring(a, b, ctx=ctx) == want_lcs, (a, b)
        on_gpu_only(gx, ctx)


@pytest.mark.parametrize("alphabet", BYTE_ALPHABETS, ids=lambda s: s.hex())
def test_full_byte_range_on_kernels(gx, ctx, alphabet, monkeypatch):
    """Bytes with the top bit set in the run kernel's byte lanes and in the
    host's tie rule behind the kernels, against the restatement."""
    monkeypatch.setenv("GX_COMPARE_CAND_CAP", "65536")
    for a, b, want_lcs, want_cmp in byte_range_cases(alphabet):
        assert gx.common_substring(a, b, ctx=ctx) == want_lcs, (a, b)
        on_gpu_only(gx, ctx)
        assert gx.compare_pair(a, b, ctx=ctx) == want_cmp, (a, b)
        on_gpu_only(gx, ctx)


def test_full_byte_range_planted(gx, ctx):
    """test_runs_at_wave_and_block_edges with a over {0x80, 0xFE}, b over
    {0x25, 0x7F} and the block over all four."""
    rng = random.Random(19)
    n, m, k = 400, 500, 30
    for diag in (63, 64, 255, 256, 511, 512):
        p = max(0, n - 1 - diag) + 4
        q = diag - (n - 1) + p
        a, b = planted(rng, n, m, p, q, k, bg_a=b"\x80\xfe", bg_b=b"\x25\x7f", block=b"\x25\x7f\x80\xfe")
        assert gx.common_substring(a, b, ctx=ctx) == (p, q, k) == ref_lcs(a, b), diag
        on_gpu_only(gx, ctx)


def test_element_fields_at_their_limits(gx, ctx, monkeypatch):
    """H = 32768, the largest height: head and tail fill their 16 bits
    (32768 in an all-equal tile), best comes within two of it."""
    H = 32768
    monkeypatch.setenv("GX_COMPARE_SEG_H", str(H))
    assert gx.compare_segment_height() == H
    rng = random.Random(41)
    n = 2 * H + 3
    a = acgt(rng, n)
    for s, t, want in ((a, a, (0, 0, n)), (a, b"T" + a, (0, 1, n)), (b"T" + a, a, (1, 0, n))):
        assert gx.common_substring(s, t, ctx=ctx) == want
        on_gpu_only(gx, ctx)
    for p, k in ((H + 1, H - 2),    # best = H - 2 strictly inside a tile
                 (1, H - 1),        # a break on the segment's first row, then H - 1 rows into the boundary
                 (H, H - 1),        # a head of H - 1 and a break on the segment's last row
                 (H + 1, H - 1),    # a tail of H - 1 into the boundary
                 (H - 1, H + 2)):   # tail 1, an all-equal tile, head 1
        expect_planted(gx, ctx, rng, 3 * H + 1, H + 50, p, 7, k)


def test_batches_split_by_subproblem_count(gx, ctx, monkeypatch):
    """The candidate buffer holds 4 Mi slots, so cap 65536 admits 64
    sub-problems a batch; the 45 pairs of nine sequences open more than that
    on later levels (up to 90 on the second)."""
    monkeypatch.setenv("GX_COMPARE_CAND_CAP", "65536")
    seqs = mutated_copies(9)
    mat = gx.compare_matrix(seqs, ctx=ctx)
    info = on_gpu_only(gx, ctx)
    assert info["batches"] > info["levels"] > 1, info
    assert (mat == gx.compare_matrix(seqs, host=True)).all()
    for j in range(9):
        for i in range(j + 1):
            score, first, _ = gx.compare_pair(seqs[i], seqs[j], ctx=ctx)
            assert [int(x) for x in mat[j, i]] == [score, len(seqs[i]), len(seqs[j]), first], (i, j)
            info = on_gpu_only(gx, ctx)
            assert info["batches"] == info["levels"], info   # (one pair never opens 64 sub-problems on a level here)


def test_cand_cap_clamps(gx, ctx, monkeypatch):
    """GX_COMPARE_CAND_CAP is clamped to [1, 65536]: above it the batches
    are those of 65536 (64 sub-problems each), 0 behaves as 1."""
    seqs = mutated_copies(9)
    want = gx.compare_matrix(seqs, host=True)
    seen = {}
    for cap in ("65536", "65537", str(10**12), "1", "0"):
        monkeypatch.setenv("GX_COMPARE_CAND_CAP", cap)
        assert (gx.compare_matrix(seqs, ctx=ctx) == want).all(), cap
        info = gx.compare_info(ctx)
        assert info["gpu_subproblems"] > 0 and info["host_subproblems"] == info["overflowed"], (cap, info)
        seen[cap] = {k: info[k] for k in ("gpu_subproblems", "host_subproblems", "overflowed", "levels", "batches")}
    assert seen["65537"] == seen[str(10**12)] == seen["65536"] and seen["65536"]["overflowed"] == 0, seen
    assert seen["0"] == seen["1"] and seen["1"]["overflowed"] > 0, seen


def test_batches_split_by_elements(gx, ctx, monkeypatch):
    """The smallest shape past the 192 Mi tile elements of one batch: 28
    pairs of 6,000 x 6,000 at H = 8 are 28 x 750 segments x 11,999 diagonals
    = 251,979,000 elements, so the first level takes two batches (22 pairs,
    197,983,500 elements, then 6)."""
    monkeypatch.setenv("GX_COMPARE_SEG_H", "8")
    monkeypatch.setenv("GX_COMPARE_CAND_CAP", "1024")
    n, per_pair = 6000, (6000 // 8) * (2 * 6000 - 1)
    assert 22 * per_pair <= 192 << 20 < 23 * per_pair < 28 * per_pair
    rng = random.Random(31)
    base = acgt(rng, n)
    seqs = []
    for _ in range(7):
        s = bytearray(base)
        for _ in range(rng.randint(30, 200)):
            s[rng.randrange(n)] = rng.choice(b"ACGT")
        seqs.append(bytes(s))
    mat = gx.compare_matrix(seqs, ctx=ctx)
    info = on_gpu_only(gx, ctx)
    assert info["batches"] >= info["levels"] + 1, info
    assert (mat == gx.compare_matrix(seqs, host=True)).all()
