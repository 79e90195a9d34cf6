"""Matching statistics and maximal exact matches on the GPU:
gx_suffix_index_match_stats and gx_suffix_index_mems on a device-resident
index, every result checked against the brute force of tests/match_check.py
and compared field by field with the host index, at the shapes where
gx_match.hip and the kernels it borrows can go wrong (the content cases of
tests/test_match_host.py):

  word edges    min_len and max_len in {1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65},
                planted matches of L - 1, L and L + 1 bytes starting and ending
                at every alignment mod 8 on both sides, three alphabets
  ends          matches at text 0, query 0, n and m_c; query = text, longer
                than the text, shorter than min_len, empty; tiny texts from
                either suffix-array solver
  boundaries    queries cut from consecutive text, lengths around 8 and 64
  maximality    left-extendable pairs, one diagonal, crossing diagonals, A^5000
                in closed form, (ACGT)^1250
  batch shapes  positions around the wave and the workgroup, candidate and kept
                totals around the scan tile, one position with thousands of
                candidates, counts only, GX_ECAP, budget, the 64-bit total,
                alternating searches, two indexes on one context
  cross-checks  compare mode's longest common substring, the exact search's
                intervals, Covid and MERS genomes, the CLI

Every device call must show in match_info the candidates of the hits' sum, as
many kept pairs as MEMs, timers above zero for exactly the phases that ran, and
word steps inside the bounds of DESIGN.md 21.2."""
import os
import subprocess

import numpy as np
import pytest

from conftest import COMPARISON, ROOT, read_fasta_records
from match_check import (check_mems, check_stats, emit_word_bound, interval_word_bound, runs, same_mems, same_stats,
                         seed_word_bound)
from test_match_host import (CASES, IDS, budget_case, ecap_protocol, error_table, mutate, unary_counts, wrap_case)
from test_suffix_host import np_rand

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "genomics-rs_amd", "gx-align")


def lengths_of(queries):
    if isinstance(queries, tuple):
        return np.diff(np.asarray(queries[1], np.int64))
    return np.array([len(q) for q in queries], np.int64)


def windows_of(queries, W):
    """min(W, m_c - j) for every position."""
    ls = lengths_of(queries)
    return np.concatenate([np.minimum(W, np.arange(m, 0, -1)) for m in ls] + [np.zeros(0, np.int64)])


def device_stats(gx, ctx, idx, queries, W):
    """The call, with what every case asserts of match_info."""
    r = idx.matching_stats(queries, max_len=W)
    info = gx.match_info(ctx)
    bound = interval_word_bound(idx.n + 1, windows_of(queries, W))
    print(f"stats nq {len(lengths_of(queries))} max_len {W}: {info}, bound {bound}")
    assert info["candidates"] == 0 and info["kept"] == 0 and info["seed_ms"] == 0 and info["emit_ms"] == 0, info
    assert info["word_compares"] <= bound, (info, bound)
    assert (info["stats_ms"] > 0) == (int(r["offsets"][-1]) > 0), info
    return r


def device_mems(gx, ctx, idx, queries, L):
    """The counts-only call and the full call (two calls when there is a MEM: the counts, then the exact
    capacity), with what every case asserts of match_info.  The word counter is deterministic and the
    counts-only call runs exactly the seed stages of the full one, so the difference of the two counters is the
    emit kernel's alone: each term is held to its own bound of DESIGN.md 21.2."""
    ls = lengths_of(queries)
    npos = int(ls.sum())
    counts = idx.mems(queries, L, max_mems=0)
    seeds = gx.match_info(ctx)
    r = idx.mems(queries, L)
    info = gx.match_info(ctx)
    total = int(r["mem_offsets"][-1])
    emitted = total > 0                            # (without a MEM the second call is not made)
    seed_bound, emit_bound = seed_word_bound(idx.n + 1, ls, L), emit_word_bound(r["length"], L)
    print(f"mems nq {len(ls)} min_len {L}: counts only {seeds}, full {info}, bounds {seed_bound} + {emit_bound}")
    for i in (seeds, info):
        assert i["candidates"] == int(r["candidates"].sum()) and i["kept"] == total, i
        assert i["stats_ms"] == 0 and (i["seed_ms"] > 0) == (npos > 0), i
    assert seeds["emit_ms"] == 0 and (info["emit_ms"] > 0) == emitted, (seeds, info)
    assert seeds["word_compares"] <= seed_bound, (seeds, seed_bound)
    assert 0 <= info["word_compares"] - seeds["word_compares"] <= emit_bound, (seeds, info, emit_bound)
    assert np.array_equal(counts["mem_offsets"], r["mem_offsets"])
    assert np.array_equal(counts["candidates"], r["candidates"]) and len(counts["qpos"]) == 0
    return r


class Text:
    """A text with its host index and its device index."""

    def __init__(self, gx, ctx, s: bytes):
        self.gx, self.ctx, self.s = gx, ctx, s
        self.host = gx.SuffixIndex(s, host=True)
        self.dev = gx.SuffixIndex(s, ctx=ctx)
        self.sa = self.dev.sa()
        assert np.array_equal(self.sa, self.host.sa())

    def check(self, queries, min_lens, max_lens):
        for W in max_lens:
            r = device_stats(self.gx, self.ctx, self.dev, queries, W)
            check_stats(self.s, queries, W, r, self.sa)
            same_stats(r, self.host.matching_stats(queries, max_len=W))
        for L in min_lens:
            r = device_mems(self.gx, self.ctx, self.dev, queries, L)
            check_mems(self.s, queries, L, r)
            same_mems(r, self.host.mems(queries, L))

    def close(self):
        self.dev.close()
        self.host.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_content(gx, ctx, case):
    _, s, queries, min_lens, max_lens = case
    t = Text(gx, ctx, s)
    t.check(queries, min_lens, max_lens)
    t.close()


@pytest.mark.parametrize("host_below", ["0", None], ids=["device_array", "host_array"])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9])
def test_tiny_texts(gx, ctx, monkeypatch, n, host_below):
    """Tiny texts reach the kernels whichever solver built the array."""
    if host_below is not None:
        monkeypatch.setenv("GX_SUFFIX_HOST_BELOW", host_below)
    s = np_rand(n, b"AC", n)
    t = Text(gx, ctx, s)
    t.check([s, s + s, b"A", b"", b"C" * 9, s[1:], b"N" + s, s + b"N", b"A" * 17], (1, 2, 9), (1, 8, 100))
    t.check([], (1,), (1,))          # the empty batch
    t.check([b"", b""], (1,), (1,))
    t.close()


def test_unary_closed_form(gx, ctx):
    s = b"A" * 5000
    t = Text(gx, ctx, s)
    r = unary_counts(t.dev)
    same_mems(r, t.host.mems([b"A" * 20, b"A" * 19 + b"C", b"C" + b"A" * 19], 5))
    assert gx.match_info(ctx)["kept"] == 3 * 4996 + 15 + 14 + 14
    t.check([b"A" * 20, b"A" * 19 + b"C", b"C" + b"A" * 19], (5,), (20,))
    t.close()


def test_refusals_leave_context_working(gx, ctx, monkeypatch):
    """The error table, GX_ECAP, the budget and the 64-bit candidate total on the device; after each the
    context and the index go on working (every helper ends with a checked call)."""
    t = Text(gx, ctx, b"BANANA")
    error_table(gx, t.dev)
    ecap_protocol(gx, t.dev)
    info = gx.match_info(ctx)
    assert info["kept"] == 4 and info["seed_ms"] > 0 and info["emit_ms"] == 0, info   # (the last call was refused: GX_ECAP)
    t.close()
    s = b"A" * 300 + b"C" * 300
    t = Text(gx, ctx, s)
    r = budget_case(gx, t.dev, s, monkeypatch)
    same_mems(r, t.host.mems([b"A" * 10, b"C" * 10 + b"A", b"G" * 5], 4))
    t.close()
    t = Text(gx, ctx, b"A" * 5000)
    wrap_case(gx, t.dev, monkeypatch)
    info = gx.match_info(ctx)
    assert info["candidates"] == 4998 and info["kept"] == 4998, info
    t.check([b"AAAC", b"CAAA"], (3,), (4,))
    t.close()


def test_alternating_calls_and_two_indexes(gx, ctx):
    """Matching calls between the three searches on one context, and two indexes taking turns: every call's
    pooled buffers and its match_info are its own."""
    s1, s2 = np_rand(2140, b"ACGT", 1200), np_rand(2141, b"ACGT", 900)
    a, b = Text(gx, ctx, s1), Text(gx, ctx, s2)
    qa = [mutate(s1[100:400], 23, b"ACGT"), s2[50:120]]
    qb = [mutate(s2[300:700], 31, b"ACGT"), s1[5:60], b""]
    pats = [s1[10:40], s2[10:40], s1[700:730]]
    for rnd in range(2):
        a.check(qa, (8,), (40,))
        ra = a.dev.search(pats, max_hits=4)
        b.check(qb, (8,), (40,))
        assert np.array_equal(ra["count"], a.host.search(pats, max_hits=4)["count"])
        rb = b.dev.search_approx(pats, 1, max_hits=4)
        a.check(qb, (12,), (12,))
        assert np.array_equal(rb["count"], b.host.search_approx(pats, 1, max_hits=4)["count"])
        re_ = a.dev.search_edit(pats, 1, max_hits=4)
        b.check(qa, (5,), (7,))
        assert np.array_equal(re_["count"], a.host.search_edit(pats, 1, max_hits=4)["count"])
    a.close()
    b.close()


def genome(name: str) -> bytes:
    s = read_fasta_records(os.path.join(COMPARISON, name + ".fasta"))[0][1]
    assert min(s) > 0x24
    return s


@pytest.mark.parametrize("text,query", [("MERS_2012_KF600620", "Covid_Wuhan"), ("Covid_Wuhan", "SARS_2003_GU553363"),
                                        ("Covid_USA-CA4", "Covid_Wuhan")])
def test_longest_match_is_compare_modes_lcs(gx, ctx, text, query):
    """max(len) of the matching statistics at a max_len above both lengths is the length of compare mode's
    longest common substring, and a position that reaches it sits where compare mode found it or at an
    equally long match."""
    s, q = genome(text), genome(query)
    dev = gx.SuffixIndex(s, ctx=ctx)
    r = device_stats(gx, ctx, dev, [q], 1 << 20)
    p1, p2, k = gx.common_substring(s, q, ctx=ctx)
    assert int(r["len"].max()) == k
    assert int(r["len"][p2]) == k and s[int(r["pos"][p2]):int(r["pos"][p2]) + k] == q[p2:p2 + k]
    dev.close()


def test_stats_against_search(gx, ctx):
    """Where the whole window occurs, lo and count are the exact search's of that window; len is its
    prefix_len everywhere."""
    s = np_rand(2130, b"ACGT", 1500)
    dev = gx.SuffixIndex(s, ctx=ctx)
    q = mutate(s[200:500], 37, b"ACGT")
    for W in (5, 12, 300):
        r = device_stats(gx, ctx, dev, [q], W)
        wins = [q[j:j + W] for j in range(len(q))]
        h = dev.search(wins)
        assert np.array_equal(r["len"], h["prefix_len"])
        whole = r["len"] == np.array([len(w) for w in wins])
        assert whole.any() and np.array_equal(r["lo"][whole], h["lo"][whole])
        assert np.array_equal(r["count"][whole], h["count"][whole])
    dev.close()


def common_prefix(a: bytes, b: bytes) -> int:
    k, m = 0, min(len(a), len(b))
    while k < m and a[k] == b[k]:
        k += 1
    return k


@pytest.mark.parametrize("text", ["Covid_USA-CA4", "MERS_2014_KY581694"])
def test_covid_genomes_and_cli(gx, ctx, tmp_path, text):
    """Covid_Wuhan as the query at min_len 20: the device equals the host index in full; the MEMs of the first
    300 query positions are the brute force's pairs on a query slice that reaches 20 bytes past them (the
    lengths by direct comparison); the CLI's file is the Python result line by line."""
    tpath, qpath = os.path.join(COMPARISON, text + ".fasta"), os.path.join(COMPARISON, "Covid_Wuhan.fasta")
    s, q = genome(text), genome("Covid_Wuhan")
    dev, host = gx.SuffixIndex(s, ctx=ctx), gx.SuffixIndex(s, host=True)
    r = device_mems(gx, ctx, dev, [q], 20)
    same_mems(r, host.mems([q], 20))
    R, leftmax = runs(s, q[:320])
    jj, ii = np.nonzero(((R >= 20) & leftmax).T[:300])
    want = [(int(j), int(i), common_prefix(s[i:], q[j:])) for j, i in zip(jj, ii)]
    k = int(np.searchsorted(r["qpos"], 300))
    assert list(zip(r["qpos"][:k].tolist(), r["tpos"][:k].tolist(), r["length"][:k].tolist())) == want
    if text.startswith("Covid"):
        assert want and r["length"].max() > 1000
    dev.close()
    host.close()
    fa = tmp_path / "queries.fasta"
    fa.write_bytes(b">wuhan\n" + q + b"\n>none\nNNNNNNNNNNNNNNNNNNNNNNNNN\n>short\nACGT\n>head\n" + q[:60] + b"\n")
    dev = gx.SuffixIndex(s, ctx=ctx)
    r = dev.mems([q, b"N" * 25, b"ACGT", q[:60]], 20)
    dev.close()
    tsv = tmp_path / "mems.tsv"
    subprocess.run([CLI, "search", "-f", tpath, "-p", str(fa), "--mem", "20", "-o", str(tsv)], check=True, timeout=120,
                   env=dict(os.environ, GX_LOG="warn"))
    names, moff = ["wuhan", "none", "short", "head"], r["mem_offsets"]
    want_lines = [f"{names[c]}\t{r['qpos'][k]}\t{r['tpos'][k]}\t{r['length'][k]}"
                  for c in range(4) for k in range(int(moff[c]), int(moff[c + 1]))]
    want_lines += [f"{names[c]}\t-\t-\t0" for c in range(4) if moff[c] == moff[c + 1]]
    assert tsv.read_text().split("\n") == want_lines + [""]
    p = subprocess.run([CLI, "search", "-f", tpath, "-p", str(fa), "--mem", "20", "-k", "1"], capture_output=True, timeout=120)
    assert p.returncode == 2   # not together with -k
    p = subprocess.run([CLI, "search", "-f", tpath, "-p", str(fa), "--mem", "20", "-e", "1"], capture_output=True, timeout=120)
    assert p.returncode == 2   # nor with -e
