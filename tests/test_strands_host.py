"""Both strands of search mode on the host (no device).

  table       the library's complement table (through gx.revcomp of all 256 bytes) is an involution, keeps every
              byte above '$' above it and equals tests/strand_check.py's, written from the definition
  revcomp     gx.revcomp and the host gx.revcomp_batch on the kernel's edge batches, byte for byte
  contract    every stranded call on a host index returns what the existing call returns on the explicit item
              batch, every field and dtype, for "reverse" and "both"; "forward" is the existing call, keys
              included; and every planted reverse read is found on its item n + p
  MEMs        a query of a forward and an inverted block: the - item's MEMs mapped by m - qpos - len cover the
              inverted block, and chain_mems(strands="both") has one chain per block on the right item
  refusals    every text and the order of the checks against tests/golden/strand_error_texts.json

The command-line flag needs a device (the tool builds its index on GPU 0): tests/test_gpu_strands.py has it."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from strand_check import (EDGE_LENGTHS, STRANDS, comp_table, edge_batches, expected_items, item_batch, rc,
                          same_as_explicit, scenario)
from strand_error_cases import TEXT, cases, run_case

with open(os.path.join(GOLDEN, "strand_error_texts.json")) as f:
    WANT = json.load(f)
CASES = cases()
ALL = 0xFFFFFFFF


def library_table(gx) -> np.ndarray:
    """strand_comp of every byte: the reverse complement of 255, 254, .., 0 is comp(0), comp(1), .., comp(255)."""
    return np.frombuffer(gx.revcomp(bytes(range(255, -1, -1))), np.uint8)


def test_table_is_an_involution_that_keeps_bytes_above_the_terminator(gx):
    t = library_table(gx)
    assert t.size == 256
    assert np.array_equal(t[t], np.arange(256, dtype=np.uint8))
    assert all(int(t[x]) > 0x24 for x in range(0x25, 256))
    assert all(int(t[x]) <= 0x24 for x in range(0, 0x25))
    assert np.array_equal(t, comp_table())
    # the definition, spelled out once more: six pairs in both cases, S, W, N and U their own
    assert gx.revcomp(b"ACGTRYKMBVDHSWNUacgtrykmbvdhswnu") == b"unwsdhbvkmryacgtUNWSDHBVKMRYACGT"


def test_revcomp_on_the_edge_lengths(gx):
    rng = np.random.default_rng(5)
    for m in EDGE_LENGTHS + (65535, 70001):
        b = rng.integers(0, 256, m, dtype=np.uint8).tobytes()
        got = gx.revcomp(b)
        assert got == rc(b), m
        assert gx.revcomp(got) == b


@pytest.mark.parametrize("strands", STRANDS)
def test_host_revcomp_batch_on_the_edge_batches(gx, strands):
    for cid, items in edge_batches():
        want_b, want_o = expected_items(items, strands)
        got_b, got_o = gx.revcomp_batch(items, strands, ctx=None, pad=True)
        assert got_o.dtype == np.uint64 and np.array_equal(got_o, want_o), cid
        assert np.array_equal(got_b[:want_b.size], want_b), cid
        assert got_b.size == want_b.size + gx.STRAND_PAD and not got_b[want_b.size:].any(), cid


@pytest.fixture(scope="module")
def host(gx):
    idx = gx.SuffixIndex(scenario().text, host=True)
    yield idx
    idx.close()


def stranded_calls(S):
    """[(id, reads, call)]: call(idx, reads, **kw) is one of the six calls with its remaining arguments."""
    out = [("search", [S.reads[r] for r in S.select(2, False)], lambda i, b, **kw: i.search(b, ALL, **kw))]
    for k in (0, 1, 2):
        subs = [S.reads[r] for r in S.select(k, True)]
        anyk = [S.reads[r] for r in S.select(k, False)]
        out.append((f"approx-k{k}", subs, lambda i, b, k=k, **kw: i.search_approx(b, k, ALL, **kw)))
        out.append((f"edit-k{k}", anyk, lambda i, b, k=k, **kw: i.search_edit(b, k, ALL, **kw)))
        out.append((f"edit-k{k}-top2-no-starts", anyk, lambda i, b, k=k, **kw: i.search_edit(b, k, 2, starts=False, **kw)))
        out.append((f"map-k{k}", anyk, lambda i, b, k=k, **kw: i.map_reads(b, k, 4, **kw)[1]))
    longq = [S.query, S.reads[1], S.reads[0]]
    out.append(("match-stats", longq, lambda i, b, **kw: i.matching_stats(b, 40, **kw)))
    out.append(("mems", longq, lambda i, b, **kw: i.mems(b, 12, **kw)))
    out.append(("mems-counts", longq, lambda i, b, **kw: i.mems(b, 12, max_mems=0, **kw)))
    out.append(("search-counts", anyk, lambda i, b, **kw: i.search(b, 0, **kw)))
    return out


CALLS = stranded_calls(scenario())


@pytest.mark.parametrize("cid,reads,call", CALLS, ids=[c[0] for c in CALLS])
def test_contract_on_the_host_index(host, cid, reads, call):
    plain = call(host, reads)
    same_as_explicit(call(host, reads, strands="forward"), plain, len(reads), "forward")
    for strands in ("reverse", "both"):
        explicit = call(host, item_batch(reads, strands))
        same_as_explicit(call(host, reads, strands=strands), explicit, len(reads), strands)


def planted_found(S, idx, strands="both"):
    """Every planted read is found on the item of its strand and on no item by accident of the other: the point of
    the feature.  Returns how many reverse reads were checked."""
    checked = 0
    n = len(S.reads)
    exact = idx.search(S.reads, ALL, strands=strands)
    edit = {k: idx.search_edit([S.reads[r] for r in S.select(k, False)], k, ALL, strands=strands) for k in (0, 1, 2)}
    approx = {k: idx.search_approx([S.reads[r] for r in S.select(k, True)], k, ALL, strands=strands) for k in (0, 1, 2)}
    for r in range(n):
        item = (n if S.reverse[r] else 0) + r
        b, e = S.cut[r]
        if S.edits[r] == 0:
            o = exact["hit_offsets"]
            assert b in exact["positions"][int(o[item]):int(o[item + 1])].tolist(), r
        for k in (0, 1, 2):
            if S.edits[r] > k:
                continue
            sel = S.select(k, False)
            it = (len(sel) if S.reverse[r] else 0) + sel.index(r)
            o = edit[k]["hit_offsets"]
            assert e in edit[k]["ends"][int(o[it]):int(o[it + 1])].tolist(), (r, k)
            if S.subs[r]:
                sel = S.select(k, True)
                it = (len(sel) if S.reverse[r] else 0) + sel.index(r)
                o = approx[k]["hit_offsets"]
                assert b in approx[k]["positions"][int(o[it]):int(o[it + 1])].tolist(), (r, k)
        checked += S.reverse[r]
    return checked


def test_planted_reverse_reads_are_found_on_their_reverse_items(host):
    S = scenario()
    assert planted_found(S, host) == sum(S.reverse) >= 20
    # and the forward strand alone misses every one of them
    fwd = host.search(S.reads, ALL)
    assert all(int(fwd["count"][r]) == 0 for r in range(len(S.reads)) if S.reverse[r] and S.edits[r] == 0)


def check_planted_cigars(gx, S, idx):
    """map_reads(strands="both"): every planted reverse read has, on item n + p, the hit that ends where its
    window ends, and that hit's CIGAR spans the read and the window; an unedited read's is all matches."""
    for k in (0, 1, 2):
        sel = S.select(k, False)
        reads = [S.reads[r] for r in sel]
        found, ext = idx.map_reads(reads, k, ALL, strands="both")
        ho, co = found["hit_offsets"], ext["cigar_offsets"]
        for j, r in enumerate(sel):
            if not S.reverse[r]:
                continue
            item = len(sel) + j
            b, e = S.cut[r]
            hs = [h for h in range(int(ho[item]), int(ho[item + 1])) if int(found["ends"][h]) == e]
            assert len(hs) == 1, (k, r)
            start = int(found["starts"][hs[0]])   # (the shortest window's: within k of the cut)
            assert abs(start - b) <= k, (k, r, start, b)
            runs = ext["cigar"][int(co[hs[0]]):int(co[hs[0] + 1])]
            read_len = sum(int(x) >> 4 for x in runs if int(x) & 15 in (0, 1))
            window = sum(int(x) >> 4 for x in runs if int(x) & 15 in (0, 2))
            assert read_len == len(S.reads[r]) and window == e - start, (k, r, gx.cigar_string(runs))
            if S.edits[r] == 0:
                assert start == b and gx.cigar_string(runs) == f"{e - b}M" and int(ext["matches"][hs[0]]) == e - b


def test_map_reads_both_strands_has_the_planted_cigars(gx, host):
    check_planted_cigars(gx, scenario(), host)


def check_inverted_blocks(S, idx):
    (a0, a1), (b0, b1) = S.blocks
    m = len(S.query)
    r = idx.chain_mems([S.query], 20, strands="both")
    mems, ch = r["mems"], r["chains"]
    assert mems["pattern"].tolist() == [0, 0] and mems["strand"].tolist() == [0, 1]
    o = mems["mem_offsets"]
    plus = [(int(mems["qpos"][k]), int(mems["tpos"][k]), int(mems["length"][k])) for k in range(int(o[0]), int(o[1]))]
    minus = [(int(mems["qpos"][k]), int(mems["tpos"][k]), int(mems["length"][k])) for k in range(int(o[1]), int(o[2]))]
    # + item: the forward block where it was cut; - item: the inverted block, at qpos 0 of rc(Q)
    assert any(q == 0 and t == a0 and ln >= a1 - a0 for q, t, ln in plus)
    hit = [(q, t, ln) for q, t, ln in minus if t == b0 and ln >= b1 - b0]
    assert len(hit) == 1 and hit[0][0] == 0
    q, t, ln = hit[0]
    back = m - q - ln   # where the same bases begin in the caller's query
    assert back <= a1 - a0 and back + ln == m
    assert rc(S.query[back:back + ln]) == S.text[t:t + ln]
    # one chain per block, each on its item
    co = ch["chain_offsets"]
    assert co.tolist() == [0, 1, 2]
    assert int(ch["tstart"][0]) == a0 and int(ch["qstart"][0]) == 0
    assert int(ch["tstart"][1]) == b0 and int(ch["qstart"][1]) == 0
    # the forward strand alone sees only the forward block
    alone = idx.chain_mems([S.query], 20)
    assert alone["chains"]["chain_offsets"].tolist() == [0, 1] and "strand" not in alone["mems"]


def test_mems_of_an_inverted_block_and_its_chain(host):
    check_inverted_blocks(scenario(), host)


def test_palindrome_reports_in_both_items(gx):
    idx = gx.SuffixIndex(b"TTACGTAA", host=True)
    r = idx.search([b"ACGT"], ALL, strands="both")   # its own reverse complement
    assert r["count"].tolist() == [1, 1] and r["positions"].tolist() == [2, 2]
    idx.close()


@pytest.fixture(scope="module")
def tiny(gx):
    idx = gx.SuffixIndex(TEXT, host=True)
    yield idx
    idx.close()


@pytest.mark.parametrize("cid,call,over", CASES, ids=[c[0] for c in CASES])
def test_refusals_on_the_host(gx, tiny, cid, call, over):
    fill = {}
    rc_, text = run_case(gx, tiny, None, call, over, fill)
    assert {"rc": rc_, "text": text} == WANT[cid]
    if cid == "revcomp_batch-ecap":   # offsets complete, bytes untouched
        assert fill["offsets"].tolist() == [0, 4, 8, 12, 16] and (fill["bytes"] == 0xEE).all()
    if cid == "search-ecap-items":
        assert fill["offsets"].tolist() == [0, 2, 2, 4, 4] and (fill["positions"] == 0xDEADBEEF).all()


def test_every_recorded_refusal_has_its_case():
    assert sorted(WANT) == sorted(c[0] for c in CASES)


def test_unknown_strand_name_is_refused(gx, tiny):
    with pytest.raises(gx.GxError):
        tiny.search([b"ACGT"], strands="sideways")
