"""The batches of tests/at_cap_cases.py on the host index and the host chain solver (no device): for every
batch the expectation composed from the pool's brute-force answers equals what the host computes for the whole
batch, field by field and dtype by dtype, and the batch meets its reach conditions on the host's own counts.
This shows without a GPU that the fixtures and the composition are right, and that the reference alone reaches
what tests/test_gpu_search_at_cap.py asserts of the device's counters."""
import numpy as np
import pytest

import at_cap_cases as ac
import edit_check
from at_cap_cases import ALL_HITS, CAP, REACH, WAVES, same_fields
from chain_check import closed_form, same


def total(a) -> int:
    return int(np.asarray(a).astype(np.int64).sum())


def test_tile_and_order():
    """tile() by hand, and every batch's order: longer than a pool, every member used, no grid-size period."""
    flat, off = ac.flat_of([[1, 2], [], [3], [4, 5, 6]], np.uint32)
    got, out = ac.tile(flat, off, np.array([3, 1, 0, 0, 2]))
    assert got.tolist() == [4, 5, 6, 1, 2, 1, 2, 3] and out.tolist() == [0, 3, 3, 5, 7, 8] and got.dtype == np.uint32
    assert not ac.aperiodic(np.arange(1024) % 256) and not ac.aperiodic(np.arange(5000) % 128)
    orders = [(ac.approx_batch().ids, len(ac.approx_batch().pool)), (ac.edit_batch().ids, len(ac.edit_batch().pool)),
              (ac.mem_batch().ids, len(ac.mem_batch().pool)), (ac.chain_anchors_batch()[0], 65),
              (ac.edit_k2_batch().ids, len(ac.edit_k2_batch().pool))]
    orders += [(ac.chain_segments_batch(H)[0], 64) for H in (64, 128, 256)]
    for ids, npool in orders:
        assert npool <= 300 and len(ids) > npool and set(ids.tolist()) == set(range(npool)) and ac.aperiodic(ids)


@pytest.fixture(scope="module")
def host(gx):
    idx = gx.SuffixIndex(ac.TEXT, host=True)
    yield idx
    idx.close()


def low_is_past_the_cap(b, per):
    """LOW lies beyond item CAP with a pattern of one or two candidates on both sides: `per` items a pattern."""
    before = total(per[b.ids[:b.low_at]])
    assert b.ids[b.low_at] == b.low and before > CAP + 256 and int(b.cand[b.low]) > 128
    for at in (b.low_at - 2, b.low_at - 1, b.low_at + 1, b.low_at + 2):
        assert 1 <= int(b.cand[b.ids[at]]) <= 2


@pytest.mark.parametrize("max_hits", [ALL_HITS, 3, 0], ids=["all", "3", "counts"])
def test_approx_batch(host, max_hits):
    b = ac.approx_batch()
    r = host.search_approx(b.patterns(), ac.K, max_hits=max_hits)
    same_fields(r, ac.approx_expected(max_hits))
    cands = total(r["candidates"])
    assert cands > REACH and cands % 256 not in (0, 255), cands
    low_is_past_the_cap(b, b.cand)
    assert (r["count"] > 3).sum() > 1000 and (r["count"] == 0).sum() > 1000   # max_hits = 3 cuts, and finds nothing to cut


@pytest.mark.parametrize("max_hits,starts", [(ALL_HITS, True), (3, False), (0, True)], ids=["all", "3-no-starts", "counts"])
def test_edit_batch(host, max_hits, starts):
    b = ac.edit_batch()
    r = host.search_edit(b.patterns(), ac.K, max_hits=max_hits, starts=starts)
    same_fields(r, ac.edit_expected(max_hits, starts))
    ends = ac.edit_pre_dedupe_ends()   # (the band model's: the host index does not report the number)
    assert total(r["candidates"]) > REACH and ends > REACH and ends % 256 not in (0, 255), ends
    assert total(r["count"]) > REACH and total(r["count"]) <= ends <= 6 * total(r["count"])
    if max_hits == ALL_HITS:
        assert int(r["hit_offsets"][-1]) == total(r["count"])
    low_is_past_the_cap(b, b.cand)
    low_is_past_the_cap(b, b.units)
    low_is_past_the_cap(b, np.array([edit_check.brute(b.s, P, ac.K)[0] for P in b.pool]))   # the reported ends


def test_edit_k2_batch(host):
    b = ac.edit_k2_batch()
    r = host.search_edit(b.patterns(), 2, max_hits=ALL_HITS)
    same_fields(r, ac.edit_expected(ALL_HITS, True, 2))
    cands = total(r["candidates"])
    assert cands > REACH and cands % 256 not in (0, 255) and total(r["count"]) > 10000, cands
    low_is_past_the_cap(b, b.cand)


def test_mem_batch(gx):
    b = ac.mem_batch()
    idx = gx.SuffixIndex(b.s, host=True)
    r = idx.mems(b.queries(), ac.MEM_MIN_LEN)
    counts = idx.mems(b.queries(), ac.MEM_MIN_LEN, max_mems=0)
    idx.close()
    same_fields(r, ac.mem_expected())
    assert np.array_equal(counts["mem_offsets"], r["mem_offsets"]) and np.array_equal(counts["candidates"], r["candidates"])
    kept, cands = int(r["mem_offsets"][-1]), total(r["candidates"])
    assert kept > REACH and cands > REACH and 2 * kept > cands   # most candidates are left-maximal
    per = np.diff(r["mem_offsets"].astype(np.int64)) / np.maximum(1, np.array([len(q) for q in b.queries()]))
    assert np.median(per) > 10   # tens of kept pairs a query position


@pytest.mark.parametrize("H", [64, 128, 256])
def test_chain_segments_batch(gx, H):
    ids, anchors, want = ac.chain_segments_batch(H)
    params = ac.CHAIN_PARAMS[H]
    same(gx.chain_anchors(anchors, host=True, **params), want, f"max_pred {H}")
    sizes = ac.segment_sizes(anchors, ac.CHAIN_GAP)
    segs, pairs = closed_form(anchors, **params)
    assert segs == len(sizes) > WAVES + 256 and set(sizes.tolist()) == set(ac.SEG_SIZES)
    # the wave that took segment s takes segment s + WAVES next: a long one after a short one and the reverse
    first, second = sizes[:-WAVES], sizes[WAVES:]
    assert int(((first <= 2) & (second >= 63)).sum()) >= 100 and int(((first >= 63) & (second <= 2)).sum()) >= 100
    assert int((first != second).sum()) >= 300
    nseg = [len(ac.segment_sizes({"qpos": anchors["qpos"][a:b], "mem_offsets": [0, b - a]}, ac.CHAIN_GAP))
            for a, b in zip(anchors["mem_offsets"][:50].astype(int), anchors["mem_offsets"][1:51].astype(int))]
    assert max(nseg) > 3 and len(ids) > 1000   # several segments a query, many queries
    assert len(want["root"]) > 1000 and int(want["n_anchors"].max()) > 4 and (want["pred"] != 0xFFFFFFFF).sum() > 10000


def test_chain_anchors_batch(gx):
    ids, across, anchors, want = ac.chain_anchors_batch()
    params = ac.CHAIN_PARAMS[64]
    same(gx.chain_anchors(anchors, host=True, **params), want)
    A = len(anchors["qpos"])
    assert A > REACH and closed_form(anchors, **params)[0] > WAVES + 256
    # the query that lies across anchor number CAP holds a chain with its root below CAP and its end above
    off = anchors["mem_offsets"].astype(np.int64)
    assert off[across] < CAP < off[across + 1]
    c0, c1 = int(want["chain_offsets"][across]), int(want["chain_offsets"][across + 1])
    assert c1 == c0 + 1
    root, end = int(off[across] + want["root"][c0]), int(off[across] + want["end"][c0])
    assert root < CAP - 64 and end > CAP + 64 and int(want["n_anchors"][c0]) == 300
    m0 = int(want["member_off"][c0])
    assert np.array_equal(want["members"][m0:m0 + 300], np.arange(300)) and m0 > 64 and int(want["member_off"][-1]) > m0 + 300
