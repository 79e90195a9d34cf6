"""The capped-grid kernels of search mode past their grid cap.

gx_approx.hip, gx_edit.hip, gx_match.hip and gx_chain.hip launch verify, emit, heads, scatter, starts, keep,
pack, flags, segments, best and walk on at most CAP = 2,048 x 256 lanes, which stride over the rest; below CAP
items every lane runs its loop body once, and the other GPU suites stay far below.  The batches of
tests/at_cap_cases.py pass the cap, so that here the loops take their second trip: the increment and the loop
bounds, the last workgroup's lanes past the total inside a live wave (aprx_verify_kernel, edit_heads_kernel),
the accumulators that persist across trips (ends and pair evaluations are held to their exact number, words and
cells to their bounds), the scan and the 64-bit-key sort of more than one chunk of partials as these drivers
call them, and in chain_score_kernel the wave that takes a second segment of another size.

Each case goes through the helper of its small suite (device_approx, device_edit, device_mems, device_chain),
so every *_info assertion made there holds here too.  Its result must equal in full, field by field and dtype
by dtype, the expectation composed from the pool's brute-force answers, and the host index.  Each case asserts
its reach from the device's own counters, so that one that no longer reaches the second trip fails.  (No build
with a broken stride was run against these tests: a kernel that skips its second trip leaves offsets unwritten
for the stages behind it to read.  What the tests can catch rests on the asserted reach and the full
comparison.)"""
import numpy as np
import pytest

import at_cap_cases as ac
from approx_check import same_approx
from at_cap_cases import ALL_HITS, REACH, WAVES, same_fields
from chain_check import same
from edit_check import same_edit
from match_check import same_mems
from test_gpu_approx import device_approx
from test_gpu_chain import device_chain
from test_gpu_edit import device_edit
from test_gpu_match import device_mems

pytestmark = pytest.mark.gpu

CAP = 2048 * 256   # kStrideGrid workgroups of kSufBlock lanes (gx_approx.hip, gx_edit.hip, gx_match.hip, gx_chain.hip)


@pytest.fixture(scope="module", autouse=True)
def the_cap_is_the_kernels(gx):
    T, _, B = gx.suffix_tile()
    assert (T, B) == (2048, 256) and T * B == CAP == ac.CAP and WAVES == CAP // 64


@pytest.fixture(scope="module")
def text(gx, ctx):
    host, dev = gx.SuffixIndex(ac.TEXT, host=True), gx.SuffixIndex(ac.TEXT, ctx=ctx)
    yield host, dev
    dev.close()
    host.close()


@pytest.mark.parametrize("max_hits", [ALL_HITS, 3], ids=["all", "3"])
def test_approx_past_the_cap(gx, ctx, text, max_hits):
    """aprx_verify_kernel and aprx_scatter_kernel at k = 1: 530,588 candidates of 33,165 patterns.  A^8 with 294
    consecutive candidates lies beyond candidate CAP between patterns of one or two (the one-atomic branch and
    the per-lane branch of the second trip), and the last workgroup's last trip is partial."""
    host, dev = text
    pats = ac.approx_batch().patterns()
    r = device_approx(gx, ctx, dev, pats, ac.K, max_hits)
    info = gx.approx_info(ctx)
    assert info["candidates"] > REACH and info["candidates"] % 256 not in (0, 255), info
    same_fields(r, ac.approx_expected(max_hits))
    same_approx(r, host.search_approx(pats, ac.K, max_hits=max_hits))


@pytest.mark.parametrize("max_hits,starts", [(ALL_HITS, True), (3, False)], ids=["all", "3-no-starts"])
def test_edit_past_the_cap(gx, ctx, text, max_hits, starts):
    """One batch carries every strided kernel of the edit search at k = 1: 1,444,909 candidates
    (edit_verify_kernel<1>, edit_emit_kernel), 2,120,033 ends before dedupe (the sort, edit_heads_kernel,
    edit_scatter_kernel; the band model of edit_check.py predicts the number) and with max_hits = ALL_HITS
    528,769 reported ends (edit_starts_kernel<1>).  With max_hits = 3 the scatter drops most heads of its second
    trip."""
    host, dev = text
    pats = ac.edit_batch().patterns()
    r = device_edit(gx, ctx, dev, pats, ac.K, max_hits, starts=starts)
    info = gx.edit_info(ctx)
    assert info["candidates"] > REACH and info["pre_dedupe_ends"] > REACH, info
    assert info["pre_dedupe_ends"] == ac.edit_pre_dedupe_ends() and info["pre_dedupe_ends"] % 256 not in (0, 255), info
    if max_hits == ALL_HITS:
        assert int(r["hit_offsets"][-1]) > REACH
    same_fields(r, ac.edit_expected(max_hits, starts))
    same_edit(r, host.search_edit(pats, ac.K, max_hits=max_hits, starts=starts))


def test_edit_k2_past_the_cap(gx, ctx, text):
    """edit_verify_kernel<2> and edit_emit_kernel at k = 2: 535,374 candidates of 17,527 patterns; ends and hits
    stay below CAP."""
    host, dev = text
    pats = ac.edit_k2_batch().patterns()
    r = device_edit(gx, ctx, dev, pats, 2, ALL_HITS)
    info = gx.edit_info(ctx)
    assert info["candidates"] > REACH and info["candidates"] % 256 not in (0, 255), info
    same_fields(r, ac.edit_expected(ALL_HITS, True, 2))
    same_edit(r, host.search_edit(pats, 2, max_hits=ALL_HITS))


def test_mems_past_the_cap(gx, ctx):
    """match_keep_kernel, match_emit_kernel, match_pack_kernel and the sort of more than CAP keys: 761,149
    candidates, 566,874 kept, at min_len 3; the counts-only call first, so that the emit kernel's words are held
    to their own bound on the second trip."""
    b = ac.mem_batch()
    host, dev = gx.SuffixIndex(b.s, host=True), gx.SuffixIndex(b.s, ctx=ctx)
    queries = b.queries()
    r = device_mems(gx, ctx, dev, queries, ac.MEM_MIN_LEN)
    info = gx.match_info(ctx)
    assert info["candidates"] > REACH and info["kept"] > REACH, info
    same_fields(r, ac.mem_expected())
    same_mems(r, host.mems(queries, ac.MEM_MIN_LEN))
    dev.close()
    host.close()


@pytest.mark.parametrize("H", [64, 128, 256])
def test_chain_second_segment(gx, ctx, H):
    """chain_score_kernel<1, 2, 4>: about 8,900 segments on 8,192 waves, so that wave s takes segment s + 8,192
    after segment s, more than a hundred times a long one after one of 1 or 2 anchors and more than a hundred
    times the reverse."""
    ids, anchors, want = ac.chain_segments_batch(H)
    r = device_chain(gx, ctx, anchors, ac.CHAIN_PARAMS[H])
    info = gx.chain_info(ctx)
    assert info["segments"] > WAVES + 256 and info["anchors"] >= WAVES, info
    same(r, want, f"max_pred {H}")
    same(r, gx.chain_anchors(anchors, host=True, **ac.CHAIN_PARAMS[H]), f"max_pred {H} (host)")


def test_chain_anchors_past_the_cap(gx, ctx):
    """flags, segments, best, heads and walk past CAP: 525,846 anchors in 15,620 segments; a chain of 300 anchors
    has its root below anchor number CAP and its end above."""
    ids, across, anchors, want = ac.chain_anchors_batch()
    r = device_chain(gx, ctx, anchors, ac.CHAIN_PARAMS[64])
    info = gx.chain_info(ctx)
    assert info["anchors"] > REACH and info["segments"] > WAVES + 256, info
    off, c = anchors["mem_offsets"].astype(np.int64), int(want["chain_offsets"][across])
    assert off[across] + int(want["root"][c]) < CAP < off[across] + int(want["end"][c])
    same(r, want)
    same(r, gx.chain_anchors(anchors, host=True, **ac.CHAIN_PARAMS[64]), "(host)")
