"""Both strands of search mode on the GPU: strand_rc_kernel through gx.revcomp_batch(ctx=ctx), and
the six stranded calls on a device index.

  kernel edges   byte-exact against tests/strand_check.py for each of the three strands on its edge batches:
                 every length of EDGE_LENGTHS at every start alignment mod 8 in the forward and in the reverse
                 half, no item, one empty item, empty items only, one item of 65,535 and one of 70,001 bytes,
                 bytes of the whole IUPAC alphabet in both cases and non-letters above '$'; the 16 bytes behind
                 the item batch read as zero; once more under GX_POOL_POISON=1, where an unwritten byte shows
  past the cap   one batch of a few MiB whose work units pass 2,048 x 256 lanes by a non-multiple of 256, the cap
                 inside a long item and short items behind it; the reach asserted from gx_strand_info
  contract       every stranded device call equals the existing device call on the explicit item batch, in every
                 field, dtype and *_info counter, and equals the host index
  map_reads      strands="both": every planted reverse read has its window's CIGAR on item n + p
  refusals       every text of tests/golden/strand_error_texts.json on the device, outputs left as it says
  CLI            without --strands the output is what the parent commit's binary wrote
                 (tests/golden/strand_cli_unflagged.json); with it the new columns"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from strand_check import STRANDS, edge_batches, expected_items, item_batch, packed, rc, same_as_explicit, scenario
from strand_error_cases import TEXT, run_case
from test_strands_host import ALL, CALLS, CASES, WANT, check_inverted_blocks, check_planted_cigars, planted_found

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "genomics-rs_amd", "gx-align")
CAP = 2048 * 256   # kStrideGrid workgroups of kSufBlock lanes (gx_strand.hip)
UNIT, PAD = 8, 16   # kStrandUnit, kSufPad


def units_of(total: int, strands: str) -> int:
    """The aligned 8-byte words of the output that strand_rc_kernel's lanes stride over (strand_units, gx_strand.h)."""
    at = total if strands == "both" else 0
    return (at + total + PAD + UNIT - 1) // UNIT - at // UNIT


def check_batch(gx, ctx, cid, items, strands):
    want_b, want_o = expected_items(items, strands)
    got_b, got_o = gx.revcomp_batch(items, strands, ctx=ctx, pad=True)
    info = gx.strand_info(ctx)
    assert got_o.dtype == np.uint64 and np.array_equal(got_o, want_o), cid
    assert got_b.size == want_b.size + PAD, cid
    bad = np.flatnonzero(got_b[:want_b.size] != want_b)
    assert bad.size == 0, (cid, strands, bad[:8].tolist())
    assert not got_b[want_b.size:].any(), (cid, strands, got_b[want_b.size:].tolist())
    total = sum(len(x) for x in items)
    assert info["items"] == len(want_o) - 1 and info["rc_bytes"] == (0 if strands == "forward" else total), (cid, info)
    return info


@pytest.mark.parametrize("strands", STRANDS)
@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_kernel_edges(gx, ctx, monkeypatch, strands, poison):
    if poison:
        monkeypatch.setenv("GX_POOL_POISON", "1")
    for cid, items in edge_batches():
        info = check_batch(gx, ctx, cid, items, strands)
        if strands != "forward":
            assert info["rc_ms"] > 0.0, (cid, info)


def test_past_the_grid_cap(gx, ctx):
    """40,000 items of 101 bytes, one of 300,001 and 2,000 of 37: 4,414,001 bytes.  Unit CAP writes byte
    8 x CAP = 4,194,304 of the reverse items, inside the long item (bytes 4,040,000 to 4,340,001), and the second
    trip goes on over the 37-byte items behind it, whose ends fall inside words."""
    T, _, B = gx.suffix_tile()
    assert T * B == CAP
    rng = np.random.default_rng(17)
    lens = [101] * 40000 + [300001] + [37] * 2000
    flat = np.frombuffer(b"ACGTRYKMBVDHSWNacgtn", np.uint8)[rng.integers(0, 20, sum(lens))].tobytes()
    items, at = [], 0
    for m in lens:
        items.append(flat[at:at + m])
        at += m
    total = at
    assert total < 5 << 20
    for strands in ("both", "reverse"):
        units = units_of(total, strands)
        assert units > CAP and (units - CAP) % 256 != 0
        start = (total % UNIT) if strands == "both" else 0   # the first unit's first byte is that far before the reverse items
        cap_byte = CAP * UNIT - start
        assert 40000 * 101 + UNIT < cap_byte < 40000 * 101 + 300001 - UNIT   # the cap falls inside the long item
        info = check_batch(gx, ctx, "cap", items, strands)
        assert units_of(info["rc_bytes"], strands) == units and info["items"] == len(lens) * (2 if strands == "both" else 1)


@pytest.fixture(scope="module")
def both(gx, ctx):
    S = scenario()
    host, dev = gx.SuffixIndex(S.text, host=True), gx.SuffixIndex(S.text, ctx=ctx)
    yield host, dev
    dev.close()
    host.close()


def counters(gx, ctx):
    """Every *_info of the context without the times: what ran behind the staging."""
    out = {}
    for name in ("search_info", "approx_info", "edit_info", "match_info", "extend_info"):
        out[name] = {k: v for k, v in getattr(gx, name)(ctx).items() if not k.endswith("_ms")}
    return out


@pytest.mark.parametrize("cid,reads,call", CALLS, ids=[c[0] for c in CALLS])
def test_contract_on_the_device(gx, ctx, both, cid, reads, call):
    host, dev = both
    plain = call(dev, reads)
    assert gx.strand_info(ctx)["rc_bytes"] == 0
    same_as_explicit(call(dev, reads, strands="forward"), plain, len(reads), "forward")
    total = sum(len(x) for x in reads)
    for strands in ("reverse", "both"):
        explicit = call(dev, item_batch(reads, strands))
        seen = counters(gx, ctx)
        got = call(dev, reads, strands=strands)
        info = gx.strand_info(ctx)
        assert counters(gx, ctx) == seen, (cid, strands)
        assert info["rc_bytes"] == total and info["rc_ms"] > 0.0, info
        assert info["items"] == len(reads) * (2 if strands == "both" else 1)
        same_as_explicit(got, explicit, len(reads), strands)
        same_as_explicit(got, call(host, reads, strands=strands), len(reads), strands)


def test_planted_reverse_reads_on_the_device(both):
    S = scenario()
    assert planted_found(S, both[1]) == sum(S.reverse)
    check_inverted_blocks(S, both[1])


def test_map_reads_both_strands_has_the_planted_cigars(gx, both):
    S = scenario()
    host, dev = both
    check_planted_cigars(gx, S, dev)
    for k in (0, 1, 2):
        reads = [S.reads[r] for r in S.select(k, False)]
        found, ext = dev.map_reads(reads, k, ALL, strands="both")
        same_as_explicit(ext, host.map_reads(reads, k, ALL, strands="both")[1], len(reads), "forward")   # (field by field)
        same_as_explicit(ext, dev.extend(item_batch(reads, "both"), found, band=k), len(reads), "both")


@pytest.fixture(scope="module")
def tiny(gx, ctx):
    idx = gx.SuffixIndex(TEXT, ctx=ctx)
    yield idx
    idx.close()


@pytest.mark.parametrize("cid,call,over", CASES, ids=[c[0] for c in CASES])
def test_refusals_on_the_device(gx, ctx, tiny, cid, call, over):
    fill = {}
    rc_, text = run_case(gx, tiny, ctx, call, over, fill)
    assert {"rc": rc_, "text": text} == WANT[cid]
    if cid == "revcomp_batch-ecap":   # offsets complete, bytes untouched
        assert fill["offsets"].tolist() == [0, 4, 8, 12, 16] and (fill["bytes"] == 0xEE).all()
    if cid == "search-ecap-items":
        assert fill["offsets"].tolist() == [0, 2, 2, 4, 4] and (fill["positions"] == 0xDEADBEEF).all()
    if "strands-range" in cid and rc_ == 3:   # refused from the offsets: nothing was staged
        assert (fill["hits"] == 0xABABABAB).all() and (fill["offsets"] == 0xDEAD).all()


# (name, genome, records, arguments): the sub-modes of gx-align search
CLI_MODES = [
    ("exact", "Human-BRCA2-cds.fasta", "test3_short.fasta", []),
    ("k1", "Human-BRCA2-cds.fasta", "test3_short.fasta", ["-k", "1"]),
    ("e1", "Human-BRCA2-cds.fasta", "test3_short.fasta", ["-e", "1"]),
    ("e1-cigar", "Human-BRCA2-cds.fasta", "test3_short.fasta", ["-e", "1", "--cigar"]),
    ("mem20", "Human-BRCA2-cds.fasta", "Human-Mouse-BRCA2-cds.fasta", ["--mem", "20"]),
    ("chain20", "Human-BRCA2-cds.fasta", "Human-Mouse-BRCA2-cds.fasta", ["--mem", "20", "--chain"]),
]


def run_cli(mode, extra):
    name, genome, records, args = mode
    fa = os.path.join(GOLDEN, "fasta")
    cmd = [CLI, "-c", os.path.join(GOLDEN, "config.toml"), "search", "-f", os.path.join(fa, genome), "-p",
           os.path.join(fa, records)] + args + extra
    return subprocess.run(cmd, capture_output=True, timeout=120, env=dict(os.environ, GX_LOG="warn"))


@pytest.mark.parametrize("mode", CLI_MODES, ids=[m[0] for m in CLI_MODES])
def test_cli_strands(mode):
    with open(os.path.join(GOLDEN, "strand_cli_unflagged.json")) as f:
        parent = json.load(f)
    plain = run_cli(mode, [])
    assert plain.returncode == 0 and plain.stdout.decode() == parent[mode[0]]
    nskip = 3 if "--mem" in mode[3] else 2   # name, strand (and the record's length)
    plain_lines = plain.stdout.decode().split("\n")[:-1]
    both = run_cli(mode, ["--strands", "both"])
    assert both.returncode == 0
    both_lines = both.stdout.decode().split("\n")[:-1]
    rev = run_cli(mode, ["--strands", "reverse"])
    assert rev.returncode == 0
    rev_lines = rev.stdout.decode().split("\n")[:-1]

    def strip(line, sign):
        f = line.split("\t")
        assert f[1] == sign, line
        if nskip == 3:
            assert int(f[2]) > 0
        return "\t".join(f[:1] + f[nskip:])

    if mode[0] == "exact":   # (once: the flag alone adds the column and nothing else; an unknown strand is a usage error)
        fwd = run_cli(mode, ["--strands", "forward"])
        assert fwd.returncode == 0 and [strip(x, "+") for x in fwd.stdout.decode().split("\n")[:-1]] == plain_lines
        assert run_cli(mode, ["--strands", "sideways"]).returncode == 2
    plus = [x for x in both_lines if x.split("\t")[1] == "+"]
    minus = [x for x in both_lines if x.split("\t")[1] == "-"]
    if "--mem" in mode[3]:
        # MEM and chain lines come per item, and the lines of items without any behind them: as sets
        assert sorted(strip(x, "+") for x in plus) == sorted(plain_lines)
        assert sorted(minus) == sorted(rev_lines) and minus
    else:
        assert both_lines == plus + minus and [strip(x, "+") for x in plus] == plain_lines
        assert minus == rev_lines and len(minus) == len(plus)
