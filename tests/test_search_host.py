"""Search mode on the host index (no device): gx_suffix_index_search with
ctx = NULL against the brute force of tests/search_check.py (an overlapping
scan for the occurrences, the explicitly sorted suffixes for `lo`, substring
tests for the longest prefix), on 200 random strings over five alphabets with
some 40 patterns each, the empty text, every max_hits edge, the GX_ECAP
protocol, every error code of DESIGN.md 18.1, SuffixTree.find, and BANANA and
MISSISSIPPI by hand."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from search_check import ALL_HITS, Brute, check_result
from test_suffix_host import BYTES_219, SIGN_EDGE, np_rand

ALPHABETS = [b"A", b"AC", b"ACGT", BYTES_219, SIGN_EDGE]


def patterns_for(s: bytes, rng) -> list:
    """Some 40 patterns: substrings at the start, the middle and the very end, the whole text and one
    byte more, substrings with one byte changed, below and above every suffix, m = 0 and m > n."""
    n = len(s)
    out = [b"", s, s + b"A", s + b"\xff", b"%", b"%" * 3, b"\xff", b"\xff" * (n + 1), s + s + b"C", b"A" * (n + 9)]
    alpha = sorted(set(s)) or [0x41]
    for m in (1, 2, 3, 7, 8, 9, 16, 17):
        if m > n:
            continue
        mid = int(rng.integers(0, n - m + 1))
        for i in (0, mid, n - m):
            out.append(s[i:i + m])
        sub = bytearray(s[mid:mid + m])
        k = int(rng.integers(0, m))
        sub[k] = alpha[(alpha.index(sub[k]) + 1) % len(alpha)] if len(alpha) > 1 else sub[k] + 1
        out.append(bytes(sub))
        sub = bytearray(s[n - m:])
        sub[-1] = 0xFF if sub[-1] != 0xFF else 0x25   # differs in its last byte, at the very end of the text
        out.append(bytes(sub))
    return out


@pytest.mark.parametrize("alpha", ALPHABETS, ids=["A", "AC", "ACGT", "bytes219", "sign_edge"])
def test_host_brute_force(gx, alpha):
    rng = np.random.default_rng(len(alpha))
    for k in range(40):
        n = int(rng.integers(1, 301))
        s = np_rand(1000 * len(alpha) + k, alpha, n)
        br = Brute(s)
        pats = patterns_for(s, rng)
        idx = gx.SuffixIndex(s, host=True)
        assert idx.sa().tolist() == br.sa
        check_result(br, pats, idx.search(pats))
        check_result(br, pats, idx.search(pats, max_hits=ALL_HITS), ALL_HITS)
        check_result(br, pats, idx.search(pats, max_hits=2), 2)
        idx.close()


def test_host_empty_text(gx):
    idx = gx.SuffixIndex(b"", host=True)
    assert idx.info() == {"n": 0, "on_device": False, "device_bytes": 0}
    assert idx.sa().tolist() == [0]
    pats = [b"", b"A", b"\xff\xff", b"%"]
    br = Brute(b"")
    check_result(br, pats, idx.search(pats, max_hits=ALL_HITS), ALL_HITS)
    r = idx.search([b""], max_hits=5)
    assert (r["lo"][0], r["count"][0], r["prefix_len"][0], r["prefix_pos"][0]) == (0, 1, 0, 0)
    assert r["positions"].tolist() == [0]
    assert idx.search([])["count"].tolist() == []
    idx.close()


def test_host_max_hits_edges(gx):
    s = np_rand(77, b"AC", 300)
    br = Brute(s)
    idx = gx.SuffixIndex(s, host=True)
    pats = [b"A", b"AC", b"CCA", b"ACACACACACAC", s[10:30], b""]
    count = br.hit(b"AC")[1]
    assert count > 3
    for mh in (0, 1, count - 1, count, count + 1, ALL_HITS):
        check_result(br, pats, idx.search(pats, max_hits=mh), mh)
    idx.close()


def raw_search(gx, idx, packed: bytes, offsets, max_hits, cap, want_positions=True):
    """gx_suffix_index_search as the C caller sees it: (rc, hits, positions, hit_offsets)."""
    off = np.asarray(offsets, np.uint64)
    npat = len(off) - 1
    pk = np.frombuffer(packed, np.uint8) if packed else np.zeros(1, np.uint8)
    hits = np.zeros(max(npat, 1), gx.HIT_DTYPE)
    pos = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    hoff = np.full(npat + 1, 0xDEAD, np.uint64)
    rc = gx.lib().gx_suffix_index_search(idx.ptr, pk.ctypes.data, off.ctypes.data, npat, hits.ctypes.data, max_hits,
                                         pos.ctypes.data if want_positions else None, cap,
                                         hoff.ctypes.data if want_positions else None)
    return rc, hits[:npat], pos, hoff


def test_host_ecap_protocol(gx):
    idx = gx.SuffixIndex(b"BANANA", host=True)
    packed, off = b"ANA" + b"A" + b"X", [0, 3, 4, 5]
    rc, hits, pos, hoff = raw_search(gx, idx, packed, off, ALL_HITS, 4)
    assert rc == 7                                                   # GX_ECAP
    assert b"5 positions needed" in gx.lib().gx_last_error()         # the needed count
    assert hits["count"].tolist() == [2, 3, 0] and hoff.tolist() == [0, 2, 5, 5]   # complete
    assert (pos == 0xDEADBEEF).all()                                 # untouched
    rc, hits, pos, hoff = raw_search(gx, idx, packed, off, ALL_HITS, int(hoff[-1]))   # allocate and repeat
    assert rc == 0 and pos.tolist() == [1, 3, 1, 3, 5] and hoff.tolist() == [0, 2, 5, 5]
    rc, hits, pos, hoff = raw_search(gx, idx, packed, off, ALL_HITS, 0)
    assert rc == 7
    rc, hits, pos, hoff = raw_search(gx, idx, packed, off, 0, 0, want_positions=False)   # counts only
    assert rc == 0 and hits["count"].tolist() == [2, 3, 0]
    idx.close()


def test_host_python_repeats_after_ecap(gx, monkeypatch):
    monkeypatch.setattr(gx, "_FIRST_CAP", 3)
    s = b"A" * 50
    idx = gx.SuffixIndex(s, host=True)
    check_result(Brute(s), [b"A", b"AA", b"C"], idx.search([b"A", b"AA", b"C"], max_hits=ALL_HITS), ALL_HITS)
    idx.close()


def test_host_errors(gx):
    L = gx.lib()
    for bad, k in ((b"AC$GT", 2), (b"AC GT", 2), (b"\x00", 0), (b"ACG\x24", 3)):
        with pytest.raises(gx.GxError) as e:
            gx.SuffixIndex(bad, host=True)
        assert e.value.code == 1 and f"at {k} " in str(e.value)
    idx = gx.SuffixIndex(b"ACGTACGT", host=True)
    # a pattern byte at or below '$': GX_EINVAL naming the pattern and the offset
    rc, *_ = raw_search(gx, idx, b"AC" + b"GT$A", [0, 2, 6], 0, 0, want_positions=False)
    assert rc == 1 and b"pattern 1" in L.gx_last_error() and b"offset 2" in L.gx_last_error()
    rc, *_ = raw_search(gx, idx, b"\x24", [0, 1], 0, 0, want_positions=False)
    assert rc == 1 and b"pattern 0" in L.gx_last_error() and b"offset 0" in L.gx_last_error()
    # offsets not non-decreasing from 0
    rc, *_ = raw_search(gx, idx, b"ACGT", [1, 2], 0, 0, want_positions=False)
    assert rc == 1
    rc, *_ = raw_search(gx, idx, b"ACGT", [0, 3, 2], 0, 0, want_positions=False)
    assert rc == 1
    # positions without hit_offsets
    hits = np.zeros(1, gx.HIT_DTYPE)
    pos = np.zeros(4, np.uint32)
    off = np.array([0, 1], np.uint64)
    pk = np.frombuffer(b"A", np.uint8)
    assert L.gx_suffix_index_search(idx.ptr, pk.ctypes.data, off.ctypes.data, 1, hits.ctypes.data, 4,
                                    pos.ctypes.data, 4, None) == 1
    # a pattern of 65,536 bytes: GX_ERANGE; 65,535 is admitted
    rc, *_ = raw_search(gx, idx, b"A" * 65536, [0, 65536], 0, 0, want_positions=False)
    assert rc == 3 and b"65535" in L.gx_last_error()
    rc, hits, *_ = raw_search(gx, idx, b"A" * 65535, [0, 65535], 0, 0, want_positions=False)
    assert rc == 0 and hits["count"][0] == 0 and hits["prefix_len"][0] == 1
    # total pattern bytes plus npat at or above 2^32 (decided on the offsets, before a byte is read)
    npat = 65536
    big = np.arange(npat + 1, dtype=np.uint64) * np.uint64(65535)
    assert int(big[-1]) + npat == 1 << 32   # the first sum that is refused
    rc, *_ = raw_search(gx, idx, b"A", big, 0, 0, want_positions=False)
    assert rc == 3 and b"split the batch" in L.gx_last_error()
    # n >= 2^30 (decided on n, before a byte is read)
    p = ctypes.c_void_p()
    one = np.zeros(1, np.uint8)
    assert L.gx_suffix_index_build(None, one.ctypes.data, 1 << 30, ctypes.byref(p)) == 3
    assert L.gx_suffix_index_build(None, None, 4, ctypes.byref(p)) == 1
    assert L.gx_search_info(None, None, None, None) == 1   # (it reports a context's last search)
    idx.close()


def test_host_total_positions_range(gx):
    """Total reported positions at or above 2^32: GX_ERANGE.  A^65536 and 65,536 times the pattern A with
    every occurrence: exactly 2^32 positions; with max_hits one lower the total is in range (GX_ECAP)."""
    idx = gx.SuffixIndex(b"A" * 65536, host=True)
    npat = 65536
    rc, hits, pos, hoff = raw_search(gx, idx, b"A" * npat, np.arange(npat + 1), ALL_HITS, 16)
    assert rc == 3 and b"lower max_hits" in gx.lib().gx_last_error()
    assert hits["count"].tolist() == [65536] * npat
    rc, hits, pos, hoff = raw_search(gx, idx, b"A" * npat, np.arange(npat + 1), 65535, 16)
    assert rc == 7 and int(hoff[-1]) == 65536 * 65535
    idx.close()


def test_suffix_tree_find(gx):
    tree = gx.SuffixTree(os.path.join(GOLDEN, "alphabets", "english.txt"), host=True)
    tree.insert_string("BANANA")
    tree.insert_string("MISSISSIPPI")
    assert tree.find("ANA") == [1, 3]
    assert tree.find("A") == [1, 3, 5]
    assert tree.find("BANANA") == [0]
    assert tree.find("NAB") == []
    assert tree.find("") == [0, 1, 2, 3, 4, 5, 6]
    assert tree.find("SSI", 1) == [2, 5]
    assert tree.find("ANA", string_idx=1) == []


def one(idx, P, max_hits=ALL_HITS):
    r = idx.search([P], max_hits=max_hits)
    return (int(r["lo"][0]), int(r["count"][0]), int(r["prefix_len"][0]), int(r["prefix_pos"][0]),
            r["positions"].tolist())


def test_banana_by_hand(gx):
    # suffixes of BANANA$ in order: $ A$ ANA$ ANANA$ BANANA$ NA$ NANA$ -> SA = 6 5 3 1 0 4 2
    idx = gx.SuffixIndex(b"BANANA", host=True)
    assert idx.sa().tolist() == [6, 5, 3, 1, 0, 4, 2]
    assert one(idx, b"ANA") == (2, 2, 3, 3, [1, 3])
    assert one(idx, b"A") == (1, 3, 1, 5, [1, 3, 5])
    assert one(idx, b"NA") == (5, 2, 2, 4, [2, 4])
    assert one(idx, b"BANANA") == (4, 1, 6, 0, [0])
    assert one(idx, b"") == (0, 7, 0, 6, [0, 1, 2, 3, 4, 5, 6])
    # ANB sorts behind ANANA$ and before BANANA$: its neighbours share 2 and 0 bytes with it
    assert one(idx, b"ANB") == (4, 0, 2, 1, [])
    # AM sorts behind A$ and before ANA$: both share 1 byte, the lower neighbour wins the tie
    assert one(idx, b"AM") == (2, 0, 1, 5, [])
    assert one(idx, b"BANANAS") == (5, 0, 6, 0, [])       # m > n
    assert one(idx, b"Z") == (7, 0, 0, 0, [])             # above every suffix
    assert one(idx, b"%") == (1, 0, 0, 0, [])             # below every suffix but '$'
    assert one(idx, b"A", max_hits=2) == (1, 3, 1, 5, [3, 5])   # SA[1..3) = 5, 3, ascending
    idx.close()


def test_mississippi_by_hand(gx):
    idx = gx.SuffixIndex(b"MISSISSIPPI", host=True)
    assert idx.sa().tolist() == [11, 10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2]
    assert one(idx, b"ISSI") == (3, 2, 4, 4, [1, 4])      # overlapping occurrences both count
    assert one(idx, b"SSI") == (10, 2, 3, 5, [2, 5])
    assert one(idx, b"I") == (1, 4, 1, 10, [1, 4, 7, 10])
    assert one(idx, b"P") == (6, 2, 1, 9, [8, 9])
    assert one(idx, b"ISSIM") == (3, 0, 4, 4, [])         # behind IPPI$ (1 shared), before ISSIPPI$ (4): the upper wins
    assert one(idx, b"SIR") == (9, 0, 2, 6, [])           # behind SIPPI$ and before SISSIPPI$, 2 shared each: the lower
    idx.close()
