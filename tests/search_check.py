"""Brute-force checker of search mode.  It shares nothing with
the suffix array under test: occurrences come from an overlapping scan of s,
`lo` from the explicitly sorted suffixes of t = s + '$' (Python compares bytes
unsigned), the longest occurring prefix from substring tests."""
import numpy as np

ALL_HITS = 0xFFFFFFFF


def lcp(a: bytes, b: bytes) -> int:
    h = 0
    while h < len(a) and h < len(b) and a[h] == b[h]:
        h += 1
    return h


class Brute:
    def __init__(self, s: bytes):
        self.s = s
        self.t = s + b"$"
        self.N = len(self.t)
        self.sa = sorted(range(self.N), key=lambda i: self.t[i:])
        self.suf = [self.t[i:] for i in self.sa]
        self.cache = {}

    def occurrences(self, P: bytes):
        if not P:
            return list(range(self.N))   # Python's len(s) + 1 empty matches
        out, i = [], self.s.find(P)
        while i >= 0:
            out.append(i)
            i = self.s.find(P, i + 1)   # (overlapping)
        return out

    def hit(self, P: bytes):
        """(lo, count, prefix_len, prefix_pos, ascending occurrences)."""
        if P in self.cache:
            return self.cache[P]
        occ = self.occurrences(P)
        lo = sum(1 for x in self.suf if x < P)   # (one that has P as a prefix is not smaller)
        L = 0
        while L < len(P) and P[:L + 1] in self.s:
            L += 1
        if occ:
            assert L == len(P)
            assert sorted(self.sa[lo:lo + len(occ)]) == occ   # the interval is exactly the occurrences
            pos = self.sa[lo]
        else:
            a = lcp(P, self.suf[lo - 1]) if lo >= 1 else 0
            b = lcp(P, self.suf[lo]) if lo < self.N else 0
            assert max(a, b) == L, (a, b, L)   # the neighbours of the insertion point hold the longest prefix
            pos = 0 if L == 0 else (self.sa[lo - 1] if a >= b else self.sa[lo])
        r = (lo, len(occ), L, pos, occ)
        self.cache[P] = r
        return r


def check_result(br: Brute, patterns, r: dict, max_hits: int = 0):
    """Every field of SuffixIndex.search's result against the brute force."""
    s, n = br.s, len(br.s)
    assert all(len(r[k]) == len(patterns) for k in ("lo", "count", "prefix_len", "prefix_pos"))
    want_off = [0]
    for p, P in enumerate(patterns):
        lo, cnt, L, pos, occ = br.hit(P)
        got = tuple(int(r[k][p]) for k in ("lo", "count", "prefix_len", "prefix_pos"))
        assert got == (lo, cnt, L, pos), (p, P[:40], len(P), got, (lo, cnt, L, pos))
        # the definition of the prefix fields, apart from the neighbour rule
        assert L == len(P) or P[:L + 1] not in s
        if P:
            assert s[got[3]:got[3] + L] == P[:L]
        else:
            assert got[3] == n
        want_off.append(want_off[-1] + min(cnt, max_hits))
    if max_hits > 0:
        assert r["hit_offsets"].tolist() == want_off
        assert len(r["positions"]) == want_off[-1]
        for p, P in enumerate(patterns):
            lo, cnt, L, pos, occ = br.hit(P)
            seg = r["positions"][want_off[p]:want_off[p + 1]].tolist()
            if cnt <= max_hits:
                assert seg == occ, (p, P[:40], seg[:8], occ[:8])
            else:   # the first max_hits entries of the interval, ascending
                assert seg == sorted(br.sa[lo:lo + max_hits]), (p, P[:40])
    else:
        assert "positions" not in r


def check_light(s: bytes, sa, patterns, r: dict, max_hits: int):
    """The same fields on a text too long to sort its suffixes here: occurrences from the overlapping scan,
    `lo` from its definition on the (separately verified) suffix array `sa`, the prefix from substring tests."""
    t, N = s + b"$", len(s) + 1
    for p, P in enumerate(patterns):
        m = len(P)
        lo, cnt, L, pos = (int(r[k][p]) for k in ("lo", "count", "prefix_len", "prefix_pos"))
        occ, i = [], s.find(P)
        while i >= 0:
            occ.append(i)
            i = s.find(P, i + 1)
        assert cnt == len(occ), (p, cnt, len(occ))
        # m + 1 bytes of a suffix compare with P as the whole suffix does
        assert lo == 0 or t[sa[lo - 1]:sa[lo - 1] + m + 1] < P, p
        assert lo == N or not t[sa[lo]:sa[lo] + m + 1] < P, p
        assert s[pos:pos + L] == P[:L] and (L == m or P[:L + 1] not in s), p
        assert L == m if cnt else L < m
        seg = r["positions"][int(r["hit_offsets"][p]):int(r["hit_offsets"][p + 1])].tolist()
        assert seg == (occ if cnt <= max_hits else sorted(int(x) for x in sa[lo:lo + max_hits])), p


def same_result(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, np.flatnonzero(a[k] != b[k])[:4])
