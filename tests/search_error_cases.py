"""The refusals of search mode's five entry points (gx_suffix_index_search, _search_approx, _search_edit,
_match_stats, _mems) as data: the inputs of every case and the raw caller that returns (return code,
gx_last_error()).  tests/golden/make_search_error_texts.py records them once into
tests/golden/search_error_texts.json; tests/test_search_errors.py holds every later library to that file.

A case is (id, mode, overrides).  Without overrides a call is the pattern ACGT on an index of ACGTACGT with
k = 1, every occurrence asked for, a capacity of 16 and no NULL argument: it succeeds.  Overrides:
  packed, off     the batch (off may name more bytes than packed holds where the call is refused before a
                  byte is read)
  null            arguments passed as NULL, by their names in gx.h
  k, max_hits, cap, length (max_len of the statistics, min_len of the MEMs)
  budget          GX_APPROX_CAND_BUDGET during the call
Where two refusals apply at once the id names both, the winner first: those cases pin the order of the checks."""
import contextlib
import os

import numpy as np

TEXT = b"ACGTACGT"
ALL_HITS = 0xFFFFFFFF
LONG = b"A" * 65536


def _pair(mode, first, second, **over):
    return (f"{mode}-{first}-before-{second}", mode, over)


def host_cases():
    """Everything that can be refused without a GPU."""
    out = []
    three = ("search", "approx", "edit")
    for mode in three + ("stats", "mems"):
        noun = "queries" if mode in ("stats", "mems") else "patterns"
        out += [
            (f"{mode}-idx-null", mode, {"null": {"idx"}}),
            (f"{mode}-offsets-null", mode, {"null": {"offsets"}}),
            (f"{mode}-{noun}-null", mode, {"null": {noun}}),
            (f"{mode}-offsets0", mode, {"off": [1, 4]}),
            (f"{mode}-offsets-decrease", mode, {"packed": b"ACGTACGT", "off": [0, 5, 3, 8]}),
            (f"{mode}-low-byte-p1-o2", mode, {"packed": b"ACGTAC$TA", "off": [0, 4, 9]}),
            (f"{mode}-low-byte-p0-o0", mode, {"packed": b"\x00CGT", "off": [0, 4]}),
            _pair(mode, "idx-null", "offsets-null", null={"idx", "offsets"}),
            _pair(mode, "offsets0", "decrease", packed=b"ACGTACGT", off=[1, 5, 3, 8]),
        ]
    for mode in three:
        out += [
            (f"{mode}-hits-null", mode, {"null": {"hits"}}),
            (f"{mode}-hit-offsets-null", mode, {"null": {"hit_offsets"}}),
            (f"{mode}-pattern-65536", mode, {"packed": LONG, "off": [0, 65536]}),
            (f"{mode}-range", mode, {"off": (np.arange(65538, dtype=np.uint64) * 65535).tolist()}),
            _pair(mode, "offsets-null", "hits-null", null={"offsets", "hits"}),
            _pair(mode, "hits-null", "hit-offsets-null", null={"hits", "hit_offsets"}),
            # (the loop takes a pattern's two checks together: pattern 0's length wins over pattern 1's order ...)
            _pair(mode, "pattern-65536", "decrease", packed=LONG, off=[0, 65536, 3]),
            # (... and pattern 1's order over pattern 2's length)
            _pair(mode, "decrease", "pattern-65536", packed=LONG, off=[0, 5, 3, 3 + 65536]),
            _pair(mode, "pattern-length", "range", off=[0, 1 << 32]),
            _pair(mode, "range", "patterns-null", off=(np.arange(65538, dtype=np.uint64) * 65535).tolist(),
                  null={"patterns"}),
        ]
    out += [
        _pair("search", "hit-offsets-null", "offsets0", null={"hit_offsets"}, off=[1, 4]),
        # approximate
        ("approx-distances-null", "approx", {"null": {"distances"}}),
        ("approx-k9", "approx", {"k": 9}),
        ("approx-short-pattern", "approx", {"packed": b"ACGTAC", "off": [0, 4, 6], "k": 2}),
        _pair("approx", "hit-offsets-null", "distances-null", null={"hit_offsets", "distances"}),
        _pair("approx", "distances-null", "k9", null={"distances"}, k=9),
        _pair("approx", "k9", "offsets0", k=9, off=[1, 4]),
        _pair("approx", "low-byte", "short-pattern", packed=b"ACGTA$", off=[0, 4, 6], k=2),
        # edit
        ("edit-distances-null", "edit", {"null": {"distances"}}),
        ("edit-starts-without-ends", "edit", {"null": {"ends"}}),
        ("edit-k9", "edit", {"k": 9}),
        ("edit-short-pattern", "edit", {"packed": b"ACGTAC", "off": [0, 4, 6], "k": 2}),
        ("edit-pattern-4097", "edit", {"packed": b"A" * 4097, "off": [0, 4097]}),
        _pair("edit", "hit-offsets-null", "distances-null", null={"hit_offsets", "distances"}),
        _pair("edit", "starts-without-ends", "k9", null={"ends"}, k=9),
        _pair("edit", "k9", "offsets0", k=9, off=[1, 4]),
        _pair("edit", "low-byte", "short-pattern", packed=b"ACGTA$", off=[0, 4, 6], k=2),
        # (again one loop: pattern 0's length over pattern 1's shortness, pattern 0's shortness over pattern 1's length)
        _pair("edit", "pattern-4097", "short-pattern", packed=b"A" * 4098, off=[0, 4097, 4098]),
        _pair("edit", "short-pattern", "pattern-4097", packed=b"A" * 4098, off=[0, 1, 4098]),
        _pair("edit", "pattern-65536", "pattern-4097", packed=LONG, off=[0, 65536]),
        # matching statistics
        ("stats-max-len-0", "stats", {"length": 0}),
        ("stats-stats-null", "stats", {"null": {"stats"}}),
        ("stats-range", "stats", {"off": [0, (1 << 32) - 16]}),
        _pair("stats", "offsets-null", "max-len-0", null={"offsets"}, length=0),
        _pair("stats", "max-len-0", "offsets0", length=0, off=[1, 4]),
        _pair("stats", "decrease", "range", off=[0, 1 << 32, 5]),
        _pair("stats", "range", "queries-null", off=[0, (1 << 32) - 16], null={"queries"}),
        _pair("stats", "low-byte", "stats-null", packed=b"AC$T", null={"stats"}),
        # MEMs
        ("mems-mem-offsets-null", "mems", {"null": {"mem_offsets"}}),
        ("mems-min-len-0", "mems", {"length": 0}),
        ("mems-range", "mems", {"off": [0, (1 << 32) - 16]}),
        _pair("mems", "offsets-null", "mem-offsets-null", null={"offsets", "mem_offsets"}),
        _pair("mems", "mem-offsets-null", "min-len-0", null={"mem_offsets"}, length=0),
        _pair("mems", "min-len-0", "offsets0", length=0, off=[1, 4]),
        _pair("mems", "decrease", "range", off=[0, 1 << 32, 5]),
        _pair("mems", "range", "queries-null", off=[0, (1 << 32) - 16], null={"queries"}),
    ]
    return out + driver_cases()


def driver_cases():
    """The refusals that arise behind the prologues, in the host drivers and the device drivers alike."""
    return [
        ("search-ecap", "search", {"cap": 1}),
        ("approx-ecap", "approx", {"cap": 1}),
        ("edit-ecap", "edit", {"cap": 1}),
        ("mems-ecap", "mems", {"length": 2, "cap": 1}),
        ("approx-seed-budget", "approx", {"budget": 3}),
        ("edit-seed-budget", "edit", {"budget": 3}),
        # (ACGT at k = 1: 4 seed hits; their bands report 2 + 3 + 2 + 3 ends, and the host, which stops at the
        # first candidate that takes it over the budget, gets there with the last one, so both sides name 10)
        ("edit-ends-budget", "edit", {"budget": 9}),
        # (AC, CG and GT twice each: 6 candidate pairs)
        ("mems-budget", "mems", {"length": 2, "budget": 5}),
    ]


@contextlib.contextmanager
def _budget(value):
    old = os.environ.get("GX_APPROX_CAND_BUDGET")
    if value is not None:
        os.environ["GX_APPROX_CAND_BUDGET"] = str(value)
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ["GX_APPROX_CAND_BUDGET"]
            else:
                os.environ["GX_APPROX_CAND_BUDGET"] = old


def run_case(gx, idx, mode, over):
    """(return code, gx_last_error()) of the case on idx (a gxamd.SuffixIndex of TEXT)."""
    null = over.get("null", set())
    packed = over.get("packed", b"ACGT")
    off = np.asarray(over.get("off", [0, 4]), np.uint64)
    n = len(off) - 1
    k, max_hits, cap = over.get("k", 1), over.get("max_hits", ALL_HITS), over.get("cap", 16)
    buf = np.frombuffer(packed, np.uint8)
    held = {}   # (the arrays live until the call returns)

    def arg(name, dtype=None, size=1):
        if name in null:
            return None
        if name == "idx":
            return idx.ptr
        if name in ("patterns", "queries"):
            return buf.ctypes.data
        if name == "offsets":
            return off.ctypes.data
        held[name] = np.zeros(max(size, 1), dtype)
        return held[name].ctypes.data

    lib = gx.lib()
    with _budget(over.get("budget")):
        if mode == "search":
            rc = lib.gx_suffix_index_search(arg("idx"), arg("patterns"), arg("offsets"), n, arg("hits", np.uint32, 4 * n),
                                            max_hits, arg("positions", np.uint32, cap), cap,
                                            arg("hit_offsets", np.uint64, n + 1))
        elif mode == "approx":
            rc = lib.gx_suffix_index_search_approx(arg("idx"), arg("patterns"), arg("offsets"), n, k,
                                                   arg("hits", np.uint32, 4 * n), max_hits,
                                                   arg("positions", np.uint32, cap), arg("distances", np.uint8, cap), cap,
                                                   arg("hit_offsets", np.uint64, n + 1))
        elif mode == "edit":
            rc = lib.gx_suffix_index_search_edit(arg("idx"), arg("patterns"), arg("offsets"), n, k,
                                                 arg("hits", np.uint32, 4 * n), max_hits, arg("ends", np.uint32, cap),
                                                 arg("distances", np.uint8, cap), arg("starts", np.uint32, cap), cap,
                                                 arg("hit_offsets", np.uint64, n + 1))
        elif mode == "stats":
            rc = lib.gx_suffix_index_match_stats(arg("idx"), arg("queries"), arg("offsets"), n, over.get("length", 4),
                                                 arg("stats", np.uint32, 4 * len(packed)))
        else:
            rc = lib.gx_suffix_index_mems(arg("idx"), arg("queries"), arg("offsets"), n, over.get("length", 4),
                                          arg("mems", np.uint32, 3 * cap), cap, arg("mem_offsets", np.uint64, n + 1),
                                          arg("candidates", np.uint64, n))
    return int(rc), lib.gx_last_error().decode()
