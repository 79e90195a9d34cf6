"""The refusals of the stranded calls as data, the way tests/extend_error_cases.py holds those of
gx_suffix_index_extend: the inputs of every case and the raw caller that returns (return code, gx_last_error()).
tests/golden/make_strand_error_texts.py records them once into tests/golden/strand_error_texts.json;
tests/test_strands_host.py (host index, ctx = NULL) and tests/test_gpu_strands.py (device) hold every later
library to that file.

A case is (id, call, overrides).  `call` is one of CALLS.  Without overrides a call has the two patterns ACGT and
GGTA on an index of ACGTACGT, strands = 3 (both), k = 1, max_hits = 4, room for 64 of everything and no NULL
argument: it succeeds.  Overrides:
  strands, k, cap
  packed, off       the batch (off may name more bytes than packed holds where the call is refused before a
                    byte is read: the range cases are built from offsets alone)
  null              arguments passed as NULL, by their names in gx.h
Where two refusals apply at once the id names both, the winner first: those cases pin the order of the checks.
The order itself: strands; the existing call's refusals of the caller's batch up to its own 32-bit refusal; the
item batch's 32-bit refusal ("strands: ..."); the rest of the existing call's."""
import ctypes

import numpy as np

TEXT = b"ACGTACGT"
CALLS = ("search", "approx", "edit", "extend", "match_stats", "mems", "revcomp_batch")
SEARCHES = ("search", "approx", "edit", "extend", "match_stats", "mems")

# offsets alone: 32,770 patterns of 65,535 bytes are 2^31 + 98,302 bytes; on both strands twice that
_N_WIDE = 32770
WIDE_OFF = (np.arange(_N_WIDE + 1, dtype=np.uint64) * np.uint64(65535))
ONE_2_31 = [0, 1 << 31]        # one query of 2^31 bytes: 2^32 item bytes on both strands
ONE_2_32 = [0, 1 << 32]        # refused for itself


def cases():
    out = []
    for call in CALLS:
        out.append((f"{call}-strands-0", call, {"strands": 0}))
        out.append((f"{call}-strands-4", call, {"strands": 4}))
    for call in SEARCHES:
        out.append((f"{call}-strands-0-before-idx-null", call, {"strands": 0, "null": {"idx"}}))
        out.append((f"{call}-idx-null", call, {"null": {"idx"}}))
    out.append(("revcomp_batch-strands-0-before-offsets-null", "revcomp_batch", {"strands": 0, "null": {"offsets"}}))
    out.append(("revcomp_batch-offsets-null", "revcomp_batch", {"null": {"offsets"}}))
    out.append(("revcomp_batch-out-offsets-null", "revcomp_batch", {"null": {"out_offsets"}}))
    # the caller's batch: numbers are the caller's
    for call in CALLS:
        out.append((f"{call}-low-byte-p1-o2", call, {"packed": b"ACGTGG$A"}))
        out.append((f"{call}-offsets-decrease", call, {"off": [0, 5, 3]}))
    for call in ("approx", "edit"):
        out.append((f"{call}-pattern-1-short", call, {"packed": b"ACGTG", "off": [0, 4, 5], "k": 1}))
    # 32-bit conditions: the caller's own first, then the item batch's, both before a byte is read
    for call in ("search", "approx", "edit"):
        out.append((f"{call}-strands-range", call, {"off": WIDE_OFF}))
        out.append((f"{call}-strands-range-reverse-is-fine-then-bytes-null", call,
                    {"off": WIDE_OFF, "strands": 2, "null": {"bytes"}}))
        out.append((f"{call}-strands-range-before-bytes-null", call, {"off": WIDE_OFF, "null": {"bytes"}}))
    for call in ("match_stats", "mems", "revcomp_batch"):
        out.append((f"{call}-strands-range", call, {"off": ONE_2_31}))
        out.append((f"{call}-batch-range-before-strands-range", call, {"off": ONE_2_32}))
        out.append((f"{call}-strands-range-before-bytes-null", call, {"off": ONE_2_31, "null": {"bytes"}}))
    out.append(("search-offsets-decrease-before-strands-range", "search",
                {"off": np.concatenate([WIDE_OFF, np.zeros(1, np.uint64)])}))
    # behind the staging: as the existing call on the item batch
    out.append(("search-ecap-items", "search", {"cap": 1}))
    out.append(("mems-ecap-items", "mems", {"packed": b"ACGTACGT", "off": [0, 8], "cap": 1}))
    out.append(("revcomp_batch-ecap", "revcomp_batch", {"cap": 15}))
    out.append(("extend-hit-of-item-3", "extend", {"hoff": [0, 0, 0, 0, 1], "starts": [5], "ends": [9]}))
    return out


def run_case(gx, idx, ctx, call, over, fill=None):
    """(return code, gx_last_error()) of the case.  idx: a gxamd.SuffixIndex of TEXT (host or device); ctx: the
    context of revcomp_batch (None: host).  fill: a dict that receives the output arrays as the call left them."""
    null = over.get("null", set())
    packed = over.get("packed", b"ACGTGGTA")
    off = np.ascontiguousarray(over.get("off", [0, 4, 8]), np.uint64)
    strands, k, cap = over.get("strands", 3), over.get("k", 1), over.get("cap", 64)
    n = len(off) - 1
    items = n * (2 if strands == 3 else 1)
    small = n <= 64   # (the range cases are refused before any per-item array is touched)
    buf = np.frombuffer(packed, np.uint8)
    hits = np.full(4 * max(items if small else 1, 1), 0xABABABAB, np.uint32)
    pos = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    dst = np.full(max(cap, 1), 0xEE, np.uint8)
    sta = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    hoff = np.full((items if small else 1) + 1, 0xDEAD, np.uint64)
    cand = np.full(max(items if small else 1, 1), 0xDEAD, np.uint64)
    lib = gx.lib()
    a = {"idx": None if "idx" in null else idx.ptr, "bytes": None if "bytes" in null else buf.ctypes.data,
         "offsets": None if "offsets" in null else off.ctypes.data}
    if call == "search":
        rc = lib.gx_suffix_index_search_strands(a["idx"], a["bytes"], a["offsets"], n, strands, hits.ctypes.data, 4,
                                                pos.ctypes.data, cap, hoff.ctypes.data)
    elif call == "approx":
        rc = lib.gx_suffix_index_search_approx_strands(a["idx"], a["bytes"], a["offsets"], n, strands, k, hits.ctypes.data, 4,
                                                       pos.ctypes.data, dst.ctypes.data, cap, hoff.ctypes.data)
    elif call == "edit":
        rc = lib.gx_suffix_index_search_edit_strands(a["idx"], a["bytes"], a["offsets"], n, strands, k, hits.ctypes.data, 4,
                                                     pos.ctypes.data, dst.ctypes.data, sta.ctypes.data, cap,
                                                     hoff.ctypes.data)
    elif call == "extend":
        xoff = np.ascontiguousarray(over.get("hoff", [0] * (items + 1) if small else [0, 0]), np.uint64)
        xs = np.ascontiguousarray(over.get("starts", [0]), np.uint32)
        xe = np.ascontiguousarray(over.get("ends", [4]), np.uint32)
        sc = gx.Scores(1, -2, -1, -5).c()
        rec = np.full(8 * max(len(xs), 1), 0xABABABAB, np.uint32)
        rc = lib.gx_suffix_index_extend_strands(a["idx"], a["bytes"], a["offsets"], n, strands, xoff.ctypes.data,
                                                xs.ctypes.data, xe.ctypes.data, ctypes.byref(sc), 1, rec.ctypes.data,
                                                pos.ctypes.data, cap, hoff.ctypes.data)
    elif call == "match_stats":
        st = np.full(4 * 64, 0xABABABAB, np.uint32)
        rc = lib.gx_suffix_index_match_stats_strands(a["idx"], a["bytes"], a["offsets"], n, strands, 8, st.ctypes.data)
    elif call == "mems":
        mem = np.full(3 * max(cap, 1), 0xDEADBEEF, np.uint32)
        rc = lib.gx_suffix_index_mems_strands(a["idx"], a["bytes"], a["offsets"], n, strands, 2, mem.ctypes.data, cap,
                                              hoff.ctypes.data, cand.ctypes.data)
        pos = mem
    else:
        rc = lib.gx_revcomp_batch(ctx.ptr if ctx else None, a["bytes"], a["offsets"], n, strands, dst.ctypes.data, cap,
                                  None if "out_offsets" in null else hoff.ctypes.data)
    if fill is not None:
        fill.update(hits=hits, positions=pos, bytes=dst, offsets=hoff)
    return int(rc), lib.gx_last_error().decode()
