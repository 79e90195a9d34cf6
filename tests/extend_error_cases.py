"""The refusals of gx_suffix_index_extend as data, the way tests/search_error_cases.py holds those of the five
search calls: the inputs of every case and the raw caller that returns (return code, gx_last_error()).
tests/golden/make_extend_error_texts.py records them once into tests/golden/extend_error_texts.json;
tests/test_extend_host.py (host index) and tests/test_gpu_extend.py (device index) hold every later library
to that file.

A case is (id, overrides).  Without overrides a call is the pattern ACGT on an index of ACGTACGT with the one
hit [0, 4), band 1, the default scores, a CIGAR capacity of 16 and no NULL argument: it succeeds.  Overrides:
  packed, off       the batch (off may name more bytes than packed holds where the call is refused before a
                    byte is read)
  hoff, starts, ends   the hits (hoff may name more hits than starts and ends hold, likewise)
  null              arguments passed as NULL, by their names in gx.h
  band, scores, cap
Where two refusals apply at once the id names both, the winner first: those cases pin the order of the checks."""
import ctypes

import numpy as np

TEXT = b"ACGTACGT"


def _pair(first, second, **over):
    return (f"{first}-before-{second}", over)


def cases():
    return [
        ("idx-null", {"null": {"idx"}}),
        ("offsets-null", {"null": {"offsets"}}),
        ("hit-offsets-null", {"null": {"hit_offsets"}}),
        ("scores-null", {"null": {"scores"}}),
        ("cigar-offsets-null", {"null": {"cigar_offsets"}}),
        ("band-16", {"band": 16, "ends": [20]}),
        ("s-match-32768", {"scores": (32768, -2, -1, -5)}),
        ("s-mismatch-32768", {"scores": (1, -32768, -1, -5)}),
        ("g-32768", {"scores": (1, -2, -32768, -5)}),
        ("h-32768", {"scores": (1, -2, -1, 32768)}),
        ("offsets0", {"off": [1, 4]}),
        ("offsets-decrease", {"packed": b"ACGTACGT", "off": [0, 5, 3, 8], "hoff": [0, 0, 0, 0]}),
        ("pattern-4097", {"packed": b"A" * 4097, "off": [0, 4097]}),
        ("low-byte-p0-o2", {"packed": b"AC$T"}),
        ("patterns-null", {"null": {"patterns"}}),
        ("hit-offsets0", {"hoff": [1, 1]}),
        ("hit-offsets-decrease", {"packed": b"ACGTACGT", "off": [0, 4, 8], "hoff": [0, 1, 0]}),
        ("hits-range", {"hoff": [0, (1 << 32) - 2049]}),
        ("starts-null", {"null": {"starts"}}),
        ("ends-null", {"null": {"ends"}}),
        ("out-null", {"null": {"out"}}),
        ("hit-end-before-start", {"starts": [5], "ends": [4]}),
        ("hit-end-behind-text", {"starts": [5], "ends": [9]}),
        ("hit-leaves-band-long", {"starts": [0], "ends": [6]}),
        ("hit-leaves-band-short", {"starts": [1], "ends": [3]}),
        ("hit-2-of-pattern-1", {"packed": b"ACGTACGT", "off": [0, 4, 8], "hoff": [0, 1, 3], "starts": [0, 4, 2],
                                "ends": [4, 8, 9]}),
        ("ecap", {"packed": b"ACTACG", "off": [0, 6], "starts": [0], "ends": [7], "cap": 2}),
        ("ecap-0", {"cap": 0}),
        _pair("idx-null", "offsets-null", null={"idx", "offsets"}),
        _pair("offsets-null", "hit-offsets-null", null={"offsets", "hit_offsets"}),
        _pair("hit-offsets-null", "scores-null", null={"hit_offsets", "scores"}),
        _pair("scores-null", "cigar-offsets-null", null={"scores", "cigar_offsets"}),
        _pair("cigar-offsets-null", "band-16", null={"cigar_offsets"}, band=16),
        _pair("band-16", "g-32768", band=16, scores=(1, -2, -32768, -5)),
        _pair("s-match-32768", "h-32768", scores=(32768, -2, -1, 32768)),
        _pair("h-32768", "offsets0", scores=(1, -2, -1, 32768), off=[1, 4]),
        _pair("pattern-4097", "hit-offsets0", packed=b"A" * 4097, off=[0, 4097], hoff=[1, 1]),
        _pair("low-byte", "hit-offsets0", packed=b"AC$T", hoff=[1, 1]),
        _pair("hit-offsets0", "hit-offsets-decrease", packed=b"ACGTACGT", off=[0, 4, 8], hoff=[1, 2, 0]),
        _pair("hit-offsets-decrease", "starts-null", packed=b"ACGTACGT", off=[0, 4, 8], hoff=[0, 1, 0], null={"starts"}),
        _pair("hits-range", "starts-null", hoff=[0, (1 << 32) - 2049], null={"starts"}),
        _pair("starts-null", "ends-null", null={"starts", "ends"}),
        _pair("ends-null", "out-null", null={"ends", "out"}),
        _pair("out-null", "hit-end-behind-text", null={"out"}, starts=[5], ends=[9]),
        _pair("hit-end-behind-text", "hit-leaves-band", starts=[0], ends=[9]),
        _pair("hit-0-band", "hit-1-window", hoff=[0, 2], starts=[0, 5], ends=[6, 4]),
    ]


def run_case(gx, idx, over, fill=None):
    """(return code, gx_last_error()) of the case on idx (a gxamd.SuffixIndex of TEXT).  fill: a dict that
    receives the output arrays as the call left them (out as EXTEND_HIT_DTYPE, cigar, cigar_offsets), preset to
    0xAB.. / 0xDEADBEEF / 0xDEAD."""
    null = over.get("null", set())
    packed = over.get("packed", b"ACGT")
    off = np.asarray(over.get("off", [0, 4]), np.uint64)
    hoff = np.asarray(over.get("hoff", [0, 1]), np.uint64)
    starts = np.asarray(over.get("starts", [0]), np.uint32)
    ends = np.asarray(over.get("ends", [4]), np.uint32)
    cap = over.get("cap", 16)
    npat = len(off) - 1
    buf = np.frombuffer(packed, np.uint8)
    sc = gx.Scores(*over.get("scores", (1, -2, -1, -5))).c()
    nh = max(len(starts), 1)
    out = np.full(8 * nh, 0xABABABAB, np.uint32).view(gx.EXTEND_HIT_DTYPE)
    cig = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    coff = np.full(nh + 1, 0xDEAD, np.uint64)
    ptr = {"idx": idx.ptr, "patterns": buf.ctypes.data, "offsets": off.ctypes.data, "hit_offsets": hoff.ctypes.data,
           "starts": starts.ctypes.data, "ends": ends.ctypes.data, "scores": ctypes.byref(sc), "out": out.ctypes.data,
           "cigar": cig.ctypes.data, "cigar_offsets": coff.ctypes.data}
    a = {k: (None if k in null else v) for k, v in ptr.items()}
    lib = gx.lib()
    rc = lib.gx_suffix_index_extend(a["idx"], a["patterns"], a["offsets"], npat, a["hit_offsets"], a["starts"], a["ends"],
                                    a["scores"], over.get("band", 1), a["out"], a["cigar"], cap, a["cigar_offsets"])
    if fill is not None:
        fill.update(out=out, cigar=cig, cigar_offsets=coff)
    return int(rc), lib.gx_last_error().decode()
