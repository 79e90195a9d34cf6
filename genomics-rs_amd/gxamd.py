"""gxamd -- Python mirror of the reference's alignment interface over the C ABI.

nlaha/genomics-rs exposes (src/lib.rs:3-6):
  sequence::{Sequence, SequenceContainer, SequenceOperations::{from_fasta, is_match}}
  config::{Scores, Config, get_config}
  alignment::algo::{alignment_table, retrace, AlignmentChoice, AlignedSequences}
This module offers the same names with the same argument meaning, backed by
libgx_amd.so (HIP kernels for gfx950 + C ABI declared in include/gx.h).

There is no CPU fallback: if libgx_amd.so is missing or no HIP device is
present, calls raise GxError.
"""
from __future__ import annotations

import ctypes
import enum
import logging
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence as Seq, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_log = logging.getLogger("gxamd")
LIB_PATH = os.environ.get("GX_LIB", os.path.join(_HERE, "libgx_amd.so"))

GX_TABLE_PLANES = 1
GX_TABLE_MATCHES = 2
GX_ALIGN_MAX_CELL = 4
GX_STAGED_PLANE_SUMS = 8
GX_STAGED_ALTERNATE = 16   # gx.h: pass k runs the k % 2 half of the staged pairs
GX_STAGED_KEEP_PLANES = 32   # gx.h: the last pass's planes stay on the device (gx_staged_table)

# status codes (include/gx.h)
_CODES = {0: "GX_OK", 1: "GX_EINVAL", 2: "GX_ESEQ", 3: "GX_ERANGE", 4: "GX_ENOMEM", 5: "GX_EHIP",
          6: "GX_EPANIC", 7: "GX_ECAP", 8: "GX_EIO", 9: "GX_EPARSE"}


class GxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_CODES.get(code, code)}: {msg}")
        self.code = code


class CScores(ctypes.Structure):
    _fields_ = [("s_match", ctypes.c_int64), ("s_mismatch", ctypes.c_int64),
                ("g", ctypes.c_int64), ("h", ctypes.c_int64)]


class CCell(ctypes.Structure):
    _fields_ = [("insert_score", ctypes.c_int64), ("delete_score", ctypes.c_int64), ("sub_score", ctypes.c_int64),
                ("insert_matches", ctypes.c_uint64), ("delete_matches", ctypes.c_uint64),
                ("sub_matches", ctypes.c_uint64)]


class CStep(ctypes.Structure):
    _fields_ = [("choice", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 7),
                ("i", ctypes.c_uint64), ("j", ctypes.c_uint64)]


class CCompareCell(ctypes.Structure):
    _fields_ = [("score", ctypes.c_uint64), ("len_i", ctypes.c_uint64), ("len_j", ctypes.c_uint64),
                ("first_lcs", ctypes.c_uint64)]


class CSuffixStats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("num_internal", "num_leaves", "num_nodes", "string_depth_sum",
                                               "max_string_depth", "longest_repeat_start", "longest_repeat_len")]


class CResult(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int64), ("matches", ctypes.c_uint64), ("mismatches", ctypes.c_uint64),
                ("gap_extensions", ctypes.c_uint64), ("opening_gaps", ctypes.c_uint64),
                ("n_steps", ctypes.c_uint64), ("start_i", ctypes.c_uint64), ("start_j", ctypes.c_uint64),
                ("max_cell_i", ctypes.c_uint64), ("max_cell_j", ctypes.c_uint64),
                ("matches_at_max", ctypes.c_uint64), ("fill_us", ctypes.c_int64), ("retrace_us", ctypes.c_int64)]


CELL_DTYPE = np.dtype([("insert_score", "<i8"), ("delete_score", "<i8"), ("sub_score", "<i8"),
                       ("insert_matches", "<u8"), ("delete_matches", "<u8"), ("sub_matches", "<u8")])
STEP_DTYPE = np.dtype([("choice", "u1"), ("pad", "u1", (7,)), ("i", "<u8"), ("j", "<u8")])

# exported symbols (include/gx.h) -- checked by tests/test_abi.py
EXPORTED = ["gx_last_error", "gx_version", "gx_context_create", "gx_context_destroy", "gx_context_trim",
            "gx_alignment_table", "gx_table_info", "gx_table_export", "gx_table_export_plane", "gx_table_export_rows",
            "gx_table_plane_sums", "gx_retrace", "gx_table_free", "gx_align", "gx_align_batch", "gx_align_batch_multi",
            "gx_stage_pairs",
            "gx_run_staged", "gx_run_staged_steps", "gx_staged_plane_sums", "gx_staged_steps",
            "gx_staged_pass_results", "gx_fill_info", "gx_walk_info", "gx_walk_records", "gx_batch_chunks", "gx_fill_twin", "gx_fill_groups", "gx_overlap_scheme", "gx_overlap_rotate_plan", "gx_fill_plane_bits", "gx_plane_bytes_per_cell", "gx_twin_admission",
            "gx_twin_admission_mode", "gx_twin_admission_rows", "gx_fill_rows", "gx_fill_score_table", "gx_plan_layout",
            "gx_plan_twin_rows", "gx_staged_table",
            "gx_fasta_load",
            "gx_config_load", "gx_format_alignment", "gx_format_table",
            "gx_common_substring_host", "gx_common_substring", "gx_compare_pair", "gx_compare_matrix",
            "gx_compare_info", "gx_compare_batches", "gx_compare_segment_height", "gx_compare_run_stats",
            "gx_common_substring_candidates_host",
            "gx_suffix_tree_stats", "gx_suffix_info", "gx_suffix_digit_passes", "gx_suffix_tile", "gx_format_suffix_stats",
            "gx_suffix_index_build", "gx_suffix_index_free", "gx_suffix_index_info", "gx_suffix_index_export",
            "gx_suffix_index_search", "gx_search_info", "gx_suffix_index_search_approx", "gx_approx_info",
            "gx_suffix_index_search_edit", "gx_edit_info",
            "gx_suffix_index_match_stats", "gx_suffix_index_mems", "gx_match_info",
            "gx_suffix_index_extend", "gx_extend_info",
            "gx_chain_anchors", "gx_chain_info",
            "gx_revcomp", "gx_revcomp_batch", "gx_strand_info",
            "gx_suffix_index_search_strands", "gx_suffix_index_search_approx_strands",
            "gx_suffix_index_search_edit_strands", "gx_suffix_index_extend_strands",
            "gx_suffix_index_match_stats_strands", "gx_suffix_index_mems_strands"]

_lib = None


def lib():
    """Load libgx_amd.so (raises if absent: there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GxError(5, f"{LIB_PATH} not built (run `make -C genomics-rs_amd` or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint8)
    L.gx_last_error.restype = ctypes.c_char_p
    L.gx_version.restype = ctypes.c_char_p
    L.gx_context_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.gx_context_destroy.argtypes = [vp]
    L.gx_context_destroy.restype = None
    L.gx_context_trim.argtypes = [vp]
    L.gx_alignment_table.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_int,
                                     ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint64)]
    L.gx_table_info.argtypes = [vp] + [ctypes.POINTER(ctypes.c_uint64)] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    L.gx_table_export.argtypes = [vp, vp, sz]
    L.gx_table_export_plane.argtypes = [vp, ctypes.c_int, vp, sz, ctypes.c_int]
    L.gx_table_export_rows.argtypes = [vp, ctypes.c_int, sz, sz, vp, sz]
    L.gx_table_plane_sums.argtypes = [vp, vp]
    L.gx_staged_plane_sums.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.gx_staged_steps.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz)]
    L.gx_staged_pass_results.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.gx_retrace.argtypes = [vp, ctypes.c_int, vp, sz, ctypes.POINTER(CResult)]
    L.gx_table_free.argtypes = [vp]
    L.gx_table_free.restype = None
    L.gx_align.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_int,
                           ctypes.c_uint32, vp, sz, ctypes.POINTER(CResult)]
    L.gx_align_batch.argtypes = [vp, vp, vp, vp, vp, sz, ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_uint32,
                                 vp, vp, vp]
    L.gx_align_batch_multi.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, sz, ctypes.POINTER(CScores), ctypes.c_int,
                                       ctypes.c_uint32, vp, vp, vp]
    L.gx_stage_pairs.argtypes = [vp, vp, vp, vp, vp, sz]
    L.gx_run_staged.argtypes = [vp, ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_int, ctypes.c_uint32, vp,
                                ctypes.POINTER(ctypes.c_double)]
    L.gx_run_staged_steps.argtypes = [vp, ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                                      ctypes.c_int, vp, ctypes.POINTER(ctypes.c_double)]
    L.gx_fill_info.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int)] * 3
    L.gx_walk_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L.gx_walk_records.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.gx_batch_chunks.argtypes = [vp]
    L.gx_fill_twin.argtypes = [vp]
    L.gx_fill_groups.argtypes = [vp]
    if hasattr(L, "gx_overlap_scheme"):   # (absent from builds before the rotating pipeline, run for A/B timing)
        L.gx_overlap_scheme.argtypes = [vp]
        L.gx_overlap_rotate_plan.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    if hasattr(L, "gx_fill_plane_bits"):   # (absent from pre-12-bit builds run for A/B timing)
        L.gx_fill_plane_bits.argtypes = [vp]
    L.gx_plane_bytes_per_cell.argtypes = [ctypes.POINTER(CScores), ctypes.c_int]
    L.gx_twin_admission.argtypes = [ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_int64,
                                    ctypes.POINTER(ctypes.c_int64)]
    L.gx_twin_admission_mode.argtypes = [ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                         ctypes.POINTER(ctypes.c_int64)]
    if hasattr(L, "gx_twin_admission_rows"):   # (absent from builds before the 256-row strips, run for A/B timing)
        L.gx_twin_admission_rows.argtypes = [ctypes.POINTER(CScores), ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                             ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
        L.gx_fill_rows.argtypes = [vp]
    if hasattr(L, "gx_fill_score_table"):   # (absent from earlier builds run for A/B timing)
        L.gx_fill_score_table.argtypes = [vp]
        L.gx_plan_twin_rows.argtypes = [ctypes.POINTER(CScores), ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_int64), sz, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int)]
    L.gx_staged_table.argtypes = [vp, sz, ctypes.POINTER(vp)]
    L.gx_plan_layout.argtypes = [ctypes.POINTER(CScores), ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                 ctypes.POINTER(ctypes.c_int64), sz, ctypes.c_int, ctypes.c_int]
    L.gx_fasta_load.argtypes = [ctypes.c_char_p, vp, sz, vp, vp, vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.gx_config_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(CScores)]
    L.gx_format_alignment.argtypes = [vp, sz, vp, sz, vp, sz, ctypes.POINTER(CResult), vp, sz, ctypes.POINTER(sz)]
    L.gx_format_table.argtypes = [vp, sz, vp, sz, vp, sz, vp, vp, vp, ctypes.c_int, vp, sz, ctypes.POINTER(sz)]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.gx_common_substring_host.argtypes = [vp, sz, vp, sz, u64p, u64p, u64p]
    L.gx_common_substring_candidates_host.argtypes = [vp, sz, vp, sz, u64p, u64p]
    L.gx_common_substring.argtypes = [vp, vp, sz, vp, sz, u64p, u64p, u64p]
    L.gx_compare_pair.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(CCompareCell), u64p]
    L.gx_compare_matrix.argtypes = [vp, vp, vp, sz, vp]
    L.gx_compare_info.argtypes = [vp, u64p, u64p, u64p, u64p]
    L.gx_compare_batches.argtypes = [vp, u64p]
    L.gx_compare_segment_height.argtypes = []
    L.gx_compare_run_stats.argtypes = [vp, u64p, ctypes.POINTER(ctypes.c_double)]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    L.gx_suffix_tree_stats.argtypes = [vp, vp, sz, ctypes.POINTER(CSuffixStats), vp, vp, vp]
    L.gx_suffix_info.argtypes = [vp, u64p, u64p, dp, dp, dp]
    L.gx_suffix_digit_passes.argtypes = [vp, u64p]
    L.gx_suffix_tile.argtypes = [ip, ip, ip]
    L.gx_format_suffix_stats.argtypes = [ctypes.POINTER(CSuffixStats), vp, sz, vp, sz, ctypes.POINTER(sz)]
    L.gx_suffix_index_build.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    L.gx_suffix_index_free.argtypes = [vp]
    L.gx_suffix_index_free.restype = None
    L.gx_suffix_index_info.argtypes = [vp, u64p, ip, u64p]
    L.gx_suffix_index_export.argtypes = [vp, vp]
    L.gx_suffix_index_search.argtypes = [vp, vp, vp, sz, vp, ctypes.c_uint32, vp, sz, vp]
    L.gx_search_info.argtypes = [vp, u64p, dp, dp]
    L.gx_suffix_index_search_approx.argtypes = [vp, vp, vp, sz, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, sz, vp]
    L.gx_approx_info.argtypes = [vp, u64p, u64p, dp, dp]
    L.gx_suffix_index_search_edit.argtypes = [vp, vp, vp, sz, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, sz, vp]
    L.gx_edit_info.argtypes = [vp, u64p, u64p, u64p, dp, dp, dp]
    L.gx_suffix_index_match_stats.argtypes = [vp, vp, vp, sz, ctypes.c_uint32, vp]
    L.gx_suffix_index_mems.argtypes = [vp, vp, vp, sz, ctypes.c_uint32, vp, sz, vp, vp]
    L.gx_match_info.argtypes = [vp, u64p, u64p, u64p, dp, dp, dp]
    L.gx_suffix_index_extend.argtypes = [vp, vp, vp, sz, vp, vp, vp, ctypes.POINTER(CScores), ctypes.c_uint32, vp, vp, sz, vp]
    L.gx_extend_info.argtypes = [vp, u64p, u64p, u64p, u64p, dp, dp]
    L.gx_chain_anchors.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, vp, vp]
    L.gx_chain_info.argtypes = [vp, u64p, u64p, u64p, u64p, dp, dp]
    u32 = ctypes.c_uint32
    L.gx_revcomp.argtypes = [vp, sz, vp]
    L.gx_revcomp_batch.argtypes = [vp, vp, vp, sz, u32, vp, sz, vp]
    L.gx_suffix_index_search_strands.argtypes = [vp, vp, vp, sz, u32, vp, u32, vp, sz, vp]
    L.gx_suffix_index_search_approx_strands.argtypes = [vp, vp, vp, sz, u32, u32, vp, u32, vp, vp, sz, vp]
    L.gx_suffix_index_search_edit_strands.argtypes = [vp, vp, vp, sz, u32, u32, vp, u32, vp, vp, vp, sz, vp]
    L.gx_suffix_index_match_stats_strands.argtypes = [vp, vp, vp, sz, u32, u32, vp]
    L.gx_suffix_index_mems_strands.argtypes = [vp, vp, vp, sz, u32, u32, vp, sz, vp, vp]
    L.gx_suffix_index_extend_strands.argtypes = [vp, vp, vp, sz, u32, vp, vp, vp, ctypes.POINTER(CScores), u32, vp, vp, sz,
                                                 vp]
    L.gx_strand_info.argtypes = [vp, u64p, u64p, dp]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise GxError(rc, lib().gx_last_error().decode(errors="replace"))


def _buf(b: bytes):
    """Keep-alive numpy view of bytes and its address."""
    a = np.frombuffer(b, dtype=np.uint8) if len(b) else np.zeros(1, np.uint8)
    return a, a.ctypes.data


# ---------------------------------------------------------------------------
# config.rs

@dataclass
class Scores:
    """config::Scores (config.rs:6-13)."""
    s_match: int = 1
    s_mismatch: int = -2
    g: int = -1
    h: int = -5

    def c(self) -> CScores:
        return CScores(self.s_match, self.s_mismatch, self.g, self.h)


@dataclass
class Config:
    scores: Scores


def get_config(filepath: str) -> Config:
    """config::get_config (config.rs:21-40).  The reference exit(1)s on a read
    or parse error; this raises GxError (GX_EIO / GX_EPARSE) instead."""
    s = CScores()
    _check(lib().gx_config_load(filepath.encode(), ctypes.byref(s)))
    return Config(Scores(s.s_match, s.s_mismatch, s.g, s.h))


# ---------------------------------------------------------------------------
# sequence.rs

@dataclass
class Sequence:
    name: str
    sequence: str

    def __str__(self):  # sequence.rs:14-18
        return f"{self.name}: {self.sequence}"


@dataclass
class SequenceContainer:
    sequences: List[Sequence] = field(default_factory=list)

    def from_fasta(self, filepath: str) -> None:
        """from_fasta (sequence.rs:45-95): appends the file's records."""
        L = lib()
        nrec = ctypes.c_size_t(0)
        need = ctypes.c_size_t(0)
        # size query: the loader reports bytes/records needed when given no room
        rc = L.gx_fasta_load(filepath.encode(), None, 0, None, None, None, None, 0, ctypes.byref(nrec),
                             ctypes.byref(need))
        if rc not in (0, 7):
            _check(rc)
        k, nb = nrec.value, need.value
        if k == 0:
            return
        buf = np.zeros(max(nb, 1), np.uint8)
        arrs = [np.zeros(k, np.uint64) for _ in range(4)]
        _check(L.gx_fasta_load(filepath.encode(), buf.ctypes.data, buf.size, *[a.ctypes.data for a in arrs], k,
                               ctypes.byref(nrec), ctypes.byref(need)))
        raw = buf.tobytes()
        no, nl, so, sl = arrs
        for r in range(nrec.value):
            name = raw[int(no[r]):int(no[r] + nl[r])].decode("utf-8")
            seq = raw[int(so[r]):int(so[r] + sl[r])].decode("utf-8")
            self.sequences.append(Sequence(name, seq))

    def is_match(self, i: int, j: int, reverse_sequences: bool) -> bool:
        """is_match (sequence.rs:102-115), host-side (the fill evaluates it on the GPU)."""
        a = self.sequences[0].sequence.encode()
        b = self.sequences[1].sequence.encode()
        ip, jp = (len(b) - i, len(a) - j) if reverse_sequences else (i, j)
        x = a[ip] if 0 <= ip < len(a) else None
        y = b[jp] if 0 <= jp < len(b) else None
        return x == y


# ---------------------------------------------------------------------------
# alignment/algo.rs

class AlignmentChoice(enum.IntEnum):
    """#[repr(u8)] AlignmentChoice (algo.rs:124-133)."""
    Match = 0
    Mismatch = 1
    Insert = 2
    Delete = 3
    OpenInsert = 4
    OpenDelete = 5


@dataclass
class AlignedSequences:
    """algo.rs:135-146."""
    s1: Sequence
    s2: Sequence
    alignment: List[Tuple[AlignmentChoice, int, int]]
    score: int
    matches: int
    mismatches: int
    gap_extensions: int
    opening_gaps: int
    # beyond the reference struct: where the walk started, timings
    start: Tuple[int, int] = (0, 0)
    max_cell: Tuple[int, int] = (0, 0)
    matches_at_max: int = 0
    fill_us: int = 0
    retrace_us: int = 0
    _steps: Optional[np.ndarray] = None

    def __str__(self):
        """Display for AlignedSequences (display.rs:9-127)."""
        L = lib()
        a, pa = _buf(self.s1.sequence.encode())
        b, pb = _buf(self.s2.sequence.encode())
        steps = self._steps if self._steps is not None else _steps_array(self.alignment)
        res = CResult(self.score, self.matches, self.mismatches, self.gap_extensions, self.opening_gaps,
                      len(steps), 0, 0, 0, 0, 0, 0, 0)
        need = ctypes.c_size_t(0)
        L.gx_format_alignment(pa, len(self.s1.sequence.encode()), pb, len(self.s2.sequence.encode()),
                              steps.ctypes.data, len(steps), ctypes.byref(res), None, 0, ctypes.byref(need))
        out = ctypes.create_string_buffer(need.value)
        _check(L.gx_format_alignment(pa, len(self.s1.sequence.encode()), pb, len(self.s2.sequence.encode()),
                                     steps.ctypes.data, len(steps), ctypes.byref(res), out, need.value, None))
        return out.value.decode("utf-8")


def _steps_array(alignment) -> np.ndarray:
    arr = np.zeros(len(alignment), STEP_DTYPE)
    for k, (c, i, j) in enumerate(alignment):
        arr[k]["choice"] = int(c)
        arr[k]["i"] = i
        arr[k]["j"] = j
    return arr


def plane_bytes_per_cell(scores: "Scores", is_local: bool) -> int:
    """Score-plane bytes per cell of a batch launch with these scores: 3
    (compact byte differences) or 12 (int32 planes); gx_plane_bytes_per_cell.
    An upper bound: a launch that takes the twin fill writes 2 (its plane
    codes; Context.fill_info reports the launch's figure)."""
    r = lib().gx_plane_bytes_per_cell(ctypes.byref(scores.c()), int(is_local))
    if r < 0:
        raise GxError(3, "invalid scores")
    return r


def plan_layout(scores: "Scores", is_local: bool, shapes: Seq[Tuple[int, int]], track: bool = False,
                grid_cap: int = 0) -> int:
    """The fill layout a launch of these (n, m) pair shapes would take
    (gx_plan_layout; host rule only, no device): 0 anti-diagonal 128-row
    strips, 1 the column step, 3 the skewed 64-row strips; -1 invalid."""
    k = len(shapes)
    n = (ctypes.c_int64 * max(k, 1))(*[a for a, _ in shapes])
    m = (ctypes.c_int64 * max(k, 1))(*[b for _, b in shapes])
    return lib().gx_plan_layout(ctypes.byref(scores.c()), int(bool(is_local)), n, m, k, int(bool(track)),
                                int(grid_cap))


def plan_twin_rows(scores: "Scores", shapes: Seq[Tuple[int, int]], grid_cap: int = 0) -> Tuple[int, int]:
    """(rows per lane, band width) a global staged launch of these (n, m) pair
    shapes with planes would take (gx_plan_twin_rows; host rule only, no
    device): rows 4 or 2, band width 0 when it would not be the twin fill."""
    k = len(shapes)
    n = (ctypes.c_int64 * max(k, 1))(*[a for a, _ in shapes])
    m = (ctypes.c_int64 * max(k, 1))(*[b for _, b in shapes])
    w = ctypes.c_int(0)
    r = lib().gx_plan_twin_rows(ctypes.byref(scores.c()), n, m, k, int(grid_cap), ctypes.byref(w))
    if r < 0:
        raise GxError(3, "invalid scores or shapes")
    return r, int(w.value)


def twin_admission(scores: "Scores", band_waves: int, col_gap: int = 0, is_local: bool = False,
                   rows_per_lane: int = 2) -> Tuple[bool, int]:
    """The twin fill's int16 admission rule (gx_twin_admission_mode): (admitted,
    bound), bound = the largest |value - base| a band of `band_waves` strips
    can reach when a twin's pairs differ by up to col_gap columns.
    rows_per_lane = 4: the rule of the 256-row strips (gx_twin_admission_rows)."""
    b = ctypes.c_int64(0)
    if rows_per_lane != 2:
        r = lib().gx_twin_admission_rows(ctypes.byref(scores.c()), int(bool(is_local)), int(band_waves),
                                         int(col_gap), int(rows_per_lane), ctypes.byref(b))
    else:
        r = lib().gx_twin_admission_mode(ctypes.byref(scores.c()), int(bool(is_local)), int(band_waves), int(col_gap),
                                         ctypes.byref(b))
    if r < 0:
        raise GxError(3, "invalid scores")
    return bool(r), int(b.value)


class Context:
    """One GPU: device-memory cache and stream (gx_context)."""

    def __init__(self, device: int = 0):
        p = ctypes.c_void_p()
        _check(lib().gx_context_create(device, ctypes.byref(p)))
        self.ptr = p
        self.device = device

    def close(self):
        if self.ptr:
            lib().gx_context_destroy(self.ptr)
            self.ptr = None

    def trim(self):
        _check(lib().gx_context_trim(self.ptr))

    def fill_info(self) -> dict:
        """The last fill launch: layout, band width, score-plane bytes per cell (gx_fill_info)."""
        v = [ctypes.c_int() for _ in range(3)]
        _check(lib().gx_fill_info(self.ptr, *[ctypes.byref(x) for x in v]))
        bits = lib().gx_fill_plane_bits(self.ptr) if hasattr(lib(), "gx_fill_plane_bits") else 8 * v[2].value
        return {"layout": v[0].value, "band_waves": v[1].value,
                "plane_bytes_per_cell": bits // 8 if bits % 8 == 0 else bits / 8,   # (twin codes: 1.5)
                "chunks": lib().gx_batch_chunks(self.ptr), "twin": lib().gx_fill_twin(self.ptr),
                "groups": lib().gx_fill_groups(self.ptr),
                "twin_rows": lib().gx_fill_rows(self.ptr) if hasattr(lib(), "gx_fill_rows") else 2,
                "score_table": lib().gx_fill_score_table(self.ptr) if hasattr(lib(), "gx_fill_score_table") else -1}

    def walk_info(self) -> dict:
        """The last device walk collected (gx_walk_info): whether it was the sequential strip walk,
        its walker priority, the table-driven chase's switch and block counts, pair 0's cycles a block,
        and the priorities of the last sequential walks launched (up to eight, the latest last)."""
        v = (ctypes.c_int * 16)()
        _check(lib().gx_walk_info(self.ptr, v))
        d = dict(zip(("sequential", "prio", "fast", "blocks_chased", "blocks_fixed_point", "pairs",
                      "cycles_per_block", "walk_cycles_per_block"), (int(x) for x in v[:8])))
        d["launch_prios"] = [int(x) for x in v[8:] if x >= 0]
        return d

    def walk_records(self) -> list:
        """That walk's records (kept under GX_WALK_RECORDS=1), per pair (gx_walk_records): {"end": (i, j), "first_strip", "blocks_chased",
        "blocks_fixed_point", "half", "strips": [((entry i, entry j, records, active), [record words])]}."""
        n = ctypes.c_size_t()
        _check(lib().gx_walk_records(self.ptr, None, 0, ctypes.byref(n)))
        buf = np.zeros(n.value, np.uint32)
        _check(lib().gx_walk_records(self.ptr, buf.ctypes.data, buf.size, ctypes.byref(n)))
        w = buf.view(np.int32).tolist()
        out, k = [], 2
        for _ in range(w[0]):
            ei, ej, first, chased, fixed, half, ns = w[k:k + 7]
            k += 7
            strips = []
            for _s in range(ns):
                seg = tuple(w[k:k + 4])
                k += 4
                nr = min(max(seg[2], 0), w[1]) if seg[3] else 0
                strips.append((seg, w[k:k + nr]))
                k += nr
            out.append({"end": (ei, ej), "first_strip": first, "blocks_chased": chased, "blocks_fixed_point": fixed,
                        "half": half, "strips": strips})
        assert k == len(w)
        return out

    def overlap_scheme(self) -> int:
        """Which overlapped pipeline the last staged / batch call ran (gx_overlap_scheme):
        2 the three-buffer rotation, 1 two A buffers and one B buffer, 0 none."""
        return lib().gx_overlap_scheme(self.ptr)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ROTATE_PLAN_FIELDS = ("job", "fslot", "wslot", "stream", "wait_walk", "collected", "labelled")


def overlap_rotate_plan(fill: int) -> dict:
    """The rotating overlapped pipeline's index arithmetic for fill 2 pass + group
    (gx_overlap_rotate_plan; host only)."""
    v = (ctypes.c_int * 7)()
    _check(lib().gx_overlap_rotate_plan(fill, v))
    return dict(zip(ROTATE_PLAN_FIELDS, (int(x) for x in v)))


_default_ctx: dict = {}


def device_for_rank(local_rank: int) -> int:
    """HIP device of a local rank: GX_DEVICE_MAP="d0,d1,..." maps rank r to
    map[r % len] (several ranks may share one GPU, e.g. "0,0" to run the
    two-rank path on a one-GPU box); otherwise the rank itself."""
    dm = os.environ.get("GX_DEVICE_MAP", "")
    devs = [int(x) for x in dm.split(",") if x.strip()]
    return devs[local_rank % len(devs)] if devs else local_rank


def default_context(device: Optional[int] = None) -> Context:
    if device is None:
        device = device_for_rank(int(os.environ.get("LOCAL_RANK", "0"))) if "GX_DEVICE" not in os.environ \
            else int(os.environ["GX_DEVICE"])
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


class AlignmentTable:
    """A device-resident Array2<AlignmentCell> (gx_table).  Consumed by retrace()."""

    def __init__(self, ptr, s1: bytes, s2: bytes, flags: int):
        self.ptr = ptr
        self.s1, self.s2 = s1, s2
        self.flags = flags

    @property
    def shape(self):
        return (len(self.s1) + 1, len(self.s2) + 1)

    def info(self):
        v = [ctypes.c_uint64() for _ in range(4)]
        us = ctypes.c_int64()
        _check(lib().gx_table_info(self.ptr, *[ctypes.byref(x) for x in v], ctypes.byref(us)))
        return {"shape": (v[0].value, v[1].value), "max_cell": (v[2].value, v[3].value), "fill_us": us.value}

    def export(self) -> np.ndarray:
        """The full table as the reference's column-major Array2 (structured
        numpy array of shape (n+1, m+1), Fortran order, dtype == AlignmentCell)."""
        n1, m1 = self.shape
        out = np.zeros(n1 * m1, CELL_DTYPE)
        _check(lib().gx_table_export(self.ptr, out.ctypes.data, out.size))
        return out.reshape((n1, m1), order="F")

    def plane(self, which: int) -> np.ndarray:
        """int64 plane (0 insert, 1 delete, 2 sub), row-major (n+1, m+1)."""
        n1, m1 = self.shape
        out = np.zeros((n1, m1), np.int64)
        _check(lib().gx_table_export_plane(self.ptr, which, out.ctypes.data, out.size, 0))
        return out

    def rows(self, which: int, row0: int, nrows: int) -> np.ndarray:
        """int64 rows row0 .. row0+nrows-1 of plane `which`, shape (nrows, m+1)."""
        m1 = self.shape[1]
        out = np.zeros((nrows, m1), np.int64)
        _check(lib().gx_table_export_rows(self.ptr, which, row0, nrows, out.ctypes.data, out.size))
        return out

    def plane_sums(self) -> List[int]:
        """Device-side checksums of the I, D, S planes (gx_table_plane_sums):
        sum over interior cells of value * (1 + i*0x9E3779B1 + j*0x85EBCA77) mod 2^64."""
        out = np.zeros(3, np.uint64)
        _check(lib().gx_table_plane_sums(self.ptr, out.ctypes.data))
        return [int(x) for x in out]

    def free(self):
        if self.ptr:
            lib().gx_table_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _first_two(sc: SequenceContainer) -> Tuple[Sequence, Sequence]:
    if len(sc.sequences) < 2:
        # the reference panics with index out of bounds (algo.rs:169)
        raise GxError(2, "index out of bounds: fewer than two sequences in the container")
    return sc.sequences[0], sc.sequences[1]


def alignment_table(sequence_container: SequenceContainer, scores: Scores, is_local: bool,
                    reverse_sequences: bool, flags: int = GX_TABLE_PLANES,
                    ctx: Optional[Context] = None, max_cell: bool = True) -> Tuple[AlignmentTable, int]:
    """alignment_table (algo.rs:151-282) on the GPU -> (table, matches_at_max).

    max_cell=False skips the running max cell and matches_at_max (returned as
    0): the untracked fill, whose score planes are kept in the compact
    byte format (gx_api_plan.cpp d8_planes_ok) when the table is built on layout 0."""
    a, b = _first_two(sequence_container)
    if len(sequence_container.sequences) > 2:   # algo.rs:161-163
        _log.warning("More than two sequences found. Only the first two will be used.")
    s1, s2 = a.sequence.encode(), b.sequence.encode()
    ctx = ctx or default_context()
    x, px = _buf(s1)
    y, py = _buf(s2)
    t = ctypes.c_void_p()
    mam = ctypes.c_uint64()
    _check(lib().gx_alignment_table(ctx.ptr, px, len(s1), py, len(s2), ctypes.byref(scores.c()), int(is_local),
                                    int(reverse_sequences), flags, ctypes.byref(t),
                                    ctypes.byref(mam) if max_cell else None))
    return AlignmentTable(t, s1, s2, flags), int(mam.value)


DISP_MAX_WIDTH = 200  # display.rs:7


def _stdout_color() -> bool:
    """The `colored` crate's decision: a terminal, unless NO_COLOR / CLICOLOR=0
    (CLICOLOR_FORCE forces colour)."""
    import sys
    if os.environ.get("CLICOLOR_FORCE", "0") != "0":
        return True
    if os.environ.get("NO_COLOR") or os.environ.get("CLICOLOR") == "0":
        return False
    return sys.stdout.isatty()


def format_alignment_table(aligned: "AlignedSequences", planes, color: bool = False) -> str:
    """Text of print_alignment_table (display.rs:131-181) with its three
    print_scores_table blocks (display.rs:183-220).  `planes` = (insert,
    delete, sub) int64 row-major (n+1, m+1) arrays (AlignmentTable.plane);
    "" when the table is too large to visualise (display.rs:139-144)."""
    a = aligned.s1.sequence.encode()
    b = aligned.s2.sequence.encode()
    x, pa = _buf(a)
    y, pb = _buf(b)
    steps = aligned._steps if aligned._steps is not None else _steps_array(aligned.alignment)
    small = len(a) < DISP_MAX_WIDTH and len(b) < DISP_MAX_WIDTH * 10
    pl = [np.ascontiguousarray(p, dtype=np.int64) for p in planes] if small else [None, None, None]
    ptrs = [p.ctypes.data if p is not None else None for p in pl]
    need = ctypes.c_size_t(0)
    L = lib()
    L.gx_format_table(pa, len(a), pb, len(b), steps.ctypes.data, len(steps), *ptrs, int(color), None, 0,
                      ctypes.byref(need))
    out = ctypes.create_string_buffer(need.value)
    _check(L.gx_format_table(pa, len(a), pb, len(b), steps.ctypes.data, len(steps), *ptrs, int(color), out,
                             need.value, None))
    return out.value.decode("utf-8")


def print_alignment_table(aligned: "AlignedSequences", planes) -> None:
    """print_alignment_table (display.rs:131-181) to stdout."""
    import sys
    sys.stdout.write(format_alignment_table(aligned, planes, _stdout_color()))


def retrace(sequence_container: SequenceContainer, table: AlignmentTable, is_local: bool) -> AlignedSequences:
    """retrace (algo.rs:287-441).  Consumes `table`.  Like the reference
    (algo.rs:438) it ends by printing the sequence table for small inputs
    (tables filled with GX_TABLE_PLANES; set GX_NO_TABLE_PRINT=1 to skip)."""
    a, b = _first_two(sequence_container)
    cap = len(table.s1) + len(table.s2) + 2
    steps = np.zeros(cap, STEP_DTYPE)
    r = CResult()
    small = len(table.s1) < DISP_MAX_WIDTH and len(table.s2) < DISP_MAX_WIDTH * 10
    planes = None
    if small and (table.flags & GX_TABLE_PLANES) and not os.environ.get("GX_NO_TABLE_PRINT"):
        planes = [table.plane(k) for k in range(3)]   # before the table is consumed
    ptr, table.ptr = table.ptr, None
    _check(lib().gx_retrace(ptr, int(is_local), steps.ctypes.data, cap, ctypes.byref(r)))
    out = _aligned(a, b, steps[: r.n_steps], r)
    if planes is not None:
        print_alignment_table(out, planes)
    return out


def _aligned(a: Sequence, b: Sequence, steps: np.ndarray, r: CResult) -> AlignedSequences:
    ch = steps["choice"]
    ii = steps["i"]
    jj = steps["j"]
    alignment = [(AlignmentChoice(int(c)), int(i), int(j)) for c, i, j in zip(ch, ii, jj)]
    return AlignedSequences(a, b, alignment, r.score, r.matches, r.mismatches, r.gap_extensions, r.opening_gaps,
                            (r.start_i, r.start_j), (r.max_cell_i, r.max_cell_j), r.matches_at_max, r.fill_us,
                            r.retrace_us, steps)


def align_raw(s1: bytes, s2: bytes, scores: Scores, is_local: bool, reverse_sequences: bool = False,
              ctx: Optional[Context] = None, max_cell: bool = True):
    """Fused alignment_table + retrace on bytes -> (steps structured array, CResult).
    max_cell: also report alignment_table's max cell / matches_at_max."""
    ctx = ctx or default_context()
    x, px = _buf(s1)
    y, py = _buf(s2)
    cap = len(s1) + len(s2) + 2
    steps = np.zeros(cap, STEP_DTYPE)
    r = CResult()
    _check(lib().gx_align(ctx.ptr, px, len(s1), py, len(s2), ctypes.byref(scores.c()), int(is_local),
                          int(reverse_sequences), GX_ALIGN_MAX_CELL if max_cell else 0, steps.ctypes.data, cap,
                          ctypes.byref(r)))
    return steps[: r.n_steps], r


def align_batch(pairs: Seq[Tuple[bytes, bytes]], scores: Scores, is_local: bool, with_steps: bool = True,
                ctx: Optional[Context] = None, max_cell: bool = True):
    """Many independent pairs in one device launch -> list of (steps, CResult)."""
    ctx = ctx or default_context()
    P = len(pairs)
    keep = [(_buf(a), _buf(b)) for a, b in pairs]
    s1p = (ctypes.c_void_p * P)(*[k[0][1] for k in keep])
    s2p = (ctypes.c_void_p * P)(*[k[1][1] for k in keep])
    n = (ctypes.c_size_t * P)(*[len(a) for a, _ in pairs])
    m = (ctypes.c_size_t * P)(*[len(b) for _, b in pairs])
    res = (CResult * P)()
    steps_arr = [np.zeros(len(a) + len(b) + 2, STEP_DTYPE) for a, b in pairs] if with_steps else None
    stp = (ctypes.c_void_p * P)(*[s.ctypes.data for s in steps_arr]) if with_steps else None
    caps = (ctypes.c_size_t * P)(*[s.size for s in steps_arr]) if with_steps else None
    _check(lib().gx_align_batch(ctx.ptr, s1p, n, s2p, m, P, ctypes.byref(scores.c()), int(is_local),
                                GX_ALIGN_MAX_CELL if max_cell else 0, stp, caps, res))
    out = []
    for p in range(P):
        st = steps_arr[p][: res[p].n_steps] if with_steps else None
        out.append((st, res[p]))
    return out


def align_batch_multi(pairs: Seq[Tuple[bytes, bytes]], scores: Scores, is_local: bool, ctxs: Seq[Context],
                      with_steps: bool = True, max_cell: bool = True):
    """align_batch over several GPUs (gx_align_batch_multi): one context per
    device, the pairs shared out by longest-processing-time on n*m cells, one
    host thread per context -> list of (steps, CResult) in pair order."""
    P = len(pairs)
    keep = [(_buf(a), _buf(b)) for a, b in pairs]
    s1p = (ctypes.c_void_p * P)(*[k[0][1] for k in keep])
    s2p = (ctypes.c_void_p * P)(*[k[1][1] for k in keep])
    n = (ctypes.c_size_t * P)(*[len(a) for a, _ in pairs])
    m = (ctypes.c_size_t * P)(*[len(b) for _, b in pairs])
    res = (CResult * P)()
    steps_arr = [np.zeros(len(a) + len(b) + 2, STEP_DTYPE) for a, b in pairs] if with_steps else None
    stp = (ctypes.c_void_p * P)(*[s.ctypes.data for s in steps_arr]) if with_steps else None
    caps = (ctypes.c_size_t * P)(*[s.size for s in steps_arr]) if with_steps else None
    cp = (ctypes.c_void_p * len(ctxs))(*[c.ptr.value for c in ctxs])
    _check(lib().gx_align_batch_multi(cp, len(ctxs), s1p, n, s2p, m, P, ctypes.byref(scores.c()), int(is_local),
                                      GX_ALIGN_MAX_CELL if max_cell else 0, stp, caps, res))
    return [(steps_arr[p][: res[p].n_steps] if with_steps else None, res[p]) for p in range(P)]


class StagedPairs:
    """Pairs kept resident in HBM for repeated hot-path runs (bench.py)."""

    def __init__(self, pairs: Seq[Tuple[bytes, bytes]], ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.P = len(pairs)
        self._keep = [(_buf(a), _buf(b)) for a, b in pairs]
        self._lens = [(len(a), len(b)) for a, b in pairs]
        s1p = (ctypes.c_void_p * self.P)(*[k[0][1] for k in self._keep])
        s2p = (ctypes.c_void_p * self.P)(*[k[1][1] for k in self._keep])
        n = (ctypes.c_size_t * self.P)(*[len(a) for a, _ in pairs])
        m = (ctypes.c_size_t * self.P)(*[len(b) for _, b in pairs])
        _check(lib().gx_stage_pairs(self.ctx.ptr, s1p, n, s2p, m, self.P))

    def run(self, scores: Scores, is_local: bool, keep_planes: bool = True, max_cell: bool = False,
            steps: int = 1, plane_sums: bool = False, alternate: bool = False, keep: bool = False):
        """`steps` back-to-back passes (pipelined one pass deep when > 1) ->
        (the last pass's results, mean fill ms).  plane_sums: also checksum
        every pass's score planes on the device (self.plane_sums()).
        alternate: pass k runs the k % 2 half of the staged pairs
        (GX_STAGED_ALTERNATE; the halves hold pairs of equal shapes).
        keep: the last pass's planes stay on the device (GX_STAGED_KEEP_PLANES)
        for self.table(p)."""
        res = (CResult * self.P)()
        fms = ctypes.c_double(0)
        flags = ((GX_ALIGN_MAX_CELL if max_cell else 0) | (GX_STAGED_PLANE_SUMS if plane_sums else 0)
                 | (GX_STAGED_ALTERNATE if alternate else 0) | (GX_STAGED_KEEP_PLANES if keep else 0))
        _check(lib().gx_run_staged_steps(self.ctx.ptr, ctypes.byref(scores.c()), int(is_local), int(keep_planes),
                                         flags, int(steps), res, ctypes.byref(fms)))
        return list(res), fms.value

    def table(self, pair: int) -> "AlignmentTable":
        """Staged pair `pair`'s score planes from the last run(keep=True), as
        an AlignmentTable (exports and checksums decode the batch format;
        gx_staged_table).  Its alignment is self.steps(pair)."""
        t = ctypes.c_void_p()
        _check(lib().gx_staged_table(self.ctx.ptr, pair, ctypes.byref(t)))
        (a, _), (b, _) = self._keep[pair]
        n, m = self._lens[pair]
        return AlignmentTable(t, bytes(a[:n]), bytes(b[:m]), GX_TABLE_PLANES)

    def plane_sums(self) -> np.ndarray:
        """uint64 [passes, pairs, 3] plane checksums of the last run(plane_sums=True)."""
        n = ctypes.c_size_t(0)
        _check(lib().gx_staged_plane_sums(self.ctx.ptr, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint64)
        _check(lib().gx_staged_plane_sums(self.ctx.ptr, out.ctypes.data, out.size, ctypes.byref(n)))
        return out[: n.value].reshape(-1, self.P, 3)

    def pass_results(self) -> List[List["CResult"]]:
        """Every pass's per-pair results of the last run, [pass][pair] (gx_staged_pass_results)."""
        n = ctypes.c_size_t(0)
        _check(lib().gx_staged_pass_results(self.ctx.ptr, None, 0, ctypes.byref(n)))
        out = (CResult * max(n.value, 1))()
        _check(lib().gx_staged_pass_results(self.ctx.ptr, out, n.value, ctypes.byref(n)))
        rows = list(out)[: n.value]
        return [rows[k * self.P:(k + 1) * self.P] for k in range(n.value // max(self.P, 1))]

    def steps(self, pair: int) -> np.ndarray:
        """The alignment of staged pair `pair` from the last pass of the last run (STEP_DTYPE array)."""
        n = ctypes.c_size_t(0)
        _check(lib().gx_staged_steps(self.ctx.ptr, pair, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), STEP_DTYPE)
        _check(lib().gx_staged_steps(self.ctx.ptr, pair, out.ctypes.data, out.size, ctypes.byref(n)))
        return out[: n.value]


# ---------------------------------------------------------------------------
# all-vs-all (BASELINE config 4)

def lpt_partition(weights: Seq[float], parts: int) -> List[List[int]]:
    """Longest-processing-time assignment of items (weight = n*m cells) to
    `parts` GPUs; each bin sorted.  Deterministic, so every rank computes the
    same plan without communicating."""
    order = sorted(range(len(weights)), key=lambda k: (-weights[k], k))
    bins: List[List[int]] = [[] for _ in range(parts)]
    load = [0.0] * parts
    for k in order:
        b = min(range(parts), key=lambda x: (load[x], x))
        bins[b].append(k)
        load[b] += weights[k]
    return [sorted(b) for b in bins]


def all_pairs(k: int, with_self: bool = True) -> List[Tuple[int, int]]:
    """(i, j) with i <= j (i < j without self pairs), in the reference compare
    matrix's fill order: row j, column i (main.rs:253-264)."""
    return [(i, j) for j in range(k) for i in range(j + 1) if i < j or with_self]


PAIR_FIELDS = ("score", "matches", "mismatches", "gap_extensions", "opening_gaps", "n_steps")


def _batch_stats(pairs, scores, is_local, ctx):
    """Product aligner for one rank's share: one gx_align_batch launch."""
    res = align_batch(pairs, scores, is_local, with_steps=False, ctx=ctx, max_cell=False)
    return [[getattr(r, f) for f in PAIR_FIELDS] for _, r in res]


def _pack(seqs: List[bytes]):
    lens = np.array([len(s) for s in seqs], np.int64)
    buf = np.frombuffer(b"".join(seqs), np.uint8) if lens.sum() else np.zeros(0, np.uint8)
    return lens, buf


def _broadcast_bytes_list(dist, items, device: str) -> List[bytes]:
    """Rank 0's list of byte strings on every rank (count + lengths, then the
    packed bytes: three broadcasts)."""
    import torch
    meta = torch.zeros(2, dtype=torch.int64, device=device)
    if dist.get_rank() == 0:
        lens, buf = _pack(items)
        meta[0], meta[1] = len(items), int(lens.sum())
    dist.broadcast(meta, 0)
    k, tot = int(meta[0]), int(meta[1])
    tl = torch.zeros(max(k, 1), dtype=torch.int64, device=device)
    tb = torch.zeros(max(tot, 1), dtype=torch.uint8, device=device)
    if dist.get_rank() == 0:
        if k:
            tl[:k].copy_(torch.from_numpy(lens))
        if tot:
            tb[:tot].copy_(torch.from_numpy(buf.copy()))
    dist.broadcast(tl, 0)
    dist.broadcast(tb, 0)
    lens = tl.cpu().numpy()[:k]
    raw = tb.cpu().numpy().tobytes()
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [raw[int(offs[x]):int(offs[x + 1])] for x in range(k)]


def all_vs_all(sequence_container: SequenceContainer, scores: Scores, is_local: bool = False,
               with_self: bool = True, ctx: Optional[Context] = None, dist=None, device: str = "cpu",
               align_fn=None) -> dict:
    """Align every pair (i <= j) of the container's sequences.

    dist = None: one GPU (ctx), one batched launch.  dist = torch.distributed
    (one process per GPU): rank 0's container is broadcast to every rank (the
    scatter; ≈30 KB per genome), each rank aligns its longest-processing-time
    share of the pairs, and the fixed-size per-pair records are all-gathered
    (RCCL over xGMI for backend "nccl", `device` = "cuda"; gloo on CPU).  No
    collective touches the DP data.  align_fn(pairs, scores, is_local) -> rows
    replaces the GPU aligner (tests of the plumbing only).

    Returns {"names", "lengths", "pairs", "records"}: records[p] = PAIR_FIELDS
    of pairs[p]; matrix(...) renders the reference's TSV layout."""
    align_fn = align_fn or (lambda prs, sc, loc: _batch_stats(prs, sc, loc, ctx or default_context()))
    seqs = [s.sequence.encode() for s in sequence_container.sequences]
    names = [s.name for s in sequence_container.sequences]
    if dist is not None:
        rank, world = dist.get_rank(), dist.get_world_size()
        # scatter: broadcast rank 0's packed sequences and names (utf-8)
        seqs = _broadcast_bytes_list(dist, seqs if rank == 0 else None, device)
        names = [x.decode("utf-8") for x in
                 _broadcast_bytes_list(dist, [x.encode("utf-8") for x in names] if rank == 0 else None, device)]
    else:
        rank, world = 0, 1
    pairs = all_pairs(len(seqs), with_self)
    weights = [float(len(seqs[i])) * len(seqs[j]) for i, j in pairs]
    mine = lpt_partition(weights, world)[rank]
    rows = align_fn([(seqs[pairs[p][0]], seqs[pairs[p][1]]) for p in mine], scores, is_local) if mine else []
    local = np.array([[p] + list(r) for p, r in zip(mine, rows)], np.int64).reshape(-1, 1 + len(PAIR_FIELDS))
    if dist is not None:
        import torch
        # gather: fixed-size records, padded to the largest share
        cap = max(len(b) for b in lpt_partition(weights, world))
        t = torch.full((cap, local.shape[1]), -1, dtype=torch.int64, device=device)
        if len(local):
            t[: len(local)].copy_(torch.from_numpy(local))
        parts = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        local = np.concatenate([x.cpu().numpy() for x in parts])
        local = local[local[:, 0] >= 0]
    records: List[Optional[List[int]]] = [None] * len(pairs)
    for row in local:
        records[int(row[0])] = [int(x) for x in row[1:]]
    if any(r is None for r in records):
        raise GxError(1, "all_vs_all: missing pair records after gather")
    return {"names": names, "lengths": [len(s) for s in seqs], "pairs": pairs, "records": records}


def similarity_tsv(result: dict, field: str = "score", blank_header: bool = False) -> str:
    """The reference compare writer's layout (main.rs:333-359): a header row of
    sequence indices, then row r = "r\\t" + one value per column; cells (r, c)
    with c <= r hold the pair's value, the rest 0 (never computed)."""
    k = len(result["lengths"])
    f = PAIR_FIELDS.index(field)
    cell = {(j, i): rec[f] for (i, j), rec in zip(result["pairs"], result["records"])}
    out = [(" \t" if blank_header else "\t") + "".join(f"{i}\t" for i in range(k)) + "\n"]
    for r in range(k):
        out.append(f"{r}\t" + "".join(f"{cell.get((r, c), 0)}\t" for c in range(k)) + "\n")
    return "".join(out)


# ---------------------------------------------------------------------------
# compare mode (main.rs:216-379)

def common_substring_host(a: bytes, b: bytes) -> Tuple[int, int, int]:
    """get_lcs(0, 1) (tree.rs:218-281) of a then b on the host solver, no device: (i, j, L)."""
    ka, pa = _buf(a)
    kb, pb = _buf(b)
    i, j, n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().gx_common_substring_host(pa, len(a), pb, len(b), ctypes.byref(i), ctypes.byref(j), ctypes.byref(n)))
    return i.value, j.value, n.value


def common_substring_candidates_host(a: bytes, b: bytes) -> Tuple[int, int]:
    """(L, number of (i, j) starts of common substrings of length L), host solver."""
    ka, pa = _buf(a)
    kb, pb = _buf(b)
    n, c = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().gx_common_substring_candidates_host(pa, len(a), pb, len(b), ctypes.byref(n), ctypes.byref(c)))
    return n.value, c.value


def common_substring(a: bytes, b: bytes, ctx: Optional["Context"] = None) -> Tuple[int, int, int]:
    """get_lcs(0, 1) of a then b on the GPU: (i, j, L)."""
    ctx = ctx or default_context()
    ka, pa = _buf(a)
    kb, pb = _buf(b)
    i, j, n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().gx_common_substring(ctx.ptr, pa, len(a), pb, len(b), ctypes.byref(i), ctypes.byref(j),
                                     ctypes.byref(n)))
    return i.value, j.value, n.value


def compare_pair(a: bytes, b: bytes, ctx: Optional["Context"] = None, host: bool = False) -> Tuple[int, int, int]:
    """One similarity-matrix element (main.rs:281-315): (score, first_lcs, get_matches calls).
    host=True runs the recursion on the host solver with no device."""
    ptr = None if host else (ctx or default_context()).ptr
    ka, pa = _buf(a)
    kb, pb = _buf(b)
    cell, calls = CCompareCell(), ctypes.c_uint64()
    _check(lib().gx_compare_pair(ptr, pa, len(a), pb, len(b), ctypes.byref(cell), ctypes.byref(calls)))
    return cell.score, cell.first_lcs, calls.value


def compare_matrix(seqs: Seq[bytes], ctx: Optional["Context"] = None, host: bool = False) -> np.ndarray:
    """The similarity matrix (main.rs:241-316) as uint64 [nseq][nseq][4]: element [j][i], i <= j, holds
    (score, len_i, len_j, first_lcs); the other half is zero."""
    ptr = None if host else (ctx or default_context()).ptr
    k = len(seqs)
    keep = [_buf(s) for s in seqs]
    ptrs = (ctypes.c_void_p * max(k, 1))(*[p for _, p in keep])
    lens = (ctypes.c_size_t * max(k, 1))(*[len(s) for s in seqs])
    out = np.zeros((k, k, 4), np.uint64)
    _check(lib().gx_compare_matrix(ptr, ptrs, lens, k, out.ctypes.data))
    return out


def compare_info(ctx: Optional["Context"] = None) -> dict:
    """gx_compare_info / gx_compare_batches / gx_compare_run_stats of the last compare call on ctx."""
    ctx = ctx or default_context()
    v = [ctypes.c_uint64() for _ in range(6)]
    ms = ctypes.c_double()
    _check(lib().gx_compare_info(ctx.ptr, *[ctypes.byref(x) for x in v[:4]]))
    _check(lib().gx_compare_run_stats(ctx.ptr, ctypes.byref(v[4]), ctypes.byref(ms)))
    _check(lib().gx_compare_batches(ctx.ptr, ctypes.byref(v[5])))
    return {"gpu_subproblems": v[0].value, "host_subproblems": v[1].value, "overflowed": v[2].value,
            "levels": v[3].value, "batches": v[5].value, "byte_compares": v[4].value, "run_ms": ms.value}


def compare_segment_height() -> int:
    """Rows per segment of the run kernel's tiles (gx_compare_segment_height)."""
    return lib().gx_compare_segment_height()


# ---------------------------------------------------------------------------
# suffix-tree mode (main.rs:154-215)

@dataclass
class TreeStats:
    """TreeStats (tree.rs:30-39); string_depth_sum is the numerator of the average."""
    num_internal: int = 0
    num_leaves: int = 0
    num_nodes: int = 0
    average_string_depth: float = 0.0
    max_string_depth: int = 0
    bwt: str = ""
    longest_repeat_len: int = 0
    longest_repeat_start: int = 0
    string_depth_sum: int = 0

    def _c(self) -> CSuffixStats:
        return CSuffixStats(self.num_internal, self.num_leaves, self.num_nodes, self.string_depth_sum,
                            self.max_string_depth, self.longest_repeat_start, self.longest_repeat_len)

    def __str__(self):  # display.rs:8-38
        return format_suffix_stats(self._c(), self.bwt.encode("latin-1"))


def format_suffix_stats(st: CSuffixStats, bwt: bytes) -> str:
    """Display for TreeStats (gx_format_suffix_stats)."""
    kb, pb = _buf(bwt)
    need = ctypes.c_size_t()
    rc = lib().gx_format_suffix_stats(ctypes.byref(st), pb, len(bwt), None, 0, ctypes.byref(need))
    if rc not in (0, 7):
        _check(rc)
    out = ctypes.create_string_buffer(need.value)
    _check(lib().gx_format_suffix_stats(ctypes.byref(st), pb, len(bwt), out, need.value, None))
    return out.value.decode("latin-1")


def suffix_tree_stats(seq: bytes, ctx: Optional["Context"] = None, want: Seq[str] = ("bwt",),
                      host: bool = False) -> dict:
    """compute_stats(0) on a tree holding seq (gx_suffix_tree_stats): a dict with "stats" (TreeStats,
    its bwt filled when wanted), "raw" (CSuffixStats) and each of "bwt" (bytes), "sa", "lcp" (uint32
    arrays of len(seq) + 1) named in `want`.  host=True: the host solver, no device."""
    ptr = None if host else (ctx or default_context()).ptr
    ks, ps = _buf(seq)
    N = len(seq) + 1
    arr = {k: np.zeros(N, np.uint8 if k == "bwt" else np.uint32) for k in ("bwt", "sa", "lcp") if k in want}
    raw = CSuffixStats()
    _check(lib().gx_suffix_tree_stats(ptr, ps, len(seq), ctypes.byref(raw),
                                      *[arr[k].ctypes.data if k in arr else None for k in ("bwt", "sa", "lcp")]))
    out = {"raw": raw}
    if "bwt" in arr:
        out["bwt"] = arr.pop("bwt").tobytes()
    out.update(arr)
    avg = raw.string_depth_sum / raw.num_internal if raw.num_internal else float("nan")   # 0 / 0 (tree.rs:801)
    out["stats"] = TreeStats(raw.num_internal, raw.num_leaves, raw.num_nodes, avg, raw.max_string_depth,
                             out.get("bwt", b"").decode("latin-1"), raw.longest_repeat_len,
                             raw.longest_repeat_start, raw.string_depth_sum)
    return out


def suffix_info(ctx: Optional["Context"] = None) -> dict:
    """gx_suffix_info of the last suffix-tree call on ctx (all zero: the host solver answered), and
    "digit_passes": the radix passes on key bits 8p .. 8p+7 for p = 0 .. 7, round 0 (text keys, as a rule
    one pass on every digit) included (gx_suffix_digit_passes)."""
    ctx = ctx or default_context()
    r, p = ctypes.c_uint64(), ctypes.c_uint64()
    ms = [ctypes.c_double() for _ in range(3)]
    _check(lib().gx_suffix_info(ctx.ptr, ctypes.byref(r), ctypes.byref(p), *[ctypes.byref(x) for x in ms]))
    digits = (ctypes.c_uint64 * 8)()
    _check(lib().gx_suffix_digit_passes(ctx.ptr, digits))
    return {"doubling_rounds": r.value, "sort_passes": p.value, "sort_ms": ms[0].value, "lcp_ms": ms[1].value,
            "fold_ms": ms[2].value, "digit_passes": list(digits)}


def suffix_tile() -> Tuple[int, int, int]:
    """(T, C, B) of gx_suffix_tile: sort items per workgroup, LCP chunk, fold block."""
    v = [ctypes.c_int() for _ in range(3)]
    _check(lib().gx_suffix_tile(*[ctypes.byref(x) for x in v]))
    return v[0].value, v[1].value, v[2].value


# ---------------------------------------------------------------------------
# search mode (no counterpart in the reference)

HIT_DTYPE = np.dtype([("lo", "<u4"), ("count", "<u4"), ("prefix_len", "<u4"), ("prefix_pos", "<u4")])
APPROX_HIT_DTYPE = np.dtype([("count", "<u4"), ("best_dist", "<u4"), ("best_pos", "<u4"), ("candidates", "<u4")])
EDIT_HIT_DTYPE = np.dtype([("count", "<u4"), ("best_dist", "<u4"), ("best_end", "<u4"), ("candidates", "<u4")])
MATCH_STAT_DTYPE = np.dtype([("len", "<u4"), ("lo", "<u4"), ("count", "<u4"), ("pos", "<u4")])
MEM_DTYPE = np.dtype([("qpos", "<u4"), ("tpos", "<u4"), ("len", "<u4")])
EXTEND_HIT_DTYPE = np.dtype([("score", "<i4"), ("n_steps", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"),
                             ("opening_gaps", "<u4"), ("gap_extensions", "<u4"), ("identities", "<u4"),
                             ("cigar_len", "<u4")])
CHAIN_DTYPE = np.dtype([("member_off", "<u8"), ("score", "<i4"), ("n_anchors", "<u4"), ("root", "<u4"), ("end", "<u4"),
                        ("qstart", "<u4"), ("tstart", "<u4"), ("qend", "<u4"), ("tend", "<u4")])
CHAIN_NONE = 0xFFFFFFFF     # GX_CHAIN_NONE: pred of a root
CHAIN_MAX_PRED = 256        # GX_CHAIN_MAX_PRED
CHAIN_DEFAULTS = {"w_match": 8, "w_drift": 1, "max_gap": 5000, "max_drift": 500, "max_pred": 64,
                  "min_score": 0}   # GX_CHAIN_DEFAULT_*
EXTEND_MAX_BAND = 15        # GX_EXTEND_MAX_BAND
EXTEND_MAX_SCORE = 32767    # GX_EXTEND_MAX_SCORE
CIGAR_OPS = "MID"           # a run is len << 4 | op
APPROX_MAX_K = 8        # GX_APPROX_MAX_K
EDIT_MAX_M = 4096       # GX_EDIT_MAX_M
NO_DIST = 0xFFFFFFFF    # best_dist of a pattern without an occurrence
ALL_HITS = 0xFFFFFFFF   # max_hits: every occurrence
_FIRST_CAP = 1 << 22    # positions asked for before the count is known (GX_ECAP names the rest)
_FIRST_RUNS = 8         # CIGAR runs a hit asked for before the count is known: a hit within three edits has at most seven
STRANDS = {"forward": 1, "reverse": 2, "both": 3}   # GX_STRAND_FWD, GX_STRAND_REV, GX_STRAND_BOTH
STRAND_PAD = 16         # GX_STRAND_PAD


def _strands(strands) -> int:
    """GX_STRAND_* of "forward", "reverse" or "both"; a number is handed to the library as it is."""
    if isinstance(strands, str):
        if strands not in STRANDS:
            raise GxError(1, f"strands is {strands!r}, not 'forward', 'reverse' or 'both'")
        return STRANDS[strands]
    return int(strands)


def _strand_items(result: dict, npat: int, s: int) -> dict:
    """With anything but the forward strand alone: the caller's pattern and the strand (0 forward, 1 reverse)
    of every item, beside the result's per-item arrays."""
    if s != 1:
        result["pattern"] = np.tile(np.arange(npat, dtype=np.uint32), 2 if s == 3 else 1)
        result["strand"] = np.repeat(np.array([0, 1] if s == 3 else [1], np.uint8), npat)
    return result


def revcomp(b: bytes) -> bytes:
    """gx_revcomp: the reverse complement of b over IUPAC in both cases; every other byte is its own complement."""
    src = np.frombuffer(bytes(b), np.uint8)
    dst = np.zeros(max(src.size, 1), np.uint8)
    _check(lib().gx_revcomp(src.ctypes.data if src.size else None, src.size, dst.ctypes.data))
    return dst[:src.size].tobytes()


def revcomp_batch(patterns, strands="both", ctx: Optional["Context"] = None, pad: bool = False,
                  cap: Optional[int] = None):
    """gx_revcomp_batch: the item batch of `patterns` (as for SuffixIndex.search) on `strands`, exactly as the
    stranded searches stage it: (packed uint8, offsets uint64 of items + 1).  With a context it is staged on the
    device and copied back; ctx=None builds it on the host.  pad=True also returns the STRAND_PAD bytes staged
    behind the items.  cap: the capacity handed to the call (None: what it needs)."""
    s = _strands(strands)
    packed, off, n = SuffixIndex._batch(patterns)
    items = n * (2 if s == 3 else 1)
    total = int(off[-1]) * (2 if s == 3 else 1)
    want = total + (STRAND_PAD if pad else 0) if cap is None else cap
    out = np.zeros(max(want, 1), np.uint8)
    ooff = np.zeros(items + 1, np.uint64)
    _check(lib().gx_revcomp_batch(ctx.ptr if ctx else None, packed.ctypes.data, off.ctypes.data, n, s, out.ctypes.data,
                                  want, ooff.ctypes.data))
    return out[:min(want, total + (STRAND_PAD if pad else 0))], ooff


def strand_info(ctx: Optional["Context"] = None) -> dict:
    """gx_strand_info of the last search-mode call on ctx: the items it staged, the reverse bytes the kernel
    wrote and that kernel's device ms."""
    ctx = ctx or default_context()
    v = [ctypes.c_uint64() for _ in range(2)]
    ms = ctypes.c_double()
    _check(lib().gx_strand_info(ctx.ptr, ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(ms)))
    return {"items": v[0].value, "rc_bytes": v[1].value, "rc_ms": ms.value}


class SuffixIndex:
    """The suffix index of seq (gx_suffix_index): with a context, text and suffix array stay on the
    device until close() and every search runs there; host=True keeps both on the host (no device).
    Close it before its context."""

    def __init__(self, seq: bytes, ctx: Optional["Context"] = None, host: bool = False):
        self.ptr = None
        self._ctx = None if host else (ctx or default_context())
        ks, ps = _buf(seq)
        p = ctypes.c_void_p()
        _check(lib().gx_suffix_index_build(self._ctx.ptr if self._ctx else None, ps, len(seq), ctypes.byref(p)))
        self.ptr = p
        self.n = len(seq)

    @staticmethod
    def _batch(patterns):
        """(packed uint8, offsets uint64, npat) of a sequence of bytes or a (packed, offsets) pair."""
        if isinstance(patterns, tuple):
            packed, off = patterns
            packed = np.ascontiguousarray(np.frombuffer(packed, np.uint8) if isinstance(packed, (bytes, bytearray))
                                          else packed, np.uint8)
            off = np.ascontiguousarray(off, np.uint64)
        else:
            packed = np.frombuffer(b"".join(patterns), np.uint8)
            off = np.zeros(len(patterns) + 1, np.uint64)
            np.cumsum(np.fromiter((len(x) for x in patterns), np.uint64, len(patterns)), out=off[1:])
        if packed.size == 0:
            packed = np.zeros(1, np.uint8)
        return packed, off, len(off) - 1

    def _grown(self, npat: int, max_hits: int, hoff, call):
        """The two-try GX_ECAP loop of the three searches: call(cap) allocates its output arrays of cap entries,
        makes the call with hit_offsets = hoff and returns (rc, arrays).  A first capacity that is too small
        comes back as GX_ECAP with hoff complete, so its last entry is the capacity of the second try.
        Returns the arrays of the call that succeeded."""
        cap = max(1, min(npat * min(max_hits, self.n + 1), _FIRST_CAP))
        for _ in range(2):
            rc, out = call(cap)
            if rc != 7:
                break
            cap = int(hoff[-1])   # GX_ECAP: hit_offsets is complete; allocate and repeat
        _check(rc)
        return out

    def search(self, patterns, max_hits: int = 0, strands="forward") -> dict:
        """gx_suffix_index_search for a batch: `patterns` is a sequence of bytes, or (packed, offsets) with
        pattern p = packed[offsets[p]:offsets[p + 1]].  Returns uint32 arrays "lo", "count", "prefix_len",
        "prefix_pos" (one entry per pattern) and, with max_hits > 0, "positions" (the first
        min(count, max_hits) suffix-array entries of each pattern's interval, ascending) and "hit_offsets"
        (uint64, npat + 1).  max_hits = ALL_HITS reports every occurrence.
        strands: "forward", "reverse" or "both" (gx_suffix_index_search_strands): every per-pattern array then
        has one entry per item of the item batch (revcomp_batch), and "pattern" and "strand" (0 forward,
        1 reverse) name each item's.  Positions are the forward text's."""
        packed, off, ncall = self._batch(patterns)
        sc = _strands(strands)
        npat = ncall * (2 if sc == 3 else 1)   # the items
        hits = np.zeros(npat, HIT_DTYPE)
        out = None
        if max_hits <= 0:
            _check(lib().gx_suffix_index_search_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc,
                                                        hits.ctypes.data, 0, None, 0, None))
        else:
            hoff = np.zeros(npat + 1, np.uint64)

            def call(cap):
                pos = np.zeros(cap, np.uint32)
                return lib().gx_suffix_index_search_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc,
                                                            hits.ctypes.data, max_hits, pos.ctypes.data, cap,
                                                            hoff.ctypes.data), pos

            pos = self._grown(npat, max_hits, hoff, call)
            out = {"positions": pos[:int(hoff[-1])], "hit_offsets": hoff}
        r = {k: np.ascontiguousarray(hits[k]) for k in ("lo", "count", "prefix_len", "prefix_pos")}
        if out:
            r.update(out)
        return _strand_items(r, ncall, sc)

    def search_approx(self, patterns, k: int, max_hits: int = 0, strands="forward") -> dict:
        """gx_suffix_index_search_approx for a batch (`patterns` as for search): every start where a pattern
        matches with at most k substitutions (0 <= k <= APPROX_MAX_K, every pattern of k + 1 bytes or more).
        Returns uint32 arrays "count", "best_dist" (NO_DIST without an occurrence), "best_pos", "candidates"
        and, with max_hits > 0, "positions" (ascending per pattern), "distances" (uint8, beside them) and
        "hit_offsets" (uint64, npat + 1).  max_hits = ALL_HITS reports every occurrence.  strands: as for search."""
        packed, off, ncall = self._batch(patterns)
        sc = _strands(strands)
        npat = ncall * (2 if sc == 3 else 1)   # the items
        hits = np.zeros(npat, APPROX_HIT_DTYPE)
        out = None
        if max_hits <= 0:
            _check(lib().gx_suffix_index_search_approx_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc, k,
                                                               hits.ctypes.data, 0, None, None, 0, None))
        else:
            hoff = np.zeros(npat + 1, np.uint64)

            def call(cap):
                pos, dst = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
                return lib().gx_suffix_index_search_approx_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc,
                                                                   k, hits.ctypes.data, max_hits, pos.ctypes.data,
                                                                   dst.ctypes.data, cap, hoff.ctypes.data), (pos, dst)

            pos, dst = self._grown(npat, max_hits, hoff, call)
            out = {"positions": pos[:int(hoff[-1])], "distances": dst[:int(hoff[-1])], "hit_offsets": hoff}
        r = {f: np.ascontiguousarray(hits[f]) for f in ("count", "best_dist", "best_pos", "candidates")}
        if out:
            r.update(out)
        return _strand_items(r, ncall, sc)

    def search_edit(self, patterns, k: int, max_hits: int = 0, starts: bool = True, strands="forward") -> dict:
        """gx_suffix_index_search_edit for a batch (`patterns` as for search): every end e where a pattern
        matches a window s[b:e] with at most k substitutions, insertions and deletions (0 <= k <= APPROX_MAX_K,
        every pattern of k + 1 to EDIT_MAX_M bytes).  Returns uint32 arrays "count", "best_dist" (NO_DIST
        without an occurrence), "best_end", "candidates" and, with max_hits > 0, "ends" (each pattern's
        smallest ends, ascending), "distances" (uint8), "starts" (the shortest window's; None with
        starts=False) and "hit_offsets" (uint64, npat + 1).  max_hits = ALL_HITS reports every occurrence.
        strands: as for search; ends and starts are the forward text's."""
        packed, off, ncall = self._batch(patterns)
        sc = _strands(strands)
        npat = ncall * (2 if sc == 3 else 1)   # the items
        hits = np.zeros(npat, EDIT_HIT_DTYPE)
        out = None
        if max_hits <= 0:
            _check(lib().gx_suffix_index_search_edit_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc, k,
                                                             hits.ctypes.data, 0, None, None, None, 0, None))
        else:
            hoff = np.zeros(npat + 1, np.uint64)

            def call(cap):
                end, dst = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
                sta = np.zeros(cap, np.uint32) if starts else None
                return lib().gx_suffix_index_search_edit_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc, k,
                                                                 hits.ctypes.data, max_hits, end.ctypes.data,
                                                                 dst.ctypes.data, sta.ctypes.data if starts else None, cap,
                                                                 hoff.ctypes.data), (end, dst, sta)

            end, dst, sta = self._grown(npat, max_hits, hoff, call)
            tot = int(hoff[-1])
            out = {"ends": end[:tot], "distances": dst[:tot], "starts": sta[:tot] if starts else None,
                   "hit_offsets": hoff}
        r = {f: np.ascontiguousarray(hits[f]) for f in ("count", "best_dist", "best_end", "candidates")}
        if out:
            r.update(out)
        return _strand_items(r, ncall, sc)

    def matching_stats(self, queries, max_len: int = 65535, strands="forward") -> dict:
        """gx_suffix_index_match_stats for a batch of long queries (`queries` as `patterns` of search, of any
        length): for every position of every query the longest prefix of its window (max_len bytes at most)
        that occurs in the text.  Returns uint32 arrays "len", "lo", "count", "pos" (one entry per query
        position; query c's are at offsets[c]:offsets[c + 1]) and "offsets" (uint64, nq + 1).
        strands: as for search; "offsets" are then the items', and a reverse item's positions are those of the
        query's reverse complement (the same bases begin at m - position - len in the query)."""
        packed, off, nq = self._batch(queries)
        sc = _strands(strands)
        if sc == 3:
            off_items = np.concatenate([off, off[-1] + off[1:]])
        else:
            off_items = off
        st = np.zeros(int(off_items[-1]), MATCH_STAT_DTYPE)
        _check(lib().gx_suffix_index_match_stats_strands(self.ptr, packed.ctypes.data, off.ctypes.data, nq, sc, max_len,
                                                         st.ctypes.data if st.size else None))
        r = {f: np.ascontiguousarray(st[f]) for f in ("len", "lo", "count", "pos")}
        r["offsets"] = off_items
        return _strand_items(r, nq, sc)

    def mems(self, queries, min_len: int, max_mems: Optional[int] = None, strands="forward") -> dict:
        """gx_suffix_index_mems for a batch of long queries: every maximal exact match of min_len bytes or
        more between a query and the text.  Returns uint32 arrays "qpos", "tpos", "length" (query c's MEMs at
        mem_offsets[c]:mem_offsets[c + 1], ordered by qpos, then tpos), "mem_offsets" (uint64, nq + 1) and
        "candidates" (uint64, the pairs examined per query).  max_mems=0 asks for the counts only (empty
        triples); None makes two calls, the counts first and then the exact capacity; a number is the
        capacity of one call (GxError 7 when it is too small).
        strands: as for search; a reverse item's qpos is a position of the query's reverse complement (the same
        bases begin at m - qpos - length in the query), tpos is the forward text's."""
        packed, off, ncall = self._batch(queries)
        sc = _strands(strands)
        nq = ncall * (2 if sc == 3 else 1)   # the items
        moff, cand = np.zeros(nq + 1, np.uint64), np.zeros(nq, np.uint64)

        def call(mem, cap):
            _check(lib().gx_suffix_index_mems_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc, min_len,
                                                      mem.ctypes.data if mem is not None else None, cap, moff.ctypes.data,
                                                      cand.ctypes.data if nq else None))

        mem = np.zeros(0, MEM_DTYPE)
        if max_mems is None or max_mems <= 0:
            call(None, 0)
            if max_mems is None and int(moff[-1]):
                mem = np.zeros(int(moff[-1]), MEM_DTYPE)
                call(mem, mem.size)
        else:
            mem = np.zeros(max_mems, MEM_DTYPE)
            call(mem, max_mems)
            mem = mem[:int(moff[-1])]
        return _strand_items({"qpos": np.ascontiguousarray(mem["qpos"]), "tpos": np.ascontiguousarray(mem["tpos"]),
                              "length": np.ascontiguousarray(mem["len"]), "mem_offsets": moff, "candidates": cand},
                             ncall, sc)

    def chain_mems(self, queries, min_len: int, strands="forward", **params) -> dict:
        """mems(queries, min_len), then chain_anchors on its result where the index lives (the device of a
        device index, the host solver of a host index): {"mems": the one, "chains": the other}.
        strands: as for mems; every item's anchors are chained as they are, a reverse item being one more query."""
        m = self.mems(queries, min_len, strands=strands)
        return {"mems": m, "chains": chain_anchors(m, ctx=self._ctx, host=self._ctx is None, **params)}

    def extend(self, reads, hits, scores: Optional["Scores"] = None, band: Optional[int] = None,
               cigars: bool = True, strands="forward") -> dict:
        """gx_suffix_index_extend: the reference's global alignment (alignment_table, then retrace) of every
        hit's window s[start:end] (s1) with its read (s2) on the cells |j - i| <= band.  `reads` as `patterns`
        of search; `hits` is a search_edit result or any mapping with "hit_offsets", "starts" and "ends"
        (read p's hits at hit_offsets[p]:hit_offsets[p + 1]).  band=None takes the largest |window - read|
        over the hits (0 <= band <= EXTEND_MAX_BAND).  Returns the record fields as arrays ("score" int32;
        "n_steps", "matches", "mismatches", "opening_gaps", "gap_extensions", "identities", "cigar_len"
        uint32, one entry per hit: views of the one record array the call filled, which a batch of millions
        of hits would take longer to take apart than to align), "cigar_offsets" (uint64, hits + 1) and, with
        cigars, "cigar" (uint32
        runs len << 4 | op, M = 0, I = 1, D = 2, in read order; hit h's at cigar_offsets[h]:cigar_offsets[h + 1];
        None with cigars=False).
        strands: as for search; `hits` then has the hits of every item of the item batch (what search_edit
        returns with the same strands), and a reverse item's hits are aligned against the read's reverse
        complement, CIGAR in that order: what SAM reports for a reverse-strand read."""
        packed, off, ncall = self._batch(reads)
        sc_ = _strands(strands)
        npat = ncall * (2 if sc_ == 3 else 1)   # the items
        hoff = np.ascontiguousarray(hits["hit_offsets"], np.uint64)
        sta = np.ascontiguousarray(hits["starts"], np.uint32)
        end = np.ascontiguousarray(hits["ends"], np.uint32)
        if hoff.size != npat + 1:
            raise GxError(1, f"hit_offsets has {hoff.size} entries for {npat} reads")
        nh = int(hoff[-1])
        if sta.size < nh or end.size < nh:
            raise GxError(1, f"starts and ends have {sta.size} and {end.size} entries for {nh} hits")
        if band is None:
            lens = np.tile(np.diff(off).astype(np.int64), 2 if sc_ == 3 else 1)
            m = np.repeat(lens, np.diff(hoff).astype(np.int64)) if nh else np.zeros(0, np.int64)
            band = int(np.abs(end[:nh].astype(np.int64) - sta[:nh].astype(np.int64) - m).max()) if nh else 0
        sc = (scores or Scores()).c()
        out = np.zeros(max(nh, 1), EXTEND_HIT_DTYPE)
        coff = np.zeros(nh + 1, np.uint64)
        cig = None

        def call(cap):
            nonlocal cig
            cig = np.zeros(max(cap, 1), np.uint32) if cigars else None
            return lib().gx_suffix_index_extend_strands(self.ptr, packed.ctypes.data, off.ctypes.data, ncall, sc_,
                                                        hoff.ctypes.data, sta.ctypes.data, end.ctypes.data,
                                                        ctypes.byref(sc), band, out.ctypes.data,
                                                        cig.ctypes.data if cigars else None, cap, coff.ctypes.data)

        rc = call(_FIRST_RUNS * nh)
        if rc == 7:
            rc = call(int(coff[-1]))   # GX_ECAP: cigar_offsets is complete; allocate and repeat
        _check(rc)
        r = {f: out[f][:nh] for f in EXTEND_HIT_DTYPE.names}
        r["cigar_offsets"] = coff
        r["cigar"] = cig[:int(coff[-1])] if cigars else None
        return _strand_items(r, ncall, sc_)

    def map_reads(self, reads, k: int, max_hits: int = 16, scores: Optional["Scores"] = None,
                  band: Optional[int] = None, strands="forward") -> Tuple[dict, dict]:
        """search_edit(reads, k, max_hits) with starts, then extend of what it reports (band=None: k).
        Returns both results.  strands: handed to both calls (as for search)."""
        found = self.search_edit(reads, k, max_hits, starts=True, strands=strands)
        return found, self.extend(reads, found, scores, k if band is None else band, strands=strands)

    def sa(self) -> np.ndarray:
        """The suffix array, n + 1 entries (gx_suffix_index_export)."""
        a = np.zeros(self.n + 1, np.uint32)
        _check(lib().gx_suffix_index_export(self.ptr, a.ctypes.data))
        return a

    def info(self) -> dict:
        n, dev, b = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_uint64()
        _check(lib().gx_suffix_index_info(self.ptr, ctypes.byref(n), ctypes.byref(dev), ctypes.byref(b)))
        return {"n": n.value, "on_device": bool(dev.value), "device_bytes": b.value}

    def close(self):
        if self.ptr:
            lib().gx_suffix_index_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if self._ctx is None or self._ctx.ptr:   # (a device index does not outlive its context)
                self.close()
        except Exception:
            pass


def search_info(ctx: Optional["Context"] = None) -> dict:
    """gx_search_info of the last search on ctx: 8-byte compare steps, device ms of the interval kernel
    and of the locate step (clamp, scan, gather)."""
    ctx = ctx or default_context()
    w = ctypes.c_uint64()
    ms = [ctypes.c_double() for _ in range(2)]
    _check(lib().gx_search_info(ctx.ptr, ctypes.byref(w), *[ctypes.byref(x) for x in ms]))
    return {"word_compares": w.value, "search_ms": ms[0].value, "locate_ms": ms[1].value}


def approx_info(ctx: Optional["Context"] = None) -> dict:
    """gx_approx_info of the last approximate search on ctx: seed hits, 8-byte steps of the verify kernel,
    device ms of the seed stages and of verify and compact."""
    ctx = ctx or default_context()
    c, w = ctypes.c_uint64(), ctypes.c_uint64()
    ms = [ctypes.c_double() for _ in range(2)]
    _check(lib().gx_approx_info(ctx.ptr, ctypes.byref(c), ctypes.byref(w), *[ctypes.byref(x) for x in ms]))
    return {"candidates": c.value, "word_compares": w.value, "seed_ms": ms[0].value, "verify_ms": ms[1].value}


def edit_info(ctx: Optional["Context"] = None) -> dict:
    """gx_edit_info of the last edit search on ctx: seed hits, the ends they reported before equal ends were
    merged, cell updates of the verify kernel, device ms of the seed stages, of verify and of the dedupe."""
    ctx = ctx or default_context()
    v = [ctypes.c_uint64() for _ in range(3)]
    ms = [ctypes.c_double() for _ in range(3)]
    _check(lib().gx_edit_info(ctx.ptr, *[ctypes.byref(x) for x in v + ms]))
    return {"candidates": v[0].value, "pre_dedupe_ends": v[1].value, "cell_updates": v[2].value,
            "seed_ms": ms[0].value, "verify_ms": ms[1].value, "dedupe_ms": ms[2].value}


def extend_info(ctx: Optional["Context"] = None) -> dict:
    """gx_extend_info of the last extend on ctx: its hits, cell updates of the fill, the trace bytes of its
    largest launch, its launches (GX_EXTEND_TRACE_BYTES bounds one), device ms of the fill and of walk, scan
    and emit."""
    ctx = ctx or default_context()
    v = [ctypes.c_uint64() for _ in range(4)]
    ms = [ctypes.c_double() for _ in range(2)]
    _check(lib().gx_extend_info(ctx.ptr, *[ctypes.byref(x) for x in v + ms]))
    return {"hits": v[0].value, "cell_updates": v[1].value, "trace_bytes": v[2].value, "chunks": v[3].value,
            "fill_ms": ms[0].value, "walk_ms": ms[1].value}


class CChainParams(ctypes.Structure):
    _fields_ = [("w_match", ctypes.c_uint32), ("w_drift", ctypes.c_uint32), ("max_gap", ctypes.c_uint32),
                ("max_drift", ctypes.c_uint32), ("max_pred", ctypes.c_uint32), ("min_score", ctypes.c_int32)]


def chain_anchors(anchors, ctx: Optional["Context"] = None, host: bool = False, counts_only: bool = False,
                  **params) -> dict:
    """gx_chain_anchors: the anchors of a batch of queries chained into colinear chains.
    `anchors` is what SuffixIndex.mems returns, or any mapping with uint32 "qpos", "tpos", "length" and the
    uint64 "mem_offsets" (query c's anchors at mem_offsets[c]:mem_offsets[c + 1], ascending by (qpos, tpos)).
    params: w_match, w_drift, max_gap, max_drift, max_pred, min_score (CHAIN_DEFAULTS).  host=True runs the
    host solver (no device).  Returns "score" (int32) and "pred" (uint32, CHAIN_NONE at a root; anchor numbers
    are within the query) of every anchor, the chains' fields as arrays ("member_off", "score_chain" = the
    chain's score, "n_anchors", "root", "end", "qstart", "tstart", "qend", "tend"), "members" (uint32) and
    "chain_offsets" (uint64, nq + 1).  One call: a query's chains and members are at most its anchors, so a
    capacity of the anchor count always suffices (above 2^22 anchors the first call has that many and a GX_ECAP
    is answered with a second call at the exact totals, which runs the dynamic programme again).
    counts_only=True asks for the counts alone (empty chains and members)."""
    unknown = set(params) - set(CHAIN_DEFAULTS)
    if unknown:
        raise TypeError(f"chain_anchors: unknown parameters {sorted(unknown)}")
    p = CChainParams(**{**CHAIN_DEFAULTS, **params})
    off = np.ascontiguousarray(anchors["mem_offsets"], np.uint64)
    nq, A = len(off) - 1, len(anchors["qpos"])
    an = np.zeros(max(A, 1), MEM_DTYPE)
    an["qpos"][:A], an["tpos"][:A], an["len"][:A] = anchors["qpos"], anchors["tpos"], anchors["length"]
    c = None if host else (ctx or default_context())
    score, pred = np.zeros(max(A, 1), np.int32), np.zeros(max(A, 1), np.uint32)
    coff, mtot = np.zeros(nq + 1, np.uint64), ctypes.c_uint64()

    def call(ch, mem):
        return lib().gx_chain_anchors(c.ptr if c else None, an.ctypes.data, off.ctypes.data, nq, ctypes.byref(p),
                                      score.ctypes.data, pred.ctypes.data, ch.ctypes.data if ch is not None else None,
                                      len(ch) if ch is not None else 0, mem.ctypes.data if mem is not None else None,
                                      len(mem) if mem is not None else 0, coff.ctypes.data, ctypes.byref(mtot))

    ch, mem = np.zeros(0, CHAIN_DTYPE), np.zeros(0, np.uint32)
    if counts_only:
        _check(call(None, None))
    else:
        # chains and members are at most the anchors: one call at that capacity, up to _FIRST_CAP; beyond it a
        # GX_ECAP leaves the totals, and the second call has exactly them
        cap = max(1, min(A, _FIRST_CAP))
        ch, mem = np.zeros(cap, CHAIN_DTYPE), np.zeros(cap, np.uint32)
        rc = call(ch, mem)
        if rc == 7:
            ch, mem = np.zeros(max(1, int(coff[-1])), CHAIN_DTYPE), np.zeros(max(1, int(mtot.value)), np.uint32)
            rc = call(ch, mem)
        _check(rc)
        ch, mem = ch[:int(coff[-1])], np.ascontiguousarray(mem[:int(mtot.value)])
    r = {"score": score[:A], "pred": pred[:A], "members": mem, "chain_offsets": coff, "members_total": int(mtot.value)}
    for f in CHAIN_DTYPE.names:
        r["score_chain" if f == "score" else f] = np.ascontiguousarray(ch[f])
    return r


def chain_info(ctx: Optional["Context"] = None) -> dict:
    """gx_chain_info of the last chain call on ctx: its anchors, segments, the pairs the score kernel
    evaluated, its reported chains, device ms of flags, scan and score and of best, heads, scans and walk
    (0 for what did not run)."""
    ctx = ctx or default_context()
    v = [ctypes.c_uint64() for _ in range(4)]
    ms = [ctypes.c_double() for _ in range(2)]
    _check(lib().gx_chain_info(ctx.ptr, *[ctypes.byref(x) for x in v + ms]))
    return {"anchors": v[0].value, "segments": v[1].value, "pair_evals": v[2].value, "chains": v[3].value,
            "score_ms": ms[0].value, "chain_ms": ms[1].value}


def cigar_string(cigar_slice) -> str:
    """The text of a hit's runs: cigar_string(r["cigar"][o[h]:o[h + 1]]) is e.g. "57M1I42M"."""
    return "".join(f"{int(x) >> 4}{CIGAR_OPS[int(x) & 15]}" for x in cigar_slice)


def match_info(ctx: Optional["Context"] = None) -> dict:
    """gx_match_info of the last matching-statistics or MEM call on ctx: candidate pairs, kept (left-maximal)
    pairs, 8-byte compare steps, device ms of the matching-statistics kernel, of the seed stages and of emit,
    sort and pack (0 for what did not run)."""
    ctx = ctx or default_context()
    v = [ctypes.c_uint64() for _ in range(3)]
    ms = [ctypes.c_double() for _ in range(3)]
    _check(lib().gx_match_info(ctx.ptr, *[ctypes.byref(x) for x in v + ms]))
    return {"candidates": v[0].value, "kept": v[1].value, "word_compares": v[2].value,
            "stats_ms": ms[0].value, "seed_ms": ms[1].value, "emit_ms": ms[2].value}


# STRING_TERMINATORS (tree.rs:66-69)
_TERMINATORS = "$!@#%^&*()-_=+{}[]|;:'<>,.?/~` \n"


class SuffixTree:
    """The crate-shaped suffixtree::tree::SuffixTree (tree.rs:41-190) without the tree: compute_stats
    reads the suffix array, get_lcs is compare mode's common_substring.  Graphviz
    output and suffix links are out of scope (suffix_links is accepted and ignored).
    host=True keeps every call on the host solvers (no device)."""

    def __init__(self, alphabet_file: str, initial_allocation: int = 0, ctx: Optional["Context"] = None,
                 host: bool = False):
        try:
            with open(alphabet_file, "r") as f:
                alphabet = f.read().replace(" ", "")
        except OSError:
            raise RuntimeError(f"Could not read alphabet file: {alphabet_file}")   # tree.rs:143
        self.alphabet = sorted(list(_TERMINATORS) + list(alphabet))
        self.strings: List[str] = []
        self.stats = TreeStats()
        self._ctx = ctx
        self._host = host

    def insert_string(self, new_string: str, enable_suffix_links: bool = False, print_time: bool = False) -> None:
        if len(self.strings) >= len(_TERMINATORS):
            raise IndexError("the suffix tree can support up to 32 strings")   # tree.rs:65
        for c in new_string:
            if c not in self.alphabet:
                raise ValueError(f"Character {c} not found in alphabet")   # tree.rs:56-63
        self.strings.append(new_string + _TERMINATORS[len(self.strings)])

    def _bare(self, idx: int) -> bytes:
        return self.strings[idx][:-1].encode("latin-1")

    def compute_stats(self, string_idx: int = 0) -> None:
        if string_idx != 0:
            raise NotImplementedError("compute_stats: only string 0 (the reference's leaf-id test holds for it alone)")
        r = suffix_tree_stats(self._bare(0), ctx=self._ctx, want=("bwt",), host=self._host)
        self.stats = r["stats"]

    def get_lcs(self, string_one_idx: int, string_two_idx: int) -> Tuple[int, int, int]:
        """get_lcs (tree.rs:218-281): (i, j, length)."""
        a, b = self._bare(string_one_idx), self._bare(string_two_idx)
        return common_substring_host(a, b) if self._host else common_substring(a, b, self._ctx)

    def find(self, pattern: str, string_idx: int = 0) -> List[int]:
        """Every position of `pattern` in string `string_idx`, ascending (search mode, DESIGN.md 18;
        the reference's tree has no such query).  The empty pattern matches at 0 .. len."""
        idx = SuffixIndex(self._bare(string_idx), ctx=self._ctx, host=self._host)
        try:
            return idx.search([pattern.encode("latin-1")], max_hits=ALL_HITS)["positions"].tolist()
        finally:
            idx.close()

    def __str__(self):  # display.rs:40-56 without the Graphviz block
        return f"\nStats: {self.stats}\n"
