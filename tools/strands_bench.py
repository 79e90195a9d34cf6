#!/usr/bin/env python3
"""Measures the stranded calls of search mode against what a caller had before them, and writes
profiles/suffix_strands.json.

Inputs of tools/search_bench.py: chr12 and the seeded synthetic genome.  Per input a million reads of 32, 100
and 150 bases (every second one with one substitution, every second pair reverse-complemented) and the mutated
1 Mi-base query of tools/match_bench.py.  search (counts and max_hits = 16), search_edit at k = 2 and mems at
min_len = 20 run

    one     with strands="both": one call, one host copy of the reads, the reverse complements made on the device
    two     as the two calls of the existing entry points that a caller's only alternative is: the forward batch,
            then a batch reverse-complemented on the host.  "two_calls_ms" is the two calls alone,
            "host_revcomp_ms" what making the second batch cost (numpy: a table lookup of the reversed reads)

in the same run, alternating, each the median of 7 whole calls after one warm-up (host clock around the
synchronising call), with the smallest and the largest beside it.  "rc_ms" is the device time of
strand_rc_kernel in the median stranded call (gx_strand_info), "h2d_saved_ms" the measured time of copying the
forward bytes once more to the device, which the stranded call does not do.  Both results are compared equal in
the same run.  Nothing is claimed here: the numbers are what they are.

    python tools/strands_bench.py [--out profiles/suffix_strands.json] [--synthetic-mi 16] [--reads 1048576]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gxamd as gx  # noqa: E402
from match_bench import mutated_query  # noqa: E402
from search_bench import reads_of  # noqa: E402
from suffix_bench import chr12, synthetic  # noqa: E402

COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "CG"):
    COMP[ord(_a)], COMP[ord(_b)] = ord(_b), ord(_a)
REPS = 7


def host_revcomp(packed: np.ndarray, off: np.ndarray):
    """The batch reverse-complemented on the host, reads of one length m or a single query."""
    n = len(off) - 1
    m = int(off[1]) if n else 0
    return np.ascontiguousarray(COMP[packed.reshape(n, m)[:, ::-1]]).reshape(-1), off


def stranded_reads(s: bytes, nreads: int, m: int, seed: int):
    """reads_of, with reads 2 and 3 of every four reverse-complemented: half of a read set comes from the - strand."""
    packed, off = reads_of(s, nreads, m, seed)
    r = packed.reshape(nreads, m).copy()
    rev = np.flatnonzero((np.arange(nreads) >> 1) % 2 == 1)
    r[rev] = COMP[r[rev][:, ::-1]]
    return r.reshape(-1), off


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def glue(fwd: dict, rev: dict, per_item, per_hit, offsets_key):
    """The two calls' results laid out as the stranded call's: per-item arrays back to back, offsets shifted."""
    out = {k: np.concatenate([fwd[k], rev[k]]) for k in per_item + per_hit if fwd.get(k) is not None}
    if offsets_key in fwd:
        out[offsets_key] = np.concatenate([fwd[offsets_key], fwd[offsets_key][-1] + rev[offsets_key][1:]])
    return out


def compare(ctx, name, one, two_calls, batch, glue_args):
    """Alternating: the stranded call, then the host reverse complement and the two calls."""
    one(), two_calls(batch, host_revcomp(*batch))   # warm-up: the pool's buffers exist afterwards
    one_ms, two_ms, rc_host_ms, rc_dev_ms = [], [], [], []
    for _ in range(REPS):
        ms, r1 = timed(one)
        one_ms.append(ms)
        rc_dev_ms.append(gx.strand_info(ctx)["rc_ms"])
        ms, rev = timed(lambda: host_revcomp(*batch))
        rc_host_ms.append(ms)
        ms, (rf, rr) = timed(lambda: two_calls(batch, rev))
        two_ms.append(ms)
    want = glue(rf, rr, *glue_args)
    equal = all(np.array_equal(r1[k], want[k]) for k in want)
    row = {"call": name, "one_call_both_ms": stats(one_ms), "two_calls_ms": stats(two_ms),
           "host_revcomp_ms": stats(rc_host_ms), "rc_ms": stats(rc_dev_ms), "equal": bool(equal)}
    row["one_over_two_calls"] = round(row["one_call_both_ms"]["median"] / row["two_calls_ms"]["median"], 3)
    row["one_over_two_calls_and_host_revcomp"] = round(
        row["one_call_both_ms"]["median"] / (row["two_calls_ms"]["median"] + row["host_revcomp_ms"]["median"]), 3)
    return row


def h2d_ms(nbytes: int):
    """A pageable host-to-device copy of nbytes, as staging makes it (hipMemcpy of the runtime the library runs on):
    median of 7 after one warm-up."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    src = np.full(max(nbytes, 1), 65, np.uint8)
    dst = ctypes.c_void_p()
    if hip.hipMalloc(ctypes.byref(dst), src.size) != 0:
        return "not measured"
    runs = []
    for k in range(REPS + 1):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        rc = hip.hipMemcpy(dst, src.ctypes.data, src.size, 1)   # hipMemcpyHostToDevice; returns when the copy is done
        hip.hipDeviceSynchronize()
        if k and rc == 0:
            runs.append((time.perf_counter() - t0) * 1e3)
    hip.hipFree(dst)
    return stats(runs) if runs else "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_strands.json"))
    ap.add_argument("--synthetic-mi", type=int, default=16)
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--inputs", default="chr12,synthetic")
    args = ap.parse_args()
    os.environ["GX_SUFFIX_HOST_BELOW"] = "0"
    ctx = gx.Context(0)
    inputs = []
    if "chr12" in args.inputs:
        inputs.append(("chr12", chr12()))
    if "synthetic" in args.inputs and args.synthetic_mi:
        mi = args.synthetic_mi
        inputs.append((f"synthetic_{mi}Mi_seed{mi}", synthetic(mi << 20, mi)))
    HIT = ("lo", "count", "prefix_len", "prefix_pos")
    EDIT = ("count", "best_dist", "best_end", "candidates")
    rows = []
    for name, s in inputs:
        dev = gx.SuffixIndex(s, ctx=ctx)
        row = {"input": name, "n": len(s), "batches": []}
        for m in (32, 100, 150):
            if m > len(s):
                continue
            batch = stranded_reads(s, args.reads, m, 2000 + m)
            b = {"reads": args.reads, "m": m, "forward_bytes": int(batch[0].size), "h2d_saved_ms": h2d_ms(batch[0].size),
                 "calls": []}
            for label, one, two, ga in (
                ("search counts", lambda: dev.search(batch, 0, strands="both"),
                 lambda f, r: (dev.search(f, 0), dev.search(r, 0)), (HIT, (), "hit_offsets")),
                ("search max_hits=16", lambda: dev.search(batch, 16, strands="both"),
                 lambda f, r: (dev.search(f, 16), dev.search(r, 16)), (HIT, ("positions",), "hit_offsets")),
                ("search_edit k=2 max_hits=16", lambda: dev.search_edit(batch, 2, 16, strands="both"),
                 lambda f, r: (dev.search_edit(f, 2, 16), dev.search_edit(r, 2, 16)),
                 (EDIT, ("ends", "distances", "starts"), "hit_offsets")),
            ):
                try:
                    c = compare(ctx, label, one, two, batch, ga)
                except gx.GxError as e:   # (a budget refusal at this shape is a result too)
                    c = {"call": label, "refused": str(e)}
                b["calls"].append(c)
                print(json.dumps({"input": name, "m": m, **c}), flush=True)
            row["batches"].append(b)
        q = mutated_query(s, 1 << 20, 1 << 16, 100, 17)
        batch = (np.frombuffer(q, np.uint8), np.array([0, len(q)], np.uint64))
        b = {"reads": 1, "m": len(q), "forward_bytes": len(q), "h2d_saved_ms": h2d_ms(len(q)), "calls": []}
        c = compare(ctx, "mems min_len=20", lambda: dev.mems(batch, 20, strands="both"),
                    lambda f, r: (dev.mems(f, 20), dev.mems(r, 20)), batch,
                    (("candidates",), ("qpos", "tpos", "length"), "mem_offsets"))
        b["calls"].append(c)
        print(json.dumps({"input": name, "m": len(q), **c}), flush=True)
        row["batches"].append(b)
        rows.append(row)
        dev.close()
    ctx.close()
    doc = {"tool": "tools/strands_bench.py",
           "timing": f"median (min, max) of {REPS} whole calls after one warm-up, host clock around the synchronising call, "
                     "the stranded call and the two-call alternative alternating in one run; rc_ms is device time of "
                     "strand_rc_kernel; h2d_saved_ms a pageable copy of the forward bytes",
           "inputs": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
