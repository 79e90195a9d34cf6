#!/usr/bin/env python3
"""Measures gx_suffix_index_extend and writes profiles/suffix_extend.json.

Inputs and protocol of tools/edit_bench.py: per input 1,048,576 reads of about 32, 100 and 150 bases with
r mod (k + 1) planted edits, k = 1, 2, 3, the hits those of search_edit at max_hits = 16 with starts; median
of 5 whole calls after one warm-up, the host clock around the synchronising call, beside the device times of
gx_extend_info of the median call (fill_ms: the fill kernels; walk_ms: walk, scan and emit).  Per shape:

  extend           the whole call with CIGARs at band = k (the Python wrapper's first capacity of eight runs a
                   hit holds them, so it is one call), and with cigars=False
  map_reads        search_edit then extend, against search_edit alone in the same run
  host             the host index on one thread, once, compared equal with the device's result
  align_batch      what a caller does without extend: the (window, pattern) pairs of the first 65,536 hits
                   copied to the host and through gx_align_batch with steps (the C call alone is timed, its
                   pointer arrays built before), scaled to the shape's hits; at k = 2 only
  sweep            GX_EXTEND_TRACE_BYTES from 16 MiB to 1 GiB on the 100-base reads at k = 2
  floor            1 and 1,024 reads of 100 bases at k = 2

"rest_ms" = whole call - fill_ms - walk_ms: the host's pass over the hits, staging, the waits and the copies.

    python tools/extend_bench.py [--out profiles/suffix_extend.json] [--inputs covid,chr12,synthetic]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gxamd as gx  # noqa: E402
from edit_bench import reads_of, same  # noqa: E402
from search_bench import median_call  # noqa: E402
from suffix_bench import GOLDEN, chr12, first_record, synthetic  # noqa: E402

SAMPLE = 65536
EXT_FIELDS = tuple(gx.EXTEND_HIT_DTYPE.names) + ("cigar", "cigar_offsets")


def align_batch_ms(ctx, s: bytes, pats, found, nsample: int) -> float:
    """ms of one gx_align_batch call with steps over the first nsample hits' (window, pattern) pairs."""
    packed, off = pats
    ho = found["hit_offsets"].astype(np.int64)
    pid = np.repeat(np.arange(len(ho) - 1), np.diff(ho))[:nsample]
    text = np.frombuffer(s, np.uint8)
    sta, end = found["starts"][:nsample].astype(np.int64), found["ends"][:nsample].astype(np.int64)
    po, pe = off[pid].astype(np.int64), off[pid + 1].astype(np.int64)
    P = len(pid)
    s1p = (ctypes.c_void_p * P)(*(text.ctypes.data + sta).tolist())
    s2p = (ctypes.c_void_p * P)(*(packed.ctypes.data + po).tolist())
    n = (ctypes.c_size_t * P)(*(end - sta).tolist())
    m = (ctypes.c_size_t * P)(*(pe - po).tolist())
    cap = (end - sta) + (pe - po) + 2
    first = np.zeros(P + 1, np.int64)
    np.cumsum(cap, out=first[1:])
    steps = np.zeros(int(first[-1]), gx.STEP_DTYPE)
    stp = (ctypes.c_void_p * P)(*(steps.ctypes.data + first[:-1] * gx.STEP_DTYPE.itemsize).tolist())
    caps = (ctypes.c_size_t * P)(*cap.tolist())
    res = (gx.CResult * P)()
    sc = gx.Scores().c()

    def call():
        rc = gx.lib().gx_align_batch(ctx.ptr, s1p, n, s2p, m, P, ctypes.byref(sc), 0, 0, stp, caps, res)
        assert rc == 0, gx.lib().gx_last_error()

    call()
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def measure(ctx, dev, host, s, nreads, m, k, baseline):
    pats = reads_of(s, nreads, m, k, 1000 * k + m)
    found = dev.search_edit(pats, k, max_hits=16)
    nh = int(found["hit_offsets"][-1])
    b = {"reads": nreads, "m": m, "k": k, "band": k, "hits": nh}
    search_ms, _ = median_call(lambda: dev.search_edit(pats, k, max_hits=16))

    def call(cigars=True):
        r = dev.extend(pats, found, band=k, cigars=cigars)
        return r, gx.extend_info(ctx)

    ms, (r, info) = median_call(call)
    ms0, (_, info0) = median_call(lambda: call(False))
    map_ms, _ = median_call(lambda: dev.map_reads(pats, k, max_hits=16))
    t0 = time.perf_counter()
    h = host.extend(pats, found, band=k)
    host_ms = (time.perf_counter() - t0) * 1e3
    b.update({"call_ms_median": round(ms, 4), "fill_ms": round(info["fill_ms"], 4), "walk_ms": round(info["walk_ms"], 4),
              "rest_ms": round(ms - info["fill_ms"] - info["walk_ms"], 4),
              "call_ms_median_no_cigars": round(ms0, 4), "walk_ms_no_cigars": round(info0["walk_ms"], 4),
              "trace_bytes": info["trace_bytes"], "chunks": info["chunks"], "runs": int(r["cigar_offsets"][-1]),
              "hits_per_s_call": round(nh / (ms * 1e-3)),
              "cell_updates": info["cell_updates"],
              "cell_updates_per_s_fill": round(info["cell_updates"] / max(info["fill_ms"] * 1e-3, 1e-9)),
              "search_edit_call_ms_median": round(search_ms, 4), "map_reads_call_ms_median": round(map_ms, 4),
              "map_reads_over_search_edit": round(map_ms / search_ms, 3),
              "host_ms_one_thread": round(host_ms, 3), "host_over_gpu": round(host_ms / ms, 3),
              "equal_to_host": same(r, h, EXT_FIELDS)})
    if baseline and nh:
        ns = min(SAMPLE, nh)
        try:
            ab = align_batch_ms(ctx, s, pats, found, ns)
            b.update({"align_batch_sample_hits": ns, "align_batch_sample_ms": round(ab, 3),
                      "align_batch_ms_scaled_to_hits": round(ab * nh / ns, 3),
                      "align_batch_over_extend": round(ab * nh / ns / ms, 2)})
        except AssertionError as e:   # (the batch aligner refused the sample: recorded, the rest goes on)
            b["align_batch_error"] = str(e)
    print(json.dumps(b), flush=True)
    return b, pats, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_extend.json"))
    ap.add_argument("--inputs", default="covid,chr12,synthetic")
    ap.add_argument("--synthetic-mi", type=int, default=16)
    ap.add_argument("--reads", type=int, default=1 << 20)
    args = ap.parse_args()
    os.environ["GX_SUFFIX_HOST_BELOW"] = "0"
    os.environ.pop("GX_APPROX_CAND_BUDGET", None)
    os.environ.pop("GX_EXTEND_TRACE_BYTES", None)   # the default
    ctx = gx.Context(0)
    inputs = []
    for name in args.inputs.split(","):
        if name == "covid":
            inputs.append(("Covid_Wuhan", first_record(os.path.join(GOLDEN, "comparison_data", "Covid_Wuhan.fasta"))))
        elif name == "chr12":
            inputs.append(("chr12", chr12()))
        elif name == "synthetic":
            mi = args.synthetic_mi
            inputs.append((f"synthetic_{mi}Mi_seed{mi}", synthetic(mi << 20, mi)))
    rows = []
    for name, s in inputs:
        dev, host = gx.SuffixIndex(s, ctx=ctx), gx.SuffixIndex(s, host=True)
        row = {"input": name, "n": len(s), "batches": [], "trace_bytes_sweep": []}
        for m in (32, 100, 150):
            for k in (1, 2, 3):
                try:
                    b, pats, found = measure(ctx, dev, host, s, args.reads, m, k, baseline=k == 2)
                except gx.GxError as e:   # (the edit search refuses a batch over its seed budget)
                    if e.code != 3:
                        raise
                    b = {"reads": args.reads, "m": m, "k": k, "refused": str(e)}
                    print(json.dumps(b), flush=True)
                row["batches"].append(b)
                if (m, k) == (100, 2) and "refused" not in b:
                    for mib in (16, 64, 256, 512, 1024):
                        os.environ["GX_EXTEND_TRACE_BYTES"] = str(mib << 20)
                        ms, (_, info) = median_call(lambda: (dev.extend(pats, found, band=k), gx.extend_info(ctx)))
                        sw = {"trace_mib": mib, "call_ms_median": round(ms, 4), "fill_ms": round(info["fill_ms"], 4),
                              "walk_ms": round(info["walk_ms"], 4), "chunks": info["chunks"], "trace_bytes": info["trace_bytes"]}
                        print(json.dumps(sw), flush=True)
                        row["trace_bytes_sweep"].append(sw)
                    os.environ.pop("GX_EXTEND_TRACE_BYTES")
        for nreads in (1, 1024):
            row["batches"].append(measure(ctx, dev, host, s, nreads, 100, 2, baseline=False)[0])
        rows.append(row)
        dev.close()
        host.close()
    ctx.close()
    doc = {"tool": "tools/extend_bench.py",
           "timing": "median of 5 whole calls after one warm-up, host clock; fill_ms / walk_ms are device time of the "
                     "median call; search_edit, map_reads, the host index (once, one thread) and gx_align_batch of a "
                     "65,536-hit sample (one call after a warm-up, scaled per hit) in the same run, same machine",
           "inputs": rows}
    if os.path.exists(args.out):   # a run over some of the inputs keeps the others' rows
        with open(args.out) as f:
            old = json.load(f)
        names = {r["input"] for r in rows}
        doc["inputs"] = [r for r in old.get("inputs", []) if r["input"] not in names] + rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
