#!/usr/bin/env python3
"""Measures search mode (gx_suffix_index_build / gx_suffix_index_search) and writes
profiles/suffix_search.json.

Protocol of tools/suffix_bench.py: median of 5 whole calls after one warm-up,
the host clock around the synchronising call, beside the device times of
gx_search_info (interval kernel; locate = clamp, scan and gather) of the median
call.  Per input: the index build against gx_suffix_tree_stats on the same
input (what dropping LCP, fold and BWT saves), then batches of reads cut from
the input, every second one with one substitution: 1,048,576 reads of 20, 32,
100 and 150 bases, counts only and with max_hits = 16, and 1 and 1,024 reads of
32 bases for the launch floor.  The same batch runs once on the host index on
one thread of the same machine (median of 5 for the small batches) and is
compared equal in the same run.

"rest_ms" = whole call - search_ms - locate_ms: staging, copies and, with
positions, the host's per-pattern sort; the sort's share alone is not measured.

    python tools/search_bench.py [--out profiles/suffix_search.json] [--synthetic-mi 16] [--host-max-mi 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gxamd as gx  # noqa: E402
from suffix_bench import GOLDEN, chr12, first_record, synthetic  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def reads_of(s: bytes, nreads: int, m: int, seed: int):
    """(packed, offsets): nreads reads of m bases cut from s, every second one with one substitution."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(s, np.uint8)
    starts = rng.integers(0, len(s) - m + 1, nreads)
    reads = a[starts[:, None] + np.arange(m)[None, :]]
    col = rng.integers(0, m, nreads)
    odd = np.flatnonzero(np.arange(nreads) % 2 == 1)
    old = reads[odd, col[odd]]
    reads[odd, col[odd]] = ACGT[(np.searchsorted(ACGT, old) + 1) % 4]
    return reads.reshape(-1), np.arange(nreads + 1, dtype=np.uint64) * np.uint64(m)


def median_call(f, reps: int = 5):
    f()   # warm-up: the pool's buffers exist afterwards
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        runs.append(((time.perf_counter() - t0) * 1e3, r))
    runs.sort(key=lambda x: x[0])
    return runs[len(runs) // 2]


def same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_search.json"))
    ap.add_argument("--synthetic-mi", type=int, default=16)
    ap.add_argument("--host-max-mi", type=float, default=16.0,
                    help="the host index is not built above this many Mi bases (recorded as not measured)")
    ap.add_argument("--reads", type=int, default=1 << 20)
    args = ap.parse_args()
    os.environ["GX_SUFFIX_HOST_BELOW"] = "0"
    ctx = gx.Context(0)
    inputs = [("Covid_Wuhan", first_record(os.path.join(GOLDEN, "comparison_data", "Covid_Wuhan.fasta"))),
              ("chr12", chr12())]
    if args.synthetic_mi:
        mi = args.synthetic_mi
        inputs.append((f"synthetic_{mi}Mi_seed{mi}", synthetic(mi << 20, mi)))
    rows = []
    for name, s in inputs:
        n = len(s)

        def build():
            gx.SuffixIndex(s, ctx=ctx).close()
            return None
        build_ms, _ = median_call(build)

        def stats():
            gx.suffix_tree_stats(s, ctx=ctx)
            return gx.suffix_info(ctx)
        stats_ms, sinfo = median_call(stats)
        dev = gx.SuffixIndex(s, ctx=ctx)
        host = None
        row = {"input": name, "n": n, "index_build_ms_median": round(build_ms, 3),
               "suffix_tree_stats_ms_median": round(stats_ms, 3),
               "stats_lcp_ms": round(sinfo["lcp_ms"], 3), "stats_fold_ms": round(sinfo["fold_ms"], 3),
               "stats_over_build": round(stats_ms / build_ms, 2), "device_bytes": dev.info()["device_bytes"]}
        if n <= args.host_max_mi * (1 << 20):
            t0 = time.perf_counter()
            host = gx.SuffixIndex(s, host=True)
            row["host_index_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        else:
            row["host_index_build_ms"] = "not measured"
        print(json.dumps(row), flush=True)
        batches = []
        shapes = [(args.reads, m) for m in (20, 32, 100, 150)] + [(1, 32), (1024, 32)]
        for nreads, m in shapes:
            if m > n:
                continue
            pats = reads_of(s, nreads, m, 1000 + m)
            for max_hits in (0, 16):
                def call():
                    r = dev.search(pats, max_hits=max_hits)
                    return r, gx.search_info(ctx)
                ms, (r, info) = median_call(call)
                b = {"reads": nreads, "m": m, "max_hits": max_hits, "call_ms_median": round(ms, 4),
                     "search_ms": round(info["search_ms"], 4), "locate_ms": round(info["locate_ms"], 4),
                     "rest_ms": round(ms - info["search_ms"] - info["locate_ms"], 4),
                     "patterns_per_s_call": round(nreads / (ms * 1e-3)),
                     "patterns_per_s_search_kernel": round(nreads / (info["search_ms"] * 1e-3)),
                     "word_compares_per_pattern": round(info["word_compares"] / nreads, 2),
                     "found": int((r["count"] > 0).sum()),
                     "positions": int(r["hit_offsets"][-1]) if max_hits else 0}
                if host is not None:
                    hruns = []
                    for _ in range(5 if nreads <= 1024 else 1):   # (small batches: the first run is cold)
                        t0 = time.perf_counter()
                        h = host.search(pats, max_hits=max_hits)
                        hruns.append((time.perf_counter() - t0) * 1e3)
                    hms = statistics.median(hruns)
                    b["host_ms_one_thread"] = round(hms, 4)
                    b["host_over_gpu"] = round(hms / ms, 3)
                    b["equal_to_host"] = same(r, h)
                else:
                    b["host_ms_one_thread"] = "not measured"
                batches.append(b)
                print(json.dumps(b), flush=True)
        row["batches"] = batches
        rows.append(row)
        dev.close()
        if host is not None:
            host.close()
    ctx.close()
    doc = {"tool": "tools/search_bench.py",
           "timing": "median of 5 whole calls after one warm-up, host clock; search_ms / locate_ms are device time "
                     "of the median call; the host index runs once (median of 5 for batches of 1,024 or fewer), one thread, same machine",
           "host_sort_share": "not measured separately: rest_ms holds staging, copies and the host sort",
           "inputs": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
