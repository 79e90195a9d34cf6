#!/usr/bin/env python3
"""Measures suffix-tree mode (gx_suffix_tree_stats) and writes profiles/suffix_tree.json.

Per input: the whole call on the GPU (median of 5 after one warm-up, host clock
around the synchronising call, BWT copied back), the phases of gx_suffix_info
(sorts, LCP kernel, statistics fold: device time of the median call), doubling
rounds and radix passes, the sort's achieved bytes per second (12 B per element
read twice -- histogram and scatter -- and written once, per pass) against the
HBM peak, and the host solver on one thread of the same box.  The host solver
is the baseline: a straightforward builder (std::sort doubling, Kasai, stack
fold) written with the kernels -- not the reference's tree, which cannot be
built here, and not a tuned library, because none is installed.

Inputs: the reference's Covid_Wuhan (30k), Slyco (155k) and chr12 (1.08M), and
seeded synthetic genomes of 16 Mi and 128 Mi bases: random ACGT with mutated
copies of blocks planted, so that max LCP is in the hundreds, not log4 n.
The small-input crossing with the host solver is found on random ACGT.

    python tools/suffix_bench.py [--out profiles/suffix_tree.json] [--sizes 16,128] [--host-max-mi 16]
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
import gxamd as gx  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s (vendor figure)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def first_record(path: str) -> bytes:
    seq, seen = [], False
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if seen:
                    break
                seen = True
            elif seen:
                seq.append(line.strip())
    return b"".join(seq)


def chr12() -> bytes:
    with open(os.path.join(GOLDEN, "suffix", "suffix_vectors.json")) as f:
        v = next(v for v in json.load(f)["vectors"] if v["name"] == "chr12")
    p = np.fromfile(os.path.join(GOLDEN, "suffix", v["acgt2"]), np.uint8)
    codes = np.stack([(p >> (2 * k)) & 3 for k in range(4)], 1).reshape(-1)[:v["n"]]
    return np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()


def synthetic(n: int, seed: int) -> bytes:
    """Random ACGT; every 256 Ki bases a 2,000-base block is copied elsewhere with
    one substitution per ~300 bases."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)].copy()
    L = 2000
    for _ in range(max(1, n >> 18)):
        src, dst = (int(x) for x in rng.integers(0, n - L, 2))
        blk = a[src:src + L].copy()
        pos = rng.integers(0, L, L // 300)
        blk[pos] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, pos.size)]
        a[dst:dst + L] = blk
    return a.tobytes()


def time_gpu(ctx, s: bytes, reps: int = 5):
    gx.suffix_tree_stats(s, ctx=ctx)   # warm-up: the pool's buffers exist afterwards
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = gx.suffix_tree_stats(s, ctx=ctx)
        ms = (time.perf_counter() - t0) * 1e3
        runs.append((ms, gx.suffix_info(ctx), r))
    runs.sort(key=lambda x: x[0])
    return runs[len(runs) // 2], [round(x[0], 3) for x in runs]


def time_host(s: bytes, reps: int):
    out, r = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = gx.suffix_tree_stats(s, host=True)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_tree.json"))
    ap.add_argument("--sizes", default="16,128", help="synthetic genome sizes in Mi bases")
    ap.add_argument("--host-max-mi", type=float, default=16.0,
                    help="the host solver is not run above this many Mi bases (recorded as not measured)")
    args = ap.parse_args()
    os.environ["GX_SUFFIX_HOST_BELOW"] = "0"
    ctx = gx.Context(0)
    T, C, B = gx.suffix_tile()
    inputs = [("Covid_Wuhan", first_record(os.path.join(GOLDEN, "comparison_data", "Covid_Wuhan.fasta"))),
              ("Slyco", first_record(os.path.join(GOLDEN, "fasta", "Slyco.fasta.gz"))),
              ("chr12", chr12()),
              ("unary_1Mi", b"A" * (1 << 20))]   # the LCP kernel's bad case: (n / C) * max LCP byte compares
    for mi in [int(x) for x in args.sizes.split(",") if x]:
        inputs.append((f"synthetic_{mi}Mi_seed{mi}", synthetic(mi << 20, mi)))
    rows = []
    for name, s in inputs:
        n = len(s)
        (ms, info, r), all_ms = time_gpu(ctx, s)
        row = {"input": name, "n": n, "gpu_call_ms_median": round(ms, 3), "gpu_call_ms_runs": all_ms,
               "doubling_rounds": info["doubling_rounds"], "sort_passes": info["sort_passes"],
               "sort_ms": round(info["sort_ms"], 3), "lcp_ms": round(info["lcp_ms"], 3),
               "fold_ms": round(info["fold_ms"], 3), "max_lcp": r["raw"].max_string_depth,
               "num_internal": r["raw"].num_internal}
        sort_bytes = info["sort_passes"] * (n + 1) * 12 * 3
        row["sort_bytes"] = sort_bytes
        row["sort_gbs"] = round(sort_bytes / (info["sort_ms"] * 1e-3) / 1e9, 1) if info["sort_ms"] > 0 else None
        row["sort_fraction_of_hbm_peak"] = round(row["sort_gbs"] / HBM_PEAK_GBS, 4) if row["sort_gbs"] else None
        if n <= args.host_max_mi * (1 << 20):
            hms, h = time_host(s, 3 if n < (1 << 21) else 1)
            row["host_ms_one_thread"] = round(hms, 3)
            row["host_over_gpu"] = round(hms / ms, 2)
            row["equal_to_host"] = bool(h["bwt"] == r["bwt"] and [getattr(h["raw"], k) for k, _ in h["raw"]._fields_]
                                        == [getattr(r["raw"], k) for k, _ in r["raw"]._fields_])
        else:
            row["host_ms_one_thread"] = "not measured"
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the small-input crossing: random ACGT, whole call against the host solver
    rng = np.random.default_rng(1)
    cross, crossing = [], None
    for n in (256, 1024, 4096, 16384, 65536, 262144):
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)].tobytes()
        (ms, _, _), _ = time_gpu(ctx, s)
        hms, _ = time_host(s, 5)
        cross.append({"n": n, "gpu_call_ms": round(ms, 4), "host_ms": round(hms, 4)})
        if crossing is None and ms < hms:
            crossing = n
    ctx.close()
    doc = {"tool": "tools/suffix_bench.py", "tile": {"sort_items_per_wg": T, "lcp_chunk": C, "fold_block": B},
           "hbm_peak_gbs": HBM_PEAK_GBS,
           "baseline": "host solver of the same change (std::sort prefix doubling, Kasai, stack fold), one thread, "
                       "same box; not the reference's tree and not a tuned library",
           "timing": "median of 5 whole calls after one warm-up, host clock; phases are device time of the median call",
           "inputs": rows, "crossing_random_acgt": cross,
           "first_measured_n_where_gpu_is_faster": crossing if crossing is not None else "none measured"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
