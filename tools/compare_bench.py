#!/usr/bin/env python3
"""Compare-mode measurements on the ten genomes of tests/golden/comparison_data
(bench.py measures the aligner and is not involved).

  python tools/compare_bench.py [--reps N] [--threads 16] [--sweep] [--out profiles/compare_matrix.json]
      one GPU: gx_compare_matrix in its default configuration against the
      host solver on `threads` threads, one pair per thread (the reference's
      rayon pool, main.rs:245-261); levels, sub-problem counts and the run
      kernel's byte compares per second.  --sweep adds the runs behind the
      budgets of DESIGN.md 16.3: GX_COMPARE_HOST_CELLS, GX_COMPARE_SEG_H and
      GX_COMPARE_CAND_CAP one at a time.
  python tools/compare_bench.py --candidates [--out profiles/compare_candidates.json]
      no GPU: how many candidate starts every sub-problem of the recursion
      holds (what the candidate buffer has to take), by sub-problem size.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("oracle", "genomics-rs_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import gxamd as gx  # noqa: E402


def genomes():
    cont = gx.SequenceContainer()
    comp = os.path.join(ROOT, "tests", "golden", "comparison_data")
    for f in sorted(os.listdir(comp)):
        if f.endswith(".fasta"):
            cont.from_fasta(os.path.join(comp, f))
    return [s.sequence.encode() for s in cont.sequences]


def timed_matrix(seqs, ctx, reps, env=None):
    old = {}
    for k, v in (env or {}).items():
        old[k] = os.environ.get(k)
        os.environ[k] = str(v)
    try:
        gx.compare_matrix(seqs, ctx=ctx)   # warm-up: buffers into the pool
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            mat = gx.compare_matrix(seqs, ctx=ctx)
            times.append((time.perf_counter() - t0) * 1e3)
        info = gx.compare_info(ctx)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    rec = {"ms_min": min(times), "ms_median": sorted(times)[len(times) // 2], "reps": reps, **info}
    rec["run_byte_compares_per_s"] = info["byte_compares"] / (info["run_ms"] * 1e-3) if info["run_ms"] else None
    return rec, mat


def host_matrix(seqs, threads):
    pairs = [(i, j) for j in range(len(seqs)) for i in range(j + 1)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        res = list(ex.map(lambda p: gx.compare_pair(seqs[p[0]], seqs[p[1]], host=True), pairs))
    return (time.perf_counter() - t0) * 1e3, dict(zip(pairs, res))


def candidates(seqs, threads, floor):
    """Candidate starts of every sub-problem with at least `floor` cells."""
    def walk(p):
        out, stack = [], [(seqs[p[0]], seqs[p[1]])]
        while stack:
            a, b = stack.pop()
            if not a or not b:
                continue
            if len(a) * len(b) >= floor:
                out.append((len(a) * len(b), gx.common_substring_candidates_host(a, b)[1]))
            i, j, n = gx.common_substring_host(a, b)
            if n:
                stack.append((a[:i], b[:j]))
                stack.append((a[i + n:], b[j + n:]))
        return out
    pairs = [(i, j) for j in range(len(seqs)) for i in range(j + 1)]
    with ThreadPoolExecutor(threads) as ex:
        return [x for r in ex.map(walk, pairs) for x in r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--candidates", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    seqs = genomes()
    if args.candidates:
        rows = candidates(seqs, args.threads, 1)
        rec = {"what": "candidate starts per sub-problem of the ten-genome matrix recursion (host solver)",
               "by_min_cells": {}}
        for floor in (1, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20):
            c = sorted(x[1] for x in rows if x[0] >= floor)
            if c:
                rec["by_min_cells"][str(floor)] = {
                    "subproblems": len(c), "max": c[-1], "p99": c[int(0.99 * (len(c) - 1))], "median": c[len(c) // 2],
                    "over": {str(cap): sum(v > cap for v in c) for cap in (1, 2, 4, 8, 16, 32, 64, 128, 256)}}
        out = args.out or os.path.join(ROOT, "profiles", "compare_candidates.json")
    else:
        ctx = gx.Context(0)
        rec = {"what": "gx_compare_matrix on the ten genomes of tests/golden/comparison_data, one GPU",
               "segment_height": gx.compare_segment_height()}
        rec["gpu_default"], mat = timed_matrix(seqs, ctx, args.reps)
        host_ms, host = host_matrix(seqs, args.threads)
        for (i, j), r in host.items():
            assert (int(mat[j, i, 0]), int(mat[j, i, 3])) == r[:2], (i, j)
        rec["host_solver"] = {"ms": host_ms, "threads": args.threads, "cpus": os.cpu_count()}
        rec["host_over_gpu"] = host_ms / rec["gpu_default"]["ms_min"]
        if args.sweep:
            rec["sweep_host_cells"] = {str(v): timed_matrix(seqs, ctx, 3, {"GX_COMPARE_HOST_CELLS": v})[0]
                                       for v in (0, 1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20,
                                                 1 << 22, 1 << 24)}
            rec["sweep_segment_height"] = {str(v): timed_matrix(seqs, ctx, 3, {"GX_COMPARE_SEG_H": v})[0]
                                           for v in (128, 256, 512, 1024, 2048, 4096, 8192)}
            rec["sweep_cand_cap"] = {str(v): timed_matrix(seqs, ctx, 3, {"GX_COMPARE_CAND_CAP": v})[0]
                                     for v in (1, 4, 16, 64, 256)}
            rec["single_pair_segment_height"] = {}
            for v in (256, 1024, 4096):
                os.environ["GX_COMPARE_SEG_H"] = str(v)
                gx.common_substring(seqs[0], seqs[5], ctx=ctx)
                t0 = time.perf_counter()
                gx.common_substring(seqs[0], seqs[5], ctx=ctx)
                ms = (time.perf_counter() - t0) * 1e3
                info = gx.compare_info(ctx)
                rec["single_pair_segment_height"][str(v)] = {"ms": ms, "run_ms": info["run_ms"]}
            del os.environ["GX_COMPARE_SEG_H"]
            # one lone sub-problem of s x s cells: a whole GPU call against the host solver
            import random
            rng = random.Random(1)
            rec["single_subproblem_us"] = {}
            for s in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
                a = bytes(rng.choice(b"ACGT") for _ in range(s))
                b = bytes(rng.choice(b"ACGT") for _ in range(s))
                best = {}
                for name, fn in (("gpu", lambda: gx.common_substring(a, b, ctx=ctx)),
                                 ("host", lambda: gx.common_substring_host(a, b))):
                    fn()
                    ts = []
                    for _ in range(20):
                        t0 = time.perf_counter()
                        fn()
                        ts.append((time.perf_counter() - t0) * 1e6)
                    best[name] = min(ts)
                rec["single_subproblem_us"][str(s * s)] = best
        ctx.close()
        out = args.out or os.path.join(ROOT, "profiles", "compare_matrix.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
