#!/usr/bin/env python3
"""Measures the approximate search (gx_suffix_index_search_approx)
and writes profiles/suffix_approx.json.

Protocol of tools/search_bench.py: median of 5 whole calls after one warm-up,
the host clock around the synchronising call, beside the device times of
gx_approx_info of the median call (seed_ms: pieces, interval kernel, total and
candidate offsets; verify_ms: verify and compact).  Per input: 1,048,576 reads
of 32, 100 and 150 bases cut from it, read r with r mod (k + 1) substitutions
planted at distinct columns, for k = 1, 2, 3, counts only and with
max_hits = 16, and 1 and 1,024 reads of 100 bases at k = 2 for the launch floor.
The host index runs the batch with positions once on one thread of the same
machine; both device rows are compared equal with it in the same run (the
counts-only row on the four hit fields).  Beside every (m, k) stands the exact
search of the same batch in the same build: what the pieces and the verify add
over k = 0.  A row whose seed hits pass GX_APPROX_CAND_BUDGET is recorded as
refused, with the total the refusal names.

"rest_ms" = whole call - seed_ms - verify_ms: staging, the wait for the total,
copies and, with positions, the host's per-pattern sort.

    python tools/approx_bench.py [--out profiles/suffix_approx.json] [--inputs covid,chr12,synthetic]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gxamd as gx  # noqa: E402
from search_bench import ACGT, median_call, same  # noqa: E402
from suffix_bench import GOLDEN, chr12, first_record, synthetic  # noqa: E402

HIT_FIELDS = ("count", "best_dist", "best_pos", "candidates")


def reads_of(s: bytes, nreads: int, m: int, k: int, seed: int):
    """(packed, offsets): nreads reads of m bases cut from s, read r with r % (k + 1) substitutions, the j-th of
    them at a random column of the j-th of k equal stretches of the read (so they are distinct)."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(s, np.uint8)
    starts = rng.integers(0, len(s) - m + 1, nreads)
    reads = a[starts[:, None] + np.arange(m)[None, :]]
    subs = np.arange(nreads) % (k + 1)
    for j in range(k):
        lo, hi = j * m // k, (j + 1) * m // k
        rows = np.flatnonzero(subs > j)
        col = rng.integers(lo, hi, len(rows))
        reads[rows, col] = ACGT[(np.searchsorted(ACGT, reads[rows, col]) + 1) % 4]
    return reads.reshape(-1), np.arange(nreads + 1, dtype=np.uint64) * np.uint64(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_approx.json"))
    ap.add_argument("--inputs", default="covid,chr12,synthetic")
    ap.add_argument("--synthetic-mi", type=int, default=16)
    ap.add_argument("--reads", type=int, default=1 << 20)
    args = ap.parse_args()
    os.environ["GX_SUFFIX_HOST_BELOW"] = "0"
    os.environ.pop("GX_APPROX_CAND_BUDGET", None)   # the default budget
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
        dev = gx.SuffixIndex(s, ctx=ctx)
        t0 = time.perf_counter()
        host = gx.SuffixIndex(s, host=True)
        row = {"input": name, "n": len(s), "host_index_build_ms": round((time.perf_counter() - t0) * 1e3, 1)}
        print(json.dumps(row), flush=True)
        batches = []
        shapes = [(args.reads, m, k) for m in (32, 100, 150) for k in (1, 2, 3)] + [(1, 100, 2), (1024, 100, 2)]
        for nreads, m, k in shapes:
            pats = reads_of(s, nreads, m, k, 1000 * k + m)
            exact_ms, _ = median_call(lambda: dev.search(pats, max_hits=16))
            h, host_ms, refused = None, None, None
            try:
                t0 = time.perf_counter()
                h = host.search_approx(pats, k, max_hits=16)
                host_ms = (time.perf_counter() - t0) * 1e3
            except gx.GxError as e:
                if e.code != 3:
                    raise
                refused = int(re.search(r"(\d+) seed hits", str(e)).group(1))
            for max_hits in (0, 16):
                b = {"reads": nreads, "m": m, "k": k, "max_hits": max_hits, "exact_search_call_ms_median": round(exact_ms, 4)}
                if refused is not None:
                    try:
                        dev.search_approx(pats, k, max_hits=max_hits)
                        raise SystemExit("the device admitted a batch the host index refused")
                    except gx.GxError as e:
                        assert e.code == 3 and f"{refused} seed hits" in str(e), str(e)
                    b.update(refused="GX_ERANGE: over GX_APPROX_CAND_BUDGET", seed_hits=refused,
                             candidates_per_pattern=round(refused / nreads, 2), seed_ms=round(gx.approx_info(ctx)["seed_ms"], 4))
                else:
                    def call():
                        r = dev.search_approx(pats, k, max_hits=max_hits)
                        return r, gx.approx_info(ctx)
                    ms, (r, info) = median_call(call)
                    b.update({"call_ms_median": round(ms, 4), "seed_ms": round(info["seed_ms"], 4),
                              "verify_ms": round(info["verify_ms"], 4),
                              "rest_ms": round(ms - info["seed_ms"] - info["verify_ms"], 4),
                              "patterns_per_s_call": round(nreads / (ms * 1e-3)),
                              "candidates_per_pattern": round(info["candidates"] / nreads, 3),
                              "word_steps_per_candidate": round(info["word_compares"] / max(info["candidates"], 1), 3),
                              "found": int((r["count"] > 0).sum()),
                              "positions": int(r["hit_offsets"][-1]) if max_hits else 0,
                              "call_over_exact_search": round(ms / exact_ms, 3),
                              "host_ms_one_thread_with_positions": round(host_ms, 3),
                              "host_over_gpu": round(host_ms / ms, 3),
                              "equal_to_host": same(r, h) if max_hits else all(np.array_equal(r[f], h[f]) for f in HIT_FIELDS)})
                batches.append(b)
                print(json.dumps(b), flush=True)
        row["batches"] = batches
        rows.append(row)
        dev.close()
        host.close()
    ctx.close()
    doc = {"tool": "tools/approx_bench.py",
           "timing": "median of 5 whole calls after one warm-up, host clock; seed_ms / verify_ms are device time of the "
                     "median call; the host index runs the batch with max_hits = 16 once, one thread, same machine",
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
