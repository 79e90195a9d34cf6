#!/usr/bin/env python3
"""Measures the chaining of a long query's anchors (gx_chain_anchors)
and writes profiles/suffix_chain.json.

Protocol of tools/search_bench.py: median of 5 whole calls after one warm-up,
the host clock around the synchronising call, beside the device times of
gx_chain_info of the median call (score_ms: flags, scan, segments, score;
chain_ms: best, heads, scans, counts, walk).  A whole call is one
gx_chain_anchors with scores, preds, chains and members at a capacity known
from a counts-only call, on anchors that already sit in one array.

Workloads: the MEMs at min_len 12 and 20 of each of the ten comparison genomes
against every other one's index (90 pairs; `mems` alone beside mems and chain);
the anchors at min_len 12, 20 and 32 of the seeded 1 Mi-base mutated query on the
seeded 16 Mi-base text of tools/match_bench.py; a synthetic batch of 4,096
queries with 1,000 anchors each; one query whose anchors form a single
unbroken segment of a million.  The host solver (ctx = NULL, one thread) runs
once on every workload and is compared equal with the device.

    python tools/chain_bench.py [--out profiles/suffix_chain.json] [--inputs genomes,synthetic,batch,segment]
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
from match_bench import mutated_query  # noqa: E402
from search_bench import median_call  # noqa: E402
from suffix_bench import GOLDEN, first_record, synthetic  # noqa: E402

FIELDS = ("score", "pred", "members", "chain_offsets", "member_off", "score_chain", "n_anchors", "root", "end", "qstart",
          "tstart", "qend", "tend")


class Raw:
    """One batch of anchors with its arrays made once: call() is gx_chain_anchors alone."""

    def __init__(self, anchors, **params):
        self.p = gx.CChainParams(**{**gx.CHAIN_DEFAULTS, **params})
        self.off = np.ascontiguousarray(anchors["mem_offsets"], np.uint64)
        self.nq, A = len(self.off) - 1, len(anchors["qpos"])
        self.an = np.zeros(max(A, 1), gx.MEM_DTYPE)
        self.an["qpos"][:A], self.an["tpos"][:A], self.an["len"][:A] = anchors["qpos"], anchors["tpos"], anchors["length"]
        self.A = A
        self.score, self.pred = np.zeros(max(A, 1), np.int32), np.zeros(max(A, 1), np.uint32)
        self.coff, self.mtot = np.zeros(self.nq + 1, np.uint64), ctypes.c_uint64()
        self.ch, self.mem = None, None

    def call(self, ctx, full=True):
        c, m = (self.ch, self.mem) if full else (None, None)
        gx._check(gx.lib().gx_chain_anchors(ctx.ptr if ctx else None, self.an.ctypes.data, self.off.ctypes.data, self.nq,
                                            ctypes.byref(self.p), self.score.ctypes.data, self.pred.ctypes.data,
                                            c.ctypes.data if c is not None else None, len(c) if c is not None else 0,
                                            m.ctypes.data if m is not None else None, len(m) if m is not None else 0,
                                            self.coff.ctypes.data, ctypes.byref(self.mtot)))

    def size(self, ctx):
        self.call(ctx, full=False)
        self.ch = np.zeros(max(1, int(self.coff[-1])), gx.CHAIN_DTYPE)
        self.mem = np.zeros(max(1, int(self.mtot.value)), np.uint32)

    def snapshot(self):
        K, M = int(self.coff[-1]), int(self.mtot.value)
        return (self.score[:self.A].copy(), self.pred[:self.A].copy(), self.coff.copy(), self.ch[:K].copy(), self.mem[:M].copy())


def measure(ctx, anchors, **params):
    """The row of one batch of anchors."""
    raw = Raw(anchors, **params)
    raw.size(ctx)

    def dev_call():
        raw.call(ctx)
        return gx.chain_info(ctx)
    ms, info = median_call(dev_call)
    got = raw.snapshot()
    cms, _ = median_call(lambda: raw.call(ctx, full=False))
    t0 = time.perf_counter()
    raw.call(None)
    host_ms = (time.perf_counter() - t0) * 1e3
    want = raw.snapshot()
    K = int(raw.coff[-1])
    row = {"queries": raw.nq, "anchors": raw.A, "params": {**gx.CHAIN_DEFAULTS, **params}, "segments": info["segments"],
           "pair_evals": info["pair_evals"], "chains": K, "members": int(raw.mtot.value),
           "longest_chain": int(raw.ch["n_anchors"][:K].max()) if K else 0,
           "best_score": int(raw.ch["score"][:K].max()) if K else 0,
           "call_ms_median": round(ms, 4), "counts_only_call_ms_median": round(cms, 4),
           "score_ms": round(info["score_ms"], 4), "chain_ms": round(info["chain_ms"], 4),
           "rest_ms": round(ms - info["score_ms"] - info["chain_ms"], 4),
           "host_ms_one_thread": round(host_ms, 3), "host_over_gpu": round(host_ms / ms, 3),
           "equal_to_host": all(np.array_equal(a, b) for a, b in zip(got, want))}
    if info["score_ms"] > 0:
        row["segments_per_s_score"] = round(info["segments"] / (info["score_ms"] * 1e-3))
        row["pair_evals_per_s_score"] = round(info["pair_evals"] / (info["score_ms"] * 1e-3))
    return row


def with_mems(ctx, dev, q, L, **params):
    """mems alone beside mems and chain, both through the Python calls a user makes."""
    mms, m = median_call(lambda: dev.mems([q], L))
    cms, _ = median_call(lambda: dev.chain_mems([q], L, **params))
    row = measure(ctx, m, **params)
    row.update(min_len=L, mems_call_ms_median=round(mms, 4), chain_mems_call_ms_median=round(cms, 4))
    return row


def batch_anchors(nq, n, seed):
    """nq queries of n anchors: a noisy diagonal with repeat noise beside it, about one anchor in four."""
    rng = np.random.default_rng(seed)
    q = np.cumsum(rng.integers(1, 60, (nq, n)), axis=1)
    t = q + rng.integers(-8, 9, (nq, n)) + 1000
    noise = rng.random((nq, n)) < 0.25
    t = np.where(noise, rng.integers(0, 60000, (nq, n)), t)
    return {"qpos": q.reshape(-1).astype(np.uint32), "tpos": t.reshape(-1).astype(np.uint32),
            "length": rng.integers(12, 40, nq * n).astype(np.uint32), "mem_offsets": np.arange(nq + 1, dtype=np.uint64) * np.uint64(n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_chain.json"))
    ap.add_argument("--inputs", default="genomes,synthetic,batch,segment")
    ap.add_argument("--synthetic-mi", type=int, default=16)
    ap.add_argument("--genomes", default="", help="comma-separated subset of the comparison genomes (default: all ten)")
    args = ap.parse_args()
    inputs = args.inputs.split(",")
    os.environ["GX_SUFFIX_HOST_BELOW"] = "0"
    os.environ.pop("GX_APPROX_CAND_BUDGET", None)   # the default budget
    ctx = gx.Context(0)
    doc = {"tool": "tools/chain_bench.py",
           "timing": "median of 5 whole calls after one warm-up, host clock; score_ms / chain_ms are device time of the "
                     "median call; the host solver (once, one thread) in the same run, same machine"}
    if "genomes" in inputs:
        d = os.path.join(GOLDEN, "comparison_data")
        names = sorted(f[:-6] for f in os.listdir(d) if f.endswith(".fasta"))
        if args.genomes:
            names = [n for n in names if n in args.genomes.split(",")]
        seqs = {n: first_record(os.path.join(d, n + ".fasta")) for n in names}
        pairs = []
        for tn in names:
            dev = gx.SuffixIndex(seqs[tn], ctx=ctx)
            for qn in names:
                if qn == tn:
                    continue
                row = {"text": tn, "query": qn, "rows": [with_mems(ctx, dev, seqs[qn], L) for L in (12, 20)]}
                pairs.append(row)
                print(json.dumps(row), flush=True)
            dev.close()
        doc["genome_pairs"] = pairs
        summary = []
        for k, L in enumerate((12, 20)):
            rs = [p["rows"][k] for p in pairs]
            summary.append({"min_len": L, "pairs": len(rs), "anchors": sum(r["anchors"] for r in rs),
                            "chains": sum(r["chains"] for r in rs),
                            "call_ms_sum": round(sum(r["call_ms_median"] for r in rs), 3),
                            "call_ms_min": min(r["call_ms_median"] for r in rs), "call_ms_max": max(r["call_ms_median"] for r in rs),
                            "host_ms_sum": round(sum(r["host_ms_one_thread"] for r in rs), 3),
                            "mems_call_ms_sum": round(sum(r["mems_call_ms_median"] for r in rs), 3),
                            "chain_mems_call_ms_sum": round(sum(r["chain_mems_call_ms_median"] for r in rs), 3),
                            "all_equal_to_host": all(r["equal_to_host"] for r in rs)})
        doc["genome_pairs_summary"] = summary
        print(json.dumps(summary), flush=True)
    if "synthetic" in inputs:
        mi = args.synthetic_mi
        s = synthetic(mi << 20, mi)
        q = mutated_query(s, 1 << 20, 1 << 16, 100, mi + 1)
        dev = gx.SuffixIndex(s, ctx=ctx)
        rows = []
        for L in (12, 20, 32):
            rows.append(with_mems(ctx, dev, q, L))
            print(json.dumps(rows[-1]), flush=True)
        dev.close()
        doc["synthetic"] = {"text": f"synthetic_{mi}Mi_seed{mi}", "query": "1Mi cut in 64Ki pieces, one substitution per 100",
                            "rows": rows}
    if "batch" in inputs:
        doc["batch_4096x1000"] = measure(ctx, batch_anchors(4096, 1000, 23))
        print(json.dumps(doc["batch_4096x1000"]), flush=True)
    if "segment" in inputs:
        n = 1 << 20
        one = {"qpos": np.arange(n, dtype=np.uint32) * np.uint32(20), "tpos": np.arange(n, dtype=np.uint32) * np.uint32(20) + np.uint32(7),
               "length": np.full(n, 15, np.uint32), "mem_offsets": np.array([0, n], np.uint64)}
        row = measure(ctx, one)
        row["score_ns_per_step"] = round(row["score_ms"] * 1e6 / n, 2)
        row["chain_ns_per_member"] = round(row["chain_ms"] * 1e6 / n, 2)
        doc["one_segment_1Mi"] = row
        print(json.dumps(row), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
