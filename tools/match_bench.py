#!/usr/bin/env python3
"""Measures matching statistics and MEMs (gx_suffix_index_match_stats,
gx_suffix_index_mems) and writes profiles/suffix_match.json.

Protocol of tools/search_bench.py: median of 5 whole calls after one warm-up,
the host clock around the synchronising call, beside the device times of
gx_match_info of the median call (stats_ms: the matching-statistics kernel;
seed_ms: interval kernel, scan, keep, counts; emit_ms: emit, sort, pack).

Workloads: each of the ten comparison genomes as the query against every other
one's index and Covid_Wuhan against itself (the near-identical worst case),
matching statistics at the default max_len and MEMs at min_len 12, 20 and 32 with
a capacity known from a counts-only call; and a seeded 1 Mi-base query, cut from
a seeded 16 Mi-base synthetic text in 64 Ki-base pieces and mutated once per
~100 bases, against that text.  The two yardsticks are taken in the same run:
the host index on one thread (once), compared equal with the device, and for
MEMs the exact search (counts only) of the query's min_len-mers staged as
patterns, which is what |Q| copies of the query would cost.

    python tools/match_bench.py [--out profiles/suffix_match.json] [--inputs genomes,synthetic]
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
from search_bench import ACGT, median_call  # noqa: E402
from suffix_bench import GOLDEN, first_record, synthetic  # noqa: E402

MIN_LENS = (12, 20, 32)
STAT_FIELDS = ("len", "lo", "count", "pos")
MEM_FIELDS = ("qpos", "tpos", "length", "mem_offsets", "candidates")


def same(a, b, fields):
    return all(np.array_equal(a[f], b[f]) for f in fields)


def mers_of(q: bytes, L: int):
    """Every L-mer of q as a pattern batch: (packed, offsets)."""
    a = np.frombuffer(q, np.uint8)
    k = len(q) - L + 1
    return np.ascontiguousarray(a[np.arange(k)[:, None] + np.arange(L)[None, :]]).reshape(-1), \
        np.arange(k + 1, dtype=np.uint64) * np.uint64(L)


def mutated_query(s: bytes, total: int, piece: int, every: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    a = np.frombuffer(s, np.uint8)
    parts = [a[i:i + piece].copy() for i in rng.integers(0, len(s) - piece, total // piece)]
    q = np.concatenate(parts)
    pos = rng.choice(len(q), len(q) // every, replace=False)
    q[pos] = ACGT[(np.searchsorted(ACGT, q[pos]) + 1) % 4]
    return q.tobytes()


def measure(ctx, dev, host, q: bytes, max_len: int, with_mers: bool = True):
    """The rows of one (text, query) pair."""
    rows = []
    t0 = time.perf_counter()
    hs = host.matching_stats([q], max_len=max_len)
    host_ms = (time.perf_counter() - t0) * 1e3

    def stats_call():
        r = dev.matching_stats([q], max_len=max_len)
        return r, gx.match_info(ctx)
    ms, (r, info) = median_call(stats_call)
    rows.append({"what": "stats", "max_len": max_len, "call_ms_median": round(ms, 4), "stats_ms": round(info["stats_ms"], 4),
                 "rest_ms": round(ms - info["stats_ms"], 4), "word_steps": info["word_compares"],
                 "word_steps_per_position": round(info["word_compares"] / len(q), 2),
                 "max_len_found": int(r["len"].max()), "mean_len": round(float(r["len"].mean()), 2),
                 "positions_per_s_call": round(len(q) / (ms * 1e-3)),
                 "host_ms_one_thread": round(host_ms, 3), "host_over_gpu": round(host_ms / ms, 3),
                 "equal_to_host": same(r, hs, STAT_FIELDS)})
    for L in MIN_LENS:
        t0 = time.perf_counter()
        hm = host.mems([q], L)
        host_ms = (time.perf_counter() - t0) * 1e3
        cap = max(1, int(hm["mem_offsets"][-1]))

        def mems_call():
            r = dev.mems([q], L, max_mems=cap)
            return r, gx.match_info(ctx)
        ms, (r, info) = median_call(mems_call)
        cms, _ = median_call(lambda: dev.mems([q], L, max_mems=0))
        b = {"what": "mems", "min_len": L, "call_ms_median": round(ms, 4), "counts_only_call_ms_median": round(cms, 4),
             "seed_ms": round(info["seed_ms"], 4), "emit_ms": round(info["emit_ms"], 4),
             "rest_ms": round(ms - info["seed_ms"] - info["emit_ms"], 4),
             "candidates": info["candidates"], "kept": info["kept"], "mems": int(r["mem_offsets"][-1]),
             "longest_mem": int(r["length"].max()) if len(r["length"]) else 0, "word_steps": info["word_compares"],
             "host_ms_one_thread": round(host_ms, 3), "host_over_gpu": round(host_ms / ms, 3),
             "equal_to_host": same(r, hm, MEM_FIELDS)}
        if with_mers and len(q) >= L:
            pats = mers_of(q, L)
            sms, _ = median_call(lambda: dev.search(pats))
            b.update(exact_search_of_the_mers_call_ms_median=round(sms, 4), mers_search_over_mems_call=round(sms / ms, 3))
        rows.append(b)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_match.json"))
    ap.add_argument("--inputs", default="genomes,synthetic")
    ap.add_argument("--synthetic-mi", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=65535)
    ap.add_argument("--genomes", default="", help="comma-separated subset of the comparison genomes (default: all ten)")
    args = ap.parse_args()
    os.environ["GX_SUFFIX_HOST_BELOW"] = "0"
    os.environ.pop("GX_APPROX_CAND_BUDGET", None)   # the default budget
    ctx = gx.Context(0)
    doc = {"tool": "tools/match_bench.py",
           "timing": "median of 5 whole calls after one warm-up, host clock; stats_ms / seed_ms / emit_ms are device time "
                     "of the median call; the host index (once, one thread) and the exact search of the min_len-mers "
                     "(counts only) in the same run, same machine"}
    if "genomes" in args.inputs.split(","):
        d = os.path.join(GOLDEN, "comparison_data")
        names = sorted(f[:-6] for f in os.listdir(d) if f.endswith(".fasta"))
        if args.genomes:
            names = [n for n in names if n in args.genomes.split(",")]
        seqs = {n: first_record(os.path.join(d, n + ".fasta")) for n in names}
        pairs = []
        for tn in names:
            dev, host = gx.SuffixIndex(seqs[tn], ctx=ctx), gx.SuffixIndex(seqs[tn], host=True)
            for qn in names:
                if qn == tn and tn != "Covid_Wuhan":
                    continue
                row = {"text": tn, "n": len(seqs[tn]), "query": qn, "m": len(seqs[qn]),
                       "rows": measure(ctx, dev, host, seqs[qn], args.max_len)}
                pairs.append(row)
                print(json.dumps(row), flush=True)
            dev.close()
            host.close()
        doc["genome_pairs"] = pairs
        # what the README quotes: per workload the sums over the 90 cross pairs, and the self pair
        cross = [p for p in pairs if p["text"] != p["query"]]
        summary = []
        for k in range(1 + len(MIN_LENS)):
            rs = [p["rows"][k] for p in cross]
            s = {"what": rs[0]["what"], "pairs": len(rs), "call_ms_sum": round(sum(r["call_ms_median"] for r in rs), 3),
                 "host_ms_sum": round(sum(r["host_ms_one_thread"] for r in rs), 3),
                 "call_ms_max": max(r["call_ms_median"] for r in rs), "call_ms_min": min(r["call_ms_median"] for r in rs),
                 "all_equal_to_host": all(r["equal_to_host"] for r in rs)}
            if rs[0]["what"] == "mems":
                s.update(min_len=rs[0]["min_len"], candidates=sum(r["candidates"] for r in rs), kept=sum(r["kept"] for r in rs),
                         mers_search_call_ms_sum=round(sum(r["exact_search_of_the_mers_call_ms_median"] for r in rs), 3))
            summary.append(s)
        doc["genome_pairs_summary"] = summary
    if "synthetic" in args.inputs.split(","):
        mi = args.synthetic_mi
        s = synthetic(mi << 20, mi)
        q = mutated_query(s, 1 << 20, 1 << 16, 100, mi + 1)
        t0 = time.perf_counter()
        dev = gx.SuffixIndex(s, ctx=ctx)
        dev_build = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host = gx.SuffixIndex(s, host=True)
        row = {"text": f"synthetic_{mi}Mi_seed{mi}", "n": len(s), "query": "1Mi cut in 64Ki pieces, one substitution per 100",
               "m": len(q), "device_index_build_ms": round(dev_build, 1),
               "host_index_build_ms": round((time.perf_counter() - t0) * 1e3, 1)}
        print(json.dumps(row), flush=True)
        row["rows"] = measure(ctx, dev, host, q, args.max_len)
        print(json.dumps(row), flush=True)
        doc["synthetic"] = row
        dev.close()
        host.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
