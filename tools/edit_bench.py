#!/usr/bin/env python3
"""Measures the edit search (gx_suffix_index_search_edit) and
writes profiles/suffix_edit.json.

Protocol of tools/approx_bench.py: median of 5 whole calls after one warm-up,
the host clock around the synchronising call, beside the device times of
gx_edit_info of the median call (seed_ms: pieces, interval kernel, total and
candidate offsets; verify_ms: the band kernel; dedupe_ms: scan, emit, sort,
heads, fill, scatter and starts).  Per input: 1,048,576 reads of about 32, 100
and 150 bases cut from it, read r with r mod (k + 1) edits planted at distinct
columns, substitution, insertion and deletion in turn, for k = 1, 2, 3; counts
only, max_hits = 16 with starts and max_hits = 16 without; and 1 and 1,024 reads
of 100 bases at k = 2 for the launch floor.  The two yardsticks are taken in the
same run and the same build: search_approx of the same batch at the same k
(what the band and the dedupe add over the word walk), and the host index on
one thread (max_hits = 16 with starts, once).  Every device row is compared
equal with the host's.  A row that passes GX_APPROX_CAND_BUDGET is recorded as
refused, with the total the refusal names.

"rest_ms" = whole call - seed_ms - verify_ms - dedupe_ms: staging, the two
waits for the totals, and the copies.

    python tools/edit_bench.py [--out profiles/suffix_edit.json] [--inputs covid,chr12,synthetic]
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
from search_bench import ACGT, median_call  # noqa: E402
from suffix_bench import GOLDEN, chr12, first_record, synthetic  # noqa: E402

HIT_FIELDS = ("count", "best_dist", "best_end", "candidates")


def reads_of(s: bytes, nreads: int, m: int, k: int, seed: int):
    """(packed, offsets): nreads reads cut as m bases from s, read r with r % (k + 1) edits, the j-th of them at a
    random column of the j-th of k equal stretches of the read, its kind (r + j) % 3: a substitution changes the
    base, an insertion puts a different base behind it, a deletion drops it."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(s, np.uint8)
    starts = rng.integers(0, len(s) - m + 1, nreads)
    reads = a[starts[:, None] + np.arange(m)[None, :]]
    copies = np.ones((nreads, m), np.int64)   # 0: deleted, 2: an inserted base behind it
    edits = np.arange(nreads) % (k + 1)
    for j in range(k):
        lo, hi = j * m // k, (j + 1) * m // k
        rows = np.flatnonzero(edits > j)
        col = rng.integers(lo, hi, len(rows))
        kind = (rows + j) % 3
        sub = kind == 0
        reads[rows[sub], col[sub]] = ACGT[(np.searchsorted(ACGT, reads[rows[sub], col[sub]]) + 1) % 4]
        copies[rows[kind == 1], col[kind == 1]] = 2
        copies[rows[kind == 2], col[kind == 2]] = 0
    flat = np.repeat(reads.reshape(-1), copies.reshape(-1))
    last = np.cumsum(copies.reshape(-1)) - 1           # where a cell's last copy went
    ins = last[copies.reshape(-1) == 2]
    flat[ins] = ACGT[(np.searchsorted(ACGT, flat[ins]) + 1) % 4]
    off = np.zeros(nreads + 1, np.uint64)
    np.cumsum(copies.sum(axis=1), out=off[1:])
    return np.ascontiguousarray(flat), off


def same(a: dict, b: dict, fields=None) -> bool:
    return all((a[f] is None and b[f] is None) or np.array_equal(a[f], b[f]) for f in (fields or a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suffix_edit.json"))
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
            approx_ms, approx_refused = None, False
            try:
                approx_ms, _ = median_call(lambda: dev.search_approx(pats, k, max_hits=16))
            except gx.GxError as e:
                if e.code != 3:
                    raise
                approx_refused = True
            h, host_ms, refused = None, None, None
            try:
                t0 = time.perf_counter()
                h = host.search_edit(pats, k, max_hits=16)
                host_ms = (time.perf_counter() - t0) * 1e3
            except gx.GxError as e:
                if e.code != 3:
                    raise
                refused = re.search(r"(\d+) (seed hits|reported ends before dedupe)", str(e)).group(0)
            for max_hits, starts in ((0, False), (16, True), (16, False)):
                b = {"reads": nreads, "m": m, "k": k, "max_hits": max_hits, "starts": starts,
                     "search_approx_call_ms_median": None if approx_refused else round(approx_ms, 4)}
                if refused is not None:
                    try:
                        dev.search_edit(pats, k, max_hits=max_hits, starts=starts)
                        raise SystemExit("the device admitted a batch the host index refused")
                    except gx.GxError as e:
                        assert e.code == 3 and refused.split()[1] in str(e), str(e)
                    info = gx.edit_info(ctx)
                    b.update(refused="GX_ERANGE: over GX_APPROX_CAND_BUDGET (" + refused + " on the host)",
                             candidates_per_pattern=round(info["candidates"] / nreads, 2),
                             pre_dedupe_ends_per_pattern=round(info["pre_dedupe_ends"] / nreads, 2),
                             seed_ms=round(info["seed_ms"], 4), verify_ms=round(info["verify_ms"], 4))
                else:
                    def call():
                        r = dev.search_edit(pats, k, max_hits=max_hits, starts=starts)
                        return r, gx.edit_info(ctx)
                    ms, (r, info) = median_call(call)
                    dev_ms = info["seed_ms"] + info["verify_ms"] + info["dedupe_ms"]
                    b.update({"call_ms_median": round(ms, 4), "seed_ms": round(info["seed_ms"], 4),
                              "verify_ms": round(info["verify_ms"], 4), "dedupe_ms": round(info["dedupe_ms"], 4),
                              "rest_ms": round(ms - dev_ms, 4),
                              "patterns_per_s_call": round(nreads / (ms * 1e-3)),
                              "candidates_per_pattern": round(info["candidates"] / nreads, 3),
                              "pre_dedupe_ends_per_pattern": round(info["pre_dedupe_ends"] / nreads, 3),
                              "cell_updates_per_candidate": round(info["cell_updates"] / max(info["candidates"], 1), 2),
                              "cell_bound_per_candidate_m_2k1": m * (2 * k + 1),
                              "cell_updates_per_s_verify": round(info["cell_updates"] / max(info["verify_ms"] * 1e-3, 1e-9)),
                              "found": int((r["count"] > 0).sum()),
                              "occurrences": int(r["hit_offsets"][-1]) if max_hits else 0,
                              "call_over_search_approx": None if approx_refused else round(ms / approx_ms, 3),
                              "host_ms_one_thread_with_starts": round(host_ms, 3),
                              "host_over_gpu": round(host_ms / ms, 3),
                              "equal_to_host": (same(r, {**h, "starts": h["starts"] if starts else None}) if max_hits
                                                else same(r, h, HIT_FIELDS))})
                batches.append(b)
                print(json.dumps(b), flush=True)
        row["batches"] = batches
        rows.append(row)
        dev.close()
        host.close()
    ctx.close()
    doc = {"tool": "tools/edit_bench.py",
           "timing": "median of 5 whole calls after one warm-up, host clock; seed_ms / verify_ms / dedupe_ms are device "
                     "time of the median call; search_approx of the same batch (max_hits = 16) and the host index "
                     "(max_hits = 16 with starts, once, one thread) in the same run, same machine",
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
