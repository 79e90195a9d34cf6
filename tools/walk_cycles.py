"""Cycles a block of the sequential strip walk (tb_seq_kernel's own counters,
gx_walk_info) with the table-driven chase and without it, on one unpipelined
pass of P synthetic pairs of length L: nothing runs beside the walk.
GX_TWIN_ROWS=2|4 picks the fill's rows a lane (the headline batch runs four).

    python tools/walk_cycles.py [--length 30000] [--pairs 8] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ.setdefault("GX_TWIN", "1")   # (a small batch: the twin fill the headline batch takes by itself)
    import bench
    import gxamd as gx
    ctx = gx.Context(0)
    pairs = bench.rank_pairs(0, a.pairs, a.length, False)
    st = gx.StagedPairs(pairs, ctx=ctx)
    scores = gx.Scores(*bench.SCORES)
    out = {"length": a.length, "pairs": a.pairs, "runs": []}
    ref = None
    for fast in ("1", "0", "1", "0"):
        os.environ["GX_TB_FAST"] = fast
        res, _ = st.run(scores, False, True, steps=1)
        info = ctx.walk_info()
        info["retrace_us"] = res[0].retrace_us
        info["fill_info"] = ctx.fill_info()
        key = [(r.score, r.n_steps, r.matches, r.mismatches, r.gap_extensions, r.opening_gaps) for r in res]
        ref = ref or key
        info["results_equal"] = key == ref
        out["runs"].append(info)
        print(json.dumps(info), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
