"""One process of profiles/batch_refactor_ab.json's A/B run: its four cases beside the bench.py headline, on the
library GX_LIB names; one JSON line.  Run it and `bench.py --gpus 1 --steps 10 --warmup 2` in alternating fresh
processes, the parent commit's library against the tree's."""
import json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "genomics-rs_amd"), os.path.join(ROOT, "oracle")]
import gxamd as gx
import bench

out = {"lib": os.environ.get("GX_LIB", "tree")}
scores = gx.Scores(*bench.SCORES)
rng = random.Random(77)
pairs1k = [(bytes(rng.choice(b"ACGT") for _ in range(1024)), bytes(rng.choice(b"ACGT") for _ in range(1024)))
           for _ in range(1024)]

# staged 1024 x 1k global, 10 steps: the three-slot pipeline with the walk on its own stream
ctx = gx.Context(0)
st = gx.StagedPairs(pairs1k, ctx=ctx)
st.run(scores, False, True, steps=2)
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    st.run(scores, False, True, steps=10)
    ts.append((time.perf_counter() - t0) / 10 * 1e3)
out["staged_1024x1k_ms_per_step"] = round(statistics.median(ts), 4)
out["staged_1024x1k_info"] = ctx.fill_info()
out["staged_1024x1k_scheme"] = ctx.overlap_scheme()
# one gx_align_batch of 1024 x 1k: the one-pass path
gx.align_batch(pairs1k, scores, False, ctx=ctx, max_cell=False)
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    gx.align_batch(pairs1k, scores, False, ctx=ctx, max_cell=False)
    ts.append((time.perf_counter() - t0) * 1e3)
out["align_batch_1024x1k_ms"] = round(statistics.median(ts), 4)
ctx.close()
# the tracked Covid config of bench.py --full
ctx = gx.Context(0)
r = bench.config_record(gx, ctx, "covid", 5, tracked=True)
out["covid_tracked_ms_per_step"] = r["ms_per_step"]
out["covid_tracked_fill_ms"] = r["fill_ms_avg"]
out["covid_tracked_bit_exact"] = r["parity"]["bit_exact"]
ctx.close()
# the local batch record of bench.py --full (scheme 1)
ctx = gx.Context(0)
r = bench.local_batch_record(gx, ctx, 3)
out["local_batch_ms_per_step"] = r["ms_per_step"]
out["local_batch_fill_ms"] = r["fill_ms_avg"]
out["local_batch_scheme"] = ctx.overlap_scheme()
out["local_batch_bit_exact"] = r["parity"]["bit_exact"]
ctx.close()
print("ABCASE " + json.dumps(out), flush=True)
