"""Each of the five batch pipelines (gx_api_batch.cpp) once, on 20 pairs of fixed shapes:
the script of profiles/batch_refactor_ab.json's kernel trace.  GX_LIB names the library.
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/batch_pipelines_once.py
then tools/kernel_trace_counts.py OUT_A OUT_B."""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "genomics-rs_amd")]
import gxamd as gx

SHAPES20 = [(1300 + 97 * k, 1100 + 61 * ((k * 7) % 20)) for k in range(20)]
rng = random.Random(2025)
pairs = [(bytes(rng.choice(b"ACGT") for _ in range(n)), bytes(rng.choice(b"ACGT") for _ in range(m))) for n, m in SHAPES20]
scores = gx.Scores(1, -2, -1, -5)
os.environ["GX_TWIN"] = "1"
os.environ["GX_LAYOUT"] = "0"
ctx = gx.Context(0)
st = gx.StagedPairs(pairs, ctx=ctx)
seen = []
def run(name, local, steps, **env):
    for k in ("GX_OVERLAP", "GX_OVERLAP_ROTATE"):
        os.environ.pop(k, None)
    os.environ.update(env)
    st.run(scores, local, True, steps=steps, plane_sums=True)
    seen.append((name, ctx.fill_info()["groups"], ctx.overlap_scheme()))
gx.align_batch(pairs, scores, False, ctx=ctx, max_cell=False)     # the one-pass batch
run("one_pass_staged", False, 1, GX_OVERLAP="0")
run("two_slot_local", True, 3, GX_OVERLAP="0")
run("three_slot_global", False, 3, GX_OVERLAP="0")
run("scheme1", False, 3, GX_OVERLAP="1", GX_OVERLAP_ROTATE="0")
run("rotation", False, 3, GX_OVERLAP="1")
ctx.close()
print("TRACE5", seen, flush=True)
assert [s[1:] for s in seen] == [(1, 0), (1, 0), (1, 0), (2, 1), (2, 2)], seen
