"""Search mode's refusals, byte for byte: return code and full gx_last_error() of every case of
tests/search_error_cases.py against tests/golden/search_error_texts.json (recorded once by
tests/golden/make_search_error_texts.py).  The five entry points share their prologues, their batch checker and
their stages, so a text, or which of two refusals wins, can change for all of them at once; this file is what
notices.

  host index    every case, no GPU
  device index  (gpu) the refusals that arise inside the device drivers: GX_ECAP of each mode, the seed
                budget, the ends budget and the MEM candidate budget, on the same inputs and against the
                same strings, since host and device share the texts
  pool          (gpu) a refused call gives back what it took: in a fresh process with GX_LOG=debug every
                such call, and a successful one per mode, is issued twice, and the second finds every
                buffer it asks for in the context's pool
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from search_error_cases import TEXT, driver_cases, host_cases, run_case

with open(os.path.join(GOLDEN, "search_error_texts.json")) as f:
    WANT = json.load(f)

HOST = host_cases()
DRIVER = driver_cases()
SUCCESSES = [(f"{mode}-ok", mode, {"length": 2}) for mode in ("search", "approx", "edit", "stats", "mems")]


def test_fixture_covers_every_case():
    assert sorted(WANT) == sorted(c[0] for c in HOST) and len(WANT) == len(HOST)


@pytest.mark.parametrize("case", HOST, ids=[c[0] for c in HOST])
def test_host_refusal(gx, case):
    cid, mode, over = case
    idx = gx.SuffixIndex(TEXT, host=True)
    rc, text = run_case(gx, idx, mode, over)
    idx.close()
    assert (rc, text) == (WANT[cid]["rc"], WANT[cid]["text"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", DRIVER, ids=[c[0] for c in DRIVER])
def test_device_refusal(gx, ctx, case):
    cid, mode, over = case
    idx = gx.SuffixIndex(TEXT, ctx=ctx)
    rc, text = run_case(gx, idx, mode, over)
    ok = run_case(gx, idx, mode, {"length": 2})   # and the index goes on working
    idx.close()
    assert (rc, text) == (WANT[cid]["rc"], WANT[cid]["text"])
    assert ok[0] == 0


CHILD = """
import sys
import gxamd
from search_error_cases import TEXT, run_case
from test_search_errors import DRIVER, SUCCESSES
ctx = gxamd.Context(0)
idx = gxamd.SuffixIndex(TEXT, ctx=ctx)
for cid, mode, over in DRIVER + SUCCESSES:
    for call in (1, 2):
        print(f"== {cid} {call}", file=sys.stderr, flush=True)
        rc, _ = run_case(gxamd, idx, mode, over)
        print(f"== rc {rc}", file=sys.stderr, flush=True)
idx.close()
ctx.close()
"""


@pytest.mark.gpu
def test_refused_call_gives_back_what_it_took():
    env = dict(os.environ, GX_LOG="debug",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), os.path.join(ROOT, "genomics-rs_amd")]))
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    calls = {}   # "id call" -> (rc, its stderr lines)
    key = None
    for line in p.stderr.split("\n"):
        if line.startswith("== rc "):
            calls[key] = (int(line[6:]), calls[key])
        elif line.startswith("== "):
            key = line[3:]
            calls[key] = []
        elif key is not None and isinstance(calls[key], list):
            calls[key].append(line)
    assert len(calls) == 2 * len(DRIVER + SUCCESSES)
    # (the first call of all does miss: the log is there to be read)
    assert any("pool miss" in ln for ln in calls[f"{DRIVER[0][0]} 1"][1])
    for cid, _, _ in DRIVER + SUCCESSES:
        want_rc = WANT[cid]["rc"] if cid in WANT else 0
        for call in (1, 2):
            assert calls[f"{cid} {call}"][0] == want_rc, (cid, call, calls[f"{cid} {call}"])
        missed = [ln for ln in calls[f"{cid} 2"][1] if "pool miss" in ln]
        assert not missed, (cid, missed)
