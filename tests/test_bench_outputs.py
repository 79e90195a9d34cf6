"""bench.py's --dump-outputs and --full.  CPU: the dump's layout and its
seeded, bounded sample, on a stand-in for the staged batch.  GPU: a small
plain run prints the headline line only and dumps the last timed step's
results and alignments, which equal the oracle digests of the same synthetic
pairs (tests/golden/synthetic_L1024.json); --full adds the moved records."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

MOVED = ("parity", "byte_planes", "int32_planes", "no_plane_fill", "single_pair", "config2", "config3",
         "config2_tracked", "config3_tracked", "local_batch", "cpu_baseline", "cpu_baseline_all_cores")
NAMES = ["alignment.npy", "alignment_offsets.npy", "alignment_pairs.npy", "results.npy"]


class _Result:
    def __init__(self, k):
        self.score, self.matches, self.mismatches, self.gap_extensions, self.opening_gaps = -k, k, 1, 2, 3
        self.n_steps, self.start_i, self.start_j = 10 + k, 0, 0


class _Staged:
    """steps(p) as gxamd.StagedPairs gives them: `choice`, `i`, `j` per step."""

    def steps(self, p):
        a = np.zeros(10 + p, np.dtype([("choice", "u1"), ("pad", "u1", (7,)), ("i", "<u8"), ("j", "<u8")]))
        a["choice"], a["i"], a["j"] = p % 6, np.arange(10 + p), p
        return a


def _load(d):
    assert sorted(os.listdir(d)) == NAMES
    return {n[:-4]: np.load(os.path.join(d, n)) for n in NAMES}


def test_dump_outputs_layout(tmp_path):
    res = [_Result(k) for k in range(5)]
    bench.dump_outputs(str(tmp_path), _Staged(), res, 0, 1)
    d = _load(tmp_path)
    assert d["results"].dtype == np.float64 and d["results"].shape == (5, len(bench.DUMP_RESULT_FIELDS))
    assert d["results"][3].tolist() == [-3, 3, 1, 2, 3, 13, 0, 0]
    assert d["alignment"].dtype == np.float32 and d["alignment"].shape == (60, 3)
    assert d["alignment_pairs"].tolist() == [0, 1, 2, 3, 4]
    assert d["alignment_offsets"].tolist() == [0, 10, 21, 33, 46, 60]
    assert d["alignment"][21:33].tolist() == [[2, i, 2] for i in range(12)]


def test_dump_outputs_rank_suffix(tmp_path):
    bench.dump_outputs(str(tmp_path), _Staged(), [_Result(0)], 1, 2)
    assert sorted(os.listdir(tmp_path)) == sorted(n[:-4] + "_rank1.npy" for n in NAMES)


def test_dump_outputs_sample_is_seeded_and_bounded(tmp_path, monkeypatch):
    res = [_Result(k) for k in range(40)]
    monkeypatch.setattr(bench, "DUMP_ALIGNMENT_BYTES", 12 * 200)   # float32 rows of 12 B: 200 of the 1,180 steps
    bench.dump_outputs(str(tmp_path / "a"), _Staged(), res, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), _Staged(), res, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in a:
        assert np.array_equal(a[n], b[n])
    picked = [int(p) for p in a["alignment_pairs"]]
    assert 0 < len(picked) < 40 and len(set(picked)) == len(picked) and picked != sorted(picked)
    assert a["alignment"].nbytes <= 12 * 200 and a["results"].shape[0] == 40
    for x, p in enumerate(picked):
        rows = a["alignment"][int(a["alignment_offsets"][x]):int(a["alignment_offsets"][x + 1])]
        assert rows.shape[0] == 10 + p and np.all(rows[:, 2] == p)


def _run_bench(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GX_BENCH_PAIRS"):
        monkeypatch.delenv(v, raising=False)
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_headline_only_and_dump(gx, tmp_path, monkeypatch, capsys):
    P, L = 8, 1024
    out = _run_bench(monkeypatch, capsys, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--length", str(L),
                                           "--pairs-per-gpu", str(P), "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "GCUPS" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] > 0
    # value = cells / time per step; both are rounded to three decimals in the line
    assert abs(out["value"] - P * L * L / (out["ms_per_step"] * 1e-3) / 1e9) <= \
        out["value"] * 0.0006 / out["ms_per_step"] + 0.001
    assert not [k for k in MOVED if k in out]
    d = _load(tmp_path)
    with open(os.path.join(GOLDEN, f"synthetic_L{L}.json")) as f:
        gold = {c["k"]: c for c in json.load(f)["cases"]}
    assert d["alignment_pairs"].tolist() == list(range(P))
    for p in range(P):
        c = gold[p]
        assert d["results"][p, :6].tolist() == [c["score"]] + c["stats"] + [c["n_steps"]]
        rows = d["alignment"][int(d["alignment_offsets"][p]):int(d["alignment_offsets"][p + 1])]
        h = hashlib.sha256()
        h.update(bytes(rows[:, 0].astype(np.uint8)))
        h.update(rows[:, 1].astype("<u8").tobytes())
        h.update(rows[:, 2].astype("<u8").tobytes())
        assert h.hexdigest() == c["alignment_sha256"]


@pytest.mark.gpu
def test_full_run_adds_the_moved_records(gx, monkeypatch, capsys):
    out = _run_bench(monkeypatch, capsys, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--length", "1024",
                                           "--pairs-per-gpu", "8", "--full", "--no-cpu-baseline",
                                           "--config-steps", "0", "--local-batch-steps", "0"])
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["parity"]["pairs_checked"] == 8 and out["parity"]["timed_passes_checked"] == 2
    for k in ("single_pair", "no_plane_fill"):
        assert k in out
