#!/usr/bin/env python3
"""Writes tests/golden/compare_digests.json from the host solver of compare
mode (gx_compare_pair without a context, no device; pinned by
tests/test_compare_host.py):

  matrix     (score, first_lcs) of every pair i <= j of the ten genomes of
             tests/golden/comparison_data, files in name order
  synthetic  three related pairs of length 2,048 (the sequences are stored,
             so that the tests do not depend on the generator's random stream)

Usage: python tests/golden/make_compare_digests.py [--threads N]"""
import argparse
import json
import os
import random
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for sub in ("oracle", "genomics-rs_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))


def related_pair(rng, length, sub_rate, indel_rate):
    a = [rng.choice("ACGT") for _ in range(length)]
    b = []
    for c in a:
        r = rng.random()
        if r < sub_rate:
            b.append(rng.choice("ACGT"))
        elif r < sub_rate + indel_rate:
            if rng.random() < 0.5:
                b.extend([c, rng.choice("ACGT")])
        else:
            b.append(c)
    b = (b + [rng.choice("ACGT") for _ in range(length)])[:length]
    return "".join(a), "".join(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 1)
    args = ap.parse_args()
    import gxamd as gx
    import oracle
    comp = os.path.join(HERE, "comparison_data")
    names, seqs = [], []
    for f in sorted(os.listdir(comp)):
        if f.endswith(".fasta"):
            with open(os.path.join(comp, f), "rb") as fh:
                for name, s in oracle.fasta_parse(fh.read()):
                    names.append(name.decode() if isinstance(name, bytes) else name)
                    seqs.append(s)
    pairs = [(i, j) for j in range(len(seqs)) for i in range(j + 1)]
    with ThreadPoolExecutor(args.threads) as ex:
        res = list(ex.map(lambda p: gx.compare_pair(seqs[p[0]], seqs[p[1]], host=True), pairs))
    matrix = [{"i": i, "j": j, "score": r[0], "first_lcs": r[1], "calls": r[2]} for (i, j), r in zip(pairs, res)]
    rng = random.Random(20240)
    synthetic = []
    for sub_rate, indel_rate in ((0.02, 0.005), (0.10, 0.02), (0.30, 0.05)):
        a, b = related_pair(rng, 2048, sub_rate, indel_rate)
        r = gx.compare_pair(a.encode(), b.encode(), host=True)
        synthetic.append({"a": a, "b": b, "score": r[0], "first_lcs": r[1], "calls": r[2]})
    out = {"source": "host solver (gx_compare_pair, ctx = NULL); tests/golden/make_compare_digests.py",
           "names": names, "lengths": [len(s) for s in seqs], "matrix": matrix, "synthetic": synthetic}
    with open(os.path.join(HERE, "compare_digests.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
