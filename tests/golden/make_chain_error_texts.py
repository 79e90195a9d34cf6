"""Record the refusals of gx_chain_anchors: return code and full gx_last_error() of every case of
tests/chain_error_cases.py on the host solver (ctx = NULL), into chain_error_texts.json.

    python tests/golden/make_chain_error_texts.py

As make_extend_error_texts.py: the file is a record of what the library said when it was made, not of what it
should say: run it again only when an error text is meant to change, against the library that has the wanted
texts.  tests/test_chain_host.py and tests/test_gpu_chain.py hold the host solver and the device driver to it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gxamd  # noqa: E402
from chain_error_cases import cases, run_case  # noqa: E402


def main():
    out = {}
    for cid, over in cases():
        rc, text = run_case(gxamd, None, over)
        assert rc != 0 and cid not in out, (cid, rc)
        out[cid] = {"rc": rc, "text": text}
    with open(os.path.join(HERE, "chain_error_texts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(out)} refusals recorded")


if __name__ == "__main__":
    main()
