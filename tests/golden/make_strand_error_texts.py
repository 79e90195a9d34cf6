"""Record the refusals of the stranded calls (gx_revcomp_batch and the six _strands searches): return code and
full gx_last_error() of every case of tests/strand_error_cases.py on a host index, into strand_error_texts.json.

    python tests/golden/make_strand_error_texts.py

As make_search_error_texts.py: the file is a record of what the library said when it was made, not of what it
should say: run it again only when an error text is meant to change, against the library that has the wanted
texts.  tests/test_strands_host.py and tests/test_gpu_strands.py hold the host index and the device to it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "genomics-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gxamd  # noqa: E402
from strand_error_cases import TEXT, cases, run_case  # noqa: E402


def main():
    idx = gxamd.SuffixIndex(TEXT, host=True)
    out = {}
    for cid, call, over in cases():
        rc, text = run_case(gxamd, idx, None, call, over)
        assert rc != 0 and cid not in out, (cid, rc)
        out[cid] = {"rc": rc, "text": text}
    idx.close()
    with open(os.path.join(HERE, "strand_error_texts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(out)} refusals recorded")


if __name__ == "__main__":
    main()
