#!/bin/bash
# Mutation check of the rotating overlapped pipeline's stream order
# (gx_api_batch.cpp pipeline_rotate): builds
# genomics-rs_amd/build_var/libgx_amd_rotate_nowait.so from the current
# objects with gx_api_batch.cpp compiled under -DGX_MUT_NO_ROTATE_WAIT
# (fill i's stream then no longer waits for walk i - 3, the last reader of the
# buffers it refills; the host has only collected fill i - 3's results).
# Run on the GPU, once:
#     GX_LIB=genomics-rs_amd/build_var/libgx_amd_rotate_nowait.so python -m pytest -m gpu tests/test_gpu_overlap_rotate.py
# and compare with the normal library, which passes.  In steady state walk
# i - 3 ended two launches before fill i can start, so the race may also pass
# (profiles/r08_rotate_mutation.txt has what happened).  Needs `make` run first.
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)/genomics-rs_amd
D=$R/build_var
mkdir -p "$D"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -DGX_MUT_NO_ROTATE_WAIT \
    -c -o "$D/gx_api_batch_rotate_nowait.o" "$R/csrc/gx_api_batch.cpp"
OBJS=$(ls "$R"/build/*.o | grep -v '/gx_api_batch.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -o "$D/libgx_amd_rotate_nowait.so" $OBJS \
    "$D/gx_api_batch_rotate_nowait.o"
rm -f "$D/gx_api_batch_rotate_nowait.o"
echo "built $D/libgx_amd_rotate_nowait.so (rotation: wait on walk i - 3 removed)"
