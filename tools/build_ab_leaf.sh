#!/usr/bin/env bash
# A/B build of the library with the leaf-pair path compiled differently: nbody-simulation-parallel_amd/libnbody_hip_leafab.so
# (OUT=<name> in the environment for another file name).
#   tools/build_ab_leaf.sh -DNBX_LEAF_PACK=0        without packed small leaves (csrc/leaf_plan.h PackBlock)
# Select it for a Python tool with NBODY_HIP_LIBRARY=<path> (capi.py).  Measurement aid; not part of `make`.
# The Makefile lists the objects: they are compiled again as *_leafab.o, next to the default build's.
set -euo pipefail
cd "$(dirname "$0")/.."
OUT="${OUT:-libnbody_hip_leafab.so}"
make lib LIB="nbody-simulation-parallel_amd/$OUT" O=_leafab.o LEAF_DEFS="$*"
echo built "nbody-simulation-parallel_amd/$OUT" "($*)"
