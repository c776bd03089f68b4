#!/usr/bin/env bash
# A/B build of the library WITH the measured-and-lost variants of the force kernel compiled in (this round's candidates under NBX_AB in
# csrc/force_kernel.hip; earlier rounds' lost variants live in the history): nbody-simulation-parallel_amd/libnbody_hip_ab.so.  Select it for a Python tool with NBODY_HIP_LIBRARY=<path>,
# e.g.  NBODY_HIP_LIBRARY=$PWD/nbody-simulation-parallel_amd/libnbody_hip_ab.so python tools/time_variants.py 1048576 4 fastpk
# Measurement aid; not part of `make`.  The Makefile lists the objects: they are compiled again as *_ab.o, next to the default build's.
set -euo pipefail
cd "$(dirname "$0")/.."
DEFS="${1:--DNBX_AB}"   # no candidate is compiled in at present: add table entries under #ifdef NBX_AB in force_kernel.hip
make lib LIB=nbody-simulation-parallel_amd/libnbody_hip_ab.so O=_ab.o FORCE_KERNEL_DEFS="$DEFS"
echo built nbody-simulation-parallel_amd/libnbody_hip_ab.so
