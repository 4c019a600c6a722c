#!/bin/bash
# build_variant.sh NAME "EXTRA HIPFLAGS" -> tfhe-rs-odd_amd/build/NAME/libtfhe_mi355.so
# The Makefile's sources and flags (the max-ilp scheduler of pbs_multibit / pbs_latency included; MB_SCHED in
# the environment replaces it), objects and library in build/NAME.
set -e
cd "$(dirname "$0")/../tfhe-rs-odd_amd"
d=build/$1
make -j"${JOBS:-8}" OBJDIR="$d" LIBDIR="$d" EXTRA_HIPFLAGS="$2" ${MB_SCHED+MB_SCHED="$MB_SCHED"} "$d/libtfhe_mi355.so"
echo built $d
