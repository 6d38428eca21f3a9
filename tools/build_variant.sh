#!/bin/bash
# A/B builds of the library: tools/build_variant.sh NAME [-DSVO_...=n ...]  ->  build_ab/NAME.so  (run with SVO_HIP_LIB, tools/ab2.sh)
# The Makefile's own rule builds it, with its sources and FLAGS plus the extra arguments.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/octree-tracer_amd/csrc
flags=$(make -s --no-print-directory -C "$csrc" --eval='_flags: ; @echo $(FLAGS)' _flags)
mkdir -p "$root/build_ab"
make -s --no-print-directory -B -C "$csrc" OUT="$root/build_ab/$name.so" FLAGS="$flags $*"
echo built build_ab/$name.so "$@"
