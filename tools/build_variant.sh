#!/bin/bash
# Build a kernel-variant copy of libetamd.so for same-box A/B runs:
#     tools/build_variant.sh <name> <source.hip> "<extra hipcc flags>"
# -> eigentrajectory_amd/variants/libetamd_<name>.so (git-ignored); select it with
#    ET_LIBETAMD=$PWD/eigentrajectory_amd/variants/libetamd_<name>.so
# The sources, their flags and the link line are csrc/Makefile's (target `variant`).
set -e
NAME=$1; SRC=$2; FLAGS=$3
R=$(cd "$(dirname "$0")/.." && pwd)
make -C "$R/eigentrajectory_amd/csrc" -s variant NAME="$NAME" SRC="$SRC" FLAGS="$FLAGS"
echo "$R/eigentrajectory_amd/variants/libetamd_$NAME.so"
