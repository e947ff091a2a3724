#!/bin/bash
# tuning builds: bash tools/variants.sh name "-DRR_PX=4 -DRR_TY=8" ...   -> rectdetect_amd/variants/lib<name>.so, selected at run time by RD_LIB_PATH
# The library's own Makefile with -DRD_TUNING (the switches of the experiments: rd_detector.h) and the caller's defines on every HIP unit, objects in a directory of the variant's.
set -e
csrc="$(cd "$(dirname "$0")/../rectdetect_amd/csrc" && pwd)"
name=$1; shift
mkdir -p "$csrc/../variants"
make -j8 -C "$csrc" BUILD="$csrc/build/var_$name" OUT="$csrc/../variants/lib$name.so" EXTRA_HIPFLAGS="-DRD_TUNING $*"
echo built "$csrc/../variants/lib$name.so"
