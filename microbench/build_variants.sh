#!/bin/bash
# Build engine variants (compile-time switches of the engine's sources and headers under csrc/) next to
# each other for A/B timing on the GPU. The switches that remain are the numeric tuning constants in #ifndef form
# (PV_*_MINBLOCKS, PV_PREP_LDS_PAD, PV_SPARSE_*, PV_LP_CHAIN_BLOCKS, PV_KEY_SEED, PV_RANK_SUB,
# PV_LATENCY_MAX, PV_KEYED_HINT_MIN, PV_SEG_STRIDE, PV_COMB_MIN_REQ, PV_FUSED_MIN_REQ, PV_ENC_SMALL_B,
# PV_ENC16_MIN, PV_KC_*, PV_PIPE_*, PV_SIDE_GRID_PER_CU, and PV_BCOMB_W / PV_HALF_* / PV_ENC_BATCH_N in
# the headers) and the diagnostic builds (PV_CLOCK_PROBE, PV_LAT_TRACE, PV_BOUNDS_CHECK,
# PV_ENABLE_TEST_HOOKS). The variant switches of settled A/B experiments (kernel forms, priorities,
# stream layouts) are gone: DESIGN.md "Variants tried and retired" lists them, their results and the
# commit that still holds their code.
#   microbench/build_variants.sh NAME "-DFLAG=.. ..." [NAME "FLAGS" ...]  -> microbench/variants/NAME.so
# Each variant is the library's Makefile run with EXTRA (the flags), BUILD and OUT: every source in its
# SRC is recompiled with the flags, not only the engine, so a switch in a shared header reaches every
# translation unit that reads it. Load one with PLENUM_AMD_LIB=microbench/variants/NAME.so
# (tests/perf_quick.py, bench.py).
cd "$(dirname "$0")/../indy-plenum_amd" || exit 1
mkdir -p ../microbench/variants
pids=()
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  V=../microbench/variants/$name
  ( make -j4 EXTRA="$flags" BUILD=$V.build OUT=$V.so $V.so && rm -rf $V.build ) > $V.build.txt 2>&1 &
  pids+=($!)
done
rc=0
for p in "${pids[@]}"; do wait $p || rc=1; done
exit $rc
