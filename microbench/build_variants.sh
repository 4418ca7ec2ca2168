#!/bin/bash
# Build engine variants (compile-time switches of csrc/pv_engine.hip) next to each other for A/B
# timing on the GPU. The switches that remain are the numeric tuning constants in #ifndef form
# (PV_*_MINBLOCKS, PV_PREP_LDS_PAD, PV_SPARSE_*, PV_LP_CHAIN_BLOCKS, PV_KEY_SEED, PV_RANK_SUB,
# PV_LATENCY_MAX, PV_KEYED_HINT_MIN, PV_SEG_STRIDE, PV_COMB_MIN_REQ, PV_FUSED_MIN_REQ, PV_ENC_SMALL_B,
# PV_ENC16_MIN, PV_KC_*, PV_PIPE_*, PV_SIDE_GRID_PER_CU, and PV_BCOMB_W / PV_HALF_* / PV_ENC_BATCH_N in
# the headers) and the diagnostic builds (PV_CLOCK_PROBE, PV_LAT_TRACE, PV_BOUNDS_CHECK,
# PV_ENABLE_TEST_HOOKS). The variant switches of settled A/B experiments (kernel forms, priorities,
# stream layouts) are gone: DESIGN.md "Variants tried and retired" lists them, their results and the
# commit that still holds their code.
#   microbench/build_variants.sh NAME "-DFLAG=.. ..." [NAME "FLAGS" ...]  -> microbench/variants/NAME.so
# Only the engine is recompiled with the flags; the other objects come from the in-tree build
# (make -C indy-plenum_amd first). Load one with PLENUM_AMD_LIB=microbench/variants/NAME.so
# (tests/perf_quick.py, bench.py).
cd "$(dirname "$0")/../indy-plenum_amd" || exit 1
mkdir -p ../microbench/variants
OTHERS="build/pv_latency.hip.o build/pv_ingress.hip.o build/host_prep.cpp.o build/signing_json.cpp.o"
for o in $OTHERS; do [ -f "$o" ] || { echo "missing $o: run make -C indy-plenum_amd" >&2; exit 1; }; done
pids=()
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  V=../microbench/variants/$name
  ( /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -Wall $flags -c -o $V.engine.o csrc/pv_engine.hip &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o $V.so $V.engine.o $OTHERS \
      -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib && rm -f $V.engine.o ) > $V.build.txt 2>&1 &
  pids+=($!)
done
rc=0
for p in "${pids[@]}"; do wait $p || rc=1; done
exit $rc
