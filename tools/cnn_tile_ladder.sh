#!/bin/bash
# Round 9: the band CNN's tile loop priced against its bare MFMA stream -- timing-only variants of the product kernel, each with ONE thing removed
# (band_cnn.hpp: CNN_EXP_*; results of the variants are WRONG by construction; DESIGN.md section 8, profiles/r9/cnn_tile_ladder.json).
#   CPU:      tools/cnn_tile_ladder.sh build [jobs]   -> build/cnn_ladder/lib_<variant>.so
#   GPU box:  tools/cnn_tile_ladder.sh run > cnn_tile_ladder.log     (interleaved with the product kernel, two runs each; stops at the first failure)
set -e -o pipefail
DIR=build/cnn_ladder
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -Wno-unused-value"
VARIANTS=${VARIANTS:-"base a_l0_b_once b_rem_b_once c_no_rem d_no_bperm e_no_relu_bias e1_no_relu e2_no_bias f_no_store g_all"}
defs() {
  case $1 in
    base) echo "" ;;
    a_l0_b_once) echo "-DCNN_EXP_L0_B_ONCE=1" ;;
    b_rem_b_once) echo "-DCNN_EXP_REM_B_ONCE=1" ;;
    c_no_rem) echo "-DCNN_REM4X4=0" ;;
    d_no_bperm) echo "-DCNN_EXP_NO_BPERM=1" ;;
    e_no_relu_bias) echo "-DCNN_EXP_NO_RELU_BIAS=3" ;;
    e1_no_relu) echo "-DCNN_EXP_NO_RELU_BIAS=1" ;;
    e2_no_bias) echo "-DCNN_EXP_NO_RELU_BIAS=2" ;;
    f_no_store) echo "-DCNN_EXP_NO_STORE=1" ;;
    g_all) echo "-DCNN_EXP_L0_B_ONCE=1 -DCNN_REM4X4=0 -DCNN_EXP_NO_RELU_BIAS=3 -DCNN_EXP_NO_STORE=1 -DCNN_EXP_STAGE_EVERY=1000000 -DCNN_EXP_NO_WFRAG=1" ;;
  esac
}
if [ "$1" = "build" ]; then
  mkdir -p $DIR
  JOBS=${2:-4}
  n=0
  for V in $VARIANTS; do
    /opt/rocm/bin/hipcc $FLAGS $(defs $V) -o $DIR/lib_$V.so llicti_amd/csrc/llicti_hip.hip &
    n=$((n + 1))
    if [ $((n % JOBS)) = 0 ]; then wait; fi
  done
  wait
  ls -la $DIR
else
  for rep in 1 2; do
    for V in $VARIANTS; do
      echo "== $V (run $rep)"
      LLICTI_HIP_SO=$PWD/$DIR/lib_$V.so timeout -k 10 120 python tools/bench_cnn.py 2>/dev/null | grep -E "lvl 0|total"
    done
  done
fi
