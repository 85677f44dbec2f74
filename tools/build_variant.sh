#!/bin/bash
# Build an A/B variant of libnavenv.so with extra -D flags on some translation units (tuning
# only), through the package Makefile's UNIT hook: one flag list, one object list.
#   tools/build_variant.sh NAME "UNIT ..." "-DFOO=1 ..."
#   UNIT: learner | env | demo_reward | demo_index | demonstrator | mlpN (the row kernels of hidden width 32*N; mlp8 = 256) | mlp0 (the row
#   kernels' C-ABI object; "mlp0 mlp8" rebuilds the dispatch and the 256-wide kernels together) |
#   mlp8agpr (mlp8 without the scheduler / VGPR-form flags); NOSCHED=1 in the environment drops
#   those flags from every unit named
# -> abl/libnavenv_NAME.so, its objects in abl/NAME.build (bind it with
#    python tools/withlib.py abl/libnavenv_NAME.so SCRIPT ...)
# The learner unit's knobs: -DNAV_WG_SKEW_FACT=R / -DNAV_WG_SKEW_OPND=R (rows moved to the first
# wave of a SIMD pair per 256 rows), -DNAV_WGRAD_TRACE (tools/wgrad_trace.py).
set -eu
cd "$(dirname "$0")/.."
name=$1; flags=${3:-}; units=""; plain=${NOSCHED:-}
for u in $2; do
  case $u in
    learner) units="$units learner_kernels" ;;
    env) units="$units env_kernels" ;;
    demo_reward|demo_index|demonstrator) units="$units $u" ;;
    mlp0) units="$units mlp_abi" ;;
    mlp[1-8]) units="$units mlp_nt${u#mlp}" ;;
    mlp8agpr) units="$units mlp_nt8"; plain=1 ;;
    *) echo "unit?"; exit 2 ;;
  esac
done
make -s -j"${JOBS:-16}" -C residual-td3-robot-navigation_amd BUILD="$PWD/abl/$name.build" \
  LIB="$PWD/abl/libnavenv_$name.so" UNIT="$units" UNIT_EXTRA="$flags" UNIT_PLAIN="$plain"
echo abl/libnavenv_$name.so
