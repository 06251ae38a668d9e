#!/bin/bash
# A/B build of the HIP library with extra -D flags: tools/ab_build.sh NAME -DFLAG... -> lemo_amd/csrc/build_ab/NAME.so
# (load it with LEMO_HIP_LIB=.../build_ab/NAME.so).  The sources are the Makefile's SRC list.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../lemo_amd/csrc"; mkdir -p build_ab/$NAME
SRC=$(sed -n 's/^SRC *:= *//p' Makefile)
[ -n "$SRC" ] || { echo "no SRC list in csrc/Makefile" >&2; exit 1; }
pids=(); OBJ=()
for f in $SRC; do
  o=build_ab/$NAME/${f%.hip}.o; OBJ+=($o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -fno-vectorize -DLEMO_NO_PACKED_FP32 -I../../include -Wno-unused-function "$@" -c $f -o $o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done                      # a failed compile ends the script
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_ab/$NAME.so "${OBJ[@]}"
echo built build_ab/$NAME.so
