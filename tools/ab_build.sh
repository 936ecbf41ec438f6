#!/bin/bash
# build a variant library: ab_build.sh <name> <file.hip[,file2.hip...]> <flags...>; result deeprecommendation_amd/libncf_hip_<name>.so
# The named files are compiled with the extra flags, every other object is the main build's (run the normal build first).
set -e
NAME=$1; SRCS=",$2,"; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
cd "$ROOT/deeprecommendation_amd/csrc"
mkdir -p build/$NAME
ALL=$(sed -n 's/^SOURCES = \[\(.*\)\]$/\1/p' build.py | tr -d '",')
for src in $ALL; do
  f=${src%.hip}
  if [[ "$SRCS" == *",$f.hip,"* ]]; then
    EXTRA=""; [[ "$f" == mlp_bf16* ]] && EXTRA="-mllvm -amdgpu-mfma-vgpr-form=1"
    $HIPCC --offload-arch=gfx950 -O3 -fPIC -std=c++17 $EXTRA "$@" -c $f.hip -o build/$NAME/$f.hip.o
    OBJS="$OBJS build/$NAME/$f.hip.o"
  else
    OBJS="$OBJS build/$f.hip.o"
  fi
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libncf_hip_$NAME.so $OBJS
echo built ../libncf_hip_$NAME.so
