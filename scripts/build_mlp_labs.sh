#!/bin/bash
# Builds variants of libpn2ops.so with lab switches in the fused-MLP sources (A/B runs through PN2OPS_LIBRARY).
# Usage: scripts/build_mlp_labs.sh <source>[,<source>...] name:-DFLAG[,-DFLAG] ...   Development aid.
# <source>: a file of pointnet2_amd/csrc without .hip -- the one that holds the switch (a switch read in several translation
# units, like PN2_WG_TIMING in the weight-gradient files, takes them all). Exit status 1 if any variant failed to build.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRCS=${1//,/ }; shift
C=$ROOT/pointnet2_amd/csrc
mkdir -p "$ROOT/build_lab"
make -C "$C" -j8 > /dev/null
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -munsafe-fp-atomics -fPIC -mllvm -amdgpu-mfma-vgpr-form=1 -fno-honor-nans"
build_variant() {                       # name, defines: the sources with the defines, linked with every other object
    local name=$1 defs=$2 s keep objs=
    keep=$(ls "$C"/build/*.o | grep -v polllab)
    for s in $SRCS; do
        hipcc $FLAGS $defs -c "$C/$s.hip" -o "$ROOT/build_lab/${s}_$name.o" || return 1
        keep=$(echo "$keep" | grep -v "/$s.o"); objs="$objs $ROOT/build_lab/${s}_$name.o"
    done
    hipcc --offload-arch=gfx950 -shared -fPIC $keep $objs -o "$ROOT/build_lab/libpn2ops_$name.so" && rm $objs
}
pids=
for spec in "$@"; do
    name=${spec%%:*}; defs=${spec#*:}; defs=${defs//,/ }
    build_variant "$name" "$defs" &
    pids="$pids $!"
done
failed=0
for p in $pids; do wait $p || failed=1; done
ls -la "$ROOT/build_lab"
exit $failed
