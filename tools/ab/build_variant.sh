#!/bin/bash
# usage: bash tools/ab/build_variant.sh NAME SOURCE [extra hipcc flags...]  -> tools/ab/lib_NAME.so = the in-tree objects with csrc/SOURCE.hip
# (pwgemm, pwntred, pwntv1, pwwgrad, pwbnbwd, ...) rebuilt under the flags
set -e
R=$(cd "$(dirname "$0")/../.." && pwd); C=$R/mobilenet-yolo-pytorch_amd/csrc; N=$1; S=${2%.hip}; shift 2
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function "$@" -c $C/$S.hip -o $T/$S.o      # (set -e: a failed compile stops here)
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $R/tools/ab/lib_$N.so $T/$S.o $(ls $C/_obj/*.o | grep -v "/$S\.o$")
