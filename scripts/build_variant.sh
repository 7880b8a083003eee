#!/bin/bash
# Build an A/B variant of libsrhip.so with extra -D flags:  scripts/build_variant.sh NAME -DSOME_SWITCH=1 ...
# -> rusty_sr_amd/build/variants/libsrhip_NAME.so (select it with SRHIP_LIB=...; build/ travels to the GPU box, exp/ does not).
# Only one object is rebuilt, the stage kernels' unless SRC names another source: SRC=<dir>/sr_grad.hip takes that file (a scratch copy
# of rusty_sr_amd/csrc/sr_grad.hip, say, for a damaged build that is never committed) in place of the source of the same file name.
# The other objects are those of the last build_lib().
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
SRC=${SRC:-rusty_sr_amd/csrc/sr_kernels.hip}
BASE=$(basename "$SRC" .hip)
V=rusty_sr_amd/build/variants
mkdir -p $V
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -pthread -Irusty_sr_amd/csrc "$@" -x hip -c "$SRC" -o $V/${BASE}_$NAME.o
# every other object of the library, whatever rusty_sr_amd/build.py's SOURCES lists today
OTHERS=$(ls rusty_sr_amd/build/*.o | grep -v "/$BASE\.hip\.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -pthread $V/${BASE}_$NAME.o $OTHERS -ldl -o $V/libsrhip_$NAME.so
rm -f $V/${BASE}_$NAME.o
echo $V/libsrhip_$NAME.so
