#!/bin/bash
# A/B builds of the one-block kernel's table-path unit (wf_kernels_ll.hip, -DWF_LL_PART=1: the two-slot kernels 2x2 and 4x2):
#   tools/build_alt.sh NAME [extra hipcc flags]  -> build/alt/lib_NAME.so
# The unit is compiled with the Makefile's flags for it (FLAGS, SETLL, SETLLTAB) followed by the extra flags — a later -D wins —
# and linked with the product's other objects as they stand, the on-the-fly part included.  The replay's switches:
#   -DWF_LL_TRANS_WAIT=0|1|2   where the transverse pass waits for its pair records (compiler / once per source / once per slot)
#   -DWF_LL_COLD_DEPTH=1|2     cold records one / two near steps ahead
#   -DWF_LL_BLOCK_EDGE=0|1|2|3 a block's first-chunk wait: bit 0 index / yaw prefetches behind it, bit 1 the previous block's output stores behind it
#   -DWF_EXP_NOCOLD            timing only, wrong results: the deficit pass without its cold-record loads
#   LICM=1 tools/build_alt.sh ...   leaves machine LICM on for the unit
# Time with the library copied over wfcrl-env_amd/libwfstep.so (bench.py) or tools/time_variants.py build/alt/lib_*.so on the
# GPU box.  build/ is not committed.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
C=wfcrl-env_amd/csrc
make -s -j8 -C $C > /dev/null
flags() { make -s -C $C --eval "print-flags: ; @echo \$($1)" print-flags; }
F="$(flags FLAGS) $(flags SETLL)"
[ -n "$LICM" ] || F="$F $(flags SETLLTAB)"
mkdir -p build/alt
/opt/rocm/bin/hipcc $F -DWF_LL_PART=1 "$@" -c -o build/alt/ll_$name.o $C/wf_kernels_ll.hip
objs=$(ls $C/*.o $C/*/*.o | grep -v -e "^$C/wf_kernels_ll.o" -e "^$C/check/")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o build/alt/lib_$name.so build/alt/ll_$name.o $objs
echo built build/alt/lib_$name.so
