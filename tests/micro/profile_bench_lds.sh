#!/bin/bash
# The rocprofv3 PMC passes of bench.py (BASELINE config 2) for the fill kernel that reads its letters from LDS,
# k_fill16l<8, false, 3, true>, the kernel the planner launches for config 2 (pw_plan.h, lds_feed): each counter set in a run of
# its own, --kernel-trace only, as profile_bench_group.sh collects them for the grouped kernel.  Run on the GPU box from the repo
# root; every pass prints a line first, and a pass that fails ends the script.
#
#     bash tests/micro/profile_bench_lds.sh [output directory, default build/profl]
#
# Writes <output directory>/pmc_kernel.json in the format bench.py reads (copy it to profiles/ to have roofline.traffic /
# valu_* reported).
set -e
R=$PWD
export TMPDIR=/tmp
O=$R/${1:-build/profl}
rm -rf $O; mkdir -p $O
cd /tmp
for c in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU" "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY" "SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU" "WRITE_SIZE" "FETCH_SIZE"; do
  n=$(echo $c | tr ' ' '_')
  echo "pass $c"
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/pmc_$n -- python3 $R/bench.py --inflight 1 --steps 2 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_$n.log 2>&1
done
cd $R
python3 tests/micro/pmc_sum.py $O "k_fill16l<8, false, 3, true>" --json $O/pmc_kernel.json --library-name "k_fill16<8, false> x4 matrix" --pairs 10000
