#!/bin/bash
# The rocprofv3 PMC passes of bench.py (BASELINE config 2) for the fill kernel with one running-best key per two cells,
# k_fill16p<8, false, 3, true>, the kernel the planner launches for config 2 (pw_plan.h, pair_keys): each counter set in a run of
# its own with NO tracing beside it (counters only), otherwise as profile_bench_lds.sh collects them for k_fill16l.  Run on the
# GPU box from the repo root; every pass prints a line first, and a pass that fails ends the script.
#
#     bash tests/micro/profile_bench_pairs.sh [output directory, default build/profp] [kernel, default k_fill16p<8, false, 3, true>]
#
# Writes <output directory>/pmc_kernel.json in the format bench.py reads (copy it to profiles/ to have roofline.traffic /
# valu_* reported).  With another kernel as the second argument (and, say, PWLIB_PAIR_KEYS=0 in the environment) the same
# passes describe that kernel.
set -e
R=$PWD
export TMPDIR=/tmp
O=$R/${1:-build/profp}
K=${2:-"k_fill16p<8, false, 3, true>"}
rm -rf $O; mkdir -p $O
cd /tmp
for c in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU" "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY" "SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU" "WRITE_SIZE" "FETCH_SIZE"; do
  n=$(echo $c | tr ' ' '_')
  echo "pass $c"
  timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d $O/pmc_$n -- python3 $R/bench.py --inflight 1 --steps 2 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_$n.log 2>&1
done
cd $R
python3 tests/micro/pmc_sum.py $O "$K" --json $O/pmc_kernel.json --library-name "k_fill16<8, false> x4 matrix" --pairs 10000
