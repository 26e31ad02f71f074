#!/bin/bash
# SQ / GRBM counters of the CURRENT kernels (run on the GPU box):  [SETS="3 4"] bash tools/pmc_sq_counters.sh <tag> [workload ...]
# One rocprofv3 --kernel-trace --pmc pass per counter set (never combined with other trace domains), the default bench command
# of each workload with --no-cpu; tools/summarize_sq.py turns the csv files into profiles/<tag>_<workload>_sq_counters.json.
# Set 3 is the row loops' control flow: executed branches and instruction fetches beside the parked cycles and the
# instruction counts they are set against, all in ONE pass so that the ratios come from the same launches; set 4 the fetch queue's
# depth and the instruction cache.  SETS picks the passes (default: all); the first pass that fails ends the script.
TAG=${1:-r04_a}; shift
WL=${@:-headline}
SETS=${SETS:-1 2 3 4}
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
SET1="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY"
SET2="SQ_WAIT_ANY SQ_INSTS_LDS SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD SQ_INSTS_SMEM SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE"
SET3="SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_BRANCH SQ_IFETCH"
SET4="SQ_IFETCH_LEVEL SQC_ICACHE_REQ SQC_ICACHE_MISSES"
for w in $WL; do
  O=$R/gpurun_out/$TAG/sq_$w
  mkdir -p $O
  for i in $SETS; do
    set=SET$i
    timeout -k 10 300 rocprofv3 --kernel-trace --pmc ${!set} --output-format csv -d $O/p$i -- python $R/bench.py --no-cpu --no-ref-width --workload $w --steps 3 --warmup 1 > $O/log$i.txt 2>&1 </dev/null \
      || { echo "counter set $i of $w failed: $O/log$i.txt"; tail -5 $O/log$i.txt; exit 1; }
  done
  python $R/tools/summarize_sq.py $O $R/gpurun_out/$TAG/${TAG}_${w}_sq_counters.json "$w"
  [ $? -eq 0 ] || exit 1
done
