#!/bin/bash
# rocprofv3 kernel stats + PMC passes (one counter block set per pass, no tracing beside the counters) of a bench
# workload, summarised per kernel with tools/pmc_summary.py (run on the GPU box from the repo root).
#   tools/prof.sh TAG SCENE "KERNEL1 KERNEL2 ..." [extra bench args]
# FRT_PROF_TREE: the checkout whose bench.py runs and whose device sources stamp the summaries (default: this
# one; a worktree of the parent commit for the "before" pass of an A/B). The output goes to this checkout's
# output directory (prof_TAG) either way.
set -o pipefail
TAG=$1; SC=$2; KS=$3; shift 3
R=${GRAFT_REPO_ROOT:-$(pwd)}
T=${FRT_PROF_TREE:-$R}
OUT=$R/gpurun_out/prof_$TAG
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
B="--scene $SC --gi-steps 0 --no-cpu-baseline --no-render-multi --no-scaling-proxy --shipped-steps 0 $*"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -f csv -d "$OUT/kt" -o run -- \
    python3 "$T/bench.py" --steps 3 --warmup 1 $B > "$OUT/kt_bench.json" 2> "$OUT/kt_bench.err" || exit $?
KRE=$(echo $KS | tr ' ' '|')
pmc() {  # dir counters...
    local d=$1; shift
    timeout -s KILL 180 rocprofv3 --pmc "$@" --kernel-include-regex "$KRE" -f csv -d "$OUT/$d" -o run -- \
        python3 "$T/bench.py" --steps 1 --warmup 0 $B > "$OUT/$d.json" 2> "$OUT/$d.err"
}
pmc sq SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY || exit $?
pmc f64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_TRANS_F64 SQ_ACTIVE_INST_VALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_LDS || exit $?
pmc fetch FETCH_SIZE || exit $?
pmc write WRITE_SIZE || exit $?
pmc clk GRBM_GUI_ACTIVE GRBM_COUNT || exit $?
# requests, not bytes: what the L2 (TCC) took and what the vector L1s (TCP) sent it, reads and writes apart, and
# the cycles the address path stood behind the cache (a wave's store instruction is one TA wavefront and as many
# 64-byte requests as it touches pieces)
pmc l2 TCC_REQ_sum TCC_READ_sum TCC_WRITE_sum TCC_TAG_STALL_sum || exit $?
pmc tcp TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCP_TOTAL_READ_sum TCP_TOTAL_WRITE_sum || exit $?
pmc ta TA_FLAT_WRITE_WAVEFRONTS_sum TA_ADDR_STALLED_BY_TC_CYCLES_sum TCP_PENDING_STALL_CYCLES_sum || exit $?
cd "$T"
for K in $KS; do
    python3 tools/pmc_summary.py "$OUT" "$K" "$SC" > "$OUT/pmc_$K.json" || exit $?
done
ls "$OUT"
