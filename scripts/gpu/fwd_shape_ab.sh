#!/bin/bash
# MFMA-shape evidence for the headline forward kernel, all on ONE box, one call:
#   1. scripts/ubench/kloop_model_v6: bare stream and full K-loop model on v_mfma_f32_32x32x16_f16 and v_mfma_f32_16x16x32_f16;
#   2. same-box A/B of two builds of the library, alternating, three rounds (python bench.py --steps 6 --warmup 2);
#   3. counters of both builds, each set in a run of its own (rocprofv3 --pmc ... --kernel-trace only):
#      GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES -> effective clock, matrix-pipe share;
#      SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -> LDS bank-conflict share.
# Arguments: the reference build and the build under test, relative to the repo root, and the output directory (default: a
# directory under TMPDIR).  Every step runs under its own time limit and the first failure ends the job.
# scripts/pmc_summary.py reduces the counter tables.
set -o pipefail
BASE=${1:-scripts/ubench/lib/libgpde_base.so}
NEW=${2:-graph-pde_amd/libgpde.so}
R=$PWD
O=${3:-${TMPDIR:-/tmp}/fwd_shape}
case $O in /*) ;; *) O=$R/$O ;; esac
mkdir -p $O
B="python $R/bench.py --no-cpu-baseline --no-alt --no-mgkn --no-reuse-probe --no-backward-probe"
timeout -k 10 240 scripts/ubench/kloop_model_v6 > $O/kloop_model_shapes.txt 2>&1 || exit 1
tail -1 $O/kloop_model_shapes.txt
: > $O/ab.txt
one() {
  GPDE_LIB=$R/$1 timeout -k 10 240 $B --steps 6 --warmup 2 2>/dev/null | tail -1 > $O/_line.json || return 1
  python -c "import json; d=json.load(open('$O/_line.json')); print('$1', d['value'], d['roofline']['frac'], d['roofline']['avg_launch_ms'])" | tee -a $O/ab.txt
}
for rep in 1 2 3; do
  one $BASE || exit 1
  one $NEW || exit 1
done
rm -f $O/_line.json
cd /tmp && export TMPDIR=/tmp
pmc() {      # tag, library, counters...
  local tag=$1 lib=$2; shift 2
  GPDE_LIB=$R/$lib timeout -k 10 300 rocprofv3 --output-format csv --pmc "$@" --kernel-trace -d $O/pmc_$tag -o run -- $B --steps 2 --warmup 1 > $O/pmc_$tag.log 2>&1 || return 1
}
pmc clock_base $BASE GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES || exit 1
pmc clock_new $NEW GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES || exit 1
pmc lds_base $BASE SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE || exit 1
pmc lds_new $NEW SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE || exit 1
cd $R
python scripts/pmc_summary.py $O clock_base clock_new lds_base lds_new | tee $O/pmc_summary.txt
find $O -type f -size +2M -delete
