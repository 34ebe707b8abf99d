#!/bin/bash
# K-loop schedule evidence for the headline forward kernel ("The levelled K loop"), all on ONE box, one call:
#   model   scripts/ubench/kloop_model_v6: the full K-loop model batch-major against levelled, then levelled with two fragment sets
#           against four resident ones, alternating, four repetitions each;
#   bits    python bench.py --steps 2 --warmup 1 --dump-outputs of both builds at g61 and g241 (out.npy byte for byte), and
#           of --train --config g61 (every dumped array; BASE against BASE first: the parent's own distance is the bar);
#   ab      same-box A/B of the two builds, alternating, three pairs (python bench.py --steps 6 --warmup 2);
#   pmc     counters of both builds, each set in a run of its own (rocprofv3 --pmc ... --kernel-trace only):
#           GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES -> effective clock, matrix-pipe share;
#           SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -> LDS bank-conflict share;
#   phases  scripts/v6_timing.py g241 on the -DGPDE_V6_TIMING builds of both, where they exist next to the libraries
#           (libgpde_T6base.so / libgpde_T6.so under scripts/ubench/lib/).
# Arguments: the reference build and the build under test, relative to the repo root, the output directory (default: a
# directory under TMPDIR) and the parts to run (default: all five).  A build is a library, run through this checkout's
# Python (GPDE_LIB), or - where the two differ in their entry points - a directory that holds another checkout with its
# own library built: then its own bench.py runs (phases: libgpde_T6base.so with that checkout's scripts/v6_timing.py).
# Every step runs under its own time limit and the first
# failure ends the job; nothing is tried twice.  scripts/pmc_summary.py reduces the counter tables.
set -o pipefail
BASE=${1:-scripts/ubench/lib/libgpde_base.so}
NEW=${2:-graph-pde_amd/libgpde.so}
R=$PWD
O=${3:-${TMPDIR:-/tmp}/fwd_kloop}
PARTS=${4:-model bits ab pmc phases}
case $O in /*) ;; *) O=$R/$O ;; esac
mkdir -p $O
BOPT="--no-cpu-baseline --no-alt --no-mgkn --no-reuse-probe --no-backward-probe"
tree() { if [ -d $R/$1 ]; then echo $R/$1; else echo $R; fi; }                  # the checkout a build runs in
libof() { if [ -d $R/$1 ]; then echo $R/$1/graph-pde_amd/libgpde.so; else echo $R/$1; fi; }
has() { case " $PARTS " in *" $1 "*) return 0 ;; *) return 1 ;; esac; }

if has model; then
  timeout -k 10 240 scripts/ubench/kloop_model_v6 > $O/kloop_model.txt 2>&1 || exit 1
  grep -E "schedule A/B|fragment A/B|saved" $O/kloop_model.txt
fi

if has bits; then
  : > $O/bits.txt
  dump() {      # tag, library, bench arguments...
    local tag=$1 lib=$2; shift 2
    GPDE_LIB=$(libof $lib) timeout -k 10 400 python $(tree $lib)/bench.py $BOPT --steps 2 --warmup 1 --dump-outputs $O/dump_$tag "$@" > $O/dump_$tag.log 2>&1 || return 1
  }
  same() {      # two dump directories: every array byte for byte
    python - $O/dump_$1 $O/dump_$2 <<'EOF' | tee -a $O/bits.txt
import os, sys
import numpy as np
a, b = sys.argv[1:3]
for f in sorted(os.listdir(a)):
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    eq = x.tobytes() == y.tobytes()
    d = 0.0 if eq else float(np.linalg.norm(x.astype(np.float64) - y) / max(np.linalg.norm(y.astype(np.float64)), 1e-300))
    print(f"{os.path.basename(a)} vs {os.path.basename(b)}: {f} {x.shape} {'IDENTICAL' if eq else 'DIFFERENT rel-L2 %.3e' % d}")
EOF
  }
  dump g61_base $BASE --config g61 || exit 1
  dump g61_new $NEW --config g61 || exit 1
  same g61_base g61_new
  dump g241_base $BASE --config g241 || exit 1
  dump g241_new $NEW --config g241 || exit 1
  same g241_base g241_new
  dump train_base $BASE --train --config g61 || exit 1
  dump train_base2 $BASE --train --config g61 || exit 1
  dump train_new $NEW --train --config g61 || exit 1
  same train_base train_base2
  same train_base train_new
  rm -rf $O/dump_*/
fi

if has ab; then
  : > $O/ab.txt
  one() {
    GPDE_LIB=$(libof $1) timeout -k 10 240 python $(tree $1)/bench.py $BOPT --steps 6 --warmup 2 2>/dev/null | tail -1 > $O/_line.json || return 1
    python -c "import json; d=json.load(open('$O/_line.json')); print('$1', d['value'], d['roofline']['frac'], d['roofline']['avg_launch_ms'], d['roofline']['kernel'])" | tee -a $O/ab.txt
  }
  for rep in 1 2 3; do
    one $BASE || exit 1
    one $NEW || exit 1
  done
  rm -f $O/_line.json
  python - $O/ab.txt <<'EOF' | tee -a $O/ab.txt
import sys
v = [float(l.split()[1]) for l in open(sys.argv[1]) if l.strip()]
base, new = v[0::2], v[1::2]
spread = max(base) - min(base)
print("ratio new / parent per pair:", " ".join(f"{n / b:.4f}" for b, n in zip(base, new)),
      f"  parent spread {spread:.3f}, least gain {min(n - b for b, n in zip(base, new)):.3f} = {min(n - b for b, n in zip(base, new)) / max(spread, 1e-9):.1f} spreads")
EOF
fi

if has pmc; then
  cd /tmp && export TMPDIR=/tmp
  pmc() {      # tag, library, counters...
    local tag=$1 lib=$2; shift 2
    GPDE_LIB=$(libof $lib) timeout -k 10 300 rocprofv3 --output-format csv --pmc "$@" --kernel-trace -d $O/pmc_$tag -o run -- python $(tree $lib)/bench.py $BOPT --steps 2 --warmup 1 > $O/pmc_$tag.log 2>&1 || return 1
  }
  pmc clock_base $BASE GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES || exit 1
  pmc clock_new $NEW GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES || exit 1
  pmc lds_base $BASE SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE || exit 1
  pmc lds_new $NEW SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE || exit 1
  cd $R
  python scripts/pmc_summary.py $O clock_base clock_new lds_base lds_new | tee $O/pmc_summary.txt
fi

if has phases; then
  for t in T6base T6; do
    T=$R; [ $t = T6base ] && T=$(tree $BASE)
    if [ -f $R/scripts/ubench/lib/libgpde_$t.so ]; then
      GPDE_LIB=$R/scripts/ubench/lib/libgpde_$t.so timeout -k 10 400 python $T/scripts/v6_timing.py g241 2>/dev/null | sed "s/^/$t: /" | tee -a $O/phases.txt || exit 1
    fi
  done
fi
find $O -type f -size +2M -delete
