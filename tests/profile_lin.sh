#!/bin/bash
# Measurements of the inplacer kernel (plo_lin.hip) on one MI355X, written to profiles/lin_* (or $LIN_PROFILE_OUT):
#   lin_kernel_stats.csv   rocprofv3 --kernel-trace --stats of one search of 10^6 seeds on 4x4x4_49_156_L (a run of its own)
#   lin_rates.txt          wall-clock candidates/s of bin/inplacer --gpu 1 against --gpu 0 with 16 OpenMP threads
#   lin_tril_ab.txt        `python bench.py --workload tril` on a build of the parent commit and on this tree, alternated
#                          in the same call (the trilinear kernel must not move); skipped without PARENT_TREE
# Usage: tests/profile_lin.sh [PARENT_TREE]   (PARENT_TREE: a checkout of the parent commit with libplinopt_hip.so built)
# Needs bin/inplacer and plinopt_amd/libplinopt_hip.so built.  Every GPU step has its own time limit; the first failure ends
# the script.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:-}
OUT=${LIN_PROFILE_OUT:-$R/profiles}
F=$R/tests/golden/data/4x4x4_49_156_L.sms
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}

# 1. kernel trace and statistics of a fixed search (10^6 seeds from seed 0)
T=$(mktemp -d)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o lin -- "$R/bin/inplacer" --gpu 1 --seed 0 -O 1000000 "$F" > /dev/null 2> "$OUT/lin_rocprof.err"
S=$(find "$T" -name '*kernel_stats.csv' | head -1)
cp "$S" "$OUT/lin_kernel_stats.csv"
rm -rf "$T"

# 2. candidates/s, wall clock of the tool (the restart line of its report)
rate() {   # label, loops, command...
    local label=$1 n=$2; shift 2
    local t0 t1
    t0=$(date +%s.%N)
    "$@" > /dev/null 2> "$OUT/lin_rate_$label.err"
    t1=$(date +%s.%N)
    python3 -c "import sys; n, a, b = int(sys.argv[2]), float(sys.argv[3]), float(sys.argv[4]); print('%s %d candidates in %.3f s: %.4g candidates/s' % (sys.argv[1], n, b - a, n / (b - a)))" "$label" "$n" "$t0" "$t1" >> "$OUT/lin_rates.txt"
    grep 'restarts on' "$OUT/lin_rate_$label.err" | sed "s/^/  $label: /" >> "$OUT/lin_rates.txt"
}
: > "$OUT/lin_rates.txt"
rate gpu1 1000000 timeout -k 10 300 "$R/bin/inplacer" --gpu 1 --seed 0 -O 1000000 "$F"
rate host16 50000 env OMP_NUM_THREADS=16 timeout -k 10 300 "$R/bin/inplacer" --gpu 0 --seed 0 -O 50000 "$F"

# 3. the trilinear workload, parent build against this tree, alternated
if [ -n "$PARENT" ]; then
    : > "$OUT/lin_tril_ab.txt"
    for k in 1 2 3; do
        for side in parent branch; do
            D=$R; [ $side = parent ] && D=$PARENT
            echo -n "$side $k " >> "$OUT/lin_tril_ab.txt"
            (cd "$D" && timeout -k 10 300 python3 bench.py --gpus 1 --workload tril --no-cpu-baseline) | tail -1 >> "$OUT/lin_tril_ab.txt"
        done
    done
fi
ls -l "$OUT"/lin_*
