#!/bin/bash
# Measurements of the orbiter's three actions (plo::orbit_kernel<MOD, ACT>, plo_orbit.hip) on one MI355X, written to
# profiles/orbit_action_* (or $ORBIT_PROFILE_OUT):
#   orbit_action_rates.txt         per action and input (2x2x2_7_Winograd, 4x4x4_49_156, 3x4x7_63_rational), 10^6 candidates from
#                                  seed 0 over Q: kernel time (the tool's HIP events) and candidates/s of bin/orbiter --gpu 1, wall
#                                  clock and candidates/s of the host loop (--gpu 0, 16 OpenMP threads) on the same candidates, and
#                                  whether the two runs agree byte for byte (winner line and written files).  With
#                                  $ORBIT_PARENT set to the root of a build of the parent commit (bin/orbiter and
#                                  plinopt_amd/libplinopt_hip.so): three runs each, alternating, of 10^6 triangular candidates
#                                  on 4x4x4_49_156 with the parent's build and with this one.
#   orbit_action_kernel_stats.csv  rocprofv3 --kernel-trace --stats of one search per action on 4x4x4_49_156 (runs of their own)
# Usage: tests/profile_orbit_actions.sh   (needs bin/orbiter and plinopt_amd/libplinopt_hip.so built).  The searches run on copies
# of the inputs.  Every GPU step has its own time limit; the first failure ends the script.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${ORBIT_PROFILE_OUT:-$R/profiles}
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
W=$(mktemp -d)
NAMES="2x2x2_7_Winograd 4x4x4_49_156 3x4x7_63_rational"
ACTIONS="triangular pluq householder"
N=1000000
RATES="$OUT/orbit_action_rates.txt"
kernel_ms() { python3 -c "import re, sys; print(re.search(r'restarts on GPU in [0-9.e+-]+ s \(kernel ([0-9.e+-]+) ms\)', open(sys.argv[1]).read()).group(1))" "$1"; }

# 1. candidates/s on the GPU and on the host, and the two outputs compared
: > "$RATES"
for act in $ACTIONS; do
    for nm in $NAMES; do
        for g in 1 0; do
            mkdir -p "$W/$act/$g"
            for x in L R P; do cp "$R/tests/golden/data/${nm}_$x.sms" "$W/$act/$g/"; done
        done
        t0=$(date +%s.%N)
        timeout -k 10 120 "$R/bin/orbiter" --gpu 1 --action $act --seed 0 -O $N "$W/$act/1/${nm}_L.sms" "$W/$act/1/${nm}_R.sms" "$W/$act/1/${nm}_P.sms" > "$W/$act/1/$nm.out" 2> "$W/$act/1/$nm.err"
        t1=$(date +%s.%N)
        OMP_NUM_THREADS=16 timeout -k 10 300 "$R/bin/orbiter" --gpu 0 --action $act --seed 0 -O $N "$W/$act/0/${nm}_L.sms" "$W/$act/0/${nm}_R.sms" "$W/$act/0/${nm}_P.sms" > "$W/$act/0/$nm.out" 2> "$W/$act/0/$nm.err"
        t2=$(date +%s.%N)
        same=identical
        cmp -s "$W/$act/1/$nm.out" "$W/$act/0/$nm.out" || same=DIFFERENT
        for x in L R P; do
            a="$W/$act/1/${nm}_$x.nnz.sms"; b="$W/$act/0/${nm}_$x.nnz.sms"
            if [ -e "$a" ] || [ -e "$b" ]; then cmp -s "$a" "$b" || same=DIFFERENT; fi
        done
        python3 -c "import sys; nm, act, n, ms, t0, t1, t2, same, win = sys.argv[1:10]; n = int(n); ms = float(ms); h = float(t2) - float(t1); print('%-18s %-11s gpu1 kernel %8.3f ms %.4g candidates/s (tool wall %.3f s); host16 %.3f s %.4g candidates/s; %s; outputs %s' % (nm, act, ms, n / (ms / 1e3), float(t1) - float(t0), h, n / h, win, same))" \
            "$nm" $act $N "$(kernel_ms "$W/$act/1/$nm.err")" "$t0" "$t1" "$t2" $same "$(head -1 "$W/$act/1/$nm.out")" >> "$RATES"
        [ $same = identical ]
    done
done

# 2. the default action against the parent commit's build: alternate, three runs each
if [ -n "$ORBIT_PARENT" ]; then
    nm=4x4x4_49_156
    for i in 1 2 3; do
        for who in parent this; do
            root=$R; [ $who = parent ] && root=$ORBIT_PARENT
            PLO_HIP_LIB="$root/plinopt_amd/libplinopt_hip.so" timeout -k 10 120 "$root/bin/orbiter" --gpu 1 --seed 0 -O $N "$W/triangular/1/${nm}_L.sms" "$W/triangular/1/${nm}_R.sms" "$W/triangular/1/${nm}_P.sms" > "$W/$who.out" 2> "$W/$who.err"
            echo "$nm triangular $who run $i: kernel $(kernel_ms "$W/$who.err") ms; $(head -1 "$W/$who.out")" >> "$RATES"
        done
    done
fi

# 3. kernel trace and statistics of one search per action
: > "$OUT/orbit_action_kernel_stats.csv"
nm=4x4x4_49_156
for act in $ACTIONS; do
    T=$(mktemp -d)
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o orbit -- "$R/bin/orbiter" --gpu 1 --action $act --seed 0 -O $N "$W/$act/1/${nm}_L.sms" "$W/$act/1/${nm}_R.sms" "$W/$act/1/${nm}_P.sms" > /dev/null 2> "$W/rocprof_$act.err"
    S=$(find "$T" -name '*kernel_stats.csv' | head -1)
    { echo "# $nm, --action $act, $N candidates"; cat "$S"; } >> "$OUT/orbit_action_kernel_stats.csv"
    rm -rf "$T"
done
rm -rf "$W"
cat "$RATES"
