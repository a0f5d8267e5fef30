#!/bin/bash
# Measurements of the orbiter kernel (plo_orbit.hip) on one MI355X, written to profiles/orbit_* (or $ORBIT_PROFILE_OUT):
#   orbit_kernel_stats.csv   rocprofv3 --kernel-trace --stats of one search per input over Q (runs of their own)
#   orbit_rates.txt          kernel time and candidates/s of bin/orbiter --gpu 1, and wall-clock candidates/s of the host
#                            loop (--gpu 0, 16 OpenMP threads), on 2x2x2_7_Winograd, 4x4x4_49_156 and 3x4x7_63_rational
# Usage: tests/profile_orbit.sh   (needs bin/orbiter and plinopt_amd/libplinopt_hip.so built).  The searches run on copies of
# the inputs.  Every GPU step has its own time limit; the first failure ends the script.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${ORBIT_PROFILE_OUT:-$R/profiles}
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
W=$(mktemp -d)
NAMES="2x2x2_7_Winograd 4x4x4_49_156 3x4x7_63_rational"
for nm in $NAMES; do for x in L R P; do cp "$R/tests/golden/data/${nm}_$x.sms" "$W/"; done; done
GPU_N=1000000
HOST_N=20000

# 1. kernel trace and statistics of a fixed search (10^6 seeds from seed 0) per input
: > "$OUT/orbit_kernel_stats.csv"
for nm in $NAMES; do
    T=$(mktemp -d)
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o orbit -- "$R/bin/orbiter" --gpu 1 --seed 0 -O $GPU_N "$W/${nm}_L.sms" "$W/${nm}_R.sms" "$W/${nm}_P.sms" > /dev/null 2> "$OUT/orbit_rocprof_$nm.err"
    S=$(find "$T" -name '*kernel_stats.csv' | head -1)
    { echo "# $nm, $GPU_N candidates"; cat "$S"; } >> "$OUT/orbit_kernel_stats.csv"
    rm -rf "$T"
done

# 2. candidates/s: kernel time of the tool's report on the GPU, wall clock of the host loop
: > "$OUT/orbit_rates.txt"
for nm in $NAMES; do
    f="$W/${nm}_L.sms $W/${nm}_R.sms $W/${nm}_P.sms"
    timeout -k 10 300 "$R/bin/orbiter" --gpu 1 --seed 0 -O $GPU_N $f > /dev/null 2> "$W/gpu.err"
    python3 -c "import re, sys; t = open(sys.argv[3]).read(); m = re.search(r'restarts on GPU in ([0-9.e+-]+) s \(kernel ([0-9.e+-]+) ms\)', t); n = int(sys.argv[2]); print('%s gpu1 %d candidates: kernel %.3f ms, %.4g candidates/s of kernel time; tool wall %.3f s' % (sys.argv[1], n, float(m.group(2)), n / (float(m.group(2)) / 1e3), float(m.group(1))))" "$nm" $GPU_N "$W/gpu.err" >> "$OUT/orbit_rates.txt"
    t0=$(date +%s.%N)
    OMP_NUM_THREADS=16 timeout -k 10 300 "$R/bin/orbiter" --gpu 0 --seed 0 -O $HOST_N $f > /dev/null 2> "$W/host.err"
    t1=$(date +%s.%N)
    python3 -c "import sys; n, a, b = int(sys.argv[2]), float(sys.argv[3]), float(sys.argv[4]); print('%s host16 %d candidates in %.3f s: %.4g candidates/s' % (sys.argv[1], n, b - a, n / (b - a)))" "$nm" $HOST_N "$t0" "$t1" >> "$OUT/orbit_rates.txt"
done
rm -rf "$W"
cat "$OUT/orbit_rates.txt"
