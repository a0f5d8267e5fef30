#!/bin/bash
# Measurements of the dependency kernel (plo_dep.hip) on one MI355X, written to profiles/dependency_* (or $DEP_PROFILE_OUT):
#   dependency_kernel_stats.csv   rocprofv3 --kernel-trace --stats of one enumeration (4x4x4_49_156_L, -l 4 -c 11, over Q; a run of its own)
#   dependency_rates.txt          kernel time (the tool's HIP events) and combinations/s of bin/dependency --gpu 1, and the wall clock of
#                                 the tool's own host loop (--gpu 0, 16 OpenMP threads) on the same input, for 4x4x4_49_156_L at -l 4 -c 11
#                                 over Q and modulo 131071, and for the matrix bin/SLPchecker rebuilds from the stored program
#                                 4x4x4_49_156_L.slp at -l 3
# Usage: tests/profile_dependency.sh   (needs bin/dependency, bin/SLPchecker and plinopt_amd/libplinopt_hip.so built).
# Every GPU step has its own time limit; the first failure ends the script.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${DEP_PROFILE_OUT:-$R/profiles}
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
W=$(mktemp -d)
L=$R/tests/golden/data/4x4x4_49_156_L.sms
"$R/bin/SLPchecker" "$R/tests/golden/data/4x4x4_49_156_L.slp" > "$W/program.sms" 2> /dev/null

# 1. kernel trace and statistics of one enumeration
T=$(mktemp -d)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$T" -o dep -- "$R/bin/dependency" --gpu 1 -l 4 -c 11 "$L" > /dev/null 2> "$W/rocprof.err"
S=$(find "$T" -name '*kernel_stats.csv' | head -1)
{ echo "# 4x4x4_49_156_L -l 4 -c 11 over Q"; cat "$S"; } > "$OUT/dependency_kernel_stats.csv"
rm -rf "$T"

# 2. combinations/s: kernel time of the tool's report on the GPU, the tool's own time on the host
: > "$OUT/dependency_rates.txt"
rate() {   # label, file, arguments
    local label=$1 f=$2; shift 2
    timeout -k 10 300 "$R/bin/dependency" --gpu 1 "$@" "$f" > "$W/gpu.out" 2> "$W/gpu.err"
    OMP_NUM_THREADS=16 timeout -k 10 900 "$R/bin/dependency" --gpu 0 "$@" "$f" > "$W/host.out" 2> "$W/host.err"
    cmp "$W/gpu.out" "$W/host.out"
    python3 -c "
import re, sys
g, h = open(sys.argv[2]).read(), open(sys.argv[3]).read()
m = re.search(r'# (\d+) combinations on GPU in ([0-9.e+-]+) s \(kernel ([0-9.e+-]+) ms\)', g)
k = re.search(r'# (\d+) combinations on host in ([0-9.e+-]+) s', h)
n, wall, ms, host = int(m.group(1)), float(m.group(2)), float(m.group(3)), float(k.group(2))
print('%s: %d combinations, %d hit lines; gpu1 kernel %.3f ms, %.4g combinations/s of kernel time, tool %.3f s; host16 %.3f s, %.4g combinations/s' % (sys.argv[1], n, int(sys.argv[4]), ms, n / (ms / 1e3), wall, host, n / host))
" "$label" "$W/gpu.err" "$W/host.err" "$(wc -l < "$W/gpu.out")" >> "$OUT/dependency_rates.txt"
}
rate "4x4x4_49_156_L -l 4 -c 11 over Q" "$L" -l 4 -c 11
rate "4x4x4_49_156_L -l 4 -c 11 modulo 131071" "$L" -l 4 -c 11 -q 131071
rate "SLPchecker matrix of 4x4x4_49_156_L.slp ($(head -1 "$W/program.sms" | cut -d' ' -f1,2 | tr ' ' x)) -l 3 -c 11 over Q" "$W/program.sms" -l 3 -c 11
rm -rf "$W"
cat "$OUT/dependency_rates.txt"
