#!/bin/bash
# Rates of the growth-factor kernel (plo_orbit_growth.hip) on one MI355X, written to profiles/orbit_growth_rates.txt (or
# $ORBIT_PROFILE_OUT): per input (2x2x2_7_Winograd, 4x4x4_49_156, 3x4x7_63_rational), 10^6 candidates from seed 0:
#   bin/orbiter -g --gpu 1   kernel time (the tool's HIP events) and candidates/s of kernel time
#   bin/orbiter -g --gpu 0   the same candidates in the tool's host loop, 16 OpenMP threads, wall clock of the search
#   bin/orbiter    --gpu 1   the density kernel on the same candidates, for comparison
# The winner lines of the two -g runs must be identical: the script fails otherwise.
# Usage: tests/profile_orbit_growth.sh   (needs bin/orbiter and plinopt_amd/libplinopt_hip.so built).  The searches run on copies
# of the inputs.  Every step has its own time limit; the first failure ends the script.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${ORBIT_PROFILE_OUT:-$R/profiles}
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
W=$(mktemp -d)
NAMES="2x2x2_7_Winograd 4x4x4_49_156 3x4x7_63_rational"
for nm in $NAMES; do for x in L R P; do cp "$R/tests/golden/data/${nm}_$x.sms" "$W/"; done; done
N=1000000
RATE='import re, sys
nm, what, n, t = sys.argv[1], sys.argv[2], int(sys.argv[3]), open(sys.argv[4]).read()
m = re.search(r"restarts on GPU in ([0-9.e+-]+) s \(kernel ([0-9.e+-]+) ms\)", t)
if m:
    print("%s %s %d candidates: kernel %.3f ms, %.4g candidates/s of kernel time; tool wall %.3f s" % (nm, what, n, float(m.group(2)), n / (float(m.group(2)) / 1e3), float(m.group(1))))
else:
    s = float(re.search(r"# Search\(\d+\): ([0-9.e+-]+)s", t).group(1))
    assert "restarts on host" in t
    print("%s %s %d candidates: search %.3f s, %.4g candidates/s" % (nm, what, n, s, n / s))'

: > "$OUT/orbit_growth_rates.txt"
for nm in $NAMES; do
    f="$W/${nm}_L.sms $W/${nm}_R.sms $W/${nm}_P.sms"
    timeout -k 10 300 "$R/bin/orbiter" -g --gpu 1 --seed 0 -O $N $f > "$W/gpu.out" 2> "$W/gpu.err"
    python3 -c "$RATE" "$nm" "growth gpu1" $N "$W/gpu.err" >> "$OUT/orbit_growth_rates.txt"
    rm -f "$W"/*.nnz.sms
    OMP_NUM_THREADS=16 timeout -k 10 600 "$R/bin/orbiter" -g --gpu 0 --seed 0 -O $N $f > "$W/host.out" 2> "$W/host.err"
    python3 -c "$RATE" "$nm" "growth host16" $N "$W/host.err" >> "$OUT/orbit_growth_rates.txt"
    rm -f "$W"/*.nnz.sms
    cmp "$W/gpu.out" "$W/host.out"
    echo "$nm winner (both): $(cat "$W/gpu.out")" >> "$OUT/orbit_growth_rates.txt"
    timeout -k 10 300 "$R/bin/orbiter" --gpu 1 --seed 0 -O $N $f > /dev/null 2> "$W/dens.err"
    python3 -c "$RATE" "$nm" "density gpu1" $N "$W/dens.err" >> "$OUT/orbit_growth_rates.txt"
    rm -f "$W"/*.nnz.sms
done
rm -rf "$W"
cat "$OUT/orbit_growth_rates.txt"
