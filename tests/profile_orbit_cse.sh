#!/bin/bash
# Measurements of the orbiter's CSE measure (bin/orbiter -z, plo::orbit_cse_kernel, plo_orbit_cse.hip) on one MI355X, printed to
# stdout (profiles/orbit_cse_rates.txt is a digest of it): per input, `-q 131071 -z -O 1000` (sub 62) on the device (--gpu 1: the
# tool's last '#' lines hold the kernel time of its HIP events and its search time) and in the tool's host loop (--gpu 0, 16
# OpenMP threads) on the same candidates, and whether the two runs agree byte for byte (winner line and written files).
# With $ORBIT_CSE_PROFILE_LIB set to a build of the library with -DPLO_ORBIT_CSE_PROFILE: the profile points of one more device run.
# Usage: tests/profile_orbit_cse.sh [input ...]   (needs bin/orbiter and plinopt_amd/libplinopt_hip.so built).  The searches run on
# copies of the inputs.  Every GPU step has its own time limit; the first failure ends the script.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
export TMPDIR=${TMPDIR:-/tmp}
W=$(mktemp -d)
NAMES=${*:-2x2x2_7_Winograd 3x3x3_23_58 4x4x4_49_156 3x6x3_40}
for nm in $NAMES; do
    for g in 1 0; do
        mkdir -p "$W/$g"
        for x in L R P; do cp "$R/tests/golden/data/${nm}_$x.sms" "$W/$g/"; done
    done
    timeout -k 10 240 "$R/bin/orbiter" --gpu 1 -q 131071 -z -O 1000 "$W/1/${nm}_L.sms" "$W/1/${nm}_R.sms" "$W/1/${nm}_P.sms" > "$W/1/$nm.out" 2> "$W/1/$nm.err"
    OMP_NUM_THREADS=16 timeout -k 10 600 "$R/bin/orbiter" --gpu 0 -q 131071 -z -O 1000 "$W/0/${nm}_L.sms" "$W/0/${nm}_R.sms" "$W/0/${nm}_P.sms" > "$W/0/$nm.out" 2> "$W/0/$nm.err"
    same=identical
    cmp -s "$W/1/$nm.out" "$W/0/$nm.out" || same=DIFFERENT
    for x in L R P; do
        if [ -e "$W/0/${nm}_$x.nnz.sms" ] || [ -e "$W/1/${nm}_$x.nnz.sms" ]; then cmp -s "$W/1/${nm}_$x.nnz.sms" "$W/0/${nm}_$x.nnz.sms" || same=DIFFERENT; fi
    done
    echo "== $nm: outputs $same; $(cat "$W/1/$nm.out")"
    grep -E "refuses|Search\(|restarts on" "$W/1/$nm.err" | sed 's/^/   device: /'
    grep -E "Search\(|restarts on" "$W/0/$nm.err" | sed 's/^/   host:   /'
    if [ -n "$ORBIT_CSE_PROFILE_LIB" ]; then
        PLO_HIP_LIB=$ORBIT_CSE_PROFILE_LIB PLO_ORBIT_CSE_STATS=1 timeout -k 10 240 "$R/bin/orbiter" --gpu 1 -q 131071 -z -O 1000 "$W/1/${nm}_L.sms" "$W/1/${nm}_R.sms" "$W/1/${nm}_P.sms" 2>&1 > /dev/null | grep "orbit CSE measure" | sed 's/^/   /'
    fi
done
rm -rf "$W"
