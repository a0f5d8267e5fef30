"""Not a test: the candidates of `bin/pruner -q p -K -O N P.slp` for the windows that have a kernel, through (a) one
plo_kernel_batch_search and (b) one plo_kernel_search(per_block = 1) per window -- the only device route before the batch
entry existed -- in one process.  Prints one JSON line per route: kernel milliseconds, wall seconds, candidates/s and the
share of the wall time spent outside the kernels; asserts that both routes return the same minima.

    python tests/pruner_k_baseline.py [-q 131071] [-O 1000] tests/golden/data/4x4x4_48_rational_R.slp
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pruner_lib as pl                                   # noqa: E402
import synth                                              # noqa: E402
from plo_testlib import FieldP                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-q", type=int, default=131071)
    ap.add_argument("-O", type=int, default=1000)
    ap.add_argument("-v", action="store_true")
    ap.add_argument("slp")
    a = ap.parse_args()
    from plinopt_amd import capi, kernel_batch_search
    L = capi.lib()
    capi.check(L.plo_init(0))
    t0 = time.time()
    wins = pl.windows(open(a.slp).read(), singles=a.v)
    mats = []
    for w in wins:
        m, n = len(w["outs"]), len(w["ins"])
        csr = pl.csr_of(pl.window_matrix(w, FieldP(a.q)), m, n)
        rows = [{csr[3][k]: csr[4][k] for k in range(csr[2][i], csr[2][i + 1])} for i in range(m)]
        if synth.km_refusal(m, n, rows, a.q) is None:     # a kernel of positive dimension, inside the limits the host can check
            mats.append(csr)
    print("# %d windows, %d with a kernel, prepared in %.1f s (Python)" % (len(wins), len(mats), time.time() - t0), file=sys.stderr)
    N = a.O

    def line(route, wall, kms, launches, cand, results):
        print(json.dumps({"route": route, "method": "K", "windows": len(mats), "restarts": N, "candidates": cand, "launches": launches, "kernel_ms": round(kms, 3),
                          "wall_s": round(wall, 4), "candidates_per_s": round(cand / wall), "host_share": round(1 - kms / 1000 / wall, 4),
                          "checksum": sum(r[0] + r[1] for r in results)}), flush=True)

    # ---- both routes once on two windows first: the first launch of a kernel loads its code object
    kernel_batch_search(mats[:2], a.q, 0, 2)
    wc, _wkeep = capi.make_csr(*mats[0])
    capi.check(L.plo_kernel_search(ctypes.byref(wc), a.q, 0, 2, 1, 0, None, None, None, ctypes.byref(capi.Best()), ctypes.byref(capi.Stats())))
    # ---- (a) one call
    t0 = time.time()
    bests, status, s = kernel_batch_search(mats, a.q, 0, N)
    line("plo_kernel_batch_search", time.time() - t0, s["kernel_ms"], s["launches"], s["candidates"], bests)
    assert not any(status), "refused: %s" % [q for q, c in enumerate(status) if c]
    # ---- (b) one call per window
    csrs = [capi.make_csr(*m) for m in mats]
    b, st = capi.Best(), capi.Stats()
    t0, kms, cand, launches, res = time.time(), 0.0, 0, 0, []
    for q, (c, _keep) in enumerate(csrs):
        capi.check(L.plo_kernel_search(ctypes.byref(c), a.q, q * N, N, 1, 0, None, None, None, ctypes.byref(b), ctypes.byref(st)))
        kms += st.kernel_ms; cand += st.candidates; launches += st.launches; res.append((b.adds, b.muls, b.seed))
    line("plo_kernel_search per window", time.time() - t0, kms, launches, cand, res)
    assert bests == res, "the two routes disagree"


if __name__ == "__main__":
    main()
