"""Not a test: the candidates of `bin/pruner -q p -O N P.slp` through the per-window route of the C API -- one
plo_cse_search per window for -D, one plo_cse_chain_create + plo_cse_chain_search per window for -G -- and, for comparison
in the same process, through one plo_cse_batch_search per method.  Prints one JSON line per route: kernel milliseconds,
wall seconds, candidates/s and the share of the wall time spent outside the kernels (plan building, uploads, launches).

    python tests/pruner_baseline.py [-q 131071] [-O 1000] tests/golden/data/4x4x4_48_rational_P.slp
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
from plo_testlib import FieldP, OracleMatrix              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-q", type=int, default=131071)
    ap.add_argument("-O", type=int, default=1000)
    ap.add_argument("-v", action="store_true")
    ap.add_argument("slp")
    a = ap.parse_args()
    from plinopt_amd import capi, cse_batch_search
    L = capi.lib()
    capi.check(L.plo_init(0))
    t0 = time.time()
    wins = pl.windows(open(a.slp).read(), singles=a.v)
    mats, lus = [], []
    for w in wins:
        m, n = len(w["outs"]), len(w["ins"])
        O = OracleMatrix(*(pl.csr_of(pl.window_matrix(w, FieldP(a.q)), m, n) + (a.q,)))
        U, Lw, _ = O.lu_factors()
        mats.append((O.m, O.n, O.rowptr, O.col, O.val))
        lus.append(((U.m, U.n, U.rowptr, U.col, U.val), (Lw.m, Lw.n, Lw.rowptr, Lw.col, Lw.val)))
    print("# %d windows prepared in %.1f s (Python)" % (len(wins), time.time() - t0), file=sys.stderr)
    N = a.O

    def line(route, method, wall, kms, cand, results):
        print(json.dumps({"route": route, "method": method, "windows": len(wins), "restarts": N, "candidates": cand, "kernel_ms": round(kms, 3), "wall_s": round(wall, 4),
                          "candidates_per_s": round(cand / wall), "host_share": round(1 - kms / 1000 / wall, 4), "checksum": sum(r[0] + r[1] for r in results)}), flush=True)

    # ---- one call per window
    csrs = [capi.make_csr(*m) for m in mats]
    b, st = capi.Best(), capi.Stats()
    t0, kms, cand, res = time.time(), 0.0, 0, []
    for w, (c, _keep) in enumerate(csrs):
        capi.check(L.plo_cse_search(ctypes.byref(c), a.q, w * N, N, 0, ctypes.byref(b), ctypes.byref(st)))
        kms += st.kernel_ms; cand += st.candidates; res.append((b.adds, b.muls, b.seed))
    line("plo_cse_search per window", "D", time.time() - t0, kms, cand, res)
    per_d = res
    pairs = [(capi.make_csr(*u), capi.make_csr(*l)) for u, l in lus]
    t0, kms, cand, res = time.time(), 0.0, 0, []
    for w, ((cu, _k1), (cl, _k2)) in enumerate(pairs):
        h = ctypes.c_void_p()
        capi.check(L.plo_cse_chain_create(ctypes.byref(cu), ctypes.byref(cl), a.q, ctypes.byref(h)))
        capi.check(L.plo_cse_chain_search(h, w * N, N, 0, ctypes.byref(b), ctypes.byref(st)))
        L.plo_cse_chain_destroy(h)
        kms += st.kernel_ms; cand += st.candidates; res.append((b.adds, b.muls, b.seed))
    line("plo_cse_chain_create + search per window", "G", time.time() - t0, kms, cand, res)
    per_g = res
    # ---- one call per method
    t0 = time.time()
    bests, status, s = cse_batch_search(mats, None, a.q, 0, N)
    line("plo_cse_batch_search", "D", time.time() - t0, s["kernel_ms"], s["candidates"], bests)
    assert not any(status) and bests == per_d, "the two routes disagree (-D)"
    t0 = time.time()
    bests, status, s = cse_batch_search([u for u, _ in lus], [l for _, l in lus], a.q, 0, N)
    line("plo_cse_batch_search", "G", time.time() - t0, s["kernel_ms"], s["candidates"], bests)
    assert not any(status) and bests == per_g, "the two routes disagree (-G)"


if __name__ == "__main__":
    main()
