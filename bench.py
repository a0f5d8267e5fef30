#!/usr/bin/env python3
"""bench.py -- candidate SLPs/sec of the randomized multi-start CSE search
(BASELINE.json metric) on N MI355X GPUs of one node.

A "step" is one pass of the hot path over one batch of seeds: every rank
evaluates `--batch` candidates of its own shard of the seed space on its GPU
(libplinopt_hip.so, plo_cse_search_plan) and the ranks then reduce the packed
(cost, seed) word with ONE 8-byte MIN all-reduce (RCCL).  Weak scaling: the
per-GPU batch is fixed, the global batch grows with N.

Prints one JSON line on rank 0.  The matrix is resident in HBM before the timed
region; nothing under /root/reference is read.

A plain run sets up, warms up, times `--steps` steps and prints the line; the CPU
baselines (seconds to minutes of host work) run only with `--full`.  `--dump-outputs DIR`
writes the result of the last timed step as DIR/<name>.npy (float64), for
comparing two builds output for output: the seeds of every step are fixed by the
arguments.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = {
    # name: (fixture file, modulus, default per-GPU batch, description)
    "32x32x32": ("32x32x32_15096_L.slp", 131071, 1024,
                 "bin/optimizer -q 131071 -D data/32x32x32_15096_L.sms (BASELINE configs[4], the metric's config): "
                 "matrix regenerated from the stored SLP (reference Makefile:79-80), 1024 random restarts per GPU per step (one workgroup per restart, 2 resident per CU)"),
    "winograd": ("2x2x2_7_Winograd_L.sms", 131071, 1000000,
                 "bin/optimizer -q 131071 -D data/2x2x2_7_Winograd_L.sms, 10^6 random restarts per step (BASELINE configs[1])"),
    "4x4x4_L": ("4x4x4_49_156_L.sms", 131071, 200000,
                "bin/optimizer -q 131071 -D data/4x4x4_49_156_L.sms, 2*10^5 random restarts per step"),
    "tril": ("4x4x4_49_156", 0, 200000,
             "bin/trilplacer data/4x4x4_49_156_{L,R,P}.sms -O N (BASELINE configs[3]): 2*10^5 restarts per step, each = one row permutation "
             "+ coherent negations, oriented and unoriented in-place program"),
    "4x4x4_P": ("4x4x4_49_156_P.sms", 131071, 100000,
                "bin/optimizer -q 131071 -D data/4x4x4_49_156_P.sms, 10^5 random restarts per step"),
    "cyclic": ("cyclic.sms", 131071, 500000, "bin/optimizer -q 131071 -D data/cyclic.sms"),
    "kmethod": ("4x4x4_49_156_L.sms", 131071, 1000000,
                "bin/optimizer -q 131071 -K -O N data/4x4x4_49_156_L.sms: 10^6 restarts of KernelOptimiser per step, each = one nullspace "
                "decomposition + Optimizer on Free + Optimizer on Dep, all in one wavefront (plo_kernel_search)"),
    "cob": ("4x4x4_49_156_L.sms", 131071, 56 ** 4,
            "bin/sparsifier -q 131071 -c 56 data/4x4x4_49_156_L.sms (BASELINE configs[2] with `-q 131071` ADDED: as written the config "
            "runs over Q, which bin/sparsifier now also enumerates on the GPU -- modulo two 31-bit primes, winners checked over Q --; this line times the "
            "enumeration modulo 131071, which visits the same candidates on this +-1 matrix) "
            "and -c 56 instead of -c 4 to reach the 10^7 candidates the config asks for: one (block,row) enumeration of "
            "localSparsifier = 56^4 = 9.8e6 change-of-basis candidate rows per step and GPU"),
}
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def dump_outputs(path, **arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float64 (every field here is an integer below 2^53, so exact)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(a, dtype=np.float64))


def load_matrix(name):
    from plo_testlib import DATA, read_sms, to_csr_mod
    fname, p, batch, desc = WORKLOADS[name]
    if fname.endswith(".slp"):
        # data/32x32x32_15096_L.sms is absent upstream; rebuild it from the stored SLP with bin/SLPchecker.
        # The tool comes from __graft_entry__.build(): the benchmark builds nothing and writes nothing into the tree,
        # which may be read-only to the user who runs it.
        import subprocess
        slpchecker = os.path.join(ROOT, "bin", "SLPchecker")
        if not os.path.exists(slpchecker):
            raise FileNotFoundError("%s not built: run __graft_entry__.build() first" % slpchecker)
        out = subprocess.run([slpchecker, "-q", str(p), os.path.join(DATA, fname)],
                             capture_output=True, text=True, check=True).stdout.splitlines()
        m, n = int(out[0].split()[0]), int(out[0].split()[1])
        rows = [[] for _ in range(m)]
        for ln in out[1:-1]:
            i, j, v = ln.split()
            rows[int(i) - 1].append((int(j) - 1, int(v)))
        rp, c, v = [0], [], []
        for r in rows:
            r.sort()
            for j, x in r:
                c.append(j)
                v.append(x)
            rp.append(len(c))
        return m, n, rp, c, v, p, batch, desc, fname
    m, n, ent = read_sms(os.path.join(DATA, fname))
    rp, c, v = to_csr_mod(m, n, ent, p)
    return m, n, rp, c, v, p, batch, desc, fname


def cpu_baseline_host_engine(m, n, rp, c, v, p, tmpdir="/tmp"):
    """Config 5 on the host cores.  The literal oracle (oracle/plo_oracle.c) rescans its pair map at every
    step (~1e11 node visits per candidate here) and cannot finish; the bounded CPU sample therefore runs the
    build's scalable exact host engine (plinopt_amd/csrc/host/plo_fast.hpp, text-identical to the oracle on every
    input the oracle can walk) through `bin/optimizer --gpu 0`, OpenMP over seeds."""
    import subprocess
    cores = min(os.cpu_count() or 1, 64)
    path = os.path.join(tmpdir, "plo_bench_l32_%d.sms" % os.getpid())
    with open(path, "w") as f:
        f.write("%d %d M\n" % (m, n))
        for i in range(m):
            for k in range(rp[i], rp[i + 1]):
                f.write("%d %d %d\n" % (i + 1, c[k] + 1, v[k]))
        f.write("0 0 0\n")
    env = dict(os.environ, OMP_NUM_THREADS=str(cores))
    t0 = time.perf_counter()
    r = subprocess.run([os.path.join(ROOT, "bin", "optimizer"), "-q", str(p), "-D", "-O", str(cores), "--gpu", "0", "--seed", "1", path],
                       env=env, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    err = r.stderr
    os.unlink(path)
    import re
    mm = re.search(r"# host search: (\d+) candidates in ([0-9.eE+-]+) s on (\d+) threads", err)
    secs = float(mm.group(2)) if mm else wall
    rate = cores / max(secs, 1e-3)
    found = [ln for ln in err.splitlines() if "Found D" in ln]
    return {"value": rate, "unit": "candidates/s", "cores": cores, "kind": "port",
            "sample": "%d seeds (1..%d) of the same matrix through bin/optimizer --gpu 0 (host engine plo_fast.hpp, OpenMP, one candidate per "
                      "thread), search %.1f s (shared index build included), wall %.1f s; %s"
                      % (cores, cores, secs, wall, found[0].strip() if found else "")}


def cpu_baseline(m, n, rp, c, v, p, target_s=12.0):
    """Times the CPU oracle (oracle/libplo_oracle.so, OpenMP over seeds) on this host's
    cores for a bounded sample of the same workload.  Reported baseline, not the product."""
    from plo_testlib import OracleMatrix, oracle
    M = OracleMatrix(m, n, rp, c, v, p)
    cores = oracle().plo_oracle_max_threads()
    M.search(0, 2000, 0, nthreads=cores)            # spin the thread pool up
    sample = 20000
    while True:                                      # grow the sample until it is ~target_s of CPU work
        t0 = time.perf_counter()
        best = M.search(0, sample, 0, nthreads=cores)
        dt = time.perf_counter() - t0
        if dt >= 0.6 * target_s or sample >= 2_000_000_000:
            break
        sample = int(sample * min(max(1.2 * target_s / max(dt, 1e-3), 2.0), 50.0))
    return {"value": sample / dt, "unit": "candidates/s", "cores": cores, "kind": "port",
            "sample": "%d seeds (0..%d) of the same matrix through oracle/plo_oracle.c, OpenMP, %.1f s; best (adds,muls,seed)=%s"
                      % (sample, sample - 1, dt, list(best))}


def dist_setup(args):
    """One process per GPU (torch.distributed.run sets RANK/LOCAL_RANK/WORLD_SIZE); backend "nccl" = RCCL over xGMI."""
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but WORLD_SIZE=%d; launch with torch.distributed.run" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the product path has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    return rank, local_rank, world, dev, barrier, max_over_ranks


PER_RANK_COLUMNS = ["kernel (HIP events)", "search wall (library call)", "all-reduce wall (includes waiting for the slowest rank)"]


def gather_per_rank(dev, world, kernel_ms, search_s, reduce_s):
    """every rank's kernel time, wall time of its searches and wall time inside the all-reduces over the timed steps, in ms (one row per
    rank): where a loss of scaling would come from -- a slow rank, launch overhead, or the reduction"""
    import torch
    import torch.distributed as dist
    mine = torch.tensor([kernel_ms, search_s * 1e3, reduce_s * 1e3], dtype=torch.float64, device=dev)
    if world > 1:
        rows = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(rows, mine)
    else:
        rows = [mine]
    return [[round(float(x), 3) for x in g.tolist()] for g in rows]


def issue_roofline(name, kernel, per_launch_ms):
    """For the kernels whose state lives in LDS the HBM roofline says nothing: report instruction issue instead, from the
    committed rocprofv3 counters of the same workload (profiles/r04_issue.json, else r03 / r02: SQ_INSTS_* / SQ_BUSY_CYCLES).
    The counters belong to one version of the kernel: `stale` says whether the source has changed since; `achieved` is scaled by
    profiled kernel time / this run's kernel time (the instruction count of a launch does not change with the clock)."""
    d = None
    for fn in ("r04_issue.json", "r03_issue.json", "r02_issue.json"):
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", fn))).get(name)
        except Exception:
            d = None
        if d:
            break
    if not d:
        return None
    unit = d["bound_unit"]
    ach = d["salu_per_clk_cu"] if unit == "scalar" else d["valu_per_clk_cu"]
    peak = 1.0 if unit == "scalar" else 2.0
    out = {"bound": "issue", "achieved": ach, "peak": peak, "unit": "%s wave-instructions/clk/CU" % unit, "frac": ach / peak, "traffic": None,
           "kernel": kernel, "kernel_ms_per_launch": per_launch_ms, "source": d["source"],
           "all_units_per_clk_cu": {k: d[k] for k in ("valu_per_clk_cu", "salu_per_clk_cu", "lds_per_clk_cu", "vmem_per_clk_cu")},
           "note": "achieved/peak from the profile of this workload, not from this run; the run's own kernel time is kernel_ms_per_launch"}
    if "kernel_source_sha16" in d:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        try:
            from make_issue_json import sources_sha16
            out["stale"] = sources_sha16(name) != d["kernel_source_sha16"]
        except Exception:
            out["stale"] = None
    else:
        out["stale"] = None                          # a round-2 entry: no hash was recorded
    return out


def bench_cob(args):
    """configs[2]: the exhaustive |Coeffs|^4 enumeration of localSparsifier (plinopt_sparsify.inl:299-314) on the GPU."""
    import torch
    from plinopt_amd import capi, cob_search
    from plo_testlib import DATA, read_sms, to_csr_mod, oracle_cob_search
    from plinopt_amd.dist import allreduce_cob_best, shard_range
    fname, p, total, desc = WORKLOADS["cob"]
    rank, local_rank, world, dev, barrier, max_over_ranks = dist_setup(args)
    capi.check(capi.lib().plo_init(local_rank))
    mm, nn, ent = read_sms(os.path.join(DATA, fname))
    rp, c, v = to_csr_mod(mm, nn, ent, p)
    n, m = nn, mm                                   # TM = M^T is n x m
    TM = [0] * (n * m)
    for i in range(mm):
        for k in range(rp[i], rp[i + 1]):
            TM[c[k] * m + i] = v[k]
    C = 56
    coeffs = [0, 1, p - 1]
    i = 2
    while len(coeffs) < C:                          # the coefficient set of localSparsifier :256-268 for a +-1 matrix
        for x in (i % p, (-i) % p, pow(i, -1, p), (-pow(i, -1, p)) % p):
            coeffs.append(x)
        i += 1
    coeffs = coeffs[:C]
    Cand = [0] * (n * n)
    steps = args.steps if args.steps is not None else 10
    warm = args.warmup if args.warmup is not None else 2
    kms = 0.0
    # N > 1: every rank enumerates the whole coefficient set of ITS OWN (block,row) call in the real tool; here the
    # benchmark keeps the per-GPU work fixed (weak scaling): rank r takes the prefixes (i,j,k) of shard r of a C^3 * world
    # space folded back onto C^3, i.e. all ranks run a full enumeration and the MAX all-reduce picks the common winner.
    # The strong-scaling split of ONE enumeration is `groups=shard_range(0, C^3, rank, world)` (tests/test_gpu_cob.py).
    groups = (0, C ** 3)

    def one():
        res, st = cob_search(n, m, TM, Cand, 0, 0, coeffs, p, groups=groups)
        return allreduce_cob_best(res, n, device=dev) or res, st

    for k in range(warm):
        res, st = one()
    barrier()
    t0 = time.perf_counter()
    for k in range(steps):
        res, st = one()
        kms += st["kernel_ms"]
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    if rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, best=list(res))          # (zeros_v, zeros_w, index, found) of the last step's enumeration
    per = kms / steps
    algo = st["algo_bytes"]
    out = {"metric": "CoB candidate rows/sec", "value": total * world * steps / dt, "unit": "candidates/s", "n_gpus": world, "steps": steps, "warmup": warm,
           "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
           "data": "synthetic coefficient set over the reference's own data/%s" % fname,
           "config": {"workload": desc, "matrix": fname, "modulus": p, "coefficients": C, "candidates_per_step": total, "block": "rows 0-3 of M^T (4 x %d)" % m},
           "best": {"zeros_v": res[0], "zeros_w": res[1], "index": res[2]},
           "roofline": {"bound": "hbm", "achieved": algo / (per * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": algo / (per * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "traffic": None, "kernel": "plo::cob_kernel", "kernel_ms_per_launch": per, "algo_bytes_per_launch": algo,
                        "note": "the 4 x m block of TM is staged in LDS once per workgroup; the kernel is bound by integer VALU issue (4 modular "
                                "products per column per candidate), HBM traffic is negligible by construction"}}
    out["roofline"]["kernel"] = "plo::cob_tab_kernel"
    ir = issue_roofline("cob", "plo::cob_tab_kernel", per)
    if ir:
        out["roofline_hbm"] = out["roofline"]; out["roofline"] = ir       # the issue view is the meaningful one; the HBM figure stays beside it
    if args.full and not args.no_cpu_baseline and world == 1:
        # BASELINE configs[2] AS WRITTEN (`bin/sparsifier -c 4 data/4x4x4_49_156_L.sms`, over Q): 4^4 = 256 candidate rows per enumeration, a few
        # dozen enumerations per run -- wall clock of the whole command on the GPU (two 31-bit primes per enumeration + check over Q) and on the host
        import re as _re
        import subprocess as _sp
        sps = os.path.join(ROOT, "bin", "sparsifier")
        aw = {}
        try:
            for tag, extra in (("gpu", []), ("host", ["--gpu", "0"])):
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    r = _sp.run([sps, "-c", "4", "-S"] + extra + [os.path.join(DATA, fname)], capture_output=True, text=True, timeout=300)
                    d = time.perf_counter() - t0
                    best = d if best is None else min(best, d)
                aw[tag + "_wall_s"] = best
                g = _re.search(r"with (\d+) non-zeroes", r.stderr)
                aw[tag + "_nnz_residue"] = int(g.group(1)) if g else None
                g = _re.search(r"# GPU \(Q[^)]*\): (\d+) enumerations in (\d+) launches[^,]*, kernels ([0-9.e+-]+) ms", r.stderr)
                if g:
                    aw["gpu_enumerations"] = int(g.group(1)); aw["gpu_launches"] = int(g.group(2)); aw["gpu_kernel_ms"] = float(g.group(3))
                g = _re.search(r"# CoB enumeration: (\d+) candidate rows", r.stderr)
                if g:
                    aw["candidate_rows"] = int(g.group(1))
            aw["note"] = ("256 candidate rows per enumeration: the command is bound by process start, HIP initialisation and one launch + copy per "
                          "enumeration (both primes in one launch, plo_cob_search_batch), not by the enumeration; the GPU pays from about 12 coefficients (2e4 rows per enumeration) on -- the "
                          "headline figure above is `-c 56` (9.8e6 rows per enumeration)")
        except Exception as e:       # the tools are built by __graft_entry__.build(); a missing binary only drops this block
            aw["error"] = str(e)
        out["as_written_c4"] = aw
        # a bounded sample of the same enumeration on one host core: grow the coefficient set until the walk takes 10 s or more
        Cb, d = 14, 0.0
        while True:
            t0 = time.perf_counter()
            oracle_cob_search(n, m, TM, Cand, 0, 0, coeffs[:Cb], p)
            d = time.perf_counter() - t0
            if d >= 10.0 or Cb >= len(coeffs):
                break
            Cb = min(len(coeffs), max(Cb + 2, int(Cb * (12.0 / max(d, 1e-3)) ** 0.25)))
        out["cpu_baseline"] = {"value": Cb ** 4 / d, "unit": "candidates/s", "cores": 1, "kind": "port",
                               "sample": "%d^4 = %d candidate rows of the same block through oracle/plo_oracle.c (rank by elimination per candidate, "
                                         "as the reference), single thread, %.1f s" % (Cb, Cb ** 4, d)}
        out["as_written_c4"]["default_tool"] = ("since round 4 bin/sparsifier walks enumerations of fewer than 20,000 candidate rows on the host by default "
                                                "(--gpu-min-rows): `-c 4` as written makes no launch at all; gpu_wall_s above is the tool with its default")
    print(json.dumps(out))


def bench_tril(args):
    """configs[3]: the restart loop of SearchTriLinearAlgorithm (plinopt_inplace.inl:837-924) on the GPU."""
    import torch
    from plinopt_amd import capi, TrilPlan
    from plo_testlib import DATA, OracleTril
    name, _, batch, desc = WORKLOADS["tril"]
    if args.batch:
        batch = args.batch
    from plinopt_amd.dist import allreduce_tril_best
    rank, local_rank, world, dev, barrier, max_over_ranks = dist_setup(args)
    capi.check(capi.lib().plo_init(local_rank))
    O = OracleTril.from_sms(*(os.path.join(DATA, name + x) for x in ("_L.sms", "_R.sms", "_P.sms")))
    G = TrilPlan(O.m, [(n, rp, col, [int(x) for x in num]) for n, (rp, col, num, den) in zip(O.dims, O.csr)])
    steps = args.steps if args.steps is not None else 10
    warm = args.warmup if args.warmup is not None else 2
    gb = batch * world                               # seeds of one step over all ranks: contiguous shards, no data-path collective

    wall = [0.0, 0.0]                                # this rank's time inside the library call and inside the all-reduce, timed steps

    def one(k, timed=False):
        s0 = k * gb
        t_a = time.perf_counter()
        r = G.search(s0 + rank * batch, batch)       # ((ADD, SCA, MUL), seed, variant) of this rank's shard
        t_b = time.perf_counter()
        seed, variant, word, fl = allreduce_tril_best(r, s0, device=dev, fields=True)      # ONE MIN all-reduce (order ADD, SCA, seed, variant)
        if timed:
            wall[0] += t_b - t_a; wall[1] += time.perf_counter() - t_b
        return r, seed, variant, fl

    for k in range(warm):
        one(k)
    barrier()
    kms = 0.0
    best = None
    t0 = time.perf_counter()
    for k in range(steps):
        r, seed, variant, fl = one(warm + k, True)
        kms += G.last_stats["kernel_ms"]
        key = (fl[0], fl[1], seed, variant)                 # (ADD, SCA) decoded by the reduction itself, whichever word layout it used
        best = key if best is None or key < best else best
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    per_rank_ms = gather_per_rank(dev, world, kms, wall[0], wall[1])
    if rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, best=[fl[0], fl[1], seed, variant])      # (ADD, SCA, seed, variant) of the last step's winner
    st = G.last_stats
    per = kms / steps
    algo = st["algo_bytes"] * batch
    out = {"metric": "candidate in-place programs/sec", "value": gb * steps / dt, "unit": "candidates/s", "n_gpus": world, "steps": steps, "warmup": warm,
           "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "i16",
           "data": "synthetic seeds over the reference's own data/%s_{L,R,P}.sms" % name,
           "config": {"workload": desc, "matrices": name, "per_gpu_batch": batch, "global_batch": gb, "rows": O.m, "dims": list(O.dims),
                      "parallelism": "seed-shard x%d + 1 MIN all-reduce/step" % world},
           "best": {"add": best[0], "sca": best[1], "seed": best[2], "variant": best[3]},
           "per_rank_ms": {"columns": PER_RANK_COLUMNS, "rows": per_rank_ms, "steps": steps},
           "roofline": {"bound": "hbm", "achieved": algo / (per * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": algo / (per * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "traffic": None, "kernel": "plo::tril_kernel", "kernel_ms_per_launch": per, "algo_bytes_per_candidate": st["algo_bytes"],
                        "note": "atom lists are LDS-resident (one wavefront per candidate); HBM sees the three CSR images (L2-resident) and one "
                                "result word per workgroup: the limiter is LDS latency of dependent scans, not HBM"},
           "kernel": {"lds_bytes": st["lds_bytes"], "waves_per_wg": st["waves_per_wg"], "grid": st["grid"]}}
    ir = issue_roofline("tril", "plo::tril_kernel", per)
    if ir:
        out["roofline_hbm"] = out["roofline"]; out["roofline"] = ir
    if args.full and not args.no_cpu_baseline and world == 1:
        n = 2000
        t0 = time.perf_counter()
        ob = O.search(0, n)
        d = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": n / d, "unit": "candidates/s", "cores": 1, "kind": "port",
                               "sample": "%d seeds of the same matrices through oracle/plo_tril_oracle.c, single thread, %.1f s; best %s" % (n, d, list(ob))}
    print(json.dumps(out))


def bench_kmethod(args):
    """The kernel method with everything on the device (plo::kmethod_kernel): restarts of KernelOptimiser
    (plinopt_optimize.inl:1299-1340), seed shards per rank, one 8-byte MIN all-reduce per step."""
    from plinopt_amd import capi, kernel_search
    from plinopt_amd.dist import allreduce_best
    from plo_testlib import OracleMatrix
    m, n, rp, c, v, p, batch, desc, fname = load_matrix("kmethod")
    if args.batch:
        batch = args.batch
    rank, local_rank, world, dev, barrier, max_over_ranks = dist_setup(args)
    capi.check(capi.lib().plo_init(local_rank))
    steps = args.steps if args.steps is not None else 10
    warm = args.warmup if args.warmup is not None else 2
    gb = batch * world

    wall = [0.0, 0.0]

    def one(k, timed=False):
        s0 = 1 + k * gb
        t_a = time.perf_counter()
        _, _, _, b, st = kernel_search((m, n, rp, c, v), p, s0 + rank * batch, batch, want_costs=False)
        t_b = time.perf_counter()
        seed, word, fl = allreduce_best((b[0], b[1], b[2]), s0, device=dev, fields=True)
        if timed:
            wall[0] += t_b - t_a; wall[1] += time.perf_counter() - t_b
        return b, seed, fl, st

    for k in range(warm):
        one(k)
    barrier()
    kms = 0.0
    best = None
    t0 = time.perf_counter()
    for k in range(steps):
        b, seed, word, st = one(warm + k, True)             # word: the decoded cost fields (sum, adds), comparable across steps whatever layout was reduced
        kms += st["kernel_ms"]
        best = (word, seed) if best is None or (word, seed) < best else best
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    per_rank_ms = gather_per_rank(dev, world, kms, wall[0], wall[1])
    if rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, best=[word[0], word[1], seed])          # (adds + muls, adds, seed) of the last step's winner
    per = kms / steps
    out = {"metric": "kernel-method restarts/sec", "value": gb * steps / dt, "unit": "restarts/s", "n_gpus": world, "steps": steps, "warmup": warm,
           "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
           "data": "synthetic seeds over the reference's own data/%s" % fname,
           "config": {"workload": desc, "matrix": fname, "rows": m, "cols": n, "nnz": len(c), "modulus": p, "per_gpu_batch": batch, "global_batch": gb,
                      "parallelism": "seed-shard x%d + 1 MIN all-reduce/step" % world},
           "best": {"seed": best[1]},
           "per_rank_ms": {"columns": PER_RANK_COLUMNS, "rows": per_rank_ms, "steps": steps},
           "roofline": issue_roofline("kmethod", "plo::kmethod_kernel", per) or {"bound": "issue", "achieved": 0.0, "peak": 1.0, "unit": "scalar wave-instructions/clk/CU", "frac": 0.0, "traffic": None},
           "kernel": {"lds_bytes": st["lds_bytes"], "waves_per_wg": st["waves_per_wg"], "grid": st["grid"], "launches_per_step": st["launches"]}}
    if args.full and not args.no_cpu_baseline and world == 1:
        M = OracleMatrix(m, n, rp, c, v, p)
        nref = 300
        t0 = time.perf_counter()
        for sd in range(1, 1 + nref):
            M.kernel_restart(sd)
        d = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": nref / d, "unit": "restarts/s", "cores": 1, "kind": "port",
                               "sample": "%d restarts through oracle/plo_oracle.c plo_oracle_kernel_restart, single thread, %.1f s" % (nref, d)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", default="32x32x32", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="candidates per GPU per step (default: per workload)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true", help="also measure the CPU baseline (a plain run times the steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's result as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.workload == "cob":
        return bench_cob(args)
    if args.workload == "tril":
        return bench_tril(args)
    if args.workload == "kmethod":
        return bench_kmethod(args)
    if args.steps is None:
        args.steps = 3 if args.workload == "32x32x32" else 20       # one config-5 step is ~3 s of GPU time
    if args.warmup is None:
        args.warmup = 1 if args.workload == "32x32x32" else 3
    import torch
    import torch.distributed as dist
    from plinopt_amd import CSEPlan, capi, allreduce_best

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but WORLD_SIZE=%d; launch with torch.distributed.run" % (args.gpus, world),
                  file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the product path has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    m, n, rp, c, v, p, batch, desc, fname = load_matrix(args.workload)
    if args.batch:
        batch = args.batch
    plan = CSEPlan(m, n, rp, c, v, p, device=local_rank)      # matrix resident in HBM from here on

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    seed_base = 0
    global_batch = batch * world
    kernel_ms = 0.0
    launches = 0
    best_word = None
    last = None                                    # (adds + muls, adds, seed) of the latest step's winner
    stats = None
    search_s = 0.0                                 # wall time of this rank's searches (library call) and of the all-reduces, timed steps only
    reduce_s = 0.0

    def step(k, timed):
        nonlocal kernel_ms, launches, best_word, last, stats, search_s, reduce_s
        s0 = seed_base + k * global_batch          # this step's global seed range
        my0 = s0 + rank * batch                    # this rank's shard (independent candidates, no exchange)
        t_a = time.perf_counter()
        local = plan.search(my0, batch, capi.COST_SUM_THEN_ADD)
        t_b = time.perf_counter()
        stats = plan.last_stats
        if timed:
            kernel_ms += stats["kernel_ms"]
            launches += stats["launches"]
        seed, word, fl = allreduce_best(local, s0, capi.COST_SUM_THEN_ADD, device=dev, fields=True)   # one MIN all-reduce of 16 bytes (cost word + "fits one word" flag)
        if timed:
            search_s += t_b - t_a
            reduce_s += time.perf_counter() - t_b
        last = (fl[0], fl[1], seed)
        if best_word is None or (fl, seed) < (best_word[2], best_word[1]):
            best_word = (word, seed, fl)
        return seed

    for k in range(args.warmup):
        step(k, False)
    barrier()
    t0 = time.perf_counter()
    for k in range(args.warmup, args.warmup + args.steps):
        step(k, True)
    barrier()
    dt = time.perf_counter() - t0
    tt = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())

    total = float(global_batch) * args.steps
    value = total / dt
    # where a loss of scaling would come from: every rank's kernel time, search wall time and time inside the all-reduce
    per_rank_ms = gather_per_rank(dev, world, kernel_ms, search_s, reduce_s)
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, best=list(last))
        # dominant kernel: cse_wave_kernel; algorithmic bytes per candidate B_cand
        per_launch_ms = kernel_ms / max(launches, 1)
        algo_bytes = stats["algo_bytes"]
        # the winner's extra 1-candidate launch is included in `launches`; price the search launch only
        search_ms = kernel_ms / args.steps
        achieved = algo_bytes * batch / (search_ms * 1e-3) / 1e9
        out = {
            "metric": "candidate SLPs/sec", "value": value, "unit": "candidates/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u32", "data": "synthetic seeds over the reference's own data/%s" % fname,
            "config": {"workload": desc, "matrix": fname, "modulus": p, "per_gpu_batch": batch,
                       "global_batch": global_batch, "parallelism": "seed-shard x%d + 1 MIN all-reduce/step" % world,
                       "nnz": len(c), "rows": m, "cols": n},
            "best": {"packed": best_word[0], "seed": best_word[1], "adds_plus_muls": best_word[2][0], "adds": best_word[2][1]},
            "per_rank_ms": {"columns": PER_RANK_COLUMNS, "rows": per_rank_ms, "steps": args.steps},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                         "kernel": "plo::cse_wave_kernel", "kernel_ms_per_launch": search_ms,
                         "launches_timed": launches, "avg_ms_all_launches": per_launch_ms,
                         "algo_bytes_per_candidate": algo_bytes,
                         "note": "state is LDS-resident by design; HBM fraction ~0, limiter is LDS/VALU issue (DESIGN.md)"},
            "kernel": {"lds_bytes": stats["lds_bytes"], "waves_per_wg": stats["waves_per_wg"], "grid": stats["grid"]},
        }
        tr = None
        try:    # measured HBM bytes (PMC) from the committed profile of this workload, scaled to one launch
            tj = [os.path.join(ROOT, "profiles", f) for f in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json")]
            tr = json.load(open([f for f in tj if os.path.exists(f)][0])).get(args.workload)
            if tr:
                out["roofline"]["traffic"] = (tr["fetch_bytes_per_candidate"] + tr["write_bytes_per_candidate"]) * batch
                out["roofline"]["traffic_source"] = "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, " + tr["source"]
                out["roofline"]["measured_hbm_GBps"] = out["roofline"]["traffic"] / (search_ms * 1e-3) / 1e9
                out["roofline"]["traffic_over_algorithmic"] = out["roofline"]["traffic"] / (algo_bytes * batch)
                # gfx950: FETCH_SIZE reads 1/2 of the bytes of WIDE (16 B per lane) streaming reads (MI355X_MICROARCH.md, HBM); this kernel's
                # reads are 4- and 8-byte accesses apart from the image copies, so the counter is given as it is and, beside it, the
                # bound with every fetched byte doubled
                out["roofline"]["traffic_fetch_x2"] = (2.0 * tr["fetch_bytes_per_candidate"] + tr["write_bytes_per_candidate"]) * batch
                out["roofline"]["traffic_over_algorithmic_fetch_x2"] = out["roofline"]["traffic_fetch_x2"] / (algo_bytes * batch)
                if "l2_hit_rate" in tr:
                    out["roofline"]["l2_hit_rate"] = tr["l2_hit_rate"]
                    out["roofline"]["l2_requests_per_candidate"] = tr.get("l2_requests_per_candidate")
                if "kernel_source_sha16" in tr:        # the counters were taken on one version of the kernel: say so when it has changed since
                    import hashlib
                    now = hashlib.sha256(open(os.path.join(ROOT, "plinopt_amd", "csrc", "plo_cse_big.hip"), "rb").read()).hexdigest()[:16]
                    out["roofline"]["traffic_stale"] = now != tr["kernel_source_sha16"]
        except Exception:
            pass
        if plan.is_hbm:
            # every figure of the note comes from the JSON files it cites (profiles/r04_traffic.json, profiles/r04_phase_clocks.json)
            note = ("candidate state (5 MB packed rows, 27 MB partitioned triple store + update log, row lists) is HBM-resident; updates of triples below "
                    "the window of top frequency levels are deferred (8-byte log records, merged per partition in LDS)")
            if tr:
                note += ("; measured HBM traffic %.2f GB per candidate = %.1fx the algorithmic bytes, %.2e L2 requests per candidate, L2 hit rate %.0f %% (%s)"
                         % ((tr["fetch_bytes_per_candidate"] + tr["write_bytes_per_candidate"]) / 1e9, out["roofline"]["traffic_over_algorithmic"],
                            tr.get("l2_requests_per_candidate", 0.0), 100.0 * tr.get("l2_hit_rate", 0.0), tr["source"].split(" ")[0]))
            try:
                pc = [os.path.join(ROOT, "profiles", f) for f in sorted(os.listdir(os.path.join(ROOT, "profiles")), reverse=True) if f.endswith("_phase_clocks.json")][0]
                d = json.load(open(pc))
                la, ll = d["alone"]["last_candidate"], d["loaded"]["last_candidate"]
                ph = lambda x: "merges %d, tie pick %d, row search %d, sweep %d, flush %d" % tuple(round(x[k] / 1e3) for k in ("level_and_merges_us", "tie_pick_us", "row_search_us", "sweep_us", "flush_us"))
                note += ("; a candidate ALONE on the chip takes %.0f ms, %d together %.0f ms each: the kernel is bound by the dependent chain of one 8-wave workgroup "
                         "per candidate, not by this streaming `frac`; phase clocks in ms, alone: %s; at full load: %s (%s)"
                         % (d["alone"]["kernel_ms"], d["loaded"]["grid"], d["loaded"]["kernel_ms"] * d["loaded"]["grid"] / d["loaded"]["ncand"], ph(la), ph(ll), os.path.relpath(pc, ROOT)))
            except Exception:
                pass
            out["roofline"]["note"] = note + " (DESIGN.md 2.3)"
            out["kernel"]["family"] = "plo::cse_big_kernel (one workgroup per candidate)"
            out["roofline"]["kernel"] = "plo::cse_big_kernel"
        if not plan.is_hbm:
            ir = issue_roofline(args.workload, "plo::cse_wave_kernel", search_ms)
            if ir:      # LDS-resident candidates: the HBM figure says nothing, report instruction issue (committed PMC counters of this workload)
                out["roofline_hbm"] = out["roofline"]; out["roofline"] = ir
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = (cpu_baseline_host_engine(m, n, rp, c, v, p) if args.workload == "32x32x32"
                                   else cpu_baseline(m, n, rp, c, v, p))
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
