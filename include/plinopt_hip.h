/* ==========================================================================
 * plinopt_hip.h -- C-ABI of libplinopt_hip.so, the MI355X (gfx950) drop-in for
 * PLinOpt's randomized multi-start search for minimum-cost straight-line
 * programs.  The reference has no FFI: the seam is the body of its OpenMP
 * restart loops.  Each entry point names the reference code it replaces
 * (paths relative to the reference tree).  Plain pointers and sizes only.
 *
 * Randomness: the reference draws from a time-seeded thread_local
 * Givaro::GivRandom (include/plinopt_optimize.inl:263-265), so it has no
 * reproducible "seed".  Here every candidate owns a stream defined by its
 * 64-bit seed:  state0 = 1 + splitmix64(seed) mod (2^31-2);
 * next(): state = 950706376*state mod (2^31-1) (the GivRandom LCG);
 * tie pick = next() mod #ties, ties in std::map order of (col_a,col_b,ratio).
 * ========================================================================== */
#ifndef PLINOPT_HIP_H
#define PLINOPT_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* status codes (0 = ok; negative = error; text via plo_last_error()) */
#define PLO_OK            0
#define PLO_E_ARG        -1   /* bad argument (null pointer, p<2, unsorted row ...) */
#define PLO_E_HIP        -2   /* HIP runtime error / no device / extension missing  */
#define PLO_E_CAPACITY   -3   /* matrix too large for the LDS-resident kernel        */
#define PLO_E_UNSUPPORTED -4  /* feature not available on the device path            */
#define PLO_E_INTERNAL   -5   /* device-side consistency check failed                */

/* Sparse matrix over Z_p in CSR: what FMatrix lM(M,F) holds at
 * include/plinopt_optimize.inl:1206 (LinBox SparseMatrix<Field,SparseSeq> after
 * rebind: rows of (column, residue) sorted by column, residues in [1,p)). */
typedef struct {
    uint32_t m, n;            /* rows, columns */
    const uint32_t *rowptr;   /* m+1 */
    const uint32_t *col;      /* nnz, strictly increasing inside a row */
    const uint32_t *val;      /* nnz, canonical residues in [1,p) */
} plo_csr_t;

/* Best candidate: Pair<size_t> nbops of CSEOptimiser (adds, muls) + its seed.
 * adds = muls = UINT32_MAX is the reference's Pair<size_t>{-1,-1} "+infinity"
 * (include/plinopt_optimize.inl:883). */
typedef struct {
    uint32_t adds, muls;
    uint64_t seed;
} plo_best_t;

typedef struct {
    double   seconds;        /* host wall clock of the call (upload excluded if plan reused) */
    double   kernel_ms;      /* sum of search-kernel durations, HIP events on the launch stream */
    uint64_t candidates;     /* candidates evaluated */
    uint32_t launches;       /* kernel launches */
    uint32_t lds_bytes;      /* dynamic LDS per workgroup */
    uint32_t waves_per_wg;   /* candidates in flight per workgroup */
    uint32_t grid;           /* workgroups per launch */
    uint64_t algo_bytes;     /* algorithmic bytes per candidate, B_cand = 8*nnz + 12*P0 + 8 */
    uint32_t reduce;         /* plo_*_search_multi: 1 = the RCCL MIN all-reduce over the devices ran and gave the host's minimum (the one returned) */
    uint32_t reserved;
    double   reduce_seconds; /* plo_*_search_multi: wall time inside the all-reduce (two 8-byte MIN all-reduces; communicator set-up excluded: cached) */
} plo_stats_t;

/* cost order of the restart loop, include/plinopt_optimize.h:53-64 */
#define PLO_COST_SUM_THEN_ADD 0   /* default cmpOpCount            */
#define PLO_COST_ADD_THEN_MUL 1   /* -DOPTIMIZE_ADDITIONS           */
#define PLO_COST_SUM          2   /* -DOPTIMIZE_SUMS                */
#define PLO_COST_RECSUB       3   /* schedule enumeration only: RecSub's order (:958-959) on RecSub's own counts (:950-951):
                                   * additions, then the multiplications BEFORE ProgramGen (multipliers emitted + non +-1
                                   * entries left); plo_best_t.muls then holds that count */

typedef struct plo_plan plo_plan_t;   /* a matrix prepared and resident in HBM */

/* Library life cycle.  device = HIP ordinal (one process per GPU). */
int plo_init(int device);
int plo_shutdown(void);
const char *plo_last_error(void);
int plo_device_count(void);

/* Upload one matrix (replaces the per-restart copies `FMatrix lM(M,F), lT(T,F)`
 * of include/plinopt_optimize.inl:1206-1207: the matrix is converted once). */
int plo_cse_plan_create(const plo_csr_t *A, uint32_t p, plo_plan_t **plan);
/* flags: PLO_PLAN_HBM forces the HBM-resident kernel family (one workgroup per candidate,
 * plo_cse_big.hip) that plo_cse_plan_create selects by itself when a candidate does not fit LDS.
 * Limits of that family (PLO_E_CAPACITY): 32766 rows, 32768 columns (created ones included), rows of 8192 entries, 65536 distinct
 * coefficients, any odd prime below 2^31 -- but a modulus too wide for a residue in the 48-bit pair key beside the columns (above
 * 2^(48 - 2 ceil(log2 columns)); a 31-bit prime: more than 256 columns) needs a matrix of at most 32 distinct coefficients (the key
 * then holds the ratio's identifier). */
#define PLO_PLAN_HBM 1u
int plo_cse_plan_create_ex(const plo_csr_t *A, uint32_t p, uint32_t flags, plo_plan_t **plan);
/* 1 if the plan runs on the HBM-resident kernel family, 0 for the LDS-resident wave kernel */
int plo_cse_plan_is_hbm(const plo_plan_t *plan);
/* Diagnostics of the HBM-resident family, summed over the candidates of the plan's last launch:
 * out[0] CSE steps (OneSub iterations, include/plinopt_optimize.inl:237-312), [1] full pair-table scans,
 * [2] frequency-level rebuilds, [3] tie picks (:260-265) resolved by bisection on the key (more ties in one
 * column than the LDS list holds), [4] pairs that went through the spill list (no room in the LDS aggregation
 * table), [5] sweeps whose claimed-slot list overflowed, [6] candidates, [7] how often the plan was rebuilt with the eager
 * pair table because a candidate outgrew the structures of the deferred updates (sized from the input's triples).
 * (On the device these are the words plo::BigStat names in plo_cse_big.hip: [0]..[6] are BS_SUM_STEPS .. BS_SUM_CANDIDATES,
 * [8] BS_SUM_EXTRA_WINDOWS, [9] BS_SUM_ROWS_SEARCHED, [10] BS_SUM_FORCED_MERGES, [11] BS_SUM_MERGE_GROUPS, [12] BS_SUM_MERGE_LOOP;
 * [7] is kept by the host.) */
int plo_cse_plan_hbm_counters(const plo_plan_t *plan, uint32_t out[8]);
/* the same, the first n <= 13 counters: [10] merges of the deferred updates forced by log or hot-table pressure, [11] groups of partitions
 * summed by the merges, [12] records of those groups loaded behind the four prefetched records of a thread, all three summed over the
 * candidates of the launch; [8] windows of the flat sweep beyond the first one of a batch of rows (a wave takes the entries
 * of its rows 2048 at a time; PLO_BIG_FWIN makes the window smaller in the tests), counted on wave 0; [9] rows walked by the row search
 * (the length of the shorter row list of a step's two columns, summed over steps: reference include/plinopt_optimize.inl:92-94 walks
 * every row). */
int plo_cse_plan_hbm_counters_ex(const plo_plan_t *plan, uint32_t *out, uint32_t n);
/* Host only (nothing is launched): what the plan of the HBM-resident family chose for its matrix and modulus.  out[0] kernel mode
 * (2 ratio identifiers: at most 32 distinct coefficients; 1 value table in LDS: at most 512; 0 value table in global memory), [1] 1 when
 * the pair keys hold the ratio's identifier instead of its residue, [2] 1 for deferred updates (0: the eager pair table), [3] 1 for the
 * kernels with 64-bit workspace offsets, [4] bits of the modulus, [5] bits of a key's ratio field, [6] bits of a key's column fields,
 * [7] bound on the columns (created ones included), [8] distinct coefficients, [9] 1 when an LDS aggregation entry carries the ratio and
 * its inverse, [10] count bits of that entry, [11] k for a Mersenne modulus 2^k - 1 (shift-and-add reduction), else 0 (Barrett),
 * [12] 1 when the table of inverses of every residue exists (moduli up to 2^20), [13] log2 of the LDS aggregation table's entries,
 * [14] log2 of the deferred store's partitions, [15] log2 of the table region's slots.  PLO_E_ARG for a plan of the wave kernel. */
int plo_cse_plan_hbm_info(const plo_plan_t *plan, uint32_t out[16]);
/* Host only (no device is touched): the workspace slice the HBM-resident family lays out for one candidate of a matrix with `rows` rows,
 * `nnz` entries, at most `ncmax` columns (created ones included) and an eager pair table of 2^table_bits slots (10..30).
 * out[0] = bytes of the front region (every array but the table, which comes last: the kernels address the front region with 32-bit
 * offsets), out[1] = bytes of the slice, out[2] = 1 when the front region passes 4 GiB and the plan takes the kernels with 64-bit offsets. */
int plo_cse_hbm_workspace_layout(uint32_t rows, uint32_t nnz, uint32_t ncmax, uint32_t table_bits, uint64_t out[3]);
int plo_cse_plan_destroy(plo_plan_t *plan);

/* Replaces the body of `#pragma omp parallel for` in CSEOptimiser,
 * include/plinopt_optimize.inl:1204-1238 (and the same pattern at :1056-1100,
 * :1137-1177): evaluates candidates seed0 .. seed0+nseeds-1 with the
 * per-candidate kernel Optimizer() (:616-631: OneSub :209-314, RemOneCSE
 * :60-194, ProgramGen :513-611, counts only) and returns the minimum under the
 * total order (cmpOpCount key, seed). Text of the winner is produced by the
 * host replaying `seed` (plo_cse_replay). */
int plo_cse_search_plan(plo_plan_t *plan, uint64_t seed0, uint64_t nseeds,
                        int cost_mode, plo_best_t *out, plo_stats_t *stats);
int plo_cse_search(const plo_csr_t *A, uint32_t p, uint64_t seed0, uint64_t nseeds,
                   int cost_mode, plo_best_t *out, plo_stats_t *stats);
/* The same search over `ndev` devices of one node from ONE process: the restart range in ndev contiguous shards (the blocks
 * bin/optimizer --gpu N uses), one host thread and one device per shard (devices[k], or 0..ndev-1 when devices is NULL;
 * the same ordinal may be listed twice), each thread with its own stream and plan; the result is the minimum under the
 * total order (cmpOpCount key of include/plinopt_optimize.h:53-64, seed) -- what the `#pragma omp critical` of
 * include/plinopt_optimize.inl:1214-1237 keeps.  stats->kernel_ms is the slowest shard's kernel time.  The minimum of the
 * shards is taken on the host and returned.  With two or more DISTINCT devices RCCL cross-checks it over a communicator of the
 * devices (librccl loaded at run time, the communicator kept for the life of the process): one 8-byte MIN all-reduce of the cost
 * key, one of the seed offset among the shards that hold the minimal key -- the lexicographic minimum whatever the width of the
 * costs.  A difference is a '#' diagnostic on stderr.  stats->reduce says whether the all-reduce ran and agreed,
 * stats->reduce_seconds its wall time.  PLO_MULTI_REDUCE=host|rccl overrides (rccl: also with one device; then a missing
 * librccl is an error).  A shard the device refuses (PLO_E_CAPACITY / PLO_E_UNSUPPORTED) makes the call return that code.
 * Across processes bench.py and plinopt_amd/dist.py reduce the same words with torch.distributed (RCCL). */
int plo_cse_search_multi(const plo_csr_t *A, uint32_t p, uint64_t seed0, uint64_t nseeds, int cost_mode,
                         int ndev, const int *devices, plo_best_t *out, plo_stats_t *stats);
/* communicators built by this process so far (one per distinct device set: a second call on the same devices builds none) */
uint64_t plo_multi_comm_inits(void);

/* Same candidates, every (adds, muls) written back: the parity-test entry.
 * seeds == NULL means seed0, seed0+1, ... */
int plo_cse_cost_many_plan(plo_plan_t *plan, const uint64_t *seeds, uint64_t seed0,
                           uint64_t n, uint32_t *adds, uint32_t *muls, plo_stats_t *stats);
int plo_cse_cost_many(const plo_csr_t *A, uint32_t p, const uint64_t *seeds, uint64_t seed0,
                      uint64_t n, uint32_t *adds, uint32_t *muls);

/* Two matrices per candidate, one random stream.  Replaces the body of the restart loop of
 * LUOptimiser, include/plinopt_optimize.inl:1056-1100: Optimizer() on a copy of U (:1068) and then
 * on a copy of L (:1072), op-counts added (:1078-1079), best kept under cmpOpCount (:1081-1099).
 * Both matrices must fit the LDS-resident kernel. */
typedef struct plo_chain plo_chain_t;
int plo_cse_chain_create(const plo_csr_t *first, const plo_csr_t *second, uint32_t p, plo_chain_t **chain);
int plo_cse_chain_destroy(plo_chain_t *chain);
int plo_cse_chain_search(plo_chain_t *chain, uint64_t seed0, uint64_t nseeds, int cost_mode,
                         plo_best_t *out, plo_stats_t *stats);
int plo_cse_chain_cost_many(plo_chain_t *chain, const uint64_t *seeds, uint64_t seed0, uint64_t n,
                            uint32_t *adds, uint32_t *muls, plo_stats_t *stats);

/* The same chained evaluation for MANY pairs in one launch: candidate c (0 <= c < npairs*per_pair) runs on pair c / per_pair with
 * seed seed0 + c.  The kernel method (nullspacedecomp :689-884) has a different pair (Free, Dep) for every restart, or small
 * block of restarts; one plan + one launch per pair would leave the GPU idle.  adds/muls (npairs*per_pair entries) and best
 * may each be NULL.  With PLO_COST_SUM the split of the winner is not returned (best->adds = the sum). */
int plo_cse_chain_batch(uint32_t npairs, const plo_csr_t *firsts, const plo_csr_t *seconds, uint32_t p, uint64_t seed0, uint32_t per_pair,
                        int cost_mode, uint32_t *adds, uint32_t *muls, plo_best_t *best, plo_stats_t *stats);

/* nprob independent restart searches in one call.  Problem q is the loop of CSEOptimiser on firsts[q] (seconds == NULL),
 * or the chained loop of LUOptimiser on (firsts[q], seconds[q]) with one random stream, as plo_cse_chain_*.
 * Candidate j of problem q (0 <= j < per_problem) has seed seed0 + q*per_problem + j.
 * bests[q] = its minimum under (cost key of cost_mode, seed), with the winner's split under every cost mode; status[q] = PLO_OK,
 * or the code with which the LDS-resident wave kernel refuses that problem (PLO_E_CAPACITY / PLO_E_UNSUPPORTED; bests[q] is then
 * +infinity and the other problems are not affected).  One workgroup per problem (plo::cse_batch_kernel), one launch per bucket
 * of LDS footprints; a problem whose pair table fills up is built again with twice the slots and launched again alone (scale 2,
 * 4, 8, 16, then PLO_E_CAPACITY for that problem).  stats->launches counts the launches, stats->candidates the candidates
 * evaluated, those of repeated problems again; the shape fields are the last launch's.  Environment: PLO_BATCH_GRID caps the
 * workgroups of a launch (tests), PLO_BATCH_STATS prints one '#' line per launch on stderr.
 * PLO_E_ARG: a null array (seconds may be), nprob == 0, per_problem == 0, an even modulus or one of 2^31 and more, cost_mode outside
 * 0..2, more than 2^32-1 candidates, a defective matrix. */
int plo_cse_batch_search(uint32_t nprob, const plo_csr_t *firsts, const plo_csr_t *seconds, uint32_t p, uint64_t seed0,
                         uint32_t per_problem, int cost_mode, plo_best_t *bests, int32_t *status, plo_stats_t *stats);

/* The kernel method (plo_kernel_search with per_block = 1) on nprob matrices in one call, one minimum each.
 * Restart j of problem q (0 <= j < per_problem) has seed seed0 + q*per_problem + j, which is also the seed of its decomposition.
 * bests[q] = the minimum under (cost key of cost_mode, seed) over the problem's own seeds, with the winner's split under every cost
 * mode and the absolute seed; status[q] = PLO_OK, or the code plo_kernel_search gives that matrix:
 *   PLO_E_UNSUPPORTED  zero dimensional kernel, zero matrix, more than 128 rows, more than 64 columns, more than 64 dependent rows;
 *   PLO_E_CAPACITY     more than 64 rows with an entry other than +-1, a pair key too wide, Dep's image does not fit the LDS, or its
 *                      tables are still too small at scale 32;
 *   PLO_E_INTERNAL     a device decomposition that contradicts the host's rank (ERR_KDEC).
 * For any status but PLO_OK bests[q] is +infinity (2^32-1, 2^32-1, 2^64-1) and the other problems are not affected.
 * One workgroup per problem (plo::kmethod_batch_kernel), one launch per bucket of LDS footprints (row starts + region + scratch, the
 * classes of plo_cse_batch_search), 8, 4, 2 or 1 waves per workgroup by LDS and at most twice per_problem.  Before the search ONE
 * sizing launch decomposes the first min(per_problem, 64) restarts of every problem and Dep's image is laid out from their largest
 * entry and pair counts (+60 %, 0.75 x); a problem whose hard bounds (dependent rows x rank entries, dependent rows x rank (rank - 1) / 2
 * pairs) are small -- at most 32 pairs, or an image that does not enlarge the wave's region -- is laid out from those and not sampled
 * (a call with only such problems has no sizing launch).  No result depends on the sample: a restart with more entries or triples than
 * laid out is reported by the device and only that problem is laid out again (scale 2, 4, .. 32: hard bound for the entries, scale x
 * the pairs for the table) and launched again alone.  stats->launches counts the sizing launch too, stats->candidates the search
 * candidates, those of repeated problems again; the shape fields are the last search launch's.  Environment: PLO_BATCH_GRID and
 * PLO_BATCH_STATS as for plo_cse_batch_search; the PLO_KMETHOD_* knobs of plo_kernel_search act on every sampled problem.
 * PLO_E_ARG, before any use of the device: a null array, nprob == 0, per_problem == 0, an even modulus, one below 3 or of 2^31 and
 * more, cost_mode outside 0..2, more than 2^32-1 candidates, a defective matrix. */
int plo_kernel_batch_search(uint32_t nprob, const plo_csr_t *mats, uint32_t p, uint64_t seed0, uint32_t per_problem,
                            int cost_mode, plo_best_t *bests, int32_t *status, plo_stats_t *stats);


/* The kernel method of bin/optimizer -K with EVERYTHING on the device (plo::kmethod_kernel): restart c (seed seed0 + c) is one
 * pass of the loop of KernelOptimiser, include/plinopt_optimize.inl:1299-1340 -- a nullspace decomposition of M
 * (nullspacedecomp :689-884: random row order, greedy row basis, NotIndep; this build's rule, restated in
 * oracle/plo_oracle.c plo_oracle_kernel_restart), then Optimizer() on Free and on Dep from one random stream (:1322-1333).
 * per_block > 1: the restarts of a block of per_block consecutive seeds share the decomposition of the block's first seed.
 * adds/muls (nrestarts entries), info (3 per restart: rank, NotIndep, number of dependent rows computed through Dep) and best may each be NULL.
 * M needs at most 128 rows, 64 columns, 64 dependent rows and a kernel of positive dimension (PLO_E_UNSUPPORTED otherwise: the caller
 * falls back to host decompositions + plo_cse_chain_batch).  PLO_E_CAPACITY: more than 64 rows with an entry other than +-1, or a Dep
 * whose pair table outgrows the LDS (sized from a sample of the decompositions: 128x64 with three random entries per row is one).
 * Empty rows of M are admitted: an empty row is a dependent row whose combination is empty, i.e. a row of Dep without entry (a matrix
 * of empty rows only is refused: PLO_E_UNSUPPORTED, "zero matrix").  With PLO_COST_SUM best->adds holds the sum and best->muls 0, as
 * plo_cse_chain_batch. */
int plo_kernel_search(const plo_csr_t *M, uint32_t p, uint64_t seed0, uint64_t nrestarts, uint32_t per_block, int cost_mode,
                      uint32_t *adds, uint32_t *muls, uint32_t *info, plo_best_t *best, plo_stats_t *stats);
/* The kernel method over PRESCRIBED row orders (bin/optimizer -N; replaces the loop body of AllKernelOpt, include/plinopt_optimize.inl:
 * 1357-1418, which decomposes M once for every order of its rows).  Order index pi (first <= pi < first + count) is the pi-th
 * permutation of 0..m-1 in lexicographic order: that of std::next_permutation from the identity, and of the reference's factoradic
 * kthpermutation (include/plinopt_library.inl:289-304).  Candidate c (0 <= c < count*sub) is restart j = c % sub of order
 * pi = first + c / sub: the decomposition in that order with NotIndep the FIRST draw of the stream of seed0 + pi (no shuffle; restated
 * in oracle/plo_oracle.c plo_oracle_kernel_order), then Optimizer() on Free and on Dep from the stream of seed0 + pi*sub + j.  Both seeds
 * depend on pi only, not on first: the results of ranges compose, and a walk of all m! orders may be split into calls, processes or
 * machines at will.  adds/muls (count*sub entries), info (3 per candidate: rank, NotIndep, dependent rows computed through Dep) and best
 * may each be NULL.  best is the minimum under (cost key of cost_mode, candidate index), the smaller index winning ties; best->seed holds
 * the winner's seed0 + pi*sub + j, so pi = (best->seed - seed0) / sub and j = (best->seed - seed0) % sub.  With PLO_COST_SUM best->adds
 * holds the sum and best->muls 0.  The call runs in launches of at most 2^25 candidates; stats->candidates, kernel_ms and launches are
 * sums over them.  PLO_E_ARG: fewer than 2 or more than 12 rows, count == 0, sub == 0, first + count > m!.  Otherwise the limits and
 * codes of plo_kernel_search (PLO_E_UNSUPPORTED: a kernel of dimension zero, a zero matrix, more than 64 columns). */
int plo_kernel_search_orders(const plo_csr_t *M, uint32_t p, uint64_t seed0, uint64_t first, uint64_t count, uint32_t sub, int cost_mode,
                             uint32_t *adds, uint32_t *muls, uint32_t *info, plo_best_t *best, plo_stats_t *stats);
/* The restart loop of KernelOptimiser (include/plinopt_optimize.inl:1299-1340) over `ndev` devices from one process: contiguous
 * shards of the restart range, one host thread and one device each, minimum under (cmpOpCount key, seed) by the RCCL MIN
 * all-reduces of plo_cse_search_multi (same conventions for devices, stats->reduce and PLO_MULTI_REDUCE).  per_block must be 1
 * with more than one device.  BASELINE `bin/optimizer -K --gpu N`. */
int plo_kernel_search_multi(const plo_csr_t *M, uint32_t p, uint64_t seed0, uint64_t nrestarts, uint32_t per_block, int cost_mode,
                            int ndev, const int *devices, plo_best_t *best, plo_stats_t *stats);


/* Change-of-basis (CoB) search of bin/sparsifier: one (block,row) enumeration of `localSparsifier`,
 * include/plinopt_sparsify.inl:282-314, i.e. |coeffs|^4 calls of `testLinComb` (:167-197).  TM is the n x m
 * matrix being sparsified (dense, row major, residues mod p), Cand the n x n matrix whose rows 0..row-1 are the
 * rows already chosen; candidate (i,j,k,l) is the row w with w[offsetblock+t] = coeffs[(i,j,k,l)[t]] (positions
 * >= n dropped, :305-310).  Result: the first candidate in lexicographic (i,j,k,l) order that is independent of
 * the chosen rows and maximises (zeros(TM^T w), zeros(w)), if it beats (w0,w1) strictly; index = ((i*C+j)*C+k)*C+l.
 * TM, Cand and coeffs are taken modulo p, so a coefficient congruent to 0 counts as a zero of w; any w0 < 0 is beaten by every
 * candidate, (w0 >= 0, w1 < 0) by every (w0, .), and (w0, w1 > n) by no (w0, .). */
typedef struct {
    int32_t  zeros_v, zeros_w;   /* score of the winner (or the incoming w0,w1 when nothing beats them) */
    uint64_t index;              /* flattened (i,j,k,l) */
    uint32_t found;              /* 1 if some candidate beat (w0,w1) */
} plo_cob_best_t;
int plo_cob_search(uint32_t n, uint32_t m, const uint32_t *TM, const uint32_t *Cand, uint32_t row, uint32_t offsetblock,
                   const uint32_t *coeffs, uint32_t ncoeffs, uint32_t p, int32_t w0, int32_t w1,
                   plo_cob_best_t *out, plo_stats_t *stats);
/* The same enumeration restricted to the prefixes (i,j,k) first_group .. first_group+ngroups-1 (in the order of the
 * loops at include/plinopt_sparsify.inl:299-303), every l: one shard of the |coeffs|^4 candidates.  The winner of the
 * whole enumeration is the shard winner of largest (zeros_v, zeros_w), smallest index among equals (one 8-byte MAX
 * all-reduce of the packed word, plinopt_amd/dist.py). */
int plo_cob_search_range(uint32_t n, uint32_t m, const uint32_t *TM, const uint32_t *Cand, uint32_t row, uint32_t offsetblock,
                         const uint32_t *coeffs, uint32_t ncoeffs, uint32_t p, int32_t w0, int32_t w1,
                         uint64_t first_group, uint64_t ngroups, plo_cob_best_t *out, plo_stats_t *stats);

/* Up to 4 enumerations of the same shape (n, m, row, offsetblock) in ONE launch -- one upload, one kernel, one download: the two
 * primes of an enumeration over the rationals (bin/sparsifier without -q calls localSparsifier :282-314 once over Q; this build
 * enumerates modulo two primes and checks the winners over Q), or the shards of one enumeration.  out[k] as plo_cob_search. */
typedef struct {
    const uint32_t *TM, *Cand, *coeffs;   /* residues modulo p, as for plo_cob_search */
    uint32_t ncoeffs, p;
    int32_t  w0, w1;
} plo_cob_problem_t;
int plo_cob_search_batch(uint32_t nprob, uint32_t n, uint32_t m, uint32_t row, uint32_t offsetblock,
                         const plo_cob_problem_t *prob, plo_cob_best_t *out, plo_stats_t *stats);

/* ---- -E, the exhaustive CSE tree: RecSub / RecOptimizer (include/plinopt_optimize.inl:889-1013, called by AllCSEOpt
 * :1252-1281) explore every schedule of pairs of frequency > 1 (not only the maximal ones).  Here a schedule is a
 * candidate addressed by an index in the mixed radix of its own path: at every step the children (distinct triples of
 * frequency > 1, in std::map order) are numbered 0..T-1; digit = index mod T, index /= T.  The product of the radices met by
 * a candidate is returned; the indices first..first+count-1 = 0..N-1 cover the whole tree as soon as N >= *maxprod (the
 * largest product seen).  Cost = op-count of the program Optimizer would print for that schedule; RecSub's order is
 * PLO_COST_ADD_THEN_MUL (:958-959).  LDS-resident plans only (PLO_E_UNSUPPORTED otherwise). */
int plo_cse_enum_cost_many_plan(plo_plan_t *plan, uint64_t first, uint64_t n, uint32_t *adds, uint32_t *muls, uint64_t *prods, plo_stats_t *stats);
int plo_cse_enum_search_plan(plo_plan_t *plan, uint64_t first, uint64_t count, int cost_mode, plo_best_t *best /* .seed = index */,
                             uint64_t *maxprod, plo_stats_t *stats);

/* ---- In-place trilinear search: replaces the body of the restart loop of SearchTriLinearAlgorithm
 * (include/plinopt_inplace.inl:837-924; driver src/trilplacer.cpp:150-152).  A (m x nA), B (m x nB) and T = transpose of
 * the product matrix (m x nT), integer CSR with columns sorted per row.  One candidate (seed) = row permutation +
 * coherent row negations drawn from the seed's stream, then the oriented (variant 0) and the unoriented (variant 1)
 * in-place program of TriLinearProgram :732-806; cost = (ADD, SCA) lexicographic as :893-897, ties to the smaller
 * (seed, variant).  seed == PLO_TRIL_BASE_SEED is the unpermuted oriented program of :829.  The device path takes
 * matrices without empty row and with rows of at most 64 entries (PLO_E_UNSUPPORTED otherwise: such inputs stay on the
 * host); integer entries here, rationals through plo_tril_plan_create_q.  The host replays the winning (seed, variant) to print the program. */
#define PLO_TRIL_BASE_SEED 0xFFFFFFFFFFFFFFFFull
typedef struct { uint32_t m, n; const uint32_t *rowptr; const uint32_t *col; const int32_t *val; } plo_icsr_t;
typedef struct { uint32_t add, sca, mul; uint32_t variant; uint64_t seed; } plo_tril_best_t;
typedef struct plo_tril_plan plo_tril_plan_t;
int  plo_tril_plan_create(const plo_icsr_t *A, const plo_icsr_t *B, const plo_icsr_t *T, plo_tril_plan_t **plan);
/* expanded != 0: `trilplacer -e` (src/trilplacer.cpp:80,114-137): the program of T is TransposedDoubleAlgorithm
 * (include/plinopt_inplace.inl:507-598) on DoubleExpand(T) (:676-716, built on the device from the m-row T); a candidate
 * returns (ADD, SCA) of that variant and MUL = m double-size AXPYs (:799). */
int  plo_tril_plan_create_x(const plo_icsr_t *A, const plo_icsr_t *B, const plo_icsr_t *T, int expanded, plo_tril_plan_t **plan);
/* Rational coefficients num/den (den == NULL: all 1), as the reference's matrices are (Givaro::Rational, include/plinopt_inplace.inl:19):
 * the atoms of the device programs carry the coefficients' images modulo the 31-bit prime 2147483629 (an additive atom its signed
 * coefficient, a multiplicative atom its factor: what cumulate/isnoop/complexity, :96-144, depend on); the tool replays and checks the
 * winner over Q.  All entries +-1: the kernel of rounds 1-2.  expanded != 0 takes rational coefficients too (round 4: the scaling
 * atoms *y, *a and the atoms of z = -y c y and c of include/plinopt_inplace.inl:532-535, 561-565).  PLO_E_UNSUPPORTED: an empty row,
 * a row of more than 64 entries, or an entry that vanishes modulo the prime. */
typedef struct { uint32_t m, n; const uint32_t *rowptr; const uint32_t *col; const int64_t *num; const int64_t *den; } plo_qcsr_t;
int  plo_tril_plan_create_q(const plo_qcsr_t *A, const plo_qcsr_t *B, const plo_qcsr_t *T, int expanded, plo_tril_plan_t **plan);
/* ---- The restart search of the direct method over the RATIONALS, bit-exact with Optimizer() over Q seed by seed (bin/optimizer --gpu-q).
 * A: rational CSR as above.  The plan is an ordinary plo_plan_t: plo_cse_search_plan, plo_cse_cost_many_plan (every cost mode) and
 * plo_cse_plan_destroy take it; candidate `seed` is the candidate `bin/optimizer --replay --seed` prints without -q.
 * How: every value a candidate can compare lies in the finite universe U = +-(V u R u {1}), V the distinct entries of A and
 * R = { b/a : a, b in V } (RemOneCSE never makes a new value).  The plan keeps residues modulo a 31-bit prime that divides no
 * numerator or denominator of U and keeps U's residues distinct -- 2147483629, else the next primes below it, 8 tried in all -- and the
 * pair keys carry the RANK in U of a ratio, so their order is Q's.  A +-1 matrix runs the +-1 kernel at its speed.
 * PLO_E_UNSUPPORTED, each with its own text and before any device call: more than 64 distinct values; an ordering of U that overflows
 * 128 bits; no separating prime among the 8; a matrix beyond the LDS-resident kernels (the HBM-resident family has no search over Q yet:
 * flags = PLO_PLAN_HBM is refused as well); plo_cse_enum_* on such a plan.  A candidate that meets a value outside U (none can, by the
 * closure argument) makes the call return PLO_E_UNSUPPORTED, never a count.  PLO_E_ARG: null pointers, unknown flags, a defect of the CSR.
 * Test knob PLO_CSE_Q_PRIME=<p>: the first prime tried is the largest one <= p. */
int  plo_cse_plan_create_q(const plo_qcsr_t *A, uint32_t flags, plo_plan_t **plan);
/* Host only (no device is touched): the prime, |V|, |U| and U ascending over Q as num[k]/den[k] (lowest terms, den > 0).  The counts are
 * filled in whenever V and U could be formed; PLO_E_CAPACITY when cap < |U| or an element does not fit 64 bits; otherwise the refusals of
 * plo_cse_plan_create_q that concern U (then *prime is 0). */
int  plo_cse_q_universe(const plo_qcsr_t *A, uint32_t *prime, uint32_t *nvalues, uint32_t *nuniverse, int64_t *num, int64_t *den, uint32_t cap);
void plo_tril_plan_destroy(plo_tril_plan_t *plan);
/* ops6[6k..6k+5] = ADD,SCA,MUL of variant 0 then of variant 1 for candidate k (seeds[k], or seed0+k when seeds==NULL) */
int  plo_tril_cost_many(plo_tril_plan_t *plan, const uint64_t *seeds, uint64_t seed0, uint64_t n, uint32_t *ops6, plo_stats_t *stats);
int  plo_tril_search(plo_tril_plan_t *plan, uint64_t seed0, uint64_t nseeds, plo_tril_best_t *best, plo_stats_t *stats);   /* PLO_E_HIP without plo_init, as plo_lin_search (no live plan exists then) */
/* The restart loop of SearchTriLinearAlgorithm (include/plinopt_inplace.inl:837-924) over `ndev` devices from one process --
 * BASELINE configs[3], `bin/trilplacer L R P` seed-sharded over the GPUs of a node with an RCCL MIN: contiguous shards of the seed
 * range, one host thread, one device and one plan (plo_tril_plan_create_q of the three matrices) each; the winner is the minimum
 * under (ADD, SCA) (:893-897), then (seed, variant), by the two MIN all-reduces of plo_cse_search_multi: (ADD << 32 | SCA), then
 * ((seed - seed0) << 1 | variant) among the shards holding the minimal cost.  Same conventions for devices, stats and
 * PLO_MULTI_REDUCE. */
int  plo_tril_search_multi(const plo_qcsr_t *A, const plo_qcsr_t *B, const plo_qcsr_t *T, int expanded, uint64_t seed0, uint64_t nseeds,
                           int ndev, const int *devices, plo_tril_best_t *best, plo_stats_t *stats);

/* ---- In-place linear search: replaces the body of the restart loop of SearchLinearAlgorithm
 * (include/plinopt_inplace.inl:621-669; driver src/inplacer.cpp:38-80).  A (m x n) as rational CSR (plo_qcsr_t above, columns
 * sorted per row; empty rows allowed: the barrier Atom(' ', l, ' ', 0) of :474-476).  One candidate (seed) = a row permutation
 * drawn from the seed's stream (no sign flips), then variant 0 = the unoriented program (:636) and variant 1 = the oriented
 * program APPENDED to variant 0's simplified one (:654: the reference does not clear lProgram), simplified and counted as one
 * program (ROWS = 2m); cost = (ADD, SCA) lexicographic as :637-641, ties to the smaller (seed, variant).  seed ==
 * PLO_LIN_BASE_SEED is the unpermuted oriented program of :613 (the incumbent; both halves of ops6 hold it).  Entries +-1 run
 * the unit kernel, others are residues modulo the 31-bit prime 2147483629 (as plo_tril_plan_create_q); the host replays and
 * checks the winner over Q.  PLO_E_UNSUPPORTED: a row of more than 64 entries, or an entry that vanishes modulo the prime;
 * PLO_E_CAPACITY: more than 16382 rows or columns, or a program that does not fit LDS.  Without a device every entry returns
 * PLO_E_HIP. */
#define PLO_LIN_BASE_SEED 0xFFFFFFFFFFFFFFFFull
typedef struct { uint32_t add, sca, rows; uint32_t variant; uint64_t seed; } plo_lin_best_t;
typedef struct plo_lin_plan plo_lin_plan_t;
int  plo_lin_plan_create_q(const plo_qcsr_t *A, plo_lin_plan_t **plan);
void plo_lin_plan_destroy(plo_lin_plan_t *plan);
/* ops6[6k..6k+5] = ADD,SCA,ROWS of variant 0 then of variant 1 for candidate k (seeds[k], or seed0+k when seeds==NULL) */
int  plo_lin_cost_many(plo_lin_plan_t *plan, const uint64_t *seeds, uint64_t seed0, uint64_t n, uint32_t *ops6, plo_stats_t *stats);
int  plo_lin_search(plo_lin_plan_t *plan, uint64_t seed0, uint64_t nseeds, plo_lin_best_t *best, plo_stats_t *stats);
/* The restart loop over `ndev` devices from one process: contiguous shards of the seed range, one host thread, one device and
 * one plan each, the minimum under (ADD, SCA), then (seed, variant), by the two MIN all-reduces of plo_cse_search_multi.  Same
 * conventions for devices, stats and PLO_MULTI_REDUCE. */
int  plo_lin_search_multi(const plo_qcsr_t *A, uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_lin_best_t *best, plo_stats_t *stats);

/* ---- De Groote orbit search: replaces the body of the restart loop of src/orbiter.cpp:272-324.  (L, R, P) is a row-major
 * triple of an m x k x n product (L: r x mk, columns a k + b; R: r x kn, columns b n + c; P: mn x r, rows a n + c) as
 * rational CSR; m, k, n come from the shapes by an exact integer square root.  A candidate (U, V, W) transforms it into
 * L.(U^-1 (x) V), R.(V^-T (x) W), (U (x) W^-1).P and is scored by three counts: nnz (non-zero entries), nno (those that are
 * not +-1) and cost = nnz (PLO_ORBIT_DENSITY, `-s`, and every run modulo a number) or L.m + R.m + P.n minus the rows of
 * L.J and R.G and columns of H.P with exactly one non-zero (PLO_ORBIT_CANONICAL, `-c`).
 * Stream of candidate `seed` (the reference's zoiRandomMatrix, :58-139, default branch :125-136, made reproducible): the
 * CandRng of the seed (splitmix64, then x <- 950706376 x mod 2^31-1); U (m x m), then V (k x k), then W (n x n), each of size
 * s drawn as: P by Fisher-Yates (for i = s down to 2, swap P[i-1] and P[next() % i]), Q the same way, D[i] = next() & 1 for
 * i = 0..s-1, then row-major for i < j: M[P[i]][Q[j]] = next() % 3 - 1; the diagonal M[P[i]][Q[i]] = D[i] ? 1 : -1.
 * That is the action PLO_ORBIT_ACT_TRIANGULAR (0), the default.  The reference offers two other distributions at compile
 * time (ACTION_FULL_PLUQ :77-96, ACTION_HOUSEHOLDER :98-123); here the action is a run-time choice of the plan.  For every
 * action a matrix of size s starts alike: P, then Q, then D as above.  Then:
 *   PLO_ORBIT_ACT_PLUQ (1): Lambda lower triangular, Lambda[i][i] = D[i] ? 1 : -1, then row-major for j < i
 *     Lambda[i][j] = next() % 3 - 1; then for i = 0..s-1 a vector u_i with u_i[Q[i]] = 1, u_i[j] = next() % 3 - 1 for
 *     j = 0..Q[i]-1 in that order and zeros behind; row P[i] of M is Lambda.u_i: M[P[i]][c] = sum_j Lambda[c][j] u_i[j].
 *     M = Pi_P Um Lambda^T (Um: the rows u_i, unit lower triangular once sorted by Q[i]): det +-1 and an integral inverse.
 *   PLO_ORBIT_ACT_HOUSEHOLDER (2): u[i] = next() % 3 - 1 for i = 0..s-1, d = sum u[i]^2.  When d is a unit of the run's field
 *     (d != 0 over Q; gcd(d, modulus) = 1 modulo a number) M[P[i]][Q[j]] = +-(delta_ij - 2 u[i] u[j] / d) with the sign of
 *     D[i] (an orthogonal matrix over Q), otherwise M is the signed permutation M[P[i]][Q[i]] = +-1.  (The reference tests
 *     d == 0 only and would divide by a non-unit of a composite modulus; the permutation branch there is this build's reading.)
 * U is drawn first, then V, then W, for every action.
 * seed == PLO_ORBIT_BASE_SEED is U = V = W = identity, for every action: the input itself.
 * Order: the lexicographic minimum of (cost, nnz, nno, seed); the tool's winner improves on the input iff its (cost, nnz, nno)
 * is smaller than the input's.
 * modulus 0 is Q: the rows of L and R and the columns of P are scaled to integers on the host, and the counts are exact.
 * PLO_E_UNSUPPORTED: a modulus of 2^31 or more, a denominator that is no unit modulo the modulus, or a Q input whose
 * transformed entries are not provably below 2^62: the row's L1 norm (after scaling) times the entry bounds of the part's two
 * factors, a direct one of size sd and an inverse of size si ((sd, si) = (k, m) for L, (n, k) for R, (m, n) for P), must stay
 * below 2^62.  TRIANGULAR: 1 x 2^(si-2).  PLUQ: sd x si 4^(si-2) (1 for si = 1).  HOUSEHOLDER: sd x si (numerators over d), and
 * the row's scale times sd si as well.  PLO_E_CAPACITY: m, k or n above 16, more
 * than 4096 rows, 2^21 transformed entries or more, or an input that does not fit LDS.  PLO_E_ARG: shapes that are not
 * m k, k n, m n, or an unknown action. */
#define PLO_ORBIT_BASE_SEED 0xFFFFFFFFFFFFFFFFull     /* U = V = W = identity: the input itself */
#define PLO_ORBIT_DENSITY   0                          /* -s */
#define PLO_ORBIT_CANONICAL 2                          /* -c */
#define PLO_ORBIT_CSE       1                          /* -z: operations of the best programs found, see below */
#define PLO_ORBIT_ACT_TRIANGULAR  0                    /* signed permutation times one triangle (the default) */
#define PLO_ORBIT_ACT_PLUQ        1                    /* a product of two triangles */
#define PLO_ORBIT_ACT_HOUSEHOLDER 2                    /* an orthogonal reflection, or a signed permutation */
typedef struct { uint32_t cost, nnz, nno, reserved; uint64_t seed; } plo_orbit_best_t;
typedef struct plo_orbit_plan plo_orbit_plan_t;
int  plo_orbit_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P,
                             uint64_t modulus /* 0 = Q */, int measure, plo_orbit_plan_t **plan);
/* the same with the action (PLO_ORBIT_ACT_*); plo_orbit_plan_create_q is action PLO_ORBIT_ACT_TRIANGULAR.  The functions
 * below serve the plans of every action. */
int  plo_orbit_plan_create_act(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P,
                               uint64_t modulus /* 0 = Q */, int measure, int action, plo_orbit_plan_t **plan);
void plo_orbit_plan_destroy(plo_orbit_plan_t *plan);
/* out3[3k..3k+2] = cost, nnz, nno of candidate k (seeds[k], or seed0+k when seeds==NULL) */
int  plo_orbit_cost_many(plo_orbit_plan_t *plan, const uint64_t *seeds, uint64_t seed0, uint64_t n,
                         uint32_t *out3 /* cost, nnz, nno per seed */, plo_stats_t *stats);
int  plo_orbit_search(plo_orbit_plan_t *plan, uint64_t seed0, uint64_t nseeds, plo_orbit_best_t *best, plo_stats_t *stats);
/* The restart loop over `ndev` devices from one process, as plo_lin_search_multi: contiguous shards, one host thread, device
 * and plan each, the minimum under (cost, nnz, nno, seed).  Same conventions for devices, stats and PLO_MULTI_REDUCE. */
int  plo_orbit_search_multi(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure,
                            uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_best_t *best, plo_stats_t *stats);
int  plo_orbit_search_multi_act(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure, int action,
                                uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_best_t *best, plo_stats_t *stats);

/* PLO_ORBIT_CSE (`-z`, reference src/orbiter.cpp:172-209): over Z_p, p an odd prime below 2^31, the transformed triple (Lj, Rg, hP)
 * is the one the density measure counts (entries that vanish modulo p dropped; hP is mn x r) and
 *   cost = c(Lj) + c(Rg) + c(hP),   c(M) = min(naive(M), min over j < sub of ops_j(M)),
 * naive(M) = sum over the rows of max(len - 1, 0) + the entries that are not +-1 (naiveOps), ops_j(M) = adds + muls of
 * Optimizer(M) with the stream of seed cse_seed0 + j: the numbers plo_cse_cost_many returns for M.  A matrix without entries
 * costs 0.  nnz, nno, the order (cost, nnz, nno, seed) and the base seed are as above; the inner seeds are the same for every
 * candidate and part.  The plans of plo_orbit_plan_create_cse are served by plo_orbit_cost_many, plo_orbit_search and
 * plo_orbit_plan_destroy; plo_orbit_plan_create_q/_act refuse the measure (PLO_E_ARG: they carry no sub).
 * PLO_E_ARG: modulus 0, even, composite or 2^31 and more, sub outside 1 .. 65536.  PLO_E_CAPACITY: r, mn, mk or kn above 64, a
 * pair key above 51 bits, an op-count bound above 16 bits, a pair table above 65536 slots, an image that does not fit LDS with
 * one wave.  The images are sized from a sizing launch over a sample of candidates; a candidate that outgrows them makes the
 * launch repeat with larger ones (counted in plo_orbit_plan_info). */
int  plo_orbit_plan_create_cse(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int action,
                               uint32_t sub, uint64_t cse_seed0, plo_orbit_plan_t **plan);
int  plo_orbit_search_multi_cse(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int action, uint32_t sub, uint64_t cse_seed0,
                                uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_best_t *best, plo_stats_t *stats);
/* out[0] waves per workgroup, out[1] LDS bytes of a workgroup; of a PLO_ORBIT_CSE plan (0 otherwise): out[2..4] pair-table slots of
 * the images of Lj, Rg, hP, out[5] the largest entry bound of the three, out[6] launches repeated for a full table so far, out[7] 1
 * when a wave keeps a copy of the whole image between the sub runs, 0 when it keeps the entries and makes the rest again */
int  plo_orbit_plan_info(plo_orbit_plan_t *plan, uint32_t out[8]);

/* PLO_ORBIT_GROWTH (`-g`): the 2-norm growth factor of the transformed triple, the reference's G2 (src/growthfactor.cpp:117-125),
 * over Q only.  For candidate `seed` the transformed triple is the one the density measure counts: same stream, same actions,
 * same base seed.  With the rows of L and R and the columns of P scaled to integers as above (scale c_g for row g of the 3r
 * rows: the lcm of its denominators) let S_g = sum of acc^2 over the outputs of row g, the acc being the exact integers of the
 * sandwich.  Then
 *   n_g = sqrt(double(S_g)) / double(c_g),      cost = sum_{i=0}^{r-1} (n_i * n_{r+i}) * n_{2r+i},
 * every operation (two conversions, square root, division, two products, one addition per i) rounded to nearest on its own, no
 * fused multiply-add, the sum starting from 0.0 with one addition per i in increasing i.  nnz and nno are as above.
 * Order: the lexicographic minimum of (cost, nnz, nno, seed); the cost is compared as its 64-bit pattern, which for a
 * non-negative finite double is the numeric order.  The tool's winner improves on the input iff its (cost, nnz, nno) is smaller.
 * plo_orbit_plan_create_growth takes the limits and refusals of the Q plans above (m, k, n <= 16, r <= 4096, LDS with 24 r more
 * bytes per wave) and proves in addition E_g B_g^2 < 2^53 for every row (E_g the outputs of the row, B_g the bound on |acc| above:
 * the row's L1 norm times the action's factor bounds) and every scale below 2^53, so that double(S_g) and double(c_g) are exact:
 * PLO_E_UNSUPPORTED otherwise (the host computes S_g in 128 bits and rounds once).  PLO_E_ARG: PLO_ORBIT_ACT_HOUSEHOLDER (an
 * orthogonal action preserves G2: there is nothing to search) or an unknown action.  There is no modulus: a norm modulo p means
 * nothing.  The other create functions refuse the measure (PLO_E_ARG).  plo_orbit_plan_destroy and plo_orbit_plan_info serve these
 * plans; plo_orbit_cost_many and plo_orbit_search return PLO_E_ARG on them (their outputs cannot carry a double). */
#define PLO_ORBIT_GROWTH    3                          /* -g */
typedef struct { double cost; uint32_t nnz, nno; uint64_t seed; } plo_orbit_gbest_t;
int  plo_orbit_plan_create_growth(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, int action, plo_orbit_plan_t **plan);
/* cost[k], nnz_nno[2k], nnz_nno[2k+1] of candidate k (seeds[k], or seed0+k when seeds==NULL) */
int  plo_orbit_growth_many(plo_orbit_plan_t *plan, const uint64_t *seeds, uint64_t seed0, uint64_t n,
                           double *cost, uint32_t *nnz_nno /* 2 per seed */, plo_stats_t *stats);
int  plo_orbit_growth_search(plo_orbit_plan_t *plan, uint64_t seed0, uint64_t nseeds, plo_orbit_gbest_t *best, plo_stats_t *stats);
/* contiguous shards over `ndev` devices and the minimum under the order above, as plo_orbit_search_multi */
int  plo_orbit_growth_search_multi(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, int action,
                                   uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_gbest_t *best, plo_stats_t *stats);

/* ---- Row-dependency enumeration: the search of the reference's `dependency` (src/dependency.cpp:74-101, 158-165).  M (m x n) as
 * rational CSR, `ncoef` coefficients cnum[v]/cden[v] (the caller's FCoeffs, in order), `level` the largest number of rows in a
 * combination (1 .. PLO_DEP_MAX_LEVEL).  A combination is a top row i with coefficient 1 and rows i < q1 < q2 < ... with
 * coefficients of the list; every combination of 2 .. level rows is formed, and a hit is one that vanishes (PLO_DEP_ZERO) or
 * has exactly one non-zero entry (PLO_DEP_ONE: `col` is its column, `residue` its value).
 * modulus p (2 <= p < 2^31): values are residues in [0, p) and the hit list is final.  modulus 0 is Q: the device works
 * modulo the prime PLO_DEP_PRIME, and since reduction modulo it is a ring map, every combination that is a hit over Q is
 * reported; the list is a superset, `kind`, `col` and `residue` are those of the residues, and the caller recomputes each
 * reported combination over Q to drop the false ones and classify the others (bin/dependency does).
 * plo_dep_search enumerates the top rows [row0, row1) and returns the hits in the reference's depth-first order: by top row,
 * then lexicographic on (q1, v1), (q2, v2), ..., a prefix before its extensions.  *nhits is always the full count; when it
 * exceeds `cap` the call returns PLO_E_CAPACITY, hits[0 .. cap) holds hits in no particular order, and the caller repeats with
 * cap = *nhits.  More than 2^24 hits in one call are PLO_E_CAPACITY whatever `cap` is: take fewer top rows per call.
 * PLO_E_UNSUPPORTED: level above PLO_DEP_MAX_LEVEL, a modulus of 2^31 or more, a denominator (of M or of a coefficient) that is no
 * unit modulo the modulus (the prime, over Q).  PLO_E_CAPACITY: more than 4096 rows, 1024 columns or 255 coefficients, or a
 * level whose vectors do not fit LDS (512 x 128, level 6, 64 coefficients is within every limit).  One device per call. */
#define PLO_DEP_MAX_LEVEL 8
#define PLO_DEP_PRIME     2147483629u
#define PLO_DEP_ZERO      0
#define PLO_DEP_ONE       1
typedef struct {
    uint32_t size;                        /* rows in the combination, 2 .. level */
    uint32_t kind;                        /* PLO_DEP_ZERO or PLO_DEP_ONE */
    uint32_t col, residue;                /* PLO_DEP_ONE: the column of the non-zero entry and its value, in [1, p) */
    uint16_t rows[PLO_DEP_MAX_LEVEL];     /* rows[0] the top row; increasing; 0 beyond `size` */
    uint8_t  coef[PLO_DEP_MAX_LEVEL];     /* coef[k]: index of row k's coefficient in the list, k >= 1; coef[0] = 0 (the top row has 1) */
} plo_dep_hit_t;
typedef struct plo_dep_plan plo_dep_plan_t;
int  plo_dep_plan_create_q(const plo_qcsr_t *M, const int64_t *cnum, const int64_t *cden, uint32_t ncoef,
                           uint64_t modulus /* 0 = Q */, uint32_t level, plo_dep_plan_t **plan);
void plo_dep_plan_destroy(plo_dep_plan_t *plan);
int  plo_dep_search(plo_dep_plan_t *plan, uint32_t row0, uint32_t row1, plo_dep_hit_t *hits, uint64_t cap, uint64_t *nhits, plo_stats_t *stats);

/* ---- The Brent equations of a triple: what the reference's MMchecker (include/plinopt_library.inl:473-558) samples at one random
 * point, checked here one by one.  L (r x mk), R (r x kn), P (mn x r) as rational CSR; with x = a k + b, y = b' n + c, z = a' n + c',
 * equation e = (x kn + y) mn + z asks  sum_t L[t][x] R[t][y] P[z][t] = [a = a'][b = b'][c = c']  modulo q, 2 <= q < 2^31, prime or
 * not (a proof over Q takes a few primes: bin/MMchecker).  A pair is x kn + y; plo_brent_check covers the pairs
 * [pair0, pair1), that is the equations [pair0 mn, pair1 mn), in as many launches as the plan's pairs per launch ask for, and
 * reports how many of them are violated, the smallest violated e (~0 when none), the residue found there and the 0 or 1 expected;
 * stats->candidates is the number of equations checked.  The result is exact and does not depend on scheduling.
 * Refusals, each with its own text; the argument checks come before any device call, the missing plo_init (PLO_E_HIP) after them:
 * PLO_E_ARG for a null pointer, for L.n != m k, R.n != k n, P.m != m n, L.m != R.m or L.m != P.n, for q < 2 or q >= 2^31, for an
 * unsorted row (or any other defect of a CSR), for a denominator that is no unit modulo q, for an empty pair range or one beyond
 * mk kn.  PLO_E_CAPACITY: mk, kn or mn above 16384 (14-bit indices: 2^28 pairs at most), r above 2^20, or a matrix of 2^31 entries
 * or more; 32x32x32 of rank 15096 is well inside.
 * plo_brent_plan_info: out[0] sums per wave in LDS (the chunk: min(mn, 4096), or PLO_BRENT_CHUNK, a test knob), [1] chunks per pair,
 * [2] waves per workgroup, [3] pairs per launch, [4] LDS bytes per workgroup, [5] mk, [6] kn, [7] mn.  One device per call. */
typedef struct { uint64_t violated, first; uint32_t value, expected; } plo_brent_result_t;   /* first = ~0 when none */
typedef struct plo_brent_plan plo_brent_plan_t;
int  plo_brent_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P,
                             uint32_t m, uint32_t k, uint32_t n, uint32_t q, plo_brent_plan_t **plan);
int  plo_brent_check(plo_brent_plan_t *plan, uint64_t pair0, uint64_t pair1, plo_brent_result_t *res, plo_stats_t *stats);
int  plo_brent_plan_info(plo_brent_plan_t *plan, uint32_t out[8]);
void plo_brent_plan_destroy(plo_brent_plan_t *plan);

/* ---- The coefficient equations of a polynomial-multiplication triple: what the reference's PMchecker (src/PMchecker.cpp) samples
 * at one random pair of polynomials, checked here one by one (bin/PMchecker).  L (r x na), R (r x nb), P (nc x r)
 * as rational CSR claim to multiply a polynomial of degree na - 1 by one of degree nb - 1 into nc coefficients.  The pair
 * (i, j) = i nb + j has the sums S[z] = sum_t L[t][i] R[t][j] P[z][t] for z < nc, 0 for z >= nc, and the defect polynomial
 * sum_z S[z] X^z - X^(i+j).  Let Z = max(nc, na + nb - 1).
 *   flen = 0 (no polynomial): w = Z equations per pair, equation e = (i nb + j) w + c asks S[c] == [c == i + j]; a P with too few
 *     rows shows as violated equations at c = i + j >= nc.
 *   flen >= 2: f of degree d = flen - 1, its coefficients fnum[c] / fden[c] (fden NULL: all 1), the constant term first; w = d, and
 *     with rho[z] = X^z mod f equation e = (i nb + j) d + c asks sum_{z < nc} S[z] rho[z][c] == rho[i + j][c].  f need not be
 *     irreducible.  When d >= Z nothing folds: the sums are compared with [c == i + j] directly, over the width d.
 * Everything is modulo q, 2 <= q < 2^31, prime or not, taken as given (a proof over Q takes a few primes: bin/PMchecker).
 * plo_polymul_check covers the pairs [pair0, pair1), that is the equations [pair0 w, pair1 w), in as many launches as the plan's
 * pairs per launch ask for, and reports as plo_brent_check does: how many are violated, the smallest violated e (~0 when none),
 * the residue found there and the residue expected; stats->candidates is the number of equations checked.  The result is exact
 * and does not depend on scheduling.
 * Refusals, each with its own text; the argument checks come before any device call, the missing plo_init (PLO_E_HIP) after them:
 * PLO_E_ARG for a null pointer (fnum with flen > 0 included), for L.m != R.m or L.m != P.n, for q < 2 or q >= 2^31, for an unsorted
 * row (or any other defect of a CSR), for flen = 1 (a constant), a leading coefficient 0 or a non-positive fden, for a denominator
 * (of a matrix or of f) or a leading coefficient that is no unit modulo q, for an empty pair range or one beyond na nb.
 * PLO_E_CAPACITY: na or nb above 16384, Z above 32768, r above 2^20, a matrix of 2^31 entries or more, a fold (d < Z) with d above
 * PLO_POLYMUL_MAX_FOLD_DEGREE (the folded sums of a pair stay in LDS), or any d above 2^24.
 * plo_polymul_plan_info: out[0] sums per wave in LDS (the chunk: min(nc, 2048) with a fold, min(w, 4096) without, or
 * PLO_POLYMUL_CHUNK, a test knob; PLO_POLYMUL_PAIRS likewise lowers [3]), [1] chunks per pair, [2] waves per workgroup, [3] pairs
 * per launch, [4] LDS bytes per workgroup, [5] na nb, [6] w, [7] 1 when the fold runs.  One device per call. */
#define PLO_POLYMUL_MAX_FOLD_DEGREE 2048u
typedef struct plo_polymul_plan plo_polymul_plan_t;
int  plo_polymul_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P,
                               const int64_t *fnum, const int64_t *fden, uint32_t flen, uint32_t q, plo_polymul_plan_t **plan);
int  plo_polymul_check(plo_polymul_plan_t *plan, uint64_t pair0, uint64_t pair1, plo_brent_result_t *res, plo_stats_t *stats);
int  plo_polymul_plan_info(plo_polymul_plan_t *plan, uint32_t out[8]);
void plo_polymul_plan_destroy(plo_polymul_plan_t *plan);

/* ---- An in-place trilinear program of bin/trilplacer, certified: what the reference leaves to a Maple session (-DINPLACE_CHECKER,
 * include/plinopt_inplace.inl:940-1067), checked here equation by equation (bin/TPchecker).  L (r x na), R (r x nb),
 * P (nc0 x r) as rational CSR, and the program as flat records: family 0 a, 1 b, 2 c; PLO_TPROG_ADD x[dst] += v x[src] within one
 * family; PLO_TPROG_SCA x[dst] *= v; PLO_TPROG_AXPY (family 2) c[dst] += v a[src] b[src2] with v = +-1 and part 0, or with
 * PLO_TPROG_EXPANDED part 1 (low) or 2 (hig); v = num / den.  The state is a[na], b[nb], c[nc], nc = nc0, or nc0 + 1 with
 * PLO_TPROG_EXPANDED; on unit inputs the program ends in a' = A a, b' = B b, c' = C c + S(a, b).  With the width w = nc (2 nc when
 * expanded: the low components, then the hig ones), T[i][j][z] = sum_t L[t][i] R[t][j] P[z][t], or with PLO_TPROG_MATMUL the
 * matrix-multiplication tensor of the (m, k, n) with na = m k, nb = k n, nc0 = m n (n = floor(sqrt(nb nc0 / na)); the entries of
 * the matrices are then not read), the equations are numbered
 *   e = (i nb + j) w + z          S[i][j][z] == T[i][j][z]; expanded: S_low[z] == T[z] (0 at z = nc0), S_hig[z] == T[z - 1] (0 at 0)
 *   E0 + x na + i, E0 = na nb w   A[x][i] == [x == i];  then nb^2 numbers for B and nc^2 for C in the same way.
 * Everything is modulo q, 2 <= q < 2^31, prime or not, taken as given (a proof over Q takes a few primes: bin/TPchecker).
 * plo_tprog_check covers the bilinear equations of the pairs i nb + j in [pair0, pair1) and, when pair0 == 0, the three
 * restoration blocks, and reports in a plo_brent_result_t (reused: the contract is the same): how many are violated, the
 * smallest violated e (~0 when none), the residue found there and the residue expected; stats->candidates is the number of
 * equations checked.  The result is exact and does not depend on scheduling.
 * Refusals, each with its own text; the argument checks come before any device call, the missing plo_init (PLO_E_HIP) after them:
 * PLO_E_ARG for a null pointer, L.m != R.m or L.m != P.n, q < 2 or q >= 2^31, a defect of a CSR, unknown flags or both at once, a
 * shape that is no m k, k n, m n under PLO_TPROG_MATMUL, a record outside the list above (family, operation, part, an index out of
 * range, an ADD across families, den <= 0), a denominator that is no unit modulo q, an empty pair range or one beyond na nb.
 * PLO_E_CAPACITY: w, na or nb above PLO_TPROG_MAX_WORDS (a lane keeps that many state words in LDS), 2^24 records or more (the
 * target's included: one per entry of P, two when expanded), r above 2^20, or a table of operands (AXPYs + r rows of na or nb
 * words) of 2^28 words or more; all of them before anything of that size is allocated.
 * plo_tprog_plan_info: out[0] PLO_TPROG_MAX_WORDS, [1] LDS words per wave of the bilinear kernel (64 w), [2] waves per workgroup
 * there, [3] waves per launch (PLO_TPROG_WAVES, a test knob, lowers it), [4] records of the c stream, the appended target
 * included, [5] na nb, [6] w, [7] AXPY rows (program and target).  PLO_TPROG_SKIP=0 (a measuring knob) makes the bilinear kernel walk
 * the ADD and SCA records whose slot is still zero in every lane instead of passing them over.  One device per call. */
#define PLO_TPROG_ADD  0u
#define PLO_TPROG_SCA  1u
#define PLO_TPROG_AXPY 2u
#define PLO_TPROG_EXPANDED 1u
#define PLO_TPROG_MATMUL   2u
#define PLO_TPROG_MAX_WORDS 512u
typedef struct { uint8_t family, op, part, reserved; uint32_t dst, src, src2; int64_t num, den; } plo_tprog_rec_t;
typedef struct plo_tprog_plan plo_tprog_plan_t;
int  plo_tprog_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P,
                             const plo_tprog_rec_t *recs, uint64_t nrec, uint32_t flags, uint32_t q, plo_tprog_plan_t **plan);
int  plo_tprog_check(plo_tprog_plan_t *plan, uint64_t pair0, uint64_t pair1, plo_brent_result_t *res, plo_stats_t *stats);
int  plo_tprog_plan_info(plo_tprog_plan_t *plan, uint32_t out[8]);
void plo_tprog_plan_destroy(plo_tprog_plan_t *plan);

/* Pack / unpack the (cost, seed) word used by the grid reduction and by the
 * single 8-byte MIN all-reduce across ranks (the `#pragma omp critical`
 * best-so-far of include/plinopt_optimize.inl:1214-1237).  seed_off is the
 * candidate's offset from seed0 (< 2^32). */
uint64_t plo_pack_cost(uint32_t adds, uint32_t muls, int cost_mode, uint32_t seed_off);

#ifdef __cplusplus
}
#endif
#endif
