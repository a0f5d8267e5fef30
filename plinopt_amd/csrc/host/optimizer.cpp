// ===========================================================================
// bin/optimizer -- front-end keeping the reference CLI contract of
// src/optimizer.cpp:150-228: flags -D -K -G -A -F -E -N -P -M -q # -v # -O #,
// SLP on stdout only (:87), `#`-prefixed statistics on stderr (:89-98).
// New flags (the reference has none): --gpu N (0 = host only), --seed S, --orders first:count (a range of -N's row orders).
//
// With -q p the restart loop of CSEOptimiser (include/plinopt_optimize.inl:
// 1204-1238) runs on the GPU through the C-ABI of libplinopt_hip.so
// (plo_cse_search); the winning seed is then replayed on the host to produce
// the program text.  Over the rationals (no -q) the loop runs on the host, as
// in the reference; with --gpu-q the restart loop of -D runs on the GPU through
// the plan of plo_cse_plan_create_q, whose candidates are those of the host loop
// over Q seed by seed.  A failing GPU call is fatal: there is no silent fallback.
// ===========================================================================
#include "plo_host.hpp"
#include "plo_fast.hpp"
#include "plo_compact.hpp"
#include "plo_dl.hpp"

#include <chrono>
#include <memory>

using namespace plo;
using Ops = std::pair<size_t, size_t>;

namespace {

static int g_failures = 0;   // GPU calls that failed and replays that disagreed with the search: the exit status is non-zero when any happened

struct HipLib {
    void *h; bool ok;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error); PLO_SYM(shutdown, plo_shutdown);
    PLO_SYM(cse_search, plo_cse_search);
    PLO_SYM_OPT(cse_search_multi, plo_cse_search_multi);
    PLO_SYM(chain_create, plo_cse_chain_create); PLO_SYM(chain_search, plo_cse_chain_search); PLO_SYM(chain_destroy, plo_cse_chain_destroy);
    PLO_SYM(plan_create, plo_cse_plan_create); PLO_SYM(plan_destroy, plo_cse_plan_destroy);
    PLO_SYM(enum_search, plo_cse_enum_search_plan);
    PLO_SYM_OPT(plan_create_q, plo_cse_plan_create_q); PLO_SYM(search_plan, plo_cse_search_plan);   // --gpu-q
    PLO_SYM(chain_batch, plo_cse_chain_batch);
    PLO_SYM_OPT(kernel_search, plo_kernel_search);   // optional: -K with the decompositions on the device
    PLO_SYM_OPT(kernel_search_multi, plo_kernel_search_multi);   // optional: the same over N devices from this process
    PLO_SYM_OPT(kernel_search_orders, plo_kernel_search_orders);   // optional: -N over 10 to 12 rows, or over a range of orders
    explicit HipLib(void *lib = nullptr) : h(lib), ok(lib != nullptr) {}   // empty until load(): the methods load it only when they use the GPU
    bool load() { *this = HipLib(open_hip_lib()); if (!h) ++g_failures; return ok; }
};

// what the command line asks for
struct Options {
    bool direct = false, kernel = false, lu = false, ab = false, exhaustive = false, allkernels = false, kfi = false;   // -D -K -G -A -E -N -F
    size_t loops = 100; uint64_t seed0 = 0; int gpu = 1, verbose = 1;
    uint32_t q = 0;                // the modulus where the kernels can hold it (below 2^31); 0 (the rationals, a larger modulus): host loops
    int engine = 0;                // --engine: 0 auto (scalable engine over Z_p), 1 literal std::map replay, 2 scalable engine
    bool fork_shards = false;      // --fork-shards: --gpu N with one forked child per device instead of one thread per device
    bool host_decomp = false;      // --host-decomp: -K eliminates on the host and ships the images (plo_cse_chain_batch)
    uint64_t kernel_block = 1;     // --kernel-block: restarts per decomposition of -K (the reference draws one decomposition per restart, :1299-1340)
    bool recsub = false;           // --recsub: -E chooses the schedule as RecSub does (:950-959): additions, then ITS multiplication count (before ProgramGen)
    bool orders = false; uint64_t first = 0, count = 0;   // --orders first:count: -N over that range of order indices only (a walk of 12! split over processes and machines; a bounded run)
    bool gpu_q = false;            // --gpu-q: over the rationals, the restart loop of -D on the device (exact: plo_cse_plan_create_q)
    bool on_gpu() const { return q != 0 && gpu > 0; }
};
template <class F> constexpr bool device_field = std::is_same<F, ZpField>::value;   // the field of the kernels: every use of the library is compiled for it alone
struct Program { Ops ops; std::string text; };   // the best program so far, over the methods

template <class... T> std::string cat(const T &...t) { std::ostringstream os; (os << ... << t); return os.str(); }
// the red error line; counted: the exit status is non-zero
bool fail(const std::string &msg) { ++g_failures; std::cerr << "# \033[1;31mERROR: " << msg << "\033[0m" << std::endl; return false; }
bool zero_kernel() { std::clog << "# \033[1;36mZero dimensional kernel.\033[0m" << std::endl; return false; }   // :1343-1346
inline bool refusal(int rc) { return rc == PLO_E_UNSUPPORTED || rc == PLO_E_CAPACITY; }   // a limit of the kernels for this input, not an error

// The library loaded and plo_init(device) done, or false with the failure said and counted: "-G: cannot use the GPU: <reason>" for
// method "-G", without the reason when `why` is false; -D (no method) says the reason alone and leaves a library that does not load to load()'s own line.
bool bring_up(HipLib &L, const std::string &method, bool why = true, int device = 0) {
    const bool loaded = L.load();
    if (loaded && L.init(device) == PLO_OK) return true;
    if (method.empty()) return loaded ? fail(L.last_error()) : false;
    return fail(method + ": cannot use the GPU" + (why ? std::string(": ") + (L.last_error ? L.last_error() : "library missing") : ""));
}

// The running minimum of a search under (cmpOpCount in `mode`, then the smaller index).  The order is total over distinct indices, so
// the result does not depend on the order of the offers; offered increasing indices, the earlier one keeps ties.
struct Best {
    Ops ops; uint64_t index = 0; bool have = false; int mode;
    Best(int mode_ = 0) : mode(mode_) {}
    void offer(const Ops &o, uint64_t i) { if (!have || cmp_op_count(o, ops, mode) || (!cmp_op_count(ops, o, mode) && i < index)) { ops = o; index = i; have = true; } }
    void offer(const Best &b) { if (b.have) offer(b.ops, b.index); }
};
// body(k, mine) for k = 0 .. count-1 over the threads; each thread offers to its own minimum, and these are merged at the end
template <class Body> Best omp_min(uint64_t count, int chunk, int mode, Body body) {
    Best best(mode);
#pragma omp parallel
    {
        Best mine(mode);
#pragma omp for schedule(dynamic, chunk) nowait
        for (long long k = 0; k < (long long)count; ++k) body((uint64_t)k, mine);
#pragma omp critical
        best.offer(mine);
    }
    return best;
}

// Replay the winner of a search, hold it to what the search said, report it, adopt it when it beats the best program so far.
// What replay() returns: the text; key, what the search compared, and cost, what the program costs (the same but for -E --recsub);
// note, a line of the method for the log before "Found"; head and tail, what the method puts around the counts of the "Found" line.
struct Found { std::string text; Ops key, cost; std::string note, head, tail; };
inline Found found(std::string text, const Ops &cost, std::string tail) { Found r; r.text = std::move(text); r.key = r.cost = cost; r.tail = std::move(tail); return r; }
// what: "-G replay of seed 5"; none_better: the method's line when the program is not adopted, or null.  false: the replay disagrees (said, counted).
template <class Replay> bool replay_and_adopt(char method, const std::string &what, const Best &won, Replay replay, const char *none_better, int verbose, Program &best) {
    const Found r = replay();
    if (r.key != won.ops) return fail(cat(what, " gives ", r.key.first, '|', r.key.second, ", search said ", won.ops.first, '|', won.ops.second));
    if (verbose > 0 && !r.note.empty()) std::clog << r.note << std::endl;
    if (verbose > 0) std::clog << "# Found " << method << ": " << r.head << r.cost.first << '|' << r.cost.second << " instead of " << best.ops.first << '|' << best.ops.second << r.tail << std::endl;
    if (cmp_op_count(r.cost, best.ops)) best = Program{r.cost, r.text};
    else if (none_better) std::clog << "# \033[1;36m" << none_better << "\033[0m" << std::endl;
    return true;
}

template <class F> std::string replay_text(const F &f, const SparseMat<typename F::Elt> &lM, uint64_t seed, Ops &ops, int engine) {
    std::ostringstream os;
    input2temps(os, lM, 'i', 't');                          // plinopt_optimize.inl:1211
    if constexpr (std::is_same<F, ZpField>::value) {
        if (engine != 1) {
            auto t0 = std::chrono::steady_clock::now();
            SharedIndex S(f, lM);
            auto t1 = std::chrono::steady_clock::now();
            FastCand C(S, seed, &os, 'o', 't', 'r');
            ops = C.optimizer();
            auto t2 = std::chrono::steady_clock::now();
            if (engine == 2) std::clog << "# engine: index " << std::chrono::duration<double>(t1 - t0).count() << " s, candidate " << std::chrono::duration<double>(t2 - t1).count()
                << " s; decs " << C.st.decs << ", fresh pairs " << C.st.fresh_inst << " (" << C.st.fresh_distinct << " distinct), level rebuilds " << C.st.rebuilds
                << " (scanned " << C.st.rebuild_scan << "), select scanned " << C.st.select_scan << ", candidate rows " << C.st.cand_rows << ", affected rows " << C.st.aff_rows
                << ", top frequency " << C.st.max_level0 << ", nnz at ProgramGen " << C.st.live_nnz_end << ", columns " << C.st.cols_end << ", sum of tie-set sizes " << C.st.sum_T << " (max " << C.st.max_T << "), steps at level 2: " << C.st.steps_l2 << " (sum T " << C.st.sum_T_l2 << "), steps at level<=4: " << C.st.steps_le4 << ", largest fresh batch " << C.st.max_fresh << std::endl;
            if (engine == 2) std::clog << "# engine: scalable, " << C.steps() << " CSE steps, " << S.keys.size() << " initial triples, " << S.pairs0 << " pair instances" << std::endl;
            return os.str();
        }
    }
    Replay<F> R(f, lM, seed, os, 'o', 't', 'r');
    ops = R.optimizer();                                    // :1212
    return os.str();
}

// host restart loop (rationals, or --gpu 0): candidates seed0..seed0+loops-1, total order (cmpOpCount, seed)
template <class F> Best host_search(const F &f, const SparseMat<typename F::Elt> &lM, uint64_t seed0, size_t loops, int engine) {
    std::unique_ptr<SharedIndex> S;
    if constexpr (std::is_same<F, ZpField>::value) if (engine != 1) S.reset(new SharedIndex(f, lM));
    return omp_min(loops, 1, 0, [&](uint64_t k, Best &mine) {
        std::ostringstream sink; Ops ops;
        if (S) { FastCand C(*S, seed0 + k); ops = C.optimizer(); }
        else { Replay<F> R(f, lM, seed0 + k, sink, 'o', 't', 'r'); ops = R.optimizer(); }
        mine.offer(ops, seed0 + k);
    });
}

// The chained-candidate search on the device: seeds s0 .. s0+cnt-1 of two Optimizer calls, on A then on B, from one stream each.
// planned: the device took the pair; rc: what the entry that stopped the search answered (the caller words it, from L.last_error()).
struct Chained { bool planned = false; int rc = PLO_OK; Ops ops; uint64_t seed = 0; plo_stats_t st{}; };
template <class E> Chained chained_search(HipLib &L, const SparseMat<E> &A, const SparseMat<E> &B, uint32_t q, uint64_t s0, uint64_t cnt) {
    const Csr ca = csr(A), cb = csr(B); const plo_csr_t a = ca.view(), b = cb.view();
    Chained c; plo_chain_t *ch = nullptr;
    c.rc = L.chain_create(&a, &b, q, &ch);
    if (c.rc != PLO_OK) return c;
    c.planned = true;
    plo_best_t best{};
    c.rc = L.chain_search(ch, s0, cnt, PLO_COST_SUM_THEN_ADD, &best, &c.st);
    L.chain_destroy(ch);
    c.ops = {best.adds, best.muls}; c.seed = best.seed;
    return c;
}

// The restart loop of a method whose program is two chained Optimizer calls (-G: U then L; -A: CoB then Alt), text(seed, ops) being
// its program for one seed: on the device, or over the host's threads.  false: the method could not run (said).
template <class F, class Text> bool two_call_search(const Options &o, char method, const char *label, const SparseMat<typename F::Elt> &A, const SparseMat<typename F::Elt> &B, Text text, Best &best) {
    if constexpr (device_field<F>) if (o.on_gpu()) {
        HipLib L;
        if (!bring_up(L, cat('-', method))) return false;
        const Chained c = chained_search(L, A, B, o.q, o.seed0, o.loops);
        if (!c.planned) { std::clog << "# -" << method << " skipped: " << L.last_error() << std::endl; return false; }
        if (c.rc != PLO_OK) return fail(cat('-', method, " GPU search failed: ", L.last_error()));
        if (o.loops > 0) best.offer(c.ops, c.seed);
        if (o.verbose > 0) std::clog << "# GPU (" << label << "): " << c.st.candidates << " candidates, kernel " << c.st.kernel_ms << " ms" << std::endl;
    }
    if (!best.have) best = omp_min(o.loops, 1, 0, [&](uint64_t k, Best &mine) { Ops ops; (void)text(o.seed0 + k, ops); mine.offer(ops, o.seed0 + k); });
    return best.have;
}

// program text of the LU method for one seed (include/plinopt_optimize.inl:1058-1079)
template <class F> std::string lu_text(const F &f, const LUFactors<F> &lu, uint64_t seed, Ops &ops) {
    std::ostringstream os;
    for (size_t k = 0; k < lu.P.size(); ++k) os << 't' << k << ":=" << 'i' << lu.P[k] << ";\n";          // :1064
    CandRng rng(seed);
    Replay<F> RU(f, lu.U, rng, os, 'v', 't', 'r'); Ops uo = RU.optimizer();                                 // :1068
    Replay<F> RL(f, lu.L, rng, os, 'x', 'v', 'g'); Ops lo = RL.optimizer();                                 // :1072
    for (size_t i = 0; i < lu.Q.size(); ++i) os << 'o' << i << ":=" << 'x' << lu.Q[i] << ";\n";          // :1076
    ops = {uo.first + lo.first, uo.second + lo.second};
    return os.str();
}

// LUOptimiser :1021-1109.  Returns false when the method could not run (reported on stderr).
template <class F> bool lu_method(const F &f, const SparseMat<typename F::Elt> &lM, const Options &o, Program &prog) {
    const LUFactors<F> lu = sparse_lu(f, lM);
    auto text = [&](uint64_t seed, Ops &ops) { return lu_text(f, lu, seed, ops); };
    Best best;
    if (!two_call_search<F>(o, 'G', "LU", lu.U, lu.L, text, best)) return false;
    return replay_and_adopt('G', cat("-G replay of seed ", best.index), best, [&] {
        Ops ops; std::string t = text(best.index, ops);
        return found(t, ops, cat("\t[seed ", best.index, "] (rank ", lu.rank, ')'));
    }, nullptr, o.verbose, prog);                                                                           // :1103-1107
}

// program text of the alternative-factorization method for one seed (include/plinopt_optimize.inl:1142-1153)
template <class F> std::string ab_text(const F &f, const ABFactors<F> &ab, uint64_t seed, Ops &ops) {
    std::ostringstream os;
    input2temps(os, ab.CoB, 'i', 't');                                                                      // :1146
    CandRng rng(seed);
    Replay<F> RC(f, ab.CoB, rng, os, 'v', 't', 'r'); Ops bo = RC.optimizer();                               // :1150
    Replay<F> RA(f, ab.Alt, rng, os, 'o', 'v', 'g'); Ops ao = RA.optimizer();                               // :1153
    ops = {bo.first + ao.first, bo.second + ao.second};
    return os.str();
}

// ABOptimiser :1114-1186 for the inner dimension coldim(M).  Returns false when the method could not run.
template <class F> bool ab_method(const F &f, const SparseMat<typename F::Elt> &lM, const Options &o, Program &prog, size_t innerdim = 0) {
    if (lM.rowdim() < lM.coldim()) { std::clog << "# -A skipped: fewer rows than columns" << std::endl; return false; }
    const ABFactors<F> ab = ab_factorize(f, lM, 1 + (o.loops >> 3), o.seed0, innerdim);                     // :1129-1130
    auto text = [&](uint64_t seed, Ops &ops) { return ab_text(f, ab, seed, ops); };
    Best best;
    if (!two_call_search<F>(o, 'A', "A", ab.CoB, ab.Alt, text, best)) return false;
    return replay_and_adopt('A', cat("-A replay of seed ", best.index), best, [&] {
        Ops ops; std::string t = text(best.index, ops);
        Found r = found(t, ops, cat("\t[seed ", best.index, ']'));
        r.head = cat('(', ab.Alt.rowdim(), 'x', ab.Alt.coldim(), 'x', ab.CoB.coldim(), ' ', ab.score[0], '/', ab.score[2], ")\t");
        return r;
    }, nullptr, o.verbose, prog);                                                                           // :1180-1184
}

// KernelOptimiser :1288-1353 with this build's decomposition rule.  The restarts are spent as blocks of --kernel-block
// seeds: block d uses the decomposition drawn from its first seed, and every seed of the block is one run of the two
// Optimizer calls on it (the reference draws a new decomposition for every restart; with a per-restart elimination on
// the host the GPU would idle).
// restarts s0 .. s0+cnt-1 of the two Optimizer calls on one decomposition, on this thread
template <class F> Best kernel_block_serial(const F &f, const KernelDecomp<F> &kd, uint64_t s0, uint64_t cnt) {
    Best best;
    for (uint64_t k = 0; k < cnt; ++k) { Ops ops; (void)kernel_text(f, kd, s0 + k, ops); best.offer(ops, s0 + k); }
    return best;
}
// the same on the device (chained-candidate kernel); throws what the device answers when it does not take or finish the block
template <class F> Best kernel_block_gpu(HipLib &L, const KernelDecomp<F> &kd, uint64_t s0, uint64_t cnt, uint32_t q, double &kms, uint64_t &ncand) {
    Best best;
    if constexpr (device_field<F>) {
        const Chained c = chained_search(L, kd.Free, kd.Dep, q, s0, cnt);
        if (!c.planned) throw std::runtime_error(std::string("chain plan: ") + L.last_error());
        if (c.rc != PLO_OK) throw std::runtime_error(std::string("GPU search failed: ") + L.last_error());
        best.offer(c.ops, c.seed); kms += c.st.kernel_ms; ncand += c.st.candidates;
    } else { (void)L; (void)kd; (void)s0; (void)cnt; (void)q; (void)kms; (void)ncand; }
    return best;
}
// restarts of many decompositions in ONE launch (plo_cse_chain_batch): decomposition j takes the seeds s0 + j*per .. + per - 1
template <class F> Best kernel_batch_gpu(HipLib &L, const std::vector<KernelDecomp<F>> &kds, uint64_t s0, uint32_t per, uint32_t q, double &kms, uint64_t &ncand) {
    Best best;
    if constexpr (device_field<F>) {
        std::vector<Csr> mats; std::vector<plo_csr_t> A, B;
        mats.reserve(2 * kds.size());                                                                      // the views point into them
        for (auto &kd : kds) { mats.push_back(csr(kd.Free)); A.push_back(mats.back().view()); mats.push_back(csr(kd.Dep)); B.push_back(mats.back().view()); }
        plo_best_t b{}; plo_stats_t st{};
        if (L.chain_batch((uint32_t)kds.size(), A.data(), B.data(), q, s0, per, PLO_COST_SUM_THEN_ADD, nullptr, nullptr, &b, &st) != PLO_OK)
            throw std::runtime_error(std::string("batched chain search: ") + L.last_error());
        best.offer({b.adds, b.muls}, b.seed); kms += st.kernel_ms; ncand += st.candidates;
    } else { (void)L; (void)kds; (void)s0; (void)per; (void)q; (void)kms; (void)ncand; }
    return best;
}

// what the --gpu N shards of a method found (run()), or that they did not run: refused, the device's limits with its words in `why`;
// failed, an error (said, counted).  where and reduce: how the shards ran and how their minimum was taken, for the note on the log.
struct Sharded { bool failed = false, refused = false; Best best; uint64_t ncand = 0; double kms = 0; std::string where, reduce, why; };

// Returns false when the method could not run.  sharded: -K searched by the --gpu N shards, only the replay is left.
template <class F> bool kernel_method(const F &f, const SparseMat<typename F::Elt> &lM, const Options &o, const Sharded &sharded, Program &prog) {
    const uint64_t seed0 = o.seed0, loops = o.loops, block = o.kernel_block;
    const uint64_t nblocks = (loops + block - 1) / block, full = loops / block, BATCH = 4096;   // full blocks go to the GPU in batches of one launch each
    Best best = sharded.best; bool on_device = best.have, use_gpu = false; double kms = sharded.kms; uint64_t ncand = sharded.ncand, d = best.have ? nblocks : 0;
    HipLib L;
    if constexpr (device_field<F>) if (o.on_gpu() && !best.have) {
        if (!bring_up(L, "-K")) return false;
        use_gpu = true;
    }
    if (best.have && o.verbose > 0) std::clog << "# " << o.gpu << " shards (" << sharded.where << sharded.reduce << "): -K" << std::endl;
    // All of it on the device (plo_kernel_search: the wave of a restart eliminates, builds both images and runs both
    // Optimizer calls): matrices of at most 128 rows and 64 columns with at most 64 dependent rows.  --host-decomp keeps the decompositions on the host (round-1 path).
    if constexpr (device_field<F>) if (use_gpu && L.kernel_search && !o.host_decomp && lM.rowdim() <= 128 && lM.coldim() <= 64) {
        KernelDecomp<F> kd0;
        if (!kernel_decomp(f, lM, seed0, kd0)) return zero_kernel();                                       // (the rank does not depend on the order)
        const Csr M = csr(lM); const plo_csr_t A = M.view();
        plo_best_t b{}; plo_stats_t st{};
        const int rc = L.kernel_search(&A, o.q, seed0, loops, (uint32_t)std::min<uint64_t>(block, 0xFFFFFFFFull), PLO_COST_SUM_THEN_ADD, nullptr, nullptr, nullptr, &b, &st);
        if (rc == PLO_OK) { best.offer({b.adds, b.muls}, b.seed); kms = st.kernel_ms; ncand = st.candidates; d = nblocks; on_device = true; }
        else if (!refusal(rc)) return fail(cat("-K on the GPU: ", L.last_error()));
    }
    if (use_gpu) for (; d < full; ) {
        const uint64_t nb = std::min<uint64_t>(BATCH, full - d), s0 = seed0 + d * block;
        std::vector<KernelDecomp<F>> kds(nb); bool zero = false;
#pragma omp parallel for schedule(dynamic, 8)
        for (long long j = 0; j < (long long)nb; ++j) if (!kernel_decomp(f, lM, s0 + (uint64_t)j * block, kds[(size_t)j])) {
#pragma omp atomic write
            zero = true;
        }
        if (zero) return zero_kernel();
        try { best.offer(kernel_batch_gpu(L, kds, s0, (uint32_t)block, o.q, kms, ncand)); }                // increasing seeds: the earlier batch keeps ties
        catch (const std::exception &e) { return fail(cat("-K on the GPU: ", e.what())); }
        d += nb;
    }
    if (!use_gpu && d < nblocks) {                                     // host path: the blocks are shared out between the threads
        bool zero = false;
        best = omp_min(nblocks, 1, 0, [&](uint64_t dd, Best &mine) {
            const uint64_t s0 = seed0 + dd * block;
            KernelDecomp<F> kd;
            if (kernel_decomp(f, lM, s0, kd)) mine.offer(kernel_block_serial(f, kd, s0, std::min<uint64_t>(block, loops - dd * block)));
            else {
#pragma omp atomic write
                zero = true;
            }
        });
        if (zero) return zero_kernel();
        d = nblocks;
    }
    for (; d < nblocks; ++d) {                                         // GPU: the last partial block
        const uint64_t s0 = seed0 + d * block;
        KernelDecomp<F> kd;
        if (!kernel_decomp(f, lM, s0, kd)) return zero_kernel();
        try { best.offer(kernel_block_gpu(L, kd, s0, std::min<uint64_t>(block, loops - d * block), o.q, kms, ncand)); }
        catch (const std::exception &e) { return fail(cat("-K on the GPU: ", e.what())); }
    }
    if (!best.have) return false;
    const uint64_t seed = best.index;
    KernelDecomp<F> kd;
    if (!kernel_decomp(f, lM, seed0 + ((seed - seed0) / block) * block, kd)) return false;                 // the decomposition of the winner's block
    return replay_and_adopt('K', cat("-K replay of seed ", seed), best, [&] {
        Ops ops; std::string t = kernel_text(f, kd, seed, ops);
        Found r = found(t, ops, cat("\t[seed ", seed, "] (rank ", kd.rank, '+', kd.notindep, ", ", kd.dep.size(), " dependent rows)"));
        if (use_gpu || on_device) r.note = cat("# GPU (K): ", ncand, " candidates on ", nblocks, " decompositions, kernel ", kms, " ms", on_device ? " (decompositions on the device)" : " (decompositions on the host)");
        return r;
    }, nullptr, o.verbose, prog);                                                                          // :1347-1351
}

inline uint64_t factorial(size_t m) { uint64_t r = 1; for (size_t k = 2; k <= m; ++k) r *= k; return r; }
// the pi-th permutation of 0..m-1 in lexicographic order: the order std::next_permutation reaches after pi steps from the
// identity, by the digits of pi in the factorial base (kthpermutation, include/plinopt_library.inl:289-304)
inline std::vector<size_t> kth_order(size_t m, uint64_t pi) {
    std::vector<size_t> left(m), ord;
    for (size_t i = 0; i < m; ++i) left[i] = i;
    for (size_t i = 0; i < m; ++i) {
        const uint64_t fc = factorial(m - 1 - i); const size_t d = (size_t)(pi / fc); pi %= fc;
        ord.push_back(left[d]); left.erase(left.begin() + (long)d);
    }
    return ord;
}

// AllKernelOpt (-N, :1357-1418) by order INDEX, for 10 to 12 rows (up to 12! = 479,001,600 orders, as the reference allows) and
// for a range of orders (--orders): candidate c = (pi - first) * sub + j is restart j of order pi, the pi-th permutation of the
// rows; its decomposition draws NotIndep from the stream of seed0 + pi, its two Optimizer calls run from seed0 + pi * sub + j.
// No order is searched twice as below, but none is left out either: 12! signatures do not fit a map.  The minimum is under
// (cmpOpCount, candidate index).  On the device the whole walk is plo_kernel_search_orders; on the host (--gpu 0, the
// rationals, a modulus above 2^31, a refusal of the device) the same definition over the threads.
template <class F> bool allorders_method(const F &f, const SparseMat<typename F::Elt> &lM, const Options &o, Program &prog) {
    const size_t m = lM.rowdim();
    const uint64_t seed0 = o.seed0, mfact = factorial(m), first = o.orders ? o.first : 0, count = o.orders ? o.count : mfact;
    const uint64_t sub = std::min<uint64_t>(std::max<uint64_t>(1, o.loops / mfact), 0xFFFFFFFFull);
    Best best; bool on_gpu = false; double kms = 0;
    if constexpr (device_field<F>) if (o.on_gpu()) {
        HipLib L;
        if (!bring_up(L, "-N")) return false;
        if (!L.kernel_search_orders) return fail("-N: libplinopt_hip.so lacks plo_kernel_search_orders");
        const Csr M = csr(lM); const plo_csr_t A = M.view();
        plo_best_t b{}; plo_stats_t st{};
        const int rc = L.kernel_search_orders(&A, o.q, seed0, first, count, (uint32_t)sub, PLO_COST_SUM_THEN_ADD, nullptr, nullptr, nullptr, &b, &st);
        if (rc == PLO_OK) { best.offer({b.adds, b.muls}, b.seed); on_gpu = true; kms = st.kernel_ms; }
        else if (refusal(rc)) std::clog << "# -N on the GPU refused (" << L.last_error() << "): host walk" << std::endl;
        else return fail(cat("-N on the GPU: ", L.last_error()));
    }
    if (!best.have) {
        bool zero = false;
        best = omp_min(count, 16, 0, [&](uint64_t k, Best &mine) {
            const uint64_t pi = first + k;
            KernelDecomp<F> kd; CandRng rng(seed0 + pi);
            if (!kernel_decomp_order(f, lM, kth_order(m, pi), rng, kd)) {
#pragma omp atomic write
                zero = true;
                return;
            }
            for (uint64_t j = 0; j < sub; ++j) { Ops ops; (void)kernel_text(f, kd, seed0 + pi * sub + j, ops); mine.offer(ops, seed0 + pi * sub + j); }   // the seeds grow with the candidate index
        });
        if (zero) return zero_kernel();
    }
    if (!best.have) return false;
    const uint64_t seed = best.index, bpi = (seed - seed0) / sub;
    KernelDecomp<F> kd; CandRng rng(seed0 + bpi);
    if (!kernel_decomp_order(f, lM, kth_order(m, bpi), rng, kd)) return false;
    return replay_and_adopt('N', "-N replay", best, [&] {
        Ops ops; std::string t = kernel_text(f, kd, seed, ops);
        return found(t, ops, cat("\t[order ", bpi, ", seed ", seed, "] (", count, " of ", mfact, " row orders from ", first, ", ", sub, " restarts each, ",
                                 on_gpu ? cat("GPU kernel ", kms, " ms)") : std::string("host)")));
    }, "No kernel permutation has less additions.", o.verbose, prog);                                       // :1409-1413
}

// AllKernelOpt (-N, :1357-1418): every order of the rows.  Up to 9 rows: m! eliminations on the host; orders that give the same
// decomposition (same computed rows, same combinations) are searched once; the restarts are shared out between the distinct
// decompositions.  10 to 12 rows, and --orders: allorders_method above.  13 rows and more: nothing, as in the reference (:1463).
template <class F> bool allkernels_method(const F &f, const SparseMat<typename F::Elt> &lM, const Options &o, Program &prog) {
    const size_t m = lM.rowdim(); const uint64_t seed0 = o.seed0;
    if (m > 12) { std::clog << "# -N skipped: " << m << " rows (the row orders are walked up to 12!, as in the reference)" << std::endl; return false; }
    if (m > 9 || o.orders) return allorders_method(f, lM, o, prog);
    std::vector<size_t> ord(m);
    for (size_t i = 0; i < m; ++i) ord[i] = i;
    std::map<std::vector<size_t>, std::pair<std::vector<size_t>, uint64_t>> distinct;     // signature -> (order, permutation index)
    uint64_t pi = 0;
    do {
        KernelDecomp<F> kd; CandRng rng(seed0 + pi);
        if (!kernel_decomp_order(f, lM, ord, rng, kd)) return zero_kernel();
        std::vector<size_t> sig(kd.dep); sig.push_back(m + kd.notindep);
        for (auto &r : kd.Dep.rows) for (auto &e : r) sig.push_back(e.first);             // the basis rows used
        distinct.emplace(sig, std::make_pair(ord, pi));
        ++pi;
    } while (std::next_permutation(ord.begin(), ord.end()));
    bool use_gpu = false; HipLib L;
    if constexpr (device_field<F>) if (o.on_gpu()) {
        if (!bring_up(L, "-N", false)) return false;
        use_gpu = true;
    }
    const uint64_t per = std::max<uint64_t>(1, o.loops / distinct.size());
    Best best; double kms = 0; uint64_t ncand = 0;
    std::vector<const std::pair<std::vector<size_t>, uint64_t> *> order;                  // decomposition k takes the seeds seed0 + k*per .. + per - 1
    for (auto &kv : distinct) order.push_back(&kv.second);
    auto decomp = [&](size_t k, KernelDecomp<F> &kd) { CandRng rng(seed0 + order[k]->second); kernel_decomp_order(f, lM, order[k]->first, rng, kd); };
    if (use_gpu) {                                                   // all distinct decompositions in one launch
        std::vector<KernelDecomp<F>> kds(order.size());
        for (size_t k = 0; k < order.size(); ++k) decomp(k, kds[k]);
        try { best = kernel_batch_gpu(L, kds, seed0, (uint32_t)per, o.q, kms, ncand); }
        catch (const std::exception &e) { std::clog << "# -N skipped: " << e.what() << std::endl; return false; }
    } else best = omp_min(order.size(), 1, 0, [&](uint64_t k, Best &mine) {
        KernelDecomp<F> kd; decomp((size_t)k, kd);
        mine.offer(kernel_block_serial(f, kd, seed0 + k * per, per));
    });
    if (!best.have) return false;
    const uint64_t seed = best.index; const size_t w = (size_t)((seed - seed0) / per);   // the winner's decomposition
    return replay_and_adopt('N', "-N replay", best, [&] {
        KernelDecomp<F> kd; decomp(w, kd);
        Ops ops; std::string t = kernel_text(f, kd, seed, ops);
        return found(t, ops, cat("\t[order ", order[w]->second, ", seed ", seed, "] (", pi, " row orders, ", distinct.size(), " distinct decompositions, ", per, " restarts each",
                                 use_gpu ? cat(", GPU kernel ", kms, " ms") : std::string(", host "), ')'));
    }, "No kernel permutation has less additions.", o.verbose, prog);                                       // :1409-1413
}

// program text of one schedule of the exhaustive CSE tree
template <class F> std::string schedule_text(const F &f, const SparseMat<typename F::Elt> &lM, uint64_t index, Ops &ops, uint64_t &prod, size_t *recsub_muls = nullptr) {
    std::ostringstream os;
    input2temps(os, lM, 'i', 't');                                                                         // :1265
    Replay<F> R(f, lM, 0, os, 'o', 't', 'r'); R.set_schedule(index);
    ops = R.optimizer(); prod = R.eprod;
    if (recsub_muls) *recsub_muls = R.recsub_muls;
    return os.str();
}

// AllCSEOpt / RecOptimizer / RecSub (-E, include/plinopt_optimize.inl:889-1013, :1252-1281): the best of ALL greedy CSE
// schedules (every pair of frequency > 1 is a child, order additions then multiplications :958-959).  The tree is walked
// by schedule index (include/plinopt_hip.h): ranges 0..N-1 with N growing to the largest radix product seen; exhaustive
// when N reaches it, otherwise stopped at `budget` schedules (the reference has no bound and no termination on anything
// but toy inputs).  Returns false when the method could not run.
template <class F> bool exhaustive_method(const F &f, const SparseMat<typename F::Elt> &lM, uint64_t budget, const Options &o, Program &prog) {
    // `best` holds the SELECTION key: (adds, muls of the program), or with --recsub (adds, RecSub's multiplication count)
    Best best(1); uint64_t maxprod = 1, done = 0; bool on_gpu = false; double kms = 0;
    HipLib L; plo_plan_t *plan = nullptr;
    if constexpr (device_field<F>) if (o.on_gpu()) {
        if (!bring_up(L, "-E")) return false;
        const Csr M = csr(lM); const plo_csr_t A = M.view();
        if (L.plan_create(&A, o.q, &plan) != PLO_OK) { std::clog << "# -E skipped: " << L.last_error() << std::endl; return false; }
        on_gpu = true;
    }
    uint64_t target = 1;
    while (done < target) {
        const uint64_t cnt = target - done;
        Best range(1); uint64_t rprod = 1;
        if (on_gpu) {
            plo_best_t b{}; plo_stats_t st{}; uint64_t mp = 0;
            if (L.enum_search(plan, done, cnt, o.recsub ? PLO_COST_RECSUB : PLO_COST_ADD_THEN_MUL, &b, &mp, &st) != PLO_OK) {
                std::clog << "# -E skipped: " << L.last_error() << std::endl; L.plan_destroy(plan); return false;
            }
            range.offer({b.adds, b.muls}, b.seed); rprod = mp; kms += st.kernel_ms;
        } else range = omp_min(cnt, 8, 1, [&](uint64_t k, Best &mine) {
            Ops ops; uint64_t pr = 1; size_t rm = 0; (void)schedule_text(f, lM, done + k, ops, pr, &rm);
            if (o.recsub) ops.second = rm;
            mine.offer(ops, done + k);
#pragma omp critical
            rprod = std::max(rprod, pr);
        });
        best.offer(range);                                                           // increasing indices: the earlier range keeps ties
        maxprod = std::max(maxprod, rprod);
        done = target;
        target = std::min<uint64_t>(std::max<uint64_t>(maxprod, done), budget);      // grow to the largest tree size seen so far
    }
    if (on_gpu) L.plan_destroy(plan);
    if (!best.have) return false;
    const bool complete = maxprod <= done;
    if (!replay_and_adopt('E', cat("-E replay of schedule ", best.index), best, [&] {
            Found r; uint64_t pr = 1; size_t rm = 0;
            r.text = schedule_text(f, lM, best.index, r.cost, pr, &rm);              // what the printed program costs
            r.key = r.cost;
            if (o.recsub) { r.key.second = rm; r.note = cat("# RecSub accounting: ", best.ops.first, '|', best.ops.second, " (additions | multiplications before ProgramGen); program ", r.cost.first, '|', r.cost.second); }
            r.tail = cat("\t[schedule ", best.index, "] (", done, complete ? std::string(" schedules: the whole tree") : cat(" schedules of a tree of at least ", maxprod),
                         on_gpu ? cat(", GPU kernel ", kms, " ms") : std::string(", host"), ')');
            return r;
        }, complete ? "No greedy CSE schedule has less additions." : nullptr, o.verbose, prog)) return false;   // :1270-1278
    if (!complete) std::clog << "# \033[1;36m-E stopped after " << done << " schedules of a tree of at least " << maxprod << ": the result is the best of those only.\033[0m" << std::endl;
    return true;
}

// --gpu N in ONE process: the multi-device entry of the library for method 'D' (plo_cse_search_multi) or 'K' (plo_kernel_search_multi)
template <class F> Sharded multi_device_search(const SparseMat<typename F::Elt> &lM, const Options &o, char method) {
    Sharded s; const bool K = method == 'K'; const std::string failed = K ? "-K shard failed: " : "shard failed: ";
    HipLib L;
    if (!L.load() || !(K ? (bool)L.kernel_search_multi : (bool)L.cse_search_multi)) {
        s.failed = true; fail(failed + "libplinopt_hip.so " + (L.cse_search ? K ? "lacks plo_kernel_search_multi" : "lacks plo_cse_search_multi" : "cannot be loaded"));
        return s;
    }
    std::vector<int> devs((size_t)o.gpu); for (int r = 0; r < o.gpu; ++r) devs[(size_t)r] = shard_device(r);
    const Csr M = csr(lM); const plo_csr_t A = M.view();
    plo_best_t b{}; plo_stats_t st{};
    const int rc = K ? L.kernel_search_multi(&A, o.q, o.seed0, o.loops, 1u, PLO_COST_SUM_THEN_ADD, o.gpu, devs.data(), &b, &st)
                     : L.cse_search_multi(&A, o.q, o.seed0, o.loops, PLO_COST_SUM_THEN_ADD, o.gpu, devs.data(), &b, &st);
    if (refusal(rc)) { s.refused = true; s.why = L.last_error(); }
    else if (rc != PLO_OK) { s.failed = true; fail(failed + L.last_error()); }
    else {
        if (b.seed != ~0ull) s.best.offer({b.adds, b.muls}, b.seed);
        s.ncand = st.candidates; s.kms = st.kernel_ms; s.where = "one GPU and one host thread each, one process";
        s.reduce = st.reduce ? cat(", minimum by RCCL MIN all-reduce in ", st.reduce_seconds * 1e3, " ms") : std::string(", minimum on the host");
    }
    return s;
}

// --gpu N with one forked child per device, each on the single-device entry of method 'D' (plo_cse_search) or 'K' (plo_kernel_search),
// or each on the host engine (-D, the test knob); the minimum under (cmpOpCount, seed) is taken here
template <class F> Sharded forked_search(const F &f, const SparseMat<typename F::Elt> &lM, const Options &o, char method, bool host_engine) {
    Sharded s; const bool K = method == 'K';
    const Csr M = csr(lM);
    auto shard = [&](int, int device, uint64_t s0, uint64_t cnt) {
        ShardOut out{};
        if (cnt == 0) { out.ok = 1; out.a = out.b = 0xFFFFFFFFu; return out; }
        if (host_engine) {
#ifdef _OPENMP
            omp_set_num_threads(1);                                                    // a forked child keeps to its own thread
#endif
            const Best b = host_search(f, lM, s0, (size_t)cnt, o.engine);
            if (b.have) { out.ok = 1; out.a = (uint32_t)b.ops.first; out.b = (uint32_t)b.ops.second; out.seed = b.index; out.candidates = cnt; }
            return out;
        }
        HipLib L;
        if (!L.load() || (K && !L.kernel_search) || L.init(device) != PLO_OK) { snprintf(out.msg, sizeof out.msg, "device %d: %s", device, L.last_error ? L.last_error() : "library missing"); return out; }
        const plo_csr_t A = M.view();
        plo_best_t b{}; plo_stats_t st{};
        const int rc = K ? L.kernel_search(&A, o.q, s0, cnt, 1u, PLO_COST_SUM_THEN_ADD, nullptr, nullptr, nullptr, &b, &st)
                         : L.cse_search(&A, o.q, s0, cnt, PLO_COST_SUM_THEN_ADD, &b, &st);
        if (rc != PLO_OK) { out.rc = rc; snprintf(out.msg, sizeof out.msg, "device %d: %s", device, L.last_error()); return out; }
        out.ok = 1; out.a = b.adds; out.b = b.muls; out.seed = b.seed; out.candidates = st.candidates; out.kernel_ms = st.kernel_ms;
        L.shutdown();
        return out;
    };
    std::vector<ShardOut> outs;
    if (!forked_shards(o.gpu, o.seed0, o.loops, shard, outs)) {
        s.refused = true;
        for (auto &out : outs) if (!out.ok && !refusal(out.rc)) s.refused = false;
        if (s.refused) s.why = outs[0].msg;
        else { s.failed = true; for (auto &out : outs) if (!out.ok) fail((K ? "-K shard failed: " : "shard failed: ") + std::string(out.msg)); }
        return s;
    }
    for (auto &out : outs) {
        s.ncand += out.candidates; s.kms = std::max(s.kms, out.kernel_ms);
        if (out.a != 0xFFFFFFFFu || out.b != 0xFFFFFFFFu) s.best.offer({out.a, out.b}, out.seed);   // (an empty shard)
    }
    s.where = host_engine ? "host engine" : "one forked process and one GPU each";
    return s;
}

template <class F> int run(const F &f, const QMat &MQ, Options o)
{
    auto t0 = std::chrono::steady_clock::now();
    std::clog << std::string(40, '#') << std::endl;
    const Ops opsinit = naive_ops(QField(), MQ);            // src/optimizer.cpp:77: computed over Q
    auto lM = rebind(MQ, f);
    Program prog{opsinit, ""};

    // the eliminations of -K, -G, -A and -N run on the host with dense or map-based rows: not attempted on inputs like
    // 32x32x32_15096_L (15096 x 1024), where only the direct method is meant to run (BASELINE config 5 uses -D)
    const double elim_cost = (double)lM.rowdim() * (double)lM.coldim() * (double)std::min(lM.rowdim(), lM.coldim());
    if (elim_cost > 2e9 && (o.ab || o.kernel || o.lu || o.allkernels)) {
        std::clog << "# -K/-G/-A/-N skipped: host elimination of a " << lM.rowdim() << 'x' << lM.coldim() << " matrix is not attempted (use -D)" << std::endl;
        o.ab = o.kernel = o.lu = o.allkernels = false;
    }
    // --gpu N, N >= 2: the seed range of -D and of -K in N contiguous shards, the minimum under (cmpOpCount, seed).
    // Default: ONE process, one host thread and one device per shard inside the library (plo_cse_search_multi,
    // plo_kernel_search_multi), the minimum by RCCL MIN all-reduces -- the seed space sharded over the GPUs of the node as
    // north_star names it; this process forks nothing.  --fork-shards (and the host-engine test knob) keep one forked child per
    // device instead: every fork happens here, BEFORE anything in this process touches the HIP runtime (a runtime does not
    // survive fork), and the library's multi-device entries are not used at all then.
    Sharded dshards, kshards;
    const bool shard_host_engine = getenv("PLO_SHARD_ENGINE") && std::string(getenv("PLO_SHARD_ENGINE")) == "host";   // test knob: every shard on the host engine
    const bool use_forks = o.fork_shards || shard_host_engine;
    if constexpr (device_field<F>) if (o.direct && o.q != 0 && o.gpu >= 2 && o.loops > 0) {
        dshards = use_forks ? forked_search(f, lM, o, 'D', shard_host_engine) : multi_device_search<F>(lM, o, 'D');
        if (dshards.failed) return 2;
        // refused: as one device does, a limit of the kernels for this input: the restarts run on the host, said aloud
        if (dshards.refused) std::clog << "# -D on the GPUs refused (" << dshards.why << "): host search" << std::endl;
        else if (o.verbose > 0) std::clog << "# " << o.gpu << " shards (" << dshards.where << "): " << dshards.ncand << " candidates, slowest kernel " << dshards.kms << " ms" << dshards.reduce << std::endl;
    }
    // the same for -K (decompositions on the device, one per restart): N shards of the restart range
    if constexpr (device_field<F>) if (o.kernel && !o.kfi && o.q != 0 && o.gpu >= 2 && o.loops > 0 && !o.host_decomp && o.kernel_block == 1 && lM.rowdim() <= 128 && lM.coldim() <= 64 && !shard_host_engine) {
        KernelDecomp<F> kd0;
        if (kernel_decomp(f, lM, o.seed0, kd0)) {                                     // (a zero dimensional kernel is reported by kernel_method)
            kshards = use_forks ? forked_search(f, lM, o, 'K', false) : multi_device_search<F>(lM, o, 'K');
            if (kshards.failed) return 2;
            // a plan the device refuses (state beyond LDS, table bounds) is what the single-device path answers with host
            // decompositions + the batched chain kernel: leave the method to kernel_method then
            if (kshards.refused && o.verbose > 0) std::clog << "# -K: the device refused the one-wave restart (" << kshards.why << "): host decompositions + batched chain kernel on one device" << std::endl;
        }
    }
    if (o.ab) {                                                                       // :1436-1440 (inner dimension = column count)
        // every inner dimension from the column count to the row count - 1 (:1437-1439); a square matrix has the identity factorization only
        const size_t id0 = lM.coldim(), id1 = std::max<size_t>(lM.rowdim(), id0 + 1);
        for (size_t id = id0; id < id1; ++id) {
            try { ab_method(f, lM, o, prog, id); }
            catch (const std::exception &e) { std::clog << "# -A skipped: " << e.what() << std::endl; }
        }
    }
    if constexpr (std::is_same<F, QField>::value)
        if (o.gpu_q && (o.kernel || o.lu || o.ab || o.exhaustive || o.allkernels)) std::clog << "# --gpu-q: -K, -G, -A, -E and -N stay on the host over Q" << std::endl;
    if (o.direct) {
        Best best = dshards.best; bool on_gpu = best.have;
        if constexpr (std::is_same<F, QField>::value) if (o.gpu_q && o.loops > 0) {
            // the same restarts on the device: its candidate `seed` is Optimizer() over Q of that seed, so the winner below is the host loop's
            HipLib L;
            if (!bring_up(L, "")) return 2;
            const QCsr M = qcsr(MQ); const plo_qcsr_t A = M.view();
            plo_plan_t *plan = nullptr; plo_best_t b{}; plo_stats_t st{};
            int rc = PLO_E_UNSUPPORTED; std::string why;
            if (!L.plan_create_q) why = "this build of the library has no search over Q";
            else if (M.wide) why = "a coefficient does not fit 64-bit numerators and denominators";
            else if ((rc = L.plan_create_q(&A, 0u, &plan)) == PLO_OK) { rc = L.search_plan(plan, o.seed0, o.loops, PLO_COST_SUM_THEN_ADD, &b, &st); if (rc != PLO_OK) why = L.last_error(); L.plan_destroy(plan); }
            else why = L.last_error();
            if (refusal(rc)) std::clog << "# -D on the GPU refused (" << why << "): host search" << std::endl;
            else if (rc != PLO_OK) { fail(cat("GPU search failed (", rc, "): ", why)); return 2; }
            else {
                on_gpu = true; best.offer({b.adds, b.muls}, b.seed);
                if (o.verbose > 0)
                    std::clog << "# GPU (over Q): " << st.candidates << " candidates, kernel " << st.kernel_ms << " ms, "
                              << (st.kernel_ms > 0 ? st.candidates / (st.kernel_ms * 1e-3) : 0.0) << " candidates/s" << std::endl;
            }
            L.shutdown();
        }
        if constexpr (device_field<F>) if (o.on_gpu() && !best.have && !dshards.refused) {
            on_gpu = true;
            HipLib L;
            if (!bring_up(L, "")) return 2;
            const Csr M = csr(lM); const plo_csr_t A = M.view();
            plo_best_t b{}; plo_stats_t st{};
            const int rc = L.cse_search(&A, o.q, o.seed0, o.loops, PLO_COST_SUM_THEN_ADD, &b, &st);
            if (refusal(rc)) {
                // a limit of the device kernels for this input (e.g. a column whose non +-1 entries span more than 64 rows in ProgramGen): said
                // aloud, and the same restarts run on the host (as -K and bin/sparsifier do when the device refuses)
                std::clog << "# -D on the GPU refused (" << L.last_error() << "): host search" << std::endl;
                on_gpu = false;
            } else if (rc != PLO_OK) { fail(cat("GPU search failed (", rc, "): ", L.last_error())); return 2; }
            else {
                if (o.loops > 0) best.offer({b.adds, b.muls}, b.seed);
                if (o.verbose > 0)
                    std::clog << "# GPU: " << st.candidates << " candidates, kernel " << st.kernel_ms << " ms, "
                              << (st.kernel_ms > 0 ? st.candidates / (st.kernel_ms * 1e-3) : 0.0) << " candidates/s" << std::endl;
            }
            L.shutdown();
        }
        if (!on_gpu) {
            auto ts = std::chrono::steady_clock::now();
            best = host_search(f, lM, o.seed0, o.loops, o.engine);
            double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
            int nthr = 1;
#ifdef _OPENMP
            nthr = omp_get_max_threads();
#endif
            if (o.verbose > 0) std::clog << "# host search: " << o.loops << " candidates in " << dt << " s on " << nthr << " threads (index build included)" << std::endl;
        }
        auto adopt = [&] {
            return !best.have || replay_and_adopt('D', cat("replay of seed ", best.index), best, [&] {
                Ops ops; std::string t = replay_text(f, lM, best.index, ops, o.engine);
                return found(t, ops, cat("\t[seed ", best.index, ']'));
            }, nullptr, o.verbose, prog);                                             // :1241-1245
        };
        if (!adopt()) {
            if (!(o.gpu_q && on_gpu)) return 3;
            best = host_search(f, lM, o.seed0, o.loops, o.engine);                    // --gpu-q: the replay over Q disagrees with the device (said above, counted): the host's own search
            if (!adopt()) return 3;
        }
    }
    if (o.kernel && !o.kfi) {                                                         // :1450-1462
        try { kernel_method(f, lM, o, kshards, prog); }
        catch (const std::exception &e) { std::clog << "# -K skipped: " << e.what() << std::endl; }
    }
    if (o.kernel && o.kfi) {
        // -F: the kernel method with the identity added to the goals (nullspacedecomp :637-685): the inputs become rows that the
        // decomposition may put in its basis, so a dependent output can be written over inputs as well as over other outputs.
        // The program of [M ; I] is searched as any other; its identity goals are then no outputs: the text is renamed
        // (goals 'q'), the real outputs are copied (`o_j := q_j`, :680-681) and the rewriting engine of bin/compacter removes
        // what only the identity goals needed (the reference does this with OpOnVars / RemoveVars, :657-663).
        try {
            auto Mx = lM; const size_t m = lM.rowdim();
            for (size_t i = 0; i < lM.coldim(); ++i) { Mx.rows.emplace_back(); Mx.rows.back().emplace_back(i, f.one()); }
            Program kprog{{~(size_t)0 >> 1, 0}, ""};
            if (kernel_method(f, Mx, o, Sharded{}, kprog) && !kprog.text.empty()) {
                std::istringstream in(kprog.text);
                std::vector<compact::Line> Pg = compact::parse(in);
                auto ren = [](std::string &t) { if (t.size() > 1 && t[0] == 'o' && isdigit((unsigned char)t[1])) t[0] = 'q'; };
                for (auto &l : Pg) { ren(l.lhs); for (auto &t : l.rhs) ren(t); }
                for (size_t j = 0; j < m; ++j) Pg.push_back(compact::Line{"o" + std::to_string(j), {"q" + std::to_string(j)}});
                compact::compact_program(Pg, false, compact::letter_outputs('o'));
                std::ostringstream os; compact::print(os, Pg);
                SlpEval<F> ev(f); std::istringstream chk(os.str());
                const Ops cops = ev.run(chk);
                if (!same_matrix(f, ev.matrix('o', lM.rowdim(), lM.coldim()), lM)) throw std::runtime_error("the cleaned program does not compute the matrix");
                if (o.verbose > 0) std::clog << "# Found K with identity goals (-F): " << cops.first << '|' << cops.second << " after cleaning (" << kprog.ops.first << '|' << kprog.ops.second
                                             << " with the identity goals) instead of " << prog.ops.first << '|' << prog.ops.second << std::endl;
                if (cmp_op_count(cops, prog.ops)) prog = Program{cops, os.str()};
            }
        } catch (const std::exception &e) { std::clog << "# -K -F skipped: " << e.what() << std::endl; }
    }
    if (o.lu) {
        try { lu_method(f, lM, o, prog); }
        catch (const std::exception &e) { std::clog << "# -G skipped: " << e.what() << std::endl; }
    }
    if (o.allkernels) {                                                               // :1463-1465
        try { allkernels_method(f, lM, o, prog); }
        catch (const std::exception &e) { std::clog << "# -N skipped: " << e.what() << std::endl; }
    }
    if (o.exhaustive) {                                                               // :1469-1471
        try { exhaustive_method(f, lM, std::max<uint64_t>(o.loops, 1ull << 22), o, prog); }
        catch (const std::exception &e) { std::clog << "# -E skipped: " << e.what() << std::endl; }
    }

    if (cmp_op_count(opsinit, prog.ops) || opsinit == prog.ops) {                     // :1473-1485
        std::ostringstream os;
        input2temps(os, lM, 'i', 't');
        Replay<F> R(f, lM, 0, os, 'o', 't', 'r');
        prog.ops = R.direct(); prog.text = os.str();
    }
    std::cout << prog.text << std::flush;                                             // src/optimizer.cpp:87
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (prog.ops.first != 0 || prog.ops.second != 0) {
        std::clog << std::string(40, '#') << std::endl;
        std::clog << "# \033[1;32m" << prog.ops.first << "\tadditions\tinstead of " << opsinit.first << "\033[0m \t" << secs << "s" << std::endl;
        std::clog << "# \033[1;32m" << prog.ops.second << "\tmultiplications\tinstead of " << opsinit.second << "\033[0m" << std::endl;
        std::clog << std::string(40, '#') << std::endl;
    }
    if (g_failures) { std::cerr << "# \033[1;31mERROR: " << g_failures << " GPU call(s) or replay check(s) failed: the program above comes from the methods that did run\033[0m" << std::endl; return 2; }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    Options o;
    bool printMaple = false, printPretty = false, replay_only = false;
    uint64_t q = 0; std::string filename, only;
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        if (a == "-h") {
            std::clog << "Usage: " << argv[0] << " [-h|-M|-P|-K|-D|-G|-E|-N|-A|-q #|-O #|--gpu #|--gpu-q|--seed #|--orders #:#] [stdin|matrixfile.sms]\n"
                      << "  -D/-K/-G: direct/kernel/LU methods (default is all)\n"
                      << "  -F: kernel method with the identity added to its goals (inputs may join the row basis)\n"
                      << "  -q #: search modulo (default is Rationals, on the host unless --gpu-q)\n"
                      << "  --gpu-q: without -q, run the restart loop of -D on the MI355X, exactly as over Q (same winner and program as --gpu 0); matrices of\n"
                      << "      at most 64 distinct values that fit the LDS-resident kernels, others are said and searched on the host; -K/-G/-A/-E/-N stay on the host\n"
                      << "  -O #: randomized search with that many loops (default " << o.loops << " loops)\n"
                      << "  --gpu #: 1 = run the restart loop on the MI355X (default with -q), 0 = host only, N >= 2 = the seeds of -D in N shards, one GPU each\n"
                      << "  --seed #: first candidate seed (default 0)\n"
                      << "  -A: also try the alternative factorizations M = Alt.CoB, every inner dimension from the column count to the row count - 1\n"
                      << "  -E: also walk the exhaustive tree of greedy CSE schedules (bounded by max(-O, 2^22) schedules; every DISTINCT triple of\n"
                      << "      frequency > 1 is a child, once -- the reference tries it once per row holding it); best by additions then multiplications\n"
                      << "      of the printed program, or with --recsub by RecSub's own counts (multiplications before ProgramGen)\n"
                      << "  -N: also walk the kernel method over EVERY order of the rows, up to 12 rows (12! orders).  Up to 9 rows equal decompositions are searched once and share\n"
                      << "      the -O restarts; 10 to 12 rows walk all m! orders by index with max(1, -O / m!) restarts each, on the GPU with -q below 2^31 and --gpu >= 1\n"
                      << "  --orders first:count: with -N, only the row orders of index first .. first+count-1 (lexicographic order of the permutations): splits a\n"
                      << "      walk over processes and machines; results of ranges compose (seeds depend on the order index only)\n"
                      << "  --only D|K|G|A|E|N: run exactly that method\n"
                      << "  --host-decomp: -K makes the nullspace decompositions on the host (default: on the device when the matrix has at most 64 rows and columns)\n"
                      << "  --kernel-block #: restarts per nullspace decomposition of -K (default 1: one decomposition per restart, as the reference)\n"
                      << "  -M/-P: also print the matrix (Maple / pretty) on the log stream\n";
            exit(-1);
        } else if (a == "-M") printMaple = true;
        else if (a == "-P") printPretty = true;
        else if (a == "-G") o.lu = true;
        else if (a == "-A") o.ab = true;
        else if (a == "-D") o.direct = true;
        else if (a == "-K") o.kernel = true;
        else if (a == "-F") o.kfi = true;
        else if (a == "-E") o.exhaustive = true;
        else if (a == "-N") o.allkernels = true;
        else if (a == "-q" && i + 1 < argc) q = strtoull(argv[++i], nullptr, 10);
        else if (a == "-v" && i + 1 < argc) o.verbose = atoi(argv[++i]);
        else if (a == "-O" && i + 1 < argc) o.loops = strtoull(argv[++i], nullptr, 10);
        else if (a == "--gpu" && i + 1 < argc) o.gpu = atoi(argv[++i]);
        else if (a == "--seed" && i + 1 < argc) o.seed0 = strtoull(argv[++i], nullptr, 10);
        else if (a == "--engine" && i + 1 < argc) { std::string e(argv[++i]); o.engine = e == "literal" ? 1 : e == "fast" ? 2 : 0; }
        else if (a == "--gpu-q") o.gpu_q = true;
        else if (a == "--replay") replay_only = true;    // print the program of candidate --seed, no search
        else if (a == "--host-decomp") o.host_decomp = true;
        else if (a == "--fork-shards") o.fork_shards = true;
        else if (a == "--kernel-block" && i + 1 < argc) o.kernel_block = std::max<uint64_t>(1, strtoull(argv[++i], nullptr, 10));
        else if (a == "--recsub") o.recsub = true;
        else if (a == "--orders" && i + 1 < argc) {
            const std::string v(argv[++i]); const size_t colon = v.find(':');
            const bool ok = colon != std::string::npos && colon > 0 && colon + 1 < v.size() && v.find_first_not_of("0123456789:") == std::string::npos && v.find(':', colon + 1) == std::string::npos
                            && colon <= 18 && v.size() - colon - 1 <= 18;
            if (!ok) { std::cerr << "# ERROR: --orders takes first:count, two natural numbers" << std::endl; return -1; }
            o.orders = true; o.first = strtoull(v.c_str(), nullptr, 10); o.count = strtoull(v.c_str() + colon + 1, nullptr, 10);
        }
        else if (a == "--only" && i + 1 < argc) { only = argv[++i]; }   // run exactly one method (D, K, G, A, E or N): for tests and timing
        else filename = a;
    }
    cap_omp_threads();
    if (!only.empty()) { o.direct = only == "D"; o.lu = only == "G"; o.ab = only == "A"; o.kernel = only == "K"; o.exhaustive = only == "E"; o.allkernels = only == "N"; }
    else if (!o.kernel && !o.direct && !o.lu) o.lu = o.direct = o.kernel = true;             // src/optimizer.cpp:208-211
    try {
        QMat MQ;
        if (filename.empty()) MQ = read_sms(std::cin);
        else { std::ifstream in(filename); if (!in) return -1; MQ = read_sms(in); }
        if (o.orders) {
            const size_t m = MQ.rowdim();
            if (!o.allkernels) { std::cerr << "# ERROR: --orders is a range of the row orders of -N (--only N)" << std::endl; return -1; }
            if (m < 2 || m > 12) { std::cerr << "# ERROR: --orders: the row orders are walked for 2 to 12 rows, the matrix has " << m << std::endl; return -1; }
            if (o.count == 0 || o.first >= factorial(m) || o.count > factorial(m) - o.first) {
                std::cerr << "# ERROR: --orders " << o.first << ':' << o.count << " is no range of the " << factorial(m) << " orders of " << m << " rows" << std::endl; return -1;
            }
        }
        if (printPretty || printMaple) {                                             // src/optimizer.cpp:65-73 (LinBox's writers are not in the tree: plain dense forms)
            auto dense = [&](const char *open, const char *rowopen, const char *sep, const char *rowclose, const char *rowsep, const char *close) {
                std::clog << open;
                for (size_t i = 0; i < MQ.rowdim(); ++i) {
                    std::clog << (i ? rowsep : "") << rowopen; size_t k = 0;
                    for (size_t j = 0; j < MQ.coldim(); ++j) {
                        if (j) std::clog << sep;
                        if (k < MQ.rows[i].size() && MQ.rows[i][k].first == j) { std::clog << MQ.rows[i][k].second; ++k; } else std::clog << 0;
                    }
                    std::clog << rowclose;
                }
                std::clog << close << ';' << std::endl << std::string(40, '#') << std::endl;
            };
            if (printPretty) dense("", "[", " ", "]", "\n", "");
            if (printMaple) dense("M:=Matrix([", "[", ",", "]", ",", "])");
        }
        if (replay_only) {
            Ops ops;
            if (q >= (1ull << 31)) { Zp64Field f(q); std::cout << replay_text(f, rebind(MQ, f), o.seed0, ops, o.engine); }
            else if (q) { ZpField f((uint32_t)q); std::cout << replay_text(f, rebind(MQ, f), o.seed0, ops, o.engine); }
            else { QField f; std::cout << replay_text(f, rebind(MQ, f), o.seed0, ops, o.engine); }
            std::clog << "# " << ops.first << "\tadditions\n# " << ops.second << "\tmultiplications" << std::endl;
            return 0;
        }
        if (q != 0 && o.gpu_q) { std::clog << "# --gpu-q is for the search over the rationals: ignored with -q" << std::endl; o.gpu_q = false; }
        if (q != 0) {
            if (q < 3 || q >= (1ull << 62)) { std::cerr << "# ERROR: modulus must be an odd prime below 2^62 in this build" << std::endl; return -1; }
            if (q < (1ull << 31)) { o.q = (uint32_t)q; return run(ZpField(o.q), MQ, o); }
            // the kernels keep 31-bit residues: larger moduli run the host loops (the reference's field is Modular<Integer>, src/optimizer.cpp:131)
            std::clog << "# modulus above 2^31: host loops (the GPU kernels hold 31-bit residues)" << std::endl;
            o.gpu = 0;
            return run(Zp64Field(q), MQ, o);
        }
        o.gpu = 0;
        return run(QField(), MQ, o);
    } catch (const std::exception &e) {
        fail(e.what());
        return -1;
    }
}
