// ===========================================================================
// plo_capi.hip -- host side of libplinopt_hip.so: the C-ABI declared in
// include/plinopt_hip.h, for all nine kernel families (CSE wave, CSE HBM, chained
// CSE, kernel method, change of basis, trilplacer and inplacer, orbit, dependency)
// and the checkers, each under its banner comment below; what they share comes
// first.  The in-place program check has its host code in plo_capi_tprog.hip,
// the plans of the CSE search over Q theirs in plo_capi_cseq.hip, both included
// at the end.
// There is NO CPU fallback in this file: without a HIP device every compute
// entry point fails with PLO_E_HIP.
// ===========================================================================
#include "plo_cse_wave.hip"
#include "plo_cse_batch.hip"
#include "plo_kmethod.hip"
#include "plo_kmethod_batch.hip"
#include "plo_cse_big.hip"
#include "plo_cob.hip"
#include "plo_tril.hip"
#include "plo_lin.hip"
#include "plo_orbit.hip"
#include "plo_orbit_cse.hip"
#include "plo_orbit_growth.hip"
#include "plo_dep.hip"
#include "plo_brent.hip"
#include "plo_polymul.hip"
#include "plo_tprog.hip"
#include "../../include/plinopt_hip.h"

#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#ifndef PLO_BIG_LOGTRIG_MAX
// log records between two merges of the deferred updates, at most (the partitions' capacity -- what a merge can sum in its LDS table --
// is the other bound: 5.6e6 on config 5).  Round 4: 8 M instead of 4 M: 7 merges per candidate instead of 8 (one forced by the log
// instead of two), 789 -> 811 candidates/s on one box (profiles/r04_ab_config5.txt); 11 MB more workspace per candidate.
#define PLO_BIG_LOGTRIG_MAX (8ull << 20)
#endif

namespace {

thread_local std::string g_err;
// The device context of the calling thread: the process-wide one set by plo_init (one process per GPU is the model of the
// tools and of bench.py), or a thread's own inside plo_cse_search_multi (one host thread per device).
struct DevCtx {
    int device = -1; hipStream_t stream = nullptr; int cus = 0; size_t lds_max = 0;
    // scratch of the change-of-basis enumeration, kept between calls (bin/sparsifier -c 4 makes dozens of 256-candidate enumerations:
    // four allocations, four frees and two event objects per call cost more than the kernel)
    uint32_t *cob_buf = nullptr; size_t cob_words = 0; hipEvent_t cob_e0 = nullptr, cob_e1 = nullptr;
};
DevCtx g_ctx0;
thread_local DevCtx *t_ctx = nullptr;
inline DevCtx &cur_ctx() { return t_ctx ? *t_ctx : g_ctx0; }
#define g_device (cur_ctx().device)
#define g_stream (cur_ctx().stream)
#define g_cus (cur_ctx().cus)
#define g_lds_max (cur_ctx().lds_max)

int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(PLO_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

uint32_t inv_mod(uint32_t a, uint32_t p) {
    int64_t t = 0, nt = 1, r = p, nr = a % p;
    while (nr) { int64_t q = r / nr, x = t - q * nt; t = nt; nt = x; x = r - q * nr; r = nr; nr = x; }
    if (t < 0) t += p;
    return (uint32_t)t;
}
uint32_t ceil_log2(uint32_t x) { uint32_t l = 0; while ((1u << l) < x) ++l; return l; }
uint32_t round_up(uint32_t x, uint32_t a) { return (x + a - 1) / a * a; }
double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// The statistics and the clock of one call: the caller's plo_stats_t or a local one, cleared, and the start time.  done(rc) sets
// `seconds` and hands rc on; an entry that returns without it leaves `seconds` at zero.
struct CallScope {
    plo_stats_t local{}, *st;
    std::chrono::steady_clock::time_point t0;
    explicit CallScope(plo_stats_t *stats) : st(stats ? stats : &local) { *st = plo_stats_t{}; t0 = std::chrono::steady_clock::now(); }
    int done(int rc) { st->seconds = seconds_since(t0); return rc; }
};
// A call before plo_init.  The CSE family refuses in few words, the families after it in more, and the entries that the tools call
// without plo_init (CSE plan creation, change of basis) take device 0 themselves.  The tools print these texts.
enum NoInit { NOINIT_CSE, NOINIT_PLAN, NOINIT_DEVICE0 };
int require_device(NoInit how) {
    if (g_device >= 0) return PLO_OK;
    if (how == NOINIT_DEVICE0) return plo_init(0);
    return fail(PLO_E_HIP, how == NOINIT_CSE ? "plo_init not called" : "plo_init was not called (or found no HIP device)");
}

// An integer environment knob: unset, or the number strtol reads from it (a flag counts as soon as it is set, whatever it holds)
std::optional<long> env_knob(const char *name) { const char *e = getenv(name); if (!e) return std::nullopt; return strtol(e, nullptr, 10); }

// Temporary device memory of one call: freed when its scope ends, whichever return is taken
template <class T> struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }      // (move-only: this also deletes the copies)
    ~DevBuf() { if (p) (void)hipFree(p); }
    operator T *() const { return p; }
};
// hipFree of those of a plan's device buffers that exist
template <class... P> void dev_free(P *...p) { for (void *q : {(void *)p...}) if (q) (void)hipFree(q); }

// One launch on g_stream between two events: launch() enqueues the kernel, *ms gets its time
template <class Launch> int timed_between(hipEvent_t e0, hipEvent_t e1, float *ms, Launch launch) {
    HIPCHK(hipEventRecord(e0, g_stream));
    launch();
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, g_stream)); HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
    return PLO_OK;
}
// the same with an event pair of its own
template <class Launch> int timed(float *ms, Launch launch) {
    struct Events { hipEvent_t e0 = nullptr, e1 = nullptr; ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); } } ev;
    HIPCHK(hipEventCreate(&ev.e0)); HIPCHK(hipEventCreate(&ev.e1));
    return timed_between(ev.e0, ev.e1, ms, launch);
}

// One timed launch and its statistics: time and count add up over the launches of a call, the shape is the latest launch's.
// shape == nullptr: time and count only (the sizing launch of the kernel method).
struct LaunchShape { uint64_t grid; uint32_t lds_bytes, waves_per_wg; uint64_t algo_bytes; };
template <class Launch> int timed_launch(plo_stats_t *st, const LaunchShape *shape, Launch launch)
{
    float ms = 0;
    const int rc = timed(&ms, launch);
    if (rc != PLO_OK) return rc;
    if (!st) return PLO_OK;
    st->kernel_ms += ms; st->launches += 1;
    if (shape) { st->grid = (uint32_t)shape->grid; st->lds_bytes = shape->lds_bytes; st->waves_per_wg = shape->waves_per_wg; st->algo_bytes = shape->algo_bytes; }
    return PLO_OK;
}
// the same for a search kernel whose plan holds the shape (trilplacer, inplacer, orbiter, dependency): its candidates are counted too
template <class Plan, class Launch> int timed_launch(Plan *pl, uint64_t grid, uint64_t ncand, plo_stats_t *st, Launch launch)
{
    const LaunchShape shape{grid, pl->lds_bytes, pl->waves_per_wg, pl->algo_bytes};
    const int rc = timed_launch(st, &shape, launch);
    if (rc == PLO_OK && st) st->candidates += ncand;
    return rc;
}

// One launch of a kernel that reports through an error word: the word cleared, the timed launch, the word read back.
// Negative: a refusal of the host side; otherwise the device's word (0 = none).  The job's err field points at d_err already.
template <class Launch> int checked_launch(uint32_t *d_err, plo_stats_t *st, const LaunchShape &shape, Launch launch) {
    HIPCHK(hipMemsetAsync(d_err, 0, sizeof(uint32_t), g_stream));
    const int trc = timed_launch(st, &shape, launch);
    if (trc != PLO_OK) return trc;
    uint32_t err = 0;
    HIPCHK(hipMemcpy(&err, d_err, sizeof err, hipMemcpyDeviceToHost));
    return (int)err;
}
// The dynamic-LDS limit of kernel `fn` raised to `lds` bytes; *per_cu: the workgroups of W waves a CU then holds by the runtime's count, 1 at least
int occupancy_for(const void *fn, uint32_t W, uint32_t lds, uint32_t *per_cu) {
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int nb = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, (int)(W * 64), lds));
    *per_cu = (uint32_t)std::max(nb, 1);
    return PLO_OK;
}
// Workgroups of a launch over `ncand` candidates, W to a workgroup: no more than the device holds at once (`resident`), never none
uint64_t grid_for(uint64_t ncand, uint32_t W, uint64_t resident) { return std::max<uint64_t>(1, std::min<uint64_t>(resident, (ncand + W - 1) / W)); }

// Waves (= candidates) per workgroup, 4, 2 or 1, for a kernel that needs lds(w) bytes with w waves: the first count that fits
// `limit`, or with most_per_cu the count that puts most waves on a CU (32 at most; the larger workgroup on a tie).
// 0 when not even one wave fits; *lds_out gets the bytes, *per_cu (optional) the waves on a CU.
template <class Lds> uint32_t pick_waves(Lds lds, bool most_per_cu, uint64_t limit, uint32_t *lds_out, uint32_t *per_cu = nullptr)
{
    uint32_t W = 0, bestw = 0;
    for (uint32_t w : {4u, 2u, 1u}) {
        const uint64_t l = lds(w);
        if (l > limit) continue;
        const uint32_t waves = std::min<uint32_t>(32u, (uint32_t)(limit / l) * w);
        if (W && (!most_per_cu || waves <= bestw)) continue;
        bestw = waves; W = w; *lds_out = (uint32_t)l;
    }
    if (per_cu) *per_cu = bestw;
    return W;
}

// (adds, muls) of a cost key with two fields of `bits` bits: 16 in the 32-bit key of the wave kernels (plo::cost_key32), 20 in the
// HBM kernel's.  PLO_COST_SUM_THEN_ADD holds (sum, adds); PLO_COST_ADD_THEN_MUL and PLO_COST_RECSUB (adds, muls).
// A sum-only key (PLO_COST_SUM) holds the sum above `bits` zero bits and no split: false, with the sum in *adds and 0 in *muls.
// That is what plo_cse_chain_batch and plo_kernel_search report; the plan and chain searches ask the device for the winner's
// split instead.
bool decode_key(uint64_t key, int cost_mode, uint32_t bits, uint32_t *adds, uint32_t *muls)
{
    const uint32_t hi = (uint32_t)(key >> bits), lo = (uint32_t)(key & ((1ull << bits) - 1ull));
    if (cost_mode == PLO_COST_SUM_THEN_ADD) { *adds = lo; *muls = hi - lo; }
    else if (cost_mode == PLO_COST_SUM) { *adds = hi; *muls = 0; return false; }
    else { *adds = hi; *muls = lo; }
    return true;
}

// The minimum under (cost key, seed) over `count` candidates from `first`, in launches of at most `chunk` candidates:
// run(first seed, count) launches with *d_best as the job's best word and leaves (key << off_bits | seed offset) there.
// 2^24 candidates and 24 bits for the HBM kernel, 2^32-1 and 32 bits otherwise.  All ones when count == 0.
template <class Run> int chunked_min(unsigned long long *d_best, uint64_t first, uint64_t count, uint64_t chunk, uint32_t off_bits, uint64_t *bkey, uint64_t *bseed, Run run)
{
    *bkey = *bseed = ~0ull;
    for (uint64_t done = 0; done < count;) {
        const uint64_t cnt = std::min<uint64_t>(chunk, count - done);
        HIPCHK(hipMemsetAsync(d_best, 0xFF, sizeof(unsigned long long), g_stream));
        const int rc = run(first + done, cnt);
        if (rc != PLO_OK) return rc;
        unsigned long long w = 0;
        HIPCHK(hipMemcpy(&w, d_best, sizeof w, hipMemcpyDeviceToHost));
        const uint64_t key = w >> off_bits, sd = first + done + (w & ((1ull << off_bits) - 1ull));
        if (key < *bkey || (key == *bkey && sd < *bseed)) { *bkey = key; *bseed = sd; }
        done += cnt;
    }
    return PLO_OK;
}

// Body of the cost_many entries of the CSE family: adds and muls of n > 0 candidates, and one optional array of 64-bit words
// that goes in (`seeds`) or comes out (`prods`).  run(d_adds, d_muls, d_words) fills in the job and launches it.
template <class Run> int cse_cost_many_run(uint64_t n, const uint64_t *seeds, uint32_t *adds, uint32_t *muls, uint64_t *prods, plo_stats_t *st, Run run)
{
    DevBuf<uint32_t> d_adds, d_muls; DevBuf<uint64_t> d_words;
    HIPCHK(hipMalloc((void **)&d_adds.p, n * sizeof(uint32_t)));
    HIPCHK(hipMalloc((void **)&d_muls.p, n * sizeof(uint32_t)));
    if (seeds || prods) HIPCHK(hipMalloc((void **)&d_words.p, n * sizeof(uint64_t)));
    if (seeds) HIPCHK(hipMemcpy(d_words, seeds, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    int rc = run(d_adds.p, d_muls.p, d_words.p);
    if (rc == PLO_OK) {
        hipError_t e1 = hipMemcpy(adds, d_adds, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
        hipError_t e2 = hipMemcpy(muls, d_muls, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
        hipError_t e3 = prods ? hipMemcpy(prods, d_words, n * sizeof(uint64_t), hipMemcpyDeviceToHost) : hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc = fail(PLO_E_HIP, "copy back failed");
    }
    st->candidates = n;
    return rc;
}

} // namespace

// what is wrong with a caller's CSR matrix over Z_p, or nullptr (the checks every entry point makes before the host
// images are built from it: the builders index by column and invert every value)
static const char *csr_defect(const plo_csr_t *A, uint32_t p)
{
    if (!A || !A->rowptr || (A->rowptr[A->m] && (!A->col || !A->val))) return "null matrix arrays";
    for (uint32_t i = 0; i < A->m; ++i) {
        if (A->rowptr[i + 1] < A->rowptr[i]) return "rowptr not monotone";
        for (uint32_t k = A->rowptr[i]; k < A->rowptr[i + 1]; ++k) {
            if (A->col[k] >= A->n) return "column index out of range";
            if (k > A->rowptr[i] && A->col[k] <= A->col[k - 1]) return "columns must be strictly increasing inside a row";
            if (A->val[k] == 0 || A->val[k] >= p) return "values must be canonical non-zero residues";
        }
    }
    return nullptr;
}

struct plo_plan {
    plo::WavePlan P{};
    void *d_tmpl = nullptr;
    uint32_t *d_err = nullptr;
    unsigned long long *d_best = nullptr;
    uint32_t waves_per_wg = 0, lds_bytes = 0, blocks_per_cu = 0;
    uint64_t algo_bytes = 0, pairs0 = 0, distinct0 = 0;
    uint32_t p = 0;
    // host copy of the CSR for re-planning with a larger table
    std::vector<uint32_t> rowptr, col, val;
    uint32_t m = 0, n = 0;
    uint32_t cap_scale = 2;
    // HBM-resident variant (one workgroup per candidate)
    bool big = false;
    plo::BigPlan B{};
    std::vector<void *> big_bufs;          // shared immutable device buffers
    bool big_no_defer = false;             // a launch with deferred updates ran out of room in one of their structures: this plan keeps the eager table
    uint32_t big_refits = 0;               // how often that happened (plo_cse_plan_hbm_counters)
    uint32_t big_cap_scale = 1;            // eager table: slots = scale x (2 x initial triples of frequency >= 2), x4 whenever a candidate fills it
    void *d_ws = nullptr; uint64_t ws_slices = 0;
    unsigned long long *d_next = nullptr; uint32_t *d_stats = nullptr;
    uint32_t big_lds = 0;
    // exact search over Q (plo_cse_plan_create_q, plo_capi_cseq.hip): val holds the residues of the entries modulo p, qres the residues of the
    // universe U in Q's order, and the pair keys carry a ratio's rank in U.  qunit: all entries are +-1; the plan then runs the +-1 kernel with
    // p = 1 -- -1 is stored as p - 1 = 0, that kernel's product a == b ? 1 : p - 1 is an xnor, and 0 < 1 is Q's order of -1 and 1.
    bool q = false, qunit = false;
    std::vector<uint32_t> qres;
};

namespace {

// the host copy of the caller's matrix
void set_matrix(plo_plan *pl, const plo_csr_t *A, uint32_t p)
{
    pl->m = A->m; pl->n = A->n; pl->p = p;
    pl->rowptr.assign(A->rowptr, A->rowptr + A->m + 1);
    pl->col.assign(A->col, A->col + A->rowptr[A->m]);
    pl->val.assign(A->val, A->val + A->rowptr[A->m]);
}

// The LDS image of a wave-kernel candidate, from the shape fields of P (m, n, nnz, NC, cap, mw, unit, multcap): the template is its
// first tmpl_bytes, the region all of it; the row starts (rs_bytes) are shared by the waves of a workgroup
void layout_wave_image(plo::WavePlan &P)
{
    const uint32_t mw = P.mw;
    uint32_t off = 0;
    P.off_tab = off;   off += P.cap * 8u;
    P.off_val = off;   off += P.nnz * 4u;
    P.off_inv = off;   off += P.unit ? 0u : P.nnz * 4u;
    P.off_col = off;   off += P.nnz * 2u;
    P.off_len = off;   off += P.m * 2u;
    off = round_up(off, 8);
    P.off_cmask = off;                      // interleaved {cmask[mw], umask[mw]} per column
    P.off_umask = off + mw * 8u;
    P.tmpl_bytes = off + P.n * 2u * mw * 8u;
    off += P.NC * 2u * mw * 8u;
    P.off_aff = off;   off += (2u * mw + 1u) * 8u;
    P.off_ties = off;  off += P.cap * 2u;
    off = round_up(off, 8);
    P.off_mult = off;  off += P.multcap * 8u;
    P.region_bytes = round_up(off, 16);
    P.rs_bytes = round_up((P.m + 1) * 2u, 16);
}

// img_out != nullptr: host part only (the template image and the plan fields; P.tmpl is left for the caller)
int build_plan(plo_plan *pl, std::vector<uint8_t> *img_out = nullptr)
{
    const uint32_t m = pl->m, n = pl->n, p = pl->p;
    const auto &rowptr = pl->rowptr; const auto &col = pl->col; const auto &val = pl->val;
    const uint32_t nnz = rowptr[m];
    plo::WavePlan &P = pl->P;
    P = plo::WavePlan{};
    uint32_t maxlen = 0; bool unit = true;
    for (uint32_t i = 0; i < m; ++i) maxlen = std::max(maxlen, rowptr[i + 1] - rowptr[i]);
    for (uint32_t k = 0; k < nnz; ++k) unit = unit && (val[k] == 1u % p || val[k] == p - 1);
    if (pl->qunit) unit = true;
    if (maxlen > 64) return fail(PLO_E_CAPACITY, "row longer than 64 entries: not handled by the LDS-resident wave kernel");
    if (m == 0 || m > 31 * 64) return fail(PLO_E_CAPACITY, "row count outside [1,1984] for the wave kernel");
    const uint32_t mw = (m + 63) / 64;
    if (!unit && mw > 1) return fail(PLO_E_CAPACITY, "more than 64 rows with non +-1 coefficients: ProgramGen of the wave kernel keeps one row per lane");   // -> HBM family
    // every CSE step lowers sum(len-1) by its frequency >= 2, so there are at most naive_adds/2 steps
    uint32_t naive = 0;
    for (uint32_t i = 0; i < m; ++i) { uint32_t l = rowptr[i + 1] - rowptr[i]; if (l > 1) naive += l - 1; }
    const uint64_t NC = (uint64_t)n + naive / 2 + 2;
    const uint32_t rb = pl->qunit ? 1u : ceil_log2(p), bb = ceil_log2((uint32_t)NC);     // residues < 2^rb, columns < 2^bb (a plan over Q keeps the residues' width for ProgramGen's keys: a rank is narrower)
    if (NC >= 0xFFFFull || 2u * bb + rb > 51u)
        return fail(PLO_E_CAPACITY, "pair key (col,col,ratio) does not fit 51 bits for this matrix/modulus");
    if (2ull * nnz >= 65535ull) return fail(PLO_E_CAPACITY, "op-count may exceed 16 bits");

    std::vector<uint32_t> inv(nnz);
    for (uint32_t k = 0; k < nnz; ++k) inv[k] = pl->qunit ? val[k] : inv_mod(val[k], p);
    std::map<uint32_t, uint32_t> qrank;                                  // over Q: rank in U of a residue
    if (pl->q && !pl->qunit) for (uint32_t k = 0; k < pl->qres.size(); ++k) qrank[pl->qres[k]] = k;
    // initial pair table (listpairs, plinopt_optimize.inl:30-41; PairMap :220-225)
    std::map<uint64_t, uint32_t> pm; uint64_t pairs0 = 0;
    for (uint32_t i = 0; i < m; ++i)
        for (uint32_t x = rowptr[i]; x < rowptr[i + 1]; ++x)
            for (uint32_t y = x + 1; y < rowptr[i + 1]; ++y) {
                uint32_t r = pl->qunit ? (val[y] == val[x] ? 1u : 0u) : (uint32_t)((uint64_t)val[y] * inv[x] % p);
                if (!qrank.empty()) r = qrank.at(r);                     // (U holds every ratio of two entries)
                uint64_t key = ((uint64_t)col[x] << (bb + rb)) | ((uint64_t)col[y] << rb) | r;
                pm[key]++; ++pairs0;
            }
    pl->pairs0 = pairs0; pl->distinct0 = pm.size();
    pl->algo_bytes = 8ull * nnz + 12ull * pairs0 + 8ull;   // B_cand, SURVEY.md 8(d)
    uint32_t cap = 64;
    while (cap < (2u * (uint32_t)pm.size() * 3u) / 4u + 16u) cap <<= 1;   // 1.5x the initial triples; a full table is detected on the device and the launch repeated with more
    cap *= pl->cap_scale / 2u;              // cap_scale starts at 2 and doubles per repeat: every repeat has twice the slots.  (Sized from cap_scale x the triples, a repeat of a matrix of few
                                            // pairs kept its 64 slots: ProgramGen's (column, |v|) keys, which the triples do not bound, then filled the same table in every repeat.)
    if (env_knob("PLO_WAVE_CAP_TIGHT")) {   // test knob: the first table just holds the initial triples and one empty slot (the insertion loop below ends), so that
        cap = 64;                           // a candidate whose live triples grow takes the repeat path; 64 slots at least, the kernel scans the table a wave at a time
        while (cap < (uint32_t)pm.size() + 1u) cap <<= 1;
        cap *= pl->cap_scale / 2u;          // cap_scale doubles per repeat as above
    }
    const uint32_t hbits = ceil_log2(cap);

    P.m = m; P.n = n; P.nnz = nnz; P.p = p; P.NC = (uint32_t)NC; P.cap = cap; P.hbits = hbits;
    P.lpr_log2 = std::max(2u, ceil_log2(std::max(maxlen, 1u))); P.mw = mw; P.unit = unit ? 1u : 0u;
    P.multcap = unit ? 0u : (uint32_t)(naive / 2 + 8); P.maxlen = maxlen; P.rb = rb; P.bb = bb;
    if (cap > 65536u) return fail(PLO_E_CAPACITY, "pair table larger than 65536 slots");
    P.mu = p ? (~0ull) / p : 0;
    layout_wave_image(P);
    const uint32_t tmpl_bytes = P.tmpl_bytes;

    // template image
    std::vector<uint8_t> img(tmpl_bytes + P.rs_bytes, 0);
    uint64_t *tab = (uint64_t *)(img.data() + P.off_tab);
    for (uint32_t s = 0; s < cap; ++s) tab[s] = PLO_EMPTY;               // empty: key all ones, count 0
    for (const auto &kv : pm) {
        uint32_t x = (uint32_t)kv.first ^ ((uint32_t)(kv.first >> 32) * 0x85EBCA6Bu);
        uint32_t s = (x * 0x9E3779B1u) >> (32u - hbits);                   // == plo::tab_hash
        while (tab[s] != PLO_EMPTY) s = (s + 1) & (cap - 1);
        tab[s] = (kv.first << PLO_VB) | kv.second;
    }
    uint32_t *tv = (uint32_t *)(img.data() + P.off_val), *ti = (uint32_t *)(img.data() + P.off_inv);
    uint16_t *tc = (uint16_t *)(img.data() + P.off_col), *tl = (uint16_t *)(img.data() + P.off_len);
    uint64_t *tm = (uint64_t *)(img.data() + P.off_cmask);
    uint16_t *rs = (uint16_t *)(img.data() + tmpl_bytes);
    for (uint32_t k = 0; k < nnz; ++k) { tv[k] = val[k]; if (!unit) ti[k] = inv[k]; tc[k] = (uint16_t)col[k]; }
    for (uint32_t i = 0; i < m; ++i) {
        tl[i] = (uint16_t)(rowptr[i + 1] - rowptr[i]); rs[i] = (uint16_t)rowptr[i];
        for (uint32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            tm[(col[k] * 2u) * mw + (i >> 6)] |= 1ull << (i & 63);
            if (unit || val[k] == 1u % p || val[k] == p - 1) tm[(col[k] * 2u + 1u) * mw + (i >> 6)] |= 1ull << (i & 63);
        }
    }
    rs[m] = (uint16_t)nnz;
    if (!qrank.empty()) {                                                // the tables of plo::QTab behind the row starts
        const uint32_t nu = (uint32_t)pl->qres.size(), qh = std::max(4u, ceil_log2(2u * nu));
        const size_t at = img.size() / 8u;
        img.resize(img.size() + 8u * (1u + ((size_t)1 << qh) + (nu + 1u) / 2u), 0);
        uint64_t *q = (uint64_t *)img.data() + at;
        q[0] = (uint64_t)qh | ((uint64_t)nu << 32);
        for (size_t s = 0; s < ((size_t)1 << qh); ++s) q[1 + s] = ~0ull;
        for (uint32_t k = 0; k < nu; ++k) {
            uint32_t s = (pl->qres[k] * 0x9E3779B1u) >> (32u - qh);                                // == plo::q_rank
            while (q[1 + s] != ~0ull) s = (s + 1u) & ((1u << qh) - 1u);
            q[1 + s] = ((uint64_t)pl->qres[k] << 16) | k;
        }
        memcpy(q + 1 + ((size_t)1 << qh), pl->qres.data(), nu * sizeof(uint32_t));
    }

    // waves per workgroup / LDS
    // waves (= candidates) per workgroup: the choice that puts most waves on a CU
    const size_t lds_max = g_lds_max ? g_lds_max : 160u * 1024u;        // (no device yet: the host-only pass of plo_cse_plan_create_q)
    if (P.rs_bytes + P.region_bytes > lds_max)
        return fail(PLO_E_CAPACITY, "candidate state does not fit the 160 KiB LDS of one CU");
    const uint32_t W = pick_waves([&](uint32_t w) { return P.rs_bytes + w * P.region_bytes; }, true, lds_max, &pl->lds_bytes);
    pl->waves_per_wg = W;

    if (img_out) { *img_out = std::move(img); return PLO_OK; }
    if (pl->d_tmpl) { (void)hipFree(pl->d_tmpl); pl->d_tmpl = nullptr; }
    HIPCHK(hipMalloc(&pl->d_tmpl, img.size()));
    HIPCHK(hipMemcpy(pl->d_tmpl, img.data(), img.size(), hipMemcpyHostToDevice));
    P.tmpl = (const uint64_t *)pl->d_tmpl;
    if (!pl->d_err) HIPCHK(hipMalloc((void **)&pl->d_err, sizeof(uint32_t)));
    if (!pl->d_best) HIPCHK(hipMalloc((void **)&pl->d_best, sizeof(unsigned long long)));

    const void *fn = unit ? (const void *)plo::cse_wave_kernel<true> : pl->q ? plo::cse_wave_q_kernel_fn() : (const void *)plo::cse_wave_kernel<false>;
    return occupancy_for(fn, W, pl->lds_bytes, &pl->blocks_per_cu);
}


template <class T> int upload(plo_plan *pl, const std::vector<T> &v, const T **dst)
{
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T) + 64));      // slack: the kernel copies in 16-byte units
    if (!v.empty()) HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    pl->big_bufs.push_back(d);
    *dst = (const T *)d;
    return PLO_OK;
}

template <bool WIDE> const void *big_kernel_fn_w(const plo::BigPlan &B)
{
    if (B.idk) return B.defer ? (const void *)plo::cse_big_kernel<2, true, true, WIDE> : (const void *)plo::cse_big_kernel<2, false, true, WIDE>;
    if (B.defer) return B.mode == 2u ? (const void *)plo::cse_big_kernel<2, true, false, WIDE> : B.mode == 1u ? (const void *)plo::cse_big_kernel<1, true, false, WIDE> : (const void *)plo::cse_big_kernel<0, true, false, WIDE>;
    return B.mode == 2u ? (const void *)plo::cse_big_kernel<2, false, false, WIDE> : B.mode == 1u ? (const void *)plo::cse_big_kernel<1, false, false, WIDE> : (const void *)plo::cse_big_kernel<0, false, false, WIDE>;
}
// (BigPlan::wide: the kernels that address the workspace slice with 64-bit offsets, layout_big_workspace)
const void *big_kernel_fn(const plo::BigPlan &B) { return B.wide ? big_kernel_fn_w<true>(B) : big_kernel_fn_w<false>(B); }

// The PLO_BIG_* knobs of a plan (tests and experiments).  The first seven are flags; the clamps of the others are where they are used.
struct BigPlanKnobs {
    std::optional<long> vt_global = env_knob("PLO_BIG_VT_GLOBAL"), norid = env_knob("PLO_BIG_NORID"), idkeys = env_knob("PLO_BIG_IDKEYS"),
                        noprune = env_knob("PLO_BIG_NOPRUNE"), eager = env_knob("PLO_BIG_EAGER"), nodual = env_knob("PLO_BIG_NODUAL"), wide = env_knob("PLO_BIG_WIDE");
    std::optional<long> fwin = env_knob("PLO_BIG_FWIN"), hbits = env_knob("PLO_BIG_HBITS"), logtrig = env_knob("PLO_BIG_LOGTRIG"), hwin = env_knob("PLO_BIG_HWIN"),
                        hotbits = env_knob("PLO_BIG_HOTBITS"), lgrp = env_knob("PLO_BIG_LGRP"), aggbits = env_knob("PLO_BIG_AGGBITS"), selcap = env_knob("PLO_BIG_SELCAP");
};
// ... and of a launch
struct BigLaunchKnobs { std::optional<long> wg_per_cu = env_knob("PLO_BIG_WG_PER_CU"), slices = env_knob("PLO_BIG_SLICES"), stats = env_knob("PLO_BIG_STATS"); };

// the distinct pair triples of the input, sorted per first column: keys, frequencies, the largest frequency; pairs0 = the pair instances
struct BigTriples { std::vector<uint64_t> keys; std::vector<uint32_t> cnts; uint64_t pairs0 = 0; uint32_t maxf = 0; };

// Deferred cold updates (plo_cse_big.hip, "Deferred cold updates"): partitioned store + log + hot table instead of the one big table.
// Taken whenever its LDS budget allows (a partition and its share of the log are summed in a 2^13-slot LDS table); PLO_BIG_EAGER=1
// keeps the eager table (the A/B switch of the tests).  Sizes the structures in pl->B; st0 and pc0 get the store's image.
void size_big_deferred(plo_plan *pl, const BigPlanKnobs &K, const BigTriples &T, std::vector<uint64_t> &st0, std::vector<uint32_t> &pc0)
{
    plo::BigPlan &B = pl->B;
    const auto &keys = T.keys; const auto &cnts = T.cnts;
    const uint32_t m = pl->m;
    B.defer = 0u;
    if (!B.prune || K.eager || pl->big_no_defer) return;
    uint64_t topsum = 0;                                      // entries of the M0 longest rows: a step rewrites at most M0 rows
    { std::vector<uint32_t> ls(m); for (uint32_t i = 0; i < m; ++i) ls[i] = pl->rowptr[i + 1] - pl->rowptr[i];
      std::sort(ls.begin(), ls.end(), std::greater<uint32_t>());
      for (uint32_t i = 0; i < m && i < T.maxf; ++i) topsum += ls[i]; }
    uint32_t pbits = 0; while ((keys.size() >> pbits) > 1280u && pbits < 11u) ++pbits;
    const uint32_t Pn = 1u << pbits;
    pc0.assign(Pn, 0u);
    auto part = [&](uint64_t k) { return pbits ? (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> (64u - pbits)) : 0u; };   // == plo::dpart
    for (uint64_t k : keys) ++pc0[part(k)];
    const uint32_t maxfill = *std::max_element(pc0.begin(), pc0.end());
    const uint32_t capp = (maxfill + maxfill / 4u + 64u + 1u) & ~1u;
    const uint64_t hotmax = std::min<uint64_t>(1ull << 17, T.pairs0);               // triples alive at any time <= pair instances of the input
    const uint64_t stepmax = 3ull * topsum + 3ull * 8192ull;                        // records one step can write
    if (capp > 5000u) return;
    const uint64_t lpp = 6080u - capp;                                              // records of a partition's log that still fit the merge beside its live triples (12 records per thread, an LDS table of 2^13 slots)
    const uint64_t budget = lpp * Pn * 5ull / 6ull;                                 // (hash imbalance of the partitions' shares)
    if (budget <= stepmax + hotmax + 4096ull) return;
    uint64_t trig = std::min<uint64_t>(budget - stepmax - hotmax - 4096ull, (uint64_t)PLO_BIG_LOGTRIG_MAX);
    if (K.logtrig) trig = std::min<uint64_t>(trig, std::max<uint64_t>(1, (uint64_t)*K.logtrig));   // test knob: merges forced by the log
    const uint64_t logcap = trig + stepmax + hotmax + 4096ull;
    B.defer = 1u; B.pbits = pbits; B.capp = capp; B.logtrig = (uint32_t)trig; B.logcap = (uint32_t)logcap;
    B.plcap = (uint32_t)std::min<uint64_t>((logcap * 6ull / 5ull + Pn - 1) / Pn + 64ull, lpp + 64ull);
    B.hwin = 8192u; if (K.hwin) B.hwin = (uint32_t)std::max<long>(1, *K.hwin);   // test knob: window size (triples kept hot)
    B.hotbits_min = std::min(16u, std::max(10u, ceil_log2((uint32_t)(4u * std::min<uint64_t>(T.pairs0, 16384u)))));
    B.hotbits_max = std::max(B.hotbits_min, std::min(19u, ceil_log2((uint32_t)(4u * hotmax + 1024u))));
    if (K.hotbits) B.hotbits_min = (uint32_t)std::min<long>(B.hotbits_max, std::max<long>(6, *K.hotbits));   // test knob: a full hot table is reported and the launch repeated with a larger one
    B.lgrp = 3000u; if (K.lgrp) B.lgrp = (uint32_t)std::min<long>(7000, std::max<long>(64, *K.lgrp));   // experiment knob: records per group of partitions summed together
    st0.assign((size_t)capp * Pn, 0ull);
    std::vector<uint32_t> fill(Pn, 0u);
    for (size_t k = 0; k < keys.size(); ++k) { const uint32_t q = part(keys[k]); st0[(size_t)q * capp + fill[q]++] = (keys[k] << PLO_GVB) | 0x8000ull | cnts[k]; }   // a record: key | insert flag | frequency
}

// Workspace layout of one candidate (the eager table has 2^hbits slots; with deferred updates hbits becomes ProgramGen's).  The kernels
// address everything but the large region -- the eager table, which the capacity refits multiply by up to 256, or the deferred store --
// as the slice's base plus a 32-bit byte offset (plo::WsArr), so that region comes LAST with a pointer of its own and everything else
// lies in front of it.  The front region is 36 bytes per entry and more: at the kernels' limits (32766 rows of 8192 entries) it can pass
// 4 GiB, and such a plan -- or any plan, with the test knob `force_wide` -- takes the kernels with 64-bit offsets (B.wide).
void layout_big_workspace(plo::BigPlan &B, bool force_wide = false)
{
    const uint64_t nnz = B.nnz, m = B.m, NC = B.NCmax, multcap = B.multcap;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) { uint64_t o = off; off = (off + bytes + 255) & ~255ull; return o; };
    if (B.defer) {
        B.o_pcount = take(4ull << B.pbits); B.o_ptail = take(4ull << B.pbits);
        B.o_log = take((uint64_t)B.logcap * 8); B.o_hot = take(8ull << B.hotbits_max);
    }
    B.o_ent = take((nnz + 128) * 4); B.o_col = take(nnz * 4); B.o_val = take(nnz * 4); B.o_inv = take(nnz * 4);
    B.o_len = take(m * 4); B.o_ucount = take(NC * 4); B.o_cntM = take(NC * 4);
    B.o_dm = take((uint64_t)B.dmcap * 8); B.o_hl = take((uint64_t)B.hlcap * 16); B.o_aff = take(m * 32);
    B.o_ncrptr = take((NC + 2) * 4); B.o_ncr = take((nnz + 64) * 4);
    B.o_tl = take((nnz + 64) * 4); B.o_clen = take(NC * 4); B.o_keep = take((m + 64) * 4);
    B.o_multc = take(multcap * 4); B.o_multv = take(multcap * 4);
    B.o_tcnt = take(NC * 4); B.o_tptr2 = take((NC + 2) * 4); B.o_tlist = take((nnz + 64) * 4); B.o_cols2 = take(NC * 4); B.o_spill = take((nnz + 64) * 8);
    B.wide = (force_wide || off > 0xFFFFFFFFull) ? 1u : 0u;           // `off` = the front region's bytes
    if (B.defer) {
        // the table region only serves ProgramGen's (column, |v|) multiset: it shares the partitions' logs, idle by then
        uint64_t pg = 1024; while (pg < 2ull * nnz + 2ull * multcap + 64ull) pg <<= 1;
        B.hbits = ceil_log2((uint32_t)pg);
        B.o_store = take(std::max<uint64_t>(((uint64_t)(B.capp + B.plcap) << B.pbits) * 8, pg * 8)); B.o_tab = B.o_store; B.o_plog = 0;
    } else B.o_tab = take(8ull << B.hbits);
    B.ws_stride = off;
}

// dynamic LDS: histogram + max(ProgramGen scratch, aggregation table of 2^aggbits u64)
int size_big_lds(plo_plan *pl, const BigPlanKnobs &K)
{
    plo::BigPlan &B = pl->B;
    const uint32_t maxlen = B.scr_stride;
    B.aggbits = std::min(13u, std::max(6u, ceil_log2((uint32_t)std::min<uint64_t>(4 * pl->pairs0 + 64, 1u << 13))));
    if (K.aggbits) B.aggbits = (uint32_t)std::min(14l, std::max(6l, *K.aggbits));
    // LDS aggregation entry: key | count.  When column, ratio, inverse ratio and a count up to m fit 64 bits the key carries
    // both x and 1/x (the flush then needs no inversion); otherwise (column, x) with a 16-bit count.
    { const uint32_t cb = ceil_log2(B.m + 2u);
      if (B.bb + 2u * B.rb + cb <= 64u && !K.nodual) { B.agg_dual = 1u; B.agg_cb = 64u - B.bb - 2u * B.rb; if (B.agg_cb > 16u) B.agg_cb = 16u; }
      else { B.agg_dual = 0u; B.agg_cb = 16u; } }
    // dynamic LDS, in words: histogram, tables of the mode, then max(ProgramGen scratch, aggregation table: 2^aggbits entries of 8 bytes, 6 in mode 2)
    const uint32_t agg_words = B.mode == 2u ? (1u << B.aggbits) + (1u << B.aggbits) / 2u : 2u << B.aggbits;
    uint32_t scr_words = std::max<uint32_t>((PLO_BIG_THREADS / 64) * maxlen, agg_words);
    uint32_t tab_words = B.mode == 1u ? 2u * ((B.nv + 1u) & ~1u) : B.mode == 2u ? ((B.nr + 1u) & ~1u) + PLO_RSTRIDE * PLO_RSTRIDE / 2u + (B.nr + 3u) / 4u * 2u + (B.defer ? 0u : (1u << B.aggbits) / 2u) : 0u;   // mode 2: ratio values, ratio ids, inverse ids, slot list of the aggregation table (eager flush only)
    if (B.defer) { tab_words += PLO_DBLOOM_WORDS; scr_words = std::max<uint32_t>(scr_words, PLO_DMREG_WORDS - PLO_DBLOOM_WORDS); }   // Bloom filter, and 64 KB in all for the merge
    pl->big_lds = (((B.maxf0 + 2u) & ~1u) + tab_words + scr_words) * 4u;
    if (pl->big_lds + sizeof(plo::BigShared) + 64 > g_lds_max) return fail(PLO_E_CAPACITY, "frequency histogram does not fit LDS");
    return PLO_OK;
}

// Plan for the HBM-resident kernel family (plo_cse_big.hip)
int build_big_plan(plo_plan *pl)
{
    const BigPlanKnobs K;
    const uint32_t m = pl->m, n = pl->n, p = pl->p;
    const auto &rowptr = pl->rowptr; const auto &col = pl->col; const auto &val = pl->val;
    const uint32_t nnz = rowptr[m];
    plo::BigPlan &B = pl->B; B = plo::BigPlan{};
    if (m == 0) return fail(PLO_E_CAPACITY, "empty matrix");
    uint32_t maxlen = 1, naive = 0; bool unit = true;
    for (uint32_t i = 0; i < m; ++i) { uint32_t l = rowptr[i + 1] - rowptr[i]; maxlen = std::max(maxlen, l); if (l > 1) naive += l - 1; }
    for (uint32_t k = 0; k < nnz; ++k) unit = unit && (val[k] == 1u || val[k] == p - 1);
    // The values of a candidate are the distinct values of the input (a CSE step moves values, it creates none): rows are
    // packed as column | +-1 flag << 15 | value index << 16, with one {value, inverse} table.
    std::vector<uint32_t> dv(val.begin(), val.end());
    std::sort(dv.begin(), dv.end()); dv.erase(std::unique(dv.begin(), dv.end()), dv.end());
    if (dv.size() > 65536) return fail(PLO_E_CAPACITY, "more than 65536 distinct coefficients: the packed row entry holds a 16-bit value index");
    // at most 32 values: the <= 1024 ratios v_i/v_j get identifiers (kernel mode 2: 6-byte aggregation entries, no product in the sweep)
    const bool ratio_ids = dv.size() <= 32 && !K.vt_global && !K.norid;
    std::vector<uint32_t> rat, rv;
    if (ratio_ids) {
        const uint32_t nv = (uint32_t)dv.size();
        rat.resize(nv * nv);
        for (uint32_t i = 0; i < nv; ++i) { const uint32_t ii = inv_mod(dv[i], p); for (uint32_t j = 0; j < nv; ++j) rat[j * nv + i] = (uint32_t)((uint64_t)dv[j] * ii % p); }   // rat[i * nv + j] = v_i / v_j
        rv = rat; std::sort(rv.begin(), rv.end()); rv.erase(std::unique(rv.begin(), rv.end()), rv.end());
    }
    // A pair key is (column, column, ratio) in 48 bits.  Ratio field: the residue (rb bits) -- or, when that leaves too few bits for the
    // columns (a 31-bit prime: 8 bits, 256 columns) and the matrix has ratio identifiers, the IDENTIFIER (rank in the sorted list of
    // ratios: keys keep their order), kb <= 10 bits: any modulus below 2^31 with 32768 columns (plo::cse_big_idkey_kernel).
    const uint32_t rb = ceil_log2(p);
    uint64_t NC = (uint64_t)n + naive / 2 + 2;
    uint32_t kb = rb; bool idk = false;
    {
        const uint32_t bbres = rb <= 44u ? (48u - rb) / 2u : 0u;            // column bits beside a residue
        const bool fits = rb <= 30u && bbres >= 2u && n + 2ull <= (1ull << bbres) && std::min<uint64_t>(NC, 32768) <= (1ull << bbres);
        if ((!fits || K.idkeys) && ratio_ids && rb <= 31u) { idk = true; kb = std::max(1u, ceil_log2((uint32_t)rv.size())); }   // (PLO_BIG_IDKEYS: test knob, identifiers although residues would fit)
        // (!fits below 15 column bits: the modulus, not the kernel's 32768 columns, is what leaves no room -- the bound NC on the created columns
        // counts, as it does for the identifiers above; clamping it to 2^bbres instead would only move the refusal into the launch)
        else if (rb > 30 || bbres < 2u || (bbres < 15u && !fits)) return fail(PLO_E_CAPACITY, "modulus too large for the 48-bit pair key (and more than 32 distinct coefficients: no ratio identifiers)");
    }
    const uint32_t bbmax = std::min(15u, (48u - kb) / 2u);
    if (n + 2ull > (1ull << bbmax) || n + 2ull > 32768ull) return fail(PLO_E_CAPACITY, "too many columns for the HBM-resident kernel (48-bit pair key / 32768 columns)");
    NC = std::min<uint64_t>(std::min<uint64_t>(NC, 1ull << bbmax), 32768);   // 32768 = 512 LDS block sums x 64; exceeding it at run time is reported by the device (BERR_COLS)
    const uint32_t bb = ceil_log2((uint32_t)NC);
    if (m >= 0x7FFFu) return fail(PLO_E_CAPACITY, "more than 32766 rows: frequency does not fit the table slot");
    if (maxlen > 8192) return fail(PLO_E_CAPACITY, "row longer than 8192 entries");

    std::vector<uint2> vt(dv.size());
    for (size_t k = 0; k < dv.size(); ++k) vt[k] = make_uint2(dv[k], inv_mod(dv[k], p));
    std::vector<uint32_t> inv(nnz), ent(nnz), tptr(n + 1, 0), trows(nnz), ucount(n, 0);
    for (uint32_t k = 0; k < nnz; ++k) {
        const uint32_t vi = (uint32_t)(std::lower_bound(dv.begin(), dv.end(), val[k]) - dv.begin());
        const bool u1 = val[k] == 1u || val[k] == p - 1;
        inv[k] = vt[vi].y; ent[k] = col[k] | (u1 ? 0x8000u : 0u) | (vi << 16);
        ++tptr[col[k] + 1]; if (u1) ++ucount[col[k]];
    }
    for (uint32_t c = 0; c < n; ++c) tptr[c + 1] += tptr[c];
    { std::vector<uint32_t> pos(tptr.begin(), tptr.end() - 1);
      for (uint32_t i = 0; i < m; ++i) for (uint32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) trows[pos[col[k]]++] = i; }
    // distinct pair triples, per first column (listpairs :30-41, PairMap :220-225)
    BigTriples T;
    std::vector<uint64_t> &keys = T.keys; std::vector<uint32_t> &cnts = T.cnts;
    {
        std::vector<uint64_t> tmp;
        for (uint32_t a = 0; a < n; ++a) {
            tmp.clear();
            for (uint32_t q = tptr[a]; q < tptr[a + 1]; ++q) {
                const uint32_t i = trows[q]; uint32_t x = rowptr[i];
                while (col[x] != a) ++x;
                for (uint32_t y = x + 1; y < rowptr[i + 1]; ++y)
                {
                    uint32_t rr = (uint32_t)((uint64_t)val[y] * inv[x] % p);
                    if (idk) rr = (uint32_t)(std::lower_bound(rv.begin(), rv.end(), rr) - rv.begin());
                    tmp.push_back(((uint64_t)a << (bb + kb)) | ((uint64_t)col[y] << kb) | rr);
                }
            }
            T.pairs0 += tmp.size();
            std::sort(tmp.begin(), tmp.end());
            for (size_t k = 0; k < tmp.size();) {
                size_t j = k; while (j < tmp.size() && tmp[j] == tmp[k]) ++j;
                keys.push_back(tmp[k]); cnts.push_back((uint32_t)(j - k)); T.maxf = std::max(T.maxf, (uint32_t)(j - k)); k = j;
            }
        }
    }
    const uint32_t maxf = T.maxf;
    pl->pairs0 = T.pairs0; pl->distinct0 = keys.size();
    pl->algo_bytes = 8ull * nnz + 16ull * keys.size();       // distinct-triple form of B_cand for HBM-resident candidates
    B.prune = K.noprune ? 0u : 1u;
    B.fwin = 2048u; if (K.fwin) B.fwin = (uint32_t)std::min<long>(2048, std::max<long>(64, *K.fwin / 64 * 64));   // test knob: windows of the flat sweep (a multiple of 64 entries)
    if (B.prune) {   // triples of frequency 1 are never chosen and never grow: they are not kept (plo_cse_big.hip, "pruning")
        size_t w = 0;
        for (size_t k = 0; k < keys.size(); ++k) if (cnts[k] >= 2u) { keys[w] = keys[k]; cnts[w] = cnts[k]; ++w; }
        keys.resize(w); cnts.resize(w);
    }
    const uint32_t multcap = (uint32_t)std::min<uint64_t>((uint64_t)naive / 2 + 8, NC);
    uint64_t cap = 1024;
    // load <= 0.5 at the start: the retirement of a pruned triple probes to the first empty slot, and dead slots are not empty
    while (cap < (uint64_t)pl->big_cap_scale * (2ull * keys.size() + 1024ull) || cap < 2ull * nnz + 2ull * multcap + 64ull) cap <<= 1;
    if (K.hbits) { const long hb = *K.hbits; if (hb >= 10 && hb <= 30 && (1ull << hb) > keys.size() + keys.size() / 8) cap = 1ull << hb; }   // experiment knob
    const uint32_t hbits = ceil_log2((uint32_t)std::min<uint64_t>(cap, 1ull << 31));
    if (cap > (1ull << 30)) return fail(PLO_E_CAPACITY, "pair table above 2^30 slots");
    std::vector<uint32_t> hist(maxf + 2, 0);
    for (size_t k = 0; k < keys.size(); ++k) ++hist[cnts[k]];
    B.m = m; B.n = n; B.nnz = nnz; B.p = p; B.NCmax = (uint32_t)NC; B.hbits = hbits; B.rb = rb; B.bb = bb; B.kb = kb; B.idk = idk ? 1u : 0u; B.unit = unit ? 1u : 0u;
    B.maxf0 = maxf + 1; B.M0 = maxf; B.multcap = multcap; B.scr_stride = maxlen;
    B.dmcap = (uint32_t)std::min<uint64_t>(1u << 20, cap); B.hlcap = (uint32_t)std::min<uint64_t>(1u << 18, cap);   // window list: <= hlcap/2 keys per window, ping-pong halves
    B.mu = (~0ull) / p;
    B.mers = 0; for (uint32_t k = 2; k < 31; ++k) if (p == (1u << k) - 1u) B.mers = k;     // Mersenne modulus: shift-and-add reduction
    std::vector<uint64_t> st0; std::vector<uint32_t> pc0;
    size_big_deferred(pl, K, T, st0, pc0);
    int rc;
    if ((rc = upload(pl, pl->rowptr, &B.rs)) || (rc = upload(pl, ent, &B.ent0)) || (rc = upload(pl, vt, &B.vt)) ||
        (rc = upload(pl, tptr, &B.tptr)) || (rc = upload(pl, trows, &B.trows)) ||
        (rc = upload(pl, ucount, &B.ucount0)) || (rc = upload(pl, hist, &B.hist0))) return rc;
    if (B.defer) { if ((rc = upload(pl, st0, &B.st0)) || (rc = upload(pl, pc0, &B.pcount0))) return rc; B.tab0 = nullptr; }
    else {
        std::vector<uint64_t> tab(cap, PLO_GEMPTY);
        for (size_t k = 0; k < keys.size(); ++k) {
            uint32_t s = (uint32_t)((keys[k] * 0x9E3779B97F4A7C15ull) >> (64u - hbits));       // == plo::ghash
            while (tab[s] != PLO_GEMPTY) s = (s + 1) & (uint32_t)(cap - 1);
            tab[s] = (keys[k] << PLO_GVB) | cnts[k];
        }
        if ((rc = upload(pl, tab, &B.tab0))) return rc;
    }
    B.nv = (uint32_t)dv.size(); B.vt_lds = (dv.size() <= 512 && !K.vt_global) ? 1u : 0u;   // (test knob: the global-memory value table)
    B.mode = B.vt_lds ? 1u : 0u; B.nr = 0;
    if (ratio_ids) {
        const uint32_t nv = (uint32_t)dv.size();
        std::vector<uint16_t> rt(PLO_RSTRIDE * PLO_RSTRIDE, 0), iv(rv.size());     // identifiers at [i * 32 + j]
        for (uint32_t i = 0; i < nv; ++i) for (uint32_t j = 0; j < nv; ++j) rt[i * PLO_RSTRIDE + j] = (uint16_t)(std::lower_bound(rv.begin(), rv.end(), rat[i * nv + j]) - rv.begin());
        for (size_t k = 0; k < rv.size(); ++k) iv[k] = (uint16_t)(std::lower_bound(rv.begin(), rv.end(), inv_mod(rv[k], p)) - rv.begin());   // the inverse of v_i/v_j is v_j/v_i: in the set
        if ((rc = upload(pl, rv, &B.rval)) || (rc = upload(pl, rt, &B.rtid)) || (rc = upload(pl, iv, &B.invid))) return rc;
        B.nr = (uint32_t)rv.size(); B.mode = 2u;
    }
    B.invtab = nullptr;
    if (p <= (1u << 20)) {                                   // 1/x for every residue (the flush needs v_a/v_c from v_c/v_a): i^-1 = -(p/i) (p mod i)^-1
        std::vector<uint32_t> it(p, 0); it[1] = 1;
        for (uint32_t i = 2; i < p; ++i) it[i] = (uint32_t)((uint64_t)(p - p / i) * it[p % i] % p);
        if ((rc = upload(pl, it, &B.invtab))) return rc;
    }
    layout_big_workspace(B, K.wide.has_value());
    if ((rc = size_big_lds(pl, K))) return rc;
    HIPCHK(hipFuncSetAttribute(big_kernel_fn(B), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl->big_lds));
    if (!pl->d_err) HIPCHK(hipMalloc((void **)&pl->d_err, sizeof(uint32_t)));
    if (!pl->d_best) HIPCHK(hipMalloc((void **)&pl->d_best, sizeof(unsigned long long)));
    if (!pl->d_next) HIPCHK(hipMalloc((void **)&pl->d_next, sizeof(unsigned long long)));
    if (!pl->d_stats) HIPCHK(hipMalloc((void **)&pl->d_stats, plo::BS_COUNT * sizeof(uint32_t)));
    B.selcap = PLO_BIG_SELCAP;
    if (K.selcap) B.selcap = (uint32_t)std::min<long>(PLO_BIG_SELCAP, std::max<long>(1, *K.selcap));   // test knob: forces the bisection tie pick
    pl->big = true; pl->waves_per_wg = PLO_BIG_THREADS / 64; pl->lds_bytes = pl->big_lds + (uint32_t)sizeof(plo::BigShared);
    return PLO_OK;
}

// frees the plan's device buffers and builds the plan again (a larger table, or the eager one: the caller has set which)
int rebuild_big_plan(plo_plan *pl)
{
    for (void *d : pl->big_bufs) (void)hipFree(d);
    pl->big_bufs.clear();
    if (pl->d_ws) { (void)hipFree(pl->d_ws); pl->d_ws = nullptr; pl->ws_slices = 0; }
    return build_big_plan(pl);
}

// PLO_BIG_STATS: the counters and phase clocks of the launch that just ended, on stderr
void print_big_stats(const plo_plan *pl)
{
    using namespace plo;
    uint32_t hs[BS_COUNT] = {0};
    if (hipMemcpy(hs, pl->d_stats, sizeof hs, hipMemcpyDeviceToHost) != hipSuccess) return;
    const uint32_t ncand = hs[BS_SUM_CANDIDATES], *mg = hs + BS_LAST_MERGE_US, *ms = hs + BS_LAST_MERGE_SUM_US, *ph = hs + BS_LAST_PHASE_US, *pg = hs + BS_LAST_PGEN_PHASE_US;
    if (pl->B.defer && ncand) fprintf(stderr, "# big kernel, deferred updates: per candidate %.1f merges (%.2f forced by log/hot pressure), %.0f log records, %.0f hot-table updates; last candidate, merge us: hot->log %u, partition pass %u, sum + write back %u, window %u\n",
            (double)hs[BS_SUM_FULLSCANS] / ncand, (double)hs[BS_SUM_FORCED_MERGES] / ncand, ((double)hs[BS_SUM_LOG_HI] * 4294967296.0 + hs[BS_SUM_LOG_LO]) / ncand, (double)hs[BS_SUM_HOTOPS] / ncand, mg[0], mg[1], mg[2], mg[3]);
    if (pl->B.defer && hs[BS_LAST_MERGE_GROUPS]) fprintf(stderr, "#   merge, sum + write back of the last candidate: %u groups; us: sum (loads + table) %u, scan + write back %u, clear + bounds %u\n", hs[BS_LAST_MERGE_GROUPS], ms[0], ms[1], ms[3]);
    if (pl->B.defer && hs[BS_OR_MERGE_TABLES]) fprintf(stderr, "#   merge, summing-table sizes of the launch's groups (OR of 1 << lb): 0x%x\n", hs[BS_OR_MERGE_TABLES]);
    fprintf(stderr, "# big kernel (last candidate): steps %u, full scans %u, level rebuilds %u; phase us: level %u select %u rows %u sweep1 %u flush1 %u sweep2 %u flush2 %u tail %u\n",
            hs[BS_LAST_STEPS], hs[BS_LAST_FULLSCANS], hs[BS_LAST_REBUILDS], ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6], ph[7]);
    fprintf(stderr, "# big kernel (last candidate): image load + CSE phase %u us, ProgramGen %u us\n", hs[BS_LAST_CSE_US], hs[BS_LAST_PGEN_US]);
    fprintf(stderr, "# big kernel (last candidate): image load alone %u us; ProgramGen us: table fill + flags %u, expand + A1 %u, A2 %u, A3 + B + count %u, Triangle set-up %u, Triangle %u, D %u\n",
            hs[BS_LAST_LOAD_US], pg[0], pg[1], pg[2], pg[3], pg[4], pg[5], pg[6]);
#ifdef PLO_BIG_PROFILE
    { unsigned long long g2[40] = {0}; if (hipMemcpyFromSymbol(g2, HIP_SYMBOL(plo::g_prof2), sizeof g2) == hipSuccess && g2[32]) {
        static const char *cls[4] = {">=256", "64..255", "16..63", "<16"};
        for (int c_ = 0; c_ < 4; ++c_) { fprintf(stderr, "#   rows/step %-8s ms per candidate: level %.1f select %.1f rows %.1f sweep %.1f flush1 %.1f flush2 %.1f tail %.1f\n", cls[c_],
            g2[c_ * 8 + 0] / 1e5 / g2[32], g2[c_ * 8 + 1] / 1e5 / g2[32], g2[c_ * 8 + 2] / 1e5 / g2[32], g2[c_ * 8 + 3] / 1e5 / g2[32], g2[c_ * 8 + 4] / 1e5 / g2[32], (g2[c_ * 8 + 6] + g2[c_ * 8 + 5]) / 1e5 / g2[32], g2[c_ * 8 + 7] / 1e5 / g2[32]); } } }
    { unsigned long long gp[16] = {0};
      if (hipMemcpyFromSymbol(gp, HIP_SYMBOL(plo::g_prof), sizeof gp) != hipSuccess) memset(gp, 0, sizeof gp);
      if (gp[3]) fprintf(stderr, "#   sweep of the steps with >= 256 rows, all candidates: %llu trips by %llu wave-sweeps; cycles per trip: chunk wait + stores %.0f, aggregation of both chunks %.0f, rest of the loop %.0f; per wave-sweep %.0f cycles, %.1f trips; probe rounds per trip %.2f, active lanes per trip %.1f\n", gp[3], gp[5], (double)gp[0] / gp[3], (double)gp[1] / gp[3], (double)gp[2] / gp[3], (double)gp[4] / gp[5], (double)gp[3] / gp[5], (double)gp[6] / gp[3], (double)gp[7] / gp[3]);
      if (gp[3] && pl->B.defer && pl->B.mode == 2u) fprintf(stderr, "#   aggregation of a trip (lane 0 of every wave, big steps), cycles: ratio-id lookup %.0f, pair read %.0f, compare-and-swap %.0f, count %.0f\n", (double)gp[14] / gp[3], (double)gp[8] / gp[3], (double)gp[9] / gp[3], (double)gp[10] / gp[3]);
      if ((gp[14] || gp[15]) && !pl->B.defer) fprintf(stderr, "#   flush 1, all candidates: entries whose pair with a has a as SECOND column %llu, with b %llu\n", gp[14], gp[15]);
      if (gp[11]) fprintf(stderr, "#   flush 1 of the steps with >= 256 rows: %llu wave-trips by %llu wave-flushes; cycles per trip: fetch + decode %.0f, probe loads %.0f, stores + bookkeeping %.0f; per wave-flush %.0f cycles, %.1f trips\n", gp[11], gp[13], (double)gp[8] / gp[11], (double)gp[9] / gp[11], (double)gp[10] / gp[11], (double)gp[12] / gp[13], (double)gp[11] / gp[13]);
    }
    { const uint32_t *s1 = hs + BS_PROF_SWEEP1_US, *s2 = hs + BS_PROF_SWEEP2_US, *nb = hs + BS_PROF_STEPS;
      fprintf(stderr, "#   steps by rows/step [>=256, 64.., 16.., <16]: %u %u %u %u; sweep1 us %u %u %u %u; sweep2 us %u %u %u %u; fallbacks %u %u; flushed keys %u %u\n",
            nb[0], nb[1], nb[2], nb[3], s1[0], s1[1], s1[2], s1[3], s2[0], s2[1], s2[2], s2[3], hs[BS_PROF_FALLBACK1], hs[BS_PROF_FALLBACK2], hs[BS_PROF_FLUSHED1], hs[BS_PROF_FLUSHED2]); }
#endif
}

// launch of the HBM-resident kernel over J.ncand candidates
int launch_big(plo_plan *pl, plo::BigJob J, plo_stats_t *st)
{
    const BigLaunchKnobs K;
    // one workspace slice per resident workgroup
    uint64_t per_cu = 2;                  // = the resident workgroups (LDS-limited); more slices only enlarge the footprint
    if (K.wg_per_cu) per_cu = std::max<uint64_t>(1, (uint64_t)*K.wg_per_cu);
    uint64_t want = std::min<uint64_t>(J.ncand, (uint64_t)g_cus * per_cu);
    if (K.slices) want = std::min<uint64_t>(want, (uint64_t)*K.slices);
    if (want == 0) want = 1;
    if (pl->ws_slices < want) {
        if (pl->d_ws) { (void)hipFree(pl->d_ws); pl->d_ws = nullptr; pl->ws_slices = 0; }
        size_t fr = 0, tot = 0; HIPCHK(hipMemGetInfo(&fr, &tot));
        uint64_t fit = (uint64_t)(fr * 0.85) / pl->B.ws_stride;
        if (fit == 0) return fail(PLO_E_CAPACITY, "not enough HBM for one candidate workspace");
        want = std::min(want, fit);
        HIPCHK(hipMalloc(&pl->d_ws, want * pl->B.ws_stride));
        pl->ws_slices = want;
    }
    const uint64_t grid = std::min<uint64_t>(pl->ws_slices, want);
    pl->B.ws = (uint8_t *)pl->d_ws;
    HIPCHK(hipMemsetAsync(pl->d_next, 0, sizeof(unsigned long long), g_stream));
    HIPCHK(hipMemsetAsync(pl->d_stats, 0, plo::BS_COUNT * sizeof(uint32_t), g_stream));
    J.err = pl->d_err; J.next = pl->d_next; J.stats = pl->d_stats;
    void *args[] = {&pl->B, &J};
    const int err = checked_launch(pl->d_err, st, LaunchShape{grid, pl->lds_bytes, pl->waves_per_wg, pl->algo_bytes},
                                   [&] { (void)hipLaunchKernel(big_kernel_fn(pl->B), dim3((uint32_t)grid), dim3(PLO_BIG_THREADS), args, pl->big_lds, g_stream); });
    if (err < 0) return err;
    if (K.stats) print_big_stats(pl);
    if (err == plo::BERR_TABLE && !pl->B.defer && pl->big_cap_scale < 256u) {
        // eager table full: the live triples of frequency >= 2 can outnumber the input's (new columns pair with every column of the rows
        // they enter); four times the slots and again (the workspace grows, fewer candidates are resident)
        pl->big_cap_scale *= 4u; ++pl->big_refits;
        const int rc = rebuild_big_plan(pl);
        return rc != PLO_OK ? rc : launch_big(pl, J, st);
    }
    if (err == plo::BERR_TABLE && pl->B.defer && !pl->big_no_defer) {
        // The structures of the deferred updates are sized from the INPUT's triples (a partition's live triples: its initial share + 25 %;
        // the log and the hot table from the longest rows); a candidate whose live triples grow beyond that -- random dense matrices
        // with few distinct values do (tests/soak_hbm.py) -- is reported by the device.  The plan is rebuilt with the eager table of
        // round 2 (sized for every pair instance of the input, dead slots reclaimed) and the launch repeated: same results, slower.
        pl->big_no_defer = true; ++pl->big_refits;
        const int rc = rebuild_big_plan(pl);
        return rc != PLO_OK ? rc : launch_big(pl, J, st);
    }
    if (err) {
        static const char *names[] = {"pair table", "frequency/row-count mismatch", "column bound", "level list", "window list", "multiplier list", "tie selection", "ProgramGen"};
        uint32_t site = 0; (void)hipMemcpy(&site, pl->d_stats + plo::BS_ERR_SITE, sizeof site, hipMemcpyDeviceToHost);
        // BERR_PGEN: ProgramGen's Triangle keeps the rows of a column one per lane (more than 64 rows with a non +-1 entry in one column), or its
        // multiset does not fit the table region: a limit of this build, not an inconsistency -- the tools then search on the host
        return fail(err == plo::BERR_COLS || err == plo::BERR_DM || err == plo::BERR_HL ? PLO_E_CAPACITY : err == plo::BERR_PGEN ? PLO_E_UNSUPPORTED : PLO_E_INTERNAL,
                    std::string("device (HBM variant): ") + (err >= 11 && err <= 18 ? names[err - 11] : "unknown") + " error " + std::to_string(err) + (site ? " (site " + std::to_string(site) + ")" : ""));
    }
    return PLO_OK;
}

// one launch over [first, first+count) candidates of a job
int launch(plo_plan *pl, plo::WaveJob J, plo_stats_t *st)
{
    const uint32_t W = pl->waves_per_wg;
    const uint64_t grid = grid_for(J.ncand, W, (uint64_t)g_cus * pl->blocks_per_cu);
    J.err = pl->d_err;
    const int err = checked_launch(pl->d_err, st, LaunchShape{grid, pl->lds_bytes, W, pl->algo_bytes}, [&] {
        if (pl->P.unit) hipLaunchKernelGGL(plo::cse_wave_kernel<true>, dim3((uint32_t)grid), dim3(W * 64), pl->lds_bytes, g_stream, pl->P, J);
        else if (pl->q) plo::cse_wave_q_launch((uint32_t)grid, W * 64, pl->lds_bytes, g_stream, pl->P, J);
        else hipLaunchKernelGGL(plo::cse_wave_kernel<false>, dim3((uint32_t)grid), dim3(W * 64), pl->lds_bytes, g_stream, pl->P, J);
    });
#ifdef PLO_WAVE_PROFILE
    if (err >= 0 && getenv("PLO_WAVE_STATS")) {
        unsigned long long g[12] = {0};
        if (hipMemcpyFromSymbol(g, HIP_SYMBOL(plo::g_wprof), sizeof g) == hipSuccess && g[9])
            fprintf(stderr, "# wave kernel, cumulative: %llu candidates, %.1f steps each; cycles per step: max scan %.0f, tie list %.0f, tie pick %.0f, sweep 1 %.0f, sweep 2 %.0f, tail %.0f; sweep 1 trips per step %.2f, per trip: loads + ballots + broadcasts %.0f, retirements %.0f\n",
                    g[9], (double)g[8] / g[9], (double)g[0] / g[8], (double)g[1] / g[8], (double)g[2] / g[8], (double)g[3] / g[8], (double)g[4] / g[8], (double)g[5] / g[8], (double)g[11] / g[8], g[11] ? (double)g[6] / g[11] : 0.0, g[11] ? (double)g[7] / g[11] : 0.0);
    }
#endif
    return err;        // >0: device error word
}

int device_error(int err) {
    switch (err) {
    case plo::ERR_MULT:  return fail(PLO_E_INTERNAL, "device: multiplier list overflow");
    case plo::ERR_STEPS: return fail(PLO_E_INTERNAL, "device: more CSE steps than the column bound");
    case plo::ERR_PGEN:  return fail(PLO_E_UNSUPPORTED, "device: ProgramGen for non +-1 coefficients not available in this build");
    case plo::ERR_QVAL:  return fail(PLO_E_UNSUPPORTED, "device: a candidate met a value outside the universe of the plan over Q");
    case plo::ERR_KDEC:  return fail(PLO_E_INTERNAL, "device: nullspace decomposition inconsistent with the rank found on the host");
    default:             return fail(PLO_E_INTERNAL, "device: pair table inconsistency");
    }
}

// Twice the slots for a plan whose launch met a full table.  The rule of every repeat: a table that no longer fits (LDS, 65536 slots) is refused with PLO_E_CAPACITY
// and the plan KEEPS THE TABLE THAT RAN -- build_plan clears the plan it fails on, and the next call would launch that, so the plan is built again with the slots it had.
int grow_plan(plo_plan *pl)
{
    pl->cap_scale *= 2;
    const int rc = build_plan(pl);
    if (rc != PLO_E_CAPACITY) return rc;
    const std::string why = g_err;
    pl->cap_scale /= 2;
    const int back = build_plan(pl);
    if (back != PLO_OK) return back;
    return fail(PLO_E_CAPACITY, "pair table full, and with twice the slots: " + why);
}

// Before a launch is repeated with larger tables: the candidates that the refused launch finished have left their words in the job's best word, and the repeat evaluates them again
int reset_best(const plo::WaveJob &J, unsigned long long *d_best) {
    if (J.best) HIPCHK(hipMemsetAsync(d_best, 0xFF, sizeof(unsigned long long), g_stream));
    return PLO_OK;
}
// run a job, growing the pair table when the device reports it full
int run_job(plo_plan *pl, plo::WaveJob J, plo_stats_t *st)
{
    for (int attempt = 0; attempt < 4; ++attempt) {
        const int err = launch(pl, J, st);
        if (err <= 0) return err;
        if (err != plo::ERR_TABLE) return device_error(err);
        int rc = grow_plan(pl);                   // table full: re-plan with twice the slots and retry
        if (rc != PLO_OK) return rc;
        if ((rc = reset_best(J, pl->d_best)) != PLO_OK) return rc;
    }
    return device_error(plo::ERR_TABLE);
}

// a job of random-restart candidates on the plan's own kernel family
int run_plan_job(plo_plan *pl, uint64_t seed0, const uint64_t *seeds, uint64_t n, uint32_t *adds, uint32_t *muls, unsigned long long *best, int cost_mode, plo_stats_t *st)
{
    if (pl->big) {
        plo::BigJob J{}; J.seed0 = seed0; J.seeds = seeds; J.ncand = n; J.adds = adds; J.muls = muls; J.best = best; J.cost_mode = (uint32_t)cost_mode;
        return launch_big(pl, J, st);
    }
    plo::WaveJob J{}; J.seed0 = seed0; J.seeds = seeds; J.ncand = n; J.adds = adds; J.muls = muls; J.best = best; J.cost_mode = (uint32_t)cost_mode;
    return run_job(pl, J, st);
}

// the entries that take a matrix: a plan for the one call
template <class Call> int with_plan(const plo_csr_t *A, uint32_t p, Call call) {
    plo_plan_t *pl = nullptr;
    int rc = plo_cse_plan_create(A, p, &pl);
    if (rc != PLO_OK) return rc;
    rc = call(pl);
    plo_cse_plan_destroy(pl);
    return rc;
}

} // namespace

// Two prepared matrices evaluated back to back per candidate with one random stream (LU method)
struct plo_chain {
    plo_plan *st[2] = {nullptr, nullptr};
    uint32_t W = 1, lds = 0, blocks_per_cu = 1;
};

namespace {
int chain_config(plo_chain *ch)
{
    const plo::WavePlan &A = ch->st[0]->P, &B = ch->st[1]->P;
    const uint32_t region = std::max(A.region_bytes, B.region_bytes), fixed = A.rs_bytes + B.rs_bytes;
    if (fixed + region > g_lds_max) return fail(PLO_E_CAPACITY, "chained candidate state does not fit LDS");
    ch->W = pick_waves([&](uint32_t w) { return fixed + w * region; }, true, g_lds_max, &ch->lds);
    return occupancy_for((const void *)plo::cse_chain_kernel, ch->W, ch->lds, &ch->blocks_per_cu);
}

// run a job, growing the pair tables when the device reports one full (run_job for two plans)
int run_chain(plo_chain *ch, plo::WaveJob J, plo_stats_t *st)
{
    plo_plan *p0 = ch->st[0];
    bool stuck = false;                           // one of the two tables could not be doubled
    J.err = p0->d_err;
    for (int attempt = 0; attempt < 4; ++attempt) {
        const uint64_t grid = grid_for(J.ncand, ch->W, (uint64_t)g_cus * ch->blocks_per_cu);
        const int err = checked_launch(p0->d_err, st, LaunchShape{grid, ch->lds, ch->W, ch->st[0]->algo_bytes + ch->st[1]->algo_bytes},
                                       [&] { hipLaunchKernelGGL(plo::cse_chain_kernel, dim3((uint32_t)grid), dim3(ch->W * 64), ch->lds, g_stream, ch->st[0]->P, ch->st[1]->P, J); });
        if (err <= 0) return err;
        if (err != plo::ERR_TABLE) return device_error(err);
        // The rule of a chain: the error word does not say whose table was full, so BOTH get twice the slots (grow_plan); one that no longer fits then
        // keeps its table (the full one may be the other's), and the launch is refused only when neither can grow or the table stays full
        bool grew[2] = {false, false};
        for (int k = 0; k < 2; ++k) {
            const int rc = grow_plan(ch->st[k]);
            if (rc == PLO_OK) grew[k] = true; else if (rc == PLO_E_CAPACITY) stuck = true; else return rc;
        }
        if (!grew[0] && !grew[1]) return PLO_E_CAPACITY;
        int rc = chain_config(ch);
        if (rc != PLO_OK) {                       // the grown images do not fit together: back to the tables that ran, the chain stays usable
            const std::string why = g_err;
            for (int k = 0; k < 2; ++k)
                if (grew[k]) { ch->st[k]->cap_scale /= 2; const int back = build_plan(ch->st[k]); if (back != PLO_OK) return back; }
            const int back = chain_config(ch); if (back != PLO_OK) return back;
            return fail(rc, "pair table full, and with twice the slots: " + why);
        }
        if ((rc = reset_best(J, p0->d_best)) != PLO_OK) return rc;
    }
    if (stuck) return fail(PLO_E_CAPACITY, "pair table full, and twice the slots do not fit the LDS-resident wave kernel");
    return device_error(plo::ERR_TABLE);
}

// One attempt of a one-shot wave search (plo_cse_chain_batch, plo_kernel_search): the error and best words and, where the caller wants them, adds and muls of every candidate;
// occupancy and grid of kernel `fn` with W waves and `lds` bytes; launch(grid, J); then the results copied back, the best word decoded as a sum-only key may be (the sum in
// .adds).  *again: a pair table was full and nothing was copied -- the caller builds larger tables and calls again.
template <class Launch> int one_shot_search(const void *fn, uint32_t W, uint32_t lds, uint64_t seed0, uint64_t ncand, int cost_mode,
                                            uint32_t *adds, uint32_t *muls, plo_best_t *best, plo_stats_t *st, bool *again, Launch launch) {
    DevBuf<uint32_t> d_adds, d_muls, d_err; DevBuf<unsigned long long> d_best;
    HIPCHK(hipMalloc((void **)&d_err.p, 4));
    HIPCHK(hipMalloc((void **)&d_best.p, 8)); HIPCHK(hipMemsetAsync(d_best, 0xFF, 8, g_stream));
    if (adds) HIPCHK(hipMalloc((void **)&d_adds.p, ncand * 4));
    if (muls) HIPCHK(hipMalloc((void **)&d_muls.p, ncand * 4));
    uint32_t per_cu = 1;
    if (const int rc = occupancy_for(fn, W, lds, &per_cu)) return rc;
    const uint64_t grid = grid_for(ncand, W, (uint64_t)g_cus * per_cu);
    plo::WaveJob J{}; J.seed0 = seed0; J.seeds = nullptr; J.ncand = ncand; J.adds = d_adds; J.muls = d_muls; J.best = best ? d_best.p : nullptr; J.cost_mode = (uint32_t)cost_mode; J.err = d_err;
    const int err = checked_launch(d_err, st, LaunchShape{grid, lds, W, 0}, [&] { launch(grid, J); });
    if (err < 0) return err;
    st->candidates = ncand;
    *again = err == plo::ERR_TABLE;
    if (*again) return PLO_OK;
    if (err) return device_error(err);
    if (adds) HIPCHK(hipMemcpy(adds, d_adds, ncand * 4, hipMemcpyDeviceToHost));
    if (muls) HIPCHK(hipMemcpy(muls, d_muls, ncand * 4, hipMemcpyDeviceToHost));
    if (best) {
        unsigned long long w = 0;
        HIPCHK(hipMemcpy(&w, d_best, 8, hipMemcpyDeviceToHost));
        decode_key(w >> 32, cost_mode, 16u, &best->adds, &best->muls);
        best->seed = seed0 + (w & 0xFFFFFFFFull);
    }
    return PLO_OK;
}
} // namespace

extern "C" {

const char *plo_last_error(void) { return g_err.c_str(); }

int plo_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

int plo_init(int device)
{
    int n = 0;
    hipError_t ce = hipGetDeviceCount(&n);
    if (ce != hipSuccess || n <= 0)
        return fail(PLO_E_HIP, std::string("no HIP device visible (") + hipGetErrorString(ce) + "): libplinopt_hip has no CPU fallback");
    if (device < 0 || device >= n) return fail(PLO_E_ARG, "device ordinal out of range");
    if (g_device == device && g_stream) { HIPCHK(hipSetDevice(device)); return PLO_OK; }      // (the calling thread may have been moved to another device since)
    if (g_device >= 0 && g_device != device) plo_shutdown();          // scratch and stream of the device left behind
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    g_cus = prop.multiProcessorCount;
    g_lds_max = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : prop.sharedMemPerBlock;
    if (g_lds_max > 160u * 1024u) g_lds_max = 160u * 1024u;
    if (g_stream) { (void)hipStreamDestroy(g_stream); g_stream = nullptr; }
    HIPCHK(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    g_device = device;
    return PLO_OK;
}

int plo_shutdown(void)
{
    DevCtx &cx = cur_ctx();
    if (cx.cob_buf) { (void)hipFree(cx.cob_buf); cx.cob_buf = nullptr; cx.cob_words = 0; }
    if (cx.cob_e0) { (void)hipEventDestroy(cx.cob_e0); (void)hipEventDestroy(cx.cob_e1); cx.cob_e0 = cx.cob_e1 = nullptr; }
    if (g_stream) { (void)hipStreamSynchronize(g_stream); (void)hipStreamDestroy(g_stream); g_stream = nullptr; }
    g_device = -1;
    return PLO_OK;
}

int plo_cse_plan_create_ex(const plo_csr_t *A, uint32_t p, uint32_t flags, plo_plan_t **out)
{
    if (!A || !out || !A->rowptr || (A->rowptr[A->m] && (!A->col || !A->val))) return fail(PLO_E_ARG, "null argument");
    if (p < 3 || p >= 0x80000000u || !(p & 1u)) return fail(PLO_E_ARG, "modulus must be an odd prime below 2^31");
    int rc = require_device(NOINIT_DEVICE0);
    if (rc != PLO_OK) return rc;
    if (const char *bad = csr_defect(A, p)) return fail(PLO_E_ARG, bad);
    plo_plan *pl = new plo_plan();
    set_matrix(pl, A, p);
    rc = (flags & PLO_PLAN_HBM) ? PLO_E_CAPACITY : build_plan(pl);
    if (rc == PLO_E_CAPACITY) rc = build_big_plan(pl);       // does not fit LDS: HBM-resident kernel family
    if (rc != PLO_OK) { plo_cse_plan_destroy(pl); return rc; }
    *out = pl;
    return PLO_OK;
}

int plo_cse_plan_create(const plo_csr_t *A, uint32_t p, plo_plan_t **out) { return plo_cse_plan_create_ex(A, p, 0u, out); }

int plo_cse_plan_is_hbm(const plo_plan_t *pl) { return pl && pl->big ? 1 : 0; }

int plo_cse_plan_hbm_counters(const plo_plan_t *pl, uint32_t out[8])
{
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    if (!pl->big || !pl->d_stats) return fail(PLO_E_UNSUPPORTED, "the counters belong to the HBM-resident kernel family");
    uint32_t hs[plo::BS_COUNT];
    HIPCHK(hipMemcpy(hs, pl->d_stats, sizeof hs, hipMemcpyDeviceToHost));
    for (int k = 0; k < 7; ++k) out[k] = hs[plo::BS_SUM_STEPS + k];      // ... BS_SUM_CANDIDATES
    out[7] = pl->big_refits;
    return PLO_OK;
}

// host only, no device: the eager layout of a matrix of the given size (multcap at its bound NCmax, list capacities as build_big_plan sets them)
int plo_cse_hbm_workspace_layout(uint32_t rows, uint32_t nnz, uint32_t ncmax, uint32_t table_bits, uint64_t out[3])
{
    if (!out || table_bits < 10u || table_bits > 30u) return PLO_E_ARG;
    plo::BigPlan B{};
    B.m = rows; B.nnz = nnz; B.NCmax = ncmax; B.multcap = ncmax; B.hbits = table_bits; B.defer = 0u;
    B.dmcap = (uint32_t)std::min<uint64_t>(1u << 20, 1ull << table_bits); B.hlcap = (uint32_t)std::min<uint64_t>(1u << 18, 1ull << table_bits);
    layout_big_workspace(B);
    out[0] = B.o_tab; out[1] = B.ws_stride; out[2] = B.wide;
    return PLO_OK;
}

int plo_cse_plan_hbm_counters_ex(const plo_plan_t *pl, uint32_t *out, uint32_t n)
{
    if (!pl || !out || n > 13u) return fail(PLO_E_ARG, "bad argument");
    uint32_t o[13] = {0};
    const int rc = plo_cse_plan_hbm_counters(pl, o);
    if (rc != PLO_OK) return rc;
    uint32_t hs[plo::BS_COUNT];
    HIPCHK(hipMemcpy(hs, pl->d_stats, sizeof hs, hipMemcpyDeviceToHost));
    o[8] = hs[plo::BS_SUM_EXTRA_WINDOWS]; o[9] = hs[plo::BS_SUM_ROWS_SEARCHED];
    o[10] = hs[plo::BS_SUM_FORCED_MERGES]; o[11] = hs[plo::BS_SUM_MERGE_GROUPS]; o[12] = hs[plo::BS_SUM_MERGE_LOOP];         // the merge: forced by log / hot pressure, groups summed, records loaded behind the prefetch
    for (uint32_t k = 0; k < n; ++k) out[k] = o[k];
    return PLO_OK;
}

// host only, nothing is launched: the choices build_big_plan made for this plan
int plo_cse_plan_hbm_info(const plo_plan_t *pl, uint32_t out[16])
{
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    if (!pl->big) return fail(PLO_E_ARG, "the plan information belongs to the HBM-resident kernel family");
    const plo::BigPlan &B = pl->B;
    const uint32_t o[16] = {B.mode, B.idk, B.defer, B.wide, B.rb, B.kb, B.bb, B.NCmax, B.nv, B.agg_dual, B.agg_cb, B.mers,
                            B.invtab ? 1u : 0u, B.aggbits, B.defer ? B.pbits : 0u, B.hbits};
    for (int k = 0; k < 16; ++k) out[k] = o[k];
    return PLO_OK;
}

int plo_cse_plan_destroy(plo_plan_t *pl)
{
    if (!pl) return PLO_OK;
    dev_free(pl->d_tmpl, pl->d_err, pl->d_best, pl->d_ws, pl->d_next, pl->d_stats);
    for (void *d : pl->big_bufs) (void)hipFree(d);
    delete pl;
    return PLO_OK;
}

uint64_t plo_pack_cost(uint32_t adds, uint32_t muls, int cost_mode, uint32_t seed_off)
{
    uint32_t key;
    switch (cost_mode) {
    case PLO_COST_ADD_THEN_MUL: key = (adds << 16) | muls; break;
    case PLO_COST_SUM:          key = (adds + muls) << 16; break;
    default:                    key = ((adds + muls) << 16) | adds; break;
    }
    return ((uint64_t)key << 32) | seed_off;
}

int plo_cse_cost_many_plan(plo_plan_t *pl, const uint64_t *seeds, uint64_t seed0, uint64_t n,
                           uint32_t *adds, uint32_t *muls, plo_stats_t *st)
{
    if (!pl || !adds || !muls) return fail(PLO_E_ARG, "null argument");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    CallScope call(st); st = call.st;
    if (n == 0) return PLO_OK;                                                   // (`seconds` stays 0)
    return call.done(cse_cost_many_run(n, seeds, adds, muls, nullptr, st, [&](uint32_t *d_adds, uint32_t *d_muls, uint64_t *d_seeds) {
        return run_plan_job(pl, seed0, d_seeds, n, d_adds, d_muls, nullptr, 0, st);
    }));
}

int plo_cse_cost_many(const plo_csr_t *A, uint32_t p, const uint64_t *seeds, uint64_t seed0, uint64_t n, uint32_t *adds, uint32_t *muls)
{
    return with_plan(A, p, [&](plo_plan_t *pl) { return plo_cse_cost_many_plan(pl, seeds, seed0, n, adds, muls, nullptr); });
}

int plo_cse_search_plan(plo_plan_t *pl, uint64_t seed0, uint64_t nseeds, int cost_mode,
                        plo_best_t *out, plo_stats_t *st)
{
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    CallScope call(st); st = call.st;
    out->adds = out->muls = 0xFFFFFFFFu; out->seed = ~0ull;
    uint64_t bkey = ~0ull, bseed = ~0ull;
    const bool big = pl->big;             // the 64-bit cost word of the HBM variant: 20-bit fields over 24-bit seed offsets; 16 over 32 otherwise
    int rc = chunked_min(pl->d_best, seed0, nseeds, big ? 1ull << 24 : 0xFFFFFFFFull, big ? 24u : 32u, &bkey, &bseed, [&](uint64_t s0, uint64_t cnt) {
        return run_plan_job(pl, s0, nullptr, cnt, nullptr, nullptr, pl->d_best, cost_mode, st);
    });
    if (rc != PLO_OK) return rc;
    if (nseeds) {
        uint32_t a = 0, mu = 0;
        if (!decode_key(bkey, cost_mode, big ? 20u : 16u, &a, &mu)) {
            plo_stats_t s2{};                                                // sum-only key: ask the device for the split
            rc = plo_cse_cost_many_plan(pl, &bseed, 0, 1, &a, &mu, &s2);
            if (rc != PLO_OK) return rc;
            if (!big && (plo_pack_cost(a, mu, cost_mode, 0) >> 32) != bkey) return fail(PLO_E_INTERNAL, "winner cost does not match the reduced key");
        }
        out->adds = a; out->muls = mu; out->seed = bseed;
    }
    st->candidates = nseeds;
    return call.done(PLO_OK);
}

// -E: the schedule space of RecSub walked by index (PickState in plo_cse_wave.hip).  LDS-resident plans only.
int plo_cse_enum_cost_many_plan(plo_plan_t *pl, uint64_t first, uint64_t n, uint32_t *adds, uint32_t *muls, uint64_t *prods, plo_stats_t *st)
{
    if (!pl || !adds || !muls) return fail(PLO_E_ARG, "null argument");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    if (pl->big) return fail(PLO_E_UNSUPPORTED, "schedule enumeration is for matrices of the LDS-resident kernel (the tree of anything larger cannot be walked)");
    if (pl->q) return fail(PLO_E_UNSUPPORTED, "schedule enumeration over Q is not built: plans of plo_cse_plan_create_q take the restart searches only");
    CallScope call(st); st = call.st;
    if (n == 0) return PLO_OK;                                                   // (`seconds` stays 0)
    if (n > 0xFFFFFFFFull) return fail(PLO_E_ARG, "at most 2^32-1 schedules per call");
    return call.done(cse_cost_many_run(n, nullptr, adds, muls, prods, st, [&](uint32_t *d_adds, uint32_t *d_muls, uint64_t *d_prods) {
        plo::WaveJob J{}; J.seed0 = first; J.seeds = nullptr; J.ncand = n; J.adds = d_adds; J.muls = d_muls; J.best = nullptr; J.cost_mode = 0;
        J.enumerate = 1u; J.prods = (unsigned long long *)d_prods; J.prodmax = nullptr;
        return run_job(pl, J, st);
    }));
}

int plo_cse_enum_search_plan(plo_plan_t *pl, uint64_t first, uint64_t count, int cost_mode, plo_best_t *out, uint64_t *maxprod, plo_stats_t *st)
{
    if (!pl || !out || !maxprod) return fail(PLO_E_ARG, "null argument");
    if (cost_mode != PLO_COST_SUM_THEN_ADD && cost_mode != PLO_COST_ADD_THEN_MUL && cost_mode != PLO_COST_RECSUB) return fail(PLO_E_ARG, "cost mode 0, 1 or 3");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    if (pl->big) return fail(PLO_E_UNSUPPORTED, "schedule enumeration is for matrices of the LDS-resident kernel (the tree of anything larger cannot be walked)");
    if (pl->q) return fail(PLO_E_UNSUPPORTED, "schedule enumeration over Q is not built: plans of plo_cse_plan_create_q take the restart searches only");
    CallScope call(st); st = call.st;
    out->adds = out->muls = 0xFFFFFFFFu; out->seed = ~0ull; *maxprod = 0;
    DevBuf<unsigned long long> d_pm;
    HIPCHK(hipMalloc((void **)&d_pm.p, sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(d_pm, 0, sizeof(unsigned long long), g_stream));
    uint64_t bkey = ~0ull, bidx = ~0ull;
    const int rc = chunked_min(pl->d_best, first, count, 0xFFFFFFFFull, 32, &bkey, &bidx, [&](uint64_t s0, uint64_t cnt) {
        plo::WaveJob J{}; J.seed0 = s0; J.seeds = nullptr; J.ncand = cnt; J.best = pl->d_best; J.cost_mode = (uint32_t)cost_mode;
        J.enumerate = 1u; J.prodmax = d_pm;
        return run_job(pl, J, st);
    });
    if (rc != PLO_OK) return rc;
    unsigned long long pm = 0;
    HIPCHK(hipMemcpy(&pm, d_pm, sizeof pm, hipMemcpyDeviceToHost));
    if (count) { decode_key(bkey, cost_mode, 16u, &out->adds, &out->muls); out->seed = bidx; }
    *maxprod = pm;
    st->candidates = count;
    return call.done(PLO_OK);
}

int plo_cse_search(const plo_csr_t *A, uint32_t p, uint64_t seed0, uint64_t nseeds, int cost_mode, plo_best_t *out, plo_stats_t *stats)
{
    return with_plan(A, p, [&](plo_plan_t *pl) { return plo_cse_search_plan(pl, seed0, nseeds, cost_mode, out, stats); });
}

} // extern "C" (the helpers below are C++)
// ---- one process, N devices -------------------------------------------------------------------------------------------
// The restart range in `ndev` contiguous shards, one host thread and one device per shard (thread-local device contexts); the
// minimum under (cost key, seed) by RCCL MIN all-reduces over a communicator of the devices.  Shared by plo_cse_search_multi,
// plo_kernel_search_multi and plo_tril_search_multi (below, behind the single-device entries they call).
namespace {
// RCCL, loaded at run time (librccl.so.1 of the ROCm installation; no link-time dependency).
struct Rccl {
    typedef void *comm_t;
    int (*CommInitAll)(comm_t *, int, const int *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, comm_t, hipStream_t) = nullptr;
    int (*CommDestroy)(comm_t) = nullptr;
    int (*GroupStart)() = nullptr; int (*GroupEnd)() = nullptr;
    bool ok = false;
    Rccl() {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL); if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL); if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        CommInitAll = (decltype(CommInitAll))dlsym(h, "ncclCommInitAll"); AllReduce = (decltype(AllReduce))dlsym(h, "ncclAllReduce");
        CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy"); GroupStart = (decltype(GroupStart))dlsym(h, "ncclGroupStart"); GroupEnd = (decltype(GroupEnd))dlsym(h, "ncclGroupEnd");
        ok = CommInitAll && AllReduce && CommDestroy && GroupStart && GroupEnd;
    }
};
Rccl &rccl() { static Rccl r; return r; }
enum { RCCL_UINT64 = 5, RCCL_MIN = 3 };      // ncclUint64, ncclMin of rccl/rccl.h

// The calling thread's current device is put back when a multi-device entry returns (the all-reduce walks the devices with
// hipSetDevice on the caller's thread; the process-wide context of plo_init still names the caller's device and stream).
struct DeviceGuard { int dev = -1; DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; } ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); } };

// One communicator per device set for the life of the process (ncclCommInitAll over 8 GPUs takes seconds: not per call), with a
// stream and a 16-byte buffer per device.  Never destroyed: the HIP runtime may be gone when static destructors run.
struct CommSet { std::vector<Rccl::comm_t> comms; std::vector<hipStream_t> strm; std::vector<unsigned long long *> dbuf; double init_seconds = 0; };
std::mutex g_comm_mu;
std::map<std::vector<int>, CommSet> &comm_cache() { static auto *m = new std::map<std::vector<int>, CommSet>(); return *m; }
uint64_t g_comm_inits = 0;                    // communicators built so far (tests: a second call on the same devices builds none)

CommSet *comm_for(const std::vector<int> &devs, std::string &why)
{
    auto &cache = comm_cache();
    auto it = cache.find(devs);
    if (it != cache.end()) return &it->second;
    Rccl &R = rccl();
    const int n = (int)devs.size();
    CommSet cs; cs.comms.assign((size_t)n, nullptr); cs.strm.assign((size_t)n, nullptr); cs.dbuf.assign((size_t)n, nullptr);
    const auto t0 = std::chrono::steady_clock::now();
    bool good = R.CommInitAll(cs.comms.data(), n, devs.data()) == 0;
    if (!good) why = "ncclCommInitAll failed";
    for (int i = 0; good && i < n; ++i) {
        good = hipSetDevice(devs[(size_t)i]) == hipSuccess && hipStreamCreateWithFlags(&cs.strm[(size_t)i], hipStreamNonBlocking) == hipSuccess &&
               hipMalloc((void **)&cs.dbuf[(size_t)i], 16) == hipSuccess;
        if (!good) why = "device buffer for the all-reduce";
    }
    if (!good) {
        for (int i = 0; i < n; ++i) { if (cs.dbuf[(size_t)i] || cs.strm[(size_t)i]) { (void)hipSetDevice(devs[(size_t)i]); if (cs.dbuf[(size_t)i]) (void)hipFree(cs.dbuf[(size_t)i]); if (cs.strm[(size_t)i]) (void)hipStreamDestroy(cs.strm[(size_t)i]); } if (cs.comms[(size_t)i]) R.CommDestroy(cs.comms[(size_t)i]); }
        return nullptr;
    }
    cs.init_seconds = seconds_since(t0);
    ++g_comm_inits;
    return &(cache[devs] = std::move(cs));
}

// Lexicographic minimum of the devices' (hi, lo) words, left in every w[i]: ONE MIN all-reduce of hi, then one of lo among the
// ranks that hold the minimal hi (the others contribute all ones) -- the two-stage form of plinopt_amd/dist.py allreduce_best, so
// that no cost is too wide for the word.  `seconds` = wall time of the two all-reduces (communicator set-up excluded: it is
// cached).  false when RCCL is not there or a call fails (the caller keeps the host minimum and says so).
bool rccl_min_pair(const std::vector<int> &devs, std::vector<std::array<unsigned long long, 2>> &w, double &seconds, std::string &why)
{
    Rccl &R = rccl();
    if (!R.ok) { why = "librccl not loadable"; return false; }
    std::lock_guard<std::mutex> lk(g_comm_mu);
    CommSet *cs = comm_for(devs, why);
    if (!cs) return false;
    const int n = (int)devs.size();
    const auto t0 = std::chrono::steady_clock::now();
    auto stage = [&](int k) -> bool {                                              // all-reduce of word k of every device
        bool good = true;
        for (int i = 0; good && i < n; ++i) good = hipSetDevice(devs[(size_t)i]) == hipSuccess && hipMemcpyAsync(cs->dbuf[(size_t)i], &w[(size_t)i][(size_t)k], 8, hipMemcpyHostToDevice, cs->strm[(size_t)i]) == hipSuccess;
        if (!good) { why = "upload of the packed word"; return false; }
        R.GroupStart();
        for (int i = 0; i < n; ++i) good = R.AllReduce(cs->dbuf[(size_t)i], cs->dbuf[(size_t)i], 1, RCCL_UINT64, RCCL_MIN, cs->comms[(size_t)i], cs->strm[(size_t)i]) == 0 && good;
        good = (R.GroupEnd() == 0) && good;
        if (!good) { why = "ncclAllReduce failed"; return false; }
        for (int i = 0; good && i < n; ++i) good = hipSetDevice(devs[(size_t)i]) == hipSuccess && hipMemcpyAsync(&w[(size_t)i][(size_t)k], cs->dbuf[(size_t)i], 8, hipMemcpyDeviceToHost, cs->strm[(size_t)i]) == hipSuccess && hipStreamSynchronize(cs->strm[(size_t)i]) == hipSuccess;
        if (!good) why = "reading the reduced word";
        return good;
    };
    std::vector<unsigned long long> hi0((size_t)n);
    for (int i = 0; i < n; ++i) hi0[(size_t)i] = w[(size_t)i][0];
    bool good = stage(0);
    if (good) { for (int i = 0; i < n; ++i) if (hi0[(size_t)i] != w[(size_t)i][0]) w[(size_t)i][1] = ~0ull; good = stage(1); }
    seconds = seconds_since(t0);
    return good;
}

// what a shard hands back: its best candidate as a (hi, lo) word pair ordered like the search's total order
struct MultiShard { int rc = PLO_OK; std::string msg; uint64_t s0 = 0, cnt = 0; plo_stats_t st{}; unsigned long long hi = ~0ull, lo = ~0ull; };

// body(shard, device ordinal) runs on its own host thread with its own device context, between plo_init and plo_shutdown
int multi_run(int ndev, const int *devices, uint64_t seed0, uint64_t nseeds, std::vector<MultiShard> &sh, const std::function<int(MultiShard &, int)> &body)
{
    sh.assign((size_t)ndev, MultiShard{});
    std::vector<std::thread> th;
    for (int r = 0; r < ndev; ++r) th.emplace_back([&, r]() {
        MultiShard &S = sh[(size_t)r];
        const uint64_t q = nseeds / (uint64_t)ndev, rem = nseeds % (uint64_t)ndev;                // the same blocks as the forked shards of the tools
        S.s0 = seed0 + (uint64_t)r * q + std::min<uint64_t>((uint64_t)r, rem); S.cnt = q + ((uint64_t)r < rem ? 1 : 0);
        if (S.cnt == 0) return;
        const int dev = devices ? devices[r] : r;
        DevCtx ctx; t_ctx = &ctx;                                                                 // this thread's device, stream and limits
        S.rc = plo_init(dev);
        if (S.rc == PLO_OK) S.rc = body(S, dev);
        if (S.rc != PLO_OK) S.msg = "device " + std::to_string(dev) + ": " + g_err;
        plo_shutdown();
        t_ctx = nullptr;
    });
    for (auto &t : th) t.join();
    // a refusal (PLO_E_CAPACITY / PLO_E_UNSUPPORTED) is reported as such when every failed shard says so: the caller may fall back
    for (auto &S : sh) if (S.rc != PLO_OK && S.rc != PLO_E_CAPACITY && S.rc != PLO_E_UNSUPPORTED) return fail(S.rc, S.msg);
    for (auto &S : sh) if (S.rc != PLO_OK) return fail(S.rc, S.msg);
    return PLO_OK;
}

// The minimum of the shards' words, taken on the host: that is the result.  With two or more DISTINCT devices (PLO_MULTI_REDUCE=rccl:
// also for one; =host: never) rccl_min_pair over the devices cross-checks it; a difference is a diagnostic on stderr and clears
// agg.reduce (never an error: the host value is right by construction).
// `winner` gets the winning shard (-1: no shard has a candidate); agg the summed statistics, `reduce` and the all-reduce time.
int multi_min(const std::vector<MultiShard> &sh, int ndev, const int *devices, plo_stats_t &agg, int &winner)
{
    winner = -1;
    agg = plo_stats_t{};
    for (size_t r = 0; r < sh.size(); ++r) {
        const MultiShard &S = sh[r];
        if (S.cnt == 0) continue;
        agg.candidates += S.st.candidates; agg.launches += S.st.launches; agg.kernel_ms = std::max(agg.kernel_ms, S.st.kernel_ms);
        agg.grid = S.st.grid; agg.lds_bytes = S.st.lds_bytes; agg.waves_per_wg = S.st.waves_per_wg; agg.algo_bytes = S.st.algo_bytes;
        if (S.hi == ~0ull && S.lo == ~0ull) continue;
        if (winner < 0 || S.hi < sh[(size_t)winner].hi || (S.hi == sh[(size_t)winner].hi && S.lo < sh[(size_t)winner].lo)) winner = (int)r;
    }
    const char *mode = getenv("PLO_MULTI_REDUCE");
    const bool want = mode ? !strcmp(mode, "rccl") : ndev >= 2;
    if (!want || winner < 0) return PLO_OK;
    std::vector<int> devs; std::vector<std::array<unsigned long long, 2>> words;
    for (int r = 0; r < ndev; ++r) { devs.push_back(devices ? devices[r] : r); words.push_back({sh[(size_t)r].hi, sh[(size_t)r].lo}); }
    bool distinct = true; for (size_t i = 0; i < devs.size(); ++i) for (size_t j = 0; j < i; ++j) distinct = distinct && devs[i] != devs[j];
    if (!distinct) return PLO_OK;                                                  // (a communicator needs distinct devices: PLO_GPU_DEVICES=0,0 in the tests)
    std::string why; double secs = 0;
    if (rccl_min_pair(devs, words, secs, why)) {
        agg.reduce = 1; agg.reduce_seconds = secs;
        for (auto &w : words) if (w[0] != sh[(size_t)winner].hi || w[1] != sh[(size_t)winner].lo) {
            fprintf(stderr, "# libplinopt_hip: RCCL MIN all-reduce gave (%llx, %llx), the host minimum is (%llx, %llx): host minimum kept\n", w[0], w[1], sh[(size_t)winner].hi, sh[(size_t)winner].lo);
            agg.reduce = 0; break;
        }
    } else if (mode) return fail(PLO_E_HIP, std::string("PLO_MULTI_REDUCE=rccl: ") + why);
    return PLO_OK;
}

// A restart search sharded over devices, for the searches that prepare a plan: every shard creates its plan, searches its block of
// seeds and destroys the plan; the winner is the minimum of the shards' bests under key(best), the search's own total order as a
// (hi, lo) word pair.  (A launch takes at most 2^31-1 candidates: longer shards go in pieces, minimum under the same order.)
template <class Plan, class Best, class Create, class Key>
int sharded_search(uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, Best *best, plo_stats_t *stats, Create create,
                   int (*search)(Plan *, uint64_t, uint64_t, Best *, plo_stats_t *), void (*destroy)(Plan *), Key key)
{
    if (ndev < 1 || ndev > 64) return fail(PLO_E_ARG, "device count outside [1,64]");
    if (nseeds == 0 || nseeds >= (1ull << 62)) return fail(PLO_E_ARG, "1 .. 2^62-1 candidates per call");
    DeviceGuard guard;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<MultiShard> sh; std::vector<Best> bests((size_t)ndev);
    int rc = multi_run(ndev, devices, seed0, nseeds, sh, [&](MultiShard &S, int) {
        Best &b = bests[(size_t)(&S - sh.data())];
        Plan *plan = nullptr;
        int r_ = create(&plan);
        if (r_ != PLO_OK) return r_;
        bool have = false;
        for (uint64_t done = 0; r_ == PLO_OK && done < S.cnt;) {
            const uint64_t piece = std::min<uint64_t>(S.cnt - done, (1ull << 31) - 1ull);
            Best pb{}; plo_stats_t ps{};
            r_ = search(plan, S.s0 + done, piece, &pb, &ps);
            if (r_ != PLO_OK) break;
            S.st.candidates += ps.candidates; S.st.launches += ps.launches; S.st.kernel_ms += ps.kernel_ms; S.st.grid = ps.grid; S.st.lds_bytes = ps.lds_bytes; S.st.waves_per_wg = ps.waves_per_wg; S.st.algo_bytes = ps.algo_bytes;
            const unsigned long long hi = key(pb).first, lo = key(pb).second;
            if (!have || hi < S.hi || (hi == S.hi && lo < S.lo)) { S.hi = hi; S.lo = lo; b = pb; have = true; }
            done += piece;
        }
        destroy(plan);
        return r_;
    });
    if (rc != PLO_OK) return rc;
    plo_stats_t agg{}; int win = -1;
    rc = multi_min(sh, ndev, devices, agg, win);
    if (rc != PLO_OK) return rc;
    if (win < 0) return fail(PLO_E_INTERNAL, "no candidate reported");
    *best = bests[(size_t)win];
    agg.seconds = seconds_since(t0);
    if (stats) *stats = agg;
    return PLO_OK;
}

// The same for the searches without a plan (plo_cse_search_multi, plo_kernel_search_multi): shard(first seed, count, best, stats) is
// the single-device entry on a shard's block; the winner is the minimum under (cmpOpCount key of `cost_mode`, seed).  No candidate
// at all is no error here: *out then holds all ones.
template <class Shard>
int planless_search_multi(uint64_t seed0, uint64_t nseeds, int cost_mode, int ndev, const int *devices, plo_best_t *out, plo_stats_t *stats, Shard shard)
{
    DeviceGuard guard;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<MultiShard> sh; std::vector<plo_best_t> bests((size_t)ndev);
    auto key = [&](const plo_best_t &b) -> unsigned long long {                                   // cmpOpCount orders of plinopt_optimize.h:53-64
        switch (cost_mode) { case PLO_COST_ADD_THEN_MUL: return ((unsigned long long)b.adds << 32) | b.muls; case PLO_COST_SUM: return ((unsigned long long)b.adds + b.muls) << 32; default: return (((unsigned long long)b.adds + b.muls) << 32) | b.adds; } };
    int rc = multi_run(ndev, devices, seed0, nseeds, sh, [&](MultiShard &S, int) {
        plo_best_t &b = bests[(size_t)(&S - sh.data())];
        const int r_ = shard(S.s0, S.cnt, &b, &S.st);
        if (r_ == PLO_OK && b.seed != ~0ull) { S.hi = key(b); S.lo = b.seed - seed0; }
        return r_;
    });
    if (rc != PLO_OK) return rc;
    plo_stats_t agg{}; int win = -1;
    rc = multi_min(sh, ndev, devices, agg, win);
    if (rc != PLO_OK) return rc;
    out->adds = out->muls = 0xFFFFFFFFu; out->seed = ~0ull;
    if (win >= 0) *out = bests[(size_t)win];
    agg.seconds = seconds_since(t0);
    if (stats) *stats = agg;
    return PLO_OK;
}
} // namespace

extern "C" {

uint64_t plo_multi_comm_inits(void) { return g_comm_inits; }

int plo_cse_search_multi(const plo_csr_t *A, uint32_t p, uint64_t seed0, uint64_t nseeds, int cost_mode, int ndev, const int *devices,
                         plo_best_t *out, plo_stats_t *stats)
{
    if (!A || !out) return fail(PLO_E_ARG, "null argument");
    if (ndev < 1 || ndev > 64) return fail(PLO_E_ARG, "device count outside [1,64]");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    return planless_search_multi(seed0, nseeds, cost_mode, ndev, devices, out, stats,
        [&](uint64_t s0, uint64_t cnt, plo_best_t *b, plo_stats_t *st) { return plo_cse_search(A, p, s0, cnt, cost_mode, b, st); });
}

int plo_cse_chain_destroy(plo_chain_t *ch)
{
    if (!ch) return PLO_OK;
    for (int k = 0; k < 2; ++k) plo_cse_plan_destroy(ch->st[k]);
    delete ch;
    return PLO_OK;
}

int plo_cse_chain_create(const plo_csr_t *first, const plo_csr_t *second, uint32_t p, plo_chain_t **out)
{
    if (!first || !second || !out) return fail(PLO_E_ARG, "null argument");
    plo_chain *ch = new plo_chain();
    int rc = plo_cse_plan_create(first, p, &ch->st[0]);
    if (rc == PLO_OK) rc = plo_cse_plan_create(second, p, &ch->st[1]);
    if (rc == PLO_OK && (ch->st[0]->big || ch->st[1]->big)) rc = fail(PLO_E_CAPACITY, "chained search needs both matrices on the LDS-resident wave kernel");
    if (rc == PLO_OK) rc = chain_config(ch);
    if (rc != PLO_OK) { plo_cse_chain_destroy(ch); return rc; }
    *out = ch;
    return PLO_OK;
}

// Many pairs in one launch (plo::cse_chain_batch_kernel): candidate c = pair c / per_pair, seed seed0 + c.
int plo_cse_chain_batch(uint32_t npairs, const plo_csr_t *firsts, const plo_csr_t *seconds, uint32_t p, uint64_t seed0, uint32_t per_pair,
                        int cost_mode, uint32_t *adds, uint32_t *muls, plo_best_t *best, plo_stats_t *st)
{
    if (!firsts || !seconds || npairs == 0 || per_pair == 0) return fail(PLO_E_ARG, "bad argument");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    if (p < 3 || p >= 0x80000000u || !(p & 1u)) return fail(PLO_E_ARG, "modulus must be an odd prime below 2^31");
    for (uint32_t k = 0; k < npairs; ++k)
        for (const plo_csr_t *A : {&firsts[k], &seconds[k]})
            if (const char *bad = csr_defect(A, p)) return fail(PLO_E_ARG, "pair " + std::to_string(k) + ": " + bad);
    const uint64_t ncand = (uint64_t)npairs * per_pair;
    if (ncand > 0xFFFFFFFFull) return fail(PLO_E_ARG, "at most 2^32-1 candidates per call");
    CallScope call(st); st = call.st;
    if (best) { best->adds = best->muls = 0xFFFFFFFFu; best->seed = ~0ull; }
    std::atomic<bool> stuck{false};                  // some plan could not take twice the slots
    for (uint32_t cap_scale = 2; cap_scale <= 16; cap_scale *= 2) {
        // host part of all plans (OpenMP), one device buffer for all images
        std::vector<plo::WavePlan> plans(2ull * npairs);
        std::vector<std::vector<uint8_t>> imgs(2ull * npairs);
        std::vector<int> rcs(2ull * npairs, PLO_OK); std::vector<std::string> errs(2ull * npairs);
        {   // host threads share the plans out (no OpenMP runtime in this library: the callers bring their own)
            std::atomic<long long> next{0};
            auto work = [&]() {
                for (;;) {
                    const long long k = next.fetch_add(1);
                    if (k >= 2ll * npairs) break;
                    const plo_csr_t *A = (k & 1) ? &seconds[k >> 1] : &firsts[k >> 1];
                    plo_plan tmp;
                    if (!A->rowptr || (A->rowptr[A->m] && (!A->col || !A->val))) { rcs[k] = PLO_E_ARG; errs[k] = "null matrix arrays"; continue; }
                    set_matrix(&tmp, A, p);
                    // the error word does not say whose table was full: a plan that no longer fits with this many slots keeps the
                    // largest table that does (the full one may be another pair's); with the first scale the refusal is the matrix's
                    for (uint32_t s = cap_scale; s >= 2u; s /= 2u) {
                        tmp.cap_scale = s;
                        rcs[k] = build_plan(&tmp, &imgs[k]);
                        if (rcs[k] != PLO_E_CAPACITY) break;
                        if (s == cap_scale) errs[k] = g_err;
                        if (s > 2u) stuck = true;
                    }
                    if (rcs[k] == PLO_OK) plans[k] = tmp.P; else if (rcs[k] != PLO_E_CAPACITY) errs[k] = g_err;
                }
            };
            const unsigned nt = std::max(1u, std::min<unsigned>(std::thread::hardware_concurrency(), std::min<unsigned>(64u, npairs)));
            std::vector<std::thread> pool;
            for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
            work();
            for (auto &th : pool) th.join();
        }
        for (size_t k = 0; k < rcs.size(); ++k) if (rcs[k] != PLO_OK) return fail(rcs[k], "pair " + std::to_string(k >> 1) + ": " + errs[k]);
        uint32_t region = 0, rsmax = 0; size_t total = 0; std::vector<size_t> offs(imgs.size());
        for (size_t k = 0; k < imgs.size(); ++k) { region = std::max(region, plans[k].region_bytes); rsmax = std::max(rsmax, plans[k].rs_bytes); offs[k] = total; total += round_up((uint32_t)imgs[k].size(), 64); }
        uint32_t lds = 0;
        const uint32_t W = pick_waves([&](uint32_t w) { return 64u + w * (2u * rsmax + region); }, false, g_lds_max, &lds);
        if (!W) return fail(PLO_E_CAPACITY, "chained candidate state does not fit LDS");
        DevBuf<uint8_t> d_img; DevBuf<plo::WavePlan> d_plans;
        std::vector<uint8_t> blob(total + 64, 0);
        for (size_t k = 0; k < imgs.size(); ++k) std::memcpy(blob.data() + offs[k], imgs[k].data(), imgs[k].size());
        HIPCHK(hipMalloc((void **)&d_img.p, blob.size()));
        HIPCHK(hipMemcpy(d_img, blob.data(), blob.size(), hipMemcpyHostToDevice));
        for (size_t k = 0; k < plans.size(); ++k) plans[k].tmpl = (const uint64_t *)(d_img + offs[k]);
        HIPCHK(hipMalloc((void **)&d_plans.p, plans.size() * sizeof(plo::WavePlan)));
        HIPCHK(hipMemcpy(d_plans, plans.data(), plans.size() * sizeof(plo::WavePlan), hipMemcpyHostToDevice));
        bool again = false;
        const int rc = one_shot_search((const void *)plo::cse_chain_batch_kernel, W, lds, seed0, ncand, cost_mode, adds, muls, best, st, &again, [&](uint64_t grid, const plo::WaveJob &J) {
            hipLaunchKernelGGL(plo::cse_chain_batch_kernel, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, (const plo::WavePlan *)d_plans, per_pair, region, rsmax, J);
        });
        if (rc != PLO_OK) return rc;
        if (again) continue;                                                         // a pair table filled up: all plans again with twice the slots
        return call.done(PLO_OK);
    }
    if (stuck) return fail(PLO_E_CAPACITY, "pair table full, and twice the slots do not fit the LDS-resident wave kernel");
    return device_error(plo::ERR_TABLE);
}

} // extern "C"
namespace {
// Host side of one problem of plo_cse_batch_search: its one or two plans and images at the table scale they were last built with
struct BatchSlot {
    uint32_t scale = 2;                  // cap_scale asked for (2, 4, 8, 16: the growth rule of plo_cse_chain_batch, per problem)
    uint32_t got[2] = {0, 0};            // the scale each plan took (one that no longer fits twice the slots keeps the largest table that does)
    plo::WavePlan P[2]{};
    std::vector<uint8_t> img[2];
    int rc = PLO_OK; std::string why;
    uint32_t foot = 0;                   // LDS bytes of the problem beside the reduction scratch, with one wave: row starts + one region
};
// Buckets of plo_cse_batch_search by that footprint: up to 4, 8, 16, 32, 64 KiB and the rest of the LDS
constexpr uint32_t BATCH_BUCKETS = 6;
uint32_t batch_bucket(uint32_t foot) { uint32_t b = 0; while (b + 1 < BATCH_BUCKETS && foot > (4096u << b)) ++b; return b; }
// Waves per workgroup of the batch kernels: 8, 4, 2 or 1, the most whose need(w) bytes fit the LDS -- the waves of a workgroup are all the parallelism one problem
// gets -- and no more than twice its candidates
template <class Need> uint32_t batch_waves(Need need, uint32_t per_problem, size_t lds_max) {
    uint32_t W = 8;
    while (W > 1u && (need(W) > lds_max || W / 2u >= per_problem)) W /= 2u;
    return W;
}

// fn(k) for 0 <= k < n on host threads (no OpenMP runtime in this library: the callers bring their own)
template <class Fn> void on_host_threads(size_t n, Fn fn) {
    std::atomic<size_t> next{0};
    auto work = [&]() { for (;;) { const size_t k = next.fetch_add(1); if (k >= n) break; fn(k); } };
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), (size_t)64, n}));
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
}

// the plans of one problem at S.scale; S.rc / S.why: the refusal of the wave kernel, if any
void batch_build(BatchSlot &S, const plo_csr_t *first, const plo_csr_t *second, uint32_t p, size_t lds_max)
{
    const uint32_t prev[2] = {S.got[0], S.got[1]};
    const int nmat = second ? 2 : 1;
    S.rc = PLO_OK; S.why.clear();
    for (int k = 0; k < nmat; ++k) {
        plo_plan tmp;
        set_matrix(&tmp, k ? second : first, p);
        int rc = PLO_E_CAPACITY;
        for (uint32_t s = S.scale; s >= 2u; s /= 2u) {
            tmp.cap_scale = s;
            rc = build_plan(&tmp, &S.img[k]);
            if (rc != PLO_E_CAPACITY) { S.got[k] = s; break; }
            if (s == S.scale) S.why = g_err;
        }
        if (rc != PLO_OK) { S.rc = rc; if (rc != PLO_E_CAPACITY) S.why = g_err; return; }
        S.P[k] = tmp.P;
    }
    if (prev[0] && S.got[0] == prev[0] && S.got[1] == prev[1]) { S.rc = PLO_E_CAPACITY; S.why = "pair table full, and with twice the slots: " + S.why; return; }
    const uint32_t region = nmat == 2 ? std::max(S.P[0].region_bytes, S.P[1].region_bytes) : S.P[0].region_bytes;
    S.foot = S.P[0].rs_bytes + (nmat == 2 ? S.P[1].rs_bytes : 0u) + region;
    if (64ull + S.foot > lds_max) { S.rc = PLO_E_CAPACITY; S.why = "candidate state does not fit the 160 KiB LDS of one CU"; }
}
} // namespace
extern "C" {

// Many restart searches in one call, one minimum each (plo::cse_batch_kernel, one workgroup per problem).
int plo_cse_batch_search(uint32_t nprob, const plo_csr_t *firsts, const plo_csr_t *seconds, uint32_t p, uint64_t seed0,
                         uint32_t per_problem, int cost_mode, plo_best_t *bests, int32_t *status, plo_stats_t *st)
{
    if (!firsts || !bests || !status || nprob == 0 || per_problem == 0) return fail(PLO_E_ARG, "bad argument");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    if (p < 3 || p >= 0x80000000u || !(p & 1u)) return fail(PLO_E_ARG, "modulus must be an odd prime below 2^31");
    if ((uint64_t)nprob * per_problem > 0xFFFFFFFFull) return fail(PLO_E_ARG, "at most 2^32-1 candidates per call");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    for (uint32_t q = 0; q < nprob; ++q) {
        if (const char *bad = csr_defect(&firsts[q], p)) return fail(PLO_E_ARG, "problem " + std::to_string(q) + ": " + bad);
        if (seconds) if (const char *bad = csr_defect(&seconds[q], p)) return fail(PLO_E_ARG, "problem " + std::to_string(q) + ", second matrix: " + bad);
    }
    CallScope call(st); st = call.st;
    for (uint32_t q = 0; q < nprob; ++q) { bests[q].adds = bests[q].muls = 0xFFFFFFFFu; bests[q].seed = ~0ull; status[q] = PLO_OK; }
    const std::optional<long> grid_cap = env_knob("PLO_BATCH_GRID");           // test knob: one workgroup can be made to take many problems in turn
    const bool batch_stats = env_knob("PLO_BATCH_STATS").has_value();          // a '#' line per launch on stderr (the measurements of DESIGN.md 2.11)
    const size_t lds_max = g_lds_max;
    DevBuf<unsigned long long> d_keys; DevBuf<uint32_t> d_adds, d_muls, d_err;
    HIPCHK(hipMalloc((void **)&d_keys.p, nprob * 8ull)); HIPCHK(hipMalloc((void **)&d_adds.p, nprob * 4ull));
    HIPCHK(hipMalloc((void **)&d_muls.p, nprob * 4ull)); HIPCHK(hipMalloc((void **)&d_err.p, nprob * 4ull));
    HIPCHK(hipMemsetAsync(d_keys, 0xFF, nprob * 8ull, g_stream));
    std::vector<BatchSlot> S(nprob);
    std::vector<uint32_t> todo(nprob), err(nprob);
    for (uint32_t q = 0; q < nprob; ++q) todo[q] = q;
    while (!todo.empty()) {
        on_host_threads(todo.size(), [&](size_t k) { const uint32_t q = todo[k]; batch_build(S[q], &firsts[q], seconds ? &seconds[q] : nullptr, p, lds_max); });
        std::vector<uint32_t> live[BATCH_BUCKETS];
        size_t total = 0, nlive = 0;
        for (const uint32_t q : todo) {
            if (S[q].rc == PLO_E_CAPACITY || S[q].rc == PLO_E_UNSUPPORTED) { status[q] = S[q].rc; continue; }     // the wave kernel refuses this problem alone
            if (S[q].rc != PLO_OK) return fail(S[q].rc, "problem " + std::to_string(q) + ": " + S[q].why);
            live[batch_bucket(S[q].foot)].push_back(q); ++nlive;
            for (int k = 0; k < (seconds ? 2 : 1); ++k) total += round_up((uint32_t)S[q].img[k].size(), 64);
        }
        if (!nlive) break;
        // one device buffer for all images, one array of problems in bucket order
        std::vector<uint8_t> blob(total + 64, 0);
        std::vector<plo::BatchProb> probs; probs.reserve(nlive);
        DevBuf<uint8_t> d_img; DevBuf<plo::BatchProb> d_probs;
        HIPCHK(hipMalloc((void **)&d_img.p, blob.size()));
        size_t off = 0;
        for (const auto &bucket : live)
            for (const uint32_t q : bucket) {
                plo::BatchProb B{}; B.q = q; B.chained = seconds ? 1u : 0u;
                for (int k = 0; k < (seconds ? 2 : 1); ++k) {
                    std::memcpy(blob.data() + off, S[q].img[k].data(), S[q].img[k].size());
                    (k ? B.P2 : B.P1) = S[q].P[k];
                    (k ? B.P2 : B.P1).tmpl = (const uint64_t *)(d_img.p + off);
                    off += round_up((uint32_t)S[q].img[k].size(), 64);
                }
                probs.push_back(B);
            }
        HIPCHK(hipMemcpy(d_img, blob.data(), blob.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc((void **)&d_probs.p, probs.size() * sizeof(plo::BatchProb)));
        HIPCHK(hipMemcpy(d_probs, probs.data(), probs.size() * sizeof(plo::BatchProb), hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(d_err, 0, nprob * 4ull, g_stream));
        size_t first = 0;
        for (const auto &bucket : live)
            for (size_t b0 = 0, b1; b0 < bucket.size(); b0 = b1) {
                // One launch takes the problems b0 .. b1-1 of the bucket: all of them, unless the largest row starts and the largest region -- of different
                // problems -- no longer fit the LDS together (only possible for footprints near the LDS: each problem alone fits, batch_build)
                plo::BatchJob J{}; J.probs = d_probs.p + first; J.per = per_problem; J.cost_mode = (uint32_t)cost_mode; J.seed0 = seed0;
                J.keys = d_keys; J.adds = d_adds; J.muls = d_muls; J.err = d_err;
                for (b1 = b0; b1 < bucket.size(); ++b1) {
                    const BatchSlot &X = S[bucket[b1]];
                    const uint32_t r1 = std::max(J.rs1max, X.P[0].rs_bytes), r2 = seconds ? std::max(J.rs2max, X.P[1].rs_bytes) : 0u;
                    const uint32_t rg = std::max(J.region, X.foot - X.P[0].rs_bytes - (seconds ? X.P[1].rs_bytes : 0u));
                    if (b1 > b0 && 64ull + r1 + r2 + rg > lds_max) break;
                    J.rs1max = r1; J.rs2max = r2; J.region = rg;
                }
                const size_t count = b1 - b0;
                J.nprob = (uint32_t)count;
                // Waves per workgroup: batch_waves.  One workgroup per problem, handed out by the hardware as workgroups retire, so that cheap and dear
                // problems balance themselves; the stride loop of the kernel only turns under the grid knob (and past 2^31 - 1 problems).
                const auto need = [&](uint32_t w) { return 64u + J.rs1max + J.rs2max + w * J.region; };
                const uint32_t W = batch_waves(need, per_problem, lds_max);
                const uint32_t lds = need(W);
                uint32_t per_cu = 1;
                if (const int rc = occupancy_for((const void *)plo::cse_batch_kernel, W, lds, &per_cu)) return rc;
                uint64_t grid = std::min<uint64_t>(count, 0x7FFFFFFFull);
                if (grid_cap && *grid_cap > 0) grid = std::min<uint64_t>(grid, (uint64_t)*grid_cap);
                const LaunchShape shape{grid, lds, W, 0};
                const double ms0 = st->kernel_ms;
                if (const int rc = timed_launch(st, &shape, [&] { hipLaunchKernelGGL(plo::cse_batch_kernel, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, J); })) return rc;
                if (batch_stats) fprintf(stderr, "# batch: scale %u, bucket %u: %zu problems, %u waves per workgroup, %u LDS bytes, %u workgroups per CU, grid %llu, %.3f ms\n",
                                         S[bucket[b0]].scale, batch_bucket(S[bucket[b0]].foot), count, W, lds, per_cu, (unsigned long long)grid, st->kernel_ms - ms0);
                st->candidates += (uint64_t)count * per_problem;
                first += count;
            }
        HIPCHK(hipMemcpy(err.data(), d_err, nprob * 4ull, hipMemcpyDeviceToHost));
        // a full pair table is that problem's alone: only those are built again with twice the slots and launched again
        std::vector<uint32_t> next;
        for (const auto &bucket : live)
            for (const uint32_t q : bucket) {
                if (!err[q]) continue;
                if (err[q] != plo::ERR_TABLE) { const int rc = device_error((int)err[q]); return fail(rc, "problem " + std::to_string(q) + ": " + g_err); }
                if (S[q].scale >= 16u) { status[q] = PLO_E_CAPACITY; continue; }
                S[q].scale *= 2u; next.push_back(q);
            }
        todo = std::move(next);
    }
    std::vector<unsigned long long> keys(nprob); std::vector<uint32_t> adds(nprob), muls(nprob);
    HIPCHK(hipMemcpy(keys.data(), d_keys, nprob * 8ull, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(adds.data(), d_adds, nprob * 4ull, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(muls.data(), d_muls, nprob * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < nprob; ++q) {
        if (status[q] != PLO_OK) continue;
        if (keys[q] == ~0ull) return fail(PLO_E_INTERNAL, "problem " + std::to_string(q) + ": no result");
        bests[q].adds = adds[q]; bests[q].muls = muls[q]; bests[q].seed = seed0 + (uint64_t)q * per_problem + (keys[q] & 0xFFFFFFFFull);
    }
    return call.done(PLO_OK);
}

int plo_cse_chain_cost_many(plo_chain_t *ch, const uint64_t *seeds, uint64_t seed0, uint64_t n,
                            uint32_t *adds, uint32_t *muls, plo_stats_t *st)
{
    if (!ch || !adds || !muls) return fail(PLO_E_ARG, "null argument");
    CallScope call(st); st = call.st;                    // (as it was: no check for the device -- a chain exists only with one -- and `seconds` stays 0)
    if (n == 0) return PLO_OK;
    return cse_cost_many_run(n, seeds, adds, muls, nullptr, st, [&](uint32_t *d_adds, uint32_t *d_muls, uint64_t *d_seeds) {
        plo::WaveJob J{}; J.seed0 = seed0; J.seeds = d_seeds; J.ncand = n; J.adds = d_adds; J.muls = d_muls; J.best = nullptr; J.cost_mode = 0;
        return run_chain(ch, J, st);
    });
}

int plo_cse_chain_search(plo_chain_t *ch, uint64_t seed0, uint64_t nseeds, int cost_mode, plo_best_t *out, plo_stats_t *st)
{
    if (!ch || !out) return fail(PLO_E_ARG, "null argument");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    CallScope call(st); st = call.st;                    // (as it was: no check for the device, and `seconds` stays 0)
    out->adds = out->muls = 0xFFFFFFFFu; out->seed = ~0ull;
    uint64_t bkey = ~0ull, bseed = ~0ull;
    unsigned long long *d_best = ch->st[0]->d_best;
    int rc = chunked_min(d_best, seed0, nseeds, 0xFFFFFFFFull, 32, &bkey, &bseed, [&](uint64_t s0, uint64_t cnt) {
        plo::WaveJob J{}; J.seed0 = s0; J.ncand = cnt; J.best = d_best; J.cost_mode = (uint32_t)cost_mode;
        return run_chain(ch, J, st);
    });
    if (rc != PLO_OK) return rc;
    if (nseeds) {
        uint32_t a = 0, mu = 0; plo_stats_t s2{};                            // the winner's costs from the device, whatever the key holds
        rc = plo_cse_chain_cost_many(ch, &bseed, 0, 1, &a, &mu, &s2);
        if (rc != PLO_OK) return rc;
        out->adds = a; out->muls = mu; out->seed = bseed;
    }
    st->candidates = nseeds;
    return PLO_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The kernel method with everything on the device (plo_kmethod.hip): decomposition, both images and both Optimizer
// calls of every restart in one wave.
namespace {
uint32_t rank_mod_p(const plo_csr_t *M, uint32_t p)
{
    const uint32_t m = M->m, n = M->n;
    std::vector<std::vector<uint64_t>> A(m, std::vector<uint64_t>(n, 0));
    for (uint32_t i = 0; i < m; ++i) for (uint32_t k = M->rowptr[i]; k < M->rowptr[i + 1]; ++k) A[i][M->col[k]] = M->val[k];
    uint32_t r = 0;
    for (uint32_t c = 0; c < n && r < m; ++c) {
        uint32_t piv = r; while (piv < m && A[piv][c] == 0) ++piv;
        if (piv == m) continue;
        std::swap(A[piv], A[r]);
        const uint64_t iv = inv_mod((uint32_t)A[r][c], p);
        for (uint32_t j = c; j < n; ++j) A[r][j] = A[r][j] * iv % p;
        for (uint32_t i = r + 1; i < m; ++i) if (A[i][c]) { const uint64_t x = A[i][c]; for (uint32_t j = c; j < n; ++j) A[i][j] = (A[i][j] + (p - x) * A[r][j]) % p; }
        ++r;
    }
    return r;
}
// layout of an image that is built on the device (no template): the fields of build_plan() from bounds instead of a matrix
int layout_plan(plo::WavePlan &P, uint32_t m, uint32_t n, uint32_t nnz, uint32_t p, uint32_t maxlen, uint32_t naive, uint32_t cap)
{
    P = plo::WavePlan{};
    const uint32_t mw = 1;
    const uint64_t NC = (uint64_t)n + naive / 2 + 2;
    const uint32_t rb = ceil_log2(p), bb = ceil_log2((uint32_t)NC);
    if (NC >= 0xFFFFull || 2u * bb + rb > 51u) return fail(PLO_E_CAPACITY, "pair key (col,col,ratio) of the dependent part does not fit 51 bits");
    if (2ull * nnz >= 65535ull || cap > 65536u) return fail(PLO_E_CAPACITY, "dependent part too large for the wave kernel");
    P.m = m; P.n = n; P.nnz = nnz; P.p = p; P.NC = (uint32_t)NC; P.cap = cap; P.hbits = ceil_log2(cap);
    P.lpr_log2 = std::max(2u, ceil_log2(std::max(maxlen, 1u))); P.mw = mw; P.unit = 0u;
    P.multcap = (uint32_t)(naive / 2 + 8); P.maxlen = maxlen; P.rb = rb; P.bb = bb; P.mu = (~0ull) / p;
    layout_wave_image(P);
    return PLO_OK;
}
// The PLO_KMETHOD_* knobs (tests and A/B runs).  depc_scratch, hard_bounds and debug are flags: set is on, whatever they hold.
struct KmKnobs {
    std::optional<long> depc_scratch = env_knob("PLO_KMETHOD_DEPC_SCRATCH"), hard_bounds = env_knob("PLO_KMETHOD_HARD_BOUNDS"), debug = env_knob("PLO_KM_DEBUG"),
                        ent_margin = env_knob("PLO_KMETHOD_ENT_MARGIN"), pairs_div = env_knob("PLO_KMETHOD_PAIRS_DIV"), ent_div = env_knob("PLO_KMETHOD_ENT_DIV");
};

// The scratch of a wave (the small arrays of the decomposition; the combinations too with the A/B knob PLO_KMETHOD_DEPC_SCRATCH, the round-3 placement) and V (m x (n+1)) and
// C (m x (rank+1)) of the elimination behind M's template.  Returns where V and C end.
uint32_t kmethod_scratch_layout(plo::KPlan &K, uint32_t depc_bytes, bool depc_inside) {
    uint32_t off = 0;
    if (!depc_inside) { K.off_depc = (int32_t)off; off += depc_bytes; }
    K.off_vrow = off;  off += 64u * 4u;
    K.off_ord = off;   off += 128u * 2u;
    K.off_piv = off;   off += 128u * 2u;
    K.off_basis = off; off += 64u * 2u;
    K.off_deps = off;  off += 64u * 2u;
    K.off_rsd = off;   off += 66u * 2u;
    K.scratch_bytes = round_up(off, 16);
    K.off_vc = round_up(K.PM.tmpl_bytes, 16);
    return K.off_vc + K.m * (K.n + 1u + K.rank + 1u) * 4u;
}

// A wave's region for a sizing launch, before Dep is laid out: M's image, the elimination arrays and, behind them, the combinations
void kmethod_sizing_region(plo::KPlan &K, uint32_t vc_end, uint32_t depc_bytes, bool depc_inside) {
    K.region = round_up(std::max(K.PM.region_bytes, vc_end), 16);
    if (depc_inside) { const uint32_t at = K.region; K.region = at + depc_bytes; K.off_depc = -(int32_t)depc_bytes; }
}
// k when p = 2^k - 1, else 0 (KPlan::mers)
uint32_t mersenne_exponent(uint32_t p) { for (uint32_t k = 2; k < 31; ++k) if (p == (1u << k) - 1u) return k; return 0; }
// rank and dependent rows of M modulo p, and what the kernel method's device code refuses of them
int kmethod_ranks(const plo_csr_t *M, uint32_t p, uint32_t *R, uint32_t *ndeps) {
    *R = rank_mod_p(M, p); *ndeps = M->m - *R;
    if (*ndeps == 0) return fail(PLO_E_UNSUPPORTED, "zero dimensional kernel");
    if (*ndeps > 64) return fail(PLO_E_UNSUPPORTED, "more than 64 dependent rows: Dep's ProgramGen keeps one row per lane");
    if (*R == 0) return fail(PLO_E_UNSUPPORTED, "zero matrix");
    return PLO_OK;
}
const char *const KMETHOD_SHAPE = "device decomposition needs at most 128 rows and 64 columns";

// The sizing launch: Dep's pair count and entries, maxima over a sample of the decompositions
// (ord: the walk over prescribed row orders -- the sample is `norders` orders at equal distances over the whole range of the call)
int kmethod_sample(plo::KPlan &K, uint64_t seed0, uint64_t nrestarts, uint32_t vc_end, uint32_t depc_bytes, bool depc_inside, plo_stats_t *st, uint32_t *pairs_max, uint32_t *ent_max,
                   const plo::KOrd *ord = nullptr, uint64_t norders = 0) {
    kmethod_sizing_region(K, vc_end, depc_bytes, depc_inside);
    uint32_t lds = 0;
    const uint32_t W = pick_waves([&](uint32_t w) { return K.PM.rs_bytes + w * (K.region + K.scratch_bytes); }, false, g_lds_max, &lds);
    if (!W) return fail(PLO_E_CAPACITY, "kernel-method state does not fit LDS");
    DevBuf<uint32_t> d_sz, d_err;
    HIPCHK(hipMalloc((void **)&d_err.p, 4)); HIPCHK(hipMemsetAsync(d_err, 0, 4, g_stream));
    HIPCHK(hipMalloc((void **)&d_sz.p, 16)); HIPCHK(hipMemsetAsync(d_sz, 0, 16, g_stream));
    HIPCHK(hipFuncSetAttribute(ord ? (const void *)plo::kmethod_size_orders_kernel : (const void *)plo::kmethod_size_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    plo::WaveJob J{}; J.seed0 = seed0; J.ncand = std::min<uint64_t>(ord ? norders : nrestarts, 4096); J.err = d_err;
    const uint64_t grid = grid_for(J.ncand, W, (uint64_t)g_cus * 2u);
    plo::KOrd O{}; if (ord) { O = *ord; O.step_num = norders; O.step_den = J.ncand; }
    const int trc = timed_launch(st, nullptr, [&] {
        if (ord) hipLaunchKernelGGL(plo::kmethod_size_orders_kernel, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, K, J, O, d_sz.p);
        else hipLaunchKernelGGL(plo::kmethod_size_kernel, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, K, J, d_sz.p);
    });
    if (trc != PLO_OK) return trc;
    uint32_t sz[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(sz, d_sz, 16, hipMemcpyDeviceToHost));
    if (sz[2]) return device_error(plo::ERR_KDEC);
    *pairs_max = sz[0]; *ent_max = sz[1];
    return PLO_OK;
}

// Layout of Dep's image and of a wave's region for the search launch.  Rows <= m - rank and entries per row <= rank are hard bounds; the number of entries and the pair count come
// from the sample of the sizing launch (+60 %; measured on 4x4x4_49_156_L: +25 % and +40 % are exceeded by a few of 10^6 restarts and the whole launch is repeated, +60 % and +80 %
// never in 3 x 10^6: the rows of a restart are packed, a restart with more entries is reported -- ERR_TABLE -- and the launch repeated with the hard bound rows x rank, as for a
// full table).  Round 2 sized the arrays for rows x rank: 17.3 KB per wave on 4x4x4_49_156_L, 7 waves per CU.
int kmethod_dep_layout(plo::KPlan &K, const KmKnobs &knobs, uint32_t cap_scale, uint32_t pairs_max, uint32_t ent_max, uint32_t vc_end, uint32_t depc_bytes, bool depc_inside) {
    const uint32_t R = K.rank, hard = K.ndeps * R;
    uint32_t capD = 64;
    while (capD < (cap_scale * pairs_max * 3u) / 4u + 16u) capD <<= 1;
    uint32_t entD = (cap_scale == 1 && !knobs.hard_bounds) ? std::min<uint32_t>(hard, ent_max + (uint32_t)((uint64_t)ent_max * (knobs.ent_margin ? (uint32_t)*knobs.ent_margin : 60u) / 100u) + 16u) : hard;
    if (knobs.ent_div && cap_scale == 1) entD = std::max<uint32_t>(R, entD / (uint32_t)std::max(1l, *knobs.ent_div));   // test knob: undersized entry arrays, exercises the repeat-with-hard-bounds path
    const int rc = layout_plan(K.PD, K.ndeps, K.m, entD, K.PM.p, R, entD, capD);
    if (rc != PLO_OK) return rc;
    K.rsD = nullptr;                                                          // Dep's row starts are computed per restart on the device
    K.region = round_up(std::max(std::max(K.PM.region_bytes, K.PD.region_bytes), vc_end), 16);
    if (depc_inside) {
        // the combinations live from the end of the decomposition to the end of Dep's image build: behind Free's region (Optimizer on Free
        // runs meanwhile) and behind the elimination arrays (they are copied out of C), over Dep's tie list / multiplier list (idle until
        // Dep's Optimizer call)
        const uint32_t at = round_up(std::max(std::max(K.PM.region_bytes, vc_end), K.PD.off_ties), 16);
        K.region = std::max(K.region, at + depc_bytes);
        K.off_depc = (int32_t)at - (int32_t)K.region;
    }
    return PLO_OK;
}

// The walk over prescribed row orders (plo_kernel_search_orders): orders first .. first + count - 1, `sub` restarts each
struct KOrdReq { uint64_t first, count; uint32_t sub; };

// Body of plo_kernel_search (ord == nullptr: `total` restarts of random orders) and of plo_kernel_search_orders (total = count * sub
// candidates), arguments checked.  The candidates go to the device in launches of at most `chunk`; the minimum is carried over the
// launches on the host, the earlier launch winning ties; a launch that reports a full table is repeated with twice the slots, and
// the launches after it keep the larger tables.
int kernel_search_run(const plo_csr_t *M, uint32_t p, uint64_t seed0, uint64_t total, uint64_t chunk, uint32_t per_block, int cost_mode,
                      uint32_t *adds, uint32_t *muls, uint32_t *info, plo_best_t *best, plo_stats_t *st, const KOrdReq *ord)
{
    CallScope call(st); st = call.st;
    if (best) { best->adds = best->muls = 0xFFFFFFFFu; best->seed = ~0ull; }
    const uint32_t m = M->m, n = M->n; uint32_t R = 0, ndeps = 0;
    if (const int rc = kmethod_ranks(M, p, &R, &ndeps)) return rc;

    const KmKnobs knobs;
    const uint32_t depc_bytes = round_up(ndeps * R * 4u, 16);
    const bool depc_inside = !knobs.depc_scratch;
    uint32_t pairs_max = 0, ent_max = 0;
    plo::KOrd O{};
    if (ord) { O.seed0 = seed0; O.first = ord->first; O.sub = ord->sub; O.fact[0] = 1u; for (uint32_t k = 1; k < 12u; ++k) O.fact[k] = O.fact[k - 1u] * k; }
    const uint64_t cseed0 = ord ? seed0 + ord->first * ord->sub : seed0;      // seed of candidate 0 of the call
    uint64_t done = 0;
    // Dep's table starts at 0.75 x the sampled PAIR count (an upper bound of its distinct triples, usually far above it): a
    // smaller image means more resident waves; a full table is reported by the device and the launch repeated with twice the slots
    for (uint32_t cap_scale = 1; cap_scale <= 32; cap_scale *= 2) {
        plo::KPlan K{};
        DevBuf<uint8_t> d_img;      // of this attempt
        // plan and image of M (the layout of Free)
        plo_plan tmp; tmp.cap_scale = std::max(2u, cap_scale);
        set_matrix(&tmp, M, p);
        std::vector<uint8_t> img;
        int rc = build_plan(&tmp, &img);
        if (rc != PLO_OK) return rc;
        K.PM = tmp.P; K.m = m; K.n = n; K.rank = R; K.ndeps = ndeps; K.per_block = per_block;
        K.mers = mersenne_exponent(p);
        const uint32_t vc_end = kmethod_scratch_layout(K, depc_bytes, depc_inside);
        HIPCHK(hipMalloc((void **)&d_img.p, img.size() + 64)); HIPCHK(hipMemcpy(d_img, img.data(), img.size(), hipMemcpyHostToDevice));
        K.PM.tmpl = (const uint64_t *)d_img.p;
        if (cap_scale == 1) {
            if ((rc = kmethod_sample(K, seed0, total, vc_end, depc_bytes, depc_inside, st, &pairs_max, &ent_max, ord ? &O : nullptr, ord ? ord->count : 0)) != PLO_OK) return rc;
            if (knobs.pairs_div) pairs_max /= (uint32_t)std::max(1l, *knobs.pairs_div);   // test knob: undersized first table, exercises the repeat-with-more-slots path
        }
        if ((rc = kmethod_dep_layout(K, knobs, cap_scale, pairs_max, ent_max, vc_end, depc_bytes, depc_inside)) != PLO_OK) return rc;
        uint32_t lds = 0, bestw = 0;
        const uint32_t W = pick_waves([&](uint32_t w) { return K.PM.rs_bytes + K.PD.rs_bytes + w * (K.region + K.scratch_bytes); }, true, g_lds_max, &lds, &bestw);
        if (!W) return fail(PLO_E_CAPACITY, "kernel-method state does not fit LDS");
        if (knobs.debug) fprintf(stderr, "# kernel method layout: region of M %u B (table %u slots), of Dep %u B (table %u slots, sampled pairs %u, entries %u of at most %u), elimination arrays end at %u B, scratch %u B; %u waves per workgroup, %u B of LDS, %u waves per CU\n",
                                 K.PM.region_bytes, K.PM.cap, K.PD.region_bytes, K.PD.cap, pairs_max, K.PD.nnz, ndeps * R, vc_end, K.scratch_bytes, W, lds, bestw);
        const void *fn = ord ? (K.PM.unit ? (const void *)plo::kmethod_orders_kernel<true> : (const void *)plo::kmethod_orders_kernel<false>)
                             : (K.PM.unit ? (const void *)plo::kmethod_kernel<true> : (const void *)plo::kmethod_kernel<false>);
        bool again = false;
        while (done < total && !again) {                                         // the launches at this table size
            const uint64_t cnt = std::min<uint64_t>(chunk, total - done);
            DevBuf<uint32_t> d_info;
            if (info) HIPCHK(hipMalloc((void **)&d_info.p, cnt * 12));
            const plo::KInfo I{d_info.p};
            O.cand0 = done;
            plo_best_t cb{0xFFFFFFFFu, 0xFFFFFFFFu, ~0ull};
            rc = one_shot_search(fn, W, lds, cseed0 + done, cnt, cost_mode, adds ? adds + done : nullptr, muls ? muls + done : nullptr, best ? &cb : nullptr, st, &again,
                                 [&](uint64_t grid, const plo::WaveJob &J) {
                if (ord) {
                    if (K.PM.unit) hipLaunchKernelGGL(plo::kmethod_orders_kernel<true>, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, K, J, I, O);
                    else hipLaunchKernelGGL(plo::kmethod_orders_kernel<false>, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, K, J, I, O);
                }
                else if (K.PM.unit) hipLaunchKernelGGL(plo::kmethod_kernel<true>, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, K, J, I);
                else hipLaunchKernelGGL(plo::kmethod_kernel<false>, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, K, J, I);
            });
            if (rc != PLO_OK) return rc;
            if (again) break;
            if (info) HIPCHK(hipMemcpy(info + 3u * done, d_info, cnt * 12, hipMemcpyDeviceToHost));
            if (best && (best->seed == ~0ull || plo_pack_cost(cb.adds, cb.muls, cost_mode, 0) < plo_pack_cost(best->adds, best->muls, cost_mode, 0))) *best = cb;
            done += cnt;
        }
#ifdef PLO_KM_PROFILE
        if (getenv("PLO_KM_STATS")) {
            unsigned long long g[8] = {0};
            if (hipMemcpyFromSymbol(g, HIP_SYMBOL(plo::g_kprof), sizeof g) == hipSuccess && g[5])
                fprintf(stderr, "# kernel method, cumulative over %llu restarts: cycles per restart: copy + decomposition %.0f, Free image %.0f, Optimizer on Free %.0f, Dep image %.0f, Optimizer on Dep %.0f; inside the decomposition: elimination loops %.0f, pivot + inverse + stores %.0f\n",
                        g[5], (double)g[0] / g[5], (double)g[1] / g[5], (double)g[2] / g[5], (double)g[3] / g[5], (double)g[4] / g[5], (double)g[6] / g[5], (double)g[7] / g[5]);
        }
#endif
        if (again) continue;                                                     // a pair table filled up: again with twice the slots
        st->candidates = total;
        return call.done(PLO_OK);
    }
    return device_error(plo::ERR_TABLE);
}
} // namespace

int plo_kernel_search(const plo_csr_t *M, uint32_t p, uint64_t seed0, uint64_t nrestarts, uint32_t per_block, int cost_mode,
                      uint32_t *adds, uint32_t *muls, uint32_t *info, plo_best_t *best, plo_stats_t *st)
{
    if (!M || nrestarts == 0 || per_block == 0) return fail(PLO_E_ARG, "bad argument");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    if (p < 3 || p >= 0x80000000u || !(p & 1u)) return fail(PLO_E_ARG, "modulus must be an odd prime below 2^31");
    if (const char *bad = csr_defect(M, p)) return fail(PLO_E_ARG, bad);
    if (M->m == 0 || M->m > 128 || M->n == 0 || M->n > 64) return fail(PLO_E_UNSUPPORTED, KMETHOD_SHAPE);
    if (nrestarts > 0xFFFFFFFFull) return fail(PLO_E_ARG, "at most 2^32-1 restarts per call");
    return kernel_search_run(M, p, seed0, nrestarts, nrestarts, per_block, cost_mode, adds, muls, info, best, st, nullptr);
}

int plo_kernel_search_orders(const plo_csr_t *M, uint32_t p, uint64_t seed0, uint64_t first, uint64_t count, uint32_t sub, int cost_mode,
                             uint32_t *adds, uint32_t *muls, uint32_t *info, plo_best_t *best, plo_stats_t *st)
{
    if (!M || count == 0 || sub == 0) return fail(PLO_E_ARG, "bad argument");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    if (M->m < 2 || M->m > 12) return fail(PLO_E_ARG, "the row orders are walked for 2 to 12 rows");
    uint64_t mfact = 1; for (uint32_t k = 2; k <= M->m; ++k) mfact *= k;
    if (first >= mfact || count > mfact - first) return fail(PLO_E_ARG, "order range beyond m!");
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    if (p < 3 || p >= 0x80000000u || !(p & 1u)) return fail(PLO_E_ARG, "modulus must be an odd prime below 2^31");
    if (const char *bad = csr_defect(M, p)) return fail(PLO_E_ARG, bad);
    if (M->n == 0 || M->n > 64) return fail(PLO_E_UNSUPPORTED, KMETHOD_SHAPE);
    // launches of at most 2^25 candidates (the device packs key << 32 | candidate, and no launch should hold a shared device for long); PLO_KORD_CHUNK: test knob, fewer
    const uint64_t chunk = (uint64_t)std::min<long>(std::max<long>(env_knob("PLO_KORD_CHUNK").value_or(1l << 25), 1l), 1l << 25);
    const KOrdReq ord{first, count, sub};
    return kernel_search_run(M, p, seed0, count * sub, chunk, 1u, cost_mode, adds, muls, info, best, st, &ord);
}

} // extern "C"
namespace {
// Host side of one problem of plo_kernel_batch_search
struct KmSlot {
    uint32_t scale = 1;                  // 1: Dep's image from the sample of the sizing launch; 2, 4, .. 32: the hard bound for its entries and scale x the pairs for its
                                         // table, M's table by max(2, scale) -- the growth rule of kernel_search_run, per problem
    bool fixed = false;                  // Dep from the hard bounds from the start (scale 2): no sample, never short of entries, and the knobs of the sample do not reach it
    uint32_t R = 0, ndeps = 0, depc_bytes = 0, vc_end = 0, pairs_max = 0, ent_max = 0;
    plo::KPlan K{};
    std::vector<uint8_t> img; size_t img_off = 0;
    int rc = PLO_OK; std::string why;
};
// rank (once), plan and image of M at S.scale and the scratch layout; S.rc / S.why: what plo_kernel_search would refuse
void kbatch_build(KmSlot &S, const plo_csr_t *M, uint32_t p, bool depc_inside)
{
    S.rc = PLO_OK; S.why.clear();
    if (S.R + S.ndeps == 0) {
        if (M->m == 0 || M->m > 128 || M->n == 0 || M->n > 64) { S.rc = PLO_E_UNSUPPORTED; S.why = KMETHOD_SHAPE; return; }
        if ((S.rc = kmethod_ranks(M, p, &S.R, &S.ndeps)) != PLO_OK) { S.why = g_err; return; }
        S.depc_bytes = round_up(S.ndeps * S.R * 4u, 16);
    }
    plo_plan tmp; tmp.cap_scale = std::max(2u, S.scale);
    set_matrix(&tmp, M, p);
    if ((S.rc = build_plan(&tmp, &S.img)) != PLO_OK) { S.why = g_err; return; }
    plo::KPlan &K = S.K;
    K = plo::KPlan{};
    K.PM = tmp.P; K.m = M->m; K.n = M->n; K.rank = S.R; K.ndeps = S.ndeps; K.per_block = 1u; K.mers = mersenne_exponent(p);
    S.vc_end = kmethod_scratch_layout(K, S.depc_bytes, depc_inside);
    kmethod_sizing_region(K, S.vc_end, S.depc_bytes, depc_inside);
}
} // namespace
extern "C" {

// The kernel method on many matrices in one call, one minimum each (plo::kmethod_batch_kernel, one workgroup per problem).
// The sizing launch decomposes the first min(per_problem, 64) of each problem's own restarts; a problem whose hard bounds are small
// (at most 32 pairs: the 64-slot minimum table holds them; or an image that does not enlarge the wave's region) is laid out from those
// and not sampled.  Results do not depend on either: a restart with more entries or triples than laid out reports ERR_TABLE and the
// problem is run again with the next scale.
int plo_kernel_batch_search(uint32_t nprob, const plo_csr_t *mats, uint32_t p, uint64_t seed0, uint32_t per_problem,
                            int cost_mode, plo_best_t *bests, int32_t *status, plo_stats_t *st)
{
    if (!mats || !bests || !status || nprob == 0 || per_problem == 0) return fail(PLO_E_ARG, "bad argument");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    if (p < 3 || p >= 0x80000000u || !(p & 1u)) return fail(PLO_E_ARG, "modulus must be an odd prime below 2^31");
    if ((uint64_t)nprob * per_problem > 0xFFFFFFFFull) return fail(PLO_E_ARG, "at most 2^32-1 candidates per call");
    for (uint32_t q = 0; q < nprob; ++q)
        if (const char *bad = csr_defect(&mats[q], p)) return fail(PLO_E_ARG, "problem " + std::to_string(q) + ": " + bad);
    if (const int rc = require_device(NOINIT_CSE)) return rc;
    CallScope call(st); st = call.st;
    for (uint32_t q = 0; q < nprob; ++q) { bests[q].adds = bests[q].muls = 0xFFFFFFFFu; bests[q].seed = ~0ull; status[q] = PLO_OK; }
    const KmKnobs knobs;
    const bool depc_inside = !knobs.depc_scratch;
    const std::optional<long> grid_cap = env_knob("PLO_BATCH_GRID");
    const bool batch_stats = env_knob("PLO_BATCH_STATS").has_value();
    const size_t lds_max = g_lds_max;
    const uint32_t nsample = std::min(per_problem, 64u);
    DevBuf<unsigned long long> d_keys; DevBuf<uint32_t> d_adds, d_muls, d_err;
    HIPCHK(hipMalloc((void **)&d_keys.p, nprob * 8ull)); HIPCHK(hipMalloc((void **)&d_adds.p, nprob * 4ull));
    HIPCHK(hipMalloc((void **)&d_muls.p, nprob * 4ull)); HIPCHK(hipMalloc((void **)&d_err.p, nprob * 4ull));
    HIPCHK(hipMemsetAsync(d_keys, 0xFF, nprob * 8ull, g_stream));
    std::vector<KmSlot> S(nprob);
    std::vector<uint32_t> todo(nprob), err(nprob);
    for (uint32_t q = 0; q < nprob; ++q) todo[q] = q;
    const auto slot_of = [&](uint32_t q) { return S[q].K.region + S[q].K.scratch_bytes; };
    const auto fits = [&](uint32_t q) { return 64ull + S[q].K.PM.rs_bytes + slot_of(q) <= lds_max; };
    for (bool first = true; !todo.empty(); first = false) {
        on_host_threads(todo.size(), [&](size_t k) { const uint32_t q = todo[k]; kbatch_build(S[q], &mats[q], p, depc_inside); });
        std::vector<uint32_t> live;
        size_t total = 0;
        for (const uint32_t q : todo) {
            if (S[q].rc == PLO_OK && !fits(q)) { S[q].rc = PLO_E_CAPACITY; S[q].why = "kernel-method state does not fit LDS"; }
            if (S[q].rc == PLO_E_CAPACITY || S[q].rc == PLO_E_UNSUPPORTED) { status[q] = S[q].rc; continue; }     // this problem alone is refused
            if (S[q].rc != PLO_OK) return fail(S[q].rc, "problem " + std::to_string(q) + ": " + S[q].why);
            S[q].img_off = total; total += round_up((uint32_t)S[q].img.size(), 64);
            live.push_back(q);
        }
        if (live.empty()) break;
        // one device buffer for the images of M of all problems
        std::vector<uint8_t> blob(total + 64, 0);
        for (const uint32_t q : live) std::memcpy(blob.data() + S[q].img_off, S[q].img.data(), S[q].img.size());
        DevBuf<uint8_t> d_img;
        HIPCHK(hipMalloc((void **)&d_img.p, blob.size()));
        HIPCHK(hipMemcpy(d_img, blob.data(), blob.size(), hipMemcpyHostToDevice));
        // The launches over `order`, none across a boundary of `cuts`: one per stretch, unless the largest row starts and the largest slot -- of different problems --
        // no longer fit the LDS together (each problem alone fits).  sizing: the decompositions of the sample into d_sz, else the search.
        uint32_t *d_sz = nullptr;
        const auto run = [&](const std::vector<uint32_t> &order, const std::vector<size_t> &cuts, bool sizing) -> int {
            std::vector<plo::KBatchProb> probs(order.size());
            for (size_t k = 0; k < order.size(); ++k) { probs[k].K = S[order[k]].K; probs[k].K.PM.tmpl = (const uint64_t *)(d_img.p + S[order[k]].img_off); probs[k].q = order[k]; }
            DevBuf<plo::KBatchProb> d_probs;
            HIPCHK(hipMalloc((void **)&d_probs.p, probs.size() * sizeof(plo::KBatchProb)));
            HIPCHK(hipMemcpy(d_probs, probs.data(), probs.size() * sizeof(plo::KBatchProb), hipMemcpyHostToDevice));
            const void *fn = sizing ? (const void *)plo::kmethod_batch_size_kernel : (const void *)plo::kmethod_batch_kernel;
            for (size_t c = 0; c + 1 < cuts.size(); ++c)
                for (size_t b0 = cuts[c], b1; b0 < cuts[c + 1]; b0 = b1) {
                    plo::KBatchJob J{}; J.probs = d_probs.p + b0; J.per = per_problem; J.nsample = nsample; J.cost_mode = (uint32_t)cost_mode; J.seed0 = seed0;
                    J.keys = d_keys; J.adds = d_adds; J.muls = d_muls; J.err = d_err; J.sz = d_sz;
                    for (b1 = b0; b1 < cuts[c + 1]; ++b1) {
                        const uint32_t rs = std::max(J.rsmax, S[order[b1]].K.PM.rs_bytes), sl = std::max(J.slot, slot_of(order[b1]));
                        if (b1 > b0 && 64ull + rs + sl > lds_max) break;
                        J.rsmax = rs; J.slot = sl;
                    }
                    const size_t count = b1 - b0;
                    J.nprob = (uint32_t)count;
                    const auto need = [&](uint32_t w) { return 64u + J.rsmax + w * J.slot; };
                    const uint32_t W = batch_waves(need, sizing ? nsample : per_problem, lds_max), lds = need(W);
                    uint32_t per_cu = 1;
                    if (const int rc = occupancy_for(fn, W, lds, &per_cu)) return rc;
                    uint64_t grid = std::min<uint64_t>(count, 0x7FFFFFFFull);
                    if (grid_cap && *grid_cap > 0) grid = std::min<uint64_t>(grid, (uint64_t)*grid_cap);
                    const LaunchShape shape{grid, lds, W, 0};
                    const double ms0 = st->kernel_ms;
                    const int rc = timed_launch(st, sizing ? nullptr : &shape, [&] {
                        if (sizing) hipLaunchKernelGGL(plo::kmethod_batch_size_kernel, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, J);
                        else hipLaunchKernelGGL(plo::kmethod_batch_kernel, dim3((uint32_t)grid), dim3(W * 64), lds, g_stream, J);
                    });
                    if (rc != PLO_OK) return rc;
                    if (batch_stats) fprintf(stderr, "# kernel batch: %s, scale %u: %zu problems, %u waves per workgroup, %u LDS bytes, %u workgroups per CU, grid %llu, %.3f ms\n",
                                             sizing ? "sizing" : "search", S[order[b0]].scale, count, W, lds, per_cu, (unsigned long long)grid, st->kernel_ms - ms0);
                    if (!sizing) st->candidates += (uint64_t)count * per_problem;
                }
            return PLO_OK;
        };
        if (first) {
            // who is sampled: not the problems whose hard bounds (ndeps x rank entries, ndeps x rank (rank - 1) / 2 pairs) are small
            std::vector<uint32_t> sampled;
            for (const uint32_t q : live) {
                KmSlot &X = S[q];
                const uint32_t hard_ent = X.ndeps * X.R, hard_pairs = X.ndeps * X.R * (X.R - 1u) / 2u;
                plo::KPlan T = X.K;
                X.fixed = kmethod_dep_layout(T, knobs, 2, hard_pairs, hard_ent, X.vc_end, X.depc_bytes, depc_inside) == PLO_OK
                          && (hard_pairs <= 32u || T.region <= X.K.region);
                if (X.fixed) { X.scale = 2; X.pairs_max = hard_pairs; X.ent_max = hard_ent; } else sampled.push_back(q);
            }
            if (!sampled.empty()) {
                DevBuf<uint32_t> sz;
                HIPCHK(hipMalloc((void **)&sz.p, nprob * 16ull)); HIPCHK(hipMemsetAsync(sz, 0, nprob * 16ull, g_stream));
                d_sz = sz.p;
                if (const int rc = run(sampled, {0, sampled.size()}, true)) return rc;
                std::vector<uint32_t> h(nprob * 4ull);
                HIPCHK(hipMemcpy(h.data(), sz, nprob * 16ull, hipMemcpyDeviceToHost));
                d_sz = nullptr;
                for (const uint32_t q : sampled) {
                    if (h[4u * q + 2u]) { status[q] = PLO_E_INTERNAL; continue; }      // ERR_KDEC: a decomposition that contradicts the host's rank
                    S[q].pairs_max = h[4u * q]; S[q].ent_max = h[4u * q + 1u];
                    if (knobs.pairs_div) S[q].pairs_max /= (uint32_t)std::max(1l, *knobs.pairs_div);   // test knob: undersized first table, as in kernel_search_run
                }
            }
        }
        // Dep's image and the wave's region of every problem at its scale, then the buckets by footprint (row starts + region + scratch)
        std::vector<uint32_t> bucket[BATCH_BUCKETS];
        for (const uint32_t q : live) {
            if (status[q] != PLO_OK) continue;
            KmSlot &X = S[q];
            const int rc = kmethod_dep_layout(X.K, knobs, X.scale, X.pairs_max, X.ent_max, X.vc_end, X.depc_bytes, depc_inside);
            if (rc == PLO_OK && !fits(q)) { status[q] = PLO_E_CAPACITY; continue; }
            if (rc == PLO_E_CAPACITY) { status[q] = rc; continue; }
            if (rc != PLO_OK) return fail(rc, "problem " + std::to_string(q) + ": " + g_err);
            bucket[batch_bucket(X.K.PM.rs_bytes + slot_of(q))].push_back(q);
        }
        std::vector<uint32_t> order; std::vector<size_t> cuts{0};
        for (const auto &b : bucket) if (!b.empty()) { order.insert(order.end(), b.begin(), b.end()); cuts.push_back(order.size()); }
        if (order.empty()) break;
        HIPCHK(hipMemsetAsync(d_err, 0, nprob * 4ull, g_stream));
        if (const int rc = run(order, cuts, false)) return rc;
        HIPCHK(hipMemcpy(err.data(), d_err, nprob * 4ull, hipMemcpyDeviceToHost));
        // a full table or more entries of Dep than laid out is that problem's alone: only those are laid out again, with the next scale, and launched again
        std::vector<uint32_t> next;
        for (const uint32_t q : order) {
            if (!err[q]) continue;
            if (err[q] == plo::ERR_KDEC) { status[q] = PLO_E_INTERNAL; continue; }
            if (err[q] != plo::ERR_TABLE) { const int rc = device_error((int)err[q]); return fail(rc, "problem " + std::to_string(q) + ": " + g_err); }
            if (S[q].scale >= 32u) { status[q] = PLO_E_CAPACITY; continue; }
            S[q].scale *= 2u; next.push_back(q);
        }
        todo = std::move(next);
    }
    std::vector<unsigned long long> keys(nprob); std::vector<uint32_t> adds(nprob), muls(nprob);
    HIPCHK(hipMemcpy(keys.data(), d_keys, nprob * 8ull, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(adds.data(), d_adds, nprob * 4ull, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(muls.data(), d_muls, nprob * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < nprob; ++q) {
        if (status[q] != PLO_OK) continue;
        if (keys[q] == ~0ull) return fail(PLO_E_INTERNAL, "problem " + std::to_string(q) + ": no result");
        bests[q].adds = adds[q]; bests[q].muls = muls[q]; bests[q].seed = seed0 + (uint64_t)q * per_problem + (keys[q] & 0xFFFFFFFFull);
    }
    return call.done(PLO_OK);
}

} // extern "C"

namespace {
// Host side of one enumeration: the right nullspace of the rows already chosen restricted to the block, the block of TM, the
// initial best word.  dependent: the chosen rows are dependent (rank(Cand with row := w) can never exceed `row`, :174).
struct CobPrep { bool dependent = false; uint32_t qn = 0, fb = 0; std::vector<uint32_t> nb, tmb; unsigned long long init = 0; };
int cob_check(uint32_t n, uint32_t m, const uint32_t *TM, const uint32_t *Cand, uint32_t row, uint32_t offsetblock, const uint32_t *coeffs, uint32_t ncoeffs, uint32_t p)
{
    if (!TM || !Cand || !coeffs) return fail(PLO_E_ARG, "null argument");
    if (p < 3 || p >= 0x80000000u || !(p & 1u)) return fail(PLO_E_ARG, "modulus must be an odd prime below 2^31");
    if (n == 0 || row >= n || offsetblock >= n || ncoeffs == 0) return fail(PLO_E_ARG, "bad dimensions");
    if (ncoeffs > 255) return fail(PLO_E_CAPACITY, "more than 255 coefficients: the candidate index does not fit 32 bits");
    if ((uint64_t)(m + 1) * (n + 1) >= 0xFFFFFFFFull) return fail(PLO_E_CAPACITY, "score does not fit 32 bits");
    return PLO_OK;
}
void cob_prepare(uint32_t n, uint32_t m, const uint32_t *TM, const uint32_t *Cand, uint32_t row, uint32_t offsetblock, uint32_t p, int32_t w0, int32_t w1, CobPrep &R)
{
    // right nullspace of the rows already chosen (rows 0..row-1 of Cand), by reduced row echelon form mod p
    std::vector<std::vector<uint32_t>> A(row, std::vector<uint32_t>(n));
    for (uint32_t i = 0; i < row; ++i) for (uint32_t j = 0; j < n; ++j) A[i][j] = Cand[(size_t)i * n + j] % p;
    std::vector<uint32_t> piv; uint32_t r0 = 0;
    for (uint32_t c = 0; c < n && r0 < row; ++c) {
        uint32_t q = r0; while (q < row && A[q][c] == 0) ++q;
        if (q == row) continue;
        std::swap(A[q], A[r0]);
        const uint32_t iv = inv_mod(A[r0][c], p);
        for (uint32_t j = c; j < n; ++j) A[r0][j] = (uint32_t)((uint64_t)A[r0][j] * iv % p);
        for (uint32_t i = 0; i < row; ++i) if (i != r0 && A[i][c]) { const uint32_t l = A[i][c]; for (uint32_t j = c; j < n; ++j) A[i][j] = (uint32_t)(((uint64_t)A[i][j] + (uint64_t)(p - l) * A[r0][j]) % p); }
        piv.push_back(c); ++r0;
    }
    R.dependent = piv.size() != row;
    if (R.dependent) return;
    std::vector<char> isp(n, 0); for (uint32_t c : piv) isp[c] = 1;
    const uint32_t fb = std::min<uint32_t>(4, n - offsetblock);
    std::vector<std::vector<uint32_t>> cols;                  // only the block positions of each basis vector
    for (uint32_t fc = 0; fc < n; ++fc) {
        if (isp[fc]) continue;
        std::vector<uint32_t> x(n, 0); x[fc] = 1;
        for (size_t k = 0; k < piv.size(); ++k) x[piv[k]] = A[k][fc] ? p - A[k][fc] : 0;
        bool any = false; for (uint32_t t = 0; t < fb; ++t) any |= x[offsetblock + t] != 0;
        if (any) cols.push_back({x[offsetblock], fb > 1 ? x[offsetblock + 1] : 0, fb > 2 ? x[offsetblock + 2] : 0, fb > 3 ? x[offsetblock + 3] : 0});
    }
    R.fb = fb; R.qn = (uint32_t)cols.size(); R.nb.assign(4 * (size_t)std::max<uint32_t>(R.qn, 1), 0);
    for (uint32_t c = 0; c < R.qn; ++c) for (uint32_t t = 0; t < 4; ++t) R.nb[(size_t)t * R.qn + c] = cols[c][t];
    R.tmb.assign(4 * (size_t)m, 0);
    for (uint32_t t = 0; t < fb; ++t) for (uint32_t j = 0; j < m; ++j) R.tmb[(size_t)t * m + j] = TM[(size_t)(offsetblock + t) * m + j] % p;
    // a candidate (zv,zw), 0 <= zw <= n, has the high word zv*(n+1)+zw+1 and beats (w0,w1) in the lexicographic order iff that exceeds
    // w0*(n+1)+w1+1 with w1 clamped to [-1,n]: (w0,-1) is beaten by every (w0,zw), (w0,w1>n) by none; every candidate beats w0 < 0
    const int64_t thr = w0 < 0 ? 0 : (int64_t)w0 * (n + 1) + std::min<int64_t>(std::max<int64_t>(w1, -1), n) + 1;
    R.init = ((unsigned long long)thr << 32) | 0xFFFFFFFFull;
}
void cob_decode(unsigned long long w, unsigned long long init, uint32_t n, int32_t w0, int32_t w1, plo_cob_best_t *out)
{
    out->found = w != init ? 1u : 0u;
    if (out->found) { const uint32_t sc = (uint32_t)(w >> 32) - 1u; out->zeros_v = (int32_t)(sc / (n + 1)); out->zeros_w = (int32_t)(sc % (n + 1)); out->index = (uint32_t)~(uint32_t)w; }
    else { out->zeros_v = w0; out->zeros_w = w1; out->index = 0; }
}

// The context's scratch buffer grown to `words` words (with 1024 to spare) and its event pair created: both are kept between calls
int cob_scratch(size_t words) {
    DevCtx &cx = cur_ctx();
    if (cx.cob_words < words) {
        if (cx.cob_buf) (void)hipFree(cx.cob_buf);
        cx.cob_buf = nullptr; cx.cob_words = 0;
        HIPCHK(hipMalloc((void **)&cx.cob_buf, (words + 1024) * 4)); cx.cob_words = words + 1024;
    }
    if (!cx.cob_e0) { HIPCHK(hipEventCreate(&cx.cob_e0)); HIPCHK(hipEventCreate(&cx.cob_e1)); }
    return PLO_OK;
}
// `up` into that buffer, then the one launch of an enumeration between the context's events: the statistics of the call but its candidates, algo_bytes and seconds
template <class Launch> int cob_launch(const std::vector<uint32_t> &up, uint64_t grid, size_t lds, plo_stats_t *st, Launch launch) {
    DevCtx &cx = cur_ctx();
    HIPCHK(hipMemcpyAsync(cx.cob_buf, up.data(), up.size() * 4, hipMemcpyHostToDevice, g_stream));
    float ms = 0;
    if (const int rc = timed_between(cx.cob_e0, cx.cob_e1, &ms, launch)) return rc;
    st->kernel_ms = ms; st->launches = 1; st->grid = (uint32_t)grid; st->lds_bytes = (uint32_t)lds; st->waves_per_wg = 4;
    return PLO_OK;
}
} // namespace

extern "C" {

int plo_cob_search(uint32_t n, uint32_t m, const uint32_t *TM, const uint32_t *Cand, uint32_t row, uint32_t offsetblock,
                   const uint32_t *coeffs, uint32_t ncoeffs, uint32_t p, int32_t w0, int32_t w1,
                   plo_cob_best_t *out, plo_stats_t *st)
{
    return plo_cob_search_range(n, m, TM, Cand, row, offsetblock, coeffs, ncoeffs, p, w0, w1, 0, (uint64_t)ncoeffs * ncoeffs * ncoeffs, out, st);
}

// Up to PLO_COB_BATCH enumerations of the same shape (n, m, row, block) in ONE launch: one upload, one kernel (blockIdx.y = the
// enumeration), one download.  bin/sparsifier over the rationals enumerates modulo two primes: one launch instead of two.
int plo_cob_search_batch(uint32_t nprob, uint32_t n, uint32_t m, uint32_t row, uint32_t offsetblock, const plo_cob_problem_t *prob, plo_cob_best_t *out, plo_stats_t *st)
{
    if (!prob || !out || nprob == 0 || nprob > PLO_COB_BATCH) return fail(PLO_E_ARG, "1 to 4 enumerations per launch");
    for (uint32_t k = 0; k < nprob; ++k) { const int rc = cob_check(n, m, prob[k].TM, prob[k].Cand, row, offsetblock, prob[k].coeffs, prob[k].ncoeffs, prob[k].p); if (rc != PLO_OK) return rc; }
    if (const int rc = require_device(NOINIT_DEVICE0)) return rc;
    CallScope call(st); st = call.st;
    CobPrep R[PLO_COB_BATCH]; uint32_t live[PLO_COB_BATCH], nlive = 0;
    for (uint32_t k = 0; k < nprob; ++k) {
        cob_prepare(n, m, prob[k].TM, prob[k].Cand, row, offsetblock, prob[k].p, prob[k].w0, prob[k].w1, R[k]);
        const uint64_t C = prob[k].ncoeffs;
        st->candidates += C * C * C * C;
        if (R[k].dependent) { out[k].found = 0; out[k].zeros_v = prob[k].w0; out[k].zeros_w = prob[k].w1; out[k].index = 0; }
        else live[nlive++] = k;
    }
    if (nlive == 0) return call.done(PLO_OK);
    // one device buffer kept by the context, one upload: [best words (2 each) | per enumeration: TM block | nullspace block | coefficients]
    DevCtx &cx = cur_ctx();
    size_t off[PLO_COB_BATCH][3], words = 2 * (size_t)nlive; bool tab = !getenv("PLO_COB_GENERIC"); size_t lds = 0;
    plo::CobBatch B{}; uint64_t maxgroups = 0, maxtotal = 0;
    for (uint32_t q = 0; q < nlive; ++q) {
        const uint32_t k = live[q], C = prob[k].ncoeffs;
        off[q][0] = words; words += R[k].tmb.size(); off[q][1] = words; words += R[k].nb.size(); off[q][2] = words; words += C;
        B.ms[q] = m | 1u; B.qs[q] = std::max<uint32_t>(R[k].qn, 1u) | 1u;
        tab = tab && 4ull * C * ((size_t)B.ms[q] + B.qs[q]) * 4 <= 72u * 1024u;
        maxgroups = std::max<uint64_t>(maxgroups, (uint64_t)C * C * C); maxtotal = std::max<uint64_t>(maxtotal, (uint64_t)C * C * C * C);
    }
    for (uint32_t q = 0; q < nlive; ++q) { const uint32_t k = live[q], C = prob[k].ncoeffs; lds = std::max<size_t>(lds, tab ? (size_t)(4ull * C * ((size_t)B.ms[q] + B.qs[q]) * 4) : (4 * (size_t)m + 4 * (size_t)R[k].qn + C) * 4); }
    if (lds > g_lds_max) return fail(PLO_E_CAPACITY, "block of TM does not fit LDS");
    if (const int rc = cob_scratch(words)) return rc;
    std::vector<uint32_t> up(words);
    for (uint32_t q = 0; q < nlive; ++q) {
        const uint32_t k = live[q], C = prob[k].ncoeffs, p = prob[k].p;
        memcpy(up.data() + 2 * q, &R[k].init, 8);
        memcpy(up.data() + off[q][0], R[k].tmb.data(), R[k].tmb.size() * 4); memcpy(up.data() + off[q][1], R[k].nb.data(), R[k].nb.size() * 4);
        for (uint32_t x = 0; x < C; ++x) up[off[q][2] + x] = prob[k].coeffs[x] % p;      // (residues, as TM and Cand: zeros(w) counts them)
        plo::CobJob &J = B.J[q];
        J.n = n; J.m = m; J.qn = R[k].qn; J.fb = R[k].fb; J.C = C; J.p = p; J.mu = (~0ull) / p; J.first = 0; J.total = (uint64_t)C * C * C * C;
        J.tm = cx.cob_buf + off[q][0]; J.nb = cx.cob_buf + off[q][1]; J.coeffs = cx.cob_buf + off[q][2]; J.best = (unsigned long long *)cx.cob_buf + q;
    }
    for (uint32_t q = nlive; q < PLO_COB_BATCH; ++q) B.J[q] = B.J[0];      // (never launched: blockIdx.y < nlive)
    B.tab = tab ? 1u : 0u;
    HIPCHK(hipFuncSetAttribute((const void *)plo::cob_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const uint64_t grid = tab ? std::max<uint64_t>(1, std::min<uint64_t>((maxgroups + 3) / 4, (uint64_t)g_cus * 2)) : std::max<uint64_t>(1, std::min<uint64_t>((maxtotal + 255) / 256, (uint64_t)g_cus * 8));
    if (const int rc = cob_launch(up, grid, lds, st, [&] { hipLaunchKernelGGL(plo::cob_batch_kernel, dim3((uint32_t)grid, nlive), dim3(256), lds, g_stream, B); })) return rc;
    unsigned long long w[PLO_COB_BATCH] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(w, cx.cob_buf, 8 * (size_t)nlive, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < nlive; ++q) { const uint32_t k = live[q]; cob_decode(w[q], R[k].init, n, prob[k].w0, prob[k].w1, &out[k]); }
    st->algo_bytes = (16ull * m + 8) * nlive;
    return call.done(PLO_OK);
}

int plo_cob_search_range(uint32_t n, uint32_t m, const uint32_t *TM, const uint32_t *Cand, uint32_t row, uint32_t offsetblock,
                         const uint32_t *coeffs, uint32_t ncoeffs, uint32_t p, int32_t w0, int32_t w1,
                         uint64_t first_group, uint64_t ngroups, plo_cob_best_t *out, plo_stats_t *st)
{
    if (!out) return fail(PLO_E_ARG, "null argument");
    { const int rc = cob_check(n, m, TM, Cand, row, offsetblock, coeffs, ncoeffs, p); if (rc != PLO_OK) return rc; }
    if (first_group > (uint64_t)ncoeffs * ncoeffs * ncoeffs || ngroups > (uint64_t)ncoeffs * ncoeffs * ncoeffs - first_group) return fail(PLO_E_ARG, "group range outside the (i,j,k) prefixes");
    if (const int rc = require_device(NOINIT_DEVICE0)) return rc;
    CallScope call(st); st = call.st;
    CobPrep R; cob_prepare(n, m, TM, Cand, row, offsetblock, p, w0, w1, R);
    if (R.dependent) {      // chosen rows are dependent: rank(Cand with row := w) can never exceed `row` (:174)
        out->found = 0; out->zeros_v = w0; out->zeros_w = w1; out->index = 0;
        st->candidates = ngroups * ncoeffs;
        return PLO_OK;                                       // (`seconds` stays 0 here, unlike the batch entry)
    }
    const uint32_t qn = R.qn, fb = R.fb; const std::vector<uint32_t> &nb = R.nb, &tmb = R.tmb; const unsigned long long init = R.init;
    const uint64_t first = first_group * ncoeffs, total = (first_group + ngroups) * ncoeffs;      // flattened (i,j,k,l) range of this call
    const size_t lds = (4 * (size_t)m + 4 * (size_t)qn + ncoeffs) * 4;
    if (lds > g_lds_max) return fail(PLO_E_CAPACITY, "block of TM does not fit LDS");
    // one device buffer kept by the context, one upload: [best word (2) | TM block | nullspace block | coefficients]
    DevCtx &cx = cur_ctx();
    const size_t o_tm = 2, o_nb = o_tm + tmb.size(), o_cf = o_nb + nb.size(), words = o_cf + ncoeffs;
    if (const int rc = cob_scratch(words)) return rc;
    std::vector<uint32_t> up(words);
    memcpy(up.data(), &init, 8); memcpy(up.data() + o_tm, tmb.data(), tmb.size() * 4); memcpy(up.data() + o_nb, nb.data(), nb.size() * 4);
    for (uint32_t x = 0; x < ncoeffs; ++x) up[o_cf + x] = coeffs[x] % p;      // (residues, as TM and Cand: zeros(w) counts them)
    uint32_t *d_tm = cx.cob_buf + o_tm, *d_nb = cx.cob_buf + o_nb, *d_cf = cx.cob_buf + o_cf; unsigned long long *d_best = (unsigned long long *)cx.cob_buf;
    plo::CobJob J{}; J.n = n; J.m = m; J.qn = qn; J.fb = fb; J.C = ncoeffs; J.p = p; J.mu = (~0ull) / p; J.first = first; J.total = total;
    J.tm = d_tm; J.nb = d_nb; J.coeffs = d_cf; J.best = d_best;
    // table form when 4*C*(m+qn) products fit LDS (odd strides: the lanes of a wave read rows l, l+1, ... of one column)
    const uint32_t mstride = m | 1u, qstride = std::max<uint32_t>(qn, 1u) | 1u;
    const size_t lds_tab = 4ull * ncoeffs * ((size_t)mstride + qstride) * 4;
    const bool use_tab = lds_tab <= 72u * 1024u && !getenv("PLO_COB_GENERIC");
    HIPCHK(hipFuncSetAttribute(use_tab ? (const void *)plo::cob_tab_kernel : (const void *)plo::cob_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(use_tab ? lds_tab : lds)));
    const uint64_t grid = use_tab ? std::max<uint64_t>(1, std::min<uint64_t>((ngroups + 3) / 4, (uint64_t)g_cus * 2)) : std::max<uint64_t>(1, std::min<uint64_t>((total - first + 255) / 256, (uint64_t)g_cus * 8));
    if (const int rc = cob_launch(up, grid, use_tab ? lds_tab : lds, st, [&] {
            if (use_tab) hipLaunchKernelGGL(plo::cob_tab_kernel, dim3((uint32_t)grid), dim3(256), lds_tab, g_stream, J, mstride, qstride);
            else hipLaunchKernelGGL(plo::cob_kernel, dim3((uint32_t)grid), dim3(256), lds, g_stream, J);
        })) return rc;
    unsigned long long w = 0;
    HIPCHK(hipMemcpy(&w, d_best, 8, hipMemcpyDeviceToHost));
    cob_decode(w, init, n, w0, w1, out);
    st->candidates = total - first;
    st->algo_bytes = 16ull * m + 8;                       // the 4 x m block of TM, once, plus the result word
    return call.done(PLO_OK);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------- trilplacer
// what the plans of the atom kernels (trilplacer, inplacer) share
struct AtomsPlan {
    void *d_img = nullptr; uint32_t *d_err = nullptr; unsigned long long *d_best = nullptr;
    uint32_t waves_per_wg = 4, lds_bytes = 0, blocks_per_cu = 1;
    uint64_t algo_bytes = 0;
    bool rational = false;           // coefficients other than +-1: residues modulo a 31-bit prime (PLO_TRIL_PRIME), the kernel's <true> instantiation
};
struct plo_tril_plan : AtomsPlan { plo::TrilPlan P{}; };
struct plo_lin_plan : AtomsPlan { plo::LinPlan P{}; };

namespace {
// Launch of a trilplacer or inplacer job (one wavefront per candidate, plo::TrilJob): `kernel` is the plan's instantiation, `tool` names it in the error text
template <class Plan, class Kernel> int atoms_launch(Plan *pl, Kernel kernel, const char *tool, plo::TrilJob J, plo_stats_t *st) {
    J.err = pl->d_err;
    const uint64_t grid = grid_for(J.ncand, pl->waves_per_wg, (uint64_t)g_cus * pl->blocks_per_cu);
    const int err = checked_launch(pl->d_err, st, LaunchShape{grid, pl->lds_bytes, pl->waves_per_wg, pl->algo_bytes},
                                   [&] { hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J); });
    if (err < 0) return err;
    st->candidates += J.ncand;
    if (err) return fail(err == plo::TERR_CAP ? PLO_E_INTERNAL : PLO_E_UNSUPPORTED, std::string("device (") + tool + "): error " + std::to_string(err));
    return PLO_OK;
}

// Body of a plo_*_cost_many entry of these searches: `width` words per candidate come back in `out`; launch(d_out, d_seeds, st) fills in
// the job and launches it
template <class Launch> int cost_many_run(const void *pl, const uint64_t *seeds, uint64_t n, uint32_t width, uint32_t *out, plo_stats_t *stats, Launch launch) {
    if (const int rc = require_device(NOINIT_PLAN)) return rc;      // (the device before the arguments, here and in atoms_search)
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    if (n >= (1ull << 31)) return fail(PLO_E_ARG, "at most 2^31-1 candidates per call");
    CallScope call(stats); plo_stats_t *st = call.st;
    if (n == 0) return PLO_OK;                                       // (`seconds` stays 0)
    DevBuf<uint32_t> d_out; DevBuf<uint64_t> d_seeds;
    HIPCHK(hipMalloc((void **)&d_out.p, n * width * sizeof(uint32_t)));
    if (seeds && (hipMalloc((void **)&d_seeds.p, n * 8) != hipSuccess || hipMemcpy(d_seeds, seeds, n * 8, hipMemcpyHostToDevice) != hipSuccess)) return fail(PLO_E_HIP, "seed upload");
    int rc = launch(d_out.p, d_seeds.p, st);
    if (rc == PLO_OK && hipMemcpy(out, d_out, n * width * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PLO_E_HIP, "copy back");
    return call.done(rc);
}

int tril_launch(plo_tril_plan *pl, plo::TrilJob J, plo_stats_t *st) {
    const int rc = atoms_launch(pl, pl->rational ? plo::tril_kernel<true> : plo::tril_kernel<false>, "trilplacer", J, st);
#ifdef PLO_TRIL_PROFILE
    { unsigned long long gp[8] = {0}; if (hipMemcpyFromSymbol(gp, HIP_SYMBOL(plo::g_tprof), sizeof gp) == hipSuccess && gp[5]) fprintf(stderr, "# tril profile (wave 0 of every workgroup, %llu candidates): cycles per candidate: perm %.0f build %.0f pushvariables %.0f simplify %.0f; fixpoint trips %.1f\n", gp[5], (double)gp[0] / gp[5], (double)gp[1] / gp[5], (double)gp[2] / gp[5], (double)gp[3] / gp[5], (double)gp[4] / gp[5]); }
#endif
    return rc;
}
int lin_launch(plo_lin_plan *pl, plo::TrilJob J, plo_stats_t *st) {
    return atoms_launch(pl, pl->rational ? plo::lin_kernel<true> : plo::lin_kernel<false>, "inplacer", J, st);
}

template <class Plan> void atoms_destroy(Plan *pl) {
    if (pl) { dev_free(pl->d_img, pl->d_err, pl->d_best); delete pl; }
}

// ---- the plo::TrilMat image of a rational CSR matrix.  Entries num/den: all +-1 gives the unit kernel (small signed values);
// otherwise the residues modulo PLO_TRIL_PRIME and the rational instantiation of the kernel (plo_tril.hip, plo_lin.hip).
#define PLO_TRIL_PRIME 2147483629u
// the rows of M as the device takes them, or the refusal; `unit` is cleared by an entry other than +-1
int trilmat_check(const plo_qcsr_t *M, bool empty_row_ok, bool &unit) {
    for (uint32_t i = 0; i < M->m; ++i) {
        const uint32_t len = M->rowptr[i + 1] - M->rowptr[i];
        if (len == 0 && !empty_row_ok) return fail(PLO_E_UNSUPPORTED, "empty row: host path only");
        if (len > 64) return fail(PLO_E_UNSUPPORTED, "row with more than 64 entries: host path only");
        for (uint32_t e = M->rowptr[i]; e < M->rowptr[i + 1]; ++e) {
            const int64_t nu = M->num[e], de = M->den ? M->den[e] : 1;
            if (nu == 0 || de == 0) return fail(PLO_E_ARG, "zero entry or zero denominator");
            if (!(de == 1 && (nu == 1 || nu == -1))) unit = false;
            if (de % (int64_t)PLO_TRIL_PRIME == 0 || nu % (int64_t)PLO_TRIL_PRIME == 0) return fail(PLO_E_UNSUPPORTED, "entry not a unit modulo the device's prime: host path only");
            if (M->col[e] >= M->n || (e > M->rowptr[i] && M->col[e] <= M->col[e - 1])) return fail(PLO_E_ARG, "columns must be sorted and in range");
        }
    }
    return PLO_OK;
}
// bytes of its image: rp, col, val, valp, each rounded to 16
size_t trilmat_bytes(const plo_qcsr_t *M) {
    const uint32_t nnz = M->rowptr[M->m];
    return round_up((M->m + 1) * 2, 16) + round_up(nnz * 2, 16) + round_up(nnz, 16) + round_up(nnz * 4, 16);
}
// writes that image at img + off (and advances off); D gets the shape and the pointers into the device copy at d_img
void trilmat_fill(const plo_qcsr_t *M, bool unit, uint8_t *img, const void *d_img, size_t &off, plo::TrilMat &D) {
    const uint32_t nnz = M->rowptr[M->m];
    D.m = M->m; D.n = M->n; D.nnz = nnz;
    uint16_t *rp = (uint16_t *)(img + off); D.rp = (const uint16_t *)((const uint8_t *)d_img + off); off += round_up((M->m + 1) * 2, 16);
    uint16_t *cl = (uint16_t *)(img + off); D.col = (const uint16_t *)((const uint8_t *)d_img + off); off += round_up(nnz * 2, 16);
    int8_t *vl = (int8_t *)(img + off); D.val = (const int8_t *)((const uint8_t *)d_img + off); off += round_up(nnz, 16);
    uint32_t *vp = (uint32_t *)(img + off); D.valp = (const uint32_t *)((const uint8_t *)d_img + off); off += round_up(nnz * 4, 16);
    for (uint32_t i = 0; i <= M->m; ++i) rp[i] = (uint16_t)M->rowptr[i];
    for (uint32_t e = 0; e < nnz; ++e) {
        cl[e] = (uint16_t)M->col[e];
        const int64_t nu = M->num[e], de = M->den ? M->den[e] : 1;
        vl[e] = unit ? (int8_t)nu : 0;
        int64_t a = nu % (int64_t)PLO_TRIL_PRIME, d = de % (int64_t)PLO_TRIL_PRIME; if (a < 0) a += PLO_TRIL_PRIME; if (d < 0) d += PLO_TRIL_PRIME;
        vp[e] = (uint32_t)((uint64_t)a * inv_mod((uint32_t)d, PLO_TRIL_PRIME) % PLO_TRIL_PRIME);
    }
}

// workgroups of `waves` waves and `lds` bytes that the 160 KiB of LDS and the 32 waves of a CU admit
uint32_t blocks_per_cu(uint32_t waves, uint32_t lds) { return std::max<uint32_t>(1, std::min<uint32_t>(32u / waves, (uint32_t)(g_lds_max / lds))); }

// A new plan with the device buffer of an image of `bytes` bytes (the TrilMat pointers point into it before it is filled), or null
template <class Plan> Plan *atoms_new(size_t bytes, bool unit) {
    Plan *pl = new Plan();
    pl->rational = !unit;
    if (hipMalloc(&pl->d_img, bytes) != hipSuccess) { delete pl; fail(PLO_E_HIP, "hipMalloc"); return nullptr; }
    return pl;
}

// The end of both create functions: four waves (256 threads) per workgroup, one when four do not fit 64 KiB, as many workgroups per CU
// as LDS and waves admit; then the image, the error and best words and the kernel's dynamic-LDS limit.  A failure destroys the plan.
template <class Plan> int atoms_finish(Plan *pl, uint32_t lds_per_wave, const std::vector<uint8_t> &img, const void *kernel, const char *tool, Plan **plan) {
    pl->waves_per_wg = 4;
    pl->lds_bytes = lds_per_wave * pl->waves_per_wg;
    if (pl->lds_bytes > 64u * 1024u) { pl->waves_per_wg = 1; pl->lds_bytes = lds_per_wave; }
    if (pl->lds_bytes > g_lds_max) { atoms_destroy(pl); return fail(PLO_E_CAPACITY, "program does not fit LDS"); }
    pl->blocks_per_cu = blocks_per_cu(pl->waves_per_wg, pl->lds_bytes);
    if (hipMemcpy(pl->d_img, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess || hipMalloc((void **)&pl->d_err, 4) != hipSuccess ||
        hipMalloc((void **)&pl->d_best, 8) != hipSuccess || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl->lds_bytes) != hipSuccess) {
        atoms_destroy(pl); return fail(PLO_E_HIP, std::string("device setup of the ") + tool + " plan failed");
    }
    *plan = pl;
    return PLO_OK;
}

// Body of plo_tril_cost_many and plo_lin_cost_many: the six counts of every candidate
template <class Plan> int atoms_cost_many(Plan *pl, int (*launch)(Plan *, plo::TrilJob, plo_stats_t *), const uint64_t *seeds, uint64_t seed0, uint64_t n, uint32_t *ops6, plo_stats_t *stats) {
    return cost_many_run(pl, seeds, n, 6, ops6, stats, [&](uint32_t *d_ops, const uint64_t *d_seeds, plo_stats_t *st) {
        plo::TrilJob J{}; J.seed0 = seed0; J.seeds = d_seeds; J.ncand = n; J.ops = d_ops; J.best = nullptr;
        return launch(pl, J, st);
    });
}

// Body of plo_tril_search and plo_lin_search: *w gets the packed word of the best candidate, (ADD << 48 | SCA << 32 | (seed - seed0) << 1 | variant)
template <class Plan> int atoms_search(Plan *pl, const void *best, int (*launch)(Plan *, plo::TrilJob, plo_stats_t *), uint64_t seed0, uint64_t nseeds, unsigned long long *w, plo_stats_t *stats) {
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    if (!pl || !best) return fail(PLO_E_ARG, "null argument");
    if (nseeds == 0 || nseeds >= (1ull << 31)) return fail(PLO_E_ARG, "1 .. 2^31-1 candidates per call");
    CallScope call(stats); plo_stats_t *st = call.st;
    const unsigned long long init = ~0ull;
    HIPCHK(hipMemcpy(pl->d_best, &init, 8, hipMemcpyHostToDevice));
    plo::TrilJob J{}; J.seed0 = seed0; J.seeds = nullptr; J.ncand = nseeds; J.ops = nullptr; J.best = pl->d_best;
    int rc = launch(pl, J, st);
    if (rc != PLO_OK) return rc;
    HIPCHK(hipMemcpy(w, pl->d_best, 8, hipMemcpyDeviceToHost));
    if (*w == init) return fail(PLO_E_INTERNAL, "no candidate reported");
    return call.done(PLO_OK);
}
} // namespace

extern "C" {

int plo_tril_plan_create(const plo_icsr_t *A, const plo_icsr_t *B, const plo_icsr_t *T, plo_tril_plan_t **plan) { return plo_tril_plan_create_x(A, B, T, 0, plan); }

int plo_tril_plan_create_q(const plo_qcsr_t *A, const plo_qcsr_t *B, const plo_qcsr_t *T, int expanded, plo_tril_plan_t **plan)
{
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    if (!A || !B || !T || !plan) return fail(PLO_E_ARG, "null argument");
    const plo_qcsr_t *Ms[3] = {A, B, T};
    if (A->m == 0 || A->m != B->m || A->m != T->m) return fail(PLO_E_ARG, "A, B and T (transposed product matrix) need the same number of rows");
    if (A->m > 16382u) return fail(PLO_E_CAPACITY, "more than 16382 rows");
    uint32_t cap = 0; size_t bytes = 0; uint64_t algo = 8; bool unit = true;
    for (const plo_qcsr_t *M : Ms) {
        if (!M->rowptr || !M->col || !M->num || M->n == 0 || M->n > 16382u) return fail(PLO_E_ARG, "bad matrix (at most 16382 variables)");
        const uint32_t nnz = M->rowptr[M->m];
        if (nnz > 65535u) return fail(PLO_E_CAPACITY, "more than 65535 non-zeros");
        if (const int rc = trilmat_check(M, false, unit)) return rc;
        cap = std::max(cap, 2u * nnz + 3u * M->m);
        if (expanded && M == T) cap = std::max(cap, 4u * nnz + 6u * M->m);        // TransposedDoubleAlgorithm: 4(len-1)+2 atoms per row, and 4 scaling atoms when the pivot is not +-1
        if (expanded && M == T && M->n >= 16382u) return fail(PLO_E_CAPACITY, "one more variable of c than the atom holds");
        bytes += trilmat_bytes(M);
        algo += 2ull * (M->m + 1) + 3ull * nnz;                 // the CSR image of the three matrices, once per candidate
    }
    cap = round_up(cap + 2, 64);
    plo_tril_plan *pl = atoms_new<plo_tril_plan>(bytes, unit);
    if (!pl) return PLO_E_HIP;
    std::vector<uint8_t> img(bytes, 0);
    size_t off = 0;
    for (int w = 0; w < 3; ++w) trilmat_fill(Ms[w], unit, img.data(), pl->d_img, off, pl->P.M[w]);
    pl->P.cap = cap; pl->P.expanded = expanded ? 1u : 0u; pl->P.p = unit ? 0u : PLO_TRIL_PRIME;
    pl->P.lds_per_wave = round_up(8u * cap + 2u * ((A->m + 1u) & ~1u) + A->m, 16) + 16u * ((cap + 63u) / 64u);   // atoms, permutation, signs; masks of a pushvariables pass
    pl->algo_bytes = algo;
    return atoms_finish(pl, pl->P.lds_per_wave, img, pl->rational ? (const void *)plo::tril_kernel<true> : (const void *)plo::tril_kernel<false>, "trilplacer", plan);
}

// integer entries (the interface of rounds 1-2): the same builder with denominators 1
int plo_tril_plan_create_x(const plo_icsr_t *A, const plo_icsr_t *B, const plo_icsr_t *T, int expanded, plo_tril_plan_t **plan)
{
    if (!A || !B || !T || !plan) return fail(PLO_E_ARG, "null argument");
    const plo_icsr_t *Ms[3] = {A, B, T};
    std::vector<int64_t> nums[3]; plo_qcsr_t Q[3];
    for (int w = 0; w < 3; ++w) {
        if (!Ms[w]->rowptr || !Ms[w]->col || !Ms[w]->val) return fail(PLO_E_ARG, "bad matrix");
        const uint32_t nnz = Ms[w]->rowptr[Ms[w]->m];
        nums[w].assign(Ms[w]->val, Ms[w]->val + nnz);
        Q[w] = plo_qcsr_t{Ms[w]->m, Ms[w]->n, Ms[w]->rowptr, Ms[w]->col, nums[w].data(), nullptr};
    }
    return plo_tril_plan_create_q(&Q[0], &Q[1], &Q[2], expanded, plan);
}

void plo_tril_plan_destroy(plo_tril_plan_t *pl) { atoms_destroy(pl); }

int plo_tril_cost_many(plo_tril_plan_t *pl, const uint64_t *seeds, uint64_t seed0, uint64_t n, uint32_t *ops6, plo_stats_t *stats) { return atoms_cost_many(pl, tril_launch, seeds, seed0, n, ops6, stats); }

int plo_tril_search(plo_tril_plan_t *pl, uint64_t seed0, uint64_t nseeds, plo_tril_best_t *best, plo_stats_t *stats)
{
    unsigned long long w = 0;
    if (const int rc = atoms_search(pl, best, tril_launch, seed0, nseeds, &w, stats)) return rc;
    best->add = (uint32_t)(w >> 48); best->sca = (uint32_t)(w >> 32) & 0xFFFFu; best->mul = pl->P.M[0].m;
    best->variant = (uint32_t)(w & 1ull); best->seed = seed0 + ((w & 0xFFFFFFFFull) >> 1);
    return PLO_OK;
}

int plo_kernel_search_multi(const plo_csr_t *M, uint32_t p, uint64_t seed0, uint64_t nrestarts, uint32_t per_block, int cost_mode,
                            int ndev, const int *devices, plo_best_t *out, plo_stats_t *stats)
{
    if (!M || !out) return fail(PLO_E_ARG, "null argument");
    if (ndev < 1 || ndev > 64) return fail(PLO_E_ARG, "device count outside [1,64]");
    if (cost_mode < 0 || cost_mode > 2) return fail(PLO_E_ARG, "unknown cost mode");
    if (per_block != 1u && ndev > 1) return fail(PLO_E_ARG, "shards of the kernel method take one decomposition per restart (per_block = 1)");
    return planless_search_multi(seed0, nrestarts, cost_mode, ndev, devices, out, stats,
        [&](uint64_t s0, uint64_t cnt, plo_best_t *b, plo_stats_t *st) { return plo_kernel_search(M, p, s0, cnt, per_block, cost_mode, nullptr, nullptr, nullptr, b, st); });
}

int plo_tril_search_multi(const plo_qcsr_t *A, const plo_qcsr_t *B, const plo_qcsr_t *T, int expanded, uint64_t seed0, uint64_t nseeds,
                          int ndev, const int *devices, plo_tril_best_t *best, plo_stats_t *stats)
{
    if (!A || !B || !T || !best) return fail(PLO_E_ARG, "null argument");
    return sharded_search(seed0, nseeds, ndev, devices, best, stats,
        [&](plo_tril_plan_t **plan) { return plo_tril_plan_create_q(A, B, T, expanded, plan); }, plo_tril_search, plo_tril_plan_destroy,
        [&](const plo_tril_best_t &pb) { return std::make_pair(((unsigned long long)pb.add << 32) | pb.sca, ((pb.seed - seed0) << 1) | (pb.variant & 1u)); });      // the order of include/plinopt_inplace.inl:893-897, then (seed, variant)
}

} // extern "C"

// ---------------------------------------------------------------------------------------------- inplacer
extern "C" {

int plo_lin_plan_create_q(const plo_qcsr_t *A, plo_lin_plan_t **plan)
{
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    if (!A || !plan) return fail(PLO_E_ARG, "null argument");
    if (!A->rowptr || !A->col || !A->num || A->m == 0 || A->n == 0) return fail(PLO_E_ARG, "bad matrix");
    if (A->m > 16382u || A->n > 16382u) return fail(PLO_E_CAPACITY, "more than 16382 rows or columns (an atom holds 14-bit variables)");
    const uint32_t m = A->m, nnz = A->rowptr[m];
    bool unit = true;
    if (const int rc = trilmat_check(A, true, unit)) return rc;
    // the concatenation of variant 1: the simplified program of variant 0 (at most 2 nnz + m atoms) and the oriented one,
    // checked row by row against 2 len + 2 more atoms (t_linear)
    // (nnz <= 64 m <= 64 * 16382 here: no overflow)
    const uint32_t cap = round_up(4u * nnz + 3u * m + 2u, 64);
    if (cap > 65535u) return fail(PLO_E_CAPACITY, "program does not fit LDS (and counts of 16 bits in the packed key)");
    const size_t bytes = trilmat_bytes(A) + 16;
    plo_lin_plan *pl = atoms_new<plo_lin_plan>(bytes, unit);
    if (!pl) return PLO_E_HIP;
    std::vector<uint8_t> img(bytes, 0);
    size_t off = 0;
    trilmat_fill(A, unit, img.data(), pl->d_img, off, pl->P.M);
    pl->P.cap = cap; pl->P.p = unit ? 0u : PLO_TRIL_PRIME;
    pl->P.lds_per_wave = round_up(8u * cap + 2u * ((m + 1u) & ~1u), 16);      // atoms, permutation
    pl->algo_bytes = 8 + 2ull * (m + 1) + 3ull * nnz;                           // the CSR image, once per candidate
    return atoms_finish(pl, pl->P.lds_per_wave, img, pl->rational ? (const void *)plo::lin_kernel<true> : (const void *)plo::lin_kernel<false>, "inplacer", plan);
}

void plo_lin_plan_destroy(plo_lin_plan_t *pl) { atoms_destroy(pl); }

int plo_lin_cost_many(plo_lin_plan_t *pl, const uint64_t *seeds, uint64_t seed0, uint64_t n, uint32_t *ops6, plo_stats_t *stats) { return atoms_cost_many(pl, lin_launch, seeds, seed0, n, ops6, stats); }

int plo_lin_search(plo_lin_plan_t *pl, uint64_t seed0, uint64_t nseeds, plo_lin_best_t *best, plo_stats_t *stats)
{
    unsigned long long w = 0;
    if (const int rc = atoms_search(pl, best, lin_launch, seed0, nseeds, &w, stats)) return rc;
    best->add = (uint32_t)(w >> 48); best->sca = (uint32_t)(w >> 32) & 0xFFFFu;
    best->variant = (uint32_t)(w & 1ull); best->rows = pl->P.M.m * (best->variant + 1u);       // one barrier per row, twice in variant 1
    best->seed = seed0 + ((w & 0xFFFFFFFFull) >> 1);
    return PLO_OK;
}

int plo_lin_search_multi(const plo_qcsr_t *A, uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_lin_best_t *best, plo_stats_t *stats)
{
    if (!A || !best) return fail(PLO_E_ARG, "null argument");
    return sharded_search(seed0, nseeds, ndev, devices, best, stats,
        [&](plo_lin_plan_t **plan) { return plo_lin_plan_create_q(A, plan); }, plo_lin_search, plo_lin_plan_destroy,
        [&](const plo_lin_best_t &pb) { return std::make_pair(((unsigned long long)pb.add << 32) | pb.sca, ((pb.seed - seed0) << 1) | (pb.variant & 1u)); });      // (ADD, SCA) of :637-641, then (seed, variant)
}

} // extern "C"

// ---------------------------------------------------------------------------------------------- orbiter
struct plo_orbit_plan {
    plo::OrbitPlan P{};
    void *d_img = nullptr; uint64_t *d_best = nullptr;
    uint32_t waves_per_wg = 4, lds_bytes = 0, blocks_per_cu = 1, grid_max = 1;
    uint64_t algo_bytes = 0;
    int action = PLO_ORBIT_ACT_TRIANGULAR;
    // PLO_ORBIT_CSE (plo_orbit_cse.hip): the layouts, the sampled bounds they come from and how often they were outgrown
    bool cse = false;
    plo::OrbitCsePlan C{};
    uint32_t *d_err = nullptr;
    uint32_t cse_scale = 1, cse_relaunches = 0;        // tables: scale x the sampled size; launches repeated for a full table
    uint32_t cse_ent[3] = {0, 0, 0}, cse_pairs[3] = {0, 0, 0};   // maxima over the sizing sample, per part
    // PLO_ORBIT_GROWTH (plo_orbit_growth.hip): the 3r sums behind a wave's region (zero on the other plans); d_best then has three words per wave slot
    bool growth = false;
    uint32_t g_off_sum = 0, g_wave_bytes = 0;
};

namespace {
// m, k, n from L (r x mk), R (r x kn), P (mn x r): n = sqrt(kn mn / mk) exactly
bool orbit_shape(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint32_t &m, uint32_t &k, uint32_t &n) {
    if (L->m != R->m || L->m != P->n || L->n == 0 || R->n == 0 || P->m == 0) return false;
    const uint64_t num = (uint64_t)R->n * P->m;
    if (num % L->n) return false;
    const uint64_t q = num / L->n;
    uint64_t s = 0;
    for (uint64_t b = 1ull << 31; b; b >>= 1) if ((s | b) * (s | b) <= q) s |= b;
    if (s == 0 || s * s != q || P->m % s || R->n % s) return false;
    n = (uint32_t)s; m = P->m / n; k = R->n / n;
    return (uint64_t)m * k == L->n && (uint64_t)k * n == R->n && (uint64_t)m * n == P->m;
}

const char *qcsr_defect(const plo_qcsr_t *A) {
    if (!A->rowptr || (A->rowptr[A->m] && (!A->col || !A->num))) return "null arrays";
    for (uint32_t i = 0; i < A->m; ++i) {
        if (A->rowptr[i + 1] < A->rowptr[i]) return "row pointers decrease";
        for (uint32_t e = A->rowptr[i]; e < A->rowptr[i + 1]; ++e) {
            if (A->num[e] == 0 || (A->den && A->den[e] <= 0)) return "zero entry or non-positive denominator";
            if (A->col[e] >= A->n || (e > A->rowptr[i] && A->col[e] <= A->col[e - 1])) return "columns must be sorted and in range";
        }
    }
    return nullptr;
}
int64_t gcd64(int64_t a, int64_t b) { if (a < 0) a = -a; if (b < 0) b = -b; while (b) { const int64_t t = a % b; a = b; b = t; } return a; }
// the residue of num/den modulo p, false when den is no unit
bool residue_of(int64_t num, int64_t den, uint32_t p, uint32_t &out) {
    int64_t d = den % (int64_t)p, a = num % (int64_t)p;
    if (d < 0) d += p;
    if (a < 0) a += p;
    if (gcd64(d, p) != 1) return false;
    out = (uint32_t)((uint64_t)a * inv_mod((uint32_t)d, p) % p);
    return true;
}

using orbit_fn_t = void (*)(plo::OrbitPlan, plo::OrbitJob);
orbit_fn_t orbit_fn(bool mod, int action) {
    switch (action) {
    case PLO_ORBIT_ACT_PLUQ: return mod ? plo::orbit_kernel<true, 1> : plo::orbit_kernel<false, 1>;
    case PLO_ORBIT_ACT_HOUSEHOLDER: return mod ? plo::orbit_kernel<true, 2> : plo::orbit_kernel<false, 2>;
    default: return mod ? plo::orbit_kernel<true> : plo::orbit_kernel<false>;
    }
}

// ---- PLO_ORBIT_CSE
using orbit_cse_fn_t = void (*)(plo::OrbitPlan, plo::OrbitJob, plo::OrbitCsePlan, uint32_t *);
orbit_cse_fn_t orbit_cse_fn(int action, bool size) {
    switch (action) {
    case PLO_ORBIT_ACT_PLUQ: return size ? plo::orbit_cse_kernel<1, true> : plo::orbit_cse_kernel<1, false>;
    case PLO_ORBIT_ACT_HOUSEHOLDER: return size ? plo::orbit_cse_kernel<2, true> : plo::orbit_cse_kernel<2, false>;
    default: return size ? plo::orbit_cse_kernel<0, true> : plo::orbit_cse_kernel<0, false>;
    }
}
using orbit_growth_fn_t = void (*)(plo::OrbitPlan, plo::OrbitGrowthJob);
orbit_growth_fn_t orbit_growth_fn(int action) { return action == PLO_ORBIT_ACT_PLUQ ? plo::orbit_growth_kernel<1> : plo::orbit_growth_kernel<0>; }
enum { ORBIT_AGAIN = 1 };            // orbit_launch: a table was full, the plan has larger ones now: launch again

// deterministic Miller-Rabin below 2^32 (bases 2, 7, 61)
bool is_prime32(uint64_t n) {
    if (n < 2) return false;
    for (uint64_t q : {2ull, 3ull, 5ull, 7ull, 61ull}) { if (n == q) return true; if (n % q == 0) return false; }
    uint64_t d = n - 1; int s = 0; while (!(d & 1)) { d >>= 1; ++s; }
    auto pw = [&](uint64_t b, uint64_t e) { uint64_t x = 1; b %= n; for (; e; e >>= 1) { if (e & 1) x = x * b % n; b = b * b % n; } return x; };
    for (uint64_t a : {2ull, 7ull, 61ull}) {
        uint64_t x = pw(a, d); if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int i = 1; i < s && comp; ++i) { x = x * x % n; if (x == n - 1) comp = false; }
        if (comp) return false;
    }
    return true;
}

// The three image layouts of a CSE plan from its sampled bounds and cse_scale, the wave's region, the waves per workgroup (the
// count that puts most waves on a CU, as the other wave plans) and the per-wave words of the search.
int orbit_cse_layout(plo_orbit_plan *pl)
{
    plo::OrbitPlan &Q = pl->P; plo::OrbitCsePlan &C = pl->C;
    const uint32_t r = Q.r, mk = Q.m * Q.k, kn = Q.k * Q.n, mn = Q.m * Q.n, p = (uint32_t)Q.p;
    const uint32_t rows[3] = {r, r, mn}, cols[3] = {mk, kn, r};
    const auto cap0 = env_knob("PLO_ORBIT_CSE_CAP");          // test knob: the slots of the first tables (a full table repeats the launch with twice as many)
    uint32_t region = 0, keep_all = 0, keep_ent = 0;
    for (int i = 0; i < 3; ++i) {
        const uint32_t hard = rows[i] * cols[i];
        // entries: the sample + 60 % (what the kernel method's Dep images use), the hard bound once a launch has been repeated
        const uint32_t ent = pl->cse_scale == 1 ? std::min<uint32_t>(hard, pl->cse_ent[i] + (uint32_t)((uint64_t)pl->cse_ent[i] * 60u / 100u) + 16u) : hard;
        // table: 0.75 x the sampled pair instances (an upper bound of the distinct triples) x scale
        uint32_t cap = 64;
        if (cap0 && *cap0 >= 64) while (cap < (uint64_t)*cap0 * pl->cse_scale) cap <<= 1;
        else while (cap < ((uint64_t)pl->cse_scale * pl->cse_pairs[i] * 3u) / 4u + 16u && cap < (1u << 17)) cap <<= 1;
        if (cap > 65536u) return fail(PLO_E_CAPACITY, "CSE measure: a pair table of more than 65536 slots");
        const uint64_t NC = (uint64_t)cols[i] + ent / 2 + 2;
        if (NC >= 0xFFFFull || 2u * ceil_log2((uint32_t)NC) + ceil_log2(p) > 51u) return fail(PLO_E_CAPACITY, "CSE measure: pair key (col,col,ratio) does not fit 51 bits for this shape and modulus");
        if (2ull * ent >= 65535ull) return fail(PLO_E_CAPACITY, "CSE measure: op-count may exceed 16 bits");
        const int rc = layout_plan(C.W[i], rows[i], cols[i], ent, p, cols[i], ent, cap);
        if (rc != PLO_OK) return rc;
        region = std::max(region, C.W[i].region_bytes);
        keep_all = std::max(keep_all, C.W[i].tmpl_bytes); keep_ent = std::max(keep_ent, C.W[i].off_cmask - C.W[i].off_val);
    }
    C.off_rs = round_up(Q.lds_per_wave, 16);
    C.off_img = C.off_rs + round_up(66u * 2u, 16);
    C.off_keep = C.off_img + round_up(region, 16);
    // the kept copy: the whole template (faster) where one wave with it fits LDS, else the entries alone
    for (;;) {
        C.wave_bytes = C.off_keep + (C.sub > 1u ? round_up(C.keep_full ? keep_all : keep_ent, 16) : 0u);
        pl->waves_per_wg = pick_waves([&](uint32_t w) { return (uint64_t)Q.shared_bytes + (uint64_t)w * C.wave_bytes; }, true, g_lds_max, &pl->lds_bytes);
        if (pl->waves_per_wg || !C.keep_full || C.sub == 1u) break;
        C.keep_full = 0;
    }
    if (!pl->waves_per_wg) return fail(PLO_E_CAPACITY, pl->cse_scale == 1 ? "CSE measure: the image of a candidate does not fit LDS with one wave" : "CSE measure: a pair table was full and a larger one does not fit LDS");
    pl->blocks_per_cu = blocks_per_cu(pl->waves_per_wg, pl->lds_bytes);
    pl->grid_max = (uint32_t)g_cus * pl->blocks_per_cu;
    if (pl->d_best) { (void)hipFree(pl->d_best); pl->d_best = nullptr; }
    HIPCHK(hipMalloc((void **)&pl->d_best, 16ull * pl->grid_max * pl->waves_per_wg));
    HIPCHK(hipFuncSetAttribute((const void *)orbit_cse_fn(pl->action, false), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl->lds_bytes));
    return PLO_OK;
}

// The sizing launch: entries and pair instances of the three parts, maxima over the base candidate and seeds 0 .. 254
int orbit_cse_size(plo_orbit_plan *pl)
{
    const plo::OrbitPlan &Q = pl->P;
    plo::OrbitCsePlan C{};
    C.off_rs = round_up(Q.lds_per_wave, 16); C.off_img = C.off_rs + round_up(66u * 2u, 16); C.off_keep = C.off_img + 128u; C.wave_bytes = C.off_keep;
    uint32_t lds = 0;
    const uint32_t W = pick_waves([&](uint32_t w) { return (uint64_t)Q.shared_bytes + (uint64_t)w * C.wave_bytes; }, false, g_lds_max, &lds);
    if (!W) return fail(PLO_E_CAPACITY, "input does not fit LDS");
    std::vector<uint64_t> seeds(256); seeds[0] = PLO_ORBIT_BASE_SEED; for (uint64_t j = 1; j < 256; ++j) seeds[j] = j - 1;
    DevBuf<uint64_t> d_seeds; DevBuf<uint32_t> d_sz;
    HIPCHK(hipMalloc((void **)&d_seeds.p, 256 * 8)); HIPCHK(hipMemcpy(d_seeds, seeds.data(), 256 * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_sz.p, 9 * 4)); HIPCHK(hipMemsetAsync(d_sz, 0, 9 * 4, g_stream));
    const orbit_cse_fn_t fn = orbit_cse_fn(pl->action, true);
    HIPCHK(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    plo::OrbitJob J{}; J.seeds = d_seeds; J.ncand = 256;
    const uint64_t grid = grid_for(J.ncand, W, (uint64_t)g_cus * 2u);
    const int rc = timed_launch((plo_stats_t *)nullptr, nullptr, [&] { hipLaunchKernelGGL(fn, dim3((uint32_t)grid), dim3(64 * W), lds, g_stream, pl->P, J, C, d_sz.p); });
    if (rc != PLO_OK) return rc;
    uint32_t sz[9] = {0};
    HIPCHK(hipMemcpy(sz, d_sz, sizeof sz, hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) { pl->cse_ent[i] = sz[i]; pl->cse_pairs[i] = sz[3 + i]; }
    return PLO_OK;
}

int orbit_launch(plo_orbit_plan *pl, plo::OrbitJob J, plo_stats_t *st) {
    const uint64_t grid = grid_for(J.ncand, pl->waves_per_wg, pl->grid_max);
    if (!pl->cse)
        return timed_launch(pl, grid, J.ncand, st, [&] {
            hipLaunchKernelGGL(orbit_fn(pl->P.p != 0, pl->action), dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J);
        });
    const int err = checked_launch(pl->d_err, st, LaunchShape{grid, pl->lds_bytes, pl->waves_per_wg, pl->algo_bytes}, [&] {
        hipLaunchKernelGGL(orbit_cse_fn(pl->action, false), dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J, pl->C, (uint32_t *)nullptr);
    });
    if (err < 0) return err;
    if (err == plo::ERR_TABLE) {                          // a table or the entry arrays were outgrown: again with twice the slots and the hard entry bound (its candidates are not counted)
        ++pl->cse_relaunches; pl->cse_scale *= 2;
        const int rc = orbit_cse_layout(pl);
        return rc != PLO_OK ? rc : (int)ORBIT_AGAIN;
    }
    if (st) st->candidates += J.ncand;
    if (err) return fail(PLO_E_INTERNAL, "device: error word " + std::to_string(err) + " in the CSE measure of the orbit search");
#ifdef PLO_ORBIT_CSE_PROFILE
    if (getenv("PLO_ORBIT_CSE_STATS")) {
        unsigned long long g[8] = {0};
        if (hipMemcpyFromSymbol(g, HIP_SYMBOL(plo::g_ocprof), sizeof g) == hipSuccess && g[5])
            fprintf(stderr, "# orbit CSE measure, cumulative over %llu candidates: cycles per candidate: factor draw %.0f, sandwich + image build %.0f, Optimizer on Lj %.0f, on Rg %.0f, on hP %.0f\n",
                    g[5], (double)g[0] / g[5], (double)g[1] / g[5], (double)g[2] / g[5], (double)g[3] / g[5], (double)g[4] / g[5]);
    }
#endif
    return PLO_OK;
}

int orbit_growth_launch(plo_orbit_plan *pl, plo::OrbitGrowthJob J, plo_stats_t *st) {
    const uint64_t grid = grid_for(J.ncand, pl->waves_per_wg, pl->grid_max);
    J.off_sum = pl->g_off_sum; J.wave_bytes = pl->g_wave_bytes;
    return timed_launch(pl, grid, J.ncand, st, [&] {
        hipLaunchKernelGGL(orbit_growth_fn(pl->action), dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J);
    });
}

// |entries| of the two factors of a part, a direct one of size sd and an inverse of size si, multiplied:
// triangular 1 x 2^(si-2); PLUQ sd x si 4^(si-2); Householder (numerators over d <= s) sd x si
__int128 orbit_factor_bound(int action, uint32_t sd, uint32_t si) {
    if (action == PLO_ORBIT_ACT_PLUQ) return (__int128)sd * (si >= 2 ? (__int128)si << (2 * (si - 2)) : 1);
    if (action == PLO_ORBIT_ACT_HOUSEHOLDER) return (__int128)sd * si;
    return (__int128)1 << (si >= 2 ? si - 2 : 0);
}

// A plan is built in three steps (orbit_plan_build below).  1: admission.  The order of the checks decides which refusal an input with two defects gets; m, k, n come back.
int orbit_admit(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure, int action, const void *plan, uint32_t &m, uint32_t &k, uint32_t &n) {
    const bool cse = measure == PLO_ORBIT_CSE, growth = measure == PLO_ORBIT_GROWTH;
    if (!L || !R || !P || !plan) return fail(PLO_E_ARG, "null argument");
    if (!cse && !growth && measure != PLO_ORBIT_DENSITY && measure != PLO_ORBIT_CANONICAL) return fail(PLO_E_ARG, "measure must be PLO_ORBIT_DENSITY or PLO_ORBIT_CANONICAL");
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    if (action != PLO_ORBIT_ACT_TRIANGULAR && action != PLO_ORBIT_ACT_PLUQ && action != PLO_ORBIT_ACT_HOUSEHOLDER) return fail(PLO_E_ARG, "action must be one of PLO_ORBIT_ACT_*");
    if (modulus == 1) return fail(PLO_E_ARG, "modulus 1");
    if (!orbit_shape(L, R, P, m, k, n)) return fail(PLO_E_ARG, "shapes are not r x mk, r x kn, mn x r");
    for (const plo_qcsr_t *A : {L, R, P}) if (const char *d = qcsr_defect(A)) return fail(PLO_E_ARG, d);
    if (modulus >= (1ull << 31)) return fail(PLO_E_UNSUPPORTED, "modulus of 2^31 or more: host path only");
    if (m > 16 || k > 16 || n > 16) return fail(PLO_E_CAPACITY, "m, k or n above 16");
    const uint32_t r = L->m;
    if (r > 4096) return fail(PLO_E_CAPACITY, "more than 4096 rows");
    if ((uint64_t)r * (m * k + k * n + m * n) >= (1ull << 21)) return fail(PLO_E_CAPACITY, "2^21 transformed entries or more (21-bit counts in the key)");
    if (cse) {
        if (r > 64 || m * n > 64) return fail(PLO_E_CAPACITY, "CSE measure: r or mn above 64 (ProgramGen of the wave kernel keeps one row per lane)");
        if (m * k > 64 || k * n > 64) return fail(PLO_E_CAPACITY, "CSE measure: mk or kn above 64 (a transformed row of more than 64 entries)");
    }
    return PLO_OK;
}

// 2: the 3r rows of L, of R and of P^T as the kernels take them: residues modulo the modulus, or over Q integers after a scale per
// row, with the proofs that every sum the kernels form stays below 2^62 (and below 2^53 for the growth measure's doubles)
struct OrbitRows { std::vector<int64_t> val, scale; std::vector<uint16_t> pos; std::vector<uint32_t> rp{0}; };
int orbit_rows_image(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint32_t m, uint32_t k, uint32_t n, uint64_t modulus, int action, bool growth, OrbitRows &I) {
    const uint32_t r = L->m;
    // the rows, each as (position, value) lists
    std::vector<std::vector<std::pair<uint16_t, std::pair<int64_t, int64_t>>>> rows(3u * r);
    for (uint32_t i = 0; i < r; ++i) {
        for (uint32_t e = L->rowptr[i]; e < L->rowptr[i + 1]; ++e) rows[i].push_back({(uint16_t)((L->col[e] / k) << 8 | (L->col[e] % k)), {L->num[e], L->den ? L->den[e] : 1}});
        for (uint32_t e = R->rowptr[i]; e < R->rowptr[i + 1]; ++e) rows[r + i].push_back({(uint16_t)((R->col[e] / n) << 8 | (R->col[e] % n)), {R->num[e], R->den ? R->den[e] : 1}});
    }
    for (uint32_t i = 0; i < P->m; ++i)
        for (uint32_t e = P->rowptr[i]; e < P->rowptr[i + 1]; ++e) rows[2u * r + P->col[e]].push_back({(uint16_t)((i / n) << 8 | (i % n)), {P->num[e], P->den ? P->den[e] : 1}});
    std::vector<int64_t> &val = I.val, &scale = I.scale;
    std::vector<uint16_t> &pos = I.pos;
    std::vector<uint32_t> &rp = I.rp;
    scale.assign(3u * r, 1);
    const uint32_t inv_size[3] = {m, k, n};            // the factor of each part with an inverse: U^-1, V^-1, W^-T
    const uint32_t dir_size[3] = {k, n, m};            // and the direct one: V, W, U
    for (uint32_t g = 0; g < 3u * r; ++g) {
        if (modulus) {
            for (auto &e : rows[g]) {
                uint32_t v = 0;
                if (!residue_of(e.second.first, e.second.second, (uint32_t)modulus, v)) return fail(PLO_E_UNSUPPORTED, "a denominator is not invertible modulo the modulus");
                if (v) { pos.push_back(e.first); val.push_back((int64_t)v); }
            }
        } else {
            // scale the row to integers by the lcm of its denominators; |sums| <= L1 * (the factors' entry bounds) < 2^62
            __int128 l = 1;
            for (auto &e : rows[g]) { const int64_t d = e.second.second; l = l / gcd64((int64_t)(l % d), d) * d; if (l > ((__int128)1 << 62)) return fail(PLO_E_UNSUPPORTED, "row scale above 2^62 (int64 bound): host path only"); }
            __int128 l1 = 0;
            for (auto &e : rows[g]) {
                const __int128 v = (__int128)e.second.first * (l / e.second.second);
                l1 += v < 0 ? -v : v;
                if (l1 > ((__int128)1 << 62)) return fail(PLO_E_UNSUPPORTED, "row L1 norm above 2^62 (int64 bound): host path only");
                pos.push_back(e.first); val.push_back((int64_t)v);
            }
            const uint32_t s = inv_size[g / r];
            if (action == PLO_ORBIT_ACT_TRIANGULAR) {
                if ((l1 << (s >= 2 ? s - 2 : 0)) >= ((__int128)1 << 62)) return fail(PLO_E_UNSUPPORTED, "row L1 norm times 2^(s-2) reaches 2^62 (int64 bound): host path only");
            } else {
                // (l1 and l are at most 2^62 and the bound below 2^37: no overflow of the 128-bit products)
                const __int128 fb = orbit_factor_bound(action, dir_size[g / r], s);
                if (l1 * fb >= ((__int128)1 << 62)) return fail(PLO_E_UNSUPPORTED, "row L1 norm times the entry bounds of the action's factors reaches 2^62 (int64 bound): host path only");
                if (action == PLO_ORBIT_ACT_HOUSEHOLDER && l * fb >= ((__int128)1 << 62)) return fail(PLO_E_UNSUPPORTED, "row scale times the Householder denominators reaches 2^62 (int64 bound): host path only");
            }
            if (growth) {
                // S_g <= E_g B_g^2 < 2^53 and c_g < 2^53: double(S_g) and double(c_g) are exact (B_g: the bound on |acc| checked above)
                const __int128 B = action == PLO_ORBIT_ACT_TRIANGULAR ? l1 << (s >= 2 ? s - 2 : 0) : l1 * orbit_factor_bound(action, dir_size[g / r], s);
                const uint32_t E = inv_size[g / r] * dir_size[g / r];
                if (B >= ((__int128)1 << 27) || (__int128)E * B * B >= ((__int128)1 << 53))
                    return fail(PLO_E_UNSUPPORTED, "growth measure: a row's outputs times its squared entry bound reach 2^53 (exact double sums): host path only");
                if (l >= ((__int128)1 << 53)) return fail(PLO_E_UNSUPPORTED, "growth measure: a row scale of 2^53 or more: host path only");
            }
            scale[g] = (int64_t)l;
        }
        rp.push_back((uint32_t)val.size());
    }
    return PLO_OK;
}

// 3: the LDS layout of the shared image and of a wave, the waves per workgroup, and the device side of the plan
int orbit_plan_setup(const OrbitRows &I, uint32_t m, uint32_t k, uint32_t n, uint32_t r, uint64_t modulus, int measure, int action, uint32_t sub, uint64_t cse_seed0, plo_orbit_plan_t **plan) {
    const bool cse = measure == PLO_ORBIT_CSE, growth = measure == PLO_ORBIT_GROWTH;
    const std::vector<int64_t> &val = I.val, &scale = I.scale; const std::vector<uint16_t> &pos = I.pos; const std::vector<uint32_t> &rp = I.rp;
    const uint32_t nnz = (uint32_t)val.size(), nrows = 3u * r, smax = std::max(m, std::max(k, n));
    plo_orbit_plan *pl = new plo_orbit_plan();
    plo::OrbitPlan &Q = pl->P;
    Q.m = m; Q.k = k; Q.n = n; Q.r = r; Q.nnz = nnz; Q.p = modulus;
    // modulo a number every run scores by density, whatever `measure` says (reference src/orbiter.cpp:425)
    Q.measure = modulus ? (uint32_t)PLO_ORBIT_DENSITY : (uint32_t)measure;      // (a CSE plan has a modulus; its kernel does not read this)
    // shared LDS: values, scales, row pointers, positions
    Q.off_scale = round_up(8u * nnz, 16); Q.off_rp = Q.off_scale + round_up(8u * nrows, 16); Q.off_pos = Q.off_rp + round_up(4u * (nrows + 1u), 16);
    Q.shared_bytes = Q.off_pos + round_up(2u * nnz, 16);
    const bool table = action == PLO_ORBIT_ACT_HOUSEHOLDER && modulus;             // 1/d modulo the modulus, d = 0..16
    if (table) { Q.off_dinv = Q.shared_bytes; Q.shared_bytes += round_up(4u * 17u, 16); }
    // a wave: A_L (m x m), B_L (k x k), A_R (k x k), B_R (n x n), A_P (m x m), B_P (n x n), T^-1, T, P and Q, row counters
    const uint32_t sz[6] = {m, k, k, n, m, n};
    uint32_t off = 0;
    for (int f = 0; f < 6; ++f) { Q.off_fac[f] = off; off += round_up(8u * sz[f] * sz[f], 16); }
    Q.off_ti = off; if (action != PLO_ORBIT_ACT_HOUSEHOLDER) off += round_up(8u * smax * smax, 16);       // Householder inverts nothing
    Q.off_t = off; off += action == PLO_ORBIT_ACT_HOUSEHOLDER ? 32u : round_up(smax * smax, 16);      // Householder: u and the signs, 16 bytes each
    if (action == PLO_ORBIT_ACT_PLUQ) {                                             // the second triangle and its inverse
        Q.off_ti2 = off; off += round_up(8u * smax * smax, 16);
        Q.off_t2 = off; off += round_up(smax * smax, 16);
    }
    Q.off_perm = off; off += 32;
    Q.off_cnt = off; if (!growth) off += round_up(2u * nrows + 2u, 16);      // (the growth kernel counts no rows)
    Q.lds_per_wave = off;
    pl->algo_bytes = 10ull * nnz + 12ull * nrows;
    pl->action = action;
    pl->growth = growth;
    if (growth) { pl->g_off_sum = round_up(Q.lds_per_wave, 16); pl->g_wave_bytes = pl->g_off_sum + round_up(24u * r, 16); }       // the 3r sums of squares
    if (!cse) {
        pl->waves_per_wg = pick_waves([&](uint32_t w) { return Q.shared_bytes + w * (growth ? pl->g_wave_bytes : Q.lds_per_wave); }, false, std::min<size_t>(g_lds_max, 64u * 1024u), &pl->lds_bytes);
        if (!pl->waves_per_wg) { delete pl; return fail(PLO_E_CAPACITY, "input does not fit LDS"); }
        pl->blocks_per_cu = blocks_per_cu(pl->waves_per_wg, pl->lds_bytes);
        pl->grid_max = (uint32_t)g_cus * pl->blocks_per_cu;
    }
    // the device image: values, scales, row pointers, positions
    const size_t bytes = (size_t)Q.shared_bytes;
    std::vector<uint8_t> img(bytes, 0);
    if (table)
        for (uint32_t d = 1; d <= 16; ++d)
            if (gcd64((int64_t)d, (int64_t)modulus) == 1) { const uint32_t v = inv_mod((uint32_t)(d % modulus), (uint32_t)modulus); memcpy(img.data() + Q.off_dinv + 4u * d, &v, 4); }
    memcpy(img.data(), val.data(), 8u * nnz); memcpy(img.data() + Q.off_scale, scale.data(), 8u * nrows);
    memcpy(img.data() + Q.off_rp, rp.data(), 4u * (nrows + 1u)); memcpy(img.data() + Q.off_pos, pos.data(), 2u * nnz);
    const void *fn = growth ? (const void *)orbit_growth_fn(action) : (const void *)orbit_fn(modulus != 0, action);
    if (hipMalloc(&pl->d_img, bytes) != hipSuccess || hipMemcpy(pl->d_img, img.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
        (!cse && (hipMalloc((void **)&pl->d_best, (growth ? 24ull : 16ull) * pl->grid_max * pl->waves_per_wg) != hipSuccess ||
                  hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl->lds_bytes) != hipSuccess))) {
        plo_orbit_plan_destroy(pl); return fail(PLO_E_HIP, "device setup of the orbiter plan failed");
    }
    uint8_t *d = (uint8_t *)pl->d_img;
    Q.val = (const int64_t *)d; Q.scale = (const int64_t *)(d + Q.off_scale); Q.rp = (const uint32_t *)(d + Q.off_rp); Q.pos = (const uint16_t *)(d + Q.off_pos);
    if (table) Q.dinv = (const uint32_t *)(d + Q.off_dinv);
    if (cse) {
        // bounds from a sizing launch over a sample of the candidates, then the layouts; a copy of the whole template per wave
        // unless it does not fit, or PLO_ORBIT_CSE_KEEP=0 asks for the entries alone (measured both ways)
        pl->cse = true;
        pl->C.sub = sub; pl->C.seed0 = cse_seed0;
        pl->C.keep_full = env_knob("PLO_ORBIT_CSE_KEEP").value_or(1) != 0 ? 1u : 0u;
        int rc = hipMalloc((void **)&pl->d_err, 4) == hipSuccess ? PLO_OK : fail(PLO_E_HIP, "hipMalloc");
        pl->C.err = pl->d_err;
        if (rc == PLO_OK) rc = orbit_cse_size(pl);
        if (rc == PLO_OK) rc = orbit_cse_layout(pl);
        if (rc != PLO_OK) { const std::string why = g_err; plo_orbit_plan_destroy(pl); return fail(rc, why); }
    }
    *plan = pl;
    return PLO_OK;
}
// the total order of the orbit search as a (hi, lo) word pair for sharded_search: (cost, nnz, nno), then the seed
std::pair<unsigned long long, unsigned long long> orbit_key(const plo_orbit_best_t &pb, uint64_t seed0) { return {((unsigned long long)pb.cost << 42) | ((unsigned long long)pb.nnz << 21) | pb.nno, pb.seed - seed0}; }

// Body of plo_orbit_search and plo_orbit_growth_search.  launch(st) starts the search with pl->d_best as the job's best words and leaves N words per wave slot there, compared
// in order, the last one the candidate (all ones in a slot that saw none); b gets the minimum.  The slots are cleared and launch() called again while it answers ORBIT_AGAIN
// (a CSE plan that outgrew a table has other slots afterwards).
template <size_t N, class Launch> int orbit_search_run(plo_orbit_plan *pl, const void *best, bool growth, uint64_t nseeds, plo_stats_t *stats, std::array<uint64_t, N> &b, Launch launch) {
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    if (!pl || !best) return fail(PLO_E_ARG, "null argument");
    if (pl->growth != growth) return fail(PLO_E_ARG, growth ? "not a plan of plo_orbit_plan_create_growth" : "a growth plan: its cost is a double, plo_orbit_growth_search returns it");
    if (nseeds == 0 || nseeds >= (1ull << 31)) return fail(PLO_E_ARG, "1 .. 2^31-1 candidates per call");
    CallScope call(stats);
    uint64_t slots;
    int rc;
    do {
        slots = (uint64_t)pl->grid_max * pl->waves_per_wg;
        HIPCHK(hipMemsetAsync(pl->d_best, 0xFF, 8 * N * slots, g_stream));
        rc = launch(call.st);
    } while (rc == ORBIT_AGAIN);
    if (rc != PLO_OK) return rc;
    std::vector<uint64_t> w(N * slots);
    HIPCHK(hipMemcpy(w.data(), pl->d_best, 8 * N * slots, hipMemcpyDeviceToHost));
    b.fill(~0ull);
    for (uint64_t s = 0; s < slots; ++s) {
        std::array<uint64_t, N> c;
        std::copy_n(w.begin() + N * s, N, c.begin());
        if (c[N - 1] != ~0ull && c < b) b = c;
    }
    if (b[N - 1] == ~0ull) return fail(PLO_E_INTERNAL, "no candidate reported");
    return call.done(PLO_OK);
}
} // namespace

// the body of the create functions; sub > 0: a PLO_ORBIT_CSE plan
static int orbit_plan_build(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure, int action, uint32_t sub, uint64_t cse_seed0, plo_orbit_plan_t **plan) {
    uint32_t m = 0, k = 0, n = 0;
    if (const int rc = orbit_admit(L, R, P, modulus, measure, action, plan, m, k, n)) return rc;
    OrbitRows I;
    if (const int rc = orbit_rows_image(L, R, P, m, k, n, modulus, action, measure == PLO_ORBIT_GROWTH, I)) return rc;
    return orbit_plan_setup(I, m, k, n, L->m, modulus, measure, action, sub, cse_seed0, plan);
}

extern "C" {

int plo_orbit_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure, plo_orbit_plan_t **plan)
{
    return plo_orbit_plan_create_act(L, R, P, modulus, measure, PLO_ORBIT_ACT_TRIANGULAR, plan);
}

int plo_orbit_plan_create_act(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure, int action, plo_orbit_plan_t **plan)
{
    if (measure == PLO_ORBIT_CSE) return fail(PLO_E_ARG, "PLO_ORBIT_CSE needs sub and cse_seed0: plo_orbit_plan_create_cse");
    // (the growth factor has its own create function; here the measure is refused with the words every unknown measure gets)
    if (measure == PLO_ORBIT_GROWTH) return fail(PLO_E_ARG, !L || !R || !P || !plan ? "null argument" : "measure must be PLO_ORBIT_DENSITY or PLO_ORBIT_CANONICAL");
    return orbit_plan_build(L, R, P, modulus, measure, action, 0, 0, plan);
}

int plo_orbit_plan_create_cse(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int action, uint32_t sub, uint64_t cse_seed0, plo_orbit_plan_t **plan)
{
    if (!L || !R || !P || !plan) return fail(PLO_E_ARG, "null argument");
    if (modulus == 0 || !(modulus & 1) || modulus >= (1ull << 31) || !is_prime32(modulus)) return fail(PLO_E_ARG, "the CSE measure needs an odd prime modulus below 2^31");
    if (sub == 0 || sub > 65536u) return fail(PLO_E_ARG, "sub outside [1, 65536]");
    return orbit_plan_build(L, R, P, modulus, PLO_ORBIT_CSE, action, sub, cse_seed0, plan);
}

int plo_orbit_plan_create_growth(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, int action, plo_orbit_plan_t **plan)
{
    if (!L || !R || !P || !plan) return fail(PLO_E_ARG, "null argument");
    if (action == PLO_ORBIT_ACT_HOUSEHOLDER) return fail(PLO_E_ARG, "the Householder action is orthogonal and preserves the 2-norm growth factor: there is nothing to search");
    return orbit_plan_build(L, R, P, 0, PLO_ORBIT_GROWTH, action, 0, 0, plan);
}

int plo_orbit_plan_info(plo_orbit_plan_t *pl, uint32_t out[8])
{
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    out[0] = pl->waves_per_wg; out[1] = pl->lds_bytes;
    for (int i = 0; i < 3; ++i) out[2 + i] = pl->cse ? pl->C.W[i].cap : 0u;
    out[5] = pl->cse ? std::max(pl->C.W[0].nnz, std::max(pl->C.W[1].nnz, pl->C.W[2].nnz)) : 0u;
    out[6] = pl->cse_relaunches; out[7] = pl->cse ? pl->C.keep_full : 0u;
    return PLO_OK;
}

void plo_orbit_plan_destroy(plo_orbit_plan_t *pl)
{
    if (pl) { dev_free(pl->d_img, pl->d_best, pl->d_err); delete pl; }
}

int plo_orbit_cost_many(plo_orbit_plan_t *pl, const uint64_t *seeds, uint64_t seed0, uint64_t n, uint32_t *out3, plo_stats_t *stats)
{
    if (pl && pl->growth) return fail(PLO_E_ARG, "a growth plan: its cost is a double, plo_orbit_growth_many returns it");
    return cost_many_run(pl, seeds, n, 3, out3, stats, [&](uint32_t *d_out, const uint64_t *d_seeds, plo_stats_t *st) {
        plo::OrbitJob J{}; J.seed0 = seed0; J.seeds = d_seeds; J.ncand = n; J.out3 = d_out; J.best = nullptr;
        int rc;
        do rc = orbit_launch(pl, J, st); while (rc == ORBIT_AGAIN);
        return rc;
    });
}

int plo_orbit_search(plo_orbit_plan_t *pl, uint64_t seed0, uint64_t nseeds, plo_orbit_best_t *best, plo_stats_t *stats)
{
    std::array<uint64_t, 2> b;                            // ((cost, nnz, nno) key, candidate)
    const int rc = orbit_search_run(pl, best, false, nseeds, stats, b, [&](plo_stats_t *st) {
        plo::OrbitJob J{}; J.seed0 = seed0; J.seeds = nullptr; J.ncand = nseeds; J.out3 = nullptr; J.best = pl->d_best;
        return orbit_launch(pl, J, st);
    });
    if (rc != PLO_OK) return rc;
    best->cost = (uint32_t)(b[0] >> 42); best->nnz = (uint32_t)(b[0] >> 21) & 0x1FFFFFu; best->nno = (uint32_t)b[0] & 0x1FFFFFu; best->reserved = 0;
    best->seed = seed0 + b[1];
    return PLO_OK;
}

int plo_orbit_search_multi(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure,
                           uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_best_t *best, plo_stats_t *stats)
{
    return plo_orbit_search_multi_act(L, R, P, modulus, measure, PLO_ORBIT_ACT_TRIANGULAR, seed0, nseeds, ndev, devices, best, stats);
}

int plo_orbit_search_multi_act(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int measure, int action,
                               uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_best_t *best, plo_stats_t *stats)
{
    if (!L || !R || !P || !best) return fail(PLO_E_ARG, "null argument");
    return sharded_search(seed0, nseeds, ndev, devices, best, stats,
        [&](plo_orbit_plan_t **plan) { return plo_orbit_plan_create_act(L, R, P, modulus, measure, action, plan); }, plo_orbit_search, plo_orbit_plan_destroy,
        [&](const plo_orbit_best_t &pb) { return orbit_key(pb, seed0); });
}

int plo_orbit_search_multi_cse(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint64_t modulus, int action, uint32_t sub, uint64_t cse_seed0,
                               uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_best_t *best, plo_stats_t *stats)
{
    if (!L || !R || !P || !best) return fail(PLO_E_ARG, "null argument");
    return sharded_search(seed0, nseeds, ndev, devices, best, stats,
        [&](plo_orbit_plan_t **plan) { return plo_orbit_plan_create_cse(L, R, P, modulus, action, sub, cse_seed0, plan); }, plo_orbit_search, plo_orbit_plan_destroy,
        [&](const plo_orbit_best_t &pb) { return orbit_key(pb, seed0); });
}

int plo_orbit_growth_many(plo_orbit_plan_t *pl, const uint64_t *seeds, uint64_t seed0, uint64_t n, double *cost, uint32_t *nnz_nno, plo_stats_t *stats)
{
    if (!pl || !cost || !nnz_nno) return fail(PLO_E_ARG, "null argument");
    if (!pl->growth) return fail(PLO_E_ARG, "not a plan of plo_orbit_plan_create_growth");
    if (n >= (1ull << 31)) return fail(PLO_E_ARG, "at most 2^31-1 candidates per call");
    std::vector<uint32_t> w(4u * n + 1u);                 // the device buffer of the shared helper: n doubles, then 2n counts
    const int rc = cost_many_run(pl, seeds, n, 4, w.data(), stats, [&](uint32_t *d_out, const uint64_t *d_seeds, plo_stats_t *st) {
        plo::OrbitGrowthJob J{}; J.seed0 = seed0; J.seeds = d_seeds; J.ncand = n; J.cost = (double *)d_out; J.cnt2 = d_out + 2u * n; J.best = nullptr;
        return orbit_growth_launch(pl, J, st);
    });
    if (rc == PLO_OK && n) { memcpy(cost, w.data(), 8u * n); memcpy(nnz_nno, w.data() + 2u * n, 8u * n); }
    return rc;
}

int plo_orbit_growth_search(plo_orbit_plan_t *pl, uint64_t seed0, uint64_t nseeds, plo_orbit_gbest_t *best, plo_stats_t *stats)
{
    std::array<uint64_t, 3> b;                            // (bits of the cost, nnz << 21 | nno, candidate): the lexicographic minimum
    const int rc = orbit_search_run(pl, best, true, nseeds, stats, b, [&](plo_stats_t *st) {
        plo::OrbitGrowthJob J{}; J.seed0 = seed0; J.seeds = nullptr; J.ncand = nseeds; J.cost = nullptr; J.cnt2 = nullptr; J.best = pl->d_best;
        return orbit_growth_launch(pl, J, st);
    });
    if (rc != PLO_OK) return rc;
    memcpy(&best->cost, &b[0], 8); best->nnz = (uint32_t)(b[1] >> 21) & 0x1FFFFFu; best->nno = (uint32_t)b[1] & 0x1FFFFFu;
    best->seed = seed0 + b[2];
    return PLO_OK;
}

int plo_orbit_growth_search_multi(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, int action,
                                  uint64_t seed0, uint64_t nseeds, int ndev, const int *devices, plo_orbit_gbest_t *best, plo_stats_t *stats)
{
    if (!L || !R || !P || !best) return fail(PLO_E_ARG, "null argument");
    // (cost bits, nnz, nno); the shards are blocks of increasing seeds and equal words keep the lower shard: the smaller seed
    return sharded_search(seed0, nseeds, ndev, devices, best, stats,
        [&](plo_orbit_plan_t **plan) { return plo_orbit_plan_create_growth(L, R, P, action, plan); }, plo_orbit_growth_search, plo_orbit_plan_destroy,
        [&](const plo_orbit_gbest_t &pb) { unsigned long long bits; memcpy(&bits, &pb.cost, 8); return std::make_pair(bits, ((unsigned long long)pb.nnz << 21) | pb.nno); });
}

} // extern "C"

// ---------------------------------------------------------------------------------------------- dependency
struct plo_dep_plan {
    plo::DepPlan P{};
    void *d_img = nullptr; unsigned long long *d_ctr = nullptr;      // d_ctr: the task counter, then the hit counter
    uint32_t waves_per_wg = 4, lds_bytes = 0, blocks_per_cu = 1, grid_max = 1, level = 0;
    uint64_t algo_bytes = 0; bool m_in_lds = false;
};

namespace {
#define PLO_DEP_MAX_HITS (1ull << 24)
// the reference's order: by top row, then (q1, v1), (q2, v2), ..., a prefix before its extensions
bool dep_before(const plo_dep_hit_t &a, const plo_dep_hit_t &b) {
    if (a.rows[0] != b.rows[0]) return a.rows[0] < b.rows[0];
    for (uint32_t k = 1; k < a.size && k < b.size; ++k) {
        if (a.rows[k] != b.rows[k]) return a.rows[k] < b.rows[k];
        if (a.coef[k] != b.coef[k]) return a.coef[k] < b.coef[k];
    }
    return a.size < b.size;
}
} // namespace

extern "C" {
int plo_dep_plan_create_q(const plo_qcsr_t *M, const int64_t *cnum, const int64_t *cden, uint32_t ncoef, uint64_t modulus, uint32_t level, plo_dep_plan_t **plan)
{
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    if (!M || !plan || (ncoef && (!cnum || !cden))) return fail(PLO_E_ARG, "null argument");
    if (modulus == 1) return fail(PLO_E_ARG, "modulus 1");
    if (level == 0 || ncoef == 0) return fail(PLO_E_ARG, "level and the number of coefficients must be positive");
    if (const char *d = qcsr_defect(M)) return fail(PLO_E_ARG, d);
    for (uint32_t v = 0; v < ncoef; ++v) if (cden[v] <= 0) return fail(PLO_E_ARG, "non-positive denominator of a coefficient");
    if (level > PLO_DEP_MAX_LEVEL) return fail(PLO_E_UNSUPPORTED, "level above " + std::to_string(PLO_DEP_MAX_LEVEL) + ": host path only");
    if (modulus >= (1ull << 31)) return fail(PLO_E_UNSUPPORTED, "modulus of 2^31 or more: host path only");
    if (M->m > 4096) return fail(PLO_E_CAPACITY, "more than 4096 rows");
    if (M->n > 1024) return fail(PLO_E_CAPACITY, "more than 1024 columns");
    if (ncoef > 255) return fail(PLO_E_CAPACITY, "more than 255 coefficients");
    const uint32_t p = modulus ? (uint32_t)modulus : PLO_DEP_PRIME, m = M->m, n = M->n, ld = n | 1u;
    std::vector<uint32_t> dense((size_t)m * ld, 0u), coef(ncoef);
    for (uint32_t i = 0; i < m; ++i)
        for (uint32_t e = M->rowptr[i]; e < M->rowptr[i + 1]; ++e)
            if (!residue_of(M->num[e], M->den ? M->den[e] : 1, p, dense[(size_t)i * ld + M->col[e]])) return fail(PLO_E_UNSUPPORTED, "a denominator of the matrix is no unit modulo " + std::to_string(p));
    for (uint32_t v = 0; v < ncoef; ++v)
        if (!residue_of(cnum[v], cden[v], p, coef[v])) return fail(PLO_E_UNSUPPORTED, "a denominator of a coefficient is no unit modulo " + std::to_string(p));
    plo_dep_plan *pl = new plo_dep_plan();
    plo::DepPlan &Q = pl->P;
    pl->level = level;
    Q.m = m; Q.n = n; Q.ld = ld; Q.C = ncoef; Q.p = p; Q.mu = (~0ull) / p;
    Q.L = std::max(2u, std::min(level, m));                   // no combination has more rows than the matrix
    Q.nvec = Q.L < 3u ? 1u : Q.L - 2u;
    Q.lds_per_wave = round_up(4u * (Q.nvec * n + 2u * PLO_DEP_MAX_LEVEL), 16);
    // M in LDS when it and four waves fit in 64 KiB; otherwise it is read through L2
    const uint32_t m_bytes = round_up(4u * m * ld, 16), c_bytes = round_up(4u * ncoef, 16);
    const uint32_t cap = (uint32_t)std::min<size_t>(g_lds_max, 64u * 1024u);
    pl->m_in_lds = (uint64_t)m_bytes + c_bytes + 4u * Q.lds_per_wave <= cap;
    Q.off_coef = pl->m_in_lds ? m_bytes : 0u; Q.off_wave = Q.off_coef + c_bytes;
    pl->waves_per_wg = pick_waves([&](uint32_t w) { return (uint64_t)Q.off_wave + (uint64_t)w * Q.lds_per_wave; }, false, cap, &pl->lds_bytes);
    if (!pl->waves_per_wg) { delete pl; return fail(PLO_E_CAPACITY, "the vectors of this level do not fit LDS"); }
    pl->blocks_per_cu = blocks_per_cu(pl->waves_per_wg, pl->lds_bytes);
    pl->grid_max = (uint32_t)g_cus * pl->blocks_per_cu;
    pl->algo_bytes = 4ull * m * ld + 4ull * ncoef;
    const size_t bytes = (size_t)m_bytes + c_bytes;
    std::vector<uint8_t> img(bytes, 0);
    if (m) memcpy(img.data(), dense.data(), 4ull * m * ld);
    memcpy(img.data() + m_bytes, coef.data(), 4ull * ncoef);
    const void *fn = pl->m_in_lds ? (const void *)plo::dep_kernel<true> : (const void *)plo::dep_kernel<false>;
    if (hipMalloc(&pl->d_img, bytes) != hipSuccess || hipMemcpy(pl->d_img, img.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void **)&pl->d_ctr, 16) != hipSuccess ||
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl->lds_bytes) != hipSuccess) {
        plo_dep_plan_destroy(pl); return fail(PLO_E_HIP, "device setup of the dependency plan failed");
    }
    Q.M = (const uint32_t *)pl->d_img; Q.coef = (const uint32_t *)((const uint8_t *)pl->d_img + m_bytes);
    *plan = pl;
    return PLO_OK;
}

void plo_dep_plan_destroy(plo_dep_plan_t *pl)
{
    if (pl) { dev_free(pl->d_img, pl->d_ctr); delete pl; }
}

int plo_dep_search(plo_dep_plan_t *pl, uint32_t row0, uint32_t row1, plo_dep_hit_t *hits, uint64_t cap, uint64_t *nhits, plo_stats_t *stats)
{
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    if (!pl || !nhits || (cap && !hits)) return fail(PLO_E_ARG, "null argument");
    if (row0 > row1 || row1 > pl->P.m) return fail(PLO_E_ARG, "top rows out of range");
    CallScope call(stats); plo_stats_t *st = call.st;
    *nhits = 0;
    const uint32_t m = pl->P.m, C = pl->P.C, nrows = row1 - row0;
    std::vector<uint64_t> toff(nrows + 1u, 0);
    for (uint32_t r = 0; r < nrows; ++r) toff[r + 1u] = toff[r] + (uint64_t)(m - 1u - (row0 + r)) * C;
    const uint64_t ntasks = toff[nrows];
    if (pl->level < 2u || ntasks == 0) return PLO_OK;           // (`seconds` stays 0)
    const uint64_t dcap = std::min<uint64_t>(cap, PLO_DEP_MAX_HITS);
    DevBuf<uint64_t> d_toff; DevBuf<plo_dep_hit_t> d_hits;
    if (hipMalloc((void **)&d_toff.p, 8ull * (nrows + 1u)) != hipSuccess || hipMemcpy(d_toff, toff.data(), 8ull * (nrows + 1u), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void **)&d_hits.p, std::max<uint64_t>(1, dcap) * sizeof(plo_dep_hit_t)) != hipSuccess ||
        hipMemsetAsync(pl->d_ctr, 0, 16, g_stream) != hipSuccess) return fail(PLO_E_HIP, "device buffers of the dependency search");
    plo::DepJob J{}; J.row0 = row0; J.nrows = nrows; J.toff = d_toff; J.ntasks = ntasks; J.next = pl->d_ctr; J.count = pl->d_ctr + 1; J.hits = d_hits; J.cap = dcap;
    const uint64_t grid = grid_for(ntasks, pl->waves_per_wg, pl->grid_max);
    int rc = timed_launch(pl, grid, ntasks, st, [&] {
        if (pl->m_in_lds) hipLaunchKernelGGL((plo::dep_kernel<true>), dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J);
        else hipLaunchKernelGGL((plo::dep_kernel<false>), dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J);
    });
    unsigned long long found = 0;
    if (rc == PLO_OK && hipMemcpy(&found, pl->d_ctr + 1, 8, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PLO_E_HIP, "copy back of the hit count");
    if (rc == PLO_OK) {
        *nhits = found;
        const uint64_t have = std::min<uint64_t>(found, dcap);
        if (have && hipMemcpy(hits, d_hits, have * sizeof(plo_dep_hit_t), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PLO_E_HIP, "copy back of the hits");
        else if (found > PLO_DEP_MAX_HITS) rc = fail(PLO_E_CAPACITY, std::to_string(found) + " hits, more than 2^24 in one call: take fewer top rows");
        else if (found > cap) rc = fail(PLO_E_CAPACITY, std::to_string(found) + " hits for a buffer of " + std::to_string(cap));
        else std::sort(hits, hits + found, dep_before);
    }
    return call.done(rc);
}
} // extern "C"

// ---------------------------------------------------------------------------------------------- Brent equations
struct plo_brent_plan {
    plo::BrentPlan P{};
    void *d_img = nullptr; unsigned long long *d_res = nullptr;      // d_res: the count of violated equations, then the packed minimum
    uint32_t waves_per_wg = 4, lds_bytes = 0, pairs_per_launch = 0, mk = 0;
    uint64_t algo_bytes = 0;
};

namespace {
#define PLO_BRENT_MAX_DIM 16384u
#define PLO_BRENT_MAX_RANK (1u << 20)
#define PLO_BRENT_MAX_CHUNK 4096u
// wave steps (one t of an intersection, or 64 entries of a row of P^T) that one launch may take by the bound below: on the order of 0.1 s
#define PLO_BRENT_LAUNCH_STEPS (1ull << 28)

// A matrix by the other index: the (row, residue) lists of its columns, rows increasing; entries that vanish modulo q are dropped.
// False when a denominator is no unit.
struct BrentCols { std::vector<uint32_t> ptr, idx, val; };
bool brent_cols(const plo_qcsr_t *A, uint32_t q, BrentCols &C) {
    C.ptr.assign((size_t)A->n + 1u, 0u);
    std::vector<uint32_t> res(A->rowptr[A->m]);
    for (uint32_t e = 0; e < A->rowptr[A->m]; ++e) {
        if (!residue_of(A->num[e], A->den ? A->den[e] : 1, q, res[e])) return false;
        if (res[e]) ++C.ptr[A->col[e] + 1u];
    }
    for (uint32_t j = 0; j < A->n; ++j) C.ptr[j + 1u] += C.ptr[j];
    C.idx.resize(C.ptr[A->n]); C.val.resize(C.ptr[A->n]);
    std::vector<uint32_t> at(C.ptr.begin(), C.ptr.end() - 1);
    for (uint32_t i = 0; i < A->m; ++i)
        for (uint32_t e = A->rowptr[i]; e < A->rowptr[i + 1]; ++e)
            if (res[e]) { const uint32_t s = at[A->col[e]]++; C.idx[s] = i; C.val[s] = res[e]; }
    return true;
}
} // namespace

extern "C" {
int plo_brent_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, uint32_t m, uint32_t k, uint32_t n, uint32_t q, plo_brent_plan_t **plan)
{
    if (!L || !R || !P || !plan) return fail(PLO_E_ARG, "null argument");
    if (m == 0 || k == 0 || n == 0) return fail(PLO_E_ARG, "m, k and n must be positive");
    if ((uint64_t)m * k != L->n || (uint64_t)k * n != R->n || (uint64_t)m * n != P->m || L->m != R->m || L->m != P->n)
        return fail(PLO_E_ARG, "shapes " + std::to_string(L->m) + "x" + std::to_string(L->n) + ", " + std::to_string(R->m) + "x" + std::to_string(R->n) + ", " +
                               std::to_string(P->m) + "x" + std::to_string(P->n) + " are not r x mk, r x kn, mn x r for " + std::to_string(m) + "x" + std::to_string(k) + "x" + std::to_string(n));
    if (q < 2u || q >= (1u << 31)) return fail(PLO_E_ARG, "modulus " + std::to_string(q) + " outside 2 .. 2^31 - 1");
    for (const plo_qcsr_t *A : {L, R, P}) if (const char *d = qcsr_defect(A)) return fail(PLO_E_ARG, d);
    const uint32_t r = L->m, mk = L->n, kn = R->n, mn = P->m;
    if (mk > PLO_BRENT_MAX_DIM || kn > PLO_BRENT_MAX_DIM || mn > PLO_BRENT_MAX_DIM) return fail(PLO_E_CAPACITY, "mk, kn or mn above 16384");
    if (r > PLO_BRENT_MAX_RANK) return fail(PLO_E_CAPACITY, "rank above 2^20");
    for (const plo_qcsr_t *A : {L, R, P}) if (A->rowptr[A->m] >= (1u << 31)) return fail(PLO_E_CAPACITY, "a matrix of 2^31 entries or more");
    BrentCols cl, cr, cp;
    for (const auto &pr : {std::make_pair(L, &cl), std::make_pair(R, &cr), std::make_pair(P, &cp)})
        if (!brent_cols(pr.first, q, *pr.second)) return fail(PLO_E_ARG, "a denominator is no unit modulo " + std::to_string(q));
    if (const int rc = require_device(NOINIT_PLAN)) return rc;

    plo_brent_plan *pl = new plo_brent_plan();
    plo::BrentPlan &Q = pl->P;
    Q.k = k; Q.n = n; Q.kn = kn; Q.mn = mn; Q.q = q; Q.mu = (~0ull) / q;
    pl->mk = mk;
    const uint32_t chunk_max = std::min(mn, PLO_BRENT_MAX_CHUNK);
    Q.chunk = chunk_max;
    if (const auto c = env_knob("PLO_BRENT_CHUNK")) Q.chunk = (uint32_t)std::min<long>(std::max<long>(*c, 1), chunk_max);   // test knob: several chunks on a small mn
    Q.nchunks = (mn + Q.chunk - 1u) / Q.chunk;
    pl->lds_bytes = round_up(4u * Q.chunk * pl->waves_per_wg, 16);
    // Pairs per launch: a pair takes, per chunk, at most min(wL[x], wR[y]) steps for its t, wX the steps 1 + ceil(|row t of P^T| / 64)
    // summed over a column, besides the bisections of its column of L and the clearing and comparing of the chunk
    std::vector<uint32_t> wp(r);
    for (uint32_t t = 0; t < r; ++t) wp[t] = 1u + (cp.ptr[t + 1u] - cp.ptr[t] + 63u) / 64u;
    auto heaviest = [&](const BrentCols &C, uint32_t cols, uint64_t *longest) {
        uint64_t best = 0; *longest = 0;
        for (uint32_t j = 0; j < cols; ++j) {
            uint64_t w = 0;
            for (uint32_t e = C.ptr[j]; e < C.ptr[j + 1u]; ++e) w += wp[C.idx[e]];
            best = std::max(best, w); *longest = std::max<uint64_t>(*longest, C.ptr[j + 1u] - C.ptr[j]);
        }
        return best;
    };
    uint64_t longl = 0, longr = 0;
    const uint64_t wl = heaviest(cl, mk, &longl), wr = heaviest(cr, kn, &longr);
    const uint64_t per_pair = (uint64_t)Q.nchunks * (std::min(wl, wr) + (longl + 63u) / 64u * 24u + 2u * ((Q.chunk + 63u) / 64u) + 1u);
    uint64_t ppl = std::max<uint64_t>(1, PLO_BRENT_LAUNCH_STEPS / per_pair);
    ppl = std::min<uint64_t>(ppl, 0xFFFFFFFFull / mn);                                  // (pair - pair0) mn + z stays below 2^32 in the packed minimum
    if (const auto c = env_knob("PLO_BRENT_PAIRS")) ppl = (uint64_t)std::min<long>(std::max<long>(*c, 1), (long)ppl);   // test knob: several launches on a small input
    pl->pairs_per_launch = (uint32_t)std::min<uint64_t>(ppl, (uint64_t)mk * kn);
    pl->algo_bytes = 8ull * (cl.idx.size() + cr.idx.size() + cp.idx.size());

    // the image: nine arrays of 32-bit words
    const std::vector<uint32_t> *arr[9] = {&cl.ptr, &cl.idx, &cl.val, &cr.ptr, &cr.idx, &cr.val, &cp.ptr, &cp.idx, &cp.val};
    size_t off[9], words = 0;
    for (int j = 0; j < 9; ++j) { off[j] = words; words += (arr[j]->size() + 3u) / 4u * 4u; }
    std::vector<uint32_t> img(std::max<size_t>(words, 4), 0u);
    for (int j = 0; j < 9; ++j) if (!arr[j]->empty()) memcpy(img.data() + off[j], arr[j]->data(), 4u * arr[j]->size());
    if (hipMalloc(&pl->d_img, 4u * img.size()) != hipSuccess || hipMemcpy(pl->d_img, img.data(), 4u * img.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void **)&pl->d_res, 16) != hipSuccess ||
        hipFuncSetAttribute((const void *)plo::brent_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4u * PLO_BRENT_MAX_CHUNK * pl->waves_per_wg)) != hipSuccess) {   // the largest any plan asks for: plans do not lower it under each other
        plo_brent_plan_destroy(pl); return fail(PLO_E_HIP, "device setup of the Brent plan failed");
    }
    const uint32_t *d = (const uint32_t *)pl->d_img;
    Q.lcp = d + off[0]; Q.lt = d + off[1]; Q.lv = d + off[2];
    Q.rcp = d + off[3]; Q.rt = d + off[4]; Q.rv = d + off[5];
    Q.prp = d + off[6]; Q.pz = d + off[7]; Q.pv = d + off[8];
    *plan = pl;
    return PLO_OK;
}

void plo_brent_plan_destroy(plo_brent_plan_t *pl)
{
    if (pl) { dev_free(pl->d_img, pl->d_res); delete pl; }
}

int plo_brent_plan_info(plo_brent_plan_t *pl, uint32_t out[8])
{
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    out[0] = pl->P.chunk; out[1] = pl->P.nchunks; out[2] = pl->waves_per_wg; out[3] = pl->pairs_per_launch;
    out[4] = pl->lds_bytes; out[5] = pl->mk; out[6] = pl->P.kn; out[7] = pl->P.mn;
    return PLO_OK;
}

int plo_brent_check(plo_brent_plan_t *pl, uint64_t pair0, uint64_t pair1, plo_brent_result_t *res, plo_stats_t *stats)
{
    if (!pl || !res) return fail(PLO_E_ARG, "null argument");
    const uint64_t npairs = (uint64_t)pl->mk * pl->P.kn;
    if (pair0 >= pair1 || pair1 > npairs) return fail(PLO_E_ARG, "pairs " + std::to_string(pair0) + " .. " + std::to_string(pair1) + ": an empty range or one beyond the " + std::to_string(npairs) + " pairs");
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    CallScope call(stats); plo_stats_t *st = call.st;
    const plo::BrentPlan &Q = pl->P;
    *res = plo_brent_result_t{0, ~0ull, 0, 0};
    int rc = PLO_OK;
    for (uint64_t p0 = pair0; rc == PLO_OK && p0 < pair1;) {
        const uint64_t cnt = std::min<uint64_t>(pl->pairs_per_launch, pair1 - p0);
        if (hipMemsetAsync(pl->d_res, 0, 8, g_stream) != hipSuccess || hipMemsetAsync(pl->d_res + 1, 0xFF, 8, g_stream) != hipSuccess) { rc = fail(PLO_E_HIP, "clearing the Brent result words"); break; }
        plo::BrentJob J{}; J.pair0 = p0; J.npairs = cnt; J.count = pl->d_res; J.first = pl->d_res + 1;
        const uint64_t grid = (cnt + pl->waves_per_wg - 1u) / pl->waves_per_wg;
        rc = timed_launch(pl, grid, cnt * Q.mn, st, [&] {
            hipLaunchKernelGGL(plo::brent_kernel, dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J);
        });
        unsigned long long w[2] = {0, 0};
        if (rc == PLO_OK && hipMemcpy(w, pl->d_res, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PLO_E_HIP, "copy back of the Brent result words");
        if (rc != PLO_OK) break;
        if (w[0]) {
            if (res->violated == 0) { res->first = p0 * Q.mn + (w[1] >> 32); res->value = (uint32_t)w[1]; }   // launches go by increasing pair
            res->violated += w[0];
        }
        p0 += cnt;
    }
    if (rc == PLO_OK && res->violated) {
        const uint64_t z = res->first % Q.mn, pair = res->first / Q.mn, x = pair / Q.kn, y = pair % Q.kn;
        res->expected = (x % Q.k == y / Q.n && z == (x / Q.k) * Q.n + y % Q.n) ? 1u : 0u;
    }
    return call.done(rc);
}
} // extern "C"

// ---------------------------------------------------------------------------------------------- polynomial-multiplication equations
struct plo_polymul_plan {
    plo::PolyMulPlan P{};
    void *d_img = nullptr; unsigned long long *d_res = nullptr;      // d_res: the count of violated equations, then the packed minimum
    uint32_t waves_per_wg = 4, lds_bytes = 0, pairs_per_launch = 0, na = 0, fold = 0;
    uint64_t algo_bytes = 0;
    std::vector<uint32_t> rho;                                       // the host's copy of the table (the expected value of the first violated equation)
};

namespace {
#define PLO_POLYMUL_MAX_Z 32768u
#define PLO_POLYMUL_MAX_CHUNK 4096u
// the dynamic LDS any plan may ask for: 4 waves of 4096 sums, or of 2048 sums and PLO_POLYMUL_MAX_FOLD_DEGREE = 2048 folded ones
#define PLO_POLYMUL_MAX_LDS (4u * 4u * PLO_POLYMUL_MAX_CHUNK)

// X^z mod f for z < Z over Z/qZ, f monic of degree d given by its d low coefficients: Z rows of d residues
std::vector<uint32_t> polymul_rho(const std::vector<uint32_t> &low, uint32_t Z, uint32_t q) {
    const uint32_t d = (uint32_t)low.size();
    std::vector<uint32_t> rho((size_t)Z * d, 0u);
    for (uint32_t z = 0; z < Z && z < d; ++z) rho[(size_t)z * d + z] = 1u;
    for (uint32_t z = d; z < Z; ++z) {                              // X rho[z - 1]: a shift, and the top coefficient times X^d = -low
        const uint32_t *prev = rho.data() + (size_t)(z - 1u) * d; uint32_t *row = rho.data() + (size_t)z * d;
        const uint64_t top = prev[d - 1u];
        for (uint32_t c = 0; c < d; ++c) {
            const uint64_t sub = top * low[c] % q, sh = c ? prev[c - 1u] : 0u;
            row[c] = (uint32_t)((sh + q - sub) % q);
        }
    }
    return rho;
}
} // namespace

extern "C" {
int plo_polymul_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, const int64_t *fnum, const int64_t *fden, uint32_t flen, uint32_t q, plo_polymul_plan_t **plan)
{
    if (!L || !R || !P || !plan || (flen && !fnum)) return fail(PLO_E_ARG, "null argument");
    if (L->m != R->m || L->m != P->n)
        return fail(PLO_E_ARG, "inner dimensions " + std::to_string(L->m) + ", " + std::to_string(R->m) + ", " + std::to_string(P->n) + " of L, R and P differ");
    if (q < 2u || q >= (1u << 31)) return fail(PLO_E_ARG, "modulus " + std::to_string(q) + " outside 2 .. 2^31 - 1");
    for (const plo_qcsr_t *A : {L, R, P}) if (const char *d = qcsr_defect(A)) return fail(PLO_E_ARG, d);
    if (flen == 1u) return fail(PLO_E_ARG, "a constant polynomial: the degree must be 1 at least");
    if (flen && fnum[flen - 1u] == 0) return fail(PLO_E_ARG, "the leading coefficient of the polynomial is 0");
    for (uint32_t c = 0; c < flen; ++c) if (fden && fden[c] <= 0) return fail(PLO_E_ARG, "a non-positive denominator in the polynomial");
    const uint32_t r = L->m, na = L->n, nb = R->n, nc = P->m, d = flen ? flen - 1u : 0u;
    const uint64_t Z64 = std::max<uint64_t>(nc, (uint64_t)na + nb - (na || nb ? 1u : 0u));
    if (na > PLO_BRENT_MAX_DIM || nb > PLO_BRENT_MAX_DIM) return fail(PLO_E_CAPACITY, "more than 16384 columns in L or R");
    if (Z64 > PLO_POLYMUL_MAX_Z) return fail(PLO_E_CAPACITY, "max(nc, na + nb - 1) above 32768");
    if (r > PLO_BRENT_MAX_RANK) return fail(PLO_E_CAPACITY, "rank above 2^20");
    for (const plo_qcsr_t *A : {L, R, P}) if (A->rowptr[A->m] >= (1u << 31)) return fail(PLO_E_CAPACITY, "a matrix of 2^31 entries or more");
    const uint32_t Z = (uint32_t)Z64;
    const bool fold = flen && d < Z;
    if (fold && d > PLO_POLYMUL_MAX_FOLD_DEGREE) return fail(PLO_E_CAPACITY, "a fold modulo a polynomial of degree above " + std::to_string(PLO_POLYMUL_MAX_FOLD_DEGREE));
    if (flen && d > (1u << 24)) return fail(PLO_E_CAPACITY, "a polynomial of degree above 2^24");
    BrentCols cl, cr, cp;
    for (const auto &pr : {std::make_pair(L, &cl), std::make_pair(R, &cr), std::make_pair(P, &cp)})
        if (!brent_cols(pr.first, q, *pr.second)) return fail(PLO_E_ARG, "a denominator is no unit modulo " + std::to_string(q));
    std::vector<uint32_t> low(d, 0u);                               // f made monic: its d low coefficients
    if (flen) {
        std::vector<uint32_t> fr(flen);
        for (uint32_t c = 0; c < flen; ++c)
            if (!residue_of(fnum[c], fden ? fden[c] : 1, q, fr[c])) return fail(PLO_E_ARG, "a denominator of the polynomial is no unit modulo " + std::to_string(q));
        if (gcd64(fr[d], q) != 1) return fail(PLO_E_ARG, "the leading coefficient of the polynomial is no unit modulo " + std::to_string(q));
        const uint64_t il = inv_mod(fr[d], q);
        for (uint32_t c = 0; c < d; ++c) low[c] = (uint32_t)(fr[c] * il % q);
    }
    if (const int rc = require_device(NOINIT_PLAN)) return rc;

    plo_polymul_plan *pl = new plo_polymul_plan();
    plo::PolyMulPlan &Q = pl->P;
    Q.nb = nb; Q.nc = nc; Q.w = flen ? d : Z; Q.d = fold ? d : 0u; Q.q = q; Q.mu = (~0ull) / q;
    pl->na = na; pl->fold = fold ? 1u : 0u;
    const uint32_t zend = fold ? nc : Q.w;                           // the z that the chunks walk
    const uint32_t chunk_max = std::max(1u, std::min(zend, fold ? PLO_POLYMUL_MAX_CHUNK / 2u : PLO_POLYMUL_MAX_CHUNK));
    Q.chunk = chunk_max;
    if (const auto c = env_knob("PLO_POLYMUL_CHUNK")) Q.chunk = (uint32_t)std::min<long>(std::max<long>(*c, 1), chunk_max);   // test knob: several chunks on a small nc
    Q.nchunks = (zend + Q.chunk - 1u) / Q.chunk;
    pl->lds_bytes = round_up(4u * (Q.chunk + Q.d) * pl->waves_per_wg, 16);
    // Pairs per launch, as for the Brent plan: per chunk at most min(wL[i], wR[j]) steps for a pair's t, besides the bisections
    // and the clearing and comparing of the chunk; the fold adds ceil(d / 64) steps per row of rho that is no identity row
    std::vector<uint32_t> wp(r);
    for (uint32_t t = 0; t < r; ++t) wp[t] = 1u + (cp.ptr[t + 1u] - cp.ptr[t] + 63u) / 64u;
    auto heaviest = [&](const BrentCols &C, uint32_t cols, uint64_t *longest) {
        uint64_t best = 0; *longest = 0;
        for (uint32_t j = 0; j < cols; ++j) {
            uint64_t w = 0;
            for (uint32_t e = C.ptr[j]; e < C.ptr[j + 1u]; ++e) w += wp[C.idx[e]];
            best = std::max(best, w); *longest = std::max<uint64_t>(*longest, C.ptr[j + 1u] - C.ptr[j]);
        }
        return best;
    };
    uint64_t longl = 0, longr = 0;
    const uint64_t wl = heaviest(cl, na, &longl), wr = heaviest(cr, nb, &longr);
    const uint64_t fold_steps = fold ? (uint64_t)((d + 63u) / 64u) * ((nc > d ? nc - d : 0u) + 2u * Q.nchunks + 2u) : 0u;
    const uint64_t per_pair = (uint64_t)Q.nchunks * (std::min(wl, wr) + (longl + 63u) / 64u * 24u + 2u * ((Q.chunk + 63u) / 64u) + 1u) + fold_steps + 1u;
    uint64_t ppl = std::max<uint64_t>(1, PLO_BRENT_LAUNCH_STEPS / per_pair);
    ppl = std::min<uint64_t>(ppl, 0xFFFFFFFFull / std::max(Q.w, 1u));                  // (pair - pair0) w + c stays below 2^32 in the packed minimum
    if (const auto c = env_knob("PLO_POLYMUL_PAIRS")) ppl = (uint64_t)std::min<long>(std::max<long>(*c, 1), (long)ppl);   // test knob: several launches on a small input
    pl->pairs_per_launch = (uint32_t)std::min<uint64_t>(ppl, std::max<uint64_t>(1, (uint64_t)na * nb));
    if (fold) pl->rho = polymul_rho(low, Z, q);
    pl->algo_bytes = 8ull * (cl.idx.size() + cr.idx.size() + cp.idx.size()) + 4ull * pl->rho.size();

    // the image: nine arrays of 32-bit words and the table
    const std::vector<uint32_t> *arr[10] = {&cl.ptr, &cl.idx, &cl.val, &cr.ptr, &cr.idx, &cr.val, &cp.ptr, &cp.idx, &cp.val, &pl->rho};
    size_t off[10], words = 0;
    for (int j = 0; j < 10; ++j) { off[j] = words; words += (arr[j]->size() + 3u) / 4u * 4u; }
    std::vector<uint32_t> img(std::max<size_t>(words, 4), 0u);
    for (int j = 0; j < 10; ++j) if (!arr[j]->empty()) memcpy(img.data() + off[j], arr[j]->data(), 4u * arr[j]->size());
    if (hipMalloc(&pl->d_img, 4u * img.size()) != hipSuccess || hipMemcpy(pl->d_img, img.data(), 4u * img.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void **)&pl->d_res, 16) != hipSuccess ||
        hipFuncSetAttribute((const void *)plo::polymul_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PLO_POLYMUL_MAX_LDS) != hipSuccess) {   // the largest any plan asks for: plans do not lower it under each other
        plo_polymul_plan_destroy(pl); return fail(PLO_E_HIP, "device setup of the polynomial-multiplication plan failed");
    }
    const uint32_t *dv = (const uint32_t *)pl->d_img;
    Q.lcp = dv + off[0]; Q.lt = dv + off[1]; Q.lv = dv + off[2];
    Q.rcp = dv + off[3]; Q.rt = dv + off[4]; Q.rv = dv + off[5];
    Q.prp = dv + off[6]; Q.pz = dv + off[7]; Q.pv = dv + off[8];
    Q.rho = dv + off[9];
    *plan = pl;
    return PLO_OK;
}

void plo_polymul_plan_destroy(plo_polymul_plan_t *pl)
{
    if (pl) { dev_free(pl->d_img, pl->d_res); delete pl; }
}

int plo_polymul_plan_info(plo_polymul_plan_t *pl, uint32_t out[8])
{
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    out[0] = pl->P.chunk; out[1] = pl->P.nchunks; out[2] = pl->waves_per_wg; out[3] = pl->pairs_per_launch;
    out[4] = pl->lds_bytes; out[5] = pl->na * pl->P.nb; out[6] = pl->P.w; out[7] = pl->fold;
    return PLO_OK;
}

int plo_polymul_check(plo_polymul_plan_t *pl, uint64_t pair0, uint64_t pair1, plo_brent_result_t *res, plo_stats_t *stats)
{
    if (!pl || !res) return fail(PLO_E_ARG, "null argument");
    const uint64_t npairs = (uint64_t)pl->na * pl->P.nb;
    if (pair0 >= pair1 || pair1 > npairs) return fail(PLO_E_ARG, "pairs " + std::to_string(pair0) + " .. " + std::to_string(pair1) + ": an empty range or one beyond the " + std::to_string(npairs) + " pairs");
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    CallScope call(stats); plo_stats_t *st = call.st;
    const plo::PolyMulPlan &Q = pl->P;
    *res = plo_brent_result_t{0, ~0ull, 0, 0};
    int rc = PLO_OK;
    for (uint64_t p0 = pair0; rc == PLO_OK && p0 < pair1;) {
        const uint64_t cnt = std::min<uint64_t>(pl->pairs_per_launch, pair1 - p0);
        if (hipMemsetAsync(pl->d_res, 0, 8, g_stream) != hipSuccess || hipMemsetAsync(pl->d_res + 1, 0xFF, 8, g_stream) != hipSuccess) { rc = fail(PLO_E_HIP, "clearing the result words"); break; }
        plo::PolyMulJob J{}; J.pair0 = p0; J.npairs = cnt; J.count = pl->d_res; J.first = pl->d_res + 1;
        const uint64_t grid = (cnt + pl->waves_per_wg - 1u) / pl->waves_per_wg;
        rc = timed_launch(pl, grid, cnt * Q.w, st, [&] {
            hipLaunchKernelGGL(plo::polymul_kernel, dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J);
        });
        unsigned long long w[2] = {0, 0};
        if (rc == PLO_OK && hipMemcpy(w, pl->d_res, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PLO_E_HIP, "copy back of the result words");
        if (rc != PLO_OK) break;
        if (w[0]) {
            if (res->violated == 0) { res->first = p0 * Q.w + (w[1] >> 32); res->value = (uint32_t)w[1]; }   // launches go by increasing pair
            res->violated += w[0];
        }
        p0 += cnt;
    }
    if (rc == PLO_OK && res->violated) {
        const uint64_t c = res->first % Q.w, pair = res->first / Q.w, i = pair / Q.nb, j = pair % Q.nb;
        res->expected = pl->fold ? pl->rho[(size_t)(i + j) * Q.d + c] : (c == i + j ? 1u : 0u);
    }
    return call.done(rc);
}
} // extern "C"

// ---------------------------------------------------------------------------------------------- in-place trilinear programs
#include "plo_capi_tprog.hip"
#include "plo_capi_cseq.hip"
