// ==========================================================================
// plo_orbit_cse.hip -- the `-z` measure of the De Groote orbit search (bin/orbiter -z; reference src/orbiter.cpp:172-209) on
// gfx950: a candidate (U, V, W) is scored by the operations of the best straight-line programs CSEOptimiser finds for its three
// transformed matrices Lj (r x mk), Rg (r x kn) and hP (mn x r) over Z_p (include/plinopt_hip.h, PLO_ORBIT_CSE):
//   cost = c(Lj) + c(Rg) + c(hP),  c(M) = min(naive(M), min over j < sub of adds + muls of Optimizer(M), stream cse_seed0 + j).
//
// One wave per candidate, as plo::orbit_kernel.  The factor draws (o_zoi, o_pluq, o_house) are that kernel's MOD = true ones and
// the sandwich arithmetic is the same; what differs is where an output goes.  For every part the wave builds the LDS image of
// plo_cse_wave.hip's run_candidate from the entries it has just computed, the way plo::kmethod_candidate builds Dep:
//   1. a length pass: lane groups of LPR >= columns lanes, one row of the part per group; a group's ballot is the row's length
//      (and the part's nnz, nno and naive count),
//   2. a prefix over the lanes (lane = row, at most 64) gives the packed row starts; more entries than the sampled bound of the
//      layout is ERR_TABLE, as a full pair table, and the host repeats the launch with larger bounds,
//   3. a fill pass computes the entries again and writes (column, value) at start + rank inside the ballot: rows sorted by column,
//   4. inverses by Fermat, column masks, the pair table cleared and filled by tab_inc.
// For hP the roles are swapped: the sandwich runs over the rows of P^T (the columns of P), so a row of the image is an output
// entry (a, c) and its columns are the r rows of P^T.
// run_candidate consumes the image, so for j > 0 it is put back: either from a copy of the whole template (OrbitCsePlan::keep_full,
// one plain LDS copy, tmpl_bytes more per wave) or from a copy of the entries alone, after which masks and table are made again
// (step 4 without the inverses).  DESIGN 2.9 says which one the plans use and why.
// Limits: r <= 64 and mn <= 64 (run_candidate<false> keeps one row per lane in ProgramGen), mk, kn, r <= 64 (a row of at most 64
// entries); the host refuses the rest.
// ==========================================================================
#pragma once
#include "plo_orbit.hip"

namespace plo {

struct OrbitCsePlan {
    WavePlan W[3];                   // layouts of the images of Lj, Rg and hP (no template: built by the wave)
    uint64_t seed0;                  // the Optimizer streams: seeds seed0 .. seed0 + sub - 1, the same for every candidate and part
    uint32_t sub;
    uint32_t keep_full;              // 1: the kept copy is the whole template; 0: the entries only (masks and table are made again)
    uint32_t off_rs, off_img, off_keep, wave_bytes;   // a wave's region: orbit_kernel's part, the row starts, the image, the kept copy
    uint32_t *err;                   // device error word (ERR_*)
};

#ifdef PLO_ORBIT_CSE_PROFILE
__device__ unsigned long long g_ocprof[8];   // lane 0 of every wave: cycles in factor draw, sandwich + image build, Optimizer on Lj, Rg, hP (restores included); candidates
#define OC_T(k_) do { const unsigned long long t__ = clock64(); oc_acc[k_] += t__ - oc_t; oc_t = t__; } while (0)
#else
#define OC_T(k_) do { } while (0)
#endif

// one part of the sandwich as the image sees it: `rows` x `cols`, entry (i, c) = output e of source row g, (g, e) = (i, c) or,
// for hP, (c, i)
struct OcPart { const int64_t *A, *B; uint32_t a_s, b_s, row0, rows, cols; bool swap; };

__device__ __forceinline__ uint32_t oc_lpr_log2(uint32_t cols) { return cols <= 4u ? 2u : 32u - (uint32_t)__clz(cols - 1u); }

// the sandwich sum of plo::orbit_kernel<true, *> for one output entry
__device__ __forceinline__ uint32_t oc_entry(const OcPart &T, const uint32_t *rp, const uint16_t *pos, const int64_t *val, uint32_t i, uint32_t c, uint64_t p)
{
    const uint32_t g = T.row0 + (T.swap ? c : i), e = T.swap ? i : c, pp = e / T.b_s, qq = e - pp * T.b_s;
    int64_t acc = 0;
    for (uint32_t x = rp[g]; x < rp[g + 1u]; ++x) {
        const uint32_t ps = pos[x], a = ps >> 8, b = ps & 0xFFu;
        const int64_t fa = T.A[a * T.a_s + pp], fb = T.B[b * T.b_s + qq];
        if (fa == 0 || fb == 0) continue;
        const uint64_t ax = (uint64_t)fa * (uint64_t)val[x] % p;
        acc += (int64_t)(ax * (uint64_t)fb % p);
        if ((uint64_t)acc >= p) acc -= (int64_t)p;
    }
    return (uint32_t)acc;
}

// Step 1: len[i] for the rows of the part; this lane's share of the non-zero entries and of those that are not +-1
__device__ __forceinline__ void oc_lengths(const OcPart &T, const uint32_t *rp, const uint16_t *pos, const int64_t *val, uint64_t p, uint32_t lane,
                                           uint16_t *len, uint32_t &nnz, uint32_t &nno)
{
    const uint32_t lpr = oc_lpr_log2(T.cols), LPR = 1u << lpr, G = 64u >> lpr, g = lane >> lpr, s = lane & (LPR - 1u);
    const uint64_t gm = LPR == 64u ? ~0ull : (((1ull << LPR) - 1ull) << (g << lpr));
    for (uint32_t i0 = 0; i0 < T.rows; i0 += G) {
        const uint32_t i = i0 + g;
        const uint32_t v = (i < T.rows && s < T.cols) ? oc_entry(T, rp, pos, val, i, s, p) : 0u;
        const uint64_t mk = __ballot(v != 0u) & gm;
        if (v != 0u) { ++nnz; nno += absone(v, (uint32_t)p) ? 0u : 1u; }
        if (i < T.rows && s == 0u) len[i] = (uint16_t)__popcll(mk);
    }
    PLO_WAVE_SYNC();
}

// Step 4 without the inverses: the column masks and the pair table of the rows now in the image (listpairs :30-41)
__device__ __forceinline__ bool oc_index(const WavePlan &W, uint8_t *img, const uint16_t *rs, uint32_t maxl, uint32_t lane)
{
    uint64_t *tab = (uint64_t *)(img + W.off_tab), *cmask = (uint64_t *)(img + W.off_cmask), *umask = (uint64_t *)(img + W.off_umask);
    const uint32_t *val = (const uint32_t *)(img + W.off_val), *inv = (const uint32_t *)(img + W.off_inv);
    const uint16_t *col = (const uint16_t *)(img + W.off_col), *len = (const uint16_t *)(img + W.off_len);
    const uint32_t p = W.p, abs_ = W.rb + W.bb, rb = W.rb; const uint64_t mu = W.mu;
    for (uint32_t s = lane; s < W.cap; s += 64u) tab[s] = PLO_EMPTY;
    for (uint32_t c = lane; c < W.n; c += 64u) { cmask[c * 2u] = 0ull; umask[c * 2u] = 0ull; }      // (at most 64 rows: one mask word)
    PLO_WAVE_SYNC();
    const uint32_t LPR = 1u << W.lpr_log2, G = 64u >> W.lpr_log2, g = lane >> W.lpr_log2, t = lane & (LPR - 1u);
    bool bad = false;
    for (uint32_t r0 = 0; r0 < W.m; r0 += G) {
        const uint32_t row = r0 + g; const bool act = row < W.m;
        const uint32_t base = act ? (uint32_t)rs[row] : 0u, ln = act ? (uint32_t)len[row] : 0u;
        const bool have = t < ln;
        const uint32_t cy = have ? col[base + t] : 0u, vy = have ? val[base + t] : 0u;
        if (have) {
            atomicOr((unsigned long long *)&cmask[cy * 2u], 1ull << row);
            if (absone(vy, p)) atomicOr((unsigned long long *)&umask[cy * 2u], 1ull << row);
        }
        for (uint32_t x = 0; x + 1u < maxl; ++x) {
            if (have && x < t) {
                const uint32_t r = fmul<false>(vy, inv[base + x], p, mu);
                bad |= !tab_inc(tab, ((uint64_t)col[base + x] << abs_) | ((uint64_t)cy << rb) | r, W.cap, W.hbits);
            }
        }
    }
    PLO_WAVE_SYNC();
    return __ballot(bad) == 0ull;
}

// c(M) of one part (see the head of the file); adds the part's nnz and nno.  ~0u after an error (the error word is set).
__device__ uint32_t oc_part_cost(const OrbitCsePlan &C, uint32_t part, const OcPart &T, const uint32_t *rp, const uint16_t *pos, const int64_t *sval, uint64_t p64,
                                 uint8_t *img, uint8_t *keep, uint16_t *rs, uint32_t lane, uint32_t &nnz, uint32_t &nno
#ifdef PLO_ORBIT_CSE_PROFILE
                                 , unsigned long long &oc_t, unsigned long long *oc_acc
#endif
                                 )
{
    const WavePlan &W = C.W[part];
    const uint32_t p = W.p; const uint64_t mu = W.mu;
    uint32_t *val = (uint32_t *)(img + W.off_val), *inv = (uint32_t *)(img + W.off_inv);
    uint16_t *col = (uint16_t *)(img + W.off_col), *len = (uint16_t *)(img + W.off_len);
    uint32_t pn = 0, po = 0;
    oc_lengths(T, rp, pos, sval, p64, lane, len, pn, po);
    pn = wave_sum(pn); po = wave_sum(po);
    nnz += pn; nno += po;
    // step 2: row starts, the longest row, naive = sum of max(len - 1, 0) + the entries that are not +-1
    const uint32_t l = lane < T.rows ? (uint32_t)len[lane] : 0u;
    uint32_t inc = l;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if ((int)lane >= o) inc += u; }
    if (lane < T.rows) rs[lane + 1u] = (uint16_t)inc;
    if (lane == 0u) rs[0] = 0;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    const uint32_t maxl = uni32(wave_max(l)), naive = uni32(wave_sum(l ? l - 1u : 0u)) + po;
    if (total > W.nnz) { if (lane == 0) atomicMax(C.err, (uint32_t)ERR_TABLE); return ~0u; }
    PLO_WAVE_SYNC();
    if (naive == 0u) { OC_T(1); return 0u; }                                   // rows of at most one entry, all +-1: nothing to compute
    // step 3
    {
        const uint32_t lpr = oc_lpr_log2(T.cols), LPR = 1u << lpr, G = 64u >> lpr, g = lane >> lpr, s = lane & (LPR - 1u);
        const uint64_t gm = LPR == 64u ? ~0ull : (((1ull << LPR) - 1ull) << (g << lpr));
        for (uint32_t i0 = 0; i0 < T.rows; i0 += G) {
            const uint32_t i = i0 + g;
            const uint32_t v = (i < T.rows && s < T.cols) ? oc_entry(T, rp, pos, sval, i, s, p64) : 0u;
            const uint64_t mk = __ballot(v != 0u) & gm;
            if (v != 0u) {
                const uint32_t at = (uint32_t)rs[i] + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
                col[at] = (uint16_t)s; val[at] = v;
            }
        }
    }
    PLO_WAVE_SYNC();
    for (uint32_t idx = lane; idx < total; idx += 64u) inv[idx] = kinv(val[idx], p, mu);
    PLO_WAVE_SYNC();
    if (!oc_index(W, img, rs, maxl, lane)) { if (lane == 0) atomicMax(C.err, (uint32_t)ERR_TABLE); return ~0u; }
    // the kept copy: words [k0, k1) of the image
    const uint32_t k0 = C.keep_full ? 0u : W.off_val >> 3, k1 = C.keep_full ? W.tmpl_bytes >> 3 : W.off_cmask >> 3;
    if (C.sub > 1u) {
        for (uint32_t i = k0 + lane; i < k1; i += 64u) ((uint64_t *)keep)[i - k0] = ((const uint64_t *)img)[i];
        PLO_WAVE_SYNC();
    }
    OC_T(1);
    uint32_t best = naive;
    for (uint32_t j = 0; j < C.sub; ++j) {
        if (j) {
            for (uint32_t i = k0 + lane; i < k1; i += 64u) ((uint64_t *)img)[i] = ((const uint64_t *)keep)[i - k0];
            PLO_WAVE_SYNC();
            if (!C.keep_full && !oc_index(W, img, rs, maxl, lane)) { if (lane == 0) atomicMax(C.err, (uint32_t)ERR_TABLE); return ~0u; }
        }
        PickState ps{1u + (uint32_t)(splitmix64(C.seed0 + j) % 2147483646ull), 0u, 0ull, 1ull, 0u};
        const uint64_t res = run_candidate<false>(W, img, rs, ps, lane, C.err);
        PLO_WAVE_SYNC();
        const uint32_t ops = (uint32_t)(res >> 32) + (uint32_t)res;
        best = ops < best ? ops : best;
    }
    OC_T(2u + part);
    return uni32(best);
}

// SIZE: the sizing launch -- draws, length pass and, per part, the maxima of the entries (sz[part]), of the pair instances
// (sz[3 + part]) and of the row length (sz[6 + part]) over the candidates; nothing else is touched
template <int ACT, bool SIZE> __global__ __launch_bounds__(256) void orbit_cse_kernel(OrbitPlan P, OrbitJob J, OrbitCsePlan C, uint32_t *sz)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int64_t *val = (int64_t *)ldyn;
    uint32_t *rp = (uint32_t *)(ldyn + P.off_rp);
    uint16_t *pos = (uint16_t *)(ldyn + P.off_pos);
    const uint32_t nrows = 3u * P.r;
    for (uint32_t e = threadIdx.x; e < P.nnz; e += blockDim.x) { val[e] = P.val[e]; pos[e] = P.pos[e]; }
    for (uint32_t e = threadIdx.x; e <= nrows; e += blockDim.x) rp[e] = P.rp[e];
    if constexpr (ACT == 2) { if (threadIdx.x < 17u) ((uint32_t *)(ldyn + P.off_dinv))[threadIdx.x] = P.dinv[threadIdx.x]; }
    __syncthreads();

    uint8_t *reg = ldyn + P.shared_bytes + (size_t)wave * C.wave_bytes;
    auto fac = [&](uint32_t f) { return (int64_t *)(reg + P.off_fac[f]); };
    int64_t *Ti = (int64_t *)(reg + P.off_ti);
    int8_t *T = (int8_t *)(reg + P.off_t);
    uint8_t *perm = reg + P.off_perm;
    uint16_t *rs = (uint16_t *)(reg + C.off_rs);
    uint8_t *img = reg + C.off_img, *keep = reg + C.off_keep;
    const uint32_t m = P.m, k = P.k, n = P.n, r = P.r;
    const uint64_t p = P.p;

    uint64_t bkey = ~0ull, bidx = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * nw;
    for (uint64_t cnd = (uint64_t)blockIdx.x * nw + wave; cnd < J.ncand; cnd += stride) {
#ifdef PLO_ORBIT_CSE_PROFILE
        unsigned long long oc_t = clock64(), oc_acc[5] = {0, 0, 0, 0, 0};
#endif
        const uint64_t seed = J.seeds ? J.seeds[cnd] : J.seed0 + cnd;
        const bool base = seed == ~0ull;
        uint32_t rng = 1u + (uint32_t)(t_splitmix(seed) % 2147483646ull);
        if constexpr (ACT == 0) {
            o_zoi<true>(m, base, rng, lane, T, Ti, perm, fac(4), true, fac(0), false, p);
            o_zoi<true>(k, base, rng, lane, T, Ti, perm, fac(1), false, fac(2), true, p);
            o_zoi<true>(n, base, rng, lane, T, Ti, perm, fac(3), false, fac(5), true, p);
        } else if constexpr (ACT == 1) {
            int64_t *Ti2 = (int64_t *)(reg + P.off_ti2);
            int8_t *T2 = (int8_t *)(reg + P.off_t2);
            o_pluq<true>(m, base, rng, lane, T, T2, Ti, Ti2, perm, fac(4), true, fac(0), false, p);
            o_pluq<true>(k, base, rng, lane, T, T2, Ti, Ti2, perm, fac(1), false, fac(2), true, p);
            o_pluq<true>(n, base, rng, lane, T, T2, Ti, Ti2, perm, fac(3), false, fac(5), true, p);
        } else {
            const uint32_t *dinv = (const uint32_t *)(ldyn + P.off_dinv);
            (void)o_house<true>(m, base, rng, lane, T, perm, fac(4), true, fac(0), false, p, dinv);
            (void)o_house<true>(k, base, rng, lane, T, perm, fac(1), false, fac(2), true, p, dinv);
            (void)o_house<true>(n, base, rng, lane, T, perm, fac(3), false, fac(5), true, p, dinv);
        }
        OC_T(0);
        uint32_t nnz = 0, nno = 0, cost = 0;
        bool failed = false;
#pragma unroll 1
        for (uint32_t part = 0; part < 3u; ++part) {
            const uint32_t a_s = part == 1u ? k : m, b_s = part == 0u ? k : n, E = a_s * b_s;
            const OcPart Tp{fac(2u * part), fac(2u * part + 1u), a_s, b_s, part * r, part == 2u ? E : r, part == 2u ? r : E, part == 2u};
            if constexpr (SIZE) {
                uint16_t *len = (uint16_t *)img;
                uint32_t pn = 0, po = 0;
                oc_lengths(Tp, rp, pos, val, p, lane, len, pn, po);
                const uint32_t l = lane < Tp.rows ? (uint32_t)len[lane] : 0u;
                const uint32_t ent = wave_sum(l), pairs = wave_sum(l * (l - (l ? 1u : 0u)) / 2u), ml = wave_max(l);
                if (lane == 0) { atomicMax(&sz[part], ent); atomicMax(&sz[3u + part], pairs); atomicMax(&sz[6u + part], ml); }
                PLO_WAVE_SYNC();
            } else {
                const uint32_t c = oc_part_cost(C, part, Tp, rp, pos, val, p, img, keep, rs, lane, nnz, nno
#ifdef PLO_ORBIT_CSE_PROFILE
                                                , oc_t, oc_acc
#endif
                                                );
                failed |= c == ~0u;
                if (failed) break;
                cost += c;
            }
        }
        if constexpr (!SIZE) {
#ifdef PLO_ORBIT_CSE_PROFILE
            if (lane == 0 && !failed) { for (int q_ = 0; q_ < 5; ++q_) atomicAdd(&g_ocprof[q_], oc_acc[q_]); atomicAdd(&g_ocprof[5], 1ull); }
#endif
            if (lane == 0 && !failed) {
                if (J.out3) { J.out3[3u * cnd] = cost; J.out3[3u * cnd + 1u] = nnz; J.out3[3u * cnd + 2u] = nno; }
                const uint64_t key = ((uint64_t)cost << 42) | ((uint64_t)nnz << 21) | (uint64_t)nno;
                if (key < bkey) { bkey = key; bidx = cnd; }       // candidates come in increasing order: ties keep the first
            }
        }
        PLO_WAVE_SYNC();
    }
    if constexpr (!SIZE) {
        if (J.best && lane == 0) {
            const uint64_t slot = (uint64_t)blockIdx.x * nw + wave;
            J.best[2u * slot] = bkey; J.best[2u * slot + 1u] = bidx;
        }
    }
}

} // namespace plo
