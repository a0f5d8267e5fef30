// ===========================================================================
// plo_capi_tprog.hip -- host side of the plo_tprog_* entries (include/plinopt_hip.h): the in-place trilinear program check of
// bin/TPchecker on the kernels of plo_tprog.hip.  Included at the end of plo_capi.hip: it stands on that file's launch helpers
// (fail, require_device, CallScope, timed_launch, env_knob, residue_of, qcsr_defect, dev_free).
// ===========================================================================
#pragma once

struct plo_tprog_plan {
    plo::TProgPlan P{};
    plo::TProgLinJob lin{};
    void *d_img = nullptr; uint32_t *d_alpha = nullptr, *d_beta = nullptr; unsigned long long *d_res = nullptr;   // d_res: the count, then the packed minimum
    uint32_t waves_per_wg = 1, lds_bytes = 0, lin_waves_per_wg = 1, lin_lds_bytes = 0, lin_units = 0, waves_per_launch = 0;
    uint32_t na = 0, nb = 0, nc0 = 0, nc = 0, w = 0, nrows = 0, flags = 0, mm_k = 0, mm_n = 0;
    uint64_t algo_bytes = 0;
    bool lin_done = false; unsigned long long lin_res[2] = {0, ~0ull};               // the three restoration blocks: once per plan
    // L and R by rows and P by rows as residues (the expected value of the first violated equation)
    std::vector<uint32_t> lrp, lcol, lval, rrp, rcol, rval, prp, pcol, pval;
};

namespace {
#define PLO_TPROG_MAX_RECORDS (1u << 24)
#define PLO_TPROG_MAX_TABLE_WORDS (1ull << 28)   // rows of alpha (or beta): 1 GiB on the host and on the device
#define PLO_TPROG_MAX_LAUNCH_WAVES 65536u        // 65536 waves of 64 pairs of at most 512 words: 2^31 equations in the packed minimum
#define PLO_TPROG_LDS_BUDGET (128u * 1024u)      // one wave of PLO_TPROG_MAX_WORDS words per lane

bool tprog_rows(const plo_qcsr_t *A, uint32_t q, std::vector<uint32_t> &rp, std::vector<uint32_t> &col, std::vector<uint32_t> &val) {
    rp.assign(1, 0u); col.clear(); val.clear();
    for (uint32_t i = 0; i < A->m; ++i) {
        for (uint32_t e = A->rowptr[i]; e < A->rowptr[i + 1]; ++e) {
            uint32_t v = 0;
            if (!residue_of(A->num[e], A->den ? A->den[e] : 1, q, v)) return false;
            if (v) { col.push_back(A->col[e]); val.push_back(v); }
        }
        rp.push_back((uint32_t)col.size());
    }
    return true;
}
uint32_t tprog_entry(const std::vector<uint32_t> &rp, const std::vector<uint32_t> &col, const std::vector<uint32_t> &val, uint32_t row, uint32_t c) {
    const auto b = col.begin() + rp[row], e = col.begin() + rp[row + 1], it = std::lower_bound(b, e, c);
    return it != e && *it == c ? val[(size_t)(it - col.begin())] : 0u;
}
// T[i][j][z] modulo q of the plan's target
uint32_t tprog_target(const plo_tprog_plan *pl, uint32_t i, uint32_t j, uint32_t z) {
    if (pl->flags & PLO_TPROG_MATMUL) return (i % pl->mm_k == j / pl->mm_n && z == (i / pl->mm_k) * pl->mm_n + j % pl->mm_n) ? 1u : 0u;
    const uint32_t q = pl->P.q; uint64_t s = 0;
    for (uint32_t e = pl->prp[z]; e < pl->prp[z + 1]; ++e) {
        const uint32_t t = pl->pcol[e];
        const uint64_t lr = (uint64_t)tprog_entry(pl->lrp, pl->lcol, pl->lval, t, i) * tprog_entry(pl->rrp, pl->rcol, pl->rval, t, j) % q;
        s = (s + lr * pl->pval[e]) % q;
    }
    return (uint32_t)s;
}
} // namespace

extern "C" {
int plo_tprog_plan_create_q(const plo_qcsr_t *L, const plo_qcsr_t *R, const plo_qcsr_t *P, const plo_tprog_rec_t *recs, uint64_t nrec, uint32_t flags, uint32_t q, plo_tprog_plan_t **plan)
{
    if (!L || !R || !P || !plan || (nrec && !recs)) return fail(PLO_E_ARG, "null argument");
    if (L->m != R->m || L->m != P->n)
        return fail(PLO_E_ARG, "inner dimensions " + std::to_string(L->m) + ", " + std::to_string(R->m) + ", " + std::to_string(P->n) + " of L, R and P differ");
    if (q < 2u || q >= (1u << 31)) return fail(PLO_E_ARG, "modulus " + std::to_string(q) + " outside 2 .. 2^31 - 1");
    for (const plo_qcsr_t *A : {L, R, P}) if (const char *d = qcsr_defect(A)) return fail(PLO_E_ARG, d);
    if (flags & ~(PLO_TPROG_EXPANDED | PLO_TPROG_MATMUL)) return fail(PLO_E_ARG, "unknown flags");
    const bool expanded = flags & PLO_TPROG_EXPANDED, matmul = flags & PLO_TPROG_MATMUL;
    if (expanded && matmul) return fail(PLO_E_ARG, "PLO_TPROG_EXPANDED and PLO_TPROG_MATMUL at once");
    const uint32_t r = L->m, na = L->n, nb = R->n, nc0 = P->m;
    if (na == 0 || nb == 0 || nc0 == 0) return fail(PLO_E_ARG, "na, nb and nc must be positive");
    const uint64_t nc64 = (uint64_t)nc0 + (expanded ? 1u : 0u), w64 = expanded ? 2u * nc64 : nc64;
    uint32_t mm_m = 0, mm_k = 0, mm_n = 0;
    if (matmul) {                                                    // LRP2MM, as plo_brent.hpp's brent_shape
        mm_n = (uint32_t)std::sqrt((double)((uint64_t)nb * nc0 / na));
        if (mm_n) { mm_m = nc0 / mm_n; mm_k = nb / mm_n; }
        if (!mm_n || (uint64_t)mm_m * mm_k != na || (uint64_t)mm_k * mm_n != nb || (uint64_t)mm_m * mm_n != nc0)
            return fail(PLO_E_ARG, std::to_string(na) + ", " + std::to_string(nb) + " and " + std::to_string(nc0) + " are not m k, k n and m n");
    }
    if (w64 > PLO_TPROG_MAX_WORDS || na > PLO_TPROG_MAX_WORDS || nb > PLO_TPROG_MAX_WORDS)
        return fail(PLO_E_CAPACITY, "na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + " or the width w = " + std::to_string(w64) + " above the " + std::to_string(PLO_TPROG_MAX_WORDS) + " state words that a lane keeps in LDS");
    if (nrec >= PLO_TPROG_MAX_RECORDS) return fail(PLO_E_CAPACITY, "2^24 records or more");
    if (r > PLO_BRENT_MAX_RANK) return fail(PLO_E_CAPACITY, "rank above 2^20");
    const uint32_t nc = (uint32_t)nc64, w = (uint32_t)w64, dims[3] = {na, nb, nc};

    // the streams: a, b and c on their own (the c one without AXPYs), and the bilinear one
    std::vector<uint32_t> sa, sb, sc, sbil;
    auto push = [](std::vector<uint32_t> &s, uint32_t op, uint32_t dst, uint32_t src, uint32_t co) { s.push_back(op); s.push_back(dst); s.push_back(src); s.push_back(co); };
    uint32_t naxpy = 0;
    for (uint64_t k = 0; k < nrec; ++k) {
        const plo_tprog_rec_t &x = recs[k];
        const std::string at = "record " + std::to_string(k) + ": ";
        if (x.family > 2u || x.op > PLO_TPROG_AXPY || x.part > 2u) return fail(PLO_E_ARG, at + "unknown family, operation or part");
        if (x.den <= 0) return fail(PLO_E_ARG, at + "non-positive denominator");
        uint32_t co = 0;
        if (!residue_of(x.num, x.den, q, co)) return fail(PLO_E_ARG, at + "a denominator is no unit modulo " + std::to_string(q));
        if (x.op == PLO_TPROG_AXPY) {
            if (x.family != 2u || x.dst >= nc || x.src >= na || x.src2 >= nb) return fail(PLO_E_ARG, at + "an AXPY is c[dst] += v a[src] b[src2] with indices in range");
            if ((x.part != 0u) != expanded) return fail(PLO_E_ARG, at + "low and hig parts go with PLO_TPROG_EXPANDED, and only they");
            if ((x.num != 1 && x.num != -1) || x.den != 1) return fail(PLO_E_ARG, at + "an AXPY has the coefficient 1 or -1");
            push(sa, 2u, naxpy, x.src, 0u); push(sb, 2u, naxpy, x.src2, 0u);
            push(sbil, PLO_TPROG_AXPY, x.part == 2u ? nc + x.dst : x.dst, naxpy, co);
            ++naxpy;
            continue;
        }
        if (x.part != 0u) return fail(PLO_E_ARG, at + "a part on a line that is no AXPY");
        if (x.dst >= dims[x.family] || (x.op == PLO_TPROG_ADD && x.src >= dims[x.family])) return fail(PLO_E_ARG, at + "index out of range");
        const uint32_t src = x.op == PLO_TPROG_ADD ? x.src : 0u;
        if (x.family == 0u) push(sa, x.op, x.dst, src, co);
        else if (x.family == 1u) push(sb, x.op, x.dst, src, co);
        else {
            push(sc, x.op, x.dst, src, co);
            push(sbil, x.op, x.dst, src, co);
            if (expanded) push(sbil, x.op, nc + x.dst, x.op == PLO_TPROG_ADD ? nc + src : 0u, co);
        }
    }
    plo_tprog_plan *pl = new plo_tprog_plan();
    std::unique_ptr<plo_tprog_plan, void (*)(plo_tprog_plan_t *)> guard(pl, plo_tprog_plan_destroy);
    if (!matmul && (!tprog_rows(L, q, pl->lrp, pl->lcol, pl->lval) || !tprog_rows(R, q, pl->rrp, pl->rcol, pl->rval) || !tprog_rows(P, q, pl->prp, pl->pcol, pl->pval)))
        return fail(PLO_E_ARG, "a denominator is no unit modulo " + std::to_string(q));
    // the target: row naxpy + t of the tables is L[t][.] and R[t][.], and c[z] -= P[z][t] alpha beta for every entry of P
    const uint64_t trows = matmul ? (uint64_t)mm_m * mm_k * mm_n : r;
    const uint64_t nrows = (uint64_t)naxpy + trows;
    // both refusals before anything of that size is allocated: the tables are dense rows (1 GiB each at most), the target's records
    // are one (two with the expanded flag) per entry of P, or m k n
    if (nrows * std::max(na, nb) >= PLO_TPROG_MAX_TABLE_WORDS) return fail(PLO_E_CAPACITY, "tables of operands of 2^28 words or more (" + std::to_string(nrows) + " rows of " + std::to_string(std::max(na, nb)) + ")");
    const uint64_t trecs = matmul ? trows : (uint64_t)pl->pcol.size() * (expanded ? 2u : 1u);
    if (sbil.size() / 4u + trecs >= PLO_TPROG_MAX_RECORDS) return fail(PLO_E_CAPACITY, "2^24 records or more with the target");
    std::vector<uint32_t> ha((size_t)trows * na, 0u), hb((size_t)trows * nb, 0u);
    if (matmul) {
        for (uint32_t a = 0; a < mm_m; ++a) for (uint32_t b = 0; b < mm_k; ++b) for (uint32_t c = 0; c < mm_n; ++c) {
            const size_t t = ((size_t)a * mm_k + b) * mm_n + c;
            ha[t * na + a * mm_k + b] = 1u; hb[t * nb + b * mm_n + c] = 1u;
            push(sbil, PLO_TPROG_AXPY, a * mm_n + c, naxpy + (uint32_t)t, q - 1u);
        }
    } else {
        for (uint32_t t = 0; t < r; ++t) {
            for (uint32_t e = pl->lrp[t]; e < pl->lrp[t + 1]; ++e) ha[(size_t)t * na + pl->lcol[e]] = pl->lval[e];
            for (uint32_t e = pl->rrp[t]; e < pl->rrp[t + 1]; ++e) hb[(size_t)t * nb + pl->rcol[e]] = pl->rval[e];
        }
        for (uint32_t z = 0; z < nc0; ++z) for (uint32_t e = pl->prp[z]; e < pl->prp[z + 1]; ++e) {
            push(sbil, PLO_TPROG_AXPY, z, naxpy + pl->pcol[e], q - pl->pval[e]);
            if (expanded) push(sbil, PLO_TPROG_AXPY, nc + z + 1u, naxpy + pl->pcol[e], q - pl->pval[e]);
        }
    }
    if (const int rc = require_device(NOINIT_PLAN)) return rc;

    pl->na = na; pl->nb = nb; pl->nc0 = nc0; pl->nc = nc; pl->w = w; pl->nrows = (uint32_t)nrows; pl->flags = flags; pl->mm_k = mm_k; pl->mm_n = mm_n;
    plo::TProgPlan &Q = pl->P;
    Q.na = na; Q.nb = nb; Q.w = w; Q.nblk = (nb + 63u) / 64u; Q.q = q; Q.mu = (~0ull) / q; Q.nrec = (uint32_t)(sbil.size() / 4u);
    pl->waves_per_wg = std::min(4u, std::max(1u, PLO_TPROG_LDS_BUDGET / (256u * w)));
    pl->lds_bytes = 256u * w * pl->waves_per_wg;
    const uint32_t words = std::max(na, std::max(nb, nc));
    pl->lin_waves_per_wg = std::min(4u, std::max(1u, PLO_TPROG_LDS_BUDGET / (256u * words)));
    pl->lin_lds_bytes = 256u * words * pl->lin_waves_per_wg;
    if (std::max(pl->lds_bytes, pl->lin_lds_bytes) > g_lds_max) return fail(PLO_E_CAPACITY, "the state words do not fit the LDS of this device");
    uint64_t wpl = PLO_TPROG_MAX_LAUNCH_WAVES;
    if (const auto c = env_knob("PLO_TPROG_WAVES")) wpl = (uint64_t)std::min<long>(std::max<long>(*c, 1), (long)wpl);   // test knob: several launches on a small input
    pl->waves_per_launch = (uint32_t)wpl;
    Q.skip = 1u;
    if (const auto c = env_knob("PLO_TPROG_SKIP")) Q.skip = *c ? 1u : 0u;                                               // measuring knob: 0 walks every ADD and SCA record
    pl->algo_bytes = 4ull * (sa.size() + sb.size() + sc.size() + sbil.size()) + 4ull * nrows * ((uint64_t)na + nb);

    // the image: the four streams (16-byte records); the tables apart: the linear kernel writes every word of their program rows
    // (one store per AXPY and unit input), the target rows behind them come from here
    const std::vector<uint32_t> *arr[4] = {&sa, &sb, &sc, &sbil};
    size_t off[4], words_img = 0;
    for (int j = 0; j < 4; ++j) { off[j] = words_img; words_img += arr[j]->size(); }
    std::vector<uint32_t> img(std::max<size_t>(words_img, 4), 0u);
    for (int j = 0; j < 4; ++j) if (!arr[j]->empty()) memcpy(img.data() + off[j], arr[j]->data(), 4u * arr[j]->size());
    const size_t wa = std::max<size_t>((size_t)nrows * na, 1), wb = std::max<size_t>((size_t)nrows * nb, 1);
    if (hipMalloc(&pl->d_img, 4u * img.size()) != hipSuccess || hipMemcpy(pl->d_img, img.data(), 4u * img.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void **)&pl->d_alpha, 4u * wa) != hipSuccess || hipMalloc((void **)&pl->d_beta, 4u * wb) != hipSuccess ||
        (!ha.empty() && hipMemcpy(pl->d_alpha + (size_t)naxpy * na, ha.data(), 4u * ha.size(), hipMemcpyHostToDevice) != hipSuccess) ||
        (!hb.empty() && hipMemcpy(pl->d_beta + (size_t)naxpy * nb, hb.data(), 4u * hb.size(), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMalloc((void **)&pl->d_res, 16) != hipSuccess ||
        hipFuncSetAttribute((const void *)plo::tprog_linear_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PLO_TPROG_LDS_BUDGET) != hipSuccess ||
        hipFuncSetAttribute((const void *)plo::tprog_bilinear_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PLO_TPROG_LDS_BUDGET) != hipSuccess)   // the largest any plan asks for: plans do not lower it under each other
        return fail(PLO_E_HIP, "device setup of the trilinear-program plan failed");
    const uint32_t *d = (const uint32_t *)pl->d_img;
    Q.recs = (const uint4 *)(d + off[3]); Q.alpha = pl->d_alpha; Q.beta = pl->d_beta;
    plo::TProgLinJob &J = pl->lin;
    const uint32_t ebase[3] = {0u, na * na, na * na + nb * nb};
    uint32_t *table[3] = {pl->d_alpha, pl->d_beta, nullptr};
    for (int f = 0; f < 3; ++f) {
        J.fam[f].recs = (const uint4 *)(d + off[f]); J.fam[f].nrec = (uint32_t)(arr[f]->size() / 4u);
        J.fam[f].n = dims[f]; J.fam[f].nblk = (dims[f] + 63u) / 64u; J.fam[f].table = table[f]; J.fam[f].ebase = ebase[f];
        pl->lin_units += J.fam[f].nblk;
    }
    J.q = q; J.mu = Q.mu; J.words = words; J.count = pl->d_res; J.first = pl->d_res + 1;
    *plan = guard.release();
    return PLO_OK;
}

void plo_tprog_plan_destroy(plo_tprog_plan_t *pl)
{
    if (pl) { dev_free(pl->d_img, pl->d_alpha, pl->d_beta, pl->d_res); delete pl; }
}

int plo_tprog_plan_info(plo_tprog_plan_t *pl, uint32_t out[8])
{
    if (!pl || !out) return fail(PLO_E_ARG, "null argument");
    out[0] = PLO_TPROG_MAX_WORDS; out[1] = 64u * pl->w; out[2] = pl->waves_per_wg; out[3] = pl->waves_per_launch;
    out[4] = pl->P.nrec; out[5] = pl->na * pl->nb; out[6] = pl->w; out[7] = pl->nrows;
    return PLO_OK;
}

int plo_tprog_check(plo_tprog_plan_t *pl, uint64_t pair0, uint64_t pair1, plo_brent_result_t *res, plo_stats_t *stats)
{
    if (!pl || !res) return fail(PLO_E_ARG, "null argument");
    const uint64_t npairs = (uint64_t)pl->na * pl->nb;
    if (pair0 >= pair1 || pair1 > npairs) return fail(PLO_E_ARG, "pairs " + std::to_string(pair0) + " .. " + std::to_string(pair1) + ": an empty range or one beyond the " + std::to_string(npairs) + " pairs");
    if (const int rc = require_device(NOINIT_PLAN)) return rc;
    CallScope call(stats); plo_stats_t *st = call.st;
    const plo::TProgPlan &Q = pl->P;
    *res = plo_brent_result_t{0, ~0ull, 0, 0};
    int rc = PLO_OK;
    auto clear = [&] { return hipMemsetAsync(pl->d_res, 0, 8, g_stream) == hipSuccess && hipMemsetAsync(pl->d_res + 1, 0xFF, 8, g_stream) == hipSuccess; };
    const uint64_t nblocks = (uint64_t)pl->na * pl->na + (uint64_t)pl->nb * pl->nb + (uint64_t)pl->nc * pl->nc;
    if (!pl->lin_done) {                                             // the tables of operands (and the three blocks), once per plan
        if (!clear()) return call.done(fail(PLO_E_HIP, "clearing the result words"));
        const uint64_t grid = (pl->lin_units + pl->lin_waves_per_wg - 1u) / pl->lin_waves_per_wg;
        const LaunchShape shape{grid, pl->lin_lds_bytes, pl->lin_waves_per_wg, pl->algo_bytes};
        rc = timed_launch(st, &shape, [&] {
            hipLaunchKernelGGL(plo::tprog_linear_kernel, dim3((uint32_t)grid), dim3(64 * pl->lin_waves_per_wg), pl->lin_lds_bytes, g_stream, pl->lin);
        });
        if (rc == PLO_OK && hipMemcpy(pl->lin_res, pl->d_res, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PLO_E_HIP, "copy back of the result words");
        if (rc != PLO_OK) return call.done(rc);
        pl->lin_done = true;
    }
    const uint64_t unit0 = (pair0 / Q.nb) * Q.nblk + (pair0 % Q.nb) / 64u, unit1 = ((pair1 - 1u) / Q.nb) * Q.nblk + ((pair1 - 1u) % Q.nb) / 64u + 1u;
    for (uint64_t u0 = unit0; rc == PLO_OK && u0 < unit1;) {
        const uint64_t cnt = std::min<uint64_t>(pl->waves_per_launch, unit1 - u0);
        if (!clear()) { rc = fail(PLO_E_HIP, "clearing the result words"); break; }
        plo::TProgJob J{}; J.pair0 = pair0; J.pair1 = pair1; J.unit0 = u0; J.nunits = (uint32_t)cnt;
        J.pairbase = (u0 / Q.nblk) * Q.nb + (u0 % Q.nblk) * 64u; J.count = pl->d_res; J.first = pl->d_res + 1;
        const uint64_t grid = (cnt + pl->waves_per_wg - 1u) / pl->waves_per_wg;
        rc = timed_launch(pl, grid, 0, st, [&] {
            hipLaunchKernelGGL(plo::tprog_bilinear_kernel, dim3((uint32_t)grid), dim3(64 * pl->waves_per_wg), pl->lds_bytes, g_stream, pl->P, J);
        });
        unsigned long long wd[2] = {0, 0};
        if (rc == PLO_OK && hipMemcpy(wd, pl->d_res, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PLO_E_HIP, "copy back of the result words");
        if (rc != PLO_OK) break;
        if (wd[0]) {
            if (res->violated == 0) { res->first = J.pairbase * Q.w + (wd[1] >> 32); res->value = (uint32_t)wd[1]; }   // launches go by increasing pair
            res->violated += wd[0];
        }
        u0 += cnt;
    }
    if (rc != PLO_OK) return call.done(rc);
    st->candidates = (pair1 - pair0) * Q.w + (pair0 == 0 ? nblocks : 0u);
    if (res->violated) {                                             // the kernel holds found - expected: the target is subtracted there
        const uint64_t z = res->first % Q.w, pair = res->first / Q.w;
        const uint32_t i = (uint32_t)(pair / Q.nb), j = (uint32_t)(pair % Q.nb);
        uint32_t want = 0;
        if (!(pl->flags & PLO_TPROG_EXPANDED)) want = tprog_target(pl, i, j, (uint32_t)z);
        else if (z < pl->nc) want = z < pl->nc0 ? tprog_target(pl, i, j, (uint32_t)z) : 0u;
        else want = z - pl->nc >= 1u ? tprog_target(pl, i, j, (uint32_t)(z - pl->nc - 1u)) : 0u;
        res->expected = want; res->value = (uint32_t)(((uint64_t)res->value + want) % Q.q);
    }
    if (pair0 == 0 && pl->lin_res[0]) {
        if (res->violated == 0) {
            const uint64_t rel = pl->lin_res[1] >> 32;
            res->first = npairs * Q.w + rel; res->value = (uint32_t)pl->lin_res[1];
            uint64_t e = rel; uint32_t n = pl->na;
            if (e >= (uint64_t)n * n) { e -= (uint64_t)n * n; n = pl->nb; if (e >= (uint64_t)n * n) { e -= (uint64_t)n * n; n = pl->nc; } }
            res->expected = e / n == e % n ? 1u : 0u;
        }
        res->violated += pl->lin_res[0];
    }
    return call.done(rc);
}
} // extern "C"
