// ===========================================================================
// plo_capi_cseq.hip -- host side of plo_cse_plan_create_q and plo_cse_q_universe (include/plinopt_hip.h): the plan of the wave
// kernels whose restart search is bit-exact with Optimizer() over the rationals.  Included at the end of plo_capi.hip: it stands on
// that file's helpers (fail, require_device, env_knob, qcsr_defect, inv_mod, ceil_log2, build_plan).
//
// Why a finite table is enough: RemOneCSE gives the new column an entry the row already had, so every entry of every
// step lies in V, the distinct entries of the input, and every pair ratio in R = { b/a : a, b in V }.  ProgramGen compares classes {v, -v},
// tests +-1 and, in Triangle, forms quotients next/iter in R.  U = +-(V u R u {1}) therefore holds every value a candidate compares; a
// 31-bit prime that divides no numerator or denominator of U and keeps its residues apart makes residue arithmetic exact on U.  What
// residues lose is Q's order, which the reference uses in ONE place: the std::map order of the pair triples (col, col, ratio), from
// which a tie is drawn.  The keys of such a plan carry the ratio's rank in U instead of its residue.
// ===========================================================================
#pragma once

namespace {
#define PLO_CSEQ_MAX_VALUES 64u      // |V|: U has at most 2 (64 + 64^2) elements, ranks of 14 bits
#define PLO_CSEQ_PRIME_TRIES 8
#define PLO_CSEQ_PRIME0 2147483629u  // the prime of the trilinear and dependency paths

// num/den in lowest terms with den > 0, 128 bits each.  Entries come in as 64-bit pairs, so a ratio of two always fits; ORDERING two
// ratios multiplies across and may not: q_mul throws, and the plan is refused.
struct QOverflow {};
struct QRat { __int128 n, d; };
__int128 q_gcd(__int128 a, __int128 b) { if (a < 0) a = -a; if (b < 0) b = -b; while (b) { const __int128 t = a % b; a = b; b = t; } return a; }
__int128 q_mul(__int128 a, __int128 b) { __int128 r; if (__builtin_mul_overflow(a, b, &r)) throw QOverflow{}; return r; }
QRat q_make(__int128 n, __int128 d) { if (d < 0) { n = -n; d = -d; } const __int128 g = q_gcd(n, d); return QRat{n / g, d / g}; }
QRat q_div(const QRat &a, const QRat &b) {                        // a / b, b != 0
    const __int128 g1 = q_gcd(a.n, b.n), g2 = q_gcd(a.d, b.d);
    return q_make(q_mul(a.n / g1, b.d / g2), q_mul(a.d / g2, b.n / g1));
}
bool q_less(const QRat &a, const QRat &b) { return q_mul(a.n, b.d) < q_mul(b.n, a.d); }
bool q_same(const QRat &a, const QRat &b) { return a.n == b.n && a.d == b.d; }
void q_sort_unique(std::vector<QRat> &v) { std::sort(v.begin(), v.end(), q_less); v.erase(std::unique(v.begin(), v.end(), q_same), v.end()); }

bool q_is_prime(uint32_t x) { if (x < 2) return false; for (uint32_t d = 2; (uint64_t)d * d <= x; ++d) if (x % d == 0) return false; return true; }
// residue of r modulo p; false when p divides its numerator or its denominator
bool q_residue(const QRat &r, uint32_t p, uint32_t &out) {
    int64_t a = (int64_t)(r.n % (__int128)p), d = (int64_t)(r.d % (__int128)p);
    if (a < 0) a += p;
    if (a == 0 || d == 0) return false;
    out = (uint32_t)((uint64_t)a * inv_mod((uint32_t)d, p) % p);
    return true;
}

struct QUniverse {
    std::vector<QRat> V, U;             // ascending over Q
    std::vector<uint32_t> ures;         // residues of U modulo prime
    uint32_t prime = 0;
    bool unit = false;                  // every entry is +-1
};

// V, U and the prime of a matrix (its CSR checked by the caller).  Host only.
int q_universe(const plo_qcsr_t *A, QUniverse &Q)
{
    const uint32_t nnz = A->rowptr[A->m];
    try {
        for (uint32_t e = 0; e < nnz; ++e) Q.V.push_back(q_make(A->num[e], A->den ? A->den[e] : 1));
        q_sort_unique(Q.V);                                     // (64-bit parts: these products fit)
    } catch (const QOverflow &) { return fail(PLO_E_UNSUPPORTED, "128-bit overflow while ordering the entries"); }
    if (Q.V.size() > PLO_CSEQ_MAX_VALUES)
        return fail(PLO_E_UNSUPPORTED, std::to_string(Q.V.size()) + " distinct values: the exact search over Q takes at most " + std::to_string(PLO_CSEQ_MAX_VALUES));
    Q.unit = true;
    for (const QRat &v : Q.V) Q.unit = Q.unit && v.d == 1 && (v.n == 1 || v.n == -1);
    try {
        Q.U.push_back(QRat{1, 1}); Q.U.push_back(QRat{-1, 1});
        for (const QRat &a : Q.V) {
            Q.U.push_back(a); Q.U.push_back(QRat{-a.n, a.d});
            for (const QRat &b : Q.V) { const QRat r = q_div(b, a); Q.U.push_back(r); Q.U.push_back(QRat{-r.n, r.d}); }
        }
        q_sort_unique(Q.U);
    } catch (const QOverflow &) {
        return fail(PLO_E_UNSUPPORTED, "128-bit overflow while forming the universe of values (the ratios of the entries cannot be ordered in 128 bits)");
    }
    // the prime: from PLO_CSEQ_PRIME0 (test knob PLO_CSE_Q_PRIME: from there) down through the primes
    uint32_t c = PLO_CSEQ_PRIME0;
    if (const auto k = env_knob("PLO_CSE_Q_PRIME")) if (*k >= 2 && *k < (1l << 31)) c = (uint32_t)*k;
    const uint32_t first = c;
    std::string tried;
    for (int tries = 0; tries < PLO_CSEQ_PRIME_TRIES && c >= 3u; --c) {
        if (!q_is_prime(c)) continue;
        ++tries; tried += (tried.empty() ? "" : ", ") + std::to_string(c);
        std::vector<uint32_t> res(Q.U.size());
        bool ok = true;
        for (size_t k = 0; ok && k < Q.U.size(); ++k) ok = q_residue(Q.U[k], c, res[k]);
        if (ok) { std::vector<uint32_t> s(res); std::sort(s.begin(), s.end()); ok = std::adjacent_find(s.begin(), s.end()) == s.end(); }
        if (ok) { Q.prime = c; Q.ures = std::move(res); return PLO_OK; }
    }
    return fail(PLO_E_UNSUPPORTED, "no prime among the first " + std::to_string(PLO_CSEQ_PRIME_TRIES) + " from " + std::to_string(first) + " down (" + (tried.empty() ? "none" : tried)
                + ") keeps the " + std::to_string(Q.U.size()) + " values of the universe apart");
}
} // namespace

extern "C" {

int plo_cse_q_universe(const plo_qcsr_t *A, uint32_t *prime, uint32_t *nvalues, uint32_t *nuniverse, int64_t *num, int64_t *den, uint32_t cap)
{
    if (!A || !prime || !nvalues || !nuniverse || (cap && (!num || !den))) return fail(PLO_E_ARG, "null argument");
    *prime = *nvalues = *nuniverse = 0;
    if (const char *d = qcsr_defect(A)) return fail(PLO_E_ARG, d);
    QUniverse Q;
    const int rc = q_universe(A, Q);
    *nvalues = (uint32_t)Q.V.size(); *nuniverse = (uint32_t)Q.U.size(); *prime = Q.prime;
    if (rc != PLO_OK) return rc;
    if (cap < Q.U.size()) return fail(PLO_E_CAPACITY, "the universe has " + std::to_string(Q.U.size()) + " elements, the arrays " + std::to_string(cap));
    for (const QRat &u : Q.U) if (u.n != (int64_t)u.n || u.d != (int64_t)u.d) return fail(PLO_E_CAPACITY, "an element of the universe does not fit 64 bits");
    for (size_t k = 0; k < Q.U.size(); ++k) { num[k] = (int64_t)Q.U[k].n; den[k] = (int64_t)Q.U[k].d; }
    return PLO_OK;
}

int plo_cse_plan_create_q(const plo_qcsr_t *A, uint32_t flags, plo_plan_t **out)
{
    if (!A || !out) return fail(PLO_E_ARG, "null argument");
    if (flags & ~(uint32_t)PLO_PLAN_HBM) return fail(PLO_E_ARG, "unknown flags");
    if (const char *d = qcsr_defect(A)) return fail(PLO_E_ARG, d);
    if (flags & PLO_PLAN_HBM) return fail(PLO_E_UNSUPPORTED, "the HBM-resident kernel family has no exact search over Q (LDS-resident plans only)");
    QUniverse Q;
    int rc = q_universe(A, Q);
    if (rc != PLO_OK) return rc;

    std::unique_ptr<plo_plan, int (*)(plo_plan *)> pl(new plo_plan(), plo_cse_plan_destroy);
    const uint32_t nnz = A->rowptr[A->m];
    pl->q = true; pl->qunit = Q.unit;
    pl->m = A->m; pl->n = A->n; pl->p = Q.unit ? 1u : Q.prime;
    pl->rowptr.assign(A->rowptr, A->rowptr + A->m + 1);
    pl->col.assign(A->col, A->col + nnz);
    pl->val.resize(nnz);
    for (uint32_t e = 0; e < nnz; ++e) {
        if (Q.unit) pl->val[e] = A->num[e] > 0 ? 1u : 0u;
        else (void)q_residue(q_make(A->num[e], A->den ? A->den[e] : 1), Q.prime, pl->val[e]);     // (an element of U: it has one)
    }
    if (!Q.unit) pl->qres = Q.ures;                                // build_plan puts the tables of plo::QTab behind the image
    // the shape limits of the LDS-resident kernels, before any device call
    std::vector<uint8_t> img;
    rc = build_plan(pl.get(), &img);
    if (rc == PLO_E_CAPACITY) return fail(PLO_E_UNSUPPORTED, "this matrix needs the HBM-resident kernel family (" + g_err + "), which has no exact search over Q");
    if (rc != PLO_OK) return rc;

    if ((rc = require_device(NOINIT_DEVICE0)) != PLO_OK) return rc;
    rc = build_plan(pl.get());
    if (rc == PLO_E_CAPACITY) return fail(PLO_E_UNSUPPORTED, "this matrix needs the HBM-resident kernel family (" + g_err + "), which has no exact search over Q");
    if (rc != PLO_OK) return rc;
    *out = pl.release();
    return PLO_OK;
}

} // extern "C"
