// ==========================================================================
// plo_orbit.hpp -- one candidate of the De Groote orbit search (bin/orbiter; reference src/orbiter.cpp:272-324) on the host.
// A candidate is (U, V, W), drawn from the seed's stream (include/plinopt_hip.h, PLO_ORBIT_*), and transforms the
// row-major triple (L, R, P) of an m x k x n product into L.(U^-1 (x) V), R.(V^-T (x) W), (U (x) W^-1).P.  Read as
// matrices, row i of L (m x k) becomes U^-T X V, row i of R (k x n) becomes V^-1 Y W and column j of P (m x n) becomes
// U Z W^-T: the "sandwich" form, without the Kronecker products.  U = Pi_P T Pi_Q^T with T upper triangular, +-1 on
// its diagonal and {-1, 0, 1} above, so U^-1 = Pi_Q T^-1 Pi_P^T is integral (back-substitution, entries of size at most
// 2^(s-2)).  That is the default action; ORBIT_ACT_PLUQ draws a product of two triangles (integral inverse by two
// substitutions) and ORBIT_ACT_HOUSEHOLDER an orthogonal matrix, kept as integer numerators over one denominator d.
// The same function scores a candidate in the host loop and replays the winner.
// ==========================================================================
#pragma once
#include "plo_host.hpp"
#include <cmath>

namespace plo {

enum { ORBIT_DENSITY = 0, ORBIT_CSE = 1, ORBIT_CANONICAL = 2, ORBIT_GROWTH = 3 };
// ORBIT_CSE (`-z`): every part is scored by min(naiveOps, the best of `sub` Optimizer runs with the streams seed0 .. seed0 + sub - 1)
struct OrbitCse { size_t sub = 1; uint64_t seed0 = 0; };
enum { ORBIT_ACT_TRIANGULAR = 0, ORBIT_ACT_PLUQ = 1, ORBIT_ACT_HOUSEHOLDER = 2 };
constexpr uint64_t ORBIT_BASE = ~0ull;

// M (s x s, row-major) and its inverse: integer numerators over the denominator den (1 but for a Householder matrix)
struct Zoi { size_t s = 0; std::vector<int64_t> M, Mi; int64_t den = 1; };

// d is a unit of the run's field: d != 0 over Q, gcd(d, modulus) = 1 modulo a number
inline bool orbit_unit(const QField &, int64_t d) { return d != 0; }
inline bool orbit_unit(const ZpField &f, int64_t d) { return std::gcd((uint64_t)d, (uint64_t)f.p) == 1; }
inline bool orbit_unit(const Zp64Field &f, int64_t d) { return std::gcd((uint64_t)d, f.p) == 1; }

// what every action draws first: Fisher-Yates P, then Q, then the s sign bits
struct ZoiStart { std::vector<size_t> P, Q; std::vector<int64_t> D; };
inline ZoiStart zoi_start(CandRng &rng, size_t s) {
    ZoiStart z; z.P.resize(s); z.Q.resize(s); z.D.resize(s);
    std::iota(z.P.begin(), z.P.end(), 0); std::iota(z.Q.begin(), z.Q.end(), 0);
    for (auto *perm : {&z.P, &z.Q})
        for (size_t i = s; i > 1; --i) std::swap((*perm)[i - 1], (*perm)[rng.next() % i]);
    for (size_t i = 0; i < s; ++i) z.D[i] = (rng.next() & 1u) ? 1 : -1;
    return z;
}

// ORBIT_ACT_PLUQ (reference src/orbiter.cpp:78-96): Lambda lower triangular (D on the diagonal, then the strict lower part
// row-major), then s vectors u_i (1 at Q[i], draws before, zeros behind); row P[i] of M is Lambda.u_i.  M = Pi_P Um Lambda^T
// with Um[i] = u_i = row Q[i] of the unit lower triangular Lu, so M^-1[a][P[i]] = sum_b Lambda^-1[b][a] Lu^-1[b][Q[i]].
inline Zoi zoi_pluq(CandRng &rng, size_t s) {
    const ZoiStart z = zoi_start(rng, s);
    std::vector<int64_t> La(s * s, 0), Lu(s * s, 0), Lai(s * s, 0), Lui(s * s, 0);
    for (size_t i = 0; i < s; ++i) La[i * s + i] = z.D[i];
    for (size_t i = 0; i < s; ++i) for (size_t j = 0; j < i; ++j) La[i * s + j] = (int64_t)(rng.next() % 3u) - 1;
    for (size_t i = 0; i < s; ++i) {
        const size_t q = z.Q[i];
        Lu[q * s + q] = 1;
        for (size_t j = 0; j < q; ++j) Lu[q * s + j] = (int64_t)(rng.next() % 3u) - 1;
    }
    // inverses of the lower triangles by forward substitution, column by column
    for (const auto &pr : {std::make_pair(&La, &Lai), std::make_pair(&Lu, &Lui)}) {
        const std::vector<int64_t> &T = *pr.first; std::vector<int64_t> &Ti = *pr.second;
        for (size_t j = 0; j < s; ++j)
            for (size_t i = j; i < s; ++i) {
                int64_t acc = i == j ? 1 : 0;
                for (size_t l = j; l < i; ++l) acc -= T[i * s + l] * Ti[l * s + j];
                Ti[i * s + j] = T[i * s + i] * acc;
            }
    }
    Zoi r; r.s = s; r.M.assign(s * s, 0); r.Mi.assign(s * s, 0);
    for (size_t i = 0; i < s; ++i) for (size_t c = 0; c < s; ++c) {
        int64_t a = 0, b = 0;
        for (size_t j = 0; j < s; ++j) { a += La[c * s + j] * Lu[z.Q[i] * s + j]; b += Lai[j * s + c] * Lui[j * s + z.Q[i]]; }
        r.M[z.P[i] * s + c] = a; r.Mi[c * s + z.P[i]] = b;
    }
    return r;
}

// ORBIT_ACT_HOUSEHOLDER (reference :99-123): u in {-1, 0, 1}^s, d = u.u; N = diag(D) (I - 2 u u^T / d) when d is a unit, else
// diag(D); N^-1 = (I - 2 u u^T / d) diag(D).  M[P[i]][Q[j]] = N[i][j], M^-1[Q[i]][P[j]] = N^-1[i][j]; numerators over d.
template <class F> Zoi zoi_householder(const F &f, CandRng &rng, size_t s) {
    const ZoiStart z = zoi_start(rng, s);
    std::vector<int64_t> u(s);
    int64_t d = 0;
    for (size_t i = 0; i < s; ++i) { u[i] = (int64_t)(rng.next() % 3u) - 1; d += u[i] * u[i]; }
    const bool refl = orbit_unit(f, d);
    Zoi r; r.s = s; r.M.assign(s * s, 0); r.Mi.assign(s * s, 0); r.den = refl ? d : 1;
    for (size_t i = 0; i < s; ++i) for (size_t j = 0; j < s; ++j) {
        const int64_t h = refl ? (i == j ? d : 0) - 2 * u[i] * u[j] : (i == j ? 1 : 0);
        r.M[z.P[i] * s + z.Q[j]] = z.D[i] * h; r.Mi[z.Q[i] * s + z.P[j]] = h * z.D[j];
    }
    return r;
}

// the stream's matrix: Fisher-Yates P, then Q, then the s sign bits, then the strict upper part row-major
inline Zoi zoi_matrix(CandRng &rng, size_t s) {
    std::vector<size_t> P(s), Q(s);
    std::iota(P.begin(), P.end(), 0); std::iota(Q.begin(), Q.end(), 0);
    for (auto *perm : {&P, &Q})
        for (size_t i = s; i > 1; --i) std::swap((*perm)[i - 1], (*perm)[rng.next() % i]);
    std::vector<int64_t> T(s * s, 0), Ti(s * s, 0);
    for (size_t i = 0; i < s; ++i) T[i * s + i] = (rng.next() & 1u) ? 1 : -1;
    for (size_t i = 0; i < s; ++i) for (size_t j = i + 1; j < s; ++j) T[i * s + j] = (int64_t)(rng.next() % 3u) - 1;
    // T^-1 by back-substitution, column by column (1/d = d for d = +-1)
    for (size_t j = 0; j < s; ++j)
        for (size_t i = j + 1; i-- > 0;) {
            int64_t acc = i == j ? 1 : 0;
            for (size_t l = i + 1; l <= j; ++l) acc -= T[i * s + l] * Ti[l * s + j];
            Ti[i * s + j] = T[i * s + i] * acc;
        }
    Zoi z; z.s = s; z.M.assign(s * s, 0); z.Mi.assign(s * s, 0);
    for (size_t i = 0; i < s; ++i) for (size_t j = i; j < s; ++j) { z.M[P[i] * s + Q[j]] = T[i * s + j]; z.Mi[Q[i] * s + P[j]] = Ti[i * s + j]; }
    return z;
}
inline Zoi zoi_identity(size_t s) { Zoi z; z.s = s; z.M.assign(s * s, 0); for (size_t i = 0; i < s; ++i) z.M[i * s + i] = 1; z.Mi = z.M; return z; }

struct OrbitUVW { Zoi U, V, W; };
template <class F> OrbitUVW orbit_uvw(const F &f, size_t m, size_t k, size_t n, uint64_t seed, int action) {
    if (seed == ORBIT_BASE) return {zoi_identity(m), zoi_identity(k), zoi_identity(n)};
    CandRng rng(seed);
    auto draw = [&](size_t s) {
        if (action == ORBIT_ACT_PLUQ) return zoi_pluq(rng, s);
        if (action == ORBIT_ACT_HOUSEHOLDER) return zoi_householder(f, rng, s);
        return zoi_matrix(rng, s);
    };
    OrbitUVW c;
    c.U = draw(m); c.V = draw(k); c.W = draw(n);
    return c;
}

// m, k, n of a triple with L r x mk, R r x kn, P mn x r (exact integer square root of kn.mn/mk), false otherwise
inline bool orbit_shape(size_t lm, size_t ln, size_t rm, size_t rn, size_t pm, size_t pn, size_t &m, size_t &k, size_t &n) {
    if (lm != rm || lm != pn || ln == 0 || rn == 0 || pm == 0) return false;
    const unsigned __int128 num = (unsigned __int128)rn * pm;
    if (num % ln) return false;
    const uint64_t q = (uint64_t)(num / ln);
    uint64_t s = 0;
    for (uint64_t b = 1ull << 31; b; b >>= 1) if ((unsigned __int128)(s | b) * (s | b) <= q) s |= b;
    if (s == 0 || s * s != q || pm % s || rn % s) return false;
    n = (size_t)s; m = pm / n; k = rn / n;
    return m * k == ln && k * n == rn && m * n == pm;
}

// (ORBIT_GROWTH: cost holds the 64-bit pattern of the growth factor, a non-negative finite double: the orders below are the numeric ones)
struct OrbitCount { size_t cost = 0, nnz = 0, nno = 0; };
static_assert(sizeof(size_t) == 8 && sizeof(double) == 8, "the growth factor travels as its bits in OrbitCount::cost");
inline size_t growth_bits(double g) { uint64_t b; memcpy(&b, &g, 8); return (size_t)b; }
inline double growth_value(size_t bits) { const uint64_t b = bits; double g; memcpy(&g, &b, 8); return g; }
inline bool operator<(const OrbitCount &a, const OrbitCount &b) { return std::tie(a.cost, a.nnz, a.nno) < std::tie(b.cost, b.nnz, b.nno); }
inline bool operator==(const OrbitCount &a, const OrbitCount &b) { return std::tie(a.cost, a.nnz, a.nno) == std::tie(b.cost, b.nnz, b.nno); }

// The triple over F, P kept as its transpose (the columns of P are what the sandwich transforms)
template <class F> struct OrbitTriple { SparseMat<typename F::Elt> L, R, PT; size_t m = 0, k = 0, n = 0; };

// n_g of PLO_ORBIT_GROWTH (include/plinopt_hip.h) for one transformed row: `in` is the input row, whose denominators give the
// scale c_g, `acc` its outputs.  S_g = sum (acc c_g)^2 as an exact 128-bit integer, then sqrt(double(S_g)) / double(c_g): the
// device's operations in the device's order (it takes the inputs whose S_g and c_g stay below 2^53, where both conversions are
// exact; beyond that each is one rounding to nearest here).  A sum that leaves 128 bits is an overflow.
inline double orbit_row_norm(const QField &, const SparseMat<Rat>::Row &in, const std::vector<Rat> &acc) {
    __int128 l = 1;
    for (const auto &e : in) l = Rat::mulck(l / Rat::gcd(l, e.second.d), e.second.d);
    unsigned __int128 S = 0;
    for (const Rat &a : acc) {
        if (a.n == 0) continue;
        if (l % a.d) throw std::logic_error("growth measure: an output is no multiple of 1/scale");
        const __int128 v = Rat::mulck(a.n, l / a.d);
        const unsigned __int128 u = v < 0 ? (unsigned __int128)(-v) : (unsigned __int128)v;
        if (u >> 63 || __builtin_add_overflow(S, u * u, &S)) throw std::overflow_error("growth measure: sum of squares beyond 128 bits");
    }
    const double s = std::sqrt((double)S), c = (double)l;
    return s / c;
}
template <class F, class Row, class Acc> double orbit_row_norm(const F &, const Row &, const Acc &) { throw std::logic_error("the growth measure is defined over Q only"); }

// one part of the sandwich: out_i(p, q) = sum over the entries (a, b, x) of row i of A[a][p] x B[b][q], for the rows of X
// (columns a * cb + b; output pr x qc); A is sa x sa over the denominator da, B is sb x sb over db (row-major); Out gets the
// rows when asked, norms the rows' 2-norms (ORBIT_GROWTH)
template <class F> void orbit_part(const F &f, const SparseMat<typename F::Elt> &X, size_t cb, const std::vector<int64_t> &A, int64_t da, size_t sa,
                                   const std::vector<int64_t> &B, int64_t db, size_t sb, OrbitCount &c, size_t &canon, SparseMat<typename F::Elt> *Out, std::vector<double> *norms = nullptr) {
    using E = typename F::Elt;
    std::vector<E> acc(sa * sb);
    std::vector<E> Af(A.size()), Bf(B.size());
    for (size_t t = 0; t < A.size(); ++t) Af[t] = da == 1 ? f.fromInt(A[t]) : f.div(f.fromInt(A[t]), f.fromInt(da));
    for (size_t t = 0; t < B.size(); ++t) Bf[t] = db == 1 ? f.fromInt(B[t]) : f.div(f.fromInt(B[t]), f.fromInt(db));
    if (Out) *Out = SparseMat<E>(X.rowdim(), sa * sb);
    for (size_t i = 0; i < X.rowdim(); ++i) {
        std::fill(acc.begin(), acc.end(), f.zero());
        for (const auto &e : X.rows[i]) {
            const size_t a = e.first / cb, b = e.first % cb;
            for (size_t p = 0; p < sa; ++p) {
                if (A[a * sa + p] == 0) continue;
                const E ax = f.mul(Af[a * sa + p], e.second);
                for (size_t q = 0; q < sb; ++q) if (B[b * sb + q] != 0) acc[p * sb + q] = f.add(acc[p * sb + q], f.mul(ax, Bf[b * sb + q]));
            }
        }
        size_t nz = 0;
        for (size_t t = 0; t < acc.size(); ++t) {
            if (f.isZero(acc[t])) continue;
            ++nz; if (!absOne(f, acc[t])) ++c.nno;
            if (Out) Out->rows[i].emplace_back(t, acc[t]);
        }
        c.nnz += nz; canon += nz == 1;
        if (norms) norms->push_back(orbit_row_norm(f, X.rows[i], acc));
    }
}

// c(M) of include/plinopt_hip.h (PLO_ORBIT_CSE): what CSEOptimiser leaves in nbops under the default cmpOpCount, summed
// (reference src/orbiter.cpp:183-189)
template <class F> size_t orbit_cse_cost(const F &f, const SparseMat<typename F::Elt> &M, const OrbitCse &z) {
    const auto nv = naive_ops(f, M);
    size_t best = nv.first + nv.second;
    if (best == 0) return 0;
    std::ostream sink(nullptr);                                                          // (no buffer: the program text goes nowhere)
    for (size_t j = 0; j < z.sub; ++j) {
        Replay<F> R(f, M, z.seed0 + j, sink);
        const auto ops = R.optimizer();
        best = std::min(best, ops.first + ops.second);
    }
    return best;
}

template <class F> OrbitCount orbit_candidate(const F &f, const OrbitTriple<F> &T, uint64_t seed, int measure, int action, OrbitTriple<F> *out = nullptr, const OrbitCse &z = OrbitCse());
// the same without the matrices
template <class F> OrbitCount orbit_candidate(const F &f, const OrbitTriple<F> &T, uint64_t seed, int measure, int action, const OrbitCse &z) { return orbit_candidate(f, T, seed, measure, action, (OrbitTriple<F> *)nullptr, z); }

// counts of candidate `seed` (cost = nnz, or L.m + R.m + P.n - the rows with one non-zero for ORBIT_CANONICAL, or the operations
// of the best programs found for ORBIT_CSE, or the bits of the 2-norm growth factor for ORBIT_GROWTH, over Q); the three transformed matrices (P transposed back) when out is given
template <class F> OrbitCount orbit_candidate(const F &f, const OrbitTriple<F> &T, uint64_t seed, int measure, int action, OrbitTriple<F> *out, const OrbitCse &z) {
    OrbitTriple<F> mine;
    if (measure == ORBIT_CSE && !out) out = &mine;
    const OrbitUVW c = orbit_uvw(f, T.m, T.k, T.n, seed, action);
    const size_t m = T.m, k = T.k, n = T.n;
    auto tr = [](const std::vector<int64_t> &M, size_t s) { std::vector<int64_t> R(s * s); for (size_t i = 0; i < s; ++i) for (size_t j = 0; j < s; ++j) R[j * s + i] = M[i * s + j]; return R; };
    OrbitCount r; size_t canon = 0;
    std::vector<double> nl, nr, np;                                                        // ORBIT_GROWTH: the 2-norms of the transformed rows
    const bool growth = measure == ORBIT_GROWTH;
    orbit_part(f, T.L, k, c.U.Mi, c.U.den, m, c.V.M, c.V.den, k, r, canon, out ? &out->L : nullptr, growth ? &nl : nullptr);                  // U^-T X V: A[a][p] = U^-1[a][p]
    orbit_part(f, T.R, n, tr(c.V.Mi, k), c.V.den, k, c.W.M, c.W.den, n, r, canon, out ? &out->R : nullptr, growth ? &nr : nullptr);           // V^-1 Y W: A[b][p] = V^-1[p][b]
    orbit_part(f, T.PT, n, tr(c.U.M, m), c.U.den, m, tr(c.W.Mi, n), c.W.den, n, r, canon, out ? &out->PT : nullptr, growth ? &np : nullptr);  // U Z W^-T: A[a][p] = U[p][a], B[c][q] = W^-1[q][c]
    r.cost = measure == ORBIT_CANONICAL ? T.L.rowdim() + T.R.rowdim() + T.PT.rowdim() - canon : r.nnz;
    if (measure == ORBIT_CSE) r.cost = orbit_cse_cost(f, out->L, z) + orbit_cse_cost(f, out->R, z) + orbit_cse_cost(f, transpose(out->PT), z);
    if (growth) {                                                                          // one product pair and one addition per i, in increasing i
        double g = 0.0;
        for (size_t i = 0; i < nl.size(); ++i) { const double lr = nl[i] * nr[i], t = lr * np[i]; g = g + t; }
        r.cost = growth_bits(g);
    }
    if (out) { out->m = m; out->k = k; out->n = n; }
    return r;
}

// The Brent equations of the triple over F, exactly: sum_t L[t][a k + b] R[t][b' n + c] P[a' n + c'][t] = [a = a'][b = b'][c = c'].
// Over Q an overflow throws; the caller reports it as a failed check.
template <class F> bool orbit_mm_check(const F &f, const OrbitTriple<F> &T) {
    using E = typename F::Elt;
    const size_t m = T.m, k = T.k, n = T.n, mk = m * k, kn = k * n, mn = m * n;
    std::vector<E> S(mk * kn * mn, f.zero());
    for (size_t t = 0; t < T.L.rowdim(); ++t)
        for (const auto &l : T.L.rows[t]) for (const auto &r : T.R.rows[t]) {
            const E lr = f.mul(l.second, r.second);
            for (const auto &p : T.PT.rows[t]) { E &s = S[(l.first * kn + r.first) * mn + p.first]; s = f.add(s, f.mul(lr, p.second)); }
        }
    for (size_t a = 0; a < m; ++a) for (size_t b = 0; b < k; ++b) for (size_t b2 = 0; b2 < k; ++b2) for (size_t c = 0; c < n; ++c)
        for (size_t a2 = 0; a2 < m; ++a2) for (size_t c2 = 0; c2 < n; ++c2) {
            const E &s = S[((a * k + b) * kn + b2 * n + c) * mn + a2 * n + c2];
            if (!(a == a2 && b == b2 && c == c2) ? !f.isZero(s) : !f.isOne(s)) return false;
        }
    return true;
}

} // namespace plo
