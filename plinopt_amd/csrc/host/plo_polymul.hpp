// ==========================================================================
// plo_polymul.hpp -- the coefficient equations of a polynomial-multiplication triple on the host (bin/PMchecker --gpu 0;
// DESIGN.md 2.13): the parser of -P, the table rho[z] = X^z mod f, the host loop, the certificate that turns checks modulo
// primes into a proof over Q, and the wording of the verdict lines.
//
// L (r x na), R (r x nb), P (nc x r).  The pair (i, j) = i nb + j has the sums S[z] = sum_t L[t][i] R[t][j] P[z][t] (z < nc, 0
// beyond) and the defect polynomial D_ij = sum_z S[z] X^z - X^(i+j).  With Z = max(nc, na + nb - 1):
//   without f: w = Z, equation e = (i nb + j) w + c asks S[c] == [c == i + j];
//   with f of degree d: w = d, equation e = (i nb + j) d + c asks sum_{z < nc} S[z] rho[z][c] == rho[i + j][c]
//   (when d >= Z the rows of rho in use are the identity: nothing folds, the sums are compared directly over the width d).
// ==========================================================================
#pragma once
#include "plo_brent.hpp"

namespace plo {

// ------------------------------------------------------------------ the verdict lines (reference src/PMchecker.cpp:146-157)
inline std::string pm_shape_text(size_t na, size_t nb, size_t nc) { return std::to_string((long long)na - 1) + 'o' + std::to_string((long long)nb - 1) + 'o' + std::to_string((long long)nc - 1); }
// `mod`: empty, or " mod <f>"; `note` goes behind the field's name (a partial check says so there)
inline std::string pm_success_line(size_t na, size_t nb, size_t nc, const std::string &field, const std::string &mod, const std::string &note = "") {
    return "# \033[1;32mSUCCESS: correct " + pm_shape_text(na, nb, nc) + " Polynomial-Multiplication over " + field + note + " \033[0m" + mod;
}
inline std::string pm_error_line(size_t na, size_t nb, size_t nc, const std::string &field, const std::string &mod) {
    return "# \033[1;31m****** ERROR, not a " + pm_shape_text(na, nb, nc) + " MM algorithm over " + field + "******\033[0m" + mod;
}

// ------------------------------------------------------------------ the polynomial of -P
// A sum of terms [+-][a[/b]][*][X[^e]] with spaces allowed anywhere between tokens; X is the indeterminate (one letter);
// repeated exponents add.  Returns the coefficients, constant term first, trailing zeros cut (empty: the zero polynomial).
// Throws std::invalid_argument with the reason for anything else.
inline std::vector<Rat> parse_poly(const std::string &text, char X = 'X') {
    const QField Qf;
    std::vector<Rat> co;
    size_t p = 0; const size_t n = text.size();
    auto skip = [&] { while (p < n && isspace((unsigned char)text[p])) ++p; };
    auto bad = [&](const std::string &why) { return std::invalid_argument("polynomial \"" + text + "\": " + why + " at position " + std::to_string(p)); };
    auto natural = [&](__int128 &v) {
        skip();
        if (p >= n || !isdigit((unsigned char)text[p])) return false;
        v = 0;
        for (; p < n && isdigit((unsigned char)text[p]); ++p) { if (v > ((__int128)1 << 100)) throw bad("number too long"); v = v * 10 + (text[p] - '0'); }
        return true;
    };
    if (!isalpha((unsigned char)X)) throw std::invalid_argument("the indeterminate must be a letter");
    skip();
    if (p >= n) throw bad("empty");
    for (bool first = true; ; first = false) {
        skip();
        if (p >= n) { if (first) throw bad("empty"); break; }
        int sign = 1;
        if (text[p] == '+' || text[p] == '-') { sign = text[p] == '-' ? -1 : 1; ++p; }
        else if (!first) throw bad("a sign is expected");
        __int128 a = 1, b = 1; bool have_num = natural(a), have_x = false; size_t e = 0;
        if (have_num) {
            skip();
            if (p < n && text[p] == '/') { ++p; if (!natural(b)) throw bad("a denominator is expected"); if (b == 0) throw bad("zero denominator"); }
            skip();
            if (p < n && text[p] == '*') { ++p; skip(); if (p >= n || text[p] != X) throw bad("the indeterminate is expected behind *"); }
        }
        skip();
        if (p < n && text[p] == X) {
            have_x = true; ++p; e = 1; skip();
            if (p < n && text[p] == '^') { ++p; __int128 ee; if (!natural(ee)) throw bad("an exponent is expected"); if (ee > (1 << 24)) throw bad("exponent above 2^24"); e = (size_t)ee; }
        }
        if (!have_num && !have_x) throw bad("a term is expected");
        if (co.size() <= e) co.resize(e + 1, Rat(0));
        co[e] = Qf.add(co[e], Rat::make(sign * a, b));
    }
    while (!co.empty() && co.back().n == 0) co.pop_back();
    return co;
}
// the text of a polynomial, highest term first: X^5+X^4-X^3-X^2-1, -2/3*X^2+1/2
template <class F> std::string poly_text(const F &f, const std::vector<typename F::Elt> &co, char X = 'X') {
    std::ostringstream os; bool any = false;
    for (size_t e = co.size(); e-- > 0;) {
        if (f.isZero(co[e])) continue;
        std::ostringstream cs; f.write(cs, co[e]);
        std::string c = cs.str(); const bool neg = !c.empty() && c[0] == '-';
        if (neg) c.erase(0, 1);
        os << (neg ? "-" : any ? "+" : "");
        if (e == 0) os << c; else { if (c != "1") os << c << '*'; os << X; if (e > 1) os << '^' << e; }
        any = true;
    }
    return any ? os.str() : "0";
}
// f over the integers, primitive, the sign of its leading coefficient kept: what the certificate bounds and what the device
// gets over Q (f and a rational multiple of f have the same remainders up to that factor, and the same zero ones)
inline std::vector<__int128> primitive_poly(const std::vector<Rat> &co) {
    __int128 l = 1, g = 0;
    for (const Rat &c : co) l = Rat::mulck(l / Rat::gcd(l, c.d), c.d);
    std::vector<__int128> out;
    for (const Rat &c : co) { out.push_back(Rat::mulck(c.n, l / c.d)); g = Rat::gcd(g, out.back()); }
    if (g > 1) for (auto &v : out) v /= g;
    return out;
}

// ------------------------------------------------------------------ what one check is about
template <class E> struct PolyMulSpec {
    size_t na = 0, nb = 0, nc = 0, Z = 0, w = 0, d = 0;   // d: the degree of f, 0 without one
    bool fold = false;                                    // d < Z: the table is in use
    std::vector<std::vector<E>> rho;                      // fold: Z rows of d coefficients, rho[z][c] that of X^c in X^z mod f
};
// fco: the coefficients of f over the field, constant term first, the last one a unit; empty: no polynomial
template <class F> PolyMulSpec<typename F::Elt> polymul_spec(const F &f, size_t na, size_t nb, size_t nc, const std::vector<typename F::Elt> &fco) {
    using E = typename F::Elt;
    PolyMulSpec<E> s; s.na = na; s.nb = nb; s.nc = nc;
    s.Z = std::max(nc, na + nb ? na + nb - 1 : 0);
    s.d = fco.empty() ? 0 : fco.size() - 1;
    s.w = fco.empty() ? s.Z : s.d;
    s.fold = !fco.empty() && s.d < s.Z;
    if (!s.fold) return s;
    const E il = f.inv(fco[s.d]);
    std::vector<E> low(s.d);                              // f made monic: X^d = -low
    for (size_t c = 0; c < s.d; ++c) low[c] = f.mul(fco[c], il);
    s.rho.assign(s.Z, std::vector<E>(s.d, f.zero()));
    for (size_t z = 0; z < s.Z && z < s.d; ++z) s.rho[z][z] = f.one();
    for (size_t z = s.d; z < s.Z; ++z) {
        const E top = s.rho[z - 1][s.d - 1];
        for (size_t c = 0; c < s.d; ++c) s.rho[z][c] = f.add(c ? s.rho[z - 1][c - 1] : f.zero(), f.neg(f.mul(top, low[c])));
    }
    return s;
}

// the w values found for the pair (i, j) from its sums S[0 .. nc), and the w expected ones
template <class F> void polymul_pair(const F &f, const PolyMulSpec<typename F::Elt> &s, const typename F::Elt *S, size_t i, size_t j,
                                     std::vector<typename F::Elt> &got, std::vector<typename F::Elt> &want) {
    got.assign(s.w, f.zero()); want.assign(s.w, f.zero());
    if (!s.fold) {
        for (size_t c = 0; c < s.nc && c < s.w; ++c) got[c] = S[c];
        if (i + j < s.w) want[i + j] = f.one();
        return;
    }
    for (size_t z = 0; z < s.nc; ++z) {
        if (f.isZero(S[z])) continue;
        if (z < s.d) got[z] = f.add(got[z], S[z]);
        else for (size_t c = 0; c < s.d; ++c) got[c] = f.add(got[c], f.mul(S[z], s.rho[z][c]));
    }
    want = s.rho[i + j];
}

// ------------------------------------------------------------------ the host loop
// violated equations among the pairs [pair0, pair1), the smallest one, the value found there and the one expected.  LT is the
// transpose of L (its rows are the columns i), PT the transpose of P.  Unless count_all, slabs behind the first failing one
// are not computed (the count is then that of the slabs that were); the smallest violated equation is the same either way.
template <class E> struct PolyMulFound { uint64_t violated = 0, first = ~0ull; E value{}, expected{}; };
template <class F> PolyMulFound<typename F::Elt> polymul_host(const F &f, const PolyMulSpec<typename F::Elt> &s, const SparseMat<typename F::Elt> &LT, const SparseMat<typename F::Elt> &R,
                                                              const SparseMat<typename F::Elt> &PT, uint64_t pair0, uint64_t pair1, bool count_all) {
    using E = typename F::Elt;
    const size_t nb = s.nb, nc = s.nc;
    PolyMulFound<E> all;
    if (pair0 >= pair1) return all;
    const long long i0 = (long long)(pair0 / nb), i1 = (long long)((pair1 - 1) / nb);
    std::atomic<long long> stop(i1 + 1);
    std::string err;
    #pragma omp parallel
    {
        std::vector<E> S(nb * nc), got, want;
        PolyMulFound<E> mine;
        #pragma omp for schedule(dynamic, 1)
        for (long long i = i0; i <= i1; ++i) {
            if (!count_all && i > stop.load()) continue;
            const size_t jlo = i == i0 ? (size_t)(pair0 % nb) : 0, jhi = i == i1 ? (size_t)((pair1 - 1) % nb) + 1 : nb;
            try {
                std::fill(S.begin() + jlo * nc, S.begin() + jhi * nc, f.zero());
                for (const auto &l : LT.rows[(size_t)i]) {
                    const size_t t = l.first;
                    for (const auto &r : R.rows[t]) {
                        if (r.first < jlo || r.first >= jhi) continue;
                        const E lr = f.mul(l.second, r.second);
                        E *row = S.data() + r.first * nc;
                        for (const auto &p : PT.rows[t]) row[p.first] = f.add(row[p.first], f.mul(lr, p.second));
                    }
                }
                bool bad = false;
                for (size_t j = jlo; j < jhi; ++j) {
                    polymul_pair(f, s, S.data() + j * nc, (size_t)i, j, got, want);
                    for (size_t c = 0; c < s.w; ++c) {
                        if (got[c] == want[c]) continue;
                        const uint64_t e = ((uint64_t)i * nb + j) * s.w + c;
                        ++mine.violated; bad = true;
                        if (e < mine.first) { mine.first = e; mine.value = got[c]; mine.expected = want[c]; }
                    }
                }
                if (bad) { long long cur = stop.load(); while (i < cur && !stop.compare_exchange_weak(cur, i)) { } }
            } catch (const std::exception &ex) {
                #pragma omp critical
                err = ex.what();
            }
        }
        #pragma omp critical
        {
            all.violated += mine.violated;
            if (mine.first < all.first) { all.first = mine.first; all.value = mine.value; all.expected = mine.expected; }
        }
    }
    if (!err.empty()) throw std::runtime_error(err);                                       // Q: an overflow is an error
    return all;
}

// ------------------------------------------------------------------ the certificate over Q
// Without f the equations are trilinear sums as the Brent equations are, and beta is brent_certificate's: D D_ij, D the product
// of the three denominator lcms, has integer coefficients below 2^beta0 in absolute value.  With f = the primitive integer
// polynomial fz of degree d < Z and leading coefficient l: modulo a prime that divides neither a denominator nor l, the folded
// equations of a pair vanish exactly when the pseudo-remainder of D D_ij by fz does (it is l^(Z-d) times the remainder, and l
// and D are units).  The pseudo-remainder takes Z - d steps A <- l A - a_k X^(k-d) fz, k = Z - 1 .. d, each of which multiplies
// the largest coefficient by at most |l| + |fz|_inf: beta = beta0 + (Z - d) bits(|l| + |fz|_inf).  Nothing is added when d >= Z.
// j = ceil(beta / 30) primes above 2^30: 2147483629, then each largest prime below the last, the excluded ones passed over.
inline BrentCert polymul_certificate(const QMat &L, const QMat &R, const QMat &P, const std::vector<__int128> &fz) {
    BrentCert c;
    c.beta = brent_certificate(L, R, P).beta;
    std::set<__int128> avoid;
    for (const QMat *M : {&L, &R, &P}) for (const auto &row : M->rows) for (const auto &e : row) if (e.second.d > 1) avoid.insert(e.second.d);
    if (!fz.empty()) {
        const size_t d = fz.size() - 1, Z = std::max(P.rowdim(), L.coldim() + R.coldim() ? L.coldim() + R.coldim() - 1 : 0);
        __int128 norm = 0;
        for (const __int128 v : fz) norm = std::max(norm, v < 0 ? -v : v);
        const __int128 lead = fz[d] < 0 ? -fz[d] : fz[d];
        if (d < Z) {
            const uint64_t more = (uint64_t)(Z - d) * brent_bits(Rat::addck(lead, norm));
            if (more > (1u << 24)) throw std::runtime_error("the certificate would take more than 2^24 bits");
            c.beta += (unsigned)more;
        }
        avoid.insert(lead);
    }
    c.j = (c.beta + 29u) / 30u;
    for (uint32_t p = 2147483629u; c.primes.size() < c.j; --p) {
        if (p <= (1u << 30)) throw std::runtime_error("no primes above 2^30 left for the certificate");
        if (!is_prime(p)) continue;
        bool divides = false;
        for (const __int128 v : avoid) if (v % p == 0) { divides = true; break; }
        if (!divides) c.primes.push_back(p);
    }
    return c;
}

} // namespace plo
