// ==========================================================================
// plo_brent.hpp -- the Brent equations of a triple on the host (bin/MMchecker --gpu 0), the certificate that
// turns checks modulo primes into a proof over Q, and the wording of the verdict lines that bin/MMchecker and bin/orbiter print.
//
// L (r x mk), R (r x kn), P (mn x r); with x = a k + b, y = b' n + c, z = a' n + c', equation e = (x kn + y) mn + z asks
//     S[x][y][z] = sum_t L[t][x] R[t][y] P[z][t]  ==  [a = a'][b = b'][c = c'].
// A pair is x kn + y.  The loop below accumulates one x slab (kn x mn) at a time, never the dense mk.kn.mn array.
// ==========================================================================
#pragma once
#include "plo_host.hpp"
#include <atomic>
#include <cmath>
#include <set>

namespace plo {

// ------------------------------------------------------------------ the verdict lines (reference include/plinopt_library.inl:529-536)
inline std::string mm_shape_text(size_t m, size_t k, size_t n) { return std::to_string(m) + 'x' + std::to_string(k) + 'x' + std::to_string(n); }
// `note` goes behind the field's name (a partial check says so there)
inline std::string mm_success_line(size_t m, size_t k, size_t n, size_t nnz, size_t nno, const std::string &field, const std::string &note = "") {
    return "# \033[1;32mSUCCESS: correct " + mm_shape_text(m, k, n) + " (" + std::to_string(nnz) + ',' + std::to_string(nno) + ") Matrix-Multiplication over " + field + note + " \033[0m";
}
inline std::string mm_error_line(size_t m, size_t k, size_t n, const std::string &field, const std::string &why = "") {
    return "# \033[1;31m****** ERROR, not a " + mm_shape_text(m, k, n) + " MM algorithm over " + field + (why.empty() ? "" : " (check failed: " + why + ")") + "******\033[0m";
}

// (m, k, n) of the reference's LRP2MM (include/plinopt_library.h:178-181): n = floor(sqrt(R.coldim P.rowdim / L.coldim)), the
// quotient an integer division; false when the outer dimensions then disagree (MMchecker's test, plinopt_library.inl:487)
inline bool brent_shape(size_t lcols, size_t rcols, size_t prows, size_t &m, size_t &k, size_t &n) {
    m = k = n = 0;
    if (lcols == 0) return false;
    n = (size_t)std::sqrt((double)(rcols * prows / lcols));
    if (n == 0) return false;
    m = prows / n; k = rcols / n;
    return lcols == m * k && rcols == k * n && prows == m * n;
}

// deterministic Miller-Rabin below 2^64 (the first twelve primes as bases)
inline bool is_prime(uint64_t n) {
    if (n < 2) return false;
    static const uint64_t B[12] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (uint64_t q : B) { if (n == q) return true; if (n % q == 0) return false; }
    uint64_t d = n - 1; int s = 0; while (!(d & 1)) { d >>= 1; ++s; }
    auto mul = [&](uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % n); };
    for (uint64_t a : B) {
        uint64_t x = 1, b = a % n;
        for (uint64_t e = d; e; e >>= 1) { if (e & 1) x = mul(x, b); b = mul(b, b); }
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int i = 1; i < s && comp; ++i) { x = mul(x, x); if (x == n - 1) comp = false; }
        if (comp) return false;
    }
    return true;
}

// ------------------------------------------------------------------ the host loop
// violated equations among the pairs [pair0, pair1), the smallest one and the sum found there.  LT is the transpose of L (its
// rows are the columns x), PT the transpose of P.  Unless count_all, slabs behind the first failing one are not computed (the
// count is then that of the slabs that were); the smallest violated equation is the same either way.
template <class E> struct BrentFound { uint64_t violated = 0, first = ~0ull; E value{}; };
template <class F> BrentFound<typename F::Elt> brent_host(const F &f, const SparseMat<typename F::Elt> &LT, const SparseMat<typename F::Elt> &R, const SparseMat<typename F::Elt> &PT,
                                                          size_t k, size_t n, uint64_t pair0, uint64_t pair1, bool count_all) {
    using E = typename F::Elt;
    const size_t kn = R.coldim(), mn = PT.coldim();
    BrentFound<E> all;
    if (pair0 >= pair1) return all;
    const long long x0 = (long long)(pair0 / kn), x1 = (long long)((pair1 - 1) / kn);
    std::atomic<long long> stop(x1 + 1);
    std::string err;
    #pragma omp parallel
    {
        std::vector<E> S(kn * mn);
        BrentFound<E> mine;
        #pragma omp for schedule(dynamic, 1)
        for (long long x = x0; x <= x1; ++x) {
            if (!count_all && x > stop.load()) continue;
            const size_t ylo = x == x0 ? (size_t)(pair0 % kn) : 0, yhi = x == x1 ? (size_t)((pair1 - 1) % kn) + 1 : kn;
            try {
                std::fill(S.begin() + ylo * mn, S.begin() + yhi * mn, f.zero());
                for (const auto &l : LT.rows[(size_t)x]) {
                    const size_t t = l.first;
                    for (const auto &r : R.rows[t]) {
                        if (r.first < ylo || r.first >= yhi) continue;
                        const E lr = f.mul(l.second, r.second);
                        E *row = S.data() + r.first * mn;
                        for (const auto &p : PT.rows[t]) row[p.first] = f.add(row[p.first], f.mul(lr, p.second));
                    }
                }
                const size_t a = (size_t)x / k, b = (size_t)x % k;
                bool bad = false;
                for (size_t y = ylo; y < yhi; ++y) {
                    const size_t b2 = y / n, c = y % n;
                    for (size_t z = 0; z < mn; ++z) {
                        const E &s = S[y * mn + z];
                        if ((b == b2 && z == a * n + c) ? f.isOne(s) : f.isZero(s)) continue;
                        const uint64_t e = ((uint64_t)x * kn + y) * mn + z;
                        ++mine.violated; bad = true;
                        if (e < mine.first) { mine.first = e; mine.value = s; }
                    }
                }
                if (bad) { long long cur = stop.load(); while (x < cur && !stop.compare_exchange_weak(cur, x)) { } }
            } catch (const std::exception &ex) {
                #pragma omp critical
                err = ex.what();
            }
        }
        #pragma omp critical
        {
            all.violated += mine.violated;
            if (mine.first < all.first) { all.first = mine.first; all.value = mine.value; }
        }
    }
    if (!err.empty()) throw std::runtime_error(err);                                       // Q: an overflow is an error
    return all;
}

// one sum S[x][y][z] over F: the intersection of two columns
template <class F> typename F::Elt brent_sum(const F &f, const SparseMat<typename F::Elt> &LT, const SparseMat<typename F::Elt> &R, const SparseMat<typename F::Elt> &PT, size_t x, size_t y, size_t z) {
    using E = typename F::Elt;
    E s = f.zero();
    auto at = [](const typename SparseMat<E>::Row &row, size_t c) -> const E * {
        auto it = std::lower_bound(row.begin(), row.end(), c, [](const std::pair<size_t, E> &e, size_t cc) { return e.first < cc; });
        return it != row.end() && it->first == c ? &it->second : nullptr;
    };
    for (const auto &l : LT.rows[x]) {
        const E *r = at(R.rows[l.first], y), *p = at(PT.rows[l.first], z);
        if (r && p) s = f.add(s, f.mul(f.mul(l.second, *r), *p));
    }
    return s;
}

// ------------------------------------------------------------------ the certificate over Q
// beta = bits(r) + N_L + N_R + N_P + D_L + D_R + D_P + 2, N_X the longest numerator of X and D_X the bits of its distinct
// denominators above 1 summed: D (S - delta), D the product of the three denominator lcms, is an integer below 2^beta in
// absolute value, so it is zero as soon as it vanishes modulo j = ceil(beta / 30) primes above 2^30 that divide no denominator.
// The primes: 2147483629, then each largest prime below the last, those that divide a denominator passed over.
struct BrentCert { unsigned beta = 0, j = 0; std::vector<uint32_t> primes; };
inline unsigned brent_bits(__int128 v) { if (v < 0) v = -v; unsigned b = 0; while (v) { ++b; v >>= 1; } return b; }
inline BrentCert brent_certificate(const QMat &L, const QMat &R, const QMat &P) {
    BrentCert c;
    std::set<__int128> alld;
    c.beta = brent_bits((__int128)L.rowdim()) + 2u;
    for (const QMat *M : {&L, &R, &P}) {
        unsigned N = 0; std::set<__int128> dens;
        for (const auto &row : M->rows) for (const auto &e : row) { N = std::max(N, brent_bits(e.second.n)); if (e.second.d > 1) dens.insert(e.second.d); }
        c.beta += N;
        for (const __int128 d : dens) { c.beta += brent_bits(d); alld.insert(d); }
    }
    c.j = (c.beta + 29u) / 30u;
    for (uint32_t p = 2147483629u; c.primes.size() < c.j; --p) {
        if (p <= (1u << 30)) throw std::runtime_error("no primes above 2^30 left for the certificate");
        if (!is_prime(p)) continue;
        bool divides = false;
        for (const __int128 d : alld) if (d % p == 0) { divides = true; break; }
        if (!divides) c.primes.push_back(p);
    }
    return c;
}

} // namespace plo
