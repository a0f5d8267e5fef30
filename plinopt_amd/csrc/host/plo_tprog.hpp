// ==========================================================================
// plo_tprog.hpp -- what an in-place trilinear program of bin/trilplacer computes, on the host (bin/TPchecker --gpu 0; DESIGN.md
// 2.14): the parser of the program text, the host loop over every equation, and the certificate that turns checks modulo primes
// into a proof over Q.  This is the definition the kernel of plo_tprog.hip is held to.
//
// L (r x na), R (r x nb), P (nc0 x r); the state is a[0..na), b[0..nb), c[0..nc), nc = nc0, or nc0 + 1 with -e.  The lines are
//   ADD   xN:=xN+-yM[*v|/v];         x, y of one family          SCA   xN:=[-]xN[*v|/v];
//   AXPY  cK:=cK +- aI * bJ;         with -e instead             cK:=cK +- (aI * bJ)*low;  cK:=cK +- (aI * bJ)*hig;
// so the final state is a' = A a, b' = B b, c' = C c + S(a, b) with S bilinear (with -e: S_low and S_hig, the coefficients of the
// symbols low and hig).  The width is w = nc, or 2 nc with -e (the low components, then the hig ones); a pair is i nb + j:
//   e = (i nb + j) w + z            S[i][j][z] == T[i][j][z] = sum_t L[t][i] R[t][j] P[z][t]
//                                   -e: S_low[z] == T[z] (z < nc0), 0 at nc0; S_hig[z] == T[z - 1] (z >= 1), 0 at 0
//                                   -m: T is the matrix-multiplication tensor of (m, k, n) = LRP2MM(L, R, P)
//   E0 + x na + i, E0 = na nb w     A[x][i] == [x == i];   then nb^2 numbers for B, then nc^2 for C.
// ==========================================================================
#pragma once
#include "plo_brent.hpp"
#include <cfloat>

namespace plo {

enum : uint8_t { TP_ADD = 0, TP_SCA = 1, TP_AXPY = 2 };
// one line: family 0 a, 1 b, 2 c.  ADD: x[dst] += coef x[src]; SCA: x[dst] *= coef; AXPY: c[dst] += coef a[src] b[src2], coef
// +-1, part 0 plain, 1 low, 2 hig
struct TpRec { uint8_t fam = 0, op = 0, part = 0; uint32_t dst = 0, src = 0, src2 = 0; Rat coef; size_t line = 0; };
struct TpProgram { std::vector<TpRec> recs; size_t nadd = 0, nsca = 0, naxpy = 0; };   // the counts as bin/trilplacer prints them
struct TpRefused : std::runtime_error { using std::runtime_error::runtime_error; };

// ------------------------------------------------------------------ the parser
// Everything behind the first ';' of a line is ignored; lines that start with '#' and lines without ':=' are ignored; spaces
// count nowhere.  Anything outside the grammar above throws TpRefused with the line number and the reason.
inline TpProgram parse_tprog(std::istream &in, size_t na, size_t nb, size_t nc, bool expanded) {
    TpProgram pg; std::string raw; size_t ln = 0;
    const size_t dims[3] = {na, nb, nc};
    const QField Qf;
    while (std::getline(in, raw)) {
        ++ln;
        const size_t b = raw.find_first_not_of(" \t\r");
        if (b == std::string::npos || raw[b] == '#') continue;
        const size_t semi = raw.find(';');
        std::string s;
        for (size_t k = b; k < raw.size() && k != semi; ++k) if (!isspace((unsigned char)raw[k])) s += raw[k];
        if (s.find(":=") == std::string::npos) continue;
        auto bad = [&](const std::string &why) { return TpRefused("line " + std::to_string(ln) + ": " + why + ": " + s); };
        if (semi == std::string::npos) throw bad("no ';'");
        size_t p = 0;
        auto number = [&](__int128 &v) {
            if (p >= s.size() || !isdigit((unsigned char)s[p])) return false;
            v = 0;
            for (; p < s.size() && isdigit((unsigned char)s[p]); ++p) { if (v > ((__int128)1 << 120)) throw bad("number too long"); v = v * 10 + (s[p] - '0'); }
            return true;
        };
        auto var = [&](int &fam, uint32_t &idx) {                 // a, b or c and an index; false when there is none
            if (p + 1 >= s.size() || s[p] < 'a' || s[p] > 'c' || !isdigit((unsigned char)s[p + 1])) return false;
            fam = s[p++] - 'a';
            __int128 v = 0; number(v);
            if (v >= (__int128)dims[fam]) throw bad("index out of range (" + std::string(1, (char)('a' + fam)) + " has " + std::to_string(dims[fam]) + " entries)");
            idx = (uint32_t)v;
            return true;
        };
        auto factor = [&](Rat &c) {                               // [*v | /v], v = [-]n[/d]; true when one is written
            c = Rat(1);
            if (p >= s.size() || (s[p] != '*' && s[p] != '/')) return false;
            const char o = s[p++];
            bool neg = false;
            if (p < s.size() && s[p] == '-') { neg = true; ++p; }
            __int128 n = 0, d = 1;
            if (!number(n)) throw bad("a number is expected behind " + std::string(1, o));
            if (p < s.size() && s[p] == '/') { ++p; if (!number(d)) throw bad("a denominator is expected"); if (d == 0) throw bad("division by zero"); }
            if (o == '/') { if (n == 0) throw bad("division by zero"); std::swap(n, d); }
            c = Rat::make(neg ? -n : n, d);
            return true;
        };
        TpRec r; r.line = ln;
        int df = 0, f1 = 0; uint32_t i1 = 0;
        if (!var(df, r.dst)) throw bad("the destination is no entry of a, b or c");
        if (s.compare(p, 2, ":=") != 0) throw bad("':=' is expected behind the destination");
        p += 2;
        r.fam = (uint8_t)df;
        bool neg = false;
        if (p < s.size() && s[p] == '-') { neg = true; ++p; }
        if (!var(f1, i1)) throw bad("a variable is expected");
        if (f1 != df || i1 != r.dst) throw bad("the destination is not the first operand");
        if (neg || p == s.size() || s[p] == '*' || s[p] == '/') {                          // SCA
            if (!neg && p == s.size()) throw bad("no operation");
            Rat c; factor(c);
            if (p != s.size()) throw bad("unexpected text behind a scaling");
            r.op = TP_SCA; r.coef = neg ? Qf.neg(c) : c; ++pg.nsca;
        } else if (s[p] == '+' || s[p] == '-') {
            const bool minus = s[p++] == '-';
            int f2 = 0, f3 = 0;
            if (p < s.size() && s[p] == '(') {                                             // -e: (aI * bJ)*low|hig
                ++p;
                if (!var(f2, r.src) || p >= s.size() || s[p++] != '*' || !var(f3, r.src2) || s.compare(p, 2, ")*") != 0) throw bad("(aI * bJ)*low or (aI * bJ)*hig is expected");
                const std::string half = s.substr(p + 2);
                if (half != "low" && half != "hig") throw bad("(aI * bJ)*low or (aI * bJ)*hig is expected");
                if (!expanded) throw bad("*" + half + " without -e");
                if (df != 2 || f2 != 0 || f3 != 1) throw bad("a line that mixes families outside an AXPY cK:=cK +- aI * bJ");
                r.op = TP_AXPY; r.part = half == "low" ? 1 : 2; r.coef = Rat(minus ? -1 : 1);
                if (r.part == 1) ++pg.naxpy;
            } else {
                if (!var(f2, r.src)) throw bad("a variable is expected behind the sign");
                if (p + 1 < s.size() && s[p] == '*' && isalpha((unsigned char)s[p + 1])) {  // AXPY
                    ++p;
                    if (!var(f3, r.src2) || p != s.size()) throw bad("aI * bJ is expected");
                    if (df != 2 || f2 != 0 || f3 != 1) throw bad("a line that mixes families outside an AXPY cK:=cK +- aI * bJ");
                    if (expanded) throw bad("an AXPY without *low or *hig under -e");
                    r.op = TP_AXPY; r.coef = Rat(minus ? -1 : 1); ++pg.naxpy;
                } else {                                                                   // ADD
                    if (f2 != df) throw bad("a line that mixes families outside an AXPY cK:=cK +- aI * bJ");
                    Rat c; const bool written = factor(c);
                    if (p != s.size()) throw bad("unexpected text behind an addition");
                    r.op = TP_ADD; r.coef = minus ? Qf.neg(c) : c; ++pg.nadd; pg.nsca += written ? 1 : 0;
                }
            }
        } else throw bad("an operator is expected behind the first operand");
        pg.recs.push_back(r);
    }
    return pg;
}

// ------------------------------------------------------------------ what one check is about
struct TpSpec {
    size_t na = 0, nb = 0, nc0 = 0, nc = 0, w = 0;        // nc = nc0 (+ 1 with -e); w = nc (2 nc with -e)
    bool expanded = false, matmul = false; size_t m = 0, k = 0, n = 0;
    uint64_t npairs() const { return (uint64_t)na * nb; }
    uint64_t E0() const { return npairs() * w; }
    uint64_t nequations() const { return E0() + (uint64_t)na * na + (uint64_t)nb * nb + (uint64_t)nc * nc; }
    size_t slot(const TpRec &r) const { return r.part == 2 ? nc + r.dst : r.dst; }
};
inline TpSpec tprog_spec(size_t na, size_t nb, size_t nc0, bool expanded, bool matmul) {
    TpSpec s; s.na = na; s.nb = nb; s.nc0 = nc0; s.expanded = expanded; s.matmul = matmul;
    s.nc = nc0 + (expanded ? 1 : 0); s.w = expanded ? 2 * s.nc : s.nc;
    if (matmul && !brent_shape(na, nb, nc0, s.m, s.k, s.n)) throw TpRefused("-m: " + std::to_string(na) + ", " + std::to_string(nb) + " and " + std::to_string(nc0) + " are not m k, k n and m n");
    return s;
}
// block 0 bilinear (x = i, y = j, z the slot), 1 A, 2 B, 3 C (x the row, y the column)
struct TpWhere { int block = 0; uint64_t x = 0, y = 0, z = 0; };
inline TpWhere tprog_where(const TpSpec &s, uint64_t e) {
    TpWhere q;
    if (e < s.E0()) { q.z = e % s.w; const uint64_t pr = e / s.w; q.x = pr / s.nb; q.y = pr % s.nb; return q; }
    e -= s.E0();
    for (const size_t n : {s.na, s.nb, s.nc}) { ++q.block; if (e < (uint64_t)n * n) { q.x = e / n; q.y = e % n; return q; } e -= (uint64_t)n * n; }
    throw std::out_of_range("equation number beyond the last");
}
inline std::string tprog_where_text(const TpSpec &s, uint64_t e) {
    const TpWhere q = tprog_where(s, e);
    std::ostringstream os;
    if (q.block == 0) {
        os << "bilinear (i,j,z) = (" << q.x << ',' << q.y << ',';
        if (!s.expanded) os << q.z << ')'; else os << (q.z < s.nc ? q.z : q.z - s.nc) << ") " << (q.z < s.nc ? "low" : "hig");
    } else os << "restoration of " << "abc"[q.block - 1] << ": " << "ABC"[q.block - 1] << '[' << q.x << "][" << q.y << ']';
    return os.str();
}

// the records' coefficients over a field
template <class F> std::vector<typename F::Elt> tprog_coefs(const F &f, const TpProgram &pg) {
    std::vector<typename F::Elt> out;
    for (const TpRec &r : pg.recs) out.push_back(f.fromRat(r.coef));
    return out;
}

// One family on its unit inputs: fin[x n + i] is entry x of the final state for the input e_i, and at[s] holds, for the AXPY
// number s, its operand of this family for every unit input (fam 2: the AXPYs are passed over, at stays empty).
template <class E> struct TpLinear { std::vector<E> fin; std::vector<std::vector<E>> at; };
template <class F> TpLinear<typename F::Elt> tprog_linear(const F &f, const TpProgram &pg, const std::vector<typename F::Elt> &co, int fam, size_t n) {
    using E = typename F::Elt;
    TpLinear<E> out; out.fin.assign(n * n, f.zero());
    for (size_t i = 0; i < n; ++i) out.fin[i * n + i] = f.one();
    for (size_t k = 0; k < pg.recs.size(); ++k) {
        const TpRec &r = pg.recs[k];
        if (r.op == TP_AXPY) {
            if (fam == 2) continue;
            const E *row = out.fin.data() + (size_t)(fam == 0 ? r.src : r.src2) * n;
            out.at.emplace_back(row, row + n);
            continue;
        }
        if (r.fam != fam) continue;
        E *dst = out.fin.data() + (size_t)r.dst * n;
        if (r.op == TP_SCA) for (size_t i = 0; i < n; ++i) dst[i] = f.mul(dst[i], co[k]);
        else { const E *src = out.fin.data() + (size_t)r.src * n; for (size_t i = 0; i < n; ++i) dst[i] = f.add(dst[i], f.mul(co[k], src[i])); }
    }
    return out;
}

// ------------------------------------------------------------------ the host loop
// Violated equations among the pairs [pair0, pair1) and, when pair0 == 0, the three restoration blocks; the smallest one, the
// value found there and the one expected.  LT is the transpose of L, PT that of P (unused with -m).  Unless count_all, rows i
// behind the first failing one and the blocks behind a failing bilinear part are not computed; the smallest violated equation
// is the same either way.  probe: an equation whose two values are wanted whether it is violated or not (~0: none).
template <class E> struct TpFound { uint64_t violated = 0, first = ~0ull; E value{}, expected{}; E probe_value{}, probe_expected{}; };
template <class F> TpFound<typename F::Elt> tprog_host(const F &f, const TpSpec &s, const TpProgram &pg, const SparseMat<typename F::Elt> &LT, const SparseMat<typename F::Elt> &R,
                                                        const SparseMat<typename F::Elt> &PT, uint64_t pair0, uint64_t pair1, bool count_all, uint64_t probe = ~0ull) {
    using E = typename F::Elt;
    const size_t na = s.na, nb = s.nb, nc = s.nc, nc0 = s.nc0, w = s.w;
    TpFound<E> all;
    if (pair0 >= pair1) return all;
    const std::vector<E> co = tprog_coefs(f, pg);
    const TpLinear<E> la = tprog_linear(f, pg, co, 0, na), lb = tprog_linear(f, pg, co, 1, nb), lc = tprog_linear(f, pg, co, 2, nc);
    const long long i0 = (long long)(pair0 / nb), i1 = (long long)((pair1 - 1) / nb);
    std::atomic<long long> stop(i1 + 1);
    std::string err;
    #pragma omp parallel
    {
        std::vector<E> st(nb * w), T(nb * nc0);
        TpFound<E> mine;
        #pragma omp for schedule(dynamic, 1)
        for (long long i = i0; i <= i1; ++i) {
            if (!count_all && i > stop.load()) continue;
            const size_t jlo = i == i0 ? (size_t)(pair0 % nb) : 0, jhi = i == i1 ? (size_t)((pair1 - 1) % nb) + 1 : nb;
            try {
                std::fill(st.begin() + jlo * w, st.begin() + jhi * w, f.zero());
                size_t ax = 0;
                for (size_t k = 0; k < pg.recs.size(); ++k) {
                    const TpRec &r = pg.recs[k];
                    if (r.op == TP_AXPY) {
                        const E al = f.mul(co[k], la.at[ax][(size_t)i]);
                        const std::vector<E> &be = lb.at[ax++];
                        if (f.isZero(al)) continue;
                        const size_t z = s.slot(r);
                        for (size_t j = jlo; j < jhi; ++j) st[j * w + z] = f.add(st[j * w + z], f.mul(al, be[j]));
                    } else if (r.fam == 2) {
                        for (size_t h = 0; h < w; h += nc) {                               // both halves with -e
                            const size_t d = h + r.dst, sr = h + r.src;
                            if (r.op == TP_SCA) for (size_t j = jlo; j < jhi; ++j) st[j * w + d] = f.mul(st[j * w + d], co[k]);
                            else for (size_t j = jlo; j < jhi; ++j) st[j * w + d] = f.add(st[j * w + d], f.mul(co[k], st[j * w + sr]));
                        }
                    }
                }
                std::fill(T.begin() + jlo * nc0, T.begin() + jhi * nc0, f.zero());
                if (s.matmul) {
                    const size_t a = (size_t)i / s.k, b = (size_t)i % s.k;
                    for (size_t c = 0; c < s.n; ++c) { const size_t j = b * s.n + c; if (j >= jlo && j < jhi) T[j * nc0 + a * s.n + c] = f.one(); }
                } else for (const auto &l : LT.rows[(size_t)i]) {
                    const size_t t = l.first;
                    for (const auto &r : R.rows[t]) {
                        if (r.first < jlo || r.first >= jhi) continue;
                        const E lr = f.mul(l.second, r.second);
                        E *row = T.data() + r.first * nc0;
                        for (const auto &p : PT.rows[t]) row[p.first] = f.add(row[p.first], f.mul(lr, p.second));
                    }
                }
                bool bad = false;
                for (size_t j = jlo; j < jhi; ++j) for (size_t z = 0; z < w; ++z) {
                    const size_t zz = z < nc ? z : z - nc;                                 // the entry of c; hig slots look one entry down
                    E want = f.zero();
                    if (z < nc) { if (zz < nc0) want = T[j * nc0 + zz]; } else if (zz >= 1) want = T[j * nc0 + zz - 1];
                    const E &got = st[j * w + z];
                    const uint64_t e = ((uint64_t)i * nb + j) * w + z;
                    if (e == probe) {
                        #pragma omp critical(tprog_probe)
                        { all.probe_value = got; all.probe_expected = want; }
                    }
                    if (got == want) continue;
                    ++mine.violated; bad = true;
                    if (e < mine.first) { mine.first = e; mine.value = got; mine.expected = want; }
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
    if (pair0 == 0 && (count_all || all.violated == 0 || (probe != ~0ull && probe >= s.E0()))) {
        uint64_t e = s.E0();
        const std::vector<E> *fin[3] = {&la.fin, &lb.fin, &lc.fin};
        const size_t dim[3] = {na, nb, nc};
        for (int b = 0; b < 3; ++b) for (size_t x = 0; x < dim[b]; ++x) for (size_t i = 0; i < dim[b]; ++i, ++e) {
            const E &got = (*fin[b])[x * dim[b] + i]; const E want = x == i ? f.one() : f.zero();
            if (e == probe) { all.probe_value = got; all.probe_expected = want; }
            if (got == want || (!count_all && all.first < s.E0())) continue;
            ++all.violated;
            if (e < all.first) { all.first = e; all.value = got; all.expected = want; }
        }
    }
    return all;
}

// ------------------------------------------------------------------ the certificate over Q
// For unit inputs every final value times Delta, the product of the denominators of all coefficients of all lines, is an integer
// (DESIGN.md 2.14).  mu bounds the magnitudes: 1 at the start, ADD mu(x) += |v| mu(y), SCA mu(x) *= |v|, AXPY mu(c) += mu(a) mu(b).
// With delta_T the denominator of T by brent_certificate's rule (the distinct denominators of L, R and P multiplied) and
// |T| delta_T < 2^bT, bT = brent's beta - 2:  |found - expected| Delta delta_T < 2^beta with
//     beta = max(bits(mu) + bits(delta_T), bT) + bits(Delta) + 1,
// every term rounded upwards: mu in long doubles pushed to the next one after each operation, the bits of a product taken as the
// sum of the bits of its factors.  j = ceil(beta / 30).  A mu beyond the long doubles gives beta = 0: no certificate, the caller
// proves over Q on the host.
inline BrentCert tprog_certificate(const TpSpec &s, const TpProgram &pg, const QMat &L, const QMat &R, const QMat &P, unsigned max_primes = 64) {
    BrentCert c;
    auto up = [](long double x) { return nextafterl(nextafterl(x, INFINITY), INFINITY); };
    auto mag = [&](const Rat &v) { const __int128 n = v.n < 0 ? -v.n : v.n; return up(up((long double)n) / ((long double)v.d * (1.0L - 0x1p-60L))); };
    std::vector<long double> mu[3] = {std::vector<long double>(s.na, 1.0L), std::vector<long double>(s.nb, 1.0L), std::vector<long double>(s.nc, 1.0L)};
    std::set<__int128> avoid;
    uint64_t dbits = 0;
    for (const TpRec &r : pg.recs) {
        if (r.coef.d > 1) { dbits += brent_bits(r.coef.d); avoid.insert(r.coef.d); }
        if (r.op == TP_AXPY) mu[2][r.dst] = up(mu[2][r.dst] + up(mu[0][r.src] * mu[1][r.src2]));
        else if (r.op == TP_SCA) mu[r.fam][r.dst] = up(mu[r.fam][r.dst] * mag(r.coef));
        else mu[r.fam][r.dst] = up(mu[r.fam][r.dst] + up(mag(r.coef) * mu[r.fam][r.src]));
    }
    long double top = 1.0L;
    for (const auto &v : mu) for (const long double x : v) top = std::max(top, x);
    unsigned bT = 1, dT = 0;
    if (!s.matmul) {
        bT = brent_certificate(L, R, P).beta - 2u;
        for (const QMat *M : {&L, &R, &P}) {
            std::set<__int128> dens;
            for (const auto &row : M->rows) for (const auto &e : row) if (e.second.d > 1) { dens.insert(e.second.d); avoid.insert(e.second.d); }
            for (const __int128 d : dens) dT += brent_bits(d);
        }
    }
    if (!(top < LDBL_MAX) || dbits > (1u << 20)) return c;                               // beta = 0: no certificate
    int ex = 0; (void)frexpl(top, &ex);                                                  // top < 2^ex
    const uint64_t beta = std::max<uint64_t>((uint64_t)std::max(ex, 1) + dT, bT) + dbits + 1u;
    if ((beta + 29u) / 30u > max_primes) return c;
    c.beta = (unsigned)beta; c.j = (c.beta + 29u) / 30u;
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
