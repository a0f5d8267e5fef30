// ==========================================================================
// plo_dep.hpp -- host side of bin/dependency (reference src/dependency.cpp): the coefficient list (:129-151), the depth-first
// enumeration of the combinations of at most `level` rows (`Explore`, :74-101), and the text of a hit (:44-71).
// The enumeration of one top row writes into a stream of its own, so the tool can run the top rows in any order and still
// print the reference's text.  Over Q the values are checked 128-bit rationals: an overflow is an exception, never a miss.
// ==========================================================================
#pragma once
#include "plo_host.hpp"

namespace plo {

// :129-140 over Q: `init` ({1, -1} and the -v values), then r, -r, 1/r, -1/r for every numerator and denominator of M not yet
// listed (`augment`, plinopt_sparsify.inl:21-35; rows in order, columns ascending), then for 2, 3, ... while the list is short;
// truncated to maxnum
inline std::vector<Rat> dep_rational_coeffs(const QMat &B, std::vector<Rat> C, size_t maxnum) {
    const QField Q;
    auto augment = [&](const Rat &r) {
        if (std::find(C.begin(), C.end(), r) != C.end()) return;
        const Rat t = Q.inv(r);
        C.push_back(r); C.push_back(Q.neg(r)); C.push_back(t); C.push_back(Q.neg(t));
    };
    for (const auto &row : B.rows) for (const auto &e : row) { augment(Rat::make(e.second.n, 1)); augment(Rat::make(e.second.d, 1)); }
    for (int64_t i = 2; C.size() < maxnum; ++i) augment(Rat(i));
    if (C.size() > maxnum) C.resize(maxnum);
    return C;
}

// :142-151: the images in list order, without zeros and repeats; a coefficient whose denominator is no unit of the field has
// no image and is dropped (the reference divides by it).  `kept` gets the rationals behind the images.
template <class F> std::vector<typename F::Elt> dep_field_coeffs(const F &f, const std::vector<Rat> &C, std::vector<Rat> *kept = nullptr) {
    std::vector<typename F::Elt> FC;
    for (const Rat &r : C) {
        typename F::Elt x;
        try { x = f.fromRat(r); } catch (const std::domain_error &) { continue; }
        if (f.isZero(x) || std::find(FC.begin(), FC.end(), x) != FC.end()) continue;
        FC.push_back(x);
        if (kept) kept->push_back(r);
    }
    return FC;
}

// showOut (:44-63): sign, letter, index, then the magnitude of a value that is not +-1 -- over Q `/den` for +-1/den and `*|r|`
// otherwise, over Z_p `*Fabs` with the sign of Fsign (plinopt_library.h:208-225) on the residue in [0, p)
template <class F> void dep_show(std::ostream &os, const F &f, char c, size_t i, const typename F::Elt &r) {
    os << (f.sign(r) < 0 ? '-' : '+') << c << i;
    if (absOne(f, r)) return;
    if constexpr (std::is_same<F, QField>::value) {
        if (r.n == 1 || r.n == -1) { os << '/' << r.d; return; }
    }
    os << '*'; f.write(os, f.abs(r));
}

template <class F> class DepSearch {
    using E = typename F::Elt;
    const F &f; const SparseMat<E> &M; const std::vector<E> &FC; const size_t m, n;

    void explore(std::ostream &os, std::vector<std::pair<size_t, size_t>> &LC, std::vector<std::vector<E>> &Ws, size_t last, size_t level) const {
        if (level == 0) return;
        const size_t depth = LC.size();                   // rows so far; their vector is Ws[depth - 1]
        for (size_t q = last + 1; q < m; ++q)
            for (size_t v = 0; v < FC.size(); ++v) {
                std::vector<E> &X = Ws[depth];
                X = Ws[depth - 1];
                for (const auto &e : M.rows[q]) X[e.first] = f.add(X[e.first], f.mul(FC[v], e.second));
                LC.emplace_back(q, v);
                line(os, LC, X);
                explore(os, LC, Ws, q, level - 1);
                LC.pop_back();
            }
    }
public:
    DepSearch(const F &ff, const SparseMat<E> &MM, const std::vector<E> &fc) : f(ff), M(MM), FC(fc), m(MM.rowdim()), n(MM.coldim()) {}

    // showLC (:65-71) of the combination LC = (row, coefficient index) pairs, the first being the top row with 1
    void show_lc(std::ostream &os, const std::vector<std::pair<size_t, size_t>> &LC) const {
        for (size_t k = 0; k < LC.size(); ++k) dep_show(os, f, 'o', LC[k].first, k ? FC[LC[k].second] : f.one());
        os << ";\n";
    }
    // the line of the combination whose value is W, when it vanishes or has one non-zero (:85-92); false when it is no hit
    bool line(std::ostream &os, const std::vector<std::pair<size_t, size_t>> &LC, const std::vector<E> &W) const {
        size_t cnt = 0, pos = 0;
        for (size_t j = 0; j < n; ++j) if (!f.isZero(W[j])) { if (++cnt == 2) return false; pos = j; }
        if (cnt == 1) dep_show(os, f, 'i', pos, f.neg(W[pos]));
        show_lc(os, LC);
        return true;
    }
    // the value of a combination, recomputed from the rows
    std::vector<E> value(const std::vector<std::pair<size_t, size_t>> &LC) const {
        std::vector<E> W(n, f.zero());
        for (size_t k = 0; k < LC.size(); ++k) {
            const E c = k ? FC[LC[k].second] : f.one();
            for (const auto &e : M.rows[LC[k].first]) W[e.first] = f.add(W[e.first], f.mul(c, e.second));
        }
        return W;
    }
    // every combination under top row i of at most `maxsize` rows (:158-165), in the reference's order
    void top_row(std::ostream &os, size_t i, size_t maxsize) const {
        if (maxsize < 2 || i + 1 >= m) return;
        const size_t depth = std::min(maxsize, m - i);
        std::vector<std::vector<E>> Ws(depth, std::vector<E>(n, f.zero()));
        for (const auto &e : M.rows[i]) Ws[0][e.first] = e.second;
        std::vector<std::pair<size_t, size_t>> LC{{i, 0}};
        explore(os, LC, Ws, i, depth - 1);
    }
};

// combinations of 2 .. maxsize rows with c coefficients: sum over the top rows of sum_s C(rows after, s - 1) c^(s - 1)
inline double dep_combinations(size_t m, size_t c, size_t maxsize) {
    double total = 0;
    for (size_t i = 0; i < m; ++i) {
        const size_t r = m - 1 - i;
        double term = 1;
        for (size_t s = 1; s < maxsize && s <= r; ++s) { term = term * (double)(r - s + 1) / (double)s * (double)c; total += term; }
    }
    return total;
}

} // namespace plo
