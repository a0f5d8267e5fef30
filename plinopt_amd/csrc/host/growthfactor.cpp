// ==========================================================================
// bin/growthfactor -- the growth factors of a matrix-multiplication triple in several norms (reference src/growthfactor.cpp):
//   growthfactor L.sms R.sms P.sms
// clog: the reference's text, line for line (:185-231): `# Norms of m x k x n Matrix-Multiplication:`, the column header, then
// eleven `##` lines in std::fixed with the default precision, each a value and its logarithm to the base k: Ginfinf, Ginf2, G2inf,
// G22, G2 (the number the names of the reference's data/ files carry, and what bin/orbiter -g searches), Q0 and five Qk.
// The arithmetic is the reference's as written: an entry is double(num)/double(den), norms are summed in entry order, G2 over i
// in increasing order as (n2(L_i) n2(R_i)) n2(Pt_i), Qk = q0 gamma / |gamma - k| (inf when gamma equals k).  Built without
// contraction of a product and a sum into one fused operation.
// Status 2: an inner-dimension mismatch (the reference's message), or shapes that are not r x mk, r x kn, mn x r (m, k, n are
// derived as bin/orbiter derives them; the reference takes a rounded square root and goes on).  -h or fewer than three files:
// the usage.
// ==========================================================================
#include "plo_orbit.hpp"
#include <iomanip>

using namespace plo;

namespace {
using Row = QMat::Row;
double access(const Rat &a) { return (double)a.n / (double)a.d; }
double absd(double a) { return a > 0 ? a : -a; }                                           // GIVABS

double norm1(const Row &v) { double s = 0; for (const auto &it : v) s += absd(access(it.second)); return s; }
double norm2(const Row &v) { double s = 0.; for (const auto &it : v) s += access(it.second) * access(it.second); return std::sqrt(s); }
double norm2(const std::vector<double> &v) { double s = 0.; for (double x : v) s += x * x; return std::sqrt(s); }

// r[j] = sum over i of (norm(L_i) norm(R_i)) |P[j][i]|, i in increasing order (:58-69 with norm1, :87-98 with norm2): read_sms keeps
// every row sorted by column, whatever the order of the file, so walking the entries of row j is the reference's order (its zero
// entries add 0.0)
template <class Norm> std::vector<double> GP(const QMat &L, const QMat &R, const QMat &P, Norm norm) {
    std::vector<double> lr(P.coldim()), r(P.rowdim(), 0.);
    for (size_t i = 0; i < P.coldim(); ++i) lr[i] = norm(L.rows[i]) * norm(R.rows[i]);
    for (size_t j = 0; j < P.rowdim(); ++j) for (const auto &e : P.rows[j]) r[j] += lr[e.first] * absd(access(e.second));
    return r;
}
double maxel(const std::vector<double> &r) { return *std::max_element(r.begin(), r.end()); }

double G2(const QMat &L, const QMat &R, const QMat &P) {                                   // :117-125
    const QMat Pt = transpose(P);
    double s = 0.;
    for (size_t i = 0; i < P.coldim(); ++i) s += norm2(L.rows[i]) * norm2(R.rows[i]) * norm2(Pt.rows[i]);
    return s;
}

double Q0(const QMat &L, const QMat &R, const QMat &P) {                                   // :128-144
    std::vector<double> n0(P.coldim(), 0.), r(P.rowdim(), 0.);
    for (size_t i = 0; i < P.coldim(); ++i) n0[i] = (double)(L.rows[i].size() * R.rows[i].size());
    for (size_t j = 0; j < P.rowdim(); ++j) {
        for (const auto &it : P.rows[j]) if (n0[it.first] > r[j]) r[j] = n0[it.first];
        r[j] += (double)P.rows[j].size();
    }
    return maxel(r);
}

double Qk(double q0, double gamma, double k) { return q0 * gamma / std::abs(gamma - k); }

QMat read_file(const std::string &f) {
    std::ifstream in(f);
    if (!in) throw std::runtime_error("cannot read " + f);
    return read_sms(in);
}
} // namespace

int main(int argc, char **argv) {
    if (argc <= 3 || std::string(argv[1]) == "-h") {
        std::clog << "Usage:" << argv[0] << " L.sms R.sms P.sms\n";
        return -1;
    }
    try {
        const QMat L = read_file(argv[1]), R = read_file(argv[2]), P = read_file(argv[3]);
        if (L.rowdim() != R.rowdim() || L.rowdim() != P.coldim()) {
            std::cerr << "# \033[1;31m****** ERROR, inner dimension mismatch: " << L.rowdim() << "(.)" << R.rowdim() << '|' << P.coldim() << " ******\033[0m" << std::endl;
            return 2;
        }
        size_t m = 0, k = 0, n = 0;
        if (!orbit_shape(L.rowdim(), L.coldim(), R.rowdim(), R.coldim(), P.rowdim(), P.coldim(), m, k, n)) {
            std::cerr << "# \033[1;31mERROR: shapes " << L.rowdim() << 'x' << L.coldim() << ", " << R.rowdim() << 'x' << R.coldim() << ", " << P.rowdim() << 'x' << P.coldim()
                      << " are not r x mk, r x kn, mn x r\033[0m\n";
            return 2;
        }
        std::clog << "# Norms of " << m << 'x' << k << 'x' << n << " Matrix-Multiplication:" << std::endl;

        const std::vector<double> gpinf = GP(L, R, P, [](const Row &v) { return norm1(v); }), gp2 = GP(L, R, P, [](const Row &v) { return norm2(v); });
        const double ginfinf = maxel(gpinf), ginf2 = maxel(gp2), g2inf = norm2(gpinf), g22 = norm2(gp2), g2 = G2(L, R, P), q0 = Q0(L, R, P);
        const double kd = (double)k, sqrtk = std::sqrt(kd), kth = sqrtk * sqrtk * sqrtk;
        const std::pair<const char *, double> lines[] = {
            {"Ginfinf:\t", ginfinf}, {"Ginf2:\t", ginf2}, {"G2inf:\t", g2inf}, {"G22:\t\t", g22}, {"G2:\t\t", g2}, {"Q0:\t\t", q0},
            {"Qkinfinf:\t", Qk(q0, ginfinf, kd)}, {"Q1inf2:\t", Qk(q0, ginf2, 1)}, {"Qk12inf:\t", Qk(q0, g2inf, 1)}, {"Qk2inf:\t", Qk(q0, g2inf, kth)}, {"Q122:\t", Qk(q0, g22, 1)}};
        std::clog << std::fixed << std::setw(8) << "#  \t\tGamma \t\tlog_" << k << std::endl;
        for (const auto &ln : lines) std::clog << "## " << ln.first << ln.second << '\t' << std::log(ln.second) / std::log(kd) << std::endl;
        return 0;
    } catch (const std::exception &e) { std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m\n"; return 4; }
}
