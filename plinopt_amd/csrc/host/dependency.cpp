// ==========================================================================
// bin/dependency -- linear dependencies between the rows of a matrix (reference src/dependency.cpp):
//   dependency [-c #] [-v "# ... #"] [-l #] [-q #] [--gpu 0|1] [stdin|matfile.sms]
// Every combination  o<i> + c1 o<q1> + c2 o<q2> + ...  (i < q1 < q2 < ...) of at most -l rows (default 4), with coefficients from
// a list of at most -c values (default 11: 1, -1, the -v values, then r, -r, 1/r, -1/r for the numerators and denominators of
// the matrix and for 2, 3, ...), that vanishes or equals a multiple of one input is printed: `+o0-o3*2;` or `-i5/2+o0+o3;`
// (the combination equals minus the `i` term), in the reference's depth-first order.  clog: the `# [DEPND]` lines.
// Fields: Q (default) or Z_q; over Z_q every value is the residue in [0, q), and a coefficient without an image is dropped.
// The enumeration runs on the GPU through plo_dep_search of libplinopt_hip.so; over Q the device works modulo a prime and
// reports a superset of the hits, which is recomputed here over Q: no true hit is lost and no false one printed.  --gpu 0, or an
// input the device refuses (a level above 8 or -l 0, a modulus of 2^31 or more, a denominator that vanishes modulo its prime, a
// coefficient wider than 64 bits, sizes beyond its limits), uses the host loop (OpenMP over the top rows) and says so.
// Refused with status 2: a matrix entry whose denominator is no unit modulo q, a modulus above 2^62.
// ==========================================================================
#include "plo_dep.hpp"
#include "plo_dl.hpp"
#include <chrono>

using namespace plo;

namespace {
struct HipDep {
    void *h = open_hip_lib(); bool ok = h != nullptr;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error);
    PLO_SYM(create, plo_dep_plan_create_q); PLO_SYM(destroy, plo_dep_plan_destroy); PLO_SYM(search, plo_dep_search);
};

struct Opts { size_t maxnum = 11, level = 4; int gpu = 1; std::vector<Rat> coeffs{Rat(1), Rat(-1)}; };

int refuse(const std::string &why) { std::cerr << "# \033[1;31mERROR: " << why << "\033[0m\n"; return 2; }

template <class F> int dep_run(const F &f, const QMat &B, uint64_t modulus, const Opts &o) {
    using E = typename F::Elt;
    const SparseMat<E> M = rebind(B, f);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Rat> kept;
    const std::vector<E> FC = dep_field_coeffs(f, dep_rational_coeffs(B, o.coeffs, o.maxnum), &kept);
    std::clog << "# [DEPND] level " << o.level << ", coefficients: [";
    for (size_t v = 0; v < FC.size(); ++v) { if (v) std::clog << ','; f.write(std::clog, FC[v]); }
    std::clog << ']' << std::endl;
    const size_t m = M.rowdim(), maxsize = o.level ? o.level : ~(size_t)0;   // -l 0: level - 1 wraps in the reference, every depth
    const DepSearch<F> S(f, M, FC);
    std::vector<std::string> out(m);
    bool on_gpu = false, refused = false; std::string why; double kms = 0;
    if (o.gpu && !FC.empty() && m > 0) {
        const QCsr cm = qcsr(B);
        std::vector<int64_t> cnum, cden;
        bool wide = cm.wide;
        for (const Rat &r : kept) {
            if (r.n > (__int128)INT64_MAX || r.n < -(__int128)INT64_MAX || r.d > (__int128)INT64_MAX) wide = true;
            cnum.push_back((int64_t)r.n); cden.push_back((int64_t)r.d);
        }
        if (wide) { refused = true; why = "a coefficient wider than 64 bits"; }
        else if (o.level == 0 || o.level > 0xFFFFFFFFull) { refused = true; why = "every depth (-l 0)"; }
        else {
            HipDep H;
            if (!H.ok) return refuse("libplinopt_hip.so cannot be loaded or lacks plo_dep_search");   // no silent fallback
            const plo_qcsr_t view = cm.view();
            plo_dep_plan_t *plan = nullptr; plo_stats_t st{};
            std::vector<plo_dep_hit_t> hits(1u << 16);
            uint64_t nh = 0;
            int rc = H.init(0);
            if (rc == PLO_OK) rc = H.create(&view, cnum.data(), cden.data(), (uint32_t)cnum.size(), modulus, (uint32_t)o.level, &plan);
            if (rc == PLO_OK) rc = H.search(plan, 0, (uint32_t)m, hits.data(), hits.size(), &nh, &st);
            kms = st.kernel_ms;
            if (rc == PLO_E_CAPACITY && plan && nh > hits.size() && nh <= (1ull << 24)) {      // the full count came back: once more, with room
                hits.resize(nh);
                rc = H.search(plan, 0, (uint32_t)m, hits.data(), hits.size(), &nh, &st);
                kms += st.kernel_ms;
            }
            if (plan) H.destroy(plan);
            if (rc == PLO_E_UNSUPPORTED || rc == PLO_E_CAPACITY) { refused = true; why = H.last_error(); }
            else if (rc != PLO_OK) return refuse(H.last_error());
            else {
                on_gpu = true;
                std::vector<std::ostringstream> os(m);
                std::vector<std::pair<size_t, size_t>> LC;
                for (uint64_t k = 0; k < nh; ++k) {
                    const plo_dep_hit_t &h = hits[k];
                    LC.clear();
                    for (uint32_t j = 0; j < h.size; ++j) LC.emplace_back(h.rows[j], h.coef[j]);
                    std::ostream &dst = os[h.rows[0]];
                    if constexpr (std::is_same<F, QField>::value) S.line(dst, LC, S.value(LC));   // the superset filter: the verdict is the one over Q
                    else {
                        if (h.kind == PLO_DEP_ONE) dep_show(dst, f, 'i', h.col, f.neg((E)h.residue));
                        S.show_lc(dst, LC);
                    }
                }
                for (size_t i = 0; i < m; ++i) out[i] = os[i].str();
            }
        }
    }
    if (!on_gpu) {
        if (o.gpu && refused) std::clog << "# the device refuses this input (" << why << "): host search" << std::endl;
        std::string err;
        #pragma omp parallel for schedule(dynamic, 1)
        for (long long i = 0; i < (long long)m; ++i) {
            try { std::ostringstream os; S.top_row(os, (size_t)i, maxsize); out[(size_t)i] = os.str(); }
            catch (const std::exception &e) {
                #pragma omp critical
                err = e.what();
            }
        }
        if (!err.empty()) throw std::runtime_error(err);                                   // Q: an overflow is an error
    }
    for (size_t i = 0; i < m; ++i) { std::clog << "# [DEPND] o" << i << std::endl; std::cout << out[i]; }
    std::cout.flush();
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::clog << "# [DEPND]: " << dt << "s" << std::endl;
    char buf[64]; snprintf(buf, sizeof buf, "%.0f", dep_combinations(m, FC.size(), maxsize));
    std::clog << "# " << buf << " combinations on " << (on_gpu ? "GPU" : "host") << " in " << dt << " s";
    if (on_gpu) std::clog << " (kernel " << kms << " ms)";
    std::clog << std::endl;
    return 0;
}

int usage(const char *prg) {
    std::clog << "Usage: " << prg << " [-h|[-c|-l|-q] #] [-v \"# ... #\"] [--gpu 0|1] [stdin|matfile.sms]\n"
              << "  -c #: max number of coefficients per iteration\n"
              << "  -v \"# ... #\": string of space separated coefficients\n"
              << "  -l #: maximal number of monomials in the combination\n"
              << "  -q #: modular generation/check (default is Rationals)\n"
              << "  --gpu 0|1: host loop, or the enumeration on the GPU (default 1)\n";
    return -1;
}
} // namespace

int main(int argc, char **argv) {
    cap_omp_threads();
    Opts o; std::string filename; unsigned __int128 q = 0;
    try {
        for (int i = 1; i < argc; ++i) {
            const std::string a(argv[i]);
            auto need = [&]() { if (i + 1 >= argc) throw std::invalid_argument("option " + a + " needs an argument"); return argv[++i]; };
            if (a == "-h") return usage(argv[0]);
            else if (a == "-q") {
                const char *s = need(); q = 0;
                if (!*s) return refuse("modulus is not a natural number");
                for (; *s; ++s) { if (!isdigit((unsigned char)*s) || q > ((unsigned __int128)1 << 100)) return refuse("modulus is not a natural number below 2^100"); q = q * 10 + (unsigned)(*s - '0'); }
            }
            else if (a == "-c") o.maxnum = (size_t)strtoull(need(), nullptr, 10);
            else if (a == "-l") o.level = (size_t)strtoull(need(), nullptr, 10);
            else if (a == "-v") { std::istringstream in(need()); std::string t; while (in >> t) o.coeffs.push_back(parse_rat(t)); }
            else if (a == "--gpu") o.gpu = atoi(need());
            else if (a.size() > 1 && a[0] == '-') return refuse("unknown option " + a);
            else filename = a;
        }
    } catch (const std::exception &e) { return refuse(e.what()); }
    if (q == 1 || q > ((unsigned __int128)1 << 62)) return refuse("modulus 1 or above 2^62");
    const uint64_t modulus = (uint64_t)q;
    try {
        QMat B;
        if (filename.empty() || filename == "-") B = read_sms(std::cin);
        else { std::ifstream in(filename); if (!in) throw std::runtime_error("cannot read " + filename); B = read_sms(in); }
        if (modulus)
            for (const auto &row : B.rows) for (const auto &e : row)
                if (Rat::gcd(e.second.d % (__int128)modulus, (__int128)modulus) != 1)
                    return refuse("a denominator (" + std::to_string((long long)e.second.d) + ") is not invertible modulo " + std::to_string(modulus));
        if (!modulus) return dep_run(QField{}, B, 0, o);
        if (modulus < (1ull << 31)) return dep_run(ZpField((uint32_t)modulus), B, modulus, o);
        return dep_run(Zp64Field(modulus), B, modulus, o);
    } catch (const std::exception &e) { std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m\n"; return 4; }
}
