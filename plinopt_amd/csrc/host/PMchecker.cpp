// ==========================================================================
// bin/PMchecker -- checks that a triple (L, R, P) is a polynomial-multiplication algorithm (reference src/PMchecker.cpp):
//   PMchecker [-b #] [-m|-q #] [-I x] [-P "P(x)"] [--gpu 0|1] [--pairs first:count] [--count] L.sms R.sms P.sms
// L (r x na), R (r x nb), P (nc x r) claim to multiply a polynomial of degree na-1 by one of degree nb-1 into nc coefficients,
// with -P modulo that polynomial.  The reference multiplies two random polynomials both ways, so its answer is probably right;
// here every coefficient equation of every pair of monomials is computed (plo_polymul.hpp), on the GPU through
// plo_polymul_check of libplinopt_hip.so, and the verdict is exact: with S[i][j][z] = sum_t L[t][i] R[t][j] P[z][t] and
// Z = max(nc, na+nb-1), equation e = (i nb + j) w + c asks S[i][j][c] == [c == i+j] over the width w = Z, or with -P f, of degree d,
// sum_z S[i][j][z] rho[z][c] == rho[i+j][c] over the width w = d, rho[z] = X^z mod f.  A P with too few rows shows as violated
// equations at c = i+j >= nc; f need not be irreducible.
// -P takes sums of terms [+-][a[/b]][*][X[^e]], spaces allowed, repeated exponents added; -I x names the indeterminate.
// clog/cerr: the reference's verdict line, `# SUCCESS: correct AoBoC Polynomial-Multiplication over <field>[ mod f]` or
// `****** ERROR, not a AoBoC MM algorithm over <field>******` (sic), then the first violated equation as (i, j, c) with the value
// found and the one expected, with --count the number of violated ones, and a `# GPU:` (or `# host:`) line.
// Fields: with -m/-q the integers modulo that number, taken as given (2 and composites included; no factor 2 is removed, unlike
// bin/MMchecker); otherwise Q, proved from checks modulo j primes above 2^30 that divide no denominator and not the leading
// coefficient of f (the `# certificate` line: beta bounds the bits of an equation's cleared defect, after its pseudo-division
// by f, j = ceil(beta / 30)); a `# pass` line per prime, the passes stop at the first prime that fails, and the values of its
// first violated equation are then printed as rationals.  -b is accepted and does nothing: the check has no randomness.
// --gpu 1 (default) uses the kernel for a modulus below 2^31 and coefficients of at most 64 bits; otherwise, and with --gpu 0,
// the host loop (OpenMP over the i slabs) on the same definition, which it announces.  A library that cannot be loaded is an
// error, never a reason for the host loop.  --pairs first:count checks the pairs (i, j) = first .. first + count - 1 only and
// says so on the verdict line; --count goes on behind the first failing launch and counts every violated equation.
// Exit status: 0 correct, 1 not a polynomial-multiplication algorithm, 2 inner dimension mismatch; 4 for what is refused here
// (a denominator or the leading coefficient of f that is no unit, a constant or unparsable -P, a modulus 1 or above 2^62,
// unreadable input, a device error).
// ==========================================================================
#include "plo_polymul.hpp"
#include "plo_dl.hpp"
#include <chrono>

using namespace plo;

namespace {
struct HipPolyMul {
    void *h = open_hip_lib(); bool ok = h != nullptr;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error);
    PLO_SYM(create, plo_polymul_plan_create_q); PLO_SYM(destroy, plo_polymul_plan_destroy);
    PLO_SYM(check, plo_polymul_check); PLO_SYM(info, plo_polymul_plan_info);
};

struct Opts { int gpu = 1; bool count = false, partial = false; uint64_t first = 0, npairs = 0; unsigned __int128 modulus = 0; char indet = 'X'; std::string poly; bool has_poly = false; };

// what one pass (all pairs of the range, one modulus) found; value, expected: the residues at `first`
struct Pass { uint64_t violated = 0, first = ~0ull, value = 0, expected = 0, equations = 0; double kms = 0; uint32_t launches = 0; };

int refuse(const std::string &why) { std::cerr << "# \033[1;31mERROR: " << why << "\033[0m\n"; return 4; }

QMat read_file(const std::string &f) {
    std::ifstream in(f);
    if (!in) throw std::runtime_error("cannot read " + f);
    return read_sms(in);
}

struct Triple { QMat L, R, P; std::vector<Rat> f; };                       // f: the coefficients of -P, empty without one

template <class F> std::vector<typename F::Elt> poly_over(const F &f, const std::vector<Rat> &co) {
    std::vector<typename F::Elt> out;
    for (const Rat &c : co) out.push_back(f.fromRat(c));
    return out;
}

template <class F> Pass host_pass(const F &f, const Triple &T, uint64_t pair0, uint64_t pair1, bool count_all) {
    const auto LT = rebind(transpose(T.L), f), R = rebind(T.R, f), PT = rebind(transpose(T.P), f);
    const auto spec = polymul_spec(f, T.L.coldim(), T.R.coldim(), T.P.rowdim(), poly_over(f, T.f));
    const auto found = polymul_host(f, spec, LT, R, PT, pair0, pair1, count_all);
    Pass ps; ps.violated = found.violated; ps.first = found.first; ps.value = (uint64_t)found.value; ps.expected = (uint64_t)found.expected;
    ps.equations = (pair1 - pair0) * (uint64_t)spec.w;
    return ps;
}

// the device's pass: one plan, then the range in pieces of the plan's pairs per launch, up to the first failing piece unless count_all
int device_pass(HipPolyMul &H, const plo_qcsr_t &l, const plo_qcsr_t &r, const plo_qcsr_t &p, const std::vector<int64_t> &fnum, const std::vector<int64_t> &fden, uint32_t q,
                uint64_t pair0, uint64_t pair1, bool count_all, Pass &ps) {
    plo_polymul_plan_t *plan = nullptr;
    int rc = H.create(&l, &r, &p, fnum.data(), fden.data(), (uint32_t)fnum.size(), q, &plan);
    uint32_t info[8] = {0};
    if (rc == PLO_OK) rc = H.info(plan, info);
    for (uint64_t p0 = pair0; rc == PLO_OK && p0 < pair1;) {
        const uint64_t cnt = std::min<uint64_t>(std::max<uint32_t>(info[3], 1u), pair1 - p0);
        plo_brent_result_t res{}; plo_stats_t st{};
        rc = H.check(plan, p0, p0 + cnt, &res, &st);
        if (rc != PLO_OK) break;
        ps.kms += st.kernel_ms; ps.launches += st.launches; ps.equations += st.candidates;
        if (res.violated) {
            if (ps.violated == 0) { ps.first = res.first; ps.value = res.value; ps.expected = res.expected; }
            ps.violated += res.violated;
            if (!count_all) break;
        }
        p0 += cnt;
    }
    if (plan) H.destroy(plan);
    return rc;
}

int usage(const char *prg) {
    std::clog << "Usage: " << prg << " [-h|-b #|-m/-q #] [-I x] [-P \"P(x)\"] [--gpu 0|1] [--pairs first:count] [--count] L.sms R.sms P.sms\n"
              << "  [-b b]: accepted and ignored: every coefficient equation is checked, there is no randomness\n"
              << "  [-m/-q m]: check is modulo m, taken as given (default: over Q, proved modulo primes)\n"
              << "  [-I x]: indeterminate (default is X)\n"
              << "  [-P P(x)]: the product is taken modulo this polynomial (default is none); it need not be irreducible\n"
              << "  [--gpu 0|1]: host loop, or the equations on the GPU (default 1)\n"
              << "  [--pairs first:count]: only the pairs (i, j) = first .. first+count-1 of the na.nb (a partial check)\n"
              << "  [--count]: count every violated equation (default: stop behind the first failing launch)\n";
    return -1;
}

int run(const Triple &T, uint64_t modulus, const Opts &o) {
    const size_t na = T.L.coldim(), nb = T.R.coldim(), nc = T.P.rowdim();
    const size_t Z = std::max(nc, na + nb ? na + nb - 1 : 0), w = T.f.empty() ? Z : T.f.size() - 1;
    const uint64_t npairs = (uint64_t)na * nb;
    const uint64_t pair0 = o.partial ? o.first : 0, pair1 = o.partial ? o.first + o.npairs : npairs;
    if (pair0 >= pair1 || pair1 > npairs) return refuse("--pairs " + std::to_string(o.first) + ":" + std::to_string(o.npairs) + " is empty or goes beyond the " + std::to_string(npairs) + " pairs");
    const QField Qf;
    const std::string field = modulus ? "Z/" + std::to_string(modulus) + "Z" : "Q";
    const std::string note = o.partial ? " [partial: pairs " + std::to_string(pair0) + " .. " + std::to_string(pair1 - 1) + " of " + std::to_string(npairs) + "]" : "";
    const std::string mod = T.f.empty() ? "" : " mod " + poly_text(Qf, T.f, o.indet);

    // over Q the passes take f as its primitive integer multiple: no prime then meets a denominator of f
    Triple TQ;
    const Triple *use = &T;
    std::vector<uint64_t> moduli{modulus};
    if (!modulus) {
        const std::vector<__int128> fz = primitive_poly(T.f);
        const BrentCert c = polymul_certificate(T.L, T.R, T.P, fz);
        moduli.assign(c.primes.begin(), c.primes.end());
        std::clog << "# certificate: beta = " << c.beta << ", j = " << c.j << ", primes";
        for (uint32_t p : c.primes) std::clog << ' ' << p;
        std::clog << std::endl;
        TQ = T; TQ.f.clear();
        for (const __int128 v : fz) TQ.f.push_back(Rat::make(v, 1));
        use = &TQ;
    }

    bool on_gpu = false;
    const QCsr cl = qcsr(T.L), cr = qcsr(T.R), cp = qcsr(T.P);
    std::vector<int64_t> fnum, fden; bool fwide = false;
    for (const Rat &c : use->f) {
        if (c.n > (__int128)INT64_MAX || c.n < -(__int128)INT64_MAX || c.d > (__int128)INT64_MAX) fwide = true;
        fnum.push_back((int64_t)c.n); fden.push_back((int64_t)c.d);
    }
    HipPolyMul *H = nullptr;
    if (o.gpu) {
        std::string why;
        if (cl.wide || cr.wide || cp.wide || fwide) why = "a coefficient wider than 64 bits";
        else if (modulus >= (1ull << 31)) why = "a modulus of 2^31 or more";
        if (why.empty()) {
            static HipPolyMul lib;
            if (!lib.ok) return refuse("libplinopt_hip.so cannot be loaded or lacks plo_polymul_check");   // no silent fallback
            if (lib.init(0) != PLO_OK) return refuse(lib.last_error());
            H = &lib; on_gpu = true;
        } else std::clog << "# the device refuses this input (" << why << "): host loop" << std::endl;
    }
    const plo_qcsr_t l = cl.view(), r = cr.view(), p = cp.view();

    const auto t0 = std::chrono::steady_clock::now();
    Pass total; uint64_t failed_mod = 0; size_t npass = 0;
    for (const uint64_t q : moduli) {
        Pass ps;
        bool done = false;
        if (on_gpu) {
            const int rc = device_pass(*H, l, r, p, fnum, fden, (uint32_t)q, pair0, pair1, o.count, ps);
            if (rc == PLO_E_CAPACITY || rc == PLO_E_UNSUPPORTED) { std::clog << "# the device refuses this input (" << H->last_error() << "): host loop" << std::endl; on_gpu = false; }
            else if (rc != PLO_OK) return refuse(H->last_error());
            else done = true;
        }
        if (!done) ps = q < (1ull << 31) ? host_pass(ZpField((uint32_t)q), *use, pair0, pair1, o.count) : host_pass(Zp64Field(q), *use, pair0, pair1, o.count);
        total.equations += ps.equations; total.kms += ps.kms; total.launches += ps.launches;
        ++npass;
        if (!modulus) std::clog << "# pass " << npass << " of " << moduli.size() << " modulo " << q << ": " << (ps.violated ? "violated" : "no violated equation") << std::endl;
        if (ps.violated) { total.violated = ps.violated; total.first = ps.first; total.value = ps.value; total.expected = ps.expected; failed_mod = q; break; }
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    if (!failed_mod) std::clog << pm_success_line(na, nb, nc, field, mod, note) << std::endl;
    else {
        std::cerr << pm_error_line(na, nb, nc, field + note, mod) << std::endl;
        const uint64_t e = total.first, c = e % w, pr = e / w, i = pr / nb, j = pr % nb;
        std::clog << "# first violated equation e=" << e << ": (i,j,c) = (" << i << ',' << j << ',' << c << "), found ";
        if (modulus) std::clog << total.value << " instead of " << total.expected;
        else {
            try {                                                                          // the pair once more, over Q
                const auto LT = transpose(T.L), PT = transpose(T.P);
                const auto spec = polymul_spec(Qf, na, nb, nc, T.f);
                std::vector<Rat> S(nc, Rat(0)), got, want;
                for (const auto &lt : LT.rows[i]) for (const auto &rt : T.R.rows[lt.first]) if (rt.first == j)
                    for (const auto &pt : PT.rows[lt.first]) S[pt.first] = Qf.add(S[pt.first], Qf.mul(Qf.mul(lt.second, rt.second), pt.second));
                polymul_pair(Qf, spec, S.data(), i, j, got, want);
                std::clog << got[c] << " instead of " << want[c];
            } catch (const std::exception &ex) { std::clog << "(" << ex.what() << ")"; }
            std::clog << "; modulo " << failed_mod << ": " << total.value << " instead of " << total.expected;
        }
        std::clog << std::endl;
        if (o.count) {
            std::clog << "# " << total.violated << " of " << (pair1 - pair0) * w << " equations violated";
            if (!modulus) std::clog << " modulo " << failed_mod << " (no more than over Q)";
            std::clog << std::endl;
        }
    }
    char rate[64]; snprintf(rate, sizeof rate, "%.4g", dt > 0 ? (double)total.equations / dt : 0.0);
    std::clog << "# " << (on_gpu ? "GPU" : "host") << ": " << total.equations << " equations in " << dt << " s, " << rate << " equations/s";
    if (on_gpu) std::clog << " (kernel " << total.kms << " ms, " << total.launches << " launches)";
    std::clog << std::endl;
    return failed_mod ? 1 : 0;
}
} // namespace

int main(int argc, char **argv) {
    cap_omp_threads();
    Opts o; std::vector<std::string> files;
    auto num = [](const char *s, unsigned __int128 &v) {                                   // a natural number, false above 2^120
        v = 0; if (!*s) return false;
        for (; *s; ++s) { if (!isdigit((unsigned char)*s) || v > ((unsigned __int128)1 << 120)) return false; v = v * 10 + (unsigned)(*s - '0'); }
        return true;
    };
    try {
        for (int i = 1; i < argc; ++i) {
            const std::string a(argv[i]);
            auto need = [&](int c) { if (i + c >= argc) throw std::invalid_argument("option " + a + " needs " + std::to_string(c) + " argument(s)"); };
            if (a == "-h") return usage(argv[0]);
            else if (a == "-b") { need(1); ++i; }
            else if (a == "-m" || a == "-q") { need(1); if (!num(argv[++i], o.modulus)) return refuse("modulus " + std::string(argv[i]) + " is not a natural number below 2^120"); }
            else if (a == "-I") { need(1); const std::string x(argv[++i]); if (x.size() != 1 || !isalpha((unsigned char)x[0])) return refuse("-I needs one letter"); o.indet = x[0]; }
            else if (a == "-P") { need(1); o.poly = argv[++i]; o.has_poly = true; }
            else if (a == "--gpu") { need(1); o.gpu = atoi(argv[++i]); }
            else if (a == "--count") o.count = true;
            else if (a == "--pairs") {
                need(1); const std::string s(argv[++i]); const size_t c = s.find(':');
                unsigned __int128 f = 0, cnt = 0;
                if (c == std::string::npos || !num(s.substr(0, c).c_str(), f) || !num(s.substr(c + 1).c_str(), cnt) || f >> 62 || cnt >> 62) return refuse("--pairs needs first:count");
                o.partial = true; o.first = (uint64_t)f; o.npairs = (uint64_t)cnt;
            }
            else if (a.size() > 1 && a[0] == '-') return refuse("unknown option " + a);
            else files.push_back(a);
        }
    } catch (const std::invalid_argument &e) { return refuse(e.what()); }
    if (files.size() != 3) return usage(argv[0]);
    if (o.modulus == 1) return refuse("modulus 1");
    if (o.modulus > ((unsigned __int128)1 << 62)) return refuse("modulus above 2^62");
    const uint64_t modulus = (uint64_t)o.modulus;                                          // taken as given (src/PMchecker.cpp:213-216); 0: Q
    try {
        Triple T;
        T.L = read_file(files[0]); T.R = read_file(files[1]); T.P = read_file(files[2]);
        if (T.L.rowdim() != T.R.rowdim() || T.L.rowdim() != T.P.coldim()) {               // src/PMchecker.cpp:71-77
            std::cerr << "# \033[1;31m****** ERROR, inner dimension mismatch: " << T.L.rowdim() << "(.)" << T.R.rowdim() << '|' << T.P.coldim() << " ******\033[0m" << std::endl;
            return 2;
        }
        if (o.has_poly) {
            try { T.f = parse_poly(o.poly, o.indet); } catch (const std::invalid_argument &e) { return refuse(e.what()); }
            if (T.f.size() < 2) return refuse("-P \"" + o.poly + "\" is a constant: the degree must be 1 at least");
        }
        if (modulus) {
            auto unit = [&](__int128 v) { return Rat::gcd(v % (__int128)modulus, (__int128)modulus) == 1; };
            for (const QMat *M : {&T.L, &T.R, &T.P}) for (const auto &row : M->rows) for (const auto &e : row)
                if (!unit(e.second.d)) return refuse("a denominator (" + std::to_string((long long)e.second.d) + ") is not invertible modulo " + std::to_string(modulus));
            for (const Rat &c : T.f) if (!unit(c.d)) return refuse("a denominator of the polynomial (" + std::to_string((long long)c.d) + ") is not invertible modulo " + std::to_string(modulus));
            if (!T.f.empty()) {
                // the leading coefficient as a residue: numerator times the inverse of the denominator, a unit exactly when the numerator is
                if (!unit(T.f.back().n)) return refuse("the leading coefficient of the polynomial is not invertible modulo " + std::to_string(modulus));
            }
        }
        return run(T, modulus, o);
    } catch (const std::exception &e) { std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m\n"; return 4; }
}
