// ==========================================================================
// bin/MMchecker -- checks that a triple (L, R, P) is a matrix-multiplication algorithm (reference src/MMchecker.cpp):
//   MMchecker [-b #] [-m|-q #] [-r r e s] [--gpu 0|1] [--pairs first:count] [--count] L.sms R.sms P.sms
// The reference multiplies two random matrices both ways, so its answer is probably right; here every Brent equation
//     sum_t L[t][a k + b] R[t][b' n + c] P[a' n + c'][t] = [a = a'][b = b'][c = c']
// is computed (plo_brent.hpp), on the GPU through plo_brent_check of libplinopt_hip.so, and the verdict is exact.
// (m, k, n) is the reference's LRP2MM.  clog/cerr: the reference's verdict line, `# SUCCESS: correct MxKxN (nnz,nno)
// Matrix-Multiplication over <field>` or `****** ERROR, not a MxKxN MM algorithm`, then the first violated equation
// e = ((a k + b) kn + b' n + c) mn + a' n + c', with --count the number of violated ones, and a `# GPU:` (or `# host:`) line.
// Fields: with -m/-q/-r the integers modulo that number (factors 2 removed, 1 becomes 2; it need not be prime); otherwise Q, proved
// from checks modulo j primes above 2^30 (the `# certificate` line: beta bounds the bits of an equation's cleared defect, j =
// ceil(beta / 30)); the passes stop at the first prime that fails, and the sum of its first violated equation is then printed
// as a rational.  -b is accepted and does nothing: the check has no randomness.
// --gpu 1 (default) uses the kernel for a modulus below 2^31 and coefficients of at most 64 bits; otherwise, and with --gpu 0,
// the host loop (OpenMP over the x slabs) on the same definition, which it announces.  A library that cannot be loaded is an
// error, never a reason for the host loop.  --pairs first:count checks the pairs (x, y) = first .. first + count - 1 only and
// says so on the verdict line; --count goes on behind the first failing launch and counts every violated equation.
// Exit status as the reference's: 0 correct, 1 not an MM algorithm, 2 inner dimension mismatch, 3 outer dimension mismatch;
// 4 for what is refused here (-I/-P, a denominator that is no unit, a modulus above 2^62, unreadable input, a device error).
// ==========================================================================
#include "plo_brent.hpp"
#include "plo_dl.hpp"
#include <chrono>

using namespace plo;

namespace {
struct HipBrent {
    void *h = open_hip_lib(); bool ok = h != nullptr;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error);
    PLO_SYM(create, plo_brent_plan_create_q); PLO_SYM(destroy, plo_brent_plan_destroy);
    PLO_SYM(check, plo_brent_check); PLO_SYM(info, plo_brent_plan_info);
};

struct Opts { int gpu = 1; bool count = false, partial = false; uint64_t first = 0, npairs = 0; unsigned __int128 modulus = 0; };

// what one pass (all pairs of the range, one modulus) found; value: the residue at `first`
struct Pass { uint64_t violated = 0, first = ~0ull, value = 0, equations = 0; double kms = 0; uint32_t launches = 0; };

int refuse(const std::string &why) { std::cerr << "# \033[1;31mERROR: " << why << "\033[0m\n"; return 4; }

QMat read_file(const std::string &f) {
    std::ifstream in(f);
    if (!in) throw std::runtime_error("cannot read " + f);
    return read_sms(in);
}

struct Triple { QMat L, R, P; size_t m = 0, k = 0, n = 0; };

template <class F> Pass host_pass(const F &f, const Triple &T, uint64_t pair0, uint64_t pair1, bool count_all) {
    const auto LT = rebind(transpose(T.L), f), R = rebind(T.R, f), PT = rebind(transpose(T.P), f);
    const auto found = brent_host(f, LT, R, PT, T.k, T.n, pair0, pair1, count_all);
    Pass ps; ps.violated = found.violated; ps.first = found.first; ps.value = (uint64_t)found.value;
    ps.equations = (pair1 - pair0) * (uint64_t)(T.m * T.n);
    return ps;
}

// the device's pass: one plan, then the range in pieces of the plan's pairs per launch, up to the first failing piece unless count_all
int device_pass(HipBrent &H, const plo_qcsr_t &l, const plo_qcsr_t &r, const plo_qcsr_t &p, const Triple &T, uint32_t q, uint64_t pair0, uint64_t pair1, bool count_all, Pass &ps) {
    plo_brent_plan_t *plan = nullptr;
    int rc = H.create(&l, &r, &p, (uint32_t)T.m, (uint32_t)T.k, (uint32_t)T.n, q, &plan);
    uint32_t info[8] = {0};
    if (rc == PLO_OK) rc = H.info(plan, info);
    for (uint64_t p0 = pair0; rc == PLO_OK && p0 < pair1;) {
        const uint64_t cnt = std::min<uint64_t>(std::max<uint32_t>(info[3], 1u), pair1 - p0);
        plo_brent_result_t res{}; plo_stats_t st{};
        rc = H.check(plan, p0, p0 + cnt, &res, &st);
        if (rc != PLO_OK) break;
        ps.kms += st.kernel_ms; ps.launches += st.launches; ps.equations += st.candidates;
        if (res.violated) {
            if (ps.violated == 0) { ps.first = res.first; ps.value = res.value; }
            ps.violated += res.violated;
            if (!count_all) break;
        }
        p0 += cnt;
    }
    if (plan) H.destroy(plan);
    return rc;
}

void count_entries(const Triple &T, uint64_t modulus, size_t &nnz, size_t &nno) {
    nnz = nno = 0;
    auto tally = [&](const auto &f) {
        for (const QMat *M : {&T.L, &T.R, &T.P}) { const auto X = rebind(*M, f); for (const auto &row : X.rows) for (const auto &e : row) { ++nnz; if (!absOne(f, e.second)) ++nno; } }
    };
    if (!modulus) tally(QField{}); else if (modulus < (1ull << 31)) tally(ZpField((uint32_t)modulus)); else tally(Zp64Field(modulus));
}

int usage(const char *prg) {
    std::clog << "Usage: " << prg << " [-h|-b #|-m/-q #|-r # # #] [--gpu 0|1] [--pairs first:count] [--count] L.sms R.sms P.sms\n"
              << "  [-b b]: accepted and ignored: every Brent equation is checked, there is no randomness\n"
              << "  [-m/-q m]: check is modulo (mod) or (mod/2^k) (default: over Q, proved modulo primes)\n"
              << "  [-r r e s]: check is modulo (r^e-s) or ((r^e-s)/2^k)\n"
              << "  [-I x], [-P P(x)]: polynomial quotients are not supported (refused)\n"
              << "  [--gpu 0|1]: host loop, or the equations on the GPU (default 1)\n"
              << "  [--pairs first:count]: only the pairs (x, y) = first .. first+count-1 of the mk.kn (a partial check)\n"
              << "  [--count]: count every violated equation (default: stop behind the first failing launch)\n";
    return -1;
}

int run(const Triple &T, uint64_t modulus, const Opts &o) {
    const size_t m = T.m, k = T.k, n = T.n, mk = m * k, kn = k * n, mn = m * n;
    const uint64_t npairs = (uint64_t)mk * kn;
    const uint64_t pair0 = o.partial ? o.first : 0, pair1 = o.partial ? o.first + o.npairs : npairs;
    if (pair0 >= pair1 || pair1 > npairs) return refuse("--pairs " + std::to_string(o.first) + ":" + std::to_string(o.npairs) + " is empty or goes beyond the " + std::to_string(npairs) + " pairs");
    const std::string field = modulus ? "Z/" + std::to_string(modulus) + "Z" : "Q";
    const std::string note = o.partial ? " [partial: pairs " + std::to_string(pair0) + " .. " + std::to_string(pair1 - 1) + " of " + std::to_string(npairs) + "]" : "";

    std::vector<uint64_t> moduli{modulus};
    if (!modulus) {
        const BrentCert c = brent_certificate(T.L, T.R, T.P);
        moduli.assign(c.primes.begin(), c.primes.end());
        std::clog << "# certificate: beta = " << c.beta << ", j = " << c.j << ", primes";
        for (uint32_t p : c.primes) std::clog << ' ' << p;
        std::clog << std::endl;
    }

    bool on_gpu = false;
    const QCsr cl = qcsr(T.L), cr = qcsr(T.R), cp = qcsr(T.P);
    HipBrent *H = nullptr;
    if (o.gpu) {
        std::string why;
        if (cl.wide || cr.wide || cp.wide) why = "a coefficient wider than 64 bits";
        else if (modulus >= (1ull << 31)) why = "a modulus of 2^31 or more";
        if (why.empty()) {
            static HipBrent lib;
            if (!lib.ok) return refuse("libplinopt_hip.so cannot be loaded or lacks plo_brent_check");   // no silent fallback
            if (lib.init(0) != PLO_OK) return refuse(lib.last_error());
            H = &lib; on_gpu = true;
        } else std::clog << "# the device refuses this input (" << why << "): host loop" << std::endl;
    }
    const plo_qcsr_t l = cl.view(), r = cr.view(), p = cp.view();

    const auto t0 = std::chrono::steady_clock::now();
    Pass total; uint64_t failed_mod = 0;
    for (const uint64_t q : moduli) {
        Pass ps;
        bool done = false;
        if (on_gpu) {
            const int rc = device_pass(*H, l, r, p, T, (uint32_t)q, pair0, pair1, o.count, ps);
            if (rc == PLO_E_CAPACITY || rc == PLO_E_UNSUPPORTED) { std::clog << "# the device refuses this input (" << H->last_error() << "): host loop" << std::endl; on_gpu = false; }
            else if (rc != PLO_OK) return refuse(H->last_error());
            else done = true;
        }
        if (!done) ps = q < (1ull << 31) ? host_pass(ZpField((uint32_t)q), T, pair0, pair1, o.count) : host_pass(Zp64Field(q), T, pair0, pair1, o.count);
        total.equations += ps.equations; total.kms += ps.kms; total.launches += ps.launches;
        if (ps.violated) { total.violated = ps.violated; total.first = ps.first; total.value = ps.value; failed_mod = q; break; }
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    if (!failed_mod) {
        size_t nnz = 0, nno = 0;
        count_entries(T, modulus, nnz, nno);
        std::clog << mm_success_line(m, k, n, nnz, nno, field, note) << std::endl;
    } else {
        std::cerr << mm_error_line(m, k, n, field + note) << std::endl;
        const uint64_t e = total.first, z = e % mn, pr = e / mn, x = pr / kn, y = pr % kn;
        const bool one = x % k == y / n && z == (x / k) * n + y % n;
        std::clog << "# first violated equation e=" << e << ": (a,b | b',c | a',c') = (" << x / k << ',' << x % k << " | " << y / n << ',' << y % n << " | " << z / n << ',' << z % n << "), sum ";
        if (modulus) std::clog << total.value;
        else {
            const QField Qf;
            try { std::clog << brent_sum(Qf, transpose(T.L), T.R, transpose(T.P), x, y, z); } catch (const std::exception &ex) { std::clog << "(" << ex.what() << ")"; }
        }
        std::clog << " instead of " << (one ? 1 : 0);
        if (!modulus) std::clog << "; modulo " << failed_mod << ": " << total.value;
        std::clog << std::endl;
        if (o.count) {
            std::clog << "# " << total.violated << " of " << (pair1 - pair0) * mn << " equations violated";
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
            else if (a == "-r") {
                need(3);
                unsigned __int128 r, e, s;
                if (!num(argv[i + 1], r) || !num(argv[i + 2], e) || !num(argv[i + 3], s)) return refuse("-r needs three natural numbers");
                i += 3;
                unsigned __int128 v = 1;
                if (r < 2) v = (r == 1 || e == 0) ? 1 : 0;                                   // 0^e and 1^e need no loop; from 2 on the guard ends it within 120 turns
                else for (unsigned __int128 t = 0; t < e; ++t) { if (v > ((unsigned __int128)1 << 120) / r) return refuse("modulus r^e - s above 2^62"); v *= r; }
                if (v <= s) return refuse("modulus r^e - s is not positive");
                o.modulus = v - s;
            }
            else if (a == "-I" || a == "-P") return refuse("polynomial quotients (" + a + ") are not supported");
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
    uint64_t modulus = 0;
    if (o.modulus > 0) {
        while (o.modulus % 2 == 0) o.modulus >>= 1;                                       // src/MMchecker.cpp:123-126
        if (o.modulus == 1) o.modulus = 2;
        if (o.modulus > ((unsigned __int128)1 << 62)) return refuse("modulus above 2^62");
        modulus = (uint64_t)o.modulus;
    }
    try {
        Triple T;
        T.L = read_file(files[0]); T.R = read_file(files[1]); T.P = read_file(files[2]);
        if (T.L.rowdim() != T.R.rowdim() || T.L.rowdim() != T.P.coldim()) {               // src/MMchecker.cpp:65-71
            std::cerr << "# \033[1;31m****** ERROR, inner dimension mismatch: " << T.L.rowdim() << "(.)" << T.R.rowdim() << '|' << T.P.coldim() << " ******\033[0m" << std::endl;
            return 2;
        }
        if (!brent_shape(T.L.coldim(), T.R.coldim(), T.P.rowdim(), T.m, T.k, T.n)) {      // include/plinopt_library.inl:487-495
            std::cerr << "# \033[1;31m****** ERROR, outer dimension mismatch: " << T.L.coldim() << ':' << T.m << 'x' << T.k << ' ' << T.R.coldim() << ':' << T.k << 'x' << T.n << ' '
                      << T.P.rowdim() << ':' << T.m << 'x' << T.n << " ******\033[0m" << std::endl;
            return 3;
        }
        if (modulus)
            for (const QMat *M : {&T.L, &T.R, &T.P}) for (const auto &row : M->rows) for (const auto &e : row)
                if (Rat::gcd(e.second.d % (__int128)modulus, (__int128)modulus) != 1)
                    return refuse("a denominator (" + std::to_string((long long)e.second.d) + ") is not invertible modulo " + std::to_string(modulus));
        return run(T, modulus, o);
    } catch (const std::exception &e) { std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m\n"; return 4; }
}
