// ==========================================================================
// bin/TPchecker -- certifies an in-place trilinear program as bin/trilplacer prints them (the reference checks these with a Maple
// session, -DINPLACE_CHECKER of include/plinopt_inplace.inl:940-1067 and bin/TTP.sh):
//   TPchecker [-e] [-m] [-q #] [--gpu 0|1] [--pairs first:count] [--count] L.sms R.sms P.sms [program.txt | stdin]
// The program must add P.((L a) o (R b)) to c and restore a and b.  For unit inputs its final state is a' = A a, b' = B b,
// c' = C c + S(a, b); every equation S[i][j][z] == sum_t L[t][i] R[t][j] P[z][t], A == I, B == I, C == I is computed
// (plo_tprog.hpp), on the GPU through plo_tprog_check of libplinopt_hip.so, and the verdict is exact.
// -e: the program is one of `trilplacer -e` (c has one more entry, the products go to the symbols low and hig).  -m: the target is
// the matrix-multiplication tensor of the shape of the three files instead of their product; -m -e is refused.
// clog/cerr: `# SUCCESS: correct in-place NAxNB->NC trilinear program (ADD|SCA|AXPY) over <field>` or
// `****** ERROR, not an in-place program of this triple over <field>******`, then the first violated equation with its block, its
// indices, the value found and the one expected, with --count the number of violated ones, and a `# GPU:` (or `# host:`) line.
// Fields: -q q is Z/qZ as given, 2 <= q <= 2^62; otherwise Q, proved from passes modulo j primes above 2^30 that divide no
// denominator (the `# certificate` line; beta bounds the bits of a cleared defect), or, where that would take more than 64
// primes, over Q on the host, which is announced.  A pass that fails is a failure over Q: its first equation is then computed
// over Q and printed as rationals besides the residues.
// --gpu 1 uses the kernels for a modulus below 2^31 and coefficients of at most 64 bits; otherwise, and with --gpu 0, the host
// loop (OpenMP over i) on the same definition, which it announces.  Without --gpu the choice is by size: the device from
// na nb (lines of c) = 4e9 on, the crossover measured, the host loop below, which it announces too; where
// the size chose the device and there is no library or no device, the host loop runs and says so.  A library that cannot be loaded is an error, never
// a reason for the host loop.  --pairs first:count checks the bilinear equations of the pairs first .. first + count - 1 only
// (the restoration blocks go with a range that starts at 0) and says so on the verdict line.
// Exit status: 0 correct, 1 not correct, 2 inner dimension mismatch, 4 for what is refused (a line outside the grammar, with its
// number; a denominator that is no unit; -m -e; an empty --pairs; unreadable input; a device error).
// ==========================================================================
#include "plo_tprog.hpp"
#include "plo_dl.hpp"
#include <chrono>

using namespace plo;

namespace {
struct HipTProg {
    void *h = open_hip_lib(); bool ok = h != nullptr;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error);
    PLO_SYM(create, plo_tprog_plan_create_q); PLO_SYM(destroy, plo_tprog_plan_destroy);
    PLO_SYM(check, plo_tprog_check); PLO_SYM(info, plo_tprog_plan_info);
};

struct Opts { int gpu = -1; bool count = false, partial = false, expanded = false, matmul = false; uint64_t first = 0, npairs = 0; unsigned __int128 modulus = 0; };

// what one pass (the range, one modulus or Q) found; value, expected: the values at `first` as text
struct Pass { uint64_t violated = 0, first = ~0ull; std::string value, expected; double kms = 0; uint32_t launches = 0; };

// na nb (lines of c) from which the device is the faster path when --gpu is not given
constexpr double TP_GPU_CROSSOVER = 4e9;

int refuse(const std::string &why) { std::cerr << "# \033[1;31mERROR: " << why << "\033[0m\n"; return 4; }

QMat read_file(const std::string &f) {
    std::ifstream in(f);
    if (!in) throw std::runtime_error("cannot read " + f);
    return read_sms(in);
}

struct Input { QMat L, R, P; TpProgram pg; TpSpec spec; };

template <class F> std::string text_of(const F &f, const typename F::Elt &e) { std::ostringstream os; f.write(os, e); return os.str(); }

template <class F> Pass host_pass(const F &f, const Input &X, uint64_t pair0, uint64_t pair1, bool count_all) {
    using M = SparseMat<typename F::Elt>;                                                  // (-m: the files give the shape only)
    const M LT = X.spec.matmul ? M() : rebind(transpose(X.L), f), R = X.spec.matmul ? M() : rebind(X.R, f), PT = X.spec.matmul ? M() : rebind(transpose(X.P), f);
    const auto found = tprog_host(f, X.spec, X.pg, LT, R, PT, pair0, pair1, count_all);
    Pass ps; ps.violated = found.violated; ps.first = found.first;
    if (found.violated) { ps.value = text_of(f, found.value); ps.expected = text_of(f, found.expected); }
    return ps;
}

int usage(const char *prg) {
    std::clog << "Usage: " << prg << " [-h] [-e] [-m] [-q #] [--gpu 0|1] [--pairs first:count] [--count] L.sms R.sms P.sms [program.txt | stdin]\n"
              << "  [-e]: the program is one of `trilplacer -e` (double-size products, split into low and hig)\n"
              << "  [-m]: the target is the matrix-multiplication tensor of the files' shape (not with -e)\n"
              << "  [-q q]: check is modulo q, taken as given (default: over Q, proved modulo primes)\n"
              << "  [--gpu 0|1]: host loop, or the equations on the GPU (default: by size)\n"
              << "  [--pairs first:count]: only the pairs (i, j) = first .. first+count-1 of the na.nb (a partial check)\n"
              << "  [--count]: print the number of violated equations\n";
    return -1;
}

int run(const Input &X, uint64_t modulus, const Opts &o) {
    const TpSpec &S = X.spec;
    const uint64_t npairs = S.npairs();
    const uint64_t pair0 = o.partial ? o.first : 0, pair1 = o.partial ? o.first + o.npairs : npairs;
    if (pair0 >= pair1 || pair1 > npairs) return refuse("--pairs " + std::to_string(o.first) + ":" + std::to_string(o.npairs) + " is empty or goes beyond the " + std::to_string(npairs) + " pairs");
    const uint64_t nequations = (pair1 - pair0) * S.w + (pair0 == 0 ? S.nequations() - S.E0() : 0);
    const QField Qf;
    const std::string field = modulus ? "Z/" + std::to_string(modulus) + "Z" : "Q";
    const std::string note = o.partial ? " [partial: pairs " + std::to_string(pair0) + " .. " + std::to_string(pair1 - 1) + " of " + std::to_string(npairs) + (pair0 ? ", no restoration block" : "") + "]" : "";

    bool over_q = false;                                                           // the whole proof over Q on the host
    std::vector<uint64_t> moduli{modulus};
    if (!modulus) {
        const BrentCert c = tprog_certificate(S, X.pg, X.L, X.R, X.P);
        if (c.j == 0) { over_q = true; std::clog << "# certificate: more than 64 primes would be needed: the proof is made over Q on the host" << std::endl; }
        else {
            moduli.assign(c.primes.begin(), c.primes.end());
            std::clog << "# certificate: beta = " << c.beta << ", j = " << c.j << ", primes";
            for (uint32_t p : c.primes) std::clog << ' ' << p;
            std::clog << std::endl;
        }
    }

    bool on_gpu = false;
    const QCsr cl = qcsr(X.L), cr = qcsr(X.R), cp = qcsr(X.P);
    std::vector<plo_tprog_rec_t> recs; bool wide = false;
    for (const TpRec &r : X.pg.recs) {
        if (r.coef.n > (__int128)INT64_MAX || r.coef.n < -(__int128)INT64_MAX || r.coef.d > (__int128)INT64_MAX) wide = true;
        recs.push_back(plo_tprog_rec_t{r.fam, r.op, r.part, 0, r.dst, r.src, r.src2, (int64_t)r.coef.n, (int64_t)r.coef.d});
    }
    HipTProg *H = nullptr;
    // --gpu not given: by size.  The host loop takes about na nb (lines of c) updates; below the crossover measured (DESIGN.md
    // 2.14: loading the library and the first launch cost a quarter of a second) it is the faster path
    size_t clines = 0;
    for (const TpRec &r : X.pg.recs) clines += r.fam == 2 ? 1 : 0;
    const double work = (double)S.na * (double)S.nb * (double)clines;
    int gpu = o.gpu;
    const bool by_size = gpu < 0;
    if (by_size) {
        double crossover = TP_GPU_CROSSOVER;
        if (const char *e = getenv("PLO_TPCHECKER_CROSSOVER")) crossover = atof(e);       // test knob: the choice on a small program
        gpu = work >= crossover ? 1 : 0;
        if (!gpu && !over_q) std::clog << "# --gpu not given: " << work << " updates are below the crossover of " << crossover << ": host loop" << std::endl;
    }
    if (gpu && !over_q) {
        std::string why;
        if (cl.wide || cr.wide || cp.wide || wide) why = "a coefficient wider than 64 bits";
        else if (modulus >= (1ull << 31)) why = "a modulus of 2^31 or more";
        if (why.empty()) {
            static HipTProg lib;
            // --gpu 1 without a library or a device is an error, never a reason for the host loop; a device that only the size
            // chose is no promise: the host loop then runs, and says so
            std::string missing;
            if (!lib.ok) missing = "libplinopt_hip.so cannot be loaded or lacks plo_tprog_check";
            else if (lib.init(0) != PLO_OK) missing = lib.last_error();
            if (missing.empty()) { H = &lib; on_gpu = true; }
            else if (!by_size) return refuse(missing);
            else std::clog << "# --gpu not given: the size asks for the device, but " << missing << ": host loop (--gpu 1 makes this an error)" << std::endl;
        } else std::clog << "# the device refuses this input (" << why << "): host loop" << std::endl;
    }
    const plo_qcsr_t l = cl.view(), r = cr.view(), p = cp.view();
    const uint32_t flags = (o.expanded ? PLO_TPROG_EXPANDED : 0u) | (o.matmul ? PLO_TPROG_MATMUL : 0u);

    const auto t0 = std::chrono::steady_clock::now();
    Pass total; uint64_t failed_mod = 0; size_t npass = 0; uint64_t done_equations = 0; bool failed = false;
    if (over_q) { total = host_pass(Qf, X, pair0, pair1, o.count); failed = total.violated != 0; done_equations = nequations; }
    else for (const uint64_t q : moduli) {
        Pass ps;
        bool done = false;
        if (on_gpu) {
            plo_tprog_plan_t *plan = nullptr;
            int rc = H->create(&l, &r, &p, recs.data(), (uint64_t)recs.size(), flags, (uint32_t)q, &plan);
            plo_brent_result_t res{}; plo_stats_t st{};
            if (rc == PLO_OK) rc = H->check(plan, pair0, pair1, &res, &st);
            if (plan) H->destroy(plan);
            if (rc == PLO_E_CAPACITY || rc == PLO_E_UNSUPPORTED) { std::clog << "# the device refuses this input (" << H->last_error() << "): host loop" << std::endl; on_gpu = false; }
            else if (rc != PLO_OK) return refuse(H->last_error());
            else {
                done = true; ps.violated = res.violated; ps.first = res.first; ps.value = std::to_string(res.value); ps.expected = std::to_string(res.expected);
                ps.kms = st.kernel_ms; ps.launches = st.launches;
            }
        }
        if (!done) ps = q < (1ull << 31) ? host_pass(ZpField((uint32_t)q), X, pair0, pair1, o.count) : host_pass(Zp64Field(q), X, pair0, pair1, o.count);
        done_equations += nequations; total.kms += ps.kms; total.launches += ps.launches;
        ++npass;
        if (!modulus) std::clog << "# pass " << npass << " of " << moduli.size() << " modulo " << q << ": " << (ps.violated ? "violated" : "no violated equation") << std::endl;
        if (ps.violated) { total.violated = ps.violated; total.first = ps.first; total.value = ps.value; total.expected = ps.expected; failed_mod = q; failed = true; break; }
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    std::ostringstream shape; shape << S.na << 'x' << S.nb << "->" << S.nc;
    if (!failed) std::clog << "# \033[1;32mSUCCESS: correct in-place " << shape.str() << " trilinear program (" << X.pg.nadd << '|' << X.pg.nsca << '|' << X.pg.naxpy << ") over " << field << note << " \033[0m" << std::endl;
    else {
        std::cerr << "# \033[1;31m****** ERROR, not an in-place program of this triple over " << field << note << "******\033[0m" << std::endl;
        const uint64_t e = total.first;
        std::clog << "# first violated equation e=" << e << ": " << tprog_where_text(S, e) << ", found ";
        if (modulus || over_q) std::clog << total.value << " instead of " << total.expected;
        else {
            try {                                                                          // that equation once more, over Q
                const uint64_t pr = e < S.E0() ? e / S.w : 0;
                const auto LT = transpose(X.L), PT = transpose(X.P);
                const auto fq = tprog_host(Qf, S, X.pg, LT, X.R, PT, pr, pr + 1, false, e);
                std::clog << fq.probe_value << " instead of " << fq.probe_expected;
            } catch (const std::exception &ex) { std::clog << "(" << ex.what() << ")"; }
            std::clog << "; modulo " << failed_mod << ": " << total.value << " instead of " << total.expected;
        }
        std::clog << std::endl;
        if (o.count) {
            std::clog << "# " << total.violated << " of " << nequations << " equations violated";
            if (failed_mod && !modulus) std::clog << " modulo " << failed_mod << " (no more than over Q)";
            std::clog << std::endl;
        }
    }
    char rate[64]; snprintf(rate, sizeof rate, "%.4g", dt > 0 ? (double)done_equations / dt : 0.0);
    std::clog << "# " << (on_gpu ? "GPU" : "host") << ": " << done_equations << " equations in " << dt << " s, " << rate << " equations/s";
    if (on_gpu) std::clog << " (kernel " << total.kms << " ms, " << total.launches << " launches)";
    std::clog << std::endl;
    return failed ? 1 : 0;
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
            else if (a == "-e") o.expanded = true;
            else if (a == "-m") o.matmul = true;
            else if (a == "-q") { need(1); if (!num(argv[++i], o.modulus)) return refuse("modulus " + std::string(argv[i]) + " is not a natural number below 2^120"); if (o.modulus == 0) return refuse("modulus 0"); }
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
    if (files.size() != 3 && files.size() != 4) return usage(argv[0]);
    if (o.matmul && o.expanded) return refuse("-m -e: the expanded programs have no matrix-multiplication target");
    if (o.modulus == 1) return refuse("modulus 1");
    if (o.modulus > ((unsigned __int128)1 << 62)) return refuse("modulus above 2^62");
    const uint64_t modulus = (uint64_t)o.modulus;                                          // taken as given; 0: Q
    try {
        Input X;
        X.L = read_file(files[0]); X.R = read_file(files[1]); X.P = read_file(files[2]);
        if (X.L.rowdim() != X.R.rowdim() || X.L.rowdim() != X.P.coldim()) {
            std::cerr << "# \033[1;31m****** ERROR, inner dimension mismatch: " << X.L.rowdim() << "(.)" << X.R.rowdim() << '|' << X.P.coldim() << " ******\033[0m" << std::endl;
            return 2;
        }
        try {
            X.spec = tprog_spec(X.L.coldim(), X.R.coldim(), X.P.rowdim(), o.expanded, o.matmul);
            if (files.size() == 4) {
                std::ifstream in(files[3]);
                if (!in) return refuse("cannot read " + files[3]);
                X.pg = parse_tprog(in, X.spec.na, X.spec.nb, X.spec.nc, o.expanded);
            } else X.pg = parse_tprog(std::cin, X.spec.na, X.spec.nb, X.spec.nc, o.expanded);
        } catch (const TpRefused &e) { return refuse(e.what()); }
        if (modulus) {
            auto unit = [&](__int128 v) { return Rat::gcd(v % (__int128)modulus, (__int128)modulus) == 1; };
            if (!o.matmul) for (const QMat *M : {&X.L, &X.R, &X.P}) for (const auto &row : M->rows) for (const auto &e : row)
                if (!unit(e.second.d)) return refuse("a denominator (" + std::to_string((long long)e.second.d) + ") is not invertible modulo " + std::to_string(modulus));
            for (const TpRec &r : X.pg.recs)
                if (!unit(r.coef.d)) return refuse("line " + std::to_string(r.line) + ": a denominator (" + std::to_string((long long)r.coef.d) + ") is not invertible modulo " + std::to_string(modulus));
        }
        return run(X, modulus, o);
    } catch (const std::exception &e) { std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m\n"; return 4; }
}
