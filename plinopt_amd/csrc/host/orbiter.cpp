// ==========================================================================
// bin/orbiter -- the De Groote orbit search of a matrix-multiplication triple (reference src/orbiter.cpp):
//   orbiter [-b bits] [-m|-q mod] [-r r e s] [-s|-c|-z|-g] [--sub n] [-O loops] [--seed s] [--gpu 0|1|N] [--action a] L.sms R.sms P.sms
// Searches the candidates (U, V, W) s .. s+O-1 (plo_orbit_*, include/plinopt_hip.h) for an equivalent triple with a smaller
// (cost, nnz, nno); when the best one improves on the input, writes <L>.nnz.sms, <R>.nnz.sms, <P>.nnz.sms next to the inputs.
// clog: the reference's '#' lines (Init. ops, Search(N), Rdcd. opt) and the exact matrix-multiplication checks of the input
// (printed, then ignored, as the reference does) and of the winner; stdout: one line `winner <cost> <nnz> <nno> <seed|base>`.
// Fields: Q (default), or Z_mod with -m/-q/-r (factors 2 removed from the modulus, 1 becomes 2; the measure is then density, or -z).
// -z (reference :172-209, PLO_ORBIT_CSE) scores a candidate by the operations of the best programs CSEOptimiser finds for its three
// matrices: min(naiveOps, the best of `sub` Optimizer runs) per matrix, sub = loops >> 4 above 16 loops, else 1 (:257), or --sub n;
// the Optimizer streams are seeds 0 .. sub-1 for every candidate.  It needs a prime modulus (-q 2147483629 stands for Q).
// -g (PLO_ORBIT_GROWTH) scores a candidate by the 2-norm growth factor of its triple, the G2 of bin/growthfactor, over Q with the
// triangular or the PLUQ action (Householder matrices are orthogonal and keep it): the search for a more accurate equivalent algorithm.
// Its cost is a double: six decimals on the '#' lines, 17 significant digits on stdout (`winner`, --costs), which determine its bits.
// The restarts run on the GPU through plo_orbit_search[_multi] of libplinopt_hip.so; --gpu 0, or an input the device refuses
// (a modulus of 2^31 or more, a Q input outside its int64 bound, sizes beyond its limits), uses the host loop (OpenMP) and
// says so.  -b is accepted for the reference's command lines: the checks here are exact.
// --action triangular|pluq|householder chooses how U, V and W are drawn (PLO_ORBIT_ACT_*; the reference's compile-time
// ACTION_FULL_PLUQ and ACTION_HOUSEHOLDER, src/orbiter.cpp:77-123), for the search, --costs and --candidate alike.
// Refused with status 2: -g with a modulus, with -z or with --action householder, -z over Q or modulo a composite number, -P/-I, shapes that are not mk, kn, mn, a denominator that is no unit modulo the modulus, a
// modulus above 2^63.  Testing aids: --costs prints `cost nnz nno` of the base candidate, then of seeds s .. s+O-1 (host);
// --candidate s|base DIR writes the three matrices of one candidate to DIR/{L,R,P}.sms.
// ==========================================================================
#include "plo_orbit.hpp"
#include "plo_brent.hpp"
#include "plo_dl.hpp"
#include <chrono>
#include <filesystem>

using namespace plo;

namespace {
struct HipOrbit {
    void *h = open_hip_lib(); bool ok = h != nullptr;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error);
    PLO_SYM(create, plo_orbit_plan_create_act); PLO_SYM(destroy, plo_orbit_plan_destroy);
    PLO_SYM(search, plo_orbit_search); PLO_SYM(search_multi, plo_orbit_search_multi_act);
    PLO_SYM(create_cse, plo_orbit_plan_create_cse); PLO_SYM(search_multi_cse, plo_orbit_search_multi_cse);
    PLO_SYM(create_growth, plo_orbit_plan_create_growth); PLO_SYM(search_growth, plo_orbit_growth_search); PLO_SYM(search_multi_growth, plo_orbit_growth_search_multi);
};

struct Opts {
    size_t loops = 100; uint64_t seed0 = 0; int gpu = 1; int measure = ORBIT_DENSITY; int action = ORBIT_ACT_TRIANGULAR; bool cse = false, growth = false;
    unsigned __int128 modulus = 0; bool costs = false, cand = false; uint64_t cseed = 0; std::string cdir;
    size_t sub = 0;                                                                       // --sub; 0: the reference's loops >> 4
};

// a cost as the tool prints it: a count, or with -g the growth factor held as its bits (six decimals, or 17 significant digits)
std::string cost_text(int measure, size_t cost, bool exact = false) {
    if (measure != ORBIT_GROWTH) return std::to_string(cost);
    char t[64]; snprintf(t, sizeof t, exact ? "%.17g" : "%.6f", growth_value(cost));
    return t;
}

std::string nnz_name(const std::string &f) { return std::filesystem::path(f).replace_extension(".nnz.sms").string(); }

template <class F> void write_triple(const F &f, const OrbitTriple<F> &T, const std::string &l, const std::string &r, const std::string &p, char ty) {
    std::ofstream ol(l), orr(r), op(p);
    write_sms(ol, f, T.L, ty); write_sms(orr, f, T.R, ty); write_sms(op, f, transpose(T.PT), ty);
}

// MMchecker (include/plinopt_library.inl:473-549), exact: prints the reference's verdict line, returns 0 when correct
template <class F> int mm_report(const F &f, const OrbitTriple<F> &T) {
    bool ok = false; std::string why;
    try { ok = orbit_mm_check(f, T); } catch (const std::exception &e) { why = e.what(); }
    if (ok) {
        OrbitCount c = orbit_candidate(f, T, ORBIT_BASE, ORBIT_DENSITY, ORBIT_ACT_TRIANGULAR, OrbitCse());
        std::clog << mm_success_line(T.m, T.k, T.n, c.nnz, c.nno, f.name()) << std::endl;          // (the wording is bin/MMchecker's too: plo_brent.hpp)
        return 0;
    }
    std::cerr << mm_error_line(T.m, T.k, T.n, f.name(), why) << std::endl;
    return 1;
}

template <class F> int orbit_run(const F &f, const QMat &QL, const QMat &QR, const QMat &QP, size_t m, size_t k, size_t n, uint64_t modulus, const Opts &o,
                                 const std::vector<std::string> &files) {
    OrbitTriple<F> T;
    T.L = rebind(QL, f); T.R = rebind(QR, f); T.PT = rebind(transpose(QP), f); T.m = m; T.k = k; T.n = n;
    const int measure = o.cse ? ORBIT_CSE : o.growth ? ORBIT_GROWTH : modulus ? ORBIT_DENSITY : o.measure;
    const OrbitCse z{o.sub ? o.sub : (o.loops > 16 ? o.loops >> 4 : 1), 0};                // :257
    if (o.costs) {
        auto line = [&](uint64_t s) { const OrbitCount c = orbit_candidate(f, T, s, measure, o.action, z); std::cout << cost_text(measure, c.cost, true) << ' ' << c.nnz << ' ' << c.nno << '\n'; };
        line(ORBIT_BASE);
        for (uint64_t j = 0; j < o.loops; ++j) line(o.seed0 + j);
        return 0;
    }
    if (o.cand) {
        OrbitTriple<F> C; const OrbitCount c = orbit_candidate(f, T, o.cseed, measure, o.action, &C, z);
        std::filesystem::create_directories(o.cdir);
        write_triple(f, C, o.cdir + "/L.sms", o.cdir + "/R.sms", o.cdir + "/P.sms", modulus ? 'M' : 'R');
        std::clog << "# candidate " << (o.cseed == ORBIT_BASE ? std::string("base") : std::to_string(o.cseed)) << ": " << cost_text(measure, c.cost, true) << ' ' << c.nnz << ' ' << c.nno << std::endl;
        return 0;
    }
    const int input_bad = mm_report(f, T);                                               // :263, printed then ignored
    const OrbitCount init = orbit_candidate(f, T, ORBIT_BASE, measure, o.action, z);
    std::clog << "# Init. ops: " << cost_text(measure, init.cost) << ", (" << init.nnz << ',' << init.nno << ')' << std::endl;
    const auto t0 = std::chrono::steady_clock::now();
    using Key = std::tuple<size_t, size_t, size_t, uint64_t>;                             // (cost, nnz, nno, seed)
    Key best{~(size_t)0, 0, 0, 0};
    bool on_gpu = false, have = false; double kms = 0;
    if (o.loops > 0) {
        bool refused = false; std::string why;
        if (o.gpu) {
            const QCsr cl = qcsr(QL), cr = qcsr(QR), cp = qcsr(QP);
            refused = cl.wide || cr.wide || cp.wide; why = "a coefficient wider than 64 bits";
            if (!refused && o.cse && modulus >= (1ull << 31)) { refused = true; why = "-z modulo a prime of 2^31 or more"; }
            if (!refused) {
                HipOrbit H;
                if (!H.ok) { std::cerr << "# \033[1;31mERROR: libplinopt_hip.so cannot be loaded or lacks plo_orbit_search\033[0m\n"; return 2; }   // no silent fallback
                const plo_qcsr_t l = cl.view(), r = cr.view(), p = cp.view();
                plo_stats_t st{}; Key dbest{};
                // The device search of one measure, whose best is a Best and whose order is keyof(best), then the seed: `multi` over o.gpu
                // shards, or one plan of `create` searched in pieces (a launch takes at most 2^31-1 candidates; minimum under the same order)
                auto device = [&](auto zero, auto multi, auto create, auto search, auto keyof) {
                    decltype(zero) b{};
                    int rc;
                    if (o.gpu >= 2) {
                        std::vector<int> devs((size_t)o.gpu); for (int j = 0; j < o.gpu; ++j) devs[(size_t)j] = shard_device(j);
                        rc = multi(devs.data(), &b, &st);
                    } else {
                        rc = H.init(0);
                        plo_orbit_plan_t *plan = nullptr;
                        if (rc == PLO_OK) rc = create(&plan);
                        for (uint64_t done = 0; rc == PLO_OK && done < o.loops;) {
                            const uint64_t piece = std::min<uint64_t>(o.loops - done, (1ull << 31) - 1ull);
                            decltype(zero) pb{}; plo_stats_t ps{};
                            rc = search(plan, o.seed0 + done, piece, &pb, &ps);
                            if (rc != PLO_OK) break;
                            if (done == 0 || keyof(pb) < keyof(b)) b = pb;
                            st.kernel_ms += ps.kernel_ms;
                            done += piece;
                        }
                        if (plan) H.destroy(plan);
                    }
                    if (rc == PLO_OK) dbest = std::tuple_cat(keyof(b), std::make_tuple((uint64_t)b.seed));
                    return rc;
                };
                const int rc = o.growth
                    ? device(plo_orbit_gbest_t{},
                             [&](const int *devs, plo_orbit_gbest_t *b, plo_stats_t *s) { return H.search_multi_growth(&l, &r, &p, o.action, o.seed0, o.loops, o.gpu, devs, b, s); },
                             [&](plo_orbit_plan_t **plan) { return H.create_growth(&l, &r, &p, o.action, plan); }, H.search_growth,
                             [](const plo_orbit_gbest_t &x) { return std::make_tuple(growth_bits(x.cost), (size_t)x.nnz, (size_t)x.nno); })
                    : device(plo_orbit_best_t{},
                             [&](const int *devs, plo_orbit_best_t *b, plo_stats_t *s) {
                                 return o.cse ? H.search_multi_cse(&l, &r, &p, modulus, o.action, (uint32_t)z.sub, z.seed0, o.seed0, o.loops, o.gpu, devs, b, s)
                                              : H.search_multi(&l, &r, &p, modulus, measure, o.action, o.seed0, o.loops, o.gpu, devs, b, s); },
                             [&](plo_orbit_plan_t **plan) { return o.cse ? H.create_cse(&l, &r, &p, modulus, o.action, (uint32_t)z.sub, z.seed0, plan) : H.create(&l, &r, &p, modulus, measure, o.action, plan); },
                             H.search, [](const plo_orbit_best_t &x) { return std::make_tuple((size_t)x.cost, (size_t)x.nnz, (size_t)x.nno); });
                if (rc == PLO_E_UNSUPPORTED || rc == PLO_E_CAPACITY) { refused = true; why = H.last_error(); }
                else if (rc != PLO_OK) { std::cerr << "# \033[1;31mERROR: " << H.last_error() << "\033[0m\n"; return 2; }
                else {
                    on_gpu = true; kms = st.kernel_ms; have = true;
                    if (o.gpu >= 2) std::clog << "# " << o.gpu << " shards (one GPU and one host thread each, one process)" << std::endl;
                    best = dbest;
                }
            }
        }
        if (!o.gpu || refused) {
            if (o.gpu) std::clog << "# the device refuses this input (" << why << "): host search" << std::endl;
            Key lb = best;
            std::string err;
            #pragma omp parallel
            {
                Key tb = lb;
                #pragma omp for schedule(dynamic, 16)
                for (long long j = 0; j < (long long)o.loops; ++j) {
                    try {
                        const OrbitCount c = orbit_candidate(f, T, o.seed0 + (uint64_t)j, measure, o.action, z);
                        tb = std::min(tb, Key{c.cost, c.nnz, c.nno, o.seed0 + (uint64_t)j});
                    } catch (const std::exception &e) {
                        #pragma omp critical
                        err = e.what();
                    }
                }
                #pragma omp critical
                lb = std::min(lb, tb);
            }
            if (!err.empty()) throw std::runtime_error(err);                               // Q: an overflow is an error
            best = lb; have = true;
        }
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::clog << "# Search(" << o.loops << "): " << dt << "s" << std::endl;
    const OrbitCount bc{std::get<0>(best), std::get<1>(best), std::get<2>(best)};
    const bool improved = have && bc < init;
    if (improved) {
        const uint64_t seed = std::get<3>(best);
        OrbitTriple<F> W;
        const OrbitCount rc = orbit_candidate(f, T, seed, measure, o.action, &W, z);
        if (!(rc == bc)) {
            std::cerr << "# \033[1;31mERROR: replay of seed " << seed << " gives " << cost_text(measure, rc.cost, true) << ' ' << rc.nnz << ' ' << rc.nno << ", search said " << cost_text(measure, bc.cost, true) << ' ' << bc.nnz << ' ' << bc.nno << "\033[0m\n";
            return 3;
        }
        std::clog << "# \033[1;36mRdcd. opt: " << cost_text(measure, bc.cost) << '<' << cost_text(measure, init.cost) << "\t(" << bc.nnz << ',' << bc.nno << ")\033[0m" << std::endl;
        const int winner_bad = mm_report(f, W);
        if (winner_bad && !input_bad) { std::cerr << "# \033[1;31mERROR: the winner of a correct input fails the check: nothing written\033[0m\n"; return 3; }
        write_triple(f, W, nnz_name(files[0]), nnz_name(files[1]), nnz_name(files[2]), modulus ? 'M' : 'R');
        std::cout << "winner " << cost_text(measure, bc.cost, true) << ' ' << bc.nnz << ' ' << bc.nno << ' ' << seed << std::endl;
    } else {
        std::cout << "winner " << cost_text(measure, init.cost, true) << ' ' << init.nnz << ' ' << init.nno << " base" << std::endl;
    }
    std::clog << "# " << o.loops << " restarts on " << (on_gpu ? "GPU" : "host") << " in " << dt << " s";
    if (on_gpu) std::clog << " (kernel " << kms << " ms)";
    if (o.cse) std::clog << ", " << o.loops * 3 * z.sub << " Optimizer runs (sub " << z.sub << ")";
    std::clog << std::endl;
    return 0;
}

int refuse(const std::string &why) { std::cerr << "# \033[1;31mERROR: " << why << "\033[0m\n"; return 2; }

QMat read_file(const std::string &f) {
    std::ifstream in(f);
    if (!in) throw std::runtime_error("cannot read " + f);
    return read_sms(in);
}

int usage(const char *prg, const Opts &o) {
    std::clog << "Usage: " << prg << " [-b #] [-m|-q #] [-r # # #] [-s|-c|-z|-g] [--sub #] [-O #] [--seed s] [--gpu 0|1|N] [--action a] L.sms R.sms P.sms\n"
              << "  [-b b]: accepted (the matrix-multiplication checks are exact)\n"
              << "  [-m/-q m]: search modulo m without its factors 2 (default Q)\n"
              << "  [-r r e s]: search modulo (r^e-s) without its factors 2\n"
              << "  [-s|-c]: search sparser|canonical (default sparser; always sparser modulo a number)\n"
              << "  [-z]: search faster: the operations of the best programs found (needs a prime modulus; -q 2147483629 stands for Q)\n"
              << "  [-g]: search more accurate: the 2-norm growth factor (over Q; triangular or pluq action)\n"
              << "  [--sub n]: Optimizer runs per matrix with -z (default loops/16, at least 1)\n"
              << "  [-O #]: randomized search with that many loops (default " << o.loops << " loops)\n"
              << "  [--seed s]: candidates s .. s+O-1 (default 0); [--gpu 0|1|N]: host loop, one GPU, N GPU shards (default 1)\n"
              << "  [--action triangular|pluq|householder]: how U, V and W are drawn (default triangular)\n"
              << "  testing aids: --costs (per-seed counts on the host), --candidate s|base DIR (one candidate's matrices)\n";
    return -1;
}
} // namespace

int main(int argc, char **argv) {
    cap_omp_threads();
    Opts o; std::vector<std::string> files;
    auto num = [](const char *s, unsigned __int128 &v) {                                   // a natural number, false above 2^127
        v = 0; if (!*s) return false;
        for (; *s; ++s) { if (!isdigit((unsigned char)*s) || v > ((unsigned __int128)1 << 120)) return false; v = v * 10 + (unsigned)(*s - '0'); }
        return true;
    };
    try {
        for (int i = 1; i < argc; ++i) {
            const std::string a(argv[i]);
            auto need = [&](int c) { if (i + c >= argc) throw std::invalid_argument("option " + a + " needs " + std::to_string(c) + " argument(s)"); };
            if (a == "-h") return usage(argv[0], o);
            else if (a == "-b") { need(1); ++i; }
            else if (a == "-m" || a == "-q") { need(1); if (!num(argv[++i], o.modulus)) return refuse("modulus " + std::string(argv[i]) + " is not a natural number below 2^120"); }
            else if (a == "-r") {
                need(3);
                unsigned __int128 r, e, s;
                if (!num(argv[i + 1], r) || !num(argv[i + 2], e) || !num(argv[i + 3], s)) return refuse("-r needs three natural numbers");
                i += 3;
                unsigned __int128 v = 1;
                for (unsigned __int128 t = 0; t < e; ++t) { if (r && v > ((unsigned __int128)1 << 120) / r) return refuse("modulus r^e - s above 2^63"); v *= r; }
                if (v <= s) return refuse("modulus r^e - s is not positive");
                o.modulus = v - s;
            }
            else if (a == "-I" || a == "-P") return refuse("polynomial quotients (" + a + ") are not supported");
            else if (a == "-O") { need(1); o.loops = (size_t)strtoull(argv[++i], nullptr, 10); }
            else if (a == "-s") { o.measure = ORBIT_DENSITY; o.cse = false; }
            else if (a == "-c") { o.measure = ORBIT_CANONICAL; o.cse = false; }
            else if (a == "-z") o.cse = true;
            else if (a == "-g") o.growth = true;
            else if (a == "--sub") { need(1); o.sub = (size_t)strtoull(argv[++i], nullptr, 10); if (o.sub == 0 || o.sub > 65536) return refuse("--sub needs a number in 1 .. 65536"); }
            else if (a == "--seed") { need(1); o.seed0 = strtoull(argv[++i], nullptr, 10); }
            else if (a == "--gpu") { need(1); o.gpu = atoi(argv[++i]); }
            else if (a == "--action") {
                need(1); const std::string w(argv[++i]);
                if (w == "triangular") o.action = ORBIT_ACT_TRIANGULAR; else if (w == "pluq") o.action = ORBIT_ACT_PLUQ;
                else if (w == "householder") o.action = ORBIT_ACT_HOUSEHOLDER; else return refuse("unknown action " + w + " (triangular, pluq or householder)");
            }
            else if (a == "--costs") o.costs = true;
            else if (a == "--candidate") { need(2); const std::string s(argv[++i]); o.cand = true; o.cseed = s == "base" ? ORBIT_BASE : strtoull(s.c_str(), nullptr, 10); o.cdir = argv[++i]; }
            else if (!a.empty() && a[0] == '-') return refuse("unknown option " + a);
            else files.push_back(a);
        }
    } catch (const std::invalid_argument &e) { return refuse(e.what()); }
    if (files.size() != 3) return usage(argv[0], o);
    uint64_t modulus = 0;
    if (o.modulus > 0) {
        while (o.modulus % 2 == 0) o.modulus >>= 1;                                       // :422-423
        if (o.modulus == 1) o.modulus = 2;
        if (o.modulus > ((unsigned __int128)1 << 63)) return refuse("modulus above 2^63");
        modulus = (uint64_t)o.modulus;
    }
    if (o.growth && o.modulus > 0) return refuse("-g (the 2-norm growth factor) is defined over Q only: not with -m, -q or -r");
    if (o.growth && o.cse) return refuse("-g and -z are two measures: choose one");
    if (o.growth && o.action == ORBIT_ACT_HOUSEHOLDER) return refuse("-g with --action householder: an orthogonal action preserves the 2-norm growth factor, there is nothing to search");
    if (o.cse && !modulus) return refuse("-z (CSE counts per candidate) is not supported over Q");
    if (o.cse && !is_prime(modulus)) return refuse("-z needs a prime modulus, " + std::to_string(modulus) + " is composite");
    try {
        const QMat L = read_file(files[0]), R = read_file(files[1]), P = read_file(files[2]);
        size_t m = 0, k = 0, n = 0;
        if (!orbit_shape(L.rowdim(), L.coldim(), R.rowdim(), R.coldim(), P.rowdim(), P.coldim(), m, k, n))
            return refuse("shapes " + std::to_string(L.rowdim()) + 'x' + std::to_string(L.coldim()) + ", " + std::to_string(R.rowdim()) + 'x' + std::to_string(R.coldim()) + ", " +
                          std::to_string(P.rowdim()) + 'x' + std::to_string(P.coldim()) + " are not r x mk, r x kn, mn x r");
        if (modulus)
            for (const QMat *M : {&L, &R, &P}) for (const auto &row : M->rows) for (const auto &e : row)
                if (Rat::gcd(e.second.d % (__int128)modulus, (__int128)modulus) != 1)
                    return refuse("a denominator (" + std::to_string((long long)e.second.d) + ") is not invertible modulo " + std::to_string(modulus));
        if (!modulus) return orbit_run(QField{}, L, R, P, m, k, n, 0, o, files);
        if (modulus < (1ull << 31)) return orbit_run(ZpField((uint32_t)modulus), L, R, P, m, k, n, modulus, o, files);
        return orbit_run(Zp64Field(modulus), L, R, P, m, k, n, modulus, o, files);
    } catch (const std::exception &e) { std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m\n"; return 4; }
}
