// ==========================================================================
// bin/inplacer -- in-place linear programs (reference src/inplacer.cpp:38-146):
//   inplacer [L.sms ...] [-t] [-O #] [--seed s] [--gpu 0|1|N]
// stdout = input2Temps then the program with its outputs (Pprint, include/plinopt_inplace.inl:163-175),
// clog = '#' statistics (ADD / SCA / ROWS, src/inplacer.cpp:75-79).  Several files are handled one
// after another; without a file the matrix is read from stdin.  -t: the program of the transposed
// matrix, reading the inputs t# (src/inplacer.cpp:42-58).
// The restart loop of SearchLinearAlgorithm (:621-669) runs on the GPU through plo_lin_search[_multi]
// of libplinopt_hip.so; the winner is replayed on the host over Q to print it.  --gpu 0, or an input the
// device refuses (a row of more than 64 entries, a program that does not fit LDS, a coefficient wider
// than 64 bits), uses the host loop (OpenMP).
// Testing aids: --costs prints the per-seed counts of the host (the candidate BASE_SEED, then seeds
// s .. s+O-1: ADD SCA ROWS of variant 0, then of variant 1); --candidate s v prints the program of one
// candidate (s = base: the unpermuted oriented program) without a search.
// ==========================================================================
#include "plo_inplace.hpp"
#include "plo_dl.hpp"
#include <chrono>
#include <fstream>
#include <tuple>

using namespace plo;

namespace {
struct HipLin {
    void *h = open_hip_lib(); bool ok = h != nullptr;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error);
    PLO_SYM(create, plo_lin_plan_create_q); PLO_SYM(destroy, plo_lin_plan_destroy);
    PLO_SYM(search, plo_lin_search); PLO_SYM(search_multi, plo_lin_search_multi);
};

bool better(const Tricount &l, const Tricount &r) { return l[0] < r[0] || (l[0] == r[0] && l[1] < r[1]); }   // :637-641, :655-659

struct Opts { size_t loops = 30; uint64_t seed0 = 0; int gpu = 1; bool transposed = false, costs = false, cand = false; uint64_t cseed = 0; int cvar = 0; };

void tri(std::ostream &os, const Tricount &t) { os << t[0] << ' ' << t[1] << ' ' << t[2]; }

// FindProgram (src/inplacer.cpp:38-80) on one matrix; returns the exit status
int find_program(std::istream &in, const Opts &o) {
    const QMat M = read_sms(in);
    const QMat A = o.transposed ? transpose(M) : M;                          // :54-58
    const size_t ntemps = o.transposed ? M.rowdim() : M.coldim();              // outdim of :43
    const char inchar = o.transposed ? 't' : 'i';
    std::clog << std::string(40, '#') << std::endl;
    if (o.costs) {
        auto line = [&](uint64_t s) { LinCandidate c = lin_candidate(A, s); if (s == ~0ull) std::cout << "base"; else std::cout << s; std::cout << ' '; tri(std::cout, c.ops[0]); std::cout << ' '; tri(std::cout, c.ops[1]); std::cout << '\n'; };
        line(~0ull);
        for (uint64_t k = 0; k < o.loops; ++k) line(o.seed0 + k);
        return 0;
    }
    if (o.cand) {
        LinCandidate c = lin_candidate(A, o.cseed);
        std::cout << lin_text(c, o.cvar, ntemps, inchar) << std::flush;
        std::clog << "# candidate " << o.cseed << " variant " << o.cvar << ": "; tri(std::clog, c.ops[o.cvar]); std::clog << std::endl;
        return 0;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const LinCandidate basec = lin_candidate(A, ~0ull);
    Tricount best = basec.ops[0]; uint64_t bseed = ~0ull; int bvar = 0;
    std::clog << "# Oriented number of operations: " << best[0] << '|' << best[1] << '|' << best[2] << std::endl;
    bool on_gpu = false; double kms = 0;
    if (o.loops > 0) {
        using Key = std::tuple<size_t, size_t, uint64_t, int>;          // (ADD, SCA, seed, variant): the order of :637-641 made total
        // the restarts on the host: best of the loop under Key
        auto host_loop = [&](uint64_t s0, uint64_t cnt) {
            Key lb{~(size_t)0, ~(size_t)0, 0, 0};
            #pragma omp parallel
            {
                Key tb = lb;
                #pragma omp for schedule(dynamic, 16)
                for (long long k = 0; k < (long long)cnt; ++k) {
                    const LinCandidate c = lin_candidate(A, s0 + (uint64_t)k);
                    for (int v = 0; v < 2; ++v) tb = std::min(tb, Key{c.ops[v][0], c.ops[v][1], s0 + (uint64_t)k, v});
                }
                #pragma omp critical
                lb = std::min(lb, tb);
            }
            return lb;
        };
        const QCsr ca = qcsr(A);
        bool refused = ca.wide;
        std::string why = "a coefficient wider than 64 bits";
        if (o.gpu && !ca.wide) {
            HipLin L;
            if (!L.ok) { std::cerr << "# \033[1;31mERROR: libplinopt_hip.so cannot be loaded or lacks plo_lin_search\033[0m\n"; return 2; }   // no silent fallback: --gpu 0 selects the host loop
            const plo_qcsr_t a = ca.view();
            plo_lin_best_t r{}; plo_stats_t st{};
            int rc;
            if (o.gpu >= 2) {
                // --gpu N: N contiguous seed shards over N devices from this process, the minimum by RCCL MIN all-reduces
                std::vector<int> devs((size_t)o.gpu); for (int k = 0; k < o.gpu; ++k) devs[(size_t)k] = shard_device(k);
                rc = L.search_multi(&a, o.seed0, o.loops, o.gpu, devs.data(), &r, &st);
            } else {
                rc = L.init(0);
                plo_lin_plan_t *plan = nullptr;
                if (rc == PLO_OK) rc = L.create(&a, &plan);
                if (rc == PLO_OK) { rc = L.search(plan, o.seed0, o.loops, &r, &st); L.destroy(plan); }
            }
            if (rc == PLO_E_UNSUPPORTED || rc == PLO_E_CAPACITY) { refused = true; why = L.last_error(); }
            else if (rc != PLO_OK) { std::cerr << "# \033[1;31mERROR: " << L.last_error() << "\033[0m\n"; return 2; }
            else {
                on_gpu = true; kms = st.kernel_ms;
                if (o.gpu >= 2) std::clog << "# " << o.gpu << " shards (one GPU and one host thread each, one process)" << std::endl;
                const Tricount g{r.add, r.sca, r.rows};
                if (better(g, best)) { best = g; bseed = r.seed; bvar = (int)r.variant; }
            }
        }
        if (!o.gpu || refused) {
            if (o.gpu) std::clog << "# the device refuses this matrix (" << why << "): host search" << std::endl;
            // best of the loop under (ADD, SCA, seed, variant), then strictly better than the unpermuted program
            const Key lb = host_loop(o.seed0, o.loops);
            const Tricount g{std::get<0>(lb), std::get<1>(lb), A.rowdim() * (size_t)(std::get<3>(lb) + 1)};
            if (better(g, best)) { best = g; bseed = std::get<2>(lb); bvar = std::get<3>(lb); }
        }
    }
    // replay of the winner for the text
    std::string text;
    if (bseed == ~0ull) text = lin_text(basec, 0, ntemps, inchar);
    else {
        const LinCandidate w = lin_candidate(A, bseed);
        if (w.ops[bvar] != best) { std::cerr << "# \033[1;31mERROR: replay of seed " << bseed << " gives " << w.ops[bvar][0] << '|' << w.ops[bvar][1] << ", search said " << best[0] << '|' << best[1] << "\033[0m\n"; return 3; }
        text = lin_text(w, bvar, ntemps, inchar);
        std::clog << "# Found " << (bvar ? "oriented (appended)" : "unoriented") << " [seed " << bseed << "], operations: " << best[0] << '|' << best[1] << '|' << best[2] << std::endl;
    }
    std::cout << text << std::flush;
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::clog << std::string(40, '#') << std::endl;                            // :75-79
    std::clog << "# \033[1;32m" << best[0] << "\tADD\033[0m\n# \033[1;32m" << best[1] << "\tSCA\033[0m\n# \033[1;32m" << best[2] << "\tROWS\033[0m\n";
    std::clog << std::string(40, '#') << std::endl;
    std::clog << "# " << o.loops << " restarts on " << (on_gpu ? "GPU" : "host") << " in " << dt << " s";
    if (on_gpu) std::clog << " (kernel " << kms << " ms)";
    std::clog << std::endl;
    return 0;
}
} // namespace

int main(int argc, char **argv) {
    cap_omp_threads();
    Opts o; std::vector<std::string> files;
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        if (a == "-h") {
            std::clog << "Usage: " << argv[0] << " [L.sms ...] [-t] [-O #] [--seed s] [--gpu 0|1|N: N >= 2 shards the restarts over N GPUs]\n"
                      << "  -t  : produces an in-place program for the transposed matrix\n"
                      << "  -O #: randomized search with that many loops (default " << o.loops << " loops)\n"
                      << "  testing aids: --costs (per-seed counts on the host), --candidate s|base v (the program of one candidate)\n";
            return 0;
        }
        else if (a == "-t") o.transposed = true;
        else if (a == "-O" && i + 1 < argc) o.loops = (size_t)atoll(argv[++i]);
        else if (a == "--seed" && i + 1 < argc) o.seed0 = strtoull(argv[++i], nullptr, 10);
        else if (a == "--gpu" && i + 1 < argc) o.gpu = atoi(argv[++i]);
        else if (a == "--costs") o.costs = true;
        else if (a == "--candidate" && i + 2 < argc) {
            const std::string s(argv[++i]);
            o.cand = true; o.cseed = s == "base" ? ~0ull : strtoull(s.c_str(), nullptr, 10); o.cvar = atoi(argv[++i]) ? 1 : 0;
        }
        else files.push_back(a);
    }
    try {
        if (files.empty()) return find_program(std::cin, o);
        for (const auto &f : files) {
            std::ifstream in(f);
            if (!in) { std::cerr << "# \033[1;31mERROR: cannot read " << f << "\033[0m\n"; return -1; }
            if (const int rc = find_program(in, o)) return rc;
        }
    } catch (const std::exception &e) { std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m\n"; return 4; }
    return 0;
}
