// ===========================================================================
// bin/pruner -- re-optimizes the sub-programs of a straight-line program: what the reference's bin/prune.sh does by
// calling bin/mirabelle.sh (its first, "D", attempt) for every temporary variable or every ordered pair of them, as one
// tool.  For each selection the window around it is cut out of the program, turned into a small matrix, searched by N
// restarts of Optimizer (-D), of the kernel method (-K) and of the LU chain (-G), and reported when the best sub-program
// found is cheaper than the lines it came from.  DESIGN.md 2.11 has the definition and the departures from the scripts.
// With no method flag the methods are -D -G (the reference's mirabelle.sh runs optimizer's default, -D -K -G).
//
//   pruner [-O N] [-q p] [-v] [-l regex] [-D] [-K] [-G] [--seed S] [--gpu 0|1] [--apply] P.slp
//
// With -q p (an odd prime below 2^31) and --gpu 1 all windows of a method go to the device in ONE call
// (plo_cse_batch_search, and plo_kernel_batch_search for -K: one workgroup per window, one minimum each); a window
// the device code refuses runs on the host.  Without -q, with a larger modulus or with --gpu 0 the same definition runs on the host (OpenMP).  stdout is
// the same either way; statistics are `#` lines on stderr.
// ===========================================================================
#include "plo_host.hpp"
#include "plo_trim.hpp"
#include "plo_dl.hpp"

#include <chrono>
#include <queue>
#include <regex>
#include <set>

using namespace plo;
using Ops = std::pair<size_t, size_t>;

namespace {

struct HipLib {
    void *h = open_hip_lib(); bool ok = h != nullptr;
    PLO_SYM(init, plo_init); PLO_SYM(last_error, plo_last_error); PLO_SYM(batch_search, plo_cse_batch_search);
    PLO_SYM(kernel_batch_search, plo_kernel_batch_search);
};

struct Options {
    size_t loops = 100; uint64_t q = 0, seed0 = 0; bool singles = false, direct = false, kernel = false, lu = false, apply = false; int gpu = 1;
    std::string pattern, file;
};

bool ident(const std::string &t) { return isalpha((unsigned char)t[0]) || t[0] == '_'; }

// one line `lhs:=expr;` of the program
struct PLine { std::vector<std::string> tk; std::string lhs; std::vector<std::string> uses; };     // uses: the variables of the right-hand side

std::string text_of(const std::vector<std::string> &tk) { std::string s; for (auto &t : tk) s += t; return s + "\n"; }

std::vector<PLine> read_program(std::istream &in) {
    std::vector<PLine> P; std::string line;
    while (std::getline(in, line)) {
        auto h = line.find('#'); if (h != std::string::npos) line.resize(h);
        if (line.find(":=") == std::string::npos) continue;
        PLine L; L.tk = SlpEval<QField>::tokenize(line);
        if (L.tk.size() < 3 || L.tk[1] != ":=" || !ident(L.tk[0])) throw std::runtime_error("SLP: bad line: " + line);
        if (L.tk.back() != ";") L.tk.emplace_back(";");
        L.lhs = L.tk[0];
        for (size_t k = 2; k < L.tk.size(); ++k) if (ident(L.tk[k]) && std::find(L.uses.begin(), L.uses.end(), L.tk[k]) == L.uses.end()) L.uses.push_back(L.tk[k]);
        P.push_back(std::move(L));
    }
    return P;
}

// The window of a selection (mirabelle.sh:78-120, by whole names): the body is every line that names a selected variable or a
// variable of the right-hand side of a selected variable's defining line; inputs are the variables the body uses and does not
// define, sorted; outputs are the variables it defines but the FIRST selected one, sorted downwards (`sort -r`, :119-120).
struct Window {
    std::vector<std::string> sel, in, out;
    std::vector<size_t> body;
    Ops before{0, 0};
    bool kept = false;
    std::string label() const { std::string s = sel[0]; for (size_t k = 1; k < sel.size(); ++k) s += " " + sel[k]; return s; }
};

Window cut_window(const std::vector<PLine> &P, const std::vector<std::string> &sel) {
    Window W; W.sel = sel;
    std::set<std::string> names(sel.begin(), sel.end());
    for (auto &v : sel)
        for (auto &L : P) if (L.lhs == v) { names.insert(L.uses.begin(), L.uses.end()); break; }
    std::set<std::string> defined, used;
    for (size_t i = 0; i < P.size(); ++i) {
        bool hit = names.count(P[i].lhs) != 0;
        for (auto &u : P[i].uses) hit = hit || names.count(u);
        if (!hit) continue;
        W.body.push_back(i); defined.insert(P[i].lhs); used.insert(P[i].uses.begin(), P[i].uses.end());
    }
    for (auto &u : used) if (!defined.count(u)) W.in.push_back(u);
    for (auto it = defined.rbegin(); it != defined.rend(); ++it) if (*it != sel[0]) W.out.push_back(*it);
    W.kept = !W.out.empty() && defined.count(sel[0]) != 0;
    if (W.kept) {
        std::string body; for (size_t i : W.body) body += text_of(P[i].tk);
        trim::Words words; std::istringstream is(body);
        W.before = trim::operations(trim::parse(is, words));          // what SLPchecker prints for these lines (mirabelle.sh:130)
    }
    return W;
}

// the window as a program over i# and o#: its matrix is outputs x inputs
template <class F> SparseMat<typename F::Elt> window_matrix(const F &f, const std::vector<PLine> &P, const Window &W) {
    std::map<std::string, std::string> nm;
    for (size_t k = 0; k < W.in.size(); ++k) nm[W.in[k]] = "i" + std::to_string(k);
    for (size_t i : W.body) if (!nm.count(P[i].lhs)) nm[P[i].lhs] = "w_" + std::to_string(i);      // (no name SlpEval would take for an input)
    std::string text;
    for (size_t i : W.body) { auto tk = P[i].tk; for (auto &t : tk) if (ident(t)) t = nm.at(t); text += text_of(tk); }
    for (size_t r = 0; r < W.out.size(); ++r) text += "o" + std::to_string(r) + ":=" + nm.at(W.out[r]) + ";\n";
    SlpEval<F> ev(f); std::istringstream is(text); ev.run(is);
    return ev.matrix('o', W.out.size(), W.in.size());
}

// minimum under (cmpOpCount, then the smaller seed)
struct Best {
    Ops ops{0, 0}; uint64_t seed = 0; bool have = false;
    void offer(const Ops &o, uint64_t s) { if (!have || cmp_op_count(o, ops) || (!cmp_op_count(ops, o) && s < seed)) { ops = o; seed = s; have = true; } }
};

// the two methods for one seed; os gets the program over i#, o# and temporaries
template <class F> Ops direct_text(const F &f, const SparseMat<typename F::Elt> &M, uint64_t seed, std::ostream &os) {
    input2temps(os, M, 'i', 't');
    Replay<F> R(f, M, seed, os, 'o', 't', 'r');
    return R.optimizer();
}
template <class F> Ops lu_text(const F &f, const LUFactors<F> &lu, uint64_t seed, std::ostream &os) {       // include/plinopt_optimize.inl:1058-1079
    for (size_t k = 0; k < lu.P.size(); ++k) os << 't' << k << ":=" << 'i' << lu.P[k] << ";\n";
    CandRng rng(seed);
    Replay<F> RU(f, lu.U, rng, os, 'v', 't', 'r'); const Ops uo = RU.optimizer();
    Replay<F> RL(f, lu.L, rng, os, 'x', 'v', 'g'); const Ops lo = RL.optimizer();
    for (size_t i = 0; i < lu.Q.size(); ++i) os << 'o' << i << ":=" << 'x' << lu.Q[i] << ";\n";
    return {uo.first + lo.first, uo.second + lo.second};
}

// -K: restart `seed` of the kernel method on M, decomposition and both Optimizer calls from that seed (plo_oracle_kernel_restart)
template <class F> Ops kernel_restart_text(const F &f, const SparseMat<typename F::Elt> &M, uint64_t seed, std::ostream &os) {
    KernelDecomp<F> kd; Ops ops{0, 0};
    if (!kernel_decomp(f, M, seed, kd)) throw std::runtime_error("zero dimensional kernel");      // (decided once per window: the rank does not depend on the order)
    os << kernel_text(f, kd, seed, ops);
    return ops;
}
// The replay of the kernel method defines a dependent output twice (`o3:=0;` from Free's emptied row, later `o3:=x0;`; nothing reads
// it in between: Dep's columns are basis rows): the text with the last definition of every variable only
std::string last_definitions(const std::string &text) {
    std::vector<std::string> lines; std::istringstream is(text); std::string line;
    while (std::getline(is, line)) lines.push_back(line);
    std::set<std::string> later; std::vector<bool> keep(lines.size(), true);
    for (size_t k = lines.size(); k-- > 0;) { const auto c = lines[k].find(":="); if (c != std::string::npos && !later.insert(lines[k].substr(0, c)).second) keep[k] = false; }
    std::string out; for (size_t k = 0; k < lines.size(); ++k) if (keep[k]) out += lines[k] + "\n";
    return out;
}

// A replayed program without its copies (`t0:=i0;`), zero lines and temporaries nothing reads, in token lines
std::vector<std::vector<std::string>> tidy(const std::string &text) {
    std::vector<std::vector<std::string>> lines; std::istringstream is(text); std::string line;
    std::map<std::string, std::string> alias;
    auto output = [](const std::string &t) { return t[0] == 'o' && t.size() > 1 && isdigit((unsigned char)t[1]); };
    while (std::getline(is, line)) {
        auto tk = SlpEval<QField>::tokenize(line);
        if (tk.size() < 4) continue;
        for (size_t k = 2; k < tk.size(); ++k) { auto it = alias.find(tk[k]); if (it != alias.end()) tk[k] = it->second; }
        if (tk.size() == 4 && ident(tk[2]) && !output(tk[0])) { alias[tk[0]] = tk[2]; continue; }
        lines.push_back(std::move(tk));
    }
    std::set<std::string> read; std::vector<std::vector<std::string>> keep;
    for (size_t k = lines.size(); k-- > 0;) {
        if (!output(lines[k][0]) && !read.count(lines[k][0])) continue;
        for (size_t j = 2; j < lines[k].size(); ++j) if (ident(lines[k][j])) read.insert(lines[k][j]);
        keep.push_back(lines[k]);
    }
    std::reverse(keep.begin(), keep.end());
    return keep;
}

struct Result { Best d, k, g; bool improved = false; Ops after{0, 0}; std::vector<std::vector<std::string>> repl; };    // repl: the replacement in the program's names

template <class F> int run(const F &f, const Options &o, const std::vector<PLine> &P) {
    using Mat = SparseMat<typename F::Elt>;
    // ---- selections and windows
    std::vector<std::string> vars;
    {
        std::set<std::string> seen; std::regex re;
        if (!o.pattern.empty()) re = std::regex(o.pattern, std::regex::extended);
        for (auto &L : P) {
            if (L.lhs[0] == 'o' || !seen.insert(L.lhs).second) continue;                       // prune.sh:73
            if (!o.pattern.empty() && !std::regex_search(L.lhs, re)) continue;
            vars.push_back(L.lhs);
        }
    }
    std::vector<Window> wins; size_t skipped = 0;
    for (auto &a : vars) {
        if (o.singles) { Window W = cut_window(P, {a}); if (W.kept) wins.push_back(std::move(W)); else ++skipped; continue; }   // prune.sh:85-87
        for (auto &b : vars) {                                                                                                 // prune.sh:79-83
            Window W = cut_window(P, a == b ? std::vector<std::string>{a} : std::vector<std::string>{a, b});
            if (a == b) W.sel = {a, b};
            if (W.kept) wins.push_back(std::move(W)); else ++skipped;
        }
    }
    const size_t nw = wins.size(), N = o.loops;
    std::vector<Mat> mats(nw); std::vector<LUFactors<F>> lus(nw);
#pragma omp parallel for schedule(dynamic, 8)
    for (long long w = 0; w < (long long)nw; ++w) { mats[w] = window_matrix(f, P, wins[w]); if (o.lu) lus[w] = sparse_lu(f, mats[w]); }
    // -K: the windows whose matrix has a kernel of positive dimension
    std::vector<size_t> with_kernel;
    if (o.kernel) {
        std::vector<char> has(nw, 0);
#pragma omp parallel for schedule(dynamic, 8)
        for (long long w = 0; w < (long long)nw; ++w) { KernelDecomp<F> kd; has[w] = kernel_decomp(f, mats[w], o.seed0 + (uint64_t)w * o.loops, kd) ? 1 : 0; }
        for (size_t w = 0; w < nw; ++w) if (has[w]) with_kernel.push_back(w);
    }
    std::clog << "# windows: " << nw << " kept, " << skipped << " skipped (no output); " << N << " restarts per window and method" << std::endl;

    // ---- search: window w uses the seeds seed0 + w*N + j
    std::vector<Result> res(nw);
    auto host_search = [&](char method, const std::vector<size_t> &which) {
#pragma omp parallel for schedule(dynamic, 1)
        for (long long k = 0; k < (long long)which.size(); ++k) {
            const size_t w = which[k]; Best b;
            for (size_t j = 0; j < N; ++j) {
                std::ostringstream sink; const uint64_t seed = o.seed0 + w * N + j;
                b.offer(method == 'D' ? direct_text(f, mats[w], seed, sink) : method == 'K' ? kernel_restart_text(f, mats[w], seed, sink) : lu_text(f, lus[w], seed, sink), seed);
            }
            (method == 'D' ? res[w].d : method == 'K' ? res[w].k : res[w].g) = b;
        }
    };
    std::vector<size_t> all(nw); for (size_t w = 0; w < nw; ++w) all[w] = w;
    bool on_gpu = false;
    if constexpr (std::is_same<F, ZpField>::value) on_gpu = o.gpu > 0 && nw > 0 && N > 0;
    for (char method : {'D', 'K', 'G'}) {
        if (!(method == 'D' ? o.direct : method == 'K' ? o.kernel : o.lu)) continue;
        const std::vector<size_t> &mine = method == 'K' ? with_kernel : all;          // the windows of this method
        std::vector<size_t> host = mine;
        if constexpr (std::is_same<F, ZpField>::value) if (on_gpu && !mine.empty()) {
            static HipLib L;                                                              // no silent fallback: --gpu 0 selects the host loop
            if (!L.ok) { std::cerr << "# \033[1;31mERROR: cannot use the GPU: library missing\033[0m" << std::endl; return 2; }
            if (L.init(0) != PLO_OK) { std::cerr << "# \033[1;31mERROR: cannot use the GPU: " << L.last_error() << "\033[0m" << std::endl; return 2; }
            std::vector<Csr> A, B; std::vector<plo_csr_t> va, vb;
            // (-K too passes every window, so that problem w has the seeds seed0 + w*N + j of the other methods: a window without a kernel is refused by its rank
            // on the host side of the call, before anything of it reaches the device)
            for (size_t w = 0; w < nw; ++w) {
                if (method == 'G') { A.push_back(csr(lus[w].U)); B.push_back(csr(lus[w].L)); } else A.push_back(csr(mats[w]));
            }
            for (auto &c : A) va.push_back(c.view());
            for (auto &c : B) vb.push_back(c.view());
            std::vector<plo_best_t> bests(nw); std::vector<int32_t> status(nw); plo_stats_t st{};
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = method == 'K' ? L.kernel_batch_search((uint32_t)nw, va.data(), (uint32_t)o.q, o.seed0, (uint32_t)N, PLO_COST_SUM_THEN_ADD, bests.data(), status.data(), &st)
                                         : L.batch_search((uint32_t)nw, va.data(), method == 'D' ? nullptr : vb.data(), (uint32_t)o.q, o.seed0, (uint32_t)N, PLO_COST_SUM_THEN_ADD, bests.data(), status.data(), &st);
            const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (rc != PLO_OK) { std::cerr << "# \033[1;31mERROR: -" << method << " GPU search failed: " << L.last_error() << "\033[0m" << std::endl; return 2; }
            host.clear();
            for (size_t w : mine) {
                if (status[w] != PLO_OK) { host.push_back(w); continue; }
                Best b; b.offer({bests[w].adds, bests[w].muls}, bests[w].seed); (method == 'D' ? res[w].d : method == 'K' ? res[w].k : res[w].g) = b;
            }
            std::clog << "# GPU: -" << method << " one " << (method == 'K' ? "plo_kernel_batch_search" : "plo_cse_batch_search") << " call over " << mine.size() << " windows: " << st.candidates << " candidates, " << st.launches << " launches, kernel "
                      << st.kernel_ms << " ms, wall " << wall << " s (" << (wall > 0 ? 100.0 * (wall - st.kernel_ms / 1000.0) / wall : 0.0) << " % on the host), "
                      << (wall > 0 ? st.candidates / wall : 0.0) << " candidates/s" << std::endl;
            if (!host.empty()) std::clog << "# refused: -" << method << " " << host.size() << " windows the " << (method == 'K' ? "kernel-method" : "wave") << " kernel does not take run on the host" << std::endl;
        }
        const auto t0 = std::chrono::steady_clock::now();
        host_search(method, host);
        if (!on_gpu) std::clog << "# host: -" << method << " " << host.size() * N << " candidates, " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s" << std::endl;
    }

    // ---- the winners replayed, checked and put into the program's names
    std::set<char> letters; for (auto &L : P) { letters.insert(L.lhs[0]); for (auto &u : L.uses) letters.insert(u[0]); }
    std::string fresh;
    for (const char *c = "abcdefghjklmnpqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"; *c && fresh.empty(); ++c) if (!letters.count(*c)) fresh = std::string(1, *c);
    if (fresh.empty()) fresh = "pruner_";
    int bad = 0;
#pragma omp parallel for schedule(dynamic, 8)
    for (long long w = 0; w < (long long)nw; ++w) {
        Result &R = res[w]; const Window &W = wins[w];
        // best of D, K, G under cmpOpCount, the earlier method winning ties
        char use = 'D'; const Best *pb = &R.d;
        if (R.k.have && (!pb->have || cmp_op_count(R.k.ops, pb->ops))) { use = 'K'; pb = &R.k; }
        if (R.g.have && (!pb->have || cmp_op_count(R.g.ops, pb->ops))) { use = 'G'; pb = &R.g; }
        const Best &b = *pb;
        if (!b.have) continue;
        R.after = b.ops;
        R.improved = b.ops.first + b.ops.second < W.before.first + W.before.second;
        if (!R.improved) continue;
        std::ostringstream os;
        const Ops ops = use == 'G' ? lu_text(f, lus[w], b.seed, os) : use == 'K' ? kernel_restart_text(f, mats[w], b.seed, os) : direct_text(f, mats[w], b.seed, os);
        auto lines = tidy(use == 'K' ? last_definitions(os.str()) : os.str());
        std::string plain; for (auto &tk : lines) plain += text_of(tk);
        SlpEval<F> ev(f); std::istringstream is(plain); ev.run(is);
        if (ops != b.ops || !same_matrix(f, ev.matrix('o', mats[w].rowdim(), mats[w].coldim()), mats[w])) {
#pragma omp critical
            { ++bad; std::cerr << "# \033[1;31mERROR: window " << W.label() << ": the replay of seed " << b.seed << " does not give the program the search counted\033[0m" << std::endl; }
            R.improved = false; continue;
        }
        std::map<std::string, std::string> nm; size_t next = 0;
        for (auto &tk : lines) for (auto &t : tk) {
            if (!ident(t)) continue;
            const bool num = t.size() > 1 && std::all_of(t.begin() + 1, t.end(), [](char ch) { return isdigit((unsigned char)ch) != 0; });
            if (num && t[0] == 'i') t = W.in[std::stoul(t.substr(1))];
            else if (num && t[0] == 'o') t = W.out[std::stoul(t.substr(1))];
            else { auto it = nm.find(t); if (it == nm.end()) it = nm.emplace(t, fresh + std::to_string(next++)).first; t = it->second; }
        }
        R.repl = std::move(lines);
    }

    if (!o.apply) {
        for (size_t w = 0; w < nw; ++w) {
            const Window &W = wins[w]; const Result &R = res[w];
            std::cout << W.label() << " [" << W.out.size() << 'x' << W.in.size() << "]: " << W.before.first << '|' << W.before.second;
            if (R.d.have) std::cout << " D " << R.d.ops.first << '|' << R.d.ops.second << " [seed " << R.d.seed << ']';
            if (R.k.have) std::cout << " K " << R.k.ops.first << '|' << R.k.ops.second << " [seed " << R.k.seed << ']';
            if (R.g.have) std::cout << " G " << R.g.ops.first << '|' << R.g.ops.second << " [seed " << R.g.seed << ']';
            const long dif = (long)(W.before.first + W.before.second) - (long)(R.after.first + R.after.second);      // mirabelle.sh:139-175
            if (R.improved) std::cout << " IMPROVEMENT";
            else if (dif == 0 && W.before.second > R.after.second) std::cout << " == less multiplications";
            else if (dif == 0 && W.before.first > R.after.first) std::cout << " == less additions";
            else if (dif == 0) std::cout << " ==";
            else std::cout << " \xE2\x89\xA4";
            std::cout << '\n';
            if (R.improved) for (auto &tk : R.repl) std::cout << text_of(tk);
        }
        return bad ? 1 : 0;
    }

    // ---- --apply: the improvement with the largest saving (ties: first window) whose lines can be ordered
    std::string original; for (auto &L : P) original += text_of(L.tk);
    Mat want; { SlpEval<F> ev(f); std::istringstream is(original); ev.run(is); want = ev.matrix(); }
    std::vector<size_t> order;
    for (size_t w = 0; w < nw; ++w) if (res[w].improved) order.push_back(w);
    auto saving = [&](size_t w) { return wins[w].before.first + wins[w].before.second - res[w].after.first - res[w].after.second; };
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return saving(x) > saving(y); });
    for (size_t w : order) {
        // the lines: those outside the body at their place, the replacement at the place of the body's first line
        struct Item { size_t pos, sub; const std::vector<std::string> *tk; };
        std::vector<Item> items; std::set<size_t> body(wins[w].body.begin(), wins[w].body.end());
        for (size_t i = 0; i < P.size(); ++i) if (!body.count(i)) items.push_back(Item{i, 0, &P[i].tk});
        for (size_t k = 0; k < res[w].repl.size(); ++k) items.push_back(Item{wins[w].body[0], k + 1, &res[w].repl[k]});
        // topological order, stable with respect to (pos, sub): always the earliest line whose variables are all defined
        std::map<std::string, size_t> def; for (size_t k = 0; k < items.size(); ++k) def[(*items[k].tk)[0]] = k;
        std::vector<std::vector<size_t>> readers(items.size()); std::vector<size_t> waits(items.size(), 0);
        for (size_t k = 0; k < items.size(); ++k) {
            std::set<size_t> deps;
            for (size_t j = 2; j < items[k].tk->size(); ++j) { auto it = def.find((*items[k].tk)[j]); if (it != def.end() && it->second != k) deps.insert(it->second); }
            for (size_t d : deps) readers[d].push_back(k);
            waits[k] = deps.size();
        }
        auto later = [&](size_t x, size_t y) { return std::make_pair(items[x].pos, items[x].sub) > std::make_pair(items[y].pos, items[y].sub); };
        std::priority_queue<size_t, std::vector<size_t>, decltype(later)> ready(later);
        for (size_t k = 0; k < items.size(); ++k) if (!waits[k]) ready.push(k);
        std::string out; size_t done = 0;
        while (!ready.empty()) { const size_t k = ready.top(); ready.pop(); out += text_of(*items[k].tk); ++done; for (size_t r : readers[k]) if (!--waits[r]) ready.push(r); }
        if (done != items.size()) { std::clog << "# --apply: window " << wins[w].label() << " cannot be put back (a cycle through a variable outside it); trying the next" << std::endl; continue; }
        Mat got; { SlpEval<F> ev(f); std::istringstream is(out); ev.run(is); got = ev.matrix('o', want.rowdim(), want.coldim()); }
        if (!same_matrix(f, got, want)) { std::cerr << "# \033[1;31mERROR: --apply: window " << wins[w].label() << " changes the program's matrix\033[0m" << std::endl; ++bad; continue; }
        std::clog << "# --apply: window " << wins[w].label() << ", " << wins[w].before.first << '|' << wins[w].before.second << " -> " << res[w].after.first << '|' << res[w].after.second << std::endl;
        std::cout << out;
        return bad ? 1 : 0;
    }
    std::clog << "# --apply: no improvement to apply; the program is unchanged" << std::endl;
    std::cout << original;
    return bad ? 1 : 0;
}

} // namespace

int main(int argc, char **argv)
{
    cap_omp_threads();
    Options o;
    for (int i = 1; i < argc; ++i) {
        const std::string a(argv[i]);
        auto more = [&]() { return i + 1 < argc; };
        if (a == "-O" && more()) o.loops = strtoull(argv[++i], nullptr, 10);
        else if (a == "-q" && more()) o.q = strtoull(argv[++i], nullptr, 10);
        else if (a == "-l" && more()) o.pattern = argv[++i];
        else if (a == "--seed" && more()) o.seed0 = strtoull(argv[++i], nullptr, 10);
        else if (a == "--gpu" && more()) o.gpu = atoi(argv[++i]);
        else if (a == "-v") o.singles = true;
        else if (a == "-D") o.direct = true;
        else if (a == "-K") o.kernel = true;
        else if (a == "-G") o.lu = true;
        else if (a == "--apply") o.apply = true;
        else if (a[0] == '-') { std::clog << "Usage: " << argv[0] << " [-O N] [-q p] [-v] [-l regex] [-D] [-K] [-G] [--seed S] [--gpu 0|1] [--apply] P.slp\n"
                                            "  methods: -D Optimizer, -K kernel method, -G LU chain; none given: -D -G (the reference's scripts run -D -K -G)\n"; return a == "-h" ? 0 : 2; }
        else o.file = a;
    }
    if (!o.direct && !o.kernel && !o.lu) o.direct = o.lu = true;
    if (o.gpu < 0 || o.gpu > 1) { std::cerr << "# \033[1;31mERROR: --gpu takes 0 or 1 (one device)\033[0m" << std::endl; return 2; }
    try {
        std::ifstream in(o.file);
        if (!in) { std::cerr << "# \033[1;31mERROR: cannot open " << o.file << "\033[0m" << std::endl; return 2; }
        const std::vector<PLine> P = read_program(in);
        if (o.q) {
            if (o.q < 3 || !(o.q & 1)) throw std::runtime_error("-q takes an odd prime");
            for (auto &L : P) for (auto &t : L.tk)       // every constant of the program must be a unit modulo p
                if (isdigit((unsigned char)t[0]) && (unsigned __int128)std::stoull(t) % o.q == 0) throw std::runtime_error("the constant " + t + " of " + L.lhs + " is no unit modulo " + std::to_string(o.q));
        }
        if (o.q >= (1ull << 31)) { if (o.gpu) std::clog << "# modulus of 2^31 or more: host search" << std::endl; return run(Zp64Field(o.q), o, P); }
        if (o.q) return run(ZpField((uint32_t)o.q), o, P);
        return run(QField(), o, P);
    } catch (const std::exception &e) {
        std::cerr << "# \033[1;31mERROR: " << e.what() << "\033[0m" << std::endl;
        return 3;
    }
}
