// ==========================================================================
// plo_dl.hpp -- what the host tools that drive the device share (bin/optimizer, bin/sparsifier, bin/trilplacer, bin/inplacer,
// bin/orbiter): where they look for libplinopt_hip.so (PLO_HIP_LIB / PLINOPT_HIP_LIB, then plinopt_amd/ beside the tool's bin/
// directory and the tool's own directory, then the loader's search path), how they name its symbols, and the CSRs of its
// entries: over Z_p, and the rational one that the plo_*_plan_create_q entries take.
// ==========================================================================
#pragma once
#include "plo_host.hpp"
#include "../../../include/plinopt_hip.h"
#include <dlfcn.h>
#include <libgen.h>

namespace plo {

// the first candidate that loads, or null (and the reason on stderr)
inline void *open_hip_lib() {
    std::vector<std::string> cand;
    for (const char *v : {"PLO_HIP_LIB", "PLINOPT_HIP_LIB"}) if (const char *e = getenv(v)) cand.emplace_back(e);   // (one name for the tools and plinopt_amd/capi.py; the older one still works)
    char buf[4096]; ssize_t k = readlink("/proc/self/exe", buf, sizeof buf - 1);
    if (k > 0) { buf[k] = 0; std::string d = dirname(buf); cand.push_back(d + "/../plinopt_amd/libplinopt_hip.so"); cand.push_back(d + "/libplinopt_hip.so"); }
    cand.emplace_back("libplinopt_hip.so");
    void *h = nullptr;
    for (auto &c : cand) { h = dlopen(c.c_str(), RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) std::cerr << "# \033[1;31mERROR: cannot load libplinopt_hip.so: " << dlerror() << "\033[0m\n";
    return h;
}

// A tool's table of the library is a struct that begins with the handle and a flag, `void *h = open_hip_lib(); bool ok = h != nullptr;`
// (bin/optimizer sets them in a constructor: it loads on demand), and then has one line per symbol: the typed pointer from the
// header's prototype, resolved from h (null without a library).  A missing PLO_SYM clears `ok`; a missing PLO_SYM_OPT is for the
// tool to test.
template <class Fn> Fn hip_sym(void *h, const char *name, bool *ok) { Fn f = h ? (Fn)dlsym(h, name) : nullptr; if (!f && ok) *ok = false; return f; }
#define PLO_SYM(field, fn) decltype(&fn) field = plo::hip_sym<decltype(&fn)>(h, #fn, &ok)
#define PLO_SYM_OPT(field, fn) decltype(&fn) field = plo::hip_sym<decltype(&fn)>(h, #fn, nullptr)

// A matrix over Z_p (residues below 2^31) as the CSR of the C-ABI
struct Csr {
    uint32_t m = 0, n = 0; std::vector<uint32_t> rp{0}, col, val;
    plo_csr_t view() const { return plo_csr_t{m, n, rp.data(), col.data(), val.data()}; }
};
template <class E> Csr csr(const SparseMat<E> &M) {
    Csr c; c.m = (uint32_t)M.rowdim(); c.n = (uint32_t)M.coldim();
    for (const auto &row : M.rows) {
        for (const auto &e : row) { c.col.push_back((uint32_t)e.first); c.val.push_back((uint32_t)e.second); }
        c.rp.push_back((uint32_t)c.col.size());
    }
    return c;
}

// A matrix over Q as the rational CSR of the C-ABI; wide: a coefficient that does not fit its 64-bit numerators and denominators
// (Rat is 128 bits wide, its denominator positive), which keeps the matrix on the host
struct QCsr {
    uint32_t m = 0, n = 0; std::vector<uint32_t> rp{0}, col; std::vector<int64_t> num, den; bool wide = false;
    plo_qcsr_t view() const { return plo_qcsr_t{m, n, rp.data(), col.data(), num.data(), den.data()}; }
};
inline QCsr qcsr(const QMat &M) {
    QCsr c; c.m = (uint32_t)M.rowdim(); c.n = (uint32_t)M.coldim();
    for (const auto &row : M.rows) {
        for (const auto &e : row) {
            c.col.push_back((uint32_t)e.first);
            if (e.second.n > (__int128)INT64_MAX || e.second.n < -(__int128)INT64_MAX || e.second.d > (__int128)INT64_MAX) c.wide = true;
            c.num.push_back((int64_t)e.second.n); c.den.push_back((int64_t)e.second.d);
        }
        c.rp.push_back((uint32_t)c.col.size());
    }
    return c;
}

} // namespace plo
