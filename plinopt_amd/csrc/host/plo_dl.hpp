// ==========================================================================
// plo_dl.hpp -- where the host tools that drive the device look for libplinopt_hip.so
// (bin/trilplacer, bin/inplacer): PLO_HIP_LIB / PLINOPT_HIP_LIB, then plinopt_amd/ beside
// the tool's bin/ directory and the tool's own directory, then the loader's search path.
// ==========================================================================
#pragma once
#include <dlfcn.h>
#include <libgen.h>
#include <unistd.h>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

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

} // namespace plo
