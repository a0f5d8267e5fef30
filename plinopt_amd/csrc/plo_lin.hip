// ==========================================================================
// plo_lin.hip -- in-place linear program search (bin/inplacer) on gfx950.
//
// Replaces the body of the restart loop of SearchLinearAlgorithm (reference
// include/plinopt_inplace.inl:621-669): one candidate = a row permutation of A
// (:626-633, no sign flips), then
//   variant 0: the unoriented program (LinearAlgorithm :397-502, :636), a random pivot per row;
//   variant 1: the oriented program APPENDED to variant 0's simplified one (:654 calls LinearAlgorithm on
//              lProgram again without clearing it), the fixpoint of simplify run over the concatenation and
//              the counts taken over it (ROWS = 2m);
// and their (ADD, SCA, ROWS) counts (complexity :133-144).  Counts only: the host replays the winner to print it.
//
// One wavefront per candidate, its atom list in LDS: the device functions of plo_tril.hip (t_linear,
// t_simplify) with X = TL_APPEND | TL_EMPTYBAR | TL_NOSIGN -- append instead of clearing, an empty row as
// the barrier Atom(' ', l, ' ', 0) of :474-476, no sign array.  The candidate's stream is the trilinear
// candidate's without the sign draws: Fisher-Yates from the seed's stream, then the draws of variant 0, then
// those of variant 1.  seed == PLO_LIN_BASE_SEED is the unpermuted oriented program of :613 (both halves of
// ops6 hold it).  Coefficients +-1, or rationals as residues modulo a 31-bit prime (lin_kernel<true>); a row
// of more than 64 entries is refused at plan creation and stays on the host.
//
// LDS of a wave: 8 bytes per atom for the concatenation (cap >= 4 nnz + 2 m + 2, see plo_capi.hip) and the
// permutation (2 bytes per row).
// ==========================================================================
#pragma once
#include "plo_tril.hip"

namespace plo {

struct LinPlan { TrilMat M; uint32_t cap; uint32_t lds_per_wave; uint32_t p; };   // p != 0: rational coefficients as residues modulo p
enum : uint32_t { LIN_X = TL_APPEND | TL_EMPTYBAR | TL_NOSIGN };

// J.ops: 6 per candidate, ADD,SCA,ROWS of variant 0 then of variant 1; J.best: the packed minimum
// (ADD << 48 | SCA << 32 | candidate << 1 | variant), the order of :637-641 made total by (seed, variant).
template <bool RAT> __global__ __launch_bounds__(256) void lin_kernel(LinPlan P, TrilJob J)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint8_t *reg = ldyn + (size_t)wave * P.lds_per_wave;
    const uint32_t cap = P.cap, m = P.M.m;
    TrilProg G;
    G.at = (uint64_t *)reg; G.n = 0;
    uint16_t *perm = (uint16_t *)(reg + 8u * cap);
    unsigned long long best = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * nw;
    for (uint64_t cnd = (uint64_t)blockIdx.x * nw + wave; cnd < J.ncand; cnd += stride) {
        const uint64_t seed = J.seeds ? J.seeds[cnd] : J.seed0 + cnd;
        uint32_t rng = 1u + (uint32_t)(t_splitmix(seed) % 2147483646ull);
        const bool basec = seed == ~0ull;
        for (uint32_t k = lane; k < m; k += 64u) perm[k] = (uint16_t)k;
        TW_SYNC();
        if (!basec) {
            // the stream is sequential: one lane draws (Fisher-Yates, :626-633)
            if (lane == 0)
                for (uint32_t i = m; i > 1u; --i) { const uint32_t j = t_rng(rng) % i; const uint16_t t = perm[i - 1u]; perm[i - 1u] = perm[j]; perm[j] = t; }
            rng = t_uni(rng);
            TW_SYNC();
        }
        uint32_t tot[6] = {0, 0, 0, 0, 0, 0};
        G.n = 0;
        t_linear<RAT, LIN_X>(G, P.M, perm, nullptr, 0u, false, basec, rng, lane, tot, cap, J.err, nullptr, P.p);         // :613 or :636
        if (basec) { tot[3] = tot[0]; tot[4] = tot[1]; tot[5] = tot[2]; }
        else t_linear<RAT, LIN_X>(G, P.M, perm, nullptr, 0u, false, true, rng, lane, tot + 3, cap, J.err, nullptr, P.p);   // :654, appended
        if (lane == 0) {
            if (J.ops) for (int k = 0; k < 6; ++k) J.ops[6u * cnd + k] = tot[k];
            for (uint32_t variant = 0; variant < 2u; ++variant) {
                const unsigned long long key = ((unsigned long long)(tot[3u * variant] & 0xFFFFu) << 48) | ((unsigned long long)(tot[3u * variant + 1u] & 0xFFFFu) << 32)
                                             | ((unsigned long long)(cnd & 0x7FFFFFFFull) << 1) | variant;
                best = key < best ? key : best;
            }
        }
    }
    if (J.best && lane == 0 && best != ~0ull) atomicMin(J.best, best);
}

} // namespace plo
