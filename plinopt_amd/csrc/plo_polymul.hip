// ==========================================================================
// plo_polymul.hip -- every coefficient equation of a polynomial-multiplication triple (bin/PMchecker) on gfx950.
//
// For L (r x na), R (r x nb), P (nc x r) and a modulus 2 <= q < 2^31 (prime or not), the pair (i, j) has the sums
//     S[z] = sum_t L[t][i] R[t][j] P[z][t]   (z < nc)
// and its defect is sum_z S[z] X^z - X^(i+j).  With Z = max(nc, na + nb - 1):
//   * no fold (no polynomial, or one of degree d >= Z): w = Z or d equations per pair, equation c asks S[c] == [c == i + j]
//     (S[c] = 0 for c >= nc);
//   * fold modulo f of degree d < Z: w = d equations, equation c asks sum_{z < nc} S[z] rho[z][c] == rho[i + j][c], where
//     rho[z] = X^z mod f, Z rows of d residues, row-major in global memory: the lanes of a wave read one row side by side.
// The matrices arrive as in plo_brent.hip: L and R by columns (t increasing), P by columns too (the rows of its transpose, z
// increasing), as residues; the host has inverted the denominators and reduced f.  Only + and * happen here.
//
// One wave owns one pair.  The accumulation is the Brent kernel's: 64 lanes at a time take entries of column i of L and bisect
// column j of R for the same t, the matches are taken in turn, and the lanes add the product L R times the entries of row t of
// P^T into the pair's sums in the wave's LDS region, z in chunks when nc exceeds the chunk.  After a chunk, without a fold the
// lanes compare its sums with 0 or 1; with a fold lane c mod 64 owns F[c] (d words of the same region, kept across the chunks) and
// adds S[z] rho[z][c] over the chunk's z: rows z < d of rho are the identity, so S[c] is added as it is, and a sum that is zero
// is passed over by the whole wave.  F is compared with row i + j of rho at the end.  A wave that found violations adds their
// number to one 64-bit counter and offers its smallest one to a 64-bit atomic minimum on (equation - first equation of the
// launch) << 32 | residue, as the Brent kernel does: the result does not depend on scheduling.  Vector stores and atomics only;
// no workgroup barrier.
// ==========================================================================
#pragma once
#include "plo_tril.hip"                 // TW_SYNC; cob_mul is plo_cob.hip's, which plo_capi.hip includes first (as for plo_brent.hip)
#include "../../include/plinopt_hip.h"

namespace plo {

struct PolyMulPlan {
    uint32_t nb, nc, w, d;           // pair = i nb + j; equations per pair; the degree of f when the fold runs, else 0
    uint32_t q; uint64_t mu;         // modulus and floor((2^64 - 1) / q) (cob_mul)
    uint32_t chunk, nchunks;         // sums per wave in LDS; ceil(nc / chunk) with a fold, ceil(w / chunk) without
    const uint32_t *lcp, *lt, *lv;   // L by columns: the entries of column i are lcp[i] .. lcp[i + 1] - 1, (t, residue), t increasing
    const uint32_t *rcp, *rt, *rv;   // R by columns
    const uint32_t *prp, *pz, *pv;   // P^T by rows: the entries of t are prp[t] .. prp[t + 1] - 1, (z, residue), z increasing
    const uint32_t *rho;             // with a fold: Z rows of d residues, rho[z d + c] the coefficient of X^c in X^z mod f
};
struct PolyMulJob {
    uint64_t pair0, npairs;          // the pairs pair0 .. pair0 + npairs - 1; npairs * w < 2^32
    unsigned long long *count;       // violated equations
    unsigned long long *first;       // min of (equation - pair0 w) << 32 | residue found, all ones when none
};

__global__ __launch_bounds__(256) void polymul_kernel(PolyMulPlan P, PolyMulJob J)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const uint64_t rel = (uint64_t)blockIdx.x * W + wave;
    if (rel >= J.npairs) return;                                    // (the kernel has no workgroup barrier)
    const uint64_t pair = J.pair0 + rel;
    const uint32_t pi = (uint32_t)(pair / P.nb), pj = (uint32_t)(pair - (uint64_t)pi * P.nb);
    const uint32_t q = P.q, d = P.d; const uint64_t mu = P.mu;
    const bool fold = d != 0u;
    uint32_t *acc = (uint32_t *)ldyn + (size_t)wave * (P.chunk + d), *F = acc + P.chunk;
    const uint32_t l0 = P.lcp[pi], l1 = P.lcp[pi + 1u], r0 = P.rcp[pj], r1 = P.rcp[pj + 1u];
    const uint32_t zend = fold ? P.nc : P.w;                        // the z that the chunks walk
    uint32_t nviol = 0; unsigned long long best = ~0ull;            // per lane

    for (uint32_t c = lane; c < d; c += 64u) F[c] = 0u;            // (lane c mod 64 alone meets F[c])
    for (uint32_t ch = 0; ch < P.nchunks; ++ch) {
        const uint32_t zlo = ch * P.chunk, zhi = min(zend, zlo + P.chunk);
        for (uint32_t i = lane; i < zhi - zlo; i += 64u) acc[i] = 0u;
        TW_SYNC();
        for (uint32_t base = l0; base < l1 && zlo < P.nc; base += 64u) {   // (without a fold the chunks from nc on hold zeros only)
            const uint32_t i = base + lane;
            uint32_t t = 0, lr = 0; bool hit = false;
            if (i < l1) {
                t = P.lt[i];
                uint32_t lo = r0, hi = r1;                          // the first entry of column j with rt >= t
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (P.rt[mid] < t) lo = mid + 1u; else hi = mid; }
                if (lo < r1 && P.rt[lo] == t) { hit = true; lr = cob_mul(P.lv[i], P.rv[lo], q, mu); }
            }
            unsigned long long todo = __ballot(hit);
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const uint32_t tt = (uint32_t)__shfl((int)t, src, 64), f = (uint32_t)__shfl((int)lr, src, 64);
                if (f == 0u) continue;                              // (a product of two zero divisors of a composite q)
                const uint32_t p1 = P.prp[tt + 1u];
                for (uint32_t e = P.prp[tt] + lane; e < p1; e += 64u) {
                    const uint32_t z = P.pz[e];
                    if (z < zlo || z >= zhi) continue;
                    uint32_t s = acc[z - zlo] + cob_mul(f, P.pv[e], q, mu);
                    if (s >= q) s -= q;
                    acc[z - zlo] = s;
                }
                TW_SYNC();                                          // the next t may meet the same sums from other lanes
            }
        }
        if (!fold) {
            for (uint32_t i = lane; i < zhi - zlo; i += 64u) {
                const uint32_t c = zlo + i, s = acc[i], want = c == pi + pj ? 1u : 0u;
                if (s != want) {
                    ++nviol;
                    best = min(best, ((rel * P.w + c) << 32) | s);
                }
            }
        } else {
            const uint32_t zf = max(zlo, d);                        // the chunk's rows of rho that are no identity rows
            for (uint32_t c = lane; c < d; c += 64u) {
                uint32_t v = F[c];
                if (c >= zlo && c < zhi) { v += acc[c - zlo]; if (v >= q) v -= q; }
                for (uint32_t z = zf; z < zhi; ++z) {
                    const uint32_t s = acc[z - zlo];                // (the same word for every lane)
                    if (s == 0u) continue;
                    v += cob_mul(s, P.rho[(size_t)z * d + c], q, mu);
                    if (v >= q) v -= q;
                }
                F[c] = v;
            }
        }
        TW_SYNC();                                                  // the next chunk clears what these lanes have just read
    }
    if (fold) {
        const uint32_t *want = P.rho + (size_t)(pi + pj) * d;
        for (uint32_t c = lane; c < d; c += 64u) {
            const uint32_t s = F[c];
            if (s != want[c]) {
                ++nviol;
                best = min(best, ((rel * d + c) << 32) | s);
            }
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        nviol += __shfl_xor(nviol, o, 64);
        const unsigned long long ob = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)best, o, 64);
        best = min(best, ob);
    }
    if (lane == 0 && nviol) { atomicAdd(J.count, (unsigned long long)nviol); atomicMin(J.first, best); }
}

} // namespace plo
