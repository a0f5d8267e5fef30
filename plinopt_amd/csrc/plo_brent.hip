// ==========================================================================
// plo_brent.hip -- every Brent equation of a triple (bin/MMchecker) on gfx950.
//
// For L (r x mk), R (r x kn), P (mn x r) and a modulus 2 <= q < 2^31 (prime or not), equation e = (x kn + y) mn + z asks
//     S[x][y][z] = sum_t L[t][x] R[t][y] P[z][t]  ==  [a = a'][b = b'][c = c']      (x = a k + b, y = b' n + c, z = a' n + c')
// (DESIGN.md 2.12).  The matrices arrive as residues: L and R by columns (the t of a column increasing), P by columns too, which
// are the rows of its transpose (the z of a t increasing).  Only + and * happen here; the host has inverted the denominators.
//
// One wave owns one pair (x, y).  64 lanes at a time take entries of column x of L and bisect column y of R for the same t; the
// matches are then taken in turn: the product L R goes to every lane, and the lanes add it times the entries of row t of P^T
// into the pair's mn sums in LDS.  The z of one t are distinct, so no two lanes meet in one sum; the t follow each other in
// program order.  When mn sums do not fit the wave's LDS region the wave walks z in chunks and repeats the intersection per
// chunk (a row's entries outside the chunk are passed over).  At the end of a chunk the lanes compare the sums with the
// expected 0 or 1.  A wave that found violations adds their number to one 64-bit counter and offers its smallest one to a
// 64-bit atomic minimum on (equation - first equation of the launch) << 32 | residue: sums of integers and a minimum, so the
// result does not depend on how the waves are scheduled.  Vector stores and atomics only.
// ==========================================================================
#pragma once
#include "plo_tril.hip"                 // TW_SYNC; cob_mul is plo_cob.hip's, which plo_capi.hip includes first (as for plo_dep.hip)
#include "../../include/plinopt_hip.h"

namespace plo {

struct BrentPlan {
    uint32_t k, n, kn, mn;           // x = a k + b, y = b' n + c, z = a' n + c'
    uint32_t q; uint64_t mu;         // modulus and floor((2^64 - 1) / q) (cob_mul)
    uint32_t chunk, nchunks;         // sums per wave in LDS; ceil(mn / chunk)
    const uint32_t *lcp, *lt, *lv;   // L by columns: the entries of column x are lcp[x] .. lcp[x + 1] - 1, (t, residue), t increasing
    const uint32_t *rcp, *rt, *rv;   // R by columns
    const uint32_t *prp, *pz, *pv;   // P^T by rows: the entries of t are prp[t] .. prp[t + 1] - 1, (z, residue), z increasing
};
struct BrentJob {
    uint64_t pair0, npairs;          // the pairs pair0 .. pair0 + npairs - 1; npairs * mn < 2^32
    unsigned long long *count;       // violated equations
    unsigned long long *first;       // min of (equation - pair0 mn) << 32 | residue found, all ones when none
};

__global__ __launch_bounds__(256) void brent_kernel(BrentPlan P, BrentJob J)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const uint64_t rel = (uint64_t)blockIdx.x * W + wave;
    if (rel >= J.npairs) return;                                    // (the kernel has no workgroup barrier)
    const uint64_t pair = J.pair0 + rel;
    const uint32_t x = (uint32_t)(pair / P.kn), y = (uint32_t)(pair - (uint64_t)x * P.kn);
    const uint32_t q = P.q; const uint64_t mu = P.mu;
    uint32_t *acc = (uint32_t *)ldyn + (size_t)wave * P.chunk;
    const uint32_t l0 = P.lcp[x], l1 = P.lcp[x + 1u], r0 = P.rcp[y], r1 = P.rcp[y + 1u];
    // the one equation of the pair that expects 1: b = b' and z = a n + c
    const uint32_t a = x / P.k, b = x - a * P.k, b2 = y / P.n, c = y - b2 * P.n;
    const uint32_t zone = b == b2 ? a * P.n + c : 0xFFFFFFFFu;
    uint32_t nviol = 0; unsigned long long best = ~0ull;            // per lane

    for (uint32_t ch = 0; ch < P.nchunks; ++ch) {
        const uint32_t zlo = ch * P.chunk, zhi = min(P.mn, zlo + P.chunk);
        for (uint32_t i = lane; i < zhi - zlo; i += 64u) acc[i] = 0u;
        TW_SYNC();
        for (uint32_t base = l0; base < l1; base += 64u) {
            const uint32_t i = base + lane;
            uint32_t t = 0, lr = 0; bool hit = false;
            if (i < l1) {
                t = P.lt[i];
                uint32_t lo = r0, hi = r1;                          // the first entry of column y with rt >= t
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
        for (uint32_t i = lane; i < zhi - zlo; i += 64u) {
            const uint32_t z = zlo + i, s = acc[i], want = z == zone ? 1u : 0u;
            if (s != want) {
                ++nviol;
                best = min(best, ((rel * P.mn + z) << 32) | s);
            }
        }
        TW_SYNC();                                                  // the next chunk clears what these lanes have just read
    }
    for (int o = 32; o >= 1; o >>= 1) {
        nviol += __shfl_xor(nviol, o, 64);
        const unsigned long long ob = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)best, o, 64);
        best = min(best, ob);
    }
    if (lane == 0 && nviol) { atomicAdd(J.count, (unsigned long long)nviol); atomicMin(J.first, best); }
}

} // namespace plo
