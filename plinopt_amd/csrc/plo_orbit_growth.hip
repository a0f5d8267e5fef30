// ==========================================================================
// plo_orbit_growth.hip -- the 2-norm growth factor of a candidate of the De Groote orbit search (bin/orbiter -g,
// PLO_ORBIT_GROWTH of include/plinopt_hip.h; the reference's G2, src/growthfactor.cpp:117-125) on gfx950, over Q.
//
// The candidate, its stream and the sandwich are orbit_kernel's (plo_orbit.hip): the draws o_zoi<false> and o_pluq<false> are
// called as they are, and the transformed entries `acc` are the same exact integers (row g of the 3r rows scaled by c_g).
// Beside nnz and nno every non-zero acc adds acc^2 into S_g, one of 3r 64-bit sums of the wave in LDS (integer additions:
// any order gives the same sum).  Then
//   n_g = sqrt(double(S_g)) / double(c_g),   cost = sum_{i < r} (n_i * n_{r+i}) * n_{2r+i}
// with every operation rounded to nearest, no fused multiply-add, the sum from 0.0 in increasing i: lane i computes term i
// into LDS and lane 0 adds the terms in index order.  The plan proves S_g and c_g below 2^53, so both conversions are exact.
// Contraction is switched off inside the bodies below (a pragma of their blocks: the library's flags stay as they are).
//
// The sums are LDS atomics by measurement: a segmented reduction over the lanes (suffix sums inside each row's run of lanes by
// shuffles, one add per run) took 10 to 30 % longer on every input tried, a 16 x 16 part with all 64 lanes on one row included
// (profiles/orbit_growth_reduction_ab.txt).
// One wave per candidate; LDS as orbit_kernel, and behind a wave's region its 3r sums (24 r bytes).
// ==========================================================================
#pragma once
#include "plo_orbit.hip"

namespace plo {

struct OrbitGrowthJob {
    uint64_t seed0; const uint64_t *seeds; uint64_t ncand;
    double *cost;                    // 1 per candidate (may be null)
    uint32_t *cnt2;                  // 2 per candidate: nnz, nno (may be null)
    uint64_t *best;                  // 3 per wave slot: the bits of the cost, nnz << 21 | nno, candidate index (may be null)
    uint32_t off_sum, wave_bytes;    // the sums within a wave's region; the region's size
};

// n_g of the header: the 2-norm of transformed row g from its sum of squares and its scale
__device__ __forceinline__ double og_norm(uint64_t S, int64_t c) {
#pragma clang fp contract(off)
    return __dsqrt_rn((double)(long long)S) / (double)(long long)c;
}

template <int ACT> __global__ __launch_bounds__(256) void orbit_growth_kernel(OrbitPlan P, OrbitGrowthJob J)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int64_t *val = (int64_t *)ldyn;
    int64_t *scale = (int64_t *)(ldyn + P.off_scale);
    uint32_t *rp = (uint32_t *)(ldyn + P.off_rp);
    uint16_t *pos = (uint16_t *)(ldyn + P.off_pos);
    const uint32_t nrows = 3u * P.r;
    for (uint32_t e = threadIdx.x; e < P.nnz; e += blockDim.x) { val[e] = P.val[e]; pos[e] = P.pos[e]; }
    for (uint32_t e = threadIdx.x; e < nrows; e += blockDim.x) scale[e] = P.scale[e];
    for (uint32_t e = threadIdx.x; e <= nrows; e += blockDim.x) rp[e] = P.rp[e];
    __syncthreads();

    uint8_t *reg = ldyn + P.shared_bytes + (size_t)wave * J.wave_bytes;
    auto fac = [&](uint32_t f) { return (int64_t *)(reg + P.off_fac[f]); };
    int64_t *Ti = (int64_t *)(reg + P.off_ti);
    int8_t *T = (int8_t *)(reg + P.off_t);
    uint8_t *perm = reg + P.off_perm;
    unsigned long long *S = (unsigned long long *)(reg + J.off_sum);      // 3r sums of squares; S[i], i < r, then holds term i
    const uint32_t m = P.m, k = P.k, n = P.n, r = P.r;

    uint64_t bbits = ~0ull, bkey = ~0ull, bidx = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * nw;
    for (uint64_t cnd = (uint64_t)blockIdx.x * nw + wave; cnd < J.ncand; cnd += stride) {
        const uint64_t seed = J.seeds ? J.seeds[cnd] : J.seed0 + cnd;
        const bool base = seed == ~0ull;
        uint32_t rng = 1u + (uint32_t)(t_splitmix(seed) % 2147483646ull);
        // the factors as in orbit_kernel: U^-1 is A_L, U is A_P; V is B_L, V^-1 is A_R; W is B_R, W^-1 is B_P
        if constexpr (ACT == 0) {
            o_zoi<false>(m, base, rng, lane, T, Ti, perm, fac(4), true, fac(0), false, 0);
            o_zoi<false>(k, base, rng, lane, T, Ti, perm, fac(1), false, fac(2), true, 0);
            o_zoi<false>(n, base, rng, lane, T, Ti, perm, fac(3), false, fac(5), true, 0);
        } else {
            int64_t *Ti2 = (int64_t *)(reg + P.off_ti2);
            int8_t *T2 = (int8_t *)(reg + P.off_t2);
            o_pluq<false>(m, base, rng, lane, T, T2, Ti, Ti2, perm, fac(4), true, fac(0), false, 0);
            o_pluq<false>(k, base, rng, lane, T, T2, Ti, Ti2, perm, fac(1), false, fac(2), true, 0);
            o_pluq<false>(n, base, rng, lane, T, T2, Ti, Ti2, perm, fac(3), false, fac(5), true, 0);
        }
        for (uint32_t e = lane; e < nrows; e += 64u) S[e] = 0;
        TW_SYNC();
        uint32_t nnz = 0, nno = 0;
#pragma unroll 1
        for (uint32_t part = 0; part < 3u; ++part) {
            const int64_t *A = fac(2u * part), *B = fac(2u * part + 1u);
            const uint32_t a_s = part == 1u ? k : m, b_s = part == 0u ? k : n, E = a_s * b_s, items = r * E, row0 = part * r;
            for (uint32_t t = lane; t < items; t += 64u) {
                const uint32_t row = t / E, e = t - row * E, pp = e / b_s, qq = e - pp * b_s;
                const uint32_t g = row0 + row;
                int64_t acc = 0;
                for (uint32_t x = rp[g]; x < rp[g + 1u]; ++x) {
                    const uint32_t ps = pos[x], a = ps >> 8, b = ps & 0xFFu;
                    const int64_t fa = A[a * a_s + pp], fb = B[b * b_s + qq];
                    if (fa == 0 || fb == 0) continue;
                    acc += fa * val[x] * fb;
                }
                if (acc != 0) {
                    ++nnz;
                    nno += (acc == scale[g] || acc == -scale[g]) ? 0u : 1u;
                    atomicAdd(S + g, (unsigned long long)(acc * acc));        // |acc| < 2^26.5 (the plan's proof): no overflow
                }
            }
        }
        TW_SYNC();
        for (uint32_t i = lane; i < r; i += 64u) {                            // only lane i & 63 reads or writes S[i]
            const double nl = og_norm(S[i], scale[i]), nr = og_norm(S[r + i], scale[r + i]), np = og_norm(S[2u * r + i], scale[2u * r + i]);
            const double term = (nl * nr) * np;
            S[i] = (unsigned long long)__double_as_longlong(term);
        }
        for (int o = 32; o >= 1; o >>= 1) { nnz += __shfl_xor(nnz, o, 64); nno += __shfl_xor(nno, o, 64); }
        TW_SYNC();
        if (lane == 0) {
            double cost = 0.0;
            for (uint32_t i = 0; i < r; ++i) cost = cost + __longlong_as_double((long long)S[i]);       // in index order: part of the definition
            const uint64_t bits = (uint64_t)__double_as_longlong(cost);       // a non-negative finite double: its bits order as it does
            if (J.cost) { J.cost[cnd] = cost; J.cnt2[2u * cnd] = nnz; J.cnt2[2u * cnd + 1u] = nno; }
            const uint64_t key = ((uint64_t)nnz << 21) | (uint64_t)nno;
            if (bits < bbits || (bits == bbits && key < bkey)) { bbits = bits; bkey = key; bidx = cnd; }   // candidates come in increasing order: ties keep the first
        }
        TW_SYNC();
    }
    if (J.best && lane == 0) {
        const uint64_t slot = (uint64_t)blockIdx.x * nw + wave;
        J.best[3u * slot] = bbits; J.best[3u * slot + 1u] = bkey; J.best[3u * slot + 2u] = bidx;
    }
}

} // namespace plo
