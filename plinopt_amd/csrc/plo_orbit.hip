// ==========================================================================
// plo_orbit.hip -- De Groote orbit search (bin/orbiter) on gfx950.
//
// Replaces the body of the restart loop of the reference's orbiter (src/orbiter.cpp:272-324): one candidate = (U, V, W)
// drawn from the seed's stream (include/plinopt_hip.h, PLO_ORBIT_*), and the counts (cost, nnz, nno) of the transformed
// triple L.(U^-1 (x) V), R.(V^-T (x) W), (U (x) W^-1).P.  Counts only: the host replays the winner to write it.
//
// No Kronecker product is formed: row i of L read as an m x k matrix X becomes U^-T X V, a row Y of R (k x n) becomes
// V^-1 Y W, a column Z of P (m x n) becomes U Z W^-T.  The three parts are one "sandwich" loop over the rows of L, R and
// P^T:  out(p, q) = sum over the row's entries (a, b, x) of A[a][p] x B[b][q], with (A, B) = (U^-1, V), (V^-T, W),
// (U^T, W^-T).  The work items of a candidate are (row, output entry) pairs, 64 per step of the wave.
// U = Pi_P T Pi_Q^T with T upper triangular, +-1 on the diagonal: U^-1 = Pi_Q T^-1 Pi_P^T, T^-1 by back-substitution, one
// lane per column, integral (entries of size at most 2^(s-2)).
//
// Values: over Q the host scales every row of L and R and every column of P to integers (and proves |sums| < 2^62); an entry
// is +-1 iff its size equals its row's scale.  Over Z_p (p < 2^31) residues with 64-bit products.
//
// Actions (PLO_ORBIT_ACT_*, a run-time choice of the plan; orbit_kernel<MOD, ACT>): the triangular draw above is ACT 0; ACT 1
// draws a PLUQ matrix (o_pluq: two lower triangles, both inverted by substitution, M and M^-1 as two s^3 products over the
// lanes) and ACT 2 a Householder matrix (o_house: integer numerators d N over Q, residues with the host's table of 1/d modulo
// p).  The instances differ only in the draw and, for Householder over Q, in the size an entry of +-1 has: the row's scale
// times the denominators of the part's two factors.
//
// One wave per candidate.  LDS of a workgroup: the input rows (values, scales, row pointers, packed positions) once, shared
// by its waves; per wave: the six s x s factors (int64), T^-1 and T of the matrix being drawn (PLUQ: both triangles and both
// inverses; Householder: u and the signs), and with -c one non-zero counter per transformed row.
// ==========================================================================
#pragma once
#include "plo_tril.hip"

namespace plo {

struct OrbitPlan {
    uint32_t m, k, n, r;             // shape; r = L.m = R.m = P.n
    uint32_t nnz;                    // entries of L, R and P^T together
    uint32_t measure;                // 0 density, 2 canonical
    uint64_t p;                      // 0: Q (scaled integers), else the modulus (< 2^31)
    const int64_t *val;              // nnz values
    const int64_t *scale;            // 3r row scales (Q)
    const uint32_t *rp;              // 3r + 1 row pointers: rows of L, then of R, then of P^T
    const uint16_t *pos;             // nnz positions: left index << 8 | right index
    // LDS layout (bytes): the shared input, then lds_per_wave per wave
    uint32_t off_scale, off_rp, off_pos, shared_bytes;
    uint32_t off_fac[6];             // A_L, B_L, A_R, B_R, A_P, B_P within a wave's region
    uint32_t off_ti, off_t, off_perm, off_cnt, lds_per_wave;
    // the actions beside the triangular one (zero and unused there)
    uint32_t off_ti2, off_t2;        // PLUQ: the second triangle's inverse (int64) and the second triangle (int8) within a wave's region
    uint32_t off_dinv;               // Householder modulo p: the table below in the shared LDS
    const uint32_t *dinv;            // 17 entries: 1/d modulo p for d = 0..16, 0 where d is no unit
};
struct OrbitJob {
    uint64_t seed0; const uint64_t *seeds; uint64_t ncand;
    uint32_t *out3;                  // 3 per candidate: cost, nnz, nno (may be null)
    uint64_t *best;                  // 2 per wave slot: (cost << 42 | nnz << 21 | nno), candidate index (may be null)
};

// an integer factor entry (of size at most 2^32: a PLUQ inverse at s = 16) as the kernel's value: itself over Q, its residue modulo p otherwise
template <bool MOD> __device__ __forceinline__ int64_t o_val(int64_t v, uint64_t p) {
    if constexpr (MOD) { int64_t x = v % (int64_t)p; return x < 0 ? x + (int64_t)p : x; }
    else return v;
}

// What every action draws first after the identity: P by Fisher-Yates, then Q.  (o_zoi keeps its own copy of these two loops:
// its text is the parent's, so that the triangular instances compile to the same resource lines.)
__device__ __forceinline__ void o_perms(uint32_t s, uint32_t &rng, uint8_t *P, uint8_t *Q) {
    for (uint32_t i = s; i > 1u; --i) { const uint32_t j = t_rng(rng) % i; const uint8_t t = P[i - 1u]; P[i - 1u] = P[j]; P[j] = t; }
    for (uint32_t i = s; i > 1u; --i) { const uint32_t j = t_rng(rng) % i; const uint8_t t = Q[i - 1u]; Q[i - 1u] = Q[j]; Q[j] = t; }
}

// Draws the stream's s x s matrix (lane 0: the stream is sequential), inverts its triangle (lane j: column j) and writes
// M into fac_m and M^-1 into fac_i, each either as is (stored [row][col]) or transposed, as the sandwich reads them.
template <bool MOD> __device__ void o_zoi(uint32_t s, bool base, uint32_t &rng, uint32_t lane, int8_t *T, int64_t *Ti, uint8_t *perm,
                                          int64_t *fac_m, bool tr_m, int64_t *fac_i, bool tr_i, uint64_t p)
{
    uint8_t *P = perm, *Q = perm + 16;
    if (lane == 0) {
        for (uint32_t i = 0; i < s; ++i) { P[i] = (uint8_t)i; Q[i] = (uint8_t)i; }
        for (uint32_t i = 0; i < s * s; ++i) T[i] = 0;
        if (base) for (uint32_t i = 0; i < s; ++i) T[i * s + i] = 1;
        else {
            for (uint32_t i = s; i > 1u; --i) { const uint32_t j = t_rng(rng) % i; const uint8_t t = P[i - 1u]; P[i - 1u] = P[j]; P[j] = t; }
            for (uint32_t i = s; i > 1u; --i) { const uint32_t j = t_rng(rng) % i; const uint8_t t = Q[i - 1u]; Q[i - 1u] = Q[j]; Q[j] = t; }
            for (uint32_t i = 0; i < s; ++i) T[i * s + i] = (t_rng(rng) & 1u) ? 1 : -1;
            for (uint32_t i = 0; i < s; ++i) for (uint32_t j = i + 1u; j < s; ++j) T[i * s + j] = (int8_t)((int)(t_rng(rng) % 3u) - 1);
        }
    }
    TW_SYNC();
    if (lane < s) {                                       // column `lane` of T^-1 (1/d = d for d = +-1)
        const uint32_t j = lane;
        for (uint32_t i = j + 1u; i-- > 0u;) {
            int64_t acc = i == j ? 1 : 0;
            for (uint32_t l = i + 1u; l <= j; ++l) acc -= (int64_t)T[i * s + l] * Ti[l * s + j];
            Ti[i * s + j] = (int64_t)T[i * s + i] * acc;
        }
        for (uint32_t i = j + 1u; i < s; ++i) Ti[i * s + j] = 0;
    }
    TW_SYNC();
    for (uint32_t e = lane; e < s * s; e += 64u) {        // M[P[i]][Q[j]] = T[i][j], M^-1[Q[i]][P[j]] = T^-1[i][j]
        const uint32_t i = e / s, j = e - i * s;
        const uint32_t mr = P[i], mc = Q[j], ir = Q[i], ic = P[j];
        fac_m[tr_m ? mc * s + mr : mr * s + mc] = o_val<MOD>(i <= j ? (int64_t)T[e] : 0, p);
        fac_i[tr_i ? ic * s + ir : ir * s + ic] = o_val<MOD>(Ti[e], p);
    }
    TW_SYNC();
}

// PLO_ORBIT_ACT_PLUQ: lane 0 draws Lambda (La) and the rows u_i, stored as the unit lower triangle Lu (row Q[i] = u_i); lanes
// 0.. and 32.. invert La and Lu by forward substitution, one lane per column; then over the s x s entries
// M[P[i]][c] = sum_j La[c][j] Lu[Q[i]][j] and M^-1[c][P[i]] = sum_j La^-1[j][c] Lu^-1[j][Q[i]].
template <bool MOD> __device__ void o_pluq(uint32_t s, bool base, uint32_t &rng, uint32_t lane, int8_t *La, int8_t *Lu, int64_t *Lai, int64_t *Lui, uint8_t *perm,
                                           int64_t *fac_m, bool tr_m, int64_t *fac_i, bool tr_i, uint64_t p)
{
    uint8_t *P = perm, *Q = perm + 16;
    if (lane == 0) {
        for (uint32_t i = 0; i < s; ++i) { P[i] = (uint8_t)i; Q[i] = (uint8_t)i; }
        for (uint32_t i = 0; i < s * s; ++i) { La[i] = 0; Lu[i] = 0; }
        if (base) for (uint32_t i = 0; i < s; ++i) { La[i * s + i] = 1; Lu[i * s + i] = 1; }
        else {
            o_perms(s, rng, P, Q);
            for (uint32_t i = 0; i < s; ++i) La[i * s + i] = (t_rng(rng) & 1u) ? 1 : -1;
            for (uint32_t i = 0; i < s; ++i) for (uint32_t j = 0; j < i; ++j) La[i * s + j] = (int8_t)((int)(t_rng(rng) % 3u) - 1);
            for (uint32_t i = 0; i < s; ++i) {
                const uint32_t q = Q[i];
                Lu[q * s + q] = 1;
                for (uint32_t j = 0; j < q; ++j) Lu[q * s + j] = (int8_t)((int)(t_rng(rng) % 3u) - 1);
            }
        }
    }
    TW_SYNC();
    if ((lane & 31u) < s) {                               // column j of La^-1 (lanes 0..s-1) and of Lu^-1 (lanes 32..32+s-1)
        const uint32_t j = lane & 31u;
        const int8_t *T = lane < 32u ? La : Lu;
        int64_t *Ti = lane < 32u ? Lai : Lui;
        for (uint32_t i = 0; i < j; ++i) Ti[i * s + j] = 0;
        for (uint32_t i = j; i < s; ++i) {
            int64_t acc = i == j ? 1 : 0;
            for (uint32_t l = j; l < i; ++l) acc -= (int64_t)T[i * s + l] * Ti[l * s + j];
            Ti[i * s + j] = (int64_t)T[i * s + i] * acc;
        }
    }
    TW_SYNC();
    for (uint32_t e = lane; e < s * s; e += 64u) {
        const uint32_t i = e / s, c = e - i * s, q = Q[i], r = P[i];
        int64_t a = 0, b = 0;
        for (uint32_t j = 0; j <= (c < q ? c : q); ++j) a += (int64_t)La[c * s + j] * (int64_t)Lu[q * s + j];
        for (uint32_t j = (c < q ? q : c); j < s; ++j) b += Lai[j * s + c] * Lui[j * s + q];
        fac_m[tr_m ? c * s + r : r * s + c] = o_val<MOD>(a, p);
        fac_i[tr_i ? r * s + c : c * s + r] = o_val<MOD>(b, p);
    }
    TW_SYNC();
}

// PLO_ORBIT_ACT_HOUSEHOLDER: lane 0 draws P, Q, the signs D and u; d = u.u.  N = diag(D) (I - 2 u u^T / d) when d is a unit
// (over Q: d != 0; modulo p: dinv[d] != 0), else diag(D); N^-1 = (I - 2 u u^T / d) diag(D).  M[P[i]][Q[j]] = N[i][j],
// M^-1[Q[i]][P[j]] = N^-1[i][j].  Over Q the factors hold the numerators d N, d N^-1 (sizes at most d) and d is returned (1 for
// the permutation branch, and always modulo p, where the factors are the residues themselves).
template <bool MOD> __device__ int64_t o_house(uint32_t s, bool base, uint32_t &rng, uint32_t lane, int8_t *u, uint8_t *perm,
                                               int64_t *fac_m, bool tr_m, int64_t *fac_i, bool tr_i, uint64_t p, const uint32_t *dinv)
{
    uint8_t *P = perm, *Q = perm + 16;
    int8_t *D = u + 16;
    if (lane == 0) {
        for (uint32_t i = 0; i < s; ++i) { P[i] = (uint8_t)i; Q[i] = (uint8_t)i; u[i] = 0; D[i] = 1; }
        if (!base) {
            o_perms(s, rng, P, Q);
            for (uint32_t i = 0; i < s; ++i) D[i] = (t_rng(rng) & 1u) ? 1 : -1;
            for (uint32_t i = 0; i < s; ++i) u[i] = (int8_t)((int)(t_rng(rng) % 3u) - 1);
        }
    }
    TW_SYNC();
    uint32_t d = 0;
    for (uint32_t i = 0; i < s; ++i) d += (uint32_t)((int)u[i] * (int)u[i]);
    const uint32_t inv = MOD ? dinv[d] : 0u;
    const bool refl = MOD ? inv != 0u : d != 0u;
    for (uint32_t e = lane; e < s * s; e += 64u) {
        const uint32_t i = e / s, j = e - i * s;
        const int64_t uu = 2 * (int)u[i] * (int)u[j], dl = i == j ? 1 : 0;
        int64_t h, hm, hi;                                // h = (d or 1) H[i][j]; hm = D[i] h, hi = h D[j]
        if constexpr (MOD) {
            h = refl ? (int64_t)(((uint64_t)dl + p - (uint64_t)o_val<true>(uu, p) * inv % p) % p) : dl;
            hm = D[i] < 0 && h ? (int64_t)p - h : h; hi = D[j] < 0 && h ? (int64_t)p - h : h;
        } else {
            h = refl ? dl * (int64_t)d - uu : dl;
            hm = D[i] * h; hi = h * D[j];
        }
        const uint32_t mr = P[i], mc = Q[j], ir = Q[i], ic = P[j];
        fac_m[tr_m ? mc * s + mr : mr * s + mc] = hm;
        fac_i[tr_i ? ic * s + ir : ir * s + ic] = hi;
    }
    TW_SYNC();
    return !MOD && refl ? (int64_t)d : 1;
}

template <bool MOD, int ACT = 0> __global__ __launch_bounds__(256) void orbit_kernel(OrbitPlan P, OrbitJob J)
{
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
    if constexpr (MOD && ACT == 2) { if (threadIdx.x < 17u) ((uint32_t *)(ldyn + P.off_dinv))[threadIdx.x] = P.dinv[threadIdx.x]; }
    __syncthreads();

    uint8_t *reg = ldyn + P.shared_bytes + (size_t)wave * P.lds_per_wave;
    auto fac = [&](uint32_t f) { return (int64_t *)(reg + P.off_fac[f]); };
    int64_t *Ti = (int64_t *)(reg + P.off_ti);
    int8_t *T = (int8_t *)(reg + P.off_t);
    uint8_t *perm = reg + P.off_perm;
    uint16_t *cnt = (uint16_t *)(reg + P.off_cnt);
    const uint32_t m = P.m, k = P.k, n = P.n, r = P.r;
    const uint64_t p = P.p;
    const bool canon = P.measure == 2u;

    uint64_t bkey = ~0ull, bidx = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * nw;
    for (uint64_t cnd = (uint64_t)blockIdx.x * nw + wave; cnd < J.ncand; cnd += stride) {
        const uint64_t seed = J.seeds ? J.seeds[cnd] : J.seed0 + cnd;
        const bool base = seed == ~0ull;
        uint32_t rng = 1u + (uint32_t)(t_splitmix(seed) % 2147483646ull);
        // U: U^-1 is A_L ([a][p] = U^-1[a][p]), U is A_P ([a][p] = U[p][a]); V: V is B_L, V^-1 is A_R ([b][p] = V^-1[p][b]);
        // W: W is B_R, W^-1 is B_P ([c][q] = W^-1[q][c])
        int64_t dU = 1, dV = 1, dW = 1;                  // Householder over Q: the denominators of U, V, W (wave-uniform)
        if constexpr (ACT == 0) {
            o_zoi<MOD>(m, base, rng, lane, T, Ti, perm, fac(4), true, fac(0), false, p);
            o_zoi<MOD>(k, base, rng, lane, T, Ti, perm, fac(1), false, fac(2), true, p);
            o_zoi<MOD>(n, base, rng, lane, T, Ti, perm, fac(3), false, fac(5), true, p);
        } else if constexpr (ACT == 1) {
            int64_t *Ti2 = (int64_t *)(reg + P.off_ti2);
            int8_t *T2 = (int8_t *)(reg + P.off_t2);
            o_pluq<MOD>(m, base, rng, lane, T, T2, Ti, Ti2, perm, fac(4), true, fac(0), false, p);
            o_pluq<MOD>(k, base, rng, lane, T, T2, Ti, Ti2, perm, fac(1), false, fac(2), true, p);
            o_pluq<MOD>(n, base, rng, lane, T, T2, Ti, Ti2, perm, fac(3), false, fac(5), true, p);
        } else {
            const uint32_t *dinv = (const uint32_t *)(ldyn + P.off_dinv);
            dU = o_house<MOD>(m, base, rng, lane, T, perm, fac(4), true, fac(0), false, p, dinv);
            dV = o_house<MOD>(k, base, rng, lane, T, perm, fac(1), false, fac(2), true, p, dinv);
            dW = o_house<MOD>(n, base, rng, lane, T, perm, fac(3), false, fac(5), true, p, dinv);
        }
        if (canon) { for (uint32_t e = lane; e < nrows; e += 64u) cnt[e] = 0; TW_SYNC(); }
        uint32_t nnz = 0, nno = 0;
#pragma unroll 1
        for (uint32_t part = 0; part < 3u; ++part) {
            const int64_t *A = fac(2u * part), *B = fac(2u * part + 1u);
            const uint32_t a_s = part == 1u ? k : m, b_s = part == 0u ? k : n, E = a_s * b_s, items = r * E, row0 = part * r;
            int64_t dd = 1;                               // the denominators of the part's factors: (U^-1, V), (V^-T, W), (U^T, W^-T)
            if constexpr (!MOD && ACT == 2) dd = part == 0u ? dU * dV : part == 1u ? dV * dW : dU * dW;
            for (uint32_t t = lane; t < items; t += 64u) {
                const uint32_t row = t / E, e = t - row * E, pp = e / b_s, qq = e - pp * b_s;
                const uint32_t g = row0 + row;
                int64_t acc = 0;
                for (uint32_t x = rp[g]; x < rp[g + 1u]; ++x) {
                    const uint32_t ps = pos[x], a = ps >> 8, b = ps & 0xFFu;
                    const int64_t fa = A[a * a_s + pp], fb = B[b * b_s + qq];
                    if (fa == 0 || fb == 0) continue;
                    if constexpr (MOD) {
                        const uint64_t ax = (uint64_t)fa * (uint64_t)val[x] % p;
                        acc += (int64_t)(ax * (uint64_t)fb % p);
                        if ((uint64_t)acc >= p) acc -= (int64_t)p;
                    } else acc += fa * val[x] * fb;
                }
                if (acc != 0) {
                    ++nnz;
                    bool one;
                    if constexpr (!MOD && ACT == 2) { const int64_t sc = scale[g] * dd; one = acc == sc || acc == -sc; }
                    else one = MOD ? (acc == 1 || (uint64_t)acc == p - 1u) : (acc == scale[g] || acc == -scale[g]);
                    nno += one ? 0u : 1u;
                    if (canon) atomicAdd((uint32_t *)(cnt + (g & ~1u)), (g & 1u) ? 0x10000u : 1u);
                }
            }
        }
        uint32_t single = 0;
        if (canon) {
            TW_SYNC();
            for (uint32_t e = lane; e < nrows; e += 64u) single += cnt[e] == 1u;
        }
        for (int o = 32; o >= 1; o >>= 1) {
            nnz += __shfl_xor(nnz, o, 64); nno += __shfl_xor(nno, o, 64); single += __shfl_xor(single, o, 64);
        }
        const uint32_t cost = canon ? nrows - single : nnz;
        if (lane == 0) {
            if (J.out3) { J.out3[3u * cnd] = cost; J.out3[3u * cnd + 1u] = nnz; J.out3[3u * cnd + 2u] = nno; }
            const uint64_t key = ((uint64_t)cost << 42) | ((uint64_t)nnz << 21) | (uint64_t)nno;
            if (key < bkey) { bkey = key; bidx = cnd; }       // candidates come in increasing order: ties keep the first
        }
        TW_SYNC();
    }
    if (J.best && lane == 0) {
        const uint64_t slot = (uint64_t)blockIdx.x * nw + wave;
        J.best[2u * slot] = bkey; J.best[2u * slot + 1u] = bidx;
    }
}

} // namespace plo
