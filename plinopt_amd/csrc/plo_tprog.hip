// ==========================================================================
// plo_tprog.hip -- every equation of an in-place trilinear program (bin/TPchecker) on gfx950: a wave-uniform interpreter of the
// program with the unit inputs spread over the lanes (the definition is plo_tprog.hpp's host loop).
//
// The program is a stream of records of four words (op, dst, src, coefficient residue), fetched 64 at a time, one per lane, and
// then taken in turn by the whole wave.  A lane keeps its state words in the wave's LDS region as [variable][lane]: consecutive
// lanes meet consecutive banks, no lane reads another lane's words, so the kernels have no barrier of any kind.
//
//   tprog_linear_kernel  the three families a, b, c on their own: a lane owns one unit input e_i of one family and runs that
//     family's ADD and SCA records (c: without the AXPYs).  At AXPY number s the wave stores its operand, a_I (or b_J), to row s
//     of the family's table, alpha[s][i] (beta[s][j]): lanes write consecutive words.  At the end the state is compared with
//     column i of the identity: the blocks A, B and C.
//   tprog_bilinear_kernel  the c family on the inputs (e_i, e_j), c = 0: a wave owns one i and 64 consecutive j.  An AXPY
//     adds coef alpha[s][i] beta[s][j] to its slot; the factor coef alpha[s][i] is one word for the whole wave, computed by the
//     lane that fetched the record, and a record whose factor is zero is passed over by the whole wave (most are).  So are the
//     ADD and SCA records that read a slot which no AXPY or ADD of this wave has written yet: one bit per slot, spread over
//     the lanes.  The target is no table: the host has appended it as AXPY records with the coefficients -P[z][t] and rows
//     alpha = L[t][.],
//     beta = R[t][.], so at the end every state word must be zero.  With -e the width is 2 nc: the low slots, then the hig ones.
//
// A wave that found violations adds their number to one 64-bit counter and offers its smallest one to a 64-bit atomic minimum on
// (equation - first equation of the launch) << 32 | residue, as the Brent kernel does: the result does not depend on
// scheduling.  Vector stores and atomics only.  31-bit residues, cob_mul.
// ==========================================================================
#pragma once
#include "plo_tril.hip"                 // cob_mul is plo_cob.hip's, which plo_capi.hip includes first (as for plo_brent.hip)
#include "../../include/plinopt_hip.h"

namespace plo {

// op: PLO_TPROG_ADD st[dst] += coef st[src]; PLO_TPROG_SCA st[dst] *= coef; 2: in a linear stream, store st[src] to row dst of
// the table; in the bilinear stream, st[dst] += coef alpha[src][i] beta[src][j]
struct TProgFamily {
    const uint4 *recs; uint32_t nrec;
    uint32_t n, nblk;                // unit inputs, and ceil(n / 64) waves
    uint32_t *table;                 // rows of n words (null for c: its stream has no store)
    uint32_t ebase;                  // the block's first equation, counted from E0
};
struct TProgLinJob {
    TProgFamily fam[3];
    uint32_t q; uint64_t mu;         // modulus and floor((2^64 - 1) / q) (cob_mul)
    uint32_t words;                  // state words per lane in a wave's region: max(na, nb, nc)
    unsigned long long *count, *first;
};
struct TProgPlan {
    uint32_t na, nb, w, nblk;        // nblk = ceil(nb / 64): the unit i nblk + jb is the wave of i and j = 64 jb .. 64 jb + 63
    uint32_t q; uint64_t mu;
    const uint4 *recs; uint32_t nrec;
    const uint32_t *alpha, *beta;    // rows of na and of nb words
    uint32_t skip;                   // 1: pass over the ADD and SCA records whose slot is still zero in every lane (0: PLO_TPROG_SKIP=0, to measure it)
};
struct TProgJob {
    uint64_t pair0, pair1;           // lanes whose pair lies outside compare nothing
    uint64_t unit0; uint32_t nunits; // the launch's waves
    uint64_t pairbase;               // the first pair of unit0: (pair - pairbase) w + z stays below 2^32
    unsigned long long *count, *first;
};

__device__ __forceinline__ void tprog_report(uint32_t lane, uint32_t nviol, unsigned long long best, unsigned long long *count, unsigned long long *first)
{
    for (int o = 32; o >= 1; o >>= 1) {
        nviol += __shfl_xor(nviol, o, 64);
        const unsigned long long ob = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)best, o, 64);
        best = min(best, ob);
    }
    if (lane == 0 && nviol) { atomicAdd(count, (unsigned long long)nviol); atomicMin(first, best); }
}

// word x of lane k, k the same in every lane
__device__ __forceinline__ uint32_t tprog_lane(uint32_t x, uint32_t k) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)k); }

__global__ __launch_bounds__(256) void tprog_linear_kernel(TProgLinJob J)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    uint32_t u = blockIdx.x * W + wave;
    uint32_t f = 0;
    while (f < 3u && u >= J.fam[f].nblk) { u -= J.fam[f].nblk; ++f; }
    if (f == 3u) return;                                            // (the kernel has no workgroup barrier)
    const TProgFamily F = J.fam[f];
    const uint32_t q = J.q, n = F.n, i = u * 64u + lane; const uint64_t mu = J.mu;
    const bool live = i < n;
    uint32_t *st = (uint32_t *)ldyn + (size_t)wave * J.words * 64u + lane;   // st[64 x]: variable x of this lane
    for (uint32_t x = 0; x < n; ++x) st[64u * x] = x == i ? 1u : 0u;
    for (uint32_t base = 0; base < F.nrec; base += 64u) {
        const uint32_t cnt = min(64u, F.nrec - base);
        uint4 mine = make_uint4(0u, 0u, 0u, 0u);
        if (lane < cnt) mine = F.recs[base + lane];
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t op = tprog_lane(mine.x, k), dst = tprog_lane(mine.y, k), src = tprog_lane(mine.z, k), co = tprog_lane(mine.w, k);
            if (op == PLO_TPROG_ADD) {
                uint32_t v = st[64u * dst] + cob_mul(co, st[64u * src], q, mu);
                if (v >= q) v -= q;
                st[64u * dst] = v;
            } else if (op == PLO_TPROG_SCA) st[64u * dst] = cob_mul(co, st[64u * dst], q, mu);
            else if (live) F.table[(size_t)dst * n + i] = st[64u * src];
        }
    }
    uint32_t nviol = 0; unsigned long long best = ~0ull;            // per lane
    if (live) for (uint32_t x = 0; x < n; ++x) {
        const uint32_t v = st[64u * x];
        if (v != (x == i ? 1u : 0u)) { ++nviol; best = min(best, ((unsigned long long)(F.ebase + x * n + i) << 32) | v); }
    }
    tprog_report(lane, nviol, best, J.count, J.first);
}

__global__ __launch_bounds__(256) void tprog_bilinear_kernel(TProgPlan P, TProgJob J)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    const uint32_t rel = blockIdx.x * W + wave;
    if (rel >= J.nunits) return;                                    // (the kernel has no workgroup barrier)
    const uint64_t unit = J.unit0 + rel;
    const uint32_t i = (uint32_t)(unit / P.nblk), j = (uint32_t)(unit - (uint64_t)i * P.nblk) * 64u + lane;
    const uint64_t pair = (uint64_t)i * P.nb + j;
    const bool live = j < P.nb && pair >= J.pair0 && pair < J.pair1;
    const uint32_t q = P.q, w = P.w, jj = min(j, P.nb - 1u); const uint64_t mu = P.mu;
    uint32_t *st = (uint32_t *)ldyn + (size_t)wave * w * 64u + lane;
    for (uint32_t z = 0; z < w; ++z) st[64u * z] = 0u;
    uint32_t live_slots = 0u;                                       // lane l, bit b: slot 64 b + l may be non-zero in some lane (w <= 512: 8 bits)
    for (uint32_t base = 0; base < P.nrec; base += 64u) {
        const uint32_t cnt = min(64u, P.nrec - base);
        uint4 mine = make_uint4(0u, 0u, 0u, 0u);
        uint32_t fac = 0u;                                          // an AXPY's coef alpha[s][i]; 1 for the other records
        if (lane < cnt) {
            mine = P.recs[base + lane];
            fac = mine.x == PLO_TPROG_AXPY ? cob_mul(mine.w, P.alpha[(size_t)mine.z * P.na + i], q, mu) : 1u;
        }
        unsigned long long todo = __ballot(fac != 0u);
        while (todo) {
            const int k = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t op = tprog_lane(mine.x, (uint32_t)k), dst = tprog_lane(mine.y, (uint32_t)k), src = tprog_lane(mine.z, (uint32_t)k), co = tprog_lane(mine.w, (uint32_t)k);
            if (op == PLO_TPROG_AXPY) {
                const uint32_t fk = tprog_lane(fac, (uint32_t)k);
                uint32_t v = st[64u * dst] + cob_mul(fk, P.beta[(size_t)src * P.nb + jj], q, mu);
                if (v >= q) v -= q;
                st[64u * dst] = v;
            } else if (op == PLO_TPROG_ADD) {
                if (P.skip && !((tprog_lane(live_slots, src & 63u) >> (src >> 6)) & 1u)) continue;   // the source is zero in every lane
                uint32_t v = st[64u * dst] + cob_mul(co, st[64u * src], q, mu);
                if (v >= q) v -= q;
                st[64u * dst] = v;
            } else {
                if (P.skip && !((tprog_lane(live_slots, dst & 63u) >> (dst >> 6)) & 1u)) continue;
                st[64u * dst] = cob_mul(co, st[64u * dst], q, mu);
                continue;
            }
            if (lane == (dst & 63u)) live_slots |= 1u << (dst >> 6);
        }
    }
    uint32_t nviol = 0; unsigned long long best = ~0ull;            // per lane
    if (live) for (uint32_t z = 0; z < w; ++z) {
        const uint32_t v = st[64u * z];
        if (v != 0u) { ++nviol; best = min(best, (((pair - J.pairbase) * w + z) << 32) | v); }
    }
    tprog_report(lane, nviol, best, J.count, J.first);
}

} // namespace plo
