// ===========================================================================
// plo_cse_batch.hip -- gfx950 kernel: MANY independent restart searches in one launch, one minimum each
// (plo_cse_batch_search; bin/pruner re-optimizes thousands of small windows of a program, a few hundred restarts each).
//
// One WORKGROUP per problem: its waves share the problem's row starts (and, chained, the second matrix's) in LDS, staged once
// per problem as cse_wave_kernel does for its single plan, and each wave runs run_candidate of plo_cse_wave.hip, unchanged, on
// its share of the problem's seeds.  The workgroup reduces to one packed (cost key, seed offset) and stores the problem's
// result itself: a problem belongs to exactly one workgroup, so there is no global atomic on the way.  Workgroups stride over
// the problems of a launch; the host launches once per bucket of LDS footprints (plo_capi.hip, plo_cse_batch_search).
//
// LDS: [0,64) reduction scratch (8 waves at most) | rs1[rs1max] | rs2[rs2max] | one candidate region per wave (the largest of the bucket).
// What a previous problem of the same workgroup left there is never read: a problem stages its own m+1 row starts and reads
// no further, every candidate loads its own template, and the rest of a region (created columns' masks, tie list, multiplier
// list) is written before it is read, as between the candidates of cse_chain_batch_kernel.
// ===========================================================================
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plo {      // (plo_capi.hip includes plo_cse_wave.hip before this file)

struct BatchProb {
    WavePlan P1, P2;        // P2 is used when chained
    uint32_t q;             // the problem's index in the caller's arrays: seeds seed0 + q*per + j, results in slot q
    uint32_t chained;
};

struct BatchJob {
    const BatchProb *probs; uint32_t nprob;      // the problems of this launch
    uint32_t per, cost_mode;
    uint64_t seed0;
    uint32_t rs1max, rs2max, region;             // bytes: the bucket's largest row-start images and candidate region
    unsigned long long *keys;                    // [slot q] packed (cost key << 32 | seed offset j) of the problem's minimum
    uint32_t *adds, *muls;                       // [slot q] the winner's counts
    uint32_t *err;                               // [slot q] device error word of the problem (ERR_*)
};

__global__ __launch_bounds__(512) void cse_batch_kernel(BatchJob J)
{
    extern __shared__ uint64_t lds64[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint16_t *rs1 = (uint16_t *)((uint8_t *)lds64 + 64u), *rs2 = (uint16_t *)((uint8_t *)lds64 + 64u + J.rs1max);
    uint8_t *reg = (uint8_t *)lds64 + 64u + J.rs1max + J.rs2max + (size_t)wave * J.region;
    for (uint32_t k = blockIdx.x; k < J.nprob; k += gridDim.x) {            // k depends on the workgroup only: the barriers below are uniform
        const BatchProb &B = J.probs[k];
        const WavePlan &P1 = B.P1, &P2 = B.P2;
        const uint32_t q = B.q, chained = B.chained;
        const uint32_t tw1 = P1.tmpl_bytes >> 3, rw1 = P1.rs_bytes >> 3;
        const uint32_t tw2 = chained ? P2.tmpl_bytes >> 3 : 0u, rw2 = chained ? P2.rs_bytes >> 3 : 0u;
        __syncthreads();                                                    // the previous problem: every wave is done with its row starts and the scratch
        for (uint32_t i = threadIdx.x; i < rw1; i += blockDim.x) ((uint64_t *)rs1)[i] = P1.tmpl[tw1 + i];
        for (uint32_t i = threadIdx.x; i < rw2; i += blockDim.x) ((uint64_t *)rs2)[i] = P2.tmpl[tw2 + i];
        __syncthreads();
        uint64_t best = ~0ull; uint32_t ba = 0, bm = 0;
        for (uint32_t j = wave; j < J.per; j += nwaves) {                   // a wave beyond `per` has no candidate and keeps ~0
            const uint64_t seed = J.seed0 + (uint64_t)q * J.per + j;
            PickState ps{1u + (uint32_t)(splitmix64(seed) % 2147483646ull), 0u, 0ull, 1ull, 0u};
            for (uint32_t i = lane; i < tw1; i += 64u) ((uint64_t *)reg)[i] = P1.tmpl[i];
            PLO_WAVE_SYNC();
            const uint64_t r1 = P1.unit ? run_candidate<true>(P1, reg, rs1, ps, lane, J.err + q) : run_candidate<false>(P1, reg, rs1, ps, lane, J.err + q);
            uint32_t a = (uint32_t)(r1 >> 32), mu_ = (uint32_t)r1;
            if (chained) {
                PLO_WAVE_SYNC();
                for (uint32_t i = lane; i < tw2; i += 64u) ((uint64_t *)reg)[i] = P2.tmpl[i];
                PLO_WAVE_SYNC();
                const uint64_t r2 = P2.unit ? run_candidate<true>(P2, reg, rs2, ps, lane, J.err + q) : run_candidate<false>(P2, reg, rs2, ps, lane, J.err + q);
                a += (uint32_t)(r2 >> 32); mu_ += (uint32_t)r2;
            }
            const uint64_t packed = ((uint64_t)cost_key32(a, mu_, J.cost_mode) << 32) | j;
            if (packed < best) { best = packed; ba = a; bm = mu_; }
            PLO_WAVE_SYNC();
        }
        if (lane == 0) lds64[wave] = best;
        __syncthreads();
        uint64_t b = lds64[0];
        for (uint32_t w = 1; w < nwaves; ++w) { const uint64_t x = lds64[w]; b = x < b ? x : b; }
        // offsets differ between waves, so exactly one wave holds the minimum (per >= 1: wave 0 always has a candidate)
        if (lane == 0 && best == b && b != ~0ull) { J.keys[q] = b; J.adds[q] = ba; J.muls[q] = bm; }
    }
}

} // namespace plo
