// ===========================================================================
// plo_kmethod_batch.hip -- gfx950 kernels: the kernel method (plo_kmethod.hip) on MANY matrices in one launch, one minimum
// each (plo_kernel_batch_search; bin/pruner -K re-optimizes hundreds of small windows of a program, a few hundred restarts each).
//
// One WORKGROUP per problem, as in plo_cse_batch.hip: its waves share the row starts of the problem's M in LDS, staged once per
// problem between two barriers, and wave w runs restarts j = w, w + waves, ... of the problem's `per`: kmethod_candidate of
// plo_kmethod.hip, unchanged, with seed = decomposition seed = seed0 + q*per + j (per_block = 1: plo_oracle_kernel_restart(seed)).
// The workgroup reduces to one packed (cost key, j) through LDS and the one wave that holds the minimum stores the problem's
// result: a problem belongs to exactly one workgroup, so there is no global atomic on the way.  Workgroups stride over the
// problems of a launch; the host launches once per bucket of LDS footprints (plo_capi.hip, plo_kernel_batch_search).
//
// LDS: [0,64) reduction scratch (8 waves at most) | rsM[rsmax] | per wave one slot of `slot` bytes, the bucket's largest
// region + scratch_bytes.  A problem addresses its scratch at reg + K.region of its OWN plan -- off_depc is relative to that --
// only the stride between the waves' slots is the bucket's.  K.rsD and PD.rs_bytes are not used: Dep's row starts are per
// restart, in the wave's scratch.
//
// What a previous problem of the same workgroup left in LDS is never read.  The single-plan kernel gives the same guarantee for
// arbitrary contents, not only for those of its own plan: the first restart of each of its waves starts on whatever an earlier
// kernel left in the CU's LDS, and every restart builds M's image over what Dep's Optimizer call -- another plan, another
// layout -- left there.  In detail: a problem stages its own m+1 row starts and reads no further; a restart loads its own
// template; the elimination writes V (n of n+1 words a row) and C (rank of rank+1 words a row) of its m rows before it reads
// them and reads no padding word; ord, piv, basis, deps, depc, vrow and rsd[0..kept] are written by the restart that reads
// them (deps and depc for the K.ndeps rows of this plan, vrow for its rank columns); Dep's build clears its table, the masks of
// its m columns and the lengths of its PD.m rows, and a row past `kept` keeps length 0, so its stale row start is never added to
// an index that is loaded; the rest of a region (created columns' masks, tie list, multiplier list) is written before it is
// read, as between the two Optimizer calls of one restart.
//
// A failed candidate (ERR_KDEC, ERR_TABLE in err[q]) returns cost 0 and may win the reduction: the host discards slot q
// whenever err[q] != 0 and, for ERR_TABLE, runs that problem again alone, which rewrites the slot.
//
// UNITM is a run-time branch per problem, as in cse_batch_kernel: both instantiations of kmethod_candidate in one kernel.  The
// registers are those of the larger one and there is no scratch (DESIGN.md 2.11 has the compiler's figures); buckets split by
// PM.unit would double the launches of a call whose problems are a few hundred restarts each.
// ===========================================================================
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plo {      // (plo_capi.hip includes plo_kmethod.hip before this file)

struct KBatchProb {
    KPlan K;
    uint32_t q;             // the problem's index in the caller's arrays: seeds seed0 + q*per + j, results in slot q
};

struct KBatchJob {
    const KBatchProb *probs; uint32_t nprob;     // the problems of this launch
    uint32_t per, cost_mode;                     // restarts per problem
    uint32_t nsample;                            // sizing launch: the first nsample <= per restarts of every problem are decomposed
    uint64_t seed0;
    uint32_t rsmax, slot;                        // bytes: the launch's largest row-start image of M and wave slot (region + scratch)
    unsigned long long *keys;                    // [slot q] packed (cost key << 32 | seed offset j) of the problem's minimum
    uint32_t *adds, *muls;                       // [slot q] the winner's counts
    uint32_t *err;                               // [slot q] device error word of the problem (ERR_*)
    uint32_t *sz;                                // sizing launch: [slot q][4] as kmethod_size_kernel's sz (pairs, entries, no dependent row)
};

__global__ __launch_bounds__(512) void kmethod_batch_kernel(KBatchJob J)
{
    extern __shared__ uint64_t lds64[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint16_t *rsM = (uint16_t *)((uint8_t *)lds64 + 64u);
    uint8_t *reg = (uint8_t *)lds64 + 64u + J.rsmax + (size_t)wave * J.slot;
    for (uint32_t k = blockIdx.x; k < J.nprob; k += gridDim.x) {            // k depends on the workgroup only: the barriers below are uniform
        const KBatchProb &B = J.probs[k];
        const KPlan &K = B.K;
        const uint32_t q = B.q, twM = K.PM.tmpl_bytes >> 3, rwM = K.PM.rs_bytes >> 3;
        __syncthreads();                                                    // the previous problem: every wave is done with its row starts and the scratch
        for (uint32_t i = threadIdx.x; i < rwM; i += blockDim.x) ((uint64_t *)rsM)[i] = K.PM.tmpl[twM + i];
        __syncthreads();
        uint8_t *scr = reg + K.region;
        uint64_t best = ~0ull; uint32_t ba = 0, bm = 0;
        for (uint32_t j = wave; j < J.per; j += nwaves) {                   // a wave beyond `per` has no candidate and keeps ~0
            const uint64_t seed = J.seed0 + (uint64_t)q * J.per + j;
            const uint64_t res = K.PM.unit ? kmethod_candidate<true, false>(K, reg, scr, rsM, nullptr, seed, seed, lane, J.err + q, nullptr)
                                           : kmethod_candidate<false, false>(K, reg, scr, rsM, nullptr, seed, seed, lane, J.err + q, nullptr);
            const uint32_t a = (uint32_t)(res >> 32), mu_ = (uint32_t)res;
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

// Sizing launch of a batch: the decompositions of the first J.nsample restarts of every problem; sz[4q + 0] = max over them of the
// number of pairs of Dep, sz[4q + 1] = max entries of Dep, sz[4q + 2] = 1 when a decomposition found no dependent row (as
// kmethod_size_kernel).  K.region here is the region before Dep is laid out (M's image, the elimination arrays, the combinations).
__global__ __launch_bounds__(512) void kmethod_batch_size_kernel(KBatchJob J)
{
    extern __shared__ uint64_t lds64[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint16_t *rsM = (uint16_t *)((uint8_t *)lds64 + 64u);
    uint8_t *reg = (uint8_t *)lds64 + 64u + J.rsmax + (size_t)wave * J.slot;
    for (uint32_t k = blockIdx.x; k < J.nprob; k += gridDim.x) {
        const KBatchProb &B = J.probs[k];
        const KPlan &K = B.K;
        const uint32_t q = B.q, twM = K.PM.tmpl_bytes >> 3, rwM = K.PM.rs_bytes >> 3;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < rwM; i += blockDim.x) ((uint64_t *)rsM)[i] = K.PM.tmpl[twM + i];
        __syncthreads();
        const KScratch S = kscratch(K, reg + K.region);
        uint32_t pmax = 0, emax = 0, none = 0;
        for (uint32_t j = wave; j < J.nsample; j += nwaves) {
            const uint64_t seed = J.seed0 + (uint64_t)q * J.per + j;        // the search's own seeds
            for (uint32_t i = lane; i < twM; i += 64u) ((uint64_t *)reg)[i] = K.PM.tmpl[i];
            PLO_WAVE_SYNC();
            uint32_t ni = 0;
            const uint32_t kept = kmethod_decompose<false>(K, reg, S, rsM, seed, lane, ni);
            if (kept == 0u) { none = 1u; continue; }
            uint32_t pairs = 0, ent = 0;
            for (uint32_t r = 0; r < kept; ++r) {
                const uint32_t ln = kmethod_dep_row(K, S, r, lane);
                pairs += ln * (ln - (ln ? 1u : 0u)) / 2u; ent += ln;
            }
            pmax = pairs > pmax ? pairs : pmax; emax = ent > emax ? ent : emax;
            PLO_WAVE_SYNC();
        }
        if (lane == 0) { atomicMax(&J.sz[4u * q], pmax); atomicMax(&J.sz[4u * q + 1u], emax); if (none) atomicMax(&J.sz[4u * q + 2u], 1u); }
    }
}

} // namespace plo
