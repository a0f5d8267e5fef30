// ==========================================================================
// plo_dep.hip -- row-dependency enumeration (bin/dependency) on gfx950.
//
// Replaces `Explore` of the reference's dependency (src/dependency.cpp:74-101) under its driver loop (:158-165): every
// combination  M[i] + c_v1 M[q1] + c_v2 M[q2] + ...  (i < q1 < q2 < ..., coefficients from a list of C) of 2 .. L rows is
// formed, and the ones that vanish or have exactly one non-zero entry are reported (plo_dep_hit_t, include/plinopt_hip.h).
// Values are residues modulo p < 2^31 (over Q: modulo PLO_DEP_PRIME, a superset that the caller filters); M is dense,
// m x n with an odd row stride `ld` so that lanes reading different rows of it in LDS hit different banks.
//
// A task is a combination of two rows (i, q1, v1); a wave draws tasks from a counter (the subtrees of small i are by far
// the largest, and come first).  The wave forms the task's vector W_2 with one lane per column, tests it, and then walks
// the subtree depth-first: the vectors W_2 .. W_{L-1} of the path sit in its LDS region, and at every node the 64 lanes
// take 64 children (q, v) per step, each lane scanning the n columns of W_node + c_v M[q] and leaving at the second
// non-zero.  So every combination is tested exactly once, as a child of its prefix; only the inner nodes (sizes below L)
// cost a cooperative axpy.  Hits are appended through one vector atomicAdd on a counter that keeps counting past the
// buffer's capacity; the host sorts them into the reference's order.
// ==========================================================================
#pragma once
#include "plo_orbit.hip"
#include "../../include/plinopt_hip.h"

namespace plo {

struct DepPlan {
    uint32_t m, n, ld, C, L;         // ld: row stride of M (odd, >= n); L: largest combination (2 .. 8)
    uint32_t p; uint64_t mu;         // modulus and floor((2^64 - 1) / p) (cob_mul)
    const uint32_t *M;               // m x ld residues
    const uint32_t *coef;            // C residues
    // LDS layout (bytes): M (when it fits), the coefficients, then lds_per_wave per wave: nvec vectors of n, the path (2 x 8 words)
    uint32_t off_coef, off_wave, nvec, lds_per_wave;
};
struct DepJob {
    uint32_t row0, nrows;            // top rows row0 .. row0 + nrows - 1
    const uint64_t *toff;            // nrows + 1 task offsets: tasks of top row row0 + r are toff[r] .. toff[r + 1] - 1
    uint64_t ntasks;
    unsigned long long *next;        // task counter
    unsigned long long *count;       // hit counter
    plo_dep_hit_t *hits; uint64_t cap;
};

// Appends the combination path[0 .. depth) + (q, v): path holds (row, coefficient index) pairs
__device__ __forceinline__ void dep_emit(const DepJob &J, const uint32_t *path, uint32_t depth, uint32_t q, uint32_t v, uint32_t kind, uint32_t col, uint32_t val)
{
    const unsigned long long slot = atomicAdd(J.count, 1ull);
    if (slot >= J.cap) return;
    plo_dep_hit_t *o = J.hits + slot;
    o->size = depth + 1u; o->kind = kind; o->col = col; o->residue = val;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)PLO_DEP_MAX_LEVEL; ++k) {
        const bool in = k < depth, me = k == depth;
        o->rows[k] = (uint16_t)(in ? path[2u * k] : (me ? q : 0u));
        o->coef[k] = (uint8_t)(in ? path[2u * k + 1u] : (me ? v : 0u));
    }
}

// dst = src + c * M[q], one lane per column (dst is another vector than src)
__device__ __forceinline__ void dep_axpy(uint32_t *dst, const uint32_t *src, uint32_t c, const uint32_t *Mq, uint32_t n, uint32_t lane, uint32_t p, uint64_t mu)
{
    for (uint32_t col = lane; col < n; col += 64u) {
        uint32_t x = src[col] + cob_mul(c, Mq[col], p, mu);
        if (x >= p) x -= p;
        dst[col] = x;
    }
    TW_SYNC();
}

// The children (q, v), last < q < m, of the node whose vector is W and whose path has `depth` rows: 64 per step, a lane each
__device__ __forceinline__ void dep_children(const DepPlan &P, const DepJob &J, const uint32_t *Mm, const uint32_t *cf, const uint32_t *W, const uint32_t *path,
                                             uint32_t depth, uint32_t last, uint32_t lane)
{
    const uint32_t n = P.n, C = P.C, p = P.p; const uint64_t mu = P.mu;
    const uint32_t nch = (P.m - 1u - last) * C;
    for (uint32_t k = lane; k < nch; k += 64u) {
        const uint32_t dq = k / C, v = k - dq * C, q = last + 1u + dq;
        const uint32_t c = cf[v];
        const uint32_t *Mq = Mm + (size_t)q * P.ld;
        uint32_t cnt = 0, pos = 0, val = 0;
        for (uint32_t col = 0; col < n; ++col) {
            uint32_t x = W[col] + cob_mul(c, Mq[col], p, mu);
            if (x >= p) x -= p;
            if (x) { if (++cnt == 2u) break; pos = col; val = x; }
        }
        if (cnt < 2u) dep_emit(J, path, depth, q, v, cnt, pos, val);
    }
}

template <bool MLDS> __global__ __launch_bounds__(256) void dep_kernel(DepPlan P, DepJob J)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t ldyn[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t m = P.m, n = P.n, ld = P.ld, C = P.C, L = P.L, p = P.p; const uint64_t mu = P.mu;
    uint32_t *cf = (uint32_t *)(ldyn + P.off_coef);
    const uint32_t *Mm = P.M;
    if constexpr (MLDS) {
        uint32_t *ml = (uint32_t *)ldyn;
        for (uint32_t e = threadIdx.x; e < m * ld; e += blockDim.x) ml[e] = P.M[e];
        Mm = ml;
    }
    for (uint32_t e = threadIdx.x; e < C; e += blockDim.x) cf[e] = P.coef[e];
    __syncthreads();
    uint32_t *Wb = (uint32_t *)(ldyn + P.off_wave + (size_t)wave * P.lds_per_wave);   // the vector of a node of d rows: Wb + (d - 2) n
    uint32_t *path = Wb + P.nvec * n;

    for (;;) {
        unsigned long long t = 0;
        if (lane == 0) t = atomicAdd(J.next, 1ull);
        t = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(t >> 32), 0, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)t, 0, 64);
        if (t >= J.ntasks) break;
        uint32_t lo = 0, hi = J.nrows;                    // toff[lo] <= t < toff[hi]
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (J.toff[mid] <= t) lo = mid; else hi = mid; }
        const uint32_t i = J.row0 + lo, rem = (uint32_t)(t - J.toff[lo]), dq = rem / C, v1 = rem - dq * C, q1 = i + 1u + dq;
        TW_SYNC();                                        // the previous task's reads of the path and of W_2 are over
        if (lane == 0) { path[0] = i; path[1] = 0; path[2] = q1; path[3] = v1; }
        // W_2 = M[i] + c_v1 M[q1], tested by the whole wave: a lane counts the non-zeros of its columns
        uint32_t cnt = 0, pos = 0, val = 0;
        {
            const uint32_t c = cf[v1];
            const uint32_t *Mi = Mm + (size_t)i * ld, *Mq = Mm + (size_t)q1 * ld;
            for (uint32_t col = lane; col < n; col += 64u) {
                uint32_t x = Mi[col] + cob_mul(c, Mq[col], p, mu);
                if (x >= p) x -= p;
                Wb[col] = x;
                if (x) { ++cnt; pos = col; val = x; }
            }
        }
        TW_SYNC();
        uint32_t total = cnt;
        for (int o = 32; o >= 1; o >>= 1) total += __shfl_xor(total, o, 64);
        if (total == 0u) { if (lane == 0) dep_emit(J, path, 1u, q1, v1, PLO_DEP_ZERO, 0u, 0u); }
        else if (total == 1u && cnt == 1u) dep_emit(J, path, 1u, q1, v1, PLO_DEP_ONE, pos, val);
        if (L < 3u) continue;
        // depth-first over the inner nodes: d rows on the path, `fresh` when the node at d has just been formed
        uint32_t d = 2u; bool fresh = true;
        for (;;) {
            if (fresh) {
                const uint32_t last = path[2u * (d - 1u)];
                dep_children(P, J, Mm, cf, Wb + (d - 2u) * n, path, d, last, lane);
                if (d + 1u < L && last + 2u < m) {        // its first child becomes an inner node (one with children of its own)
                    TW_SYNC();
                    if (lane == 0) { path[2u * d] = last + 1u; path[2u * d + 1u] = 0u; }
                    dep_axpy(Wb + (d - 1u) * n, Wb + (d - 2u) * n, cf[0], Mm + (size_t)(last + 1u) * ld, n, lane, p, mu);
                    ++d;
                    continue;
                }
                fresh = false;
            }
            if (d == 2u) break;                           // the task's own node is done
            uint32_t q = path[2u * (d - 1u)], v = path[2u * (d - 1u) + 1u] + 1u;   // the next sibling of the node at d
            if (v == C) { v = 0u; ++q; }
            if (q + 1u < m) {
                TW_SYNC();
                if (lane == 0) { path[2u * (d - 1u)] = q; path[2u * (d - 1u) + 1u] = v; }
                dep_axpy(Wb + (d - 2u) * n, Wb + (d - 3u) * n, cf[v], Mm + (size_t)q * ld, n, lane, p, mu);
                fresh = true;
            } else --d;
        }
    }
}

} // namespace plo
