// Micro-benchmark behind DESIGN.md 2.2 (the hashes of the merge and the flush): issue rate of the integer instructions a hash can be
// built from -- v_add_u32 as the full-rate yardstick, the 24-bit products v_mul_u32_u24 / v_mad_u32_u24, and the 32-bit ones
// v_mul_lo_u32, v_mul_hi_u32 and v_mad_u64_u32 that `key * 64-bit constant` compiles to.  One kernel per class: 8 independent chains
// per lane, 4 waves per SIMD on every CU, a fixed trip count; the instructions are inline assembly so that the compiler can neither
// fold a chain nor pick another opcode.  Prints wave-instructions per clock per SIMD, from the waves' own cycle counters and, as a
// cross-check, from the HIP event time and the device's clock rate.
// Build: hipcc -O3 --offload-arch=gfx950 -o /tmp/int_mul_rate tests/micro/int_mul_rate.hip ; run: /tmp/int_mul_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#define CHAINS 8
#define CK(x_) do { if ((x_) != hipSuccess) { fprintf(stderr, "%s failed\n", #x_); exit(1); } } while (0)
#define REPS 4            /* instructions per chain and round */
template <int OP> __device__ __forceinline__ void step(uint32_t &x, uint64_t &w, uint32_t y, uint32_t z)
{
    if (OP == 0) asm volatile("v_add_u32 %0, %0, %1" : "+v"(x) : "v"(y));
    if (OP == 1) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(x) : "v"(y));
    if (OP == 2) asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(x) : "v"(y), "v"(z));
    if (OP == 3) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(x) : "v"(y));
    if (OP == 4) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(x) : "v"(y));
    if (OP == 5) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(w) : "v"(y), "v"(z) : "vcc");
}
template <int OP> __global__ __launch_bounds__(256) void k(uint32_t rounds, uint32_t seed, unsigned long long *cyc, uint32_t *sink)
{
    uint32_t x[CHAINS]; uint64_t w[CHAINS];
    const uint32_t y = (seed * 2654435761u + threadIdx.x) | 1u, z = seed ^ (blockIdx.x * 40503u);
#pragma unroll
    for (int u = 0; u < CHAINS; ++u) { x[u] = y + (uint32_t)u * 977u; w[u] = ((uint64_t)z << 32) | x[u]; }
    const unsigned long long t0 = clock64();
    for (uint32_t r = 0; r < rounds; ++r) {
#pragma unroll
        for (int q = 0; q < REPS; ++q) {
#pragma unroll
            for (int u = 0; u < CHAINS; ++u) step<OP>(x[u], w[u], y, z);
        }
    }
    const unsigned long long t1 = clock64();
    uint32_t acc = 0;
#pragma unroll
    for (int u = 0; u < CHAINS; ++u) acc += x[u] + (uint32_t)w[u] + (uint32_t)(w[u] >> 32);
    if ((threadIdx.x & 63u) == 0) atomicAdd(cyc, t1 - t0);
    if (acc == 0x1234567u) sink[0] = acc;
}
template <int OP> void run(const char *name, int cus, int khz, unsigned long long *d_cyc, uint32_t *sink)
{
    const uint32_t rounds = 4000, wg_per_cu = 4;          // 4 workgroups of 4 waves per CU: 4 waves per SIMD
    const uint32_t grid = (uint32_t)cus * wg_per_cu;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL((k<OP>), dim3(grid), dim3(256), 0, 0, 10u, 1u, d_cyc, sink);      // warm
    CK(hipMemset(d_cyc, 0, 8));
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((k<OP>), dim3(grid), dim3(256), 0, 0, rounds, 1u, d_cyc, sink);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    unsigned long long c = 0; CK(hipMemcpy(&c, d_cyc, 8, hipMemcpyDeviceToHost));
    const double per_wave = (double)rounds * REPS * CHAINS, waves = grid * 4.0;
    const double cyc_per_wave = (double)c / waves;
    const double by_counter = wg_per_cu * per_wave / cyc_per_wave;                        // 4 waves of a SIMD run side by side
    const double by_event = waves * per_wave / (cus * 4.0) / ((double)ms * khz);
    printf("%-14s %.3f wave-instructions per clock per SIMD by the waves' cycle counters (%.2f cycles per wave-instruction), %.3f by event time at %d MHz, kernel %.3f ms\n",
           name, by_counter, 1.0 / by_counter, by_event, khz / 1000, ms);
}
int main()
{
    hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    unsigned long long *d_cyc; uint32_t *sink;
    CK(hipMalloc(&d_cyc, 8)); CK(hipMalloc(&sink, 8));
    printf("%s, %d CUs, %d MHz; 8 chains per lane, 4 waves per SIMD, %d instructions per wave\n", pr.name, pr.multiProcessorCount, pr.clockRate / 1000, 4000 * REPS * CHAINS);
    run<0>("v_add_u32", pr.multiProcessorCount, pr.clockRate, d_cyc, sink);
    run<1>("v_mul_u32_u24", pr.multiProcessorCount, pr.clockRate, d_cyc, sink);
    run<2>("v_mad_u32_u24", pr.multiProcessorCount, pr.clockRate, d_cyc, sink);
    run<3>("v_mul_lo_u32", pr.multiProcessorCount, pr.clockRate, d_cyc, sink);
    run<4>("v_mul_hi_u32", pr.multiProcessorCount, pr.clockRate, d_cyc, sink);
    run<5>("v_mad_u64_u32", pr.multiProcessorCount, pr.clockRate, d_cyc, sink);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
