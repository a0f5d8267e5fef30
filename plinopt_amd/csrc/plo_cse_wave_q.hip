// ===========================================================================
// plo_cse_wave_q.hip -- the one-wave CSE kernel over Q, cse_wave_kernel<false, true> of plo_cse_wave.hip, as a translation unit of
// its own: the kernels of plo_capi.hip's unit then compile to exactly what they were without it (see the note in plo_cse_wave.hip).
// A +-1 matrix over Q needs no kernel of its own: it runs cse_wave_kernel<true> on a plan with p = 1 (plo_capi_cseq.hip).
// ===========================================================================
#define PLO_CSE_WAVE_Q_UNIT
#include "plo_cse_wave.hip"

namespace plo {

template __global__ void cse_wave_kernel<false, true>(WavePlan, WaveJob);

const void *cse_wave_q_kernel_fn() { return (const void *)cse_wave_kernel<false, true>; }

void cse_wave_q_launch(uint32_t grid, uint32_t block, uint32_t lds_bytes, hipStream_t stream, const WavePlan &P, const WaveJob &J)
{
    hipLaunchKernelGGL((cse_wave_kernel<false, true>), dim3(grid), dim3(block), lds_bytes, stream, P, J);
}

} // namespace plo
