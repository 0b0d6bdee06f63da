// t41_sdr_amd/csrc/tx_cw_kernel.hip -- gfx950 kernel of the T41 CW exciter, CW_ExciterIQData() (CW_Excite.cpp:66-118):
// tx_interp.hpp's stored-tone exciter, keyed and with the x 20, fed from cosBuffer2 / sinBuffer2 x 0.127 (:69-70).  The TX
// IQ correction's signs are the opposite of ExciterIQData()'s and there is no Q x 1.00 (:77-87); the host side sets them.
// A translation unit of its own (tx_cw_kernel.o); tx_host.cpp sees it through tx_internal.hpp.
#include <hip/hip_runtime.h>

#include "tx_interp.hpp"

namespace t41 {

__global__ __launch_bounds__(64) void tx_cw_kernel(const TxCwArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kInterpFloats];
  if ((int)blockIdx.x >= a.nchan) return;
  tone_exciter<true, true>(a, lds, 0.127f, a.i_scale, a.iq_phase, a.key);
}

hipError_t launch_tx_cw(const TxCwArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tx_cw_kernel, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
