// t41_sdr_amd/csrc/tx_cal_kernel.hip -- gfx950 kernel of the transmit half of the IQ calibration, ProcessIQData2()
// (Process2.cpp:309-349): tx_interp.hpp's stored-tone exciter, no key and no x 20 (:344-345), fed from cosBuffer3 /
// sinBuffer3 x bandOutputFactor (:313-314).  The TX IQ correction is per channel: LSB scales I by -IQXAmp, USB by +IQXAmp
// (:317-325).  A translation unit of its own (tx_cal_kernel.o); tx_host.cpp sees it through tx_internal.hpp.
#include <hip/hip_runtime.h>

#include "tx_interp.hpp"

namespace t41 {

__global__ __launch_bounds__(64) void tx_cal_kernel(const TxCalArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kInterpFloats];
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  // the channel's candidate, or the params' factors
  const float amp = a.corr ? a.corr[2 * (size_t)ch] : a.iq_amp;
  const float iq_phase = a.corr ? a.corr[2 * (size_t)ch + 1] : a.iq_phase;
  tone_exciter<false, false>(a, lds, a.level, a.lsb ? -amp : amp, iq_phase, nullptr);
}

hipError_t launch_tx_cal(const TxCalArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tx_cal_kernel, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
