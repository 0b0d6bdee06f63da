// t41_sdr_amd/csrc/fastconv.hip -- the long-FFT fast convolution kernels' instantiations (fastconv_kernels.hpp).
#include "fastconv_kernels.hpp"
#include "rx_launch.hpp"

namespace t41 {

// one kFcWaves-wave workgroup per channel with LDS_FLOATS of dynamic LDS, which the runtime is told of once per kernel
template <auto KERNEL, int LDS_FLOATS>
static hipError_t launch_fc(const RxArgs &a, hipStream_t s) {
  constexpr size_t kLds = LDS_FLOATS * sizeof(float);
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(KERNEL, dim3(a.nchan), dim3(64 * kFcWaves), kLds, s, a);
  return hipGetLastError();
}

// real audio with the fixed gain, f32 samples out (`fused_back`): the interpolators run behind pass 3 of the fast
// convolution (no `aud24` round trip, no third kernel); cplx: AM / the AGC take the complex valid half
template <int R>
static hipError_t launch_fastconv_r(const RxArgs &a, bool cplx, bool fused_back, hipStream_t s) {
  if (cplx) return launch_fc<&fastconv_kernel<R, true>, fc_lds_floats(R)>(a, s);
  if (fused_back) return launch_fc<&fastconv_kernel<R, false, true>, fcb_lds_floats(R)>(a, s);
  return launch_fc<&fastconv_kernel<R, false>, fc_lds_floats(R)>(a, s);
}

hipError_t launch_fastconv(const RxArgs &a, bool cplx, bool fused_back, hipStream_t s) {
  return a.seg == 8 ? launch_fastconv_r<8>(a, cplx, fused_back, s)
       : a.seg == 4 ? launch_fastconv_r<4>(a, cplx, fused_back, s)
                    : launch_fastconv_r<2>(a, cplx, fused_back, s);
}

// FFT_LENGTH 4096, SSB audio with the fixed gain, f32 samples: the whole chain in one kernel
hipError_t launch_fastconv_fused(const RxArgs &a, const KernelForm &k, hipStream_t s) {
  // (an input map -- receiver groups -- selects the same kernel in its mapped form; no call without a map reaches it)
  return with_bools(
      [&](auto PLN, auto MAP) {
        if constexpr (MAP) return launch_fc<&fastconv_fused_map_kernel<PLN>, fcb_lds_floats(8)>(a, s);
        else return launch_fc<&fastconv_fused_kernel<PLN>, fcb_lds_floats(8)>(a, s);
      },
      k.plain, k.map_form);
}

T41RX_CLK_READER(t41rx_debug_read_clk_fc)
T41RX_BUILD_FLAGS(fastconv)

}  // namespace t41
