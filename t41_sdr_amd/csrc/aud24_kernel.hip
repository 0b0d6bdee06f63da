// t41_sdr_amd/csrc/aud24_kernel.hip -- aud24_finish_kernel: the audio @24 kS/s as a call's result (t41rx_set_audio_rate)
// behind the tap kernels and the chain-splitting stages.  Those leave float_buffer_L as it stands in front of
// Process.cpp:917 in the context's scratch, [channel][frame * 256]; this kernel takes the place of the interpolators:
// one multiply by g = VolumeToAmplification(audioVolume) (Process.cpp:929's arm_scale_f32 without DF, which only makes up
// for the zero stuffing), arm_float_to_q15 for the q15 entries (Process.cpp:936), and the store in the call's layout.
// A thread owns one 16-byte piece of the output (4 f32 or 8 q15 samples): a wave reads and writes consecutive addresses
// within a frame.  The fused kernels without taps store the same values themselves (rx512_kernel.hpp: A24).
#include <hip/hip_runtime.h>

#include "rx_kernels.hpp"

namespace t41 {

namespace {
// arm_float_to_q15 (CMSIS-DSP scalar path without ARM_MATH_ROUNDING): (q15_t)__SSAT((q31_t)(x * 32768.0f), 16); two of
// them packed, first sample in the low half -- rx_device.hpp's q15_pack2, which the 192 kS/s q15 output goes through
__device__ __forceinline__ unsigned q15_pack2(float x0, float x1) {
  int a = (int)(x0 * 32768.0f), b = (int)(x1 * 32768.0f);  // v_cvt_i32_f32: toward zero, saturating
  a = a < -32768 ? -32768 : (a > 32767 ? 32767 : a);
  b = b < -32768 ? -32768 : (b > 32767 ? 32767 : b);
  return ((unsigned)a & 0xffffu) | ((unsigned)b << 16);
}
}  // namespace

// OMAP (t41rx_set_output_map): the frame goes to row a.out_map[channel] of the output; a muted channel's threads leave
// before they read the audio.
template <bool Q15, bool OMAP>
__device__ __forceinline__ void aud24_finish_body(const Aud24Args &a) {
#pragma clang fp contract(off)
  constexpr int kPieces = Q15 ? 32 : 64;  // 16-byte pieces of a frame's 256 samples
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t frames = (size_t)a.nchan * (size_t)a.nframes;
  if (i >= frames * kPieces) return;
  const size_t job = i / kPieces;  // (channel, frame), frame fastest: the scratch's own order
  const int piece = (int)(i % kPieces);
  const size_t ch = job / (size_t)a.nframes, f = job % (size_t)a.nframes;
  const float *src = a.aud + job * 256;
  const int row = OMAP ? a.out_map[ch] : 0;
  if (OMAP && row < 0) return;
  const size_t o = (OMAP ? (size_t)row : ch) * (size_t)a.chan_stride + f * (size_t)a.frame_stride;  // samples
  const float g = a.coef[a.set_of ? a.set_of[ch] : 0].sc[kScOutScale] * 0.125f;  // (exact: DF = 8)
  if (!Q15) {
    const float4 x = *reinterpret_cast<const float4 *>(src + 4 * piece);
    *reinterpret_cast<float4 *>(static_cast<float *>(a.out) + o + 4 * piece) = make_float4(x.x * g, x.y * g, x.z * g, x.w * g);
  } else {
    const float4 lo = *reinterpret_cast<const float4 *>(src + 8 * piece), hi = *reinterpret_cast<const float4 *>(src + 8 * piece + 4);
    const uint4 q = make_uint4(q15_pack2(lo.x * g, lo.y * g), q15_pack2(lo.z * g, lo.w * g), q15_pack2(hi.x * g, hi.y * g), q15_pack2(hi.z * g, hi.w * g));
    *reinterpret_cast<uint4 *>(static_cast<int16_t *>(a.out) + o + 8 * piece) = q;
  }
}

template <bool Q15>
__global__ __launch_bounds__(256) void aud24_finish_kernel(const Aud24Args a) {
  aud24_finish_body<Q15, false>(a);
}
template <bool Q15>
__global__ __launch_bounds__(256) void aud24_finish_omap_kernel(const Aud24Args a) {
  aud24_finish_body<Q15, true>(a);
}

hipError_t launch_aud24_finish(const Aud24Args &a, hipStream_t s) {
  // (an output map without a listened channel comes with no audio buffer: no thread stores)
  if (a.nchan <= 0 || a.nframes <= 0 || !a.aud || (!a.out && !a.out_map) || !a.coef) return hipErrorInvalidConfiguration;
  const size_t pieces = (size_t)a.nchan * (size_t)a.nframes * (a.q15 ? 32 : 64);
  const dim3 grid((unsigned)((pieces + 255) / 256));
  if (a.out_map) {
    if (a.q15) hipLaunchKernelGGL(aud24_finish_omap_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(aud24_finish_omap_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  }
  if (a.q15) hipLaunchKernelGGL(aud24_finish_kernel<true>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(aud24_finish_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
