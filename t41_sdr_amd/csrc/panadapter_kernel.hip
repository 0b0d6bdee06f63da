// t41_sdr_amd/csrc/panadapter_kernel.hip -- the panadapter stage (t41rx_set_panadapter): what ShowSpectrum() draws, per
// receiver and at the firmware's cadence.  A translation unit of its own (panadapter_kernel.o), like the other stages'
// kernels (a kernel that joins display_kernel's translation unit moves that kernel's LDS and with it its code); host
// side: rx_display.cpp.
//
// One 64-lane wave = one channel, all the update frames (updateDisplayFlag == 1) of a process call: their rows of the
// compact dbg_pre tap, which rx512_kernel's tap instantiations wrote for exactly those frames (RxArgs::tap_period).  Per
// row, in the firmware's order and with contraction off:
//   CalcZoom1Magn() (spectrumZoom 0) / ZoomFFTExe() (1..4) up to FFT_spec     FFT.cpp:67-152, 208-243   display_kernel's
//                                                                              transform: zoom_fft.hpp, fft512, zoom_lowpass
//   pixelold[] = the row before's pixelnew[]                                  FFT.cpp:151, 216, Display.cpp:368, 472
//   pixelnew[x] = baseOffset + pixel_offset + (int16_t)(dBScale * log10f_fast(FFT_spec[x]))   FFT.cpp:157, 245
//   y_new = spectrumNoiseFloor - pixelnew[x] - currentNF, y_old = .. - pixelold[x] - oldNF, both held to
//     [SPECTRUM_TOP_Y, SPECTRUM_BOTTOM] = [100, 249]                          Display.cpp:250-256, 343-358
//   waterfall[x] = gradient[230 - y_new held to 0 .. 116], x = 0 .. 510       Display.cpp:460-466   ([511] is never written: 0)
//   oldNF = currentNF                                                         Display.cpp:474
//   dbm, the TCVSDR_SMETER form, from the row's audioMaxSquaredAve            Display.cpp:959-962, 980-981
// Lane l holds bins l + 64 r, i.e. display columns x = (l + 64 r + 256) & 511, r = 0..7, of everything: FFT_spec_old and
// pixelold stay in registers from row to row and go back to the channel's memory once per launch.
#include "display_pixel.hpp"
#include "rx_device.hpp"
#include "zoom_fft.hpp"

namespace t41 {

namespace {

constexpr int kSpectrumTopY = 100, kSpectrumBottom = 249;  // SPEC_BOX_T + 1, SPECTRUM_TOP_Y + SPECTRUM_HEIGHT - 1 (Display.h:13-22)

// the zoom chain's LDS, only where a zoom chain runs: spectrumZoom 0 keeps to the FFT's exchange buffer
template <bool ZOOMED>
struct PanZoomLds {
  float stage[2][2048];  // I / Q after the Fs/4 shift
  float ring[2][512];
  float dec[2][512];     // decimated samples of this row
};
template <>
struct PanZoomLds<false> {};

__device__ __forceinline__ int pan_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// DrawSmeterBar() with TCVSDR_SMETER (Display.cpp:959-962, 980-981): dbm_calibration + gainCorrection + (float32_t)attenuator
// + slope * log10f_fast(audioMaxSquaredAve) + cons in float, left to right; then - (float32_t)RFgain * 1.5 (a double
// product) and - rfGainAllBands in double; stored to the float dbm
__device__ __forceinline__ float pan_dbm(float gain_correction, int attenuator, float ave, int RFgain, int rfGainAllBands) {
#pragma clang fp contract(off)
  const float dbm_calibration = 22.0f, slope = 10.0f, cons = -92.0f;
  float t = dbm_calibration + gain_correction;
  t = t + (float)attenuator;
  t = t + slope * log10f_fast(ave);
  t = t + cons;
  double d = (double)t - (double)(float)RFgain * 1.5;
  d = d - (double)rfGainAllBands;
  return (float)d;
}

}  // namespace

// panadapter_kernel<ZOOMED>, and its list form under a panadapter map (t41rx_set_panadapter_map): the text is
// panadapter_kernel.inc
#define T41_STAGE_KERNEL panadapter_kernel
#define T41_STAGE_ARGS PanArgs
#define T41_STAGE_LIST 0
#include "panadapter_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL panadapter_list_kernel
#define T41_STAGE_ARGS PanListArgs
#define T41_STAGE_LIST 1
#include "panadapter_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST

hipError_t launch_panadapter(const PanArgs &a, hipStream_t s) {
  const dim3 grid(a.nchan), block(64);
  if (a.zoom > 0) hipLaunchKernelGGL(panadapter_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(panadapter_kernel<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

// the list form: one wave per entry; nobody listed launches nothing (a grid of zero blocks is a launch error)
hipError_t launch_panadapter_list(const PanListArgs &a, hipStream_t s) {
  if (a.nlist <= 0) return hipSuccess;
  const dim3 grid(a.nlist), block(64);
  if (a.zoom > 0) hipLaunchKernelGGL(panadapter_list_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(panadapter_list_kernel<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
