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

template <bool ZOOMED>
__global__ __launch_bounds__(64) void panadapter_kernel(const PanArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float xbuf[8 * kFftRow * 2];  // FFT exchange
  __shared__ PanZoomLds<ZOOMED> z;
  __shared__ unsigned short grad[128];
  const int lane = threadIdx.x;
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  constexpr int L = 2048, R = 512;
  float *ds = a.mem + (size_t)ch * kPanFloats;
  int *dsi = reinterpret_cast<int *>(ds);
  const cf *tab = reinterpret_cast<const cf *>(a.tab);
  cf tw1[7], tw2[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    tw1[q] = tab[kTabTw1 + 64 * q + lane];
    tw2[q] = tab[kTabTw2 + 64 * q + lane];
  }
  const int zoom = ZOOMED ? a.zoom : 0;
  float st[16], fh[3];  // zoom filter memories of my chain
  int ptr = 0;
  if constexpr (ZOOMED) zoom_load(st, fh, ptr, z.ring, ds, lane);
  float old[8];  // FFT_spec_old
  int pold[8];   // pixelold
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int x = (lane + 64 * r + 256) & 511;  // display column of bin lane + 64 r
    old[r] = ds[kDispOld + x];
    pold[r] = reinterpret_cast<const short *>(ds + kPanPixel)[x];
  }
  double win[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) win[r] = a.win[lane + 64 * r];
  for (int i = lane; i < 128; i += 64) grad[i] = i < kPanGradient ? a.gradient[i] : (unsigned short)0;
  __syncthreads();
  const int nf = a.noise_floor[ch];                            // currentNF: constant for every row of a call
  int oldnf = dsi[kPanNewSpectrum] != 0 ? dsi[kPanOldNf] : nf;  // newSpectrumFlag == 0: oldNF = currentNF
  const float gain_correction = a.gain_correction[ch];
  for (int k = 0; k < a.nrows; ++k) {
    const size_t row = (size_t)ch * (size_t)a.max_rows + (size_t)k;
    const float *pI = a.pre + row * (2 * L), *pQ = pI + L;
    cf v[8];
    if constexpr (!ZOOMED) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {  // float * double -> double -> float, FFT.cpp:222-223
        const int i = lane + 64 * r;
        v[r] = cf{(float)((double)pI[i] * win[r]), (float)((double)pQ[i] * win[r])};
      }
    } else {
      __syncthreads();
      for (int n = lane; n < L; n += 64) {  // FreqShift1 (Freq_Shift.cpp:42-65): x j^n
        const float xi = pI[n], xq = pQ[n];
        const int m = n & 3;
        z.stage[0][n] = (m == 0) ? xi : (m == 1) ? -xq : (m == 2) ? -xi : xq;
        z.stage[1][n] = (m == 0) ? xq : (m == 1) ? xi : (m == 2) ? -xq : -xi;
      }
      __syncthreads();
      zoom_frame(st, fh, ptr, z.stage, z.dec, z.ring, a.iir, a.fir, win, zoom, lane, v);
    }
    fft512<false>(v, tw1, tw2, xbuf, lane);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int x = (lane + 64 * r + 256) & 511;  // bins 0..255 -> upper half, 256..511 -> lower half
      const float m = v[r].x * v[r].x + v[r].y * v[r].y;
      // the pixel: from the un-smoothed FFT_spec at zoom 0 (FFT.cpp:245), from the smoothed one at zoom 1..4 (:157)
      const float spec = zoom_lowpass(zoom, m, old[r]);
      const int p = display_pixel(a.base, a.dBScale, spec);
      const int yn = pan_clamp(a.noise_floor_y - p - nf, kSpectrumTopY, kSpectrumBottom);
      const int yo = pan_clamp(a.noise_floor_y - pold[r] - oldnf, kSpectrumTopY, kSpectrumBottom);
      const unsigned short wf = x < R - 1 ? grad[pan_clamp(230 - yn, 0, kPanGradient - 1)] : (unsigned short)0;
      pold[r] = p;
      if (a.spec) a.spec[row * R + x] = spec;
      // 2-byte stores from the registers, 128 contiguous bytes per instruction.  (Staged through LDS so that a row leaves
      // as 64 16-byte stores it was slower: 5903 against 5850 us per 4096 x 128 launch at period 1, DESIGN.md "Panadapter")
      if (a.pixel) a.pixel[row * R + x] = (int16_t)p;
      if (a.y_new) a.y_new[row * R + x] = (int16_t)yn;
      if (a.y_old) a.y_old[row * R + x] = (int16_t)yo;
      if (a.waterfall) a.waterfall[row * R + x] = wf;
    }
    oldnf = nf;
    if (lane == 0 && a.smeter) {
      const float *mx = a.mx + row * 3;
      float *sm = a.smeter + row * 4;
      sm[0] = mx[0];
      sm[1] = mx[1];
      sm[2] = mx[2];
      sm[3] = pan_dbm(gain_correction, a.attenuator, mx[2], a.RFgain, a.rfGainAllBands);
    }
  }
  // the memory back
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int x = (lane + 64 * r + 256) & 511;
    ds[kDispOld + x] = old[r];
    reinterpret_cast<short *>(ds + kPanPixel)[x] = (short)pold[r];
  }
  if (lane == 0 && a.nrows > 0) {
    dsi[kPanOldNf] = oldnf;
    dsi[kPanNewSpectrum] = 1;
  }
  if constexpr (ZOOMED) {
    __syncthreads();
    zoom_store(ds, st, fh, ptr, z.ring, lane);
  }
}

hipError_t launch_panadapter(const PanArgs &a, hipStream_t s) {
  const dim3 grid(a.nchan), block(64);
  if (a.zoom > 0) hipLaunchKernelGGL(panadapter_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(panadapter_kernel<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
