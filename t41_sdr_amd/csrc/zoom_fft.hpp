// t41_sdr_amd/csrc/zoom_fft.hpp -- ZoomFFTExe() (spectrumZoom 1..4, FFT.cpp:67-152) and CalcZoom1Magn() (spectrumZoom 0,
// FFT.cpp:208-251) between the Fs/4 shift and the spectrum: the zoom memories, the 4-stage IIR and the decimating FIR, the
// ring, the windowed read and the FFT_spec / FFT_spec_old low-pass.  Device code of display_kernel.hip and cal_kernel.hip
// (which keeps a copy of zoom_frame() for its speed), one 64-lane wave per channel; where the samples come from, the FFT, the pixels and the output rows are the kernels'.
//
// The IIR and the FIR are serial in the sample index: every lane runs the I (even lanes) or the Q (odd lanes) chain
// redundantly, sample by sample, with the reference's order of operations; everything else is wave-parallel.  The
// contraction pragma is lexical: every function here that does arithmetic carries it as its body's first line.
#pragma once
#include "rx_internal.hpp"
#include "wave_fft.hpp"

namespace t41 {

// The zoom memories of a lane's chain (lane & 1) travel as three pieces: st[16], IIR_biquad_Zoom_FFT_{I,Q}_state (x1, x2,
// y1, y2 per stage); fh[3], the decimating FIR's last 3 inputs; ptr, zoom_sample_ptr.  (As one struct they cost cal_kernel
// 5 % at zoom 0: the frame loop's register copies come out single where they were paired.)

// a channel's record ds[kDispIir / kDispFir / kDispPtr / kDispRing] -> registers and the ring in LDS, and back
__device__ __forceinline__ void zoom_load(float (&st)[16], float (&fh)[3], int &ptr, float (*ring)[512], const float *ds, int lane) {
  const int chain = lane & 1;
#pragma unroll
  for (int i = 0; i < 16; ++i) st[i] = ds[kDispIir + 16 * chain + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) fh[i] = ds[kDispFir + 4 * chain + i];
  ptr = reinterpret_cast<const int *>(ds)[kDispPtr];
  for (int i = lane; i < 2 * 512; i += 64) (&ring[0][0])[i] = ds[kDispRing + i];
}
__device__ __forceinline__ void zoom_store(float *ds, const float (&st)[16], const float (&fh)[3], int ptr, float (*ring)[512], int lane) {
  const int chain = lane & 1;
  if (lane < 2) {
#pragma unroll
    for (int i = 0; i < 16; ++i) ds[kDispIir + 16 * chain + i] = st[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) ds[kDispFir + 4 * chain + i] = fh[i];
  }
  if (lane == 0) reinterpret_cast<int *>(ds)[kDispPtr] = ptr;
  for (int i = lane; i < 2 * 512; i += 64) ds[kDispRing + i] = (&ring[0][0])[i];
}

// One frame of ZoomFFTExe() up to the FFT's input: stage[chain][0..2047], the samples after the Fs/4 shift (the caller has
// synchronised behind writing them), through the IIR and the FIR into dec, dec into the ring, and the ring's 512 samples,
// oldest first, times the zoom multiplier and the window into v[r], sample lane + 64 r.  (cal_kernel.hip restates this
// function's body: see there.)
__device__ __forceinline__ void zoom_frame(float (&st)[16], float (&fh)[3], int &ptr, float (*stage)[2048], float (*dec)[512], float (*ring)[512],
                                           const float *iir, const float *fir, const double (&win)[8], int zoom, int lane, cf (&v)[8]) {
#pragma clang fp contract(off)
  constexpr int L = 2048, R = 512;
  const int chain = lane & 1;
  const int M = 1 << zoom;
  const int sample_no = (L / M > R) ? R : L / M;
  float h0 = fh[0], h1 = fh[1], h2 = fh[2];
  for (int n = 0; n < L; ++n) {
    float x = stage[chain][n];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {  // arm_biquad_cascade_df1_f32: acc = b0 x + b1 x1 + b2 x2 + a1 y1 + a2 y2
      const float *c = iir + 5 * s4;
      float acc = c[0] * x;
      acc += c[1] * st[4 * s4 + 0];
      acc += c[2] * st[4 * s4 + 1];
      acc += c[3] * st[4 * s4 + 2];
      acc += c[4] * st[4 * s4 + 3];
      st[4 * s4 + 1] = st[4 * s4 + 0];
      st[4 * s4 + 0] = x;
      st[4 * s4 + 3] = st[4 * s4 + 2];
      st[4 * s4 + 2] = acc;
      x = acc;
    }
    if ((n & (M - 1)) == 0) {  // arm_fir_decimate_f32, 4 taps: y[k] = sum_i c[i] state[k M + i], newest sample = x
      const int k = n >> zoom;
      float acc = fir[0] * h0;
      acc += fir[1] * h1;
      acc += fir[2] * h2;
      acc += fir[3] * x;
      if (k < sample_no && lane < 2) dec[chain][k] = acc;
    }
    h0 = h1;
    h1 = h2;
    h2 = x;
  }
  fh[0] = h0;
  fh[1] = h1;
  fh[2] = h2;
  __syncthreads();
  for (int k = lane; k < sample_no; k += 64) {  // FFT.cpp:98-104
    ring[0][(ptr + k) & 511] = dec[0][k];
    ring[1][(ptr + k) & 511] = dec[1][k];
  }
  ptr = (ptr + sample_no) & 511;
  __syncthreads();
  const float multiplier = (zoom > 3) ? (float)(1 << zoom) : (float)zoom;  // FFT.cpp:106-109
#pragma unroll
  for (int r = 0; r < 8; ++r) {  // float * float -> float, * double -> double -> float, FFT.cpp:110-111
    const int idx = lane + 64 * r;
    const float mx = multiplier * ring[0][(ptr + idx) & 511], my = multiplier * ring[1][(ptr + idx) & 511];
    v[r] = cf{(float)((double)mx * win[r]), (float)((double)my * win[r])};
  }
  // (zoom_sample_ptr ends where it started after the 512 reads)
}

// FFT_spec of a bin from its squared magnitude m, and the bin's FFT_spec_old updated in place.  spectrumZoom 0
// (FFT.cpp:241-243): the low-pass runs in float + double into FFT_spec_old only, FFT_spec stays un-smoothed; spectrumZoom
// 1..4 (FFT.cpp:136-137): all float, and FFT_spec is the smoothed value.
__device__ __forceinline__ float zoom_lowpass(int zoom, float m, float &old) {
#pragma clang fp contract(off)
  const float LPFcoeff = 0.7f;
  if (zoom == 0) {
    old = (float)((double)(LPFcoeff * m) + (1.0 - (double)LPFcoeff) * (double)old);
    return m;
  }
  const float onem = (float)(1.0 - (double)LPFcoeff);
  old = LPFcoeff * m + onem * old;
  return old;
}

}  // namespace t41
