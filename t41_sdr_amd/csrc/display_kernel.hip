// t41_sdr_amd/csrc/display_kernel.hip -- the display FFT side output (t41rx_set_display_spectrum).
#include "rx_device.hpp"
#include "rx_launch.hpp"
#include "zoom_fft.hpp"

namespace t41 {

// ------------------------------------------------------------------------------------------
// Display FFT side output: CalcZoom1Magn() (spectrumZoom 0, FFT.cpp:208-251) and ZoomFFTExe()
// (spectrumZoom 1..4, FFT.cpp:67-152) up to FFT_spec / FFT_spec_old; the pixel mapping behind them
// is display code.  One wave per channel on the dbg_pre tap of the frames just processed (the
// firmware runs it once per display refresh, not per frame: nothing here is tuned).  The zoom chain
// between the Fs/4 shift and the FFT, and the low-pass behind it, are zoom_fft.hpp's, shared with
// cal_kernel.hip.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void display_kernel(const DispArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float xbuf[8 * kFftRow * 2];  // FFT exchange
  __shared__ float stage[2][2048];                                     // zoom: I / Q after the Fs/4 shift
  __shared__ float ring[2][512];
  __shared__ float dec[2][512];                                        // zoom: decimated samples of this frame
  const int lane = threadIdx.x;
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  constexpr int L = 2048, R = 512;
  float *ds = a.disp + (size_t)ch * kDispFloats;
  const cf *tab = reinterpret_cast<const cf *>(a.tab);
  cf tw1[7], tw2[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    tw1[q] = tab[kTabTw1 + 64 * q + lane];
    tw2[q] = tab[kTabTw2 + 64 * q + lane];
  }
  const int zoom = a.zoom;
  float st[16], fh[3];  // zoom filter memories of my chain
  int ptr = 0;
  if (zoom > 0) zoom_load(st, fh, ptr, ring, ds, lane);
  float old[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) old[r] = ds[kDispOld + ((lane + 64 * r + 256) & 511)];  // index of bin lane + 64 r
  double win[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) win[r] = a.win[lane + 64 * r];
  for (int f = 0; f < a.nframes; ++f) {
    const float *pI = a.pre + ((size_t)ch * a.nframes + f) * (2 * L), *pQ = pI + L;
    cf v[8];
    if (zoom == 0) {
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
        stage[0][n] = (m == 0) ? xi : (m == 1) ? -xq : (m == 2) ? -xi : xq;
        stage[1][n] = (m == 0) ? xq : (m == 1) ? xi : (m == 2) ? -xq : -xi;
      }
      __syncthreads();
      zoom_frame(st, fh, ptr, stage, dec, ring, a.iir, a.fir, win, zoom, lane, v);
    }
    fft512<false>(v, tw1, tw2, xbuf, lane);
    float *so = a.spec + ((size_t)ch * a.nframes + f) * R, *oo = a.spec_old + ((size_t)ch * a.nframes + f) * R;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int x = (lane + 64 * r + 256) & 511;  // bins 0..255 -> upper half, 256..511 -> lower half
      const float m = v[r].x * v[r].x + v[r].y * v[r].y;
      const float spec = zoom_lowpass(zoom, m, old[r]);
      so[x] = spec;
      oo[x] = old[r];
    }
  }
  // state back
#pragma unroll
  for (int r = 0; r < 8; ++r) ds[kDispOld + ((lane + 64 * r + 256) & 511)] = old[r];
  if (zoom > 0) {
    __syncthreads();
    zoom_store(ds, st, fh, ptr, ring, lane);
  }
}

hipError_t launch_display(const DispArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(display_kernel, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

T41RX_BUILD_FLAGS(display_kernel)

}  // namespace t41
