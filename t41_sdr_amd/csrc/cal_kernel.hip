// t41_sdr_amd/csrc/cal_kernel.hip -- the receive half of the IQ calibration, ProcessIQData2() (Process2.cpp:352-397), with
// the sideband measurement of PlotCalSpectrum() (:478-547) behind it.  A translation unit of its own (cal_kernel.o; a kernel
// that joins display_kernel's translation unit moves that kernel's LDS and with it its code); host side: rx_cal.cpp.  It
// uses the display side output's FFT, twiddle, window and zoom tables, and zoom_fft.hpp's zoom memories and low-pass.  The
// chain itself (IIR, decimating FIR, ring, windowed read) is this kernel's own copy of zoom_fft.hpp's zoom_frame(), statement
// for statement: through the helper the compiler lays the frame loop out otherwise and a sweep at zoom 0 takes 2 % longer
// ("Shared exciter interpolators and zoom chain").  A change to one of the two goes into the other.
//
// One 64-lane wave = one channel = one (amplitude, phase) candidate, all the frames of a call.  Per frame, in the firmware's
// order and with contraction off:
//   updateDisplayFlag                                 Process2.cpp:485-488   one byte per frame, wave-uniform: a frame
//                                                     without it reads no samples and advances no memory (:387-395, FFT.cpp:209)
//   q15 -> float (the queues swapped) or f32          :359-360
//   x 10^(rfGainAllBands/20), x recBandFactor         :365-373
//   RX IQ correction, USB / LSB: I x -IQAmp, IQPhaseCorrection()   :376-384   no DC high-pass
//   FreqShift1()                                      :385
//   CalcZoom1Magn() on the first 512 shifted samples  :387-389, FFT.cpp:208-251      (spectrumZoom 0)
//   ZoomFFTExe() on the 2048 shifted samples          :391-395, FFT.cpp:67-157       (spectrumZoom 1..4)
//   pixelnew[] = baseOffset + pixel_offset + (int16_t)(dBScale * log10f_fast(FFT_spec[]))   FFT.cpp:157, 245
// and in every frame, from the channel's current pixelnew[]: arm_max_q15 over the two windows and adjdB (:498-505, 524).
#include "rx_experiments.hpp"
#include "rx_kernels.hpp"
#include "rx_launch.hpp"
#include "display_pixel.hpp"
#include "wave_fft.hpp"
#include "zoom_fft.hpp"

namespace t41 {

namespace {

// one sample up to and including FreqShift1(): n & 3 selects the quarter turn (Freq_Shift.cpp:42-65)
__device__ __forceinline__ cf cal_sample(const CalArgs &a, size_t idx, int n, float neg_amp, float phase) {
#pragma clang fp contract(off)
  float I, Q;
  if (a.q15) {  // arm_q15_to_float: (float)x / 32768
    I = (float)reinterpret_cast<const int16_t *>(a.I)[idx] / 32768.0f;
    Q = (float)reinterpret_cast<const int16_t *>(a.Q)[idx] / 32768.0f;
  } else {
    I = reinterpret_cast<const float *>(a.I)[idx];
    Q = reinterpret_cast<const float *>(a.Q)[idx];
  }
  I = I * a.g_rf;
  Q = Q * a.g_rf;
  I = I * a.rec_band;
  Q = Q * a.rec_band;
  if (a.corr_on) {
    I = I * neg_amp;
    if (phase < 0.0f) Q = Q + I * phase;
    else I = I + Q * phase;
  }
  const int m = n & 3;
  return cf{(m == 0) ? I : (m == 1) ? -Q : (m == 2) ? -I : Q, (m == 0) ? Q : (m == 1) ? I : (m == 2) ? -Q : -I};
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const int o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(64) void cal_kernel(const CalArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float xbuf[8 * kFftRow * 2];  // FFT exchange
  __shared__ float stage[2][2048];                                     // zoom: I / Q after the Fs/4 shift
  __shared__ float ring[2][512];
  __shared__ float dec[2][512];                                        // zoom: decimated samples of this frame
  __shared__ short pix[512];                                           // pixelnew[]
  const int lane = threadIdx.x;
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  constexpr int L = 2048, R = 512;
  float *ds = a.cal + (size_t)ch * kCalFloats;
  const cf *tab = reinterpret_cast<const cf *>(a.tab);
  cf tw1[7], tw2[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    tw1[q] = tab[kTabTw1 + 64 * q + lane];
    tw2[q] = tab[kTabTw2 + 64 * q + lane];
  }
  const int zoom = a.zoom;
  // the channel's candidate, or the params' factors
  const float neg_amp = -(a.corr ? a.corr[2 * (size_t)ch] : a.iq_amp);
  const float phase = a.corr ? a.corr[2 * (size_t)ch + 1] : a.iq_phase;
  // the calibration memory: zoom filter memories of my chain, the ring, the low-pass memory, the pixels
  float st[16], fh[3];
  int ptr = 0;
  if (zoom > 0) {
    zoom_load(st, fh, ptr, ring, ds, lane);
    ptr &= 511;
  }
  float old[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) old[r] = ds[kDispOld + ((lane + 64 * r + 256) & 511)];  // index of bin lane + 64 r
  for (int i = lane; i < R; i += 64) pix[i] = reinterpret_cast<const short *>(ds + kCalPixel)[i];
  double win[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) win[r] = a.win[lane + 64 * r];
  const size_t in0 = (size_t)ch * (size_t)a.chan_stride;
  for (int f = 0; f < a.nframes; ++f) {
    const bool upd = a.update ? a.update[f] != 0 : true;  // the same for every lane and every channel
    if (upd) {
      const size_t fr = in0 + (size_t)f * L;
      cf v[8];
      if (zoom == 0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {  // float * double -> double -> float, FFT.cpp:221-222
          const int i = lane + 64 * r;
          const cf x = cal_sample(a, fr + i, i, neg_amp, phase);
          v[r] = cf{(float)((double)x.x * win[r]), (float)((double)x.y * win[r])};
        }
      } else {
        __syncthreads();
        for (int n = lane; n < L; n += 64) {
          const cf x = cal_sample(a, fr + n, n, neg_amp, phase);
          stage[0][n] = x.x;
          stage[1][n] = x.y;
        }
        __syncthreads();
        // ---- zoom_fft.hpp's zoom_frame(), restated
        const int M = 1 << zoom;
        const int sample_no = (L / M > R) ? R : L / M;
        float h0 = fh[0], h1 = fh[1], h2 = fh[2];
        for (int n = 0; n < L; ++n) {
          float x = stage[lane & 1][n];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {  // arm_biquad_cascade_df1_f32: acc = b0 x + b1 x1 + b2 x2 + a1 y1 + a2 y2
            const float *c = a.iir + 5 * s4;
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
            float acc = a.fir[0] * h0;
            acc += a.fir[1] * h1;
            acc += a.fir[2] * h2;
            acc += a.fir[3] * x;
            if (k < sample_no && lane < 2) dec[lane & 1][k] = acc;
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
        const float multiplier = (zoom > 3) ? (float)(1 << zoom) : (float)zoom;  // FFT.cpp:105-108
#pragma unroll
        for (int r = 0; r < 8; ++r) {  // float * float -> float, * double -> double -> float, FFT.cpp:110-111
          const int idx = lane + 64 * r;
          const float mx = multiplier * ring[0][(ptr + idx) & 511], my = multiplier * ring[1][(ptr + idx) & 511];
          v[r] = cf{(float)((double)mx * win[r]), (float)((double)my * win[r])};
        }
      }
      fft512<false>(v, tw1, tw2, xbuf, lane);
      const size_t row = ((size_t)ch * a.nframes + f) * R;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int x = (lane + 64 * r + 256) & 511;  // bins 0..255 -> upper half, 256..511 -> lower half
        const float m = v[r].x * v[r].x + v[r].y * v[r].y;
        // the pixel: from the un-smoothed FFT_spec at zoom 0 (FFT.cpp:245), from the smoothed one at zoom 1..4 (:157)
        const float spec = zoom_lowpass(zoom, m, old[r]);
        const short p = display_pixel(a.base, a.dBScale, spec);  // (display_pixel.hpp, shared with the panadapter stage)
        pix[x] = p;
        if (a.spec) a.spec[row + x] = spec;
        if (a.pixel) a.pixel[row + x] = p;
      }
    }
    __syncthreads();
    // PlotCalSpectrum(): arm_max_q15 over [bin - capture, bin + capture) of both windows, from the current pixelnew[]
    int m0 = -32768, m1 = -32768;
    for (int i = lane; i < a.width; i += 64) {
      const int p0 = pix[a.lo0 + i], p1 = pix[a.lo1 + i];
      m0 = p0 > m0 ? p0 : m0;
      m1 = p1 > m1 ? p1 : m1;
    }
    m0 = wave_max(m0);
    m1 = wave_max(m1);
    if (lane == 0) {
      int ref = 0, adj = 0;  // LSB: window 0 is the wanted sideband; USB: window 1; any other mode: both stay 0
      if (a.sideband == 1) {
        ref = m0;
        adj = m1;
      } else if (a.sideband == 2) {
        ref = m1;
        adj = m0;
      }
      float *res = a.result + ((size_t)ch * a.nframes + f) * 3;
      res[0] = (float)ref;
      res[1] = (float)adj;
      res[2] = (float)((double)((float)adj - (float)ref) / 1.95);  // Process2.cpp:524: the literal is a double
    }
    __syncthreads();
  }
  // the calibration memory back
#pragma unroll
  for (int r = 0; r < 8; ++r) ds[kDispOld + ((lane + 64 * r + 256) & 511)] = old[r];
  for (int i = lane; i < R; i += 64) reinterpret_cast<short *>(ds + kCalPixel)[i] = pix[i];
  if (zoom > 0) zoom_store(ds, st, fh, ptr, ring, lane);
}

hipError_t launch_cal(const CalArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(cal_kernel, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

T41RX_BUILD_FLAGS(cal_kernel)

}  // namespace t41
