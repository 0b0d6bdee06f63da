// t41_sdr_amd/csrc/cw_kernel.hip -- gfx950 kernels of the CW receive block (Process.cpp:878-913; FFT_LENGTH 512): the
// tone detector of DoCWReceiveProcessing() (CWProcessing.cpp:322-373, goertzel_mag :830-857) and the narrow audio filter
// selected by CWFilterIndex (five six-section arm_biquad_cascade_df2T_f32 instances, CWProcessing.cpp:36-48).
//
// Both run on the call's audio @24 kS/s in the stage scratch ([channel][frame * 256]) behind the noise blanker and in
// front of the back kernel's interpolators (launch_back512): first the detector, which only reads the audio, then the
// filter, in place.  Built into rx_host.o (included by rx_host.cpp, a HIP translation unit compiled without
// contraction; the kernels also turn contraction off by pragma), so the library's object set is unchanged.
//
// Every value is formed by the reference's operations in the order of the f32 restatement (tests/cw_model.py), one
// rounding per multiply and per add, so both stages are that restatement bit for bit.
//
// NARROW FILTER: a six-stage serial cascade on df2t_pipe.hpp's pipeline (the step, the hand-over, the ring), one section
// per lane, 8 lanes per channel (6 used, stage s reads stage s - 1 by a DPP row shift) and 8 CHANNELS PER WAVE.  The
// 6-deep pipeline runs through all frames of the call, so its fill and drain (5 steps each) are paid once per launch.
// Input arrives in 64-sample chunks per channel (coalesced loads, prefetched a chunk ahead) through an 8 x 64 LDS buffer;
// stage-5 lanes store into an 8-row ring, from which complete chunks go back coalesced.
//
// DETECTOR: one wave per channel, frame after frame (corrResultR of the block before enters aveCorrResult, so frames are
// not independent).  The block, its 63-sample history, the filtered block, the sine table and the taps sit in LDS.  The
// 64-tap FIR runs in parallel over samples (4 per lane, each sum in tap order).  The 511 lags of arm_correlate_f32 are
// paired -- lag u with lag 256 + u, u = 0 .. 254, and lag 255 alone -- so that every pair is exactly 256 multiply-adds:
// walking sample i = 0 .. 255 of the filtered block (one broadcast read), the pair's products go to lag u's sum while
// i <= u and to lag 256 + u's after it, both in increasing sample index; 4 pairs per lane, consecutive lanes read
// consecutive table words.  The Goertzel recurrence restarts every block and rides the same walk on the same broadcast
// sample, its dependent chain hidden behind the 4 independent sums.  The maximum over the lags is order-free.
//
// INTERPOLATORS BEHIND THE NARROW FILTER (cw_back_kernel): Process.cpp:917-937 operation for operation, where the fused
// back kernel folds the volume into the x4 taps and contracts; see cw_kernels.hpp.
#include <hip/hip_runtime.h>

#include "cw_kernels.hpp"
#include "df2t_pipe.hpp"
#include "rx_internal.hpp"  // kStInt1, kStInt2: the interpolator histories in the per-channel records

namespace t41 {

namespace cw {
constexpr int kInPitch = df2t::kChunk + 4;  // (4 banks apart per channel row: the 8 broadcast b128 reads do not conflict)
constexpr int kRowShr1 = 0x111;             // DPP row_shr:1: lane l reads lane l - 1 (stage s reads stage s - 1)
}  // namespace cw

__global__ __launch_bounds__(64) void cw_filter_kernel(CwFilterArgs a) {
#pragma clang fp contract(off)
  using namespace cw;
  using namespace df2t;
  __shared__ __attribute__((aligned(16))) float xin[kCwChanPerWave * kInPitch];
  __shared__ __attribute__((aligned(16))) float ring[kCwChanPerWave * kRowPitch];
  const int lane = threadIdx.x;
  const int grp = lane >> 3, stage = lane & 7;
  const int ch0 = blockIdx.x * kCwChanPerWave;
  const int nlive = min(kCwChanPerWave, a.nchan - ch0);  // channels of this wave (the ragged last one has fewer)
  const bool live = stage < kCwStages && grp < nlive;
  float *x = a.aud + (size_t)ch0 * a.nsamp;
  float *st = a.state + (size_t)(ch0 + grp) * kCwStateFloats + kCwStFilter + 2 * kCwStages * a.index + 2 * stage;
  const int nchunk = a.nsamp / kChunk;

  Pipe<kCwStages, kRowShr1, false, true> p;
  p.head = stage == 0;
  p.tail = live && stage == kCwStages - 1;
  if (live) {
    const float *c = a.coef + 5 * stage;
    p.q = Section{c[0], c[1], c[2], c[3], c[4], st[0], st[1]};
  }
  const float *in_row = xin + grp * kInPitch;
  p.row = ring + grp * kRowPitch;

  // samples 64 k .. 64 k + 63 of every channel of the wave back to the scratch, coalesced
  auto store_chunk = [&](int k) {
    for (int kk = 0; kk < nlive; ++kk)
      x[(size_t)kk * a.nsamp + (size_t)k * kChunk + lane] = ring[kk * kRowPitch + (k & 1) * kChunk + lane];
  };

  float nxt[kCwChanPerWave];
#pragma unroll
  for (int kk = 0; kk < kCwChanPerWave; ++kk) nxt[kk] = kk < nlive ? x[(size_t)kk * a.nsamp + lane] : 0.0f;
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int kk = 0; kk < kCwChanPerWave; ++kk) xin[kk * kInPitch + lane] = nxt[kk];
    if (c + 1 < nchunk) {
#pragma unroll
      for (int kk = 0; kk < kCwChanPerWave; ++kk)
        if (kk < nlive) nxt[kk] = x[(size_t)kk * a.nsamp + (size_t)(c + 1) * kChunk + lane];
    }
    __syncthreads();
    if (c == 0) {  // the pipeline fills: stage s starts at step s
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(in_row + j);
        p.run(v.x, j, 0, j >= stage);
        p.run(v.y, j + 1, 0, j + 1 >= stage);
        p.run(v.z, j + 2, 0, j + 2 >= stage);
        p.run(v.w, j + 3, 0, j + 3 >= stage);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(in_row + j);
        p.run(v.x, j, c, true);
        p.run(v.y, j + 1, c, true);
        p.run(v.z, j + 2, c, true);
        p.run(v.w, j + 3, c, true);
      }
    }
    __syncthreads();
    if (c > 0) store_chunk(c - 1);
  }
  // the pipeline drains: step 64 n + d runs stages d + 1 .. 5 on the last samples
#pragma unroll
  for (int d = 0; d < kCwStages - 1; ++d) p.run(0.0f, kChunk + d, nchunk - 1, stage > d);
  __syncthreads();
  store_chunk(nchunk - 1);
  if (live) {
    st[0] = p.q.d1;
    st[1] = p.q.d2;
  }
}

__global__ __launch_bounds__(64) void cw_detect_kernel(CwDetectArgs a) {
#pragma clang fp contract(off)
  constexpr int N = kCwBlock, T = kCwFirTaps;
  __shared__ float s[T - 1 + N + 1];  // arm_fir_f32's state: 63 samples of history, then the block
  __shared__ float A[N];              // float_buffer_CW: the filtered block
  __shared__ float B[N];              // sinBuffer
  __shared__ float C[T];              // CW_Filter_Coeffs2
  const int lane = threadIdx.x;
  float *st = a.state + (size_t)blockIdx.x * kCwStateFloats;
  const float *x = a.aud + (size_t)blockIdx.x * a.nframes * N;
  float *out = a.out + (size_t)blockIdx.x * a.nframes * 4;

  C[lane] = a.fir[lane];
#pragma unroll
  for (int m = 0; m < 4; ++m) B[lane + 64 * m] = a.sinb[lane + 64 * m];
  if (lane < T - 1) s[lane] = st[kCwStFir + lane];
  float corrR = st[kCwStCorrR], aveL = st[kCwStAveL], aveR = st[kCwStAveR];

  float nx[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) nx[m] = x[lane + 64 * m];
  for (int f = 0; f < a.nframes; ++f) {
#pragma unroll
    for (int m = 0; m < 4; ++m) s[T - 1 + lane + 64 * m] = nx[m];
    if (f + 1 < a.nframes) {
#pragma unroll
      for (int m = 0; m < 4; ++m) nx[m] = x[(size_t)(f + 1) * N + lane + 64 * m];
    }
    __syncthreads();
    // arm_fir_f32: y[n] = sum_i coeffs[i] * state[n + i], one accumulator in tap order
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < T; ++i) {
      const float c = C[i];
#pragma unroll
      for (int m = 0; m < 4; ++m) y[m] = y[m] + c * s[lane + 64 * m + i];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) A[lane + 64 * m] = y[m];
    const float hist = lane < T - 1 ? s[N + lane] : 0.0f;  // the block's last 63 samples: the next block's history
    __syncthreads();
    if (lane < T - 1) s[lane] = hist;

    // arm_correlate_f32 over the lag pairs, and goertzel_mag's recurrence on the same walk
    float lo[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float q1 = 0.0f, q2 = 0.0f;
#pragma unroll 4
    for (int i = 0; i < N; ++i) {
      const float v = A[i];
      float q0 = a.coeff * q1;
      q0 = q0 - q2;
      q0 = q0 + v;
      q2 = q1;
      q1 = q0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int u = lane + 64 * m;
        const float p = v * B[(i - u - 1) & (N - 1)];
        const float l1 = lo[m] + p, h1 = hi[m] + p;
        lo[m] = i <= u ? l1 : lo[m];
        hi[m] = i <= u ? hi[m] : h1;
      }
    }
    // arm_max_f32 over the 511 lags (pair 255 has no second lag)
    float mx = lo[0];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      mx = lo[m] > mx ? lo[m] : mx;
      if (lane + 64 * m < N - 1) mx = hi[m] > mx ? hi[m] : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float o = __shfl_xor(mx, off);
      mx = o > mx ? o : mx;
    }
    // CWProcessing.cpp:336-357 with float_buffer_R = float_buffer_L: one computation serves both sides
    const float corrL = mx;
    aveL = (float)(.7 * (double)corrL + .3 * (double)aveL);
    const float ave = (corrR + corrL) / 2.0f;  // corrResultR is still the block before's (:339 runs before :348)
    const float re = (q1 - q2 * a.cosine) / 128.0f;
    const float im = (q2 * a.sine) / 128.0f;
    const float g1 = sqrtf(re * re + im * im);
    corrR = corrL;
    aveR = (float)(.7 * (double)corrR + .3 * (double)aveR);
    const float g = (g1 + g1) / 2.0f;
    const float comb = 10.0f * ave * 100.0f * g;
    if (lane < 4) out[(size_t)f * 4 + lane] = lane == 0 ? corrL : lane == 1 ? g : lane == 2 ? ave : comb;
  }
  __syncthreads();
  if (lane < T - 1) st[kCwStFir + lane] = s[lane];
  if (lane == 0) {
    st[kCwStCorrR] = corrR;
    st[kCwStAveL] = aveL;
    st[kCwStAveR] = aveR;
  }
}

// One wave per channel, frame after frame: the x2 interpolator's 23-sample and the x4 interpolator's 7-sample histories
// come from the channel's record (where the fused kernels keep them too) and return there behind the call's last frame.
// Lane l forms outputs l, l + 64, ..: every store instruction writes consecutive addresses.
__global__ __launch_bounds__(64) void cw_back_kernel(CwBackArgs a) {
#pragma clang fp contract(off)
  constexpr int N = kCwBlock, P1 = 24, P2 = 8;
  __shared__ float s1[P1 - 1 + N + 1];      // arm_fir_interpolate_f32's state of the x2 stage: history, then the block
  __shared__ float s2[P2 - 1 + 2 * N + 1];  // ... of the x4 stage
  __shared__ float c1[48], c2[32];
  const int lane = threadIdx.x;
  float *st = a.state + (size_t)blockIdx.x * a.state_stride;
  const float *x = a.aud + (size_t)blockIdx.x * a.nframes * N;
  if (lane < 48) c1[lane] = a.int1[lane];
  if (lane < 32) c2[lane] = a.int2[lane];
  if (lane < P1 - 1) s1[lane] = st[kStInt1 + 1 + lane];
  if (lane < P2 - 1) s2[lane] = st[kStInt2 + 1 + lane];
  for (int f = 0; f < a.nframes; ++f) {
#pragma unroll
    for (int m = 0; m < 4; ++m) s1[P1 - 1 + lane + 64 * m] = x[(size_t)f * N + lane + 64 * m];
    __syncthreads();
    // x2: output 2 n + (j - 1) = sum_t state[n + t] * coeffs[(2 - j) + 2 t]
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int o = lane + 64 * k, n = o >> 1, c0 = 1 - (o & 1);
      float acc = 0.0f;
      for (int t = 0; t < P1; ++t) acc += s1[n + t] * c1[c0 + 2 * t];
      s2[P2 - 1 + o] = acc;
    }
    const float h1 = lane < P1 - 1 ? s1[N + lane] : 0.0f;
    __syncthreads();
    if (lane < P1 - 1) s1[lane] = h1;
    // x4: output 4 n + (j - 1) = sum_t state[n + t] * coeffs[(4 - j) + 4 t]; then the volume
    const size_t base = (size_t)blockIdx.x * a.chan_stride + (size_t)f * a.frame_stride;
    for (int k = 0; k < 32; ++k) {
      const int o = lane + 64 * k, n = o >> 2, c0 = 3 - (o & 3);
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < P2; ++t) acc += s2[n + t] * c2[c0 + 4 * t];
      const float y = acc * a.scale;
      if (!a.q15) {
        static_cast<float *>(a.out)[base + o] = y;
      } else {  // arm_float_to_q15: (q15_t)__SSAT((q31_t)(x * 32768.0f), 16), toward zero
        int q = (int)(y * 32768.0f);
        q = q < -32768 ? -32768 : (q > 32767 ? 32767 : q);
        static_cast<short *>(a.out)[base + o] = (short)q;
      }
    }
    const float h2 = lane < P2 - 1 ? s2[2 * N + lane] : 0.0f;
    __syncthreads();
    if (lane < P2 - 1) s2[lane] = h2;
  }
  __syncthreads();
  if (lane < P1 - 1) st[kStInt1 + 1 + lane] = s1[lane];
  if (lane < P2 - 1) st[kStInt2 + 1 + lane] = s2[lane];
}

hipError_t launch_cw_filter(const CwFilterArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nsamp <= 0 || a.nsamp % df2t::kChunk || a.index < 0 || a.index >= kCwFilters) return hipErrorInvalidConfiguration;
  const unsigned waves = (unsigned)((a.nchan + kCwChanPerWave - 1) / kCwChanPerWave);
  hipLaunchKernelGGL(cw_filter_kernel, dim3(waves), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_back(const CwBackArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || !a.aud || !a.state || !a.out) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(cw_back_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_detect(const CwDetectArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(cw_detect_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
