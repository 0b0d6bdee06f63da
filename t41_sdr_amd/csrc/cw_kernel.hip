// t41_sdr_amd/csrc/cw_kernel.hip -- gfx950 kernels of the CW receive block (Process.cpp:878-913; FFT_LENGTH 512): the
// tone detector of DoCWReceiveProcessing() (CWProcessing.cpp:322-373, goertzel_mag :830-857) and the narrow audio filter
// selected by CWFilterIndex (five six-section arm_biquad_cascade_df2T_f32 instances, CWProcessing.cpp:36-48).
//
// Both run on the call's audio @24 kS/s in the stage scratch ([channel][frame * 256]) behind the noise blanker and in
// front of the back kernel's interpolators (launch_back512): first the detector, which only reads the audio, then the
// filter, in place.  A translation unit of its own (cw_kernel.o), compiled without contraction like the host designer
// (the kernels also turn contraction off by pragma); rx_cw.cpp is its host side and sees it through cw_kernels.hpp.
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
// DECODER (cw_decode_kernel): the rest of DoCWReceiveProcessing() behind the detector -- `combinedCoeff > 50` and
// DoCWDecoding() with its two adaptive histograms (CWProcessing.cpp:365-371, :501-815) -- on integer and double
// arithmetic, word for word tests/cw_decode_model.py, where the choices the firmware leaves open (the clock, the arrays'
// extent, power-on, the tree past its literal) are written down.  One lane per channel; see the kernel.
//
// INTERPOLATORS BEHIND THE NARROW FILTER (cw_back_kernel): Process.cpp:917-937 operation for operation, where the fused
// back kernel folds the volume into the x4 taps and contracts; see cw_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstring>

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
// cw_back_omap_kernel below is this kernel's text again with the output map's row: a change here goes there too
// (tests/test_output_map.py holds the twin's rows to this kernel's, bit for bit).
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

// The same behind an output map (t41rx_set_output_map): the channel's audio goes to row a.out_map[channel]; a muted
// channel's block leaves before it reads the audio or the interpolator memories, which stay in the record as they were.
// A kernel of its own text: cw_back_kernel sharing a body with it compiles to another instruction stream.
__global__ __launch_bounds__(64) void cw_back_omap_kernel(CwBackArgs a) {
#pragma clang fp contract(off)
  constexpr int N = kCwBlock, P1 = 24, P2 = 8;
  const int row = a.out_map[blockIdx.x];
  if (row < 0) return;  // block-uniform, ahead of every barrier
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
    const size_t base = (size_t)row * a.chan_stride + (size_t)f * a.frame_stride;
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

// ---- the Morse decoder (cw_decode_kernel) -----------------------------------------------------------------------------
namespace cwd {
constexpr int kChunk = 32;                 // frames per staging pass: one key bit per frame in a 32-bit mask
constexpr int kOutPitch = 2 * kChunk + 1;  // (odd: lane c writes row c, no bank conflicts)
constexpr double kScaleConstant = 1.0 / (1.0 - 0.8);  // SCALE_CONSTANT: slightly above 5

// a histogram word of the LDS copy; a word past the carried allotment reads 0 (only a hand-made checkpoint gets there)
__device__ inline int rd(const int *h, int i, int cap) { return (unsigned)i < (unsigned)cap ? h[i] : 0; }
__device__ inline int sub32(int a, int b) { return (int)((unsigned)a - (unsigned)b); }

// JackClusteredArrayMax(&h[base], elements, ., ., ., spread) by all 64 lanes: lane l takes i = spread + l, + 64, ..; the
// window sums come from the LDS copy.  `>=` in increasing i keeps a lane's last maximum, and the reduction prefers the
// larger index among equal sums: the last index holding the maximum wins, as in the serial loop.
__device__ inline void clustered_max(const int *h, int cap, int base, int elements, int spread, int lane, int *maxCount, int *maxIndex) {
  int best = 0, idx = -1;
  for (int i = spread + lane; i < elements - spread; i += 64) {
    int t = 0;
    for (int j = -spread; j <= spread; ++j) t += rd(h, base + i + j, cap);
    if (t >= best) {
      best = t;
      idx = i;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int ob = __shfl_xor(best, off), oi = __shfl_xor(idx, off);
    if (ob > best || (ob == best && oi > idx)) {
      best = ob;
      idx = oi;
    }
  }
  *maxCount = idx > 0 ? rd(h, base + idx, cap) : 0;
  *maxIndex = idx > 0 ? idx : 0;
}
}  // namespace cwd

// One lane per channel, 64 channels per wave, frame after frame; the scalars live in registers from the first frame of
// the call to the last.  Per pass of 32 frames the wave reads the 32 combinedCoeff words of each of its channels with
// one load (consecutive frames in consecutive lanes), turns them into key bits by a ballot that the channel's lane
// keeps, runs the frames, and stores the staged {character, ditLength} words row by row.
// A histogram call (at most one per channel and 5000 ms of its clock) is served by the whole wave inside the frame
// loop, since its results feed the next frame: the lanes with an event are balloted and taken one at a time, the
// channel's parameters broadcast, its histogram copied to LDS, and all 64 lanes do the scaling pass, the clustered
// maxima and the top-of-range scan there.  What the lane itself can do -- the value references, the averages, the
// geometric mean -- it does before the wave serves it.
__global__ __launch_bounds__(64) void cw_decode_kernel(CwDecodeArgs a) {
#pragma clang fp contract(off)
  using namespace cwd;
  __shared__ int hl[kCwDecGapWords];
  __shared__ int outl[64 * kOutPitch];
  __shared__ unsigned char tree[kCwTreeChars + 3];
  const int lane = threadIdx.x;
  const int ch0 = blockIdx.x * 64;
  const int nlive = min(64, a.nchan - ch0);
  const bool live = lane < nlive;
  int32_t *w = a.state + (size_t)(ch0 + (live ? lane : 0)) * kCwDecWords;
  for (int i = lane; i < kCwTreeChars; i += 64) tree[i] = a.tree[i];

  int st = w[kCwDecState];
  unsigned n = (unsigned)w[kCwDecN];
  int oldTime = w[kCwDecOldTime], signalStart = w[kCwDecSignalStart], signalEnd = w[kCwDecSignalEnd];
  int elapsed = w[kCwDecElapsed], gapLength = w[kCwDecGapLength];
  unsigned ditLength = (unsigned)w[kCwDecDitLength];
  int dahLength = w[kCwDecDahLength], gapAtom = w[kCwDecGapAtom], gapChar = w[kCwDecGapChar];
  float tgm = __int_as_float(w[kCwDecTgm]);
  int aveDit = w[kCwDecAveDit], aveDah = w[kCwDecAveDah], valRef1 = w[kCwDecValRef1], valRef2 = w[kCwDecValRef2];
  int gapRef1 = w[kCwDecGapRef1], valFlag = w[kCwDecValFlag], signalStartOld = w[kCwDecSignalStartOld];
  int dashJump = w[kCwDecDashJump], index = w[kCwDecIndex];
  bool charFlag = w[kCwDecCharFlag] != 0, blankFlag = w[kCwDecBlankFlag] != 0;
  int topGap = w[kCwDecTopGap], topGapOld = w[kCwDecTopGapOld];
  int currentTime = w[kCwDecCurrentTime], interGap = w[kCwDecInterGap], noSignal = w[kCwDecNoSignal];
  __syncthreads();

  for (int f0 = 0; f0 < a.nframes; f0 += kChunk) {
    const int nf = min(kChunk, a.nframes - f0);
    unsigned keys = 0;  // bit k: combinedCoeff > 50 in frame f0 + k (CWProcessing.cpp:365)
    for (int k0 = 0; k0 < nlive; k0 += 8) {  // (8 channels' loads in flight)
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (k0 + j < nlive && lane < nf) ? a.cw[((size_t)(ch0 + k0 + j) * a.nframes + f0 + lane) * 4 + 3] : 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned m = (unsigned)__ballot(v[j] > 50.0f);
        if (lane == k0 + j) keys = m;
      }
    }
    for (int fr = 0; fr < nf; ++fr) {
      const bool key = (keys >> fr) & 1u;
      const int now = (int)((unsigned)a.t0 + (unsigned)(((unsigned long long)n * (unsigned)a.num) / (unsigned)a.den));
      if (n == 0) oldTime = a.t0;  // static long oldTime = millis();
      int ch = 0, ev = 0, evval = 0;  // ev: 1 = DoGapHistogram(evval), 2 = DoSignalHistogram(evval)
      if (st == 0) {
        if (key) {
          signalStart = now;
          st = 1;
          gapLength = sub32(signalStart, signalEnd);
          if (gapLength > 20 && (unsigned)gapLength < (unsigned)(tgm * 3.0f) && sub32(signalStart, oldTime) > 5000) {
            ev = 1;
            evval = gapLength;
            oldTime = signalStart;
          }
        } else {
          noSignal = now;
          interGap = sub32(noSignal, signalEnd);
          if ((double)interGap > (double)ditLength * 1.95 && charFlag)
            st = 5;
          else if ((double)interGap > (double)ditLength * 4.5 && !blankFlag && !charFlag)
            st = 6;
        }
      } else if (st == 1) {
        if (!key) {
          currentTime = now;
          elapsed = sub32(currentTime, signalStart);
          if (elapsed < 20) {
            st = 0;
          } else {
            if (elapsed > 20 && elapsed < kCwHistElements && sub32(currentTime, oldTime) > 5000) {
              ev = 2;
              evval = elapsed;
              oldTime = currentTime;
              // DoSignalHistogram() up to the arrays, :765-789
              if (valFlag == 0) {
                valRef1 = elapsed;
                signalStartOld = now;
                valFlag = 1;
              }
              if ((unsigned)now - (unsigned)signalStartOld > 20u && valFlag == 1) {
                gapRef1 = gapLength;
                valRef2 = elapsed;
                valFlag = 0;
              }
              const float v1 = (float)valRef1, v2 = (float)valRef2, g1 = (float)gapRef1;
              if ((v2 >= v1 * 2.0f && g1 <= v1 * 2.0f) || (v1 >= v2 * 2.0f && g1 <= v2 * 2.0f)) {
                const bool ditFirst = valRef2 >= valRef1;
                const int dit = ditFirst ? valRef1 : valRef2, dah = ditFirst ? valRef2 : valRef1;
                aveDit = (int)(0.9 * (double)aveDit + 0.1 * (double)dit);
                aveDah = (int)(0.9 * (double)aveDah + 0.1 * (double)dah);
              }
              // sqrt() in double, then to float.  The device's f64 sqrt is correctly rounded, as the host's.  (And the
              // float behind it does not hang on the double's last bit: the product N is an integer below 2^30 and a
              // midpoint m between two floats has 25 bits, so N - m^2 is zero or at least 2^-51 of N -- the root is an
              // integer or two double ulps and more away from every midpoint.)
              tgm = (float)sqrt((double)(int)((unsigned)aveDit * (unsigned)aveDah));
            }
            signalEnd = currentTime;
            st = 2;
          }
        }
      } else if (st == 2) {
        if ((double)elapsed > 0.5 * (double)ditLength) {
          dashJump >>= 1;
          index = (index + (elapsed < (int)tgm ? 1 : dashJump)) & 255;
          charFlag = true;
        }
        st = 0;
      } else if (st == 5) {
        ch = index < kCwTreeChars ? (int)tree[index] : (int)'-';  // (past the literal: the tree's own filler)
        index = 0;
        dashJump = 128;
        charFlag = false;
        blankFlag = false;
        st = 0;
      } else if (st == 6) {
        ch = (int)' ';
        blankFlag = true;
        st = 0;
      }
      ++n;
      if (!live) ev = 0;

      // the histogram calls of this frame, one channel at a time, by the whole wave
      unsigned long long pending = __ballot(ev != 0);
      while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        // (wave-uniform by construction; said so, so that the branches and loop bounds below are scalar)
        const int type = __builtin_amdgcn_readfirstlane(__shfl(ev, src)), val = __builtin_amdgcn_readfirstlane(__shfl(evval, src));
        const float t = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(__shfl(tgm, src))));
        int32_t *g = a.state + (size_t)(ch0 + src) * kCwDecWords + (type == 1 ? kCwDecOffGap : kCwDecOffSig);
        const int cap = type == 1 ? kCwDecGapWords : kCwDecSigWords;
        __syncthreads();
        for (int k = lane; k < cap; k += 64) hl[k] = g[k];
        __syncthreads();
        bool scaled;
        if (type == 2) {
          // :791-814
          if (lane == 0 && (unsigned)val < (unsigned)cap) hl[val] += 1;
          __syncthreads();
          const int offset = (int)((unsigned)t - 1u);
          int tempDit, dit, tempDah, dah;
          clustered_max(hl, cap, 0, offset, 1, lane, &tempDit, &dit);
          clustered_max(hl, cap, offset, kCwHistElements - offset, 3, lane, &tempDah, &dah);
          scaled = (double)tempDit > kScaleConstant && (double)tempDah > kScaleConstant;
          __syncthreads();
          if (scaled)
            for (int k = lane; k < kCwHistElements; k += 64) hl[k] = (int)(0.8 * (double)hl[k]);
          if (lane == src) {
            ditLength = (unsigned)dit;
            dahLength = dah + offset;
          }
        } else {
          // DoGapHistogram(), :660-698
          scaled = rd(hl, val, cap) > 10;
          __syncthreads();
          if (scaled)
            for (int k = lane; k < kCwHistElements; k += 64) hl[k] = (int)(unsigned)(.8 * (double)(float)hl[k]);
          __syncthreads();
          if (lane == 0 && (unsigned)val < (unsigned)cap) hl[val] += 1;
          __syncthreads();
          int atom = __shfl(gapAtom, src), top = __shfl(topGap, src), chr = 0;
          const int topOld = __shfl(topGapOld, src);
          const bool atomBranch = (float)val <= t;
          if (atomBranch) {
            int cnt, atomIndex;
            clustered_max(hl, cap, 0, (int)(unsigned)t, 1, lane, &cnt, &atomIndex);
            if (atomIndex) atom = atomIndex;
            // :674-684: the highest non-empty word below 2 * gapAtom, counting down from word 750
            const int twice = (int)(2u * (unsigned)atom);
            int found = 0;
            for (int i = 1 + lane; i <= kCwHistElements; i += 64)
              if (hl[i] > 0 && i < twice) found = i;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) found = max(found, __shfl_xor(found, off));
            if (found)
              top = found;
            else if (top > twice)
              top = topOld;  // discard outliers
          } else if ((float)val <= t * 2.0f) {
            int cnt;
            clustered_max(hl, cap, (int)t + 1, (int)(unsigned)(t * 2.0f), 3, lane, &cnt, &chr);
          }
          if (lane == src) {
            gapAtom = atom;
            if (atomBranch) {
              topGap = top;
              topGapOld = top;
            }
            if (chr) gapChar = chr;
          }
        }
        __syncthreads();
        // what changed goes back: words 0 .. 749 after a scaling pass, and the incremented word where that pass did not
        // cover it (no pass, or a gap of 750 ms and more: gapLen runs up to 3 * thresholdGeometricMean)
        if (scaled)
          for (int k = lane; k < kCwHistElements; k += 64) g[k] = hl[k];
        if (lane == 0 && (unsigned)val < (unsigned)cap && (!scaled || val >= kCwHistElements)) g[val] = hl[val];
      }
      outl[lane * kOutPitch + 2 * fr] = ch;
      outl[lane * kOutPitch + 2 * fr + 1] = (int)ditLength;
    }
    __syncthreads();
    for (int kk = 0; kk < nlive; ++kk)
      if (lane < 2 * nf) a.text[((size_t)(ch0 + kk) * a.nframes + f0) * 2 + lane] = outl[kk * kOutPitch + lane];
    __syncthreads();
  }
  if (live) {
    w[kCwDecState] = st;
    w[kCwDecN] = (int)n;
    w[kCwDecOldTime] = oldTime;
    w[kCwDecSignalStart] = signalStart;
    w[kCwDecSignalEnd] = signalEnd;
    w[kCwDecElapsed] = elapsed;
    w[kCwDecGapLength] = gapLength;
    w[kCwDecDitLength] = (int)ditLength;
    w[kCwDecDahLength] = dahLength;
    w[kCwDecGapAtom] = gapAtom;
    w[kCwDecGapChar] = gapChar;
    w[kCwDecTgm] = __float_as_int(tgm);
    w[kCwDecAveDit] = aveDit;
    w[kCwDecAveDah] = aveDah;
    w[kCwDecValRef1] = valRef1;
    w[kCwDecValRef2] = valRef2;
    w[kCwDecGapRef1] = gapRef1;
    w[kCwDecValFlag] = valFlag;
    w[kCwDecSignalStartOld] = signalStartOld;
    w[kCwDecDashJump] = dashJump;
    w[kCwDecIndex] = index;
    w[kCwDecCharFlag] = charFlag ? 1 : 0;
    w[kCwDecBlankFlag] = blankFlag ? 1 : 0;
    w[kCwDecTopGap] = topGap;
    w[kCwDecTopGapOld] = topGapOld;
    w[kCwDecCurrentTime] = currentTime;
    w[kCwDecInterGap] = interGap;
    w[kCwDecNoSignal] = noSignal;
  }
}

// ResetHistograms() (CWProcessing.cpp:501-517), one wave per channel
__global__ __launch_bounds__(64) void cw_decode_reset_kernel(int32_t *state, const uint8_t *mask, int nchan) {
  const int chan = blockIdx.x, lane = threadIdx.x;
  if (chan >= nchan || (mask && !mask[chan])) return;
  int32_t *w = state + (size_t)chan * kCwDecWords;
  for (int k = lane; k < kCwHistElements; k += 64) {
    w[kCwDecOffSig + k] = 0;
    w[kCwDecOffGap + k] = 0;
  }
  if (lane == 0) {
    w[kCwDecGapAtom] = 80;
    w[kCwDecDitLength] = 80;
    w[kCwDecGapChar] = 240;
    w[kCwDecDahLength] = 240;
    w[kCwDecTgm] = __float_as_int(160.0f);
    w[kCwDecAveDit] = 80;
    w[kCwDecAveDah] = 240;
    w[kCwDecValRef1] = 0;
    w[kCwDecValRef2] = 0;
  }
}

void cw_decode_power_on(int32_t *w) {
  for (int k = 0; k < kCwDecWords; ++k) w[k] = 0;
  const float tgm = 160.0f;
  w[kCwDecGapAtom] = 80;
  w[kCwDecDitLength] = 80;
  w[kCwDecGapChar] = 240;
  w[kCwDecDahLength] = 240;
  std::memcpy(&w[kCwDecTgm], &tgm, sizeof(tgm));
  w[kCwDecAveDit] = 80;
  w[kCwDecAveDah] = 240;
  w[kCwDecDashJump] = 128;  // DECODER_BUFFER_SIZE
}

hipError_t launch_cw_decode(const CwDecodeArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || !a.cw || !a.state || !a.text || a.num < 0 || a.den <= 0) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(cw_decode_kernel, dim3((unsigned)((a.nchan + 63) / 64)), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_decode_reset(int32_t *state, const uint8_t *mask, int nchan, hipStream_t s) {
  if (nchan <= 0 || !state) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(cw_decode_reset_kernel, dim3((unsigned)nchan), dim3(64), 0, s, state, mask, nchan);
  return hipGetLastError();
}

hipError_t launch_cw_filter(const CwFilterArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nsamp <= 0 || a.nsamp % df2t::kChunk || a.index < 0 || a.index >= kCwFilters) return hipErrorInvalidConfiguration;
  const unsigned waves = (unsigned)((a.nchan + kCwChanPerWave - 1) / kCwChanPerWave);
  hipLaunchKernelGGL(cw_filter_kernel, dim3(waves), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_back(const CwBackArgs &a, hipStream_t s) {
  // (an output map without a listened channel comes with no audio buffer: no block stores)
  if (a.nchan <= 0 || a.nframes <= 0 || !a.aud || !a.state || (!a.out && !a.out_map)) return hipErrorInvalidConfiguration;
  if (a.out_map) hipLaunchKernelGGL(cw_back_omap_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(cw_back_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_detect(const CwDetectArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(cw_detect_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
