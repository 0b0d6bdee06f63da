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

// MAP: the CW filter map's form (t41rx_set_cw_filter_map).  The grid is the filtered channels' list over eight, the wave
// takes its eight channels from the list and every group of eight lanes its own channel's CWFilterIndex; see the text.
#define T41_STAGE_KERNEL cw_filter_kernel
#define T41_STAGE_ARGS CwFilterArgs
#define T41_STAGE_MAP 0
#include "cw_filter_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_MAP
#define T41_STAGE_KERNEL cw_filter_map_kernel
#define T41_STAGE_ARGS CwFilterMapArgs
#define T41_STAGE_MAP 1
#include "cw_filter_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_MAP

// LIST: the stage map's form (t41rx_set_stage_map).  The grid is the list's length and the wave takes its channel from the
// list, one scalar load; the rows of `out` of the channels the list leaves out are not written.
#define T41_STAGE_KERNEL cw_detect_kernel
#define T41_STAGE_LIST 0
#include "cw_detect_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL cw_detect_list_kernel
#define T41_STAGE_LIST 1
#include "cw_detect_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST

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

// The same with parameter sets next to the stages (t41rx_set_param_sets_ex with T41RX_SETS_STAGES): the text a third time,
// with or without the output map's row, and the volume factor and the taps from entry set_of[channel] of the sets' table.
// A block is one channel, so the set's number and the volume factor are scalar loads and the taps' rows are read from a
// uniform base; every product and every sum is cw_back_kernel's, in its order (tests/test_stage_sets.py holds the rows to
// that kernel's on a plain context of the channel's set, bit for bit).
__global__ __launch_bounds__(64) void cw_back_sets_kernel(CwBackSetsArgs a) {
#pragma clang fp contract(off)
  constexpr int N = kCwBlock, P1 = 24, P2 = 8;
  const int row = a.out_map ? a.out_map[blockIdx.x] : (int)blockIdx.x;
  if (row < 0) return;  // block-uniform, ahead of every barrier
  __shared__ float s1[P1 - 1 + N + 1];      // arm_fir_interpolate_f32's state of the x2 stage: history, then the block
  __shared__ float s2[P2 - 1 + 2 * N + 1];  // ... of the x4 stage
  __shared__ float c1[48], c2[32];
  const int lane = threadIdx.x;
  const CwSetBack *set = a.sets + a.set_of[blockIdx.x];
  const float scale = set->scale;
  float *st = a.state + (size_t)blockIdx.x * a.state_stride;
  const float *x = a.aud + (size_t)blockIdx.x * a.nframes * N;
  if (lane < 48) c1[lane] = set->int1[lane];
  if (lane < 32) c2[lane] = set->int2[lane];
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
      const float y = acc * scale;
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
// LIST: the stage map's form (t41rx_set_stage_map).  Lane l of block b serves channel list[64 b + l]; lanes past the list's
// end stay dead, as lanes past nchan are without a map.  Every place that named channel ch0 + k names list[ch0 + k]: the
// detector's rows, the histograms the wave serves, the rows of `text`.  The rows of the channels the list leaves out are
// not written.
#define T41_STAGE_KERNEL cw_decode_kernel
#define T41_STAGE_LIST 0
#include "cw_decode_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL cw_decode_list_kernel
#define T41_STAGE_LIST 1
#include "cw_decode_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST

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
  if (a.list && (a.nlist <= 0 || a.nlist > a.nchan)) return hipErrorInvalidConfiguration;
  if (a.list) hipLaunchKernelGGL(cw_decode_list_kernel, dim3((unsigned)((a.nlist + 63) / 64)), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(cw_decode_kernel, dim3((unsigned)((a.nchan + 63) / 64)), dim3(64), 0, s, a);
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

hipError_t launch_cw_filter_map(const CwFilterMapArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nsamp <= 0 || a.nsamp % df2t::kChunk || !a.list || !a.index_of || a.nlist <= 0 || a.nlist > a.nchan) return hipErrorInvalidConfiguration;
  const unsigned waves = (unsigned)((a.nlist + kCwChanPerWave - 1) / kCwChanPerWave);
  hipLaunchKernelGGL(cw_filter_map_kernel, dim3(waves), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_back(const CwBackArgs &a, hipStream_t s) {
  // (an output map without a listened channel comes with no audio buffer: no block stores)
  if (a.nchan <= 0 || a.nframes <= 0 || !a.aud || !a.state || (!a.out && !a.out_map)) return hipErrorInvalidConfiguration;
  if (a.out_map) hipLaunchKernelGGL(cw_back_omap_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(cw_back_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_back_sets(const CwBackSetsArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || !a.aud || !a.state || (!a.out && !a.out_map) || !a.set_of || !a.sets) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(cw_back_sets_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cw_detect(const CwDetectArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || (a.list && (a.nlist <= 0 || a.nlist > a.nchan))) return hipErrorInvalidConfiguration;
  if (a.list) hipLaunchKernelGGL(cw_detect_list_kernel, dim3((unsigned)a.nlist), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(cw_detect_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
