// t41_sdr_amd/csrc/nr_kernels.hip -- gfx950 kernels of the receive path's optional stages between the
// demodulator and the interpolators (Process.cpp:841-866): noise reduction (Kim1_NR() Noise.cpp:108-313,
// SpectralNoiseReduction() Noise.cpp:379-655, Xanr() as LMS noise reduction Noise.cpp:322-370) and the
// automatic notch (Xanr() again).  All off in the firmware's defaults; FFT_LENGTH 512.
//
// They run on the call's demodulated audio @24 kS/s, which the fused kernel leaves in a scratch
// ([channel][frame * 256], rx_kernels.hpp: RxArgs::aud_out), in place, frame by frame; the long-FFT
// pipeline's back kernel then interpolates (launch_back512).
//
//  * anr_kernel: Xanr() is a 64-tap adaptive FIR whose every output feeds back into its taps, sample by
//    sample, and whose sums the reference accumulates in tap order.  ONE LANE PER CHANNEL: a wave runs 64
//    channels' filters, every lane the reference's loop as written (same operations, same order, no
//    contraction -- bit-identical to the scalar code; the step is shared by the TWO waves of the workgroup, see
//    anr_pass_y), taps in 64 registers, the delay line's live window
//    in an LDS tile laid out [time][channel] (row pitch 65 floats: conflict-free both for the transposing
//    stage-in / stage-out and for the per-lane window reads).  The tile is filled and drained with
//    coalesced row accesses of the [channel][time] scratch.
//  * nrspec_kernel<KIND>: the two spectral-weighting functions, one wave per channel.  Both transform
//    half-overlapped 256-sample frames, two per block, with real input; here the block's two frames ride
//    as real and imaginary part through ONE 512-point transform of the path's register-resident FFT
//    (zero-interleaved, so that bins 0..255 hold the 256-point transform), are separated by conjugate
//    symmetry, weighted, and go back through ONE inverse transform the same way.  The reference weights bin
//    i together with bin 255 - i (not 256 - i) and keeps the real part of the inverse transform: the real
//    part sees the conjugate-symmetric half of the weighted spectrum, i.e. bin k weighted by
//    (G[k] + G[k-1]) / 2 -- which is what is applied here.  Per-bin statistics: two bins per lane.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "nr_kernels.hpp"
#include "rx_kernels.hpp"
#include "rx_stagesets.hpp"
#include "wave_fft.hpp"

namespace t41 {

// ------------------------------------------------------------------------------------------
// Xanr(): 16 channels per wave, a channel's 64 taps on the four lanes (c, c + 16, c + 32, c + 48)
// ------------------------------------------------------------------------------------------
// Round 3 ran one lane per channel (64 taps in 64 registers): a sample's step was ~430 instructions, 300 of them the
// products, squares and the taps' update -- independent work that one wave had to issue between the 64 additions of the
// filter's output, which the reference accumulates in tap order and which therefore stay a chain.  Round 4 spreads that
// work over the wave: lane (g, c) = 16 g + c holds 16 taps of channel c, so products / update are 8 packed
// instructions per lane instead of 32, and the chain walks through the four lane groups in tap order: every lane adds
// its 16 products to whatever partial sum it holds, the partial sum that matters sits in the "active" group, and after
// 16 additions it moves on to the next group by ONE lane-swap instruction (v_permlane16_swap / v_permlane32_swap; the
// groups are visited in the order 0, 1, 3, 2 because those are the moves the two instructions make).  Same additions,
// same order, same roundings as the scalar loop; a sample costs the chain's 64 dependent additions and little else.
constexpr int kAnrCw = 16;                     // channels per wave / workgroup
constexpr int kAnrRow = kAnrCw + 1;            // LDS row pitch in floats (odd: the transposing stage-in / stage-out and the window reads are conflict-free)
constexpr int kAnrTile = kAnrHist + 256;       // rows of the input tile: 79 of history + the frame
constexpr int kAnrSigOff = ((kAnrTile + 256) * kAnrRow + 3) & ~3;
constexpr size_t kAnrLdsBytes = ((size_t)kAnrSigOff + 3 * kAnrCw * 4) * sizeof(float);  // input tile + output tile + three (round 4: two) slots of 16 x (sigma, 1 / sigma', 1 - 2 mu sigma / sigma' as a double)

// first tap of lane group g: the chain visits the groups in the order 0, 1, 3, 2
__device__ __forceinline__ int anr_tap_base(int g) { return 16 * ((g == 2) ? 3 : (g == 3) ? 2 : g); }
// the partial sum moves from the group that has just finished to the one that continues (every other lane: don't care)
template <int PHASE>
__device__ __forceinline__ float anr_hand_on(float y) {
  float a = y, b = y;
  if (PHASE == 0) {        // group 0 -> group 1
    lane_swap16(a, b);
    return a;
  } else if (PHASE == 1) { // group 1 -> group 3
    lane_swap32(a, b);
    return a;
  } else {                 // group 3 -> group 2
    lane_swap16(a, b);
    return b;
  }
}
// group 2's value to every group
__device__ __forceinline__ float anr_from_group2(float y) {
  float a = y, b = y;
  lane_swap32(a, b);  // b = {y2, y3, y2, y3}
  float c = b, d = b;
  lane_swap16(c, d);  // c = {y2, y2, y2, y2}
  return c;
}
// sum of p[0 .. 15] in tap order on top of the running sum, through the four groups: the reference's 64 additions
__device__ __forceinline__ float anr_chain(const f2 (&p)[8]) {
#pragma clang fp contract(off)
  float y = 0;
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      y += p[t].y;
      y += p[t].x;
    }
    if (ph == 0) y = anr_hand_on<0>(y);
    else if (ph == 1) y = anr_hand_on<1>(y);
    else if (ph == 2) y = anr_hand_on<2>(y);
  }
  return y;  // valid in group 2
}

// One pass of Noise.cpp:331-369 over the 256 samples in T[kAnrHist ..], split over the workgroup's TWO waves (same
// lane -> (group, channel) map in both): wave 1 takes the window's sum of squares (ANR_sigma) and what depends on it
// alone (an IEEE double division), wave 0 the filter output, the error, the leak logic and the taps' update; sigma
// crosses through LDS (two slots: wave 1 may be a sample ahead) behind ONE workgroup barrier per sample.  Every value
// by the same operations in the same order as the scalar loop.
// O (may be null): output tile; SIG: [3][16] float4.
template <bool NOTCH>
__device__ __forceinline__ void anr_pass_y(const float *T, float *O, const float *SIG, f2 (&w)[8], float &lidx, float &ngamma, int lane) {
#pragma clang fp contract(off)
  const float ANR_den_mult = 6.25e-10, ANR_gamma = 0.1, ANR_lidx_min = 120.0, ANR_lidx_max = 200.0;
  const float ANR_lincr = 1.0, ANR_ldecr = 3.0, ANR_two_mu = 0.0001;
  const int c = lane & 15, g = lane >> 4, tb = anr_tap_base(g);
  // The taps' update of sample i is fused into the products of sample i + 1 (it needs sample i's window, which dp still
  // holds): tap pair t is updated, then used.  Same values as updating all taps first.
  float c0 = 1.0f, c1 = 0.0f;  // pending update of the previous sample (none yet: w * 1 + 0 * d would not be exact for
  bool pending = false;        // -0 / NaN taps, so it is skipped rather than applied)
  // Round 5: a sample's window is requested at the top of the PREVIOUS sample's step, into a third register set -- the
  // delay line is the input signal, so every window of the frame is in the tile before the pass starts.  Requested at
  // the top of its own step, as in round 4, the window is waited for twice per sample (two batches of eight reads) at the
  // head of the dependent sequence.  (Requested behind the products into the previous window's registers -- two sets --
  // the chain's first sixteen additions no longer interleave with the products: 148 against 140 us per frame.)
  // (ONE lane-dependent base, opaque to the compiler, and the sixteen rows at immediate offsets from it: eight
  // ds_read2_b32 -- the pairs are 17 dwords apart, 15 x 17 = 255 just fits the offset field.  Left to itself hipcc keeps
  // eight address registers, adds the sample's offset to each and issues sixteen single reads: 25 instructions for 9.)
  typedef const __attribute__((address_space(3))) float *LdsRow;
  LdsRow wbase = (LdsRow)(T + c + (kAnrTaps - 16 - tb) * kAnrRow);
  asm volatile("" : "+v"(wbase));
  auto window = [&](int i, f2 (&dj)[8], float &d_in) {
    d_in = T[i * kAnrRow + c + kAnrHist * kAnrRow];  // ANR_d[ANR_in_idx]
    LdsRow row = wbase + i * kAnrRow;
#pragma unroll
    for (int t = 0; t < 16; t += 2)
      dj[t / 2] = f2{row[(14 - t) * kAnrRow], row[(15 - t) * kAnrRow]};
  };
  // dj: this sample's window (in registers); dp: the previous sample's, for the pending update; dx: takes the next one's
  auto step = [&](int i, int slot, const f2 (&dj)[8], const f2 (&dp)[8], f2 (&dx)[8], const float d_in, float &d_next) {
    if (i + 1 < 256) window(i + 1, dx, d_next);
    // (wave 1 runs a sample ahead: this sample's sigma, with what depends on sigma alone, has been in its slot since the
    // previous sample's barrier)
    const float4 sg = *reinterpret_cast<const float4 *>(SIG + 4 * (kAnrCw * slot + c));  // (slot = i % 3: static per unrolled step)
    __builtin_amdgcn_sched_barrier(0);  // (the requests go out HERE: left alone, the scheduler sinks them behind the chain)
    f2 p[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if (pending) w[t] = splat(c0) * w[t] + splat(c1) * dp[t];
      p[t] = w[t] * dj[t];
    }
    const float y = anr_from_group2(anr_chain(p));
    __syncthreads();  // keeps wave 1 exactly one sample ahead (it must not overwrite a slot this wave has yet to read)
    const float sigma = sg.x, inv_sigp = sg.y;  // inv_sigp = (float)(1.0 / ((double)sigma + 1e-10))
    const double one_m = __hiloint2double(__float_as_int(sg.w), __float_as_int(sg.z));  // 1.0 - (double)(ANR_two_mu * sigma * inv_sigp)
    const float error = d_in - y;
    if (O && g == 0) O[i * kAnrRow + c] = NOTCH ? error : y;
    // |nel|, |nev|: the reference's `if (x < 0) x = -x` and fabsf() differ for x = -0 only, and the two are only ever
    // compared with each other; as operand modifiers of that comparison they cost nothing (as written hipcc compares the
    // DOUBLES with zero and selects: two half-rate compares and two selects per sample)
    const float nel = fabsf((float)((double)error * one_m));
    const float nev = fabsf((float)((double)d_in - (1.0 - (double)(ANR_two_mu * ngamma)) * (double)y - (double)(ANR_two_mu * error * sigma * inv_sigp)));
    if (nev < nel) {  // as written (Noise.cpp:351-356): the else-if belongs to the inner if.  (Branches on purpose: most samples
      // skip the block; the same logic as selects is seven instructions on every sample and measured 2 us per frame slower)
      lidx += ANR_lincr;
      if (lidx > ANR_lidx_max) {
        lidx = ANR_lidx_max;
      } else {
        lidx -= ANR_ldecr;
        if (lidx < ANR_lidx_min) lidx = ANR_lidx_min;
      }
    }
    ngamma = ANR_gamma * (lidx * lidx) * (lidx * lidx) * ANR_den_mult;
    c0 = (float)(1.0 - (double)(ANR_two_mu * ngamma));
    c1 = ANR_two_mu * error * inv_sigp;
    pending = true;
  };
  f2 da[8], db[8], dc[8];
  float din_a, din_b = 0.0f, din_c = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) dc[t] = splat(0.0f);
  window(0, da, din_a);
  __syncthreads();  // wave 1's sigma of sample 0
  for (int i = 0; i < 255; i += 3) {  // 85 x 3 samples
    step(i, 0, da, dc, db, din_a, din_b);      // window i in da, i - 1 in dc; i + 1 -> db
    step(i + 1, 1, db, da, dc, din_b, din_c);  // i + 2 -> dc
    step(i + 2, 2, dc, db, da, din_c, din_a);  // i + 3 -> da
  }
  step(255, 0, da, dc, db, din_a, din_b);  // (255 = 3 x 85)
#pragma unroll
  for (int t = 0; t < 8; ++t) db[t] = da[t];  // the last sample's update below takes its window from db
  // the last sample's update (its window is in db)
#pragma unroll
  for (int t = 0; t < 8; ++t) w[t] = splat(c0) * w[t] + splat(c1) * db[t];
}
__device__ __forceinline__ void anr_pass_sigma(const float *T, float *SIG, int lane) {
#pragma clang fp contract(off)
  const int c = lane & 15, g = lane >> 4, tb = anr_tap_base(g);
  auto sigma_of = [&](int i) {
    const float *row = T + i * kAnrRow + c;
    f2 q[8];
#pragma unroll
    for (int t = 0; t < 16; t += 2) {
      const f2 d = f2{row[(kAnrTaps - 2 - tb - t) * kAnrRow], row[(kAnrTaps - 1 - tb - t) * kAnrRow]};
      q[t / 2] = d * d;
    }
    const float sigma = anr_chain(q);  // (group 2 holds it)
    const float ANR_two_mu = 0.0001;
    const float inv_sigp = (float)(1.0 / ((double)sigma + 1e-10));
    const double one_m = 1.0 - (double)(ANR_two_mu * sigma * inv_sigp);
    if (g == 2)
      *reinterpret_cast<float4 *>(SIG + 4 * (kAnrCw * (i % 3) + c)) =
          make_float4(sigma, inv_sigp, __int_as_float(__double2loint(one_m)), __int_as_float(__double2hiint(one_m)));
  };
  // one sample AHEAD of the filter wave: sigma of sample i is in its slot before the barrier of sample i - 1, so the filter
  // wave reads it at the top of its step, not behind its chain (the slot it overwrites, i + 1's = i - 1's, was read at the
  // top of step i - 1, a barrier ago)
  sigma_of(0);
  __syncthreads();
  for (int i = 0; i < 256; ++i) {
    if (i + 1 < 256) sigma_of(i + 1);
    __syncthreads();
  }
}

// LIST: the stage map's form (t41rx_set_stage_map).  Column c of workgroup b serves channel list[16 b + c]: the audio
// staging addresses the listed channel's rows (a scalar load per column), and the state rows, channel-minor, are gathered
// and scattered per lane -- 16 lanes of a request name 16 arbitrary channels of a row where the form without a map reads
// 64 consecutive bytes.  That is once per launch and state row, against 256 samples per frame of the serial chain.
#define T41_STAGE_KERNEL anr_kernel
#define T41_STAGE_LIST 0
#include "anr_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL anr_list_kernel
#define T41_STAGE_LIST 1
#include "anr_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
// MAP: the noise-reduction map's form (t41rx_set_nr_map).  The list form again, and workgroup b takes its place in the list,
// its live columns and which of the two passes it runs from row b of the map's table (rx_nrmap.hpp: NrMapRow) instead of
// the grid and the launch: one launch serves the LMS channels, the notch channels and the channels with both.
#define T41_STAGE_KERNEL anr_map_kernel
#define T41_STAGE_LIST 2
#include "anr_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST

// ------------------------------------------------------------------------------------------
// Kim1_NR() / SpectralNoiseReduction(), one wave per channel
// ------------------------------------------------------------------------------------------
// sum over the wave, the same value in every lane: an inclusive scan inside the VALU (four row shifts, two row
// broadcasts: DPP, no LDS round trips -- the spectral function's gain loop calls this once per bin) and lane 63's total
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<kDppRowShr1, 0xf, true>(0.0f, v);
  v += dpp_f<kDppRowShr2, 0xf, true>(0.0f, v);
  v += dpp_f<kDppRowShr4, 0xf, true>(0.0f, v);
  v += dpp_f<kDppRowShr8, 0xf, true>(0.0f, v);
  v += dpp_f<kDppRowBcast15, 0xa, false>(0.0f, v);
  v += dpp_f<kDppRowBcast31, 0xc, false>(0.0f, v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// the same sum, for its total only: six fused DPP additions (what wave_sum() compiles to spends three instructions on each
// of the two row-stitching steps); same operands, same order
__device__ __forceinline__ float wave_sum_fused(float v) {
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 0"
      : "+v"(v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ void lds_fence() { asm volatile("" ::: "memory"); }
constexpr unsigned fbits(float x) { return __builtin_bit_cast(unsigned, x); }
// is the (non-negative) power ratio with bit pattern rb within 5e-5 of one of the values NN changes at?  (Non-negative
// floats order like their bit patterns; NaN patterns sit above every bound: "not near", and NN = 1 like the formula's.)
__device__ __forceinline__ bool nr_ratio_near_edge(unsigned rb) {
  bool near = false;
  for (float b : {0.4f, 0.35f, 0.25f, 0.15f, 0.05f}) near = near || (rb >= fbits(b - 5e-5f) && rb <= fbits(b + 5e-5f));
  return near;
}

// KINDL = KIND, or KIND + kNrList for the stage map's form (t41rx_set_stage_map): the grid is the list's length and the
// wave takes its channel from the list, one scalar load.  The switch rides on the KIND argument, as the input map rides on
// rx512_kernel's PART, so that nrspec_kernel<1> and nrspec_kernel<2> keep their names and their instruction streams.
constexpr int kNrList = 4;
template <int KINDL>
__global__ __launch_bounds__(64) void nrspec_kernel(const NrArgs a) {
#pragma clang fp contract(off)
  constexpr int KIND = KINDL & 3;
  constexpr bool LIST = (KINDL & kNrList) != 0;
  static_assert(KIND == 1 || KIND == 2, "Kim1_NR() or SpectralNoiseReduction()");
  constexpr int KLDS = KIND;
#include "nrspec_lds.inc"
  const int lane = threadIdx.x;
  if (!LIST && (int)blockIdx.x >= a.nchan) return;
  const int ch = LIST ? a.list[blockIdx.x] : (int)blockIdx.x;
#include "nrspec_body.inc"
}

// The noise-reduction map's form (t41rx_set_nr_map): workgroup b takes its channel AND its kind from the spectral list,
// two scalar loads, and runs the text of nrspec_kernel<1> or of nrspec_kernel<2> under a wave-uniform branch -- one launch
// serves the Kim channels and the spectral channels of a call, and costs the longer of the two chains, not their sum.
// The LDS is laid out once, for Kim1_NR() (the larger: its frame histories); a spectral workgroup leaves those idle.
__global__ __launch_bounds__(64) void nrspec_map_kernel(const NrMapArgs a) {
#pragma clang fp contract(off)
  constexpr int KLDS = 1;
#include "nrspec_lds.inc"
  const int lane = threadIdx.x;
  const int ch = a.spec_list[blockIdx.x];
  if (a.spec_kind[blockIdx.x] == 1) {
    constexpr int KIND = 1;
#include "nrspec_body.inc"
  } else {
    constexpr int KIND = 2;
#include "nrspec_body.inc"
  }
}

// Parameter sets next to the stages (t41rx_set_param_sets_ex with T41RX_SETS_STAGES): nrspec_map_kernel's text again, and
// the five values the body reads of its argument block -- NR_alpha, NR_beta, NR_PSI, the VAD range -- come from the
// channel's row of a table [nchan] made at set time.  The workgroup's channel is uniform (a scalar load of the list), so
// the row is one scalar load of eight dwords and the values sit in scalar registers, as the kernel arguments of the other
// forms do; nothing is written through the scalar path.  `a` below is what the body names: the block's pointers and
// counts with the row's values in the places of the block's.
__global__ __launch_bounds__(64) void nrspec_sets_kernel(const NrSetsArgs b) {
#pragma clang fp contract(off)
  constexpr int KLDS = 1;
#include "nrspec_lds.inc"
  const int lane = threadIdx.x;
  const int ch = b.spec_list[blockIdx.x];
  const NrSetRow row = b.set_rows[ch];
  const struct {
    float *aud, *spec;
    const float *tab_nr;
    const float2 *tab;
    int nframes;
    float alpha, beta, psi;
    int vad_lo, vad_hi;
  } a = {b.aud, b.spec, b.tab_nr, b.tab, b.nframes, row.alpha, row.beta, row.psi, row.vad_lo, row.vad_hi};
  if (b.spec_kind[blockIdx.x] == 1) {
    constexpr int KIND = 1;
#include "nrspec_body.inc"
  } else {
    constexpr int KIND = 2;
#include "nrspec_body.inc"
  }
}

namespace {
// the spectral function and Xanr() of one call take the same channels (with a list: both the same list)
hipError_t launch_nr_list(const NrArgs &a, hipStream_t s) {
  if (a.nlist <= 0 || a.nlist > a.nchan) return hipErrorInvalidConfiguration;
  if (a.nr_option == 1)
    hipLaunchKernelGGL((nrspec_kernel<1 + kNrList>), dim3(a.nlist), dim3(64), 0, s, a);
  else if (a.nr_option == 2)
    hipLaunchKernelGGL((nrspec_kernel<2 + kNrList>), dim3(a.nlist), dim3(64), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.nr_option == 3 || a.notch) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&anr_list_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAnrLdsBytes);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(anr_list_kernel, dim3((a.nlist + kAnrCw - 1) / kAnrCw), dim3(128), kAnrLdsBytes, s, a);
    e = hipGetLastError();
  }
  return e;
}
}  // namespace

static_assert(kAnrCw == 16, "rx_nrmap.hpp (kNrMapCols) cuts the Xanr() list into workgroups of this many columns");
hipError_t launch_nr_map(const NrMapArgs &a, hipStream_t s) {
  if (a.nspec < 0 || a.nspec > a.nchan || a.nrows < 0 || a.nrows > a.nchan / kAnrCw + 3) return hipErrorInvalidConfiguration;
  hipError_t e = hipSuccess;
  if (a.nspec > 0) {
    hipLaunchKernelGGL(nrspec_map_kernel, dim3(a.nspec), dim3(64), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.nrows > 0) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&anr_map_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAnrLdsBytes);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(anr_map_kernel, dim3(a.nrows), dim3(128), kAnrLdsBytes, s, a);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_nr_sets(const NrSetsArgs &a, hipStream_t s) {
  if (a.nspec < 0 || a.nspec > a.nchan || a.nrows < 0 || a.nrows > a.nchan / kAnrCw + 3 || !a.set_rows) return hipErrorInvalidConfiguration;
  if (a.nspec > 0) {
    hipLaunchKernelGGL(nrspec_sets_kernel, dim3(a.nspec), dim3(64), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  NrMapArgs m = a;  // Xanr()'s launch alone
  m.nspec = 0;
  return a.nrows > 0 ? launch_nr_map(m, s) : hipSuccess;
}

hipError_t launch_nr(const NrArgs &a, hipStream_t s) {
  if (a.list) return launch_nr_list(a, s);
  if (a.nr_option == 1)
    hipLaunchKernelGGL((nrspec_kernel<1>), dim3(a.nchan), dim3(64), 0, s, a);
  else if (a.nr_option == 2)
    hipLaunchKernelGGL((nrspec_kernel<2>), dim3(a.nchan), dim3(64), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.nr_option == 3 || a.notch) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&anr_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAnrLdsBytes);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(anr_kernel, dim3((a.nchan + kAnrCw - 1) / kAnrCw), dim3(128), kAnrLdsBytes, s, a);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace t41
