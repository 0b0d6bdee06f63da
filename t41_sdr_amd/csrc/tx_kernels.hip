// t41_sdr_amd/csrc/tx_kernels.hip -- gfx950 kernel of the T41 transmit exciter, ExciterIQData()
// (Exciter.cpp:46-169): the receive path's resamplers run backwards with fixed tables.
//
// One 64-lane wave = one channel, all the frames of a call, every stage fused; the delay lines live
// in the wave's LDS for the whole call (HBM state read once, written once).  Per frame a channel
// reads 4 KiB (2048 q15 microphone samples) and writes 8 KiB (2048 q15 I + 2048 q15 Q).
//   arm_q15_to_float                               Exciter.cpp:63-64
//   /4, 48 taps (coeffs192K_10K_LPF_FIR)           :84      dec1: 8 outputs per lane
//   /2, 24 taps (coeffs48K_8K_LPF_FIR[0..23])      :88      dec2: 4 outputs per lane
//   DoExciterEQ() where xmitEQFlag is on           :94-98   tx_kernel<true> only, see below
//   copy L -> R                                    :98
//   Hilbert +45 / -45 degrees, 100 taps each       :110-111 4 consecutive outputs per lane, one window
//   TX IQ amplitude / phase correction             :117-127
//   x2, 48 taps; x4, 32 taps, per channel          :141-148 polyphase (arm_fir_interpolate_f32)
//   x 20, arm_float_to_q15                         :151-162
// Every FIR sums its taps in CMSIS-DSP's order with separate multiplies and adds (no FMA
// contraction): the q15 outputs then equal the reference arithmetic's except where a float sits
// within rounding of a truncation boundary.
// Not tuned (scalar f32 MACs, LDS windows): a side path of this library, SURVEY 8f rank 3.
//
// The x2 / x4 interpolators, their delay lines' load, roll and store, and the q15 packing are tx_interp.hpp's, shared with
// the CW and the calibration exciter: both instantiations keep the arithmetic they had (the same floating-point operations
// in the same order, no contraction), not the instruction stream.
//
// The transmit equaliser (DoExciterEQ(), Filter.cpp:176-224) is the tx_kernel<true> instantiation; tx_kernel<false> holds
// none of its code.  It runs in place on the frame's 256 samples @24 kS/s, between the /2
// decimator and the Hilbert pair, on df2t_pipe.hpp's pipeline with eq_kernel.hip's lane mapping: 14 bands of 4 cascaded
// DF2T sections on the same input, one section per lane (lane 4 * band + stage), band k's output times its signed level,
// the products summed as EQ1 + EQ2, then + EQ3, .., + EQ14.  Stage 0 takes its sample by an LDS broadcast.  The Hilbert
// pair needs the whole block, so the 4-deep pipeline fills and drains once per frame: 259 steps, the 3 fill and 3 drain
// steps guarded per lane.  The ring lies over the first 1848 floats of the 192 kS/s delay line, which is dead between
// the /4 decimator and the roll at the frame's end: the equaliser adds no LDS.
#include <hip/hip_runtime.h>

#include "df2t_pipe.hpp"
#include "tx_interp.hpp"

namespace t41 {

namespace {

// LDS layout of the wave (floats): every delay line as [history | new], history first
constexpr int kXs = 0;                    // 47 + 2048 (+1)
constexpr int kY1 = kXs + 2096;           // 23 + 512 (+1)
constexpr int kHl = kY1 + 536;            // 99 + 256 (+1): both Hilbert filters see the same samples (Exciter.cpp:98)
constexpr int kIl = kHl + 356;            // the interpolators' lines, tx_interp.hpp
constexpr int kLdsFloats = kIl + kInterpFloats;

// ---- transmit equaliser (tx_kernel<true>)
static_assert(kTxEqBands == df2t::kBands, "df2t::sum_bands sums the equaliser's bands");
constexpr int kEqStages = kTxEqSections / kTxEqBands;
constexpr int kEqChunk = df2t::kChunk;      // samples per sum pass
constexpr int kEqRingAt = kXs;              // over the new samples @192 kS/s, which the /4 decimator has consumed
static_assert(kEqRingAt % 4 == 0 && kEqRingAt + kTxEqBands * df2t::kRowPitch <= kXs + 2048,
              "the ring must leave the delay line's last 47 samples alone: the roll at the frame's end reads them");
typedef df2t::Pipe<kEqStages, df2t::kQuadFromPrev, true, false> EqPipe;

// the kernel's argument block: TxArgs, with the equaliser's table, levels and memories behind it where it is on
template <bool EQ>
struct TxKernelArgs {
  typedef TxArgs type;
};
template <>
struct TxKernelArgs<true> {
  typedef TxEqArgs type;
};
}  // namespace

// EQ: xmitEQFlag
template <bool EQ>
__global__ __launch_bounds__(64) void tx_kernel(const typename TxKernelArgs<EQ>::type a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int lane = threadIdx.x;
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  float *st = a.state + (size_t)ch * kTxDelayFloats;
  CoefPtr cf = (CoefPtr)a.coef;

  // ---- equaliser: this lane's section and level, HBM -> VGPRs, once per call
  const bool eq_live = lane < kTxEqSections;
  EqPipe eq;
  if constexpr (EQ) {
    eq.head = (lane & 3) == 0;
    eq.tail = eq_live && (lane & 3) == kEqStages - 1;
    if (eq_live) {
      const float *c = a.eq_coef + 5 * lane;
      const float *m = a.eq_state + (size_t)ch * kTxEqStateFloats;
      eq.q = df2t::Section{c[0], c[1], c[2], c[3], c[4], m[2 * lane], m[2 * lane + 1]};
      eq.level = a.eq_scale[lane >> 2];
    }
  }

  // ---- delay lines: HBM -> LDS, once per call
  if (lane < 47) lds[kXs + lane] = st[kTxStDec1 + lane];
  if (lane < 23) lds[kY1 + lane] = st[kTxStDec2 + lane];
  for (int i = lane; i < 99; i += 64) lds[kHl + i] = st[kTxStHilL + i];  // (FIR_Hilbert_state_R holds the same samples)
  interp_load(lds + kIl, st, lane);
  wave_sync();

  for (int f = 0; f < a.nframes; ++f) {
    const size_t base = ((size_t)ch * a.nframes + f) * 2048;
    // ---- arm_q15_to_float (x / 32768, exact)
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const uint4 w = *reinterpret_cast<const uint4 *>(a.inL + base + 512 * it + 8 * lane);
      const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lds[kXs + 47 + 512 * it + 8 * lane + 2 * k] = (float)(short)(ww[k] & 0xffffu) * (1.0f / 32768.0f);
        lds[kXs + 47 + 512 * it + 8 * lane + 2 * k + 1] = (float)((int)ww[k] >> 16) * (1.0f / 32768.0f);
      }
    }
    wave_sync();
    // ---- /4: y[m] = sum_i c[i] state[4 m + i], m = lane + 64 j
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
      const int m = lane + 64 * j;
      float acc = 0.0f;
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        const float4 t = lds4(lds + kXs + 4 * m + 4 * q);
        acc += t.x * cf->c192[4 * q];
        acc += t.y * cf->c192[4 * q + 1];
        acc += t.z * cf->c192[4 * q + 2];
        acc += t.w * cf->c192[4 * q + 3];
      }
      lds[kY1 + 23 + m] = acc;
    }
    wave_sync();
    // ---- /2: y[m] = sum_i c[i] state[2 m + i], m = lane + 64 j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = lane + 64 * j;
      float acc = 0.0f;
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        const float2 t = *reinterpret_cast<const float2 *>(lds + kY1 + 2 * m + 2 * q);
        acc += t.x * cf->c48[2 * q];
        acc += t.y * cf->c48[2 * q + 1];
      }
      lds[kHl + 99 + m] = acc;
    }
    wave_sync();
    // ---- DoExciterEQ() on those 256 samples, in place (Filter.cpp:176-224)
    if constexpr (EQ) {
      float *x = lds + kHl + 99;
      eq.row = lds + kEqRingAt + (eq_live ? (lane >> 2) : 0) * df2t::kRowPitch;
      eq.r0 = eq.r1 = eq.r2 = eq.r3 = 0.0f;
      const int stage = lane & 3;
      // samples 64 k .. 64 k + 63 through the sum and back over the input
      auto sum_chunk = [&](int k) { x[k * kEqChunk + lane] = df2t::sum_bands(lds + kEqRingAt + (k & 1) * kEqChunk + lane); };
      // chunk 0, the pipeline fills: stage s starts at step s
#pragma unroll
      for (int j = 0; j < kEqChunk; ++j) eq.run(x[j], j, 0, j >= 3 || j >= stage);
      for (int c = 1; c < 256 / kEqChunk; ++c) {
#pragma unroll
        for (int j = 0; j < kEqChunk; ++j) eq.run(x[kEqChunk * c + j], j, c, true);
        wave_sync();
        sum_chunk(c - 1);
      }
      // the pipeline drains: step 256 + d runs stages d + 1 .. 3 on the frame's last samples
      eq.run(0.0f, kEqChunk + 0, 256 / kEqChunk - 1, stage > 0);
      eq.run(0.0f, kEqChunk + 1, 256 / kEqChunk - 1, stage > 1);
      eq.run(0.0f, kEqChunk + 2, 256 / kEqChunk - 1, stage > 2);
      wave_sync();
      sum_chunk(256 / kEqChunk - 1);
      wave_sync();
      // Forget what was loaded through cf.  Otherwise the compiler keeps the interpolators' coefficients in SGPRs across
      // the frame loop, the serial loop above loses its lane masks to spill lanes (72 v_readlane_b32 in it, not 8) and a
      // launch of 4096 x 32 takes 3 % longer; loading them again behind the equaliser costs nothing measurable.
      asm volatile("" : "+s"(cf));
    }
    // ---- Hilbert pair: y[n] = sum_i c[i] state[n + i], n = 4 lane + j, one window for both filters
    float I4[4], Q4[4];
    {
      float w[104];
#pragma unroll
      for (int q = 0; q < 26; ++q) {
        const float4 t = lds4(lds + kHl + 4 * lane + 4 * q);
        w[4 * q] = t.x;
        w[4 * q + 1] = t.y;
        w[4 * q + 2] = t.z;
        w[4 * q + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float ai = 0.0f, aq = 0.0f;
#pragma unroll
        for (int i = 0; i < 100; ++i) {
          ai += w[j + i] * cf->h45[i];
          aq += w[j + i] * cf->hn45[i];
        }
        I4[j] = ai;
        Q4[j] = aq;
      }
    }
    // ---- TX IQ correction (Exciter.cpp:117-127; IQPhaseCorrection Utility.cpp:178-187)
    if (a.corr_on) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        I4[j] = I4[j] * a.i_scale;
        if (a.iq_phase < 0.0f) Q4[j] = Q4[j] + I4[j] * a.iq_phase;
        else I4[j] = I4[j] + Q4[j] * a.iq_phase;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) Q4[j] = Q4[j] * 1.00f;
    // ---- x2 (48 taps, 24 per phase) then x4 (32 taps, 8 per phase), I then Q
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float *s1 = lds + kIl + kInt1Pitch * c, *s2 = lds + kIl + kInt2At + kInt2Pitch * c;
      wave_sync();
      *reinterpret_cast<float2 *>(s1 + 23 + 4 * lane + 1) = make_float2(c ? Q4[1] : I4[1], c ? Q4[2] : I4[2]);  // (23 + 4 lane + 1 is even)
      s1[23 + 4 * lane] = c ? Q4[0] : I4[0];
      s1[23 + 4 * lane + 3] = c ? Q4[3] : I4[3];
      wave_sync();
      interp2_block(s1, s2, cf, lane);
      wave_sync();
      // n = lane + 64 u: 8 bytes per lane and u
      int16_t *out = (c ? a.outR : a.outL) + base;
#pragma unroll 2
      for (int u = 0; u < 8; ++u) {
        const int n = lane + 64 * u;
        float o[4];
        interp4_point(s2, n, cf, o);
        // x 20 (Exciter.cpp:151-152), arm_float_to_q15 (:161-162)
        *reinterpret_cast<uint2 *>(out + 4 * n) = make_uint2(q15_pack2(o[0] * 20.0f, o[1] * 20.0f), q15_pack2(o[2] * 20.0f, o[3] * 20.0f));
      }
    }
    // ---- roll the delay lines: the last numTaps - 1 samples move to the front
    wave_sync();
    {
      const float x1 = (lane < 47) ? lds[kXs + 2048 + lane] : 0.0f;
      const float y1 = (lane < 23) ? lds[kY1 + 512 + lane] : 0.0f;
      const float h0 = lds[kHl + 256 + lane], h1 = (lane < 35) ? lds[kHl + 256 + 64 + lane] : 0.0f;
      const InterpTails it = interp_tails(lds + kIl, lane);
      wave_sync();
      if (lane < 47) lds[kXs + lane] = x1;
      if (lane < 23) lds[kY1 + lane] = y1;
      lds[kHl + lane] = h0;
      if (lane < 35) lds[kHl + 64 + lane] = h1;
      interp_heads(lds + kIl, it, lane);
    }
    wave_sync();
  }
  // ---- delay lines back to HBM
  if (lane < 47) st[kTxStDec1 + lane] = lds[kXs + lane];
  if (lane < 23) st[kTxStDec2 + lane] = lds[kY1 + lane];
  for (int i = lane; i < 99; i += 64) {
    st[kTxStHilL + i] = lds[kHl + i];
    st[kTxStHilR + i] = lds[kHl + i];
  }
  interp_store(st, lds + kIl, lane);
  if constexpr (EQ) {
    if (eq_live) {
      float *m = a.eq_state + (size_t)ch * kTxEqStateFloats;
      m[2 * lane] = eq.q.d1;
      m[2 * lane + 1] = eq.q.d2;
    }
  }
}

hipError_t launch_tx(const TxArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tx_kernel<false>, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tx_eq(const TxEqArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tx_kernel<true>, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
