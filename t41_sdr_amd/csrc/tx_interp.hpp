// t41_sdr_amd/csrc/tx_interp.hpp -- the exciters' interpolator back end: the x2 (48 taps) and x4 (32 taps) polyphase
// interpolators of ExciterIQData() (Exciter.cpp:141-148), CW_ExciterIQData() (CW_Excite.cpp:93-100) and ProcessIQData2()
// (Process2.cpp:327-334) on the SSB exciter's own delay lines FIR_int1_EX_I/Q, FIR_int2_EX_I/Q, and the stored-tone exciter
// that CW and the IQ calibration share.  Device code of tx_kernels.hip, tx_cw_kernel.hip and tx_cal_kernel.hip.
//
// One 64-lane wave = one channel; the four delay lines live in the wave's LDS for a whole call as [history | new], HBM state
// read once and written once.  Every FIR sums its taps in CMSIS-DSP's order with separate multiplies and adds.  The
// contraction pragma is lexical: every function here that does arithmetic carries it as its body's first line, because not
// every translation unit that includes this header is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "tx_internal.hpp"

namespace t41 {

// (static: the receive side's wave_fft.hpp has a wave_sync() of its own, which also pins the ALU schedule)
static __device__ __forceinline__ void wave_sync() {
  // one wave per workgroup: LDS executes its instructions in order; only the compiler must not reorder
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ float4 lds4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
typedef const __attribute__((address_space(4))) TxCoef *CoefPtr;

// (q15_t)__SSAT((q31_t)(x * 32768.0f), 16): CMSIS-DSP's arm_float_to_q15 without ARM_MATH_ROUNDING
__device__ __forceinline__ unsigned q15_pack2(float x0, float x1) {
#pragma clang fp contract(off)
  int a = (int)(x0 * 32768.0f), b = (int)(x1 * 32768.0f);
  a = a < -32768 ? -32768 : (a > 32767 ? 32767 : a);
  b = b < -32768 ? -32768 : (b > 32767 ? 32767 : b);
  return ((unsigned)a & 0xffffu) | ((unsigned)b << 16);
}

// LDS of the interpolators (floats from a base `il`): the x2 lines [2][23 + 256 (+1)], then the x4 lines [2][7 + 512 (+1)],
// I then Q
constexpr int kInt1Pitch = 280;
constexpr int kInt2Pitch = 520;
constexpr int kInt2At = 2 * kInt1Pitch;
constexpr int kInterpFloats = kInt2At + 2 * kInt2Pitch;

// the four delay lines' histories: a channel's record `st` -> LDS, and back
__device__ __forceinline__ void interp_load(float *il, const float *st, int lane) {
  if (lane < 23) {
    il[lane] = st[kTxStInt1I + lane];
    il[kInt1Pitch + lane] = st[kTxStInt1Q + lane];
  }
  if (lane < 7) {
    il[kInt2At + lane] = st[kTxStInt2I + lane];
    il[kInt2At + kInt2Pitch + lane] = st[kTxStInt2Q + lane];
  }
}
__device__ __forceinline__ void interp_store(float *st, const float *il, int lane) {
  if (lane < 23) {
    st[kTxStInt1I + lane] = il[lane];
    st[kTxStInt1Q + lane] = il[kInt1Pitch + lane];
  }
  if (lane < 7) {
    st[kTxStInt2I + lane] = il[kInt2At + lane];
    st[kTxStInt2Q + lane] = il[kInt2At + kInt2Pitch + lane];
  }
}

// the roll at a frame's end, the last numTaps - 1 samples to the front: the tails are read before a wave_sync() and the
// heads written after it (a pair, so that a kernel can roll its other lines between the same two barriers)
struct InterpTails {
  float i1a, i1b, i2a, i2b;
};
__device__ __forceinline__ InterpTails interp_tails(const float *il, int lane) {
  InterpTails t;
  t.i1a = (lane < 23) ? il[256 + lane] : 0.0f;
  t.i1b = (lane < 23) ? il[kInt1Pitch + 256 + lane] : 0.0f;
  t.i2a = (lane < 7) ? il[kInt2At + 512 + lane] : 0.0f;
  t.i2b = (lane < 7) ? il[kInt2At + kInt2Pitch + 512 + lane] : 0.0f;
  return t;
}
__device__ __forceinline__ void interp_heads(float *il, const InterpTails &t, int lane) {
  if (lane < 23) {
    il[lane] = t.i1a;
    il[kInt1Pitch + lane] = t.i1b;
  }
  if (lane < 7) {
    il[kInt2At + lane] = t.i2a;
    il[kInt2At + kInt2Pitch + lane] = t.i2b;
  }
}

// x2, 48 taps, 24 per phase, on one line: out[2 n + j - 1] = sum_t state[n + t] c[(2 - j) + 2 t], n = 4 lane + u, from a
// 28-float window of s1 into the new part of s2
__device__ __forceinline__ void interp2_block(const float *s1, float *s2, CoefPtr cf, int lane) {
#pragma clang fp contract(off)
  float w[28];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const float4 t = lds4(s1 + 4 * lane + 4 * q);
    w[4 * q] = t.x;
    w[4 * q + 1] = t.y;
    w[4 * q + 2] = t.z;
    w[4 * q + 3] = t.w;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float o0 = 0.0f, o1 = 0.0f;
#pragma unroll
    for (int t = 0; t < 24; ++t) {
      o0 += w[u + t] * cf->c48[1 + 2 * t];
      o1 += w[u + t] * cf->c48[2 * t];
    }
    s2[7 + 8 * lane + 2 * u] = o0;
    s2[7 + 8 * lane + 2 * u + 1] = o1;
  }
}

// x4, 32 taps, 8 per phase, the four outputs of one n: out[4 n + j - 1] = sum_t state[n + t] c[(4 - j) + 4 t]
__device__ __forceinline__ void interp4_point(const float *s2, int n, CoefPtr cf, float (&o)[4]) {
#pragma clang fp contract(off)
  o[0] = o[1] = o[2] = o[3] = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const float x = s2[n + t];
    o[0] += x * cf->c192[3 + 4 * t];
    o[1] += x * cf->c192[2 + 4 * t];
    o[2] += x * cf->c192[1 + 4 * t];
    o[3] += x * cf->c192[4 * t];
  }
}

// The stored-tone exciter: CW_ExciterIQData() (CW_Excite.cpp:66-118; KEYED, X20) and the transmit half of
// ProcessIQData2() (Process2.cpp:309-349; neither), the SSB exciter's back half fed from a 256-sample tone table instead of
// the microphone.  Per frame a channel reads 16 gate bytes (KEYED) and writes 8 KiB.
//   tone_cos / tone_sin x level                      CW_Excite.cpp:69-70    Process2.cpp:313-314   arm_scale_f32
//   TX IQ amplitude / phase correction               :77-87                 :317-325     IQPhaseCorrection Utility.cpp:178-187
//   x2, 48 taps; x4, 32 taps, per channel            :93-100                :327-334
//   x 20 (X20), arm_float_to_q15                     :103-114               :344-345
//   the key (KEYED): modeSelectOutExL/R gain 0 / on  T41_SDR.ino:1193-1289, per 128-sample audio block, after the q15
// Args is TxCwArgs or TxCalArgs; level, i_scale, iq_phase and the gate come from the kernel around this body.
//
// The frame loop.  A frame's 256 input samples are the same in every frame and depend on nothing that changes inside a
// call, so they are computed once and written once behind the x2 delay line's history.  Both interpolators are FIRs: after
// one frame every delay line holds samples that came from that input alone (the x2 line's last 23 inputs; the x4 line's
// last 7 x2 outputs, which reach back 4 + 23 inputs), whatever the call started from.  So the memories are final after the
// call's first frame, the second frame's samples no longer depend on the call's initial state, and every later frame
// repeats the second bit for bit.  Frames 0 and 1 are computed, frame 1 is kept as packed q15 in 32 VGPRs per lane, and
// from frame 2 on only the gate is applied and the frame stored: the arithmetic of a call is constant and its cost is the
// 8 KiB per frame of stores, 16 bytes per lane and instruction.
template <bool KEYED, bool X20, class Args>
__device__ __forceinline__ void tone_exciter(const Args &a, float *il, float level, float i_scale, float iq_phase, const uint8_t *key) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int ch = blockIdx.x;
  float *st = a.state + (size_t)ch * kTxDelayFloats;
  const CoefPtr cf = (CoefPtr)a.coef;
  if (KEYED && key) key += (size_t)ch * a.nframes * kTxCwKeyPerFrame;

  interp_load(il, st, lane);
  // ---- the frame's input, samples 4 lane .. 4 lane + 3, once per call
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float I = a.tone_cos[4 * lane + j] * level;
    float Q = a.tone_sin[4 * lane + j] * level;
    if (a.corr_on) {
      I = I * i_scale;
      if (iq_phase < 0.0f) Q = Q + I * iq_phase;
      else I = I + Q * iq_phase;
    }
    il[23 + 4 * lane + j] = I;
    il[kInt1Pitch + 23 + 4 * lane + j] = Q;
  }
  wave_sync();

  // a frame as packed q15: keep[c][v] holds samples 8 lane + 512 v .. + 7 of side c, all of audio block 4 v + lane / 16
  uint4 keep[2][4];
  unsigned kb = (KEYED && key) ? key[lane & 15] : 1u;
  for (int f = 0; f < a.nframes; ++f) {
    // the frame's 16 gate bytes sit in lanes 0 .. 15; the next frame's are fetched ahead of this frame's stores
    unsigned gate = ~0u;
    if (KEYED) {
      gate = (unsigned)__ballot(kb != 0);
      if (key && f + 1 < a.nframes) kb = key[(size_t)(f + 1) * kTxCwKeyPerFrame + (lane & 15)];
    }
    if (f < 2) {
      // ---- x2 then x4, I then Q
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float *s2 = il + kInt2At + kInt2Pitch * c;
        interp2_block(il + kInt1Pitch * c, s2, cf, lane);
        wave_sync();
        // n = 2 lane + e + 128 v: 16 bytes per lane and v
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          unsigned p[4];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            float o[4];
            interp4_point(s2, 2 * lane + e + 128 * v, cf, o);
            if (X20) {
#pragma unroll
              for (int k = 0; k < 4; ++k) o[k] = o[k] * 20.0f;
            }
            p[2 * e] = q15_pack2(o[0], o[1]);
            p[2 * e + 1] = q15_pack2(o[2], o[3]);
          }
          keep[c][v] = make_uint4(p[0], p[1], p[2], p[3]);
        }
      }
      // ---- roll the delay lines (the x2 lines' new part stays)
      wave_sync();
      const InterpTails t = interp_tails(il, lane);
      wave_sync();
      interp_heads(il, t, lane);
      wave_sync();
    }
    // ---- the key, then the frame to HBM: a gated block is written as zeros
    const size_t base = ((size_t)ch * a.nframes + f) * 2048;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int16_t *out = (c ? a.outR : a.outL) + base;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const bool on = (gate >> (4 * v + (lane >> 4))) & 1u;
        *reinterpret_cast<uint4 *>(out + 8 * lane + 512 * v) = on ? keep[c][v] : make_uint4(0u, 0u, 0u, 0u);
      }
    }
  }
  interp_store(st, il, lane);
}

}  // namespace t41
