// t41_sdr_amd/csrc/tx_cw_kernel.hip -- gfx950 kernel of the T41 CW exciter, CW_ExciterIQData() (CW_Excite.cpp:66-118):
// the SSB exciter's back half (tx_kernels.hip) fed from a stored tone instead of the microphone.
//
// One 64-lane wave = one channel, all the frames of a call.  The four interpolator delay lines (FIR_int1_EX_I/Q,
// FIR_int2_EX_I/Q: the SSB exciter's own instances, so its state and checkpoint) live in the wave's LDS for the whole
// call, HBM state read once and written once.  Per frame a channel reads 16 gate bytes and writes 8 KiB.
//   cosBuffer2 / sinBuffer2 x 0.127                  CW_Excite.cpp:69-70
//   TX IQ amplitude / phase correction               :77-87      signs opposite to ExciterIQData()'s, no Q x 1.00
//   x2, 48 taps; x4, 32 taps, per channel            :93-100     polyphase (arm_fir_interpolate_f32), CMSIS tap order
//   x 20, arm_float_to_q15                           :103-114
//   the key: modeSelectOutExL/R gain 0 / on          T41_SDR.ino:1193-1289, per 128-sample audio block, after the q15
// Multiplies and adds are separate (no FMA contraction), as in tx_kernel.  The two interpolator blocks are restated
// here and not shared with tx_kernels.hip through a header, and the file is compiled as part of tx_host.cpp: tx_kernels.o,
// and with it tx_kernel<false> and tx_kernel<true>, is untouched.
//
// The frame loop.  A frame's 256 input samples are the same in every frame and depend on nothing that changes inside a
// call, so they are computed once, into registers, and written once behind the x2 delay line's history.  Both
// interpolators are FIRs: after one frame every delay line holds samples that came from that input alone (the x2
// line's last 23 inputs; the x4 line's last 7 x2 outputs, which reach back 4 + 23 inputs), whatever the call started
// from.  So the memories are final after the call's first frame, the second frame's samples no longer depend on the
// call's initial state, and every later frame repeats the second bit for bit.  The kernel computes frames 0 and 1,
// keeps frame 1 as packed q15 in 32 VGPRs per lane, and from frame 2 on only applies the gate and stores: the
// arithmetic of a call is constant and its cost is the 8 KiB per frame of stores, 16 bytes per lane and instruction.
#include <hip/hip_runtime.h>

#include "tx_internal.hpp"

namespace t41 {

namespace {

__device__ __forceinline__ void wave_sync() {
  // one wave per workgroup: LDS executes its instructions in order; only the compiler must not reorder
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ float4 lds4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
typedef const __attribute__((address_space(4))) TxCoef *CoefPtr;

// (q15_t)__SSAT((q31_t)(x * 32768.0f), 16): CMSIS-DSP's arm_float_to_q15 without ARM_MATH_ROUNDING
__device__ __forceinline__ unsigned q15_pack2(float x0, float x1) {
  int a = (int)(x0 * 32768.0f), b = (int)(x1 * 32768.0f);
  a = a < -32768 ? -32768 : (a > 32767 ? 32767 : a);
  b = b < -32768 ? -32768 : (b > 32767 ? 32767 : b);
  return ((unsigned)a & 0xffffu) | ((unsigned)b << 16);
}

// LDS layout of the wave (floats): [history | new] per delay line, as tx_kernel's
constexpr int kI1 = 0;              // [2][23 + 256 (+1)]
constexpr int kI2 = kI1 + 2 * 280;  // [2][7 + 512 (+1)]
constexpr int kLdsFloats = kI2 + 2 * 520;

}  // namespace

__global__ __launch_bounds__(64) void tx_cw_kernel(const TxCwArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int lane = threadIdx.x;
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  float *st = a.state + (size_t)ch * kTxDelayFloats;
  const CoefPtr cf = (CoefPtr)a.coef;
  const uint8_t *key = a.key ? a.key + (size_t)ch * a.nframes * kTxCwKeyPerFrame : nullptr;

  // ---- delay lines: HBM -> LDS, once per call
  if (lane < 23) {
    lds[kI1 + lane] = st[kTxStInt1I + lane];
    lds[kI1 + 280 + lane] = st[kTxStInt1Q + lane];
  }
  if (lane < 7) {
    lds[kI2 + lane] = st[kTxStInt2I + lane];
    lds[kI2 + 520 + lane] = st[kTxStInt2Q + lane];
  }
  // ---- the frame's input, samples 4 lane .. 4 lane + 3, once per call: arm_scale_f32 by (float)0.127
  // (CW_Excite.cpp:69-70), then the TX IQ correction (:77-87; IQPhaseCorrection Utility.cpp:178-187)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float I = a.tone_cos[4 * lane + j] * 0.127f;
    float Q = a.tone_sin[4 * lane + j] * 0.127f;
    if (a.corr_on) {
      I = I * a.i_scale;
      if (a.iq_phase < 0.0f) Q = Q + I * a.iq_phase;
      else I = I + Q * a.iq_phase;
    }
    lds[kI1 + 23 + 4 * lane + j] = I;
    lds[kI1 + 280 + 23 + 4 * lane + j] = Q;
  }
  wave_sync();

  // a frame as packed q15: keep[c][v] holds samples 8 lane + 512 v .. + 7 of side c, all of audio block 4 v + lane / 16
  uint4 keep[2][4];
  unsigned kb = key ? key[lane & 15] : 1u;
  for (int f = 0; f < a.nframes; ++f) {
    // the frame's 16 gate bytes sit in lanes 0 .. 15; the next frame's are fetched ahead of this frame's stores
    const unsigned gate = (unsigned)__ballot(kb != 0);
    if (key && f + 1 < a.nframes) kb = key[(size_t)(f + 1) * kTxCwKeyPerFrame + (lane & 15)];
    if (f < 2) {
      // ---- x2 (48 taps, 24 per phase) then x4 (32 taps, 8 per phase), I then Q
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float *s1 = lds + kI1 + 280 * c, *s2 = lds + kI2 + 520 * c;
        {
          // out[2 n + j - 1] = sum_t state[n + t] c[(2 - j) + 2 t], n = 4 lane + u
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
        wave_sync();
        // out[4 n + j - 1] = sum_t state[n + t] c[(4 - j) + 4 t], n = 2 lane + e + 128 v: 16 bytes per lane and v
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          unsigned p[4];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int n = 2 * lane + e + 128 * v;
            float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              const float x = s2[n + t];
              o[0] += x * cf->c192[3 + 4 * t];
              o[1] += x * cf->c192[2 + 4 * t];
              o[2] += x * cf->c192[1 + 4 * t];
              o[3] += x * cf->c192[4 * t];
            }
            // x 20 (CW_Excite.cpp:103-104), arm_float_to_q15 (:113-114)
            p[2 * e] = q15_pack2(o[0] * 20.0f, o[1] * 20.0f);
            p[2 * e + 1] = q15_pack2(o[2] * 20.0f, o[3] * 20.0f);
          }
          keep[c][v] = make_uint4(p[0], p[1], p[2], p[3]);
        }
      }
      // ---- roll the delay lines: the last numTaps - 1 samples move to the front (the x2 lines' new part stays)
      wave_sync();
      {
        const float i1a = (lane < 23) ? lds[kI1 + 256 + lane] : 0.0f, i1b = (lane < 23) ? lds[kI1 + 280 + 256 + lane] : 0.0f;
        const float i2a = (lane < 7) ? lds[kI2 + 512 + lane] : 0.0f, i2b = (lane < 7) ? lds[kI2 + 520 + 512 + lane] : 0.0f;
        wave_sync();
        if (lane < 23) {
          lds[kI1 + lane] = i1a;
          lds[kI1 + 280 + lane] = i1b;
        }
        if (lane < 7) {
          lds[kI2 + lane] = i2a;
          lds[kI2 + 520 + lane] = i2b;
        }
      }
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
  // ---- delay lines back to HBM
  if (lane < 23) {
    st[kTxStInt1I + lane] = lds[kI1 + lane];
    st[kTxStInt1Q + lane] = lds[kI1 + 280 + lane];
  }
  if (lane < 7) {
    st[kTxStInt2I + lane] = lds[kI2 + lane];
    st[kTxStInt2Q + lane] = lds[kI2 + 520 + lane];
  }
}

hipError_t launch_tx_cw(const TxCwArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tx_cw_kernel, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
