// t41_sdr_amd/csrc/tx_cal_kernel.hip -- gfx950 kernel of the transmit half of the IQ calibration, ProcessIQData2()
// (Process2.cpp:309-349): tx_cw_kernel's sibling, the same interpolators fed from the 3 kHz tone.
//
// One 64-lane wave = one channel, all the frames of a call, the four interpolator delay lines (FIR_int1_EX_I/Q,
// FIR_int2_EX_I/Q: the SSB exciter's own instances) in the wave's LDS, as in tx_cw_kernel.hip, behind which this file is
// compiled as part of tx_host.cpp and whose helpers (wave_sync, lds4, q15_pack2, the LDS layout) it uses.
//   cosBuffer3 / sinBuffer3 x bandOutputFactor       Process2.cpp:313-314
//   TX IQ amplitude / phase correction, per channel  :317-325    LSB: I x -IQXAmp, USB: I x +IQXAmp, IQPhaseCorrection()
//   x2, 48 taps; x4, 32 taps, per channel            :327-334
//   arm_float_to_q15                                 :344-345    no x 20 and no key
// Multiplies and adds are separate (no FMA contraction).  The two interpolator blocks are restated, not shared with
// tx_cw_kernel through a template: tx_cw_kernel keeps its instruction stream.
//
// The frame loop is tx_cw_kernel's: a frame's input is the same in every frame, both interpolators are FIRs, so the
// memories are final after the call's first frame and every frame from the third on repeats the second bit for bit.
// Frames 0 and 1 are computed, frame 1 is kept as packed q15 in 32 VGPRs per lane and stored again for every later frame.
#include <hip/hip_runtime.h>

#include "tx_internal.hpp"

namespace t41 {

__global__ __launch_bounds__(64) void tx_cal_kernel(const TxCalArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int lane = threadIdx.x;
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  float *st = a.state + (size_t)ch * kTxDelayFloats;
  const CoefPtr cf = (CoefPtr)a.coef;
  // the channel's candidate, or the params' factors
  const float amp = a.corr ? a.corr[2 * (size_t)ch] : a.iq_amp;
  const float iq_phase = a.corr ? a.corr[2 * (size_t)ch + 1] : a.iq_phase;
  const float i_scale = a.lsb ? -amp : amp;

  // ---- delay lines: HBM -> LDS, once per call
  if (lane < 23) {
    lds[kI1 + lane] = st[kTxStInt1I + lane];
    lds[kI1 + 280 + lane] = st[kTxStInt1Q + lane];
  }
  if (lane < 7) {
    lds[kI2 + lane] = st[kTxStInt2I + lane];
    lds[kI2 + 520 + lane] = st[kTxStInt2Q + lane];
  }
  // ---- the frame's input, samples 4 lane .. 4 lane + 3, once per call: arm_scale_f32 by bandOutputFactor
  // (Process2.cpp:313-314), then the TX IQ correction (:317-325; IQPhaseCorrection Utility.cpp:178-187)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float I = a.tone_cos[4 * lane + j] * a.level;
    float Q = a.tone_sin[4 * lane + j] * a.level;
    if (a.corr_on) {
      I = I * i_scale;
      if (iq_phase < 0.0f) Q = Q + I * iq_phase;
      else I = I + Q * iq_phase;
    }
    lds[kI1 + 23 + 4 * lane + j] = I;
    lds[kI1 + 280 + 23 + 4 * lane + j] = Q;
  }
  wave_sync();

  // a frame as packed q15: keep[c][v] holds samples 8 lane + 512 v .. + 7 of side c
  uint4 keep[2][4];
  for (int f = 0; f < a.nframes; ++f) {
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
            // arm_float_to_q15 straight from the interpolator (Process2.cpp:344-345)
            p[2 * e] = q15_pack2(o[0], o[1]);
            p[2 * e + 1] = q15_pack2(o[2], o[3]);
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
    // ---- the frame to HBM
    const size_t base = ((size_t)ch * a.nframes + f) * 2048;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int16_t *out = (c ? a.outR : a.outL) + base;
#pragma unroll
      for (int v = 0; v < 4; ++v) *reinterpret_cast<uint4 *>(out + 8 * lane + 512 * v) = keep[c][v];
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

hipError_t launch_tx_cal(const TxCalArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tx_cal_kernel, dim3(a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
