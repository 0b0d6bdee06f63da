// t41_sdr_amd/csrc/eq_kernel.hip -- gfx950 kernel of the receive equalizer (receiveEQFlag; DoReceiveEQ(),
// Filter.cpp:117-165, call site Process.cpp:828-832).  Off in the firmware's defaults; FFT_LENGTH 512.
//
// It runs on the call's demodulated audio @24 kS/s in the scratch the fused kernel leaves behind
// ([channel][frame * 256]), in place, before the noise reduction / notch (nr_kernels.hip), the noise blanker
// (nb_kernel.hip) and the back kernel's interpolators (launch_back512).
//
// Built into rx_host.o (included by rx_host.cpp, a HIP translation unit compiled without contraction; the kernel also
// turns contraction off by pragma), so the library's object set is unchanged.
//
// The stage: 14 bands of 4 cascaded arm_biquad_cascade_df2T_f32 sections on the same input, each band's output times
// its signed level, and the 14 products summed as EQ1 + EQ2, then + EQ3, .., + EQ14.  Every value is formed by the
// reference's operations in the reference's order (acc = b0*x + d1; d1 = b1*x + d2; d1 += a1*acc; d2 = b2*x;
// d2 += a2*acc; one rounding each, no contraction, no reassociation of the sum), so the output is the f32 restatement's
// (tests/eq_model.py) bit for bit.  The band filters' poles sit at |z| ~ 0.98: a reordered recurrence drifts.
//
// ONE WAVE PER CHANNEL, one biquad section per lane: lane 4 * band + stage (56 of 64 lanes; a band is one DPP quad).
// Every step, stage s takes stage s - 1's output of the step before by a quad_perm move and stage 0 takes the next
// input sample: a 4-deep pipeline that runs through all frames of the call, so its fill and drain (3 steps each, the
// only steps with a per-lane guard) are paid once per launch.  The section's coefficients and its two state words stay
// in VGPRs for the whole call.  Stage-3 lanes scale their band's output, gather 4 samples in registers and store them
// into a 14 x 128 LDS ring (two 64-sample chunks); once a chunk is complete, every lane sums one sample's 14 band values
// in the reference's order and stores it back, coalesced.  The input arrives in 64-sample chunks (one coalesced load,
// prefetched a chunk ahead) through a 64-float LDS buffer every lane reads by broadcast.
#include <hip/hip_runtime.h>

#include "eq_kernels.hpp"

namespace t41 {

namespace eq {
constexpr int kChunk = 64;               // samples per input chunk / per sum pass
constexpr int kRing = 2 * kChunk;        // band-output ring: the chunk being summed and the one being filtered
constexpr int kRowPitch = kRing + 4;     // (4 banks apart per band row: the 14 b128 stores do not conflict)
constexpr int kQuadFromPrev = 0 | (0 << 2) | (1 << 4) | (2 << 6);  // quad_perm [0, 0, 1, 2]: stage s reads stage s - 1

struct Section {
  float b0, b1, b2, a1, a2, d1, d2;
};

// one step of one section on its input xx; the state only changes where `valid` (the pipeline's fill / drain)
__device__ __forceinline__ float step(Section &q, float xx, bool valid) {
#pragma clang fp contract(off)
  const float acc = q.b0 * xx + q.d1;
  float d1 = q.b1 * xx + q.d2;
  d1 += q.a1 * acc;
  float d2 = q.b2 * xx;
  d2 += q.a2 * acc;
  q.d1 = valid ? d1 : q.d1;
  q.d2 = valid ? d2 : q.d2;
  return acc;
}

__device__ __forceinline__ float from_prev_stage(float acc) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, acc), kQuadFromPrev, 0xf, 0xf, false));
}
}  // namespace eq

__global__ __launch_bounds__(64) void eq_kernel(EqArgs a) {
#pragma clang fp contract(off)
  using namespace eq;
  __shared__ __attribute__((aligned(16))) float xin[kChunk];
  __shared__ __attribute__((aligned(16))) float ring[kEqBands * kRowPitch];
  const int lane = threadIdx.x;
  const int band = lane >> 2, stage = lane & 3;
  const bool live = lane < kEqSections;
  const bool head = stage == 0;
  const bool tail = live && stage == 3;
  float *st = a.state + (size_t)blockIdx.x * kEqStateFloats;
  float *x = a.aud + (size_t)blockIdx.x * a.nsamp;
  const int nchunk = a.nsamp / kChunk;

  Section q{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float sc = 0.0f;
  if (live) {
    const float *c = a.coef + 5 * lane;
    q = Section{c[0], c[1], c[2], c[3], c[4], st[2 * lane], st[2 * lane + 1]};
    sc = a.scale[band];
  }
  float *row = ring + (live ? band : 0) * kRowPitch;

  float acc = 0.0f;
  float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;  // stage 3: the band's scaled output, samples u with u & 3 = 0 .. 3
  // one step at chunk position j (global step T = 64 c + j, sample T - stage); stage 3 yields sample u = T - 3, and
  // every 4th step (j & 3 == 2) completes samples u - 3 .. u, 4-aligned, for the ring
  auto run = [&](float in, int j, int c, bool valid) {
    const float prev = from_prev_stage(acc);
    acc = step(q, head ? in : prev, valid);
    const float y = acc * sc;
    switch (j & 3) {
      case 3: r0 = y; break;
      case 0: r1 = y; break;
      case 1: r2 = y; break;
      default:
        r3 = y;
        if (tail) {
          const int u0 = (kChunk * c + j - 6) & (kRing - 1);
          *reinterpret_cast<float4 *>(row + u0) = make_float4(r0, r1, r2, r3);
        }
    }
  };
  // samples 64 k .. 64 k + 63 through the sum, in the reference's order, and back
  auto sum_chunk = [&](int k) {
    const float *col = ring + (k & 1) * kChunk + lane;
    float s = col[0] + col[kRowPitch];
#pragma unroll
    for (int b = 2; b < kEqBands; ++b) s += col[b * kRowPitch];
    x[(size_t)k * kChunk + lane] = s;
  };

  float nxt = x[lane];
  for (int c = 0; c < nchunk; ++c) {
    xin[lane] = nxt;
    if (c + 1 < nchunk) nxt = x[(size_t)(c + 1) * kChunk + lane];
    __syncthreads();
    if (c == 0) {  // the pipeline fills: stage s starts at step s
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(xin + j);
        run(v.x, j, 0, j >= stage);
        run(v.y, j + 1, 0, j + 1 >= stage);
        run(v.z, j + 2, 0, j + 2 >= stage);
        run(v.w, j + 3, 0, true);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(xin + j);
        run(v.x, j, c, true);
        run(v.y, j + 1, c, true);
        run(v.z, j + 2, c, true);
        run(v.w, j + 3, c, true);
      }
    }
    __syncthreads();
    if (c > 0) sum_chunk(c - 1);
  }
  // the pipeline drains: step 64 n + d runs stages d + 1 .. 3 on the last samples
  run(0.0f, kChunk + 0, nchunk - 1, stage > 0);
  run(0.0f, kChunk + 1, nchunk - 1, stage > 1);
  run(0.0f, kChunk + 2, nchunk - 1, stage > 2);
  __syncthreads();
  sum_chunk(nchunk - 1);
  if (live) {
    st[2 * lane] = q.d1;
    st[2 * lane + 1] = q.d2;
  }
}

hipError_t launch_eq(const EqArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nsamp <= 0 || a.nsamp % eq::kChunk) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(eq_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
