// t41_sdr_amd/csrc/eq_kernel.hip -- gfx950 kernel of the receive equalizer (receiveEQFlag; DoReceiveEQ(),
// Filter.cpp:117-165, call site Process.cpp:828-832).  Off in the firmware's defaults; FFT_LENGTH 512.
//
// It runs on the call's demodulated audio @24 kS/s in the scratch the fused kernel leaves behind
// ([channel][frame * 256]), in place, before the noise reduction / notch (nr_kernels.hip), the noise blanker
// (nb_kernel.hip) and the back kernel's interpolators (launch_back512).
//
// A translation unit of its own (eq_kernel.o), compiled without contraction like the host designer (the kernel also turns
// contraction off by pragma); rx_audio.cpp is its host side and sees it through eq_kernels.hpp.
//
// The stage: 14 bands of 4 cascaded arm_biquad_cascade_df2T_f32 sections on the same input, each band's output times
// its signed level, and the 14 products summed as EQ1 + EQ2, then + EQ3, .., + EQ14, every value by the reference's
// operations in the reference's order: the output is the f32 restatement's (tests/eq_model.py) bit for bit.  The step,
// the pipeline, the ring and the sum are df2t_pipe.hpp's.
//
// ONE WAVE PER CHANNEL, one section per lane: lane 4 * band + stage (56 of 64 lanes; a band is one DPP quad).  The
// 4-deep pipeline runs through all frames of the call, so its fill and drain (3 steps each) are paid once per launch.
// Stage-3 lanes store their band's scaled output into a 14-row ring; once a chunk is complete, every lane sums one
// sample's 14 band values and stores it back, coalesced.  The input arrives in 64-sample chunks (one coalesced load,
// prefetched a chunk ahead) through a 64-float LDS buffer every lane reads by broadcast.
#include <hip/hip_runtime.h>

#include "df2t_pipe.hpp"
#include "eq_kernels.hpp"

namespace t41 {

static_assert(kEqBands == df2t::kBands, "df2t::sum_bands sums the equalizer's bands");

__global__ __launch_bounds__(64) void eq_kernel(EqArgs a) {
#pragma clang fp contract(off)
  using namespace df2t;
  __shared__ __attribute__((aligned(16))) float xin[kChunk];
  __shared__ __attribute__((aligned(16))) float ring[kEqBands * kRowPitch];
  const int lane = threadIdx.x;
  const int band = lane >> 2, stage = lane & 3;
  const bool live = lane < kEqSections;
  float *st = a.state + (size_t)blockIdx.x * kEqStateFloats;
  float *x = a.aud + (size_t)blockIdx.x * a.nsamp;
  const int nchunk = a.nsamp / kChunk;

  Pipe<kEqStages, kQuadFromPrev, true, false> p;
  p.head = stage == 0;
  p.tail = live && stage == kEqStages - 1;
  if (live) {
    const float *c = a.coef + 5 * lane;
    p.q = Section{c[0], c[1], c[2], c[3], c[4], st[2 * lane], st[2 * lane + 1]};
    p.level = a.scale[band];
  }
  p.row = ring + (live ? band : 0) * kRowPitch;
  // samples 64 k .. 64 k + 63 through the sum and back
  auto sum_chunk = [&](int k) { x[(size_t)k * kChunk + lane] = sum_bands(ring + (k & 1) * kChunk + lane); };

  float nxt = x[lane];
  for (int c = 0; c < nchunk; ++c) {
    xin[lane] = nxt;
    if (c + 1 < nchunk) nxt = x[(size_t)(c + 1) * kChunk + lane];
    __syncthreads();
    if (c == 0) {  // the pipeline fills: stage s starts at step s
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(xin + j);
        p.run(v.x, j, 0, j >= stage);
        p.run(v.y, j + 1, 0, j + 1 >= stage);
        p.run(v.z, j + 2, 0, j + 2 >= stage);
        p.run(v.w, j + 3, 0, true);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(xin + j);
        p.run(v.x, j, c, true);
        p.run(v.y, j + 1, c, true);
        p.run(v.z, j + 2, c, true);
        p.run(v.w, j + 3, c, true);
      }
    }
    __syncthreads();
    if (c > 0) sum_chunk(c - 1);
  }
  // the pipeline drains: step 64 n + d runs stages d + 1 .. 3 on the last samples
  p.run(0.0f, kChunk + 0, nchunk - 1, stage > 0);
  p.run(0.0f, kChunk + 1, nchunk - 1, stage > 1);
  p.run(0.0f, kChunk + 2, nchunk - 1, stage > 2);
  __syncthreads();
  sum_chunk(nchunk - 1);
  if (live) {
    st[2 * lane] = p.q.d1;
    st[2 * lane + 1] = p.q.d2;
  }
}

hipError_t launch_eq(const EqArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nsamp <= 0 || a.nsamp % df2t::kChunk) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(eq_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
