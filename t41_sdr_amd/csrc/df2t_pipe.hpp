// t41_sdr_amd/csrc/df2t_pipe.hpp -- the biquad pipeline of the receive equalizer (eq_kernel.hip), the transmit equaliser
// (tx_kernels.hip, tx_kernel<true>) and the CW narrow filter (cw_kernel.hip, cw_filter_kernel): cascades of
// arm_biquad_cascade_df2T_f32 sections, one section per lane.  Device code only; product code: nothing from oracle/.
//
// THE STEP.  A section {b0, b1, b2, a1, a2} (CMSIS DF2T, the a's negated) with its memories d1, d2 forms
//   acc = b0*x + d1;  d1 = b1*x + d2;  d1 += a1*acc;  d2 = b2*x;  d2 += a2*acc
// with one rounding per multiply and per add, in that order, as the firmware's CMSIS-DSP build does: no contraction
// (the pragma below; the translation units are compiled without it too).  The filters' poles sit at |z| ~ 0.98 .. 0.99,
// so a contracted or reordered recurrence does not stay within a few ulp, it drifts; with this step the kernels are the
// f32 restatements (tests/df2t_model.py) bit for bit.  This file is the only place the recurrence is written.
//
// THE PIPELINE.  A cascade of S sections occupies S neighbouring lanes, stage s on the s-th of them; the coefficients and
// the two memories stay in VGPRs for the whole call.  At step T stage 0 takes input sample T, and stage s > 0 takes what
// stage s - 1 produced at step T - 1 by one DPP move (control word DPP: a quad_perm for 4 stages, a row shift for more):
// stage s works on sample T - s.  The first S - 1 steps fill the pipeline (stage s idles until step s) and S - 1 more
// steps behind the last sample drain it (stage s runs on through step n - 1 + s); these are the only steps with a
// per-lane guard, `valid`, under which the step still computes but leaves d1, d2 alone.  A kernel whose stream is
// continuous over the call fills and drains once per launch; one that needs whole blocks does so once per block.
//
// THE RING.  Stage S - 1 yields sample u = T - (S - 1).  Its lane keeps the last four in registers, slot u & 3, and when
// slot 3 arrives stores samples u - 3 .. u, 4-aligned, with one b128 store into its cascade's row of an LDS ring of
// kRing = 2 kChunk samples: the chunk the consumer reads and the chunk being filtered.  Steps are counted as chunk c,
// position j (T = kChunk c + j, j a compile-time constant in the unrolled loops; the drain is j = kChunk .. of the last
// chunk), so the slot is (j - (S - 1)) & 3 and the store goes to (kChunk c + j - (S + 2)) & (kRing - 1).  Rows lie
// kRowPitch = kRing + 4 floats apart, 4 banks, so the rows' b128 stores do not conflict.  Chunk k of the ring is complete
// once chunk k + 1's steps (or the drain) are done.  While j < S + 2 in chunk 0, slot 3 arrives before a whole group of
// the stream has: that store lands in the ring's last groups, which are written again before anything reads them.  The
// equalizers let it happen; the CW filter skips it (Guard).
#pragma once
#include <hip/hip_runtime.h>

namespace t41 {
namespace df2t {

constexpr int kChunk = 64;             // samples per input chunk / per pass over the ring
constexpr int kRing = 2 * kChunk;      // ring: the chunk being consumed and the one being filtered
constexpr int kRowPitch = kRing + 4;   // (4 banks apart per row: the rows' b128 stores do not conflict)
constexpr int kQuadFromPrev = 0 | (0 << 2) | (1 << 4) | (2 << 6);  // quad_perm [0, 0, 1, 2]: stage s reads stage s - 1
constexpr int kBands = 14;             // the equalizers' bands (sum_bands)

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

// the hand-over between stages: the value of the lane the DPP control word names
template <int DPP>
__device__ __forceinline__ float from_lane(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), DPP, 0xf, 0xf, false));
}

// One lane of a pipeline of S stages.  Scaled: the last stage's output times `level` goes to the ring (the equalizers'
// arm_scale_f32).  Guard: no store before the stream's first group (see THE RING).
template <int S, int DPP, bool Scaled, bool Guard>
struct Pipe {
  Section q{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float level = 0.0f;                                 // Scaled: the cascade's signed level
  float acc = 0.0f;                                   // this stage's output of the step before
  float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;   // last stage: output samples u with u & 3 = 0 .. 3
  bool head = false, tail = false;                    // stage 0; stage S - 1 of a live cascade
  float *row = nullptr;                               // the cascade's ring row (16-byte aligned)

  // one step at chunk c, position j, on input sample `in` (read by the head)
  __device__ __forceinline__ void run(float in, int j, int c, bool valid) {
#pragma clang fp contract(off)
    const float prev = from_lane<DPP>(acc);
    acc = step(q, head ? in : prev, valid);
    const float y = Scaled ? acc * level : acc;
    switch ((j - (S - 1)) & 3) {
      case 0: r0 = y; break;
      case 1: r1 = y; break;
      case 2: r2 = y; break;
      default:
        r3 = y;
        if (tail && (!Guard || c > 0 || j >= S + 2)) {
          const int u0 = (kChunk * c + j - (S + 2)) & (kRing - 1);
          *reinterpret_cast<float4 *>(row + u0) = make_float4(r0, r1, r2, r3);
        }
    }
  }
};

// one sample's kBands scaled band outputs, `col` in ring row 0: EQ1 + EQ2, then + EQ3, .., + EQ14 (arm_add_f32's order)
__device__ __forceinline__ float sum_bands(const float *col) {
  float s = col[0] + col[kRowPitch];
#pragma unroll
  for (int b = 2; b < kBands; ++b) s += col[b * kRowPitch];
  return s;
}

}  // namespace df2t
}  // namespace t41
