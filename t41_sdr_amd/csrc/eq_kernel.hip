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

// LIST: the stage map's form (t41rx_set_stage_map).  The grid is the list's length and the wave takes its channel from the
// list, one scalar load; everything else is the kernel as it is without a map.
// LEVELS: the equalizer level map's forms (t41rx_set_receive_eq_map), plain and list: the band's level is the channel's own.
#define T41_STAGE_LEVELS 0
#define T41_STAGE_KERNEL eq_kernel
#define T41_STAGE_LIST 0
#include "eq_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL eq_list_kernel
#define T41_STAGE_LIST 1
#include "eq_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#undef T41_STAGE_LEVELS
#define T41_STAGE_LEVELS 1
#define T41_STAGE_KERNEL eq_levels_kernel
#define T41_STAGE_LIST 0
#include "eq_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL eq_levels_list_kernel
#define T41_STAGE_LIST 1
#include "eq_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#undef T41_STAGE_LEVELS

hipError_t launch_eq(const EqArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nsamp <= 0 || a.nsamp % df2t::kChunk || (a.list && a.nlist <= 0)) return hipErrorInvalidConfiguration;
  if (a.levels && a.list) hipLaunchKernelGGL(eq_levels_list_kernel, dim3((unsigned)a.nlist), dim3(64), 0, s, a);
  else if (a.levels) hipLaunchKernelGGL(eq_levels_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  else if (a.list) hipLaunchKernelGGL(eq_list_kernel, dim3((unsigned)a.nlist), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(eq_kernel, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
