// t41_sdr_amd/csrc/nb_kernel.hip -- gfx950 kernel of the receive noise blanker (NB_on; NoiseBlanker() /
// AltNoiseBlanking(), DSP_Fn.cpp:105-362, call site Process.cpp:873-876).  Off in the firmware's defaults;
// FFT_LENGTH 512.
//
// It runs on the call's demodulated audio @24 kS/s in the scratch the fused kernel leaves behind
// ([channel][frame * 256]), in place, after the noise reduction / notch (nr_kernels.hip) and before the back kernel's
// interpolators (launch_back512).
//
// A translation unit of its own (nb_kernel.o), compiled without contraction like the host designer (the kernel also turns
// contraction off by pragma); rx_audio.cpp is its host side and sees it through nb_kernels.hpp.
//
// Per 256-sample block: an order-10 LPC fit (autocorrelation, Levinson-Durbin), the prediction-error filter and its
// matched filter (two arm_fir_f32 from a zeroed state), a threshold from the filtered block's variance, a scan for
// samples above it, and for every detection 7 samples replaced by a weighted sum of forward and backward predictions.
// Every value is formed by the reference's operations in the reference's order (CMSIS-DSP's single f32 accumulator in
// tap order, arm_var_f32 two-pass around the mean, no contraction), so the blanker takes the f32 restatement's decisions
// and values (tests/nb_model.py).  IEEE comparisons and NaN propagation are kept: an all-zero block has alfa = 0 and NaN
// coefficients, a NaN threshold and no detection, exactly as in the reference.
//
// Given its input, a block does not depend on the blocks before it: the only memory, last_frame_end, is the previous
// block's INPUT x[242 .. 254] (repairs never reach past x[234]).  So ONE WAVE PER (channel, frame): frame f > 0 reads
// its carry straight from frame f - 1's samples in the scratch (this kernel writes samples 0 .. 239 only), frame 0 from
// the carry buffer slot `sel`, and the call's last frame writes slot sel ^ 1 -- ping-pong, as the long-FFT path's
// oscillator copies (nco_sel), so no wave waits for another.
//
// Lane-parallel: the two FIR passes (4 outputs per lane, each an 11-term sum in tap order) and the candidate test of the
// scan (a ballot per sample slot).  Serial, by order: the 11 autocorrelation sums (one lane per lag, 256 - lag terms
// each), the two passes of the variance, Levinson-Durbin, and the repairs (each impulse's forward seed may read samples
// an earlier impulse repaired).  Those serial sums bind the kernel ("Noise blanker").
#include <hip/hip_runtime.h>

#include "nb_kernels.hpp"

namespace t41 {

namespace nb {
constexpr int kOff = 12;                 // zeros in front of a block in LDS: the FIRs' zeroed state (10 used, 16-byte aligned)
constexpr int kRow = kOff + kNbBlock + 16;
}  // namespace nb
using nb::kOff;
using nb::kRow;

// LIST: the stage map's form (t41rx_set_stage_map).  The first nlist * nframes blocks are the kernel as it is without a
// map on channel list[blk / nframes].  The context's slot flips for every channel, so the blocks behind them carry the
// channels the list leaves out over: 4 channels per block, slot sel to slot sel ^ 1 of the same channel.  Nobody else
// touches a bypassed channel's slots, and slot sel is only ever read in this launch: no wave waits for another.
#define T41_STAGE_KERNEL nb_kernel
#define T41_STAGE_LIST 0
#include "nb_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL nb_list_kernel
#define T41_STAGE_LIST 1
#include "nb_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_LIST

hipError_t launch_nb(const NbArgs &a, hipStream_t s) {
  if (a.list && (a.nlist <= 0 || a.nrest < 0 || a.nlist + a.nrest != a.nchan || (a.nrest > 0 && !a.rest))) return hipErrorInvalidConfiguration;
  const long long blocks = a.list ? (long long)a.nlist * a.nframes + (a.nrest + 3) / 4 : (long long)a.nchan * a.nframes;
  if (a.nchan <= 0 || a.nframes <= 0 || blocks <= 0 || blocks * 64 > 0xffffffffll) return hipErrorInvalidConfiguration;
  if (a.list) hipLaunchKernelGGL(nb_list_kernel, dim3((unsigned)blocks), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(nb_kernel, dim3((unsigned)blocks), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
