// t41_sdr_amd/csrc/rx_dispatch.hip -- launch_rx(): which kernel family runs a call.  No kernel is instantiated here.
#include "rx_experiments.hpp"
#include "rx_launch.hpp"
#include "t41rx.h"

namespace t41 {

// what this library's kernel translation units were built as (rx_experiments.hpp): 0 = the product.  Every object
// answers for itself, so one diagnostic object among product ones is seen
int kernel_build_flags() {
  return kKernelBuildFlags | build_flags_rx512_ssb() | build_flags_rx512_am() | build_flags_rx512_nfm() | build_flags_rx512_sam() |
         build_flags_rx_long() | build_flags_fastconv() | build_flags_display_kernel() | build_flags_cal_kernel();
}

// FFT_LENGTH 512 R (R = 2, 4, 8): front half (R segments per frame) -> N-point fast convolution -> back half
static hipError_t launch_long(const RxArgs &a, const CallPlan &p, hipStream_t s) {
  if (p.one_kernel) return launch_fastconv_fused(a, p.form, s);
  hipError_t e = launch_long_front(a, p.form, s);
  if (e != hipSuccess) return e;
  e = launch_fastconv(a, p.cplx, p.fused_back, s);
  if (e != hipSuccess || p.fused_back) return e;
  return launch_long_back(a, p.form, s);
}

hipError_t launch_rx(const RxArgs &a, const CallPlan &p, hipStream_t s) {
  if (!p.valid || a.seg != p.seg) return hipErrorInvalidValue;
  if (p.seg > 1) return launch_long(a, p, s);
  // the one guard: the plan and the arguments agree on the tap kernels (side outputs and the hand-over ride on them).
  // rx_args() fills the pointers from the same plan, so this is not reached
  const bool debug = a.dbg_nco || a.dbg_dec || a.dbg_demod || a.spect || a.dbg_pre || a.aud_out;
  if (debug != p.form.taps) return hipErrorInvalidValue;
  switch (p.form.family) {
    case Family::ssb: return launch512_ssb(a, p.form, s);
    case Family::am: return launch512_am(a, p.form, s);
    case Family::nfm: return launch512_nfm(a, p.form, s);
    case Family::sam: return launch512_sam(a, p.form, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace t41
