// t41_sdr_amd/csrc/rx_launch.hpp -- the launchers of the kernel families, one translation unit each (rx_dispatch.hip picks).
#pragma once
#include <type_traits>

#include "rx_kernels.hpp"

namespace t41 {

// run-time booleans -> template arguments: with_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...).
// f is instantiated for every combination, so it takes the booleans of a plan (rx_plan.hpp: plan_call()) and leaves out,
// with `if constexpr` on form_compiled(), the combinations the plan never produces.
template <class F>
hipError_t with_bools(F &&f) {
  return f();
}
template <class F, class... Bools>
hipError_t with_bools(F &&f, bool b, Bools... rest) {
  auto bind = [&](auto B) { return with_bools([&](auto... bs) { return f(B, bs...); }, rest...); };
  return b ? bind(std::true_type{}) : bind(std::false_type{});
}

// FFT_LENGTH 512, the whole chain in rx512_kernel<MODE, ...> (rx512_ssb.hip / rx512_am.hip / rx512_nfm.hip / rx512_sam.hip)
hipError_t launch512_ssb(const RxArgs &a, const KernelForm &k, hipStream_t s);
hipError_t launch512_am(const RxArgs &a, const KernelForm &k, hipStream_t s);
hipError_t launch512_nfm(const RxArgs &a, const KernelForm &k, hipStream_t s);
hipError_t launch512_sam(const RxArgs &a, const KernelForm &k, hipStream_t s);
// FFT_LENGTH 1024 / 2048 / 4096: the two ends of the pipeline (rx_long.hip: rx512_kernel<..., PART = 1 / 2>) ...
hipError_t launch_long_front(const RxArgs &a, const KernelForm &k, hipStream_t s);
hipError_t launch_long_back(const RxArgs &a, const KernelForm &k, hipStream_t s);
// ... and the N-point fast convolution between them, or the one-kernel form (fastconv.hip)
hipError_t launch_fastconv(const RxArgs &a, bool cplx, bool fused_back, hipStream_t s);
hipError_t launch_fastconv_fused(const RxArgs &a, const KernelForm &k, hipStream_t s);

// what each kernel object was built as (rx_experiments.hpp: T41RX_BUILD_FLAGS), one function per object of the Makefile's
// RXK_OBJS; kernel_build_flags() (rx_dispatch.hip) is the OR of them and the dispatch unit's own
int build_flags_rx512_ssb();
int build_flags_rx512_am();
int build_flags_rx512_nfm();
int build_flags_rx512_sam();
int build_flags_rx_long();
int build_flags_fastconv();
int build_flags_display_kernel();
int build_flags_cal_kernel();

}  // namespace t41
