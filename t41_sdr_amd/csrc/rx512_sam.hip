// t41_sdr_amd/csrc/rx512_sam.hip -- the rx512_kernel<kModeSam, ...> instantiations: the synchronous detector (Demod.cpp:40-139)
// on the general front end; barrier form, pipelined PLL (AGC off) and the two-stage pipeline behind the AGC (PSA).
#include "rx512_launch.hpp"

namespace t41 {

hipError_t launch512_sam(const RxArgs &a, const KernelForm &k, hipStream_t s) { return launch512<kModeSam>(a, k, s); }

T41RX_CLK_READER(t41rx_debug_read_clk_sam)
T41RX_BUILD_FLAGS(rx512_sam)

}  // namespace t41
