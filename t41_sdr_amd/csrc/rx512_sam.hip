// t41_sdr_amd/csrc/rx512_sam.hip -- the rx512_kernel<kModeSam, ...> instantiations: the synchronous detector (Demod.cpp:40-139)
// on the general front end; barrier form, pipelined PLL (AGC off) and the two-stage pipeline behind the AGC (PSA).
#include "rx512_launch.hpp"

namespace t41 {

hipError_t launch512_sam(const RxArgs &a, hipStream_t s, bool debug, bool a24) { return launch512<kModeSam>(a, s, debug, a24); }

T41RX_CLK_READER(t41rx_debug_read_clk_sam)
T41RX_BUILD_FLAGS(rx512_sam)

}  // namespace t41
