// t41_sdr_amd/csrc/rx512_am.hip -- the rx512_kernel<kModeAm, ...> instantiations (FFT_LENGTH 512, the whole chain fused).
#include "rx512_launch.hpp"

namespace t41 {

hipError_t launch512_am(const RxArgs &a, const KernelForm &k, hipStream_t s) { return launch512<kModeAm>(a, k, s); }

T41RX_CLK_READER(t41rx_debug_read_clk_am)
T41RX_BUILD_FLAGS(rx512_am)

}  // namespace t41
