// t41_sdr_amd/csrc/rx_long.hip -- the two ends of the long-FFT pipeline (FFT_LENGTH 1024 / 2048 / 4096): rx512_kernel<..., PART = 1>
// (loads .. /8 decimation -> `mid`) and <..., PART = 2> (`aud24` -> interpolators -> stores), a 2048-sample segment at a time;
// the N-point fast convolution between them is fastconv.hip.  launch_back512: the PART 2 kernel behind the noise-reduction
// stages at FFT_LENGTH 512.
#include "rx512_launch.hpp"

namespace t41 {

hipError_t launch_long_front(const RxArgs &a, const KernelForm &k, hipStream_t s) {
  if (k.family == Family::nfm)  // nfmdemod()'s "last sample" chains the frames: sequential, on the general front end
    return with_bools([&](auto Q15, auto MAP) { return launch_rx512<kModeNfm, false, 1, false, false, Q15, false, false, MAP>(a, s); },
                      k.q15, k.map_form);
  // everything else: one wave per (channel, run of segments), the segments run independently (SEGPAR).
  // An input map (receiver groups) selects the same instantiation in its mapped form; the back end reads no antenna samples.
  return with_bools(
      [&](auto PLN, auto Q15, auto MAP) {
        if constexpr (!long_front_compiled(PLN, Q15)) return hipErrorInvalidValue;  // never planned: not compiled
        else return launch_rx512<kModeSsb, false, 1, PLN, false, Q15, true, false, MAP>(a, s);
      },
      k.plain, k.q15, k.map_form);
}

// SSB / NFM audio with the fixed gain: the gain law and the demodulators keep no state here
template <bool Q15>
static hipError_t launch_back_par(const RxArgs &a, hipStream_t s) {
  return launch_rx512<kModeSsb, false, 2, false, false, Q15, true>(a, s);
}

hipError_t launch_long_back(const RxArgs &a, const KernelForm &k, hipStream_t s) {
  return with_bools(
      [&](auto AM, auto AGC, auto Q15) {
        if constexpr (AM || AGC) return launch_rx512<AM ? kModeAm : kModeSsb, false, 2, false, AGC, Q15>(a, s);  // sequential
        else return launch_back_par<Q15>(a, s);
      },
      k.family == Family::am, k.agc, k.q15);
}

hipError_t launch_back512(const RxArgs &a, hipStream_t s) {
  // the long-FFT pipeline's segment-parallel back kernel with one segment per frame: it takes its interpolator
  // memories from the channel's record and leaves the call's last ones there
  if (a.seg != 1 || !a.aud24) return hipErrorInvalidValue;
  // (q15: arm_float_to_q15 behind the volume, Process.cpp:936)
  // An output map (a.out_map): the same kernel in its output-map form, whose waves store to the channel's row or leave.
  // Only an output map brings a call with parameter sets here (the stages that split the chain refuse the sets): the
  // form's set twin then interpolates with the taps of the channel's own set, which carry its volume
  return with_bools(
      [&](auto Q15, auto OUT, auto SET) {
        if constexpr (OUT) return launch_rx512<kModeSsb, false, 2, false, false, Q15, true, false, false, SET, false, true>(a, s);
        else if constexpr (SET) return hipErrorInvalidValue;  // never planned: not compiled
        else return launch_back_par<Q15>(a, s);
      },
      a.q15 != 0, a.out_map != nullptr, a.set_of != nullptr);
}

T41RX_CLK_READER(t41rx_debug_read_clk_long)
T41RX_BUILD_FLAGS(rx_long)

}  // namespace t41
