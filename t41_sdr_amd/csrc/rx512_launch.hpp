// t41_sdr_amd/csrc/rx512_launch.hpp -- the one launcher of rx512_kernel (grid and block from the kernel's own geometry)
// and launch512(), which instantiates the form an FFT_LENGTH 512 call's plan names (the rules are rx_plan.hpp's);
// included by the translation units that instantiate the kernel (one per demodulator family, and rx_long.hip).
#pragma once
#include "rx512_kernel.hpp"
#include "rx_launch.hpp"

namespace t41 {

// The block is the kernel's __launch_bounds__ (Rx512Geo), the grid covers the kernel's `job`s, one per wave:
// a channel, or with SEGPAR a (channel, run of a.seg_run segments) pair.
// PART 0, AGC off: one 16-wave workgroup per CU (all 160 KiB of LDS, declared statically by the kernel) -- a
// 4096-channel batch is one full, balanced wave of work on 256 CUs, and every wave keeps its channel for all the
// frames of the launch.  Everything else: 4-wave workgroups (see Geo).
// MAP: the call carries an input map (RxArgs::in_map, receiver groups) -- the same instantiation in its mapped form
// (PART + kPartMap), same geometry.
// SET: the call carries parameter sets (RxArgs::set_of, t41rx_set_param_sets) -- the mapped form's twin that takes a
// channel's constants from its set (PART + kPartMap + kPartSet), same geometry.
// A24: the call's result is the audio @24 kS/s (t41rx_set_audio_rate) -- the mapped or set form's twin that stores behind
// the demodulator (+ kPartA24).  Same geometry: the parent's, 16 waves and all of the CU's LDS for the resident forms, so
// that what differs between a 24 kS/s launch and its 192 kS/s twin is the back end alone.
// OUT: the call carries an output map (RxArgs::out_map, t41rx_set_output_map) -- the twin of the mapped forms that stores
// to the channel's row or leaves the frame behind the demodulator (+ kPartOut), same geometry; also the form of the
// segment-parallel back kernel behind the hand-over (PART 2).
template <int MODE, bool DEBUG, int PART, bool PLAIN, bool AGC, bool WQ15, bool SEGPAR = false, bool PIPE = false, bool MAP = false, bool SET = false,
          bool A24 = false, bool OUT = false>
static hipError_t launch_rx512(const RxArgs &a, hipStream_t s) {
  static_assert(!SET || MAP || (PART == 2 && OUT), "the set form exists as a twin of the mapped form and of the back kernel's output-map form only");
  static_assert(!A24 || MAP, "the 24 kS/s form exists as a twin of the mapped forms only");
  static_assert(!OUT || MAP || PART == 2, "the output-map form exists as a twin of the mapped forms and of the back kernel only");
  constexpr size_t NW = Rx512Geo<MODE, PART, AGC, PIPE>::kWaves;
  const size_t runs = SEGPAR ? (size_t)((a.nframes + a.seg_run - 1) / a.seg_run) : 1;
  const size_t jobs = (size_t)a.nchan * runs;
  hipLaunchKernelGGL((rx512_kernel<MODE, DEBUG, PART + (MAP ? kPartMap : 0) + (SET ? kPartSet : 0) + (A24 ? kPartA24 : 0) + (OUT ? kPartOut : 0), PLAIN, AGC, WQ15, SEGPAR, PIPE>),
                     dim3((unsigned)((jobs + NW - 1) / NW)), dim3(NW * 64), 0, s, a);
  return hipGetLastError();
}

// FFT_LENGTH 512, the whole chain in one kernel (PART 0): the instantiation the call's plan names (rx_plan.hpp).
template <int MODE>
static hipError_t launch512(const RxArgs &a, const KernelForm &k, hipStream_t s) {
  return with_bools(
      [&](auto DBG, auto PLN, auto AGC, auto Q15, auto PIPE, auto MAP, auto SET, auto A24, auto OUT) {
        // what the plan never names is not compiled
        if constexpr (!form_compiled(MODE == kModeSam, DBG, PLN, AGC, PIPE, MAP, SET, A24, OUT)) return hipErrorInvalidValue;
        else return launch_rx512<MODE, DBG, 0, PLN, AGC, Q15, false, PIPE, MAP, SET, A24, OUT>(a, s);
      },
      k.taps, k.plain, k.agc, k.q15, k.pipe, k.map_form, k.set_form, k.a24_form, k.omap_form);
}

}  // namespace t41
