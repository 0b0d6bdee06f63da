// t41_sdr_amd/csrc/rx512_launch.hpp -- the one launcher of rx512_kernel (grid and block from the kernel's own geometry)
// and the rules that pick the instantiation for an FFT_LENGTH 512 call; included by the translation units that
// instantiate the kernel (one per demodulator family, and rx_long.hip).
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
template <int MODE, bool DEBUG, int PART, bool PLAIN, bool AGC, bool WQ15, bool SEGPAR = false, bool PIPE = false, bool MAP = false, bool SET = false,
          bool A24 = false>
static hipError_t launch_rx512(const RxArgs &a, hipStream_t s) {
  static_assert(!SET || MAP, "the set form exists as a twin of the mapped form only");
  static_assert(!A24 || MAP, "the 24 kS/s form exists as a twin of the mapped forms only");
  constexpr size_t NW = Rx512Geo<MODE, PART, AGC, PIPE>::kWaves;
  const size_t runs = SEGPAR ? (size_t)((a.nframes + a.seg_run - 1) / a.seg_run) : 1;
  const size_t jobs = (size_t)a.nchan * runs;
  hipLaunchKernelGGL((rx512_kernel<MODE, DEBUG, PART + (MAP ? kPartMap : 0) + (SET ? kPartSet : 0) + (A24 ? kPartA24 : 0), PLAIN, AGC, WQ15, SEGPAR, PIPE>),
                     dim3((unsigned)((jobs + NW - 1) / NW)), dim3(NW * 64), 0, s, a);
  return hipGetLastError();
}

// FFT_LENGTH 512, the whole chain in one kernel (PART 0).  `debug`: side outputs / stage taps.  `a24`: the audio leaves
// @24 kS/s -- a.out's strides count 256 samples per frame; with `debug` the host has set a.aud_out and finishes the call
// itself (launch_aud24_finish), without it the call takes the 24 kS/s twin of its mapped form and carries a map.
template <int MODE>
static hipError_t launch512(const RxArgs &a, hipStream_t s, bool debug, bool a24) {
  constexpr bool SAM = MODE == kModeSam;
  // the side outputs / stage taps and the synchronous detector run on the general front end
  const bool plain = a.plain && !debug && !SAM;
  // the pipelined variants (agc_prep_pipe, sam_chain_pipe, PSA): calls of four frames or more without taps; shorter
  // calls have nothing to overlap and take the barrier form, which computes the same values
  const bool pipe = (a.agc || SAM) && a.agc_pipe && !debug && a.nframes >= 4;
  // an input map changes none of the rules above: a mapped call takes the instantiation the same call would take without
  // the map, in its mapped form, and a call without a map never reaches a mapped one.  Parameter sets likewise: the
  // host has made sure that every set answers the rules above alike (t41rx_param_sets_compatible) and passes an input
  // map with them, so the call takes the set twin of the mapped instantiation; a call without sets never reaches one
  if (a.set_of != nullptr && (a.in_map == nullptr || a.set_gain == nullptr)) return hipErrorInvalidValue;
  // the 24 kS/s rate likewise: the twin of the mapped instantiation the call would take @192 kS/s (an identity map from the
  // host when the caller set none); the tap kernels hand the audio over instead (a.aud_out) and have no such twin
  const bool fused24 = a24 && !debug;
  if ((fused24 && a.in_map == nullptr) || (a24 && debug && a.aud_out == nullptr)) return hipErrorInvalidValue;
  return with_bools(
      [&](auto DBG, auto PLN, auto AGC, auto Q15, auto PIPE, auto MAP, auto SET, auto A24) {
        // what the rules above never select is not compiled
        if constexpr ((DBG && (PLN || PIPE)) || (PLN && SAM) || (PIPE && !(AGC || SAM)) || (SET && !MAP) || (A24 && (!MAP || DBG))) return hipErrorInvalidValue;
        else return launch_rx512<MODE, DBG, 0, PLN, AGC, Q15, false, PIPE, MAP, SET, A24>(a, s);
      },
      debug, plain, a.agc != 0, a.q15 != 0, pipe, a.in_map != nullptr, a.set_of != nullptr, fused24);
}

}  // namespace t41
