// t41_sdr_amd/csrc/rx_plan.hpp -- which kernels a t41rx_process_* call runs: plan_call(), the one owner of that decision.
// The process call states what it is (CallFacts), plan_call() answers (CallPlan), and everything that allocates, fills
// the kernels' arguments or launches reads the answer: rx_host.cpp (prepare_call, rx_args, launch_chain), the launchers
// (rx_dispatch.hip, rx512_launch.hpp, rx_long.hip, fastconv.hip), the FT8 and CW stages, and the parameter sets' rule
// (rx_sets.cpp).  Plain C++17: no HIP, no context type -- tests/call_plan_check.cpp walks every CallFacts on a CPU.
#pragma once

namespace t41 {

// the demodulator families, one rx512_kernel MODE each (rx_chains.hpp: kModeSsb ..; USB and LSB are one kernel)
enum class Family { ssb = 0, am = 1, nfm = 2, sam = 3 };

struct CallFacts {
  int seg = 1;  // fft_length / 512
  Family family = Family::ssb;
  bool agc = false, q15 = false, nfm_atan = false;
  bool plain_gains = false;  // what gains_of() returns: unit band / IQ gains
  int n_frames = 1;
  bool seg_run_set = false;  // T41RX_SEG_RUN at creation
  bool map = false, sets = false, a24 = false;  // the caller's input map, parameter sets loaded, audio at 24 kS/s
  // the stage taps and the side outputs; pan_rows: the panadapter has an update frame in this call
  bool tap_nco = false, tap_dec = false, tap_demod = false, spect = false, disp = false, pan_rows = false, ft8 = false;
  // the stages that split the chain behind the demodulator
  bool eq = false, nr = false, nb = false, cw_filter = false, cw_det = false;
  bool omap = false;  // the caller's output map (t41rx_set_output_map): audio rows for the listened channels only
  // the CW filter map (t41rx_set_cw_filter_map) is loaded and leaves some channel without the narrow filter (index 5).
  // cw_filter then says that some channel has it; a map that filters nobody is a call without the filter
  bool cw_unfiltered = false;
  // the parameter sets were loaded with T41RX_SETS_STAGES (t41rx_set_param_sets_ex): they run next to the chain-splitting
  // stages.  Read only where sets && stages
  bool stage_sets = false;
};

// an rx512_kernel instantiation of the whole chain (PART 0): two calls with equal forms launch the same kernel
struct KernelForm {
  Family family = Family::ssb;
  bool taps = false;   // DEBUG: the tap kernels -- side outputs, stage taps, the hand-over
  bool plain = false, agc = false, q15 = false;
  bool pipe = false;   // the pipelined AGC / SAM variants
  bool map_form = false, set_form = false, a24_form = false;  // the mapped form and its set and 24 kS/s twins
  bool omap_form = false;  // the output-map twin of the mapped forms: the wave stores to row out_map[ch], or to none
};
constexpr bool operator==(const KernelForm &x, const KernelForm &y) {
  return x.family == y.family && x.taps == y.taps && x.plain == y.plain && x.agc == y.agc && x.q15 == y.q15 && x.pipe == y.pipe &&
         x.map_form == y.map_form && x.set_form == y.set_form && x.a24_form == y.a24_form && x.omap_form == y.omap_form;
}

// is this form instantiated?  The launchers' `if constexpr` leaves out exactly what this refuses.
constexpr bool form_compiled(bool sam, bool taps, bool plain, bool agc, bool pipe, bool map_form, bool set_form, bool a24_form, bool omap_form = false) {
  return !((taps && (plain || pipe)) || (plain && sam) || (pipe && !(agc || sam)) || (set_form && !map_form) || (a24_form && (!map_form || taps)) ||
           (omap_form && (!map_form || taps)));
}
constexpr bool form_compiled(const KernelForm &k) {
  return form_compiled(k.family == Family::sam, k.taps, k.plain, k.agc, k.pipe, k.map_form, k.set_form, k.a24_form, k.omap_form);
}
// the long-FFT front end (PART 1): PLAIN is built for f32 samples only
constexpr bool long_front_compiled(bool plain, bool q15) { return !(plain && q15); }

// what writes the call's audio
enum class Back {
  fused,      // the stores of the fused kernel, 192 kS/s or 24 kS/s
  back512,    // launch_back512: interpolators, volume, stores
  cw_back,    // CW filter + cw_back_kernel
  cw_24k,     // CW filter + the 24 kS/s finish
  cw_mixed,   // CW filter map with both classes: cw_back_kernel for the filtered channels, launch_back512 for the others
  finish24,   // the 24 kS/s finish
  long_pipe,  // the long-FFT pipeline's own back end
};
enum class Ft8Source { none, handover, caller_tap, own_tap };  // where the FT8 stage reads the demodulated audio

struct CallPlan {
  bool valid = true;  // false: a combination the setters keep apart; no call reaches it
  const char *why = "";
  bool nfm_atan_long = false;  // the one invalid combination prepare_call() refuses with a text of its own
  int seg = 1;
  KernelForm form;
  bool handover = false;     // the kernel stops behind the demodulator and leaves the audio @24 kS/s in the scratch
  bool scratch = false;      // d_mid / d_aud24 are needed
  bool need_ident = false;   // a mapped form without a map of the caller's: the identity map
  bool pipe_buffer = false;  // the pipelined kernels' buffer exists from the first AGC / SAM call of >= 4 frames, taps or not
  // fft_length 1024 / 2048 / 4096: the one-kernel form, or front end + fast convolution (+ back end)
  bool one_kernel = false, cplx = false, fused_back = false;
  Back back = Back::fused;
  Ft8Source ft8_source = Ft8Source::none;
  // the FT8 stage's own demod tap is allocated and written.  (At 24 kS/s the stage reads the hand-over and the tap is
  // written all the same: the kernels' arguments are what they were before the plan.)
  bool ft8_own_tap = false;
};

constexpr CallPlan plan_call(const CallFacts &f) {
  CallPlan p;
  const bool lng = f.seg > 1, sam = f.family == Family::sam;
  const bool stages = f.eq || f.nr || f.nb || f.cw_filter || f.cw_det;
  const bool stage_taps = f.tap_nco || f.tap_dec || f.tap_demod;
  if (f.nfm_atan && lng) {
    p.valid = false;
    p.nfm_atan_long = true;
    p.why = "nfm_demod = 1 is built for fft_length 512";
  } else if (f.sets && (lng || (stages && !f.stage_sets))) {
    p.valid = false;
    p.why = "parameter sets are loaded with a long fft_length or a chain-splitting stage";
  } else if (lng && (f.a24 || stage_taps || stages)) {
    p.valid = false;
    p.why = "audio at 24 kS/s, the stage taps and the chain-splitting stages are built for fft_length 512";
  } else if (f.omap && lng) {
    p.valid = false;
    p.why = "the output map is built for fft_length 512";
  }
  p.seg = f.seg;
  // fft_length 512.  Everything that reads behind the demodulator rides on the tap kernels (the FT8 stage through a demod
  // tap or the hand-over); they hand the audio over when a stage follows or when it leaves @24 kS/s.  The long lengths have
  // neither (params_valid and the setters refuse the side outputs there).
  const bool taps = !lng && (stage_taps || f.spect || f.disp || f.pan_rows || f.ft8 || stages);
  // An output map on the tap kernels hands over as well: they have no output-map twins, the back kernels know the map
  p.handover = !lng && (stages || ((f.a24 || f.omap) && taps));
  p.scratch = lng || p.handover;
  // AGC on (with the synchronous detector behind it: PSA), or the synchronous detector alone, in calls of four frames or
  // more: shorter calls have nothing to overlap and take the barrier form, which computes the same values
  p.pipe_buffer = (f.agc || sam) && !lng && f.n_frames >= 4;
  KernelForm &k = p.form;
  k.family = f.family;
  k.taps = taps;
  k.agc = f.agc;
  k.q15 = f.q15;
  // PLAIN -- unit gains, the correction stage drops out.  512: the taps and the synchronous detector run on the general
  // front end.  Long: f32 samples only; NFM's sequential front end has no such form
  k.plain = f.plain_gains && (lng ? !f.q15 && f.family != Family::nfm : !taps && !sam);
  k.pipe = p.pipe_buffer && !taps;
  // a mapped call takes the instantiation the same call would take without the map, in its mapped form.  The set forms
  // and the fused 24 kS/s forms are twins of the mapped ones: without a map of the caller's they run with the identity
  k.a24_form = f.a24 && !taps && !lng;
  k.set_form = f.sets && !lng;
  // ... and so is the output-map form: the fused kernel without taps places its stores by the map, or leaves the frame
  // behind the demodulator for a muted channel
  k.omap_form = f.omap && !taps && !lng;
  k.map_form = f.map || k.set_form || k.a24_form || k.omap_form;
  p.need_ident = k.map_form && !f.map;
  if (lng) {
    // 4096, SSB audio with the fixed gain, f32 samples: the whole chain in one kernel (T41RX_SEG_RUN selects the
    // pipeline: the tests that compare the two).  Else AM and the AGC take the complex valid half; real audio with the
    // fixed gain and f32 samples out runs the interpolators behind the fast convolution, no third kernel
    p.one_kernel = f.seg == 8 && f.family != Family::nfm && f.family != Family::am && !f.agc && !f.q15 && !f.seg_run_set;
    p.cplx = !p.one_kernel && (f.agc || f.family == Family::am);
    p.fused_back = !p.one_kernel && !p.cplx && !f.q15;
  }
  p.back = lng           ? Back::long_pipe
           : f.cw_filter ? (f.a24 ? Back::cw_24k : f.cw_unfiltered ? Back::cw_mixed : Back::cw_back)
           : !p.handover ? Back::fused
           : f.a24       ? Back::finish24
                         : Back::back512;
  p.ft8_source = !f.ft8 ? Ft8Source::none : p.handover ? Ft8Source::handover : f.tap_demod ? Ft8Source::caller_tap : Ft8Source::own_tap;
  p.ft8_own_tap = f.ft8 && !stages && !f.tap_demod;
  return p;
}

}  // namespace t41
