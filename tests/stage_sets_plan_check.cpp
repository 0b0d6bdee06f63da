// tests/stage_sets_plan_check.cpp -- walks every CallFacts through plan_call() (t41_sdr_amd/csrc/rx_plan.hpp) for
// CallFacts::stage_sets, the fact that parameter sets were loaded with T41RX_SETS_STAGES (t41rx_set_param_sets_ex).
// With the fact false the plan must be what it was before the fact existed: stated here as the literal expectations of
// tests/call_plan_check.cpp (which combinations are refused, and the relations of a valid plan), not as a call to the code
// under test.  With it true, `sets && stages` at fft_length 512 is a valid call that takes the tap kernel in its set form,
// hands over, and ends in the back end the same call takes without sets; everywhere else the fact is not read.
// A program of its own for tests/test_stage_sets_plan.py: no GPU, no HIP.  Exit status 0 and a count of the plans walked,
// or 1 with the first violating facts.
#include <cstdio>
#include <cstring>

#include "rx_plan.hpp"

using namespace t41;

namespace {

const CallFacts *g_facts = nullptr;

bool violated(const char *what) {
  const CallFacts &f = *g_facts;
  std::printf("stage sets plan: violated: %s\n", what);
  std::printf("  seg %d family %d agc %d q15 %d nfm_atan %d plain_gains %d n_frames %d seg_run_set %d map %d sets %d stage_sets %d a24 %d omap %d\n"
              "  tap_nco %d tap_dec %d tap_demod %d spect %d disp %d pan_rows %d ft8 %d | eq %d nr %d nb %d cw_filter %d cw_det %d cw_unfiltered %d\n",
              f.seg, (int)f.family, f.agc, f.q15, f.nfm_atan, f.plain_gains, f.n_frames, f.seg_run_set, f.map, f.sets, f.stage_sets, f.a24, f.omap,
              f.tap_nco, f.tap_dec, f.tap_demod, f.spect, f.disp, f.pan_rows, f.ft8, f.eq, f.nr, f.nb, f.cw_filter, f.cw_det, f.cw_unfiltered);
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond)
#define IMPLIES(x, y) \
  if ((x) && !(y)) return violated(#x " => " #y)
#define IFF(x, y) \
  if ((x) != (y)) return violated(#x " <=> " #y)

bool same_plan(const CallPlan &a, const CallPlan &b) {
  return a.valid == b.valid && std::strcmp(a.why, b.why) == 0 && a.nfm_atan_long == b.nfm_atan_long && a.seg == b.seg && a.form == b.form &&
         a.handover == b.handover && a.scratch == b.scratch && a.need_ident == b.need_ident && a.pipe_buffer == b.pipe_buffer &&
         a.one_kernel == b.one_kernel && a.cplx == b.cplx && a.fused_back == b.fused_back && a.back == b.back &&
         a.ft8_source == b.ft8_source && a.ft8_own_tap == b.ft8_own_tap;
}

// stage_sets false: tests/call_plan_check.cpp's expectations, with the output map's refusal at the long lengths
// (tests/output_map_plan_check.cpp) and the back end of a filter map with both classes
bool check_as_before(const CallFacts &f, const CallPlan &p) {
  const bool lng = f.seg > 1, sam = f.family == Family::sam;
  const bool stages = f.eq || f.nr || f.nb || f.cw_filter || f.cw_det;
  const bool stage_taps = f.tap_nco || f.tap_dec || f.tap_demod;
  const bool refused = (lng && (f.a24 || f.sets || stage_taps || stages || f.nfm_atan || f.omap)) || (f.sets && stages);
  IFF(!p.valid, refused);
  REQUIRE(p.why != nullptr);
  IFF(!p.valid, p.why[0] != 0);
  IMPLIES(f.sets && stages && !(f.nfm_atan && lng),
          std::strcmp(p.why, "parameter sets are loaded with a long fft_length or a chain-splitting stage") == 0);
  if (!p.valid) return true;
  const KernelForm &k = p.form;
  REQUIRE(p.seg == f.seg);
  IFF(p.back == Back::fused, !p.handover && f.seg == 1);
  IMPLIES(p.back == Back::back512 || p.back == Back::cw_back || p.back == Back::cw_24k || p.back == Back::cw_mixed || p.back == Back::finish24,
          p.handover && f.seg == 1);
  IFF(p.back == Back::long_pipe, lng);
  IFF(p.back == Back::cw_back || p.back == Back::cw_24k || p.back == Back::cw_mixed, f.cw_filter);
  IFF(p.back == Back::cw_mixed, f.cw_filter && !f.a24 && f.cw_unfiltered);
  IMPLIES(p.back == Back::cw_24k || p.back == Back::finish24, f.a24);
  IMPLIES(p.back == Back::cw_back || p.back == Back::back512, !f.a24);
  IMPLIES(p.handover, k.taps && p.scratch);
  IMPLIES(lng, p.scratch);
  IMPLIES(stages, p.handover);
  IMPLIES(k.a24_form, k.map_form && !k.taps && f.seg == 1);
  IMPLIES(f.a24, k.a24_form != p.handover);
  IMPLIES(k.set_form, k.map_form && f.seg == 1);
  IFF(k.set_form, f.sets);
  IMPLIES(f.map, k.map_form);
  IMPLIES(k.pipe, (f.agc || sam) && !k.taps && f.n_frames >= 4 && f.seg == 1 && p.pipe_buffer);
  IMPLIES(k.plain, f.plain_gains);
  IMPLIES(k.plain && !lng, !k.taps && !sam);
  IFF(p.need_ident, k.map_form && !f.map);
  IFF(p.ft8_source == Ft8Source::none, !f.ft8);
  REQUIRE(k.family == f.family && k.agc == f.agc && k.q15 == f.q15);
  IMPLIES(!lng, form_compiled(k));
  return true;
}

// stage_sets true, sets and a stage at fft_length 512: valid, taps + set form + hand-over, the back of the call without sets
bool check_staged(const CallFacts &f, const CallPlan &p) {
  REQUIRE(p.valid && p.why != nullptr && p.why[0] == 0);
  const KernelForm &k = p.form;
  REQUIRE(k.taps && k.set_form && k.map_form && !k.plain && !k.pipe && !k.a24_form && !k.omap_form);
  REQUIRE(p.handover && p.scratch);
  REQUIRE(form_compiled(k));
  IFF(p.need_ident, !f.map);
  CallFacts g = f;
  g.sets = false;
  const CallPlan q = plan_call(g);  // (a call this program has checked under check_as_before: sets false)
  REQUIRE(q.valid && p.back == q.back && q.handover && q.form.taps);
  REQUIRE(p.back != Back::fused && p.back != Back::long_pipe);
  IFF(p.back == Back::back512, !f.cw_filter && !f.a24);
  IFF(p.back == Back::finish24, !f.cw_filter && f.a24);
  IFF(p.back == Back::cw_24k, f.cw_filter && f.a24);
  IFF(p.back == Back::cw_mixed, f.cw_filter && !f.a24 && f.cw_unfiltered);
  IFF(p.back == Back::cw_back, f.cw_filter && !f.a24 && !f.cw_unfiltered);
  REQUIRE(p.ft8_source == q.ft8_source && p.ft8_own_tap == q.ft8_own_tap && p.pipe_buffer == q.pipe_buffer);
  REQUIRE(k.family == f.family && k.agc == f.agc && k.q15 == f.q15);
  return true;
}

}  // namespace

int main() {
  const int segs[2] = {1, 8}, frames[2] = {3, 4};  // (the plan reads seg as seg > 1 and seg == 8)
  long long walked = 0, staged = 0;
  for (int seg : segs)
    for (int fam = 0; fam < 4; ++fam)
      for (unsigned bits = 0; bits < (1u << 22); ++bits) {
        CallFacts f;
        f.seg = seg;
        f.family = (Family)fam;
        unsigned b = bits;
        auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
        f.agc = next(), f.q15 = next(), f.nfm_atan = next(), f.plain_gains = next();
        f.seg_run_set = next(), f.map = next(), f.sets = next(), f.a24 = next();
        f.tap_nco = next(), f.tap_dec = next(), f.tap_demod = next(), f.spect = next(), f.disp = next(), f.pan_rows = next(), f.ft8 = next();
        f.eq = next(), f.nr = next(), f.nb = next(), f.cw_filter = next(), f.cw_det = next();
        f.omap = next(), f.cw_unfiltered = next();
        if (f.cw_unfiltered && !f.cw_filter) continue;  // (cw_unfiltered is a fact of a call with the filter: rx_plan.hpp)
        g_facts = &f;
        const bool stages = f.eq || f.nr || f.nb || f.cw_filter || f.cw_det;
        for (int n : frames) {
          f.n_frames = n;
          f.stage_sets = false;
          const CallPlan before = plan_call(f);
          if (!check_as_before(f, before)) return 1;
          f.stage_sets = true;
          const CallPlan with = plan_call(f);
          ++walked;
          const bool lng = seg > 1;
          if (f.sets && stages && !lng) {
            if (!check_staged(f, with)) return 1;
            ++staged;
          } else if (!same_plan(before, with)) {
            // (at a long length sets && stages stays refused, in the same words: the fact changes nothing there either)
            violated("stage_sets is read only where sets && stages at fft_length 512");
            return 1;
          }
        }
      }
  std::printf("stage sets plan: %lld facts walked, %lld staged calls, no violation\n", walked, staged);
  return 0;
}
