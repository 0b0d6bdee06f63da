// tests/stage_params_plan_check.cpp -- walks every CallFacts, CallFacts::cw_unfiltered included, through plan_call()
// (t41_sdr_amd/csrc/rx_plan.hpp) and checks what the CW filter map (t41rx_set_cw_filter_map) adds to a plan and that it
// changes nothing without one.  A program of its own for tests/test_stage_params_plan.py: no GPU, no HIP.  Exit status 0
// and a count of the plans walked, or 1 with the first violating facts.
#include <cstdio>
#include <cstring>

#include "rx_plan.hpp"

using namespace t41;

namespace {

const CallFacts *g_facts = nullptr;

bool violated(const char *what) {
  const CallFacts &f = *g_facts;
  std::printf("stage params plan: violated: %s\n", what);
  std::printf("  seg %d family %d agc %d q15 %d nfm_atan %d plain_gains %d n_frames %d seg_run_set %d map %d sets %d a24 %d omap %d\n"
              "  tap_nco %d tap_dec %d tap_demod %d spect %d disp %d pan_rows %d ft8 %d | eq %d nr %d nb %d cw_filter %d cw_det %d cw_unfiltered %d\n",
              f.seg, (int)f.family, f.agc, f.q15, f.nfm_atan, f.plain_gains, f.n_frames, f.seg_run_set, f.map, f.sets, f.a24, f.omap,
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

// the plan of these facts before the filter map existed: the back end's expression as it stood, everything else is not
// touched by the new fact (same_plan against the plan with the fact cleared holds that)
Back back_before(const CallFacts &f, const CallPlan &p) {
  return f.seg > 1 ? Back::long_pipe : f.cw_filter ? (f.a24 ? Back::cw_24k : Back::cw_back) : !p.handover ? Back::fused : f.a24 ? Back::finish24 : Back::back512;
}

bool check(const CallFacts &f, const CallPlan &p) {
  const bool lng = f.seg > 1;
  const bool stages = f.eq || f.nr || f.nb || f.cw_filter || f.cw_det;
  CallFacts cleared = f;
  cleared.cw_unfiltered = false;
  const CallPlan q = plan_call(cleared);
  // every existing CallFacts keeps its plan
  if (!f.cw_unfiltered) {
    REQUIRE(same_plan(p, q));
    REQUIRE(p.back == back_before(f, p));
    REQUIRE(p.back != Back::cw_mixed);
  }
  // the new fact touches the back end alone, and only that of a 192 kS/s call with some channel filtered
  {
    CallPlan r = p;
    r.back = q.back;
    REQUIRE(same_plan(r, q));
  }
  IFF(p.back == Back::cw_mixed, !lng && f.cw_filter && f.cw_unfiltered && !f.a24);
  IMPLIES(p.back != Back::cw_mixed, p.back == q.back);
  // an all-off map (nobody filtered: cw_filter false, cw_unfiltered true) never plans a CW back end, and is the plan of a
  // call without the filter
  IMPLIES(!f.cw_filter, p.back != Back::cw_back && p.back != Back::cw_24k && p.back != Back::cw_mixed);
  IMPLIES(!f.cw_filter, same_plan(p, q));
  if (!p.valid) return true;
  // tests/call_plan_check.cpp's invariants of the back end, with cw_mixed among the hand-over back ends
  IFF(p.back == Back::fused, !p.handover && f.seg == 1);
  IMPLIES(p.back == Back::back512 || p.back == Back::cw_back || p.back == Back::cw_24k || p.back == Back::cw_mixed || p.back == Back::finish24,
          p.handover && f.seg == 1);
  IFF(p.back == Back::long_pipe, lng);
  IFF(p.back == Back::cw_back || p.back == Back::cw_24k || p.back == Back::cw_mixed, f.cw_filter);
  IMPLIES(p.back == Back::cw_24k || p.back == Back::finish24, f.a24);
  IMPLIES(p.back == Back::cw_back || p.back == Back::cw_mixed || p.back == Back::back512, !f.a24);
  IMPLIES(p.handover, p.form.taps && p.scratch);
  IMPLIES(stages, p.handover);
  IMPLIES(f.cw_filter && f.a24, p.back == Back::cw_24k);  // one finish serves both classes
  REQUIRE(lng || form_compiled(p.form));
  return true;
}

}  // namespace

int main() {
  static_assert(plan_call(CallFacts{}).back == Back::fused, "plan_call() is constexpr");
  const int segs[4] = {1, 2, 4, 8}, frames[2] = {3, 5};
  long long walked = 0;
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
        g_facts = &f;
        for (int nf : frames) {  // either side of the pipelined forms' threshold
          f.n_frames = nf;
          if (!check(f, plan_call(f))) return 1;
          ++walked;
        }
      }
  std::printf("stage params plan: %lld plans walked, no violation\n", walked);
  return 0;
}
