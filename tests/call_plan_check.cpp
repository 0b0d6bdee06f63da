// tests/call_plan_check.cpp -- walks every CallFacts through plan_call() (t41_sdr_amd/csrc/rx_plan.hpp) and checks what
// the consumers of a plan rely on.  A program of its own for tests/test_call_plan.py: no GPU, no HIP.  Exit status 0 and a
// count of the plans walked, or 1 with the first violating facts.
#include <cstdio>
#include <cstring>

#include "rx_plan.hpp"

using namespace t41;

namespace {

const CallFacts *g_facts = nullptr;

void print_facts(const CallFacts &f) {
  std::printf("  seg %d family %d agc %d q15 %d nfm_atan %d plain_gains %d n_frames %d seg_run_set %d map %d sets %d a24 %d\n"
              "  tap_nco %d tap_dec %d tap_demod %d spect %d disp %d pan_rows %d ft8 %d | eq %d nr %d nb %d cw_filter %d cw_det %d\n",
              f.seg, (int)f.family, f.agc, f.q15, f.nfm_atan, f.plain_gains, f.n_frames, f.seg_run_set, f.map, f.sets, f.a24, f.tap_nco,
              f.tap_dec, f.tap_demod, f.spect, f.disp, f.pan_rows, f.ft8, f.eq, f.nr, f.nb, f.cw_filter, f.cw_det);
}

bool violated(const char *what) {
  std::printf("call plan: violated: %s\n", what);
  print_facts(*g_facts);
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond)
// x => y
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

bool check(const CallFacts &f, const CallPlan &p) {
  const bool lng = f.seg > 1, sam = f.family == Family::sam;
  const bool stages = f.eq || f.nr || f.nb || f.cw_filter || f.cw_det;
  const bool stage_taps = f.tap_nco || f.tap_dec || f.tap_demod;
  // the combinations the setters refuse
  const bool refused = (lng && (f.a24 || f.sets || stage_taps || stages || f.nfm_atan)) || (f.sets && stages);
  IFF(!p.valid, refused);
  REQUIRE(p.why != nullptr);
  IFF(!p.valid, p.why[0] != 0);
  if (!p.valid) return true;

  const KernelForm &k = p.form;
  REQUIRE(p.seg == f.seg);
  // exactly one back end (an enum), and it matches the rest
  IFF(p.back == Back::fused, !p.handover && f.seg == 1);
  IMPLIES(p.back == Back::back512 || p.back == Back::cw_back || p.back == Back::cw_24k || p.back == Back::finish24, p.handover && f.seg == 1);
  IFF(p.back == Back::long_pipe, lng);
  IFF(p.back == Back::cw_back || p.back == Back::cw_24k, f.cw_filter);
  IMPLIES(p.back == Back::cw_24k || p.back == Back::finish24, f.a24);
  IMPLIES(p.back == Back::cw_back || p.back == Back::back512, !f.a24);
  IMPLIES(p.handover, k.taps && p.scratch);
  IMPLIES(lng, p.scratch);
  IMPLIES(stages, p.handover);
  IMPLIES(k.a24_form, k.map_form && !k.taps && f.seg == 1);
  IMPLIES(f.a24, k.a24_form != p.handover);  // a 24 kS/s call stores from the fused twin or finishes from the hand-over
  IMPLIES(k.set_form, k.map_form && f.seg == 1);
  IFF(k.set_form, f.sets);
  IMPLIES(f.map, k.map_form);
  IMPLIES(k.pipe, (f.agc || sam) && !k.taps && f.n_frames >= 4 && f.seg == 1 && p.pipe_buffer);
  IMPLIES(k.plain, f.plain_gains);
  IMPLIES(k.plain && !lng, !k.taps && !sam);
  IMPLIES(k.plain && lng, !f.q15);
  IFF(p.need_ident, k.map_form && !f.map);
  IFF(p.ft8_source == Ft8Source::own_tap, f.ft8 && !p.handover && !f.tap_demod);
  IFF(p.ft8_source == Ft8Source::none, !f.ft8);
  IMPLIES(p.ft8_source == Ft8Source::handover, p.handover);
  IMPLIES(p.ft8_source == Ft8Source::caller_tap, f.tap_demod);
  IMPLIES(p.ft8_source == Ft8Source::own_tap, p.ft8_own_tap);
  IMPLIES(f.ft8 && !lng, k.taps);
  REQUIRE(k.family == f.family && k.agc == f.agc && k.q15 == f.q15);
  // the form named is instantiated: the whole chain at 512, the front end at the long lengths
  IMPLIES(!lng, form_compiled(k));
  IMPLIES(lng, long_front_compiled(k.plain, k.q15) && !k.taps && !k.pipe && !k.set_form && !k.a24_form);
  IMPLIES(p.one_kernel || p.cplx || p.fused_back, lng);
  IMPLIES(p.one_kernel, f.seg == 8 && !p.cplx && !p.fused_back && !f.q15 && !f.agc);
  IMPLIES(p.fused_back, !p.cplx && !f.q15);
  return true;
}

}  // namespace

int main() {
  static_assert(plan_call(CallFacts{}).valid, "plan_call() is constexpr");
  const int segs[4] = {1, 2, 4, 8}, frames[4] = {1, 3, 4, 5};
  long long walked = 0;
  for (int seg : segs)
    for (int fam = 0; fam < 4; ++fam)
      for (unsigned bits = 0; bits < (1u << 20); ++bits) {
        CallFacts f;
        f.seg = seg;
        f.family = (Family)fam;
        unsigned b = bits;
        auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
        f.agc = next(), f.q15 = next(), f.nfm_atan = next(), f.plain_gains = next();
        f.seg_run_set = next(), f.map = next(), f.sets = next(), f.a24 = next();
        f.tap_nco = next(), f.tap_dec = next(), f.tap_demod = next(), f.spect = next(), f.disp = next(), f.pan_rows = next(), f.ft8 = next();
        f.eq = next(), f.nr = next(), f.nb = next(), f.cw_filter = next(), f.cw_det = next();
        g_facts = &f;
        CallPlan of[4];
        for (int i = 0; i < 4; ++i) {
          f.n_frames = frames[i];
          of[i] = plan_call(f);
          if (!check(f, of[i])) return 1;
          ++walked;
        }
        // the plan depends on n_frames only through n_frames >= 4
        if (!same_plan(of[0], of[1]) || !same_plan(of[2], of[3])) {
          violated("the plan depends on n_frames only through n_frames >= 4");
          return 1;
        }
      }
  std::printf("call plan: %lld plans walked, no violation\n", walked);
  return 0;
}
