// tests/output_map_plan_check.cpp -- walks every CallFacts, CallFacts::omap included, through plan_call()
// (t41_sdr_amd/csrc/rx_plan.hpp) and checks what the output map (t41rx_set_output_map) adds to a plan and that it changes
// nothing without one.  A program of its own for tests/test_output_map_plan.py: no GPU, no HIP.  Exit status 0 and a count
// of the plans walked, or 1 with the first violating facts.
#include <cstdio>

#include "rx_plan.hpp"

using namespace t41;

namespace {

const CallFacts *g_facts = nullptr;

bool violated(const char *what) {
  const CallFacts &f = *g_facts;
  std::printf("output map plan: violated: %s\n", what);
  std::printf("  seg %d family %d agc %d q15 %d nfm_atan %d plain_gains %d n_frames %d seg_run_set %d map %d sets %d a24 %d omap %d\n"
              "  tap_nco %d tap_dec %d tap_demod %d spect %d disp %d pan_rows %d ft8 %d | eq %d nr %d nb %d cw_filter %d cw_det %d\n",
              f.seg, (int)f.family, f.agc, f.q15, f.nfm_atan, f.plain_gains, f.n_frames, f.seg_run_set, f.map, f.sets, f.a24, f.omap,
              f.tap_nco, f.tap_dec, f.tap_demod, f.spect, f.disp, f.pan_rows, f.ft8, f.eq, f.nr, f.nb, f.cw_filter, f.cw_det);
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond)
#define IMPLIES(x, y) \
  if ((x) && !(y)) return violated(#x " => " #y)
#define IFF(x, y) \
  if ((x) != (y)) return violated(#x " <=> " #y)

bool check(const CallFacts &f, const CallPlan &p) {
  const bool lng = f.seg > 1;
  CallFacts cleared = f;
  cleared.omap = false;
  const CallPlan q = plan_call(cleared);
  if (!f.omap) {
    // without a map: no output-map form, and back end and hand-over as computed from a copy of the facts without it
    REQUIRE(!p.form.omap_form);
    REQUIRE(p.back == q.back && p.handover == q.handover);
    REQUIRE(p.valid == q.valid);
  }
  // the long lengths refuse the map, in words
  IMPLIES(f.omap && lng, !p.valid && p.why != nullptr && p.why[0] != 0);
  IMPLIES(f.omap && !lng, p.valid == q.valid);
  if (!p.valid) return true;
  const KernelForm &k = p.form;
  IMPLIES(k.omap_form, k.map_form && !k.taps && f.seg == 1);
  IMPLIES(k.omap_form, f.omap);
  // a mapped call at 512 stores from the fused twin or finishes from the hand-over, never both and never neither
  IMPLIES(f.omap && !lng, k.omap_form != p.handover);
  IMPLIES(f.omap && p.handover, k.taps && p.scratch && p.back != Back::fused);
  REQUIRE(lng || form_compiled(k));
  IFF(p.need_ident, k.map_form && !f.map);
  return true;
}

}  // namespace

int main() {
  const int segs[4] = {1, 2, 4, 8}, frames[2] = {3, 5};
  long long walked = 0;
  for (int seg : segs)
    for (int fam = 0; fam < 4; ++fam)
      for (unsigned bits = 0; bits < (1u << 21); ++bits) {
        CallFacts f;
        f.seg = seg;
        f.family = (Family)fam;
        unsigned b = bits;
        auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
        f.agc = next(), f.q15 = next(), f.nfm_atan = next(), f.plain_gains = next();
        f.seg_run_set = next(), f.map = next(), f.sets = next(), f.a24 = next();
        f.tap_nco = next(), f.tap_dec = next(), f.tap_demod = next(), f.spect = next(), f.disp = next(), f.pan_rows = next(), f.ft8 = next();
        f.eq = next(), f.nr = next(), f.nb = next(), f.cw_filter = next(), f.cw_det = next();
        f.omap = next();
        g_facts = &f;
        for (int nf : frames) {  // either side of the pipelined forms' threshold
          f.n_frames = nf;
          if (!check(f, plan_call(f))) return 1;
          ++walked;
        }
      }
  std::printf("output map plan: %lld plans walked, no violation\n", walked);
  return 0;
}
