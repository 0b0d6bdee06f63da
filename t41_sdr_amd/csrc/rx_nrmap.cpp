// t41_sdr_amd/csrc/rx_nrmap.cpp -- the noise-reduction map (t41rx_set_nr_map / _get_nr_map): nrOptionSelect and ANR_notchOn
// per channel.  Where the stage map (rx_stagemap.cpp) says on which channels "the noise reduction" runs, this says which
// of the four functions.  The same rules as the other maps: configuration, checked here on the host before anything
// changes, uploaded behind a device synchronisation, kept by t41rx_reset().  The lists are rx_nrmap.hpp's, made of the map
// and of the stage map, so they are made again when either changes (nr_map_refresh(), from t41rx_set_stage_map).  A call
// with a map loaded launches nrspec_map_kernel over the spectral list and anr_map_kernel over the Xanr() list's rows
// (nr_kernels.hip), each only if its list has a channel.  The plan (rx_plan.hpp) sees the map as "noise reduction on".
#include <string>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {

static_assert(sizeof(NrMapRow) == sizeof(int4), "a row of the table is the int4 anr_map_kernel reads");

namespace {

// the device copy of the lists (nr_map_layout())
std::vector<int32_t> nr_map_words(const NrMapLists &l, int nchan) {
  const NrMapLayout lay = nr_map_layout(nchan);
  std::vector<int32_t> w(lay.words, 0);
  for (size_t i = 0; i < l.spec.size(); ++i) {
    w[lay.spec + i] = l.spec[i];
    w[lay.spec_kind + i] = l.spec_kind[i];
  }
  for (size_t i = 0; i < l.anr.size(); ++i) w[lay.anr + i] = l.anr[i];
  for (size_t i = 0; i < l.rows.size(); ++i) {
    w[lay.rows + 4 * i + 0] = l.rows[i].offset;
    w[lay.rows + 4 * i + 1] = l.rows[i].live;
    w[lay.rows + 4 * i + 2] = l.rows[i].cls;
  }
  return w;
}

// the spectral function's array-bounds check of params_valid() (design.cpp), for these parameters with nrOptionSelect 2
int spectral_check(const t41rx_params &p) {
  t41rx_params q = p;
  q.nrOptionSelect = 2;
  const char *why = nullptr;
  return params_valid(q, &why) ? T41RX_OK : fail(T41RX_ERR_ARG, why ? why : "bad params");
}

}  // namespace

// the stage map changed (rx_stagemap.cpp, behind its device synchronisation): the lists follow it
int nr_map_refresh(t41rx_ctx *ctx) {
  if (!ctx->nr.map_on) return T41RX_OK;
  NrMapLists lists;
  if (!build_nr_map_lists(ctx->nr.kind_map.data(), ctx->nr.notch_map.data(), ctx->nchan, ctx->nchan,
                          ctx->stages.on ? ctx->stages.map.data() : nullptr, lists))
    return fail(T41RX_ERR_STATE, "noise-reduction map: the loaded map no longer builds");  // (not reached: the map was checked when it was set)
  const std::vector<int32_t> words = nr_map_words(lists, ctx->nchan);
  HIP_TRY(hipMemcpy(ctx->nr.d_map.get(), words.data(), sizeof(int32_t) * words.size(), hipMemcpyHostToDevice));
  ctx->nr.lists = std::move(lists);
  return T41RX_OK;
}

// t41rx_set_params() / t41rx_set_coeffs() with a map loaded: a map with an entry 2 needs the spectral function's pass band
int nr_map_check_params(const t41rx_ctx *ctx, const t41rx_params &p) {
  if (sets_staged(ctx)) return T41RX_OK;  // (the check is each channel's, against its own set: sets_check_set0)
  return ctx->nr.map_on && ctx->nr.lists.spectral ? spectral_check(p) : T41RX_OK;
}

// Process.cpp:841-866 with the channel's own two values: the spectral launch, Xanr()'s behind it on the same stream
int nr_map_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  const NrMapLists &l = ctx->nr.lists;
  if (l.spec.empty() && l.rows.empty()) return T41RX_OK;  // nobody runs anything: nothing to launch
  const NrMapLayout lay = nr_map_layout(ctx->nchan);
  const int32_t *d = ctx->nr.d_map.get();
  NrMapArgs n{};
  n.aud = ctx->d_aud24.get();
  n.anr = ctx->nr.d_anr.get();
  n.spec = ctx->nr.d_spec.get();
  n.tab_nr = ctx->nr.d_tab.get();
  n.tab = ctx->d_tab.get();
  n.nchan = ctx->nchan;
  n.nframes = n_frames;
  n.alpha = ctx->params.NR_alpha;  // (shared: those of the context for every channel)
  n.beta = ctx->params.NR_beta;
  n.psi = ctx->params.NR_PSI;
  nr_vad_range(ctx->params.FLoCut, ctx->params.FHiCut, &n.vad_lo, &n.vad_hi);
  n.list = d + lay.anr;
  n.nlist = (int)l.anr.size();
  n.spec_list = d + lay.spec;
  n.spec_kind = d + lay.spec_kind;
  n.nspec = (int)l.spec.size();
  n.rows = reinterpret_cast<const int4 *>(d + lay.rows);
  n.nrows = (int)l.rows.size();
  return hip_check(launch_nr_map(n, s), "noise-reduction map kernel launch");
}

}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_set_nr_map(t41rx_ctx *ctx, const int32_t *nr_of_channel, const int32_t *notch_of_channel, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ")";
  if (!nr_of_channel && !notch_of_channel) {
    if (n != 0) return fail(T41RX_ERR_ARG, "noise-reduction map: two null maps remove the map and take n 0" + counts);
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the lists they found)
    ctx->nr.map_on = false;
    return stage_sets_refresh(ctx);  // (staged parameter sets: every channel's kind and notch are its own set's again)
  }
  if (!nr_of_channel || !notch_of_channel)
    return fail(T41RX_ERR_ARG, std::string("noise-reduction map: ") + (nr_of_channel ? "notch_of_channel" : "nr_of_channel") +
                                   " is null and the other array is not: the map takes both" + counts);
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "noise-reduction map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
  if (ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "the noise-reduction map is built for fft_length 512, like the noise reduction and the notch");
  // everything is checked here, on the host, before anything changes: the kernels index every buffer with these lists unchecked
  NrMapLists lists;
  const NrMapVerdict v = build_nr_map_lists(nr_of_channel, notch_of_channel, n, ctx->nchan, ctx->stages.on ? ctx->stages.map.data() : nullptr, lists);
  switch (v.fault) {
    case NrMapFault::none:
      break;
    case NrMapFault::count:
    case NrMapFault::null_map:
      return fail(T41RX_ERR_ARG, "noise-reduction map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
    case NrMapFault::kind:
      return fail(T41RX_ERR_ARG, "noise-reduction map: channel " + std::to_string(v.channel) + " has nrOptionSelect " + std::to_string(nr_of_channel[v.channel]) +
                                     ", not 0 (off), 1 (Kim), 2 (spectral) or 3 (LMS)" + counts);
    case NrMapFault::notch:
      return fail(T41RX_ERR_ARG, "noise-reduction map: channel " + std::to_string(v.channel) + " has ANR_notchOn " + std::to_string(notch_of_channel[v.channel]) +
                                     ", not 0 or 1" + counts);
  }
  if (sets_staged(ctx)) {
    // parameter sets next to the stages: the spectral check is each channel's, against the pass band of its own set
    StageSetsNr probe;
    const int rc = stage_sets_build(ctx, ctx->params, ctx->sets.params.data(), (int)ctx->sets.params.size(), ctx->sets.set_of.data(),
                                    nr_of_channel, notch_of_channel, probe);
    if (rc != T41RX_OK) return rc;
  } else if (lists.spectral) {  // (params_valid()'s error and text)
    const int rc = spectral_check(ctx->params);
    if (rc != T41RX_OK) return rc;
  }
  // (an all-zero map is accepted next to parameter sets, as nrOptionSelect 0 and ANR_notchOn 0 are)
  if (lists.any && sets_plain(ctx)) return sets_refuse_stage(kNrMapStageName);
  const std::vector<int32_t> words = nr_map_words(lists, ctx->nchan);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<int32_t> fresh;  // (the first map; later ones reuse the buffer: a failure leaves the previous map whole)
  if (!ctx->nr.d_map) HIP_TRY(dev_alloc(fresh, sizeof(int32_t) * words.size()));
  HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->nr.d_map.get(), words.data(), sizeof(int32_t) * words.size(), hipMemcpyHostToDevice));
  if (fresh) ctx->nr.d_map = std::move(fresh);
  ctx->nr.kind_map.assign(nr_of_channel, nr_of_channel + n);
  ctx->nr.notch_map.assign(notch_of_channel, notch_of_channel + n);
  ctx->nr.lists = std::move(lists);
  ctx->nr.map_on = true;
  return stage_sets_refresh(ctx);  // (staged parameter sets: the map supplies every channel's kind and notch)
}

int t41rx_get_nr_map(const t41rx_ctx *ctx, int32_t *nr_of_channel_out, int32_t *notch_of_channel_out, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (nr_of_channel_out || notch_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "noise-reduction map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    for (int i = 0; i < n; ++i) {
      if (nr_of_channel_out) nr_of_channel_out[i] = ctx->nr.map_on ? ctx->nr.kind_map[(size_t)i] : ctx->params.nrOptionSelect;
      if (notch_of_channel_out) notch_of_channel_out[i] = ctx->nr.map_on ? ctx->nr.notch_map[(size_t)i] : ctx->params.ANR_notchOn;
    }
  }
  return ctx->nr.map_on ? 1 : 0;
}

}  // extern "C"
