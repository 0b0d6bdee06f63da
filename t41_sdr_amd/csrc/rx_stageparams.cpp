// t41_sdr_amd/csrc/rx_stageparams.cpp -- stage parameters per channel: the CW filter map (t41rx_set_cw_filter_map /
// _get_cw_filter_map) and the equalizer level map (t41rx_set_receive_eq_map / _get_receive_eq_map).  Where the stage map
// (rx_stagemap.cpp) says on which channels a stage runs, these say with which parameters.  The same rules as the other
// maps: configuration, checked here on the host before anything changes, uploaded behind a device synchronisation, kept
// by t41rx_reset().  The filter map's lists are rx_stageparams.hpp's; what a call does with them is cw_filter_run()'s
// (rx_cw.cpp) under the plan (rx_plan.hpp: CallFacts::cw_unfiltered, Back::cw_mixed).  The level map is read by eq_run()
// (rx_audio.cpp) and is not the plan's business.
#include <string>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {

static_assert(kCwFilterOff == kCwFilters, "rx_stageparams.hpp names the off value as cw_kernels.hpp does");

namespace {

// the four rows of CwStage::d_map (rx_ctx.hpp: CwMapRow) of a map and its lists; the list's padding names channel 0
std::vector<int32_t> cw_map_rows(const int32_t *filter_of_channel, const CwFilterLists &l, int nchan) {
  const size_t pitch = cw_map_pitch(nchan);
  std::vector<int32_t> rows((size_t)kCwMapRows * pitch, 0);
  for (int c = 0; c < nchan; ++c) {
    rows[(size_t)kCwMapIndex * pitch + (size_t)c] = filter_of_channel[c];
    rows[(size_t)kCwMapRowsFiltered * pitch + (size_t)c] = l.rows_filtered[(size_t)c];
    rows[(size_t)kCwMapRowsPlain * pitch + (size_t)c] = l.rows_plain[(size_t)c];
  }
  for (size_t i = 0; i < l.filtered.size(); ++i) rows[(size_t)kCwMapList * pitch + i] = l.filtered[i];
  return rows;
}

}  // namespace

// the output map changed (rx_outmap.cpp, behind its device synchronisation): the two row maps follow it
int cw_filter_map_refresh(t41rx_ctx *ctx) {
  if (!ctx->cw.map_on) return T41RX_OK;
  CwFilterLists lists;
  if (!build_cw_filter_lists(ctx->cw.filter_map.data(), ctx->nchan, ctx->nchan, true, ctx->out_map_on ? ctx->out_map.data() : nullptr, lists))
    return fail(T41RX_ERR_STATE, "CW filter map: the loaded map no longer builds");  // (not reached: the map was checked when it was set)
  const std::vector<int32_t> rows = cw_map_rows(ctx->cw.filter_map.data(), lists, ctx->nchan);
  HIP_TRY(hipMemcpy(ctx->cw.d_map.get(), rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice));
  ctx->cw.lists = std::move(lists);
  return T41RX_OK;
}

}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_set_cw_filter_map(t41rx_ctx *ctx, const int32_t *filter_of_channel, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ")";
  if (!filter_of_channel) {
    if (n != 0) return fail(T41RX_ERR_ARG, "CW filter map: a null map removes the map and takes n 0" + counts);
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the lists they found)
    ctx->cw.map_on = false;
    return T41RX_OK;
  }
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the CW filter map is built for fft_length 512, like the CW audio filters");
  // everything is checked here, on the host, before anything changes: the kernels index every buffer with these lists unchecked
  CwFilterLists lists;
  const CwFilterMapVerdict v = build_cw_filter_lists(filter_of_channel, n, ctx->nchan, ctx->cw.have_filters,
                                                     ctx->out_map_on ? ctx->out_map.data() : nullptr, lists);
  switch (v.fault) {
    case CwFilterMapFault::none:
      break;
    case CwFilterMapFault::count:
    case CwFilterMapFault::null_map:
      return fail(T41RX_ERR_ARG, "CW filter map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
    case CwFilterMapFault::range:
      return fail(T41RX_ERR_ARG, "CW filter map: channel " + std::to_string(v.channel) + " has CWFilterIndex " + std::to_string(filter_of_channel[v.channel]) +
                                     ", neither 0 .. 4 nor 5 (off)" + counts);
    case CwFilterMapFault::tables:
      return fail(T41RX_ERR_ARG, "CW filter map: channel " + std::to_string(v.channel) + " has CWFilterIndex " + std::to_string(filter_of_channel[v.channel]) +
                                     " and no filter tables are loaded (t41rx_set_cw_tables)" + counts);
  }
  // (a map that filters nobody is accepted next to parameter sets, as t41rx_set_cw_filter(ctx, 5) is)
  if (!lists.filtered.empty() && sets_plain(ctx)) return sets_refuse_stage("the CW audio filter");
  const std::vector<int32_t> rows = cw_map_rows(filter_of_channel, lists, ctx->nchan);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<int32_t> fresh;  // (the first map; later ones reuse the buffer: a failure leaves the previous map whole)
  if (!ctx->cw.d_map) HIP_TRY(dev_alloc(fresh, sizeof(int32_t) * rows.size()));
  HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->cw.d_map.get(), rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice));
  if (fresh) ctx->cw.d_map = std::move(fresh);
  ctx->cw.filter_map.assign(filter_of_channel, filter_of_channel + n);
  ctx->cw.lists = std::move(lists);
  ctx->cw.map_on = true;
  return T41RX_OK;
}

int t41rx_get_cw_filter_map(const t41rx_ctx *ctx, int32_t *filter_of_channel_out, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (filter_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "CW filter map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    for (int i = 0; i < n; ++i) filter_of_channel_out[i] = ctx->cw.map_on ? ctx->cw.filter_map[(size_t)i] : ctx->cw.filter;
  }
  return ctx->cw.map_on ? 1 : 0;
}

int t41rx_set_receive_eq_map(t41rx_ctx *ctx, const int32_t *equalizerRec, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ")";
  if (!equalizerRec) {
    if (n != 0) return fail(T41RX_ERR_ARG, "receive-equalizer level map: a null map removes the map and takes n 0" + counts);
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the levels they found)
    ctx->eq.map_on = false;
    return T41RX_OK;
  }
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "receive-equalizer level map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the receive-equalizer level map is built for fft_length 512, like the receive equalizer");
  // (t41rx_set_receive_eq() takes every level vector, as the firmware's menu stores what it is given: none is refused here)
  const size_t words = (size_t)kEqBands * (size_t)n;
  std::vector<float> scale(words);
  for (size_t i = 0; i < words; ++i) {
    // recEQ_LevelScale[b] = (float)EEPROMData.equalizerRec[b] / 100.0, negated for bands 1, 3, .., 13: eq_run()'s expression
    const float lvl = (float)((double)(float)equalizerRec[i] / 100.0);
    scale[i] = ((i % kEqBands) % 2 == 0) ? -lvl : lvl;
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<float> fresh;  // (the first map; later ones reuse the buffer: a failure leaves the previous map whole)
  if (!ctx->eq.d_levels) HIP_TRY(dev_alloc(fresh, sizeof(float) * words));
  HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->eq.d_levels.get(), scale.data(), sizeof(float) * words, hipMemcpyHostToDevice));
  if (fresh) ctx->eq.d_levels = std::move(fresh);
  ctx->eq.level_map.assign(equalizerRec, equalizerRec + words);
  ctx->eq.map_on = true;
  return T41RX_OK;
}

int t41rx_get_receive_eq_map(const t41rx_ctx *ctx, int32_t *equalizerRec_out, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (equalizerRec_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "receive-equalizer level map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    for (size_t i = 0; i < (size_t)kEqBands * (size_t)n; ++i)
      equalizerRec_out[i] = ctx->eq.map_on ? ctx->eq.level_map[i] : ctx->eq.levels[i % kEqBands];
  }
  return ctx->eq.map_on ? 1 : 0;
}

}  // extern "C"
