// t41_sdr_amd/csrc/rx_stagemap.cpp -- the stage map (t41rx_set_stage_map / _get_stage_map): which of the stages behind the
// demodulator -- the receive equalizer, the noise reduction / notch, the noise blanker, the CW detector and the Morse
// decoder -- run on which channel of a receiver group.  The fourth map of the series and the same rules as the output map
// (rx_outmap.cpp): configuration, checked here on the host before anything changes, uploaded behind a device
// synchronisation.  The lists are rx_stagemap.hpp's; what a call does with them is each stage's own *_run (rx_audio.cpp,
// rx_cw.cpp): the list form of its kernel over the list's length, or no launch for an empty list.  The plan of a call
// (rx_plan.hpp) does not see the map.
#include <string>
#include <vector>

#include "rx_ctx.hpp"

using namespace t41;

static_assert(stage_bit(kStageEq) == T41RX_STAGE_EQ && stage_bit(kStageNr) == T41RX_STAGE_NR && stage_bit(kStageNb) == T41RX_STAGE_NB &&
                  stage_bit(kStageCwDetect) == T41RX_STAGE_CW_DETECT && stage_bit(kStageCwDecode) == T41RX_STAGE_CW_DECODE &&
                  kStageAll == T41RX_STAGE_ALL,
              "rx_stagemap.hpp numbers the stages as include/t41rx.h does");

extern "C" {

int t41rx_set_stage_map(t41rx_ctx *ctx, const uint32_t *stages_of_channel, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ")";
  if (!stages_of_channel) {
    if (n != 0) return fail(T41RX_ERR_ARG, "stage map: a null map removes the map and takes n 0" + counts);
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the lists they found)
    ctx->stages.on = false;
    if (const int rc = nr_map_refresh(ctx)) return rc;  // (the noise-reduction map's lists are made of this map too: rx_nrmap.cpp)
    return stage_sets_refresh(ctx);                     // (... and those of parameter sets loaded next to the stages: rx_sets.cpp)
  }
  if (ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "the stage map is built for fft_length 512 (the stages it lists refuse the long lengths themselves)");
  // everything is checked here, on the host, before anything changes: the kernels index every buffer with these lists unchecked
  StageLists lists;
  const StageMapVerdict v = build_stage_lists(stages_of_channel, n, ctx->nchan, lists);
  switch (v.fault) {
    case StageMapFault::none:
      break;
    case StageMapFault::count:
    case StageMapFault::null_map:
      return fail(T41RX_ERR_ARG, "stage map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
    case StageMapFault::bits:
      return fail(T41RX_ERR_ARG, "stage map: channel " + std::to_string(v.channel) + " has mask " + std::to_string(stages_of_channel[v.channel]) +
                                     ", bits outside T41RX_STAGE_ALL (" + std::to_string(kStageAll) + ")" + counts);
    case StageMapFault::decode_without_detect:
      return fail(T41RX_ERR_ARG, "stage map: channel " + std::to_string(v.channel) + " has T41RX_STAGE_CW_DECODE without T41RX_STAGE_CW_DETECT: " +
                                     "the decoder reads the detector's rows of its own channel" + counts);
  }
  const size_t nch = (size_t)ctx->nchan;
  std::vector<int32_t> rows((size_t)(kStageCount + 1) * nch, 0);
  for (int s = 0; s <= kStageCount; ++s) {
    const std::vector<int32_t> &l = s < kStageCount ? lists.list[s] : lists.nb_rest;
    for (size_t i = 0; i < l.size(); ++i) rows[(size_t)s * nch + i] = l[i];
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<int32_t> fresh;  // (the first map; later ones reuse the buffer: a failure leaves the previous map whole)
  if (!ctx->stages.d_lists) HIP_TRY(dev_alloc(fresh, sizeof(int32_t) * rows.size()));
  HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->stages.d_lists.get(), rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice));
  if (fresh) ctx->stages.d_lists = std::move(fresh);
  ctx->stages.map.assign(stages_of_channel, stages_of_channel + n);
  ctx->stages.lists = std::move(lists);
  ctx->stages.on = true;
  if (const int rc = nr_map_refresh(ctx)) return rc;
  return stage_sets_refresh(ctx);
}

int t41rx_get_stage_map(const t41rx_ctx *ctx, uint32_t *stages_of_channel_out, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (stages_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "stage map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    for (int i = 0; i < n; ++i) stages_of_channel_out[i] = ctx->stages.on ? ctx->stages.map[(size_t)i] : kStageAll;
  }
  return ctx->stages.on ? 1 : 0;
}

}  // extern "C"
