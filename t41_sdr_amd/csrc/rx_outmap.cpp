// t41_sdr_amd/csrc/rx_outmap.cpp -- the output map (t41rx_set_output_map / _get_output_map / t41rx_audio_rows): which row
// of the audio buffer a channel of a receiver group writes, or that it writes none.  The mirror of the input map
// (rx_host.cpp: t41rx_set_input_map): configuration, checked here on the host before anything changes, uploaded behind a
// device synchronisation.  What a call does with it is the plan's (rx_plan.hpp: CallFacts::omap): the output-map twins
// of the fused kernels, or the hand-over and a back kernel that knows the map.
#include <string>
#include <vector>

#include "rx_ctx.hpp"

using namespace t41;

extern "C" {

int t41rx_set_output_map(t41rx_ctx *ctx, const int32_t *row_of_channel, int n, int n_rows) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ", n_rows " + std::to_string(n_rows) + ")";
  if (!row_of_channel) {
    if (n != 0 || n_rows != 0) return fail(T41RX_ERR_ARG, "output map: a null map switches the map off and takes n 0 and n_rows 0" + counts);
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the map they found)
    ctx->out_map_on = false;
    ctx->out_rows = 0;
    ctx->out_listened = 0;
    return cw_filter_map_refresh(ctx);  // (a CW filter map's row maps name the channels' own rows again)
  }
  if (ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "the output map is built for fft_length 512 (the long-FFT pipeline's back kernel interpolates and stores every channel)");
  // everything is checked here, on the host, before anything changes: the kernels index the audio with these entries unchecked
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "output map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
  if (n_rows < 0 || n_rows > ctx->nchan) return fail(T41RX_ERR_ARG, "output map: n_rows must lie in [0, n_channels]" + counts);
  std::vector<int32_t> owner((size_t)n_rows, -1);  // the channel that names a row: two waves would store to one row
  int listened = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t r = row_of_channel[i];
    if (r == -1) continue;
    if (r < -1 || r >= n_rows)
      return fail(T41RX_ERR_ARG, "output map: channel " + std::to_string(i) + " names row " + std::to_string(r) + ", neither -1 nor in [0, n_rows)" + counts);
    if (owner[(size_t)r] >= 0)
      return fail(T41RX_ERR_ARG, "output map: channel " + std::to_string(i) + " names row " + std::to_string(r) + ", which channel " +
                                     std::to_string(owner[(size_t)r]) + " names already" + counts);
    owner[(size_t)r] = i;
    ++listened;
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<int32_t> fresh;  // (the first map; later ones reuse the buffer: a failure leaves the previous map whole)
  if (!ctx->d_out_map) HIP_TRY(dev_alloc(fresh, sizeof(int32_t) * (size_t)n));
  HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->d_out_map.get(), row_of_channel, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
  if (fresh) ctx->d_out_map = std::move(fresh);
  ctx->out_map.assign(row_of_channel, row_of_channel + n);
  ctx->out_rows = n_rows;
  ctx->out_listened = listened;
  ctx->out_map_on = true;
  return cw_filter_map_refresh(ctx);  // (a CW filter map's row maps follow the rows)
}

int t41rx_get_output_map(const t41rx_ctx *ctx, int32_t *row_of_channel_out, int n, int *n_rows_out) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (ctx->out_map_on && row_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "output map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    for (int i = 0; i < n; ++i) row_of_channel_out[i] = ctx->out_map[(size_t)i];
  }
  if (n_rows_out) *n_rows_out = audio_rows(ctx);
  return ctx->out_map_on ? 1 : 0;
}

int t41rx_audio_rows(const t41rx_ctx *ctx) { return ctx ? audio_rows(ctx) : fail(T41RX_ERR_ARG, "null argument"); }

}  // extern "C"
