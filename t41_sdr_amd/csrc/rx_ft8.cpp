// t41_sdr_amd/csrc/rx_ft8.cpp -- host side of FT8 receive up to the waterfall (ft8_kernel.hip): the stage of a process
// call, the entry for 12 kS/s audio (DEMOD_FT8_WAV), the stage's own state record, and the setters -- the FT8 map's among
// them (t41rx_set_ft8_map; its list is rx_ft8map.hpp's): with a map the stage and the audio entry launch the list forms of
// their kernels over the list's length, or nothing for an empty list.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {
namespace {

// the FT8 memory (power-on: every word zero -- syncFlag false, ft8_flag 0, an empty buffer) and arm_rfft_q15's tables
int ensure_ft8(t41rx_ctx *ctx) {
  if (ctx->ft8.d_state) return T41RX_OK;
  DevBuf<int32_t> st;
  DevBuf<uint32_t> tab;
  const size_t bytes = sizeof(int32_t) * kFt8Words * (size_t)ctx->nchan;
  if (dev_alloc(st, bytes) != hipSuccess || dev_alloc(tab, sizeof(uint32_t) * kFt8TabWords) != hipSuccess)
    return fail(T41RX_ERR_NOMEM, "FT8 state allocation failed");
  std::vector<uint32_t> h((size_t)kFt8TabWords);
  ft8_make_fft_tables(h.data());
  if (hipMemset(st.get(), 0, bytes) != hipSuccess ||
      hipMemcpy(tab.get(), h.data(), sizeof(uint32_t) * h.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(T41RX_ERR_HIP, "FT8 state upload failed");
  ctx->ft8.d_state = std::move(st);
  ctx->ft8.d_tab = std::move(tab);
  return T41RX_OK;
}

constexpr uint32_t kFt8Magic = 0x46313454u;  // "T41F"
constexpr size_t kFt8HeaderBytes = 32;
size_t ft8_record_bytes(const t41rx_ctx *ctx) { return kFt8HeaderBytes + sizeof(int32_t) * kFt8Words * (size_t)ctx->nchan; }

}  // namespace

int ft8_power_on(t41rx_ctx *ctx) {
  if (!ctx->ft8.d_state) return T41RX_OK;
  return hip_check(hipMemset(ctx->ft8.d_state.get(), 0, sizeof(int32_t) * kFt8Words * (size_t)ctx->nchan), "FT8 reset");
}

int ft8_prepare(t41rx_ctx *ctx, const CallPlan &plan, int n_frames, hipStream_t s) {
  if (ctx->ft8.map_on) {
    // an FT8 map: only the listed channels are asked, each for its own effective set (set 0, plain or staged sets alike)
    for (const Ft8Pair &e : ctx->ft8.list) {
      const int set = sets_loaded(ctx) ? ctx->sets.set_of[(size_t)e.channel] : 0;
      const t41rx_params &p = set ? ctx->sets.params[(size_t)set - 1] : ctx->params;
      if (p.mode != T41RX_DEMOD_USB)
        return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive: the firmware demodulates DEMOD_FT8 as USB (Process.cpp:616-617); channel " + std::to_string(e.channel) +
                                               " is listed in the FT8 map (row " + std::to_string(e.row) + ") and runs parameter set " + std::to_string(set) +
                                               ", whose mode is not T41RX_DEMOD_USB");
    }
  } else {
    if (ctx->params.mode != T41RX_DEMOD_USB)
      return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive: the firmware demodulates DEMOD_FT8 as USB (Process.cpp:616-617); this context's mode is not T41RX_DEMOD_USB");
    for (const t41rx_params &p : ctx->sets.params)  // (parameter sets without an FT8 map: FT8 runs on every channel)
      if (p.mode != T41RX_DEMOD_USB)
        return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive: the firmware demodulates DEMOD_FT8 as USB (Process.cpp:616-617); a loaded parameter set's mode is not T41RX_DEMOD_USB");
  }
  if (n_frames > ctx->ft8.frames) return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the FT8 status buffer was set with");
  if (const int rc = ensure_ft8(ctx)) return rc;
  if (plan.ft8_own_tap && n_frames > ctx->ft8.tap_frames) {
    // the demod tap of the context's own (grown on demand, kept)
    HIP_TRY(hipStreamSynchronize(s));
    ctx->ft8.tap_frames = 0;
    ctx->ft8.d_tap.reset();
    HIP_TRY(dev_alloc(ctx->ft8.d_tap, sizeof(float) * 256 * (size_t)n_frames * (size_t)ctx->nchan));
    ctx->ft8.tap_frames = n_frames;
  }
  return T41RX_OK;
}

// Process.cpp:627-685 on float_buffer_L as the demodulator and the AGC leave it, in front of the equalizer: the
// hand-over buffer when the call has one, else the demod tap (the plan's ft8_source).  The stage only reads the audio.
int ft8_run(t41rx_ctx *ctx, const CallPlan &plan, const RxArgs &a, int n_frames, hipStream_t s) {
  // what both forms of the kernel take (Ft8Args, and Ft8ListArgs with the list behind the same members)
  auto fill = [&](auto &f) {
    f.aud = plan.ft8_source == Ft8Source::handover ? a.aud_out : a.dbg_demod;
    f.state = ctx->ft8.d_state.get();
    f.power = ctx->ft8.power;
    f.status = ctx->ft8.status;
    f.window = ctx->ft8.d_win.get();
    f.mag_db = ctx->ft8.d_mag.get();
    f.tab = ctx->ft8.d_tab.get();
    f.nchan = ctx->nchan;
    f.nframes = n_frames;
    f.t0 = ctx->ft8.clock.t0;
    f.num = ctx->ft8.clock.num;
    f.den = ctx->ft8.clock.den;
  };
  if (ctx->ft8.map_on) {
    // the list form over the list's length; nobody listed: nothing to launch (a grid of zero blocks is a launch error)
    if (ctx->ft8.list.empty()) return T41RX_OK;
    Ft8ListArgs f{};
    fill(f);
    f.list = ctx->ft8.d_list.get();
    f.nlist = (int)ctx->ft8.list.size();
    return hip_check(launch_ft8_list(f, s), "FT8 list kernel launch");
  }
  Ft8Args f{};
  fill(f);
  return hip_check(launch_ft8(f, s), "FT8 kernel launch");
}

namespace {
// ---- FT8 from 12 kS/s audio (DEMOD_FT8_WAV) ----
// everything is checked before anything is allocated, launched or written
int ft8_audio_refusal(const t41rx_ctx *ctx, const void *pcm, int n_frames, unsigned align_mask) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!ctx->ft8.have_tables) return fail(T41RX_ERR_ARG, "FT8 audio: no tables loaded (t41rx_set_ft8_tables)");
  if (!ctx->ft8.on) return fail(T41RX_ERR_ARG, "FT8 audio: FT8 receive is off (t41rx_set_ft8: no d_power / d_status to write)");
  if (n_frames < 1) return fail(T41RX_ERR_ARG, "FT8 audio: n_frames must be >= 1");
  if (n_frames > T41RX_FT8_MAX_FRAMES) return fail(T41RX_ERR_ARG, "FT8 audio: n_frames must be <= 1380 (at most one completed slot per call)");
  if (n_frames > ctx->ft8.frames) return fail(T41RX_ERR_ARG, "FT8 audio: n_frames exceeds the max_frames the FT8 status buffer was set with");
  if (!pcm) return fail(T41RX_ERR_ARG, "FT8 audio: no samples (NULL pointer)");
  if (reinterpret_cast<uintptr_t>(pcm) & align_mask) return fail(T41RX_ERR_ARG, "FT8 audio: the sample pointer is not aligned to its type");
  return T41RX_OK;
}

int ft8_audio_device(t41rx_ctx *ctx, const void *d_pcm, int n_frames, bool q15) {
  if (const int rc = ft8_audio_refusal(ctx, d_pcm, n_frames, q15 ? 1u : 3u)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  if (const int rc = ensure_ft8(ctx)) return rc;
  auto fill = [&](auto &a) {
    a.pcm = d_pcm;
    a.state = ctx->ft8.d_state.get();
    a.power = ctx->ft8.power;
    a.status = ctx->ft8.status;
    a.window = ctx->ft8.d_win.get();
    a.mag_db = ctx->ft8.d_mag.get();
    a.tab = ctx->ft8.d_tab.get();
    a.nchan = ctx->nchan;
    a.nframes = n_frames;
    a.q15 = q15 ? 1 : 0;
  };
  if (ctx->ft8.map_on) {
    // pcm, d_power and d_status by row; a row nobody names is not read, and nobody listed launches nothing
    if (ctx->ft8.list.empty()) return T41RX_OK;
    Ft8AudioListArgs a{};
    fill(a);
    a.list = ctx->ft8.d_list.get();
    a.nlist = (int)ctx->ft8.list.size();
    return hip_check(launch_ft8_audio_list(a, nullptr), "FT8 audio list kernel launch");
  }
  Ft8AudioArgs a{};
  fill(a);
  return hip_check(launch_ft8_audio(a, nullptr), "FT8 audio kernel launch");
}

int ft8_audio_host(t41rx_ctx *ctx, const void *pcm, int n_frames, bool q15) {
  if (const int rc = ft8_audio_refusal(ctx, pcm, n_frames, q15 ? 1u : 3u)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const size_t row_bytes = (size_t)n_frames * kFt8AudioFrame * (q15 ? sizeof(int16_t) : sizeof(float));
  const size_t bytes = (size_t)ft8_rows(ctx) * row_bytes;
  if (ctx->ft8.map_on && ctx->ft8.list.empty()) return T41RX_OK;  // (nobody listed: no row is read)
  DevBuf<char> staged;
  if (dev_alloc(staged, bytes) != hipSuccess) return fail(T41RX_ERR_NOMEM, "FT8 audio: staging allocation failed");
  if (ctx->ft8.map_on && (int)ctx->ft8.list.size() < ctx->ft8.rows) {
    for (const Ft8Pair &e : ctx->ft8.list)  // (a row nobody names is not read)
      HIP_TRY(hipMemcpy(staged.get() + (size_t)e.row * row_bytes, static_cast<const char *>(pcm) + (size_t)e.row * row_bytes, row_bytes, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(staged.get(), pcm, bytes, hipMemcpyHostToDevice));
  }
  if (const int rc = ft8_audio_device(ctx, staged.get(), n_frames, q15)) return rc;
  HIP_TRY(hipDeviceSynchronize());  // (the staging buffer is read until the kernel ends)
  return T41RX_OK;
}

int ft8_audio_mark(t41rx_ctx *ctx, const uint8_t *channels, int n, int end) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (channels && n != ctx->nchan) return fail(T41RX_ERR_ARG, "n must equal n_channels");
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive is built for fft_length 512");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = ensure_ft8(ctx)) return rc;
  DevBuf<uint8_t> mask;
  if (const int rc = upload_channel_mask(ctx, channels, mask)) return rc;
  HIP_TRY(launch_ft8_audio_mark(ctx->ft8.d_state.get(), mask.get(), ctx->nchan, end, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return T41RX_OK;
}
}  // namespace

}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_set_ft8_tables(t41rx_ctx *ctx, const float *window, const float *mag_db) {
  if (!ctx || !window || !mag_db) return fail(T41RX_ERR_ARG, "null argument");
  for (int i = 0; i < kFt8Fft; ++i)
    if (!std::isfinite(window[i])) return fail(T41RX_ERR_ARG, "FT8 window: non-finite entry");
  for (int i = 0; i < kFt8MagEntries; ++i)
    if (!std::isfinite(mag_db[i])) return fail(T41RX_ERR_ARG, "FT8 mag_db table: non-finite entry");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old tables)
  if (!ctx->ft8.d_win) HIP_TRY(dev_alloc(ctx->ft8.d_win, sizeof(float) * kFt8Fft));
  if (!ctx->ft8.d_mag) HIP_TRY(dev_alloc(ctx->ft8.d_mag, sizeof(float) * kFt8MagEntries));
  HIP_TRY(hipMemcpy(ctx->ft8.d_win.get(), window, sizeof(float) * kFt8Fft, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->ft8.d_mag.get(), mag_db, sizeof(float) * kFt8MagEntries, hipMemcpyHostToDevice));
  ctx->ft8.have_tables = true;
  return T41RX_OK;
}

int t41rx_set_ft8(t41rx_ctx *ctx, int on, uint8_t *d_power, int32_t *d_status, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (on != 0 && on != 1) return fail(T41RX_ERR_ARG, "FT8 receive: on must be 0 or 1");
  if (on) {
    if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive is built for fft_length 512");
    if (!d_power || !d_status) return fail(T41RX_ERR_ARG, "FT8 receive: no power or status buffer (d_power / d_status is NULL)");
    if (reinterpret_cast<uintptr_t>(d_status) & 15u) return fail(T41RX_ERR_ARG, "FT8 receive: d_status must be 16-byte aligned");
    if (max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
    if (max_frames > kFt8MaxFrames)
      return fail(T41RX_ERR_ARG, "FT8 receive: max_frames must be <= 1380 (92 blocks of 15 frames: at most one completed slot per call)");
    if (!ctx->ft8.have_tables) return fail(T41RX_ERR_ARG, "FT8 receive: no tables loaded (t41rx_set_ft8_tables)");
  }
  ctx->ft8.on = on;
  ctx->ft8.power = on ? d_power : nullptr;
  ctx->ft8.status = on ? d_status : nullptr;
  ctx->ft8.frames = on ? max_frames : 0;
  return T41RX_OK;
}
int t41rx_get_ft8(const t41rx_ctx *ctx) { return ctx ? ctx->ft8.on : T41RX_ERR_ARG; }

// The FT8 map.  Everything is checked here, on the host, before anything changes: the list kernels index every buffer
// with the pairs unchecked.  A refused call leaves the previous map whole.
int t41rx_set_ft8_map(t41rx_ctx *ctx, const int32_t *row_of_channel, int n, int n_rows) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ", FT8 rows " + std::to_string(ft8_rows(ctx)) + ")";
  const std::string resize = ": FT8 receive is on and its d_power / d_status are sized by the rows; switch FT8 off, set the map, "
                             "and switch FT8 on with buffers of the new size";
  if (!row_of_channel) {
    if (n != 0 || n_rows != 0) return fail(T41RX_ERR_ARG, "FT8 map: a null map removes the map and takes n 0 and n_rows 0" + counts);
    if (ctx->ft8.on && ft8_rows(ctx) != ctx->nchan)
      return fail(T41RX_ERR_ARG, "FT8 map: removing the map would change the rows from " + std::to_string(ft8_rows(ctx)) + " to n_channels" + resize + counts);
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the list they found)
    ctx->ft8.map_on = false;
    return T41RX_OK;
  }
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "FT8 map: FT8 receive is built for fft_length 512");
  std::vector<Ft8Pair> list;
  const Ft8MapVerdict v = build_ft8_list(row_of_channel, n, n_rows, ctx->nchan, ctx->ft8.on ? ft8_rows(ctx) : 0, list);
  switch (v.fault) {
    case Ft8MapFault::none:
      break;
    case Ft8MapFault::count:
    case Ft8MapFault::null_map:
      return fail(T41RX_ERR_ARG, "FT8 map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
    case Ft8MapFault::rows:
      return fail(T41RX_ERR_ARG, "FT8 map: n_rows (" + std::to_string(n_rows) + ") must be 1 .. n_channels" + counts);
    case Ft8MapFault::entry:
      return fail(T41RX_ERR_ARG, "FT8 map: channel " + std::to_string(v.channel) + " has row " + std::to_string(row_of_channel[v.channel]) +
                                     ", outside [-1, n_rows " + std::to_string(n_rows) + ")" + counts);
    case Ft8MapFault::twice:
      return fail(T41RX_ERR_ARG, "FT8 map: row " + std::to_string(row_of_channel[v.channel]) + " is named twice, by channel " + std::to_string(v.other) +
                                     " and channel " + std::to_string(v.channel) + counts);
    case Ft8MapFault::resize:
      return fail(T41RX_ERR_ARG, "FT8 map: n_rows (" + std::to_string(n_rows) + ") differs from the current rows" + resize + counts);
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<Ft8Pair> fresh;  // (the first map; later ones reuse the buffer: a failure leaves the previous map whole)
  if (!ctx->ft8.d_list) HIP_TRY(dev_alloc(fresh, sizeof(Ft8Pair) * (size_t)ctx->nchan));
  if (!list.empty())
    HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->ft8.d_list.get(), list.data(), sizeof(Ft8Pair) * list.size(), hipMemcpyHostToDevice));
  if (fresh) ctx->ft8.d_list = std::move(fresh);
  ctx->ft8.map.assign(row_of_channel, row_of_channel + n);
  ctx->ft8.list = std::move(list);
  ctx->ft8.rows = n_rows;
  ctx->ft8.map_on = true;
  return T41RX_OK;
}

int t41rx_get_ft8_map(const t41rx_ctx *ctx, int32_t *row_of_channel_out, int n, int *n_rows_out) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (row_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "FT8 map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    for (int i = 0; i < n; ++i) row_of_channel_out[i] = ctx->ft8.map_on ? ctx->ft8.map[(size_t)i] : i;
  }
  if (n_rows_out) *n_rows_out = ft8_rows(ctx);
  return ctx->ft8.map_on ? 1 : 0;
}

int t41rx_ft8_rows(const t41rx_ctx *ctx) { return ctx ? ft8_rows(ctx) : T41RX_ERR_ARG; }

int t41rx_set_ft8_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  return set_stage_clock(ctx->ft8.clock, "FT8", t0_ms, num, den);
}

int t41rx_ft8_sync(t41rx_ctx *ctx, const uint8_t *channels, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (channels && n != ctx->nchan) return fail(T41RX_ERR_ARG, "n must equal n_channels");
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive is built for fft_length 512");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = ensure_ft8(ctx)) return rc;
  DevBuf<uint8_t> mask;
  if (const int rc = upload_channel_mask(ctx, channels, mask)) return rc;
  const StageClock &k = ctx->ft8.clock;
  HIP_TRY(launch_ft8_sync(ctx->ft8.d_state.get(), mask.get(), ctx->nchan, k.t0, k.num, k.den, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return T41RX_OK;
}

size_t t41rx_ft8_state_bytes(const t41rx_ctx *ctx) { return ctx ? ft8_record_bytes(ctx) : 0; }

int t41rx_ft8_get_state(t41rx_ctx *ctx, void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  if (bytes < ft8_record_bytes(ctx)) return fail(T41RX_ERR_STATE, "FT8 state buffer too small");
  const int32_t hdr[8] = {(int32_t)kFt8Magic, T41RX_ABI_VERSION, ctx->nchan, kFt8Words, 0, 0, 0, 0};
  std::memcpy(host_buf, hdr, sizeof(hdr));
  char *body = static_cast<char *>(host_buf) + kFt8HeaderBytes;
  const size_t n = ft8_record_bytes(ctx) - kFt8HeaderBytes;
  if (!ctx->ft8.d_state) {  // the stage has not run: its words are the power-on ones
    std::memset(body, 0, n);
    return T41RX_OK;
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(body, ctx->ft8.d_state.get(), n, hipMemcpyDeviceToHost));
  return T41RX_OK;
}

int t41rx_ft8_set_state(t41rx_ctx *ctx, const void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive is built for fft_length 512");
  if (bytes != ft8_record_bytes(ctx)) return fail(T41RX_ERR_STATE, "FT8 state size mismatch");
  int32_t hdr[8];
  std::memcpy(hdr, host_buf, sizeof(hdr));
  if ((uint32_t)hdr[0] != kFt8Magic || hdr[1] != T41RX_ABI_VERSION || hdr[2] != ctx->nchan || hdr[3] != kFt8Words)
    return fail(T41RX_ERR_STATE, "FT8 state header does not match this context (magic / abi / channels / words per channel)");
  // what ft8_kernel indexes, loops or branches with; everything is checked before anything is written
  const int32_t *all = reinterpret_cast<const int32_t *>(static_cast<const char *>(host_buf) + kFt8HeaderBytes);
  for (int ch = 0; ch < ctx->nchan; ++ch) {
    const int32_t *w = all + (size_t)kFt8Words * (size_t)ch;
    if (w[kFt8DataLoop] < 0 || w[kFt8DataLoop] > 14) return fail(T41RX_ERR_STATE, "FT8 state: dataLoop out of range (0 .. 14)");
    if (w[kFt8Leftover] < 0 || w[kFt8Leftover] > 3) return fail(T41RX_ERR_STATE, "FT8 state: leftover out of range (0 .. 3)");
    for (int k : {kFt8Sync, kFt8Flag, kFt8DspFlag, kFt8Half})
      if (w[k] != 0 && w[k] != 1) return fail(T41RX_ERR_STATE, "FT8 state: flag (syncFlag, ft8_flag, DSP_Flag, half) not 0 or 1");
    // (the firmware leaves FT_8_counter at 92 between a slot's last block and the restart, with ft8_flag 0: it indexes nothing then)
    if (w[kFt8Counter] < 0 || w[kFt8Counter] > (w[kFt8Flag] == 0 ? kFt8SlotBlocks : kFt8SlotBlocks - 1))
      return fail(T41RX_ERR_STATE, "FT8 state: FT_8_counter out of range (0 .. 91)");
    for (int k = kFt8Named; k < kFt8Scalars; ++k)
      if (w[k] != 0) return fail(T41RX_ERR_STATE, "FT8 state: reserved word not zero");
    for (int k = kFt8Scalars; k < kFt8Words; ++k)
      if (w[k] < -32768 || w[k] > 32767) return fail(T41RX_ERR_STATE, "FT8 state: buffer word is not a q15 sample");
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = ensure_ft8(ctx)) return rc;
  HIP_TRY(hipMemcpy(ctx->ft8.d_state.get(), all, bytes - kFt8HeaderBytes, hipMemcpyHostToDevice));
  return T41RX_OK;
}

int t41rx_ft8_audio_device_q15(t41rx_ctx *ctx, const int16_t *d_pcm, int n_frames) { return ft8_audio_device(ctx, d_pcm, n_frames, true); }
int t41rx_ft8_audio_device(t41rx_ctx *ctx, const float *d_audio, int n_frames) { return ft8_audio_device(ctx, d_audio, n_frames, false); }
int t41rx_ft8_audio_host_q15(t41rx_ctx *ctx, const int16_t *pcm, int n_frames) { return ft8_audio_host(ctx, pcm, n_frames, true); }
int t41rx_ft8_audio_host(t41rx_ctx *ctx, const float *audio, int n_frames) { return ft8_audio_host(ctx, audio, n_frames, false); }
int t41rx_ft8_audio_begin(t41rx_ctx *ctx, const uint8_t *channels, int n) { return ft8_audio_mark(ctx, channels, n, 0); }
int t41rx_ft8_audio_end(t41rx_ctx *ctx, const uint8_t *channels, int n) { return ft8_audio_mark(ctx, channels, n, 1); }

}  // extern "C"
