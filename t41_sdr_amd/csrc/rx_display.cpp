// t41_sdr_amd/csrc/rx_display.cpp -- host side of the display stages behind a process call: the display FFT side output
// (display_kernel.hip) and the panadapter stage (panadapter_kernel.hip), with the window and the zoom filters they share
// with the calibration -- and the panadapter map (t41rx_set_panadapter_map; its list is rx_panmap.hpp's): with a map the
// stage launches the list form of its kernel over the list's length, or nothing for an empty list.
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {

void zoom_filter_args(int zoom, float (&iir)[20], float (&fir)[4]) {
  if (zoom > 0) {
    std::memcpy(iir, kZoomIirCoeffs[zoom - 1], sizeof(iir));
    design_zoom_fir(zoom, fir);
  }
}

// the display FFT's window, 0.5 - 0.5 cos(6.28 i / 512) as the reference's double expression, once per context
int ensure_window(t41rx_ctx *ctx) {
  if (ctx->d_win) return T41RX_OK;
  DevBuf<double> win;
  double w[512];
  for (int i = 0; i < 512; ++i) w[i] = 0.5 - 0.5 * std::cos(6.28 * i / 512);  // FFT.cpp:110, 222 ("Hanning", 6.28 as written)
  HIP_TRY(dev_alloc(win, sizeof(w)));
  HIP_TRY(hipMemcpy(win.get(), w, sizeof(w), hipMemcpyHostToDevice));
  ctx->d_win = std::move(win);
  return T41RX_OK;
}

// ---- display FFT side output
// refusal of its checkpoint section
int display_check(const t41rx_ctx *c, const int32_t *hdr, const float *d) {
  if (!(c->disp.spec && c->disp.d_state)) return fail(T41RX_ERR_STATE, "checkpoint carries display-FFT state but the display spectrum is off here");
  if (hdr[6] != c->disp.zoom) return fail(T41RX_ERR_STATE, "checkpoint: display-FFT state of another spectrumZoom");
  for (int ch = 0; ch < c->nchan; ++ch) {
    int32_t ptr;
    std::memcpy(&ptr, d + (size_t)kDispFloats * (size_t)ch + kDispPtr, sizeof(ptr));
    if (ptr < 0 || ptr >= 512) return fail(T41RX_ERR_STATE, "checkpoint: zoom_sample_ptr out of range");
  }
  return T41RX_OK;
}

int display_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  DispArgs d{};
  d.pre = ctx->disp.d_pre.get();
  d.disp = ctx->disp.d_state.get();
  d.spec = ctx->disp.spec;
  d.spec_old = ctx->disp.old;
  d.tab = ctx->d_tab.get();
  d.win = ctx->d_win.get();
  d.nchan = ctx->nchan;
  d.nframes = n_frames;
  d.zoom = ctx->disp.zoom;
  zoom_filter_args(d.zoom, d.iir, d.fir);
  return hip_check(launch_display(d, s), "display kernel launch");
}

// ---- panadapter
int pan_prepare(t41rx_ctx *ctx, int n_frames) {
  Panadapter &p = ctx->pan;
  p.call_rows = 0;
  p.call_first = n_frames;
  if (!p.on) return T41RX_OK;
  // (parameter sets: DrawSmeterBar()'s dBm takes the two gains by value, one pair per launch -- but under a panadapter
  // map, whose list carries every listed channel's own pair)
  if (p.out.smeter && !p.map_on)
    for (const t41rx_params &s : ctx->sets.params)
      if (s.RFgain != ctx->params.RFgain || s.rfGainAllBands != ctx->params.rfGainAllBands)
        return fail(T41RX_ERR_UNSUPPORTED, "panadapter: the S-meter's dBm reads one RFgain / rfGainAllBands per context and a loaded "
                                               "parameter set differs from set 0 in them; drop the smeter rows or give the sets equal gains");
  p.call_rows = pan_rows_of_call(p.counter, n_frames, p.period, p.phase, &p.call_first);
  if (p.call_rows > p.max_rows)
    return fail(T41RX_ERR_ARG, "the call holds more update frames than the max_rows the panadapter buffers were set with");
  if (!p.d_pre || !p.d_max || !p.d_mem || !p.d_nf || !p.d_gc || !p.d_grad || !ctx->d_win)
    return fail(T41RX_ERR_STATE, "panadapter enabled without its buffers");
  return T41RX_OK;
}

int pan_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  Panadapter &pan = ctx->pan;
  // what both forms of the kernel take (PanArgs, and PanListArgs with the list behind the same members)
  auto fill = [&](auto &p) {
    p.pre = pan.d_pre.get();
    p.mx = pan.d_max.get();
    p.mem = pan.d_mem.get();
    p.tab = ctx->d_tab.get();
    p.win = ctx->d_win.get();
    p.gradient = pan.d_grad.get();
    p.noise_floor = pan.d_nf.get();
    p.gain_correction = pan.d_gc.get();
    p.pixel = pan.out.pixel;
    p.y_new = pan.out.y_new;
    p.y_old = pan.out.y_old;
    p.waterfall = pan.out.waterfall;
    p.spec = pan.out.spec;
    p.smeter = pan.out.smeter;
    p.nchan = ctx->nchan;
    p.nrows = pan.call_rows;
    p.max_rows = pan.max_rows;
    p.zoom = pan.zoom;
    zoom_filter_args(p.zoom, p.iir, p.fir);
    p.dBScale = kDbScale[pan.scale];
    p.base = kBaseOffset[pan.scale] + pan.pixel_offset;
    p.noise_floor_y = pan.floor_y;
    p.attenuator = pan.attenuator;
    p.RFgain = ctx->params.RFgain;
    p.rfGainAllBands = ctx->params.rfGainAllBands;
  };
  if (pan.call_rows > 0 && pan.map_on) {
    // the list form over the list's length; nobody listed: nothing to launch (the call wrote no tap either)
    if (!pan.list.empty()) {
      PanListArgs p{};
      fill(p);
      p.list = pan.d_list.get();
      p.nlist = (int)pan.list.size();
      const hipError_t e = launch_panadapter_list(p, s);
      if (e != hipSuccess) return hip_fail(e, "panadapter list kernel launch");
    }
  } else if (pan.call_rows > 0) {
    PanArgs p{};
    fill(p);
    const hipError_t e = launch_panadapter(p, s);
    if (e != hipSuccess) return hip_fail(e, "panadapter kernel launch");
  }
  // (under a map: the rows every listed channel wrote)
  pan.last_rows = pan.call_rows;
  pan.last_first = pan.call_rows > 0 ? pan.counter + pan.call_first : -1;
  pan.counter += n_frames;
  return T41RX_OK;
}

// DrawSmeterBar()'s two gains of every set, [K + 1] with set 0 first, and the channels' table (null: no sets): what
// rx_panmap.hpp makes the list's entries of
namespace {
std::vector<PanGains> pan_gains(const t41rx_ctx *ctx) {
  std::vector<PanGains> gains{PanGains{ctx->params.RFgain, ctx->params.rfGainAllBands}};
  for (const t41rx_params &s : ctx->sets.params) gains.push_back(PanGains{s.RFgain, s.rfGainAllBands});
  return gains;
}
const int32_t *pan_set_of(const t41rx_ctx *ctx) { return sets_loaded(ctx) ? ctx->sets.set_of.data() : nullptr; }
}  // namespace

// the parameter sets or set 0 changed (behind the setter's device synchronisation): the listed channels' gains follow
int pan_map_refresh(t41rx_ctx *ctx) {
  Panadapter &pan = ctx->pan;
  if (!pan.map_on) return T41RX_OK;
  std::vector<PanEntry> list = pan_list_of(pan.map.data(), ctx->nchan, pan_gains(ctx).data(), pan_set_of(ctx));
  if (!list.empty()) HIP_TRY(hipMemcpy(pan.d_list.get(), list.data(), sizeof(PanEntry) * list.size(), hipMemcpyHostToDevice));
  pan.list = std::move(list);
  return T41RX_OK;
}

// t41rx_reset(): the panadapter memory and its frame counter to power-on (pixelold = 0, newSpectrumFlag = 0)
int pan_reset(t41rx_ctx *ctx) {
  if (ctx->pan.d_mem) HIP_TRY(hipMemset(ctx->pan.d_mem.get(), 0, sizeof(float) * kPanFloats * (size_t)ctx->nchan));
  ctx->pan.counter = 0;
  ctx->pan.last_rows = 0;
  ctx->pan.last_first = -1;
  return T41RX_OK;
}

namespace {
// the per-channel levels, on the device; values == nullptr: zeros
template <class T>
int pan_upload_levels(t41rx_ctx *ctx, DevBuf<T> &d, const T *values) {
  std::vector<T> h((size_t)ctx->nchan, T(0));
  if (values) std::memcpy(h.data(), values, sizeof(T) * h.size());
  if (!d) HIP_TRY(dev_alloc(d, sizeof(T) * h.size()));
  HIP_TRY(hipMemcpy(d.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}
}  // namespace

}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_set_display_spectrum(t41rx_ctx *ctx, float *d_spec, float *d_spec_old, int spectrumZoom, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null context");
  if ((d_spec == nullptr) != (d_spec_old == nullptr)) return fail(T41RX_ERR_ARG, "set both pointers or neither");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  DisplayTap &disp = ctx->disp;
  if (!d_spec) {
    disp.spec = disp.old = nullptr;
    disp.frames = 0;
    return T41RX_OK;
  }
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the display FFT is built for fft_length 512");
  if (ctx->pan.on) return fail(T41RX_ERR_UNSUPPORTED, "the panadapter stage is on and owns the display tap (t41rx_set_panadapter)");
  if (spectrumZoom < 0 || spectrumZoom > 4) return fail(T41RX_ERR_ARG, "spectrumZoom must be 0 (1x) .. 4 (16x)");  // MAX_ZOOM_ENTRIES, ButtonProc.h:6
  if (max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
  if ((reinterpret_cast<uintptr_t>(d_spec) | reinterpret_cast<uintptr_t>(d_spec_old)) & 3u) return fail(T41RX_ERR_ARG, "unaligned pointer");
  // Anything that fails from here on leaves the side output switched OFF (a previous successful
  // call's pointers must not survive next to a freed tap buffer: the display kernel would read it).
  disp.spec = disp.old = nullptr;
  const int had_frames = disp.frames;
  disp.frames = 0;
  if (max_frames > had_frames || !disp.d_pre)
    HIP_TRY(dev_alloc(disp.d_pre, sizeof(float) * 4096 * (size_t)max_frames * (size_t)ctx->nchan));
  if (!disp.d_state) HIP_TRY(dev_alloc(disp.d_state, sizeof(float) * kDispFloats * (size_t)ctx->nchan));
  if (const int rc = ensure_window(ctx)) return rc;
  HIP_TRY(hipMemset(disp.d_state.get(), 0, sizeof(float) * kDispFloats * (size_t)ctx->nchan));  // ZoomFFTPrep(): a fresh start
  if (max_frames < had_frames) max_frames = had_frames;  // (the tap buffer was kept: it still holds that many)
  disp.spec = d_spec;
  disp.old = d_spec_old;
  disp.frames = max_frames;
  disp.zoom = spectrumZoom;
  return T41RX_OK;
}

int t41rx_set_panadapter_tables(t41rx_ctx *ctx, const uint16_t *gradient, int n) {
  if (!ctx || !gradient) return fail(T41RX_ERR_ARG, "null argument");
  if (n != kPanGradient) return fail(T41RX_ERR_ARG, "panadapter tables: gradient[] has 117 words (Display.cpp:148-161)");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old table)
  if (!ctx->pan.d_grad) HIP_TRY(dev_alloc(ctx->pan.d_grad, sizeof(uint16_t) * kPanGradient));
  HIP_TRY(hipMemcpy(ctx->pan.d_grad.get(), gradient, sizeof(uint16_t) * kPanGradient, hipMemcpyHostToDevice));
  ctx->pan.have_tables = true;
  return T41RX_OK;
}

int t41rx_set_panadapter(t41rx_ctx *ctx, int on, int spectrumZoom, int currentScale, int pixel_offset, int spectrumNoiseFloor,
                         int update_period, int update_phase, const t41rx_panadapter_out *out, int max_rows) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  Panadapter &pan = ctx->pan;
  if (!on) {
    if (ctx->beacon.on) return fail(T41RX_ERR_UNSUPPORTED, "the beacon monitor is on and reads the panadapter's rows: switch it off first (t41rx_set_beacon)");
    pan.on = false;
    return T41RX_OK;
  }
  // every refusal in front of the first change: a refused call leaves the stage as it was
  if (!out) return fail(T41RX_ERR_ARG, "null argument");
  if (ctx->beacon.on && !out->smeter)
    return fail(T41RX_ERR_UNSUPPORTED, "the beacon monitor is on and reads the smeter rows: switch it off first (t41rx_set_beacon)");
  if (ctx->beacon.on && max_rows > ctx->beacon.max_rows)
    return fail(T41RX_ERR_ARG, "max_rows exceeds the max_rows the beacon monitor's buffers were set with");
  if (!pan.have_tables) return fail(T41RX_ERR_ARG, "panadapter: no colour table loaded (t41rx_set_panadapter_tables)");
  if (spectrumZoom < 0 || spectrumZoom > 4) return fail(T41RX_ERR_ARG, "spectrumZoom must be 0 (1x) .. 4 (16x)");
  if (currentScale < 0 || currentScale > 4) return fail(T41RX_ERR_ARG, "currentScale must be 0 .. 4");
  if (pixel_offset < -32768 || pixel_offset > 32767) return fail(T41RX_ERR_ARG, "pixel_offset must fit an int16");
  if (spectrumNoiseFloor < -32768 || spectrumNoiseFloor > 32767) return fail(T41RX_ERR_ARG, "spectrumNoiseFloor must fit an int16");
  if (update_period < 1) return fail(T41RX_ERR_ARG, "update_period must be >= 1");
  if (update_phase < 0 || update_phase >= update_period) return fail(T41RX_ERR_ARG, "update_phase must lie in [0, update_period)");
  if (max_rows < 1) return fail(T41RX_ERR_ARG, "max_rows must be >= 1");
  if ((reinterpret_cast<uintptr_t>(out->pixel) | reinterpret_cast<uintptr_t>(out->y_new) | reinterpret_cast<uintptr_t>(out->y_old) |
       reinterpret_cast<uintptr_t>(out->waterfall) | reinterpret_cast<uintptr_t>(out->spec) | reinterpret_cast<uintptr_t>(out->audio_spect) |
       reinterpret_cast<uintptr_t>(out->smeter)) & 15u)
    return fail(T41RX_ERR_ARG, "panadapter: the row buffers must be 16-byte aligned");  // (one rule for all: the audio-spectrum rows leave as 8-byte stores)
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the panadapter stage is built for fft_length 512");
  if (ctx->disp.spec || ctx->spect)
    return fail(T41RX_ERR_UNSUPPORTED, "t41rx_set_display_spectrum / t41rx_set_audio_spectrum is set and owns its tap: switch it off first");
  // anything that fails from here on leaves the stage switched off
  pan.on = false;
  // the taps, sized by the rows: one per channel, or the panadapter map's n_rows
  const int width = pan_rows(ctx);
  if (max_rows > pan.alloc_rows || width != pan.alloc_width || !pan.d_pre || !pan.d_max) {
    pan.alloc_rows = pan.alloc_width = 0;
    pan.d_pre.reset();
    pan.d_max.reset();
    HIP_TRY(dev_alloc(pan.d_pre, sizeof(float) * 4096 * (size_t)max_rows * (size_t)width));
    HIP_TRY(dev_alloc(pan.d_max, sizeof(float) * 3 * (size_t)max_rows * (size_t)width));
    pan.alloc_rows = max_rows;
    pan.alloc_width = width;
  }
  if (!pan.d_mem) HIP_TRY(dev_alloc(pan.d_mem, sizeof(float) * kPanFloats * (size_t)ctx->nchan));
  if (const int rc = ensure_window(ctx)) return rc;
  if (!pan.d_nf)
    if (const int rc = pan_upload_levels<int32_t>(ctx, pan.d_nf, nullptr)) return rc;
  if (!pan.d_gc)
    if (const int rc = pan_upload_levels<float>(ctx, pan.d_gc, nullptr)) return rc;
  // power-on: ZoomFFTPrep(), FFT_spec_old = 0, pixelold = 0, newSpectrumFlag = 0; the frame counter starts at 0
  HIP_TRY(hipMemset(pan.d_mem.get(), 0, sizeof(float) * kPanFloats * (size_t)ctx->nchan));
  pan.out = *out;
  pan.zoom = spectrumZoom;
  pan.scale = currentScale;
  pan.pixel_offset = pixel_offset;
  pan.floor_y = spectrumNoiseFloor;
  pan.period = update_period;
  pan.phase = update_phase;
  pan.max_rows = max_rows;
  pan.counter = 0;
  pan.last_rows = 0;
  pan.last_first = -1;
  pan.on = true;
  return T41RX_OK;
}

// The panadapter map.  Everything is checked here, on the host, before anything changes: the tap instantiations and the
// list kernels index every buffer with the rows unchecked.  A refused call leaves the previous map whole.
int t41rx_set_panadapter_map(t41rx_ctx *ctx, const int32_t *row_of_channel, int n, int n_rows) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  Panadapter &pan = ctx->pan;
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ", panadapter rows " + std::to_string(pan_rows(ctx)) + ")";
  const std::string resize = ": the panadapter is on and its row buffers are sized by the rows; switch the beacon monitor and the "
                             "panadapter off, set the map, and switch them on with buffers of the new size";
  if (!row_of_channel) {
    if (n != 0 || n_rows != 0) return fail(T41RX_ERR_ARG, "panadapter map: a null map removes the map and takes n 0 and n_rows 0" + counts);
    if (pan.on && pan_rows(ctx) != ctx->nchan)
      return fail(T41RX_ERR_ARG, "panadapter map: removing the map would change the rows from " + std::to_string(pan_rows(ctx)) + " to n_channels" + resize + counts);
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the list they found)
    pan.map_on = false;
    return T41RX_OK;
  }
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "panadapter map: the panadapter stage is built for fft_length 512");
  std::vector<PanEntry> list;
  const PanMapVerdict v = build_pan_list(row_of_channel, n, n_rows, ctx->nchan, pan.on ? pan_rows(ctx) : 0, pan_gains(ctx).data(), pan_set_of(ctx), list);
  switch (v.fault) {
    case PanMapFault::none:
      break;
    case PanMapFault::count:
    case PanMapFault::null_map:
      return fail(T41RX_ERR_ARG, "panadapter map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
    case PanMapFault::rows:
      return fail(T41RX_ERR_ARG, "panadapter map: n_rows (" + std::to_string(n_rows) + ") must be 1 .. n_channels" + counts);
    case PanMapFault::entry:
      return fail(T41RX_ERR_ARG, "panadapter map: channel " + std::to_string(v.channel) + " has row " + std::to_string(row_of_channel[v.channel]) +
                                     ", outside [-1, n_rows " + std::to_string(n_rows) + ")" + counts);
    case PanMapFault::twice:
      return fail(T41RX_ERR_ARG, "panadapter map: row " + std::to_string(row_of_channel[v.channel]) + " is named twice, by channel " + std::to_string(v.other) +
                                     " and channel " + std::to_string(v.channel) + counts);
    case PanMapFault::resize:
      return fail(T41RX_ERR_ARG, "panadapter map: n_rows (" + std::to_string(n_rows) + ") differs from the current rows" + resize + counts);
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<PanEntry> fresh_list;  // (the first map; later ones reuse the buffers: a failure leaves the previous map whole)
  DevBuf<int32_t> fresh_map;
  if (!pan.d_list) HIP_TRY(dev_alloc(fresh_list, sizeof(PanEntry) * (size_t)ctx->nchan));
  if (!pan.d_map) HIP_TRY(dev_alloc(fresh_map, sizeof(int32_t) * (size_t)ctx->nchan));
  if (!list.empty())
    HIP_TRY(hipMemcpy(fresh_list ? fresh_list.get() : pan.d_list.get(), list.data(), sizeof(PanEntry) * list.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(fresh_map ? fresh_map.get() : pan.d_map.get(), row_of_channel, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
  if (fresh_list) pan.d_list = std::move(fresh_list);
  if (fresh_map) pan.d_map = std::move(fresh_map);
  pan.map.assign(row_of_channel, row_of_channel + n);
  pan.list = std::move(list);
  pan.rows = n_rows;
  pan.map_on = true;
  return T41RX_OK;
}

int t41rx_get_panadapter_map(const t41rx_ctx *ctx, int32_t *row_of_channel_out, int n, int *n_rows_out) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (row_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "panadapter map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    for (int i = 0; i < n; ++i) row_of_channel_out[i] = ctx->pan.map_on ? ctx->pan.map[(size_t)i] : i;
  }
  if (n_rows_out) *n_rows_out = pan_rows(ctx);
  return ctx->pan.map_on ? 1 : 0;
}

int t41rx_panadapter_rows(const t41rx_ctx *ctx) { return ctx ? pan_rows(ctx) : T41RX_ERR_ARG; }

int t41rx_set_panadapter_levels(t41rx_ctx *ctx, const int32_t *noise_floor, const float *gain_correction, int attenuator) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  for (int c = 0; noise_floor && c < ctx->nchan; ++c)
    if (noise_floor[c] < -32768 || noise_floor[c] > 32767) return fail(T41RX_ERR_ARG, "panadapter levels: a noise floor must fit an int16");
  for (int c = 0; gain_correction && c < ctx->nchan; ++c)
    if (!std::isfinite(gain_correction[c])) return fail(T41RX_ERR_ARG, "panadapter levels: non-finite gain correction");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old levels)
  if (const int rc = pan_upload_levels<int32_t>(ctx, ctx->pan.d_nf, noise_floor)) return rc;
  if (const int rc = pan_upload_levels<float>(ctx, ctx->pan.d_gc, gain_correction)) return rc;
  ctx->pan.attenuator = attenuator;
  return T41RX_OK;
}

int t41rx_get_panadapter(const t41rx_ctx *ctx, int64_t *frame_counter, int32_t *rows_written, int64_t *first_row_frame) {
  if (!ctx) return T41RX_ERR_ARG;
  if (frame_counter) *frame_counter = ctx->pan.counter;
  if (rows_written) *rows_written = ctx->pan.last_rows;
  if (first_row_frame) *first_row_frame = ctx->pan.last_first;
  return ctx->pan.on ? 1 : 0;
}

int t41rx_set_panadapter_counter(t41rx_ctx *ctx, int64_t n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (n < 0) return fail(T41RX_ERR_ARG, "the frame counter must be >= 0");
  ctx->pan.counter = n;
  return T41RX_OK;
}

}  // extern "C"
