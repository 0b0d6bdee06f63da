// t41_sdr_amd/csrc/rx_cal.cpp -- host side of the IQ calibration's receive half (cal_kernel.hip): its settings, the
// correction candidates, and the t41rx_calibrate_* entry points.  No part of a process call.
#include <cmath>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {

// t41rx_reset(): the calibration memory to power-on: FFT_spec_old, zoom memories, ring, pointer and pixelnew[] all zero
int cal_reset(t41rx_ctx *ctx) {
  if (ctx->cal.d_mem) HIP_TRY(hipMemset(ctx->cal.d_mem.get(), 0, sizeof(float) * kCalFloats * (size_t)ctx->nchan));
  return T41RX_OK;
}

namespace {

// what every t41rx_calibrate_* entry checks, then the launch.  I / Q are float_buffer_L's and float_buffer_R's sources
// (the q15 entries have swapped the queues already)
int calibrate_impl(t41rx_ctx *ctx, const void *dI, const void *dQ, int shared_input, const uint8_t *d_update, float *d_result,
                   int16_t *d_pixel, float *d_spec, int n_frames, void *hip_stream, bool q15) {
  if (!ctx || !dI || !dQ || !d_result) return fail(T41RX_ERR_ARG, "null argument");
  if (!ctx->cal.on) return fail(T41RX_ERR_ARG, "calibration is not switched on (t41rx_set_calibration)");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the calibration is built for fft_length 512");
  if (ctx->layout != T41RX_LAYOUT_CHANNEL_MAJOR) return fail(T41RX_ERR_UNSUPPORTED, "the calibration is built for the channel-major layout");
  if (((reinterpret_cast<uintptr_t>(dI) | reinterpret_cast<uintptr_t>(dQ)) & (q15 ? 1u : 3u)) ||
      ((reinterpret_cast<uintptr_t>(d_result) | reinterpret_cast<uintptr_t>(d_spec)) & 3u) || (reinterpret_cast<uintptr_t>(d_pixel) & 1u))
    return fail(T41RX_ERR_ARG, "unaligned pointer");
  if (!ctx->cal.d_mem || !ctx->d_win) return fail(T41RX_ERR_STATE, "calibration enabled without its buffers");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const Calibration &cal = ctx->cal;
  CalArgs a{};
  a.I = dI;
  a.Q = dQ;
  a.update = d_update;
  a.result = d_result;
  a.pixel = d_pixel;
  a.spec = d_spec;
  a.cal = cal.d_mem.get();
  a.tab = ctx->d_tab.get();
  a.win = ctx->d_win.get();
  a.corr = cal.per_channel ? cal.d_corr.get() : nullptr;
  a.zoom = cal.zoom;
  zoom_filter_args(a.zoom, a.iir, a.fir);
  a.chan_stride = shared_input ? 0 : (long long)n_frames * 2048;
  a.nchan = ctx->nchan;
  a.nframes = n_frames;
  a.q15 = q15 ? 1 : 0;
  a.g_rf = blob_view(ctx->blob.data()).scalars[kScRfGain];  // the same expression, Process.cpp:117 / Process2.cpp:365
  a.rec_band = 1.0f;                                        // recBandFactor[], Process2.cpp:299
  a.iq_amp = ctx->params.IQAmpCorrectionFactor;
  a.iq_phase = ctx->params.IQPhaseCorrectionFactor;
  a.corr_on = (ctx->params.mode == T41RX_DEMOD_LSB || ctx->params.mode == T41RX_DEMOD_USB) ? 1 : 0;
  a.dBScale = cal.dbscale;
  a.base = cal.base;
  a.lo0 = cal.lo0;
  a.lo1 = cal.lo1;
  a.width = cal.width;
  a.sideband = ctx->params.mode == T41RX_DEMOD_LSB ? 1 : ctx->params.mode == T41RX_DEMOD_USB ? 2 : 0;
  return hip_check(launch_cal(a, (hipStream_t)hip_stream), "calibration kernel launch");
}

// host-pointer form: temporaries of its own (the audio path's staging buffers are not touched); the rows of d_pixel /
// d_spec a call leaves alone keep the caller's contents, so those two travel both ways
int calibrate_host_impl(t41rx_ctx *ctx, const void *I, const void *Q, int shared_input, const uint8_t *update, float *result,
                        int16_t *pixel, float *spec, int n_frames, bool q15) {
  if (!ctx || !I || !Q || !result) return fail(T41RX_ERR_ARG, "null argument");
  if (!ctx->cal.on) return fail(T41RX_ERR_ARG, "calibration is not switched on (t41rx_set_calibration)");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const size_t rows = (size_t)ctx->nchan * (size_t)n_frames;
  const size_t in_bytes = (shared_input ? (size_t)n_frames : rows) * 2048 * (q15 ? sizeof(int16_t) : sizeof(float));
  DevBuf<char> dI, dQ, dU;
  DevBuf<float> dR, dS;
  DevBuf<int16_t> dP;
  HIP_TRY(dev_alloc(dI, in_bytes));
  HIP_TRY(dev_alloc(dQ, in_bytes));
  HIP_TRY(dev_alloc(dR, rows * 3 * sizeof(float)));
  HIP_TRY(hipMemcpy(dI.get(), I, in_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dQ.get(), Q, in_bytes, hipMemcpyHostToDevice));
  if (update) {
    HIP_TRY(dev_alloc(dU, (size_t)n_frames));
    HIP_TRY(hipMemcpy(dU.get(), update, (size_t)n_frames, hipMemcpyHostToDevice));
  }
  if (pixel) {
    HIP_TRY(dev_alloc(dP, rows * 512 * sizeof(int16_t)));
    HIP_TRY(hipMemcpy(dP.get(), pixel, rows * 512 * sizeof(int16_t), hipMemcpyHostToDevice));
  }
  if (spec) {
    HIP_TRY(dev_alloc(dS, rows * 512 * sizeof(float)));
    HIP_TRY(hipMemcpy(dS.get(), spec, rows * 512 * sizeof(float), hipMemcpyHostToDevice));
  }
  const int rc = calibrate_impl(ctx, dI.get(), dQ.get(), shared_input, reinterpret_cast<const uint8_t *>(dU.get()), dR.get(), dP.get(),
                                dS.get(), n_frames, nullptr, q15);
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(result, dR.get(), rows * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (pixel) HIP_TRY(hipMemcpy(pixel, dP.get(), rows * 512 * sizeof(int16_t), hipMemcpyDeviceToHost));
  if (spec) HIP_TRY(hipMemcpy(spec, dS.get(), rows * 512 * sizeof(float), hipMemcpyDeviceToHost));
  return T41RX_OK;
}

}  // namespace
}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_set_calibration(t41rx_ctx *ctx, int on, int spectrumZoom, int currentScale, int pixel_offset, int bin0, int bin1,
                          int capture_bins) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  Calibration &cal = ctx->cal;
  if (!on) {
    cal.on = false;
    return T41RX_OK;
  }
  if (spectrumZoom < 0 || spectrumZoom > 4) return fail(T41RX_ERR_ARG, "spectrumZoom must be 0 (1x) .. 4 (16x)");
  if (currentScale < 0 || currentScale > 4) return fail(T41RX_ERR_ARG, "currentScale must be 0 .. 4");
  if (pixel_offset < -32768 || pixel_offset > 32767) return fail(T41RX_ERR_ARG, "pixel_offset must fit an int16");
  if (capture_bins < 1) return fail(T41RX_ERR_ARG, "capture_bins must be >= 1");
  for (const int b : {bin0, bin1})
    if ((long long)b - capture_bins < 2 || (long long)b + capture_bins > 512)
      return fail(T41RX_ERR_ARG, "a window [bin - capture_bins, bin + capture_bins) must lie within [2, 512]");
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the calibration is built for fft_length 512");
  if (ctx->layout != T41RX_LAYOUT_CHANNEL_MAJOR) return fail(T41RX_ERR_UNSUPPORTED, "the calibration is built for the channel-major layout");
  // anything that fails from here on leaves calibration switched off
  cal.on = false;
  if (!cal.d_mem) HIP_TRY(dev_alloc(cal.d_mem, sizeof(float) * kCalFloats * (size_t)ctx->nchan));
  if (const int rc = ensure_window(ctx)) return rc;
  HIP_TRY(hipMemset(cal.d_mem.get(), 0, sizeof(float) * kCalFloats * (size_t)ctx->nchan));  // power-on: ZoomFFTPrep(), pixelnew[] = 0
  cal.zoom = spectrumZoom;
  cal.dbscale = kDbScale[currentScale];
  cal.base = kBaseOffset[currentScale] + pixel_offset;
  cal.lo0 = bin0 - capture_bins;
  cal.lo1 = bin1 - capture_bins;
  cal.width = 2 * capture_bins;
  cal.on = true;
  return T41RX_OK;
}

int t41rx_set_cal_corrections(t41rx_ctx *ctx, const float *amp, const float *phase) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!amp && !phase) {  // back to the params' factors
    ctx->cal.per_channel = false;
    return T41RX_OK;
  }
  if (!amp || !phase) return fail(T41RX_ERR_ARG, "calibration corrections: amp and phase must both be given or both be NULL");
  std::vector<float> h(2 * (size_t)ctx->nchan);
  for (int c = 0; c < ctx->nchan; ++c) {
    if (!std::isfinite(amp[c]) || !std::isfinite(phase[c])) return fail(T41RX_ERR_ARG, "calibration corrections: non-finite value");
    h[2 * (size_t)c] = amp[c];
    h[2 * (size_t)c + 1] = phase[c];
  }
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old candidates)
  if (!ctx->cal.d_corr) HIP_TRY(dev_alloc(ctx->cal.d_corr, sizeof(float) * h.size()));
  HIP_TRY(hipMemcpy(ctx->cal.d_corr.get(), h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
  ctx->cal.per_channel = true;
  return T41RX_OK;
}

int t41rx_calibrate_device(t41rx_ctx *ctx, const float *dI, const float *dQ, int shared_input, const uint8_t *d_update,
                           float *d_result, int16_t *d_pixel, float *d_spec, int n_frames, void *hip_stream) {
  return calibrate_impl(ctx, dI, dQ, shared_input, d_update, d_result, d_pixel, d_spec, n_frames, hip_stream, false);
}

// float_buffer_L (= I) is filled from the R queue and float_buffer_R (= Q) from the L queue (Process2.cpp:359-360)
int t41rx_calibrate_device_q15(t41rx_ctx *ctx, const int16_t *dQ_in_L, const int16_t *dQ_in_R, int shared_input,
                               const uint8_t *d_update, float *d_result, int16_t *d_pixel, float *d_spec, int n_frames,
                               void *hip_stream) {
  return calibrate_impl(ctx, dQ_in_R, dQ_in_L, shared_input, d_update, d_result, d_pixel, d_spec, n_frames, hip_stream, true);
}

int t41rx_calibrate_host(t41rx_ctx *ctx, const float *I, const float *Q, int shared_input, const uint8_t *update, float *result,
                         int16_t *pixel, float *spec, int n_frames) {
  return calibrate_host_impl(ctx, I, Q, shared_input, update, result, pixel, spec, n_frames, false);
}

int t41rx_calibrate_host_q15(t41rx_ctx *ctx, const int16_t *Q_in_L, const int16_t *Q_in_R, int shared_input, const uint8_t *update,
                             float *result, int16_t *pixel, float *spec, int n_frames) {
  return calibrate_host_impl(ctx, Q_in_R, Q_in_L, shared_input, update, result, pixel, spec, n_frames, true);
}

}  // extern "C"
