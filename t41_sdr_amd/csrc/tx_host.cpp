// t41_sdr_amd/csrc/tx_host.cpp -- host side of the C ABI in include/t41tx.h (transmit exciter).
// Owns what the reference keeps in the exciter's static CMSIS instances (T41_SDR.ino:278-299,
// 877-888): per channel, resident in HBM between calls.  No CPU implementation exists here:
// without a HIP device every create / process call fails with T41RX_ERR_HIP.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "dev_buf.hpp"
#include "last_error.hpp"  // fail(): failures reach t41rx_last_error(), like the receive path's
#include "tx_internal.hpp"

using namespace t41;

struct t41tx_ctx {
  int device = 0;
  int nchan = 0;
  t41tx_params params{};
  DevBuf<float> d_state;  // [nchan][kTxDelayFloats] delay lines, then [nchan][kTxEqStateFloats] equaliser memories
  DevBuf<TxCoef> d_coef;
  DevBuf<int16_t> d_in, d_outL, d_outR;  // staging of the host-pointer entries
  size_t staging = 0;
  // transmit equaliser (xmitEQFlag, Exciter.cpp:94-98; t41tx_set_transmit_eq): the caller's band table and the levels
  // EEPROMData.equalizerXmt (gwv.cpp:50).  Configuration: kept across t41tx_set_params(), not part of a checkpoint.
  int eq_on = 0;
  bool eq_have_bands = false;
  float eq_coef[kTxEqCoefs] = {};
  int32_t eq_levels[kTxEqBands] = {0, 0, 100, 100, 100, 100, 100, 100, 100, 100, 100, 0, 0, 0};
  // CW exciter (CW_ExciterIQData(), CW_Excite.cpp:66-118; t41tx_set_cw_tone): the caller's cosBuffer2 / sinBuffer2.
  // Configuration like the equaliser's: kept across t41tx_set_params() and t41tx_reset(), not part of a checkpoint.
  bool cw_have_tone = false;
  float cw_cos[kTxCwTone] = {}, cw_sin[kTxCwTone] = {};
  // calibration exciter (ProcessIQData2(), Process2.cpp:309-349; t41tx_set_cal_tone, t41tx_set_cal_corrections): the
  // caller's cosBuffer3 / sinBuffer3 and bandOutputFactor, and a correction candidate per channel.  Configuration too.
  bool cal_have_tone = false;
  float cal_cos[kTxCwTone] = {}, cal_sin[kTxCwTone] = {}, cal_level = 0.0f;
  DevBuf<float> d_cal_corr;  // [nchan][2] amplitude, phase; allocated by the first t41tx_set_cal_corrections()
  bool cal_per_channel = false;
};

namespace {
// every mode the receive side accepts: ExciterIQData() runs in all of them and only applies the TX
// IQ correction in LSB / USB (Exciter.cpp:117-140)
bool valid(const t41tx_params &p) { return (p.mode >= T41RX_DEMOD_USB && p.mode <= T41RX_DEMOD_NFM) || p.mode == T41RX_DEMOD_SAM; }
// the checkpoint: 8 int32 words, then kTxStateFloats floats per channel
constexpr uint32_t kTxStateMagic = 0x58313454u;  // "T41X"
constexpr size_t kTxStateHeaderBytes = 8 * sizeof(int32_t);
size_t record_bytes(const t41tx_ctx *c) { return sizeof(float) * kTxStateFloats * (size_t)c->nchan; }
float *eq_state(const t41tx_ctx *c) { return c->d_state.get() + (size_t)kTxDelayFloats * (size_t)c->nchan; }

// staging of the host-pointer entries: one input and two output buffers of `*bytes` each (a call's q15 samples of one
// side), grown on demand
int ensure_staging(t41tx_ctx *ctx, int n_frames, size_t *bytes) {
  *bytes = sizeof(int16_t) * 2048 * (size_t)n_frames * (size_t)ctx->nchan;
  if (*bytes <= ctx->staging) return T41RX_OK;
  ctx->d_in.reset();
  ctx->d_outL.reset();
  ctx->d_outR.reset();
  ctx->staging = 0;
  if (dev_alloc(ctx->d_in, *bytes) != hipSuccess || dev_alloc(ctx->d_outL, *bytes) != hipSuccess || dev_alloc(ctx->d_outR, *bytes) != hipSuccess)
    return fail(T41RX_ERR_NOMEM, "staging allocation failed");
  ctx->staging = *bytes;
  return T41RX_OK;
}

// the tail of the host-pointer entries: rc is what the device entry returned for the staging buffers; wait for the launch
// and copy both sides out
int staged_out(const t41tx_ctx *ctx, int rc, int16_t *oL, int16_t *oR, size_t bytes) {
  if (rc != T41RX_OK) return rc;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(oL, ctx->d_outL.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(oR, ctx->d_outR.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(T41RX_ERR_HIP, "copy out failed");
  return T41RX_OK;
}

// the argument checks of the tone exciters' entries (CW, calibration); device pointers must be 16-byte aligned as well
int check_tone_call(const t41tx_ctx *ctx, bool t41tx_ctx::*have_tone, const char *no_tone, const int16_t *oL, const int16_t *oR, int n_frames,
                    bool device_ptrs) {
  if (!ctx || !oL || !oR) return fail(T41RX_ERR_ARG, "null argument");
  if (!(ctx->*have_tone)) return fail(T41RX_ERR_ARG, no_tone);
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  if (device_ptrs && ((reinterpret_cast<uintptr_t>(oL) | reinterpret_cast<uintptr_t>(oR)) & 15u))
    return fail(T41RX_ERR_ARG, "device pointers must be 16-byte aligned");
  return T41RX_OK;
}
constexpr const char *kNoCwTone = "CW exciter: no tone table loaded (t41tx_set_cw_tone)";
constexpr const char *kNoCalTone = "calibration exciter: no tone table loaded (t41tx_set_cal_tone)";

// what TxArgs, TxCwArgs and TxCalArgs have in common
template <class Args>
void common_args(Args &a, const t41tx_ctx *ctx, int16_t *oL, int16_t *oR, int n_frames) {
  a.outL = oL;
  a.outR = oR;
  a.state = ctx->d_state.get();
  a.coef = ctx->d_coef.get();
  a.nchan = ctx->nchan;
  a.nframes = n_frames;
  a.corr_on = (ctx->params.mode == T41RX_DEMOD_LSB || ctx->params.mode == T41RX_DEMOD_USB) ? 1 : 0;
  a.iq_phase = ctx->params.IQXPhaseCorrectionFactor;
}
}  // namespace

extern "C" {

void t41tx_default_params(t41tx_params *p) {
  if (!p) return;
  p->mode = T41RX_DEMOD_USB;
  p->IQXAmpCorrectionFactor = 1.0f;    // gwv.cpp:73
  p->IQXPhaseCorrectionFactor = 0.0f;  // gwv.cpp:74
}

int t41tx_create(t41tx_ctx **out, int device_id, int n_channels, const t41tx_params *p) {
  if (!out || !p) return fail(T41RX_ERR_ARG, "null argument");
  *out = nullptr;
  if (n_channels <= 0) return fail(T41RX_ERR_ARG, "n_channels must be > 0");
  if (!valid(*p)) return fail(T41RX_ERR_ARG, "mode must be USB, LSB, AM, NFM or SAM");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return fail(T41RX_ERR_HIP, "no such HIP device");
  DeviceGuard g(device_id);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  std::unique_ptr<t41tx_ctx> c(new (std::nothrow) t41tx_ctx());  // (freed before g restores the caller's device)
  if (!c) return fail(T41RX_ERR_NOMEM, "host allocation failed");
  c->device = device_id;
  c->nchan = n_channels;
  c->params = *p;
  TxCoef h;
  std::memcpy(h.c192, kTx192k10k, sizeof(h.c192));
  std::memcpy(h.c48, kTx48k8k, sizeof(h.c48));
  std::memcpy(h.h45, kTxHilbert45, sizeof(h.h45));
  std::memcpy(h.hn45, kTxHilbertNeg45, sizeof(h.hn45));
  const size_t sb = sizeof(float) * kTxStateFloats * (size_t)n_channels;
  if (dev_alloc(c->d_state, sb) != hipSuccess || dev_alloc(c->d_coef, sizeof(TxCoef)) != hipSuccess ||
      hipMemset(c->d_state.get(), 0, sb) != hipSuccess || hipMemcpy(c->d_coef.get(), &h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess)
    return fail(T41RX_ERR_HIP, "device allocation failed");
  *out = c.release();
  return T41RX_OK;
}

int t41tx_destroy(t41tx_ctx *ctx) {
  if (!ctx) return T41RX_OK;
  DeviceGuard g(ctx->device);
  (void)hipDeviceSynchronize();
  delete ctx;
  return T41RX_OK;
}

int t41tx_set_params(t41tx_ctx *ctx, const t41tx_params *p) {
  if (!ctx || !p) return fail(T41RX_ERR_ARG, "null argument");
  if (!valid(*p)) return fail(T41RX_ERR_ARG, "mode must be USB, LSB, AM, NFM or SAM");
  ctx->params = *p;
  return T41RX_OK;
}

int t41tx_reset(t41tx_ctx *ctx) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemset(ctx->d_state.get(), 0, sizeof(float) * kTxStateFloats * (size_t)ctx->nchan) != hipSuccess)
    return fail(T41RX_ERR_HIP, "state reset failed");
  return T41RX_OK;
}

int t41tx_n_channels(const t41tx_ctx *ctx) { return ctx ? ctx->nchan : fail(T41RX_ERR_ARG, "null argument"); }

int t41tx_set_transmit_eq_bands(t41tx_ctx *ctx, const float *coeffs) {
  if (!ctx || !coeffs) return fail(T41RX_ERR_ARG, "null argument");
  for (int i = 0; i < kTxEqCoefs; ++i)
    if (!std::isfinite(coeffs[i])) return fail(T41RX_ERR_ARG, "transmit-equaliser band table: non-finite coefficient");
  std::memcpy(ctx->eq_coef, coeffs, sizeof(ctx->eq_coef));  // (passed by value to every launch: the next call uses it)
  ctx->eq_have_bands = true;
  return T41RX_OK;
}

int t41tx_set_transmit_eq(t41tx_ctx *ctx, int xmitEQFlag, const int32_t *equalizerXmt) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (xmitEQFlag != 0 && xmitEQFlag != 1) return fail(T41RX_ERR_ARG, "xmitEQFlag must be 0 or 1");
  if (xmitEQFlag && !ctx->eq_have_bands)
    return fail(T41RX_ERR_ARG, "transmit equaliser: no band table loaded (t41tx_set_transmit_eq_bands)");
  if (equalizerXmt) std::memcpy(ctx->eq_levels, equalizerXmt, sizeof(ctx->eq_levels));
  ctx->eq_on = xmitEQFlag;
  return T41RX_OK;
}

int t41tx_get_transmit_eq(const t41tx_ctx *ctx, int32_t *equalizerXmt_out) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (equalizerXmt_out) std::memcpy(equalizerXmt_out, ctx->eq_levels, sizeof(ctx->eq_levels));
  return ctx->eq_on;
}

size_t t41tx_state_bytes(const t41tx_ctx *ctx) { return ctx ? kTxStateHeaderBytes + record_bytes(ctx) : 0; }

int t41tx_get_state(t41tx_ctx *ctx, void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  if (bytes < t41tx_state_bytes(ctx)) return fail(T41RX_ERR_STATE, "state buffer too small");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const int32_t hdr[8] = {(int32_t)kTxStateMagic, T41RX_ABI_VERSION, ctx->nchan, kTxStateFloats, 0, 0, 0, 0};
  std::memcpy(host_buf, hdr, sizeof(hdr));
  const size_t n = (size_t)kTxStateFloats * (size_t)ctx->nchan;
  std::vector<float> dev(n);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dev.data(), ctx->d_state.get(), sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(T41RX_ERR_HIP, "state copy out failed");
  // a channel's record: its delay lines, then its equaliser memories
  char *out = static_cast<char *>(host_buf) + kTxStateHeaderBytes;
  const float *eq = dev.data() + (size_t)kTxDelayFloats * (size_t)ctx->nchan;
  for (int c = 0; c < ctx->nchan; ++c, out += sizeof(float) * kTxStateFloats) {
    std::memcpy(out, dev.data() + (size_t)kTxDelayFloats * c, sizeof(float) * kTxDelayFloats);
    std::memcpy(out + sizeof(float) * kTxStEq, eq + (size_t)kTxEqStateFloats * c, sizeof(float) * kTxEqStateFloats);
  }
  return T41RX_OK;
}

int t41tx_set_state(t41tx_ctx *ctx, const void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  if (bytes < kTxStateHeaderBytes) return fail(T41RX_ERR_STATE, "state size mismatch");
  int32_t hdr[8];
  std::memcpy(hdr, host_buf, sizeof(hdr));
  if ((uint32_t)hdr[0] != kTxStateMagic || hdr[1] != T41RX_ABI_VERSION || hdr[2] != ctx->nchan || hdr[3] != kTxStateFloats)
    return fail(T41RX_ERR_STATE, "checkpoint header does not match this context (magic / abi / channels / record size)");
  if (bytes != t41tx_state_bytes(ctx)) return fail(T41RX_ERR_STATE, "state size mismatch");
  // everything is checked before anything is written: a refused checkpoint changes nothing
  const size_t n = (size_t)kTxStateFloats * (size_t)ctx->nchan;
  std::vector<float> rec(n);  // (host_buf need not be aligned for float)
  std::memcpy(rec.data(), static_cast<const char *>(host_buf) + kTxStateHeaderBytes, sizeof(float) * n);
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(rec[i])) return fail(T41RX_ERR_STATE, "checkpoint: non-finite value in a channel record");
  std::vector<float> dev(n);
  float *eq = dev.data() + (size_t)kTxDelayFloats * (size_t)ctx->nchan;
  for (int c = 0; c < ctx->nchan; ++c) {
    const float *r = rec.data() + (size_t)kTxStateFloats * c;
    std::memcpy(dev.data() + (size_t)kTxDelayFloats * c, r, sizeof(float) * kTxDelayFloats);
    std::memcpy(eq + (size_t)kTxEqStateFloats * c, r + kTxStEq, sizeof(float) * kTxEqStateFloats);
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(ctx->d_state.get(), dev.data(), sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess)
    return fail(T41RX_ERR_HIP, "state copy in failed");
  return T41RX_OK;
}

int t41tx_process_device_q15(t41tx_ctx *ctx, const int16_t *dL, const int16_t *dR, int16_t *oL, int16_t *oR, int n_frames,
                             void *hip_stream) {
  (void)dR;  // decimated and then overwritten by the L channel in the reference (Exciter.cpp:85, 89, 98)
  if (!ctx || !dL || !oL || !oR) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  if ((reinterpret_cast<uintptr_t>(dL) | reinterpret_cast<uintptr_t>(oL) | reinterpret_cast<uintptr_t>(oR)) & 15u)
    return fail(T41RX_ERR_ARG, "device pointers must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  TxArgs a{};
  common_args(a, ctx, oL, oR, n_frames);
  a.inL = dL;
  a.i_scale = (ctx->params.mode == T41RX_DEMOD_LSB) ? +ctx->params.IQXAmpCorrectionFactor : -ctx->params.IQXAmpCorrectionFactor;
  hipError_t e;
  if (ctx->eq_on) {
    TxEqArgs q{};
    static_cast<TxArgs &>(q) = a;
    q.eq_state = eq_state(ctx);
    std::memcpy(q.eq_coef, ctx->eq_coef, sizeof(q.eq_coef));
    for (int b = 0; b < kTxEqBands; ++b) {
      // equalizerXmt[b] = (float)EEPROMData.equalizerXmt[b] / 100.0 into an int array (Filter.cpp:178, gwv.h:44): the
      // level truncated toward zero to a whole number; arm_scale_f32 takes it, negated as an int for bands 1, 3, .., 13
      // (Filter.cpp:195-208), as a float
      const int whole = (int)((double)(float)ctx->eq_levels[b] / 100.0);
      q.eq_scale[b] = (float)((b % 2 == 0) ? -whole : whole);
    }
    e = launch_tx_eq(q, (hipStream_t)hip_stream);
  } else {
    e = launch_tx(a, (hipStream_t)hip_stream);
  }
  if (e != hipSuccess) return fail(T41RX_ERR_HIP, "kernel launch failed");
  return T41RX_OK;
}

int t41tx_process_host_q15(t41tx_ctx *ctx, const int16_t *L, const int16_t *R, int16_t *oL, int16_t *oR, int n_frames) {
  (void)R;
  if (!ctx || !L || !oL || !oR) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  size_t bytes;
  if (const int rc = ensure_staging(ctx, n_frames, &bytes)) return rc;
  if (hipMemcpy(ctx->d_in.get(), L, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(T41RX_ERR_HIP, "copy in failed");
  return staged_out(ctx, t41tx_process_device_q15(ctx, ctx->d_in.get(), nullptr, ctx->d_outL.get(), ctx->d_outR.get(), n_frames, nullptr), oL, oR,
                    bytes);
}

int t41tx_set_cw_tone(t41tx_ctx *ctx, const float *cosBuffer2, const float *sinBuffer2) {
  if (!ctx || !cosBuffer2 || !sinBuffer2) return fail(T41RX_ERR_ARG, "null argument");
  for (int i = 0; i < kTxCwTone; ++i)
    if (!std::isfinite(cosBuffer2[i]) || !std::isfinite(sinBuffer2[i])) return fail(T41RX_ERR_ARG, "CW tone table: non-finite value");
  std::memcpy(ctx->cw_cos, cosBuffer2, sizeof(ctx->cw_cos));  // (passed by value to every launch: the next call uses it)
  std::memcpy(ctx->cw_sin, sinBuffer2, sizeof(ctx->cw_sin));
  ctx->cw_have_tone = true;
  return T41RX_OK;
}

int t41tx_process_cw_device_q15(t41tx_ctx *ctx, const uint8_t *d_key, int16_t *oL, int16_t *oR, int n_frames, void *hip_stream) {
  if (const int rc = check_tone_call(ctx, &t41tx_ctx::cw_have_tone, kNoCwTone, oL, oR, n_frames, true)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  TxCwArgs a{};
  common_args(a, ctx, oL, oR, n_frames);
  a.key = d_key;
  // the opposite signs of ExciterIQData()'s (CW_Excite.cpp:79, 84)
  a.i_scale = (ctx->params.mode == T41RX_DEMOD_LSB) ? -ctx->params.IQXAmpCorrectionFactor : +ctx->params.IQXAmpCorrectionFactor;
  std::memcpy(a.tone_cos, ctx->cw_cos, sizeof(a.tone_cos));
  std::memcpy(a.tone_sin, ctx->cw_sin, sizeof(a.tone_sin));
  if (launch_tx_cw(a, (hipStream_t)hip_stream) != hipSuccess) return fail(T41RX_ERR_HIP, "kernel launch failed");
  return T41RX_OK;
}

int t41tx_process_cw_host_q15(t41tx_ctx *ctx, const uint8_t *key, int16_t *oL, int16_t *oR, int n_frames) {
  if (const int rc = check_tone_call(ctx, &t41tx_ctx::cw_have_tone, kNoCwTone, oL, oR, n_frames, false)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  size_t bytes;
  if (const int rc = ensure_staging(ctx, n_frames, &bytes)) return rc;
  // the gate rides in the input staging buffer: 16 bytes per frame where the microphone's samples take 4096
  const size_t key_bytes = (size_t)kTxCwKeyPerFrame * (size_t)n_frames * (size_t)ctx->nchan;
  if (key && hipMemcpy(ctx->d_in.get(), key, key_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(T41RX_ERR_HIP, "copy in failed");
  const uint8_t *d_key = key ? reinterpret_cast<const uint8_t *>(ctx->d_in.get()) : nullptr;
  return staged_out(ctx, t41tx_process_cw_device_q15(ctx, d_key, ctx->d_outL.get(), ctx->d_outR.get(), n_frames, nullptr), oL, oR, bytes);
}

int t41tx_set_cal_tone(t41tx_ctx *ctx, const float *cosBuffer3, const float *sinBuffer3, float level) {
  if (!ctx || !cosBuffer3 || !sinBuffer3) return fail(T41RX_ERR_ARG, "null argument");
  if (!std::isfinite(level)) return fail(T41RX_ERR_ARG, "calibration tone: non-finite level");
  for (int i = 0; i < kTxCwTone; ++i)
    if (!std::isfinite(cosBuffer3[i]) || !std::isfinite(sinBuffer3[i])) return fail(T41RX_ERR_ARG, "calibration tone table: non-finite value");
  std::memcpy(ctx->cal_cos, cosBuffer3, sizeof(ctx->cal_cos));  // (passed by value to every launch: the next call uses it)
  std::memcpy(ctx->cal_sin, sinBuffer3, sizeof(ctx->cal_sin));
  ctx->cal_level = level;
  ctx->cal_have_tone = true;
  return T41RX_OK;
}

int t41tx_set_cal_corrections(t41tx_ctx *ctx, const float *amp, const float *phase) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!amp && !phase) {  // back to the params' factors
    ctx->cal_per_channel = false;
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
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  if (!ctx->d_cal_corr && dev_alloc(ctx->d_cal_corr, sizeof(float) * h.size()) != hipSuccess)
    return fail(T41RX_ERR_NOMEM, "calibration corrections: device allocation failed");
  // (a launch still in flight reads the old candidates: wait for it, as the state copies do)
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(ctx->d_cal_corr.get(), h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(T41RX_ERR_HIP, "calibration corrections: copy in failed");
  ctx->cal_per_channel = true;
  return T41RX_OK;
}

int t41tx_process_cal_device_q15(t41tx_ctx *ctx, int16_t *oL, int16_t *oR, int n_frames, void *hip_stream) {
  if (const int rc = check_tone_call(ctx, &t41tx_ctx::cal_have_tone, kNoCalTone, oL, oR, n_frames, true)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  TxCalArgs a{};
  common_args(a, ctx, oL, oR, n_frames);
  a.corr = ctx->cal_per_channel ? ctx->d_cal_corr.get() : nullptr;
  a.level = ctx->cal_level;
  a.iq_amp = ctx->params.IQXAmpCorrectionFactor;
  a.lsb = ctx->params.mode == T41RX_DEMOD_LSB ? 1 : 0;  // Process2.cpp:318, 322: CW's signs, not ExciterIQData()'s
  std::memcpy(a.tone_cos, ctx->cal_cos, sizeof(a.tone_cos));
  std::memcpy(a.tone_sin, ctx->cal_sin, sizeof(a.tone_sin));
  if (launch_tx_cal(a, (hipStream_t)hip_stream) != hipSuccess) return fail(T41RX_ERR_HIP, "kernel launch failed");
  return T41RX_OK;
}

int t41tx_process_cal_host_q15(t41tx_ctx *ctx, int16_t *oL, int16_t *oR, int n_frames) {
  if (const int rc = check_tone_call(ctx, &t41tx_ctx::cal_have_tone, kNoCalTone, oL, oR, n_frames, false)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  size_t bytes;
  if (const int rc = ensure_staging(ctx, n_frames, &bytes)) return rc;
  return staged_out(ctx, t41tx_process_cal_device_q15(ctx, ctx->d_outL.get(), ctx->d_outR.get(), n_frames, nullptr), oL, oR, bytes);
}

}  // extern "C"
