// t41_sdr_amd/csrc/rx_host.cpp -- host side of the C ABI in include/t41rx.h.
//
// Owns what the reference keeps in firmware globals: the coefficient arrays
// (FIR_dec1_coeffs ... FIR_filter_mask, T41_SDR.ino:398-399, Filter.cpp:39-41), the CMSIS
// instance state (T41_SDR.ino:384-397), the oscillator state (Freq_Shift.cpp:13-14) and the
// overlap-save block (T41_SDR.ino:403-404) -- here per channel and resident in HBM.
// There is no CPU implementation of the path in this library: without a HIP device every
// create/process call fails with T41RX_ERR_HIP.
//
// This file is the core: create / destroy, parameters, coefficients, oscillators, layout and input map, the taps, and
// the process call.  The context, and where each stage's host side lives, is in rx_ctx.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "rx_ctx.hpp"

using namespace t41;

namespace {
thread_local std::string g_last_error;  // t41rx_last_error(); t41tx_* failures set it too (tx_host.cpp)
}  // namespace

int t41::fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

namespace {

constexpr float kPiF = 3.1415926535897932384626433832795f;  // FIR.h:10

// FreqShift2's per-call constants (Freq_Shift.cpp:121-124) turned into what the kernel needs:
// the rotation per sample as a 0.64 fixed-point fraction of a turn, the steady-state
// amplitude of the oscillator's gain loop, and the eight per-lane sample offsets.
ChanNco make_nco(int32_t nco_freq_hz, int side_tone_hz) {
  ChanNco n{};
  const long f = (long)nco_freq_hz + (long)side_tone_hz;
  const float inc = (float)(2.0 * kPiF * f / 192000.0);  // NCO_INC (float32_t)
  const double c = std::cos((double)inc), s = std::sin((double)inc);  // OSC_COS / OSC_SIN
  const long double ang = atan2l((long double)s, (long double)c);
  long double turns = ang / (2.0L * 3.14159265358979323846264338327950288L);
  if (turns < 0.0L) turns += 1.0L;
  const long double scaled = floorl(turns * 18446744073709551616.0L + 0.5L);
  n.phase_inc = (scaled >= 18446744073709551616.0L) ? 0ull : (uint64_t)scaled;
  n.w_abs = (double)hypotl((long double)c, (long double)s);
  // fixed point of r <- r (1.95 - r^2) |W|  (Freq_Shift.cpp:130-134)
  n.r_star_sq = 1.95 - 1.0 / n.w_abs;
  const double amp = (double)1.1f * std::sqrt(n.r_star_sq) * n.w_abs;  // freqAdjFactor * |Osc|
  for (int k = 0; k < 8; ++k) {
    // 1.1 A e^{j k ang} (-j)^k: the (-j)^k folds FreqShift1's x j^n (Freq_Shift.cpp:42-65) into the
    // conjugate multiply of the mixer; a rotation by k quarter turns is exact
    const double c = amp * (double)cosl(ang * k), s = amp * (double)sinl(ang * k);
    double re, im;
    switch (k & 3) {
      case 0: re = c; im = s; break;
      case 1: re = s; im = -c; break;   // (c + js)(-j) = s - jc
      case 2: re = -c; im = -s; break;
      default: re = -s; im = c; break;  // (c + js)(j) = -s + jc
    }
    n.wk[k][0] = (float)re;
    n.wk[k][1] = (float)im;
  }
  return n;
}

}  // namespace

// (the side tone folded into the oscillator is the channel's own set's)
int t41::upload_nco(t41rx_ctx *ctx) {
  std::vector<ChanNco> h((size_t)ctx->nchan);
  for (int i = 0; i < ctx->nchan; ++i) {
    const int set = sets_loaded(ctx) ? ctx->sets.set_of[(size_t)i] : 0;
    float *blob = set == 0 ? ctx->blob.data() : ctx->sets.blobs[(size_t)set - 1].data();
    h[(size_t)i] = make_nco(ctx->nco_hz[(size_t)i], (int)blob_view(blob).scalars[kScSideTone]);
  }
  HIP_TRY(hipMemcpy(ctx->d_nco.get(), h.data(), sizeof(ChanNco) * h.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}

// blob -> the device's coefficient block
void t41::fill_dev_coef(const BlobView &v, DevCoef &dc) {
  std::memset(&dc, 0, sizeof(dc));
  std::memcpy(dc.dec1, v.dec1, sizeof(float) * kDec1Taps);
  // FIR_dec2_coeffs times the level adjust volScaleFactor (Process.cpp:481-492), the multiply right behind that filter
  for (int i = 0; i < kDec2Taps; ++i) dc.dec2[i] = v.dec2[i] * v.scalars[kScLevel];
  std::memcpy(dc.int1, v.int1, sizeof(float) * kInt1Taps);
  // FIR_int2_coeffs times the volume factor DF * VolumeToAmplification(audioVolume) (Process.cpp:929):
  // the x4 interpolator is the last stage before it, so the kernels apply it through the taps
  for (int i = 0; i < kInt2Taps; ++i) dc.int2[i] = v.int2[i] * v.scalars[kScOutScale];
  std::memcpy(dc.lp1, v.lp1, sizeof(float) * 5);
  std::memcpy(dc.sc, v.scalars, sizeof(float) * kNumScalars);
  std::memcpy(dc.agc, v.agc, sizeof(float) * kNumAgc);
  std::memcpy(dc.deemph, kDeemphFir24000, sizeof(float) * kDeemphTaps);
}

// what plan_call() reads of a parameter struct (the process call adds the context's part; rx_sets.cpp compares two sets)
CallFacts t41::params_facts(const t41rx_params &p, bool plain_gains) {
  CallFacts f;
  f.seg = p.fft_length / 512;
  f.family = p.mode == T41RX_DEMOD_AM ? Family::am : p.mode == T41RX_DEMOD_NFM ? Family::nfm : p.mode == T41RX_DEMOD_SAM ? Family::sam : Family::ssb;
  f.agc = p.AGCMode != 0;
  f.nfm_atan = p.mode == T41RX_DEMOD_NFM && p.nfm_demod == 1;
  f.plain_gains = plain_gains;
  f.nr = p.nrOptionSelect != 0 || p.ANR_notchOn != 0;
  return f;
}

// the first stage's gains of a blob's scalars, and whether they are `plain`
bool t41::gains_of(const float *sc, SetGains &g) {
  const bool iq_on = sc[kScIqCorrOn] != 0.0f;
  const float gi = iq_on ? sc[kScBandGain] * sc[kScNegIqAmp] : sc[kScBandGain];
  g = SetGains{};
  g.g_rf = sc[kScRfGain];
  g.g_band = sc[kScBandGain];
  g.neg_iq_amp = sc[kScNegIqAmp];
  g.iq_phase = sc[kScIqPhase];
  g.iq_corr_on = iq_on ? 1 : 0;
  // PLAIN folds "I <- -I" (IQ correction on, amplitude factor 1) into the sign of the RF gain; with
  // the correction on and gi = +1 (IQAmpCorrectionFactor = -1) the general kernel must run
  return (iq_on ? gi == -1.0f : gi == 1.0f) && sc[kScBandGain] == 1.0f && (!iq_on || sc[kScIqPhase] == 0.0f);
}

namespace {
// blob -> device constant block + lane-ordered tables
int upload_coeffs(t41rx_ctx *ctx) {
  const int N = ctx->params.fft_length;
  BlobView v = blob_view(ctx->blob.data());
  DevCoef dc;
  fill_dev_coef(v, dc);
  HIP_TRY(hipMemcpy(ctx->d_coef.get(), &dc, sizeof(dc), hipMemcpyHostToDevice));

  const int R = N / 512;  // 2048-sample segments per frame
  std::vector<float2> tab;
  fill_tab512(v, N, tab);
  const float invN = 1.0f / (float)N;  // exact power of two: folding it into the mask is lossless
  if (N != 512) {
    // N = R x 512 decomposition: radix-R twiddles W_N^(k' q) and the mask in [q][m] order
    std::vector<float2> t4((size_t)tab_long_entries(R));
    const double tp = 6.283185307179586476925286766559;
    for (int q = 1; q < R; ++q)
      for (int k = 0; k < 512; ++k) {
        const double a = -tp * (double)(k * q) / (double)N;
        t4[(size_t)(512 * (q - 1) + k)] = make_float2((float)std::cos(a), (float)std::sin(a));
      }
    for (int q = 0; q < R; ++q)
      for (int m = 0; m < 512; ++m) {
        const int k = q + R * m;
        t4[(size_t)((R - 1) * 512 + 512 * q + m)] = make_float2(v.mask[2 * k] * invN, v.mask[2 * k + 1] * invN);
      }
    HIP_TRY(hipMemcpy(ctx->d_tab4k.get(), t4.data(), sizeof(float2) * t4.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(ctx->d_tab.get(), tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}
}  // namespace

// blob -> the constant table of the fused kernels (the mask only at fft_length 512: the long pipeline has its own)
void t41::fill_tab512(const BlobView &v, int N, std::vector<float2> &tab) {
  tab.assign((size_t)kTabEntries512, make_float2(0.0f, 0.0f));
  const float invN = 1.0f / (float)N;  // exact power of two: folding it into the mask is lossless
  if (N == 512) {
    for (int r = 0; r < 8; ++r)
      for (int l = 0; l < 64; ++l) {
        const int k = l + 64 * r;
        tab[(size_t)(kTabMask + 64 * r + l)] = make_float2(v.mask[2 * k] * invN, v.mask[2 * k + 1] * invN);
      }
  }
  const double two_pi = 6.283185307179586476925286766559;
  for (int q = 1; q < 8; ++q)
    for (int l = 0; l < 64; ++l) {
      const double a1 = -two_pi * (double)(l * q) / 512.0;
      const double a2 = -two_pi * (double)((l & 7) * q) / 64.0;
      tab[(size_t)(kTabTw1 + 64 * (q - 1) + l)] = make_float2((float)std::cos(a1), (float)std::sin(a1));
      tab[(size_t)(kTabTw2 + 64 * (q - 1) + l)] = make_float2((float)std::cos(a2), (float)std::sin(a2));
    }
  for (int i = 0; i < 256; ++i) {
    const double a = two_pi * (double)i / 256.0;
    tab[(size_t)(kTabSinCos + i)] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  // DC high-pass (FIR.cpp:87-89, a1 = 0.854352383886757938) carry multipliers for the DPP scan
  for (int l = 0; l < 64; ++l) {
    const double a1 = 0.854352383886757938;
    tab[(size_t)(kTabHp8 + l)] = make_float2((float)std::pow(a1, 8.0 * ((l & 15) + 1)), (float)std::pow(a1, 8.0 * ((l & 31) + 1)));
    tab[(size_t)(kTabHp4 + l)] = make_float2((float)std::pow(a1, 4.0 * ((l & 15) + 1)), (float)std::pow(a1, 4.0 * ((l & 31) + 1)));
  }
  // AM demodulator (Process.cpp:698-705): carry multipliers of its two wave scans.  DC blocker
  // w = m + 0.99 w_old: powers of ca^4 in double; biquad_lowpass1 (DF1): powers of the 2x2
  // transition matrix over one lane's four samples, P1 = M^4, M = [[a1, a2], [1, 0]], in f32.
  {
    const double ca = (double)0.99f, a4 = ca * ca * ca * ca;
    struct M2 { float a, b, c, d; };
    auto mm = [](M2 x, M2 y) { return M2{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d}; };
    const M2 M{v.lp1[3], v.lp1[4], 1.0f, 0.0f};
    const M2 Mq = mm(M, M), P1 = mm(Mq, Mq);
    for (int l = 0; l < 64; ++l) {
      double p15 = a4, p31 = a4;
      M2 Q15 = P1, Q31 = P1;
      for (int i = 0; i < (l & 15); ++i) { p15 *= a4; Q15 = mm(Q15, P1); }
      for (int i = 0; i < (l & 31); ++i) { p31 *= a4; Q31 = mm(Q31, P1); }
      float2 *e = &tab[(size_t)(kTabAm + 6 * l)];
      std::memcpy(&e[0], &p15, sizeof(double));
      std::memcpy(&e[1], &p31, sizeof(double));
      e[2] = make_float2(Q15.a, Q15.b);
      e[3] = make_float2(Q15.c, Q15.d);
      e[4] = make_float2(Q31.a, Q31.b);
      e[5] = make_float2(Q31.c, Q31.d);
    }
  }
  // arm_sin_f32's table for the synchronous detector (Demod.cpp:75-76): sin(2 pi k / 512), k = 0..512, rounded from
  // double (the library's own literals are not available here: DESIGN.md section 2), exact zeros where it has them
  {
    float *t = reinterpret_cast<float *>(&tab[(size_t)kTabSam]);
    for (int k = 0; k <= 512; ++k) t[k] = (float)std::sin(6.283185307179586476925286766559 * (double)k / 512.0);
    t[0] = 0.0f;
    t[256] = 0.0f;
    t[512] = -0.0f;
  }
}

namespace {

// a broken hand-over protocol of the pipelined kernels leaves wrong samples and a count of waits that ran out, not a hung
// GPU -- reported at the calls that synchronise anyway
int pipe_timeouts(const t41rx_ctx *ctx) {  // < 0: the counter could not be read
  if (!ctx->d_agc_pipe) return 0;
  unsigned n = 0;
  if (hipMemcpy(&n, ctx->d_agc_pipe.get() + pipe_layout(ctx->nchan).timeout, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return (int)n;
}
}  // namespace

int t41::pipe_timeouts_clear(t41rx_ctx *ctx) {
  if (!ctx->d_agc_pipe) return T41RX_OK;
  HIP_TRY(hipMemset(ctx->d_agc_pipe.get() + pipe_layout(ctx->nchan).timeout, 0, sizeof(unsigned long long)));
  return T41RX_OK;
}
// what the synchronising entry points answer when a wait inside the pipelined kernels has run out
int t41::pipe_status(const t41rx_ctx *ctx) {
  const int n = pipe_timeouts(ctx);
  if (n < 0) return fail(T41RX_ERR_HIP, "could not read the pipelined kernels' time-out counter");
  if (n > 0)
    return fail(T41RX_ERR_STATE, "a wait inside the pipelined AGC / SAM kernel ran out: the samples since the last reset or restored checkpoint are not valid");
  return T41RX_OK;
}

namespace {

// ---- a process call: (a) prepare_call, (b) rx_args, (c) launch_chain

// what the call is, for plan_call() (rx_plan.hpp); behind pan_prepare(), which counts the call's panadapter rows
CallFacts call_facts(const t41rx_ctx *ctx, int n_frames, bool q15) {
  SetGains g;
  CallFacts f = params_facts(ctx->params, gains_of(blob_view(const_cast<float *>(ctx->blob.data())).scalars, g));
  f.nr = nr_on(ctx);  // (a noise-reduction map: some entry non-zero)
  f.q15 = q15;
  f.n_frames = n_frames;
  f.seg_run_set = ctx->seg_run_set;
  f.map = ctx->n_streams > 0;
  f.sets = sets_loaded(ctx);
  f.stage_sets = sets_staged(ctx);
  f.a24 = audio_24k(ctx);
  // (a diagnostic library's stamps ride behind the demod tap pointer at the long lengths, T41RX_STAMP_TAPS: no tap to the plan)
  const bool taps = f.seg == 1 || !ctx->stamp_taps;
  f.tap_nco = taps && ctx->dbg_nco;
  f.tap_dec = taps && ctx->dbg_dec;
  f.tap_demod = taps && ctx->dbg_demod;
  f.spect = ctx->spect != nullptr;
  f.disp = ctx->disp.spec != nullptr;
  f.pan_rows = pan_call_rows(ctx);  // (a panadapter map that lists nobody: the call is one without the stage)
  f.ft8 = ctx->ft8.on != 0;
  f.eq = ctx->eq.on != 0;
  f.nb = ctx->nb.on != 0;
  f.cw_filter = cw_filter_on(ctx);
  f.cw_det = cw_det_on(ctx);
  f.omap = ctx->out_map_on;
  // the CW filter map: cw_filter above says that some channel is filtered, this that some channel is not
  f.cw_unfiltered = ctx->cw.map_on && ctx->cw.lists.filtered.size() < (size_t)ctx->nchan;
  return f;
}

// (a) what the call needs allocated (stages and scratch on first use, kept) and the refusals that depend on the context
int prepare_call(t41rx_ctx *ctx, const CallPlan &plan, int n_frames, hipStream_t s) {
  int rc = T41RX_OK;
  if (ctx->beacon.on && (rc = beacon_prepare(ctx)) != T41RX_OK) return rc;
  if ((nr_on(ctx) && (rc = ensure_nr(ctx)) != T41RX_OK) || (ctx->nb.on && (rc = ensure_nb(ctx)) != T41RX_OK) ||
      (ctx->eq.on && (rc = ensure_eq(ctx)) != T41RX_OK) ||
      ((cw_filter_on(ctx) || cw_det_on(ctx)) && (rc = ensure_cw(ctx)) != T41RX_OK))
    return rc;
  if (plan.scratch && n_frames > ctx->scratch_frames) {
    // scratch between the kernels of the long-FFT pipeline / behind the hand-over (grown on demand, kept)
    HIP_TRY(hipStreamSynchronize(s));
    ctx->scratch_frames = 0;
    ctx->d_mid.reset();
    ctx->d_aud24.reset();
    const size_t per = (size_t)ctx->nchan * (size_t)n_frames * (size_t)(256 * plan.seg);  // fft_length / 2 per frame
    HIP_TRY(dev_alloc(ctx->d_mid, per * 2 * sizeof(float)));
    HIP_TRY(dev_alloc(ctx->d_aud24, per * 2 * sizeof(float)));  // complex when the back kernel demodulates
    ctx->scratch_frames = n_frames;
  }
  if (plan.nfm_atan_long) return fail(T41RX_ERR_UNSUPPORTED, plan.why);
  if (plan.pipe_buffer && !ctx->d_agc_pipe) {
    const size_t bytes = pipe_layout(ctx->nchan).bytes;
    DevBuf<char> pipe;  // the context only ever sees a buffer whose counters are zero
    HIP_TRY(dev_alloc(pipe, bytes));
    HIP_TRY(hipMemset(pipe.get(), 0, bytes));
    ctx->d_agc_pipe = std::move(pipe);
  }
  // (staged parameter sets ending in the fused back kernel: its set twin is an output-map form, run with the identity)
  const bool ident_back = sets_staged(ctx) && plan.back == Back::back512 && !ctx->out_map_on;
  if ((plan.need_ident || ident_back) && !ctx->d_ident) {  // 0, 1, ..: the map of a mapped form's call without one of the caller's
    std::vector<int32_t> ident((size_t)ctx->nchan);
    for (int i = 0; i < ctx->nchan; ++i) ident[(size_t)i] = i;
    DevBuf<int32_t> fresh;
    HIP_TRY(dev_alloc(fresh, sizeof(int32_t) * ident.size()));
    HIP_TRY(hipMemcpy(fresh.get(), ident.data(), sizeof(int32_t) * ident.size(), hipMemcpyHostToDevice));
    ctx->d_ident = std::move(fresh);
  }
  if (ctx->params.AGCMode != 0 && (int)blob_view(ctx->blob.data()).agc[kAgcAttackBuffsize] != kAgcDelay)
    return fail(T41RX_ERR_STATE, "coefficient blob carries an AGC look-ahead the kernel is not built for");
  if (!plan.valid) return fail(T41RX_ERR_STATE, plan.why);  // (the setters keep these apart: not reached)
  if ((ctx->dbg_nco || ctx->dbg_dec || ctx->dbg_demod) && n_frames > ctx->tap_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the debug tap buffers were set with");
  if (ctx->spect && n_frames > ctx->spect_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the audio-spectrum buffers were set with");
  if (ctx->disp.spec && n_frames > ctx->disp.frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the display-spectrum buffers were set with");
  if (cw_dec_on(ctx) && n_frames > ctx->cw.text_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the CW decoder's buffer was set with");
  if (cw_det_on(ctx) && n_frames > ctx->cw.frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the CW detector's buffer was set with");
  int split_ch = -1, split_set = -1;
  if (cw_det_on(ctx))
    if (const char *stage = cw_split_stage(ctx, &split_ch, &split_set))
      return fail(T41RX_ERR_UNSUPPORTED, std::string("CW detector: the ") + stage +
                                             (split_ch < 0    ? std::string()
                                              : split_set < 0 ? " of channel " + std::to_string(split_ch) + " (noise-reduction map)"
                                                              : " of channel " + std::to_string(split_ch) + " (parameter set " + std::to_string(split_set) + ")") +
                                             " leaves float_buffer_L different from float_buffer_R and neither the notch nor the noise "
                                             "blanker joins them behind it; the library carries one audio stream");
  if (ctx->disp.spec && (!ctx->disp.d_pre || !ctx->disp.d_state || !ctx->d_win)) return fail(T41RX_ERR_STATE, "display spectrum enabled without its buffers");
  if (ctx->ft8.on && (rc = ft8_prepare(ctx, plan, n_frames, s)) != T41RX_OK) return rc;
  // the decoder's words, behind every refusal: its checkpoint section appears with the first call in which it runs
  if (cw_dec_on(ctx) && (rc = ensure_cw_decode(ctx)) != T41RX_OK) return rc;
  return T41RX_OK;
}

// (b) the kernels' arguments
RxArgs rx_args(t41rx_ctx *ctx, const CallPlan &plan, const float *dI, const float *dQ, float *dAudio, int n_frames, bool q15) {
  RxArgs a{};
  a.I = dI;
  a.Q = dQ;
  a.out = dAudio;
  a.state = ctx->d_state.get();
  a.coef = ctx->d_coef.get();
  a.tab = ctx->d_tab.get();
  a.nco = ctx->d_nco.get();
  a.nchan = ctx->nchan;
  a.nframes = plan.seg * n_frames;  // 2048-sample segments
  {  // time-major: [frame][channel][frame_len] (fft_length 512: set_buffer_layout / set_params)
    const Strides io = strides_of(ctx, ctx->nchan, a.nframes, 2048);
    a.chan_stride = io.chan;
    a.frame_stride = io.frame;
  }
  if (ctx->n_streams > 0) {  // receiver groups: I / Q hold n_streams rows in the same layout, the output nchan as above
    const Strides in = strides_of(ctx, ctx->n_streams, a.nframes, 2048);
    a.in_map = ctx->d_in_map.get();
    a.in_chan_stride = in.chan;
    a.in_frame_stride = in.frame;
  }
  a.seg = plan.seg;
  a.nframes4k = n_frames;
  a.mid = ctx->d_mid.get();
  a.aud24 = ctx->d_aud24.get();
  a.tab4k = ctx->d_tab4k.get();
  {
    SetGains g;
    a.plain = gains_of(blob_view(ctx->blob.data()).scalars, g) ? 1 : 0;
    a.g_rf = g.g_rf;
    a.g_band = g.g_band;
    a.neg_iq_amp = g.neg_iq_amp;
    a.iq_phase = g.iq_phase;
    a.iq_corr_on = g.iq_corr_on;
  }
  if (sets_loaded(ctx)) {
    // parameter sets: the arrays [K + 1] in place of set 0's block and table, the channels' table and the sets' gains.
    // The rule (t41rx_param_sets_compatible) makes everything else in here -- plain, agc, nfm_atan, the pipelined
    // form -- the same for every set
    a.coef = ctx->sets.d_coef.get();
    a.tab = ctx->sets.d_tab.get();
    a.set_of = ctx->sets.d_set_of.get();
    a.set_gain = ctx->sets.d_gain.get();
  }
  if (plan.need_ident) {  // the input keeps its place under the map's strides
    a.in_map = ctx->d_ident.get();
    a.in_chan_stride = a.chan_stride;
    a.in_frame_stride = a.frame_stride;
  }
  a.q15 = q15 ? 1 : 0;
  a.nco_rd = ctx->nco_sel;
  a.ovl_real = ctx->params.mode == T41RX_DEMOD_NFM ? 1 : 0;
  a.nfm_atan = (ctx->params.mode == T41RX_DEMOD_NFM && ctx->params.nfm_demod == 1) ? 1 : 0;
  {
    // Segment-parallel kernels of the long-FFT pipeline: about 4096 wave slots (256 CUs x 16) to
    // fill; a wave that starts inside the call pays one extra sub-block to rebuild its filter
    // memories, so runs are as long as still gives every slot a wave (and never longer than 8).
    const long segs = (long)a.nframes, waves = 4096;
    long run = (long)ctx->nchan * segs / waves;
    if (ctx->seg_run_set) run = ctx->seg_run;  // the tests' hook (T41RX_SEG_RUN at creation)
    a.seg_run = (int)(run < 1 ? 1 : (run > 8 ? 8 : (run > segs ? segs : run)));
  }
  a.agc = ctx->params.AGCMode != 0 ? 1 : 0;
  if (plan.pipe_buffer) a.agc_pipe = reinterpret_cast<float *>(ctx->d_agc_pipe.get());
  a.dbg_pre = ctx->disp.spec ? ctx->disp.d_pre.get() : nullptr;
  a.dbg_nco = ctx->dbg_nco;
  a.dbg_dec = ctx->dbg_dec;
  a.dbg_demod = ctx->dbg_demod;
  if (plan.ft8_own_tap) a.dbg_demod = ctx->ft8.d_tap.get();  // the FT8 stage reads the demod tap
  a.spect = ctx->spect;
  a.spect_max = ctx->spect_max;
  if (pan_call_rows(ctx)) {
    // the panadapter owns the display taps (one owner each: the setters refuse the other): compact rows for the call's
    // update frames.  A call without one sets no tap and so launches what a context without the stage launches.
    a.dbg_pre = ctx->pan.d_pre.get();
    a.spect = ctx->pan.out.audio_spect;
    a.spect_max = ctx->pan.d_max.get();
    a.tap_period = ctx->pan.period;
    a.tap_first = ctx->pan.call_first;
    a.tap_rows = ctx->pan.max_rows;
    if (ctx->pan.map_on) a.tap_map = ctx->pan.d_map.get();  // the taps by row, [n_rows][max_rows], for the listed channels only
  }
  // the kernel stops behind the demodulator.  (At 24 kS/s the strides above stay the input's: a tap kernel without a map
  // places its input with them, and stores no audio)
  if (plan.handover) a.aud_out = ctx->d_aud24.get();
  if (plan.form.a24_form) {  // 24 kS/s from the fused kernel: the output's strides count frames of 256
    const Strides o = strides_of(ctx, audio_rows(ctx), a.nframes, 256);
    a.chan_stride = o.chan;
    a.frame_stride = o.frame;
  } else if (plan.form.omap_form) {  // an output map on the fused kernel (a mapped form: the input has its own strides): n_rows rows
    const Strides o = strides_of(ctx, audio_rows(ctx), a.nframes, 2048);
    a.chan_stride = o.chan;
    a.frame_stride = o.frame;
  }
  // the output map: the fused twins read it, and the back kernels behind a hand-over (launch_chain)
  if (ctx->out_map_on) a.out_map = ctx->d_out_map.get();
  return a;
}

}  // namespace

// the finish of a 24 kS/s call that left its audio in the scratch (Back::finish24, Back::cw_24k): volume, q15 conversion, the call's layout
int t41::aud24_finish_run(t41rx_ctx *ctx, const RxArgs &a, int n_frames, hipStream_t s) {
  const Strides o = strides_of(ctx, audio_rows(ctx), n_frames, 256);  // (an output map: n_rows rows)
  Aud24Args f{};
  f.aud = ctx->d_aud24.get();
  f.out = a.out;
  f.chan_stride = o.chan;
  f.frame_stride = o.frame;
  f.nchan = ctx->nchan;
  f.nframes = n_frames;
  f.q15 = a.q15;
  f.coef = a.coef;      // (with parameter sets: the sets' array and the channels' table)
  f.set_of = a.set_of;
  f.out_map = a.out_map;
  return hip_check(launch_aud24_finish(f, s), "24 kS/s finish kernel launch");
}

namespace {

// (c) the stage chain: fused front end, FT8 on the demodulated audio, then on the audio @24 kS/s the equalizer, noise
// reduction / notch and the blanker, the CW detector, decoder and narrow filter, the back end, and the display stages
int launch_chain(t41rx_ctx *ctx, const CallPlan &plan, RxArgs a, int n_frames, hipStream_t s) {
  int rc = hip_check(launch_rx(a, plan, s), "kernel launch");
  if (rc != T41RX_OK) return rc;
  if (ctx->ft8.on && (rc = ft8_run(ctx, plan, a, n_frames, s)) != T41RX_OK) return rc;
  if (ctx->eq.on && (rc = eq_run(ctx, n_frames, s)) != T41RX_OK) return rc;
  if (nr_on(ctx) && (rc = nr_run(ctx, n_frames, s)) != T41RX_OK) return rc;
  if (ctx->nb.on && (rc = nb_run(ctx, n_frames, s)) != T41RX_OK) return rc;
  if (cw_det_on(ctx) && (rc = cw_detect_run(ctx, n_frames, s)) != T41RX_OK) return rc;
  if (cw_dec_on(ctx) && (rc = cw_decode_run(ctx, n_frames, s)) != T41RX_OK) return rc;
  if (plan.handover && a.out_map) {
    // an output map behind the hand-over: the tap kernel placed its input with the strides so far and stored no audio;
    // the back kernels place n_rows rows
    const Strides o = strides_of(ctx, audio_rows(ctx), a.nframes, 2048);
    a.chan_stride = o.chan;
    a.frame_stride = o.frame;
  }
  switch (plan.back) {
    case Back::cw_back:
    case Back::cw_24k:
    case Back::cw_mixed:
      rc = cw_filter_run(ctx, plan, a, n_frames, s);
      break;
    case Back::finish24:
      // 24 kS/s: the volume and the stores alone (Process.cpp:929-937 without DF); the interpolator memories stay as they are
      rc = aud24_finish_run(ctx, a, n_frames, s);
      break;
    case Back::back512:
      // then the interpolators, volume and stores (Process.cpp:917-937) from a.aud24
      a.aud_out = nullptr;
      // parameter sets next to the stages: the back kernel's set twin is its output-map form; without a map of the
      // caller's every channel stores to its own row (the strides are those of n_channels rows already)
      if (a.set_of && !a.out_map) a.out_map = ctx->d_ident.get();
      rc = hip_check(launch_back512(a, s), "interpolator kernel launch");
      break;
    case Back::fused:
    case Back::long_pipe:
      break;  // the front kernels stored the audio
  }
  if (rc != T41RX_OK) return rc;
  if (a.seg > 1) ctx->nco_sel ^= 1;  // the kernels wrote the other copy
  if (ctx->disp.spec && (rc = display_run(ctx, n_frames, s)) != T41RX_OK) return rc;
  if (ctx->pan.on && (rc = pan_run(ctx, n_frames, s)) != T41RX_OK) return rc;
  // the beacon monitor reads the rows the panadapter wrote: a call without an update frame launches nothing for it
  if (ctx->beacon.on && ctx->pan.last_rows > 0 && (rc = beacon_run(ctx, s)) != T41RX_OK) return rc;
  return T41RX_OK;
}

int process_device_impl(t41rx_ctx *ctx, const float *dI, const float *dQ, float *dAudio, int n_frames,
                        void *hip_stream, bool q15) {
  // (an output map with no row, t41rx_set_output_map: no audio is written and the pointer is not looked at)
  const bool no_audio = ctx && audio_rows(ctx) == 0;
  if (no_audio) dAudio = nullptr;
  if (!ctx || !dI || !dQ || (!dAudio && !no_audio)) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  if ((reinterpret_cast<uintptr_t>(dI) | reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dAudio)) & 15u)
    return fail(T41RX_ERR_ARG, "I/Q/audio device pointers must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const hipStream_t s = (hipStream_t)hip_stream;
  // the panadapter stage: which frames of this call are update frames, in front of the plan and everything that allocates
  int rc = pan_prepare(ctx, n_frames);
  if (rc != T41RX_OK) return rc;
  const CallPlan plan = plan_call(call_facts(ctx, n_frames, q15));
  if ((rc = prepare_call(ctx, plan, n_frames, s)) != T41RX_OK) return rc;
  return launch_chain(ctx, plan, rx_args(ctx, plan, dI, dQ, dAudio, n_frames, q15), n_frames, s);
}

// staging buffers of the host-pointer entry points, sized in bytes per array: the two inputs (with an input map they
// hold n_streams rows, the output n_channels) and the output
int ensure_staging(t41rx_ctx *ctx, size_t in_bytes, size_t out_bytes) {
  Staging &st = ctx->staging;
  if (in_bytes > st.in_floats * sizeof(float)) {
    st.in_floats = 0;
    st.d_in_i.reset();
    st.d_in_q.reset();
    const size_t nfl = (in_bytes + sizeof(float) - 1) / sizeof(float);
    HIP_TRY(dev_alloc(st.d_in_i, nfl * sizeof(float)));
    HIP_TRY(dev_alloc(st.d_in_q, nfl * sizeof(float)));
    st.in_floats = nfl;
  }
  if (out_bytes > st.out_floats * sizeof(float)) {
    st.out_floats = 0;
    st.d_out.reset();
    const size_t nfl = (out_bytes + sizeof(float) - 1) / sizeof(float);
    HIP_TRY(dev_alloc(st.d_out, nfl * sizeof(float)));
    st.out_floats = nfl;
  }
  return T41RX_OK;
}

}  // namespace

extern "C" {

int t41rx_abi_version(void) { return T41RX_ABI_VERSION; }

const char *t41rx_strerror(int status) {
  switch (status) {
    case T41RX_OK: return "ok";
    case T41RX_ERR_ARG: return "invalid argument";
    case T41RX_ERR_UNSUPPORTED: return "not supported by this build";
    case T41RX_ERR_HIP: return "HIP runtime/device error";
    case T41RX_ERR_NOMEM: return "out of memory";
    case T41RX_ERR_STATE: return "blob/state mismatch";
    default: return "unknown status";
  }
}

const char *t41rx_last_error(void) { return g_last_error.c_str(); }

int t41rx_supported_fft_length(int fft_length) {
  return (fft_length == 512 || fft_length == 1024 || fft_length == 2048 || fft_length == 4096) ? 1 : 0;
}

void t41rx_default_params(t41rx_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->fft_length = 512;               // SDT.h:39
  p->mode = T41RX_DEMOD_USB;         // bands[] 20 m row, T41_SDR.ino:163
  p->FLoCut = 200;
  p->FHiCut = 3000;
  p->rfGainAllBands = 1;             // gwv.cpp:17
  p->RFgain = 1;                     // bands[].RFgain
  p->IQAmpCorrectionFactor = 1.0f;   // gwv.cpp:71
  p->IQPhaseCorrectionFactor = 0.0f; // gwv.cpp:72
  p->AGCMode = 0;                    // firmware default is 1 (gwv.cpp:15); 0 = fixed gain
  p->audioVolume = 30;               // gwv.cpp:16
  p->nfmFilterBW = 12000;            // Filter.cpp:16
  p->xmtMode = T41RX_SSB_MODE;       // gwv.cpp:22
  p->CWFreqShift = 750;
  p->am_lpf_f0 = 3000;               // boot band 40 m: max(FHiCut, -FLoCut) = 3000
  p->AGC_thresh = 20;                // bands[] "AGC" column, T41_SDR.ino:145-168
  p->nrOptionSelect = 0;             // gwv.cpp:23
  p->ANR_notchOn = 0;                // Process.cpp:45
  p->NR_PSI = 0.0;                   // gwv.cpp:61-63
  p->NR_alpha = 0.95;
  p->NR_beta = 0.85;
}

size_t t41rx_coeff_blob_bytes(int fft_length) {
  if (!(fft_length == 512 || fft_length == 1024 || fft_length == 2048 || fft_length == 4096)) return 0;
  return blob_floats(fft_length) * sizeof(float);
}

int t41rx_design_coeffs(const t41rx_params *p, void *blob, size_t blob_bytes) {
  if (!p || !blob) return fail(T41RX_ERR_ARG, "null argument");
  const char *why = nullptr;
  if (!params_valid(*p, &why)) return fail(T41RX_ERR_ARG, why ? why : "bad params");
  if (blob_bytes < t41rx_coeff_blob_bytes(p->fft_length)) return fail(T41RX_ERR_ARG, "blob buffer too small");
  return design_blob(*p, blob, blob_bytes);
}

int t41rx_create(t41rx_ctx **out, int device_id, int n_channels, const t41rx_params *p) {
  // A library whose kernels were built with diagnostics (rx_experiments.hpp: -DT41RX_EXPERIMENT=1 with T41RX_STAMP /
  // _PIPE_STAT / _CLK) writes stamps or counters next to the samples: it may not stand in for the product by accident.
  // The tools that use such builds say so in the environment.
  if (kernel_build_flags() != 0) {
    const char *allow = std::getenv("T41RX_ALLOW_EXPERIMENT");
    if (!allow || std::atoi(allow) == 0)
      return fail(T41RX_ERR_UNSUPPORTED,
                  "this libt41rx was built with kernel diagnostics (stamps / counters); set T41RX_ALLOW_EXPERIMENT=1 to use it");
    static bool warned = false;
    if (!warned) {
      warned = true;
      std::fprintf(stderr, "libt41rx: EXPERIMENT BUILD (kernel_build_flags %d) -- diagnostics on\n", kernel_build_flags());
    }
  }

  if (!out || !p) return fail(T41RX_ERR_ARG, "null argument");
  *out = nullptr;
  if (n_channels <= 0) return fail(T41RX_ERR_ARG, "n_channels must be > 0");
  const char *why = nullptr;
  if (!params_valid(*p, &why)) return fail(T41RX_ERR_ARG, why ? why : "bad params");

  if (!t41rx_supported_fft_length(p->fft_length)) return fail(T41RX_ERR_UNSUPPORTED, "no kernel for this fft_length");

  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail(T41RX_ERR_HIP, "no such HIP device");
  DeviceGuard g(device_id);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");

  std::unique_ptr<t41rx_ctx> ctx(new (std::nothrow) t41rx_ctx());  // (destroyed before g on the way out)
  if (!ctx) return fail(T41RX_ERR_NOMEM, "host allocation failed");
  ctx->device = device_id;
  ctx->nchan = n_channels;
  ctx->params = *p;
  ctx->blob.assign(blob_floats(p->fft_length), 0.0f);
  ctx->nco_hz.assign((size_t)n_channels, 0);
  if (const char *e = std::getenv("T41RX_SEG_RUN")) {  // a test hook, read here and nowhere else (include/t41rx.h)
    ctx->seg_run_set = true;
    ctx->seg_run = std::atol(e);
  }
  if (kernel_build_flags() != 0) {  // the diagnostic builds' own variables: a product library reads neither
    ctx->pipe_stat = std::getenv("T41RX_PIPE_STAT") != nullptr;
    ctx->stamp_taps = std::getenv("T41RX_STAMP_TAPS") != nullptr;
  }
  int rc = design_blob(*p, ctx->blob.data(), ctx->blob.size() * sizeof(float));
  if (rc != T41RX_OK) return fail(rc, "coefficient design failed");
  hipError_t e;
  const size_t sbytes = sizeof(float) * state_floats(p->fft_length) * (size_t)n_channels;
  if ((e = dev_alloc(ctx->d_state, sbytes)) != hipSuccess || (e = dev_alloc(ctx->d_coef, sizeof(DevCoef))) != hipSuccess ||
      (e = dev_alloc(ctx->d_tab, sizeof(float2) * kTabEntries512)) != hipSuccess ||
      (e = dev_alloc(ctx->d_nco, sizeof(ChanNco) * (size_t)n_channels)) != hipSuccess ||
      (p->fft_length != 512 && (e = dev_alloc(ctx->d_tab4k, sizeof(float2) * tab_long_entries(p->fft_length / 512))) != hipSuccess))
    return hip_fail(e, "hipMalloc");
  if ((rc = upload_coeffs(ctx.get())) != T41RX_OK || (rc = upload_nco(ctx.get())) != T41RX_OK ||
      (rc = reset_state(ctx.get())) != T41RX_OK)
    return rc;
  *out = ctx.release();
  return T41RX_OK;
}

int t41rx_destroy(t41rx_ctx *ctx) {
  if (!ctx) return T41RX_OK;
  DeviceGuard g(ctx->device);
  (void)hipDeviceSynchronize();
  if (ctx->d_agc_pipe && ctx->pipe_stat) {  // the diagnostic build's counters (rx_chains.hpp: PIPE_STAT_*)
    unsigned long long c[16] = {};
    std::vector<unsigned long long> all((size_t)ctx->nchan * 16);
    (void)hipMemcpy(all.data(), ctx->d_agc_pipe.get() + pipe_layout(ctx->nchan).counters, all.size() * sizeof(unsigned long long),
                    hipMemcpyDeviceToHost);
    for (size_t i = 0; i < all.size(); ++i) c[i & 15] += all[i];
    std::fprintf(stderr, "pipe_stat chain_cycles %llu chains %llu slow_blocks %llu back_wait %llu duty_wait %llu blocks %llu chain_stage %llu chain_steps %llu front %llu prep %llu back %llu wave_iterations %llu chain_state_wait %llu\n",
                 c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], c[12]);
  }
  ft8_decode_release(ctx);
  delete ctx;  // (its device buffers go here, on its device)
  return T41RX_OK;
}

int t41rx_set_params(t41rx_ctx *ctx, const t41rx_params *p) {
  if (!ctx || !p) return fail(T41RX_ERR_ARG, "null argument");
  const char *why = nullptr;
  if (!params_valid(*p, &why)) return fail(T41RX_ERR_ARG, why ? why : "bad params");
  if (p->fft_length != ctx->params.fft_length) return fail(T41RX_ERR_ARG, "fft_length cannot change on a live context");
  if (sets_loaded(ctx))  // (the rule's text stands; staged sets: and the spectral check of set 0's channels)
    if (const int src = sets_check_set0(ctx, *p)) return src;
  if (nr_map_check_params(ctx, *p) != T41RX_OK) return T41RX_ERR_ARG;  // (a noise-reduction map with an entry 2: the pass band's check)

  std::vector<float> nb(ctx->blob.size());
  int rc = design_blob(*p, nb.data(), nb.size() * sizeof(float));
  if (rc != T41RX_OK) return fail(rc, "coefficient design failed");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  ctx->blob.swap(nb);
  ctx->params = *p;
  if ((rc = upload_coeffs(ctx)) != T41RX_OK) return rc;
  if (sets_loaded(ctx) && (rc = sets_upload(ctx)) != T41RX_OK) return rc;  // entry 0 of the set arrays
  if ((rc = pan_map_refresh(ctx)) != T41RX_OK) return rc;  // (a panadapter map: the listed channels' gains of set 0)
  return upload_nco(ctx);  // the CW side-tone offset may have changed
}

int t41rx_get_params(const t41rx_ctx *ctx, t41rx_params *p) {
  if (!ctx || !p) return fail(T41RX_ERR_ARG, "null argument");
  *p = ctx->params;
  return T41RX_OK;
}

int t41rx_get_coeffs(const t41rx_ctx *ctx, void *blob, size_t blob_bytes) {
  if (!ctx || !blob) return fail(T41RX_ERR_ARG, "null argument");
  const size_t need = ctx->blob.size() * sizeof(float);
  if (blob_bytes < need) return fail(T41RX_ERR_ARG, "blob buffer too small");
  std::memcpy(blob, ctx->blob.data(), need);
  return T41RX_OK;
}

int t41rx_set_coeffs(t41rx_ctx *ctx, const void *blob, size_t blob_bytes) {
  if (!ctx || !blob) return fail(T41RX_ERR_ARG, "null argument");
  const size_t need = ctx->blob.size() * sizeof(float);
  if (blob_bytes < need) return fail(T41RX_ERR_STATE, "blob too small for this context");
  const int32_t *h = reinterpret_cast<const int32_t *>(blob);
  if ((uint32_t)h[0] != kBlobMagic || h[1] != T41RX_ABI_VERSION) return fail(T41RX_ERR_STATE, "bad blob header");
  if (h[2] != ctx->params.fft_length) return fail(T41RX_ERR_STATE, "blob fft_length differs from the context");
  if ((h[3] < T41RX_DEMOD_USB || h[3] > T41RX_DEMOD_NFM) && h[3] != T41RX_DEMOD_SAM) return fail(T41RX_ERR_STATE, "bad demodulation mode in blob");
  // the parameters the blob was designed for become the context's (every rank that installs a
  // broadcast blob then runs -- and later re-designs from -- the designer's parameters)
  if (h[4] != (int32_t)sizeof(t41rx_params)) return fail(T41RX_ERR_STATE, "blob carries another t41rx_params layout");
  t41rx_params bp;
  std::memcpy(&bp, h + 8, sizeof(bp));
  const char *why = nullptr;
  if (!params_valid(bp, &why) || bp.fft_length != h[2] || bp.mode != h[3])
    return fail(T41RX_ERR_STATE, std::string("blob parameters invalid: ") + (why ? why : "header mismatch"));
  if (sets_loaded(ctx))  // (the rule's text stands; staged sets: and the spectral check of set 0's channels)
    if (const int src = sets_check_set0(ctx, bp)) return src;
  if (nr_map_check_params(ctx, bp) != T41RX_OK) return T41RX_ERR_ARG;

  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  std::memcpy(ctx->blob.data(), blob, need);
  ctx->params = bp;
  int rc = upload_coeffs(ctx);
  if (rc != T41RX_OK) return rc;
  if (sets_loaded(ctx) && (rc = sets_upload(ctx)) != T41RX_OK) return rc;  // entry 0 of the set arrays
  if ((rc = pan_map_refresh(ctx)) != T41RX_OK) return rc;  // (a panadapter map: the listed channels' gains of set 0)
  return upload_nco(ctx);
}

int t41rx_set_nco_freq(t41rx_ctx *ctx, const int32_t *nco_freq_hz, int n) {
  if (!ctx || !nco_freq_hz) return fail(T41RX_ERR_ARG, "null argument");
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "n must equal n_channels");
  for (int i = 0; i < n; ++i)
    if (nco_freq_hz[i] < -96000 || nco_freq_hz[i] > 96000) return fail(T41RX_ERR_ARG, "NCOFreq beyond +-Fs/2");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  std::memcpy(ctx->nco_hz.data(), nco_freq_hz, sizeof(int32_t) * (size_t)n);
  return upload_nco(ctx);
}

int t41rx_set_buffer_layout(t41rx_ctx *ctx, int layout) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (layout != T41RX_LAYOUT_CHANNEL_MAJOR && layout != T41RX_LAYOUT_TIME_MAJOR) return fail(T41RX_ERR_ARG, "unknown buffer layout");
  if (layout == T41RX_LAYOUT_TIME_MAJOR && ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "the time-major layout is built for fft_length 512 (the long-FFT pipeline's kernels walk a channel's samples contiguously)");
  ctx->layout = layout;
  return T41RX_OK;
}
int t41rx_get_buffer_layout(const t41rx_ctx *ctx) { return ctx ? ctx->layout : T41RX_ERR_ARG; }

int t41rx_set_input_map(t41rx_ctx *ctx, const int32_t *stream_of_channel, int n, int n_streams) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ", n_streams " + std::to_string(n_streams) + ")";
  if (!stream_of_channel) {
    if (n_streams != 0) return fail(T41RX_ERR_ARG, "input map: a null map switches the map off and takes n_streams 0" + counts);
    DeviceGuard g(ctx->device);
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the map they found)
    ctx->n_streams = 0;
    return T41RX_OK;
  }
  // everything is checked here, on the host, before anything changes: the kernels index I / Q with these entries unchecked
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "input map: n (" + std::to_string(n) + ") must equal n_channels" + counts);
  if (n_streams < 1 || n_streams > ctx->nchan) return fail(T41RX_ERR_ARG, "input map: n_streams must lie in [1, n_channels]" + counts);
  for (int i = 0; i < n; ++i)
    if (stream_of_channel[i] < 0 || stream_of_channel[i] >= n_streams)
      return fail(T41RX_ERR_ARG, "input map: channel " + std::to_string(i) + " names stream " + std::to_string(stream_of_channel[i]) +
                                     ", outside [0, n_streams)" + counts);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<int32_t> fresh;  // (the first map; later ones reuse the buffer: a failure leaves the previous map whole)
  if (!ctx->d_in_map) HIP_TRY(dev_alloc(fresh, sizeof(int32_t) * (size_t)n));
  HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->d_in_map.get(), stream_of_channel, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
  if (fresh) ctx->d_in_map = std::move(fresh);
  ctx->in_map.assign(stream_of_channel, stream_of_channel + n);
  ctx->n_streams = n_streams;
  return T41RX_OK;
}

int t41rx_get_input_map(const t41rx_ctx *ctx, int32_t *stream_of_channel_out, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (ctx->n_streams > 0 && stream_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "input map: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    std::memcpy(stream_of_channel_out, ctx->in_map.data(), sizeof(int32_t) * (size_t)n);
  }
  return ctx->n_streams;
}

int t41rx_set_audio_rate(t41rx_ctx *ctx, int rate) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (rate != T41RX_AUDIO_RATE_192K && rate != T41RX_AUDIO_RATE_24K) return fail(T41RX_ERR_ARG, "unknown audio rate");
  if (rate == T41RX_AUDIO_RATE_24K && ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "audio at 24 kS/s is built for fft_length 512 (the long-FFT pipeline's back kernel interpolates and stores at 192 kS/s)");
  ctx->audio_rate = rate;  // (calls in flight were launched with the rate they found)
  return T41RX_OK;
}
int t41rx_get_audio_rate(const t41rx_ctx *ctx) { return ctx ? ctx->audio_rate : T41RX_ERR_ARG; }
int t41rx_audio_frame_len(const t41rx_ctx *ctx) { return ctx ? audio_frame_len(ctx) : T41RX_ERR_ARG; }

int t41rx_n_channels(const t41rx_ctx *ctx) { return ctx ? ctx->nchan : T41RX_ERR_ARG; }
int t41rx_frame_len(const t41rx_ctx *ctx) { return ctx ? 4 * ctx->params.fft_length : T41RX_ERR_ARG; }

int t41rx_process_device(t41rx_ctx *ctx, const float *dI, const float *dQ, float *dAudio, int n_frames,
                         void *hip_stream) {
  return process_device_impl(ctx, dI, dQ, dAudio, n_frames, hip_stream, false);
}

// float_buffer_L (= I) is filled from the R queue and float_buffer_R (= Q) from the L queue
// (Process.cpp:107-108)
int t41rx_process_device_q15(t41rx_ctx *ctx, const int16_t *dQ_in_L, const int16_t *dQ_in_R, int16_t *dQ_out_L,
                             int n_frames, void *hip_stream) {
  return process_device_impl(ctx, reinterpret_cast<const float *>(dQ_in_R), reinterpret_cast<const float *>(dQ_in_L),
                             reinterpret_cast<float *>(dQ_out_L), n_frames, hip_stream, true);
}

int t41rx_process_host_q15(t41rx_ctx *ctx, const int16_t *Q_in_L, const int16_t *Q_in_R, int16_t *Q_out_L, int n_frames) {
  if (!ctx || !Q_in_L || !Q_in_R || (!Q_out_L && audio_rows(ctx) != 0)) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const size_t in_bytes = (size_t)input_rows(ctx) * (size_t)n_frames * (size_t)(4 * ctx->params.fft_length) * sizeof(int16_t);  // an input map: n_streams rows come in
  const size_t bytes = (size_t)audio_rows(ctx) * (size_t)n_frames * (size_t)audio_frame_len(ctx) * sizeof(int16_t);  // an output map: n_rows rows go out
  int rc = ensure_staging(ctx, in_bytes, bytes);
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipMemcpy(ctx->staging.d_in_i.get(), Q_in_L, in_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->staging.d_in_q.get(), Q_in_R, in_bytes, hipMemcpyHostToDevice));
  if (audio_rows_unused(ctx)) HIP_TRY(hipMemcpy(ctx->staging.d_out.get(), Q_out_L, bytes, hipMemcpyHostToDevice));  // (unused rows are not written)
  rc = t41rx_process_device_q15(ctx, reinterpret_cast<const int16_t *>(ctx->staging.d_in_i.get()), reinterpret_cast<const int16_t *>(ctx->staging.d_in_q.get()),
                                reinterpret_cast<int16_t *>(ctx->staging.d_out.get()), n_frames, nullptr);
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (bytes) HIP_TRY(hipMemcpy(Q_out_L, ctx->staging.d_out.get(), bytes, hipMemcpyDeviceToHost));
  return pipe_status(ctx);  // (these calls synchronise: samples of a run whose hand-over broke do not leave with OK)
}

int t41rx_process_host(t41rx_ctx *ctx, const float *I, const float *Q, float *audio, int n_frames) {
  if (!ctx || !I || !Q || (!audio && audio_rows(ctx) != 0)) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const size_t in_fl = (size_t)input_rows(ctx) * (size_t)n_frames * (size_t)(4 * ctx->params.fft_length);  // an input map: n_streams rows come in
  const size_t nfl = (size_t)audio_rows(ctx) * (size_t)n_frames * (size_t)audio_frame_len(ctx);  // an output map: n_rows rows go out
  {
    const int rc0 = ensure_staging(ctx, in_fl * sizeof(float), nfl * sizeof(float));
    if (rc0 != T41RX_OK) return rc0;
  }
  HIP_TRY(hipMemcpy(ctx->staging.d_in_i.get(), I, in_fl * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->staging.d_in_q.get(), Q, in_fl * sizeof(float), hipMemcpyHostToDevice));
  if (audio_rows_unused(ctx)) HIP_TRY(hipMemcpy(ctx->staging.d_out.get(), audio, nfl * sizeof(float), hipMemcpyHostToDevice));  // (unused rows are not written)
  int rc = t41rx_process_device(ctx, ctx->staging.d_in_i.get(), ctx->staging.d_in_q.get(), ctx->staging.d_out.get(), n_frames, nullptr);
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (nfl) HIP_TRY(hipMemcpy(audio, ctx->staging.d_out.get(), nfl * sizeof(float), hipMemcpyDeviceToHost));
  return pipe_status(ctx);  // (these calls synchronise: samples of a run whose hand-over broke do not leave with OK)
}

int t41rx_set_debug_taps(t41rx_ctx *ctx, float *d_post_nco, float *d_dec, float *d_demod, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const bool any = d_post_nco || d_dec || d_demod;
  // (T41RX_STAMP_TAPS: the -DT41RX_STAMP diagnostic kernels of the long-FFT pipeline put their cycle stamps behind the demod tap)
  if (any && ctx->params.fft_length != 512 && !ctx->stamp_taps)
    return fail(T41RX_ERR_UNSUPPORTED, "the stage taps are built for fft_length 512");
  if (any && max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
  ctx->dbg_nco = d_post_nco;
  ctx->dbg_dec = d_dec;
  ctx->dbg_demod = d_demod;
  ctx->tap_frames = any ? max_frames : 0;
  return T41RX_OK;
}

int t41rx_set_audio_spectrum(t41rx_ctx *ctx, float *d_spect, float *d_max, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null context");
  if ((d_spect == nullptr) != (d_max == nullptr)) return fail(T41RX_ERR_ARG, "set both pointers or neither");
  if (d_spect && ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the audio spectrum is built for fft_length 512");
  if ((reinterpret_cast<uintptr_t>(d_spect) | reinterpret_cast<uintptr_t>(d_max)) & 3u) return fail(T41RX_ERR_ARG, "unaligned pointer");
  if (d_spect && max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
  if (d_spect && ctx->pan.on) return fail(T41RX_ERR_UNSUPPORTED, "the panadapter stage is on and owns the audio-spectrum tap (t41rx_set_panadapter)");
  ctx->spect = d_spect;
  ctx->spect_max = d_max;
  ctx->spect_frames = d_spect ? max_frames : 0;
  return T41RX_OK;
}

}  // extern "C"
