// t41_sdr_amd/csrc/rx_host.cpp -- host side of the C ABI in include/t41rx.h.
//
// Owns what the reference keeps in firmware globals: the coefficient arrays
// (FIR_dec1_coeffs ... FIR_filter_mask, T41_SDR.ino:398-399, Filter.cpp:39-41), the CMSIS
// instance state (T41_SDR.ino:384-397), the oscillator state (Freq_Shift.cpp:13-14) and the
// overlap-save block (T41_SDR.ino:403-404) -- here per channel and resident in HBM.
// There is no CPU implementation of the path in this library: without a HIP device every
// create/process call fails with T41RX_ERR_HIP.
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

#include "cw_kernels.hpp"
#include "cw_kernel.hip"  // the CW receive stages' kernels and launchers
#include "dev_buf.hpp"
#include "eq_kernels.hpp"
#include "eq_kernel.hip"  // the receive equalizer's kernel and launcher
#include "ft8_kernels.hpp"
#include "ft8_kernel.hip"  // the FT8 receive stage's kernels and launchers
#include "ft8_decode_kernels.hpp"
#include "ft8_decode_kernel.hip"  // the FT8 decode's kernels and launcher
#include "last_error.hpp"
#include "nb_kernels.hpp"
#include "nb_kernel.hip"  // the noise blanker's kernel and launcher
#include "nr_kernels.hpp"
#include "panadapter_kernel.hip"  // the panadapter stage's kernel and launcher
#include "rx_experiments.hpp"
#include "rx_internal.hpp"
#include "rx_kernels.hpp"

using namespace t41;

struct t41rx_ctx {
  int device = 0;
  int nchan = 0;
  t41rx_params params{};
  std::vector<float> blob;       // canonical coefficient blob (host)
  std::vector<int32_t> nco_hz;   // NCOFreq per channel (host)
  DevBuf<float> d_state;         // [nchan][state_floats]
  DevBuf<DevCoef> d_coef;
  DevBuf<float2> d_tab;
  DevBuf<ChanNco> d_nco;
  float *dbg_nco = nullptr, *dbg_dec = nullptr, *dbg_demod = nullptr;
  float *spect = nullptr, *spect_max = nullptr;  // audio-spectrum side output (t41rx_set_audio_spectrum)
  int tap_frames = 0, spect_frames = 0;          // frames per call those buffers are sized for
  // display FFT side output (t41rx_set_display_spectrum)
  float *disp_spec = nullptr, *disp_old = nullptr;  // caller's buffers
  DevBuf<float> d_pre, d_disp;                       // input tap [nchan][disp_frames][4096], state [nchan][kDispFloats]
  DevBuf<double> d_win;
  int disp_frames = 0, disp_zoom = 0;
  // FFT_LENGTH 4096 pipeline: constant table + scratch between its three kernels
  DevBuf<float2> d_tab4k;
  DevBuf<float> d_mid, d_aud24;
  DevBuf<char> d_agc_pipe;  // FFT_LENGTH 512, AGC on or SAM: the pipelined kernels' buffer (pipe_layout), allocated on first use
  int scratch_frames = 0;
  int layout = T41RX_LAYOUT_CHANNEL_MAJOR;  // of I / Q / audio (t41rx_set_buffer_layout)
  int nco_sel = 0;               // long FFT: which NcoState copy is current (flips with every process call)
  // receiver groups (t41rx_set_input_map): channel c reads row in_map[c] of the n_streams rows of I / Q; n_streams == 0:
  // no map, one row per channel.  Configuration like `layout`: in no checkpoint, untouched by reset / set_state / set_params
  std::vector<int32_t> in_map;   // (host)
  int n_streams = 0;
  DevBuf<int32_t> d_in_map;      // [nchan], allocated with the first map
  // noise reduction / notch (Process.cpp:841-866): state of Xanr() and of the two spectral functions, window tables;
  // allocated when a call first needs them
  DevBuf<float> d_nr_anr, d_nr_spec, d_nr_tab;
  // noise blanker (NB_on, Process.cpp:873-876; t41rx_set_noise_blanker): AltNoiseBlanking()'s last_frame_end per channel,
  // two slots [2][nchan][kNbCarryPitch] (nb_kernel.hip); allocated when the blanker first runs
  int nb_on = 0;
  DevBuf<float> d_nb;
  int nb_sel = 0;  // the slot holding the current carry (flips with every blanker launch)
  // receive equalizer (receiveEQFlag, Process.cpp:828-832; t41rx_set_receive_eq): the caller's band table, the levels
  // (EEPROMData.equalizerRec, EEPROM.cpp:59: 100 each), and rec_EQ_Band1_state .. rec_EQ_Band14_state per channel
  // [nchan][kEqStateFloats] (eq_kernel.hip), allocated when the equalizer first runs
  int eq_on = 0;
  bool eq_have_bands = false;
  float eq_coef[kEqCoefs] = {};
  int32_t eq_levels[kEqBands] = {100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100};
  DevBuf<float> d_eq;
  // CW receive (Process.cpp:878-913; t41rx_set_cw_tables / _filter / _detector): the caller's filter tables and decode
  // FIR, CWFilterIndex (5 = off), decoderFlag with the caller's result buffer, and the stages' memories per channel
  // [nchan][kCwStateFloats] (cw_kernel.hip), allocated when a CW stage first runs.  Both stages run only while
  // params.xmtMode == T41RX_CW_MODE.
  int cw_filter = kCwFilters;
  int cw_det = 0;
  bool cw_have_filters = false, cw_have_fir = false;
  float cw_coef[kCwFilters * kCwFilterCoefs] = {};
  float cw_fir[kCwFirTaps] = {};
  float *cw_out = nullptr;  // [nchan][n_frames][4]
  int cw_frames = 0;        // frames per call cw_out is sized for
  DevBuf<float> d_cw;
  // the Morse decoder behind the detector (DoCWDecoding(), CWProcessing.cpp:519-639; t41rx_set_cw_decode_tree / _decoder /
  // _clock): the caller's bigMorseCodeTree, the switch with the caller's text buffer, the clock millis(n) = t0 +
  // floor(n * num / den), and the decoder's words per channel [nchan][kCwDecWords] (cw_kernels.hpp), allocated when the
  // decoder first runs.  It runs exactly when the detector runs and the switch is on.
  bool cw_have_tree = false;
  uint8_t cw_tree[kCwTreeChars + 3] = {};
  int cw_dec = 0;
  int32_t *cw_text = nullptr;  // [nchan][n_frames][2]
  int cw_text_frames = 0;      // frames per call cw_text is sized for
  int32_t cw_t0 = 0, cw_num = 32, cw_den = 3;  // 2048 samples at 192 kS/s
  DevBuf<int32_t> d_cwdec;
  // IQ calibration (ProcessIQData2() / PlotCalSpectrum(), Process2.cpp:352-397, 478-547; t41rx_set_calibration): its
  // settings, a correction candidate per channel, and the calibration memory [nchan][kCalFloats] (cal_kernel.hip),
  // allocated when calibration is first configured.  The context's own: no checkpoint section, no audio-path kernel
  // touches it.
  bool cal_on = false, cal_per_channel = false;
  int cal_zoom = 0, cal_base = 0, cal_lo0 = 0, cal_lo1 = 0, cal_width = 0;
  float cal_dbscale = 0.0f;
  DevBuf<float> d_cal, d_cal_corr;
  // the panadapter stage (ShowSpectrum() / DrawSmeterBar(), Display.cpp:240-504, 955-1030; t41rx_set_panadapter_tables /
  // _panadapter / _panadapter_levels): the caller's gradient[] (device copy), the settings, the caller's row buffers, the
  // levels per channel (device copies), the compact taps of a call's update frames [nchan][max_rows][...] that the tap
  // kernels write and panadapter_kernel reads, and the panadapter memory [nchan][kPanFloats] (rx_internal.hpp).  The
  // context's own: no checkpoint section, t41rx_set_state() leaves it alone.  The frame counter lives here, on the host.
  bool pan_on = false, pan_have_tables = false;
  t41rx_panadapter_out pan_out{};
  int pan_zoom = 0, pan_scale = 0, pan_pixel_offset = 0, pan_floor_y = 0, pan_period = 1, pan_phase = 0, pan_max_rows = 0;
  int pan_attenuator = 0;
  int pan_alloc_rows = 0;       // rows d_pan_pre / d_pan_max hold
  long long pan_counter = 0;    // frames processed since the setter / t41rx_reset() / t41rx_set_panadapter_counter()
  int pan_call_first = 0, pan_call_rows = 0;  // of the call being prepared: its first update frame, their number
  int pan_last_rows = 0;        // t41rx_get_panadapter(): rows the last call wrote, and the frame index of the first
  long long pan_last_first = -1;
  DevBuf<uint16_t> d_pan_grad;
  DevBuf<int32_t> d_pan_nf;
  DevBuf<float> d_pan_gc, d_pan_pre, d_pan_max, d_pan_mem;
  // FT8 receive up to the waterfall (Process.cpp:627-686, ft8.cpp:153-268; t41rx_set_ft8_tables / _ft8 / _ft8_clock /
  // t41rx_ft8_sync): the caller's window and mag_db (device copies), arm_rfft_q15's tables, the switch with the caller's
  // power and status buffers, the clock millis(n) = t0 + floor(n * num / den), and the FT8 memory per channel
  // [nchan][kFt8Words] (ft8_kernels.hpp), allocated at first use.  The context's own: no checkpoint section (its record is
  // t41rx_ft8_get_state / _set_state).  The stage reads the demodulated audio where the demod tap sits: d_aud24 when other
  // stages split the chain, else the caller's demod tap buffer, else d_ft8_tap.
  int ft8_on = 0;
  bool ft8_have_tables = false;
  uint8_t *ft8_power = nullptr;   // [nchan][2][kFt8HalfBytes]
  int32_t *ft8_status = nullptr;  // [nchan][n_frames][4]
  int ft8_frames = 0;             // frames per call ft8_status is sized for
  int32_t ft8_t0 = 0, ft8_num = 32, ft8_den = 3;  // 2048 samples at 192 kS/s
  DevBuf<int32_t> d_ft8;
  DevBuf<float> d_ft8_win, d_ft8_mag, d_ft8_tap;
  DevBuf<uint32_t> d_ft8_tab;
  int ft8_tap_frames = 0;
  // FT8 decode of a finished slot (ft8.cpp:270-616, 669-703, 727-790; t41rx_set_ft8_decode_tables / _ft8_decode /
  // _ft8_decode_debug, t41rx_ft8_decode_device / _host): the caller's kCostas_map, kGray_map, kNm, kMn, kNrw as validated
  // (device copy, with the positions worked out from them), kMax_candidates / kMin_score / kLDPC_iterations, the stage taps,
  // and the call's `select` on its way to the device: a pinned copy, an event behind its upload (the next call waits for
  // it before it overwrites the copy), the device array.  The decode reads the waterfall and the tables and touches no state.
  bool ft8d_have_tables = false;
  int ft8d_max_candidates = T41RX_FT8_MAX_CANDIDATES, ft8d_min_score = 40, ft8d_iterations = 10;
  float *ft8d_dbg_log174 = nullptr;
  uint8_t *ft8d_dbg_plain = nullptr;
  DevBuf<Ft8DecodeTables> d_ft8d_tab;
  DevBuf<int8_t> d_ft8d_sel;
  DevBuf<t41rx_ft8_result> d_ft8d_res;  // staging for t41rx_ft8_decode_host
  int8_t *h_ft8d_sel = nullptr;         // pinned
  hipEvent_t ft8d_sel_ev = nullptr;
  // staging for t41rx_process_host
  DevBuf<float> d_in_i, d_in_q, d_out;
  size_t staging_in_floats = 0, staging_floats = 0;  // floats d_in_i / d_in_q and d_out hold
};

namespace {
thread_local std::string g_last_error;  // t41rx_last_error(); t41tx_* failures set it too (tx_host.cpp)
}  // namespace

int t41::fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

namespace {

int hip_fail(hipError_t e, const char *what) {
  return fail(T41RX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
int hip_check(hipError_t e, const char *what) { return e == hipSuccess ? T41RX_OK : hip_fail(e, what); }
#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t e__ = (expr);                           \
    if (e__ != hipSuccess) return hip_fail(e__, #expr); \
  } while (0)

constexpr float kPiF = 3.1415926535897932384626433832795f;  // FIR.h:10
// displayScale[] (Display.cpp:127-135): dBScale, baseOffset -- the calibration's and the panadapter's pixel mapping
constexpr float kDbScale[5] = {10.0f, 20.0f, 40.0f, 100.0f, 200.0f};
constexpr int kBaseOffset[5] = {24, 10, 58, 120, 200};

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

int upload_nco(t41rx_ctx *ctx) {
  std::vector<ChanNco> h((size_t)ctx->nchan);
  const int side = (int)blob_view(ctx->blob.data()).scalars[kScSideTone];
  for (int i = 0; i < ctx->nchan; ++i) h[(size_t)i] = make_nco(ctx->nco_hz[(size_t)i], side);
  HIP_TRY(hipMemcpy(ctx->d_nco.get(), h.data(), sizeof(ChanNco) * h.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}

// blob -> device constant block + lane-ordered tables
int upload_coeffs(t41rx_ctx *ctx) {
  const int N = ctx->params.fft_length;
  BlobView v = blob_view(ctx->blob.data());
  DevCoef dc;
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
  HIP_TRY(hipMemcpy(ctx->d_coef.get(), &dc, sizeof(dc), hipMemcpyHostToDevice));

  const int R = N / 512;  // 2048-sample segments per frame
  std::vector<float2> tab((size_t)kTabEntries512, make_float2(0.0f, 0.0f));
  const float invN = 1.0f / (float)N;  // exact power of two: folding it into the mask is lossless
  if (N == 512) {
    for (int r = 0; r < 8; ++r)
      for (int l = 0; l < 64; ++l) {
        const int k = l + 64 * r;
        tab[(size_t)(kTabMask + 64 * r + l)] = make_float2(v.mask[2 * k] * invN, v.mask[2 * k + 1] * invN);
      }
  } else {
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
  HIP_TRY(hipMemcpy(ctx->d_tab.get(), tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}

// InitializeDataArrays() + SpectralNoiseReductionInit() (T41_SDR.ino:479-504, 657): Xanr()'s and the spectral functions'
// memories at power-on
hipError_t nr_power_on(float *anr, float *spec, int nchan) {
  std::vector<float> ha((size_t)kAnrStRows * (size_t)nchan), hs((size_t)kNrSpecFloats * (size_t)nchan);
  nr_reset_anr(ha.data(), (size_t)nchan);
  for (int c = 0; c < nchan; ++c) nr_reset_record(hs.data() + (size_t)kNrSpecFloats * (size_t)c);
  const hipError_t e = hipMemcpy(anr, ha.data(), sizeof(float) * ha.size(), hipMemcpyHostToDevice);
  return e != hipSuccess ? e : hipMemcpy(spec, hs.data(), sizeof(float) * hs.size(), hipMemcpyHostToDevice);
}

// state and tables of the noise-reduction stages, on first use
int ensure_nr(t41rx_ctx *ctx) {
  if (ctx->d_nr_anr) return T41RX_OK;
  DevBuf<float> anr, spec, tab;
  if (dev_alloc(anr, sizeof(float) * kAnrStRows * (size_t)ctx->nchan) != hipSuccess ||
      dev_alloc(spec, sizeof(float) * kNrSpecFloats * (size_t)ctx->nchan) != hipSuccess ||
      dev_alloc(tab, sizeof(float) * kNrTabFloats) != hipSuccess)
    return fail(T41RX_ERR_NOMEM, "noise-reduction state allocation failed");
  float h[kNrTabFloats];
  nr_make_tables(h);
  if (hipMemcpy(tab.get(), h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess ||
      nr_power_on(anr.get(), spec.get(), ctx->nchan) != hipSuccess)
    return fail(T41RX_ERR_HIP, "noise-reduction state upload failed");
  ctx->d_nr_anr = std::move(anr);
  ctx->d_nr_spec = std::move(spec);
  ctx->d_nr_tab = std::move(tab);
  return T41RX_OK;
}

// a stage memory whose power-on value is zero, on first use
int ensure_zeroed(DevBuf<float> &b, size_t bytes, const char *what) {
  if (b) return T41RX_OK;
  DevBuf<float> z;
  if (dev_alloc(z, bytes) != hipSuccess) return fail(T41RX_ERR_NOMEM, std::string(what) + " state allocation failed");
  if (hipMemset(z.get(), 0, bytes) != hipSuccess) return fail(T41RX_ERR_HIP, std::string(what) + " state upload failed");
  b = std::move(z);
  return T41RX_OK;
}
// the noise blanker's carry, both slots (nb_sel stays 0 until the blanker first runs)
int ensure_nb(t41rx_ctx *ctx) {
  return ensure_zeroed(ctx->d_nb, sizeof(float) * 2 * kNbCarryPitch * (size_t)ctx->nchan, "noise-blanker");
}
// the receive equalizer's biquad memories (Filter.cpp:43-56)
int ensure_eq(t41rx_ctx *ctx) {
  return ensure_zeroed(ctx->d_eq, sizeof(float) * kEqStateFloats * (size_t)ctx->nchan, "receive-equalizer");
}

// the CW stages' memories: five filter states, the decode FIR's history, the detector's carried words (zeroed statics)
int ensure_cw(t41rx_ctx *ctx) {
  return ensure_zeroed(ctx->d_cw, sizeof(float) * kCwStateFloats * (size_t)ctx->nchan, "CW-receive");
}

// the decoder's words at power-on: what ResetHistograms() leaves, currentDashJump = 128, everything else zero
hipError_t cw_decode_upload_power_on(int32_t *d, int nchan) {
  std::vector<int32_t> h((size_t)kCwDecWords * (size_t)nchan);
  for (int c = 0; c < nchan; ++c) cw_decode_power_on(h.data() + (size_t)kCwDecWords * (size_t)c);
  return hipMemcpy(d, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice);
}
int ensure_cw_decode(t41rx_ctx *ctx) {
  if (ctx->d_cwdec) return T41RX_OK;
  DevBuf<int32_t> d;
  if (dev_alloc(d, sizeof(int32_t) * kCwDecWords * (size_t)ctx->nchan) != hipSuccess) return fail(T41RX_ERR_NOMEM, "CW-decoder state allocation failed");
  if (cw_decode_upload_power_on(d.get(), ctx->nchan) != hipSuccess) return fail(T41RX_ERR_HIP, "CW-decoder state upload failed");
  ctx->d_cwdec = std::move(d);
  return T41RX_OK;
}
// what cw_decode_kernel indexes, loops or branches with (cw_kernel.hip), per channel of a host section
int check_cw_decode(const t41rx_ctx *c, const int32_t *, const float *sec) {
  const int32_t *all = reinterpret_cast<const int32_t *>(sec);
  for (int ch = 0; ch < c->nchan; ++ch) {
    const int32_t *w = all + (size_t)kCwDecWords * (size_t)ch;
    const int st = w[kCwDecState];
    if (!(st == 0 || st == 1 || st == 2 || st == 5 || st == 6)) return fail(T41RX_ERR_STATE, "checkpoint: CW decoder state number out of range");
    if (w[kCwDecIndex] < 0 || w[kCwDecIndex] > 255) return fail(T41RX_ERR_STATE, "checkpoint: CW decoder currentDecoderIndex out of range");
    if (w[kCwDecDashJump] < 0 || w[kCwDecDashJump] > 128) return fail(T41RX_ERR_STATE, "checkpoint: CW decoder currentDashJump out of range");
    float tgm;
    std::memcpy(&tgm, &w[kCwDecTgm], sizeof(tgm));
    if (!std::isfinite(tgm) || !(tgm >= 1.0f && tgm < 750.0f))
      return fail(T41RX_ERR_STATE, "checkpoint: CW decoder thresholdGeometricMean not finite or out of range");
    // (the averages' product is formed in 32 bits; the value references enter the averages)
    for (int k : {kCwDecAveDit, kCwDecAveDah, kCwDecValRef1, kCwDecValRef2})
      if (w[k] < 0 || w[k] > 32767) return fail(T41RX_ERR_STATE, "checkpoint: CW decoder averages or value references out of range");
    for (int k : {kCwDecValFlag, kCwDecCharFlag, kCwDecBlankFlag})
      if (w[k] != 0 && w[k] != 1) return fail(T41RX_ERR_STATE, "checkpoint: CW decoder flag (valFlag, charProcessFlag, blankFlag) not 0 or 1");
    for (int k = kCwDecOffSig; k < kCwDecWords; ++k)  // seven of them are summed in 32 bits
      if (w[k] < 0 || w[k] > (1 << 27)) return fail(T41RX_ERR_STATE, "checkpoint: CW decoder histogram count out of range");
  }
  return T41RX_OK;
}

// the FT8 memory (power-on: every word zero -- syncFlag false, ft8_flag 0, an empty buffer) and arm_rfft_q15's tables
int ensure_ft8(t41rx_ctx *ctx) {
  if (ctx->d_ft8) return T41RX_OK;
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
  ctx->d_ft8 = std::move(st);
  ctx->d_ft8_tab = std::move(tab);
  return T41RX_OK;
}
int ft8_power_on(t41rx_ctx *ctx) {
  if (!ctx->d_ft8) return T41RX_OK;
  return hip_check(hipMemset(ctx->d_ft8.get(), 0, sizeof(int32_t) * kFt8Words * (size_t)ctx->nchan), "FT8 reset");
}
constexpr uint32_t kFt8Magic = 0x46313454u;  // "T41F"
constexpr size_t kFt8HeaderBytes = 32;
size_t ft8_record_bytes(const t41rx_ctx *ctx) { return kFt8HeaderBytes + sizeof(int32_t) * kFt8Words * (size_t)ctx->nchan; }

// a broken hand-over protocol of the pipelined kernels leaves wrong samples and a count of waits that ran out, not a hung
// GPU -- reported at the calls that synchronise anyway
int pipe_timeouts(const t41rx_ctx *ctx) {  // < 0: the counter could not be read
  if (!ctx->d_agc_pipe) return 0;
  unsigned n = 0;
  if (hipMemcpy(&n, ctx->d_agc_pipe.get() + pipe_layout(ctx->nchan).timeout, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return (int)n;
}
int pipe_timeouts_clear(t41rx_ctx *ctx) {
  if (!ctx->d_agc_pipe) return T41RX_OK;
  HIP_TRY(hipMemset(ctx->d_agc_pipe.get() + pipe_layout(ctx->nchan).timeout, 0, sizeof(unsigned long long)));
  return T41RX_OK;
}
// what the synchronising entry points answer when a wait inside the pipelined kernels has run out
int pipe_status(const t41rx_ctx *ctx) {
  const int n = pipe_timeouts(ctx);
  if (n < 0) return fail(T41RX_ERR_HIP, "could not read the pipelined kernels' time-out counter");
  if (n > 0)
    return fail(T41RX_ERR_STATE, "a wait inside the pipelined AGC / SAM kernel ran out: the samples since the last reset or restored checkpoint are not valid");
  return T41RX_OK;
}

// ---- checkpoint (t41rx_get_state / t41rx_set_state): header, the path's records, then the sections header word 5 names
constexpr uint32_t kStateMagic = 0x54343153u;  // "T41S"
constexpr size_t kStateHeaderBytes = 32;
constexpr int32_t kSecNr = 1, kSecDisp = 2, kSecNb = 4, kSecEq = 8, kSecCw = 16, kSecCwDec = 32;

// One checkpoint section: the memories of a stage built for fft_length 512 only.
struct Section {
  int32_t bit;                         // in header word 5
  const char *name;                    // (in the refusals)
  size_t chan_floats;                  // size per channel
  bool (*present)(const t41rx_ctx *);  // carried by this context's checkpoints
  int (*ensure)(t41rx_ctx *);          // allocation on restore, where the stage allocates lazily (or null)
  int (*check)(const t41rx_ctx *, const int32_t *hdr, const float *sec);  // refusal of a host section (or null)
  int (*get)(const t41rx_ctx *, void *host, size_t bytes);                // device -> host
  int (*put)(t41rx_ctx *, const void *host, size_t bytes);                // host -> device
  int (*reset)(t41rx_ctx *, size_t bytes);                                // power-on of what the context has allocated
};
// in bit order
const Section kSections[] = {
    // noise reduction / notch: Xanr()'s taps, delay line and leak words [kAnrStRows][n_channels], then the Kim / spectral
    // records [n_channels][kNrSpecFloats] (Noise.cpp:19-56) -- present once the stages have run
    {kSecNr, "noise-reduction", (size_t)kAnrStRows + (size_t)kNrSpecFloats,
     [](const t41rx_ctx *c) { return c->d_nr_anr != nullptr; }, ensure_nr,
     [](const t41rx_ctx *c, const int32_t *, const float *anr) {
       // what the kernels index with or divide by (nr_kernels.hip): Xanr()'s leak index, the spectral functions' ring pointers
       const float *spec = anr + (size_t)kAnrStRows * (size_t)c->nchan;
       for (int ch = 0; ch < c->nchan; ++ch) {
         const float lidx = anr[(size_t)kAnrStLidx * c->nchan + ch], ng = anr[(size_t)kAnrStNgamma * c->nchan + ch];
         if (!(lidx >= 0.0f && lidx <= 1000.0f) || !std::isfinite(ng)) return fail(T41RX_ERR_STATE, "checkpoint: notch leak words out of range");
         const float *sc = spec + (size_t)kNrSpecFloats * (size_t)ch + kNrScal;
         // (the kernel casts them with (int) and uses them as array indices and counters: integral values only)
         auto whole = [](float v) { return v == std::floor(v); };
         if (!(sc[0] >= 0.0f && sc[0] <= 2.0f) || !(sc[1] >= 0.0f && sc[1] <= 14.0f) || !(sc[2] == 0.0f || sc[2] == 1.0f || sc[2] == 2.0f) ||
             !(sc[3] >= 0.0f && sc[3] <= 1.0e6f) || !whole(sc[0]) || !whole(sc[1]) || !whole(sc[3]))
           return fail(T41RX_ERR_STATE, "checkpoint: noise-reduction ring pointers out of range or not integral");
       }
       return T41RX_OK;
     },
     [](const t41rx_ctx *c, void *h, size_t bytes) {
       const size_t ab = sizeof(float) * (size_t)kAnrStRows * (size_t)c->nchan;
       HIP_TRY(hipMemcpy(h, c->d_nr_anr.get(), ab, hipMemcpyDeviceToHost));
       HIP_TRY(hipMemcpy(static_cast<char *>(h) + ab, c->d_nr_spec.get(), bytes - ab, hipMemcpyDeviceToHost));
       return T41RX_OK;
     },
     [](t41rx_ctx *c, const void *h, size_t bytes) {
       const size_t ab = sizeof(float) * (size_t)kAnrStRows * (size_t)c->nchan;
       HIP_TRY(hipMemcpy(c->d_nr_anr.get(), h, ab, hipMemcpyHostToDevice));
       HIP_TRY(hipMemcpy(c->d_nr_spec.get(), static_cast<const char *>(h) + ab, bytes - ab, hipMemcpyHostToDevice));
       return T41RX_OK;
     },
     [](t41rx_ctx *c, size_t) {
       return c->d_nr_anr ? hip_check(nr_power_on(c->d_nr_anr.get(), c->d_nr_spec.get(), c->nchan), "noise-reduction reset") : T41RX_OK;
     }},
    // display FFT: zoom filters, ring, FFT_spec_old [n_channels][kDispFloats] (FFT.cpp:14-26) -- present while
    // t41rx_set_display_spectrum is on (which allocates it); header word 6 = its spectrumZoom
    {kSecDisp, "display-FFT", (size_t)kDispFloats,
     [](const t41rx_ctx *c) { return c->disp_spec && c->d_disp; }, nullptr,
     [](const t41rx_ctx *c, const int32_t *hdr, const float *d) {
       if (!(c->disp_spec && c->d_disp)) return fail(T41RX_ERR_STATE, "checkpoint carries display-FFT state but the display spectrum is off here");
       if (hdr[6] != c->disp_zoom) return fail(T41RX_ERR_STATE, "checkpoint: display-FFT state of another spectrumZoom");
       for (int ch = 0; ch < c->nchan; ++ch) {
         int32_t ptr;
         std::memcpy(&ptr, d + (size_t)kDispFloats * (size_t)ch + kDispPtr, sizeof(ptr));
         if (ptr < 0 || ptr >= 512) return fail(T41RX_ERR_STATE, "checkpoint: zoom_sample_ptr out of range");
       }
       return T41RX_OK;
     },
     [](const t41rx_ctx *c, void *h, size_t n) { return hip_check(hipMemcpy(h, c->d_disp.get(), n, hipMemcpyDeviceToHost), "hipMemcpy"); },
     [](t41rx_ctx *c, const void *h, size_t n) { return hip_check(hipMemcpy(c->d_disp.get(), h, n, hipMemcpyHostToDevice), "hipMemcpy"); },
     [](t41rx_ctx *c, size_t n) { return c->d_disp ? hip_check(hipMemset(c->d_disp.get(), 0, n), "hipMemset") : T41RX_OK; }},  // ZoomFFTPrep()
    // noise blanker: last_frame_end[0 .. 12] (DSP_Fn.cpp:143), [n_channels][kNbCarryPitch] (3 floats of padding) -- the
    // current one of the two slots out, slot 0 in; present once the blanker has run
    {kSecNb, "noise-blanker", (size_t)kNbCarryPitch,
     [](const t41rx_ctx *c) { return c->d_nb != nullptr; }, ensure_nb, nullptr,
     [](const t41rx_ctx *c, void *h, size_t n) {
       return hip_check(hipMemcpy(h, c->d_nb.get() + (size_t)c->nb_sel * (n / sizeof(float)), n, hipMemcpyDeviceToHost), "hipMemcpy");
     },
     [](t41rx_ctx *c, const void *h, size_t n) {
       c->nb_sel = 0;
       return hip_check(hipMemcpy(c->d_nb.get(), h, n, hipMemcpyHostToDevice), "hipMemcpy");
     },
     [](t41rx_ctx *c, size_t n) {  // both slots: last_frame_end is a static, zero at power-on
       c->nb_sel = 0;
       return c->d_nb ? hip_check(hipMemset(c->d_nb.get(), 0, 2 * n), "hipMemset") : T41RX_OK;
     }},
    // receive equalizer: rec_EQ_Band1_state .. rec_EQ_Band14_state (Filter.cpp:43-56), [n_channels][kEqStateFloats] --
    // present once the equalizer has run
    {kSecEq, "receive-equalizer", (size_t)kEqStateFloats,
     [](const t41rx_ctx *c) { return c->d_eq != nullptr; }, ensure_eq, nullptr,
     [](const t41rx_ctx *c, void *h, size_t n) { return hip_check(hipMemcpy(h, c->d_eq.get(), n, hipMemcpyDeviceToHost), "hipMemcpy"); },
     [](t41rx_ctx *c, const void *h, size_t n) { return hip_check(hipMemcpy(c->d_eq.get(), h, n, hipMemcpyHostToDevice), "hipMemcpy"); },
     [](t41rx_ctx *c, size_t n) { return c->d_eq ? hip_check(hipMemset(c->d_eq.get(), 0, n), "hipMemset") : T41RX_OK; }},  // (zeroed statics)
    // CW receive: CW_AudioFilter1_state .. CW_AudioFilter5_state (CWProcessing.cpp:37-41), the decode FIR's history
    // (FIR_CW_DecodeL_state, T41_SDR.ino:281), corrResultR, aveCorrResultL / R, [n_channels][kCwStateFloats] -- present
    // once a CW stage has run
    {kSecCw, "CW-receive", (size_t)kCwStateFloats,
     [](const t41rx_ctx *c) { return c->d_cw != nullptr; }, ensure_cw, nullptr,
     [](const t41rx_ctx *c, void *h, size_t n) { return hip_check(hipMemcpy(h, c->d_cw.get(), n, hipMemcpyDeviceToHost), "hipMemcpy"); },
     [](t41rx_ctx *c, const void *h, size_t n) { return hip_check(hipMemcpy(c->d_cw.get(), h, n, hipMemcpyHostToDevice), "hipMemcpy"); },
     [](t41rx_ctx *c, size_t n) { return c->d_cw ? hip_check(hipMemset(c->d_cw.get(), 0, n), "hipMemset") : T41RX_OK; }},  // (zeroed statics)
    // CW decoder: DoCWDecoding()'s statics and the globals it shares with its histograms (CWProcessing.cpp:26-99,
    // :538-550), then signalHistogram, then gapHistogram, [n_channels][kCwDecWords] int32 words (cw_kernels.hpp names
    // them) -- present once the decoder has run
    {kSecCwDec, "CW-decoder", (size_t)kCwDecWords,
     [](const t41rx_ctx *c) { return c->d_cwdec != nullptr; }, ensure_cw_decode, check_cw_decode,
     [](const t41rx_ctx *c, void *h, size_t n) { return hip_check(hipMemcpy(h, c->d_cwdec.get(), n, hipMemcpyDeviceToHost), "hipMemcpy"); },
     [](t41rx_ctx *c, const void *h, size_t n) { return hip_check(hipMemcpy(c->d_cwdec.get(), h, n, hipMemcpyHostToDevice), "hipMemcpy"); },
     [](t41rx_ctx *c, size_t) {
       return c->d_cwdec ? hip_check(cw_decode_upload_power_on(c->d_cwdec.get(), c->nchan), "CW-decoder reset") : T41RX_OK;
     }},
};

size_t section_bytes(const Section &s, int nchan) { return sizeof(float) * s.chan_floats * (size_t)nchan; }
size_t path_bytes(const t41rx_ctx *ctx) { return sizeof(float) * state_floats(ctx->params.fft_length) * (size_t)ctx->nchan; }
int32_t state_sections(const t41rx_ctx *ctx) {
  int32_t sec = 0;
  for (const Section &s : kSections)
    if (s.present(ctx)) sec |= s.bit;
  return sec;
}
size_t state_bytes(const t41rx_ctx *ctx, int32_t sec) {
  size_t n = kStateHeaderBytes + path_bytes(ctx);
  for (const Section &s : kSections)
    if (sec & s.bit) n += section_bytes(s, ctx->nchan);
  return n;
}

// what the kernels consume of the path's records as they stand: the oscillator amplitude and the AGC state words
int check_records(const t41rx_ctx *ctx, const float *rec) {
  const size_t sf = state_floats(ctx->params.fft_length);
  const size_t ag = st_agc(ctx->params.fft_length) + kAgcHistFloats;
  for (int c = 0; c < ctx->nchan; ++c) {
    const float *r = rec + sf * (size_t)c;
    NcoState ns;
    std::memcpy(&ns, r + kStNco, sizeof(ns));
    if (!(ns.r > 0.25 && ns.r < 4.0)) return fail(T41RX_ERR_STATE, "checkpoint: oscillator amplitude out of range");
    int32_t w[3];
    std::memcpy(w, r + ag + kAgcStState, sizeof(w));
    if (w[0] < 0 || w[0] > 4 || w[1] < 0 || w[1] > 1 || w[2] < 0 || w[2] > (1 << 20))
      return fail(T41RX_ERR_STATE, "checkpoint: AGC state words out of range");
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(r[ag + k])) return fail(T41RX_ERR_STATE, "checkpoint: AGC levels not finite");
    // AMDecodeSAM's statics (Demod.cpp:19-23): the kernel wraps phzerror with one conditional step
    // each way, which is the reference's pair of `while` loops only for a phase already in [0, 2 pi] (2 pi itself is
    // what a tiny negative phase + 2 pi rounds to: the loops leave it, and so does the kernel)
    const float phz = r[kStMisc + kMiscSamPhz], fil = r[kStMisc + kMiscSamFil], om = r[kStMisc + kMiscSamOmega];
    if (!(phz >= 0.0f && phz <= 6.2831855f) || !std::isfinite(fil) || !(std::fabs(fil) < 4.0f) || !(std::fabs(om) <= 1.05f))
      return fail(T41RX_ERR_STATE, "checkpoint: synchronous-detector PLL words out of range");
  }
  return T41RX_OK;
}

int reset_state(t41rx_ctx *ctx) {
  const size_t sf = state_floats(ctx->params.fft_length);
  std::vector<float> h(sf * (size_t)ctx->nchan, 0.0f);
  for (int c = 0; c < ctx->nchan; ++c) {
    NcoState ns;
    ns.phase = 0;  // Osc_Vect_Q = 1, Osc_Vect_I = 0 (Freq_Shift.cpp:13-14)
    ns.r = 1.0;
    std::memcpy(h.data() + sf * (size_t)c + kStNco, &ns, sizeof(ns));
    std::memcpy(h.data() + sf * (size_t)c + kStNco + 4, &ns, sizeof(ns));
  }
  HIP_TRY(hipMemcpy(ctx->d_state.get(), h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
  ctx->nco_sel = 0;
  for (const Section &s : kSections) {
    const int rc = s.reset(ctx, section_bytes(s, ctx->nchan));
    if (rc != T41RX_OK) return rc;
  }
  return ft8_power_on(ctx);
}

// ---- a process call: (a) prepare_call, (b) rx_args, (c) launch_chain
bool nr_on(const t41rx_ctx *ctx) { return ctx->params.nrOptionSelect != 0 || ctx->params.ANR_notchOn != 0; }  // (fft_length 512: params_valid)
// the CW block runs in T41State == CW_RECEIVE (Process.cpp:878), which in receive is xmtMode == CW_MODE
// (T41_SDR.ino:1039-1040, 1144-1148); with another xmtMode the switches are kept and nothing runs
bool cw_filter_on(const t41rx_ctx *ctx) { return ctx->params.xmtMode == T41RX_CW_MODE && ctx->cw_filter != kCwFilters; }
bool cw_det_on(const t41rx_ctx *ctx) { return ctx->params.xmtMode == T41RX_CW_MODE && ctx->cw_det != 0; }
// the decoder runs exactly when the detector runs (in the firmware one decoderFlag gates both, CWProcessing.cpp:322-372)
bool cw_dec_on(const t41rx_ctx *ctx) { return cw_det_on(ctx) && ctx->cw_dec != 0; }
// the fused kernel stops behind the demodulator; stage kernels; back kernel (fft_length 512: t41rx_set_noise_blanker,
// t41rx_set_receive_eq, t41rx_set_cw_filter, t41rx_set_cw_detector)
bool stages_on(const t41rx_ctx *ctx) { return ctx->eq_on || nr_on(ctx) || ctx->nb_on || cw_filter_on(ctx) || cw_det_on(ctx); }
// The library carries one audio stream where the firmware has float_buffer_L and float_buffer_R; the detector reads both.
// The stage that leaves L different from R in front of it, or null: the equalizer writes L only (Filter.cpp:151-164),
// Kim1_NR() and SpectralNoiseReduction() end with R = L (Noise.cpp:307-308, 636-637) but x30 behind Kim scales L only
// (Process.cpp:846), Xanr() writes R only and x1.5 behind it scales L only (Noise.cpp:345-347, Process.cpp:855); the
// notch and the blanker end in arm_copy_f32(R, L) (Process.cpp:865, 875), which joins them again.
const char *cw_split_stage(const t41rx_ctx *ctx) {
  if (ctx->params.ANR_notchOn != 0 || ctx->nb_on) return nullptr;
  if (ctx->params.nrOptionSelect == 1) return "Kim noise reduction (nrOptionSelect 1)";
  if (ctx->params.nrOptionSelect == 3) return "LMS noise reduction (nrOptionSelect 3)";
  if (ctx->eq_on && ctx->params.nrOptionSelect == 0) return "receive equalizer";
  return nullptr;
}
// the pipelined kernels' buffer: AGC on (with the synchronous detector behind it: PSA), or the synchronous detector alone
bool pipe_on(const t41rx_ctx *ctx, int n_frames) {
  return (ctx->params.AGCMode != 0 || ctx->params.mode == T41RX_DEMOD_SAM) && ctx->params.fft_length == 512 && n_frames >= 4;
}

// (a) what the call needs allocated (stages and scratch on first use, kept) and the refusals that depend on the context
int prepare_call(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  const int seg = ctx->params.fft_length / 512;
  int rc = T41RX_OK;
  // the panadapter stage: which frames of this call are update frames, in front of everything that allocates
  ctx->pan_call_rows = 0;
  ctx->pan_call_first = n_frames;
  if (ctx->pan_on) {
    ctx->pan_call_rows = pan_rows_of_call(ctx->pan_counter, n_frames, ctx->pan_period, ctx->pan_phase, &ctx->pan_call_first);
    if (ctx->pan_call_rows > ctx->pan_max_rows)
      return fail(T41RX_ERR_ARG, "the call holds more update frames than the max_rows the panadapter buffers were set with");
    if (!ctx->d_pan_pre || !ctx->d_pan_max || !ctx->d_pan_mem || !ctx->d_pan_nf || !ctx->d_pan_gc || !ctx->d_pan_grad || !ctx->d_win)
      return fail(T41RX_ERR_STATE, "panadapter enabled without its buffers");
  }
  if ((nr_on(ctx) && (rc = ensure_nr(ctx)) != T41RX_OK) || (ctx->nb_on && (rc = ensure_nb(ctx)) != T41RX_OK) ||
      (ctx->eq_on && (rc = ensure_eq(ctx)) != T41RX_OK) ||
      ((cw_filter_on(ctx) || cw_det_on(ctx)) && (rc = ensure_cw(ctx)) != T41RX_OK))
    return rc;
  if ((seg > 1 || stages_on(ctx)) && n_frames > ctx->scratch_frames) {
    // scratch between the kernels of the long-FFT pipeline / the noise-reduction pipeline (grown on demand, kept)
    HIP_TRY(hipStreamSynchronize(s));
    ctx->scratch_frames = 0;
    ctx->d_mid.reset();
    ctx->d_aud24.reset();
    const size_t per = (size_t)ctx->nchan * (size_t)n_frames * (size_t)(256 * seg);  // fft_length / 2 per frame
    HIP_TRY(dev_alloc(ctx->d_mid, per * 2 * sizeof(float)));
    HIP_TRY(dev_alloc(ctx->d_aud24, per * 2 * sizeof(float)));  // complex when the back kernel demodulates
    ctx->scratch_frames = n_frames;
  }
  if (ctx->params.mode == T41RX_DEMOD_NFM && ctx->params.nfm_demod == 1 && seg > 1)
    return fail(T41RX_ERR_UNSUPPORTED, "nfm_demod = 1 is built for fft_length 512");
  if (pipe_on(ctx, n_frames) && !ctx->d_agc_pipe) {
    const size_t bytes = pipe_layout(ctx->nchan).bytes;
    DevBuf<char> pipe;  // the context only ever sees a buffer whose counters are zero
    HIP_TRY(dev_alloc(pipe, bytes));
    HIP_TRY(hipMemset(pipe.get(), 0, bytes));
    ctx->d_agc_pipe = std::move(pipe);
  }
  if (ctx->params.AGCMode != 0 && (int)blob_view(ctx->blob.data()).agc[kAgcAttackBuffsize] != kAgcDelay)
    return fail(T41RX_ERR_STATE, "coefficient blob carries an AGC look-ahead the kernel is not built for");
  if ((ctx->dbg_nco || ctx->dbg_dec || ctx->dbg_demod) && n_frames > ctx->tap_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the debug tap buffers were set with");
  if (ctx->spect && n_frames > ctx->spect_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the audio-spectrum buffers were set with");
  if (ctx->disp_spec && n_frames > ctx->disp_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the display-spectrum buffers were set with");
  if (cw_dec_on(ctx) && n_frames > ctx->cw_text_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the CW decoder's buffer was set with");
  if (cw_det_on(ctx) && n_frames > ctx->cw_frames)
    return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the CW detector's buffer was set with");
  if (cw_det_on(ctx))
    if (const char *stage = cw_split_stage(ctx))
      return fail(T41RX_ERR_UNSUPPORTED, std::string("CW detector: the ") + stage +
                                             " leaves float_buffer_L different from float_buffer_R and neither the notch nor the noise "
                                             "blanker joins them behind it; the library carries one audio stream");
  if (ctx->disp_spec && (!ctx->d_pre || !ctx->d_disp || !ctx->d_win)) return fail(T41RX_ERR_STATE, "display spectrum enabled without its buffers");
  if (ctx->ft8_on) {
    if (ctx->params.mode != T41RX_DEMOD_USB)
      return fail(T41RX_ERR_UNSUPPORTED, "FT8 receive: the firmware demodulates DEMOD_FT8 as USB (Process.cpp:616-617); this context's mode is not T41RX_DEMOD_USB");
    if (n_frames > ctx->ft8_frames) return fail(T41RX_ERR_ARG, "n_frames exceeds the max_frames the FT8 status buffer was set with");
    if ((rc = ensure_ft8(ctx)) != T41RX_OK) return rc;
    if (!stages_on(ctx) && !ctx->dbg_demod && n_frames > ctx->ft8_tap_frames) {
      // the demod tap of the context's own (grown on demand, kept)
      HIP_TRY(hipStreamSynchronize(s));
      ctx->ft8_tap_frames = 0;
      ctx->d_ft8_tap.reset();
      HIP_TRY(dev_alloc(ctx->d_ft8_tap, sizeof(float) * 256 * (size_t)n_frames * (size_t)ctx->nchan));
      ctx->ft8_tap_frames = n_frames;
    }
  }
  // the decoder's words, behind every refusal: its checkpoint section appears with the first call in which it runs
  if (cw_dec_on(ctx) && (rc = ensure_cw_decode(ctx)) != T41RX_OK) return rc;
  return T41RX_OK;
}

// (b) the kernels' arguments
RxArgs rx_args(t41rx_ctx *ctx, const float *dI, const float *dQ, float *dAudio, int n_frames, bool q15) {
  const int seg = ctx->params.fft_length / 512;
  RxArgs a{};
  a.I = dI;
  a.Q = dQ;
  a.out = dAudio;
  a.state = ctx->d_state.get();
  a.coef = ctx->d_coef.get();
  a.tab = ctx->d_tab.get();
  a.nco = ctx->d_nco.get();
  a.nchan = ctx->nchan;
  a.nframes = seg * n_frames;  // 2048-sample segments
  if (ctx->layout == T41RX_LAYOUT_TIME_MAJOR) {  // [frame][channel][frame_len] (fft_length 512: set_buffer_layout / set_params)
    a.chan_stride = 2048;
    a.frame_stride = (long long)ctx->nchan * 2048;
  } else {
    a.chan_stride = (long long)a.nframes * 2048;
    a.frame_stride = 2048;
  }
  if (ctx->n_streams > 0) {  // receiver groups: I / Q hold n_streams rows in the same layout, the output nchan as above
    a.in_map = ctx->d_in_map.get();
    a.in_chan_stride = a.chan_stride;
    a.in_frame_stride = ctx->layout == T41RX_LAYOUT_TIME_MAJOR ? (long long)ctx->n_streams * 2048 : a.frame_stride;
  }
  a.seg = seg;
  a.nframes4k = n_frames;
  a.mid = ctx->d_mid.get();
  a.aud24 = ctx->d_aud24.get();
  a.tab4k = ctx->d_tab4k.get();
  {
    const float *sc = blob_view(ctx->blob.data()).scalars;
    const bool iq_on = sc[kScIqCorrOn] != 0.0f;
    const float gi = iq_on ? sc[kScBandGain] * sc[kScNegIqAmp] : sc[kScBandGain];
    a.g_rf = sc[kScRfGain];
    a.g_band = sc[kScBandGain];
    a.neg_iq_amp = sc[kScNegIqAmp];
    a.iq_phase = sc[kScIqPhase];
    a.iq_corr_on = iq_on ? 1 : 0;
    // PLAIN folds "I <- -I" (IQ correction on, amplitude factor 1) into the sign of the RF gain; with
    // the correction on and gi = +1 (IQAmpCorrectionFactor = -1) the general kernel must run
    a.plain = ((iq_on ? gi == -1.0f : gi == 1.0f) && sc[kScBandGain] == 1.0f && (!iq_on || sc[kScIqPhase] == 0.0f)) ? 1 : 0;
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
    if (const char *e = std::getenv("T41RX_SEG_RUN")) run = std::atol(e);  // experiments
    a.seg_run = (int)(run < 1 ? 1 : (run > 8 ? 8 : (run > segs ? segs : run)));
  }
  a.agc = ctx->params.AGCMode != 0 ? 1 : 0;
  if (pipe_on(ctx, n_frames)) a.agc_pipe = reinterpret_cast<float *>(ctx->d_agc_pipe.get());
  a.dbg_pre = ctx->disp_spec ? ctx->d_pre.get() : nullptr;
  a.dbg_nco = ctx->dbg_nco;
  a.dbg_dec = ctx->dbg_dec;
  a.dbg_demod = ctx->dbg_demod;
  if (ctx->ft8_on && !stages_on(ctx) && !a.dbg_demod) a.dbg_demod = ctx->d_ft8_tap.get();  // the FT8 stage reads the demod tap
  a.spect = ctx->spect;
  a.spect_max = ctx->spect_max;
  if (ctx->pan_on && ctx->pan_call_rows > 0) {
    // the panadapter owns the display taps (one owner each: the setters refuse the other): compact rows for the call's
    // update frames.  A call without one sets no tap and so launches what a context without the stage launches.
    a.dbg_pre = ctx->d_pan_pre.get();
    a.spect = ctx->pan_out.audio_spect;
    a.spect_max = ctx->d_pan_max.get();
    a.tap_period = ctx->pan_period;
    a.tap_first = ctx->pan_call_first;
    a.tap_rows = ctx->pan_max_rows;
  }
  if (stages_on(ctx)) a.aud_out = ctx->d_aud24.get();  // the fused kernel stops behind the demodulator
  return a;
}

// (c) the stage chain: fused front end, then on the audio @24 kS/s the equalizer, noise reduction / notch and the
// blanker, the CW detector and narrow filter, the back end, and the display FFT
int launch_chain(t41rx_ctx *ctx, RxArgs a, int n_frames, hipStream_t s) {
  hipError_t e = launch_rx(a, ctx->params.fft_length, ctx->params.mode, s);
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  if (ctx->ft8_on) {
    // Process.cpp:627-685 on float_buffer_L as the demodulator and the AGC leave it, in front of the equalizer: the
    // hand-over buffer when other stages split the chain, else the demod tap.  The stage only reads the audio.
    Ft8Args f{};
    f.aud = a.aud_out ? a.aud_out : a.dbg_demod;
    f.state = ctx->d_ft8.get();
    f.power = ctx->ft8_power;
    f.status = ctx->ft8_status;
    f.window = ctx->d_ft8_win.get();
    f.mag_db = ctx->d_ft8_mag.get();
    f.tab = ctx->d_ft8_tab.get();
    f.nchan = ctx->nchan;
    f.nframes = n_frames;
    f.t0 = ctx->ft8_t0;
    f.num = ctx->ft8_num;
    f.den = ctx->ft8_den;
    f.threads = 256;
    if (const char *env = std::getenv("T41RX_FT8_THREADS")) f.threads = std::atoi(env) == 64 ? 64 : 256;  // experiments (tools/ft8_probe.py)
    e = launch_ft8(f, s);
    if (e != hipSuccess) return hip_fail(e, "FT8 kernel launch");
  }
  if (ctx->eq_on) {
    // Process.cpp:828-832 on the call's audio @24 kS/s
    EqArgs q{};
    q.aud = ctx->d_aud24.get();
    q.state = ctx->d_eq.get();
    q.nchan = ctx->nchan;
    q.nsamp = n_frames * 256;
    std::memcpy(q.coef, ctx->eq_coef, sizeof(q.coef));
    for (int b = 0; b < kEqBands; ++b) {
      // recEQ_LevelScale[b] = (float)EEPROMData.equalizerRec[b] / 100.0 (Filter.cpp:119-121); arm_scale_f32 by its
      // negative for bands 1, 3, .., 13 (Filter.cpp:138-151)
      const float lvl = (float)((double)(float)ctx->eq_levels[b] / 100.0);
      q.scale[b] = (b % 2 == 0) ? -lvl : lvl;
    }
    e = launch_eq(q, s);
    if (e != hipSuccess) return hip_fail(e, "receive-equalizer kernel launch");
  }
  if (nr_on(ctx)) {
    // Process.cpp:841-866 behind it
    NrArgs n{};
    n.aud = ctx->d_aud24.get();
    n.anr = ctx->d_nr_anr.get();
    n.spec = ctx->d_nr_spec.get();
    n.tab_nr = ctx->d_nr_tab.get();
    n.tab = ctx->d_tab.get();
    n.nchan = ctx->nchan;
    n.nframes = n_frames;
    n.nr_option = ctx->params.nrOptionSelect;
    n.notch = ctx->params.ANR_notchOn;
    n.alpha = ctx->params.NR_alpha;
    n.beta = ctx->params.NR_beta;
    n.psi = ctx->params.NR_PSI;
    nr_vad_range(ctx->params.FLoCut, ctx->params.FHiCut, &n.vad_lo, &n.vad_hi);
    e = launch_nr(n, s);
    if (e != hipSuccess) return hip_fail(e, "noise-reduction kernel launch");
  }
  if (ctx->nb_on) {
    // Process.cpp:873-876 behind them
    NbArgs b{};
    b.aud = ctx->d_aud24.get();
    b.carry = ctx->d_nb.get();
    b.nchan = ctx->nchan;
    b.nframes = n_frames;
    b.sel = ctx->nb_sel;
    e = launch_nb(b, s);
    if (e != hipSuccess) return hip_fail(e, "noise-blanker kernel launch");
    ctx->nb_sel ^= 1;  // the last frame wrote the other slot
  }
  if (cw_det_on(ctx)) {
    // Process.cpp:878-879 behind it: DoCWReceiveProcessing() reads the audio, its results go to the caller's buffer
    CwDetectArgs d{};
    d.aud = ctx->d_aud24.get();
    d.state = ctx->d_cw.get();
    d.out = ctx->cw_out;
    d.nchan = ctx->nchan;
    d.nframes = n_frames;
    {
      // goertzel_mag(256, 750, 24000, .) (CWProcessing.cpp:835-842) in its types: k = (int)(0.5 + 256.0f * 750 / 24000) = 8
      const float fn = (float)kCwBlock;
      const int k = (int)(0.5 + (double)((fn * 750) / 24000));
      const float omega = (float)((2.0 * 3.14159265358979323846 * k) / (double)fn);
      d.sine = (float)std::sin((double)omega);
      d.cosine = (float)std::cos((double)omega);
      d.coeff = (float)(2.0 * (double)d.cosine);
      // sineTone() (Utility.cpp:72-74): float theta = kf * 0.19634950849362; sinBuffer[kf] = sin(theta)
      for (int kf = 0; kf < kCwBlock; ++kf) {
        const float theta = (float)(kf * 0.19634950849362);
        d.sinb[kf] = (float)std::sin((double)theta);
      }
    }
    std::memcpy(d.fir, ctx->cw_fir, sizeof(d.fir));
    e = launch_cw_detect(d, s);
    if (e != hipSuccess) return hip_fail(e, "CW detector kernel launch");
  }
  if (cw_dec_on(ctx)) {
    // CWProcessing.cpp:365-371 behind it: the threshold on the detector's combinedCoeff and DoCWDecoding()
    CwDecodeArgs d{};
    d.cw = ctx->cw_out;
    d.state = ctx->d_cwdec.get();
    d.text = ctx->cw_text;
    d.nchan = ctx->nchan;
    d.nframes = n_frames;
    d.t0 = ctx->cw_t0;
    d.num = ctx->cw_num;
    d.den = ctx->cw_den;
    std::memcpy(d.tree, ctx->cw_tree, sizeof(d.tree));
    e = launch_cw_decode(d, s);
    if (e != hipSuccess) return hip_fail(e, "CW decoder kernel launch");
  }
  if (cw_filter_on(ctx)) {
    // Process.cpp:882-912: the narrow filter CWFilterIndex selects, on its own memory
    CwFilterArgs f{};
    f.aud = ctx->d_aud24.get();
    f.state = ctx->d_cw.get();
    f.nchan = ctx->nchan;
    f.nsamp = n_frames * 256;
    f.index = ctx->cw_filter;
    std::memcpy(f.coef, ctx->cw_coef + kCwFilterCoefs * ctx->cw_filter, sizeof(f.coef));
    e = launch_cw_filter(f, s);
    if (e != hipSuccess) return hip_fail(e, "CW filter kernel launch");
  }
  if (cw_filter_on(ctx)) {
    // then the interpolators, volume and stores (Process.cpp:917-937) in the firmware's own operations and order
    // (cw_back_kernel): the narrow filter's audio is held to the oracle's interpolators bit for bit
    const BlobView v = blob_view(ctx->blob.data());
    CwBackArgs b{};
    b.aud = ctx->d_aud24.get();
    b.state = ctx->d_state.get();
    b.out = a.out;
    b.nchan = ctx->nchan;
    b.nframes = n_frames;
    b.chan_stride = a.chan_stride;
    b.frame_stride = a.frame_stride;
    b.state_stride = (long long)state_floats(512);
    b.q15 = a.q15;
    b.scale = v.scalars[kScOutScale];
    std::memcpy(b.int1, v.int1, sizeof(b.int1));
    std::memcpy(b.int2, v.int2, sizeof(b.int2));
    e = launch_cw_back(b, s);
    if (e != hipSuccess) return hip_fail(e, "CW interpolator kernel launch");
  } else if (stages_on(ctx)) {
    // then the interpolators, volume and stores (Process.cpp:917-937) from a.aud24
    a.aud_out = nullptr;
    e = launch_back512(a, s);
    if (e != hipSuccess) return hip_fail(e, "interpolator kernel launch");
  }
  if (a.seg > 1) ctx->nco_sel ^= 1;  // the kernels wrote the other copy
  if (ctx->disp_spec) {
    DispArgs d{};
    d.pre = ctx->d_pre.get();
    d.disp = ctx->d_disp.get();
    d.spec = ctx->disp_spec;
    d.spec_old = ctx->disp_old;
    d.tab = ctx->d_tab.get();
    d.win = ctx->d_win.get();
    d.nchan = ctx->nchan;
    d.nframes = n_frames;
    d.zoom = ctx->disp_zoom;
    if (d.zoom > 0) {
      std::memcpy(d.iir, kZoomIirCoeffs[d.zoom - 1], sizeof(d.iir));
      design_zoom_fir(d.zoom, d.fir);
    }
    e = launch_display(d, s);
    if (e != hipSuccess) return hip_fail(e, "display kernel launch");
  }
  if (ctx->pan_on) {
    if (ctx->pan_call_rows > 0) {
      PanArgs p{};
      p.pre = ctx->d_pan_pre.get();
      p.mx = ctx->d_pan_max.get();
      p.mem = ctx->d_pan_mem.get();
      p.tab = ctx->d_tab.get();
      p.win = ctx->d_win.get();
      p.gradient = ctx->d_pan_grad.get();
      p.noise_floor = ctx->d_pan_nf.get();
      p.gain_correction = ctx->d_pan_gc.get();
      p.pixel = ctx->pan_out.pixel;
      p.y_new = ctx->pan_out.y_new;
      p.y_old = ctx->pan_out.y_old;
      p.waterfall = ctx->pan_out.waterfall;
      p.spec = ctx->pan_out.spec;
      p.smeter = ctx->pan_out.smeter;
      p.nchan = ctx->nchan;
      p.nrows = ctx->pan_call_rows;
      p.max_rows = ctx->pan_max_rows;
      p.zoom = ctx->pan_zoom;
      if (p.zoom > 0) {
        std::memcpy(p.iir, kZoomIirCoeffs[p.zoom - 1], sizeof(p.iir));
        design_zoom_fir(p.zoom, p.fir);
      }
      p.dBScale = kDbScale[ctx->pan_scale];
      p.base = kBaseOffset[ctx->pan_scale] + ctx->pan_pixel_offset;
      p.noise_floor_y = ctx->pan_floor_y;
      p.attenuator = ctx->pan_attenuator;
      p.RFgain = ctx->params.RFgain;
      p.rfGainAllBands = ctx->params.rfGainAllBands;
      e = launch_panadapter(p, s);
      if (e != hipSuccess) return hip_fail(e, "panadapter kernel launch");
    }
    ctx->pan_last_rows = ctx->pan_call_rows;
    ctx->pan_last_first = ctx->pan_call_rows > 0 ? ctx->pan_counter + ctx->pan_call_first : -1;
    ctx->pan_counter += n_frames;
  }
  return T41RX_OK;
}

int process_device_impl(t41rx_ctx *ctx, const float *dI, const float *dQ, float *dAudio, int n_frames,
                        void *hip_stream, bool q15) {
  if (!ctx || !dI || !dQ || !dAudio) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  if ((reinterpret_cast<uintptr_t>(dI) | reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dAudio)) & 15u)
    return fail(T41RX_ERR_ARG, "I/Q/audio device pointers must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const hipStream_t s = (hipStream_t)hip_stream;
  const int rc = prepare_call(ctx, n_frames, s);
  if (rc != T41RX_OK) return rc;
  return launch_chain(ctx, rx_args(ctx, dI, dQ, dAudio, n_frames, q15), n_frames, s);
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

// the per-channel levels, on the device; values == nullptr: zeros
template <class T>
int pan_upload_levels(t41rx_ctx *ctx, DevBuf<T> &d, const T *values) {
  std::vector<T> h((size_t)ctx->nchan, T(0));
  if (values) std::memcpy(h.data(), values, sizeof(T) * h.size());
  if (!d) HIP_TRY(dev_alloc(d, sizeof(T) * h.size()));
  HIP_TRY(hipMemcpy(d.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}

// IQ calibration: what every t41rx_calibrate_* entry checks, then the launch.  I / Q are float_buffer_L's and
// float_buffer_R's sources (the q15 entries have swapped the queues already)
int calibrate_impl(t41rx_ctx *ctx, const void *dI, const void *dQ, int shared_input, const uint8_t *d_update, float *d_result,
                   int16_t *d_pixel, float *d_spec, int n_frames, void *hip_stream, bool q15) {
  if (!ctx || !dI || !dQ || !d_result) return fail(T41RX_ERR_ARG, "null argument");
  if (!ctx->cal_on) return fail(T41RX_ERR_ARG, "calibration is not switched on (t41rx_set_calibration)");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the calibration is built for fft_length 512");
  if (ctx->layout != T41RX_LAYOUT_CHANNEL_MAJOR) return fail(T41RX_ERR_UNSUPPORTED, "the calibration is built for the channel-major layout");
  if (((reinterpret_cast<uintptr_t>(dI) | reinterpret_cast<uintptr_t>(dQ)) & (q15 ? 1u : 3u)) ||
      ((reinterpret_cast<uintptr_t>(d_result) | reinterpret_cast<uintptr_t>(d_spec)) & 3u) || (reinterpret_cast<uintptr_t>(d_pixel) & 1u))
    return fail(T41RX_ERR_ARG, "unaligned pointer");
  if (!ctx->d_cal || !ctx->d_win) return fail(T41RX_ERR_STATE, "calibration enabled without its buffers");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  CalArgs a{};
  a.I = dI;
  a.Q = dQ;
  a.update = d_update;
  a.result = d_result;
  a.pixel = d_pixel;
  a.spec = d_spec;
  a.cal = ctx->d_cal.get();
  a.tab = ctx->d_tab.get();
  a.win = ctx->d_win.get();
  a.corr = ctx->cal_per_channel ? ctx->d_cal_corr.get() : nullptr;
  a.zoom = ctx->cal_zoom;
  if (a.zoom > 0) {
    std::memcpy(a.iir, kZoomIirCoeffs[a.zoom - 1], sizeof(a.iir));
    design_zoom_fir(a.zoom, a.fir);
  }
  a.chan_stride = shared_input ? 0 : (long long)n_frames * 2048;
  a.nchan = ctx->nchan;
  a.nframes = n_frames;
  a.q15 = q15 ? 1 : 0;
  a.g_rf = blob_view(ctx->blob.data()).scalars[kScRfGain];  // the same expression, Process.cpp:117 / Process2.cpp:365
  a.rec_band = 1.0f;                                        // recBandFactor[], Process2.cpp:299
  a.iq_amp = ctx->params.IQAmpCorrectionFactor;
  a.iq_phase = ctx->params.IQPhaseCorrectionFactor;
  a.corr_on = (ctx->params.mode == T41RX_DEMOD_LSB || ctx->params.mode == T41RX_DEMOD_USB) ? 1 : 0;
  a.dBScale = ctx->cal_dbscale;
  a.base = ctx->cal_base;
  a.lo0 = ctx->cal_lo0;
  a.lo1 = ctx->cal_lo1;
  a.width = ctx->cal_width;
  a.sideband = ctx->params.mode == T41RX_DEMOD_LSB ? 1 : ctx->params.mode == T41RX_DEMOD_USB ? 2 : 0;
  const hipError_t e = launch_cal(a, (hipStream_t)hip_stream);
  if (e != hipSuccess) return hip_fail(e, "calibration kernel launch");
  return T41RX_OK;
}

// host-pointer form: temporaries of its own (the audio path's staging buffers are not touched); the rows of d_pixel /
// d_spec a call leaves alone keep the caller's contents, so those two travel both ways
int calibrate_host_impl(t41rx_ctx *ctx, const void *I, const void *Q, int shared_input, const uint8_t *update, float *result,
                        int16_t *pixel, float *spec, int n_frames, bool q15) {
  if (!ctx || !I || !Q || !result) return fail(T41RX_ERR_ARG, "null argument");
  if (!ctx->cal_on) return fail(T41RX_ERR_ARG, "calibration is not switched on (t41rx_set_calibration)");
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

// rows of I / Q a process call reads: one per channel, or the input map's n_streams
int input_rows(const t41rx_ctx *ctx) { return ctx->n_streams > 0 ? ctx->n_streams : ctx->nchan; }

// staging buffers of the host-pointer entry points, sized in bytes per array: the two inputs (with an input map they
// hold n_streams rows, the output n_channels) and the output
int ensure_staging(t41rx_ctx *ctx, size_t in_bytes, size_t out_bytes) {
  if (in_bytes > ctx->staging_in_floats * sizeof(float)) {
    ctx->staging_in_floats = 0;
    ctx->d_in_i.reset();
    ctx->d_in_q.reset();
    const size_t nfl = (in_bytes + sizeof(float) - 1) / sizeof(float);
    HIP_TRY(dev_alloc(ctx->d_in_i, nfl * sizeof(float)));
    HIP_TRY(dev_alloc(ctx->d_in_q, nfl * sizeof(float)));
    ctx->staging_in_floats = nfl;
  }
  if (out_bytes > ctx->staging_floats * sizeof(float)) {
    ctx->staging_floats = 0;
    ctx->d_out.reset();
    const size_t nfl = (out_bytes + sizeof(float) - 1) / sizeof(float);
    HIP_TRY(dev_alloc(ctx->d_out, nfl * sizeof(float)));
    ctx->staging_floats = nfl;
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

// the product's host side is never a diagnostic build; what the KERNEL objects were built as is asked at run time
// (kernel_build_flags(), below): tools/build_variant.sh links this very object with diagnostic kernels
static_assert(T41RX_EXPERIMENT == 0 && t41::kKernelBuildFlags == 0, "rx_host.cpp is product code: build it without T41RX_EXPERIMENT / diagnostic switches");

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
  if (ctx->d_agc_pipe && std::getenv("T41RX_PIPE_STAT")) {  // the diagnostic build's counters (rx_chains.hpp: PIPE_STAT_*)
    unsigned long long c[16] = {};
    std::vector<unsigned long long> all((size_t)ctx->nchan * 16);
    (void)hipMemcpy(all.data(), ctx->d_agc_pipe.get() + pipe_layout(ctx->nchan).counters, all.size() * sizeof(unsigned long long),
                    hipMemcpyDeviceToHost);
    for (size_t i = 0; i < all.size(); ++i) c[i & 15] += all[i];
    std::fprintf(stderr, "pipe_stat chain_cycles %llu chains %llu slow_blocks %llu back_wait %llu duty_wait %llu blocks %llu chain_stage %llu chain_steps %llu front %llu prep %llu back %llu wave_iterations %llu chain_state_wait %llu\n",
                 c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], c[12]);
  }
  if (ctx->ft8d_sel_ev) (void)hipEventDestroy(ctx->ft8d_sel_ev);
  if (ctx->h_ft8d_sel) (void)hipHostFree(ctx->h_ft8d_sel);
  delete ctx;  // (its device buffers go here, on its device)
  return T41RX_OK;
}

int t41rx_set_params(t41rx_ctx *ctx, const t41rx_params *p) {
  if (!ctx || !p) return fail(T41RX_ERR_ARG, "null argument");
  const char *why = nullptr;
  if (!params_valid(*p, &why)) return fail(T41RX_ERR_ARG, why ? why : "bad params");
  if (p->fft_length != ctx->params.fft_length) return fail(T41RX_ERR_ARG, "fft_length cannot change on a live context");


  std::vector<float> nb(ctx->blob.size());
  int rc = design_blob(*p, nb.data(), nb.size() * sizeof(float));
  if (rc != T41RX_OK) return fail(rc, "coefficient design failed");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  ctx->blob.swap(nb);
  ctx->params = *p;
  if ((rc = upload_coeffs(ctx)) != T41RX_OK) return rc;
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

  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  std::memcpy(ctx->blob.data(), blob, need);
  ctx->params = bp;
  int rc = upload_coeffs(ctx);
  if (rc != T41RX_OK) return rc;
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

int t41rx_reset(t41rx_ctx *ctx) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  {  // (and the pipelined kernels' time-out counter)
    const int rc = pipe_timeouts_clear(ctx);
    if (rc != T41RX_OK) return rc;
  }
  // the calibration memory to power-on: FFT_spec_old, zoom memories, ring, pointer and pixelnew[] all zero
  if (ctx->d_cal) HIP_TRY(hipMemset(ctx->d_cal.get(), 0, sizeof(float) * kCalFloats * (size_t)ctx->nchan));
  // the panadapter memory and its frame counter likewise (pixelold = 0, newSpectrumFlag = 0)
  if (ctx->d_pan_mem) HIP_TRY(hipMemset(ctx->d_pan_mem.get(), 0, sizeof(float) * kPanFloats * (size_t)ctx->nchan));
  ctx->pan_counter = 0;
  ctx->pan_last_rows = 0;
  ctx->pan_last_first = -1;
  return reset_state(ctx);
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

int t41rx_set_noise_blanker(t41rx_ctx *ctx, int NB_on) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (NB_on != 0 && NB_on != 1) return fail(T41RX_ERR_ARG, "NB_on must be 0 or 1");
  if (NB_on && ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the noise blanker is built for fft_length 512");
  ctx->nb_on = NB_on;
  return T41RX_OK;
}
int t41rx_get_noise_blanker(const t41rx_ctx *ctx) { return ctx ? ctx->nb_on : T41RX_ERR_ARG; }

int t41rx_set_receive_eq_bands(t41rx_ctx *ctx, const float *coeffs) {
  if (!ctx || !coeffs) return fail(T41RX_ERR_ARG, "null argument");
  for (int i = 0; i < kEqCoefs; ++i)
    if (!std::isfinite(coeffs[i])) return fail(T41RX_ERR_ARG, "receive-equalizer band table: non-finite coefficient");
  std::memcpy(ctx->eq_coef, coeffs, sizeof(ctx->eq_coef));  // (passed by value to every launch: the next call uses it)
  ctx->eq_have_bands = true;
  return T41RX_OK;
}

int t41rx_set_receive_eq(t41rx_ctx *ctx, int receiveEQFlag, const int32_t *equalizerRec) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (receiveEQFlag != 0 && receiveEQFlag != 1) return fail(T41RX_ERR_ARG, "receiveEQFlag must be 0 or 1");
  if (receiveEQFlag && ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "the receive equalizer is built for fft_length 512");
  if (receiveEQFlag && !ctx->eq_have_bands)
    return fail(T41RX_ERR_ARG, "receive equalizer: no band table loaded (t41rx_set_receive_eq_bands)");
  if (equalizerRec) std::memcpy(ctx->eq_levels, equalizerRec, sizeof(ctx->eq_levels));
  ctx->eq_on = receiveEQFlag;
  return T41RX_OK;
}

int t41rx_get_receive_eq(const t41rx_ctx *ctx, int32_t *equalizerRec_out) {
  if (!ctx) return T41RX_ERR_ARG;
  if (equalizerRec_out) std::memcpy(equalizerRec_out, ctx->eq_levels, sizeof(ctx->eq_levels));
  return ctx->eq_on;
}

int t41rx_set_cw_tables(t41rx_ctx *ctx, const float *audio_filters, const float *decode_fir) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (audio_filters)
    for (int i = 0; i < kCwFilters * kCwFilterCoefs; ++i)
      if (!std::isfinite(audio_filters[i])) return fail(T41RX_ERR_ARG, "CW filter tables: non-finite coefficient");
  if (decode_fir)
    for (int i = 0; i < kCwFirTaps; ++i)
      if (!std::isfinite(decode_fir[i])) return fail(T41RX_ERR_ARG, "CW decode FIR: non-finite coefficient");
  // (passed by value to every launch: the next call uses them; no memory is reset)
  if (audio_filters) {
    std::memcpy(ctx->cw_coef, audio_filters, sizeof(ctx->cw_coef));
    ctx->cw_have_filters = true;
  }
  if (decode_fir) {
    std::memcpy(ctx->cw_fir, decode_fir, sizeof(ctx->cw_fir));
    ctx->cw_have_fir = true;
  }
  return T41RX_OK;
}

int t41rx_set_cw_filter(t41rx_ctx *ctx, int CWFilterIndex) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (CWFilterIndex < 0 || CWFilterIndex > kCwFilters) return fail(T41RX_ERR_ARG, "CWFilterIndex must be 0 .. 4, or 5 (off)");
  if (CWFilterIndex != kCwFilters) {
    if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the CW audio filters are built for fft_length 512");
    if (!ctx->cw_have_filters) return fail(T41RX_ERR_ARG, "CW audio filter: no filter tables loaded (t41rx_set_cw_tables)");
  }
  ctx->cw_filter = CWFilterIndex;
  return T41RX_OK;
}
int t41rx_get_cw_filter(const t41rx_ctx *ctx) { return ctx ? ctx->cw_filter : T41RX_ERR_ARG; }

int t41rx_set_cw_detector(t41rx_ctx *ctx, int decoderFlag, float *d_cw, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (decoderFlag != 0 && decoderFlag != 1) return fail(T41RX_ERR_ARG, "decoderFlag must be 0 or 1");
  if (decoderFlag) {
    if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the CW detector is built for fft_length 512");
    if (!d_cw) return fail(T41RX_ERR_ARG, "CW detector: no result buffer (d_cw is NULL)");
    if (reinterpret_cast<uintptr_t>(d_cw) & 3u) return fail(T41RX_ERR_ARG, "unaligned pointer");
    if (max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
    if (!ctx->cw_have_fir) return fail(T41RX_ERR_ARG, "CW detector: no decode FIR loaded (t41rx_set_cw_tables)");
  }
  ctx->cw_det = decoderFlag;
  ctx->cw_out = decoderFlag ? d_cw : nullptr;
  ctx->cw_frames = decoderFlag ? max_frames : 0;
  return T41RX_OK;
}
int t41rx_get_cw_detector(const t41rx_ctx *ctx) { return ctx ? ctx->cw_det : T41RX_ERR_ARG; }

int t41rx_set_cw_decode_tree(t41rx_ctx *ctx, const uint8_t *tree, int n) {
  if (!ctx || !tree) return fail(T41RX_ERR_ARG, "null argument");
  if (n != kCwTreeChars) return fail(T41RX_ERR_ARG, "CW decode tree: n must be 129 (bigMorseCodeTree)");
  std::memcpy(ctx->cw_tree, tree, (size_t)kCwTreeChars);  // (passed by value to every launch: the next call uses it)
  ctx->cw_have_tree = true;
  return T41RX_OK;
}

int t41rx_set_cw_decoder(t41rx_ctx *ctx, int on, int32_t *d_text, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (on != 0 && on != 1) return fail(T41RX_ERR_ARG, "CW decoder: on must be 0 or 1");
  if (on) {
    if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the CW decoder is built for fft_length 512");
    if (!d_text) return fail(T41RX_ERR_ARG, "CW decoder: no text buffer (d_text is NULL)");
    if (reinterpret_cast<uintptr_t>(d_text) & 3u) return fail(T41RX_ERR_ARG, "unaligned pointer");
    if (max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
    if (!ctx->cw_have_tree) return fail(T41RX_ERR_ARG, "CW decoder: no decode tree loaded (t41rx_set_cw_decode_tree)");
  }
  ctx->cw_dec = on;
  ctx->cw_text = on ? d_text : nullptr;
  ctx->cw_text_frames = on ? max_frames : 0;
  return T41RX_OK;
}
int t41rx_get_cw_decoder(const t41rx_ctx *ctx) { return ctx ? ctx->cw_dec : T41RX_ERR_ARG; }

int t41rx_set_cw_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (num < 0 || den <= 0) return fail(T41RX_ERR_ARG, "CW clock: num must be >= 0 and den > 0");
  ctx->cw_t0 = t0_ms;  // (passed by value to every launch: the next call uses it; the frame counters stay)
  ctx->cw_num = num;
  ctx->cw_den = den;
  return T41RX_OK;
}

int t41rx_reset_cw_histograms(t41rx_ctx *ctx, const uint8_t *channels, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (channels && n != ctx->nchan) return fail(T41RX_ERR_ARG, "n must equal n_channels");
  if (!ctx->d_cwdec) return T41RX_OK;  // the decoder has not run: its words are the power-on ones, which are ResetHistograms()'s
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<uint8_t> mask;
  if (channels) {
    HIP_TRY(dev_alloc(mask, (size_t)ctx->nchan));
    HIP_TRY(hipMemcpy(mask.get(), channels, (size_t)ctx->nchan, hipMemcpyHostToDevice));
  }
  HIP_TRY(launch_cw_decode_reset(ctx->d_cwdec.get(), mask.get(), ctx->nchan, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return T41RX_OK;
}

int t41rx_set_ft8_tables(t41rx_ctx *ctx, const float *window, const float *mag_db) {
  if (!ctx || !window || !mag_db) return fail(T41RX_ERR_ARG, "null argument");
  for (int i = 0; i < kFt8Fft; ++i)
    if (!std::isfinite(window[i])) return fail(T41RX_ERR_ARG, "FT8 window: non-finite entry");
  for (int i = 0; i < kFt8MagEntries; ++i)
    if (!std::isfinite(mag_db[i])) return fail(T41RX_ERR_ARG, "FT8 mag_db table: non-finite entry");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old tables)
  if (!ctx->d_ft8_win) HIP_TRY(dev_alloc(ctx->d_ft8_win, sizeof(float) * kFt8Fft));
  if (!ctx->d_ft8_mag) HIP_TRY(dev_alloc(ctx->d_ft8_mag, sizeof(float) * kFt8MagEntries));
  HIP_TRY(hipMemcpy(ctx->d_ft8_win.get(), window, sizeof(float) * kFt8Fft, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->d_ft8_mag.get(), mag_db, sizeof(float) * kFt8MagEntries, hipMemcpyHostToDevice));
  ctx->ft8_have_tables = true;
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
    if (!ctx->ft8_have_tables) return fail(T41RX_ERR_ARG, "FT8 receive: no tables loaded (t41rx_set_ft8_tables)");
  }
  ctx->ft8_on = on;
  ctx->ft8_power = on ? d_power : nullptr;
  ctx->ft8_status = on ? d_status : nullptr;
  ctx->ft8_frames = on ? max_frames : 0;
  return T41RX_OK;
}
int t41rx_get_ft8(const t41rx_ctx *ctx) { return ctx ? ctx->ft8_on : T41RX_ERR_ARG; }

int t41rx_set_ft8_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (num < 0 || den <= 0) return fail(T41RX_ERR_ARG, "FT8 clock: num must be >= 0 and den > 0");
  ctx->ft8_t0 = t0_ms;  // (passed by value to every launch: the next call uses it; the frame counters stay)
  ctx->ft8_num = num;
  ctx->ft8_den = den;
  return T41RX_OK;
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
  if (channels) {
    HIP_TRY(dev_alloc(mask, (size_t)ctx->nchan));
    HIP_TRY(hipMemcpy(mask.get(), channels, (size_t)ctx->nchan, hipMemcpyHostToDevice));
  }
  HIP_TRY(launch_ft8_sync(ctx->d_ft8.get(), mask.get(), ctx->nchan, ctx->ft8_t0, ctx->ft8_num, ctx->ft8_den, nullptr));
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
  if (!ctx->d_ft8) {  // the stage has not run: its words are the power-on ones
    std::memset(body, 0, n);
    return T41RX_OK;
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(body, ctx->d_ft8.get(), n, hipMemcpyDeviceToHost));
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
  HIP_TRY(hipMemcpy(ctx->d_ft8.get(), all, bytes - kFt8HeaderBytes, hipMemcpyHostToDevice));
  return T41RX_OK;
}

// ---- FT8 from 12 kS/s audio (DEMOD_FT8_WAV) ----
namespace {
// everything is checked before anything is allocated, launched or written
int ft8_audio_refusal(const t41rx_ctx *ctx, const void *pcm, int n_frames, unsigned align_mask) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!ctx->ft8_have_tables) return fail(T41RX_ERR_ARG, "FT8 audio: no tables loaded (t41rx_set_ft8_tables)");
  if (!ctx->ft8_on) return fail(T41RX_ERR_ARG, "FT8 audio: FT8 receive is off (t41rx_set_ft8: no d_power / d_status to write)");
  if (n_frames < 1) return fail(T41RX_ERR_ARG, "FT8 audio: n_frames must be >= 1");
  if (n_frames > T41RX_FT8_MAX_FRAMES) return fail(T41RX_ERR_ARG, "FT8 audio: n_frames must be <= 1380 (at most one completed slot per call)");
  if (n_frames > ctx->ft8_frames) return fail(T41RX_ERR_ARG, "FT8 audio: n_frames exceeds the max_frames the FT8 status buffer was set with");
  if (!pcm) return fail(T41RX_ERR_ARG, "FT8 audio: no samples (NULL pointer)");
  if (reinterpret_cast<uintptr_t>(pcm) & align_mask) return fail(T41RX_ERR_ARG, "FT8 audio: the sample pointer is not aligned to its type");
  return T41RX_OK;
}

int ft8_audio_device(t41rx_ctx *ctx, const void *d_pcm, int n_frames, bool q15) {
  if (const int rc = ft8_audio_refusal(ctx, d_pcm, n_frames, q15 ? 1u : 3u)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  if (const int rc = ensure_ft8(ctx)) return rc;
  Ft8AudioArgs a{};
  a.pcm = d_pcm;
  a.state = ctx->d_ft8.get();
  a.power = ctx->ft8_power;
  a.status = ctx->ft8_status;
  a.window = ctx->d_ft8_win.get();
  a.mag_db = ctx->d_ft8_mag.get();
  a.tab = ctx->d_ft8_tab.get();
  a.nchan = ctx->nchan;
  a.nframes = n_frames;
  a.q15 = q15 ? 1 : 0;
  const hipError_t e = launch_ft8_audio(a, nullptr);
  if (e != hipSuccess) return hip_fail(e, "FT8 audio kernel launch");
  return T41RX_OK;
}

int ft8_audio_host(t41rx_ctx *ctx, const void *pcm, int n_frames, bool q15) {
  if (const int rc = ft8_audio_refusal(ctx, pcm, n_frames, q15 ? 1u : 3u)) return rc;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const size_t bytes = (size_t)ctx->nchan * (size_t)n_frames * kFt8AudioFrame * (q15 ? sizeof(int16_t) : sizeof(float));
  DevBuf<char> staged;
  if (dev_alloc(staged, bytes) != hipSuccess) return fail(T41RX_ERR_NOMEM, "FT8 audio: staging allocation failed");
  HIP_TRY(hipMemcpy(staged.get(), pcm, bytes, hipMemcpyHostToDevice));
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
  if (channels) {
    HIP_TRY(dev_alloc(mask, (size_t)ctx->nchan));
    HIP_TRY(hipMemcpy(mask.get(), channels, (size_t)ctx->nchan, hipMemcpyHostToDevice));
  }
  HIP_TRY(launch_ft8_audio_mark(ctx->d_ft8.get(), mask.get(), ctx->nchan, end, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return T41RX_OK;
}
}  // namespace

int t41rx_ft8_audio_device_q15(t41rx_ctx *ctx, const int16_t *d_pcm, int n_frames) { return ft8_audio_device(ctx, d_pcm, n_frames, true); }
int t41rx_ft8_audio_device(t41rx_ctx *ctx, const float *d_audio, int n_frames) { return ft8_audio_device(ctx, d_audio, n_frames, false); }
int t41rx_ft8_audio_host_q15(t41rx_ctx *ctx, const int16_t *pcm, int n_frames) { return ft8_audio_host(ctx, pcm, n_frames, true); }
int t41rx_ft8_audio_host(t41rx_ctx *ctx, const float *audio, int n_frames) { return ft8_audio_host(ctx, audio, n_frames, false); }
int t41rx_ft8_audio_begin(t41rx_ctx *ctx, const uint8_t *channels, int n) { return ft8_audio_mark(ctx, channels, n, 0); }
int t41rx_ft8_audio_end(t41rx_ctx *ctx, const uint8_t *channels, int n) { return ft8_audio_mark(ctx, channels, n, 1); }

// ---- FT8 decode of a finished slot ----
int t41rx_set_ft8_decode_tables(t41rx_ctx *ctx, const uint8_t *costas, const uint8_t *gray, const uint8_t *nm, const uint8_t *mn,
                                const uint8_t *nrw) {
  if (!ctx || !costas || !gray || !nm || !mn || !nrw) return fail(T41RX_ERR_ARG, "null argument");
  // what the kernels index with: everything is checked before anything is written
  Ft8DecodeTables h{};
  for (int k = 0; k < 7; ++k) {
    if (costas[k] > 7) return fail(T41RX_ERR_ARG, "FT8 decode tables: kCostas_map entry outside 0..7");
    h.costas[k] = costas[k];
  }
  for (int k = 0; k < 8; ++k) {
    if (gray[k] > 7) return fail(T41RX_ERR_ARG, "FT8 decode tables: kGray_map entry outside 0..7");
    h.gray[k] = gray[k];
  }
  for (int c = 0; c < kLdpcM; ++c) {
    if (nrw[c] < 1 || nrw[c] > 7) return fail(T41RX_ERR_ARG, "FT8 decode tables: kNrw entry outside 1..7");
    h.nrw[c] = nrw[c];
    for (int k = 0; k < nrw[c]; ++k) {
      if (nm[c * 7 + k] < 1 || nm[c * 7 + k] > kLdpcN) return fail(T41RX_ERR_ARG, "FT8 decode tables: kNm entry outside 1..174");
      h.nm[c * 7 + k] = (uint8_t)(nm[c * 7 + k] - 1);
    }
  }
  for (int p = 0; p < kFt8BitChecks; ++p) {
    if (mn[p] < 1 || mn[p] > kLdpcM) return fail(T41RX_ERR_ARG, "FT8 decode tables: kMn entry outside 1..83");
    h.mn[p] = (uint8_t)(mn[p] - 1);
  }
  for (int i = 0; i < kLdpcN; ++i)
    for (int j = 0; j < 3; ++j) {
      const int c = h.mn[3 * i + j];
      int at = -1, count = 0;
      for (int k = 0; k < h.nrw[c]; ++k)
        if (h.nm[c * 7 + k] == i) {
          at = k;
          ++count;
        }
      if (count != 1) return fail(T41RX_ERR_ARG, "FT8 decode tables: a check of kMn does not list its bit exactly once in kNm");
      h.pos[3 * i + j] = (uint8_t)at;
    }
  // the other way round (bp_decode()'s `kMn[ibj][kk] - 1 == i`): every entry of a check is one of its bit's three checks, once
  for (int c = 0; c < kLdpcM; ++c)
    for (int k = 0; k < h.nrw[c]; ++k) {
      const int b = h.nm[c * 7 + k];
      int at = -1, count = 0;
      for (int j = 0; j < 3; ++j)
        if (h.mn[3 * b + j] == c) {
          at = j;
          ++count;
        }
      if (count != 1) return fail(T41RX_ERR_ARG, "FT8 decode tables: a bit of kNm does not list its check exactly once in kMn");
      h.kk[c * 7 + k] = (uint8_t)at;
    }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old tables)
  if (!ctx->d_ft8d_tab) HIP_TRY(dev_alloc(ctx->d_ft8d_tab, sizeof(Ft8DecodeTables)));
  HIP_TRY(hipMemcpy(ctx->d_ft8d_tab.get(), &h, sizeof(h), hipMemcpyHostToDevice));
  ctx->ft8d_have_tables = true;
  return T41RX_OK;
}

int t41rx_set_ft8_decode(t41rx_ctx *ctx, int max_candidates, int min_score, int ldpc_iterations) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (max_candidates < 1 || max_candidates > T41RX_FT8_MAX_CANDIDATES) return fail(T41RX_ERR_ARG, "FT8 decode: max_candidates must be 1..20");
  if (ldpc_iterations < 1 || ldpc_iterations > 50) return fail(T41RX_ERR_ARG, "FT8 decode: ldpc_iterations must be 1..50");
  ctx->ft8d_max_candidates = max_candidates;
  ctx->ft8d_min_score = min_score;
  ctx->ft8d_iterations = ldpc_iterations;
  return T41RX_OK;
}

int t41rx_get_ft8_decode(const t41rx_ctx *ctx, int *max_candidates, int *min_score, int *ldpc_iterations) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (max_candidates) *max_candidates = ctx->ft8d_max_candidates;
  if (min_score) *min_score = ctx->ft8d_min_score;
  if (ldpc_iterations) *ldpc_iterations = ctx->ft8d_iterations;
  return T41RX_OK;
}

int t41rx_set_ft8_decode_debug(t41rx_ctx *ctx, float *d_log174, uint8_t *d_plain) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  ctx->ft8d_dbg_log174 = d_log174;
  ctx->ft8d_dbg_plain = d_plain;
  return T41RX_OK;
}

int t41rx_ft8_decode_device(t41rx_ctx *ctx, const uint8_t *d_waterfall, size_t channel_stride_bytes, const int8_t *select, int n,
                            t41rx_ft8_result *d_results, void *hip_stream) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!d_results) return fail(T41RX_ERR_ARG, "FT8 decode: no result buffer (d_results is NULL)");
  if (!ctx->ft8d_have_tables) return fail(T41RX_ERR_ARG, "FT8 decode: no tables loaded (t41rx_set_ft8_decode_tables)");
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "FT8 decode: n must equal n_channels");
  bool slot1 = false;
  if (select)
    for (int c = 0; c < n; ++c) {
      if (select[c] < -1 || select[c] > 1) return fail(T41RX_ERR_ARG, "FT8 decode: select must be -1 (skip), 0 or 1");
      slot1 = slot1 || select[c] == 1;
    }
  if (!d_waterfall) {
    if (!ctx->ft8_on) return fail(T41RX_ERR_ARG, "FT8 decode: d_waterfall is NULL and FT8 receive is off (no d_power to read)");
    d_waterfall = ctx->ft8_power;
    channel_stride_bytes = 2 * (size_t)kFt8HalfBytes;
  }
  if ((reinterpret_cast<uintptr_t>(d_waterfall) & 3u) || (channel_stride_bytes & 3u))
    return fail(T41RX_ERR_ARG, "FT8 decode: the waterfall and its channel stride must be 4-byte aligned");
  if (n > 1 && channel_stride_bytes < (size_t)kFt8HalfBytes * (slot1 ? 2 : 1))
    return fail(T41RX_ERR_ARG, "FT8 decode: channel_stride_bytes is smaller than the slots the call reads");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const hipStream_t s = (hipStream_t)hip_stream;
  if (select) {
    if (!ctx->d_ft8d_sel) {
      HIP_TRY(dev_alloc(ctx->d_ft8d_sel, (size_t)n));
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_ft8d_sel), (size_t)n, hipHostMallocDefault));
      HIP_TRY(hipEventCreateWithFlags(&ctx->ft8d_sel_ev, hipEventDisableTiming));
    } else {
      HIP_TRY(hipEventSynchronize(ctx->ft8d_sel_ev));  // the upload of the call before has read the pinned copy
    }
    std::memcpy(ctx->h_ft8d_sel, select, (size_t)n);
    HIP_TRY(hipMemcpyAsync(ctx->d_ft8d_sel.get(), ctx->h_ft8d_sel, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(ctx->ft8d_sel_ev, s));
  }
  const size_t taps = (size_t)n * T41RX_FT8_MAX_CANDIDATES * kLdpcN;
  if (ctx->ft8d_dbg_log174) HIP_TRY(hipMemsetAsync(ctx->ft8d_dbg_log174, 0, taps * sizeof(float), s));  // unused rows read zero
  if (ctx->ft8d_dbg_plain) HIP_TRY(hipMemsetAsync(ctx->ft8d_dbg_plain, 0, taps, s));
  Ft8DecodeArgs a{};
  a.waterfall = d_waterfall;
  a.stride = channel_stride_bytes;
  a.select = select ? ctx->d_ft8d_sel.get() : nullptr;
  a.tab = ctx->d_ft8d_tab.get();
  a.results = d_results;
  a.dbg_log174 = ctx->ft8d_dbg_log174;
  a.dbg_plain = ctx->ft8d_dbg_plain;
  a.nchan = n;
  a.max_candidates = ctx->ft8d_max_candidates;
  a.min_score = ctx->ft8d_min_score;
  a.iterations = ctx->ft8d_iterations;
  const hipError_t e = launch_ft8_decode(a, s);
  if (e != hipSuccess) return hip_fail(e, "FT8 decode kernel launch");
  return T41RX_OK;
}

int t41rx_ft8_decode_host(t41rx_ctx *ctx, const uint8_t *d_waterfall, size_t channel_stride_bytes, const int8_t *select, int n,
                          t41rx_ft8_result *results) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!results) return fail(T41RX_ERR_ARG, "FT8 decode: no result buffer (results is NULL)");
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "FT8 decode: n must equal n_channels");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  if (!ctx->d_ft8d_res) HIP_TRY(dev_alloc(ctx->d_ft8d_res, sizeof(t41rx_ft8_result) * (size_t)n));
  if (const int rc = t41rx_ft8_decode_device(ctx, d_waterfall, channel_stride_bytes, select, n, ctx->d_ft8d_res.get(), nullptr)) return rc;
  HIP_TRY(hipMemcpy(results, ctx->d_ft8d_res.get(), sizeof(t41rx_ft8_result) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return T41RX_OK;
}

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
  if (!ctx || !Q_in_L || !Q_in_R || !Q_out_L) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const size_t bytes = (size_t)ctx->nchan * (size_t)n_frames * (size_t)(4 * ctx->params.fft_length) * sizeof(int16_t);
  const size_t in_bytes = bytes / (size_t)ctx->nchan * (size_t)input_rows(ctx);  // an input map: n_streams rows come in
  int rc = ensure_staging(ctx, in_bytes, bytes);
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipMemcpy(ctx->d_in_i.get(), Q_in_L, in_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->d_in_q.get(), Q_in_R, in_bytes, hipMemcpyHostToDevice));
  rc = t41rx_process_device_q15(ctx, reinterpret_cast<const int16_t *>(ctx->d_in_i.get()), reinterpret_cast<const int16_t *>(ctx->d_in_q.get()),
                                reinterpret_cast<int16_t *>(ctx->d_out.get()), n_frames, nullptr);
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(Q_out_L, ctx->d_out.get(), bytes, hipMemcpyDeviceToHost));
  return pipe_status(ctx);  // (these calls synchronise: samples of a run whose hand-over broke do not leave with OK)
}

int t41rx_process_host(t41rx_ctx *ctx, const float *I, const float *Q, float *audio, int n_frames) {
  if (!ctx || !I || !Q || !audio) return fail(T41RX_ERR_ARG, "null argument");
  if (n_frames <= 0) return fail(T41RX_ERR_ARG, "n_frames must be > 0");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const size_t nfl = (size_t)ctx->nchan * (size_t)n_frames * (size_t)(4 * ctx->params.fft_length);
  const size_t in_fl = nfl / (size_t)ctx->nchan * (size_t)input_rows(ctx);  // an input map: n_streams rows come in
  {
    const int rc0 = ensure_staging(ctx, in_fl * sizeof(float), nfl * sizeof(float));
    if (rc0 != T41RX_OK) return rc0;
  }
  HIP_TRY(hipMemcpy(ctx->d_in_i.get(), I, in_fl * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ctx->d_in_q.get(), Q, in_fl * sizeof(float), hipMemcpyHostToDevice));
  int rc = t41rx_process_device(ctx, ctx->d_in_i.get(), ctx->d_in_q.get(), ctx->d_out.get(), n_frames, nullptr);
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(audio, ctx->d_out.get(), nfl * sizeof(float), hipMemcpyDeviceToHost));
  return pipe_status(ctx);  // (these calls synchronise: samples of a run whose hand-over broke do not leave with OK)
}

size_t t41rx_state_bytes(const t41rx_ctx *ctx) { return ctx ? state_bytes(ctx, state_sections(ctx)) : 0; }

int t41rx_get_state(t41rx_ctx *ctx, void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  if (bytes < t41rx_state_bytes(ctx)) return fail(T41RX_ERR_STATE, "state buffer too small");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  int rc = pipe_status(ctx);
  if (rc != T41RX_OK) return rc;
  const int32_t sec = state_sections(ctx);
  const size_t sf = state_floats(ctx->params.fft_length);
  int32_t hdr[8] = {(int32_t)kStateMagic, T41RX_ABI_VERSION, ctx->params.fft_length, ctx->nchan,
                    (int32_t)sf, sec, (sec & kSecDisp) ? ctx->disp_zoom : 0, 0};
  std::memcpy(host_buf, hdr, sizeof(hdr));
  char *out = static_cast<char *>(host_buf) + kStateHeaderBytes;
  HIP_TRY(hipMemcpy(out, ctx->d_state.get(), path_bytes(ctx), hipMemcpyDeviceToHost));
  // canonical checkpoint: the current oscillator state in both slots
  float *rec = reinterpret_cast<float *>(out);
  for (int c = 0; c < ctx->nchan; ++c) {
    float *n = rec + sf * (size_t)c + kStNco;
    std::memcpy(n + 4 * (ctx->nco_sel ^ 1), n + 4 * ctx->nco_sel, sizeof(NcoState));
  }
  out += path_bytes(ctx);
  for (const Section &s : kSections) {
    if (!(sec & s.bit)) continue;
    if ((rc = s.get(ctx, out, section_bytes(s, ctx->nchan))) != T41RX_OK) return rc;
    out += section_bytes(s, ctx->nchan);
  }
  return T41RX_OK;
}

int t41rx_set_state(t41rx_ctx *ctx, const void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  if (bytes < kStateHeaderBytes) return fail(T41RX_ERR_STATE, "state size mismatch");
  int32_t hdr[8];
  std::memcpy(hdr, host_buf, sizeof(hdr));
  if ((uint32_t)hdr[0] != kStateMagic || hdr[1] != T41RX_ABI_VERSION || hdr[2] != ctx->params.fft_length ||
      hdr[3] != ctx->nchan || hdr[4] != (int32_t)state_floats(ctx->params.fft_length))
    return fail(T41RX_ERR_STATE, "checkpoint header does not match this context (magic / abi / fft_length / channels)");
  const int32_t sec = hdr[5];
  int32_t known = 0;
  for (const Section &s : kSections) known |= s.bit;
  if (sec & ~known) return fail(T41RX_ERR_STATE, "checkpoint: unknown sections");
  if (bytes != state_bytes(ctx, sec)) return fail(T41RX_ERR_STATE, "state size mismatch");
  // everything is checked before anything is written: a refused checkpoint changes nothing
  const float *rec = reinterpret_cast<const float *>(static_cast<const char *>(host_buf) + kStateHeaderBytes);
  const char *sections = reinterpret_cast<const char *>(rec) + path_bytes(ctx), *p = sections;
  int rc = T41RX_OK;
  for (const Section &s : kSections) {
    if (!(sec & s.bit)) continue;
    if (ctx->params.fft_length != 512)
      return fail(T41RX_ERR_STATE, std::string("checkpoint: ") + s.name + " section at a long fft_length");
    if (s.check && (rc = s.check(ctx, hdr, reinterpret_cast<const float *>(p))) != T41RX_OK) return rc;
    p += section_bytes(s, ctx->nchan);
  }
  if ((rc = check_records(ctx, rec)) != T41RX_OK) return rc;
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  for (const Section &s : kSections)
    if ((sec & s.bit) && s.ensure && (rc = s.ensure(ctx)) != T41RX_OK) return rc;
  HIP_TRY(hipMemcpy(ctx->d_state.get(), rec, path_bytes(ctx), hipMemcpyHostToDevice));
  ctx->nco_sel = 0;  // (a checkpoint carries the current oscillator state in both slots)
  // The side stages' memories follow the checkpoint too: restored where it carries them, back to power-on where it
  // does not (a checkpoint taken before the stages first ran) -- never the values of the stream being replaced.
  p = sections;
  for (const Section &s : kSections) {
    const size_t n = section_bytes(s, ctx->nchan);
    if ((rc = (sec & s.bit) ? s.put(ctx, p, n) : s.reset(ctx, n)) != T41RX_OK) return rc;
    if (sec & s.bit) p += n;
  }
  if ((rc = ft8_power_on(ctx)) != T41RX_OK) return rc;  // (the FT8 memory has a record of its own: a checkpoint starts it afresh)
  return pipe_timeouts_clear(ctx);  // the restored state is valid again
}

int t41rx_set_debug_taps(t41rx_ctx *ctx, float *d_post_nco, float *d_dec, float *d_demod, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const bool any = d_post_nco || d_dec || d_demod;
  // (T41RX_STAMP_TAPS: the -DT41RX_STAMP diagnostic kernels of the long-FFT pipeline put their cycle stamps behind the demod tap)
  if (any && ctx->params.fft_length != 512 && !std::getenv("T41RX_STAMP_TAPS"))
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
  if (d_spect && ctx->pan_on) return fail(T41RX_ERR_UNSUPPORTED, "the panadapter stage is on and owns the audio-spectrum tap (t41rx_set_panadapter)");
  ctx->spect = d_spect;
  ctx->spect_max = d_max;
  ctx->spect_frames = d_spect ? max_frames : 0;
  return T41RX_OK;
}

int t41rx_set_display_spectrum(t41rx_ctx *ctx, float *d_spec, float *d_spec_old, int spectrumZoom, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null context");
  if ((d_spec == nullptr) != (d_spec_old == nullptr)) return fail(T41RX_ERR_ARG, "set both pointers or neither");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  if (!d_spec) {
    ctx->disp_spec = ctx->disp_old = nullptr;
    ctx->disp_frames = 0;
    return T41RX_OK;
  }
  if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the display FFT is built for fft_length 512");
  if (ctx->pan_on) return fail(T41RX_ERR_UNSUPPORTED, "the panadapter stage is on and owns the display tap (t41rx_set_panadapter)");
  if (spectrumZoom < 0 || spectrumZoom > 4) return fail(T41RX_ERR_ARG, "spectrumZoom must be 0 (1x) .. 4 (16x)");  // MAX_ZOOM_ENTRIES, ButtonProc.h:6
  if (max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
  if ((reinterpret_cast<uintptr_t>(d_spec) | reinterpret_cast<uintptr_t>(d_spec_old)) & 3u) return fail(T41RX_ERR_ARG, "unaligned pointer");
  // Anything that fails from here on leaves the side output switched OFF (a previous successful
  // call's pointers must not survive next to a freed tap buffer: the display kernel would read it).
  ctx->disp_spec = ctx->disp_old = nullptr;
  const int had_frames = ctx->disp_frames;
  ctx->disp_frames = 0;
  if (max_frames > had_frames || !ctx->d_pre)
    HIP_TRY(dev_alloc(ctx->d_pre, sizeof(float) * 4096 * (size_t)max_frames * (size_t)ctx->nchan));
  if (!ctx->d_disp) HIP_TRY(dev_alloc(ctx->d_disp, sizeof(float) * kDispFloats * (size_t)ctx->nchan));
  if (const int rc = ensure_window(ctx)) return rc;
  HIP_TRY(hipMemset(ctx->d_disp.get(), 0, sizeof(float) * kDispFloats * (size_t)ctx->nchan));  // ZoomFFTPrep(): a fresh start
  if (max_frames < had_frames) max_frames = had_frames;  // (the tap buffer was kept: it still holds that many)
  ctx->disp_spec = d_spec;
  ctx->disp_old = d_spec_old;
  ctx->disp_frames = max_frames;
  ctx->disp_zoom = spectrumZoom;
  return T41RX_OK;
}

int t41rx_set_panadapter_tables(t41rx_ctx *ctx, const uint16_t *gradient, int n) {
  if (!ctx || !gradient) return fail(T41RX_ERR_ARG, "null argument");
  if (n != kPanGradient) return fail(T41RX_ERR_ARG, "panadapter tables: gradient[] has 117 words (Display.cpp:148-161)");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old table)
  if (!ctx->d_pan_grad) HIP_TRY(dev_alloc(ctx->d_pan_grad, sizeof(uint16_t) * kPanGradient));
  HIP_TRY(hipMemcpy(ctx->d_pan_grad.get(), gradient, sizeof(uint16_t) * kPanGradient, hipMemcpyHostToDevice));
  ctx->pan_have_tables = true;
  return T41RX_OK;
}

int t41rx_set_panadapter(t41rx_ctx *ctx, int on, int spectrumZoom, int currentScale, int pixel_offset, int spectrumNoiseFloor,
                         int update_period, int update_phase, const t41rx_panadapter_out *out, int max_rows) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  if (!on) {
    ctx->pan_on = false;
    return T41RX_OK;
  }
  // every refusal in front of the first change: a refused call leaves the stage as it was
  if (!out) return fail(T41RX_ERR_ARG, "null argument");
  if (!ctx->pan_have_tables) return fail(T41RX_ERR_ARG, "panadapter: no colour table loaded (t41rx_set_panadapter_tables)");
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
  if (ctx->disp_spec || ctx->spect)
    return fail(T41RX_ERR_UNSUPPORTED, "t41rx_set_display_spectrum / t41rx_set_audio_spectrum is set and owns its tap: switch it off first");
  // anything that fails from here on leaves the stage switched off
  ctx->pan_on = false;
  if (max_rows > ctx->pan_alloc_rows || !ctx->d_pan_pre || !ctx->d_pan_max) {
    ctx->pan_alloc_rows = 0;
    HIP_TRY(dev_alloc(ctx->d_pan_pre, sizeof(float) * 4096 * (size_t)max_rows * (size_t)ctx->nchan));
    HIP_TRY(dev_alloc(ctx->d_pan_max, sizeof(float) * 3 * (size_t)max_rows * (size_t)ctx->nchan));
    ctx->pan_alloc_rows = max_rows;
  }
  if (!ctx->d_pan_mem) HIP_TRY(dev_alloc(ctx->d_pan_mem, sizeof(float) * kPanFloats * (size_t)ctx->nchan));
  if (const int rc = ensure_window(ctx)) return rc;
  if (!ctx->d_pan_nf)
    if (const int rc = pan_upload_levels<int32_t>(ctx, ctx->d_pan_nf, nullptr)) return rc;
  if (!ctx->d_pan_gc)
    if (const int rc = pan_upload_levels<float>(ctx, ctx->d_pan_gc, nullptr)) return rc;
  // power-on: ZoomFFTPrep(), FFT_spec_old = 0, pixelold = 0, newSpectrumFlag = 0; the frame counter starts at 0
  HIP_TRY(hipMemset(ctx->d_pan_mem.get(), 0, sizeof(float) * kPanFloats * (size_t)ctx->nchan));
  ctx->pan_out = *out;
  ctx->pan_zoom = spectrumZoom;
  ctx->pan_scale = currentScale;
  ctx->pan_pixel_offset = pixel_offset;
  ctx->pan_floor_y = spectrumNoiseFloor;
  ctx->pan_period = update_period;
  ctx->pan_phase = update_phase;
  ctx->pan_max_rows = max_rows;
  ctx->pan_counter = 0;
  ctx->pan_last_rows = 0;
  ctx->pan_last_first = -1;
  ctx->pan_on = true;
  return T41RX_OK;
}

int t41rx_set_panadapter_levels(t41rx_ctx *ctx, const int32_t *noise_floor, const float *gain_correction, int attenuator) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  for (int c = 0; noise_floor && c < ctx->nchan; ++c)
    if (noise_floor[c] < -32768 || noise_floor[c] > 32767) return fail(T41RX_ERR_ARG, "panadapter levels: a noise floor must fit an int16");
  for (int c = 0; gain_correction && c < ctx->nchan; ++c)
    if (!std::isfinite(gain_correction[c])) return fail(T41RX_ERR_ARG, "panadapter levels: non-finite gain correction");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old levels)
  if (const int rc = pan_upload_levels<int32_t>(ctx, ctx->d_pan_nf, noise_floor)) return rc;
  if (const int rc = pan_upload_levels<float>(ctx, ctx->d_pan_gc, gain_correction)) return rc;
  ctx->pan_attenuator = attenuator;
  return T41RX_OK;
}

int t41rx_get_panadapter(const t41rx_ctx *ctx, int64_t *frame_counter, int32_t *rows_written, int64_t *first_row_frame) {
  if (!ctx) return T41RX_ERR_ARG;
  if (frame_counter) *frame_counter = ctx->pan_counter;
  if (rows_written) *rows_written = ctx->pan_last_rows;
  if (first_row_frame) *first_row_frame = ctx->pan_last_first;
  return ctx->pan_on ? 1 : 0;
}

int t41rx_set_panadapter_counter(t41rx_ctx *ctx, int64_t n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (n < 0) return fail(T41RX_ERR_ARG, "the frame counter must be >= 0");
  ctx->pan_counter = n;
  return T41RX_OK;
}

int t41rx_set_calibration(t41rx_ctx *ctx, int on, int spectrumZoom, int currentScale, int pixel_offset, int bin0, int bin1,
                          int capture_bins) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  if (!on) {
    ctx->cal_on = false;
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
  ctx->cal_on = false;
  if (!ctx->d_cal) HIP_TRY(dev_alloc(ctx->d_cal, sizeof(float) * kCalFloats * (size_t)ctx->nchan));
  if (const int rc = ensure_window(ctx)) return rc;
  HIP_TRY(hipMemset(ctx->d_cal.get(), 0, sizeof(float) * kCalFloats * (size_t)ctx->nchan));  // power-on: ZoomFFTPrep(), pixelnew[] = 0
  ctx->cal_zoom = spectrumZoom;
  ctx->cal_dbscale = kDbScale[currentScale];
  ctx->cal_base = kBaseOffset[currentScale] + pixel_offset;
  ctx->cal_lo0 = bin0 - capture_bins;
  ctx->cal_lo1 = bin1 - capture_bins;
  ctx->cal_width = 2 * capture_bins;
  ctx->cal_on = true;
  return T41RX_OK;
}

int t41rx_set_cal_corrections(t41rx_ctx *ctx, const float *amp, const float *phase) {
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
  HIP_TRY(hipDeviceSynchronize());  // (a launch still in flight reads the old candidates)
  if (!ctx->d_cal_corr) HIP_TRY(dev_alloc(ctx->d_cal_corr, sizeof(float) * h.size()));
  HIP_TRY(hipMemcpy(ctx->d_cal_corr.get(), h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
  ctx->cal_per_channel = true;
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
