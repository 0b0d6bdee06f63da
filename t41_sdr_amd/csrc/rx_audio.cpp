// t41_sdr_amd/csrc/rx_audio.cpp -- host side of the audio stages between the demodulator and the interpolators: the
// receive equalizer (eq_kernel.hip), the noise reduction / notch (nr_kernels.hip) and the noise blanker (nb_kernel.hip).
// Their memories on first use, the launches of a process call, their checkpoint sections and their setters.
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {

int ensure_zeroed(DevBuf<float> &b, size_t bytes, const char *what) {
  if (b) return T41RX_OK;
  DevBuf<float> z;
  if (dev_alloc(z, bytes) != hipSuccess) return fail(T41RX_ERR_NOMEM, std::string(what) + " state allocation failed");
  if (hipMemset(z.get(), 0, bytes) != hipSuccess) return fail(T41RX_ERR_HIP, std::string(what) + " state upload failed");
  b = std::move(z);
  return T41RX_OK;
}

// ---- receive equalizer
// its biquad memories (Filter.cpp:43-56)
int ensure_eq(t41rx_ctx *ctx) {
  return ensure_zeroed(ctx->eq.d_state, sizeof(float) * kEqStateFloats * (size_t)ctx->nchan, "receive-equalizer");
}

// Process.cpp:828-832 on the call's audio @24 kS/s
int eq_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  const StageList l = stage_list(ctx, kStageEq);
  if (l.empty()) return T41RX_OK;  // the stage map lists no channel: nothing to launch
  EqArgs q{};
  q.list = l.list;
  q.nlist = l.n;
  q.aud = ctx->d_aud24.get();
  q.state = ctx->eq.d_state.get();
  q.nchan = ctx->nchan;
  q.nsamp = n_frames * 256;
  if (ctx->eq.map_on) q.levels = ctx->eq.d_levels.get();  // (the level map: converted at set time by the expression below)
  std::memcpy(q.coef, ctx->eq.coef, sizeof(q.coef));
  for (int b = 0; b < kEqBands; ++b) {
    // recEQ_LevelScale[b] = (float)EEPROMData.equalizerRec[b] / 100.0 (Filter.cpp:119-121); arm_scale_f32 by its
    // negative for bands 1, 3, .., 13 (Filter.cpp:138-151)
    const float lvl = (float)((double)(float)ctx->eq.levels[b] / 100.0);
    q.scale[b] = (b % 2 == 0) ? -lvl : lvl;
  }
  return hip_check(launch_eq(q, s), "receive-equalizer kernel launch");
}

// ---- noise reduction / notch
namespace {
// InitializeDataArrays() + SpectralNoiseReductionInit() (T41_SDR.ino:479-504, 657): Xanr()'s and the spectral functions'
// memories at power-on
hipError_t nr_power_on(float *anr, float *spec, int nchan) {
  std::vector<float> ha((size_t)kAnrStRows * (size_t)nchan), hs((size_t)kNrSpecFloats * (size_t)nchan);
  nr_reset_anr(ha.data(), (size_t)nchan);
  for (int c = 0; c < nchan; ++c) nr_reset_record(hs.data() + (size_t)kNrSpecFloats * (size_t)c);
  const hipError_t e = hipMemcpy(anr, ha.data(), sizeof(float) * ha.size(), hipMemcpyHostToDevice);
  return e != hipSuccess ? e : hipMemcpy(spec, hs.data(), sizeof(float) * hs.size(), hipMemcpyHostToDevice);
}
}  // namespace

// state and tables of the noise-reduction stages, on first use
int ensure_nr(t41rx_ctx *ctx) {
  if (ctx->nr.d_anr) return T41RX_OK;
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
  ctx->nr.d_anr = std::move(anr);
  ctx->nr.d_spec = std::move(spec);
  ctx->nr.d_tab = std::move(tab);
  return T41RX_OK;
}

// Process.cpp:841-866 behind the equalizer
int nr_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  if (sets_staged(ctx)) return nr_sets_run(ctx, n_frames, s);  // parameter sets next to the stages: every channel its own set's values (rx_sets.cpp)
  if (ctx->nr.map_on) return nr_map_run(ctx, n_frames, s);  // the noise-reduction map: every channel its own two values (rx_nrmap.cpp)
  const StageList l = stage_list(ctx, kStageNr);
  if (l.empty()) return T41RX_OK;  // the stage map lists no channel: nothing to launch
  NrArgs n{};
  n.list = l.list;  // (the spectral function and Xanr() of this call: the same list)
  n.nlist = l.n;
  n.aud = ctx->d_aud24.get();
  n.anr = ctx->nr.d_anr.get();
  n.spec = ctx->nr.d_spec.get();
  n.tab_nr = ctx->nr.d_tab.get();
  n.tab = ctx->d_tab.get();
  n.nchan = ctx->nchan;
  n.nframes = n_frames;
  n.nr_option = ctx->params.nrOptionSelect;
  n.notch = ctx->params.ANR_notchOn;
  n.alpha = ctx->params.NR_alpha;
  n.beta = ctx->params.NR_beta;
  n.psi = ctx->params.NR_PSI;
  nr_vad_range(ctx->params.FLoCut, ctx->params.FHiCut, &n.vad_lo, &n.vad_hi);
  return hip_check(launch_nr(n, s), "noise-reduction kernel launch");
}

// its checkpoint section: Xanr()'s rows, then the Kim / spectral records
int nr_check(const t41rx_ctx *c, const int32_t *, const float *anr) {
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
}
int nr_get(const t41rx_ctx *c, void *h, size_t bytes) {
  const size_t ab = sizeof(float) * (size_t)kAnrStRows * (size_t)c->nchan;
  HIP_TRY(hipMemcpy(h, c->nr.d_anr.get(), ab, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(static_cast<char *>(h) + ab, c->nr.d_spec.get(), bytes - ab, hipMemcpyDeviceToHost));
  return T41RX_OK;
}
int nr_put(t41rx_ctx *c, const void *h, size_t bytes) {
  const size_t ab = sizeof(float) * (size_t)kAnrStRows * (size_t)c->nchan;
  HIP_TRY(hipMemcpy(c->nr.d_anr.get(), h, ab, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->nr.d_spec.get(), static_cast<const char *>(h) + ab, bytes - ab, hipMemcpyHostToDevice));
  return T41RX_OK;
}
int nr_reset(t41rx_ctx *c, size_t) {
  return c->nr.d_anr ? hip_check(nr_power_on(c->nr.d_anr.get(), c->nr.d_spec.get(), c->nchan), "noise-reduction reset") : T41RX_OK;
}

// ---- noise blanker
// its carry, both slots (nb.sel stays 0 until the blanker first runs)
int ensure_nb(t41rx_ctx *ctx) {
  return ensure_zeroed(ctx->nb.d_carry, sizeof(float) * 2 * kNbCarryPitch * (size_t)ctx->nchan, "noise-blanker");
}

// Process.cpp:873-876 behind the noise reduction
int nb_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  const StageList l = stage_list(ctx, kStageNb), rest = stage_list(ctx, kStageCount);
  if (l.empty()) return T41RX_OK;  // the stage map lists no channel: nothing to launch, and the slot does not flip
  NbArgs b{};
  b.list = l.list;  // (the launch carries the channels it leaves out from slot sel to slot sel ^ 1: nb_kernel.hip)
  b.nlist = l.n;
  b.rest = rest.list;
  b.nrest = rest.n;
  b.aud = ctx->d_aud24.get();
  b.carry = ctx->nb.d_carry.get();
  b.nchan = ctx->nchan;
  b.nframes = n_frames;
  b.sel = ctx->nb.sel;
  const hipError_t e = launch_nb(b, s);
  if (e != hipSuccess) return hip_fail(e, "noise-blanker kernel launch");
  ctx->nb.sel ^= 1;  // the last frame wrote the other slot
  return T41RX_OK;
}

// its checkpoint section: the current one of the two slots out, slot 0 in
int nb_get(const t41rx_ctx *c, void *h, size_t n) {
  return hip_check(hipMemcpy(h, c->nb.d_carry.get() + (size_t)c->nb.sel * (n / sizeof(float)), n, hipMemcpyDeviceToHost), "hipMemcpy");
}
int nb_put(t41rx_ctx *c, const void *h, size_t n) {
  c->nb.sel = 0;
  return hip_check(hipMemcpy(c->nb.d_carry.get(), h, n, hipMemcpyHostToDevice), "hipMemcpy");
}
int nb_reset(t41rx_ctx *c, size_t n) {  // both slots: last_frame_end is a static, zero at power-on
  c->nb.sel = 0;
  return c->nb.d_carry ? hip_check(hipMemset(c->nb.d_carry.get(), 0, 2 * n), "hipMemset") : T41RX_OK;
}

}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_set_noise_blanker(t41rx_ctx *ctx, int NB_on) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (NB_on != 0 && NB_on != 1) return fail(T41RX_ERR_ARG, "NB_on must be 0 or 1");
  if (NB_on && ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the noise blanker is built for fft_length 512");
  if (NB_on && sets_plain(ctx)) return sets_refuse_stage("the noise blanker");
  ctx->nb.on = NB_on;
  return T41RX_OK;
}
int t41rx_get_noise_blanker(const t41rx_ctx *ctx) { return ctx ? ctx->nb.on : T41RX_ERR_ARG; }

int t41rx_set_receive_eq_bands(t41rx_ctx *ctx, const float *coeffs) {
  if (!ctx || !coeffs) return fail(T41RX_ERR_ARG, "null argument");
  for (int i = 0; i < kEqCoefs; ++i)
    if (!std::isfinite(coeffs[i])) return fail(T41RX_ERR_ARG, "receive-equalizer band table: non-finite coefficient");
  std::memcpy(ctx->eq.coef, coeffs, sizeof(ctx->eq.coef));  // (passed by value to every launch: the next call uses it)
  ctx->eq.have_bands = true;
  return T41RX_OK;
}

int t41rx_set_receive_eq(t41rx_ctx *ctx, int receiveEQFlag, const int32_t *equalizerRec) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (receiveEQFlag != 0 && receiveEQFlag != 1) return fail(T41RX_ERR_ARG, "receiveEQFlag must be 0 or 1");
  if (receiveEQFlag && ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "the receive equalizer is built for fft_length 512");
  if (receiveEQFlag && !ctx->eq.have_bands)
    return fail(T41RX_ERR_ARG, "receive equalizer: no band table loaded (t41rx_set_receive_eq_bands)");
  if (receiveEQFlag && sets_plain(ctx)) return sets_refuse_stage("the receive equalizer");
  if (equalizerRec) std::memcpy(ctx->eq.levels, equalizerRec, sizeof(ctx->eq.levels));
  ctx->eq.on = receiveEQFlag;
  return T41RX_OK;
}

int t41rx_get_receive_eq(const t41rx_ctx *ctx, int32_t *equalizerRec_out) {
  if (!ctx) return T41RX_ERR_ARG;
  if (equalizerRec_out) std::memcpy(equalizerRec_out, ctx->eq.levels, sizeof(ctx->eq.levels));
  return ctx->eq.on;
}

}  // extern "C"
