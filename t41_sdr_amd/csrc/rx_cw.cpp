// t41_sdr_amd/csrc/rx_cw.cpp -- host side of the CW receive stages (cw_kernel.hip): the narrow audio filter with its back
// end, the tone detector and the Morse decoder behind it.  Their memories on first use, the launches of a process call,
// the decoder's checkpoint checks, and the setters.
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {

int upload_channel_mask(const t41rx_ctx *ctx, const uint8_t *channels, DevBuf<uint8_t> &mask) {
  if (!channels) return T41RX_OK;
  HIP_TRY(dev_alloc(mask, (size_t)ctx->nchan));
  HIP_TRY(hipMemcpy(mask.get(), channels, (size_t)ctx->nchan, hipMemcpyHostToDevice));
  return T41RX_OK;
}

int set_stage_clock(StageClock &clock, const char *what, int32_t t0_ms, int32_t num, int32_t den) {
  if (num < 0 || den <= 0) return fail(T41RX_ERR_ARG, std::string(what) + " clock: num must be >= 0 and den > 0");
  clock = {t0_ms, num, den};  // (passed by value to every launch: the next call uses it; the frame counters stay)
  return T41RX_OK;
}

// the CW stages' memories: five filter states, the decode FIR's history, the detector's carried words (zeroed statics)
int ensure_cw(t41rx_ctx *ctx) {
  return ensure_zeroed(ctx->cw.d_state, sizeof(float) * kCwStateFloats * (size_t)ctx->nchan, "CW-receive");
}

namespace {
// the decoder's words at power-on: what ResetHistograms() leaves, currentDashJump = 128, everything else zero
hipError_t cw_decode_upload_power_on(int32_t *d, int nchan) {
  std::vector<int32_t> h((size_t)kCwDecWords * (size_t)nchan);
  for (int c = 0; c < nchan; ++c) cw_decode_power_on(h.data() + (size_t)kCwDecWords * (size_t)c);
  return hipMemcpy(d, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice);
}
}  // namespace

int ensure_cw_decode(t41rx_ctx *ctx) {
  if (ctx->cw.d_dec) return T41RX_OK;
  DevBuf<int32_t> d;
  if (dev_alloc(d, sizeof(int32_t) * kCwDecWords * (size_t)ctx->nchan) != hipSuccess) return fail(T41RX_ERR_NOMEM, "CW-decoder state allocation failed");
  if (cw_decode_upload_power_on(d.get(), ctx->nchan) != hipSuccess) return fail(T41RX_ERR_HIP, "CW-decoder state upload failed");
  ctx->cw.d_dec = std::move(d);
  return T41RX_OK;
}
int cw_decode_reset(t41rx_ctx *c, size_t) {
  return c->cw.d_dec ? hip_check(cw_decode_upload_power_on(c->cw.d_dec.get(), c->nchan), "CW-decoder reset") : T41RX_OK;
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

// The library carries one audio stream where the firmware has float_buffer_L and float_buffer_R; the detector reads both.
// The stage that leaves L different from R in front of it, or null: the equalizer writes L only (Filter.cpp:151-164),
// Kim1_NR() and SpectralNoiseReduction() end with R = L (Noise.cpp:307-308, 636-637) but x30 behind Kim scales L only
// (Process.cpp:846), Xanr() writes R only and x1.5 behind it scales L only (Noise.cpp:345-347, Process.cpp:855); the
// notch and the blanker end in arm_copy_f32(R, L) (Process.cpp:865, 875), which joins them again.
namespace {
const char *cw_split_stage_of(const t41rx_ctx *ctx, int nrOptionSelect, int ANR_notchOn) {
  if (ANR_notchOn != 0 || ctx->nb.on) return nullptr;
  if (nrOptionSelect == 1) return "Kim noise reduction (nrOptionSelect 1)";
  if (nrOptionSelect == 3) return "LMS noise reduction (nrOptionSelect 3)";
  if (ctx->eq.on && nrOptionSelect == 0) return "receive equalizer";
  return nullptr;
}
}  // namespace
// With a noise-reduction map (t41rx_set_nr_map) the rule is each channel's, with the channel's own two values in place of
// the context's: the first channel that trips it, in *channel.
// With parameter sets loaded next to the stages (T41RX_SETS_STAGES) it is each channel's too, with the channel's effective
// values (rx_stagesets.hpp): the map's, or without a map its own set's, and then *set says which.
const char *cw_split_stage(const t41rx_ctx *ctx, int *channel, int *set) {
  *channel = -1;
  *set = -1;
  if (sets_staged(ctx)) {
    for (int c = 0; c < ctx->nchan; ++c)
      if (const char *stage = cw_split_stage_of(ctx, ctx->sets.stage.kind[(size_t)c], ctx->sets.stage.notch[(size_t)c])) {
        *channel = c;
        if (!ctx->nr.map_on) *set = ctx->sets.set_of[(size_t)c];
        return stage;
      }
    return nullptr;
  }
  if (!ctx->nr.map_on) return cw_split_stage_of(ctx, ctx->params.nrOptionSelect, ctx->params.ANR_notchOn);
  for (int c = 0; c < ctx->nchan; ++c)
    if (const char *stage = cw_split_stage_of(ctx, ctx->nr.kind_map[(size_t)c], ctx->nr.notch_map[(size_t)c])) {
      *channel = c;
      return stage;
    }
  return nullptr;
}

// Process.cpp:878-879 behind the blanker: DoCWReceiveProcessing() reads the audio, its results go to the caller's buffer
int cw_detect_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  const StageList l = stage_list(ctx, kStageCwDetect);
  if (l.empty()) return T41RX_OK;  // the stage map lists no channel: nothing to launch
  CwDetectArgs d{};
  d.list = l.list;
  d.nlist = l.n;
  d.aud = ctx->d_aud24.get();
  d.state = ctx->cw.d_state.get();
  d.out = ctx->cw.out;
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
  std::memcpy(d.fir, ctx->cw.fir, sizeof(d.fir));
  return hip_check(launch_cw_detect(d, s), "CW detector kernel launch");
}

// CWProcessing.cpp:365-371 behind it: the threshold on the detector's combinedCoeff and DoCWDecoding()
int cw_decode_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  const StageList l = stage_list(ctx, kStageCwDecode);  // (a subset of the detector's: the setter's rule)
  if (l.empty()) return T41RX_OK;  // the stage map lists no channel: nothing to launch
  CwDecodeArgs d{};
  d.list = l.list;
  d.nlist = l.n;
  d.cw = ctx->cw.out;
  d.state = ctx->cw.d_dec.get();
  d.text = ctx->cw.text;
  d.nchan = ctx->nchan;
  d.nframes = n_frames;
  d.t0 = ctx->cw.clock.t0;
  d.num = ctx->cw.clock.num;
  d.den = ctx->cw.clock.den;
  std::memcpy(d.tree, ctx->cw.tree, sizeof(d.tree));
  return hip_check(launch_cw_decode(d, s), "CW decoder kernel launch");
}

int cw_filter_run(t41rx_ctx *ctx, const CallPlan &plan, const RxArgs &a, int n_frames, hipStream_t s) {
  // Process.cpp:882-912: the narrow filter CWFilterIndex selects, on its own memory
  hipError_t e = hipSuccess;
  const int32_t *map = ctx->cw.d_map.get();
  const size_t pitch = cw_map_pitch(ctx->nchan);
  if (ctx->cw.map_on) {
    // the filter map (t41rx_set_cw_filter_map): the filtered channels' list, each with its own index (the plan sends a
    // map that filters nobody past this function: the list is not empty)
    CwFilterMapArgs f{};
    f.aud = ctx->d_aud24.get();
    f.state = ctx->cw.d_state.get();
    f.list = map + (size_t)kCwMapList * pitch;
    f.index_of = map + (size_t)kCwMapIndex * pitch;
    f.nlist = (int)ctx->cw.lists.filtered.size();
    f.nchan = ctx->nchan;
    f.nsamp = n_frames * 256;
    std::memcpy(f.coef, ctx->cw.coef, sizeof(f.coef));
    e = launch_cw_filter_map(f, s);
  } else {
    CwFilterArgs f{};
    f.aud = ctx->d_aud24.get();
    f.state = ctx->cw.d_state.get();
    f.nchan = ctx->nchan;
    f.nsamp = n_frames * 256;
    f.index = ctx->cw.filter;
    std::memcpy(f.coef, ctx->cw.coef + kCwFilterCoefs * ctx->cw.filter, sizeof(f.coef));
    e = launch_cw_filter(f, s);
  }
  if (e != hipSuccess) return hip_fail(e, "CW filter kernel launch");
  // 24 kS/s (t41rx_set_audio_rate): the filtered audio is the result -- volume and stores, no interpolator
  if (plan.back == Back::cw_24k) return aud24_finish_run(ctx, a, n_frames, s);
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
  b.out_map = a.out_map;  // (the output map: a's strides then place its n_rows rows)
  // both classes in one call: this kernel for the filtered channels, the unfiltered ones muted, each at its own row
  if (plan.back == Back::cw_mixed) b.out_map = map + (size_t)kCwMapRowsFiltered * pitch;
  b.scale = v.scalars[kScOutScale];
  std::memcpy(b.int1, v.int1, sizeof(b.int1));
  std::memcpy(b.int2, v.int2, sizeof(b.int2));
  if (sets_staged(ctx)) {
    // parameter sets next to the stages: the volume factor and the taps of the channel's own set (rx_sets.cpp makes the table)
    CwBackSetsArgs bs{};
    static_cast<CwBackArgs &>(bs) = b;
    bs.set_of = ctx->sets.d_set_of.get();
    bs.sets = ctx->sets.d_cw_back.get();
    e = launch_cw_back_sets(bs, s);
  } else {
    e = launch_cw_back(b, s);
  }
  if (e != hipSuccess) return hip_fail(e, "CW interpolator kernel launch");
  if (plan.back == Back::cw_mixed) {
    // ... and the fused back kernel for the unfiltered ones, as a call without the filter ends (launch_chain: back512)
    RxArgs r = a;
    r.aud_out = nullptr;
    r.out_map = map + (size_t)kCwMapRowsPlain * pitch;
    e = launch_back512(r, s);
    if (e != hipSuccess) return hip_fail(e, "interpolator kernel launch");
  }
  return T41RX_OK;
}

}  // namespace t41

using namespace t41;

extern "C" {

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
    std::memcpy(ctx->cw.coef, audio_filters, sizeof(ctx->cw.coef));
    ctx->cw.have_filters = true;
  }
  if (decode_fir) {
    std::memcpy(ctx->cw.fir, decode_fir, sizeof(ctx->cw.fir));
    ctx->cw.have_fir = true;
  }
  return T41RX_OK;
}

int t41rx_set_cw_filter(t41rx_ctx *ctx, int CWFilterIndex) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (CWFilterIndex < 0 || CWFilterIndex > kCwFilters) return fail(T41RX_ERR_ARG, "CWFilterIndex must be 0 .. 4, or 5 (off)");
  if (CWFilterIndex != kCwFilters) {
    if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the CW audio filters are built for fft_length 512");
    if (!ctx->cw.have_filters) return fail(T41RX_ERR_ARG, "CW audio filter: no filter tables loaded (t41rx_set_cw_tables)");
    if (sets_plain(ctx)) return sets_refuse_stage("the CW audio filter");
  }
  ctx->cw.filter = CWFilterIndex;
  return T41RX_OK;
}
int t41rx_get_cw_filter(const t41rx_ctx *ctx) { return ctx ? ctx->cw.filter : T41RX_ERR_ARG; }

int t41rx_set_cw_detector(t41rx_ctx *ctx, int decoderFlag, float *d_cw, int max_frames) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (decoderFlag != 0 && decoderFlag != 1) return fail(T41RX_ERR_ARG, "decoderFlag must be 0 or 1");
  if (decoderFlag) {
    if (ctx->params.fft_length != 512) return fail(T41RX_ERR_UNSUPPORTED, "the CW detector is built for fft_length 512");
    if (!d_cw) return fail(T41RX_ERR_ARG, "CW detector: no result buffer (d_cw is NULL)");
    if (reinterpret_cast<uintptr_t>(d_cw) & 3u) return fail(T41RX_ERR_ARG, "unaligned pointer");
    if (max_frames <= 0) return fail(T41RX_ERR_ARG, "max_frames must be > 0");
    if (!ctx->cw.have_fir) return fail(T41RX_ERR_ARG, "CW detector: no decode FIR loaded (t41rx_set_cw_tables)");
    if (sets_plain(ctx)) return sets_refuse_stage("the CW detector");
  }
  ctx->cw.det = decoderFlag;
  ctx->cw.out = decoderFlag ? d_cw : nullptr;
  ctx->cw.frames = decoderFlag ? max_frames : 0;
  return T41RX_OK;
}
int t41rx_get_cw_detector(const t41rx_ctx *ctx) { return ctx ? ctx->cw.det : T41RX_ERR_ARG; }

int t41rx_set_cw_decode_tree(t41rx_ctx *ctx, const uint8_t *tree, int n) {
  if (!ctx || !tree) return fail(T41RX_ERR_ARG, "null argument");
  if (n != kCwTreeChars) return fail(T41RX_ERR_ARG, "CW decode tree: n must be 129 (bigMorseCodeTree)");
  std::memcpy(ctx->cw.tree, tree, (size_t)kCwTreeChars);  // (passed by value to every launch: the next call uses it)
  ctx->cw.have_tree = true;
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
    if (!ctx->cw.have_tree) return fail(T41RX_ERR_ARG, "CW decoder: no decode tree loaded (t41rx_set_cw_decode_tree)");
    if (sets_plain(ctx)) return sets_refuse_stage("the CW decoder");
  }
  ctx->cw.dec = on;
  ctx->cw.text = on ? d_text : nullptr;
  ctx->cw.text_frames = on ? max_frames : 0;
  return T41RX_OK;
}
int t41rx_get_cw_decoder(const t41rx_ctx *ctx) { return ctx ? ctx->cw.dec : T41RX_ERR_ARG; }

int t41rx_set_cw_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  return set_stage_clock(ctx->cw.clock, "CW", t0_ms, num, den);
}

int t41rx_reset_cw_histograms(t41rx_ctx *ctx, const uint8_t *channels, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (channels && n != ctx->nchan) return fail(T41RX_ERR_ARG, "n must equal n_channels");
  if (!ctx->cw.d_dec) return T41RX_OK;  // the decoder has not run: its words are the power-on ones, which are ResetHistograms()'s
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  DevBuf<uint8_t> mask;
  if (const int rc = upload_channel_mask(ctx, channels, mask)) return rc;
  HIP_TRY(launch_cw_decode_reset(ctx->cw.d_dec.get(), mask.get(), ctx->nchan, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  return T41RX_OK;
}

}  // extern "C"
