// t41_sdr_amd/csrc/rx_sets.cpp -- parameter sets (t41rx_set_param_sets / _get_param_sets / _param_sets_compatible): one
// t41rx_params per group of channels of a context.  The context's own parameters are set 0; the extra sets 1..K are
// designed here exactly as set 0 is (design_blob, fill_dev_coef, fill_tab512, gains_of) and uploaded as arrays [K + 1]
// the set forms of rx512_kernel index with set_of_channel[ch].  The rule that decides which sets may share a context is
// compatible() below, once.
#include <cstring>
#include <string>
#include <vector>

#include "rx_ctx.hpp"

using namespace t41;

namespace {

const char *family_name(int mode) {
  return mode == T41RX_DEMOD_AM ? "AM" : mode == T41RX_DEMOD_NFM ? "NFM" : mode == T41RX_DEMOD_SAM ? "SAM" : "USB/LSB";
}

bool plain_of(const t41rx_params &p) {
  std::vector<float> blob(blob_floats(p.fft_length));
  if (design_blob(p, blob.data(), blob.size() * sizeof(float)) != T41RX_OK) return false;  // (the callers have validated p)
  SetGains g;
  return gains_of(blob_view(blob.data()).scalars, g);
}

// The rule: the plan (rx_plan.hpp) names the same rx512_kernel instantiation for both, and both name the same stages.
// The clauses say which difference it is; the last check asks plan_call() itself, so the rule cannot drift from what is
// launched.  `who` opens the refusal ("set 2 against set 0: ").
// flags: T41RX_SETS_STAGES drops the one clause on nrOptionSelect / ANR_notchOn -- each channel then takes its own set's
// two values (rx_stagesets.hpp) -- and keeps every other.
int compatible(const t41rx_params &a, const t41rx_params &b, const std::string &who, uint32_t flags) {
  auto no = [&](const std::string &why) { return fail(T41RX_ERR_UNSUPPORTED, "parameter sets: " + who + why); };
  if (a.fft_length != b.fft_length)
    return no("fft_length differs (" + std::to_string(a.fft_length) + " and " + std::to_string(b.fft_length) + ")");
  if (a.fft_length != 512)
    return no("fft_length " + std::to_string(a.fft_length) + ": the long-FFT pipeline carries one parameter set; sets are built for fft_length 512");
  const bool staged = (flags & T41RX_SETS_STAGES) != 0;
  CallFacts fa = params_facts(a, plain_of(a)), fb = params_facts(b, plain_of(b));
  if (staged) fa.nr = fb.nr = false;  // (which stages a call runs is the context's matter then, not the pair's)
  if (fa.family != fb.family)  // (USB and LSB are one kernel)
    return no(std::string("the demodulators differ (") + family_name(a.mode) + " and " + family_name(b.mode) + "): one kernel runs all the channels of a context");
  if ((a.AGCMode != 0) != (b.AGCMode != 0)) return no("the AGC is off in one and on in the other (AGCMode 0 against 1..4)");
  if (a.nfm_demod != b.nfm_demod) return no("nfm_demod differs");
  if (a.xmtMode != b.xmtMode) return no("xmtMode differs");
  if (!staged && (a.nrOptionSelect != 0 || b.nrOptionSelect != 0 || a.ANR_notchOn != 0 || b.ANR_notchOn != 0))
    return no("noise reduction / notch (nrOptionSelect, ANR_notchOn) split the fused chain and read one parameter set on the host: both must be 0");
  if (fa.plain_gains != fb.plain_gains)
    return no("the first stage's gains are unit gains in one (RFgain 1, IQAmpCorrectionFactor 1, IQPhaseCorrectionFactor 0) and general in "
              "the other: two kernels");
  if (!(plan_call(fa).form == plan_call(fb).form)) return no("the two take different kernels");
  return T41RX_OK;
}

// the arrays the set kernels read, entry 0 from the context's own blob, entry i from blobs[i - 1]
int upload_arrays(const t41rx_ctx *ctx, const std::vector<std::vector<float>> &blobs, DevCoef *d_coef, float2 *d_tab, SetGains *d_gain) {
  const size_t n = blobs.size() + 1;
  std::vector<DevCoef> coef(n);
  std::vector<SetGains> gain(n);
  std::vector<float2> tabs, one;
  tabs.reserve(n * (size_t)kTabEntries512);
  for (size_t i = 0; i < n; ++i) {
    // (blob_view() takes a mutable pointer; nothing is written through it)
    const BlobView v = blob_view(const_cast<float *>(i == 0 ? ctx->blob.data() : blobs[i - 1].data()));
    fill_dev_coef(v, coef[i]);
    fill_tab512(v, 512, one);
    tabs.insert(tabs.end(), one.begin(), one.end());
    (void)gains_of(v.scalars, gain[i]);
  }
  HIP_TRY(hipMemcpy(d_coef, coef.data(), sizeof(DevCoef) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_tab, tabs.data(), sizeof(float2) * tabs.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_gain, gain.data(), sizeof(SetGains) * n, hipMemcpyHostToDevice));
  return T41RX_OK;
}

// what cw_back_sets_kernel reads of every set (cw_kernels.hpp): what cw_filter_run() passes by value of set 0's blob
int upload_cw_back(const t41rx_ctx *ctx, const std::vector<std::vector<float>> &blobs, CwSetBack *d_cw_back) {
  std::vector<CwSetBack> h(blobs.size() + 1);
  for (size_t i = 0; i < h.size(); ++i) {
    const BlobView v = blob_view(const_cast<float *>(i == 0 ? ctx->blob.data() : blobs[i - 1].data()));
    std::memset(&h[i], 0, sizeof(CwSetBack));
    h[i].scale = v.scalars[kScOutScale];
    std::memcpy(h[i].int1, v.int1, sizeof(h[i].int1));
    std::memcpy(h[i].int2, v.int2, sizeof(h[i].int2));
  }
  HIP_TRY(hipMemcpy(d_cw_back, h.data(), sizeof(CwSetBack) * h.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}

// what the noise reduction reads of a parameter set
StageSetNr stage_nr_of(const t41rx_params &p) {
  StageSetNr s;
  s.kind = p.nrOptionSelect;
  s.notch = p.ANR_notchOn;
  s.alpha = p.NR_alpha;
  s.beta = p.NR_beta;
  s.psi = p.NR_PSI;
  int lo = 0, hi = 0;
  nr_vad_range(p.FLoCut, p.FHiCut, &lo, &hi);
  s.vad_lo = lo;
  s.vad_hi = hi;
  t41rx_params q = p;
  q.nrOptionSelect = 2;  // (the spectral function's array-bounds check of params_valid(), design.cpp)
  s.spectral_ok = params_valid(q, nullptr);
  return s;
}

// the device copies of a StageSetsNr: the lists as the noise-reduction map's are laid out, and the rows
int upload_stage_nr(const StageSetsNr &st, int nchan, int32_t *d_nr_map, NrSetRow *d_nr_rows) {
  const NrMapLayout lay = nr_map_layout(nchan);
  std::vector<int32_t> w(lay.words, 0);
  const NrMapLists &l = st.lists;
  for (size_t i = 0; i < l.spec.size(); ++i) {
    w[lay.spec + i] = l.spec[i];
    w[lay.spec_kind + i] = l.spec_kind[i];
  }
  for (size_t i = 0; i < l.anr.size(); ++i) w[lay.anr + i] = l.anr[i];
  for (size_t i = 0; i < l.rows.size(); ++i) {
    w[lay.rows + 4 * i + 0] = l.rows[i].offset;
    w[lay.rows + 4 * i + 1] = l.rows[i].live;
    w[lay.rows + 4 * i + 2] = l.rows[i].cls;
  }
  HIP_TRY(hipMemcpy(d_nr_map, w.data(), sizeof(int32_t) * w.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_nr_rows, st.rows.data(), sizeof(NrSetRow) * st.rows.size(), hipMemcpyHostToDevice));
  return T41RX_OK;
}

}  // namespace

int t41::stage_sets_build(const t41rx_ctx *ctx, const t41rx_params &set0, const t41rx_params *extra, int n_extra, const int32_t *set_of,
                          const int32_t *kind_map, const int32_t *notch_map, StageSetsNr &out) {
  std::vector<StageSetNr> nr((size_t)n_extra + 1);
  nr[0] = stage_nr_of(set0);
  for (int i = 0; i < n_extra; ++i) nr[(size_t)i + 1] = stage_nr_of(extra[i]);
  const StageSetsVerdict v = build_stage_sets(nr.data(), n_extra + 1, set_of, ctx->nchan, ctx->nchan, kind_map, notch_map,
                                              ctx->stages.on ? ctx->stages.map.data() : nullptr, out);
  if (v) return T41RX_OK;
  if (v.fault == StageSetsFault::spectral) {
    t41rx_params q = v.set == 0 ? set0 : extra[v.set - 1];
    q.nrOptionSelect = 2;
    const char *why = nullptr;
    (void)params_valid(q, &why);  // (params_valid()'s text, as t41rx_set_params() gives it for that set)
    return fail(T41RX_ERR_ARG, "parameter sets: channel " + std::to_string(v.channel) + " runs the spectral noise reduction on set " +
                                   std::to_string(v.set) + ": " + (why ? why : "nrOptionSelect = 2: the pass band fails the spectral function's check"));
  }
  // (not reached: the setters have checked the table, the map and the structs)
  return fail(T41RX_ERR_ARG, "parameter sets: channel " + std::to_string(v.channel) + ": the noise-reduction values of the sets and the map do not build");
}

// the sets, the noise-reduction map, the stage map or set 0 changed (behind the setter's device synchronisation)
int t41::stage_sets_refresh(t41rx_ctx *ctx) {
  if (!sets_staged(ctx)) return T41RX_OK;
  StageSetsNr fresh;
  const int rc = stage_sets_build(ctx, ctx->params, ctx->sets.params.data(), (int)ctx->sets.params.size(), ctx->sets.set_of.data(),
                                  ctx->nr.map_on ? ctx->nr.kind_map.data() : nullptr, ctx->nr.map_on ? ctx->nr.notch_map.data() : nullptr, fresh);
  if (rc != T41RX_OK) return rc;  // (not reached: every setter that can break the check has made it before it changed anything)
  if (const int up = upload_stage_nr(fresh, ctx->nchan, ctx->sets.d_nr_map.get(), ctx->sets.d_nr_rows.get())) return up;
  ctx->sets.stage = std::move(fresh);
  return T41RX_OK;
}

// Process.cpp:841-866 with the channel's own set's values: nr_map_run()'s two launches over the effective lists, the
// spectral one in its form that reads NR_alpha, NR_beta, NR_PSI and the VAD range from the channel's row
int t41::nr_sets_run(t41rx_ctx *ctx, int n_frames, hipStream_t s) {
  const NrMapLists &l = ctx->sets.stage.lists;
  if (l.spec.empty() && l.rows.empty()) return T41RX_OK;  // nobody runs anything: nothing to launch
  const NrMapLayout lay = nr_map_layout(ctx->nchan);
  const int32_t *d = ctx->sets.d_nr_map.get();
  NrSetsArgs n{};
  n.aud = ctx->d_aud24.get();
  n.anr = ctx->nr.d_anr.get();
  n.spec = ctx->nr.d_spec.get();
  n.tab_nr = ctx->nr.d_tab.get();
  n.tab = ctx->d_tab.get();  // (the twiddles: the same in every set's table)
  n.nchan = ctx->nchan;
  n.nframes = n_frames;
  n.list = d + lay.anr;
  n.nlist = (int)l.anr.size();
  n.spec_list = d + lay.spec;
  n.spec_kind = d + lay.spec_kind;
  n.nspec = (int)l.spec.size();
  n.rows = reinterpret_cast<const int4 *>(d + lay.rows);
  n.nrows = (int)l.rows.size();
  n.set_rows = ctx->sets.d_nr_rows.get();
  return hip_check(launch_nr_sets(n, s), "noise-reduction kernel launch (parameter sets)");
}

// t41rx_set_params() / t41rx_set_coeffs() with sets loaded: the new set 0 against every loaded set
int t41::sets_check_set0(const t41rx_ctx *ctx, const t41rx_params &p) {
  for (size_t i = 0; i < ctx->sets.params.size(); ++i) {
    const int rc = compatible(p, ctx->sets.params[i], "the new set 0 against set " + std::to_string(i + 1) + ": ", ctx->sets.flags);
    if (rc != T41RX_OK) return rc;
  }
  if (!sets_staged(ctx)) return T41RX_OK;
  StageSetsNr probe;  // the spectral check of set 0's channels against the new pass band
  return stage_sets_build(ctx, p, ctx->sets.params.data(), (int)ctx->sets.params.size(), ctx->sets.set_of.data(),
                          ctx->nr.map_on ? ctx->nr.kind_map.data() : nullptr, ctx->nr.map_on ? ctx->nr.notch_map.data() : nullptr, probe);
}

// set 0 has changed: the set arrays again (the extra sets' entries are rewritten with what they held)
int t41::sets_upload(t41rx_ctx *ctx) {
  if (const int rc = upload_arrays(ctx, ctx->sets.blobs, ctx->sets.d_coef.get(), ctx->sets.d_tab.get(), ctx->sets.d_gain.get())) return rc;
  if (!sets_staged(ctx)) return T41RX_OK;
  if (const int rc = upload_cw_back(ctx, ctx->sets.blobs, ctx->sets.d_cw_back.get())) return rc;
  return stage_sets_refresh(ctx);  // (set 0's noise-reduction values and pass band)
}

extern "C" {

int t41rx_param_sets_compatible(const t41rx_params *a, const t41rx_params *b) { return t41rx_param_sets_compatible_ex(a, b, 0); }

int t41rx_param_sets_compatible_ex(const t41rx_params *a, const t41rx_params *b, int32_t flag_bits) {
  if (!a || !b) return fail(T41RX_ERR_ARG, "null argument");
  const uint32_t flags = (uint32_t)flag_bits;
  if (flags & ~T41RX_SETS_STAGES) return fail(T41RX_ERR_ARG, "parameter sets: unknown flag bits (" + std::to_string(flags & ~T41RX_SETS_STAGES) + "); T41RX_SETS_STAGES is the one flag");
  const char *why = nullptr;
  if (!params_valid(*a, &why)) return fail(T41RX_ERR_ARG, std::string("parameter sets: the first struct is invalid: ") + (why ? why : "bad params"));
  if (!params_valid(*b, &why)) return fail(T41RX_ERR_ARG, std::string("parameter sets: the second struct is invalid: ") + (why ? why : "bad params"));
  return compatible(*a, *b, "", flags);
}

int t41rx_set_param_sets(t41rx_ctx *ctx, const t41rx_params *sets, int n_sets, const int32_t *set_of_channel, int n) {
  return t41rx_set_param_sets_ex(ctx, sets, n_sets, set_of_channel, n, 0);
}

int t41rx_get_param_sets_flags(const t41rx_ctx *ctx) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  return sets_loaded(ctx) ? (int)ctx->sets.flags : 0;
}

int t41rx_set_param_sets_ex(t41rx_ctx *ctx, const t41rx_params *sets, int n_sets, const int32_t *set_of_channel, int n, int32_t flag_bits) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const uint32_t flags = (uint32_t)flag_bits;
  if (flags & ~T41RX_SETS_STAGES) return fail(T41RX_ERR_ARG, "parameter sets: unknown flag bits (" + std::to_string(flags & ~T41RX_SETS_STAGES) + "); T41RX_SETS_STAGES is the one flag");
  const bool staged = (flags & T41RX_SETS_STAGES) != 0;
  const std::string counts = " (n_channels " + std::to_string(ctx->nchan) + ", n_sets " + std::to_string(n_sets) + ")";
  if (n_sets == 0) {
    if (sets || set_of_channel) return fail(T41RX_ERR_ARG, "parameter sets: n_sets 0 removes the sets and takes two null pointers" + counts);
    if (!sets_loaded(ctx)) return T41RX_OK;
    DeviceGuard g(ctx->device);
    if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(hipDeviceSynchronize());  // (calls in flight were launched with the sets they found)
    ctx->sets = ParamSets{};
    if (const int rc = pan_map_refresh(ctx)) return rc;  // (a panadapter map: every listed channel's gains are set 0's again)
    return upload_nco(ctx);  // every channel's side tone is set 0's again
  }
  // everything is checked here, on the host, before anything changes: the kernels index the set arrays with these entries unchecked
  if (n_sets < 0 || n_sets > T41RX_MAX_PARAM_SETS - 1)
    return fail(T41RX_ERR_ARG, "parameter sets: n_sets must lie in [0, " + std::to_string(T41RX_MAX_PARAM_SETS - 1) + "]" + counts);
  if (!sets || !set_of_channel) return fail(T41RX_ERR_ARG, "parameter sets: null argument" + counts);
  if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "parameter sets: n (" + std::to_string(n) + ") must equal n_channels" + counts);
  for (int i = 0; i < n; ++i)
    if (set_of_channel[i] < 0 || set_of_channel[i] > n_sets)
      return fail(T41RX_ERR_ARG, "parameter sets: channel " + std::to_string(i) + " names set " + std::to_string(set_of_channel[i]) +
                                     ", outside [0, n_sets]" + counts);
  for (int i = 0; i < n_sets; ++i) {
    const char *why = nullptr;
    if (!params_valid(sets[i], &why))
      return fail(T41RX_ERR_ARG, "parameter sets: set " + std::to_string(i + 1) + " is invalid: " + (why ? why : "bad params"));
  }
  if (ctx->params.fft_length != 512)
    return fail(T41RX_ERR_UNSUPPORTED, "parameter sets: fft_length " + std::to_string(ctx->params.fft_length) +
                                           ": the long-FFT pipeline carries one parameter set; sets are built for fft_length 512");
  if (!staged)
    if (const char *stage = split_stage_on(ctx)) return sets_refuse_stage(stage);
  for (int i = 0; i < n_sets; ++i) {
    const int rc = compatible(ctx->params, sets[i], "set " + std::to_string(i + 1) + " against set 0: ", flags);
    if (rc != T41RX_OK) return rc;
  }
  ParamSets fresh;
  fresh.flags = flags;
  if (staged) {  // every channel's effective kind and notch, its row, the lists; the spectral check against the channel's own set
    const int rc = stage_sets_build(ctx, ctx->params, sets, n_sets, set_of_channel, ctx->nr.map_on ? ctx->nr.kind_map.data() : nullptr,
                                    ctx->nr.map_on ? ctx->nr.notch_map.data() : nullptr, fresh.stage);
    if (rc != T41RX_OK) return rc;
  }
  fresh.params.assign(sets, sets + n_sets);
  fresh.blobs.resize((size_t)n_sets);
  for (int i = 0; i < n_sets; ++i) {
    fresh.blobs[(size_t)i].assign(blob_floats(512), 0.0f);
    const int rc = design_blob(sets[i], fresh.blobs[(size_t)i].data(), fresh.blobs[(size_t)i].size() * sizeof(float));
    if (rc != T41RX_OK) return fail(rc, "parameter sets: coefficient design of set " + std::to_string(i + 1) + " failed");
    if (sets[i].AGCMode != 0 && (int)blob_view(fresh.blobs[(size_t)i].data()).agc[kAgcAttackBuffsize] != kAgcDelay)
      return fail(T41RX_ERR_UNSUPPORTED, "parameter sets: set " + std::to_string(i + 1) + " asks for an AGC look-ahead the kernel is not built for");
  }
  fresh.set_of.assign(set_of_channel, set_of_channel + n);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  // fresh buffers, filled before the context sees them: a failure leaves the previous sets whole
  const size_t k1 = (size_t)n_sets + 1;
  HIP_TRY(dev_alloc(fresh.d_coef, sizeof(DevCoef) * k1));
  HIP_TRY(dev_alloc(fresh.d_tab, sizeof(float2) * k1 * (size_t)kTabEntries512));
  HIP_TRY(dev_alloc(fresh.d_gain, sizeof(SetGains) * k1));
  HIP_TRY(dev_alloc(fresh.d_set_of, sizeof(int32_t) * (size_t)n));
  int rc = upload_arrays(ctx, fresh.blobs, fresh.d_coef.get(), fresh.d_tab.get(), fresh.d_gain.get());
  if (rc != T41RX_OK) return rc;
  HIP_TRY(hipMemcpy(fresh.d_set_of.get(), set_of_channel, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
  if (staged) {
    HIP_TRY(dev_alloc(fresh.d_nr_map, sizeof(int32_t) * nr_map_layout(n).words));
    HIP_TRY(dev_alloc(fresh.d_nr_rows, sizeof(NrSetRow) * (size_t)n));
    HIP_TRY(dev_alloc(fresh.d_cw_back, sizeof(CwSetBack) * k1));
    if ((rc = upload_stage_nr(fresh.stage, n, fresh.d_nr_map.get(), fresh.d_nr_rows.get())) != T41RX_OK) return rc;
    if ((rc = upload_cw_back(ctx, fresh.blobs, fresh.d_cw_back.get())) != T41RX_OK) return rc;
  }
  ctx->sets = std::move(fresh);
  if ((rc = pan_map_refresh(ctx)) != T41RX_OK) return rc;  // (a panadapter map: the listed channels' gains follow their own sets)
  return upload_nco(ctx);  // the side tone follows the channel's own set
}

int t41rx_get_param_sets(const t41rx_ctx *ctx, t41rx_params *sets_out, int cap, int32_t *set_of_channel_out, int n) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const int k = (int)ctx->sets.params.size();
  if (k > 0 && sets_out) {
    if (cap < k) return fail(T41RX_ERR_ARG, "parameter sets: cap (" + std::to_string(cap) + ") is smaller than the number of sets (" + std::to_string(k) + ")");
    std::memcpy(sets_out, ctx->sets.params.data(), sizeof(t41rx_params) * (size_t)k);
  }
  if (k > 0 && set_of_channel_out) {
    if (n != ctx->nchan) return fail(T41RX_ERR_ARG, "parameter sets: n (" + std::to_string(n) + ") must equal n_channels (" + std::to_string(ctx->nchan) + ")");
    std::memcpy(set_of_channel_out, ctx->sets.set_of.data(), sizeof(int32_t) * (size_t)n);
  }
  return k;
}

}  // extern "C"
