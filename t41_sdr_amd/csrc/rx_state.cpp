// t41_sdr_amd/csrc/rx_state.cpp -- checkpoints and reset of a receive context (t41rx_get_state / t41rx_set_state /
// t41rx_reset): header, the path's records, then the sections header word 5 names -- one table of them, in bit order,
// whose rows name the functions each stage exports (rx_ctx.hpp).
#include <cmath>
#include <cstring>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {
namespace {

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
  // a section that is one device buffer names it; get / put are then one hipMemcpy of it and reset one hipMemset to
  // zero, unless the row gives its own
  void *(*buf)(const t41rx_ctx *);
  int (*get)(const t41rx_ctx *, void *host, size_t bytes);  // device -> host
  int (*put)(t41rx_ctx *, const void *host, size_t bytes);  // host -> device
  int (*reset)(t41rx_ctx *, size_t bytes);                  // power-on of what the context has allocated
};
// in bit order
const Section kSections[] = {
    // noise reduction / notch: Xanr()'s taps, delay line and leak words [kAnrStRows][n_channels], then the Kim / spectral
    // records [n_channels][kNrSpecFloats] (Noise.cpp:19-56) -- present once the stages have run
    {kSecNr, "noise-reduction", (size_t)kAnrStRows + (size_t)kNrSpecFloats,
     [](const t41rx_ctx *c) { return c->nr.d_anr != nullptr; }, ensure_nr, nr_check, nullptr, nr_get, nr_put, nr_reset},
    // display FFT: zoom filters, ring, FFT_spec_old [n_channels][kDispFloats] (FFT.cpp:14-26) -- present while
    // t41rx_set_display_spectrum is on (which allocates it); header word 6 = its spectrumZoom; reset is ZoomFFTPrep()
    {kSecDisp, "display-FFT", (size_t)kDispFloats,
     [](const t41rx_ctx *c) { return c->disp.spec && c->disp.d_state; }, nullptr, display_check,
     [](const t41rx_ctx *c) -> void * { return c->disp.d_state.get(); }, nullptr, nullptr, nullptr},
    // noise blanker: last_frame_end[0 .. 12] (DSP_Fn.cpp:143), [n_channels][kNbCarryPitch] (3 floats of padding) -- the
    // current one of the two slots out, slot 0 in; present once the blanker has run
    {kSecNb, "noise-blanker", (size_t)kNbCarryPitch,
     [](const t41rx_ctx *c) { return c->nb.d_carry != nullptr; }, ensure_nb, nullptr, nullptr, nb_get, nb_put, nb_reset},
    // receive equalizer: rec_EQ_Band1_state .. rec_EQ_Band14_state (Filter.cpp:43-56), [n_channels][kEqStateFloats] --
    // present once the equalizer has run (zeroed statics)
    {kSecEq, "receive-equalizer", (size_t)kEqStateFloats,
     [](const t41rx_ctx *c) { return c->eq.d_state != nullptr; }, ensure_eq, nullptr,
     [](const t41rx_ctx *c) -> void * { return c->eq.d_state.get(); }, nullptr, nullptr, nullptr},
    // CW receive: CW_AudioFilter1_state .. CW_AudioFilter5_state (CWProcessing.cpp:37-41), the decode FIR's history
    // (FIR_CW_DecodeL_state, T41_SDR.ino:281), corrResultR, aveCorrResultL / R, [n_channels][kCwStateFloats] -- present
    // once a CW stage has run (zeroed statics)
    {kSecCw, "CW-receive", (size_t)kCwStateFloats,
     [](const t41rx_ctx *c) { return c->cw.d_state != nullptr; }, ensure_cw, nullptr,
     [](const t41rx_ctx *c) -> void * { return c->cw.d_state.get(); }, nullptr, nullptr, nullptr},
    // CW decoder: DoCWDecoding()'s statics and the globals it shares with its histograms (CWProcessing.cpp:26-99,
    // :538-550), then signalHistogram, then gapHistogram, [n_channels][kCwDecWords] int32 words (cw_kernels.hpp names
    // them) -- present once the decoder has run; its power-on words are not all zero
    {kSecCwDec, "CW-decoder", (size_t)kCwDecWords,
     [](const t41rx_ctx *c) { return c->cw.d_dec != nullptr; }, ensure_cw_decode, check_cw_decode,
     [](const t41rx_ctx *c) -> void * { return c->cw.d_dec.get(); }, nullptr, nullptr, cw_decode_reset},
};

int section_get(const Section &s, const t41rx_ctx *c, void *h, size_t n) {
  return s.get ? s.get(c, h, n) : hip_check(hipMemcpy(h, s.buf(c), n, hipMemcpyDeviceToHost), "hipMemcpy");
}
int section_put(const Section &s, t41rx_ctx *c, const void *h, size_t n) {
  return s.put ? s.put(c, h, n) : hip_check(hipMemcpy(s.buf(c), h, n, hipMemcpyHostToDevice), "hipMemcpy");
}
int section_reset(const Section &s, t41rx_ctx *c, size_t n) {
  if (s.reset) return s.reset(c, n);
  return s.buf(c) ? hip_check(hipMemset(s.buf(c), 0, n), "hipMemset") : T41RX_OK;
}

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

}  // namespace

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
    const int rc = section_reset(s, ctx, section_bytes(s, ctx->nchan));
    if (rc != T41RX_OK) return rc;
  }
  return ft8_power_on(ctx);
}

}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_reset(t41rx_ctx *ctx) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  HIP_TRY(hipDeviceSynchronize());
  int rc = pipe_timeouts_clear(ctx);  // (and the pipelined kernels' time-out counter)
  if (rc != T41RX_OK) return rc;
  // the memories outside the checkpoint likewise: the calibration's, the panadapter's with its frame counter, and the
  // beacon monitor's behind it
  if ((rc = cal_reset(ctx)) != T41RX_OK || (rc = pan_reset(ctx)) != T41RX_OK || (rc = beacon_reset(ctx)) != T41RX_OK) return rc;
  return reset_state(ctx);
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
                    (int32_t)sf, sec, (sec & kSecDisp) ? ctx->disp.zoom : 0, 0};
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
    if ((rc = section_get(s, ctx, out, section_bytes(s, ctx->nchan))) != T41RX_OK) return rc;
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
    if ((rc = (sec & s.bit) ? section_put(s, ctx, p, n) : section_reset(s, ctx, n)) != T41RX_OK) return rc;
    if (sec & s.bit) p += n;
  }
  if ((rc = ft8_power_on(ctx)) != T41RX_OK) return rc;  // (the FT8 memory has a record of its own: a checkpoint starts it afresh)
  return pipe_timeouts_clear(ctx);  // the restored state is valid again
}

}  // extern "C"
