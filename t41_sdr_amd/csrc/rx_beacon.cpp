// t41_sdr_amd/csrc/rx_beacon.cpp -- host side of the beacon monitor stage (beacon_kernel.hip): the stage behind the
// panadapter in a process call, its switch-on (BeaconLoop()'s unsynced branch, Beacon.cpp:570-615), the stage's own state
// record, and the setters.
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "rx_ctx.hpp"

namespace t41 {
namespace {

constexpr uint32_t kBeaconMagic = 0x42313454u;  // "T41B"
constexpr size_t kBeaconHeaderBytes = 32;
constexpr int kBeaconRecordWords = kBeaconWords + kBeaconCount;  // per channel: the status words, then snr[18]
size_t beacon_record_bytes(const t41rx_ctx *ctx) { return kBeaconHeaderBytes + sizeof(int32_t) * kBeaconRecordWords * (size_t)ctx->nchan; }

// The unsynced branch at frame n_on: currentBeacon = GetBeacon20mNow(), count = 0, changeBandFlag = true, `band` = the
// last monitored band (the channel's only one); min / max / snrCount as the statics' initialisers; a table of zeros
// (BeaconInit(), Beacon.cpp:131-136).
int beacon_switch_on(t41rx_ctx *ctx, long long n_on) {
  BeaconStage &b = ctx->beacon;
  const float mn = 0.0f, mx = -1000.0f;
  std::vector<int32_t> h((size_t)kBeaconWords * (size_t)ctx->nchan, 0);
  for (int c = 0; c < ctx->nchan; ++c) {
    int32_t *w = h.data() + (size_t)kBeaconWords * (size_t)c;
    std::memcpy(&w[kBeaconMin], &mn, sizeof(mn));
    std::memcpy(&w[kBeaconMax], &mx, sizeof(mx));
    w[kBeaconChangeBand] = 1;
    w[kBeaconCurrent] = beacon_slot(n_on, b.clock.t0, b.clock.num, b.clock.den);
    w[kBeaconBand] = w[kBeaconOwnBand] = b.band[(size_t)c];
  }
  HIP_TRY(hipMemcpy(b.d_state.get(), h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(b.snr, 0, sizeof(float) * kBeaconCount * (size_t)ctx->nchan));
  return T41RX_OK;
}

// n * num of the clock must not wrap in int64 (the kernel indexes the table with what the clock gives)
bool beacon_clock_reaches(const StageClock &k, long long n) {
  return k.num == 0 || n <= (std::numeric_limits<long long>::max() - kBeaconCycleMs) / k.num;
}

}  // namespace

int beacon_prepare(t41rx_ctx *ctx) {
  const BeaconStage &b = ctx->beacon;
  const Panadapter &p = ctx->pan;
  if (!p.on || !p.out.smeter || !b.d_state || !b.snr) return fail(T41RX_ERR_STATE, "beacon monitor enabled without the panadapter's smeter rows or its buffers");
  if (p.call_rows > b.max_rows) return fail(T41RX_ERR_ARG, "the call holds more update frames than the max_rows the beacon monitor's buffers were set with");
  if (p.call_rows > 0 && !beacon_clock_reaches(b.clock, p.counter + p.call_first + (long long)(p.call_rows - 1) * p.period))
    return fail(T41RX_ERR_ARG, "beacon clock: the frame number times num does not fit 64 bits");
  return T41RX_OK;
}

int beacon_run(t41rx_ctx *ctx, hipStream_t s) {
  const BeaconStage &b = ctx->beacon;
  const Panadapter &p = ctx->pan;
  // what both forms of the kernel take (BeaconArgs, and BeaconListArgs with the list behind the same members)
  auto fill = [&](auto &a) {
    a.smeter = p.out.smeter;
    a.state = b.d_state.get();
    a.snr = b.snr;
    a.events = b.events;
    a.nchan = ctx->nchan;
    a.nrows = p.last_rows;
    a.pan_rows = p.max_rows;
    a.ev_rows = b.max_rows;
    a.n_first = p.last_first;
    a.period = p.period;
    a.mode = b.mode;
    a.t0 = b.clock.t0;
    a.num = b.clock.num;
    a.den = b.clock.den;
  };
  if (p.map_on) {
    // a panadapter map: the listed channels only, each on the smeter row it names; nobody listed: nothing to launch
    if (p.list.empty()) return T41RX_OK;
    BeaconListArgs a{};
    fill(a);
    a.list = p.d_list.get();
    a.nlist = (int)p.list.size();
    return hip_check(launch_beacon_list(a, s), "beacon list kernel launch");
  }
  BeaconArgs a{};
  fill(a);
  return hip_check(launch_beacon(a, s), "beacon kernel launch");
}

// t41rx_reset(): the panadapter's frame counter is 0 again; the monitor starts as it does at its switch
int beacon_reset(t41rx_ctx *ctx) { return ctx->beacon.on ? beacon_switch_on(ctx, 0) : T41RX_OK; }

}  // namespace t41

using namespace t41;

extern "C" {

int t41rx_set_beacon(t41rx_ctx *ctx, int on, int mode, const int32_t *band, float *d_snr, int32_t *d_events, int max_rows) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  BeaconStage &b = ctx->beacon;
  if (!on) {
    b.on = false;
    b.snr = nullptr;
    b.events = nullptr;
    b.max_rows = 0;
    return T41RX_OK;
  }
  // every refusal in front of the first change: a refused call leaves the stage as it was
  if (on != 1) return fail(T41RX_ERR_ARG, "beacon monitor: on must be 0 or 1");
  if (mode != 0 && mode != 1) return fail(T41RX_ERR_ARG, "beacon monitor: mode must be 0 (the firmware's cycle) or 1 (continuous)");
  if (!band) return fail(T41RX_ERR_ARG, "beacon monitor: no bands (band is NULL)");
  for (int c = 0; c < ctx->nchan; ++c)
    if (band[c] < 0 || band[c] >= kBeaconBands) return fail(T41RX_ERR_ARG, "beacon monitor: a channel's band must be 0 .. 4");
  if (!d_snr) return fail(T41RX_ERR_ARG, "beacon monitor: no table buffer (d_snr is NULL)");
  if (reinterpret_cast<uintptr_t>(d_snr) & 3u) return fail(T41RX_ERR_ARG, "beacon monitor: d_snr is not aligned to a float");
  if (reinterpret_cast<uintptr_t>(d_events) & 15u) return fail(T41RX_ERR_ARG, "beacon monitor: d_events must be 16-byte aligned");
  if (!ctx->pan.on) return fail(T41RX_ERR_UNSUPPORTED, "beacon monitor: the panadapter stage is off (t41rx_set_panadapter)");
  if (!ctx->pan.out.smeter) return fail(T41RX_ERR_UNSUPPORTED, "beacon monitor: the panadapter stage writes no smeter rows");
  if (max_rows < ctx->pan.max_rows) return fail(T41RX_ERR_ARG, "beacon monitor: max_rows is smaller than the panadapter's");
  if (!beacon_clock_reaches(b.clock, ctx->pan.counter)) return fail(T41RX_ERR_ARG, "beacon clock: the frame number times num does not fit 64 bits");
  // anything that fails from here on leaves the stage switched off
  b.on = false;
  if (!b.d_state) HIP_TRY(dev_alloc(b.d_state, sizeof(int32_t) * kBeaconWords * (size_t)ctx->nchan));
  b.band.assign(band, band + ctx->nchan);
  b.mode = mode;
  b.snr = d_snr;
  b.events = d_events;
  b.max_rows = max_rows;
  if (const int rc = beacon_switch_on(ctx, ctx->pan.counter)) return rc;
  b.on = true;
  return T41RX_OK;
}

int t41rx_set_beacon_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (t0_ms < 0 || t0_ms >= kBeaconCycleMs) return fail(T41RX_ERR_ARG, "beacon clock: t0_ms must lie in [0, 180000)");
  return set_stage_clock(ctx->beacon.clock, "beacon", t0_ms, num, den);
}

int t41rx_get_beacon(t41rx_ctx *ctx, float *snr, int32_t *status) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  const BeaconStage &b = ctx->beacon;
  if (!b.on) return 0;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  if (snr) HIP_TRY(hipMemcpy(snr, b.snr, sizeof(float) * kBeaconCount * (size_t)ctx->nchan, hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemcpy(status, b.d_state.get(), sizeof(int32_t) * kBeaconWords * (size_t)ctx->nchan, hipMemcpyDeviceToHost));
  return 1;
}

size_t t41rx_beacon_state_bytes(const t41rx_ctx *ctx) { return ctx ? beacon_record_bytes(ctx) : 0; }

int t41rx_beacon_get_state(t41rx_ctx *ctx, void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  if (bytes < beacon_record_bytes(ctx)) return fail(T41RX_ERR_STATE, "beacon state buffer too small");
  const BeaconStage &b = ctx->beacon;
  if (!b.on) return fail(T41RX_ERR_STATE, "the beacon monitor is off: it has no state");
  std::vector<float> snr((size_t)kBeaconCount * (size_t)ctx->nchan);
  std::vector<int32_t> st((size_t)kBeaconWords * (size_t)ctx->nchan);
  const int rc = t41rx_get_beacon(ctx, snr.data(), st.data());
  if (rc < 0) return rc;
  const int32_t hdr[8] = {(int32_t)kBeaconMagic, T41RX_ABI_VERSION, ctx->nchan, kBeaconRecordWords, 0, 0, 0, 0};
  std::memcpy(host_buf, hdr, sizeof(hdr));
  char *out = static_cast<char *>(host_buf) + kBeaconHeaderBytes;
  for (int c = 0; c < ctx->nchan; ++c) {
    std::memcpy(out, st.data() + (size_t)kBeaconWords * (size_t)c, sizeof(int32_t) * kBeaconWords);
    std::memcpy(out + sizeof(int32_t) * kBeaconWords, snr.data() + (size_t)kBeaconCount * (size_t)c, sizeof(float) * kBeaconCount);
    out += sizeof(int32_t) * kBeaconRecordWords;
  }
  return T41RX_OK;
}

int t41rx_beacon_set_state(t41rx_ctx *ctx, const void *host_buf, size_t bytes) {
  if (!ctx || !host_buf) return fail(T41RX_ERR_ARG, "null argument");
  BeaconStage &b = ctx->beacon;
  if (!b.on) return fail(T41RX_ERR_STATE, "the beacon monitor is off: switch it on first (t41rx_set_beacon)");
  if (bytes != beacon_record_bytes(ctx)) return fail(T41RX_ERR_STATE, "beacon state size mismatch");
  int32_t hdr[8];
  std::memcpy(hdr, host_buf, sizeof(hdr));
  if ((uint32_t)hdr[0] != kBeaconMagic || hdr[1] != T41RX_ABI_VERSION || hdr[2] != ctx->nchan || hdr[3] != kBeaconRecordWords)
    return fail(T41RX_ERR_STATE, "beacon state header does not match this context (magic / abi / channels / words per channel)");
  // what beacon_kernel branches, compares or steps with; everything is checked before anything is written
  const int32_t *all = reinterpret_cast<const int32_t *>(static_cast<const char *>(host_buf) + kBeaconHeaderBytes);
  std::vector<int32_t> st((size_t)kBeaconWords * (size_t)ctx->nchan), bands((size_t)ctx->nchan);
  std::vector<float> snr((size_t)kBeaconCount * (size_t)ctx->nchan);
  for (int c = 0; c < ctx->nchan; ++c) {
    const int32_t *w = all + (size_t)kBeaconRecordWords * (size_t)c;
    if (w[kBeaconSnrCount] < 0) return fail(T41RX_ERR_STATE, "beacon state: snrCount negative");
    if (w[kBeaconCnt] < 0 || w[kBeaconCnt] > kBeaconCount) return fail(T41RX_ERR_STATE, "beacon state: count out of range (0 .. 18)");
    if (w[kBeaconChangeBand] != 0 && w[kBeaconChangeBand] != 1) return fail(T41RX_ERR_STATE, "beacon state: changeBandFlag not 0 or 1");
    if (w[kBeaconCurrent] < 0 || w[kBeaconCurrent] >= kBeaconCount) return fail(T41RX_ERR_STATE, "beacon state: currentBeacon out of range (0 .. 17)");
    if (w[kBeaconBand] < 0 || w[kBeaconBand] >= kBeaconBands || w[kBeaconOwnBand] < 0 || w[kBeaconOwnBand] >= kBeaconBands)
      return fail(T41RX_ERR_STATE, "beacon state: band out of range (0 .. 4)");
    // (the channel has one column of beaconSNR: while it listens, `band` is its own)
    if ((w[kBeaconCnt] > 0 || w[kBeaconChangeBand] == 0) && w[kBeaconBand] != w[kBeaconOwnBand])
      return fail(T41RX_ERR_STATE, "beacon state: listening on a band that is not the channel's");
    std::memcpy(st.data() + (size_t)kBeaconWords * (size_t)c, w, sizeof(int32_t) * kBeaconWords);
    std::memcpy(snr.data() + (size_t)kBeaconCount * (size_t)c, w + kBeaconWords, sizeof(float) * kBeaconCount);
    bands[(size_t)c] = w[kBeaconOwnBand];
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(b.d_state.get(), st.data(), sizeof(int32_t) * st.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b.snr, snr.data(), sizeof(float) * snr.size(), hipMemcpyHostToDevice));
  b.band = std::move(bands);
  return T41RX_OK;
}

}  // extern "C"
