// t41_sdr_amd/csrc/rx_ft8_decode.cpp -- host side of the FT8 decode of a finished slot (ft8_decode_kernel.hip): the
// tables as validated, the settings and stage taps, and the decode entry points.  No part of a process call.
#include <cstring>

#include "rx_ctx.hpp"

using namespace t41;

void t41::ft8_decode_release(t41rx_ctx *ctx) {
  if (ctx->ft8d.sel_ev) (void)hipEventDestroy(ctx->ft8d.sel_ev);
  if (ctx->ft8d.h_sel) (void)hipHostFree(ctx->ft8d.h_sel);
}

extern "C" {

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
  if (!ctx->ft8d.d_tab) HIP_TRY(dev_alloc(ctx->ft8d.d_tab, sizeof(Ft8DecodeTables)));
  HIP_TRY(hipMemcpy(ctx->ft8d.d_tab.get(), &h, sizeof(h), hipMemcpyHostToDevice));
  ctx->ft8d.have_tables = true;
  return T41RX_OK;
}

int t41rx_set_ft8_decode(t41rx_ctx *ctx, int max_candidates, int min_score, int ldpc_iterations) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (max_candidates < 1 || max_candidates > T41RX_FT8_MAX_CANDIDATES) return fail(T41RX_ERR_ARG, "FT8 decode: max_candidates must be 1..20");
  if (ldpc_iterations < 1 || ldpc_iterations > 50) return fail(T41RX_ERR_ARG, "FT8 decode: ldpc_iterations must be 1..50");
  ctx->ft8d.max_candidates = max_candidates;
  ctx->ft8d.min_score = min_score;
  ctx->ft8d.iterations = ldpc_iterations;
  return T41RX_OK;
}

int t41rx_get_ft8_decode(const t41rx_ctx *ctx, int *max_candidates, int *min_score, int *ldpc_iterations) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (max_candidates) *max_candidates = ctx->ft8d.max_candidates;
  if (min_score) *min_score = ctx->ft8d.min_score;
  if (ldpc_iterations) *ldpc_iterations = ctx->ft8d.iterations;
  return T41RX_OK;
}

int t41rx_set_ft8_decode_debug(t41rx_ctx *ctx, float *d_log174, uint8_t *d_plain) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  ctx->ft8d.dbg_log174 = d_log174;
  ctx->ft8d.dbg_plain = d_plain;
  return T41RX_OK;
}

int t41rx_ft8_decode_device(t41rx_ctx *ctx, const uint8_t *d_waterfall, size_t channel_stride_bytes, const int8_t *select, int n,
                            t41rx_ft8_result *d_results, void *hip_stream) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!d_results) return fail(T41RX_ERR_ARG, "FT8 decode: no result buffer (d_results is NULL)");
  if (!ctx->ft8d.have_tables) return fail(T41RX_ERR_ARG, "FT8 decode: no tables loaded (t41rx_set_ft8_decode_tables)");
  // the context's own d_power under an FT8 map (t41rx_set_ft8_map) is decoded by row: select, the results and the debug
  // buffers are [n_rows], and the kernels below run with nchan = n_rows.  A caller's own waterfall stays by channel.
  const bool by_row = !d_waterfall && ctx->ft8.on && ctx->ft8.map_on;
  if (by_row) {
    if (n != ft8_rows(ctx)) return fail(T41RX_ERR_ARG, "FT8 decode: with an FT8 map the context's own d_power is decoded by row: n must equal t41rx_ft8_rows()");
  } else if (n != ctx->nchan) {
    return fail(T41RX_ERR_ARG, "FT8 decode: n must equal n_channels");
  }
  bool slot1 = false;
  if (select)
    for (int c = 0; c < n; ++c) {
      if (select[c] < -1 || select[c] > 1) return fail(T41RX_ERR_ARG, "FT8 decode: select must be -1 (skip), 0 or 1");
      slot1 = slot1 || select[c] == 1;
    }
  if (!d_waterfall) {
    if (!ctx->ft8.on) return fail(T41RX_ERR_ARG, "FT8 decode: d_waterfall is NULL and FT8 receive is off (no d_power to read)");
    d_waterfall = ctx->ft8.power;
    channel_stride_bytes = 2 * (size_t)kFt8HalfBytes;
  }
  if ((reinterpret_cast<uintptr_t>(d_waterfall) & 3u) || (channel_stride_bytes & 3u))
    return fail(T41RX_ERR_ARG, "FT8 decode: the waterfall and its channel stride must be 4-byte aligned");
  if (n > 1 && channel_stride_bytes < (size_t)kFt8HalfBytes * (slot1 ? 2 : 1))
    return fail(T41RX_ERR_ARG, "FT8 decode: channel_stride_bytes is smaller than the slots the call reads");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  const hipStream_t s = (hipStream_t)hip_stream;
  Ft8Decode &d = ctx->ft8d;
  if (select) {
    if (!d.d_sel) {
      // (n_channels entries: a by-row call takes fewer, and a later call by channel all of them)
      HIP_TRY(dev_alloc(d.d_sel, (size_t)ctx->nchan));
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&d.h_sel), (size_t)ctx->nchan, hipHostMallocDefault));
      HIP_TRY(hipEventCreateWithFlags(&d.sel_ev, hipEventDisableTiming));
    } else {
      HIP_TRY(hipEventSynchronize(d.sel_ev));  // the upload of the call before has read the pinned copy
    }
    std::memcpy(d.h_sel, select, (size_t)n);
    HIP_TRY(hipMemcpyAsync(d.d_sel.get(), d.h_sel, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(d.sel_ev, s));
  }
  const size_t taps = (size_t)n * T41RX_FT8_MAX_CANDIDATES * kLdpcN;
  if (d.dbg_log174) HIP_TRY(hipMemsetAsync(d.dbg_log174, 0, taps * sizeof(float), s));  // unused rows read zero
  if (d.dbg_plain) HIP_TRY(hipMemsetAsync(d.dbg_plain, 0, taps, s));
  Ft8DecodeArgs a{};
  a.waterfall = d_waterfall;
  a.stride = channel_stride_bytes;
  a.select = select ? d.d_sel.get() : nullptr;
  a.tab = d.d_tab.get();
  a.results = d_results;
  a.dbg_log174 = d.dbg_log174;
  a.dbg_plain = d.dbg_plain;
  a.nchan = n;
  a.max_candidates = d.max_candidates;
  a.min_score = d.min_score;
  a.iterations = d.iterations;
  return hip_check(launch_ft8_decode(a, s), "FT8 decode kernel launch");
}

int t41rx_ft8_decode_host(t41rx_ctx *ctx, const uint8_t *d_waterfall, size_t channel_stride_bytes, const int8_t *select, int n,
                          t41rx_ft8_result *results) {
  if (!ctx) return fail(T41RX_ERR_ARG, "null argument");
  if (!results) return fail(T41RX_ERR_ARG, "FT8 decode: no result buffer (results is NULL)");
  if (n < 1 || n > ctx->nchan) return fail(T41RX_ERR_ARG, "FT8 decode: n must equal n_channels (with an FT8 map and the context's own d_power: t41rx_ft8_rows())");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(T41RX_ERR_HIP, "hipSetDevice failed");
  if (!ctx->ft8d.d_res) HIP_TRY(dev_alloc(ctx->ft8d.d_res, sizeof(t41rx_ft8_result) * (size_t)ctx->nchan));
  if (const int rc = t41rx_ft8_decode_device(ctx, d_waterfall, channel_stride_bytes, select, n, ctx->ft8d.d_res.get(), nullptr)) return rc;
  HIP_TRY(hipMemcpy(results, ctx->ft8d.d_res.get(), sizeof(t41rx_ft8_result) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return T41RX_OK;
}

}  // extern "C"
