// t41_sdr_amd/csrc/beacon_kernel.inc -- the text of beacon_kernel, included twice by beacon_kernel.hip: T41_STAGE_KERNEL
// names the kernel, T41_STAGE_ARGS its argument block, T41_STAGE_LIST 0 makes the kernel as it is without a panadapter map
// -- lane c is channel c and reads the smeter rows of channel c --, 1 its list form (t41rx_set_panadapter_map): lane i
// takes entry i of the host-built list (rx_panmap.hpp), indexes the statics, the table and the events by the entry's
// channel and the smeter rows by its row; lanes beyond the list's end return.  Two kernels of one text, not one body with
// a run-time switch: the form without a map must stay the instruction stream it was.
#if T41_STAGE_LIST
#define T41_BEACON_ROW ent.row
#else
#define T41_BEACON_ROW ch
#endif
__global__ __launch_bounds__(64) void T41_STAGE_KERNEL(T41_STAGE_ARGS a) {
#pragma clang fp contract(off)
#if T41_STAGE_LIST
  const int slot_of_lane = blockIdx.x * 64 + threadIdx.x;
  if (slot_of_lane >= a.nlist) return;  // lanes beyond the list's end
  const PanEntry ent = a.list[slot_of_lane];  // the host has checked the channel and the row (t41rx_set_panadapter_map)
  const int ch = ent.channel;
#else
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= a.nchan) return;
#endif
  int32_t *w = a.state + (size_t)ch * kBeaconWords;
  float mn = __int_as_float(w[kBeaconMin]), mx = __int_as_float(w[kBeaconMax]);
  int snrCount = w[kBeaconSnrCount], count = w[kBeaconCnt];
  bool changeBandFlag = w[kBeaconChangeBand] != 0;
  int currentBeacon = w[kBeaconCurrent], band = w[kBeaconBand];
  const int own = w[kBeaconOwnBand];
  const float *sm = a.smeter + (size_t)T41_BEACON_ROW * (size_t)a.pan_rows * 4;
  float *snr = a.snr + (size_t)ch * kBeaconCount;
  int4 *ev = a.events ? reinterpret_cast<int4 *>(a.events) + (size_t)ch * (size_t)a.ev_rows : nullptr;

  for (int r = 0; r < a.nrows; ++r) {
    const float dbm = sm[4 * r + 3];
    const int slot = beacon_slot(a.n_first + (long long)r * a.period, a.t0, a.num, a.den);
    int recorded = -1, seen = snrCount;
    if (count == 0 && changeBandFlag) {
      // change band; a band that is not monitored lets the next call come back here
      band++;
      if (band > 4) band = 0;
      if (band == own) changeBandFlag = false;  // monitorFreq[band]: the rest of this slot is for settling
    } else if (count > 0) {
      snrCount++;
      seen = snrCount;
      if (dbm < mn) mn = dbm;
      if (dbm > mx) mx = dbm;
      const int beacon = beacon_now(slot, band);
      if (beacon != currentBeacon) {
        float value = 0.0f;
        if (snrCount != kBeaconNoiseCount) {
          const float d = mx - mn;
          value = d > 0.0f ? d : 0.0f;
        }
        if ((unsigned)beacon < (unsigned)kBeaconCount) snr[beacon] = value;  // (always: the host checks the clock's range)
        recorded = beacon;
        snrCount = 0;
        currentBeacon = beacon;
        mn = 0.0f;
        mx = -1000.0f;
        count++;
        if (a.mode == 1) count = 1;  // continuous: every later change records
        if (count > kBeaconCount) {
          count = 0;
          changeBandFlag = true;
        }
      }
    } else {
      // count == 0 && !changeBandFlag: wait for the next beacon change (currentBeacon stays)
      const int beacon = beacon_now(slot, band);
      if (beacon != currentBeacon) count++;
    }
    if (ev && r < a.ev_rows) ev[r] = make_int4(recorded, seen, count, band);
  }

  w[kBeaconMin] = __float_as_int(mn);
  w[kBeaconMax] = __float_as_int(mx);
  w[kBeaconSnrCount] = snrCount;
  w[kBeaconCnt] = count;
  w[kBeaconChangeBand] = changeBandFlag ? 1 : 0;
  w[kBeaconCurrent] = currentBeacon;
  w[kBeaconBand] = band;
}
#undef T41_BEACON_ROW
