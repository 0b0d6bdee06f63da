// t41_sdr_amd/csrc/beacon_kernel.hip -- the beacon monitor stage: BeaconLoop()'s synced branch (Beacon.cpp:466-569) on the
// panadapter's dbm, one call per panadapter row.  Product code: nothing from oracle/.
//
// The firmware calls BeaconLoop() once per loop() pass (T41_SDR.ino:1014), which is once per ShowBeacon() sweep, and
// ShowBeacon() ends in DrawSmeterBar() "for the dbm calc": the dbm BeaconLoop() reads is the sweep's, smeter[3] of the
// panadapter row.  The firmware has one receiver and walks it over the monitored bands; a channel here has a fixed
// stream, so its monitorFreq[] has exactly one band set -- its own -- and the walk over the other four is the four
// calls of `band++` that find nothing to do.  What BeaconLoop() draws or sends (DisplayBeacons(), DisplayBeaconsSNR(),
// T41BeaconSendData()) stays with the caller: the stage leaves beaconSNR[.][band] and one event record per call.
#include "beacon_kernels.hpp"

namespace t41 {

// One lane per channel, 64 channels per wave, row after row; the statics live in registers from the first row of the
// call to the last.  Comparisons are the firmware's plain `<` / `>` (a NaN dbm moves neither min nor max, -inf moves min
// only), `max - min` is a float subtraction, and nothing is contracted or reassociated.
__global__ __launch_bounds__(64) void beacon_kernel(BeaconArgs a) {
#pragma clang fp contract(off)
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= a.nchan) return;
  int32_t *w = a.state + (size_t)ch * kBeaconWords;
  float mn = __int_as_float(w[kBeaconMin]), mx = __int_as_float(w[kBeaconMax]);
  int snrCount = w[kBeaconSnrCount], count = w[kBeaconCnt];
  bool changeBandFlag = w[kBeaconChangeBand] != 0;
  int currentBeacon = w[kBeaconCurrent], band = w[kBeaconBand];
  const int own = w[kBeaconOwnBand];
  const float *sm = a.smeter + (size_t)ch * (size_t)a.pan_rows * 4;
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

hipError_t launch_beacon(const BeaconArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nrows <= 0) return hipSuccess;
  hipLaunchKernelGGL(beacon_kernel, dim3((unsigned)((a.nchan + 63) / 64)), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
