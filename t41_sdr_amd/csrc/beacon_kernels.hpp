// t41_sdr_amd/csrc/beacon_kernels.hpp -- argument block and launcher of the beacon monitor stage (beacon_kernel.hip):
// BeaconLoop()'s synced branch (Beacon.cpp:455-569), one call per panadapter row, on the row's dbm.  Product code:
// nothing from oracle/.  The library carries no beacon names, maps or bearings: indices 0 .. 17 are the interface.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rx_panmap.hpp"

namespace t41 {

constexpr int kBeaconCount = 18;      // beacons of the NCDXF schedule, one slot of 10 s each
constexpr int kBeaconBands = 5;       // 20, 17, 15, 12, 10 m
constexpr int kBeaconCycleMs = 180000;
constexpr int kBeaconNoiseCount = 23;  // NOISE_HI - NOISE_LO - 2 (Beacon.cpp:455-456, :528)
// Per channel kBeaconWords int32 words, the record's layout and the device's alike: BeaconLoop()'s statics by name, the
// file's `band`, and the one band monitorFreq[] has set for this channel.
enum BeaconWord : int {
  kBeaconMin = 0,      // min, float bits
  kBeaconMax,          // max, float bits
  kBeaconSnrCount,     // snrCount
  kBeaconCnt,          // count
  kBeaconChangeBand,   // changeBandFlag, 0 / 1
  kBeaconCurrent,      // currentBeacon
  kBeaconBand,         // band, the loop's
  kBeaconOwnBand,      // the channel's band: monitorFreq[b] == (b == this)
  kBeaconWords         // 8
};

struct BeaconArgs {
  const float *smeter;  // the panadapter's rows of this call [nchan][pan_rows][4]: dbm is word 3
  int32_t *state;       // [nchan][kBeaconWords]
  float *snr;           // [nchan][18]: beaconSNR[.][band of the channel]
  int32_t *events;      // [nchan][ev_rows][4] or null: {beacon recorded or -1, snrCount, count, band}
  int nchan, nrows;     // rows 0 .. nrows-1 of every channel, in order
  int pan_rows, ev_rows;  // rows per channel the two buffers hold
  long long n_first;    // the panadapter's frame number of row 0; row r has n_first + r * period
  int period;
  int mode;             // 0: the firmware's cycle; 1: continuous
  int32_t t0, num, den; // the clock: slot(n) = ((t0 + floor(n * num / den)) / 1000 % 180) / 10
};
hipError_t launch_beacon(const BeaconArgs &a, hipStream_t s);
// the list form under a panadapter map (t41rx_set_panadapter_map; rx_panmap.hpp): a lane per entry of `list`, which
// indexes state, snr and events by the entry's channel and smeter by its row.  BeaconArgs' members in BeaconArgs' order
// (beacon_kernel.inc is one text for both), then the list.  An empty list is not launched.
struct BeaconListArgs {
  const float *smeter;  // [rows][pan_rows][4]
  int32_t *state;       // [nchan][kBeaconWords]
  float *snr;           // [nchan][18]
  int32_t *events;      // [nchan][ev_rows][4] or null
  int nchan, nrows;
  int pan_rows, ev_rows;
  long long n_first;
  int period;
  int mode;
  int32_t t0, num, den;
  const PanEntry *list; // [nlist] (device), ascending by channel, no row twice
  int nlist;            // 1 .. nchan
};
hipError_t launch_beacon_list(const BeaconListArgs &a, hipStream_t s);

// the schedule in int64, host and device alike: GetBeacon20mNow() and GetBeaconNow(band) (Beacon.cpp:204-211) at frame n
__host__ __device__ inline int beacon_slot(long long n, int t0, int num, int den) {
  const long long ms = (long long)t0 + n * (long long)num / (long long)den;
  return (int)((ms / 1000 % 180) / 10);
}
__host__ __device__ inline int beacon_now(int slot, int band) {
  const int index = slot - band;
  return index + (index < 0 ? kBeaconCount : 0);
}

}  // namespace t41
