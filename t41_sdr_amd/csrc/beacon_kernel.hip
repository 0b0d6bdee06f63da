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
// beacon_kernel, and its list form under a panadapter map: the text is beacon_kernel.inc
#define T41_STAGE_KERNEL beacon_kernel
#define T41_STAGE_ARGS BeaconArgs
#define T41_STAGE_LIST 0
#include "beacon_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL beacon_list_kernel
#define T41_STAGE_ARGS BeaconListArgs
#define T41_STAGE_LIST 1
#include "beacon_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST

hipError_t launch_beacon(const BeaconArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nrows <= 0) return hipSuccess;
  hipLaunchKernelGGL(beacon_kernel, dim3((unsigned)((a.nchan + 63) / 64)), dim3(64), 0, s, a);
  return hipGetLastError();
}

// the list form: one lane per entry; nobody listed launches nothing
hipError_t launch_beacon_list(const BeaconListArgs &a, hipStream_t s) {
  if (a.nlist <= 0 || a.nrows <= 0) return hipSuccess;
  hipLaunchKernelGGL(beacon_list_kernel, dim3((unsigned)((a.nlist + 63) / 64)), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
