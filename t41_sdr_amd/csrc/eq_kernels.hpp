// t41_sdr_amd/csrc/eq_kernels.hpp -- argument block and launcher of the receive equalizer (eq_kernel.hip; DoReceiveEQ(),
// Filter.cpp:117-165, call site Process.cpp:828-832).  Product code: nothing from oracle/.  The band table is the
// caller's (the firmware's EQ_Band1Coeffs .. EQ_Band14Coeffs): the library holds no copy of its own.
#pragma once
#include <hip/hip_runtime.h>

namespace t41 {

constexpr int kEqBands = 14;                         // EQ bands 1 .. 14
constexpr int kEqStages = 4;                         // IIR_NUMSTAGES: biquads per band
constexpr int kEqSections = kEqBands * kEqStages;    // 56
constexpr int kEqCoefs = 5 * kEqSections;            // {b0, b1, b2, a1, a2} per section, a's negated (CMSIS DF2T)
constexpr int kEqStateFloats = 2 * kEqSections;      // rec_EQ_Band1_state .. rec_EQ_Band14_state: 112 floats per channel

struct EqArgs {
  float *aud;     // [nchan][nsamp] demodulated audio @24 kS/s, equalized in place
  float *state;   // [nchan][kEqStateFloats]: [band][stage][d1, d2], as rec_EQ_Bandk_state
  int nchan, nsamp;  // nsamp = n_frames * 256 (a multiple of 64)
  float coef[kEqCoefs];   // [band][stage][5]
  float scale[16];        // per band: -recEQ_LevelScale for bands 1, 3, .., 13, +recEQ_LevelScale for 2, 4, .., 14
  // the stage map (t41rx_set_stage_map), or null: the nlist > 0 channels the stage runs on, ascending; the others' audio
  // and memories are neither read nor written
  const int *list;
  int nlist;
  // the level map (t41rx_set_receive_eq_map), or null: [nchan][kEqBands] signed levels in `scale`'s form, which then is
  // not read
  const float *levels;
};
hipError_t launch_eq(const EqArgs &a, hipStream_t s);

}  // namespace t41
