// t41_sdr_amd/csrc/nb_kernels.hpp -- argument block and launcher of the receive noise blanker (nb_kernel.hip;
// NoiseBlanker() / AltNoiseBlanking(), DSP_Fn.cpp:105-362, call site Process.cpp:873-876).  Product code: nothing
// from oracle/.
#pragma once
#include <hip/hip_runtime.h>

namespace t41 {

constexpr int kNbBlock = 256;     // NB_FFT_SIZE = FFT_LENGTH / 2 (DSP_Fn.h:6)
constexpr int kNbOrder = 10;      // NB_taps: the LPC order
constexpr int kNbPL = 3;          // (NB_impulse_samples - 1) / 2
constexpr int kNbImpulse = 7;     // NB_impulse_samples: samples replaced around a detection
constexpr int kNbBoundary = 14;   // boundary_blank: the scan stops before NB_FFT_SIZE - 14
constexpr int kNbMaxImpulses = 20;
constexpr int kNbCarry = kNbOrder + kNbPL;  // last_frame_end[0..12] = the previous block's x[242 .. 254]
constexpr int kNbCarryPitch = 16;           // floats per channel in the carry buffer (13 used)

struct NbArgs {
  float *aud;     // [nchan][nframes * 256] demodulated audio @24 kS/s, processed in place (samples 0 .. 239 written)
  float *carry;   // [2][nchan][kNbCarryPitch]: last_frame_end, ping-pong
  int nchan, nframes;
  int sel;        // carry slot frame 0 reads; the last frame writes slot sel ^ 1
  // the stage map (t41rx_set_stage_map), or null: the nlist > 0 channels the blanker runs on, ascending, and the nrest =
  // nchan - nlist it leaves out, whose carry the launch copies from slot sel to slot sel ^ 1
  const int *list, *rest;
  int nlist, nrest;
};
hipError_t launch_nb(const NbArgs &a, hipStream_t s);

}  // namespace t41
