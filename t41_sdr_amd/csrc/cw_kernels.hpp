// t41_sdr_amd/csrc/cw_kernels.hpp -- argument blocks and launchers of the CW receive stages (cw_kernel.hip): the tone
// detector of DoCWReceiveProcessing() (CWProcessing.cpp:322-373, goertzel_mag :830-857) and the narrow audio filter
// selected by CWFilterIndex (Process.cpp:878-913).  Product code: nothing from oracle/.  The filter tables
// (CW_AudioFilterCoeffs1..5) and the decode FIR (CW_Filter_Coeffs2) are the caller's: the library holds no copy of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace t41 {

constexpr int kCwFilters = 5;                        // CWFilterIndex 0 .. 4 (5 = off)
constexpr int kCwStages = 6;                         // biquads per filter (S1_CW_AudioFilter1..5, numStages 6)
constexpr int kCwFilterCoefs = 5 * kCwStages;        // {b0, b1, b2, a1, a2} per section, a's negated (CMSIS DF2T)
constexpr int kCwFirTaps = 64;                       // CW_Filter_Coeffs2
constexpr int kCwBlock = 256;                        // samples per block @24 kS/s
// per-channel state, 128 floats: the five filters' memories [filter][stage][d1, d2] (CW_AudioFilter1_state ..
// CW_AudioFilter5_state), the decode FIR's 63-sample history (FIR_CW_DecodeL_state), corrResultR of the block before,
// the running averages aveCorrResultL / aveCorrResultR, two words of zero
constexpr int kCwStFilter = 0;
constexpr int kCwStFir = 2 * kCwStages * kCwFilters;  // 60
constexpr int kCwStCorrR = kCwStFir + kCwFirTaps - 1;  // 123
constexpr int kCwStAveL = kCwStCorrR + 1;
constexpr int kCwStAveR = kCwStCorrR + 2;
constexpr int kCwStateFloats = 128;
constexpr int kCwChanPerWave = 8;                    // the filter kernel packs 8 channels into a wave (8 lanes each, 6 used)

struct CwFilterArgs {
  float *aud;     // [nchan][nsamp] audio @24 kS/s, filtered in place
  float *state;   // [nchan][kCwStateFloats]
  int nchan, nsamp;  // nsamp = n_frames * 256
  int index;         // CWFilterIndex 0 .. 4: which of the five memories advances
  float coef[kCwFilterCoefs];  // the selected filter's [stage][5]
};
hipError_t launch_cw_filter(const CwFilterArgs &a, hipStream_t s);

// The same with a CWFilterIndex per channel (t41rx_set_cw_filter_map): the filter runs on the nlist channels of `list`,
// each with the memory and the coefficient row of its own index; the others' audio and memories are neither read nor
// written.  Eight channels of the list per wave.
struct CwFilterMapArgs {
  float *aud;           // [nchan][nsamp] audio @24 kS/s, the listed channels' rows filtered in place
  float *state;         // [nchan][kCwStateFloats]
  const int *list;      // the filtered channels, ascending; readable up to the next multiple of kCwChanPerWave entries
  const int *index_of;  // [nchan] CWFilterIndex per channel; 0 .. 4 for every channel of the list
  int nlist, nchan, nsamp;
  float coef[kCwFilters * kCwFilterCoefs];  // all five filters' [filter][stage][5]
};
hipError_t launch_cw_filter_map(const CwFilterMapArgs &a, hipStream_t s);

struct CwDetectArgs {
  const float *aud;  // [nchan][nframes * 256] audio @24 kS/s (read only)
  float *state;      // [nchan][kCwStateFloats]
  float *out;        // [nchan][nframes][4]: corrResultL, goertzelMagnitude, aveCorrResult, combinedCoeff
  int nchan, nframes;
  float coeff, cosine, sine;  // goertzel_mag(256, 750, 24000, .)'s constants in the firmware's types (host)
  float fir[kCwFirTaps];      // CW_Filter_Coeffs2
  float sinb[kCwBlock];       // sinBuffer (Utility.cpp:72-74)
  // the stage map (t41rx_set_stage_map), or null: the nlist > 0 channels the detector runs on, ascending; the others'
  // rows of `out` are not written
  const int *list;
  int nlist;
};
hipError_t launch_cw_detect(const CwDetectArgs &a, hipStream_t s);

// Behind the narrow filter: Process.cpp:917-937 as the firmware orders it -- arm_fir_interpolate_f32 x2 (48 taps) and x4
// (32 taps), each output one accumulator over its phase's taps, then the volume as a multiply of its own
// (arm_scale_f32) and, for q15 samples out, arm_float_to_q15.  The fused back kernel folds the volume into the x4 taps
// and accumulates with fused multiply-adds; this one is the oracle's interpolators bit for bit.
struct CwBackArgs {
  const float *aud;  // [nchan][nframes * 256] audio @24 kS/s
  float *state;      // the path's per-channel records (rx_internal.hpp: kStInt1, kStInt2), state_stride floats apart
  void *out;         // audio out, f32 or q15
  int nchan, nframes;
  long long chan_stride, frame_stride, state_stride;  // of out, in samples; of state, in floats
  int q15;
  float scale;       // DF * VolumeToAmplification(audioVolume)
  float int1[48];    // FIR_int1_coeffs
  float int2[32];    // FIR_int2_coeffs (not scaled)
  // the output map (t41rx_set_output_map), or null: channel c's audio goes to row out_map[c] of out; with out_map[c] < 0
  // the channel's block leaves before it reads the audio or the interpolator memories
  const int *out_map;
};
hipError_t launch_cw_back(const CwBackArgs &a, hipStream_t s);

// The same with parameter sets (t41rx_set_param_sets_ex with T41RX_SETS_STAGES): the volume factor and the two
// interpolators' taps are those of the channel's own set, entry set_of[channel] of a table the host makes of every set's
// blob (rx_sets.cpp) -- int2 unscaled, where DevCoef::int2 carries the volume folded in.  scale, int1 and int2 of the
// block above are not read.
struct CwSetBack {
  float scale;     // DF * VolumeToAmplification(audioVolume) of the set
  float pad[15];   // (the taps on a 64-byte boundary)
  float int1[48];  // FIR_int1_coeffs
  float int2[32];  // FIR_int2_coeffs (not scaled)
};
struct CwBackSetsArgs : CwBackArgs {
  const int *set_of;      // [nchan] the channel's set
  const CwSetBack *sets;  // [K + 1]
};
hipError_t launch_cw_back_sets(const CwBackSetsArgs &a, hipStream_t s);

// ---- the Morse decoder behind the detector: DoCWDecoding() and its histograms (CWProcessing.cpp:365-371, :501-815) ----
// Per channel kCwDecWords int32 words, the checkpoint section's layout and the device's alike: kCwDecScalars scalars (by
// name below; thresholdGeometricMean as its float's bits, the two flags as 0 / 1, words 28 .. 31 zero), then
// signalHistogram (kCwDecSigWords), then gapHistogram (kCwDecGapWords).  The firmware gives either histogram a 3072-word
// allotment and clears and scales words 0 .. 749 only; from power-on no access goes past word 2303 (gap) or 749
// (signal), so carrying 2304 and 768 words makes every firmware access an exact in-bounds one (tests/cw_decode_model.py).
constexpr int kCwDecScalars = 32, kCwDecSigWords = 768, kCwDecGapWords = 2304;
constexpr int kCwDecOffSig = kCwDecScalars, kCwDecOffGap = kCwDecScalars + kCwDecSigWords;
constexpr int kCwDecWords = kCwDecOffGap + kCwDecGapWords;  // 3104
constexpr int kCwHistElements = 750;                       // HISTOGRAM_ELEMENTS
constexpr int kCwTreeChars = 129;                          // bigMorseCodeTree
enum CwDecWord : int {
  kCwDecState = 0,     // decodeStates: 0, 1, 2, 5, 6
  kCwDecN,             // decoder frames since power-on or reset (unsigned): millis(n) = t0 + floor(n * num / den)
  kCwDecOldTime,       // oldTime (set to millis(0) by the frame with n == 0, as the static's initialiser does)
  kCwDecSignalStart,
  kCwDecSignalEnd,
  kCwDecElapsed,       // signalElapsedTime
  kCwDecGapLength,
  kCwDecDitLength,     // (unsigned long)
  kCwDecDahLength,
  kCwDecGapAtom,
  kCwDecGapChar,
  kCwDecTgm,           // thresholdGeometricMean, float bits
  kCwDecAveDit,
  kCwDecAveDah,
  kCwDecValRef1,
  kCwDecValRef2,
  kCwDecGapRef1,
  kCwDecValFlag,
  kCwDecSignalStartOld,
  kCwDecDashJump,      // currentDashJump (byte)
  kCwDecIndex,         // currentDecoderIndex (byte)
  kCwDecCharFlag,      // charProcessFlag
  kCwDecBlankFlag,
  kCwDecTopGap,        // topGapIndex
  kCwDecTopGapOld,
  kCwDecCurrentTime,
  kCwDecInterGap,      // interElementGap
  kCwDecNoSignal,      // noSignalTimeStamp
  kCwDecNamed          // 28
};
static_assert(kCwDecNamed <= kCwDecScalars, "scalars");

struct CwDecodeArgs {
  const float *cw;   // the detector's results of this call [nchan][nframes][4]: combinedCoeff is word 3
  int32_t *state;    // [nchan][kCwDecWords]
  int32_t *text;     // [nchan][nframes][2]: {character code or 0, ditLength behind the frame}
  int nchan, nframes;
  int32_t t0, num, den;               // the clock (t41rx_set_cw_clock)
  uint8_t tree[kCwTreeChars + 3];     // bigMorseCodeTree (the caller's)
  // the stage map (t41rx_set_stage_map), or null: the nlist > 0 channels the decoder runs on, ascending -- a subset of the
  // detector's list, whose rows of `cw` it reads; the others' rows of `text` are not written
  const int *list;
  int nlist;
};
hipError_t launch_cw_decode(const CwDecodeArgs &a, hipStream_t s);
// ResetHistograms() (CWProcessing.cpp:501-517) on the channels whose mask byte is non-zero (mask: device pointer, or null
// for all): words 0 .. 749 of both histograms and the scalars it names
hipError_t launch_cw_decode_reset(int32_t *state, const uint8_t *mask, int nchan, hipStream_t s);
// the power-on words of one channel (host): what ResetHistograms() leaves, currentDashJump = 128, everything else zero
void cw_decode_power_on(int32_t *w);

}  // namespace t41
