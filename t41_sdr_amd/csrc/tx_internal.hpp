// t41_sdr_amd/csrc/tx_internal.hpp -- layouts shared by the host side and the HIP kernel of the
// transmit exciter.  Product code: must not include or link anything from oracle/.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/t41rx.h"
#include "../../include/t41tx.h"

namespace t41 {

extern const float kTx192k10k[48], kTx48k8k[48], kTxHilbert45[100], kTxHilbertNeg45[100];

// device coefficient block (scalar-loadable)
struct TxCoef {
  float c192[48];   // /4 decimator (48 taps) and x4 interpolator (first 32)
  float c48[48];    // /2 decimator (first 24) and x2 interpolator (48)
  float h45[100];   // FIR_Hilbert_L
  float hn45[100];  // FIR_Hilbert_R
};

// per-channel state (floats): the CMSIS instance states' history parts, T41_SDR.ino:278-299
constexpr int kTxStDec1 = 0;     // 47 (+1 pad): last 47 input samples @192 kS/s
constexpr int kTxStDec2 = 48;    // 23 (+1): last 23 /4 outputs
constexpr int kTxStHilL = 72;    // 99 (+1): last 99 samples @24 kS/s
constexpr int kTxStHilR = 172;   // 99 (+1)
constexpr int kTxStInt1I = 272;  // 23 (+1)
constexpr int kTxStInt1Q = 296;  // 23 (+1)
constexpr int kTxStInt2I = 320;  // 7 (+1)
constexpr int kTxStInt2Q = 328;  // 7 (+1)
constexpr int kTxDelayFloats = 336;  // the delay lines above: the kernel's stride in [nchan][kTxDelayFloats]

// the transmit equaliser (DoExciterEQ(), Filter.cpp:176-224): 14 bands of 4 DF2T sections, as the receive one
constexpr int kTxEqBands = 14;
constexpr int kTxEqSections = 4 * kTxEqBands;   // 56: one per lane
constexpr int kTxEqCoefs = 5 * kTxEqSections;   // {b0, b1, b2, a1, a2} per section, a's negated (CMSIS DF2T)
// xmt_EQ_Band1_state .. xmt_EQ_Band14_state (Filter.cpp:74-87): [band][stage][d1, d2] = 2 * lane, 2 * lane + 1.  On the
// device they lie behind all the delay lines, [nchan][kTxEqStateFloats] (the delay lines keep their stride, and with it
// the equaliser-off kernel its code); a checkpoint's channel record holds both.
constexpr int kTxEqStateFloats = 2 * kTxEqSections;  // 112
constexpr int kTxStEq = kTxDelayFloats;              // where a channel record holds them
constexpr int kTxStateFloats = kTxDelayFloats + kTxEqStateFloats;  // 448 per channel: record size and device memory

struct TxArgs {
  const int16_t *__restrict__ inL;
  int16_t *__restrict__ outL;
  int16_t *__restrict__ outR;
  float *__restrict__ state;
  const TxCoef *__restrict__ coef;
  int nchan, nframes;
  float i_scale;   // +IQXAmp (LSB) / -IQXAmp (USB), Exciter.cpp:117-126
  float iq_phase;  // IQXPhaseCorrectionFactor
  int corr_on;     // LSB or USB
};

// the equaliser-on kernel's arguments: the caller's band table and the signed levels travel by value, so a change takes
// effect at the next call
struct TxEqArgs : TxArgs {
  float *__restrict__ eq_state;  // [nchan][kTxEqStateFloats]
  float eq_coef[kTxEqCoefs];  // [band][stage][5]
  float eq_scale[16];         // per band: -xmtEQ_LevelScale for bands 1, 3, .., 13, + for 2, 4, .., 14 (Filter.cpp:197-210)
};

// the CW exciter's arguments (CW_ExciterIQData(), CW_Excite.cpp:66-118): it drives the x2 / x4 interpolators of TxArgs'
// state (kTxStInt1I .. kTxStInt2Q) and touches nothing else of a channel's record.  The caller's tone table travels by
// value, like the equaliser's band table: a new one takes effect at the next call.
constexpr int kTxCwTone = 256;       // cosBuffer2 / sinBuffer2: one frame @24 kS/s
constexpr int kTxCwKeyPerFrame = 16; // gate bytes per frame: one per 128-sample audio block @192 kS/s
struct TxCwArgs {
  const uint8_t *__restrict__ key;  // [nchan][nframes * 16], nonzero = the block passes; nullptr = every block passes
  int16_t *__restrict__ outL;
  int16_t *__restrict__ outR;
  float *__restrict__ state;        // [nchan][kTxDelayFloats]
  const TxCoef *__restrict__ coef;
  int nchan, nframes;
  float i_scale;   // -IQXAmp (LSB) / +IQXAmp (USB), CW_Excite.cpp:77-87: the opposite of TxArgs'
  float iq_phase;  // IQXPhaseCorrectionFactor
  int corr_on;     // LSB or USB
  float tone_cos[kTxCwTone];
  float tone_sin[kTxCwTone];
};

// the calibration exciter's arguments (ProcessIQData2(), Process2.cpp:309-349): the CW exciter's shape on the same
// memories, with cosBuffer3 / sinBuffer3, the caller's level and a correction candidate per channel
struct TxCalArgs {
  int16_t *__restrict__ outL;
  int16_t *__restrict__ outR;
  float *__restrict__ state;        // [nchan][kTxDelayFloats]
  const TxCoef *__restrict__ coef;
  const float *__restrict__ corr;   // [nchan][2] = IQXAmp, IQXPhase per channel; nullptr = iq_amp / iq_phase for all
  int nchan, nframes;
  float level;     // bandOutputFactor, Process2.cpp:309
  float iq_amp;    // IQXAmpCorrectionFactor: LSB scales I by its negative, USB by it (Process2.cpp:317-325)
  float iq_phase;  // IQXPhaseCorrectionFactor
  int corr_on;     // LSB or USB
  int lsb;
  float tone_cos[kTxCwTone];
  float tone_sin[kTxCwTone];
};

hipError_t launch_tx(const TxArgs &a, hipStream_t s);       // xmitEQFlag off
hipError_t launch_tx_cal(const TxCalArgs &a, hipStream_t s);  // ProcessIQData2(), transmit half
hipError_t launch_tx_eq(const TxEqArgs &a, hipStream_t s);  // xmitEQFlag on
hipError_t launch_tx_cw(const TxCwArgs &a, hipStream_t s);  // CW_ExciterIQData()

}  // namespace t41
