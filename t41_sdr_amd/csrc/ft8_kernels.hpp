// t41_sdr_amd/csrc/ft8_kernels.hpp -- argument block and launchers of the FT8 receive stage (ft8_kernel.hip): the audio
// collector of DEMOD_FT8 (Process.cpp:627-686) and process_FT8_FFT() / extract_power() (ft8.cpp:223-268) up to the
// finished waterfall, with update_synchronization()'s slot timing (ft8.cpp:154-166).  Product code: nothing from oracle/.
// The Blackman window and the mag_db table are the caller's (t41rx_set_ft8_tables): the library holds no copy of its own.
// arm_rfft_q15's constant tables are CMSIS-DSP's and are rebuilt on the host (ft8_make_fft_tables).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rx_ft8map.hpp"

namespace t41 {

constexpr int kFt8Gulp = 1024;                      // input_gulp_size: samples @6.4 kS/s per 15 frames
constexpr int kFt8Fft = 2048;                       // FFT_SIZE
constexpr int kFt8BufWords = 3 * kFt8Gulp;          // ft8_dsp_buffer
constexpr int kFt8Row = 368;                        // ft8_buffer
constexpr int kFt8BlockBytes = 4 * kFt8Row;         // offset_step: two time offsets x two frequency offsets
constexpr int kFt8SlotBlocks = 92;                  // ft8_msg_samples
constexpr int kFt8HalfBytes = kFt8SlotBlocks * kFt8BlockBytes;
constexpr int kFt8Bins = 2 * kFt8Row + 1;           // FFT bins 0 .. 736 are read
constexpr int kFt8MagEntries = 16385;               // mag_db by (re*re + im*im) >> 17 = 0 .. 16384
constexpr int kFt8MaxFrames = 1380;                 // 92 x 15: at most one completion per channel and call
// per channel kFt8Words int32 words, the record's layout and the device's alike: kFt8Scalars scalars (by name below, the
// rest zero), then ft8_dsp_buffer, one q15 sample per word
constexpr int kFt8Scalars = 16;
constexpr int kFt8Words = kFt8Scalars + kFt8BufWords;  // 3088
enum Ft8Word : int {
  kFt8N = 0,      // FT8 frames since power-on or reset (unsigned): millis(n) = t0 + floor(n * num / den)
  kFt8Sync,       // syncFlag
  kFt8Flag,       // ft8_flag
  kFt8DspFlag,    // DSP_Flag
  kFt8Counter,    // FT_8_counter, 0 .. 91
  kFt8DataLoop,   // 0 .. 14
  kFt8Leftover,   // 0 .. 3
  kFt8Start,      // start_time (unsigned)
  kFt8Half,       // which half of the power buffer is being written
  kFt8Named
};
static_assert(kFt8Named <= kFt8Scalars, "scalars");
// arm_rfft_q15's tables as packed q15 pairs (first value in the low half): twiddleCoef_1024_q15's 768 (cos, sin), then
// realCoefAQ15 and realCoefBQ15 at modifier 4 for bins 0 .. 736
constexpr int kFt8TabTw = 0, kFt8TabA = 768, kFt8TabB = kFt8TabA + kFt8Bins, kFt8TabWords = kFt8TabB + kFt8Bins;

struct Ft8Args {
  const float *aud;       // [nchan][nframes * 256] float_buffer_L behind the demodulator and the AGC (read only)
  int32_t *state;         // [nchan][kFt8Words]
  uint8_t *power;         // [nchan][2][kFt8HalfBytes] export_fft_power, two halves
  int32_t *status;        // [nchan][nframes][4]: FT_8_counter behind the frame, ft8_flag, 0 or 1 + the half completed, dataLoop
  const float *window;    // [kFt8Fft] (device)
  const float *mag_db;    // [kFt8MagEntries] (device)
  const uint32_t *tab;    // [kFt8TabWords] (device)
  int nchan, nframes;
  int32_t t0, num, den;   // the clock (t41rx_set_ft8_clock)
};
hipError_t launch_ft8(const Ft8Args &a, hipStream_t s);
// the list form under an FT8 map (t41rx_set_ft8_map; rx_ft8map.hpp): a workgroup per pair of `list`, which indexes state
// and aud by the pair's channel, power and status by its row.  Ft8Args' members in Ft8Args' order (ft8_kernel.inc is one
// text for both), then the list.  An empty list is not launched.
struct Ft8ListArgs {
  const float *aud;       // [nchan][nframes * 256]
  int32_t *state;         // [nchan][kFt8Words]
  uint8_t *power;         // [rows][2][kFt8HalfBytes]
  int32_t *status;        // [rows][nframes][4]
  const float *window;
  const float *mag_db;
  const uint32_t *tab;
  int nchan, nframes;
  int32_t t0, num, den;
  const Ft8Pair *list;    // [nlist] (device), ascending by channel, no row twice
  int nlist;              // 1 .. nchan: the grid
};
hipError_t launch_ft8_list(const Ft8ListArgs &a, hipStream_t s);
// auto_sync_FT8()'s success branch on the channels whose mask byte is non-zero (mask: device pointer, or null for all)
hipError_t launch_ft8_sync(int32_t *state, const uint8_t *mask, int nchan, int32_t t0, int32_t num, int32_t den, hipStream_t s);
// FT8 from 12 kS/s audio: the collector of DEMOD_FT8_WAV (Process.cpp:278-335) in front of the same transform, on the same
// record, power halves and status words.  128 samples per frame, 68 cells of each third of the buffer per frame.
constexpr int kFt8AudioFrame = 128;
constexpr int kFt8AudioCells = 68;
struct Ft8AudioArgs {
  const void *pcm;        // [nchan][nframes * 128] int16 (q15 != 0) or float, channel-major (read only)
  int32_t *state;         // [nchan][kFt8Words]
  uint8_t *power;         // [nchan][2][kFt8HalfBytes]
  int32_t *status;        // [nchan][nframes][4], as Ft8Args::status
  const float *window;    // [kFt8Fft] (device)
  const float *mag_db;    // [kFt8MagEntries] (device)
  const uint32_t *tab;    // [kFt8TabWords] (device)
  int nchan, nframes;     // nframes <= kFt8MaxFrames
  int q15;
};
hipError_t launch_ft8_audio(const Ft8AudioArgs &a, hipStream_t s);
// its list form: state by the pair's channel; pcm, power and status by its row
struct Ft8AudioListArgs {
  const void *pcm;        // [rows][nframes * 128]
  int32_t *state;         // [nchan][kFt8Words]
  uint8_t *power;         // [rows][2][kFt8HalfBytes]
  int32_t *status;        // [rows][nframes][4]
  const float *window;
  const float *mag_db;
  const uint32_t *tab;
  int nchan, nframes;
  int q15;
  const Ft8Pair *list;    // [nlist] (device)
  int nlist;              // 1 .. nchan: the grid
};
hipError_t launch_ft8_audio_list(const Ft8AudioListArgs &a, hipStream_t s);
// setupFT8Wav()'s FT_8_counter = 0 (end = 0) or the mode's exit, syncFlag = FT_8_counter = ft8_flag = 0 (end = 1), on the
// channels whose mask byte is non-zero (mask: device pointer, or null for all)
hipError_t launch_ft8_audio_mark(int32_t *state, const uint8_t *mask, int nchan, int end, hipStream_t s);
// the tables above (host)
void ft8_make_fft_tables(uint32_t *tab);

}  // namespace t41
