// t41_sdr_amd/csrc/rx_kernels.hpp -- kernel argument block + launcher declaration (what the host files see of the kernels).
#pragma once
#include <hip/hip_runtime.h>

#include "rx_internal.hpp"
#include "rx_panmap.hpp"
#include "rx_plan.hpp"

namespace t41 {

// constant table (float2 units), one per context, FFT_LENGTH = 512:
//   mask  [8][64] : FIR_filter_mask[lane + 64 r] / N
//   tw1   [7][64] : W512^(lane * q),        q = 1..7   (forward sign)
//   tw2   [7][64] : W64^((lane & 7) * q),   q = 1..7
//   sincos[256]   : (cos, sin)(2 pi i / 256)
//   hp8[64], hp4[64]: DC high-pass scan multipliers (a1^(n((l&15)+1)), a1^(n((l&31)+1))), n = 8, 4
constexpr int kTabMask = 0;
constexpr int kTabTw1 = 512;
constexpr int kTabTw2 = kTabTw1 + 7 * 64;
constexpr int kTabSinCos = kTabTw2 + 7 * 64;
constexpr int kTabHp8 = kTabSinCos + 256;
constexpr int kTabHp4 = kTabHp8 + 64;
//   am[64][6]     : per-lane constants of the AM demodulator's two wave scans (chunks of 4 samples
//                   per lane): the DC blocker's 0.99^(4((l&15)+1)) and 0.99^(4((l&31)+1)) as doubles
//                   (2 float2), and the biquad's transition-matrix powers (M^4)^((l&15)+1),
//                   (M^4)^((l&31)+1) as 2 x 2 float2 each
constexpr int kTabAm = kTabHp4 + 64;
//   sam[260]      : arm_sin_f32's table, 513 floats sin(2 pi k / 512) (+ padding), for the synchronous detector
constexpr int kTabSam = kTabAm + 64 * 6;
constexpr int kTabEntries512 = kTabSam + 260;

// the gains of the first stage of one parameter set (RxArgs::set_gain): what RxArgs carries by value for set 0
struct SetGains {
  float g_rf, g_band, neg_iq_amp, iq_phase;
  int iq_corr_on;
  int pad[3];
};
static_assert(sizeof(SetGains) == 32, "SetGains: one 32-byte scalar load");

struct RxArgs {
  const float *__restrict__ I;
  const float *__restrict__ Q;
  float *__restrict__ out;
  float *__restrict__ state;
  const DevCoef *__restrict__ coef;
  const float2 *__restrict__ tab;
  const ChanNco *__restrict__ nco;
  int nchan;
  int nframes;
  // where (channel c, frame f) of I / Q / out starts, in samples: c * chan_stride + f * frame_stride (t41rx_set_buffer_layout)
  long long chan_stride;
  long long frame_stride;
  float *dbg_nco;
  float *dbg_dec;
  float *dbg_demod;
  float *dbg_pre;          // [nchan][nframes][2][2048]: I / Q after the IQ correction, before the Fs/4 shift (display FFT input)
  float *spect;            // audioSpectBuffer side output [nchan][nframes][1024] (or null)
  float *spect_max;        // [nchan][nframes][3]: audioMaxSquared, AudioMaxIndex, audioMaxSquaredAve
  // FFT_LENGTH 4096 pipeline scratch (device, owned by the context)
  float *mid;              // [nchan][nseg * 256] complex: /8-decimated, level-adjusted I/Q
  float *aud24;            // [nchan][nseg * 256] real: filtered audio @24 kS/s
  const float2 *tab4k;     // tw4096[7][512] | mask4096[8][512] (see kTab4k*)
  int nframes4k;           // number of long frames (= nframes / seg for the part kernels)
  int seg;                 // 2048-sample segments per frame = fft_length / 512 (1 for the fused 512 kernel)
  int plain;               // 1: unit band/IQ gains and zero IQ phase correction -> specialised kernel
  int agc;                 // 1: AGCMode != 0 (look-ahead AGC, DSP_Fn.cpp:504-631)
  // the gains of the first stage, by value: a kernel argument is one scalar-load round trip away
  // at kernel start, a field behind `coef` is two
  float g_rf;              // sc[kScRfGain]
  float g_band;            // sc[kScBandGain]
  float neg_iq_amp;        // sc[kScNegIqAmp]
  float iq_phase;          // sc[kScIqPhase]
  int iq_corr_on;          // sc[kScIqCorrOn] != 0
  int q15;                 // 1: I, Q, out point at int16 (q15) samples instead of f32 (Process.cpp:102-111, 936)
  int nfm_atan;            // NFM: 1 = atan2 discriminator + block-wise de-emphasis (t41rx_params::nfm_demod)
  int seg_run;             // long FFT, segment-parallel kernels: consecutive segments one wave runs
  int ovl_real;            // long FFT, NFM: the overlap block is real (Process.cpp:765-816) -- its imaginary half, last_sample_buffer_R,
                           // is read as zero and left as the last complex mode wrote it
  int nco_rd;              // long FFT: which of the two NcoState copies holds the call's start state (the other is written)
  // noise reduction / notch pipeline (FFT_LENGTH 512, tap kernels): when set, the fused kernel stops behind the
  // demodulator and leaves the frame's 256 audio samples @24 kS/s here, [nchan][nframes * 256] in time order;
  // nr_kernels.hip then runs Process.cpp:841-866 on them in place and launch_back512() interpolates (aud24 = this)
  float *aud_out;
  // AGC on, pipelined kernel (rx_chains.hpp: agc_prep_pipe): per channel three slots of 1024 floats -- the serial
  // chain's operands and results and the samples the gain is applied to, for the frames in flight (or null: barrier form)
  float *agc_pipe;
  // receiver groups (t41rx_set_input_map), or null: channel c reads row in_map[c] of I / Q, whose (row, frame) starts at
  // in_map[c] * in_chan_stride + f * in_frame_stride samples; chan_stride / frame_stride then place the output alone.
  // The host has checked every entry against the number of rows.  Only the mapped instantiations read these fields.
  const int *__restrict__ in_map;
  long long in_chan_stride;
  long long in_frame_stride;
  // the panadapter stage's update cadence (t41rx_set_panadapter), or tap_period == 0: every frame writes its own row of
  // dbg_pre / spect / spect_max, [nchan][nframes].  tap_period > 0: the call's frames tap_first + k tap_period (k >= 0)
  // are its update frames and write the compact row k of [nchan][tap_rows]; every other frame writes no tap and does not
  // advance audioMaxSquaredAve.  By value, so a device-pointer call uploads nothing: the host has worked out tap_first
  // from its frame counter and checked the row count against tap_rows.  Only the tap instantiations read these fields.
  int tap_period;
  int tap_first;
  int tap_rows;
  // parameter sets (t41rx_set_param_sets), or null: channel c runs with set set_of[c] -- coefficient block coef[set],
  // constant table tab + set * kTabEntries512 (the mask and the AM scan constants; every other part is the same in all
  // of them and is read from set 0's) and the first stage's gains set_gain[set] in place of the five words above.  The
  // host has checked every entry against the number of sets.  Only the set instantiations read these fields; a call
  // with sets always carries in_map too (an identity map when the caller set none).
  const int *__restrict__ set_of;
  const SetGains *__restrict__ set_gain;
  // the output map (t41rx_set_output_map), or null: channel c stores its audio to row out_map[c] of `out`, whose (row,
  // frame) starts at out_map[c] * chan_stride + f * frame_stride samples, or with out_map[c] < 0 stores none and leaves
  // its interpolator memories alone.  The host has checked every entry against the number of rows and that no row is
  // named twice.  Only the output-map instantiations read this field.
  const int *__restrict__ out_map;
  // the panadapter map (t41rx_set_panadapter_map), or null: with tap_period > 0 channel c writes the update frames' rows of
  // dbg_pre / spect / spect_max to row tap_map[c] of [n_rows][tap_rows] -- the row takes the channel's place in the three
  // tap addresses and nothing else changes -- or, with tap_map[c] < 0, writes no tap in any frame and leaves
  // audioMaxSquaredAve alone.  The host has checked every entry against the number of rows and that no row is named
  // twice.  Only the tap instantiations read this field.
  const int32_t *tap_map;
};

// constant table of the N = 512 R point fast convolution (float2 units):
//   tw  [R-1][512] : W_N^(k' q), q = 1..R-1, k' < 512 (forward sign)
//   mask[R][512]   : FIR_filter_mask[q + R m] / N at [q][m]
constexpr int tab_long_entries(int R) { return (R - 1) * 512 + R * 512; }

// the front of the call's plan (rx_plan.hpp): the fused kernel, the tap kernel, or the long-FFT pipeline.  With
// p.form.a24_form a.chan_stride / a.frame_stride place frames of 256 output samples (the input's strides are then
// a.in_chan_stride / a.in_frame_stride: the call carries a map); with p.handover the caller finishes from a.aud_out
hipError_t launch_rx(const RxArgs &a, const CallPlan &p, hipStream_t s);
// what the kernel objects of this library were built as (rx_experiments.hpp; rx_dispatch.hip: the OR of every object's
// own answer): 0 = the product, bit 1 = a diagnostic build (stamps / counters)
int kernel_build_flags();
// FFT_LENGTH 512, behind launch_rx() with aud_out set: interpolators, volume and stores from a.aud24 (f32 or q15 samples out)
hipError_t launch_back512(const RxArgs &a, hipStream_t s);

// The audio @24 kS/s as the call's result, behind the tap kernels and the chain-splitting stages (aud24_kernel.hip) in
// place of launch_back512() / the CW path's interpolators: out = aud * g (one f32 multiply, Process.cpp:929 without DF),
// arm_float_to_q15 for the q15 entries, in the call's layout.  The interpolator memories are not touched.
struct Aud24Args {
  const float *aud;        // [nchan][nframes * 256], time order (RxArgs::aud_out)
  void *out;               // f32 or q15 samples, frames of 256
  long long chan_stride;   // where (channel c, frame f) of out starts, in samples: c * chan_stride + f * frame_stride
  long long frame_stride;
  int nchan, nframes;
  int q15;
  // g = coef[set_of ? set_of[c] : 0].sc[kScOutScale] / DF: the context's block, or with parameter sets the channel's own set's
  const DevCoef *coef;
  const int *set_of;
  // the output map, or null: channel c's frames go to row out_map[c] of out, or with out_map[c] < 0 nowhere
  const int *out_map;
};
hipError_t launch_aud24_finish(const Aud24Args &a, hipStream_t s);

// display FFT (CalcZoom1Magn / ZoomFFTExe, FFT.cpp:67-251) on the dbg_pre tap of the frames just processed
struct DispArgs {
  const float *pre;        // RxArgs::dbg_pre
  float *disp;             // [nchan][kDispFloats] display state
  float *spec;             // [nchan][nframes][512] FFT_spec
  float *spec_old;         // [nchan][nframes][512] FFT_spec_old
  const float2 *tab;       // the context's constant table (FFT twiddles)
  const double *win;       // [512]: 0.5 - 0.5 cos(6.28 i / 512), as the reference's double expression
  float iir[20];           // mag_coeffs[spectrumZoom] (unused for zoom 0)
  float fir[4];            // Fir_Zoom_FFT_Decimate_coeffs
  int nchan, nframes, zoom;
};
hipError_t launch_display(const DispArgs &a, hipStream_t s);

// IQ calibration, receive half and measurement (ProcessIQData2() / PlotCalSpectrum(), Process2.cpp:352-397, 478-547)
struct CalArgs {
  const void *I;           // float_buffer_L's source: f32, or the R queue's q15 samples (Process2.cpp:359)
  const void *Q;           // float_buffer_R's: f32, or the L queue's
  const uint8_t *update;   // [nframes] updateDisplayFlag per frame, shared by all channels; null = every frame 1
  float *result;           // [nchan][nframes][3]: refAmplitude, adjAmplitude, adjdB
  int16_t *pixel;          // [nchan][nframes][512] pixelnew, rows of update frames only (or null)
  float *spec;             // [nchan][nframes][512] FFT_spec, rows of update frames only (or null)
  float *cal;              // [nchan][kCalFloats] calibration memory
  const float2 *tab;       // the context's constant table (FFT twiddles)
  const double *win;       // [512]: 0.5 - 0.5 cos(6.28 i / 512)
  const float *corr;       // [nchan][2] = IQAmp, IQPhase per channel; null = iq_amp / iq_phase for all
  float iir[20];           // mag_coeffs[spectrumZoom] (unused for zoom 0)
  float fir[4];            // Fir_Zoom_FFT_Decimate_coeffs
  long long chan_stride;   // samples between two channels' input; 0 = every channel reads the same recording
  int nchan, nframes, zoom, q15;
  float g_rf;              // (float)pow(10, rfGainAllBands / 20), Process2.cpp:365
  float rec_band;          // recBandFactor[currentBand] = 1.0, :372-373
  float iq_amp, iq_phase;  // IQAmpCorrectionFactor (I is scaled by its negative, :377, 381), IQPhaseCorrectionFactor
  int corr_on;             // LSB or USB
  float dBScale;           // displayScale[currentScale].dBScale
  int base;                // displayScale[currentScale].baseOffset + pixel_offset
  int lo0, lo1, width;     // the windows [bin0 - capture, bin0 + capture), [bin1 - capture, bin1 + capture)
  int sideband;            // 1 LSB (ref = window 0), 2 USB (ref = window 1), 0 any other mode (no measurement)
};
hipError_t launch_cal(const CalArgs &a, hipStream_t s);

// the panadapter stage (t41rx_set_panadapter; panadapter_kernel.hip): display FFT, ShowSpectrum()'s pixel mapping and
// waterfall row and DrawSmeterBar()'s dBm on the compact tap rows of a call's update frames
struct PanArgs {
  const float *pre;             // RxArgs::dbg_pre, compact: [nchan][max_rows][2][2048]
  const float *mx;              // RxArgs::spect_max, compact: [nchan][max_rows][3]
  float *mem;                   // [nchan][kPanFloats] panadapter memory
  const float2 *tab;            // the context's constant table (FFT twiddles)
  const double *win;            // [512]: 0.5 - 0.5 cos(6.28 i / 512)
  const uint16_t *gradient;     // [kPanGradient]
  const int32_t *noise_floor;   // [nchan] currentNoiseFloor[currentBand]
  const float *gain_correction; // [nchan] bands[currentBand].gainCorrection
  // the caller's rows [nchan][max_rows][...], each may be null
  int16_t *pixel, *y_new, *y_old;  // [512]
  uint16_t *waterfall;             // [512]
  float *spec;                     // [512] FFT_spec
  float *smeter;                   // [4]: audioMaxSquared, AudioMaxIndex, audioMaxSquaredAve, dbm
  float iir[20];                // mag_coeffs[spectrumZoom] (unused for zoom 0)
  float fir[4];                 // Fir_Zoom_FFT_Decimate_coeffs
  int nchan, nrows, max_rows, zoom;
  float dBScale;                // displayScale[currentScale].dBScale
  int base;                     // displayScale[currentScale].baseOffset + pixel_offset
  int noise_floor_y;            // spectrumNoiseFloor
  int attenuator, RFgain, rfGainAllBands;  // DrawSmeterBar()'s integers (Display.cpp:980-981)
};
hipError_t launch_panadapter(const PanArgs &a, hipStream_t s);
// the list form under a panadapter map (t41rx_set_panadapter_map; rx_panmap.hpp): a wave per entry of `list`, which
// indexes mem, noise_floor and gain_correction by the entry's channel, pre, mx and the caller's rows by its row, and takes
// RFgain / rfGainAllBands from the entry (the two members here are not read).  PanArgs' members in PanArgs' order
// (panadapter_kernel.inc is one text for both), then the list.  An empty list is not launched.
struct PanListArgs {
  const float *pre;             // [rows][max_rows][2][2048]
  const float *mx;              // [rows][max_rows][3]
  float *mem;                   // [nchan][kPanFloats]
  const float2 *tab;
  const double *win;
  const uint16_t *gradient;
  const int32_t *noise_floor;   // [nchan]
  const float *gain_correction; // [nchan]
  // the caller's rows [rows][max_rows][...], each may be null
  int16_t *pixel, *y_new, *y_old;
  uint16_t *waterfall;
  float *spec;
  float *smeter;
  float iir[20];
  float fir[4];
  int nchan, nrows, max_rows, zoom;
  float dBScale;
  int base;
  int noise_floor_y;
  int attenuator, RFgain, rfGainAllBands;
  const PanEntry *list;         // [nlist] (device), ascending by channel, no row twice
  int nlist;                    // 1 .. nchan: the grid
};
hipError_t launch_panadapter_list(const PanListArgs &a, hipStream_t s);

}  // namespace t41
