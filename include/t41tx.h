/* include/t41tx.h -- C ABI of the MI355X-native T41 transmit exciter (the TX mirror of t41rx.h).
 *
 * Drop-in boundary for the reference's
 *     void ExciterIQData();        (software/T41_SDR/Exciter.cpp:46-169)
 * which turns one frame of microphone samples (16 blocks of 128 q15 samples per AudioRecordQueue,
 * Q_in_L_Ex / Q_in_R_Ex, 192 kS/s) into the I and Q drive of the SSB exciter (Q_out_L_Ex /
 * Q_out_R_Ex, q15, 192 kS/s): decimate by 4 (48 taps, coeffs192K_10K_LPF_FIR) and by 2 (24 taps,
 * coeffs48K_8K_LPF_FIR), two 100-tap Hilbert FIRs (+45 / -45 degrees), the TX IQ amplitude / phase
 * correction, interpolate by 2 (48 taps) and by 4 (32 taps) per channel, x 20, arm_float_to_q15.
 * The globals it reads become t41tx_params; its static CMSIS instance states (T41_SDR.ino:278-299)
 * become per-channel state owned by the context.  Citations: software/T41_SDR/ of the reference.
 * The transmit equaliser (xmitEQFlag, DoExciterEQ(), Filter.cpp:176-224) is restated as an optional stage between the
 * decimators and the Hilbert pair, off by default like the firmware's; its switch, levels and band table are context
 * switches below, not t41tx_params fields.
 * The CW exciter, void CW_ExciterIQData(); (CW_Excite.cpp:66-118), is the second entry of the same context
 * (t41tx_set_cw_tone, t41tx_process_cw_*_q15 below): a stored tone, the TX IQ correction with CW's signs, and the
 * same two interpolators per channel.  Not restated: the data exciter.
 * The transmit half of the IQ calibration, ProcessIQData2() (Process2.cpp:309-349), is the third entry
 * (t41tx_set_cal_tone, t41tx_set_cal_corrections, t41tx_process_cal_*_q15 below); its receive half and the sideband
 * measurement are t41rx_calibrate_* in t41rx.h.
 */
#ifndef T41TX_H
#define T41TX_H
#include <stddef.h>
#include <stdint.h>

#ifndef T41RX_API /* exported entry point (see t41rx.h) */
#if defined(__GNUC__) || defined(__clang__)
#define T41RX_API __attribute__((visibility("default")))
#else
#define T41RX_API
#endif
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* status codes and mode numbers are t41rx.h's (T41RX_OK, T41RX_ERR_*, T41RX_DEMOD_*) */
/* t41rx_last_error() (t41rx.h) also returns the message of the calling thread's last failed t41tx_* call */

typedef struct t41tx_params {
  int32_t mode;                     /* bands[currentBand].mode: LSB / USB select the sign of the I scaling (Exciter.cpp:117-126) */
  float   IQXAmpCorrectionFactor;   /* IQXAmpCorrectionFactor[currentBandA], gwv.cpp:73 */
  float   IQXPhaseCorrectionFactor; /* IQXPhaseCorrectionFactor[currentBandA], gwv.cpp:74 */
} t41tx_params;

typedef struct t41tx_ctx t41tx_ctx;

T41RX_API void t41tx_default_params(t41tx_params *p);             /* USB, 1, 0 (gwv.cpp:73-74) */
/* SetupMode() for transmit: allocate n_channels exciters on HIP device device_id, filter states cleared */
T41RX_API int t41tx_create(t41tx_ctx **out, int device_id, int n_channels, const t41tx_params *p);
T41RX_API int t41tx_destroy(t41tx_ctx *ctx);
T41RX_API int t41tx_set_params(t41tx_ctx *ctx, const t41tx_params *p);  /* states are kept, like the firmware's */
T41RX_API int t41tx_reset(t41tx_ctx *ctx);                               /* all CMSIS instance states to zero */
T41RX_API int t41tx_n_channels(const t41tx_ctx *ctx);

/* The transmit equaliser (Exciter.cpp:94-98): 14 bands of 4 cascaded arm_biquad_cascade_df2T_f32 sections on the frame's
 * 256 samples @24 kS/s, each band's output times its level (negated for bands 1, 3, .., 13), the 14 products summed
 * as EQ1 + EQ2, + EQ3, .., + EQ14, in place, before the copy L -> R: both Hilbert filters see equalised samples.
 * t41tx_set_transmit_eq_bands(): the firmware's EQ_Band1Coeffs .. EQ_Band14Coeffs (the S1_Xmt .. S14_Xmt instances
 *   point at the receive equaliser's tables, Filter.cpp:89-102) as [14][4][5] floats, {b0, b1, b2, a1, a2} per section
 *   with the a's negated (CMSIS DF2T order).  The library has no table of its own: it must be loaded before the
 *   equaliser can be switched on.  T41RX_ERR_ARG for NULL or a non-finite value.  Kept across t41tx_set_params(); a new
 *   table takes effect from the next process call and does not reset the filter memories.
 * t41tx_set_transmit_eq(): xmitEQFlag 0 or 1 (T41RX_ERR_ARG otherwise, and for 1 before a band table is loaded).
 *   equalizerXmt = EEPROMData.equalizerXmt[14], or NULL to keep the current levels; they start at the firmware's
 *   {0, 0, 100, 100, 100, 100, 100, 100, 100, 100, 100, 0, 0, 0} (gwv.cpp:50).  Any int is taken as the firmware would
 *   hold it.  As written in the reference: DoExciterEQ() stores (float)level / 100.0 into an int array
 *   (Filter.cpp:178, gwv.h:44), so a level counts in whole hundreds, truncated toward zero -- 99 -> 0, 100 and 199 -> 1,
 *   200 -> 2, -50 -> 0, -100 -> -1.  Switch and levels are kept across t41tx_set_params().
 * The memories xmt_EQ_Band1_state .. xmt_EQ_Band14_state (112 floats per channel, Filter.cpp:74-87) start at zero and
 * change only while the equaliser runs (all 14 cascades advance then, even where a level is 0): switched off and on
 * again they are stale, as in the reference.  t41tx_reset() zeroes them. */
T41RX_API int t41tx_set_transmit_eq_bands(t41tx_ctx *ctx, const float *coeffs);
T41RX_API int t41tx_set_transmit_eq(t41tx_ctx *ctx, int xmitEQFlag, const int32_t *equalizerXmt);
/* 0 / 1, or T41RX_ERR_ARG for a NULL context; the 14 levels into equalizerXmt_out unless it is NULL */
T41RX_API int t41tx_get_transmit_eq(const t41tx_ctx *ctx, int32_t *equalizerXmt_out);

/* Checkpoint of every channel's memories: 8 int32 words
 *     [0] magic "T41X"  [1] T41RX_ABI_VERSION  [2] n_channels  [3] floats per channel record  [4..7] reserved, zero
 * then n_channels records of that many floats: the delay lines of every FIR and the equaliser's 112 floats, always
 * present, so t41tx_state_bytes() is fixed for a context (0 for a NULL one).  t41tx_get_state() synchronises the device
 * first (T41RX_ERR_STATE for a buffer smaller than t41tx_state_bytes()).  t41tx_set_state() refuses (T41RX_ERR_STATE)
 * another magic, ABI, channel count, record size or byte count and any non-finite float, and then changes nothing.
 * The equaliser's switch, levels and band table are configuration, not state: a checkpoint does not carry them. */
T41RX_API size_t t41tx_state_bytes(const t41tx_ctx *ctx);
T41RX_API int    t41tx_get_state(t41tx_ctx *ctx, void *host_buf, size_t bytes);
T41RX_API int    t41tx_set_state(t41tx_ctx *ctx, const void *host_buf, size_t bytes);

/* ExciterIQData() on every channel, n_frames consecutive frames of 2048 samples per queue.
 * Device pointers, [n_channels][n_frames * 2048] int16 each; dQ_in_R_Ex may be NULL: the firmware
 * decimates that queue and then overwrites the result with a copy of the L channel
 * (Exciter.cpp:98), so its samples never reach the output.  Enqueued on hip_stream, no sync. */
T41RX_API int t41tx_process_device_q15(t41tx_ctx *ctx, const int16_t *dQ_in_L_Ex, const int16_t *dQ_in_R_Ex,
                             int16_t *dQ_out_L_Ex, int16_t *dQ_out_R_Ex, int n_frames, void *hip_stream);
/* host-pointer form: copies in, runs the same kernel, copies out, synchronises */
T41RX_API int t41tx_process_host_q15(t41tx_ctx *ctx, const int16_t *Q_in_L_Ex, const int16_t *Q_in_R_Ex,
                           int16_t *Q_out_L_Ex, int16_t *Q_out_R_Ex, int n_frames);

/* CW transmit: CW_ExciterIQData() (CW_Excite.cpp:66-118).  Per frame: cosBuffer2 / sinBuffer2 (256 samples @24 kS/s) times
 * (float)0.127 into I / Q; in LSB I times -IQXAmpCorrectionFactor, in USB times +IQXAmpCorrectionFactor (the opposite of
 * ExciterIQData()'s signs), then IQPhaseCorrection() (Utility.cpp:178-187), in any other mode no correction; x2 (48 taps)
 * and x4 (32 taps) per channel, x 20, arm_float_to_q15: 2048 q15 I and 2048 q15 Q @192 kS/s.
 * Shared memories: the firmware's CW exciter drives the SSB exciter's own CMSIS instances FIR_int1_EX_I / Q and
 * FIR_int2_EX_I / Q, and so does this one: a CW call continues from the interpolator memories the last call of either
 * kind left (the first CW frame after SSB frames differs from a cold one, and the other way round), t41tx_reset() and
 * the checkpoint cover them, and the record size is unchanged.  A CW call touches no other memory: the decimators',
 * the Hilbert pair's and the equaliser's stay as they were, and the equaliser's switch does not apply.
 * t41tx_set_cw_tone(): cosBuffer2 and sinBuffer2, 256 floats each, as sineTone() fills them (Utility.cpp:66-83: numCycles
 *   = 8 is 750 Hz).  The firmware computes them with its own libm, so the library has no table of its own: one must be
 *   loaded before a CW call.  T41RX_ERR_ARG for NULL or a non-finite value; any finite value is taken, and an oversized
 *   table saturates in arm_float_to_q15 as the firmware's would.  Configuration: kept across t41tx_set_params() and
 *   t41tx_reset(), not part of a checkpoint; a new table takes effect from the next call.
 * The key.  The firmware runs the exciter continuously in the CW transmit states and keys by switching the output
 *   mixers modeSelectOutExL / R between gain 0 and on (T41_SDR.ino:1193-1289); a mixer gain takes effect at an audio-block
 *   boundary, 128 samples.  d_key holds one byte per block, 16 per frame, [n_channels][n_frames * 16]: nonzero passes
 *   the block of both outputs, zero writes zeros; NULL passes every block.  The gate sits behind arm_float_to_q15 and
 *   the interpolator memories advance whether a block is gated or not.  powerOutCW[] and the sidetone stay with the caller.
 * t41tx_process_cw_device_q15(): n_frames consecutive frames on every channel.  Device pointers; the outputs are
 *   [n_channels][n_frames * 2048] int16 each, 16-byte aligned.  Enqueued on hip_stream, no sync.  T41RX_ERR_ARG before
 *   a tone table is loaded, for n_frames <= 0 and for NULL or misaligned outputs. */
T41RX_API int t41tx_set_cw_tone(t41tx_ctx *ctx, const float *cosBuffer2, const float *sinBuffer2);
T41RX_API int t41tx_process_cw_device_q15(t41tx_ctx *ctx, const uint8_t *d_key, int16_t *dQ_out_L_Ex, int16_t *dQ_out_R_Ex,
                                int n_frames, void *hip_stream);
/* host-pointer form: copies the key in (it shares the staging buffers of t41tx_process_host_q15), runs the same kernel,
 * copies out, synchronises */
T41RX_API int t41tx_process_cw_host_q15(t41tx_ctx *ctx, const uint8_t *key, int16_t *Q_out_L_Ex, int16_t *Q_out_R_Ex,
                              int n_frames);

/* IQ calibration, transmit half: what ProcessIQData2() plays (Process2.cpp:309-349).  Per frame: cosBuffer3 / sinBuffer3
 * (256 samples @24 kS/s, 3000 Hz, Utility.cpp:78-80) times level into I / Q; in LSB I times -IQXAmpCorrectionFactor, in USB
 * times +IQXAmpCorrectionFactor (ProcessIQData2()'s signs, :317-325: the CW exciter's, not ExciterIQData()'s), then
 * IQPhaseCorrection(), in any other mode no correction; x2 (48 taps) and x4 (32 taps) per channel; arm_float_to_q15
 * straight from the interpolators (:344-345): no x 20 and no key.  The interpolators are the SSB exciter's own instances
 * FIR_int1_EX_I / Q and FIR_int2_EX_I / Q: a calibration call continues from the memories the last SSB, CW or calibration
 * call left, t41tx_reset() and the checkpoint cover them, the record size is unchanged, and no other memory is touched.
 * t41tx_set_cal_tone(): cosBuffer3 and sinBuffer3, 256 floats each, and level = the firmware's bandOutputFactor
 *   (Process2.cpp:309; the caller computes it, CWPowerCalibrationFactor[] stays with the caller).  The library has no
 *   table of its own: one must be loaded before a calibration call.  T41RX_ERR_ARG for NULL or a non-finite value.
 *   Configuration: kept across t41tx_set_params() and t41tx_reset(), not part of a checkpoint.
 * t41tx_set_cal_corrections(): one (amplitude, phase) candidate per channel, host arrays of n_channels floats, copied
 *   (synchronises).  Both NULL: every channel uses the params' IQXAmpCorrectionFactor / IQXPhaseCorrectionFactor, the
 *   state of a new context.  One NULL, or a non-finite value: T41RX_ERR_ARG, and the candidates stay as they were.
 *   They apply to the calibration calls only.  Configuration, like the tone.
 * t41tx_process_cal_device_q15(): n_frames consecutive frames on every channel.  Device pointers; the outputs are
 *   [n_channels][n_frames * 2048] int16 each, 16-byte aligned.  Enqueued on hip_stream, no sync.  T41RX_ERR_ARG before
 *   a tone table is loaded, for n_frames <= 0 and for NULL or misaligned outputs. */
T41RX_API int t41tx_set_cal_tone(t41tx_ctx *ctx, const float *cosBuffer3, const float *sinBuffer3, float level);
T41RX_API int t41tx_set_cal_corrections(t41tx_ctx *ctx, const float *amp, const float *phase);
T41RX_API int t41tx_process_cal_device_q15(t41tx_ctx *ctx, int16_t *dQ_out_L_Ex, int16_t *dQ_out_R_Ex, int n_frames,
                                 void *hip_stream);
/* host-pointer form: runs the same kernel into the staging buffers of t41tx_process_host_q15, copies out, synchronises */
T41RX_API int t41tx_process_cal_host_q15(t41tx_ctx *ctx, int16_t *Q_out_L_Ex, int16_t *Q_out_R_Ex, int n_frames);

#ifdef __cplusplus
}
#endif
#endif /* T41TX_H */
