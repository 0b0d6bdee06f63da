/*
 * include/t41rx.h -- C ABI of the MI355X-native T41 receive DSP hot path.
 *
 * Drop-in boundary for tmr4/T41_SDR's `void ProcessIQData();` (Process.h:15, body
 * Process.cpp:70-944).  The reference function takes no arguments: it reads/writes firmware
 * globals.  Each entry point below names the reference global(s)/function it stands in for
 * (file:line relative to /root/reference/software/T41_SDR/).  Plain pointers and sizes only;
 * no C++/torch types cross this boundary.
 *
 * Data model: a context owns `n_channels` independent receive channels (the reference has
 * exactly one: its static globals).  One `t41rx_process_*` call = one ProcessIQData() call on
 * every channel (or `n_frames` consecutive calls), with all per-channel persistent state
 * (FIR delay lines, NCO phase, overlap-save block, DC-block state ...) kept in device memory.
 *
 * Buffers (the reference's float_buffer_L / float_buffer_R, T41_SDR.ino:375-376, after the
 * arm_q15_to_float conversion of Process.cpp:107-108, i.e. float_buffer_L = I, _R = Q):
 *   I, Q   : const float [n_channels][n_frames * frame_len]   planar f32, read-only
 *   audio  : float       [n_channels][n_frames * frame_len]   mono f32 @192 kS/s
 *            (= float_buffer_L just before arm_float_to_q15, Process.cpp:929-936; or, with
 *            t41rx_set_audio_rate(T41RX_AUDIO_RATE_24K), [n_channels][n_frames * 256] @24 kS/s:
 *            float_buffer_L in front of the interpolators, Process.cpp:917, times the volume)
 *   frame_len = BUFFER_SIZE * N_BLOCKS = 4 * fft_length  (2048 for FFT_LENGTH 512;
 *   SDT.h:39,70, T41_SDR.ino:368).
 *
 * Errors: the reference returns nothing and hangs in while(1) on init failure
 * (T41_SDR.ino:574-616).  Every function here returns an int status (0 = OK, <0 = error) and
 * never aborts.  There is NO CPU fallback: if the HIP device or kernels are unavailable the
 * call fails with T41RX_ERR_HIP.
 */
#ifndef T41RX_H
#define T41RX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T41RX_ABI_VERSION 5

/* The library is built with -fvisibility=hidden and an export list (t41_sdr_amd/csrc/exports.map): the entry points
 * declared here and in t41tx.h are its only dynamic symbols. */
#ifndef T41RX_API
#if defined(__GNUC__) || defined(__clang__)
#define T41RX_API __attribute__((visibility("default")))
#else
#define T41RX_API
#endif
#endif

/* status codes */
#define T41RX_OK 0
#define T41RX_ERR_ARG (-1)        /* bad argument (null pointer, size, range) */
#define T41RX_ERR_UNSUPPORTED (-2)/* valid in the reference but not built here */
#define T41RX_ERR_HIP (-3)        /* HIP runtime / device error; see t41rx_last_error() */
#define T41RX_ERR_NOMEM (-4)
#define T41RX_ERR_STATE (-5)      /* blob / state size or version mismatch */

/* demodulation modes: bands[currentBand].mode, SDT.h:58-68 */
#define T41RX_DEMOD_USB 0
#define T41RX_DEMOD_LSB 1
#define T41RX_DEMOD_AM 2
#define T41RX_DEMOD_NFM 3
#define T41RX_DEMOD_SAM 8 /* synchronous AM, AMDecodeSAM() Demod.cpp:40-139 (SDT.h:67); fft_length 512 */

/* xmtMode, SDT.h:48-50 (only affects the CW side-tone offset of the NCO, Freq_Shift.cpp:108-120) */
#define T41RX_SSB_MODE 0
#define T41RX_CW_MODE 1
#define T41RX_DATA_MODE 2

/* The firmware globals ProcessIQData() reads, gathered into one POD (SURVEY 8b "Parameters"). */
typedef struct t41rx_params {
  int32_t fft_length;              /* FFT_LENGTH, SDT.h:39. 512 = reference; see t41rx_supported_fft_length */
  int32_t mode;                    /* bands[currentBand].mode: T41RX_DEMOD_USB / LSB / AM / NFM / SAM (SDT.h:58-68) */
  int32_t FLoCut;                  /* bands[currentBand].FLoCut [Hz], SDT.h:186 */
  int32_t FHiCut;                  /* bands[currentBand].FHiCut [Hz], SDT.h:185 */
  int32_t rfGainAllBands;          /* gwv.cpp:17, Process.cpp:117 */
  int32_t RFgain;                  /* bands[currentBand].RFgain, Process.cpp:133 */
  float   IQAmpCorrectionFactor;   /* IQAmpCorrectionFactor[currentBand], gwv.cpp:71 */
  float   IQPhaseCorrectionFactor; /* IQPhaseCorrectionFactor[currentBand], gwv.cpp:72 */
  int32_t AGCMode;                 /* gwv.cpp:15; 0 = off (fixed_gain 20, DSP_Fn.cpp:494-502), 1..4 = long/slow/
                                      med/fast look-ahead AGC (DSP_Fn.cpp:373-402, 504-631) */
  int32_t audioVolume;             /* gwv.cpp:16, Process.cpp:929 */
  int32_t nfmFilterBW;             /* Filter.cpp:16, Process.cpp:259 */
  int32_t xmtMode;                 /* gwv.cpp:22 */
  int32_t CWFreqShift;             /* Freq_Shift.cpp:113-116 */
  int32_t am_lpf_f0;               /* cutoff biquad_lowpass1 was designed for at boot, T41_SDR.ino:560-566 */
  int32_t AGC_thresh;              /* bands[currentBand].AGC_thresh [dB], SDT.h:190, DSP_Fn.cpp:408 */
  int32_t nfm_demod;               /* NFM discriminator: 0 = nfmdemod() (quadri-correlator) + limiter, what the
                                      firmware runs (Process.cpp:716-727); 1 = the alternative its source keeps
                                      commented out: fmdemod_atan_cf (Demod.cpp:368-392, ApproxAtan2 :148-197 with its
                                      2 pi for pi / 2 as written) + limiter + deemphasis_nfm_ff applied block-wise
                                      (Demod.cpp:324-344, Process.cpp:734-735).  fft_length 512 only. */
  /* The optional stages between the demodulator and the interpolators, Process.cpp:841-866 (all off in the firmware's
   * defaults).  fft_length 512; the functions are written for blocks of 256 audio samples. */
  int32_t nrOptionSelect;          /* gwv.cpp:23: 0 off; 1 Kim1_NR() (Noise.cpp:108-313) then x30; 2 SpectralNoiseReduction()
                                      (Noise.cpp:379-655); 3 Xanr() as LMS noise reduction (Noise.cpp:322-370) then x1.5 --
                                      as written the call site scales Xanr()'s INPUT, so 3 only changes the gain (and advances
                                      the adaptive filter the notch shares) */
  int32_t ANR_notchOn;             /* Process.cpp:45, :862-866: 1 = Xanr() as automatic notch behind the noise reduction */
  float   NR_PSI;                  /* gwv.cpp:61 (0.0): Kim1_NR()'s noise-floor switch */
  float   NR_alpha;                /* gwv.cpp:62 (0.95): time smoothing of the gains (Kim, spectral) */
  float   NR_beta;                 /* gwv.cpp:63 (0.85): Kim1_NR()'s smoothing over neighbouring bins */
} t41rx_params;

typedef struct t41rx_ctx t41rx_ctx; /* opaque: coefficient arrays + per-channel state + device buffers */

/* ---- library ---- */
T41RX_API int         t41rx_abi_version(void);
T41RX_API const char *t41rx_strerror(int status);
T41RX_API const char *t41rx_last_error(void);          /* thread-local detail of the last failing call */
T41RX_API int         t41rx_supported_fft_length(int fft_length); /* 1 for 512, 1024, 2048, 4096 */

/* Defaults of gwv.cpp:14-96 / bands[] T41_SDR.ino:145-168 (20 m row: USB, 200..3000 Hz) with
 * AGCMode forced to 0. */
T41RX_API void t41rx_default_params(t41rx_params *p);

/* ---- coefficient design: host-side, no GPU needed ----
 * The arrays CalcFilters() (Filter.cpp:235-249), InitFilterMask() (Filter.cpp:260-284),
 * SetDecIntFilters() (Filter.cpp:396-438) and InitializeDataArrays() (T41_SDR.ino:560-566) leave
 * behind, serialised as one blob:
 *   header (32 x int32: magic, abi, fft_length, mode, sizeof(t41rx_params), 3 reserved, then the
 *   t41rx_params the blob was designed for, padded to 24 words) |
 *   FIR_dec1_coeffs[28] | FIR_dec2_coeffs[46] | FIR_int1_coeffs[48] | FIR_int2_coeffs[32] |
 *   biquad_lowpass1_coeffs[5] | scalars[16] (gains, level adjust, volume, the SAM PLL constants) | AGC constants[16] (what AGCPrep() +
 *   AGCLoadValues() leave behind, DSP_Fn.cpp:368-468; zeros for AGCMode 0) |
 *   FIR_filter_mask[2*fft_length]                                                (all f32)
 * This blob is what rank 0 broadcasts over RCCL after a filter change. */
T41RX_API size_t t41rx_coeff_blob_bytes(int fft_length);
T41RX_API int    t41rx_design_coeffs(const t41rx_params *p, void *blob, size_t blob_bytes);

/* ---- context ---- */
/* InitializeDataArrays() (T41_SDR.ino:473-667): allocate state for n_channels channels on HIP
 * device `device_id`, power-on state, design + upload coefficients for *p.
 * The environment is read here and by no other call.  T41RX_SEG_RUN=n is a test hook: the context's long-FFT calls run
 * their segment-parallel kernels with runs of n segments, and at fft_length 4096 the two-kernel pipeline where the
 * one-kernel form would run (the tests compare the two); set it before the context exists.  A library whose kernels were
 * built with diagnostics is refused (T41RX_ERR_UNSUPPORTED) unless T41RX_ALLOW_EXPERIMENT=1; only such a library reads
 * the diagnostics' own T41RX_PIPE_STAT and T41RX_STAMP_TAPS. */
T41RX_API int t41rx_create(t41rx_ctx **out, int device_id, int n_channels, const t41rx_params *p);
T41RX_API int t41rx_destroy(t41rx_ctx *ctx);

/* SetupMode()/CalcFilters() (Filter.cpp:235-249, 341-385): parameters changed between two
 * ProcessIQData() calls.  Coefficients are re-designed and uploaded; like the reference, the
 * streaming state (FIR delay lines etc.) is NOT reset.  fft_length cannot change. */
T41RX_API int t41rx_set_params(t41rx_ctx *ctx, const t41rx_params *p);
T41RX_API int t41rx_get_params(const t41rx_ctx *ctx, t41rx_params *p);

/* Coefficient blob of the context (see t41rx_design_coeffs).  set = install a blob designed
 * elsewhere (e.g. received by broadcast); it must match the context's fft_length.  The context
 * takes over the parameters stored in the blob (mode, AGCMode, cut-offs, gains ...), so afterwards
 * t41rx_get_params() returns the designer's and a later t41rx_set_params() starts from them. */
T41RX_API int t41rx_get_coeffs(const t41rx_ctx *ctx, void *blob, size_t blob_bytes);
T41RX_API int t41rx_set_coeffs(t41rx_ctx *ctx, const void *blob, size_t blob_bytes);

/* NCOFreq (T41_SDR.ino:131, Tune.cpp:141-196), one value per channel, host array of n_channels.
 * Phase-continuous: the oscillator state (Osc_Vect_Q/I, Freq_Shift.cpp:13-14) is kept. */
T41RX_API int t41rx_set_nco_freq(t41rx_ctx *ctx, const int32_t *nco_freq_hz, int n);

/* Power-on state: Osc_Vect_Q = 1, Osc_Vect_I = 0, all delay lines zero, first_block = 1
 * (Freq_Shift.cpp:13-14, Process.cpp:42,47). */
T41RX_API int t41rx_reset(t41rx_ctx *ctx);

/* NB_on (Process.cpp:873-876): 1 = the receive noise blanker NoiseBlanker() / AltNoiseBlanking() (DSP_Fn.cpp:105-362)
 * on the demodulated audio @24 kS/s, behind the noise reduction and the notch and in front of the interpolators: an
 * order-10 LPC fit per 256-sample block, a matched-filter detector at 2.5 x its spread, and 7 samples around each of up
 * to 20 detected impulses replaced by forward / backward linear prediction.  0 = off (the default; the firmware's
 * NB_on = 0).  Only 0 and 1 are accepted (T41RX_ERR_ARG otherwise); fft_length 512 only (T41RX_ERR_UNSUPPORTED for
 * NB_on = 1 at a long fft_length).  A context switch, not a t41rx_params field: it survives t41rx_set_params() and
 * t41rx_set_coeffs().  Its one memory, last_frame_end (the previous block's samples 242 .. 254), starts at zero,
 * changes only while the blanker runs (switched off and on again it is stale, as in the reference), is zeroed by
 * t41rx_reset() and travels in the checkpoint (section bit 2).  Takes effect from the next process call. */
T41RX_API int t41rx_set_noise_blanker(t41rx_ctx *ctx, int NB_on);
T41RX_API int t41rx_get_noise_blanker(const t41rx_ctx *ctx);  /* 0 / 1, or T41RX_ERR_ARG for a NULL context */

/* receiveEQFlag (Process.cpp:828-832): 1 = the receive equalizer DoReceiveEQ() (Filter.cpp:117-165) on the demodulated
 * audio @24 kS/s, in front of the noise reduction, the notch and the noise blanker (the audio spectrum / S-meter side
 * output is taken before it): 14 bands of 4 cascaded arm_biquad_cascade_df2T_f32 sections on the same input, band k's
 * output times -recEQ_LevelScale[k-1] for odd k and +recEQ_LevelScale[k-1] for even k, recEQ_LevelScale[i] =
 * (float)equalizerRec[i] / 100.0, summed EQ1 + EQ2, then + EQ3, .., + EQ14.  0 = off (the default).
 *
 * t41rx_set_receive_eq_bands(): the band table, coeffs[14][4][5] floats = the firmware's EQ_Band1Coeffs ..
 *   EQ_Band14Coeffs (FIR.cpp:279-370) concatenated, {b0, b1, b2, a1, a2} per section with the a's negated (CMSIS DF2T
 *   order).  The library has no table of its own: it must be loaded before the equalizer can be switched on.  T41RX_ERR_ARG
 *   for NULL or a non-finite value.  Kept across t41rx_set_params() and t41rx_set_coeffs(); a new table takes effect
 *   from the next process call and does not reset the filter memories (the firmware's tables are constant, so this has
 *   no reference counterpart).
 * t41rx_set_receive_eq(): receiveEQFlag 0 or 1 (T41RX_ERR_ARG otherwise; T41RX_ERR_UNSUPPORTED for 1 at a long
 *   fft_length; T41RX_ERR_ARG for 1 before a band table is loaded).  equalizerRec = EEPROMData.equalizerRec[14], or
 *   NULL to keep the current levels (100 each until set, EEPROM.cpp:59); any int is taken as the firmware would hold it.
 *   A context switch, not a t41rx_params field: switch and levels survive t41rx_set_params() and t41rx_set_coeffs().
 *   Takes effect from the next process call.
 * The filter memories (rec_EQ_Band1_state .. rec_EQ_Band14_state, Filter.cpp:43-56; 112 floats per channel) start at
 * zero, change only while the equalizer runs (switched off and on again they are stale, as in the reference), are
 * zeroed by t41rx_reset() and travel in the checkpoint (section bit 3). */
T41RX_API int t41rx_set_receive_eq_bands(t41rx_ctx *ctx, const float *coeffs);
T41RX_API int t41rx_set_receive_eq(t41rx_ctx *ctx, int receiveEQFlag, const int32_t *equalizerRec);
/* 0 / 1, or T41RX_ERR_ARG for a NULL context; the 14 levels into equalizerRec_out unless it is NULL */
T41RX_API int t41rx_get_receive_eq(const t41rx_ctx *ctx, int32_t *equalizerRec_out);

/* CW receive (Process.cpp:878-913): the block ProcessIQData() runs in T41State == CW_RECEIVE, on the audio @24 kS/s
 * behind the noise blanker and in front of the interpolators -- first the tone detector of DoCWReceiveProcessing()
 * (CWProcessing.cpp:322-373), then the narrow audio filter CWFilterIndex selects.  fft_length 512 only.
 *
 * Gating: both stages run only while t41rx_params.xmtMode == T41RX_CW_MODE.  That is the firmware's condition in
 * receive: loop() turns xmtMode == CW_MODE with the key up into radioState = CW_RECEIVE_STATE (T41_SDR.ino:1039-1040),
 * whose state machine sets T41State = CW_RECEIVE (T41_SDR.ino:1144-1148); xmtMode itself is the mode button's
 * (ButtonProc.cpp:324-354).  With any other xmtMode the settings below are kept, nothing runs, no memory advances and
 * d_cw is not written.
 *
 * t41rx_set_cw_tables(): audio_filters[5][6][5] = the firmware's CW_AudioFilterCoeffs1 .. 5 (FIR.cpp:15-65), {b0, b1,
 *   b2, a1, a2} per section in CMSIS DF2T order with the a's negated as the firmware stores them; decode_fir[64] =
 *   CW_Filter_Coeffs2 (FIR.cpp:93).  Either may be NULL to keep what is loaded.  The library has no table of its own.
 *   T41RX_ERR_ARG for a non-finite value (nothing is loaded then).  Kept across t41rx_set_params() / t41rx_set_coeffs();
 *   a new table takes effect from the next process call and resets no memory.
 * t41rx_set_cw_filter(): CWFilterIndex 0 .. 4 (0.8 / 1.0 / 1.3 / 1.8 / 2.0 kHz low-pass, six
 *   arm_biquad_cascade_df2T_f32 sections each, CWProcessing.cpp:36-48) or 5 = off (the default, as in the firmware);
 *   T41RX_ERR_ARG otherwise and for 0 .. 4 before the filter tables are loaded, T41RX_ERR_UNSUPPORTED for 0 .. 4 at a
 *   long fft_length.  Every index has its own memory: a filter switched away from and back resumes from its stale
 *   memory, as in the firmware.  While the filter runs, the interpolators and the volume behind it (Process.cpp:917-937)
 *   are computed in the firmware's own operations and order (no volume folded into the taps, no fused multiply-adds).
 *   t41rx_get_cw_filter(): the index, or T41RX_ERR_ARG for a NULL context.
 * t41rx_set_cw_detector(): decoderFlag 0 or 1 (T41RX_ERR_ARG otherwise).  With 1, every 256-sample block goes through
 *   the 64-tap decode FIR (arm_fir_f32), its full correlation with a 750 Hz sine (arm_correlate_f32, 511 lags; sinBuffer,
 *   Utility.cpp:72-74) and arm_max_f32 over the lags, and goertzel_mag() at 750 Hz (CWProcessing.cpp:830-857); d_cw, a
 *   device pointer [n_channels][n_frames][4] (n_frames of the process call), receives corrResultL, goertzelMagnitude,
 *   aveCorrResult and combinedCoeff = 10 * aveCorrResult * 100 * goertzelMagnitude of every frame.  aveCorrResult is
 *   (corrResultR + corrResultL) / 2 with corrResultR still the block before's (CWProcessing.cpp:339 runs before :348;
 *   0 at power-on).  The comparison `combinedCoeff > 50` (CWProcessing.cpp:365) and the Morse decoder behind it
 *   (DoCWDecoding()) are t41rx_set_cw_decoder()'s, below.  T41RX_ERR_ARG for 1 with a NULL d_cw, max_frames <= 0 or
 *   before decode_fir is loaded; T41RX_ERR_UNSUPPORTED for 1 at a long fft_length.  A process call with more than
 *   max_frames frames is refused (T41RX_ERR_ARG), as for the stage taps.  t41rx_get_cw_detector(): 0 / 1, or
 *   T41RX_ERR_ARG for a NULL context.
 * One audio stream: the library carries float_buffer_L only.  The filter reads L only; the detector reads L and R, so
 *   it is exact only while the stages in front of it leave them equal.  A process call with the detector running is
 *   refused (T41RX_ERR_UNSUPPORTED, t41rx_last_error() names the stage) when the receive equalizer (writes L only),
 *   nrOptionSelect 1 (x30 on L only) or 3 (Xanr() writes R, x1.5 on L only) is on and neither the notch nor the noise
 *   blanker (both end in R -> L) runs behind it.
 * Context switches, not t41rx_params fields: they survive t41rx_set_params() and t41rx_set_coeffs() and take effect
 * from the next process call.  The memories (5 x 12 biquad words, the FIR's 63-sample history, corrResultR,
 * aveCorrResultL / R; 128 floats per channel) start at zero, change only while their stage runs, are zeroed by
 * t41rx_reset() and travel in the checkpoint (section bit 4). */
T41RX_API int t41rx_set_cw_tables(t41rx_ctx *ctx, const float *audio_filters, const float *decode_fir);
T41RX_API int t41rx_set_cw_filter(t41rx_ctx *ctx, int CWFilterIndex);
T41RX_API int t41rx_get_cw_filter(const t41rx_ctx *ctx);
T41RX_API int t41rx_set_cw_detector(t41rx_ctx *ctx, int decoderFlag, float *d_cw, int max_frames);
T41RX_API int t41rx_get_cw_detector(const t41rx_ctx *ctx);

/* The Morse decoder: the rest of DoCWReceiveProcessing() behind the detector -- audioTemp = combinedCoeff > 50
 * (CWProcessing.cpp:365-371), DoCWDecoding() (:519-639) and its two adaptive histograms, DoGapHistogram() (:655-699) and
 * DoSignalHistogram() (:759-815) over JackClusteredArrayMax() (:719-745) -- one state machine per channel, on the
 * firmware's integer, float and double operations as written.  The display behind it (MorseCharacterDisplay(), the
 * scrolling decodeBuffer, the lock indicator, UpdateIBWPM()) stays with the caller.  fft_length 512 only.
 *
 * Gating: the decoder runs exactly when the detector runs and the decoder is switched on -- xmtMode == T41RX_CW_MODE,
 * t41rx_set_cw_detector(1) and t41rx_set_cw_decoder(1); in the firmware one decoderFlag gates both.  It reads the
 * detector's combinedCoeff of the call from d_cw.  Otherwise d_text is not written and no word of its state moves.
 *
 * What the firmware leaves open, decided here as in the restatement the kernel is held to (tests/cw_decode_model.py):
 *   The clock.  The firmware reads millis() several times inside one DoCWDecoding() call; here one value serves the
 *     whole frame: millis(n) = t0_ms + floor(n * num / den), the product in 64 bits, the sum kept to its low 32 bits as
 *     an int32.  n is the channel's count of decoder frames since power-on or t41rx_reset() (32 bits, unsigned; it
 *     travels in the checkpoint).  t41rx_set_cw_clock(): num >= 0, den > 0 (T41RX_ERR_ARG otherwise); the default is
 *     t0_ms = 0, num / den = 32 / 3 -- 2048 samples at 192 kS/s; it takes effect from the next process call and does
 *     not touch n.  `static long oldTime = millis()` runs on the first call: the frame with n == 0 starts by setting
 *     oldTime = millis(0).  signalStart and signalEnd start at 0.
 *   The arrays.  Both histograms live in 3072-word allotments (initCW(), :859-873) of which only words 0 .. 749 are
 *     ever cleared or scaled; gapHistogram[gapLen] is written for gapLen < 3 * thresholdGeometricMean, the clustered
 *     maximum of :688 scans up to word 3 * thresholdGeometricMean, :675 reads word 750.  From power-on both averages
 *     stay below 750 (only signals shorter than 750 ms enter them), so every index stays below 2304: 2304 words of
 *     gapHistogram and 768 of signalHistogram are carried per channel, zero at power-on, and every firmware access is an
 *     exact in-bounds access.  (A hand-made checkpoint may hold averages up to 32767 and so reach past the carried
 *     words: such a word reads 0 and is not written.)  The firstNonEmpty loop of :797-802 has no effect and is left out.
 *   Power-on.  The firmware's own is partly indeterminate (ditLength is not set before the first retune): the values
 *     ResetHistograms() (:501-517) leaves, zero / false for everything it does not touch, currentDashJump = 128.
 *   The tree.  bigMorseCodeTree (:540) is 129 characters; a byte index of 129 .. 255 reads past the literal in the
 *     firmware and prints '-' here, the tree's own filler.
 *
 * t41rx_set_cw_decode_tree(): the 129 bytes of bigMorseCodeTree; n must be 129 (T41RX_ERR_ARG otherwise and for NULL).
 *   The library has no table of its own.  Kept across t41rx_set_params() / t41rx_set_coeffs().
 * t41rx_set_cw_decoder(): on = 0 or 1 (T41RX_ERR_ARG otherwise).  With 1, d_text, a device pointer
 *   [n_channels][n_frames][2] of int32 (n_frames of the process call), receives per frame {the character the frame
 *   printed or 0, ditLength behind the frame}: a frame prints at most one character -- state 5 prints
 *   bigMorseCodeTree[currentDecoderIndex], state 6 prints ' '.  currentWPM = 1200 / ditLength is left to the caller.
 *   T41RX_ERR_ARG for 1 with a NULL d_text, max_frames <= 0 or before the tree is loaded; T41RX_ERR_UNSUPPORTED for 1 at
 *   a long fft_length.  A process call with more than max_frames frames is refused (T41RX_ERR_ARG).
 *   t41rx_get_cw_decoder(): 0 / 1, or T41RX_ERR_ARG for a NULL context.
 * t41rx_reset_cw_histograms(): ResetHistograms(), what the firmware runs at every retune (Encoders.cpp:119-121), on the
 *   channels whose byte in channels[n] is non-zero (n = n_channels; NULL = all channels): words 0 .. 749 of both
 *   histograms to zero, gapAtom = ditLength = aveDitLength = 80, gapChar = dahLength = aveDahLength = 240,
 *   thresholdGeometricMean = 160, valRef1 = valRef2 = 0 -- and nothing else: not the state machine, not n.
 * Context switches, not t41rx_params fields: tree, switch and clock survive t41rx_set_params() and t41rx_set_coeffs().
 * The decoder's words start at power-on, change only while it runs, return to power-on with t41rx_reset() and travel in
 * the checkpoint (section bit 5). */
T41RX_API int t41rx_set_cw_decode_tree(t41rx_ctx *ctx, const uint8_t *tree, int n);
T41RX_API int t41rx_set_cw_decoder(t41rx_ctx *ctx, int on, int32_t *d_text, int max_frames);
T41RX_API int t41rx_get_cw_decoder(const t41rx_ctx *ctx);
T41RX_API int t41rx_set_cw_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den);
T41RX_API int t41rx_reset_cw_histograms(t41rx_ctx *ctx, const uint8_t *channels, int n);

T41RX_API int t41rx_n_channels(const t41rx_ctx *ctx);
T41RX_API int t41rx_frame_len(const t41rx_ctx *ctx);

/* How the frames of one process call lie in I / Q / audio (f32 and q15 entry points alike).  The reference has one
 * channel and one frame per call (float_buffer_L/R[2048], T41_SDR.ino:375-376), so a batch of channels over several
 * frames has two natural shapes:
 *   T41RX_LAYOUT_CHANNEL_MAJOR (default)  [n_channels][n_frames * frame_len]: every channel's samples of the call
 *                                         contiguous in time (one long float_buffer per channel);
 *   T41RX_LAYOUT_TIME_MAJOR               [n_frames][n_channels][frame_len]: the [n_channels][frame_len] buffers of
 *                                         n_frames consecutive single-frame calls stacked as they arrive, one batch of
 *                                         frames every 10.67 ms (ABI 5).
 * Same arithmetic, same results, same state either way: only the addresses of (channel, frame) differ.  The side
 * outputs and stage taps keep their documented [n_channels][n_frames][...] shapes.  fft_length 512 only for the
 * time-major layout (T41RX_ERR_UNSUPPORTED otherwise; a later set_params to a long fft_length is refused likewise). */
#define T41RX_LAYOUT_CHANNEL_MAJOR 0
#define T41RX_LAYOUT_TIME_MAJOR 1
T41RX_API int t41rx_set_buffer_layout(t41rx_ctx *ctx, int layout);
T41RX_API int t41rx_get_buffer_layout(const t41rx_ctx *ctx);

/* ---- audio at 24 kS/s: the receive chain without its interpolators (ABI 5) ----
 * The firmware interpolates the finished audio x2 and x4 (Process.cpp:917-920) because the Teensy's DAC runs at 192 kS/s.
 * A caller that streams, records or decodes the audio wants the 24 kS/s the demodulator works at, and takes it here.
 *   T41RX_AUDIO_RATE_192K (default)  every process entry writes frame_len samples per channel and frame, as documented
 *                                    with the entries;
 *   T41RX_AUDIO_RATE_24K             every process entry -- device and host, f32 and q15, both buffer layouts, with or
 *                                    without an input map and parameter sets -- writes 256 samples per channel and frame:
 *                                    channel-major [n_channels][n_frames * 256], time-major [n_frames][n_channels][256].
 *                                    The inputs keep their frames of frame_len samples.
 * Sample i of a frame is float_buffer_L[i] as it stands in front of Process.cpp:917 -- behind the demodulator, the AGC and
 * every optional stage that is on (equaliser, noise reduction, notch, blanker, CW filter) -- multiplied once, as an f32
 * multiply of its own, by g = VolumeToAmplification(audioVolume) (Process.cpp:955-967): Process.cpp:929's factor without
 * DF, which only makes up for the interpolators' zero stuffing.  With parameter sets g is the channel's own set's.  The
 * q15 entries convert with the arm_float_to_q15 the 192 kS/s q15 output goes through (Process.cpp:936).
 * The interpolator memories are neither read nor written at 24 kS/s: after a switch back to 192 kS/s the interpolators
 * continue from what they last held, as the firmware's statics would if lines 917-920 were skipped meanwhile (the first
 * frames' worth of their impulse responses, 24 + 8 samples of history, then belong to older audio).  t41rx_state_bytes(),
 * the checkpoint layout and every section are the same at either rate; every other memory, side output, stage tap and
 * stage (FT8, audio spectrum, display spectrum, panadapter, beacon monitor, CW detector and decoder) computes and
 * holds what it does at 192 kS/s.
 * The rate is configuration, like the buffer layout: in no checkpoint, kept across t41rx_reset / t41rx_set_state /
 * t41rx_set_params, and it may change between any two calls.  fft_length 512 only: at a long fft_length
 * T41RX_AUDIO_RATE_24K is refused with T41RX_ERR_UNSUPPORTED (the long-FFT pipeline's back kernel interpolates); an
 * unknown rate is T41RX_ERR_ARG; a refused call leaves the rate as it was.
 * t41rx_audio_frame_len(): samples per channel and frame the process entries write at the current rate, frame_len or 256
 * (t41rx_frame_len() stays the input frame). */
#define T41RX_AUDIO_RATE_192K 0
#define T41RX_AUDIO_RATE_24K 1
T41RX_API int t41rx_set_audio_rate(t41rx_ctx *ctx, int rate);
T41RX_API int t41rx_get_audio_rate(const t41rx_ctx *ctx);
T41RX_API int t41rx_audio_frame_len(const t41rx_ctx *ctx);

/* ---- receiver groups: many channels on one shared I/Q stream (ABI 5) ----
 * One radio delivers one 192 kS/s stream and the channels of a context are the receivers tuned across it (NCOFreq per
 * channel, t41rx_set_nco_freq).  With an input map set, channel c reads row stream_of_channel[c] of I / Q, and I / Q
 * (Q_in_R / Q_in_L) of every process call hold n_streams rows instead of n_channels:
 *   channel-major  in  [n_streams][n_frames * frame_len]      out [n_channels][n_frames * frame_len]
 *   time-major     in  [n_frames][n_streams][frame_len]       out [n_frames][n_channels][frame_len]
 * so input and output differ in their channel strides and, time-major, in their frame strides too.  The audio, every side
 * output, every stage tap and every stage behind the demodulator keep their [n_channels]... shapes.  Addresses only: a
 * mapped call computes, bit for bit, what the same call computes without a map on inputs replicated as
 * I_rep[c] = I[stream_of_channel[c]].  Streams have no state; all state stays per channel: t41rx_state_bytes() and every
 * checkpoint are what they are without a map.  The map is configuration, like the buffer layout: it is in no checkpoint
 * and survives t41rx_reset, t41rx_set_state, t41rx_set_params and t41rx_set_coeffs.
 * t41rx_set_input_map(): stream_of_channel is a host array of n == n_channels entries, each in [0, n_streams), with
 *   1 <= n_streams <= n_channels; rows may repeat, go unused, and come in any order.  NULL with n_streams == 0 switches
 *   the map off: one row per channel again.  Everything is checked on the host before anything changes: any violation
 *   returns T41RX_ERR_ARG with a t41rx_last_error() text and leaves the previous map as it was.  Synchronises the device,
 *   then uploads (the ordering rule of t41rx_set_nco_freq): the map holds from the next process call on.
 * t41rx_get_input_map(): returns n_streams, or 0 with the map off (negative: an error status).  stream_of_channel_out,
 *   n == n_channels entries, receives the map when one is set; it may be NULL when only the count is wanted.
 * The host-pointer process forms allocate and copy in n_streams rows.  The calibration calls (t41rx_calibrate_*) keep
 * their own shared_input and ignore the map. */
T41RX_API int t41rx_set_input_map(t41rx_ctx *ctx, const int32_t *stream_of_channel, int n, int n_streams);
T41RX_API int t41rx_get_input_map(const t41rx_ctx *ctx, int32_t *stream_of_channel_out, int n);

/* ---- receiver groups: an output map, audio rows only for the channels somebody listens to (ABI 5) ----
 * The mirror of the input map.  A skimmer or a bank of FT8 receivers runs thousands of channels for their detectors and
 * decoders; a listener hears one or two.  With an output map set, channel c writes its audio to row row_of_channel[c] of
 * the audio buffer, or with row_of_channel[c] == -1 writes none, and the audio of every t41rx_process_* entry holds
 * n_rows rows instead of n_channels:
 *   channel-major  out [n_rows][n_frames * audio_frame_len]
 *   time-major     out [n_frames][n_rows][audio_frame_len]
 * for the device and the host entries, f32 and q15, at both audio rates, with or without an input map and parameter
 * sets.  The inputs, every side output, every stage tap and every stage result keep their [n_channels]... shapes.
 * With n_rows == 0 the audio pointer may be NULL (without a map a NULL audio pointer stays T41RX_ERR_ARG).
 * A listened channel c with row r: row r is, bit for bit, the row channel c gets from the same call without an output
 * map.  A muted channel: everything up to the demodulator and everything that reads behind it -- the AGC, every stage
 * that is on (the narrow CW filter and its memories too), every tap and side output, FT8, the panadapter, the beacon
 * monitor, the CW detector and decoder, every state record -- computes and holds what it does without a map, bit for
 * bit, with two exceptions: the two interpolators do not run and nothing is stored to the audio buffer.  The
 * interpolator memories of a muted channel stay in its state record as they were: the 24 kS/s rule
 * (t41rx_set_audio_rate) per channel.  When the channel is listened to again the interpolators continue from what they
 * last held.  Rows no channel names are not written.
 * The map is configuration, like the input map: it is in no checkpoint, survives t41rx_reset, t41rx_set_state,
 * t41rx_set_params and t41rx_set_coeffs, and may change between any two calls.  t41rx_state_bytes() and every
 * checkpoint section are what they are without a map.  The calibration entries (t41rx_calibrate_*) and the
 * t41rx_ft8_audio_* entries write no audio and ignore the map.  fft_length 512 only: at a long fft_length
 * t41rx_set_output_map() answers T41RX_ERR_UNSUPPORTED (the long-FFT pipeline's back kernel stores every channel).
 * t41rx_set_output_map(): row_of_channel is a host array of n == n_channels entries, each -1 or in [0, n_rows), with
 *   0 <= n_rows <= n_channels.  No row may be named twice (two waves would store to one row); rows may go unused.  NULL
 *   with n == 0 and n_rows == 0 switches the map off: one row per channel again.  Everything is checked on the host
 *   before anything changes: any violation returns T41RX_ERR_ARG with a t41rx_last_error() text that names the entry and
 *   leaves the previous map as it was.  Synchronises the device, then uploads (the ordering rule of
 *   t41rx_set_input_map): the map holds from the next process call on.
 * t41rx_get_output_map(): returns 1 with a map set, 0 with none (negative: an error status).  n_rows_out receives
 *   t41rx_audio_rows(); row_of_channel_out, n == n_channels entries, receives the map when one is set.  Either may be NULL.
 * t41rx_audio_rows(): rows of audio the process entries write: n_rows with a map, n_channels without.  The host-pointer
 *   process forms allocate and copy back that many rows; with a map that leaves rows unused they copy the caller's rows
 *   in first, so that an unused row comes back as it went in. */
T41RX_API int t41rx_set_output_map(t41rx_ctx *ctx, const int32_t *row_of_channel, int n, int n_rows);
T41RX_API int t41rx_get_output_map(const t41rx_ctx *ctx, int32_t *row_of_channel_out, int n, int *n_rows_out);
T41RX_API int t41rx_audio_rows(const t41rx_ctx *ctx);

/* ---- receiver groups: a stage map, the stages behind the demodulator only on the channels that ask (ABI 5) ----
 * The fourth map of the series.  The stages between the demodulator and the interpolators are switches of the whole
 * context (t41rx_set_receive_eq, nrOptionSelect / ANR_notchOn, t41rx_set_noise_blanker, t41rx_set_cw_detector,
 * t41rx_set_cw_decoder) and the expensive part of a call; a skimmer wants the notch and the equalizer on the two
 * channels somebody hears and the Morse decoder on the slices that show a carrier.  With a stage map set, every channel
 * carries a mask of T41RX_STAGE_* bits.
 * The rule: stage S runs on channel c in a call exactly when the context's switch for S is on, as the setters and
 * parameters above say, and bit S of stages_of_channel[c] is set.  A channel whose bit is clear is processed as the same
 * channel of a context in which S is switched off: the stage neither reads nor writes the channel's audio, S's memory for
 * the channel stays exactly as it was (the firmware's stale statics when a flag goes off and on again, and the rule the
 * output map applies to a muted channel's interpolators), and the channel's rows of the detector's and the decoder's
 * result buffers are not written.  A bit for a stage that is off in the context is allowed and has no effect until the
 * stage is switched on.  T41RX_STAGE_NR covers nrOptionSelect and the notch together: both take the same channels.
 * What the map does not reach: which kernels a call runs stays a function of the context's switches (a call with a stage
 * on hands over to the stage scratch even if that stage lists no channel); the narrow CW filter (t41rx_set_cw_filter)
 * stays a switch of the context -- it selects the call's back kernel, whose operation order differs from the other's, so
 * a filter per channel would need two back ends per call --; the side outputs and the stage taps stay context-wide
 * (FT8 receive has a map of its own, t41rx_set_ft8_map, and so have the panadapter and the beacon monitor behind it,
 * t41rx_set_panadapter_map); the refusal between parameter sets and the chain-splitting stages
 * stands for sets loaded without T41RX_SETS_STAGES (t41rx_set_param_sets_ex).
 * The map composes with the input map, the output map, both audio rates, both layouts, f32 and q15, and the host and
 * device entries: none of them sees it.
 * The map is configuration, like the output map: it is in no checkpoint, survives t41rx_reset, t41rx_set_state,
 * t41rx_set_params and t41rx_set_coeffs, and may change between any two calls.  t41rx_state_bytes(), every checkpoint
 * section and t41rx_reset() are what they are without a map and carry all channels.  fft_length 512 only: at a long
 * fft_length t41rx_set_stage_map() answers T41RX_ERR_UNSUPPORTED, as the stages themselves refuse there.
 * t41rx_set_stage_map(): stages_of_channel is a host array of n == n_channels masks.  NULL with n == 0 removes the map:
 *   every stage on every channel again, and the launches of a context that never had one.  Everything is checked on the
 *   host before anything changes: n != n_channels, a bit outside T41RX_STAGE_ALL, or a channel with
 *   T41RX_STAGE_CW_DECODE and without T41RX_STAGE_CW_DETECT (the decoder reads the detector's rows of its own channel)
 *   return T41RX_ERR_ARG with a t41rx_last_error() text that names the entry and leave the previous map as it was.
 *   Synchronises the device, then uploads (the ordering rule of t41rx_set_input_map): the map holds from the next
 *   process call on.  A caller who wants every stage on every channel sets no map: the identity map runs the list forms
 *   of the stage kernels over all channels and buys nothing.
 * t41rx_get_stage_map(): returns 1 with a map set, 0 with none (negative: an error status).  stages_of_channel_out,
 *   n == n_channels entries, receives the map, or T41RX_STAGE_ALL in every entry with none; it may be NULL. */
#define T41RX_STAGE_EQ        1u   /* DoReceiveEQ(),               Process.cpp:828-832 */
#define T41RX_STAGE_NR        2u   /* nrOptionSelect and the notch, Process.cpp:841-866 */
#define T41RX_STAGE_NB        4u   /* NoiseBlanker(),              Process.cpp:873-876 */
#define T41RX_STAGE_CW_DETECT 8u   /* DoCWReceiveProcessing(),     Process.cpp:878-879 */
#define T41RX_STAGE_CW_DECODE 16u  /* DoCWDecoding() behind it */
#define T41RX_STAGE_ALL       31u
T41RX_API int t41rx_set_stage_map(t41rx_ctx *ctx, const uint32_t *stages_of_channel, int n);  /* NULL, 0: remove */
T41RX_API int t41rx_get_stage_map(const t41rx_ctx *ctx, uint32_t *stages_of_channel_out, int n);

/* ---- receiver groups: stage parameters per channel -- the CW filter and the equalizer's levels (ABI 5) ----
 * The stage map says on which channels a stage runs, not with which parameters: every listener of a CW skimmer got the
 * same CWFilterIndex and the same fourteen equalizerRec levels.  These two maps give each channel its own.  Both are new
 * entry points: no call above changes what it does, and a context that sets neither launches what it always launched.
 *
 * THE CW FILTER MAP.  The rule: while a map is loaded, channel c is processed exactly as the same channel of a context
 * without a map whose t41rx_set_cw_filter() value is filter_of_channel[c] -- 0 .. 4, or 5 for off.  That covers the
 * channel's audio row, the five per-filter memories (only the selected one advances, the other four stay stale, as the
 * firmware's statics do), the interpolator memories and every other state word.  The context-wide index is kept, is not
 * consulted while a map is loaded, and is still what t41rx_get_cw_filter() returns; removing the map returns to it.  As
 * before, nothing of the CW block runs unless xmtMode == T41RX_CW_MODE.  The detector and the decoder read ahead of the
 * filter and do not see the map.
 * How a call runs it: the narrow filter runs in one launch over the list of filtered channels, each with its own index.
 * A filtered channel ends in the firmware's interpolators operation for operation, an unfiltered one in the fused back
 * kernel; the two differ in the last bit, so a call at 192 kS/s with both classes launches both back kernels, each in
 * its output-map form with the other class muted.  At 24 kS/s one finish serves both.  A map that filters nobody is a
 * call without the filter; a map that filters everybody a call with it.
 * t41rx_set_cw_filter_map(): filter_of_channel is a host array of n == n_channels values.  NULL with n == 0 removes the
 *   map.  Everything is checked on the host before anything changes, and a refused call leaves the previous map whole:
 *   n != n_channels, an entry outside [0, 5] (the text names the channel), or an entry < 5 before t41rx_set_cw_tables()
 *   loaded the filter tables return T41RX_ERR_ARG; fft_length != 512 returns T41RX_ERR_UNSUPPORTED; so does a map with
 *   an entry < 5 while parameter sets are loaded, in the words of the other chain-splitting stages, and
 *   t41rx_set_param_sets() refuses a context with such a map.  A map of 5s is accepted next to parameter sets, as
 *   t41rx_set_cw_filter(ctx, 5) is.  Synchronises the device, then uploads (the ordering rule of t41rx_set_input_map).
 *   Composes with the input map, the output map (set before or after), the stage map, both audio rates, both layouts,
 *   f32 and q15.
 * t41rx_get_cw_filter_map(): returns 1 with a map loaded, 0 with none (negative: an error status).
 *   filter_of_channel_out, n == n_channels entries, receives the map, or the context-wide index in every entry with
 *   none; it may be NULL.
 *
 * THE EQUALIZER LEVEL MAP.  The rule: while a map is loaded and the equalizer runs on channel c -- the context's switch
 * is on (t41rx_set_receive_eq) and the stage map's T41RX_STAGE_EQ bit is set or no stage map is loaded -- channel c is
 * processed exactly as a context whose t41rx_set_receive_eq(1, equalizerRec[c]) would process it.  The switch, the band
 * table and the stage map stay what they are; the context-wide levels are kept and returned by t41rx_get_receive_eq()
 * as before.  The levels are converted on the host, (float)equalizerRec / 100.0 with the sign of odd bands turned, as
 * for the context-wide vector, and uploaded when the map is set.
 * t41rx_set_receive_eq_map(): equalizerRec is a host array [n][14] with n == n_channels.  NULL with n == 0 removes the
 *   map.  n != n_channels returns T41RX_ERR_ARG, fft_length != 512 T41RX_ERR_UNSUPPORTED, and the previous map stays
 *   whole; no level vector is refused, as t41rx_set_receive_eq() refuses none.  Synchronises the device, then uploads.
 * t41rx_get_receive_eq_map(): returns 1 with a map loaded, 0 with none (negative: an error status).  equalizerRec_out,
 *   [n][14] with n == n_channels, receives the map, or the context-wide levels in every row with none; it may be NULL.
 *
 * Both maps are configuration, like the stage map: they are in no checkpoint, survive t41rx_reset, t41rx_set_state,
 * t41rx_set_params and t41rx_set_coeffs, and may change between any two calls.  t41rx_state_bytes() and every
 * checkpoint section are what they are without a map.  nrOptionSelect and the notch have a map of their own
 * (t41rx_set_nr_map, below), and so have FT8 receive (t41rx_set_ft8_map) and the panadapter with the beacon monitor
 * (t41rx_set_panadapter_map).  Still per context: the two display side outputs; the refusal between parameter
 * sets and the chain-splitting stages stands for sets loaded without T41RX_SETS_STAGES (t41rx_set_param_sets_ex). */
T41RX_API int t41rx_set_cw_filter_map(t41rx_ctx *ctx, const int32_t *filter_of_channel, int n);  /* NULL, 0: remove */
T41RX_API int t41rx_get_cw_filter_map(const t41rx_ctx *ctx, int32_t *filter_of_channel_out, int n);
T41RX_API int t41rx_set_receive_eq_map(t41rx_ctx *ctx, const int32_t *equalizerRec, int n);  /* [n][14]; NULL, 0: remove */
T41RX_API int t41rx_get_receive_eq_map(const t41rx_ctx *ctx, int32_t *equalizerRec_out, int n);

/* ---- receiver groups: the noise-reduction kind and the notch per channel (ABI 5) ----
 * The stage map's T41RX_STAGE_NR bit says on which channels "the noise reduction" runs; which of the four functions --
 * Kim1_NR(), SpectralNoiseReduction(), Xanr() as LMS noise reduction, Xanr() as the automatic notch -- was one value for
 * the whole context (params.nrOptionSelect, params.ANR_notchOn).  This map gives each channel its own two values.  New
 * entry points: no call above changes what it does, and a context that sets no map launches what it always launched.
 * The rule: while a map is loaded, channel c is processed exactly as the same channel of a context without a map whose
 * parameters carry nrOptionSelect = nr_of_channel[c] (0 .. 3) and ANR_notchOn = notch_of_channel[c] (0 / 1).  That covers
 * the channel's audio row, Xanr()'s record, the Kim / spectral record and every other state word, bit for bit -- the
 * firmware's stale statics when a channel's kind changes between two calls included: the spectral function leaves
 * NR_X[.][1..2] and NR_E alone and Kim1_NR() then starts from them; LMS and notch share one Xanr() record.  The context's
 * own nrOptionSelect / ANR_notchOn are kept, are not consulted while a map is loaded, and are still what
 * t41rx_get_params() returns; removing the map returns to them.  NR_alpha, NR_beta, NR_PSI and the VAD range from FLoCut /
 * FHiCut stay those of the context for every channel.  A function runs on channel c when its map entry asks for it and
 * either no stage map is loaded or the channel's T41RX_STAGE_NR bit is set; a channel with 0 / 0, or with the bit clear,
 * is processed as the stage map processes a channel whose bit is clear: audio not touched, both records as they were.
 * How a call runs it: one launch serves the Kim and the spectral channels, each workgroup reading its channel and its kind
 * from a list, and one launch behind it serves Xanr() -- LMS only, notch only, LMS then notch -- from a list sorted by
 * those three classes, so a mixed call costs about the longest of the serial chains, not their sum.  A launch whose list
 * is empty is not made.  "Noise reduction on" is "some entry of the map is non-zero": an all-zero map launches what a
 * context with nrOptionSelect 0 and ANR_notchOn 0 launches; a map with a non-zero entry hands over to the stage scratch
 * even if the stage map lists nobody.
 * The CW detector's one-audio-stream rule (a process call with the detector on refuses Kim or LMS noise reduction without
 * the notch or the blanker behind it) is evaluated per channel with the channel's own two values while a map is loaded:
 * the call is refused if any channel trips it, and the text names the first such channel.
 * t41rx_set_nr_map(): two host arrays of n == n_channels values.  NULL, NULL with n == 0 removes the map.  Everything is
 *   checked on the host before anything changes, and a refused call leaves the previous map whole: n != n_channels, one
 *   array NULL, an entry outside 0 .. 3 or 0 .. 1 (the text names the channel) return T41RX_ERR_ARG; fft_length != 512
 *   returns T41RX_ERR_UNSUPPORTED; a map with an entry 2 while the context's pass band fails the spectral function's
 *   array-bounds check returns what t41rx_set_params() returns for nrOptionSelect = 2 there, with its text; a map with a
 *   non-zero entry while parameter sets are loaded returns T41RX_ERR_UNSUPPORTED in the words of the chain-splitting
 *   stages, and t41rx_set_param_sets() refuses a context with such a map.  An all-zero map stands next to parameter
 *   sets.  While a map with an entry 2 is loaded t41rx_set_params() and t41rx_set_coeffs() refuse a pass band that fails
 *   that check, and the previous parameters stay.  Synchronises the device, then uploads (the ordering rule of
 *   t41rx_set_input_map).  Configuration, like the other maps: in no checkpoint, survives t41rx_reset, t41rx_set_state,
 *   t41rx_set_params and t41rx_set_coeffs, may change between any two calls; t41rx_state_bytes() and every checkpoint
 *   section are what they are without a map.  Composes with the input map, the output map, the stage map (set before or
 *   after), the CW filter map, the level map, both audio rates, both layouts, f32 and q15, host and device entries.
 * t41rx_get_nr_map(): returns 1 with a map loaded, 0 with none (negative: an error status).  The two outputs, n ==
 *   n_channels entries each, receive the map, or the context's own values in every entry with none; either may be NULL. */
T41RX_API int t41rx_set_nr_map(t41rx_ctx *ctx, const int32_t *nr_of_channel, const int32_t *notch_of_channel, int n);  /* NULL, NULL, 0: remove */
T41RX_API int t41rx_get_nr_map(const t41rx_ctx *ctx, int32_t *nr_of_channel_out, int32_t *notch_of_channel_out, int n);

/* ---- receiver groups: parameter sets, one t41rx_params per group of channels (ABI 5) ----
 * The receivers of one band differ in more than NCOFreq: the phone receivers are LSB at 2.8 kHz, the FT8 receiver is USB
 * at 200..3000 Hz, the CW receivers want a few hundred hertz (the FT8 receiver next to LSB ones: t41rx_set_ft8_map, which
 * asks only the channels it lists for USB).  A context's own t41rx_params (t41rx_create,
 * t41rx_set_params, t41rx_get_params, as ever) is set 0.  On top of it a context holds up to T41RX_MAX_PARAM_SETS - 1
 * extra sets, numbered 1..K, and a table set_of_channel[n_channels].  Channel c is processed exactly as a context created
 * with sets[set_of_channel[c]] would process it, with the same NCOFreq[c], input and history: audio, side outputs, taps
 * and the channel's state records match bit for bit.  The sets are configuration, like the input map: state,
 * t41rx_state_bytes() and every checkpoint section are what they are without them, the sets survive t41rx_reset and
 * t41rx_set_state, and a checkpoint taken with sets restores into a context without.  The CW side tone folded into the
 * oscillator follows the channel's own set.
 *
 * The compatibility rule (one rule; t41rx_param_sets_compatible() is it): two sets may share a context when the
 * library picks the same kernel for both and both name the same stages.  They must have equal
 *     fft_length, which must be 512 (the long-FFT pipeline refuses sets);
 *     demodulator family -- USB and LSB are one family; AM, NFM and SAM one each;
 *     AGC off (AGCMode 0) versus on (AGCMode 1..4);
 *     nfm_demod;  xmtMode;
 *     nrOptionSelect and ANR_notchOn, both 0 (the stages that split the chain read set 0 on the host: see below);
 *     the classification of the first stage's gains as "plain" -- RFgain 1 and, in the modes with the IQ correction
 *       (USB, LSB, AM, SAM), IQAmpCorrectionFactor 1 and IQPhaseCorrectionFactor 0 -- or general.
 * Free to differ: USB / LSB; FLoCut, FHiCut; rfGainAllBands; RFgain and the IQ corrections within the general class;
 * audioVolume; AGCMode among 1..4 and AGC_thresh; am_lpf_f0, nfmFilterBW, CWFreqShift; the NR_* numbers (unused).
 *
 * t41rx_set_param_sets(): sets[i] becomes set i + 1 (host array of n_sets entries, 1 <= n_sets < T41RX_MAX_PARAM_SETS);
 *   set_of_channel is a host array of n == n_channels entries in [0, n_sets].  n_sets == 0 with both pointers NULL
 *   removes the sets.  Everything is checked on the host before anything changes; a refused call leaves the previous sets
 *   in place: T41RX_ERR_ARG for a wrong n, an entry out of range, n_sets beyond the cap or an invalid set (the text names
 *   it), T41RX_ERR_UNSUPPORTED with the reason for a set the rule refuses against set 0 or another set, at a long
 *   fft_length, and while a stage that splits the chain is on -- the receive equalizer, noise reduction / notch, the noise
 *   blanker, the CW filter, the CW detector and decoder.  Those stages refuse to be switched on while sets are loaded
 *   (T41RX_ERR_UNSUPPORTED), in the same words.  What only taps the fused chain works with sets: the audio spectrum, the
 *   display spectrum, the panadapter and the beacon monitor behind it, FT8 receive, the stage taps.  The calibration calls
 *   keep reading the context's own parameters.  Synchronises the device, then uploads: the sets hold from the next
 *   process call on.
 * t41rx_set_params() changes set 0 and is refused (T41RX_ERR_UNSUPPORTED) if it would break the rule against a loaded
 *   set; t41rx_set_coeffs() applies to set 0 and is held to the same rule through the blob's embedded parameters;
 *   t41rx_get_coeffs() returns set 0's blob.
 * t41rx_get_param_sets(): returns K, the number of extra sets (0: none; negative: an error status).  sets_out (cap
 *   entries, cap >= K) and set_of_channel_out (n == n_channels entries) receive them; either may be NULL.
 * t41rx_param_sets_compatible(): the rule on two parameter structs, on the host, without a context: T41RX_OK, or
 *   T41RX_ERR_UNSUPPORTED with the clause in t41rx_last_error() (T41RX_ERR_ARG for NULL or an invalid struct). */
#define T41RX_MAX_PARAM_SETS 64
T41RX_API int t41rx_set_param_sets(t41rx_ctx *ctx, const t41rx_params *sets, int n_sets, const int32_t *set_of_channel, int n);
T41RX_API int t41rx_get_param_sets(const t41rx_ctx *ctx, t41rx_params *sets_out, int cap, int32_t *set_of_channel_out, int n);
T41RX_API int t41rx_param_sets_compatible(const t41rx_params *a, const t41rx_params *b);

/* ---- receiver groups: parameter sets next to the chain-splitting stages (ABI 5) ----
 * The refusals above stand for sets loaded without T41RX_SETS_STAGES.  Sets loaded through t41rx_set_param_sets_ex() with
 * that flag ("staged sets") run next to the receive equalizer, noise reduction / notch, the noise blanker, the narrow CW
 * filter, the CW detector and the CW decoder.  New entry points: flags == 0 is t41rx_set_param_sets() /
 * t41rx_param_sets_compatible() word for word (those are this call with flags 0), an unknown flag bit returns
 * T41RX_ERR_ARG, and t41rx_get_param_sets() returns staged sets as ever.
 * The rule: channel c is processed exactly as the same channel of a context created with sets[set_of_channel[c]] and
 * carrying the same stage switches, stage map, CW filter map, equalizer level map, noise-reduction map, output map, input
 * map, audio rate and layout: audio, side outputs, taps, the detector's and the decoder's rows and every state record, bit
 * for bit; f32 and q15, both layouts, host and device entries, 192 and 24 kS/s.
 * The compatibility rule under the flag keeps every clause except "both 0" on nrOptionSelect / ANR_notchOn; xmtMode
 * stays equal, so the CW block runs for all sets or for none.  Without a noise-reduction map a channel takes its own
 * set's nrOptionSelect and ANR_notchOn; with a map the map supplies the two, as it overrides the context's without sets.
 * Either way the channel takes its own set's NR_alpha, NR_beta, NR_PSI and the VAD range of its own pass band.  Under
 * staged sets the noise reduction always runs through the map's two launches, over lists made of the effective values.
 * The narrow CW filter's interpolators take the volume and the taps of the channel's own set.
 * The spectral function's array-bounds check (t41rx_set_params with nrOptionSelect = 2) is made per channel against the
 * channel's own set, by every setter that can break it -- this one, t41rx_set_nr_map(), and t41rx_set_params() /
 * t41rx_set_coeffs() for set 0: T41RX_ERR_ARG, the text names the channel and the set, and everything stays as it was.
 * A set whose own nrOptionSelect is 2 and whose pass band fails the check is an invalid t41rx_params and is refused as
 * such (T41RX_ERR_ARG, "set i is invalid") whether a channel names it or not; a set with another kind and such a pass
 * band is accepted as long as no channel runs kind 2 on it.
 * Setter interplay: the stage setters and the two maps (t41rx_set_cw_filter_map with an entry < 5, t41rx_set_nr_map with a
 * non-zero entry) accept while staged sets are loaded, and staged sets load while those stages are on.
 * t41rx_set_param_sets() called while a stage is on refuses as ever and leaves loaded staged sets in place; sets loaded
 * without the flag followed by a stage setter refuse as ever.  The CW detector's one-audio-stream rule is evaluated per
 * channel with the channel's effective kind and notch; the refusal names the first offending channel.  Still refused, in
 * the words above: the long fft_lengths, and FT8 receive on a non-USB set -- without an FT8 map; with one
 * (t41rx_set_ft8_map) only the listed channels' sets are asked for USB.  The panadapter and the beacon monitor work with
 * staged sets as with plain ones -- on every channel, or with a panadapter map (t41rx_set_panadapter_map) on the listed
 * ones, each with its own set's RFgain / rfGainAllBands --; the side outputs are switches of the context.
 * flags is an int32_t holding T41RX_SETS_* bits (the scalar types of this header are int, int32_t, int64_t, size_t and
 * float); a negative value has unknown bits set.
 * t41rx_get_param_sets_flags(): the flags of the loaded sets; 0 with none or with sets loaded without a flag
 *   (negative: an error status). */
#define T41RX_SETS_STAGES 1u
T41RX_API int t41rx_set_param_sets_ex(t41rx_ctx *ctx, const t41rx_params *sets, int n_sets, const int32_t *set_of_channel, int n, int32_t flags);
T41RX_API int t41rx_get_param_sets_flags(const t41rx_ctx *ctx);
T41RX_API int t41rx_param_sets_compatible_ex(const t41rx_params *a, const t41rx_params *b, int32_t flags);

/* ---- the hot path: ProcessIQData() on every channel ----
 * Device-pointer form: dI, dQ, dAudio are device pointers ([n_channels][n_frames*frame_len], or time-major:
 * t41rx_set_buffer_layout; with an input map dI / dQ hold n_streams rows: t41rx_set_input_map; with an output map
 * dAudio holds n_rows rows: t41rx_set_output_map);
 * the kernel is enqueued on `hip_stream` (a hipStream_t, may be NULL = default stream) and the
 * call returns without synchronising. */
T41RX_API int t41rx_process_device(t41rx_ctx *ctx, const float *dI, const float *dQ, float *dAudio,
                         int n_frames, void *hip_stream);
/* Host-pointer form (the reference's calling convention: caller-owned host arrays): copies
 * in, runs the same kernel, copies out, synchronises. */
T41RX_API int t41rx_process_host(t41rx_ctx *ctx, const float *I, const float *Q, float *audio,
                       int n_frames);

/* The same call on the firmware's own sample format either side of the path: q15 samples as the
 * AudioRecordQueues deliver them and as the AudioPlayQueue takes them.  Restates
 *   arm_q15_to_float(Q_in_R.readBuffer(), &float_buffer_L[...]); arm_q15_to_float(Q_in_L.readBuffer(),
 *   &float_buffer_R[...])                     Process.cpp:107-108 (note the swap: I comes from the R queue)
 *   arm_float_to_q15(float_buffer_L, q15_buffer_LTemp, 2048); Q_out_L.play(...)    Process.cpp:936-937
 * with CMSIS-DSP's conversions (x / 32768; truncating, saturating (q15_t)__SSAT((q31_t)(x * 32768), 16)).
 * Layout [n_channels][n_frames*frame_len] int16, the 16 blocks of 128 of a frame back to back (or time-major,
 * t41rx_set_buffer_layout; with an input map the two input queues hold n_streams rows, t41rx_set_input_map).  The side outputs and stage taps work here as on the f32 entry points (ABI 5): the
 * reference computes its display FFT and audio spectrum inside every ProcessIQData() call on exactly these q15-fed
 * buffers (Process.cpp:107-108 -> :184-186, :211-215, :550-570). */
T41RX_API int t41rx_process_device_q15(t41rx_ctx *ctx, const int16_t *dQ_in_L, const int16_t *dQ_in_R,
                             int16_t *dQ_out_L, int n_frames, void *hip_stream);
T41RX_API int t41rx_process_host_q15(t41rx_ctx *ctx, const int16_t *Q_in_L, const int16_t *Q_in_R,
                           int16_t *Q_out_L, int n_frames);

/* ---- checkpoint of the streaming state (the reference never persists it) ----
 * Layout (ABI 5): a 32-byte header of eight int32 words
 *     [0] magic "T41S"  [1] T41RX_ABI_VERSION  [2] fft_length  [3] n_channels  [4] floats per channel record
 *     [5] section mask (below)  [6] spectrumZoom of the display section (0 without one)  [7] reserved, 0
 * then the path's per-channel records (FIR delay lines, oscillator, overlap block, AGC, demodulator words), then the
 * sections header word 5 names, in this order:
 *     bit 0  noise reduction / notch: Xanr()'s taps, delay line and leak words, then the Kim / spectral per-bin memories
 *            (Noise.cpp:19-56) -- present once one of those stages has run in this context;
 *     bit 1  display FFT: zoom filters, ring, FFT_spec_old (FFT.cpp:14-26) -- present while
 *            t41rx_set_display_spectrum() is on;
 *     bit 2  noise blanker: last_frame_end[0 .. 12] (DSP_Fn.cpp:143), 16 floats per channel (13 used) -- present once
 *            the blanker has run in this context; refused at a long fft_length;
 *     bit 3  receive equalizer: rec_EQ_Band1_state .. rec_EQ_Band14_state (Filter.cpp:43-56), 112 floats per channel --
 *            present once the equalizer has run in this context; refused at a long fft_length;
 *     bit 4  CW receive: CW_AudioFilter1_state .. CW_AudioFilter5_state (60 floats), the decode FIR's history (63),
 *            corrResultR, aveCorrResultL, aveCorrResultR, 2 zeros: 128 floats per channel -- present once the narrow
 *            filter or the detector has run in this context; refused at a long fft_length;
 *     bit 5  CW decoder: 3104 int32 words per channel -- 32 scalars, then signalHistogram[768], then gapHistogram[2304].
 *            The scalars by word offset: 0 decodeStates, 1 n (the frame count of the clock), 2 oldTime, 3 signalStart,
 *            4 signalEnd, 5 signalElapsedTime, 6 gapLength, 7 ditLength, 8 dahLength, 9 gapAtom, 10 gapChar,
 *            11 thresholdGeometricMean (the float's bits), 12 aveDitLength, 13 aveDahLength, 14 valRef1, 15 valRef2,
 *            16 gapRef1, 17 valFlag, 18 signalStartOld, 19 currentDashJump, 20 currentDecoderIndex, 21 charProcessFlag,
 *            22 blankFlag, 23 topGapIndex, 24 topGapIndexOld, 25 currentTime, 26 interElementGap, 27 noSignalTimeStamp,
 *            28 .. 31 zero -- present once the decoder has run in this context; refused at a long fft_length.
 * t41rx_state_bytes() therefore GROWS when a noise-reduction stage, the noise blanker, the receive equalizer, a CW
 * stage or the CW decoder first runs or the display spectrum is switched on:
 * query it right before every t41rx_get_state() (a buffer sized at creation gets T41RX_ERR_STATE "state buffer too
 * small").  fft_length cannot change on a live context, so the path records' size never does.
 * t41rx_set_state() refuses (T41RX_ERR_STATE) a checkpoint of another ABI, FFT length or channel count, one with an
 * unknown section bit or a size that does not follow from its header, a display section while the display spectrum is
 * off here or taken at another spectrumZoom, and any word the kernels use as an index, a divisor or a state number that
 * is out of range or not integral: AGC state words, oscillator amplitude, synchronous-detector PLL words (phase in
 * [0, 2 pi], frequency within +-pll_fmax), the notch's leak index, the noise reduction's ring pointers, the zoom ring's
 * pointer; of the CW decoder a decodeStates outside {0, 1, 2, 5, 6}, currentDecoderIndex outside 0 .. 255,
 * currentDashJump outside 0 .. 128, a thresholdGeometricMean that is not finite or outside [1, 750), averages or value
 * references outside 0 .. 32767, a flag (valFlag, charProcessFlag, blankFlag) outside 0 / 1, a histogram count that is
 * negative or above 2^27 (seven of them are summed).  What it does to the side stages: a section the checkpoint carries is restored; a memory this context has
 * allocated but the checkpoint does not carry goes back to its power-on values (InitializeDataArrays() /
 * SpectralNoiseReductionInit() / ZoomFFTPrep() / the blanker's zero carry / the equalizer's zero memories) -- never the values of the stream being replaced.
 * T41RX_ERR_STATE is also what t41rx_get_state(), t41rx_process_host() and t41rx_process_host_q15() -- the calls that
 * synchronise -- return if a wait inside the pipelined AGC / SAM kernels has run out since the last t41rx_reset() or
 * restored checkpoint (their waits are bounded so that a broken hand-over cannot hang the GPU; it cannot happen unless
 * the kernel is wrong, and then the samples are not to be trusted). */
T41RX_API size_t t41rx_state_bytes(const t41rx_ctx *ctx);
T41RX_API int    t41rx_get_state(t41rx_ctx *ctx, void *host_buf, size_t bytes);
T41RX_API int    t41rx_set_state(t41rx_ctx *ctx, const void *host_buf, size_t bytes);

/* ---- stage taps for parity debugging (device pointers, may each be NULL) ----
 * When set, the next process calls also write, per channel and frame:
 *   post_nco : [n_channels][n_frames*frame_len*2]  I/Q after FreqShift2 (planar: I then Q per frame)
 *   dec      : [n_channels][n_frames*fft_length]   I/Q after decimate-by-8 (+ level adjust)
 *   demod    : [n_channels][n_frames*fft_length/2] audio @24 kS/s before interpolation, as the demodulator (and AGC)
 *              leave it: before every optional stage (receive equalizer, noise reduction / notch, noise blanker)
 * max_frames = the n_frames the buffers are sized for: a process call with more frames is refused
 * (T41RX_ERR_ARG) instead of writing past them.  fft_length 512 only (T41RX_ERR_UNSUPPORTED). */
T41RX_API int t41rx_set_debug_taps(t41rx_ctx *ctx, float *d_post_nco, float *d_dec, float *d_demod, int max_frames);

/* ---- the path's display by-product: the audio spectrum and the S-meter's input ----
 * What ProcessIQData() leaves behind when updateDisplayFlag == 1 (Process.cpp:550-570; NFM:
 * :790-805): audioSpectBuffer[1023 - k] = iFFT_buffer[k]^2 over the 1024 floats of the masked
 * spectrum (squares of the individual re / im values, reversed), arm_max_f32 of it, and the
 * running average the S-meter reads (Display.cpp:980-985).  Device pointers, both NULL = off
 * (the default).  While set, every processed frame writes
 *   d_spect : [n_channels][n_frames][1024]  audioSpectBuffer
 *   d_max   : [n_channels][n_frames][3]     audioMaxSquared, (float)AudioMaxIndex, audioMaxSquaredAve
 * and updates the per-channel audioMaxSquaredAve.  The pixel mapping (audioYPixel) is display
 * code and stays with the caller.  fft_length 512; f32 and q15 entry points.  max_frames as above. */
T41RX_API int t41rx_set_audio_spectrum(t41rx_ctx *ctx, float *d_spect, float *d_max, int max_frames);

/* ---- the display FFT: what ShowSpectrum() draws from (FFT.cpp:67-251) ----
 * CalcZoom1Magn() (spectrumZoom = 0: Hann-windowed 512-point FFT of the frame's first 512 I/Q samples
 * after gains, DC high-pass and IQ correction, Process.cpp:185-187) or ZoomFFTExe() (spectrumZoom
 * 1..4 = 2x..16x: Fs/4 shift, 4-stage elliptic IIR mag_coeffs[zoom], 4-tap decimating FIR by 2^zoom,
 * 512-sample ring, window, FFT; Process.cpp:211-215), both up to FFT_spec[512] (squared magnitudes,
 * halves swapped so that DC sits at index 256) and the display's low-pass memory FFT_spec_old[512].
 * The pixel mapping behind them (log10f_fast, display scale, pixel offsets) is t41rx_set_panadapter()'s, below.
 * Device pointers, both NULL = off (the default).  While set, every processed frame is treated as
 * one with updateDisplayFlag == 1 and writes
 *   d_spec     : [n_channels][n_frames][512]  FFT_spec
 *   d_spec_old : [n_channels][n_frames][512]  FFT_spec_old
 * Setting it (or changing spectrumZoom) starts from cleared zoom filters, ring and low-pass memory.
 * fft_length 512; f32 and q15 entry points; max_frames as for the stage taps. */
T41RX_API int t41rx_set_display_spectrum(t41rx_ctx *ctx, float *d_spec, float *d_spec_old, int spectrumZoom, int max_frames);

/* ---- IQ calibration: ProcessIQData2() and the sideband measurement (Process2.cpp:295-399, 478-547) ----
 * DoReceiveCalibrate() / DoXmitCalibrate() loop over ShowSpectrum2(), whose PlotCalSpectrum() runs ProcessIQData2() and
 * turns two windows of pixelnew[] into adjdB, the level of the unwanted sideband against the wanted one; the operator
 * turns an encoder until it is smallest.  Here the batch axis replaces the operator: every channel of a context tries its
 * own (IQAmpCorrectionFactor, IQPhaseCorrectionFactor) candidate, if need be on the same recording.  The transmit half
 * (the tone through the TX correction and the exciter's interpolators) is t41tx_process_cal_*_q15 in t41tx.h; this is the
 * receive half.  Per frame, in the firmware's order:
 *   updateDisplayFlag, one byte per frame for all channels (PlotCalSpectrum() sets it on the first call of a sweep only):
 *     a frame with flag 0 reads no samples and advances no memory (Process2.cpp:387-395, FFT.cpp:209); with flag 1:
 *   q15 -> float with the queues swapped (:359-360), or f32; x 10^(rfGainAllBands/20); x recBandFactor (1.0);
 *   in USB and LSB I x -IQAmpCorrectionFactor, then IQPhaseCorrection() (:376-384) -- no DC high-pass; FreqShift1();
 *   spectrumZoom 0: CalcZoom1Magn() on the first 512 samples AFTER the shift (the audio path calls it before);
 *   spectrumZoom 1..4: ZoomFFTExe() on the shifted 2048 samples;
 *   pixelnew[x] = baseOffset + pixel_offset + (int16_t)(dBScale * log10f_fast(v)), v = FFT_spec[x] un-smoothed at zoom 0
 *     (FFT.cpp:245) and smoothed at zoom >= 1 (:157); {dBScale, baseOffset} = displayScale[currentScale] (Display.cpp:127-135);
 * and in every frame, flag 0 included, from the channel's current pixelnew[]: arm_max_q15 over [bin0 - capture_bins,
 * bin0 + capture_bins) and [bin1 - capture_bins, bin1 + capture_bins); LSB: refAmplitude = window 0, adjAmplitude =
 * window 1, USB the other way round, any other mode both 0; adjdB = ((float)adj - (float)ref) / 1.95 (:498-505, 524).
 * The calibration memory -- FFT_spec_old[512], the zoom filters' memories, the ring and its pointer, pixelnew[512] per
 * channel -- is the context's own: allocated when calibration is first configured, set to power-on values (all zero) by
 * t41rx_set_calibration() and t41rx_reset(), and NOT part of the checkpoint: t41rx_state_bytes() and the section mask are
 * unchanged.  The calibration calls read and write nothing of the audio path's state, and the other way round.
 * t41rx_set_calibration(): on = 0 switches it off (the other arguments are ignored).  T41RX_ERR_ARG for spectrumZoom or
 *   currentScale outside 0..4, a pixel_offset that does not fit an int16, capture_bins < 1, or a window that leaves
 *   [2, 512] (ShowSpectrum2() zeroes pixelnew[0..1] every sweep: windows off those two bins sidestep that);
 *   T41RX_ERR_UNSUPPORTED at a long fft_length or on a time-major context.  The firmware's settings are below; it
 *   calibrates at currentScale 1 (20.0, 10), capture_bins 10, spectrumZoom 0 for receive and 2 for transmit calibration.
 * t41rx_set_cal_corrections(): one candidate per channel, host arrays of n_channels floats, copied (synchronises).  Both
 *   NULL: every channel uses the params' IQAmpCorrectionFactor / IQPhaseCorrectionFactor.  One NULL, or a non-finite
 *   value: T41RX_ERR_ARG.  They apply to the calibration calls only.
 * t41rx_calibrate_device(): n_frames frames on every channel.  dI / dQ: [n_channels][n_frames * 2048] f32, or with
 *   shared_input != 0 one channel's [n_frames * 2048] that every channel reads (the sweep's shape: thousands of
 *   candidates, one recording).  d_update: [n_frames] bytes, NULL = every frame 1.  d_result: [n_channels][n_frames][3] =
 *   refAmplitude, adjAmplitude, adjdB, written for every frame.  d_pixel [n_channels][n_frames][512] int16 and d_spec
 *   [n_channels][n_frames][512] f32 (pixelnew and FFT_spec) may be NULL; their rows are written for update frames only,
 *   other rows are left alone.  Enqueued on hip_stream, no sync.  T41RX_ERR_ARG before t41rx_set_calibration(on), for
 *   n_frames <= 0, and for NULL input or a NULL d_result.  The _q15 form takes the two queues' int16 samples; the _host
 *   forms copy in (d_pixel / d_spec too), run the same kernel, copy out and synchronise.  An input map
 *   (t41rx_set_input_map) is the audio path's: the calibration calls ignore it and keep their own shared_input. */
#define T41RX_CAL_RX_LSB_BIN0 310 /* cal_bins[], Process2.cpp:429-444 */
#define T41RX_CAL_RX_LSB_BIN1 460
#define T41RX_CAL_RX_USB_BIN0 65
#define T41RX_CAL_RX_USB_BIN1 192
#define T41RX_CAL_TX_LSB_BIN0 240
#define T41RX_CAL_TX_LSB_BIN1 305
#define T41RX_CAL_TX_USB_BIN0 209
#define T41RX_CAL_TX_USB_BIN1 273
#define T41RX_CAL_CAPTURE_BINS 10 /* :415 */
#define T41RX_CAL_RX_ZOOM 0
#define T41RX_CAL_TX_ZOOM 2
#define T41RX_CAL_SCALE 1
T41RX_API int t41rx_set_calibration(t41rx_ctx *ctx, int on, int spectrumZoom, int currentScale, int pixel_offset, int bin0,
                          int bin1, int capture_bins);
T41RX_API int t41rx_set_cal_corrections(t41rx_ctx *ctx, const float *amp, const float *phase);
T41RX_API int t41rx_calibrate_device(t41rx_ctx *ctx, const float *dI, const float *dQ, int shared_input, const uint8_t *d_update,
                           float *d_result, int16_t *d_pixel, float *d_spec, int n_frames, void *hip_stream);
T41RX_API int t41rx_calibrate_device_q15(t41rx_ctx *ctx, const int16_t *dQ_in_L, const int16_t *dQ_in_R, int shared_input,
                               const uint8_t *d_update, float *d_result, int16_t *d_pixel, float *d_spec, int n_frames,
                               void *hip_stream);
T41RX_API int t41rx_calibrate_host(t41rx_ctx *ctx, const float *I, const float *Q, int shared_input, const uint8_t *update,
                         float *result, int16_t *pixel, float *spec, int n_frames);
T41RX_API int t41rx_calibrate_host_q15(t41rx_ctx *ctx, const int16_t *Q_in_L, const int16_t *Q_in_R, int shared_input,
                             const uint8_t *update, float *result, int16_t *pixel, float *spec, int n_frames);

/* ---- FT8 receive up to the finished waterfall (Process.cpp:627-686, ft8.cpp:153-268) ----
 * In DEMOD_FT8 the firmware demodulates as USB and, on float_buffer_L as the demodulator and the AGC leave it (in front of
 * the equalizer: the position of the demod tap), resamples to 6.4 kS/s into the rolling q15 buffer ft8_dsp_buffer[3072];
 * every 15 frames process_FT8_FFT() turns it into four rows of 368 bytes of export_fft_power, and 92 such blocks per 15 s
 * slot are the waterfall ft8_decode() searches.  Here FT8 is a switch on a USB context, not a mode of its own; find_sync()
 * and ft8_decode() up to the CRC check are t41rx_ft8_decode_*() below, on the finished half; the RTC, the unpacking of the
 * 77 payload bits into text and the decoded[] log stay with the caller.  Per channel and frame, in the firmware's order:
 *   while syncFlag: arm_float_to_q15 (truncating, saturating) and the 68-iteration collector loop as written -- words
 *     1020..1023 and 2044..2047 are never rolled, with leftover >= 1 iteration i rolls the sample iteration i - leftover of
 *     the same frame has just written, the `leftover` cell behind frames 3 / 7 / 11 is rolled by the next frame --
 *     ++dataLoop, the leftover cells at 4 / 8 / 12, the last cell and DSP_Flag = 1 at 15;
 *   when DSP_Flag == 1 and ft8_flag == 1: for time_sub 0 and 512 (q15_t)((float)buf[i + time_sub] * window[i]),
 *     arm_rfft_q15 (2048 points), arm_shift_q15 by 5, (re*re + im*im) >> 17 (0 .. 16384, the sum in 64 bits), mag_db[] by
 *     that value, and for freq_sub 0 / 1 and j < 368 (int)((mag_db[.][2j + freq_sub] + mag_db[.][2j + freq_sub + 1]) / 2)
 *     clipped to 0..255 at 1472 * FT_8_counter + 736 * (time_sub / 512) + 368 * freq_sub + j; FT_8_counter++, at 92
 *     ft8_flag = 0; DSP_Flag = 0.  A DSP_Flag left standing while ft8_flag was 0 makes block 0 of the next slot fire on the
 *     first frame after the restart, off the 15-frame phase, as in the firmware;
 *   when ft8_flag == 0 and syncFlag: update_synchronization() in uint32 on millis(n) = t0 + floor(n * num / den):
 *     (millis(n) - start_time) % 15000 <= 200 sets ft8_flag = 1, FT_8_counter = 0;
 *   n, the channel's count of FT8 frames since power-on or reset, advances (on unsynced channels nothing else does).
 * arm_rfft_q15 is restated as CMSIS-DSP's Cortex-M7 build computes it (radix-4 q15 stages with their scaling, bit
 * reversal, the real split stage with q15 tables rounded half away from zero): tests/ft8_model.py lists what that leaves
 * open.  The stage only reads the audio: the audio out is bit for bit what it is with the stage off.
 * t41rx_set_ft8_tables(): window = ft_blackman_i(i, 2048), i < 2048; mag_db[m] = 10.0 * log((float)(10 * m) + 0.1), m <=
 *   16384, both from the firmware's libm (host arrays, copied; synchronises).  The library has no table of its own.
 *   T41RX_ERR_ARG for NULL or a non-finite entry.
 * t41rx_set_ft8(): on = 1 with device buffers d_power [n_channels][2][92 * 1472] uint8 -- two halves, so that a finished
 *   slot stays readable while the next is written; the library never clears them -- and d_status [n_channels][n_frames][4]
 *   int32 (16-byte aligned) = {FT_8_counter behind the frame, ft8_flag, 0 or 1 + the half completed in this frame,
 *   dataLoop}, written for every frame of every process call of at most max_frames frames (a longer call:
 *   T41RX_ERR_ARG).  max_frames <= 1380 (T41RX_ERR_ARG above): two completions of one channel are at least 92 x 15
 *   frames apart, so a half reported complete is intact when the call returns.  on = 1 gets T41RX_ERR_UNSUPPORTED at a
 *   long fft_length, T41RX_ERR_ARG with a NULL buffer or before the tables are loaded.  on = 0 switches the stage off (the
 *   other arguments are ignored; the FT8 memory stays).  While on, a process call with mode != T41RX_DEMOD_USB is refused
 *   with T41RX_ERR_UNSUPPORTED (t41rx_last_error() says why).  f32 and q15 entry points, both buffer layouts.  Kept across
 *   t41rx_set_params() / t41rx_set_coeffs().  t41rx_get_ft8() returns the switch.  With an FT8 map (t41rx_set_ft8_map,
 *   below) both buffers hold t41rx_ft8_rows() rows in place of n_channels.
 * t41rx_set_ft8_clock(): millis(n) = t0_ms + floor(n * num / den) in uint32; default 0, 32, 3 (one frame of 2048 samples
 *   at 192 kS/s).  From the next call; n is not touched.  T41RX_ERR_ARG for num < 0 or den <= 0.
 * t41rx_ft8_sync(): auto_sync_FT8()'s success branch on the channels whose byte is non-zero (host array of n = n_channels
 *   bytes; NULL = all): start_time = millis(n), ft8_flag = 1, FT_8_counter = 0, syncFlag = true, nothing else
 *   (synchronises).  The caller's clock decides when: the firmware calls it once second() % 15 turns 0.
 * The FT8 memory -- 16 int32 scalars {n, syncFlag, ft8_flag, DSP_Flag, FT_8_counter, dataLoop, leftover, start_time, half
 * being written, 7 zeros} and the 3072 buffer words per channel -- is the context's own: allocated at first use, at
 * power-on values (all zero) after t41rx_reset() and after t41rx_set_state(), and NOT part of the checkpoint:
 * t41rx_state_bytes() and the section mask are unchanged.  Its record is t41rx_ft8_state_bytes() / _get_state / _set_state:
 * a header of 8 int32 {magic "T41F", ABI, n_channels, words per channel = 3088, 0, 0, 0, 0}, then [n_channels][3088] int32.
 * _set_state refuses (T41RX_ERR_STATE, nothing written) another size or header, dataLoop outside 0..14, leftover outside
 * 0..3, FT_8_counter outside 0..91 (92 only next to ft8_flag 0, where the firmware leaves it between a slot's last block
 * and the restart), a flag or `half` outside 0 / 1, a non-zero reserved word, a buffer word outside -32768..32767. */
#define T41RX_FT8_ROW_BYTES 368    /* ft8_buffer */
#define T41RX_FT8_BLOCK_BYTES 1472 /* offset_step */
#define T41RX_FT8_SLOT_BLOCKS 92   /* ft8_msg_samples */
#define T41RX_FT8_MAX_FRAMES 1380
#define T41RX_FT8_STATE_WORDS 3088
T41RX_API int t41rx_set_ft8_tables(t41rx_ctx *ctx, const float *window, const float *mag_db);
T41RX_API int t41rx_set_ft8(t41rx_ctx *ctx, int on, uint8_t *d_power, int32_t *d_status, int max_frames);
T41RX_API int t41rx_get_ft8(const t41rx_ctx *ctx);
T41RX_API int t41rx_set_ft8_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den);
T41RX_API int t41rx_ft8_sync(t41rx_ctx *ctx, const uint8_t *channels, int n);
T41RX_API size_t t41rx_ft8_state_bytes(const t41rx_ctx *ctx);
T41RX_API int t41rx_ft8_get_state(t41rx_ctx *ctx, void *host_buf, size_t bytes);
T41RX_API int t41rx_ft8_set_state(t41rx_ctx *ctx, const void *host_buf, size_t bytes);

/* ---- FT8 from 12 kS/s audio: the collector of DEMOD_FT8_WAV (Process.cpp:278-335, ft8.cpp:259-268, :1359-1374) ----
 * For a caller who already has audio -- WSJT-X style 12 kHz recordings, another receiver's audio -- the firmware's WAV mode
 * feeds the same ft8_dsp_buffer without the receive chain: 128 samples at 12 kS/s per ProcessIQData().  These entry points
 * run it on the FT8 memory, the d_power halves and the d_status words of t41rx_set_ft8() (which must be on); the receive
 * path does not run, and t41rx_ft8_decode_*() reads the finished half as it does behind the live stage.  Per channel and
 * frame of 128 samples, in the firmware's order:
 *   q = arm_float_to_q15(x), truncating and saturating (NaN -> 0); int16 samples are taken as they are (readWave()'s
 *     raw / 32768.0f through that conversion is the identity);
 *   for i < 68 and k = i + 68 * dataLoop: buf[k] = buf[k + 1024]; buf[1024 + k] = buf[2048 + k]; buf[2048 + k] =
 *     q[(i * 15) >> 3].  No leftover, no last cell, no syncFlag gate, no DSP_Flag: words 1020..1023, 2044..2047 and
 *     3068..3071 keep what the record held;
 *   ++dataLoop == 15: dataLoop = 0 and process_FT8_FFT() unconditionally (ft8_flag is not asked): the block's 1472 bytes at
 *     1472 * FT_8_counter of the half being written, FT_8_counter++; at 92 ft8_flag = 0, the frame's status reports 1 + that
 *     half, `half` flips and FT_8_counter = 0.  update_synchronization() is never called;
 *   n advances (a 128-sample frame lasts the 32 / 3 ms of a live one); syncFlag, DSP_Flag, leftover and start_time stay.
 * From a power-on record a slot completes in frame 1379 (counted from 0) and the next one starts in the other half.  A
 * record with FT_8_counter at 92 (the live stage leaves it there next to ft8_flag 0; the firmware always passes through
 * setupFT8Wav() first) would index past the half: such a block writes nothing and the counter stays until _begin / _end.
 * The x2 interpolation for listening (Process.cpp:293-297), the pacing by the audio queues and the SD card stay with the
 * caller.
 * t41rx_ft8_audio_device_q15() / _device(): device buffers [n_channels][n_frames * 128], int16 or float, ALWAYS
 *   channel-major: the input map (t41rx_set_input_map) and t41rx_set_buffer_layout() do not apply to these entries.  Float
 *   samples go through arm_float_to_q15.  d_status gets [n_channels][n_frames][4] as from a process call.  On the default
 *   stream, without synchronising.  T41RX_ERR_ARG -- nothing launched, nothing in the FT8 memory, d_power or d_status
 *   changed -- while FT8 receive is off, before the tables are loaded, for n_frames < 1, n_frames > max_frames of
 *   t41rx_set_ft8(), n_frames > T41RX_FT8_MAX_FRAMES, a NULL pointer or one not aligned to its sample type.
 * t41rx_ft8_audio_host_q15() / _host(): the same from host arrays; synchronises.
 * t41rx_ft8_audio_begin(): setupFT8Wav()'s FT_8_counter = 0 on the channels whose byte is non-zero (host array of n =
 *   n_channels bytes; NULL = all).  t41rx_ft8_audio_end(): the mode's exit (Process.cpp:339-342), syncFlag = 0,
 *   FT_8_counter = 0, ft8_flag = 0.  Neither touches dataLoop or anything else, as in the firmware; both synchronise.
 * The receive path's audio, t41rx_state_bytes() and every checkpoint are untouched; t41rx_ft8_get_state / _set_state carry
 * everything, as before. */
#define T41RX_FT8_AUDIO_FRAME 128
T41RX_API int t41rx_ft8_audio_device_q15(t41rx_ctx *ctx, const int16_t *d_pcm, int n_frames);
T41RX_API int t41rx_ft8_audio_device(t41rx_ctx *ctx, const float *d_audio, int n_frames);
T41RX_API int t41rx_ft8_audio_host_q15(t41rx_ctx *ctx, const int16_t *pcm, int n_frames);
T41RX_API int t41rx_ft8_audio_host(t41rx_ctx *ctx, const float *audio, int n_frames);
T41RX_API int t41rx_ft8_audio_begin(t41rx_ctx *ctx, const uint8_t *channels, int n);
T41RX_API int t41rx_ft8_audio_end(t41rx_ctx *ctx, const uint8_t *channels, int n);

/* ---- FT8 decode of a finished slot (ft8.cpp:270-616, 669-703, 727-790) ----
 * find_sync(), and for every candidate of its heap extract_likelihood(), bp_decode(), pack_bits() and the CRC check, on a
 * waterfall that stays on the device: [92 blocks][4 = 2 * time_sub + freq_sub][368 bins] uint8 per channel and slot, the
 * layout t41rx_set_ft8()'s d_power has per half.  In the firmware's order and arithmetic:
 *   find_sync(): alt 0..3, time_offset -7..19, freq_offset 48..359 (ft8_min_bin .. 368 - 9); the score is the sum of
 *     8 * p8[kCostas_map[k]] - (p8[0] + .. + p8[7]) over the Costas symbols (at 0, 36, 72) that fall inside blocks 0..91,
 *     divided by their number as C divides (toward zero); score < min_score skips; the min-heap is replayed as written
 *     (eviction only on score > heap[0].score, heap[0] = heap[last] and heapify_down, insertion and heapify_up with >=).
 *     The candidates come out as the heap ARRAY in array order, the order ft8_decode() walks: not sorted, and which of
 *     several equal-minimum candidates survives follows from the replay.
 *   extract_likelihood(): max4 differences of the symbol's eight bins through kGray_map; variance = (sum2 - sum * sum *
 *     inv_n) * inv_n and norm_factor = sqrtf(16.0f / variance) in f32, one rounding per operation.  A variance of 0 gives
 *     inf and 0 * inf = NaN, a negative one NaN: NaN is carried as IEEE does, `zn > 0` is false, plain is all zero, and the
 *     all-zero codeword passes ldpc_check() and the CRC -- as in the firmware.
 *   bp_decode(): f32 in source order, no contraction, IEEE division; plain is the hard decision of the last iteration
 *     begun; n_errors = min_errors.  Then pack_bits(plain, 91) and crc() (CRC-14, polynomial 0x2757) over 82 bits of the
 *     masked copy.
 * t41rx_ft8_candidate: the Candidate as find_sync() leaves it, then n_errors, iterations = the index of the iteration whose
 *   check found 0 errors, else ldpc_iterations, flags bit 0: n_errors == 0, bit 1: the CRC matches (looked at only with bit
 *   0), a91 = pack_bits(plain, 91) with the CRC bits in place when bit 0 is set, else 0.  flags == 3 is what ft8_decode()
 *   hands to unpack77_fields(); freq_hz = (freq_offset + freq_sub / 2.0f) * 6.25f.
 * t41rx_ft8_result: num_candidates = find_sync()'s return, num_valid = the records with flags == 3, select as given;
 *   records from num_candidates on are zero.
 * t41rx_set_ft8_decode_tables(): kCostas_map[7], kGray_map[8], kNm[83][7], kMn[174][3], kNrw[83] from ft8_constants.cpp
 *   (host arrays, copied; synchronises).  The library has no table of its own.  T41RX_ERR_ARG, nothing written, for NULL,
 *   a kCostas_map or kGray_map entry above 7, kNrw outside 1..7, kNm[i][j < kNrw[i]] outside 1..174, kMn outside 1..83, or
 *   a bit i and j for which check kMn[i][j] does not list bit i exactly once (and the converse): these keep the kernels'
 *   indexing inside their arrays.
 * t41rx_set_ft8_decode(): kMax_candidates 1..20, kMin_score, kLDPC_iterations 1..50; defaults 20, 40, 10 (ft8.cpp:64-72).
 *   T41RX_ERR_ARG outside.  t41rx_get_ft8_decode() reads them back (any pointer may be NULL).
 * t41rx_set_ft8_decode_debug(): device pointers or NULL (the default).  While set, every decode call writes
 *   d_log174 [n_channels][20][174] f32, extract_likelihood()'s output, and d_plain [n_channels][20][174] uint8, bp_decode()'s;
 *   rows of unused candidates are zero.
 * t41rx_ft8_decode_device(): channel c reads d_waterfall + c * channel_stride_bytes + select[c] * T41RX_FT8_SLOT_BYTES,
 *   select[c] in {-1 = skip, 0, 1}; select is a host array of n == n_channels entries (copied before the call returns), or
 *   NULL for all 0.  d_waterfall == NULL: the context's own d_power (t41rx_set_ft8) with its stride of two slots, select
 *   naming the half (d_status word 2 - 1).  A skipped channel's result is zero with select = -1.  Enqueued on hip_stream,
 *   no sync; calls on one context belong on one stream.  It reads the waterfall and the tables and touches no state of the
 *   receive path.  T41RX_ERR_ARG, before anything is launched, for: no tables loaded, n != n_channels, a NULL d_results, a
 *   select entry outside {-1, 0, 1}, a NULL d_waterfall while FT8 receive is off, a waterfall or stride that is not
 *   4-byte aligned, a stride smaller than what the call reads.
 * t41rx_ft8_decode_host(): the same on the default stream, with the results copied to a host array; synchronises. */
#define T41RX_FT8_MAX_CANDIDATES 20 /* kMax_candidates */
#define T41RX_FT8_SLOT_BYTES 135424 /* 92 * 1472 */
typedef struct {
  int16_t score, time_offset, freq_offset;
  uint8_t time_sub, freq_sub;
  int16_t n_errors;
  uint8_t iterations, flags;
  uint8_t a91[12];
  uint8_t reserved[8];
} t41rx_ft8_candidate; /* 32 bytes */
typedef struct {
  int32_t num_candidates, num_valid, select, reserved;
  t41rx_ft8_candidate cand[T41RX_FT8_MAX_CANDIDATES];
} t41rx_ft8_result; /* 656 bytes */
T41RX_API int t41rx_set_ft8_decode_tables(t41rx_ctx *ctx, const uint8_t *costas, const uint8_t *gray, const uint8_t *nm,
                                const uint8_t *mn, const uint8_t *nrw);
T41RX_API int t41rx_set_ft8_decode(t41rx_ctx *ctx, int max_candidates, int min_score, int ldpc_iterations);
T41RX_API int t41rx_get_ft8_decode(const t41rx_ctx *ctx, int *max_candidates, int *min_score, int *ldpc_iterations);
T41RX_API int t41rx_set_ft8_decode_debug(t41rx_ctx *ctx, float *d_log174, uint8_t *d_plain);
T41RX_API int t41rx_ft8_decode_device(t41rx_ctx *ctx, const uint8_t *d_waterfall, size_t channel_stride_bytes, const int8_t *select,
                            int n, t41rx_ft8_result *d_results, void *hip_stream);
T41RX_API int t41rx_ft8_decode_host(t41rx_ctx *ctx, const uint8_t *d_waterfall, size_t channel_stride_bytes, const int8_t *select,
                          int n, t41rx_ft8_result *results);

/* ---- receiver groups: the FT8 map -- FT8 receive only on the channels that ask (ABI 5) ----
 * FT8 receive was the one large stage still context-wide: a workgroup on every channel, d_power of 270 KB per channel,
 * and a refusal as soon as any loaded parameter set was not USB.  The map is the output map's idea: a row per channel,
 * or none.  New entry points: no call above changes what it does, and a context that sets no map launches what it
 * always launched.
 * The rule: FT8 receive runs on channel c in a call exactly when the context's switch (t41rx_set_ft8) is on and
 * row_of_channel[c] >= 0.  A listed channel is processed exactly as the same channel of a context without a map: its
 * status words, its power bytes and its FT8 memory are bit for bit the same; only their place differs -- d_power is
 * [n_rows][2][92 * 1472], d_status [n_rows][n_frames][4], and channel c writes row row_of_channel[c].  A channel with -1 is
 * processed as with FT8 off: its FT8 memory stays exactly as it was (n included) and no row is written for it.  A row no
 * channel names is never written.  A map that lists nobody is allowed: the stage then launches nothing.  Which kernels a
 * call runs stays a function of the context's switches, as with the stage map.
 * The FT8 memory and its record stay [n_channels][3088]: t41rx_ft8_state_bytes / _get_state / _set_state, t41rx_ft8_sync,
 * t41rx_ft8_audio_begin and _end keep addressing channels and are unchanged.
 * USB per channel: with a map loaded a process call asks only the listed channels for T41RX_DEMOD_USB, each against its
 * own effective set -- set 0, plain or staged sets alike --, and the refusal (T41RX_ERR_UNSUPPORTED) names the first
 * offending channel and its set.  Without a map the refusals of t41rx_set_ft8 stand as they were.
 * The audio entries (t41rx_ft8_audio_*): under a map pcm is [n_rows][n_frames * 128]; row r feeds the channel that names it,
 * and a row nobody names is not read.
 * The decode: with d_waterfall == NULL (the context's own d_power) and a map loaded, t41rx_ft8_decode_* work by row:
 * n == t41rx_ft8_rows(); select, the results and the debug buffers are [n_rows]...; row r reads d_power + r * two slots +
 * select[r] * T41RX_FT8_SLOT_BYTES.  With a caller's own d_waterfall everything stays by channel as ever.
 * The map is configuration, like the stage map: it is in no checkpoint and survives t41rx_reset, t41rx_set_state,
 * t41rx_set_params and t41rx_set_coeffs.  fft_length 512 only: T41RX_ERR_UNSUPPORTED at a long fft_length.
 * The known remainder: the demod tap the stage reads and the hand-over buffer stay [n_channels] -- the fused front end
 * writes them for every channel --, so the tap is now the larger allocation of a short list.
 * t41rx_set_ft8_map(): row_of_channel is a host array of n == n_channels entries, each -1 or a row in [0, n_rows).  NULL
 *   with n == 0 and n_rows == 0 removes the map.  Everything is checked on the host before anything changes; a refused
 *   call leaves the previous map in place and t41rx_last_error() names the entry: T41RX_ERR_ARG for n != n_channels,
 *   n_rows outside 1..n_channels, an entry outside [-1, n_rows), a row named twice, and -- while FT8 receive is on --
 *   n_rows different from the current t41rx_ft8_rows(): the buffers given to t41rx_set_ft8 are sized by the rows, so the
 *   caller switches FT8 off, sets the map, and switches FT8 on with buffers of the new size.  Removing the map while FT8
 *   is on is held to the same rule against n_channels.  At equal n_rows the map may change between any two calls (a
 *   skimmer moves its FT8 decoders).  Synchronises the device, then uploads (the ordering rule of t41rx_set_input_map).
 * t41rx_get_ft8_map(): returns 1 with a map set, 0 with none (negative: an error status).  row_of_channel_out, n ==
 *   n_channels entries, receives the map, or 0, 1, .. with none; n_rows_out receives t41rx_ft8_rows(); either may be NULL.
 * t41rx_ft8_rows(): n_rows, or n_channels with no map: the rows of d_power, d_status and the audio entries' pcm. */
T41RX_API int t41rx_set_ft8_map(t41rx_ctx *ctx, const int32_t *row_of_channel, int n, int n_rows);  /* NULL, 0, 0: remove */
T41RX_API int t41rx_get_ft8_map(const t41rx_ctx *ctx, int32_t *row_of_channel_out, int n, int *n_rows_out);
T41RX_API int t41rx_ft8_rows(const t41rx_ctx *ctx);

/* ---- the panadapter: ShowSpectrum()'s pixels and waterfall row, DrawSmeterBar()'s dBm (Display.cpp:240-504, 955-1030) ----
 * A stage of the receive path, default off, fft_length 512: per channel the display FFT of t41rx_set_display_spectrum(),
 * and behind it, in the firmware's integer arithmetic, what ShowSpectrum() draws from -- at the firmware's cadence.  A
 * context that does not switch it on is unchanged; with it on, the audio of every call is bit for bit the audio without it.
 *
 * Cadence.  The stage counts the frames of the process calls, n = 0 at t41rx_set_panadapter() and t41rx_reset(); the
 *   counter is host-side configuration (t41rx_get_panadapter / t41rx_set_panadapter_counter), in no checkpoint.  Frame n
 *   is an update frame -- one with updateDisplayFlag == 1 -- when n % update_period == update_phase; the firmware sets the
 *   flag once per sweep of 511 ProcessIQData() calls (Display.cpp:259-267): update_period 511.  Every other frame does no
 *   display work (Process.cpp:185-187, 212, 550, 791; FFT.cpp:209): no display FFT, no zoom filter, ring, low-pass or pixel
 *   memory advances, and audioMaxSquaredAve (the path's own word, in the checkpoint as before) stays -- while the stage is
 *   on it advances on update frames only.  At spectrumZoom 1..4 the zoom chain therefore sees the update frames' samples
 *   back to back: the firmware's own discontinuity.  A process call without an update frame launches exactly the kernels
 *   of a context without the stage; the update frames of a call are frames f with (n0 + f) % update_period == update_phase,
 *   n0 the counter in front of the call, and their rows k = 0, 1, .. are written in frame order.
 * Per row, x = 0 .. 511 (x = 256 is DC, as for FFT_spec):
 *   spec[x]      FFT_spec: t41rx_set_display_spectrum()'s transform (un-smoothed at spectrumZoom 0, smoothed at 1..4)
 *   pixel[x]     pixelnew[x] = baseOffset + pixel_offset + (int16_t)(dBScale * log10f_fast(FFT_spec[x])) (FFT.cpp:157, 245),
 *                {dBScale, baseOffset} = displayScale[currentScale] (Display.cpp:127-135)
 *   y_new[x]     spectrumNoiseFloor - pixelnew[x] - currentNF held to [100, 249] = [SPECTRUM_TOP_Y, SPECTRUM_BOTTOM]
 *   y_old[x]     spectrumNoiseFloor - pixelold[x] - oldNF likewise: pixelold[] = the row before's pixelnew[] (zero at
 *                power-on), oldNF = the row before's currentNF, or this row's on the first row after t41rx_set_panadapter()
 *                or t41rx_reset() (newSpectrumFlag, Display.cpp:250-256, 474)
 *   waterfall[x] gradient[230 - y_new[x] held to 0 .. 116] for x = 0 .. 510 (Display.cpp:460-466); the firmware never
 *                writes waterfall[511]: 0 here
 *   audio_spect  audioSpectBuffer[1024] of the update frame, as t41rx_set_audio_spectrum() writes it
 *   smeter[4]    audioMaxSquared, (float)AudioMaxIndex, audioMaxSquaredAve behind the frame, and dbm: the TCVSDR_SMETER
 *                form of Display.cpp:980-981 in its operand types and order -- dbm_calibration (22) + gainCorrection +
 *                (float32_t)attenuator + slope (10) * log10f_fast(audioMaxSquaredAve) + cons (-92) in float, then
 *                - (float32_t)RFgain * 1.5 - rfGainAllBands in double, stored to a float, without contraction (whether the
 *                firmware's compiler contracts slope * log + sum is not pinned: DESIGN.md).  RFgain and rfGainAllBands
 *                are the params' (under a panadapter map: the channel's own set's, t41rx_set_panadapter_map).
 *   The drawing itself, map() for the bar's length, audioYPixel and the control-app records stay with the caller.
 * The stage's memory -- the display state, pixelold[512], oldNF and newSpectrumFlag per channel -- is the context's own,
 *   like the calibration memory: zero at t41rx_set_panadapter(on) and t41rx_reset(), NOT part of the checkpoint
 *   (t41rx_state_bytes(), the section mask and the ABI are unchanged) and left alone by t41rx_set_state().
 * t41rx_set_panadapter_tables(): gradient[] (Display.cpp:148-161), n == 117 uint16 colour words, a host array, copied
 *   (synchronises).  The library has no table of its own.  T41RX_ERR_ARG for NULL or n != 117.
 * t41rx_set_panadapter(): on = 0 switches the stage off (the other arguments are ignored).  out: device pointers of the
 *   caller's row buffers [n_channels][max_rows][...] ([t41rx_panadapter_rows()][max_rows][...] under a panadapter map,
 *   below), each 16-byte aligned or NULL (not written); the struct is copied.
 *   A call with k update frames writes rows 0 .. k-1 of every channel and leaves the others alone.  The stage's own tap
 *   buffer holds max_rows rows (16 KiB each per channel), not frames.  T41RX_ERR_ARG, nothing changed: no table loaded,
 *   spectrumZoom or currentScale outside 0..4, pixel_offset or spectrumNoiseFloor outside int16, update_period < 1,
 *   update_phase outside [0, update_period), max_rows < 1, a NULL out, an unaligned pointer.  T41RX_ERR_UNSUPPORTED: a
 *   long fft_length; t41rx_set_display_spectrum() or t41rx_set_audio_spectrum() set -- and either of those is refused
 *   likewise while the stage is on: each tap has one owner.  The firmware's values: spectrumNoiseFloor 247 (gwv.cpp:18),
 *   update_period 511.  Synchronises.
 * t41rx_set_panadapter_levels(): currentNoiseFloor[currentBand] and bands[currentBand].gainCorrection per channel, host
 *   arrays of n_channels entries, copied (NULL = zeros; zeros until first set), and `attenuator` (Display.cpp:146).  They
 *   hold from the next process call: a noise floor changed between two rows gives the next row oldNF != currentNF.
 *   T41RX_ERR_ARG for a noise floor outside int16 or a non-finite correction.  Synchronises.
 * A process call (every mode, f32 and q15 entries, both layouts, with an input map; the device forms enqueue without a
 *   sync) that would hold more than max_rows update frames is refused with T41RX_ERR_ARG and processes nothing.
 * t41rx_get_panadapter(): 1 / 0 = the stage is on / off (negative: an error status); any pointer may be NULL.
 *   frame_counter: n behind the last call; rows_written: the rows the last process call wrote; first_row_frame: the n of
 *   its row 0, or -1 when it wrote none.  t41rx_set_panadapter_counter(): n >= 0 (T41RX_ERR_ARG otherwise). */
typedef struct t41rx_panadapter_out {
  int16_t  *pixel;       /* [n_channels][max_rows][512]  pixelnew */
  int16_t  *y_new;       /* [n_channels][max_rows][512] */
  int16_t  *y_old;       /* [n_channels][max_rows][512] */
  uint16_t *waterfall;   /* [n_channels][max_rows][512] */
  float    *spec;        /* [n_channels][max_rows][512]  FFT_spec */
  float    *audio_spect; /* [n_channels][max_rows][1024] audioSpectBuffer */
  float    *smeter;      /* [n_channels][max_rows][4]    audioMaxSquared, AudioMaxIndex, audioMaxSquaredAve, dbm */
} t41rx_panadapter_out;
#define T41RX_PANADAPTER_GRADIENT 117
#define T41RX_PANADAPTER_NOISE_FLOOR 247 /* spectrumNoiseFloor, gwv.cpp:18 */
#define T41RX_PANADAPTER_PERIOD 511      /* SPECTRUM_RES - 1 ProcessIQData() calls per sweep, Display.cpp:259 */
T41RX_API int t41rx_set_panadapter_tables(t41rx_ctx *ctx, const uint16_t *gradient, int n);
T41RX_API int t41rx_set_panadapter(t41rx_ctx *ctx, int on, int spectrumZoom, int currentScale, int pixel_offset, int spectrumNoiseFloor,
                         int update_period, int update_phase, const t41rx_panadapter_out *out, int max_rows);
T41RX_API int t41rx_set_panadapter_levels(t41rx_ctx *ctx, const int32_t *noise_floor, const float *gain_correction, int attenuator);
T41RX_API int t41rx_get_panadapter(const t41rx_ctx *ctx, int64_t *frame_counter, int32_t *rows_written, int64_t *first_row_frame);
T41RX_API int t41rx_set_panadapter_counter(t41rx_ctx *ctx, int64_t n);

/* ---- receiver groups: the panadapter map -- display rows only for the channels that ask (ABI 5) ----
 * A skimmer of thousands of receivers shows a spectrum for the one or two somebody looks at, and monitors the beacons
 * with five.  Without a map the panadapter taps 16 KiB per row on every channel, runs a wave per channel, wants seven
 * row buffers of n_channels rows, and refuses smeter rows as soon as a loaded parameter set differs from set 0 in RFgain
 * or rfGainAllBands.  The map is the FT8 map's idea: a row per channel, or none.  New entry points: no call above changes
 * what it does, and a context that sets no map launches what it always launched.
 * The rule: the panadapter stage runs on channel c in a call exactly when the context's switch (t41rx_set_panadapter)
 * is on and row_of_channel[c] >= 0.  A listed channel is processed exactly as the same channel of a context without a
 * map: its rows 0 .. k-1 of a call with k update frames, in all seven buffers, its panadapter memory and the path's
 * audioMaxSquaredAve are bit for bit the same; only the rows' place differs -- the buffers of t41rx_panadapter_out are
 * [n_rows][max_rows][...], and channel c writes out.*[row_of_channel[c]][0 .. k-1].  A channel with -1 is processed as
 * with the panadapter off: it writes no tap, audioMaxSquaredAve stays, its panadapter memory stays exactly as it was and
 * no row is written for it.  A row no channel names is never written; rows >= k of a named row are left alone as ever.
 * A map that lists nobody is allowed: a call then launches exactly the kernels of a context without the stage, and the
 * frame counter still counts (t41rx_get_panadapter's rows_written stays the call's number of update frames: the rows a
 * listed channel would have written).  The audio of every call is bit for bit the audio without the stage, as before.
 * The beacon monitor runs on the listed channels only, each reading the smeter row its channel names.  d_snr
 * [n_channels][18], d_events [n_channels][max_rows][4] and the record (t41rx_beacon_state_bytes / _get_state /
 * _set_state, t41rx_get_beacon) keep addressing channels; an unlisted channel's record, snr row and event rows are not
 * touched, and a channel listed later continues from the record it has.
 * Sizes under a map: the stage's own taps hold n_rows x max_rows rows; the panadapter memory, the levels
 * (t41rx_set_panadapter_levels: n_channels entries) and the frame counter stay per channel / per context.
 * dBm per channel: with a map loaded each listed channel's dbm takes RFgain and rfGainAllBands from its own effective
 * parameter set -- set 0, plain sets and sets loaded with T41RX_SETS_STAGES alike --, so a listed channel's smeter rows
 * equal those of a context created with its set, and the process call's refusal of sets that differ in the two gains
 * is not raised.  Without a map that refusal stands word for word.
 * The map is configuration, like the stage map: it is in no checkpoint and survives t41rx_reset, t41rx_set_state,
 * t41rx_set_params and t41rx_set_coeffs (the listed channels' gains follow a changed set).  fft_length 512 only:
 * T41RX_ERR_UNSUPPORTED at a long fft_length.  The two display side outputs (t41rx_set_display_spectrum,
 * t41rx_set_audio_spectrum) have no map.
 * t41rx_set_panadapter_map(): row_of_channel is a host array of n == n_channels entries, each -1 or a row in [0, n_rows).
 *   NULL with n == 0 and n_rows == 0 removes the map.  Everything is checked on the host before anything changes; a
 *   refused call leaves the previous map in place and t41rx_last_error() names the entry: T41RX_ERR_ARG for n !=
 *   n_channels, n_rows outside 1..n_channels, an entry outside [-1, n_rows), a row named twice, and -- while the
 *   panadapter is on -- n_rows different from the current t41rx_panadapter_rows(): the buffers given to
 *   t41rx_set_panadapter are sized by the rows, so the caller switches the stage off, sets the map, and switches it on
 *   with buffers of the new size.  Switching off is refused while the beacon monitor is on, so the order is: beacon off,
 *   panadapter off, map, panadapter on, beacon on.  Removing the map while the panadapter is on is held to the same rule
 *   against n_channels.  At equal n_rows the map may change between any two calls (somebody looks at another receiver).
 *   Synchronises the device, then uploads (the ordering rule of t41rx_set_input_map); a process call uploads nothing.
 * t41rx_get_panadapter_map(): returns 1 with a map set, 0 with none (negative: an error status).  row_of_channel_out, n
 *   == n_channels entries, receives the map, or 0, 1, .. with none; n_rows_out receives t41rx_panadapter_rows(); either
 *   may be NULL.
 * t41rx_panadapter_rows(): n_rows, or n_channels with no map: the rows of the seven buffers of t41rx_panadapter_out. */
T41RX_API int t41rx_set_panadapter_map(t41rx_ctx *ctx, const int32_t *row_of_channel, int n, int n_rows);  /* NULL, 0, 0: remove */
T41RX_API int t41rx_get_panadapter_map(const t41rx_ctx *ctx, int32_t *row_of_channel_out, int n, int *n_rows_out);
T41RX_API int t41rx_panadapter_rows(const t41rx_ctx *ctx);

/* ---- the beacon monitor: BeaconLoop()'s per-beacon SNR table (Beacon.cpp:204-208, 455-569) ----
 * A stage behind the panadapter stage, default off.  The firmware calls BeaconLoop() once per loop() pass, which is once
 * per ShowBeacon() sweep, and the only thing it reads is the sweep's dbm: here one BeaconLoop() call per panadapter row,
 * rows 0 .. k-1 of a process call in order, dbm = the row's smeter[3], the clock evaluated at the row's frame number n
 * (the panadapter's counter).  A process call that wrote no row launches nothing for the stage, and a context that does
 * not switch it on launches exactly what it launched before.  The audio of every call, t41rx_state_bytes(), the section
 * mask and the ABI are unchanged.
 *
 * A channel is one receiver on one band: monitorFreq[] of a channel has exactly one band set, band[c] in 0 .. 4 (20, 17,
 * 15, 12, 10 m); it cannot retune.  The firmware's walk over the other four bands is kept as the four calls of `band++`
 * that find nothing to do.  Five channels, one per band, fill the 18 x 5 table the firmware needs over 15 minutes for in
 * one cycle of three.  The library carries no beacon names, maps or bearings: indices 0 .. 17 are the interface.
 * Clock.  slot(n) = ((t0_ms + floor(n * num / den)) / 1000 % 180) / 10 in int64 -- GetBeacon20mNow() -- and
 *   GetBeaconNow(band) = slot - band, plus 18 if negative.  t0_ms in [0, 180000), num >= 0, den > 0; the default 0, 32, 3
 *   is one frame of 2048 samples at 192 kS/s, the CW and FT8 stages' clock.  n is the row's update frame, the FIRST frame
 *   of the firmware's sweep; a caller who wants the time of the sweep's end folds the sweep's length into t0_ms.
 *   t41rx_set_beacon() reads the clock (for currentBeacon): set the clock first.  T41RX_ERR_ARG otherwise, and when
 *   n * num would not fit 64 bits (also from a process call, which then processes nothing).
 * Per call of BeaconLoop(), the synced branch as written:
 *   count == 0 && changeBandFlag: band++, wrapping at 5; on the channel's own band changeBandFlag = false.
 *   count > 0: snrCount++; `if (dbm < min) min = dbm; if (dbm > max) max = dbm;` (plain comparisons: a NaN moves neither,
 *     -inf moves min only); on GetBeaconNow(band) != currentBeacon: snr[that NEW beacon] = (snrCount == 23) ? 0 :
 *     (max - min > 0 ? max - min : 0), a float subtraction; snrCount = 0, currentBeacon = it, min = 0, max = -1000,
 *     count++, and count > 18 gives count = 0, changeBandFlag = true.  The firmware's quirks stay: the slot that ended is
 *     booked under the beacon that just began, the call that sees the change has already entered min / max, and a slot
 *     of exactly 23 calls reads as noise.
 *   count == 0 && !changeBandFlag: on GetBeaconNow(band) != currentBeacon count++ (currentBeacon stays).
 *   mode 0 is this cycle: 18 records, then the walk over the four other bands and a wait for the next change -- with
 *     one monitored band it loses the slots the firmware loses.  mode 1 is continuous: count is held at 1 once the first
 *     change has been seen, so every later change records; everything else is identical.
 * Switching on is the unsynced branch (Beacon.cpp:610-614) at the panadapter's n: currentBeacon = slot(n), count = 0,
 *   changeBandFlag = true, band = the channel's, min = 0, max = -1000, snrCount = 0, and a table of zeros (BeaconInit()).
 *   t41rx_reset() does the same at n = 0.  t41rx_set_state() leaves the stage alone.
 * t41rx_set_beacon(): band: host array of n_channels entries, copied.  d_snr: device float [n_channels][18], the channel's
 *   column beaconSNR[.][band]; written by the stage only, it persists across calls (zeroed at switch-on and reset).
 *   d_events: device int32 [n_channels][max_rows][4], 16-byte aligned, or NULL: per row {beacon recorded or -1, snrCount as
 *   the call compared it (before a record clears it), count behind the call, band behind the call}; a call with k rows
 *   writes records 0 .. k-1.  on = 0 switches the stage off (the other arguments are ignored).  T41RX_ERR_ARG, nothing
 *   changed: a band outside 0..4, a mode outside 0..1, a NULL band, a NULL or unaligned d_snr, an unaligned d_events,
 *   max_rows smaller than the panadapter's.  T41RX_ERR_UNSUPPORTED: the panadapter stage off, or on without an smeter
 *   buffer.  While the stage is on, t41rx_set_panadapter() refuses to switch the panadapter off or on again without
 *   smeter (T41RX_ERR_UNSUPPORTED) or with more max_rows than the stage's (T41RX_ERR_ARG).  Synchronises.
 * t41rx_get_beacon(): 1 / 0 = the stage is on / off (negative: an error status).  On: synchronises and copies the table
 *   [n_channels][18] and the status [n_channels][8] int32 {min as float bits, max as float bits, snrCount, count,
 *   changeBandFlag, currentBeacon, band, the channel's band} to host arrays; either may be NULL.
 * The stage's record is t41rx_beacon_state_bytes() / _get_state / _set_state: a header of 8 int32 {magic "T41B", ABI,
 *   n_channels, words per channel = 26, 0, 0, 0, 0}, then per channel the 8 status words and snr[18].  Both need the stage
 *   on (T41RX_ERR_STATE otherwise); _set_state refuses (T41RX_ERR_STATE, nothing written) another size or header, a
 *   negative snrCount, count outside 0..18, changeBandFlag outside 0 / 1, currentBeacon outside 0..17, a band outside
 *   0..4, and a channel that listens (count > 0 or changeBandFlag 0) on a band that is not its own.  The record's bands
 *   replace t41rx_set_beacon()'s; mode, clock and buffers are configuration and stay.
 * DisplayBeacons(), DisplayBeaconsSNR() and T41BeaconSendData(), the maps and bearings, and BeaconInit() / BeaconExit()'s
 *   retuning and 500 .. 1500 Hz filter (FLoCut / FHiCut of the params) stay with the caller. */
#define T41RX_BEACON_COUNT 18
#define T41RX_BEACON_BANDS 5
#define T41RX_BEACON_STATUS_WORDS 8
T41RX_API int t41rx_set_beacon(t41rx_ctx *ctx, int on, int mode, const int32_t *band, float *d_snr, int32_t *d_events, int max_rows);
T41RX_API int t41rx_set_beacon_clock(t41rx_ctx *ctx, int32_t t0_ms, int32_t num, int32_t den);
T41RX_API int t41rx_get_beacon(t41rx_ctx *ctx, float *snr, int32_t *status);
T41RX_API size_t t41rx_beacon_state_bytes(const t41rx_ctx *ctx);
T41RX_API int t41rx_beacon_get_state(t41rx_ctx *ctx, void *host_buf, size_t bytes);
T41RX_API int t41rx_beacon_set_state(t41rx_ctx *ctx, const void *host_buf, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* T41RX_H */
