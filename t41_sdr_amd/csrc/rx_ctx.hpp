// t41_sdr_amd/csrc/rx_ctx.hpp -- the receive context (struct t41rx_ctx) and what the host files of the receive side share.
// Private to them: rx_host.cpp (the core and the process call), rx_state.cpp (checkpoints and reset) and one file per
// stage family -- rx_audio.cpp, rx_cw.cpp, rx_ft8.cpp, rx_ft8_decode.cpp, rx_display.cpp, rx_beacon.cpp, rx_cal.cpp -- and
// rx_sets.cpp (the parameter sets), rx_outmap.cpp (the output map), rx_stagemap.cpp (the stage map) and
// rx_stageparams.cpp (the CW filter map and the equalizer level map); the FT8 map lives with its stage in rx_ft8.cpp, the
// panadapter map with its stage in rx_display.cpp.  Each
// stage family holds its part of the context in a struct of its own below, and exports the few functions the process
// call and the checkpoint table name.  No kernel is compiled into a host file: they see the kernels through the
// *_kernels.hpp headers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "beacon_kernels.hpp"
#include "cw_kernels.hpp"
#include "dev_buf.hpp"
#include "eq_kernels.hpp"
#include "ft8_decode_kernels.hpp"
#include "ft8_kernels.hpp"
#include "last_error.hpp"
#include "nb_kernels.hpp"
#include "nr_kernels.hpp"
#include "rx_experiments.hpp"
#include "rx_internal.hpp"
#include "rx_kernels.hpp"
#include "rx_nrmap.hpp"
#include "rx_stagemap.hpp"
#include "rx_stageparams.hpp"
#include "rx_stagesets.hpp"

// the product's host side is never a diagnostic build; what the KERNEL objects were built as is asked at run time
// (kernel_build_flags(), rx_dispatch.hip): tools/build_variant.sh links these very objects with diagnostic kernels
static_assert(T41RX_EXPERIMENT == 0 && t41::kKernelBuildFlags == 0, "the receive host is product code: build it without T41RX_EXPERIMENT / diagnostic switches");

namespace t41 {

// noise reduction / notch (Process.cpp:841-866): state of Xanr() and of the two spectral functions, window tables;
// allocated when a call first needs them
struct NrStage {
  DevBuf<float> d_anr, d_spec, d_tab;
  // the noise-reduction map (t41rx_set_nr_map; rx_nrmap.cpp): nrOptionSelect and ANR_notchOn per channel, the lists made
  // of them and of the stage map (rx_nrmap.hpp), and their device copy (nr_map_layout()).  Configuration like the stage
  // map: in no checkpoint, untouched by reset / set_state / set_params.  map_on == false: every channel takes the
  // context's params.nrOptionSelect / params.ANR_notchOn.
  bool map_on = false;
  std::vector<int32_t> kind_map, notch_map;  // [nchan] each (host)
  NrMapLists lists;
  DevBuf<int32_t> d_map;                     // allocated with the first map
};

// noise blanker (NB_on, Process.cpp:873-876; t41rx_set_noise_blanker): AltNoiseBlanking()'s last_frame_end per channel,
// two slots [2][nchan][kNbCarryPitch] (nb_kernel.hip); allocated when the blanker first runs
struct NbStage {
  int on = 0;
  DevBuf<float> d_carry;
  int sel = 0;  // the slot holding the current carry (flips with every blanker launch)
};

// receive equalizer (receiveEQFlag, Process.cpp:828-832; t41rx_set_receive_eq): the caller's band table, the levels
// (EEPROMData.equalizerRec, EEPROM.cpp:59: 100 each), and rec_EQ_Band1_state .. rec_EQ_Band14_state per channel
// [nchan][kEqStateFloats] (eq_kernel.hip), allocated when the equalizer first runs
struct EqStage {
  int on = 0;
  bool have_bands = false;
  float coef[kEqCoefs] = {};
  int32_t levels[kEqBands] = {100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100};
  DevBuf<float> d_state;
  // the level map (t41rx_set_receive_eq_map; rx_stageparams.cpp): equalizerRec per channel and its device form, the
  // signed level scales [nchan][kEqBands] as eq_run() makes them of `levels`.  Configuration like the stage map: in no
  // checkpoint, untouched by reset / set_state / set_params.  map_on == false: every channel takes `levels`.
  bool map_on = false;
  std::vector<int32_t> level_map;  // [nchan][kEqBands] (host)
  DevBuf<float> d_levels;          // allocated with the first map
};

// a stage's clock, millis(n) = t0 + floor(n * num / den): 2048 samples at 192 kS/s
struct StageClock {
  int32_t t0 = 0, num = 32, den = 3;
};

// CW receive (Process.cpp:878-913; t41rx_set_cw_tables / _filter / _detector): the caller's filter tables and decode
// FIR, CWFilterIndex (5 = off), decoderFlag with the caller's result buffer, and the stages' memories per channel
// [nchan][kCwStateFloats] (cw_kernel.hip), allocated when a CW stage first runs.  Both stages run only while
// params.xmtMode == T41RX_CW_MODE.
struct CwStage {
  int filter = kCwFilters;
  int det = 0;
  bool have_filters = false, have_fir = false;
  float coef[kCwFilters * kCwFilterCoefs] = {};
  float fir[kCwFirTaps] = {};
  float *out = nullptr;  // [nchan][n_frames][4]
  int frames = 0;        // frames per call `out` is sized for
  DevBuf<float> d_state;
  // the Morse decoder behind the detector (DoCWDecoding(), CWProcessing.cpp:519-639; t41rx_set_cw_decode_tree / _decoder /
  // _clock): the caller's bigMorseCodeTree, the switch with the caller's text buffer, the clock, and the decoder's words per
  // channel [nchan][kCwDecWords] (cw_kernels.hpp), allocated when the decoder first runs.  It runs exactly when the detector
  // runs and the switch is on.
  bool have_tree = false;
  uint8_t tree[kCwTreeChars + 3] = {};
  int dec = 0;
  int32_t *text = nullptr;  // [nchan][n_frames][2]
  int text_frames = 0;      // frames per call `text` is sized for
  StageClock clock;
  DevBuf<int32_t> d_dec;
  // the filter map (t41rx_set_cw_filter_map; rx_stageparams.cpp): CWFilterIndex per channel, the lists made of it and of
  // the output map (rx_stageparams.hpp), and their device copy -- four rows of cw_map_pitch(nchan) entries: the indices,
  // the filtered channels' list, the filtered and the unfiltered channels' rows.  Configuration like the stage map: in
  // no checkpoint, untouched by reset / set_state / set_params.  map_on == false: every channel takes `filter`.
  bool map_on = false;
  std::vector<int32_t> filter_map;  // [nchan] (host)
  CwFilterLists lists;
  DevBuf<int32_t> d_map;            // allocated with the first map
};
// a row of CwStage::d_map: nchan entries, up to a multiple of eight (cw_filter_map_kernel reads its list eight at a time)
inline size_t cw_map_pitch(int nchan) { return ((size_t)nchan + kCwChanPerWave - 1) / kCwChanPerWave * kCwChanPerWave; }
enum CwMapRow : int { kCwMapIndex = 0, kCwMapList, kCwMapRowsFiltered, kCwMapRowsPlain, kCwMapRows };

// FT8 receive up to the waterfall (Process.cpp:627-686, ft8.cpp:153-268; t41rx_set_ft8_tables / _ft8 / _ft8_clock /
// t41rx_ft8_sync): the caller's window and mag_db (device copies), arm_rfft_q15's tables, the switch with the caller's
// power and status buffers, the clock, and the FT8 memory per channel [nchan][kFt8Words] (ft8_kernels.hpp), allocated at
// first use.  The context's own: no checkpoint section (its record is t41rx_ft8_get_state / _set_state).  The stage reads
// the demodulated audio where the demod tap sits: d_aud24 when other stages split the chain, else the caller's demod tap
// buffer, else d_tap.
struct Ft8Stage {
  int on = 0;
  bool have_tables = false;
  uint8_t *power = nullptr;   // [nchan][2][kFt8HalfBytes]
  int32_t *status = nullptr;  // [nchan][n_frames][4]
  int frames = 0;             // frames per call `status` is sized for
  StageClock clock;
  DevBuf<int32_t> d_state;
  DevBuf<float> d_win, d_mag, d_tap;
  DevBuf<uint32_t> d_tab;
  int tap_frames = 0;
  // the FT8 map (t41rx_set_ft8_map; rx_ft8.cpp): the caller's row per channel, the rows d_power / d_status then hold, the
  // list of {channel, row} pairs made of it (rx_ft8map.hpp) and its device copy [nchan] pairs.  With a map `power` is
  // [rows][2][kFt8HalfBytes] and `status` [rows][n_frames][4]; the FT8 memory and the demod tap stay [nchan].
  // Configuration like the stage map: in no checkpoint, untouched by reset / set_state / set_params.  map_on == false:
  // no map, the stage runs on every channel and channel c writes row c.
  bool map_on = false;
  std::vector<int32_t> map;   // [nchan] (host)
  int rows = 0;
  std::vector<Ft8Pair> list;  // ascending by channel (host)
  DevBuf<Ft8Pair> d_list;     // allocated with the first map
};

// FT8 decode of a finished slot (ft8.cpp:270-616, 669-703, 727-790; t41rx_set_ft8_decode_tables / _ft8_decode /
// _ft8_decode_debug, t41rx_ft8_decode_device / _host): the caller's kCostas_map, kGray_map, kNm, kMn, kNrw as validated
// (device copy, with the positions worked out from them), kMax_candidates / kMin_score / kLDPC_iterations, the stage taps,
// and the call's `select` on its way to the device: a pinned copy, an event behind its upload (the next call waits for
// it before it overwrites the copy), the device array.  The decode reads the waterfall and the tables and touches no state.
struct Ft8Decode {
  bool have_tables = false;
  int max_candidates = T41RX_FT8_MAX_CANDIDATES, min_score = 40, iterations = 10;
  float *dbg_log174 = nullptr;
  uint8_t *dbg_plain = nullptr;
  DevBuf<Ft8DecodeTables> d_tab;
  DevBuf<int8_t> d_sel;
  DevBuf<t41rx_ft8_result> d_res;  // staging for t41rx_ft8_decode_host
  int8_t *h_sel = nullptr;         // pinned
  hipEvent_t sel_ev = nullptr;
};

// display FFT side output (t41rx_set_display_spectrum)
struct DisplayTap {
  float *spec = nullptr, *old = nullptr;  // caller's buffers
  DevBuf<float> d_pre, d_state;           // input tap [nchan][frames][4096], state [nchan][kDispFloats]
  int frames = 0, zoom = 0;
};

// the panadapter stage (ShowSpectrum() / DrawSmeterBar(), Display.cpp:240-504, 955-1030; t41rx_set_panadapter_tables /
// _panadapter / _panadapter_levels): the caller's gradient[] (device copy), the settings, the caller's row buffers, the
// levels per channel (device copies), the compact taps of a call's update frames [rows][max_rows][...] that the tap
// kernels write and panadapter_kernel reads, and the panadapter memory [nchan][kPanFloats] (rx_internal.hpp).  The
// context's own: no checkpoint section, t41rx_set_state() leaves it alone.  The frame counter lives here, on the host.
struct Panadapter {
  bool on = false, have_tables = false;
  t41rx_panadapter_out out{};
  int zoom = 0, scale = 0, pixel_offset = 0, floor_y = 0, period = 1, phase = 0, max_rows = 0;
  int attenuator = 0;
  int alloc_rows = 0;       // rows d_pre / d_max hold
  long long counter = 0;    // frames processed since the setter / t41rx_reset() / t41rx_set_panadapter_counter()
  int call_first = 0, call_rows = 0;  // of the call being prepared: its first update frame, their number
  int last_rows = 0;        // t41rx_get_panadapter(): rows the last call wrote, and the frame index of the first
  long long last_first = -1;
  DevBuf<uint16_t> d_grad;
  DevBuf<int32_t> d_nf;
  DevBuf<float> d_gc, d_pre, d_max, d_mem;
  // the panadapter map (t41rx_set_panadapter_map; rx_display.cpp): the caller's row per channel with its device copy
  // (RxArgs::tap_map), the rows the taps and the caller's buffers then hold, and the list of {channel, row, RFgain,
  // rfGainAllBands} entries made of it, of the parameter sets and of set 0 (rx_panmap.hpp) with its device copy [nchan]
  // entries -- made again when any of the three changes (pan_map_refresh).  With a map d_pre / d_max and the caller's seven
  // buffers are [rows][max_rows][...]; the memory and the levels stay [nchan].  Configuration like the stage map: in no
  // checkpoint, untouched by reset / set_state / set_params.  map_on == false: no map, the stage runs on every channel
  // and channel c writes row c.
  bool map_on = false;
  std::vector<int32_t> map;    // [nchan] (host)
  int rows = 0;
  int alloc_width = 0;         // rows of channels d_pre / d_max hold
  std::vector<PanEntry> list;  // ascending by channel (host)
  DevBuf<PanEntry> d_list;     // allocated with the first map
  DevBuf<int32_t> d_map;       // allocated with the first map
};

// the beacon monitor behind the panadapter (BeaconLoop(), Beacon.cpp:455-569; t41rx_set_beacon / _beacon_clock): the
// switch with the caller's table and event buffers, the mode, the channels' bands (host copy, for t41rx_reset()), the
// clock, and BeaconLoop()'s statics per channel [nchan][kBeaconWords] (beacon_kernels.hpp).  The context's own: no
// checkpoint section (its record is t41rx_beacon_get_state / _set_state).  It runs in the calls that wrote panadapter rows.
struct BeaconStage {
  bool on = false;
  int mode = 0, max_rows = 0;
  float *snr = nullptr;       // [nchan][18] (by channel under a panadapter map too: only the smeter rows go by row)
  int32_t *events = nullptr;  // [nchan][max_rows][4], or null
  std::vector<int32_t> band;  // [nchan]
  StageClock clock;
  DevBuf<int32_t> d_state;
};

// IQ calibration (ProcessIQData2() / PlotCalSpectrum(), Process2.cpp:352-397, 478-547; t41rx_set_calibration): its
// settings, a correction candidate per channel, and the calibration memory [nchan][kCalFloats] (cal_kernel.hip),
// allocated when calibration is first configured.  The context's own: no checkpoint section, no audio-path kernel
// touches it.
struct Calibration {
  bool on = false, per_channel = false;
  int zoom = 0, base = 0, lo0 = 0, lo1 = 0, width = 0;
  float dbscale = 0.0f;
  DevBuf<float> d_mem, d_corr;
};

// parameter sets (t41rx_set_param_sets; rx_sets.cpp): the extra sets 1..K with their designed blobs, the channels' table,
// and what the set kernels read -- the coefficient blocks [K + 1], the constant tables [K + 1][kTabEntries512], the first
// stage's gains [K + 1] (entry 0 of each is the context's own set, kept in step with d_coef / d_tab) and the table.
// Configuration like the input map: in no checkpoint, untouched by reset / set_state.  K == 0: no sets, nothing
// allocated, the calls pass what they always passed.
struct ParamSets {
  std::vector<t41rx_params> params;        // [K]
  std::vector<std::vector<float>> blobs;   // [K]
  std::vector<int32_t> set_of;             // [nchan]
  DevBuf<DevCoef> d_coef;
  DevBuf<float2> d_tab;
  DevBuf<SetGains> d_gain;
  DevBuf<int32_t> d_set_of;
  // loaded with T41RX_SETS_STAGES (t41rx_set_param_sets_ex): the sets run next to the chain-splitting stages.  Then, and
  // only then: every channel's effective nrOptionSelect / ANR_notchOn, its noise-reduction row and the lists made of
  // them (rx_stagesets.hpp) with their device copies -- the lists in nr_map_layout(), the rows [nchan] -- and what
  // cw_back_sets_kernel reads of every set [K + 1].  Made again when the sets, the noise-reduction map, the stage map or
  // set 0 change (stage_sets_refresh).
  uint32_t flags = 0;
  StageSetsNr stage;
  DevBuf<int32_t> d_nr_map;
  DevBuf<NrSetRow> d_nr_rows;
  DevBuf<CwSetBack> d_cw_back;
};

// the stage map (t41rx_set_stage_map; rx_stagemap.cpp): the caller's mask per channel, the lists made of it
// (rx_stagemap.hpp) and their device copy -- kStageCount + 1 rows of nchan entries, row s the list of stage s, the last
// row the blanker's complement.  Configuration like the output map: in no checkpoint, untouched by reset / set_state /
// set_params.  on == false: no map, every stage launches what it always launched.
struct StageMap {
  bool on = false;
  std::vector<uint32_t> map;  // [nchan] (host)
  StageLists lists;
  DevBuf<int32_t> d_lists;    // allocated with the first map
};
// what a stage's *_run passes to its launcher: null and 0 without a map
struct StageList {
  const int32_t *list = nullptr;
  int n = 0;
  bool mapped = false;
  bool empty() const { return mapped && n == 0; }  // nothing to launch: a grid of zero blocks is a launch error
};

// staging for t41rx_process_host
struct Staging {
  DevBuf<float> d_in_i, d_in_q, d_out;
  size_t in_floats = 0, out_floats = 0;  // floats d_in_i / d_in_q and d_out hold
};

}  // namespace t41

struct t41rx_ctx {
  int device = 0;
  int nchan = 0;
  t41rx_params params{};
  std::vector<float> blob;       // canonical coefficient blob (host)
  std::vector<int32_t> nco_hz;   // NCOFreq per channel (host)
  t41::DevBuf<float> d_state;    // [nchan][state_floats]
  t41::DevBuf<t41::DevCoef> d_coef;
  t41::DevBuf<float2> d_tab;
  t41::DevBuf<t41::ChanNco> d_nco;
  float *dbg_nco = nullptr, *dbg_dec = nullptr, *dbg_demod = nullptr;
  float *spect = nullptr, *spect_max = nullptr;  // audio-spectrum side output (t41rx_set_audio_spectrum)
  int tap_frames = 0, spect_frames = 0;          // frames per call those buffers are sized for
  // FFT_LENGTH 4096 pipeline: constant table + scratch between its three kernels
  t41::DevBuf<float2> d_tab4k;
  t41::DevBuf<float> d_mid, d_aud24;
  t41::DevBuf<char> d_agc_pipe;  // FFT_LENGTH 512, AGC on or SAM: the pipelined kernels' buffer (pipe_layout), allocated on first use
  int scratch_frames = 0;
  int layout = T41RX_LAYOUT_CHANNEL_MAJOR;  // of I / Q / audio (t41rx_set_buffer_layout)
  // the rate the process entries return the audio at (t41rx_set_audio_rate).  Configuration like `layout`: in no
  // checkpoint, untouched by reset / set_state / set_params.  24 kS/s: fft_length 512 only (the setter refuses)
  int audio_rate = T41RX_AUDIO_RATE_192K;
  // [nchan] 0, 1, ..: the map of a call that takes a mapped form without a map of the caller's (CallPlan::need_ident: the
  // set forms and the fused 24 kS/s forms are twins of the mapped ones), made by the first such call
  t41::DevBuf<int32_t> d_ident;
  int nco_sel = 0;               // long FFT: which NcoState copy is current (flips with every process call)
  // the environment as t41rx_create() found it.  T41RX_SEG_RUN=n, a test hook: the long-FFT pipeline's run length, and at
  // FFT_LENGTH 4096 the two-kernel pipeline in place of the one-kernel form.  T41RX_PIPE_STAT / T41RX_STAMP_TAPS: read on
  // a diagnostic library only (kernel_build_flags() != 0) -- the counters' print-out at destruction, and the demod tap
  // at the long FFT lengths, where the -DT41RX_STAMP kernels put their cycle stamps
  bool seg_run_set = false, pipe_stat = false, stamp_taps = false;
  long seg_run = 0;
  // receiver groups (t41rx_set_input_map): channel c reads row in_map[c] of the n_streams rows of I / Q; n_streams == 0:
  // no map, one row per channel.  Configuration like `layout`: in no checkpoint, untouched by reset / set_state / set_params
  std::vector<int32_t> in_map;   // (host)
  int n_streams = 0;
  t41::DevBuf<int32_t> d_in_map;  // [nchan], allocated with the first map
  // the output map (t41rx_set_output_map; rx_outmap.cpp): channel c stores its audio to row out_map[c] of the out_rows
  // rows of the audio buffer, or with -1 to none; out_map_on == false: no map, one row per channel.  Configuration like
  // the input map: in no checkpoint, untouched by reset / set_state / set_params
  std::vector<int32_t> out_map;   // (host)
  bool out_map_on = false;
  int out_rows = 0;               // may be 0 with the map on: nobody listens
  int out_listened = 0;           // channels with a row; fewer than out_rows: rows go unused and are not written
  t41::DevBuf<int32_t> d_out_map;  // [nchan], allocated with the first map
  t41::DevBuf<double> d_win;      // the display FFT's window (ensure_window): display spectrum, panadapter, calibration
  t41::ParamSets sets;
  t41::StageMap stages;
  t41::NrStage nr;
  t41::NbStage nb;
  t41::EqStage eq;
  t41::CwStage cw;
  t41::Ft8Stage ft8;
  t41::Ft8Decode ft8d;
  t41::DisplayTap disp;
  t41::Panadapter pan;
  t41::BeaconStage beacon;
  t41::Calibration cal;
  t41::Staging staging;
};

namespace t41 {

inline int hip_fail(hipError_t e, const char *what) {
  return fail(T41RX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
inline int hip_check(hipError_t e, const char *what) { return e == hipSuccess ? T41RX_OK : hip_fail(e, what); }
#define HIP_TRY(expr)                                        \
  do {                                                       \
    hipError_t e__ = (expr);                                 \
    if (e__ != hipSuccess) return t41::hip_fail(e__, #expr); \
  } while (0)

// ---- which stages a process call runs.  These are the switches; which kernels a call runs with them -- the tap kernels,
// the hand-over, the scratch, the pipelined forms, the back end -- is decided once per call by plan_call() (rx_plan.hpp),
// from the CallFacts the process call fills with these predicates (rx_host.cpp: call_facts)
// (a noise-reduction map, t41rx_set_nr_map: on when some entry of the map is non-zero; the context's two values are not consulted)
// (parameter sets loaded with T41RX_SETS_STAGES: on when some channel's effective kind or notch is non-zero)
inline bool nr_on(const t41rx_ctx *ctx) {
  if (!ctx->sets.params.empty() && (ctx->sets.flags & T41RX_SETS_STAGES)) return ctx->sets.stage.lists.any;
  return ctx->nr.map_on ? ctx->nr.lists.any : ctx->params.nrOptionSelect != 0 || ctx->params.ANR_notchOn != 0;  // (fft_length 512: params_valid)
}
// the CW block runs in T41State == CW_RECEIVE (Process.cpp:878), which in receive is xmtMode == CW_MODE
// (T41_SDR.ino:1039-1040, 1144-1148); with another xmtMode the switches are kept and nothing runs
// (a filter map, t41rx_set_cw_filter_map: the narrow filter runs when some channel has an index; the context's is not consulted)
inline bool cw_filter_on(const t41rx_ctx *ctx) {
  return ctx->params.xmtMode == T41RX_CW_MODE && (ctx->cw.map_on ? !ctx->cw.lists.filtered.empty() : ctx->cw.filter != kCwFilters);
}
inline bool cw_det_on(const t41rx_ctx *ctx) { return ctx->params.xmtMode == T41RX_CW_MODE && ctx->cw.det != 0; }
// the decoder runs exactly when the detector runs (in the firmware one decoderFlag gates both, CWProcessing.cpp:322-372)
inline bool cw_dec_on(const t41rx_ctx *ctx) { return cw_det_on(ctx) && ctx->cw.dec != 0; }
// parameter sets: loaded, and what a chain-splitting stage's switch answers then (those stages read set 0's parameters
// on the host; rx_sets.cpp refuses in the other order with split_stage_on())
inline bool sets_loaded(const t41rx_ctx *ctx) { return !ctx->sets.params.empty(); }
// ... loaded with T41RX_SETS_STAGES: the stages run next to them, each channel with its own set's values; and loaded
// without: the stages' setters refuse (sets_refuse_stage)
inline bool sets_staged(const t41rx_ctx *ctx) { return sets_loaded(ctx) && (ctx->sets.flags & T41RX_SETS_STAGES) != 0; }
inline bool sets_plain(const t41rx_ctx *ctx) { return sets_loaded(ctx) && !sets_staged(ctx); }
constexpr const char *kNrMapStageName = "the noise reduction / notch of a noise-reduction map";
inline int sets_refuse_stage(const char *stage) {
  return fail(T41RX_ERR_UNSUPPORTED, std::string(stage) + " splits the fused chain and reads one parameter set on the host: it cannot run "
                                         "while parameter sets are loaded (t41rx_set_param_sets); remove the sets first");
}
// the chain-splitting stage whose switch is on, or null (the context-wide noise reduction / notch are parameters: the
// sets' rule has them; a noise-reduction map with a non-zero entry is a switch of the context like the others)
inline const char *split_stage_on(const t41rx_ctx *ctx) {
  return ctx->eq.on ? "the receive equalizer" : ctx->nb.on ? "the noise blanker"
         : (ctx->nr.map_on && ctx->nr.lists.any) ? kNrMapStageName
         : (ctx->cw.filter != kCwFilters || (ctx->cw.map_on && !ctx->cw.lists.filtered.empty())) ? "the CW audio filter"
         : ctx->cw.det ? "the CW detector" : ctx->cw.dec ? "the CW decoder" : nullptr;
}
// rows of I / Q a process call reads: one per channel, or the input map's n_streams
// samples per channel and frame the process entries write: the input frame, or its 256 samples @24 kS/s
inline bool audio_24k(const t41rx_ctx *ctx) { return ctx->audio_rate == T41RX_AUDIO_RATE_24K; }
inline int audio_frame_len(const t41rx_ctx *ctx) { return audio_24k(ctx) ? 256 : 4 * ctx->params.fft_length; }
// rx_host.cpp: volume, conversion and stores of a 24 kS/s call from the scratch (launch_chain, cw_filter_run)
int aud24_finish_run(t41rx_ctx *ctx, const RxArgs &a, int n_frames, hipStream_t s);
inline int input_rows(const t41rx_ctx *ctx) { return ctx->n_streams > 0 ? ctx->n_streams : ctx->nchan; }
// rows of audio a process call writes: one per channel, or the output map's n_rows
inline int audio_rows(const t41rx_ctx *ctx) { return ctx->out_map_on ? ctx->out_rows : ctx->nchan; }
// rows of d_power / d_status (and of the audio entry's pcm): one per channel, or the FT8 map's n_rows
inline int ft8_rows(const t41rx_ctx *ctx) { return ctx->ft8.map_on ? ctx->ft8.rows : ctx->nchan; }
// rows of the panadapter's taps and of the caller's seven row buffers: one per channel, or the panadapter map's n_rows
inline int pan_rows(const t41rx_ctx *ctx) { return ctx->pan.map_on ? ctx->pan.rows : ctx->nchan; }
// the call being prepared writes display taps and runs the panadapter kernel: the stage is on, the call has an update
// frame (pan_prepare) and, with a map, somebody is listed
inline bool pan_call_rows(const t41rx_ctx *ctx) {
  return ctx->pan.on && ctx->pan.call_rows > 0 && !(ctx->pan.map_on && ctx->pan.list.empty());
}
// the list of a stage of a call (rx_stagemap.hpp: StageIndex), row kStageCount: the blanker's complement
inline StageList stage_list(const t41rx_ctx *ctx, int row) {
  if (!ctx->stages.on) return StageList{};
  const std::vector<int32_t> &l = row < kStageCount ? ctx->stages.lists.list[row] : ctx->stages.lists.nb_rest;
  return StageList{ctx->stages.d_lists.get() + (size_t)row * (size_t)ctx->nchan, (int)l.size(), true};
}
// the output map leaves rows unused: the host-pointer forms then carry the caller's rows through the staging buffer, so
// that a row no channel names comes back as it went in
inline bool audio_rows_unused(const t41rx_ctx *ctx) { return ctx->out_map_on && ctx->out_listened < ctx->out_rows; }
// where (row, frame) of a call's I / Q or audio starts, in samples: rows of frames of `len` samples in the context's layout
struct Strides {
  long long chan, frame;
};
inline Strides strides_of(const t41rx_ctx *ctx, int rows, int frames, int len) {
  if (ctx->layout == T41RX_LAYOUT_TIME_MAJOR) return Strides{len, (long long)rows * len};  // [frame][row][len]
  return Strides{(long long)frames * len, len};
}

// ---- helpers more than one file uses
// a stage memory whose power-on value is zero, on first use (rx_audio.cpp)
int ensure_zeroed(DevBuf<float> &b, size_t bytes, const char *what);
// the optional channel mask of a per-channel command (nullptr: every channel) on the device (rx_cw.cpp)
int upload_channel_mask(const t41rx_ctx *ctx, const uint8_t *channels, DevBuf<uint8_t> &mask);
// a stage clock's setter: `what` opens the refusal (rx_cw.cpp)
int set_stage_clock(StageClock &clock, const char *what, int32_t t0_ms, int32_t num, int32_t den);
// the zoom filters of a display-FFT launch (spectrumZoom 1..4: IIR_biquad_Zoom_FFT's coefficients and the decimating FIR;
// zoom 0 leaves them alone) and the display FFT's window, once per context (rx_display.cpp)
void zoom_filter_args(int zoom, float (&iir)[20], float (&fir)[4]);
int ensure_window(t41rx_ctx *ctx);
// displayScale[] (Display.cpp:127-135): dBScale, baseOffset -- the calibration's and the panadapter's pixel mapping
constexpr float kDbScale[5] = {10.0f, 20.0f, 40.0f, 100.0f, 200.0f};
constexpr int kBaseOffset[5] = {24, 10, 58, 120, 200};
// blob -> the device's coefficient block, constant table (FFT_LENGTH 512 form) and first-stage gains with their `plain`
// classification (rx_host.cpp: what upload_coeffs() and rx_args() make of set 0, rx_sets.cpp of every set)
void fill_dev_coef(const BlobView &v, DevCoef &dc);
void fill_tab512(const BlobView &v, int fft_length, std::vector<float2> &tab);
bool gains_of(const float *scalars, SetGains &g);  // returns plain
CallFacts params_facts(const t41rx_params &p, bool plain_gains);  // what plan_call() reads of a parameter struct
int upload_nco(t41rx_ctx *ctx);
// rx_sets.cpp: set 0 changed (set_params / set_coeffs) -- the rule against the loaded sets, and entry 0 of the set arrays
int sets_check_set0(const t41rx_ctx *ctx, const t41rx_params &p);
int sets_upload(t41rx_ctx *ctx);
// rx_sets.cpp, sets loaded with T41RX_SETS_STAGES: the channels' effective values, rows and lists of these sets, table
// and noise-reduction map (null, null: none) with the context's stage map -- the refusal's text names the channel and the
// set --; the context's own made again and uploaded (nothing without such sets); a call's noise-reduction launches
int stage_sets_build(const t41rx_ctx *ctx, const t41rx_params &set0, const t41rx_params *extra, int n_extra, const int32_t *set_of,
                     const int32_t *kind_map, const int32_t *notch_map, StageSetsNr &out);
int stage_sets_refresh(t41rx_ctx *ctx);
int nr_sets_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
// the pipelined kernels' time-out counter (rx_host.cpp)
int pipe_timeouts_clear(t41rx_ctx *ctx);
int pipe_status(const t41rx_ctx *ctx);
// the path's records and every stage memory to power-on (rx_state.cpp)
int reset_state(t41rx_ctx *ctx);

// ---- what the stages give the process call (`*_run`: fill the stage's argument block and launch, on the call's audio @24
// kS/s in d_aud24) and the checkpoint table (`ensure_*` also allocates on restore; get / put / reset where a section is
// more than one buffer)
// rx_audio.cpp
int ensure_nr(t41rx_ctx *ctx);
int ensure_nb(t41rx_ctx *ctx);
int ensure_eq(t41rx_ctx *ctx);
int eq_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int nr_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int nb_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int nr_check(const t41rx_ctx *ctx, const int32_t *hdr, const float *sec);
int nr_get(const t41rx_ctx *ctx, void *host, size_t bytes);
int nr_put(t41rx_ctx *ctx, const void *host, size_t bytes);
int nr_reset(t41rx_ctx *ctx, size_t bytes);
int nb_get(const t41rx_ctx *ctx, void *host, size_t bytes);
int nb_put(t41rx_ctx *ctx, const void *host, size_t bytes);
int nb_reset(t41rx_ctx *ctx, size_t bytes);
// rx_cw.cpp
int ensure_cw(t41rx_ctx *ctx);
int ensure_cw_decode(t41rx_ctx *ctx);
const char *cw_split_stage(const t41rx_ctx *ctx, int *channel, int *set);  // (*channel: with a noise-reduction map or staged sets the first channel that trips it, else -1; *set: its set where the set supplied the values, else -1)
int cw_detect_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int cw_decode_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int cw_filter_run(t41rx_ctx *ctx, const CallPlan &plan, const RxArgs &a, int n_frames, hipStream_t s);  // the narrow filter and its back end
int check_cw_decode(const t41rx_ctx *ctx, const int32_t *hdr, const float *sec);
int cw_decode_reset(t41rx_ctx *ctx, size_t bytes);
// rx_stageparams.cpp: the filter map's row maps again, behind a change of the output map (no map loaded: nothing)
int cw_filter_map_refresh(t41rx_ctx *ctx);
// rx_nrmap.cpp: the noise-reduction map's launches of a call (nr_run() with a map loaded); its lists again, behind a change
// of the stage map (no map loaded: nothing); and the new parameters of t41rx_set_params / _set_coeffs against a loaded map
int nr_map_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int nr_map_refresh(t41rx_ctx *ctx);
int nr_map_check_params(const t41rx_ctx *ctx, const t41rx_params &p);
// rx_ft8.cpp
int ft8_prepare(t41rx_ctx *ctx, const CallPlan &plan, int n_frames, hipStream_t s);  // the call's refusals, the memory and the demod tap of its own
int ft8_run(t41rx_ctx *ctx, const CallPlan &plan, const RxArgs &a, int n_frames, hipStream_t s);
int ft8_power_on(t41rx_ctx *ctx);
// rx_ft8_decode.cpp
void ft8_decode_release(t41rx_ctx *ctx);  // t41rx_destroy(): the pinned copy and the event
// rx_display.cpp
int display_check(const t41rx_ctx *ctx, const int32_t *hdr, const float *sec);
int display_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int pan_prepare(t41rx_ctx *ctx, int n_frames);  // which frames of the call are update frames, and the stage's refusals
int pan_run(t41rx_ctx *ctx, int n_frames, hipStream_t s);
int pan_reset(t41rx_ctx *ctx);
int pan_map_refresh(t41rx_ctx *ctx);  // the parameter sets or set 0 changed (behind the setter's synchronisation): the map's list again (no map: nothing)
// rx_beacon.cpp
int beacon_prepare(t41rx_ctx *ctx);  // the call's refusals, once pan_prepare() has counted its rows
int beacon_run(t41rx_ctx *ctx, hipStream_t s);  // behind pan_run(), on the rows it wrote
int beacon_reset(t41rx_ctx *ctx);  // behind pan_reset(): switch-on again at frame 0
// rx_cal.cpp
int cal_reset(t41rx_ctx *ctx);

}  // namespace t41
