// t41_sdr_amd/csrc/rx_stagesets.hpp -- parameter sets loaded with T41RX_SETS_STAGES (t41rx_set_param_sets_ex; rx_sets.cpp):
// what the noise reduction of a call reads per channel.  From the sets' noise-reduction values (set 0 is the context's
// own), the channels' table, the optional noise-reduction map and the optional stage map: the EFFECTIVE nrOptionSelect and
// ANR_notchOn of every channel, the row {NR_alpha, NR_beta, NR_PSI, VAD range} nrspec_sets_kernel reads for it, and the
// lists of rx_nrmap.hpp made of the effective values.  Plain C++: no HIP, no context type, so that a CPU program can walk
// it (tests/stage_sets_check.cpp), as tests/nr_map_check.cpp walks rx_nrmap.hpp.
//
// The rule: channel c is processed as the same channel of a context created with sets[set_of_channel[c]].
//  * kind and notch: the map's entries where a map is loaded (it overrides the parameters, as it overrides the context's
//    without sets), else those of the channel's own set.
//  * NR_alpha, NR_beta, NR_PSI and the VAD range: always those of the channel's own set.
//  * the spectral function's array-bounds check (params_valid() with nrOptionSelect 2) is the channel's: a channel whose
//    effective kind is 2 needs a set whose pass band passes it, whatever the stage map says (the stage map may change
//    between two calls without a check).  A set no channel names, or whose channels all run another kind, is not asked.
// It is made again whenever the sets, the map, the stage map or set 0 change.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "rx_nrmap.hpp"

namespace t41 {

// what the noise reduction reads of one parameter set (the host fills it from t41rx_params: nr_vad_range(), params_valid())
struct StageSetNr {
  int32_t kind = 0, notch = 0;  // nrOptionSelect, ANR_notchOn
  float alpha = 0.0f, beta = 0.0f, psi = 0.0f;
  int32_t vad_lo = 0, vad_hi = 0;
  bool spectral_ok = false;     // the pass band passes the spectral function's array-bounds check
};

// a channel's row of the device table: one 32-byte scalar load of the channel's workgroup
struct NrSetRow {
  float alpha, beta, psi;
  int32_t vad_lo, vad_hi;
  int32_t pad[3];
};
static_assert(sizeof(NrSetRow) == 32, "a row is eight dwords");

struct StageSetsNr {
  std::vector<int32_t> kind, notch;  // [n_channels] effective
  std::vector<NrSetRow> rows;        // [n_channels]
  NrMapLists lists;                  // of the effective values and the stage map
};

enum class StageSetsFault : int {
  none = 0,
  count,     // n != n_channels, no channels, no sets, or a missing array
  set,       // set_of_channel[channel] outside [0, n_sets)
  kind,      // an entry of the map, or a set's nrOptionSelect, outside 0 .. 3 (channel; set where it is the set's)
  notch,     // ... ANR_notchOn outside 0 .. 1
  spectral,  // channel `channel` runs kind 2 on set `set`, whose pass band fails the check
};
struct StageSetsVerdict {
  StageSetsFault fault = StageSetsFault::none;
  int channel = -1, set = -1;
  explicit operator bool() const { return fault == StageSetsFault::none; }
};

// the detector's one-audio-stream rule reads these: a channel's effective two values
constexpr int32_t stage_sets_kind(const StageSetNr *sets, const int32_t *set_of, const int32_t *kind_map, int c) {
  return kind_map ? kind_map[c] : sets[set_of[c]].kind;
}
constexpr int32_t stage_sets_notch(const StageSetNr *sets, const int32_t *set_of, const int32_t *notch_map, int c) {
  return notch_map ? notch_map[c] : sets[set_of[c]].notch;
}

// Checks everything (before anything is built) and fills `out`; a refusal leaves `out` as it was.
// sets: [n_sets] with set 0 first; kind_map / notch_map: the noise-reduction map's two arrays, both or neither;
// stages_of_channel: the stage map's masks, or null.
inline StageSetsVerdict build_stage_sets(const StageSetNr *sets, int n_sets, const int32_t *set_of_channel, int n, int n_channels,
                                         const int32_t *kind_map, const int32_t *notch_map, const uint32_t *stages_of_channel,
                                         StageSetsNr &out) {
  if (n_channels <= 0 || n != n_channels || n_sets <= 0 || !sets || !set_of_channel || (kind_map == nullptr) != (notch_map == nullptr))
    return {StageSetsFault::count, -1, -1};
  for (int c = 0; c < n; ++c)
    if (set_of_channel[c] < 0 || set_of_channel[c] >= n_sets) return {StageSetsFault::set, c, -1};
  StageSetsNr fresh;
  fresh.kind.resize((size_t)n);
  fresh.notch.resize((size_t)n);
  fresh.rows.resize((size_t)n);
  for (int c = 0; c < n; ++c) {
    const int32_t k = set_of_channel[c];
    const StageSetNr &s = sets[k];
    const int32_t kind = stage_sets_kind(sets, set_of_channel, kind_map, c), notch = stage_sets_notch(sets, set_of_channel, notch_map, c);
    if (kind < 0 || kind > 3) return {StageSetsFault::kind, c, kind_map ? -1 : k};
    if (notch < 0 || notch > 1) return {StageSetsFault::notch, c, notch_map ? -1 : k};
    if (kind == 2 && !s.spectral_ok) return {StageSetsFault::spectral, c, k};
    fresh.kind[(size_t)c] = kind;
    fresh.notch[(size_t)c] = notch;
    fresh.rows[(size_t)c] = NrSetRow{s.alpha, s.beta, s.psi, s.vad_lo, s.vad_hi, {0, 0, 0}};
  }
  if (!build_nr_map_lists(fresh.kind.data(), fresh.notch.data(), n, n_channels, stages_of_channel, fresh.lists))
    return {StageSetsFault::count, -1, -1};  // (not reached: every entry was checked above)
  out = std::move(fresh);
  return {};
}

}  // namespace t41
