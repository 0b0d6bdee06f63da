// t41_sdr_amd/csrc/rx_stageparams.hpp -- the CW filter map's lists (t41rx_set_cw_filter_map; rx_stageparams.cpp): from
// the caller's CWFilterIndex per channel and the output map's row per channel, the ascending list of the channels the
// narrow filter runs on and the row map of each of the two back kernels.  Plain C++: no HIP, no context type, so that a
// CPU program can walk it (tests/stage_params_check.cpp), as tests/stage_map_check.cpp walks rx_stagemap.hpp.
//
// The rule the lists serve: channel c is processed as the same channel of a context whose CWFilterIndex is
// filter_of_channel[c].  A filtered channel (0 .. 4) ends in the oracle's interpolators (cw_back_kernel), an unfiltered
// one (5) in the fused back kernel (launch_back512); the two differ in the last bit, so a call with both classes launches
// both, each in its output-map form with the rows of the other class muted: rows_filtered[c] is the channel's row for a
// filtered channel and -1 for the others, rows_plain[c] the other way round.  The channel's row is the caller's
// row_of_channel[c], or c without an output map.  The output-map forms leave a muted channel's interpolator memories as
// they were, so every channel's memories advance exactly once.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace t41 {

constexpr int32_t kCwFilterOff = 5;  // CWFilterIndex 5: no narrow filter (cw_kernels.hpp: kCwFilters)

struct CwFilterLists {
  std::vector<int32_t> filtered;       // the channels with an index 0 .. 4, ascending
  std::vector<int32_t> rows_filtered;  // [n_channels]: the row of a filtered channel, -1 for the others
  std::vector<int32_t> rows_plain;     // [n_channels]: the row of an unfiltered channel, -1 for the others
};

// why a map is refused
enum class CwFilterMapFault : int {
  none = 0,
  count,     // n != n_channels (or no channels at all)
  null_map,  // no array
  range,     // an entry outside [0, 5]; `channel` names it
  tables,    // an entry < 5 and no filter tables loaded; `channel` names the first such entry
};
struct CwFilterMapVerdict {
  CwFilterMapFault fault = CwFilterMapFault::none;
  int channel = -1;
  explicit operator bool() const { return fault == CwFilterMapFault::none; }
};

// Checks the map (every entry, before anything is built) and fills `out`; a refused map leaves `out` as it was.
// row_of_channel: the output map's [n_channels] (validated by its own setter), or null without one.
inline CwFilterMapVerdict build_cw_filter_lists(const int32_t *filter_of_channel, int n, int n_channels, bool tables_loaded,
                                                const int32_t *row_of_channel, CwFilterLists &out) {
  if (n_channels <= 0 || n != n_channels) return {CwFilterMapFault::count, -1};
  if (!filter_of_channel) return {CwFilterMapFault::null_map, -1};
  for (int c = 0; c < n; ++c)
    if (filter_of_channel[c] < 0 || filter_of_channel[c] > kCwFilterOff) return {CwFilterMapFault::range, c};
  if (!tables_loaded)
    for (int c = 0; c < n; ++c)
      if (filter_of_channel[c] != kCwFilterOff) return {CwFilterMapFault::tables, c};
  CwFilterLists fresh;
  fresh.rows_filtered.assign((size_t)n, -1);
  fresh.rows_plain.assign((size_t)n, -1);
  for (int c = 0; c < n; ++c) {
    const int32_t row = row_of_channel ? row_of_channel[c] : c;
    if (filter_of_channel[c] != kCwFilterOff) {
      fresh.filtered.push_back(c);
      fresh.rows_filtered[(size_t)c] = row;
    } else {
      fresh.rows_plain[(size_t)c] = row;
    }
  }
  out = std::move(fresh);
  return {};
}

}  // namespace t41
