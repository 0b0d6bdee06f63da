// t41_sdr_amd/csrc/rx_panmap.hpp -- the panadapter map's list (t41rx_set_panadapter_map; rx_display.cpp): from the caller's
// row per channel, the ascending list of {channel, row, RFgain, rfGainAllBands} entries the list forms of the panadapter
// and beacon kernels run on (panadapter_kernel.hip: one wave per entry; beacon_kernel.hip: one lane per entry).  Plain
// C++: no HIP, no context type, so that a CPU program can walk it (tests/pan_map_check.cpp), as tests/ft8_map_check.cpp
// walks build_ft8_list().
//
// The rule the list serves: the panadapter stage runs on channel c exactly when the context's switch
// (t41rx_set_panadapter) is on and row_of_channel[c] >= 0, and then writes row row_of_channel[c] of the seven row buffers
// and of the two taps.  The two gains of DrawSmeterBar()'s dBm ride in the entry: each listed channel's own effective
// parameter set's, so that the sets of a context may differ in them.  The list knows nothing of the switch but the one
// thing the setter's last refusal needs: the rows the buffers given to t41rx_set_panadapter were sized for.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace t41 {

// one entry of the list as the kernels read it: four int32, one 16-byte scalar load
struct PanEntry {
  int32_t channel, row, RFgain, rfGainAllBands;
};
static_assert(sizeof(PanEntry) == 16, "PanEntry: one 16-byte scalar load");

// DrawSmeterBar()'s two integers of one parameter set (t41rx_params::RFgain, ::rfGainAllBands)
struct PanGains {
  int32_t RFgain, rfGainAllBands;
};

// why a map is refused
enum class PanMapFault : int {
  none = 0,
  count,     // n != n_channels (or no channels at all)
  null_map,  // no array
  rows,      // n_rows outside 1 .. n_channels
  entry,     // an entry outside [-1, n_rows); `channel` names it
  twice,     // a row named twice; `channel` names the second channel, `other` the first
  resize,    // the panadapter is on and n_rows differs from the rows its buffers were sized for
};
struct PanMapVerdict {
  PanMapFault fault = PanMapFault::none;
  int channel = -1, other = -1;
  explicit operator bool() const { return fault == PanMapFault::none; }
};

// Checks the map, every entry, before anything is built.  rows_in_use: the rows the row buffers hold while the
// panadapter is on (t41rx_panadapter_rows()), 0 while it is off.  A map that lists nobody is a map.
inline PanMapVerdict check_pan_map(const int32_t *row_of_channel, int n, int n_rows, int n_channels, int rows_in_use) {
  if (n_channels <= 0 || n != n_channels) return {PanMapFault::count, -1, -1};
  if (!row_of_channel) return {PanMapFault::null_map, -1, -1};
  if (n_rows < 1 || n_rows > n_channels) return {PanMapFault::rows, -1, -1};
  std::vector<int32_t> owner((size_t)n_rows, -1);
  for (int c = 0; c < n; ++c) {
    const int32_t r = row_of_channel[c];
    if (r < -1 || r >= n_rows) return {PanMapFault::entry, c, -1};
    if (r < 0) continue;
    if (owner[(size_t)r] >= 0) return {PanMapFault::twice, c, owner[(size_t)r]};
    owner[(size_t)r] = c;
  }
  if (rows_in_use > 0 && n_rows != rows_in_use) return {PanMapFault::resize, -1, -1};
  return {};
}

// The list of a checked map, ascending by channel.  gains: [K + 1], entry 0 the context's own set; set_of: the channels'
// table [n] with entries 0 .. K (the parameter sets' setter has checked them), or null: every channel runs set 0.  Plain
// sets and sets loaded next to the stages give a channel the same two gains: its own set's.  Made again whenever the
// map, the sets or set 0 change.
inline std::vector<PanEntry> pan_list_of(const int32_t *row_of_channel, int n, const PanGains *gains, const int32_t *set_of) {
  std::vector<PanEntry> list;
  for (int c = 0; c < n; ++c) {
    if (row_of_channel[c] < 0) continue;
    const PanGains &g = gains[set_of ? set_of[c] : 0];
    list.push_back(PanEntry{c, row_of_channel[c], g.RFgain, g.rfGainAllBands});
  }
  return list;
}

// check_pan_map() and pan_list_of() in one: a refused map leaves `out` as it was
inline PanMapVerdict build_pan_list(const int32_t *row_of_channel, int n, int n_rows, int n_channels, int rows_in_use, const PanGains *gains,
                                    const int32_t *set_of, std::vector<PanEntry> &out) {
  const PanMapVerdict v = check_pan_map(row_of_channel, n, n_rows, n_channels, rows_in_use);
  if (!v) return v;
  out = pan_list_of(row_of_channel, n, gains, set_of);
  return {};
}

}  // namespace t41
