// t41_sdr_amd/csrc/rx_ft8map.hpp -- the FT8 map's list (t41rx_set_ft8_map; rx_ft8.cpp): from the caller's row per channel,
// the ascending list of {channel, row} pairs the list forms of the FT8 kernels run on (ft8_kernel.hip: one workgroup per
// pair).  Plain C++: no HIP, no context type, so that a CPU program can walk it (tests/ft8_map_check.cpp), as
// tests/stage_map_check.cpp walks build_stage_lists().
//
// The rule the list serves: FT8 receive runs on channel c exactly when the context's switch (t41rx_set_ft8) is on and
// row_of_channel[c] >= 0, and then writes row row_of_channel[c] of d_power / d_status.  The list knows nothing of the
// switch but the one thing the setter's last refusal needs: the rows the buffers given to t41rx_set_ft8 were sized for.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace t41 {

// one entry of the list as the kernels read it: two int32, {channel, row}
struct Ft8Pair {
  int32_t channel, row;
};

// why a map is refused
enum class Ft8MapFault : int {
  none = 0,
  count,     // n != n_channels (or no channels at all)
  null_map,  // no array
  rows,      // n_rows outside 1 .. n_channels
  entry,     // an entry outside [-1, n_rows); `channel` names it
  twice,     // a row named twice; `channel` names the second channel, `other` the first
  resize,    // FT8 receive is on and n_rows differs from the rows its buffers were sized for
};
struct Ft8MapVerdict {
  Ft8MapFault fault = Ft8MapFault::none;
  int channel = -1, other = -1;
  explicit operator bool() const { return fault == Ft8MapFault::none; }
};

// Checks the map (every entry, before anything is built) and fills `out`, ascending by channel; a refused map leaves
// `out` as it was.  rows_in_use: the rows d_power / d_status hold while FT8 receive is on (t41rx_ft8_rows()), 0 while
// it is off.  A map that lists nobody is a map: the list is empty.
inline Ft8MapVerdict build_ft8_list(const int32_t *row_of_channel, int n, int n_rows, int n_channels, int rows_in_use,
                                    std::vector<Ft8Pair> &out) {
  if (n_channels <= 0 || n != n_channels) return {Ft8MapFault::count, -1, -1};
  if (!row_of_channel) return {Ft8MapFault::null_map, -1, -1};
  if (n_rows < 1 || n_rows > n_channels) return {Ft8MapFault::rows, -1, -1};
  std::vector<int32_t> owner((size_t)n_rows, -1);
  for (int c = 0; c < n; ++c) {
    const int32_t r = row_of_channel[c];
    if (r < -1 || r >= n_rows) return {Ft8MapFault::entry, c, -1};
    if (r < 0) continue;
    if (owner[(size_t)r] >= 0) return {Ft8MapFault::twice, c, owner[(size_t)r]};
    owner[(size_t)r] = c;
  }
  if (rows_in_use > 0 && n_rows != rows_in_use) return {Ft8MapFault::resize, -1, -1};
  std::vector<Ft8Pair> fresh;
  for (int c = 0; c < n; ++c)
    if (row_of_channel[c] >= 0) fresh.push_back(Ft8Pair{c, row_of_channel[c]});
  out = std::move(fresh);
  return {};
}

}  // namespace t41
