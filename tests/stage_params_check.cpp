// tests/stage_params_check.cpp -- walks build_cw_filter_lists() (t41_sdr_amd/csrc/rx_stageparams.hpp), the pure function
// that turns the CW filter map (t41rx_set_cw_filter_map) and the output map into the ascending list of filtered channels
// and the row map of each of the two back kernels.  A program of its own for tests/test_stage_params_lists.py: no GPU,
// no HIP.  Exit status 0 and a count of the maps walked, or 1 with the first violation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rx_stageparams.hpp"

using namespace t41;

namespace {

long g_walked = 0;

bool violated(const char *what, const std::vector<int32_t> &map) {
  std::printf("stage params lists: violated: %s\n  map (%zu channels):", what, map.size());
  for (size_t c = 0; c < map.size() && c < 80; ++c) std::printf(" %d", map[c]);
  std::printf("\n");
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond, map)

// (the tests' own generator: the same maps in every run)
uint32_t g_rng = 12345u;
uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

// an accepted map with this output map (null: none)
bool check_lists(const std::vector<int32_t> &map, const std::vector<int32_t> *omap) {
  ++g_walked;
  const int n = (int)map.size();
  CwFilterLists l;
  const CwFilterMapVerdict v = build_cw_filter_lists(map.data(), n, n, true, omap ? omap->data() : nullptr, l);
  REQUIRE(bool(v) && v.fault == CwFilterMapFault::none && v.channel == -1);
  // the filtered list is exactly the channels with an index, ascending
  size_t k = 0;
  for (int c = 0; c < n; ++c)
    if (map[(size_t)c] != kCwFilterOff) {
      REQUIRE(k < l.filtered.size() && l.filtered[k] == c);
      ++k;
    }
  REQUIRE(k == l.filtered.size());
  for (size_t i = 1; i < l.filtered.size(); ++i) REQUIRE(l.filtered[i - 1] < l.filtered[i]);
  // the two row maps are disjoint and together the caller's map (the identity without one); each holds its own class
  REQUIRE(l.rows_filtered.size() == (size_t)n && l.rows_plain.size() == (size_t)n);
  for (int c = 0; c < n; ++c) {
    const int32_t row = omap ? (*omap)[(size_t)c] : c, f = l.rows_filtered[(size_t)c], p = l.rows_plain[(size_t)c];
    const bool filtered = map[(size_t)c] != kCwFilterOff;
    REQUIRE(f == -1 || p == -1);
    REQUIRE((filtered ? f : p) == row);
    REQUIRE((filtered ? p : f) == -1);
    REQUIRE(f >= -1 && p >= -1);
  }
  return true;
}

// a refused map: the fault, the channel it names, and `out` as it was
bool check_refusal(const std::vector<int32_t> &map, const int32_t *data, int n, int n_channels, bool tables, CwFilterMapFault fault, int channel) {
  ++g_walked;
  CwFilterLists l;
  l.filtered = {41, 42};
  l.rows_filtered = {7};
  l.rows_plain = {8, 9, 10};
  const CwFilterMapVerdict v = build_cw_filter_lists(data, n, n_channels, tables, nullptr, l);
  REQUIRE(!v && v.fault == fault && v.channel == channel);
  REQUIRE(l.filtered.size() == 2 && l.filtered[0] == 41 && l.filtered[1] == 42);
  REQUIRE(l.rows_filtered.size() == 1 && l.rows_filtered[0] == 7);
  REQUIRE(l.rows_plain.size() == 3 && l.rows_plain[0] == 8 && l.rows_plain[2] == 10);
  return true;
}

// the four output maps of a size: none, the identity, all muted, a random one (a permutation with some channels muted)
bool check_with_output_maps(const std::vector<int32_t> &map) {
  const int n = (int)map.size();
  std::vector<int32_t> ident((size_t)n), muted((size_t)n, -1), random((size_t)n);
  for (int c = 0; c < n; ++c) ident[(size_t)c] = random[(size_t)c] = c;
  for (int c = n - 1; c > 0; --c) std::swap(random[(size_t)c], random[(size_t)(rnd() % (uint32_t)(c + 1))]);
  for (int c = 0; c < n; ++c)
    if (rnd() % 3 == 0) random[(size_t)c] = -1;
  return check_lists(map, nullptr) && check_lists(map, &ident) && check_lists(map, &muted) && check_lists(map, &random);
}

}  // namespace

int main() {
  // every map over {0..5}^n, n <= 4
  for (int n = 1; n <= 4; ++n) {
    int total = 1;
    for (int i = 0; i < n; ++i) total *= 6;
    for (int code = 0; code < total; ++code) {
      std::vector<int32_t> map((size_t)n);
      int r = code;
      for (int c = 0; c < n; ++c) {
        map[(size_t)c] = r % 6;
        r /= 6;
      }
      if (!check_with_output_maps(map)) return 1;
    }
  }
  // the sizes either side of the filter kernel's eight-channel wave and of a 64-channel block, random maps; with them
  // nobody filtered and everybody filtered
  const int sizes[8] = {1, 7, 8, 9, 16, 17, 64, 65};
  for (int n : sizes)
    for (int kind = 0; kind < 5; ++kind) {
      std::vector<int32_t> map((size_t)n);
      for (int c = 0; c < n; ++c) map[(size_t)c] = kind == 3 ? kCwFilterOff : kind == 4 ? c % 5 : (int32_t)(rnd() % 6);
      if (!check_with_output_maps(map)) return 1;
    }
  // the refusals, each at the first, a middle and the last channel
  for (int n : sizes) {
    const std::vector<int32_t> good((size_t)n, 2);
    for (int wrong : {0, n - 1, n + 1, -1})
      if (wrong != n && !check_refusal(good, good.data(), wrong, n, true, CwFilterMapFault::count, -1)) return 1;
    if (!check_refusal(good, good.data(), 0, 0, true, CwFilterMapFault::count, -1)) return 1;
    if (!check_refusal(good, nullptr, n, n, true, CwFilterMapFault::null_map, -1)) return 1;
    for (int at : {0, n / 2, n - 1})
      for (int32_t bad : {-1, 6, 1 << 30, INT32_MIN}) {
        std::vector<int32_t> map((size_t)n, kCwFilterOff);
        map[(size_t)at] = bad;
        if (!check_refusal(map, map.data(), n, n, true, CwFilterMapFault::range, at)) return 1;
        // (an entry out of range is named ahead of the missing tables)
        if (!check_refusal(map, map.data(), n, n, false, CwFilterMapFault::range, at)) return 1;
      }
    for (int at : {0, n / 2, n - 1}) {
      std::vector<int32_t> map((size_t)n, kCwFilterOff);
      map[(size_t)at] = 4;
      if (!check_refusal(map, map.data(), n, n, false, CwFilterMapFault::tables, at)) return 1;
    }
    // without tables a map of 5s is accepted
    ++g_walked;
    CwFilterLists l;
    const std::vector<int32_t> off((size_t)n, kCwFilterOff);
    if (!build_cw_filter_lists(off.data(), n, n, false, nullptr, l) || !l.filtered.empty()) return violated("an all-off map needs no tables", off) ? 0 : 1;
  }
  std::printf("stage params lists: %ld maps walked, no violation\n", g_walked);
  return 0;
}
