// tests/pan_map_check.cpp -- walks check_pan_map() / pan_list_of() / build_pan_list() (t41_sdr_amd/csrc/rx_panmap.hpp), the
// pure functions that check the panadapter map's rows (t41rx_set_panadapter_map) and turn them, with the parameter sets'
// gains, into the ascending list of {channel, row, RFgain, rfGainAllBands} entries the list forms of the panadapter and
// beacon kernels run on.  A program of its own for tests/test_panadapter_map_lists.py: no GPU, no HIP.  Exit status 0 and
// a count of the maps walked, or 1 with the first violation.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rx_panmap.hpp"

using namespace t41;

namespace {

long g_walked = 0;

bool violated(const char *what, const std::vector<int32_t> &map) {
  std::printf("panadapter map lists: violated: %s\n  map (%zu channels):", what, map.size());
  for (size_t c = 0; c < map.size() && c < 80; ++c) std::printf(" %d", map[c]);
  std::printf("\n");
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond, map)

// set s has RFgain 10 + s and rfGainAllBands -3 s: every set's pair is its own
std::vector<PanGains> gains_of_sets(int k1) {
  std::vector<PanGains> g;
  for (int s = 0; s < k1; ++s) g.push_back(PanGains{10 + s, -3 * s});
  return g;
}

// the list a refused call must leave alone
std::vector<PanEntry> sentinel() { return {PanEntry{7, 9, 1, 2}, PanEntry{8, 3, 4, 5}}; }
bool is_sentinel(const std::vector<PanEntry> &l) {
  return l.size() == 2 && l[0].channel == 7 && l[0].row == 9 && l[0].RFgain == 1 && l[0].rfGainAllBands == 2 && l[1].channel == 8 && l[1].row == 3 &&
         l[1].RFgain == 4 && l[1].rfGainAllBands == 5;
}

// an accepted map: the list is exactly the channels with a row, ascending by channel, each with its own row and the two
// gains of its own set; no row twice
bool check_list(const std::vector<int32_t> &map, int n_rows, const std::vector<int32_t> *set_of = nullptr, int k1 = 1, int rows_in_use = 0) {
  ++g_walked;
  const int n = (int)map.size();
  const std::vector<PanGains> gains = gains_of_sets(k1);
  std::vector<PanEntry> l = sentinel();
  const PanMapVerdict v = build_pan_list(map.data(), n, n_rows, n, rows_in_use, gains.data(), set_of ? set_of->data() : nullptr, l);
  REQUIRE(bool(v) && v.fault == PanMapFault::none && v.channel == -1 && v.other == -1);
  size_t k = 0;
  for (int c = 0; c < n; ++c)
    if (map[(size_t)c] >= 0) {
      const int s = set_of ? (*set_of)[(size_t)c] : 0;
      REQUIRE(k < l.size() && l[k].channel == c && l[k].row == map[(size_t)c]);
      REQUIRE(l[k].RFgain == 10 + s && l[k].rfGainAllBands == -3 * s);
      ++k;
    }
  REQUIRE(k == l.size() && (int)l.size() <= n_rows);
  for (size_t i = 1; i < l.size(); ++i) REQUIRE(l[i - 1].channel < l[i].channel);
  std::vector<int> seen((size_t)n_rows, 0);
  for (const PanEntry &e : l) REQUIRE(e.channel >= 0 && e.channel < n && e.row >= 0 && e.row < n_rows && seen[(size_t)e.row]++ == 0);
  return true;
}

// a refused map: the fault, the entries it names, and the list left as it was
bool check_refusal(const std::vector<int32_t> &map, const int32_t *ptr, int n, int n_rows, int nchan, int rows_in_use, PanMapFault want, int channel,
                   int other = -1) {
  ++g_walked;
  const std::vector<PanGains> gains = gains_of_sets(1);
  std::vector<PanEntry> l = sentinel();
  const PanMapVerdict v = build_pan_list(ptr, n, n_rows, nchan, rows_in_use, gains.data(), nullptr, l);
  REQUIRE(!v && v.fault == want && v.channel == channel && v.other == other);
  REQUIRE(is_sentinel(l));
  const PanMapVerdict w = check_pan_map(ptr, n, n_rows, nchan, rows_in_use);
  REQUIRE(w.fault == v.fault && w.channel == v.channel && w.other == v.other);
  return true;
}

bool run() {
  // the three maps of tests/test_panadapter_map.py: 1 of 5; 2 of 5 with the rows permuted and a row nobody names; all 5 permuted
  {
    std::vector<int32_t> map{-1, -1, -1, 0, -1};
    if (!check_list(map, 1)) return false;
    std::vector<PanEntry> l;
    const std::vector<PanGains> g = gains_of_sets(1);
    build_pan_list(map.data(), 5, 1, 5, 0, g.data(), nullptr, l);
    REQUIRE(l.size() == 1 && l[0].channel == 3 && l[0].row == 0);
  }
  {
    std::vector<int32_t> map{-1, 2, -1, -1, 0};
    if (!check_list(map, 3)) return false;
    std::vector<PanEntry> l;
    const std::vector<PanGains> g = gains_of_sets(1);
    build_pan_list(map.data(), 5, 3, 5, 0, g.data(), nullptr, l);
    REQUIRE(l.size() == 2 && l[0].channel == 1 && l[0].row == 2 && l[1].channel == 4 && l[1].row == 0);
  }
  {
    std::vector<int32_t> map{3, 0, 4, 1, 2};
    if (!check_list(map, 5)) return false;
    std::vector<PanEntry> l;
    const std::vector<PanGains> g = gains_of_sets(1);
    build_pan_list(map.data(), 5, 5, 5, 0, g.data(), nullptr, l);
    REQUIRE(l.size() == 5 && l[0].row == 3 && l[1].row == 0 && l[2].row == 4 && l[3].row == 1 && l[4].row == 2 && l[4].channel == 4);
  }
  // 4096 channels with 2 listed, and nobody
  {
    std::vector<int32_t> map(4096, -1);
    if (!check_list(map, 1)) return false;
    if (!check_list(map, 2)) return false;
    map[4095] = 0;
    map[17] = 1;
    if (!check_list(map, 2)) return false;
    std::vector<PanEntry> l;
    const std::vector<PanGains> g = gains_of_sets(1);
    build_pan_list(map.data(), 4096, 2, 4096, 0, g.data(), nullptr, l);
    REQUIRE(l.size() == 2 && l[0].channel == 17 && l[0].row == 1 && l[1].channel == 4095 && l[1].row == 0 && l[1].RFgain == 10);
  }
  // lists of 0, 1 and all
  for (int n : {1, 5, 64, 70}) {
    if (!check_list(std::vector<int32_t>((size_t)n, -1), 1)) return false;
    std::vector<int32_t> one((size_t)n, -1);
    one[(size_t)(n / 2)] = n - 1;  // the last row of n
    if (!check_list(one, n)) return false;
    std::vector<int32_t> all((size_t)n);
    for (int c = 0; c < n; ++c) all[(size_t)c] = n - 1 - c;
    if (!check_list(all, n)) return false;
  }
  // the gains come from the channel's own set: a table over three sets, plain and staged sets alike (the list does not
  // know the flag), and again after a set change
  {
    std::vector<int32_t> map{-1, 2, 4, -1, 0, 1, 3}, set_of{2, 1, 0, 1, 2, 2, 0};
    if (!check_list(map, 5, &set_of, 3)) return false;
    std::vector<PanGains> g = gains_of_sets(3);
    std::vector<PanEntry> l = pan_list_of(map.data(), 7, g.data(), set_of.data());
    REQUIRE(l.size() == 5 && l[0].channel == 1 && l[0].RFgain == 11 && l[0].rfGainAllBands == -3);
    REQUIRE(l[1].channel == 2 && l[1].RFgain == 10 && l[1].rfGainAllBands == 0 && l[2].channel == 4 && l[2].RFgain == 12 && l[2].rfGainAllBands == -6);
    ++g_walked;
    // set 1 changes, then the table: the rebuilt list follows, rows and channels stay
    g[1] = PanGains{40, 7};
    l = pan_list_of(map.data(), 7, g.data(), set_of.data());
    REQUIRE(l.size() == 5 && l[0].RFgain == 40 && l[0].rfGainAllBands == 7 && l[0].row == 2 && l[1].RFgain == 10 && l[2].RFgain == 12);
    ++g_walked;
    set_of[4] = 1;
    l = pan_list_of(map.data(), 7, g.data(), set_of.data());
    REQUIRE(l[2].channel == 4 && l[2].row == 0 && l[2].RFgain == 40 && l[2].rfGainAllBands == 7);
    ++g_walked;
    // the sets removed: every listed channel takes set 0's
    l = pan_list_of(map.data(), 7, g.data(), nullptr);
    for (const PanEntry &e : l) REQUIRE(e.RFgain == 10 && e.rfGainAllBands == 0);
    ++g_walked;
  }
  // every refusal
  const int32_t kMin = std::numeric_limits<int32_t>::min(), kMax = std::numeric_limits<int32_t>::max();
  std::vector<int32_t> ok(19, -1);
  for (int c = 0; c < 19; c += 2) ok[(size_t)c] = c / 2;  // rows 0 .. 9
  if (!check_list(ok, 10)) return false;
  if (!check_refusal(ok, ok.data(), 18, 10, 19, 0, PanMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 20, 10, 19, 0, PanMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 0, 10, 19, 0, PanMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 0, 0, 0, 0, PanMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), -1, 1, -1, 0, PanMapFault::count, -1)) return false;
  if (!check_refusal(ok, nullptr, 19, 10, 19, 0, PanMapFault::null_map, -1)) return false;
  for (int n_rows : {0, -1, 20, kMin, kMax})
    if (!check_refusal(ok, ok.data(), 19, n_rows, 19, 0, PanMapFault::rows, -1)) return false;
  for (int c : {0, 7, 18})
    for (int32_t bad : {-2, 10, 11, kMin, kMax}) {
      std::vector<int32_t> map = ok;
      map[(size_t)c] = bad;
      if (!check_refusal(map, map.data(), 19, 10, 19, 0, PanMapFault::entry, c)) return false;
    }
  for (int c : {1, 7, 17}) {
    std::vector<int32_t> map = ok;
    map[(size_t)c] = 9;  // channel 18's row
    if (!check_refusal(map, map.data(), 19, 10, 19, 0, PanMapFault::twice, 18, c)) return false;
  }
  // the first offending entry is the one named
  {
    std::vector<int32_t> map = ok;
    map[3] = 0;    // row 0 a second time
    map[5] = 10;   // out of range
    if (!check_refusal(map, map.data(), 19, 10, 19, 0, PanMapFault::twice, 3, 0)) return false;
    map[1] = -2;
    if (!check_refusal(map, map.data(), 19, 10, 19, 0, PanMapFault::entry, 1)) return false;
  }
  // the panadapter on: the rows are fixed
  if (!check_list(ok, 10, nullptr, 1, 10)) return false;
  if (!check_refusal(ok, ok.data(), 19, 10, 19, 19, PanMapFault::resize, -1)) return false;
  if (!check_refusal(ok, ok.data(), 19, 10, 19, 9, PanMapFault::resize, -1)) return false;
  if (!check_refusal(ok, ok.data(), 19, 11, 19, 10, PanMapFault::resize, -1)) return false;
  {
    std::vector<int32_t> map = ok;
    map[5] = 10;  // an entry's fault is reported ahead of the rows'
    if (!check_refusal(map, map.data(), 19, 10, 19, 19, PanMapFault::entry, 5)) return false;
  }
  return true;
}

}  // namespace

int main() {
  if (!run()) return 1;
  std::printf("panadapter map lists: %ld maps walked, no violation\n", g_walked);
  return 0;
}
