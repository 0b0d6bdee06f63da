// tests/ft8_map_check.cpp -- walks build_ft8_list() (t41_sdr_amd/csrc/rx_ft8map.hpp), the pure function that checks the FT8
// map's rows (t41rx_set_ft8_map) and turns them into the ascending list of {channel, row} pairs the list forms of the FT8
// kernels run on.  A program of its own for tests/test_ft8_map_lists.py: no GPU, no HIP.  Exit status 0 and a count of the
// maps walked, or 1 with the first violation.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rx_ft8map.hpp"

using namespace t41;

namespace {

long g_walked = 0;

bool violated(const char *what, const std::vector<int32_t> &map) {
  std::printf("FT8 map lists: violated: %s\n  map (%zu channels):", what, map.size());
  for (size_t c = 0; c < map.size() && c < 80; ++c) std::printf(" %d", map[c]);
  std::printf("\n");
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond, map)

// the list a refused call must leave alone
std::vector<Ft8Pair> sentinel() { return {Ft8Pair{7, 9}, Ft8Pair{8, 3}}; }
bool is_sentinel(const std::vector<Ft8Pair> &l) {
  return l.size() == 2 && l[0].channel == 7 && l[0].row == 9 && l[1].channel == 8 && l[1].row == 3;
}

// an accepted map: the list is exactly the channels with a row, ascending by channel, each with its own row; no row twice
bool check_list(const std::vector<int32_t> &map, int n_rows, int rows_in_use = 0) {
  ++g_walked;
  const int n = (int)map.size();
  std::vector<Ft8Pair> l = sentinel();
  const Ft8MapVerdict v = build_ft8_list(map.data(), n, n_rows, n, rows_in_use, l);
  REQUIRE(bool(v) && v.fault == Ft8MapFault::none && v.channel == -1 && v.other == -1);
  size_t k = 0;
  for (int c = 0; c < n; ++c)
    if (map[(size_t)c] >= 0) {
      REQUIRE(k < l.size() && l[k].channel == c && l[k].row == map[(size_t)c]);
      ++k;
    }
  REQUIRE(k == l.size() && (int)l.size() <= n_rows);
  for (size_t i = 1; i < l.size(); ++i) REQUIRE(l[i - 1].channel < l[i].channel);
  std::vector<int> seen((size_t)n_rows, 0);
  for (const Ft8Pair &e : l) REQUIRE(e.channel >= 0 && e.channel < n && e.row >= 0 && e.row < n_rows && seen[(size_t)e.row]++ == 0);
  return true;
}

// a refused map: the fault, the entries it names, and the list left as it was
bool check_refusal(const std::vector<int32_t> &map, const int32_t *ptr, int n, int n_rows, int nchan, int rows_in_use, Ft8MapFault want, int channel,
                   int other = -1) {
  ++g_walked;
  std::vector<Ft8Pair> l = sentinel();
  const Ft8MapVerdict v = build_ft8_list(ptr, n, n_rows, nchan, rows_in_use, l);
  REQUIRE(!v && v.fault == want && v.channel == channel && v.other == other);
  REQUIRE(is_sentinel(l));
  return true;
}

// every map of n channels over n_rows rows, entries -1 .. n_rows - 1: accepted exactly when no row is named twice, and a
// refusal names the second channel of the first pair and the first
bool every_map(int n, int n_rows) {
  std::vector<int32_t> map((size_t)n, -1);
  for (;;) {
    int second = -1, first = -1;
    for (int c = 0; c < n && second < 0; ++c)
      for (int b = 0; b < c; ++b)
        if (map[(size_t)c] >= 0 && map[(size_t)b] == map[(size_t)c]) {
          second = c;
          first = b;
          break;
        }
    if (second < 0 ? !check_list(map, n_rows) : !check_refusal(map, map.data(), n, n_rows, n, 0, Ft8MapFault::twice, second, first)) return false;
    int c = 0;
    while (c < n && map[(size_t)c] == n_rows - 1) map[(size_t)c++] = -1;
    if (c == n) return true;
    ++map[(size_t)c];
  }
}

bool run() {
  // every map of 1 .. 4 channels
  for (int n = 1; n <= 4; ++n)
    for (int n_rows = 1; n_rows <= n; ++n_rows)
      if (!every_map(n, n_rows)) return false;
  // lists of 0, 1 and all
  for (int n : {1, 5, 64, 4096}) {
    if (!check_list(std::vector<int32_t>((size_t)n, -1), 1)) return false;
    std::vector<int32_t> one((size_t)n, -1);
    one[(size_t)(n / 2)] = 0;
    if (!check_list(one, 1)) return false;
    one[(size_t)(n / 2)] = n - 1;  // the last row of n
    if (!check_list(one, n)) return false;
    std::vector<int32_t> all((size_t)n);
    for (int c = 0; c < n; ++c) all[(size_t)c] = c;
    if (!check_list(all, n)) return false;
    std::vector<Ft8Pair> l;
    const std::vector<int32_t> &map = all;
    build_ft8_list(all.data(), n, n, n, 0, l);
    REQUIRE((int)l.size() == n && l.front().channel == 0 && l.back().channel == n - 1 && l.back().row == n - 1);
  }
  // a pseudo-random permutation of 4096 rows, every fourth channel unlisted
  {
    const int n = 4096;
    std::vector<int32_t> map((size_t)n);
    for (int c = 0; c < n; ++c) map[(size_t)c] = c;
    uint32_t x = 12345u;
    for (int c = n - 1; c > 0; --c) {
      x = x * 1664525u + 1013904223u;
      const int j = (int)((x >> 8) % (uint32_t)(c + 1));
      const int32_t t = map[(size_t)c];
      map[(size_t)c] = map[(size_t)j];
      map[(size_t)j] = t;
    }
    for (int c = 0; c < n; c += 4) map[(size_t)c] = -1;
    if (!check_list(map, n)) return false;
  }
  // every refusal
  const int32_t kMin = std::numeric_limits<int32_t>::min(), kMax = std::numeric_limits<int32_t>::max();
  std::vector<int32_t> ok(19, -1);
  for (int c = 0; c < 19; c += 2) ok[(size_t)c] = c / 2;  // rows 0 .. 9
  if (!check_list(ok, 10)) return false;
  if (!check_refusal(ok, ok.data(), 18, 10, 19, 0, Ft8MapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 20, 10, 19, 0, Ft8MapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 0, 10, 19, 0, Ft8MapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 0, 0, 0, 0, Ft8MapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), -1, 1, -1, 0, Ft8MapFault::count, -1)) return false;
  if (!check_refusal(ok, nullptr, 19, 10, 19, 0, Ft8MapFault::null_map, -1)) return false;
  for (int n_rows : {0, -1, 20, kMin, kMax})
    if (!check_refusal(ok, ok.data(), 19, n_rows, 19, 0, Ft8MapFault::rows, -1)) return false;
  for (int c : {0, 7, 18})
    for (int32_t bad : {-2, 10, 11, kMin, kMax}) {
      std::vector<int32_t> map = ok;
      map[(size_t)c] = bad;
      if (!check_refusal(map, map.data(), 19, 10, 19, 0, Ft8MapFault::entry, c)) return false;
    }
  for (int c : {1, 7, 17}) {
    std::vector<int32_t> map = ok;
    map[(size_t)c] = 9;  // channel 18's row
    if (!check_refusal(map, map.data(), 19, 10, 19, 0, Ft8MapFault::twice, 18, c)) return false;
  }
  // the first offending entry is the one named
  {
    std::vector<int32_t> map = ok;
    map[3] = 0;    // row 0 a second time
    map[5] = 10;   // out of range
    if (!check_refusal(map, map.data(), 19, 10, 19, 0, Ft8MapFault::twice, 3, 0)) return false;
    map[1] = -2;
    if (!check_refusal(map, map.data(), 19, 10, 19, 0, Ft8MapFault::entry, 1)) return false;
  }
  // FT8 receive on: the rows are fixed
  if (!check_list(ok, 10, 10)) return false;
  if (!check_refusal(ok, ok.data(), 19, 10, 19, 19, Ft8MapFault::resize, -1)) return false;
  if (!check_refusal(ok, ok.data(), 19, 10, 19, 9, Ft8MapFault::resize, -1)) return false;
  if (!check_refusal(ok, ok.data(), 19, 11, 19, 10, Ft8MapFault::resize, -1)) return false;
  {
    std::vector<int32_t> map = ok;
    map[5] = 10;  // an entry's fault is reported ahead of the rows'
    if (!check_refusal(map, map.data(), 19, 10, 19, 19, Ft8MapFault::entry, 5)) return false;
  }
  return true;
}

}  // namespace

int main() {
  if (!run()) return 1;
  std::printf("FT8 map lists: %ld maps walked, no violation\n", g_walked);
  return 0;
}
