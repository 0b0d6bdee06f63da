// tests/nr_map_check.cpp -- walks build_nr_map_lists() (t41_sdr_amd/csrc/rx_nrmap.hpp), the pure function that turns the
// noise-reduction map (t41rx_set_nr_map) and the stage map into the spectral list with its kinds, the Xanr() list sorted
// by class and the table of workgroups over it.  A program of its own for tests/test_nr_map_lists.py: no GPU, no HIP.
// Exit status 0 and a count of the maps walked, or 1 with the first violation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rx_nrmap.hpp"

using namespace t41;

namespace {

long g_walked = 0;

// a map as one code per channel: nrOptionSelect + 4 * ANR_notchOn
bool violated(const char *what, const std::vector<int32_t> &map) {
  std::printf("nr map lists: violated: %s\n  map (%zu channels, kind + 4 notch):", what, map.size());
  for (size_t c = 0; c < map.size() && c < 80; ++c) std::printf(" %d", map[c]);
  std::printf("\n");
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond, map)

// (the tests' own generator: the same maps in every run)
uint32_t g_rng = 24680u;
uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

void split(const std::vector<int32_t> &map, std::vector<int32_t> &kind, std::vector<int32_t> &notch) {
  kind.resize(map.size());
  notch.resize(map.size());
  for (size_t c = 0; c < map.size(); ++c) {
    kind[c] = map[c] & 3;
    notch[c] = map[c] >> 2;
  }
}

// an accepted map with this stage map (null: none)
bool check_lists(const std::vector<int32_t> &map, const std::vector<uint32_t> *stages) {
  ++g_walked;
  const int n = (int)map.size();
  std::vector<int32_t> kind, notch;
  split(map, kind, notch);
  NrMapLists l;
  const NrMapVerdict v = build_nr_map_lists(kind.data(), notch.data(), n, n, stages ? stages->data() : nullptr, l);
  REQUIRE(bool(v) && v.fault == NrMapFault::none && v.channel == -1);
  auto runs = [&](int c) { return !stages || ((*stages)[(size_t)c] & stage_bit(kStageNr)) != 0; };
  // the spectral list is exactly the running channels with kind 1 or 2, ascending, and its kinds are theirs
  REQUIRE(l.spec.size() == l.spec_kind.size());
  size_t k = 0;
  bool any = false, spectral = false;
  for (int c = 0; c < n; ++c) {
    any = any || map[(size_t)c] != 0;
    spectral = spectral || kind[(size_t)c] == 2;
    if (runs(c) && (kind[(size_t)c] == 1 || kind[(size_t)c] == 2)) {
      REQUIRE(k < l.spec.size() && l.spec[k] == c && l.spec_kind[k] == kind[(size_t)c]);
      ++k;
    }
  }
  REQUIRE(k == l.spec.size());
  for (size_t i = 1; i < l.spec.size(); ++i) REQUIRE(l.spec[i - 1] < l.spec[i]);
  // "on" and the pass band's check ask the map alone, not the stage map
  REQUIRE(l.any == any && l.spectral == spectral);
  // every row: one class, 1 .. 16 live columns inside the list, on a workgroup boundary; classes in order, and only the
  // last row of a class may be short
  std::vector<int> served((size_t)n, 0);
  REQUIRE(l.anr.size() == l.rows.size() * (size_t)kNrMapCols);
  for (size_t r = 0; r < l.rows.size(); ++r) {
    const NrMapRow &row = l.rows[r];
    REQUIRE(row.cls >= 0 && row.cls < kNrClasses);
    REQUIRE(row.live >= 1 && row.live <= kNrMapCols);
    REQUIRE(row.offset >= 0 && row.offset % kNrMapCols == 0 && (size_t)(row.offset + kNrMapCols) <= l.anr.size());
    REQUIRE(row.offset == (int32_t)(r * (size_t)kNrMapCols));
    if (r > 0) REQUIRE(l.rows[r - 1].cls <= row.cls);
    if (r > 0 && l.rows[r - 1].cls == row.cls) REQUIRE(l.rows[r - 1].live == kNrMapCols);
    for (int i = 0; i < kNrMapCols; ++i) {
      const int32_t c = l.anr[(size_t)(row.offset + i)];
      REQUIRE(c >= 0 && c < n);  // (the padding too: a channel of the row's own class)
      REQUIRE(nr_map_class(kind[(size_t)c], notch[(size_t)c]) == row.cls && runs(c));
      if (i < row.live) ++served[(size_t)c];
      if (i > 0 && i < row.live) REQUIRE(l.anr[(size_t)(row.offset + i - 1)] < c);
      if (i >= row.live) REQUIRE(c == l.anr[(size_t)(row.offset + row.live - 1)]);
    }
  }
  // every channel of the Xanr() list is in exactly one row, and nobody else in any
  for (int c = 0; c < n; ++c) {
    const bool wants = runs(c) && nr_map_class(kind[(size_t)c], notch[(size_t)c]) >= 0;
    REQUIRE(served[(size_t)c] == (wants ? 1 : 0));
  }
  // an empty list yields no launch: no entry, no row
  bool want_spec = false, want_anr = false;
  for (int c = 0; c < n; ++c) {
    want_spec = want_spec || (runs(c) && (kind[(size_t)c] == 1 || kind[(size_t)c] == 2));
    want_anr = want_anr || (runs(c) && (kind[(size_t)c] == 3 || notch[(size_t)c] == 1));
  }
  REQUIRE(want_spec == !l.spec.empty() && want_anr == !l.rows.empty() && want_anr == !l.anr.empty());
  // the device copy holds them
  const NrMapLayout lay = nr_map_layout(n);
  REQUIRE(l.spec.size() <= lay.spec_kind - lay.spec && l.spec_kind.size() <= lay.anr - lay.spec_kind);
  REQUIRE(l.anr.size() <= lay.rows - lay.anr && 4 * l.rows.size() <= lay.words - lay.rows && lay.rows % 4 == 0);
  return true;
}

// a refused map: the fault, the channel it names, and `out` as it was
bool check_refusal(const std::vector<int32_t> &map, const int32_t *kind, const int32_t *notch, int n, int n_channels, NrMapFault fault, int channel) {
  ++g_walked;
  NrMapLists l;
  l.spec = {41, 42};
  l.spec_kind = {2};
  l.anr = {8, 9, 10};
  l.rows = {NrMapRow{16, 3, 2, 0}};
  l.any = true;
  const NrMapVerdict v = build_nr_map_lists(kind, notch, n, n_channels, nullptr, l);
  REQUIRE(!v && v.fault == fault && v.channel == channel);
  REQUIRE(l.spec.size() == 2 && l.spec[0] == 41 && l.spec[1] == 42 && l.spec_kind.size() == 1 && l.spec_kind[0] == 2);
  REQUIRE(l.anr.size() == 3 && l.anr[0] == 8 && l.anr[2] == 10);
  REQUIRE(l.rows.size() == 1 && l.rows[0].offset == 16 && l.rows[0].live == 3 && l.rows[0].cls == 2 && l.any && !l.spectral);
  return true;
}

// the four stage maps of a size: none, the identity (every stage everywhere), nobody listed, a random one
bool check_with_stage_maps(const std::vector<int32_t> &map) {
  const size_t n = map.size();
  std::vector<uint32_t> all(n, kStageAll), nobody(n, kStageAll & ~stage_bit(kStageNr)), random(n);
  for (size_t c = 0; c < n; ++c) random[c] = rnd() & kStageAll & ~stage_bit(kStageCwDecode);
  return check_lists(map, nullptr) && check_lists(map, &all) && check_lists(map, &nobody) && check_lists(map, &random);
}

// the code of a class of the Xanr() list that is not also in the spectral list
constexpr int32_t kCodeOfClass[kNrClasses] = {3, 4, 7};

}  // namespace

int main() {
  // every map over ({0..3} x {0, 1})^n, n <= 3
  for (int n = 1; n <= 3; ++n) {
    int total = 1;
    for (int i = 0; i < n; ++i) total *= 8;
    for (int code = 0; code < total; ++code) {
      std::vector<int32_t> map((size_t)n);
      int r = code;
      for (int c = 0; c < n; ++c) {
        map[(size_t)c] = r % 8;
        r /= 8;
      }
      if (!check_with_stage_maps(map)) return 1;
    }
  }
  // the sizes either side of one, two and four workgroups of sixteen columns
  const int sizes[7] = {1, 15, 16, 17, 33, 64, 65};
  for (int n : sizes) {
    // random maps; the empty map; all one class (every class, and each of the eight combinations)
    for (int kind = 0; kind < 2 + 8; ++kind) {
      std::vector<int32_t> map((size_t)n);
      for (int c = 0; c < n; ++c) map[(size_t)c] = kind < 2 ? (int32_t)(rnd() % 8) : kind - 2;
      if (!check_with_stage_maps(map)) return 1;
    }
    // a class of exactly 1, 16 and 17 channels among channels of the other classes, Kim and spectral interleaved
    for (int cls = 0; cls < kNrClasses; ++cls)
      for (int count : {1, 16, 17}) {
        if (count > n) continue;
        std::vector<int32_t> map((size_t)n);
        for (int c = 0; c < n; ++c) map[(size_t)c] = (c & 1) ? (c & 2 ? 1 : 2) : kCodeOfClass[(cls + 1 + (c >> 1) % 2) % kNrClasses];
        // the class's channels spread over the size
        for (int i = 0; i < count; ++i) map[(size_t)((long)i * n / count)] = kCodeOfClass[cls];
        int have = 0;
        for (int c = 0; c < n; ++c) have += map[(size_t)c] == kCodeOfClass[cls];
        if (have != count) return violated("the generator made the class's size", map) ? 0 : 1;
        if (!check_with_stage_maps(map)) return 1;
      }
  }
  // the refusals, each at the first, a middle and the last channel
  for (int n : sizes) {
    const std::vector<int32_t> good((size_t)n, 2), zero((size_t)n, 0);
    for (int wrong : {0, n - 1, n + 1, -1})
      if (wrong != n && !check_refusal(good, good.data(), zero.data(), wrong, n, NrMapFault::count, -1)) return 1;
    if (!check_refusal(good, good.data(), zero.data(), 0, 0, NrMapFault::count, -1)) return 1;
    if (!check_refusal(good, nullptr, zero.data(), n, n, NrMapFault::null_map, -1)) return 1;
    if (!check_refusal(good, good.data(), nullptr, n, n, NrMapFault::null_map, -1)) return 1;
    if (!check_refusal(good, nullptr, nullptr, n, n, NrMapFault::null_map, -1)) return 1;
    for (int at : {0, n / 2, n - 1})
      for (int32_t bad : {-1, 4, 1 << 30, INT32_MIN}) {
        std::vector<int32_t> k((size_t)n, 1), t((size_t)n, 1);
        k[(size_t)at] = bad;
        if (!check_refusal(k, k.data(), t.data(), n, n, NrMapFault::kind, at)) return 1;
        k[(size_t)at] = 3;
        t[(size_t)at] = bad == 4 ? 2 : bad;
        if (!check_refusal(t, k.data(), t.data(), n, n, NrMapFault::notch, at)) return 1;
      }
  }
  std::printf("nr map lists: %ld maps walked, no violation\n", g_walked);
  return 0;
}
