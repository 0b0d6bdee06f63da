// tests/stage_map_check.cpp -- walks build_stage_lists() (t41_sdr_amd/csrc/rx_stagemap.hpp), the pure function that turns
// the stage map's masks (t41rx_set_stage_map) into the ascending channel list of each stage and the blanker's complement.
// A program of its own for tests/test_stage_map_lists.py: no GPU, no HIP.  Exit status 0 and a count of the maps walked,
// or 1 with the first violation.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "rx_stagemap.hpp"

using namespace t41;

namespace {

long g_walked = 0;

bool violated(const char *what, const std::vector<uint32_t> &map) {
  std::printf("stage map lists: violated: %s\n  map (%zu channels):", what, map.size());
  for (size_t c = 0; c < map.size() && c < 80; ++c) std::printf(" %u", map[c]);
  std::printf("\n");
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond, map)

// a mask the setter accepts
bool valid_mask(uint32_t m) {
  return !(m & ~kStageAll) && (!(m & stage_bit(kStageCwDecode)) || (m & stage_bit(kStageCwDetect)));
}

// an accepted map: every list is exactly the channels with the bit, ascending; the complement is the rest
bool check_lists(const std::vector<uint32_t> &map) {
  ++g_walked;
  const int n = (int)map.size();
  StageLists l;
  const StageMapVerdict v = build_stage_lists(map.data(), n, n, l);
  REQUIRE(bool(v) && v.fault == StageMapFault::none && v.channel == -1);
  for (int s = 0; s < kStageCount; ++s) {
    size_t k = 0;
    for (int c = 0; c < n; ++c)
      if (map[(size_t)c] & stage_bit(s)) {
        REQUIRE(k < l.list[s].size() && l.list[s][k] == c);
        ++k;
      }
    REQUIRE(k == l.list[s].size());
    for (size_t i = 1; i < l.list[s].size(); ++i) REQUIRE(l.list[s][i - 1] < l.list[s][i]);
  }
  // the blanker's two lists partition the channels
  REQUIRE(l.list[kStageNb].size() + l.nb_rest.size() == (size_t)n);
  std::vector<int> seen((size_t)n, 0);
  for (int32_t c : l.list[kStageNb]) REQUIRE(c >= 0 && c < n && seen[(size_t)c]++ == 0);
  for (int32_t c : l.nb_rest) REQUIRE(c >= 0 && c < n && seen[(size_t)c]++ == 0 && !(map[(size_t)c] & stage_bit(kStageNb)));
  for (size_t i = 1; i < l.nb_rest.size(); ++i) REQUIRE(l.nb_rest[i - 1] < l.nb_rest[i]);
  // the decoder's channels are the detector's: it reads their rows
  size_t k = 0;
  for (int32_t c : l.list[kStageCwDecode]) {
    while (k < l.list[kStageCwDetect].size() && l.list[kStageCwDetect][k] < c) ++k;
    REQUIRE(k < l.list[kStageCwDetect].size() && l.list[kStageCwDetect][k] == c);
  }
  return true;
}

// a refused map: the fault, the entry, and the lists left as they were
bool check_refusal(const std::vector<uint32_t> &map, const uint32_t *ptr, int n, int nchan, StageMapFault want, int channel) {
  ++g_walked;
  StageLists l;
  l.list[kStageEq] = {7, 9};
  l.nb_rest = {3};
  const StageMapVerdict v = build_stage_lists(ptr, n, nchan, l);
  REQUIRE(!v && v.fault == want && v.channel == channel);
  REQUIRE(l.list[kStageEq].size() == 2 && l.list[kStageEq][1] == 9 && l.nb_rest.size() == 1 && l.list[kStageNr].empty());
  return true;
}

// `count` channels listed for stage s out of n, spread out, channel 0 and the last one among them when count > 1
std::vector<uint32_t> listed(int n, int count, int s) {
  std::vector<uint32_t> map((size_t)n, 0u);
  for (int i = 0; i < count; ++i) {
    const int c = count == 1 ? n / 2 : (int)(((long long)i * (n - 1)) / (count - 1));
    map[(size_t)c] |= stage_bit(s) | (s == kStageCwDecode ? stage_bit(kStageCwDetect) : 0u);
  }
  return map;
}

bool run() {
  // every accepted mask over 1, 2 and 3 channels
  std::vector<uint32_t> masks;
  for (uint32_t m = 0; m <= kStageAll; ++m)
    if (valid_mask(m)) masks.push_back(m);
  if (masks.size() != 24) return violated("24 of the 32 masks are accepted", masks);
  for (uint32_t a : masks) {
    if (!check_lists({a})) return false;
    for (uint32_t b : masks) {
      if (!check_lists({a, b})) return false;
      for (uint32_t c : masks)
        if (!check_lists({a, b, c})) return false;
    }
  }
  // the empty lists and all channels, at the sizes the kernels' work units break at
  for (int n : {1, 15, 16, 17, 19, 63, 64, 65, 70, 4096}) {
    if (!check_lists(std::vector<uint32_t>((size_t)n, 0u))) return false;
    if (!check_lists(std::vector<uint32_t>((size_t)n, kStageAll))) return false;
    for (uint32_t m : masks)
      if (!check_lists(std::vector<uint32_t>((size_t)n, m))) return false;
  }
  // lists of 1 / 16 / 17 / 64 / 65 of 70 for every stage: their lengths
  for (int s = 0; s < kStageCount; ++s)
    for (int count : {1, 16, 17, 64, 65}) {
      const std::vector<uint32_t> map = listed(70, count, s);
      if (!check_lists(map)) return false;
      StageLists l;
      build_stage_lists(map.data(), 70, 70, l);
      REQUIRE((int)l.list[s].size() == count);
      REQUIRE((int)l.nb_rest.size() == (s == kStageNb ? 70 - count : 70));
      REQUIRE(count == 1 || (l.list[s].front() == 0 && l.list[s].back() == 69));
    }
  // a pseudo-random map of 4096 channels
  {
    std::vector<uint32_t> map(4096);
    uint32_t x = 12345u;
    for (auto &m : map) {
      do {
        x = x * 1664525u + 1013904223u;
        m = (x >> 20) & kStageAll;
      } while (!valid_mask(m));
    }
    if (!check_lists(map)) return false;
  }
  // every refusal
  const std::vector<uint32_t> ok(19, kStageAll);
  if (!check_refusal(ok, ok.data(), 18, 19, StageMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 20, 19, StageMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 0, 19, StageMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), 0, 0, StageMapFault::count, -1)) return false;
  if (!check_refusal(ok, ok.data(), -1, -1, StageMapFault::count, -1)) return false;
  if (!check_refusal(ok, nullptr, 19, 19, StageMapFault::null_map, -1)) return false;
  for (int c : {0, 7, 18})
    for (uint32_t bad : {32u, 33u, 64u, 0x80000000u, 0xffffffffu}) {
      std::vector<uint32_t> map = ok;
      map[(size_t)c] = bad;
      if (!check_refusal(map, map.data(), 19, 19, StageMapFault::bits, c)) return false;
    }
  for (int c : {0, 7, 18})
    for (uint32_t m = 0; m <= kStageAll; ++m) {
      if (valid_mask(m)) continue;
      std::vector<uint32_t> map = ok;
      map[(size_t)c] = m;  // CW_DECODE without CW_DETECT, whatever else
      if (!check_refusal(map, map.data(), 19, 19, StageMapFault::decode_without_detect, c)) return false;
    }
  // the first offending entry is the one named
  {
    std::vector<uint32_t> map = ok;
    map[3] = 16u;
    map[5] = 64u;
    if (!check_refusal(map, map.data(), 19, 19, StageMapFault::decode_without_detect, 3)) return false;
  }
  return true;
}

}  // namespace

int main() {
  if (!run()) return 1;
  std::printf("stage map lists: %ld maps walked, no violation\n", g_walked);
  return 0;
}
