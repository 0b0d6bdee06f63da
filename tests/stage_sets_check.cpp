// tests/stage_sets_check.cpp -- walks build_stage_sets() (t41_sdr_amd/csrc/rx_stagesets.hpp), the pure function that
// turns the parameter sets' noise-reduction values, the channels' table, the optional noise-reduction map and the optional
// stage map into every channel's effective kind and notch, its row of the device table and the lists of the two launches.
// Against a three-line restatement: kind / notch are the map's where there is one, else the set's; the row is the set's;
// the lists are build_nr_map_lists() of the effective values (itself walked by tests/nr_map_check.cpp).  And every
// refusal, which leaves `out` as it was.  A program of its own for tests/test_stage_sets_lists.py: no GPU, no HIP.
// Exit status 0 and a count of the cases walked, or 1 with the first violation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rx_stagesets.hpp"

using namespace t41;

namespace {

long g_walked = 0;

struct Case {
  std::vector<StageSetNr> sets;
  std::vector<int32_t> set_of, kind_map, notch_map;  // maps empty: none
  std::vector<uint32_t> stages;                      // empty: none
};

bool violated(const char *what, const Case &k) {
  std::printf("stage sets: violated: %s\n  %zu sets (kind notch ok):", what, k.sets.size());
  for (const StageSetNr &s : k.sets) std::printf(" (%d %d %d)", s.kind, s.notch, (int)s.spectral_ok);
  std::printf("\n  set_of:");
  for (int32_t v : k.set_of) std::printf(" %d", v);
  std::printf("\n  map (kind + 4 notch):");
  for (size_t c = 0; c < k.kind_map.size(); ++c) std::printf(" %d", k.kind_map[c] + 4 * k.notch_map[c]);
  std::printf("\n  stage map:");
  for (uint32_t v : k.stages) std::printf(" %u", v);
  std::printf("\n");
  return false;
}
#define REQUIRE(cond) \
  if (!(cond)) return violated(#cond, k)

uint32_t g_rng = 13579u;
uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

bool same_lists(const NrMapLists &a, const NrMapLists &b) {
  if (a.spec != b.spec || a.spec_kind != b.spec_kind || a.anr != b.anr || a.any != b.any || a.spectral != b.spectral || a.rows.size() != b.rows.size())
    return false;
  for (size_t i = 0; i < a.rows.size(); ++i)
    if (a.rows[i].offset != b.rows[i].offset || a.rows[i].live != b.rows[i].live || a.rows[i].cls != b.rows[i].cls) return false;
  return true;
}

StageSetsVerdict build(const Case &k, StageSetsNr &out) {
  const bool map = !k.kind_map.empty();
  return build_stage_sets(k.sets.data(), (int)k.sets.size(), k.set_of.data(), (int)k.set_of.size(), (int)k.set_of.size(),
                          map ? k.kind_map.data() : nullptr, map ? k.notch_map.data() : nullptr, k.stages.empty() ? nullptr : k.stages.data(), out);
}

// a sentinel `out` and the check that a refusal left it alone
StageSetsNr sentinel() {
  StageSetsNr s;
  s.kind = {7, 8};
  s.notch = {9};
  s.rows = {NrSetRow{1.0f, 2.0f, 3.0f, 4, 5, {0, 0, 0}}};
  s.lists.spec = {41};
  s.lists.any = true;
  return s;
}
bool untouched(const StageSetsNr &s) {
  return s.kind.size() == 2 && s.kind[0] == 7 && s.kind[1] == 8 && s.notch.size() == 1 && s.notch[0] == 9 && s.rows.size() == 1 &&
         s.rows[0].alpha == 1.0f && s.rows[0].vad_hi == 5 && s.lists.spec.size() == 1 && s.lists.spec[0] == 41 && s.lists.any && !s.lists.spectral;
}

// the restatement, and the first channel the spectral check trips at
bool check_case(const Case &k) {
  ++g_walked;
  const int n = (int)k.set_of.size();
  const bool map = !k.kind_map.empty();
  std::vector<int32_t> kind((size_t)n), notch((size_t)n);
  int bad = -1;
  for (int c = 0; c < n; ++c) {
    const StageSetNr &s = k.sets[(size_t)k.set_of[(size_t)c]];
    kind[(size_t)c] = map ? k.kind_map[(size_t)c] : s.kind;
    notch[(size_t)c] = map ? k.notch_map[(size_t)c] : s.notch;
    if (bad < 0 && kind[(size_t)c] == 2 && !s.spectral_ok) bad = c;
  }
  StageSetsNr out = sentinel();
  const StageSetsVerdict v = build(k, out);
  if (bad >= 0) {
    REQUIRE(!v && v.fault == StageSetsFault::spectral && v.channel == bad && v.set == k.set_of[(size_t)bad]);
    REQUIRE(untouched(out));
    return true;
  }
  REQUIRE(bool(v) && v.fault == StageSetsFault::none && v.channel == -1 && v.set == -1);
  REQUIRE(out.kind == kind && out.notch == notch && out.rows.size() == (size_t)n);
  for (int c = 0; c < n; ++c) {
    const StageSetNr &s = k.sets[(size_t)k.set_of[(size_t)c]];
    const NrSetRow &r = out.rows[(size_t)c];
    REQUIRE(std::memcmp(&r.alpha, &s.alpha, 4) == 0 && std::memcmp(&r.beta, &s.beta, 4) == 0 && std::memcmp(&r.psi, &s.psi, 4) == 0);
    REQUIRE(r.vad_lo == s.vad_lo && r.vad_hi == s.vad_hi && r.pad[0] == 0 && r.pad[1] == 0 && r.pad[2] == 0);
  }
  NrMapLists want;
  REQUIRE(bool(build_nr_map_lists(kind.data(), notch.data(), n, n, k.stages.empty() ? nullptr : k.stages.data(), want)));
  REQUIRE(same_lists(out.lists, want));
  return true;
}

bool check_refusal(const Case &k, const StageSetNr *sets, int n_sets, const int32_t *set_of, int n, int n_channels, const int32_t *km,
                   const int32_t *tm, StageSetsFault fault, int channel, int set) {
  ++g_walked;
  StageSetsNr out = sentinel();
  const StageSetsVerdict v = build_stage_sets(sets, n_sets, set_of, n, n_channels, km, tm, nullptr, out);
  REQUIRE(!v && v.fault == fault && v.channel == channel && v.set == set);
  REQUIRE(untouched(out));
  return true;
}

StageSetNr a_set(int code, bool ok, int i) {
  StageSetNr s;
  s.kind = code & 3;
  s.notch = code >> 2;
  s.alpha = 0.5f + 0.01f * (float)i;
  s.beta = 0.25f + 0.01f * (float)i;
  s.psi = 10.0f + (float)i;
  s.vad_lo = 1 + i;
  s.vad_hi = 30 + 2 * i;
  s.spectral_ok = ok;
  return s;
}

// with no map, every map over the codes of `map_codes`^n is too many: all-equal maps of every code, and a few random ones
bool check_with_maps_and_stage_maps(Case k) {
  const size_t n = k.set_of.size();
  std::vector<std::vector<uint32_t>> stage_maps = {{}, std::vector<uint32_t>(n, kStageAll), std::vector<uint32_t>(n, kStageAll & ~stage_bit(kStageNr)),
                                                   std::vector<uint32_t>(n)};
  for (size_t c = 0; c < n; ++c) stage_maps[3][c] = rnd() & kStageAll & ~stage_bit(kStageCwDecode);
  for (const std::vector<uint32_t> &sm : stage_maps) {
    k.stages = sm;
    k.kind_map.clear();
    k.notch_map.clear();
    if (!check_case(k)) return false;
    for (int code = 0; code < 8 + 2; ++code) {
      k.kind_map.assign(n, 0);
      k.notch_map.assign(n, 0);
      for (size_t c = 0; c < n; ++c) {
        const int v = code < 8 ? code : (int)(rnd() % 8);
        k.kind_map[c] = v & 3;
        k.notch_map[c] = v >> 2;
      }
      if (!check_case(k)) return false;
    }
  }
  return true;
}

}  // namespace

int main() {
  // every (sets, table) with up to 2 sets over the eight codes x {band passes, band fails} and up to 3 channels
  for (int n_sets = 1; n_sets <= 2; ++n_sets) {
    int set_total = 1;
    for (int i = 0; i < n_sets; ++i) set_total *= 16;
    for (int sc = 0; sc < set_total; ++sc)
      for (int n = 1; n <= 3; ++n) {
        int tab_total = 1;
        for (int i = 0; i < n; ++i) tab_total *= n_sets;
        for (int tc = 0; tc < tab_total; ++tc) {
          Case k;
          int r = sc;
          for (int i = 0; i < n_sets; ++i) {
            k.sets.push_back(a_set(r % 8, (r / 8) % 2 != 0, i));
            r /= 16;
          }
          r = tc;
          for (int c = 0; c < n; ++c) {
            k.set_of.push_back(r % n_sets);
            r /= n_sets;
          }
          if (!check_with_maps_and_stage_maps(k)) return 1;
        }
      }
  }
  // 19 channels on 3 sets in a non-monotone table, and the sizes either side of a workgroup of sixteen columns, random sets
  for (int n : {15, 16, 17, 19, 33, 65})
    for (int rep = 0; rep < 3; ++rep) {
      Case k;
      const int n_sets = 1 + (int)(rnd() % 4);
      for (int i = 0; i < n_sets; ++i) k.sets.push_back(a_set((int)(rnd() % 8), rnd() % 4 != 0, i));
      for (int c = 0; c < n; ++c) k.set_of.push_back((int32_t)(rnd() % (uint32_t)n_sets));
      if (!check_with_maps_and_stage_maps(k)) return 1;
    }
  // the refusals
  {
    Case k;
    k.sets = {a_set(1, true, 0), a_set(3, true, 1)};
    k.set_of = {0, 1, 1, 0};
    const std::vector<int32_t> km = {0, 1, 2, 3}, tm = {0, 1, 0, 1};
    const StageSetNr *s = k.sets.data();
    const int32_t *t = k.set_of.data();
    const StageSetsFault count = StageSetsFault::count;
    if (!check_refusal(k, s, 2, t, 3, 4, nullptr, nullptr, count, -1, -1) || !check_refusal(k, s, 2, t, 5, 4, nullptr, nullptr, count, -1, -1) ||
        !check_refusal(k, s, 2, t, 0, 0, nullptr, nullptr, count, -1, -1) || !check_refusal(k, s, 0, t, 4, 4, nullptr, nullptr, count, -1, -1) ||
        !check_refusal(k, nullptr, 2, t, 4, 4, nullptr, nullptr, count, -1, -1) || !check_refusal(k, s, 2, nullptr, 4, 4, nullptr, nullptr, count, -1, -1) ||
        !check_refusal(k, s, 2, t, 4, 4, km.data(), nullptr, count, -1, -1) || !check_refusal(k, s, 2, t, 4, 4, nullptr, tm.data(), count, -1, -1))
      return 1;
    for (int at : {0, 2, 3})
      for (int32_t bad : {-1, 2, 1 << 30, INT32_MIN}) {
        std::vector<int32_t> tab = k.set_of;
        tab[(size_t)at] = bad;
        if (!check_refusal(k, s, 2, tab.data(), 4, 4, nullptr, nullptr, StageSetsFault::set, at, -1)) return 1;
        std::vector<int32_t> kk = km, tt = tm;
        kk[(size_t)at] = bad == 2 ? 4 : bad;
        if (!check_refusal(k, s, 2, t, 4, 4, kk.data(), tt.data(), StageSetsFault::kind, at, -1)) return 1;
        kk = km;
        tt[(size_t)at] = bad;
        if (!check_refusal(k, s, 2, t, 4, 4, kk.data(), tt.data(), StageSetsFault::notch, at, -1)) return 1;
      }
    // a set's own value out of range (the setters validate the structs first; the function does not rely on it)
    std::vector<StageSetNr> broken = k.sets;
    broken[1].kind = 4;
    if (!check_refusal(k, broken.data(), 2, t, 4, 4, nullptr, nullptr, StageSetsFault::kind, 1, 1)) return 1;
    broken = k.sets;
    broken[0].notch = 2;
    if (!check_refusal(k, broken.data(), 2, t, 4, 4, nullptr, nullptr, StageSetsFault::notch, 0, 0)) return 1;
    // the spectral check names the first channel and its set; a failing set nobody runs kind 2 on is accepted
    broken = k.sets;
    broken[1].spectral_ok = false;
    if (!check_refusal(k, broken.data(), 2, t, 4, 4, km.data(), tm.data(), StageSetsFault::spectral, 2, 1)) return 1;
    broken[1].kind = 2;
    if (!check_refusal(k, broken.data(), 2, t, 4, 4, nullptr, nullptr, StageSetsFault::spectral, 1, 1)) return 1;
    const std::vector<int32_t> nobody = {0, 0, 0, 0};
    StageSetsNr out;
    ++g_walked;
    if (!build_stage_sets(broken.data(), 2, nobody.data(), 4, 4, nullptr, nullptr, nullptr, out)) return violated("a failing set no channel names is accepted", k) ? 0 : 1;
  }
  std::printf("stage sets: %ld cases walked, no violation\n", g_walked);
  return 0;
}
