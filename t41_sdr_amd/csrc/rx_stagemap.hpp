// t41_sdr_amd/csrc/rx_stagemap.hpp -- the stage map's lists (t41rx_set_stage_map; rx_stagemap.cpp): from the caller's mask
// per channel, the ascending list of channels each stage runs on.  Plain C++: no HIP, no context type, so that a CPU
// program can walk it (tests/stage_map_check.cpp), as tests/call_plan_check.cpp walks plan_call().
//
// The rule the lists serve: stage S runs on channel c exactly when the context's switch for S is on and bit S of the
// channel's mask is set.  The lists know nothing of the switches: a stage that is off launches nothing and never asks
// for its list.  The blanker alone also needs the channels it leaves out (StageLists::nb_rest): its carry ping-pongs
// between two slots and the slot flips for the whole context, so the list form copies a bypassed channel's carry to the
// slot the next call reads (nb_kernel.hip).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace t41 {

// the bits of a channel's mask, in the order the stages run (include/t41rx.h: T41RX_STAGE_*)
enum StageIndex : int { kStageEq = 0, kStageNr, kStageNb, kStageCwDetect, kStageCwDecode, kStageCount };
constexpr uint32_t kStageAll = (1u << kStageCount) - 1u;  // 31
constexpr uint32_t stage_bit(int stage) { return 1u << stage; }

struct StageLists {
  std::vector<int32_t> list[kStageCount];  // ascending channel numbers
  std::vector<int32_t> nb_rest;            // the channels not in list[kStageNb], ascending
};

// why a map is refused
enum class StageMapFault : int {
  none = 0,
  count,                  // n != n_channels (or no channels at all)
  null_map,               // no array
  bits,                   // a bit outside kStageAll; `channel` names the entry
  decode_without_detect,  // CW_DECODE without CW_DETECT: the decoder would read detector rows nobody wrote; `channel`
};
struct StageMapVerdict {
  StageMapFault fault = StageMapFault::none;
  int channel = -1;
  explicit operator bool() const { return fault == StageMapFault::none; }
};

// Checks the map (every entry, before anything is built) and fills `out`; a refused map leaves `out` as it was.
inline StageMapVerdict build_stage_lists(const uint32_t *stages_of_channel, int n, int n_channels, StageLists &out) {
  if (n_channels <= 0 || n != n_channels) return {StageMapFault::count, -1};
  if (!stages_of_channel) return {StageMapFault::null_map, -1};
  for (int c = 0; c < n; ++c) {
    const uint32_t m = stages_of_channel[c];
    if (m & ~kStageAll) return {StageMapFault::bits, c};
    if ((m & stage_bit(kStageCwDecode)) && !(m & stage_bit(kStageCwDetect))) return {StageMapFault::decode_without_detect, c};
  }
  StageLists fresh;
  for (int c = 0; c < n; ++c) {
    const uint32_t m = stages_of_channel[c];
    for (int s = 0; s < kStageCount; ++s)
      if (m & stage_bit(s)) fresh.list[s].push_back(c);
    if (!(m & stage_bit(kStageNb))) fresh.nb_rest.push_back(c);
  }
  out = std::move(fresh);
  return {};
}

}  // namespace t41
