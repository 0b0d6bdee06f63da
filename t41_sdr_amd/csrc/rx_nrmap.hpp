// t41_sdr_amd/csrc/rx_nrmap.hpp -- the noise-reduction map's lists (t41rx_set_nr_map; rx_nrmap.cpp): from the caller's
// nrOptionSelect and ANR_notchOn per channel and the optional stage map, what the two launches of a call read.  Plain
// C++: no HIP, no context type, so that a CPU program can walk it (tests/nr_map_check.cpp), as tests/stage_map_check.cpp
// walks rx_stagemap.hpp.
//
// The rule the lists serve: channel c is processed as the same channel of a context whose nrOptionSelect is
// nr_of_channel[c] and whose ANR_notchOn is notch_of_channel[c].  A function runs on channel c when its map entry asks for
// it and either no stage map is loaded or the channel's T41RX_STAGE_NR bit is set; a channel nobody asks anything for is
// in no list and is not touched.
//  * The spectral list: the channels with kind 1 (Kim1_NR()) or 2 (SpectralNoiseReduction()), ascending, and their kinds;
//    nrspec_map_kernel runs one workgroup per entry.
//  * The Xanr() list: the channels with kind 3 or the notch, sorted into the three classes anr_map_kernel distinguishes
//    -- LMS only, notch only, LMS then notch -- ascending within a class.  A workgroup of the kernel serves up to kAnrCw
//    = 16 columns and runs ONE class (the two passes are wave-uniform branches around a sample-serial chain), so every
//    class starts on a multiple of 16 in the list and a table of workgroups goes with it: {offset into the list, live
//    columns 1 .. 16, class}.  The padding behind a class repeats its last channel; no row reaches it.
// A channel with (1, 1) or (2, 1) is in both lists: the spectral launch runs first, the Xanr() launch behind it.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "rx_stagemap.hpp"

namespace t41 {

constexpr int kNrMapCols = 16;  // columns of a workgroup of anr_map_kernel (nr_kernels.hip: kAnrCw)

// the classes of the Xanr() list, in the list's order
enum NrMapClass : int32_t { kNrClassLms = 0, kNrClassNotch = 1, kNrClassBoth = 2, kNrClasses = 3 };

// a workgroup of anr_map_kernel: list[offset .. offset + live) are its channels (the kernel reads the row as one int4)
struct NrMapRow {
  int32_t offset, live, cls, pad;
};

struct NrMapLists {
  std::vector<int32_t> spec;       // channels with kind 1 or 2 that run, ascending
  std::vector<int32_t> spec_kind;  // [spec.size()]: 1 or 2
  std::vector<int32_t> anr;        // the Xanr() list, class by class, each class from a multiple of kNrMapCols
  std::vector<NrMapRow> rows;      // the workgroups over `anr`
  bool any = false;                // some entry of the map is non-zero, whatever the stage map says: "noise reduction on"
  bool spectral = false;           // some entry asks for kind 2, whatever the stage map says (the pass band's check)
};

// why a map is refused
enum class NrMapFault : int {
  none = 0,
  count,     // n != n_channels (or no channels at all)
  null_map,  // one of the two arrays missing
  kind,      // nr_of_channel[channel] outside 0 .. 3
  notch,     // notch_of_channel[channel] outside 0 .. 1
};
struct NrMapVerdict {
  NrMapFault fault = NrMapFault::none;
  int channel = -1;
  explicit operator bool() const { return fault == NrMapFault::none; }
};

// the class of a channel's two entries in the Xanr() list, or -1: Xanr() does not run
constexpr int nr_map_class(int32_t kind, int32_t notch) { return kind == 3 ? (notch ? kNrClassBoth : kNrClassLms) : (notch ? kNrClassNotch : -1); }

// Checks the map (every entry, before anything is built) and fills `out`; a refused map leaves `out` as it was.
// stages_of_channel: the stage map's [n_channels] masks (validated by its own setter), or null without one.
inline NrMapVerdict build_nr_map_lists(const int32_t *nr_of_channel, const int32_t *notch_of_channel, int n, int n_channels,
                                       const uint32_t *stages_of_channel, NrMapLists &out) {
  if (n_channels <= 0 || n != n_channels) return {NrMapFault::count, -1};
  if (!nr_of_channel || !notch_of_channel) return {NrMapFault::null_map, -1};
  for (int c = 0; c < n; ++c) {
    if (nr_of_channel[c] < 0 || nr_of_channel[c] > 3) return {NrMapFault::kind, c};
    if (notch_of_channel[c] < 0 || notch_of_channel[c] > 1) return {NrMapFault::notch, c};
  }
  NrMapLists fresh;
  std::vector<int32_t> of_class[kNrClasses];
  for (int c = 0; c < n; ++c) {
    const int32_t kind = nr_of_channel[c], notch = notch_of_channel[c];
    fresh.any = fresh.any || kind != 0 || notch != 0;
    fresh.spectral = fresh.spectral || kind == 2;
    if (stages_of_channel && !(stages_of_channel[c] & stage_bit(kStageNr))) continue;
    if (kind == 1 || kind == 2) {
      fresh.spec.push_back(c);
      fresh.spec_kind.push_back(kind);
    }
    const int cls = nr_map_class(kind, notch);
    if (cls >= 0) of_class[cls].push_back(c);
  }
  for (int cls = 0; cls < kNrClasses; ++cls) {
    const std::vector<int32_t> &l = of_class[cls];
    for (size_t i = 0; i < l.size(); i += (size_t)kNrMapCols) {
      const size_t live = l.size() - i < (size_t)kNrMapCols ? l.size() - i : (size_t)kNrMapCols;
      fresh.rows.push_back(NrMapRow{(int32_t)fresh.anr.size(), (int32_t)live, cls, 0});
      for (size_t k = 0; k < (size_t)kNrMapCols; ++k) fresh.anr.push_back(l[i + (k < live ? k : live - 1)]);
    }
  }
  out = std::move(fresh);
  return {};
}

// what the device copy of the lists holds at most, in int32 words: the spectral list and its kinds (n_channels each), the
// Xanr() list (every class padded to a multiple of kNrMapCols) and the rows (four words each, on a 16-byte boundary)
struct NrMapLayout {
  size_t spec, spec_kind, anr, rows, words;
};
inline NrMapLayout nr_map_layout(int n_channels) {
  const size_t n = (size_t)n_channels, max_rows = (n + kNrMapCols - 1) / kNrMapCols + kNrClasses;
  NrMapLayout l{};
  l.spec = 0;
  l.spec_kind = n;
  l.anr = 2 * n;
  l.rows = (l.anr + max_rows * kNrMapCols + 3) / 4 * 4;
  l.words = l.rows + 4 * max_rows;
  return l;
}

}  // namespace t41
