// t41_sdr_amd/csrc/ft8_decode_kernels.hpp -- argument block and launcher of the FT8 decode of a finished slot
// (ft8_decode_kernel.hip): find_sync(), extract_likelihood(), bp_decode(), pack_bits(), crc() and the loop of ft8_decode() up
// to the CRC check (ft8.cpp:270-616, 669-703, 727-790).  Product code: nothing from oracle/.  kCostas_map, kGray_map, kNm,
// kMn and kNrw are the caller's (t41rx_set_ft8_decode_tables): the library holds no copy of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/t41rx.h"
#include "ft8_kernels.hpp"

namespace t41 {

constexpr int kFt8NN = 79, kFt8ND = 58;                    // NN, ND: channel symbols, data symbols
constexpr int kLdpcN = 174, kLdpcK = 91, kLdpcM = 83;      // N, K, M of the LDPC (174, 91) code
constexpr int kFt8MinBin = 48;                                                // ft8_min_bin
constexpr int kFt8TimeOffsets = kFt8SlotBlocks - kFt8NN + 7 + 7;              // time_offset -7 .. 19
constexpr int kFt8FreqOffsets = kFt8Row - 8 - kFt8MinBin;                     // freq_offset 48 .. 359
constexpr int kFt8ScoresPerAlt = kFt8TimeOffsets * kFt8FreqOffsets;           // 8424
constexpr int kFt8CheckEntries = kLdpcM * 7, kFt8BitChecks = kLdpcN * 3;        // 581, 522
constexpr int kFt8CrcPolynomial = 0x2757, kFt8CrcWidth = 14;                  // initalize_constants()
static_assert(kFt8HalfBytes == T41RX_FT8_SLOT_BYTES, "slot");
static_assert(kFt8TimeOffsets == 27 && kFt8FreqOffsets == 312, "find_sync's loops");

// the validated tables as the kernels read them, one byte each (device).  pos and kk are worked out once from kNm / kMn:
// pos[i][j] is the index of bit i inside check kMn[i][j], kk[c][k] the index of check c among the three of bit kNm[c][k]
struct Ft8DecodeTables {
  uint8_t costas[8];
  uint8_t gray[8];
  uint8_t nrw[kLdpcM + 1];
  uint8_t nm[kFt8CheckEntries + 3];   // kNm - 1 (unused entries 0)
  uint8_t kk[kFt8CheckEntries + 3];
  uint8_t mn[kFt8BitChecks + 2];      // kMn - 1
  uint8_t pos[kFt8BitChecks + 2];
};

struct Ft8DecodeArgs {
  const uint8_t *waterfall;     // channel c reads waterfall + c * stride + select[c] * kFt8HalfBytes (4-byte aligned)
  size_t stride;
  const int8_t *select;         // [nchan] (device) or null: all 0
  const Ft8DecodeTables *tab;   // (device)
  t41rx_ft8_result *results;    // [nchan]
  float *dbg_log174;            // [nchan][20][174] or null
  uint8_t *dbg_plain;           // [nchan][20][174] or null
  int nchan, max_candidates, min_score, iterations;
};
hipError_t launch_ft8_decode(const Ft8DecodeArgs &a, hipStream_t s);

}  // namespace t41
