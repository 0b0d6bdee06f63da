// t41_sdr_amd/csrc/ft8_decode_kernel.hip -- FT8 decode of a finished slot: find_sync() (ft8.cpp:337-420),
// extract_likelihood() (:424-462), bp_decode() (:518-594), pack_bits() (:598-616), crc() (:672-703) and the loop of
// ft8_decode() up to the CRC check (:759-783), per channel.  A translation unit of its own (ft8_decode_kernel.o); host side:
// rx_ft8_decode.cpp.  tests/ft8_decode_model.py is the same operations in numpy, and the kernels equal it byte for byte.
//
//   ft8_sync_kernel  one workgroup per channel.  Per alt (time_sub, freq_sub) the alt's 92 rows of 368 bytes are staged in
//                    LDS (they lie 1472 bytes apart in the waterfall), the 27 x 312 scores are computed in parallel into LDS
//                    as int16 -- integer sums, a symbol's eight bins cut out of three aligned dwords, C's division toward
//                    zero -- and wave 0 replays the firmware's min-heap over them in the firmware's order.  The heap's 20
//                    entries live one per lane (score; alt * 8424 + index); heapify_down / heapify_up move
//                    them with lane shuffles, every decision uniform across the wave.  The replay itself is serial, but an
//                    entry below min_score never acts, and while the heap is full neither does one with score <=
//                    heap[0].score (no eviction, no room): the wave ballots over 64 entries at a time for the next one
//                    that acts.  The heap ARRAY goes out in array order, as ft8_decode() walks it.
//   ft8_ldpc_kernel  one wave per (channel, candidate).  Lane k < 58 reads data symbol k's eight bins through kGray_map
//                    and owns bits 3k .. 3k + 2; log174 are exact integers, their sum and sum of squares stay below 2^24 and
//                    are reduced across the wave as integers; variance and norm_factor in f32, one rounding per operation.
//                    bp_decode() with log174, tov[174][3], toc[83][7] and plain in LDS: the 581 check entries and the 522
//                    bit-check pairs strided over the lanes, ldpc_check() by ballot and popcount, a uniform exit; then
//                    pack_bits(), the CRC-14 and the record.  NaN (a variance of 0 or below) is carried as IEEE does.
// f32 throughout in source order: no contraction, IEEE division and square root, denormals kept.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ft8_decode_kernels.hpp"

namespace t41 {

namespace ft8dec {

constexpr int kSyncThreads = 256;

// ---- find_sync ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSyncThreads) void ft8_sync_kernel(Ft8DecodeArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t rows[kFt8SlotBlocks * kFt8Row];
  __shared__ short sc[kFt8ScoresPerAlt];
  const int ch = blockIdx.x, t = threadIdx.x;
  t41rx_ft8_result *res = a.results + ch;
  const int sel = a.select ? (int)a.select[ch] : 0;
  // the record starts out zero (unused candidates stay so) with `select` in place
  for (int i = t; i < (int)(sizeof(t41rx_ft8_result) / 4); i += kSyncThreads) reinterpret_cast<int32_t *>(res)[i] = i == 2 ? sel : 0;
  if (sel < 0) return;
  const uint8_t *wf = a.waterfall + (size_t)ch * a.stride + (size_t)sel * kFt8HalfBytes;
  const int ncand = a.max_candidates, min_score = a.min_score;
  int costas[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) costas[k] = a.tab->costas[k];
  int hs = 0, hscore = 0, hpay = 0;  // the heap: its size, and entry `lane` of wave 0 (score; alt * 8424 + index)

  for (int alt = 0; alt < 4; ++alt) {
    __syncthreads();
    constexpr int kRowWords = kFt8Row / 4;
    for (int i = t; i < kFt8SlotBlocks * kRowWords; i += kSyncThreads) {
      const int r = i / kRowWords, d = i - r * kRowWords;
      reinterpret_cast<uint32_t *>(rows)[i] = reinterpret_cast<const uint32_t *>(wf + (size_t)r * kFt8BlockBytes + alt * kFt8Row)[d];
    }
    __syncthreads();
    for (int idx = t; idx < kFt8ScoresPerAlt; idx += kSyncThreads) {
      const int ti = idx / kFt8FreqOffsets, f = idx - ti * kFt8FreqOffsets + kFt8MinBin, time_offset = ti - 7;
      int score = 0, num_symbols = 0;
#pragma unroll
      for (int m = 0; m <= 72; m += 36) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          const int r = time_offset + k + m;
          if (r < 0 || r >= kFt8SlotBlocks) continue;
          // p8[0..7] = the row's bytes f .. f + 7 as one 64-bit word, cut out of three aligned dwords (f + 7 <= 366: the
          // third one lies inside the row); their sum by two byte-wise sums of absolute differences against 0
          const uint32_t *rw = reinterpret_cast<const uint32_t *>(rows + r * kFt8Row) + (f >> 2);
          const uint32_t w0 = rw[0], w1 = rw[1], w2 = rw[2];
          const int sh = 8 * (f & 3);
          const uint32_t lo = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), hi = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
          const int sum8 = (int)__builtin_amdgcn_sad_u8(hi, 0u, __builtin_amdgcn_sad_u8(lo, 0u, 0u));
          const int hit = (int)(((((uint64_t)hi << 32) | lo) >> (8 * costas[k])) & 0xffu);
          score += 8 * hit - sum8;
          ++num_symbols;
        }
      }
      sc[idx] = (short)(score / num_symbols);  // toward zero; |score / num_symbols| <= 1785
    }
    __syncthreads();
    if (t < 64) {
      const int lane = t;
      for (int base = 0; base < kFt8ScoresPerAlt; base += 64) {
        const int i = base + lane;
        const int s = i < kFt8ScoresPerAlt ? (int)sc[i] : 0;
        const bool q = i < kFt8ScoresPerAlt && s >= min_score;
        unsigned long long pend = __ballot(q);
        while (pend) {
          int l;
          if (hs == ncand) {
            const int h0 = __shfl(hscore, 0);
            const unsigned long long act = __ballot(q && s > h0) & pend;
            if (!act) break;
            l = __ffsll(act) - 1;
            // heap[0] = heap[heap_size - 1]; --heap_size; heapify_down()
            const int ls = __shfl(hscore, hs - 1), lp = __shfl(hpay, hs - 1);
            if (lane == 0) {
              hscore = ls;
              hpay = lp;
            }
            --hs;
            int cur = 0;
            while (true) {
              int largest = cur, best = __shfl(hscore, cur);
              const int left = 2 * cur + 1, right = left + 1;
              if (left < hs) {
                const int v = __shfl(hscore, left);
                if (v < best) {
                  largest = left;
                  best = v;
                }
              }
              if (right < hs) {
                const int v = __shfl(hscore, right);
                if (v < best) {
                  largest = right;
                  best = v;
                }
              }
              if (largest == cur) break;
              const int cs = __shfl(hscore, cur), cp = __shfl(hpay, cur), bp = __shfl(hpay, largest);
              if (lane == cur) {
                hscore = best;
                hpay = bp;
              } else if (lane == largest) {
                hscore = cs;
                hpay = cp;
              }
              cur = largest;
            }
          } else {
            l = __ffsll(pend) - 1;
          }
          pend = l == 63 ? 0ull : (pend & (~0ull << (l + 1)));
          // heap[heap_size] = the entry; ++heap_size; heapify_up()
          const int es = __shfl(s, l);
          if (lane == hs) {
            hscore = es;
            hpay = alt * kFt8ScoresPerAlt + base + l;
          }
          ++hs;
          int cur = hs - 1;
          while (cur > 0) {
            const int parent = (cur - 1) / 2;
            const int cs = __shfl(hscore, cur), ps = __shfl(hscore, parent);
            if (cs >= ps) break;
            const int cp = __shfl(hpay, cur), pp = __shfl(hpay, parent);
            if (lane == cur) {
              hscore = ps;
              hpay = pp;
            } else if (lane == parent) {
              hscore = cs;
              hpay = cp;
            }
            cur = parent;
          }
        }
      }
    }
  }
  if (t < 64) {
    if (t < hs) {
      const int alt = hpay / kFt8ScoresPerAlt, idx = hpay - alt * kFt8ScoresPerAlt, ti = idx / kFt8FreqOffsets;
      t41rx_ft8_candidate *c = &res->cand[t];
      c->score = (int16_t)hscore;
      c->time_offset = (int16_t)(ti - 7);
      c->freq_offset = (int16_t)(idx - ti * kFt8FreqOffsets + kFt8MinBin);
      c->time_sub = (uint8_t)(alt / 2);
      c->freq_sub = (uint8_t)(alt % 2);
    }
    if (t == 0) res->num_candidates = hs;
  }
}

// ---- extract_likelihood, bp_decode, pack_bits, crc --------------------------------------------------------------------------
__device__ __forceinline__ int max4i(int a, int b, int c, int d) { return max(max(a, b), max(c, d)); }

__device__ __forceinline__ float fast_tanh(float x) {
#pragma clang fp contract(off)
  if (x < -4.97f) return -1.0f;
  if (x > 4.97f) return 1.0f;
  const float x2 = x * x;
  const float a = x * (945.0f + x2 * (105.0f + x2));
  const float b = 945.0f + x2 * (420.0f + x2 * 15.0f);
  return a / b;
}

__device__ __forceinline__ float fast_atanh(float x) {
#pragma clang fp contract(off)
  const float x2 = x * x;
  const float a = x * (945.0f + x2 * (-735.0f + x2 * 64.0f));
  const float b = (945.0f + x2 * (-1050.0f + x2 * 225.0f));
  return a / b;
}

__global__ __launch_bounds__(64) void ft8_ldpc_kernel(Ft8DecodeArgs a) {
#pragma clang fp contract(off)
  __shared__ float cw[kLdpcN], zn[kLdpcN], tov[kFt8BitChecks], toc[kFt8CheckEntries];
  __shared__ uint8_t plain[kLdpcN + 2], packed[12];
  __shared__ __attribute__((aligned(4))) Ft8DecodeTables tb;
  static_assert(sizeof(Ft8DecodeTables) % 4 == 0, "copied by words");
  const int ch = blockIdx.x / a.max_candidates, ci = blockIdx.x - ch * a.max_candidates, lane = threadIdx.x;
  t41rx_ft8_result *res = a.results + ch;
  if (ci >= res->num_candidates) return;  // (a skipped channel has none)
  for (int i = lane; i < (int)(sizeof(Ft8DecodeTables) / 4); i += 64)
    reinterpret_cast<uint32_t *>(&tb)[i] = reinterpret_cast<const uint32_t *>(a.tab)[i];
  t41rx_ft8_candidate *cand = &res->cand[ci];
  const int time_offset = cand->time_offset, freq_offset = cand->freq_offset, alt = 2 * cand->time_sub + cand->freq_sub;
  const uint8_t *wf = a.waterfall + (size_t)ch * a.stride + (size_t)res->select * kFt8HalfBytes;
  __syncthreads();

  // extract_likelihood(): lane k decodes data symbol k
  int l0 = 0, l1 = 0, l2 = 0;
  if (lane < kFt8ND) {
    const int sym_idx = (lane < kFt8ND / 2) ? (lane + 7) : (lane + 14);
    const uint8_t *ps = wf + (size_t)(time_offset + sym_idx) * kFt8BlockBytes + alt * kFt8Row + freq_offset;
    int s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s2[j] = ps[tb.gray[j]];
    l0 = max4i(s2[4], s2[5], s2[6], s2[7]) - max4i(s2[0], s2[1], s2[2], s2[3]);
    l1 = max4i(s2[2], s2[3], s2[6], s2[7]) - max4i(s2[0], s2[1], s2[4], s2[5]);
    l2 = max4i(s2[1], s2[3], s2[5], s2[7]) - max4i(s2[0], s2[2], s2[4], s2[6]);
  }
  int isum = l0 + l1 + l2, isum2 = l0 * l0 + l1 * l1 + l2 * l2;  // below 2^24: exact in f32 in any order
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    isum += __shfl_xor(isum, d);
    isum2 += __shfl_xor(isum2, d);
  }
  {
    const float sum = (float)isum, sum2 = (float)isum2;
    const float inv_n = 1.0f / kLdpcN;
    const float variance = (sum2 - sum * sum * inv_n) * inv_n;
    const float norm_factor = sqrtf(16.0f / variance);
    if (lane < kFt8ND) {
      cw[3 * lane + 0] = (float)l0 * norm_factor;
      cw[3 * lane + 1] = (float)l1 * norm_factor;
      cw[3 * lane + 2] = (float)l2 * norm_factor;
    }
  }
  for (int p = lane; p < kFt8BitChecks; p += 64) tov[p] = 0.0f;
  __syncthreads();

  // bp_decode()
  int min_errors = kLdpcM, iter = 0;
  for (; iter < a.iterations; ++iter) {
    if (lane < kFt8ND) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int i = 3 * lane + j;
        const float z = cw[i] + tov[3 * i + 0] + tov[3 * i + 1] + tov[3 * i + 2];
        zn[i] = z;
        plain[i] = (z > 0) ? 1 : 0;
      }
    }
    __syncthreads();
    int errors = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // ldpc_check(): checks lane and lane + 64
      const int c = lane + 64 * h;
      unsigned x = 0;
      if (c < kLdpcM)
        for (int k = 0; k < tb.nrw[c]; ++k) x ^= plain[tb.nm[c * 7 + k]];
      errors += __popcll(__ballot(x != 0));
    }
    if (errors < min_errors) {
      min_errors = errors;
      if (errors == 0) break;
    }
    for (int e = lane; e < kFt8CheckEntries; e += 64) {
      const int c = e / 7, k = e - 7 * c;
      if (k < tb.nrw[c]) {
        const int ibj = tb.nm[e];
        const float v = zn[ibj] - tov[3 * ibj + tb.kk[e]];
        toc[e] = fast_tanh(-v / 2);
      }
    }
    __syncthreads();
    for (int p = lane; p < kFt8BitChecks; p += 64) {
      const int ichk = tb.mn[p], skip = tb.pos[p];
      float Tmn = 1.0f;
      for (int k = 0; k < tb.nrw[ichk]; ++k)
        if (k != skip) Tmn *= toc[ichk * 7 + k];
      tov[p] = 2 * fast_atanh(-Tmn);
    }
    __syncthreads();
  }

  // pack_bits(plain, K), the CRC over the masked copy, the record
  if (lane < 12) {
    unsigned b = 0;
    for (int j = 0; j < 8; ++j) {
      const int i = 8 * lane + j;
      if (i < kLdpcK && plain[i]) b |= 0x80u >> j;
    }
    packed[lane] = (uint8_t)b;
  }
  __syncthreads();
  if (lane == 0) {
    int flags = 0;
    if (min_errors == 0) {
      const unsigned chksum = ((packed[9] & 0x07u) << 11) | ((unsigned)packed[10] << 3) | (packed[11] >> 5);
      unsigned remainder = 0;
      for (int idx_bit = 0; idx_bit < 96 - 14; ++idx_bit) {
        if (idx_bit % 8 == 0) {
          const int idx_byte = idx_bit / 8;
          const unsigned m = idx_byte < 9 ? packed[idx_byte] : (idx_byte == 9 ? (packed[9] & 0xF8u) : 0u);
          remainder ^= m << (kFt8CrcWidth - 8);
        }
        if (remainder & (1u << (kFt8CrcWidth - 1)))
          remainder = ((remainder << 1) ^ (unsigned)kFt8CrcPolynomial) & 0xFFFFu;
        else
          remainder = (remainder << 1) & 0xFFFFu;
      }
      flags = 1 | ((chksum == (remainder & ((1u << kFt8CrcWidth) - 1))) ? 2 : 0);
    }
    cand->n_errors = (int16_t)min_errors;
    cand->iterations = (uint8_t)iter;
    cand->flags = (uint8_t)flags;
    if (flags == 3) atomicAdd(&res->num_valid, 1);
  }
  if (lane < 12 && min_errors == 0) cand->a91[lane] = packed[lane];
  const size_t tap = ((size_t)ch * T41RX_FT8_MAX_CANDIDATES + ci) * kLdpcN;
  if (a.dbg_log174)
    for (int i = lane; i < kLdpcN; i += 64) a.dbg_log174[tap + i] = cw[i];
  if (a.dbg_plain)
    for (int i = lane; i < kLdpcN; i += 64) a.dbg_plain[tap + i] = plain[i];
}

}  // namespace ft8dec

hipError_t launch_ft8_decode(const Ft8DecodeArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || !a.waterfall || !a.tab || !a.results || a.max_candidates < 1 || a.max_candidates > T41RX_FT8_MAX_CANDIDATES ||
      a.iterations < 1 || (reinterpret_cast<uintptr_t>(a.waterfall) & 3u) || (a.stride & 3u))
    return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(ft8dec::ft8_sync_kernel, dim3((unsigned)a.nchan), dim3(ft8dec::kSyncThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ft8dec::ft8_ldpc_kernel, dim3((unsigned)a.nchan * (unsigned)a.max_candidates), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace t41
