// t41_sdr_amd/csrc/ft8_kernel.hip -- FT8 receive up to the finished waterfall: the audio collector of DEMOD_FT8
// (Process.cpp:627-686), process_FT8_FFT() / extract_power() (ft8.cpp:223-268) and update_synchronization()
// (ft8.cpp:154-166), per channel, frame after frame.  Included by rx_host.cpp (the library's object set stays what it was).
//
// Integer arithmetic throughout: tests/ft8_model.py is the same operations in numpy, and the kernel equals it bit for bit.
//   collector  arm_float_to_q15 of the 69 samples the frame uses, then the 68-iteration loop in its closed parallel form:
//              every read is of the buffer as the frame found it, except that from iteration `leftover` on the middle
//              third takes what iteration i - leftover has just written (the firmware's same-frame forwarding).
//   block      when DSP_Flag == 1 and ft8_flag == 1, for time_sub 0 and 512: (q15_t)((float)buf[i] * window[i]),
//              arm_rfft_q15 as the Cortex-M7 build computes it -- 1024 complex q15 points in LDS, five radix-4 stages of
//              arm_radix4_butterfly_q15 with their saturating and halving adds, the bit reversal folded into the last
//              stage's stores, arm_split_rfft_q15 on bins 0 .. 736 only -- arm_shift_q15 by 5, the squared magnitude
//              >> 17, mag_db[] by that value, and the four rows of 368 bytes.
//   timing     ft8_flag, FT_8_counter, the half of the power buffer being written, update_synchronization() in uint32.
// One workgroup (or, for the probe, one wave) per channel stays resident for the whole call; the channel's buffer lives
// in LDS from the first frame to the last.
//
// LDS layout of the transform.  A point is one dword (re in the low half).  The stages read and write with ds_read_b32 /
// ds_write_b32, whose banks are dword % 32 per 32-lane half.  Stage strides 256 and 64 are conflict-free as they stand;
// strides 16 and 4 put a half-wave on 16 and 8 banks.  The buffer is therefore indexed through
//   sw(i) = i ^ (bits 5..6 of i) << 2 ^ (bit 6 of i) << 4,
// an XOR of low bits with higher ones (a bijection that keeps aligned groups of 4 together): at stride 16 the two
// groups of a half-wave differ in bit 6 and land on the two halves of the banks, at stride 4 the eight groups differ in
// bits 4..6 and land on eight different quads.  The last stage reads its four neighbours as one 16-byte word and scatters
// them to their bit-reversed places in a second buffer indexed through sw2(k) = k ^ (k >> 5 & 31): consecutive lanes
// differ in the high bits of the reversed index, which sw2 folds into the bank; the split stage then reads it linearly.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ft8_kernels.hpp"

namespace t41 {

namespace ft8 {
struct Cq {
  int r, i;
};
__device__ __forceinline__ int sat16(int x) { return min(max(x, -32768), 32767); }
__device__ __forceinline__ int sw(int i) { return i ^ (((i >> 5) & 3) << 2) ^ (((i >> 6) & 1) << 4); }
__device__ __forceinline__ int sw2(int k) { return k ^ ((k >> 5) & 31); }
__device__ __forceinline__ Cq unpack(unsigned v) { return Cq{(int)(short)(v & 0xffffu), (int)v >> 16}; }
__device__ __forceinline__ unsigned pack(Cq c) { return ((unsigned)c.r & 0xffffu) | ((unsigned)c.i << 16); }
__device__ __forceinline__ Cq shr(Cq a, int n) { return Cq{a.r >> n, a.i >> n}; }
__device__ __forceinline__ Cq qadd(Cq a, Cq b) { return Cq{sat16(a.r + b.r), sat16(a.i + b.i)}; }
__device__ __forceinline__ Cq qsub(Cq a, Cq b) { return Cq{sat16(a.r - b.r), sat16(a.i - b.i)}; }
__device__ __forceinline__ Cq hadd(Cq a, Cq b) { return Cq{(a.r + b.r) >> 1, (a.i + b.i) >> 1}; }
__device__ __forceinline__ Cq hsub(Cq a, Cq b) { return Cq{(a.r - b.r) >> 1, (a.i - b.i) >> 1}; }
// x * conj(W): re = __SMUAD(C, x) >> 16, im = the upper half of __SMUSDX(C, x); 32-bit sums that wrap
__device__ __forceinline__ Cq twmul(unsigned w, Cq x) {
  const int c = (int)(short)(w & 0xffffu), s = (int)w >> 16;
  return Cq{(int)((unsigned)(c * x.r) + (unsigned)(s * x.i)) >> 16, (int)((unsigned)(c * x.i) - (unsigned)(s * x.r)) >> 16};
}
// arm_float_to_q15 without ARM_MATH_ROUNDING: (q15_t)__SSAT((q31_t)(x * 32768.0f), 16), toward zero
__device__ __forceinline__ int to_q15(float x) { return sat16((int)(x * 32768.0f)); }
}  // namespace ft8

template <int NT>
__global__ __launch_bounds__(NT) void ft8_kernel(Ft8Args a) {
#pragma clang fp contract(off)
  using namespace ft8;
  __shared__ short sbuf[kFt8BufWords];
  __shared__ __attribute__((aligned(16))) unsigned fz[1024];
  __shared__ unsigned nat[1024];
  __shared__ unsigned tw[768];
  __shared__ unsigned short mg[kFt8Bins + 3];
  __shared__ short qs[68];
  constexpr int kIt = (68 + NT - 1) / NT;  // collector iterations per thread
  const int ch = blockIdx.x, t = threadIdx.x;
  int32_t *w = a.state + (size_t)ch * kFt8Words;
  auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };  // the scalars are the same in every lane
  unsigned n = (unsigned)uni(w[kFt8N]);
  int sync = uni(w[kFt8Sync]), flag = uni(w[kFt8Flag]), dsp = uni(w[kFt8DspFlag]), counter = uni(w[kFt8Counter]);
  int dataLoop = uni(w[kFt8DataLoop]), leftover = uni(w[kFt8Leftover]), half = uni(w[kFt8Half]);
  const unsigned start = (unsigned)uni(w[kFt8Start]);
  for (int i = t; i < kFt8BufWords; i += NT) sbuf[i] = (short)w[kFt8Scalars + i];
  for (int i = t; i < 768; i += NT) tw[i] = a.tab[kFt8TabTw + i];
  __syncthreads();

  for (int f = 0; f < a.nframes; ++f) {
    const float *x = a.aud + ((size_t)ch * a.nframes + f) * 256;
    int done = 0;
    if (sync) {
      // ---- collector (Process.cpp:633-662)
      const int base = 68 * dataLoop;
      short q[kIt], r1[kIt], r2[kIt];
#pragma unroll
      for (int u = 0; u < kIt; ++u) {
        const int i = t + NT * u;
        if (i < 68) {
          q[u] = (short)to_q15(x[(i * 15) >> 2]);
          r1[u] = sbuf[1024 + base + i];
          r2[u] = sbuf[2048 + base + i];
          qs[i] = q[u];
        }
      }
      const short q255 = (short)to_q15(x[255]);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kIt; ++u) {
        const int i = t + NT * u;
        if (i < 68) {
          sbuf[base + i] = r1[u];
          sbuf[1024 + base + i] = (leftover >= 1 && i >= leftover) ? qs[i - leftover] : r2[u];
          // (a record with leftover ahead of dataLoop / 4 would run past the buffer's end: such a write is dropped)
          if (2048 + base + i + leftover < kFt8BufWords) sbuf[2048 + base + i + leftover] = q[u];
        }
      }
      ++dataLoop;
      if (dataLoop == 15) {
        if (t == 0) sbuf[kFt8BufWords - 1] = q255;  // fill last cell
        dataLoop = 0;
        leftover = 0;
        dsp = 1;
      } else if (dataLoop == 4 || dataLoop == 8 || dataLoop == 12) {
        if (t == 0 && 2048 + dataLoop * 68 + leftover < kFt8BufWords) sbuf[2048 + dataLoop * 68 + leftover] = q255;
        ++leftover;
      }
      __syncthreads();
    }
    if (dsp == 1 && flag == 1) {
      // ---- process_FT8_FFT() (ft8.cpp:259-268): extract_power(offset_step * FT_8_counter)
      uint8_t *row = a.power + ((size_t)ch * 2 + (size_t)half) * kFt8HalfBytes + (size_t)kFt8BlockBytes * (size_t)counter;
      for (int ts = 0; ts < 2; ++ts) {
        // window_ft8_dsp_buffer[i] = (q15_t)((float)ft8_dsp_buffer[i + time_sub] * window[i]); point p = samples 2p, 2p + 1
        for (int p = t; p < 1024; p += NT) {
          const float2 wv = reinterpret_cast<const float2 *>(a.window)[p];
          const int re = (int)((float)sbuf[2 * p + 512 * ts] * wv.x), im = (int)((float)sbuf[2 * p + 1 + 512 * ts] * wv.y);
          fz[sw(p)] = pack(Cq{re, im});
        }
        __syncthreads();
        // first stage: inputs >> 2; outputs b and c stored swapped, here and in every stage (arm_radix4_butterfly_q15)
        for (int j = t; j < 256; j += NT) {
          const Cq A = shr(unpack(fz[sw(j)]), 2), B = shr(unpack(fz[sw(j + 256)]), 2);
          const Cq C = shr(unpack(fz[sw(j + 512)]), 2), D = shr(unpack(fz[sw(j + 768)]), 2);
          const Cq R = qadd(A, C), S = qsub(A, C), T = qadd(B, D), U = qsub(B, D);
          fz[sw(j)] = pack(hadd(R, T));
          fz[sw(j + 256)] = pack(twmul(tw[2 * j], qsub(R, T)));
          fz[sw(j + 512)] = pack(twmul(tw[j], Cq{sat16(S.r + U.i), sat16(S.i - U.r)}));      // __QSAX
          fz[sw(j + 768)] = pack(twmul(tw[3 * j], Cq{sat16(S.r - U.i), sat16(S.i + U.r)}));  // __QASX
        }
        __syncthreads();
        // middle stages: n2 = 64, 16, 4; twiddle step 4, 16, 64
#pragma unroll
        for (int lg = 6; lg >= 2; lg -= 2) {
          const int n2 = 1 << lg, mod = 256 >> lg;
          for (int b = t; b < 256; b += NT) {
            const int jj = b & (n2 - 1), i0 = ((b >> lg) << (lg + 2)) + jj, ic = jj * mod;
            const Cq A = unpack(fz[sw(i0)]), B = unpack(fz[sw(i0 + n2)]), C = unpack(fz[sw(i0 + 2 * n2)]), D = unpack(fz[sw(i0 + 3 * n2)]);
            const Cq R = qadd(A, C), S = qsub(A, C), T = qadd(B, D), U = qsub(B, D);
            fz[sw(i0)] = pack(shr(hadd(R, T), 1));
            fz[sw(i0 + n2)] = pack(twmul(tw[2 * ic], hsub(R, T)));
            fz[sw(i0 + 2 * n2)] = pack(twmul(tw[ic], Cq{(S.r + U.i) >> 1, (S.i - U.r) >> 1}));      // __SHSAX
            fz[sw(i0 + 3 * n2)] = pack(twmul(tw[3 * ic], Cq{(S.r - U.i) >> 1, (S.i + U.r) >> 1}));  // __SHASX
          }
          __syncthreads();
        }
        // last stage: four neighbours, one halving; arm_bitreversal_16 folded into the stores
        for (int g = t; g < 256; g += NT) {
          const uint4 v = *reinterpret_cast<const uint4 *>(&fz[sw(4 * g)]);
          const Cq A = unpack(v.x), B = unpack(v.y), C = unpack(v.z), D = unpack(v.w);
          const Cq R = qadd(A, C), S = qsub(A, C), T = qadd(B, D), U = qsub(B, D);
          const int k0 = (int)(__brev((unsigned)(4 * g)) >> 22);  // reversed 10-bit index; + 512, 256, 768 for 4 g + 1, 2, 3
          nat[sw2(k0)] = pack(hadd(R, T));
          nat[sw2(k0 + 512)] = pack(hsub(R, T));
          nat[sw2(k0 + 256)] = pack(Cq{(S.r + U.i) >> 1, (S.i - U.r) >> 1});
          nat[sw2(k0 + 768)] = pack(Cq{(S.r - U.i) >> 1, (S.i + U.r) >> 1});
        }
        __syncthreads();
        // arm_split_rfft_q15 on bins 0 .. 736, arm_shift_q15 by 5, arm_cmplx_mag_squared_q15
        for (int k = t; k < kFt8Bins; k += NT) {
          int re, im;
          const Cq P = unpack(nat[sw2(k)]);
          if (k == 0) {
            re = (P.r + P.i) >> 1;
            im = 0;
          } else {
            const Cq Q = unpack(nat[sw2(1024 - k)]), Ac = unpack(a.tab[kFt8TabA + k]), Bc = unpack(a.tab[kFt8TabB + k]);
            const unsigned outR = (unsigned)(P.r * Ac.r) - (unsigned)(P.i * Ac.i) + (unsigned)(Q.r * Bc.r) + (unsigned)(Q.i * Bc.i);
            const unsigned outI = (unsigned)(Q.r * Bc.i) - (unsigned)(Q.i * Bc.r) + (unsigned)(P.r * Ac.i) + (unsigned)(P.i * Ac.r);
            re = (int)(short)((int)outR >> 16);
            im = (int)(short)((int)outI >> 16);
          }
          re = sat16(re * 32);
          im = sat16(im * 32);
          mg[k] = (unsigned short)(((unsigned)(re * re) + (unsigned)(im * im)) >> 17);  // 0 .. 16384 (the sum in more than 31 bits)
        }
        __syncthreads();
        // the two rows of this time offset: freq_sub 0 / 1, 368 bytes each (ft8.cpp:244-254)
        for (int e = t; e < 2 * kFt8Row; e += NT) {
          const int fs = e >= kFt8Row ? 1 : 0, j = e - kFt8Row * fs;
          const float db = (a.mag_db[mg[2 * j + fs]] + a.mag_db[mg[2 * j + fs + 1]]) / 2;
          const int scaled = (int)db;  // toward zero, saturating, NaN -> 0
          row[2 * kFt8Row * ts + e] = (uint8_t)(scaled < 0 ? 0 : (scaled > 255 ? 255 : scaled));
        }
        __syncthreads();
      }
      ++counter;
      if (counter == kFt8SlotBlocks) {
        flag = 0;  // (ft8_decode_flag = 1: the decode belongs to the caller; this frame reports the finished half)
        done = 1 + half;
        half ^= 1;
      }
      dsp = 0;
    }
    if (flag == 0 && sync) {
      // update_synchronization() (ft8.cpp:154-166)
      const unsigned now = (unsigned)a.t0 + (unsigned)(((unsigned long long)n * (unsigned)a.num) / (unsigned)a.den);
      if ((now - start) % 15000u <= 200u) {
        flag = 1;
        counter = 0;
      }
    }
    ++n;
    if (t == 0) *reinterpret_cast<int4 *>(a.status + ((size_t)ch * a.nframes + f) * 4) = make_int4(counter, flag, done, dataLoop);
  }
  __syncthreads();
  for (int i = t; i < kFt8BufWords; i += NT) w[kFt8Scalars + i] = (int)sbuf[i];
  if (t == 0) {
    w[kFt8N] = (int)n;
    w[kFt8Sync] = sync;
    w[kFt8Flag] = flag;
    w[kFt8DspFlag] = dsp;
    w[kFt8Counter] = counter;
    w[kFt8DataLoop] = dataLoop;
    w[kFt8Leftover] = leftover;
    w[kFt8Half] = half;
  }
}

// auto_sync_FT8()'s success branch (ft8.cpp:133-136), one lane per channel
__global__ __launch_bounds__(64) void ft8_sync_kernel(int32_t *state, const uint8_t *mask, int nchan, int32_t t0, int32_t num, int32_t den) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= nchan || (mask && !mask[ch])) return;
  int32_t *w = state + (size_t)ch * kFt8Words;
  const unsigned n = (unsigned)w[kFt8N];
  w[kFt8Start] = (int)((unsigned)t0 + (unsigned)(((unsigned long long)n * (unsigned)num) / (unsigned)den));
  w[kFt8Flag] = 1;
  w[kFt8Counter] = 0;
  w[kFt8Sync] = 1;
}

void ft8_make_fft_tables(uint32_t *tab) {
  // round(x * 2^15), half away from zero, saturated (CMSIS-DSP's table generators); in double
  auto q15 = [](double x) {
    const double r = x >= 0.0 ? std::floor(x * 32768.0 + 0.5) : std::ceil(x * 32768.0 - 0.5);
    return (int)(r < -32768.0 ? -32768.0 : (r > 32767.0 ? 32767.0 : r));
  };
  auto pair = [](int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); };
  const double two_pi = 6.283185307179586476925286766559;
  for (int k = 0; k < 768; ++k) tab[kFt8TabTw + k] = pair(q15(std::cos(two_pi * k / 1024)), q15(std::sin(two_pi * k / 1024)));
  for (int k = 0; k < kFt8Bins; ++k) {
    const double s = std::sin(two_pi * k / 2048), c = std::cos(two_pi * k / 2048);
    tab[kFt8TabA + k] = pair(q15(0.5 * (1.0 - s)), q15(-0.5 * c));
    tab[kFt8TabB + k] = pair(q15(0.5 * (1.0 + s)), q15(0.5 * c));
  }
}

hipError_t launch_ft8(const Ft8Args &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || !a.aud || !a.state || !a.power || !a.status || !a.window || !a.mag_db || !a.tab || a.num < 0 || a.den <= 0)
    return hipErrorInvalidConfiguration;
  if (a.threads == 64)
    hipLaunchKernelGGL(ft8_kernel<64>, dim3((unsigned)a.nchan), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(ft8_kernel<256>, dim3((unsigned)a.nchan), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ft8_sync(int32_t *state, const uint8_t *mask, int nchan, int32_t t0, int32_t num, int32_t den, hipStream_t s) {
  if (nchan <= 0 || !state || num < 0 || den <= 0) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(ft8_sync_kernel, dim3((unsigned)((nchan + 63) / 64)), dim3(64), 0, s, state, mask, nchan, t0, num, den);
  return hipGetLastError();
}

}  // namespace t41
