// t41_sdr_amd/csrc/ft8_kernel.hip -- FT8 receive up to the finished waterfall: the audio collector of DEMOD_FT8
// (Process.cpp:627-686), process_FT8_FFT() / extract_power() (ft8.cpp:223-268) and update_synchronization()
// (ft8.cpp:154-166), per channel, frame after frame.  A translation unit of its own (ft8_kernel.o); host side: rx_ft8.cpp.
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
//
// The block's text is ft8_block.inc, compiled into the kernels that run it: ft8_kernel and ft8_audio_kernel (FT8 from
// 12 kS/s audio, below), each with its list form (t41rx_set_ft8_map: ft8_kernel.inc, ft8_audio_kernel.inc).  Two kernels from one text, not one body inlined into two: as a force-inlined device function it
// compiles ft8_kernel to another instruction stream (the swizzled indices simplified another way, two instructions more),
// and a template argument for the source would rename the live kernel (profiles/ft8_audio_isa_fingerprint.txt).
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

// ft8_kernel<256>, and its list form under an FT8 map (t41rx_set_ft8_map): the text is ft8_kernel.inc
#define T41_STAGE_KERNEL ft8_kernel
#define T41_STAGE_ARGS Ft8Args
#define T41_STAGE_LIST 0
#include "ft8_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL ft8_list_kernel
#define T41_STAGE_ARGS Ft8ListArgs
#define T41_STAGE_LIST 1
#include "ft8_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST

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

// ---- FT8 from 12 kS/s audio: the collector of DEMOD_FT8_WAV (Process.cpp:278-335), tests/ft8_audio_model.py bit for bit.
// Per frame of 128 samples the firmware rolls 68 cells k = i + 68 * dataLoop of each third of the buffer and writes
// q[(i * 15) >> 3] into the last; nothing gates a frame, and a cell is read only by the iteration that then writes it.  A
// thread therefore owns its cells -- c, c + 1024, c + 2048 -- and the collector needs no barrier; it takes up to a whole
// gulp (frames d0 <= d < d1 of the 15, cells 68 * d0 .. 68 * d1 - 1, four per thread) in one pass, with one barrier in
// front of the transform when d1 == 15.  Cells 1020..1023 of each third are never touched.  process_FT8_FFT() runs
// unconditionally (ft8_flag is not asked), the slot's end sets FT_8_counter = 0 (:325), and update_synchronization() is never
// called.  The status words have a closed form in the frame's number and are written behind the loop.
// A record with FT_8_counter at 92 (what the live stage leaves next to ft8_flag 0) would index past the half: such a block
// is dropped and the counter stays, until t41rx_ft8_audio_begin() / _end().
namespace ft8 {
__device__ __forceinline__ short audio_q15(short x) { return x; }  // (raw / 32768.0f through arm_float_to_q15 is the identity)
__device__ __forceinline__ short audio_q15(float x) { return (short)to_q15(x); }
}  // namespace ft8

// ft8_audio_kernel<short | float>, and its list form: the text is ft8_audio_kernel.inc
#define T41_STAGE_KERNEL ft8_audio_kernel
#define T41_STAGE_ARGS Ft8AudioArgs
#define T41_STAGE_LIST 0
#include "ft8_audio_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST
#define T41_STAGE_KERNEL ft8_audio_list_kernel
#define T41_STAGE_ARGS Ft8AudioListArgs
#define T41_STAGE_LIST 1
#include "ft8_audio_kernel.inc"
#undef T41_STAGE_KERNEL
#undef T41_STAGE_ARGS
#undef T41_STAGE_LIST

// setupFT8Wav()'s FT_8_counter = 0 (ft8.cpp:1372; end = 0) or the mode's exit (Process.cpp:339-342; end = 1), one lane per channel
__global__ __launch_bounds__(64) void ft8_audio_mark_kernel(int32_t *state, const uint8_t *mask, int nchan, int end) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= nchan || (mask && !mask[ch])) return;
  int32_t *w = state + (size_t)ch * kFt8Words;
  w[kFt8Counter] = 0;
  if (end) {
    w[kFt8Sync] = 0;
    w[kFt8Flag] = 0;
  }
}

hipError_t launch_ft8_audio(const Ft8AudioArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || a.nframes > kFt8MaxFrames || !a.pcm || !a.state || !a.power || !a.status || !a.window || !a.mag_db || !a.tab)
    return hipErrorInvalidConfiguration;
  if (a.q15)
    hipLaunchKernelGGL(ft8_audio_kernel<short>, dim3((unsigned)a.nchan), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(ft8_audio_kernel<float>, dim3((unsigned)a.nchan), dim3(256), 0, s, a);
  return hipGetLastError();
}

// the list form: a workgroup per pair (the setter checked the pairs: channel < nchan, row < the rows of power / status / pcm)
hipError_t launch_ft8_audio_list(const Ft8AudioListArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || a.nframes > kFt8MaxFrames || !a.pcm || !a.state || !a.power || !a.status || !a.window || !a.mag_db || !a.tab ||
      !a.list || a.nlist <= 0 || a.nlist > a.nchan)
    return hipErrorInvalidConfiguration;
  if (a.q15)
    hipLaunchKernelGGL(ft8_audio_list_kernel<short>, dim3((unsigned)a.nlist), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(ft8_audio_list_kernel<float>, dim3((unsigned)a.nlist), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ft8_audio_mark(int32_t *state, const uint8_t *mask, int nchan, int end, hipStream_t s) {
  if (nchan <= 0 || !state) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(ft8_audio_mark_kernel, dim3((unsigned)((nchan + 63) / 64)), dim3(64), 0, s, state, mask, nchan, end);
  return hipGetLastError();
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
  hipLaunchKernelGGL(ft8_kernel<256>, dim3((unsigned)a.nchan), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ft8_list(const Ft8ListArgs &a, hipStream_t s) {
  if (a.nchan <= 0 || a.nframes <= 0 || !a.aud || !a.state || !a.power || !a.status || !a.window || !a.mag_db || !a.tab || a.num < 0 || a.den <= 0 ||
      !a.list || a.nlist <= 0 || a.nlist > a.nchan)
    return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(ft8_list_kernel<256>, dim3((unsigned)a.nlist), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ft8_sync(int32_t *state, const uint8_t *mask, int nchan, int32_t t0, int32_t num, int32_t den, hipStream_t s) {
  if (nchan <= 0 || !state || num < 0 || den <= 0) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(ft8_sync_kernel, dim3((unsigned)((nchan + 63) / 64)), dim3(64), 0, s, state, mask, nchan, t0, num, den);
  return hipGetLastError();
}

}  // namespace t41
