// t41_sdr_amd/csrc/anr_kernel.inc -- the text of anr_kernel, included three times by nr_kernels.hip: T41_STAGE_KERNEL names the kernel,
// T41_STAGE_LIST 0 makes the kernel as it is without a stage map, 1 its list form (t41rx_set_stage_map), 2 the
// noise-reduction map's form (t41rx_set_nr_map): the list form whose workgroups take their segment of the list and their
// passes from the map's table.  Three kernels
// of one text, not one body shared by three kernels: an argument block handed on by reference compiles to another
// instruction stream, and the form without a map must stay the stream it was.
// What the forms differ in, as the text below names it: the argument block, and which passes the workgroup runs -- for
// forms 0 and 1 the launch's two switches, read where they are used, for form 2 the class of the workgroup's row.
#if T41_STAGE_LIST == 2
#define T41_ANR_ARGS NrMapArgs
#define T41_ANR_LMS (wg.z != 1)    // (rx_nrmap.hpp: the classes LMS only 0, notch only 1, LMS then notch 2)
#define T41_ANR_NOTCH (wg.z != 0)
#else
#define T41_ANR_ARGS NrArgs
#define T41_ANR_LMS (a.nr_option == 3)
#define T41_ANR_NOTCH (a.notch)
#endif
__global__ __launch_bounds__(128, 2) void T41_STAGE_KERNEL(const T41_ANR_ARGS a) {
  // (The copy / scale loops below are kept rolled: fully unrolled, with every address hoisted out of the frame loop, they
  // took the kernel to 353 VGPRs; 161 now.  Measured at the end of round 4, all bit-identical to this form
  // (tools/anr_ab_check.py) and none faster than 1 %: no workgroup barrier per sample -- sigma through two slots guarded
  // by LDS counters, wave 1 up to two samples ahead --, the next sample's window and this sample's sigma requested a
  // chain ahead of their use, both outcomes of the leak logic formed off the path and selected, the window read through
  // one lane-dependent base with immediate offsets (8 ds_read2_b32 instead of 16 address computations and 16 reads), the
  // first sample's "no pending update" as a compile-time case (16 selects per sample fewer): 187 -> 165 instructions per
  // sample, 138 us per frame either way.  Timing experiments: 16 instead of 64 additions per chain -25 us (4.5 cycles
  // per addition), no leak decision -5, no sigma wave -6.  A sample is ONE dependent sequence -- update, product, 64
  // additions, 5 lane swaps, error, two double-precision expressions, select, update -- on one wave; what it costs is that
  // sequence's latency, ~1000 cycles, and neither the instruction count nor the synchronisation.)
#pragma clang fp contract(off)
  constexpr bool LIST = T41_STAGE_LIST != 0;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *T = sm, *O = sm + kAnrTile * kAnrRow, *SIG = sm + kAnrSigOff;  // (16-byte aligned)
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // 0: filter output and update, 1: sum of squares
  const int c = lane & 15, g = lane >> 4, tb = anr_tap_base(g);
#if T41_STAGE_LIST == 2
  const int4 wg = a.rows[blockIdx.x];  // {offset into the list, live columns 1 .. 16, class}: uniform, one scalar load
  const int ch0 = wg.x;
  const int nlive = wg.y;
#else
  const int ch0 = blockIdx.x * kAnrCw;
  const int nserved = LIST ? a.nlist : a.nchan;
  const int nlive = (nserved - ch0 < kAnrCw) ? nserved - ch0 : kAnrCw;
#endif
  const int col = ch0 + (c < nlive ? c : nlive - 1);  // dead lanes shadow the last live channel (their stores are skipped)
  const int ch = LIST ? a.list[col] : col;            // (a list: the last LISTED channel of the workgroup)
  const size_t nch = (size_t)a.nchan;
  f2 w[8];  // ANR_w (wave 0): this lane's 16 taps, two per register pair: (.x, .y) = taps (tb + 2 t + 1, tb + 2 t)
  float lidx = 0, ngamma = 0;
  if (wv == 0) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
      w[t] = f2{a.anr[(size_t)(kAnrStW + tb + 2 * t + 1) * nch + ch], a.anr[(size_t)(kAnrStW + tb + 2 * t) * nch + ch]};
    _Pragma("unroll 4") for (int r = g; r < kAnrHist; r += 4) T[r * kAnrRow + c] = a.anr[(size_t)(kAnrStHist + r) * nch + ch];
    lidx = a.anr[(size_t)kAnrStLidx * nch + ch], ngamma = a.anr[(size_t)kAnrStNgamma * nch + ch];
  }
  for (int f = 0; f < a.nframes; ++f) {
    // stage the frame in: column cc of the tile = channel ch0 + cc, 256 consecutive samples, 4 x 256 B per channel (the
    // two waves take alternate channels)
    __syncthreads();
_Pragma("nounroll")
    for (int cc = wv; cc < nlive; cc += 2) {
      const float *src = a.aud + ((size_t)(LIST ? a.list[ch0 + cc] : ch0 + cc) * a.nframes + f) * 256;
#pragma unroll
      for (int q = 0; q < 4; ++q) T[(kAnrHist + lane + 64 * q) * kAnrRow + cc] = src[lane + 64 * q];
    }
_Pragma("nounroll")
    for (int cc = nlive + ((nlive ^ wv) & 1); cc < kAnrCw; cc += 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) T[(kAnrHist + lane + 64 * q) * kAnrRow + cc] = 0.0f;
    }
    __syncthreads();
    if (T41_ANR_LMS) {  // Process.cpp:852-857: Xanr() as noise reduction; its result stays in float_buffer_R, float_buffer_L is scaled by 1.5
      if (wv == 0) anr_pass_y<false>(T, nullptr, SIG, w, lidx, ngamma, lane);
      else anr_pass_sigma(T, SIG, lane);
      __syncthreads();
      if (wv == 0) {
        if (T41_ANR_NOTCH) {
          // the notch pass sees the scaled block behind the unscaled one: its delay line = the last 79 unscaled samples
          _Pragma("unroll 4") for (int r = g; r < kAnrHist; r += 4) T[r * kAnrRow + c] = T[(256 + r) * kAnrRow + c];
          __builtin_amdgcn_wave_barrier();
          _Pragma("unroll 4") for (int i = g; i < 256; i += 4) T[(kAnrHist + i) * kAnrRow + c] = T[(kAnrHist + i) * kAnrRow + c] * 1.5f;
        } else {
          _Pragma("unroll 4") for (int i = g; i < 256; i += 4) O[i * kAnrRow + c] = T[(kAnrHist + i) * kAnrRow + c] * 1.5f;
        }
      }
      __syncthreads();
    }
    if (T41_ANR_NOTCH) {  // Process.cpp:862-866
      if (wv == 0) anr_pass_y<true>(T, O, SIG, w, lidx, ngamma, lane);
      else anr_pass_sigma(T, SIG, lane);
      __syncthreads();
    }
    // the delay line's live part for the next block
    if (wv == 0)
      _Pragma("unroll 4") for (int r = g; r < kAnrHist; r += 4) T[r * kAnrRow + c] = T[(256 + r) * kAnrRow + c];
    __syncthreads();
_Pragma("nounroll")
    for (int cc = wv; cc < nlive; cc += 2) {
      float *dst = a.aud + ((size_t)(LIST ? a.list[ch0 + cc] : ch0 + cc) * a.nframes + f) * 256;
#pragma unroll
      for (int q = 0; q < 4; ++q) dst[lane + 64 * q] = O[(lane + 64 * q) * kAnrRow + cc];
    }
  }
  if (wv == 0 && c < nlive) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      a.anr[(size_t)(kAnrStW + tb + 2 * t + 1) * nch + ch] = w[t].x;
      a.anr[(size_t)(kAnrStW + tb + 2 * t) * nch + ch] = w[t].y;
    }
    _Pragma("unroll 4") for (int r = g; r < kAnrHist; r += 4) a.anr[(size_t)(kAnrStHist + r) * nch + ch] = T[r * kAnrRow + c];
    if (g == 0) {
      a.anr[(size_t)kAnrStLidx * nch + ch] = lidx;
      a.anr[(size_t)kAnrStNgamma * nch + ch] = ngamma;
    }
  }
}
#undef T41_ANR_ARGS
#undef T41_ANR_LMS
#undef T41_ANR_NOTCH
