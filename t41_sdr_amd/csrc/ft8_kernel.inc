// t41_sdr_amd/csrc/ft8_kernel.inc -- the text of ft8_kernel, included twice by ft8_kernel.hip: T41_STAGE_KERNEL names the
// kernel, T41_STAGE_ARGS its argument block, T41_STAGE_LIST 0 makes the kernel as it is without an FT8 map -- workgroup b
// is channel b and writes row b --, 1 its list form (t41rx_set_ft8_map): workgroup b takes entry b of the host-built list
// of {channel, row} pairs, indexes the FT8 memory and the audio by the channel, d_power and d_status by the row.  Two
// kernels of one text, not one body with a run-time switch: the form without a map must stay the instruction stream it
// was (profiles/ft8_map_isa_fingerprint.txt).  What the forms differ in is T41_FT8_ROW below and the two lines that
// fetch the pair.
#if T41_STAGE_LIST
#define T41_FT8_ROW prow
#else
#define T41_FT8_ROW ch
#endif
// (NT: 256, a workgroup per channel, is the one instantiation.  The wave-per-channel arm, NT = 64, was measured and is
// gone -- DESIGN.md, "FT8 receive"; the parameter stays because the kernel's name carries it)
template <int NT>
__global__ __launch_bounds__(NT) void T41_STAGE_KERNEL(T41_STAGE_ARGS a) {
#pragma clang fp contract(off)
  using namespace ft8;
  __shared__ short sbuf[kFt8BufWords];
  __shared__ __attribute__((aligned(16))) unsigned fz[1024];
  __shared__ unsigned nat[1024];
  __shared__ unsigned tw[768];
  __shared__ unsigned short mg[kFt8Bins + 3];
  __shared__ short qs[68];
  constexpr int kIt = (68 + NT - 1) / NT;  // collector iterations per thread
#if T41_STAGE_LIST
  const Ft8Pair pr = a.list[blockIdx.x];  // uniform: one scalar load of the pair (blockIdx.x < nlist, the grid)
  const int ch = pr.channel, prow = pr.row, t = threadIdx.x;
#else
  const int ch = blockIdx.x, t = threadIdx.x;
#endif
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
      uint8_t *row = a.power + ((size_t)T41_FT8_ROW * 2 + (size_t)half) * kFt8HalfBytes + (size_t)kFt8BlockBytes * (size_t)counter;
#include "ft8_block.inc"
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
    if (t == 0) *reinterpret_cast<int4 *>(a.status + ((size_t)T41_FT8_ROW * a.nframes + f) * 4) = make_int4(counter, flag, done, dataLoop);
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
#undef T41_FT8_ROW
