// t41_sdr_amd/csrc/ft8_audio_kernel.inc -- the text of ft8_audio_kernel, included twice by ft8_kernel.hip, as ft8_kernel.inc
// is: T41_STAGE_KERNEL names the kernel, T41_STAGE_ARGS its argument block, T41_STAGE_LIST 0 makes the kernel as it is
// without an FT8 map, 1 its list form (t41rx_set_ft8_map): workgroup b takes entry b of the list of {channel, row} pairs,
// indexes the FT8 memory by the channel, and pcm, d_power and d_status by the row.
#if T41_STAGE_LIST
#define T41_FT8_ROW prow
#else
#define T41_FT8_ROW ch
#endif
template <typename Sample>
__global__ __launch_bounds__(256) void T41_STAGE_KERNEL(T41_STAGE_ARGS a) {
#pragma clang fp contract(off)
  using namespace ft8;
  constexpr int NT = 256;
  __shared__ short sbuf[kFt8BufWords];
  __shared__ __attribute__((aligned(16))) unsigned fz[1024];
  __shared__ unsigned nat[1024];
  __shared__ unsigned tw[768];
  __shared__ unsigned short mg[kFt8Bins + 3];
#if T41_STAGE_LIST
  const Ft8Pair pr = a.list[blockIdx.x];  // uniform: one scalar load of the pair (blockIdx.x < nlist, the grid)
  const int ch = pr.channel, prow = pr.row, t = threadIdx.x;
#else
  const int ch = blockIdx.x, t = threadIdx.x;
#endif
  int32_t *w = a.state + (size_t)ch * kFt8Words;
  auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
  const int flag0 = uni(w[kFt8Flag]), counter0 = uni(w[kFt8Counter]), dataLoop0 = uni(w[kFt8DataLoop]), half0 = uni(w[kFt8Half]);
  int flag = flag0, counter = counter0, half = half0;
  for (int i = t; i < kFt8BufWords; i += NT) sbuf[i] = (short)w[kFt8Scalars + i];
  for (int i = t; i < 768; i += NT) tw[i] = a.tab[kFt8TabTw + i];
  __syncthreads();

  const Sample *x = static_cast<const Sample *>(a.pcm) + (size_t)T41_FT8_ROW * (size_t)a.nframes * kFt8AudioFrame;
  int d0 = dataLoop0;
  for (int f = 0; f < a.nframes;) {
    const int d1 = min(15, d0 + a.nframes - f);
    for (int c = kFt8AudioCells * d0 + t; c < kFt8AudioCells * d1; c += NT) {  // c <= 1019
      const int d = c / kFt8AudioCells, i = c - kFt8AudioCells * d;
      const short q = audio_q15(x[(f + d - d0) * kFt8AudioFrame + ((i * 15) >> 3)]);  // frame < nframes, sample <= 125
      sbuf[c] = sbuf[c + 1024];
      sbuf[c + 1024] = sbuf[c + 2048];
      sbuf[c + 2048] = q;
    }
    f += d1 - d0;
    d0 = d1;
    if (d1 == 15) {
      d0 = 0;
      __syncthreads();
      if (counter < kFt8SlotBlocks) {
        uint8_t *row = a.power + ((size_t)T41_FT8_ROW * 2 + (size_t)half) * kFt8HalfBytes + (size_t)kFt8BlockBytes * (size_t)counter;
  #include "ft8_block.inc"
        ++counter;
        if (counter == kFt8SlotBlocks) {
          flag = 0;
          half ^= 1;
          counter = 0;
        }
      }
    }
  }
  // the status words: nb blocks have run behind frame f
  for (int f = t; f < a.nframes; f += NT) {
    const int fed = dataLoop0 + f + 1, nb = fed / 15;
    int c = counter0, fl = flag0, done = 0;
    if (counter0 < kFt8SlotBlocks) {
      c = counter0 + nb;
      if (c >= kFt8SlotBlocks) {  // at most one completion in kFt8MaxFrames frames
        c -= kFt8SlotBlocks;
        fl = 0;
      }
      if (fed == 15 * (kFt8SlotBlocks - counter0)) done = 1 + half0;
    }
    *reinterpret_cast<int4 *>(a.status + ((size_t)T41_FT8_ROW * a.nframes + f) * 4) = make_int4(c, fl, done, fed - 15 * nb);
  }
  __syncthreads();
  for (int i = t; i < kFt8BufWords; i += NT) w[kFt8Scalars + i] = (int)sbuf[i];
  if (t == 0) {
    w[kFt8N] = (int)((unsigned)w[kFt8N] + (unsigned)a.nframes);
    w[kFt8Flag] = flag;
    w[kFt8Counter] = counter;
    w[kFt8DataLoop] = d0;
    w[kFt8Half] = half;
  }
}
#undef T41_FT8_ROW
