// t41_sdr_amd/csrc/cw_filter_kernel.inc -- the text of cw_filter_kernel, included twice by cw_kernel.hip: T41_STAGE_KERNEL
// names the kernel, T41_STAGE_ARGS its argument block, T41_STAGE_MAP 0 makes the kernel as it is without a CW filter map,
// 1 its map form (t41rx_set_cw_filter_map).  Two kernels of one text, not one body shared by two kernels and no run-time
// branch: the form without a map must stay the instruction stream it was.
//
// MAP: wave b serves the channels list[8 b] .. list[8 b + 7] of the ascending list of filtered channels (the ragged last
// wave fewer, as without a map); the eight channel numbers are wave-uniform and come by scalar loads -- the list is padded
// to a multiple of eight entries -- and every row of the audio is named through them.  The eight lanes of a group then
// take their own channel's CWFilterIndex from index_of[channel]: it selects the coefficient row of the full 5 x 30 table
// and the [filter][stage] slot of the channel's state, per lane, once per launch.
__global__ __launch_bounds__(64) void T41_STAGE_KERNEL(T41_STAGE_ARGS a) {
#pragma clang fp contract(off)
  using namespace cw;
  using namespace df2t;
  __shared__ __attribute__((aligned(16))) float xin[kCwChanPerWave * kInPitch];
  __shared__ __attribute__((aligned(16))) float ring[kCwChanPerWave * kRowPitch];
  const int lane = threadIdx.x;
  const int grp = lane >> 3, stage = lane & 7;
  const int ch0 = blockIdx.x * kCwChanPerWave;
#if T41_STAGE_MAP
  const int nlive = min(kCwChanPerWave, a.nlist - ch0);  // channels of this wave (the ragged last one has fewer)
  const bool live = stage < kCwStages && grp < nlive;
  int chn[kCwChanPerWave];  // wave-uniform: the wave's channels (entries past nlive are the list's padding, never used)
#pragma unroll
  for (int kk = 0; kk < kCwChanPerWave; ++kk) chn[kk] = a.list[ch0 + kk];
  const int mine = live ? a.list[ch0 + grp] : 0;
  const int index = live ? a.index_of[mine] : 0;
  float *st = a.state + (size_t)mine * kCwStateFloats + kCwStFilter + 2 * kCwStages * index + 2 * stage;
#define T41_CW_ROW(kk) (a.aud + (size_t)chn[kk] * a.nsamp)
#else
  const int nlive = min(kCwChanPerWave, a.nchan - ch0);  // channels of this wave (the ragged last one has fewer)
  const bool live = stage < kCwStages && grp < nlive;
  float *x = a.aud + (size_t)ch0 * a.nsamp;
  float *st = a.state + (size_t)(ch0 + grp) * kCwStateFloats + kCwStFilter + 2 * kCwStages * a.index + 2 * stage;
#define T41_CW_ROW(kk) (x + (size_t)(kk) * a.nsamp)
#endif
  const int nchunk = a.nsamp / kChunk;

  Pipe<kCwStages, kRowShr1, false, true> p;
  p.head = stage == 0;
  p.tail = live && stage == kCwStages - 1;
  if (live) {
#if T41_STAGE_MAP
    const float *c = a.coef + kCwFilterCoefs * index + 5 * stage;
#else
    const float *c = a.coef + 5 * stage;
#endif
    p.q = Section{c[0], c[1], c[2], c[3], c[4], st[0], st[1]};
  }
  const float *in_row = xin + grp * kInPitch;
  p.row = ring + grp * kRowPitch;

  // samples 64 k .. 64 k + 63 of every channel of the wave back to the scratch, coalesced
  auto store_chunk = [&](int k) {
#if T41_STAGE_MAP
#pragma unroll
    for (int kk = 0; kk < kCwChanPerWave; ++kk)
      if (kk < nlive) T41_CW_ROW(kk)[(size_t)k * kChunk + lane] = ring[kk * kRowPitch + (k & 1) * kChunk + lane];
#else
    for (int kk = 0; kk < nlive; ++kk)
      x[(size_t)kk * a.nsamp + (size_t)k * kChunk + lane] = ring[kk * kRowPitch + (k & 1) * kChunk + lane];
#endif
  };

  float nxt[kCwChanPerWave];
#pragma unroll
  for (int kk = 0; kk < kCwChanPerWave; ++kk) nxt[kk] = kk < nlive ? T41_CW_ROW(kk)[lane] : 0.0f;
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int kk = 0; kk < kCwChanPerWave; ++kk) xin[kk * kInPitch + lane] = nxt[kk];
    if (c + 1 < nchunk) {
#pragma unroll
      for (int kk = 0; kk < kCwChanPerWave; ++kk)
        if (kk < nlive) nxt[kk] = T41_CW_ROW(kk)[(size_t)(c + 1) * kChunk + lane];
    }
    __syncthreads();
    if (c == 0) {  // the pipeline fills: stage s starts at step s
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(in_row + j);
        p.run(v.x, j, 0, j >= stage);
        p.run(v.y, j + 1, 0, j + 1 >= stage);
        p.run(v.z, j + 2, 0, j + 2 >= stage);
        p.run(v.w, j + 3, 0, j + 3 >= stage);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(in_row + j);
        p.run(v.x, j, c, true);
        p.run(v.y, j + 1, c, true);
        p.run(v.z, j + 2, c, true);
        p.run(v.w, j + 3, c, true);
      }
    }
    __syncthreads();
    if (c > 0) store_chunk(c - 1);
  }
  // the pipeline drains: step 64 n + d runs stages d + 1 .. 5 on the last samples
#pragma unroll
  for (int d = 0; d < kCwStages - 1; ++d) p.run(0.0f, kChunk + d, nchunk - 1, stage > d);
  __syncthreads();
  store_chunk(nchunk - 1);
  if (live) {
    st[0] = p.q.d1;
    st[1] = p.q.d2;
  }
#undef T41_CW_ROW
}
