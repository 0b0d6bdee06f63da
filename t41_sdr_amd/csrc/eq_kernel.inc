// t41_sdr_amd/csrc/eq_kernel.inc -- the text of eq_kernel, included twice by eq_kernel.hip: T41_STAGE_KERNEL names the kernel,
// T41_STAGE_LIST 0 makes the kernel as it is without a stage map, 1 its list form (t41rx_set_stage_map).  Two kernels
// of one text, not one body shared by two kernels: an argument block handed on by reference compiles to another
// instruction stream, and the form without a map must stay the stream it was.
// T41_STAGE_LEVELS 1 (t41rx_set_receive_eq_map) makes either form with the levels per channel: a band's signed level comes
// from row `channel` of a.levels ([nchan][kEqBands], converted on the host like a.scale) and nothing else changes.
__global__ __launch_bounds__(64) void T41_STAGE_KERNEL(EqArgs a) {
#pragma clang fp contract(off)
  constexpr bool LIST = T41_STAGE_LIST != 0;
  using namespace df2t;
  __shared__ __attribute__((aligned(16))) float xin[kChunk];
  __shared__ __attribute__((aligned(16))) float ring[kEqBands * kRowPitch];
  const int lane = threadIdx.x;
  const int band = lane >> 2, stage = lane & 3;
  const bool live = lane < kEqSections;
  const unsigned ch = LIST ? (unsigned)a.list[blockIdx.x] : blockIdx.x;
  float *st = a.state + (size_t)ch * kEqStateFloats;
  float *x = a.aud + (size_t)ch * a.nsamp;
  const int nchunk = a.nsamp / kChunk;

  Pipe<kEqStages, kQuadFromPrev, true, false> p;
  p.head = stage == 0;
  p.tail = live && stage == kEqStages - 1;
  if (live) {
    const float *c = a.coef + 5 * lane;
    p.q = Section{c[0], c[1], c[2], c[3], c[4], st[2 * lane], st[2 * lane + 1]};
#if T41_STAGE_LEVELS
    p.level = a.levels[(size_t)ch * kEqBands + band];
#else
    p.level = a.scale[band];
#endif
  }
  p.row = ring + (live ? band : 0) * kRowPitch;
  // samples 64 k .. 64 k + 63 through the sum and back
  auto sum_chunk = [&](int k) { x[(size_t)k * kChunk + lane] = sum_bands(ring + (k & 1) * kChunk + lane); };

  float nxt = x[lane];
  for (int c = 0; c < nchunk; ++c) {
    xin[lane] = nxt;
    if (c + 1 < nchunk) nxt = x[(size_t)(c + 1) * kChunk + lane];
    __syncthreads();
    if (c == 0) {  // the pipeline fills: stage s starts at step s
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(xin + j);
        p.run(v.x, j, 0, j >= stage);
        p.run(v.y, j + 1, 0, j + 1 >= stage);
        p.run(v.z, j + 2, 0, j + 2 >= stage);
        p.run(v.w, j + 3, 0, true);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kChunk; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(xin + j);
        p.run(v.x, j, c, true);
        p.run(v.y, j + 1, c, true);
        p.run(v.z, j + 2, c, true);
        p.run(v.w, j + 3, c, true);
      }
    }
    __syncthreads();
    if (c > 0) sum_chunk(c - 1);
  }
  // the pipeline drains: step 64 n + d runs stages d + 1 .. 3 on the last samples
  p.run(0.0f, kChunk + 0, nchunk - 1, stage > 0);
  p.run(0.0f, kChunk + 1, nchunk - 1, stage > 1);
  p.run(0.0f, kChunk + 2, nchunk - 1, stage > 2);
  __syncthreads();
  sum_chunk(nchunk - 1);
  if (live) {
    st[2 * lane] = p.q.d1;
    st[2 * lane + 1] = p.q.d2;
  }
}
