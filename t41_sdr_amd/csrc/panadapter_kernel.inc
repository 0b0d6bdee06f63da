// t41_sdr_amd/csrc/panadapter_kernel.inc -- the text of panadapter_kernel, included twice by panadapter_kernel.hip:
// T41_STAGE_KERNEL names the kernel, T41_STAGE_ARGS its argument block, T41_STAGE_LIST 0 makes the kernel as it is without
// a panadapter map -- wave b is channel b, reads tap row b and writes row b --, 1 its list form
// (t41rx_set_panadapter_map): wave b takes entry b of the host-built list of {channel, row, RFgain, rfGainAllBands}
// entries, indexes the panadapter memory and the levels by the channel, the two taps and the seven row buffers by the
// row, and takes DrawSmeterBar()'s two gains from the entry.  Two kernels of one text, not one body with a run-time
// switch: the form without a map must stay the instruction stream it was (profiles/pan_map_isa_fingerprint.txt).  What
// the forms differ in is the three names below and the lines that fetch the entry.
//
// Both forms are one wave per block: the early return in front of __syncthreads() is safe only because of that.
#if T41_STAGE_LIST
#define T41_PAN_ROW prow
#define T41_PAN_RFGAIN ent_rf
#define T41_PAN_RFGAIN_ALL ent_all
#else
#define T41_PAN_ROW ch
#define T41_PAN_RFGAIN a.RFgain
#define T41_PAN_RFGAIN_ALL a.rfGainAllBands
#endif
template <bool ZOOMED>
__global__ __launch_bounds__(64) void T41_STAGE_KERNEL(const T41_STAGE_ARGS a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float xbuf[8 * kFftRow * 2];  // FFT exchange
  __shared__ PanZoomLds<ZOOMED> z;
  __shared__ unsigned short grad[128];
  const int lane = threadIdx.x;
#if T41_STAGE_LIST
  if ((int)blockIdx.x >= a.nlist) return;
  // wave-uniform and read-only: one 16-byte scalar load of the entry; the host has checked the channel and the row
  // (t41rx_set_panadapter_map), the kernel does not
  typedef const __attribute__((address_space(4))) PanEntry *EntryPtr;
  const EntryPtr ent = (EntryPtr)a.list + blockIdx.x;
  const int ch = ent->channel, prow = ent->row, ent_rf = ent->RFgain, ent_all = ent->rfGainAllBands;
#else
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
#endif
  constexpr int L = 2048, R = 512;
  float *ds = a.mem + (size_t)ch * kPanFloats;
  int *dsi = reinterpret_cast<int *>(ds);
  const cf *tab = reinterpret_cast<const cf *>(a.tab);
  cf tw1[7], tw2[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    tw1[q] = tab[kTabTw1 + 64 * q + lane];
    tw2[q] = tab[kTabTw2 + 64 * q + lane];
  }
  const int zoom = ZOOMED ? a.zoom : 0;
  float st[16], fh[3];  // zoom filter memories of my chain
  int ptr = 0;
  if constexpr (ZOOMED) zoom_load(st, fh, ptr, z.ring, ds, lane);
  float old[8];  // FFT_spec_old
  int pold[8];   // pixelold
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int x = (lane + 64 * r + 256) & 511;  // display column of bin lane + 64 r
    old[r] = ds[kDispOld + x];
    pold[r] = reinterpret_cast<const short *>(ds + kPanPixel)[x];
  }
  double win[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) win[r] = a.win[lane + 64 * r];
  for (int i = lane; i < 128; i += 64) grad[i] = i < kPanGradient ? a.gradient[i] : (unsigned short)0;
  __syncthreads();
  const int nf = a.noise_floor[ch];                            // currentNF: constant for every row of a call
  int oldnf = dsi[kPanNewSpectrum] != 0 ? dsi[kPanOldNf] : nf;  // newSpectrumFlag == 0: oldNF = currentNF
  const float gain_correction = a.gain_correction[ch];
  for (int k = 0; k < a.nrows; ++k) {
    const size_t row = (size_t)T41_PAN_ROW * (size_t)a.max_rows + (size_t)k;
    const float *pI = a.pre + row * (2 * L), *pQ = pI + L;
    cf v[8];
    if constexpr (!ZOOMED) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {  // float * double -> double -> float, FFT.cpp:222-223
        const int i = lane + 64 * r;
        v[r] = cf{(float)((double)pI[i] * win[r]), (float)((double)pQ[i] * win[r])};
      }
    } else {
      __syncthreads();
      for (int n = lane; n < L; n += 64) {  // FreqShift1 (Freq_Shift.cpp:42-65): x j^n
        const float xi = pI[n], xq = pQ[n];
        const int m = n & 3;
        z.stage[0][n] = (m == 0) ? xi : (m == 1) ? -xq : (m == 2) ? -xi : xq;
        z.stage[1][n] = (m == 0) ? xq : (m == 1) ? xi : (m == 2) ? -xq : -xi;
      }
      __syncthreads();
      zoom_frame(st, fh, ptr, z.stage, z.dec, z.ring, a.iir, a.fir, win, zoom, lane, v);
    }
    fft512<false>(v, tw1, tw2, xbuf, lane);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int x = (lane + 64 * r + 256) & 511;  // bins 0..255 -> upper half, 256..511 -> lower half
      const float m = v[r].x * v[r].x + v[r].y * v[r].y;
      // the pixel: from the un-smoothed FFT_spec at zoom 0 (FFT.cpp:245), from the smoothed one at zoom 1..4 (:157)
      const float spec = zoom_lowpass(zoom, m, old[r]);
      const int p = display_pixel(a.base, a.dBScale, spec);
      const int yn = pan_clamp(a.noise_floor_y - p - nf, kSpectrumTopY, kSpectrumBottom);
      const int yo = pan_clamp(a.noise_floor_y - pold[r] - oldnf, kSpectrumTopY, kSpectrumBottom);
      const unsigned short wf = x < R - 1 ? grad[pan_clamp(230 - yn, 0, kPanGradient - 1)] : (unsigned short)0;
      pold[r] = p;
      if (a.spec) a.spec[row * R + x] = spec;
      // 2-byte stores from the registers, 128 contiguous bytes per instruction.  (Staged through LDS so that a row leaves
      // as 64 16-byte stores it was slower: 5903 against 5850 us per 4096 x 128 launch at period 1, DESIGN.md "Panadapter")
      if (a.pixel) a.pixel[row * R + x] = (int16_t)p;
      if (a.y_new) a.y_new[row * R + x] = (int16_t)yn;
      if (a.y_old) a.y_old[row * R + x] = (int16_t)yo;
      if (a.waterfall) a.waterfall[row * R + x] = wf;
    }
    oldnf = nf;
    if (lane == 0 && a.smeter) {
      const float *mx = a.mx + row * 3;
      float *sm = a.smeter + row * 4;
      sm[0] = mx[0];
      sm[1] = mx[1];
      sm[2] = mx[2];
      sm[3] = pan_dbm(gain_correction, a.attenuator, mx[2], T41_PAN_RFGAIN, T41_PAN_RFGAIN_ALL);
    }
  }
  // the memory back
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int x = (lane + 64 * r + 256) & 511;
    ds[kDispOld + x] = old[r];
    reinterpret_cast<short *>(ds + kPanPixel)[x] = (short)pold[r];
  }
  if (lane == 0 && a.nrows > 0) {
    dsi[kPanOldNf] = oldnf;
    dsi[kPanNewSpectrum] = 1;
  }
  if constexpr (ZOOMED) {
    __syncthreads();
    zoom_store(ds, st, fh, ptr, z.ring, lane);
  }
}
#undef T41_PAN_ROW
#undef T41_PAN_RFGAIN
#undef T41_PAN_RFGAIN_ALL
