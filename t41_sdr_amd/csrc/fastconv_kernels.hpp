// t41_sdr_amd/csrc/fastconv_kernels.hpp -- FFT_LENGTH 1024 / 2048 / 4096 (BASELINE config 4): the N-point overlap-save fast convolution, fastconv_kernel<R, CPLX, BACK> and the one-kernel form fastconv_fused_kernel<PLAIN>.
#pragma once
#include "rx_device.hpp"

namespace t41 {

// ------------------------------------------------------------------------------------------
// FFT_LENGTH 4096 (BASELINE config 4, a synthetic generalisation: the firmware is compiled for
// 512; 1024 and 2048 likewise with R = 2, 4 in place of 8): overlap-save fast convolution, one
// channel per 4-wave workgroup.  4096 = 8 x 512:
//   pass 1 (DIF radix-8 over p, x[k' + 512 p]): DFT8, twiddle W4096^(k' q)  -> Z[q][k'] in place
//   pass 2 per q: fft512 over k' -> X[q + 8 m]; x mask; inverse fft512 over m -> W[q][k'] in place
//   pass 3 (inverse of pass 1): conj twiddle, inverse DFT8 over q -> y[k' + 512 p], natural order
// The 4096-point working array lives in LDS (32 KiB, every access is lane-contiguous), the
// 512-point sub-FFTs are the same register/LDS-exchange code as the 512 path.  Each pass is 8
// independent pieces (column blocks / rows): wave w takes pieces w and w + 4, workgroup barriers
// separate the passes.  (One wave per channel left a CU with 4 latency-bound waves: 28.5 us for
// 1024 channels; four per channel: 3 workgroups = 12 waves per CU.)
// ------------------------------------------------------------------------------------------
// The working array is R rows of 512 complex; a row is padded to the size of the fft512 exchange
// scratch (8 x kFftRow complex = 576), because while a wave holds a row in registers for its
// 512-point FFTs the row's own LDS is free to be that scratch: no separate scratch buffers,
// 36 KiB per workgroup at R = 8, four workgroups (16 waves) per CU.
constexpr int kFcRow = 8 * kFftRow;  // complex units per padded row
static_assert(kFcRow >= 512, "row padding");
constexpr int fc_lds_floats(int R) { return 2 * kFcRow * R + 2 * (448 + 56); }  // working array + the 512-point FFT's twiddles

// Waves per channel and LDS budget.  The kernel is bound by the latency of its barrier-separated
// phases, not by any throughput (stamps: a workgroup alone on a CU is hardly faster than one of
// three, and 8 waves per channel bought 3 %), so what counts is how many channels a CU holds at
// once -- and that every channel of the 1024-channel batch is resident in ONE round (3 per CU =
// 768 slots left a second round at a third of the occupancy: 16 frame-times where 10.7 would do).
// Fused kernel, R = 8: four workgroups per CU = 40 KiB each = [working array 36 KiB | twiddles
// 4 KiB] and nothing else: the frame's audio, then the output transposition buffers and the x4
// interpolator's boundary samples alias the working array (one more barrier), and what crosses the
// frames (24 audio samples, 7 x2 outputs) waits in two registers of wave 0.
constexpr int kFcWaves = 4;
constexpr int kFcWavesPerSimd = 4;  // waves per SIMD the register allocation is held to (four workgroups per CU)
constexpr int fc_arr_floats(int R) { return 2 * kFcRow * R < kFcWaves * 2048 + 8 * (R + 1) ? kFcWaves * 2048 + 8 * (R + 1) : 2 * kFcRow * R; }  // >= four transposition buffers + YT
constexpr int fcb_lds_floats(int R) { return fc_arr_floats(R) + 2 * (448 + 56); }
static_assert(fcb_lds_floats(8) * 4 * 4 <= 160 * 1024, "four fused workgroups per CU");
template <int R, bool INV>
__device__ __forceinline__ void dft_r(cf (&v)[R]) {
  if constexpr (R == 8) {
    dft8<INV>(v);
  } else if constexpr (R == 4) {
    const cf a0 = v[0] + v[2], a1 = v[0] - v[2], a2 = v[1] + v[3];
    // -j (v1 - v3) forward, +j (v1 - v3) inverse
    const cf d = v[1] - v[3];
    v[0] = a0 + a2;
    v[2] = a0 - a2;
    v[1] = INV ? add_pj(a1, d) : add_mj(a1, d);
    v[3] = INV ? add_mj(a1, d) : add_pj(a1, d);
  } else {
    const cf a0 = v[0] + v[1], a1 = v[0] - v[1];
    v[0] = a0;
    v[1] = a1;
  }
}

// N = 512 R, R = 2, 4, 8 (FFT_LENGTH 1024, 2048, 4096).  CPLX: hand the complex valid half on as it
// is (AM, AGC on: the back kernel applies the AGC / gain and demodulates), else the SSB audio
// fixed_gain * Re.
// BACK: SSB / NFM audio with the fixed gain goes straight on through the x2 / x4 interpolators and
// out (Process.cpp:917-931) instead of to the `aud24` scratch and a third kernel: pass 3 leaves
// the frame's N/2 audio samples in LDS (where the working array was), then every wave runs whole
// 256-sample segments of the back end (s = wave, wave + 4) with the arithmetic of rx512_kernel's,
// the x4 interpolator's 7-sample history crossing the segment boundaries through LDS.
template <int R, bool CPLX, bool BACK = false>
__global__ __launch_bounds__((64 * kFcWaves), kFcWavesPerSimd) void fastconv_kernel(const RxArgs a) {
  static_assert(!(BACK && CPLX), "the fused back end takes real audio");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int N = 512 * R, D = N / 2;
  constexpr int NWV = kFcWaves, NT = 64 * NWV;  // waves / threads per channel
  constexpr int H = 8 / NWV;                       // column blocks (passes 1, 3) / rows (pass 2) / segments (back end) per wave
  int lane = threadIdx.x & 63;  // (re-defined per phase, see FRESH_LANE)
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  cf *A = reinterpret_cast<cf *>(smem);
  // behind the working array: the 512-point FFT's twiddles (tw1 [7][64], tw2 compacted to [7][8]),
  // read at the point of use -- the registers they would occupy hold what must not wait for L2
  constexpr int kArr = BACK ? fc_arr_floats(R) : 2 * kFcRow * R;
  cf *ltw = reinterpret_cast<cf *>(smem + kArr);
  float *AU = smem;                    // BACK, from pass 3 to the x2 interpolator: [0] pad, [1..23] history, [24 + i] audio sample i of the frame
  float *YT = smem + kFcWaves * 2048;  // BACK, behind the transposition buffers: [s][0] pad, [s][1..7] = the last 7 x2 outputs before segment s
  static_assert(!BACK || 24 + D + 8 <= kFcWaves * 2048, "the audio fits where the working array was");
  // BACK, wave 0: lane i < 24 = audio history entry i ([0] pad), lane i < 8 = x2 history entry i
  float hi_reg = 0.0f, yt_reg = 0.0f;
  float *st = a.state + (size_t)ch * state_floats(N);
  const cf *twN = reinterpret_cast<const cf *>(a.tab4k);                    // [R-1][512]
  const cf *maskN = reinterpret_cast<const cf *>(a.tab4k) + (R - 1) * 512;  // [R][512]
  const cf *tab = reinterpret_cast<const cf *>(a.tab);
  const float fixed_gain = ((CoefPtr)a.coef)->sc[kScFixedGain];

  for (int i = threadIdx.x; i < 448; i += NT) ltw[i] = tab[kTabTw1 + i];
  if (threadIdx.x < 56) ltw[448 + threadIdx.x] = tab[kTabTw2 + 64 * (threadIdx.x >> 3) + (threadIdx.x & 7)];
  if (BACK) {  // interpolator memories of the channel
    if (threadIdx.x < 24) hi_reg = st[kStInt1 + threadIdx.x];
    if (threadIdx.x < 8) yt_reg = st[kStInt2 + threadIdx.x];
  }
  // the outer radix-R pass' twiddles of this wave's two column blocks (r = wv, wv + 4): re-read
  // from L2 for passes 1 and 3 of every frame, requested ahead of the barrier in front of the pass
  // (pass 2 wants the 28 registers they would hold)
  cf twp[H][R > 1 ? R - 1 : 1];
  auto load_twp = [&]() {
    // (two scalar bases, one per h, and R - 1 lane offsets shared by both: a base per entry runs the kernel out of SGPRs)
    const LaneOff lo = fresh_off(2 * lane);
#pragma unroll
    for (int q = 1; q < R; ++q) {
      const LaneOff oq = LaneOff{lo.bytes + 4096u * (q - 1)};
#pragma unroll
      for (int h = 0; h < H; ++h) twp[h][q - 1] = ldg_cf(twN + 64 * (wv + NWV * h), oq);
    }
  };

#ifdef T41RX_STAMP
  unsigned long long stamp_acc = 0, stamp_last, stamp_t0;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_t0)::"memory");
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_last)::"memory");
#endif
  cf x1[H][R];
  auto load_x1 = [&](int f) {
    const cf *mid = reinterpret_cast<const cf *>(a.mid + ((size_t)ch * a.nframes4k + f) * (2 * D));
    const cf *prev = (f == 0) ? reinterpret_cast<const cf *>(st + kStOverlap) : mid - D;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int k = lane + 64 * (wv + NWV * h);
#pragma unroll
      for (int p = 0; p < R; ++p) {
        const int e = k + 512 * p;  // index into [previous | new]
        x1[h][p] = (p < R / 2) ? prev[e] : mid[e - D];
        if (p < R / 2 && f == 0 && a.ovl_real) x1[h][p].y = 0.0f;  // NFM: last_sample_buffer_R is not part of the block
      }
    }
  };
  for (int f = 0; f < a.nframes4k; ++f) {
    FRESH_LANE();
    // issue priority falls with progress: the arbiter favours the oldest waves, so without it the
    // first workgroup of a CU finishes long before the last (108 .. 195 us, stamps), which then
    // runs alone -- and alone a workgroup is latency-bound
    switch ((4 * f) / a.nframes4k) {
      case 0: PRIO(3); break;
      case 1: PRIO(2); break;
      case 2: PRIO(1); break;
      default: PRIO(0); break;
    }
    // ---- overlap-save assemble (Process.cpp:498-522): [previous N/2 | new N/2].  Inside a call the
    // previous block is the preceding frame's `mid` (just read, L2-warm); the state record supplies
    // it for the call's first frame and receives the last frame's block.  Pass 1 takes its inputs
    // x[k + 512 p] straight from there (8 bytes per lane, 512 per instruction): the array is first
    // written with pass 1's results.
    // (requesting the next frame's inputs before the back end instead -- the registers are there --
    // measured 1..3 % slower: the loads queue up behind the back end's 64 KiB of stores)
    load_x1(f);
    STAMP(2);
    load_twp();
    STAMP(0);         // (tail of the previous frame: stores issued, history rolled)
    __syncthreads();  // the previous frame's back end is done with the array (first frame: the twiddles are staged)
    STAMP(1);
    FRESH_LANE();
    // ---- pass 1
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int k = lane + 64 * (wv + NWV * h);
      cf v[R];
#pragma unroll
      for (int p = 0; p < R; ++p) v[p] = x1[h][p];
      if (f == a.nframes4k - 1) {  // next call's "previous"
#pragma unroll
        for (int p = R / 2; p < R; ++p) {
          cf *ov = reinterpret_cast<cf *>(st + kStOverlap) + (k + 512 * p - D);
          if (a.ovl_real) ov->x = v[p].x;  // NFM: last_sample_buffer_L alone (Process.cpp:765-816), R stays as it is
          else *ov = v[p];
        }
      }
      dft_r<R, false>(v);
#pragma unroll
      for (int q = 1; q < R; ++q) v[q] = cmul(v[q], twp[h][q - 1]);
#pragma unroll
      for (int q = 0; q < R; ++q) A[k + kFcRow * q] = v[q];
    }
    // the filter mask of this wave's rows of pass 2 (q = wv, wv + 4): requested here, so its L2
    // round trip runs under the barrier and the forward FFTs
    cf mk[H][8];
    const LaneOff lom = fresh_off(2 * lane);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int q = wv + NWV * h;
      if (q < R) {
#pragma unroll
        for (int r = 0; r < 8; ++r) mk[h][r] = ldg_cf(maskN + 512 * q, lom, 64 * r);
      }
    }
    STAMP(5);
    __syncthreads();
    STAMP(6);
    FRESH_LANE();
    // ---- pass 2: 512-point FFT, mask (pre-scaled by 1/N), inverse 512-point FFT, per q
    if constexpr (R == 8 && H == 2) {  // both rows of the wave in lockstep
      const int q0 = wv, q1 = wv + NWV;
      cf v[8], u[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = A[kFcRow * q0 + lane + 64 * r];
#pragma unroll
      for (int r = 0; r < 8; ++r) u[r] = A[kFcRow * q1 + lane + 64 * r];
      float *xv = smem + 2 * kFcRow * q0, *xu = smem + 2 * kFcRow * q1;  // the rows themselves (now in registers) are the exchange scratch
      fft512_ldstw_x2<false>(v, u, ltw + lane, ltw + 448 + (lane & 7), xv, xu, lane);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        v[r] = cmul(v[r], mk[0][r]);
        u[r] = cmul(u[r], mk[1][r]);
      }
      fft512_ldstw_x2<true>(v, u, ltw + lane, ltw + 448 + (lane & 7), xv, xu, lane);
      wave_sync();
#pragma unroll
      for (int r = 0; r < 8; ++r) A[kFcRow * q0 + lane + 64 * r] = v[r];
#pragma unroll
      for (int r = 0; r < 8; ++r) A[kFcRow * q1 + lane + 64 * r] = u[r];
    } else {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const int q = wv + NWV * h;
        if (q < R) {
          cf v[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = A[kFcRow * q + lane + 64 * r];
          float *xbuf = smem + 2 * kFcRow * q;  // the row itself (now in registers) is the exchange scratch
          wave_sync();
          fft512_ldstw<false>(v, ltw + lane, ltw + 448 + (lane & 7), xbuf, lane, []() {});
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = cmul(v[r], mk[h][r]);
          fft512_ldstw<true>(v, ltw + lane, ltw + 448 + (lane & 7), xbuf, lane, []() {});
          wave_sync();
#pragma unroll
          for (int r = 0; r < 8; ++r) A[kFcRow * q + lane + 64 * r] = v[r];
        }
      }
    }
    load_twp();
    STAMP(7);
    __syncthreads();
    STAMP(8);
    FRESH_LANE();
    // ---- pass 3; AGC off: fixed gain (DSP_Fn.cpp:494-502); SSB: audio = Re of the valid half
    float *au = a.aud24 + ((size_t)ch * a.nframes4k + f) * D;
    float y3[H][R / 2];  // BACK: the audio samples k + 512 j of this wave's column blocks
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int k = lane + 64 * (wv + NWV * h);
      cf v[R];
#pragma unroll
      for (int q = 0; q < R; ++q) v[q] = A[k + kFcRow * q];
#pragma unroll
      for (int q = 1; q < R; ++q) v[q] = cmulc(v[q], twp[h][q - 1]);
      dft_r<R, true>(v);
#pragma unroll
      for (int p = R / 2; p < R; ++p) {
        if (CPLX)
          reinterpret_cast<cf *>(a.aud24)[((size_t)ch * a.nframes4k + f) * D + k + 512 * (p - R / 2)] = v[p];
        else if (BACK)
          y3[h][p - R / 2] = fixed_gain * v[p].x;
        else
          au[k + 512 * (p - R / 2)] = fixed_gain * v[p].x;
      }
    }
    if (BACK) {
      const CoefPtr cf0 = (CoefPtr)a.coef;
      float ci[48];  // the x2 interpolator's taps: requested here, so the scalar loads' latency runs under the barrier
      load_taps<48>(ci, (CFloatPtr)cf0, kCoInt1);
      STAMP(9);
      __syncthreads();  // every wave has read its columns: the working array is free
      FRESH_LANE();
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int j = 0; j < R / 2; ++j) AU[24 + lane + 64 * (wv + NWV * h) + 512 * j] = y3[h][j];
      if (threadIdx.x < 24) AU[threadIdx.x] = hi_reg;
      if (threadIdx.x < 8) YT[threadIdx.x] = yt_reg;
      __syncthreads();  // the frame's audio is complete
      STAMP(10);
      FRESH_LANE();
      if (threadIdx.x < 24) hi_reg = AU[D + threadIdx.x];  // the next frame's history, before the transposition takes the place
      // ---- interpolate by 2 (48 taps, phase length 24), segment s: inputs n = 4 lane .. 4 lane + 3
      f2 u1[H][4];  // outputs (2n, 2n+1) of input n = 4 lane + u
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const int sg = wv + NWV * h;
        if (sg < R) {
          const float *ib = AU + 256 * sg;
          float w[28];
#pragma unroll
          for (int i = 0; i < 7; ++i) {
            const float4 t = lds4(ib + 4 * lane + 4 * i);
            w[4 * i] = t.x;
            w[4 * i + 1] = t.y;
            w[4 * i + 2] = t.z;
            w[4 * i + 3] = t.w;
          }
          asm volatile("" ::"v"(w[0]));  // (rx512_kernel.hpp: or the 16-byte reads are narrowed to ds_read2_b32 + address adds)
#pragma unroll
          for (int u = 0; u < 4; ++u) u1[h][u] = splat(0.0f);
#pragma unroll
          for (int b = 0; b < 24; b += 8) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
              for (int t = 0; t < 8; ++t) u1[h][u] = pk_fma(splat(w[u + b + t + 1]), f2{ci[2 * b + 1 + 2 * t], ci[2 * b + 2 * t]}, u1[h][u]);
            }
          }
          if (lane == 63) {  // what the next segment's x4 interpolator remembers
            *reinterpret_cast<float4 *>(YT + 8 * (sg + 1)) = make_float4(0.0f, u1[h][0].y, u1[h][1].x, u1[h][1].y);
            *reinterpret_cast<float4 *>(YT + 8 * (sg + 1) + 4) = make_float4(u1[h][2].x, u1[h][2].y, u1[h][3].x, u1[h][3].y);
          }
        }
      }
      float c4[32];  // the x4 interpolator's taps, likewise
      load_taps<32>(c4, (CFloatPtr)cf0, kCoInt2);
      STAMP(11);
      __syncthreads();
      STAMP(12);
      FRESH_LANE();
      if (f == a.nframes4k - 1) {  // the channel's interpolator memories after the call
        if (threadIdx.x < 24) st[kStInt1 + threadIdx.x] = hi_reg;
        else if (threadIdx.x >= 64 && threadIdx.x < 72) st[kStInt2 + threadIdx.x - 64] = YT[8 * R + threadIdx.x - 64];
      }
      // ---- interpolate by 4 (32 taps, phase length 8): inputs n = 8 lane .. 8 lane + 7; volume;
      // LDS transposition (2048 floats of the idle working array per wave); 1-KiB stores
      float *gOf = a.out + ((size_t)ch * a.nframes4k + f) * (size_t)(8 * D);
      float *tr = smem + 2048 * wv;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const int sg = wv + NWV * h;
        if (sg < R) {
          float w[15];
          const float x1[8] = {u1[h][0].x, u1[h][0].y, u1[h][1].x, u1[h][1].y, u1[h][2].x, u1[h][2].y, u1[h][3].x, u1[h][3].y};
#pragma unroll
          for (int i = 0; i < 7; ++i) {
            const float up = lane_up1(x1[i + 1]);
            const float hs = YT[8 * sg + i + 1];
            w[i] = (lane == 0) ? hs : up;
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) w[7 + i] = x1[i];
          wave_sync();  // the buffer's previous readers are done
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            f2 o01 = splat(0.0f), o23 = splat(0.0f);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              const f2 x = splat(w[u + t]);
              o01 = pk_fma(x, f2{c4[4 * t + 3], c4[4 * t + 2]}, o01);
              o23 = pk_fma(x, f2{c4[4 * t + 1], c4[4 * t]}, o23);
            }
            *reinterpret_cast<float4 *>(tr + 4 * (8 * lane + (u ^ (lane & 7)))) = make_float4(o01.x, o01.y, o23.x, o23.y);
          }
          wave_sync();
          float *gO = gOf + 2048 * sg;
          const LaneOff lof = fresh_off(4 * lane);
#pragma unroll
          for (int i = 0; i < 8; ++i) {  // float4 F = 64 i + lane: row F >> 3 = the source lane, column lane & 7
            const int row = 8 * i + (lane >> 3);
            const float4 t = lds4(tr + 4 * (8 * row + ((lane & 7) ^ (row & 7))));
            stg_stream(gO + 256 * i, lof, t);
          }
        }
      }
      if (threadIdx.x < 8) yt_reg = YT[8 * R + threadIdx.x];  // the frame's last x2 outputs: the next frame's history
    }
  }
#ifdef T41RX_STAMP
  STAMP(13);
  {
    unsigned long long rt;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt)::"memory");
    if (lane == 28) stamp_acc = stamp_t0;
    if (lane == 29) stamp_acc = rt;
    unsigned hwid, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (lane == 27) stamp_acc = hwid | ((unsigned long long)(xcc & 0xf) << 32);
  }
  // behind the front kernel's stamps: [nchan][waves][64] uint64
  if (a.dbg_demod)
    reinterpret_cast<unsigned long long *>(a.dbg_demod + (size_t)a.nchan * a.nframes * 256)[(size_t)a.nchan * 64 + ((size_t)ch * NWV + wv) * 64 + lane] = stamp_acc;
#endif
}

// ------------------------------------------------------------------------------------------
// FFT_LENGTH 4096, SSB, f32 samples, AGC off: the WHOLE chain in one kernel.  The two-kernel pipeline
// above moves every decimated sample through HBM once (`mid`: 16 KiB written and 32 KiB read back per
// channel-frame, a quarter more traffic than the path needs) and its front kernel takes longer than
// the fast convolution it feeds.  Here the workgroup that owns a channel's fast convolution also runs
// its front end: wave w takes segments 2w and 2w + 1 of the frame (2 x 2048 input samples) through DC
// high-pass, mixer and the two decimators with the segment-parallel kernel's arithmetic -- a wave
// that does not start the frame rebuilds the filter memories it needs from the 512 input samples in
// front of its first segment (L2-warm: the neighbouring wave is reading them), wave 0 takes them from
// the channel's record, where wave 3 left them at the end of the previous frame -- with its LDS slice
// in the idle working array; the 2 x 256 decimated samples of a wave cross to the radix-8 pass'
// column layout through that array too, and the previous block (the overlap-save "old" half) waits
// in 16 registers per lane in exactly the layout pass 1 wants.  From pass 1 on: fastconv_kernel<8,
// false, true>.  HBM sees the frame once in and once out.
// ------------------------------------------------------------------------------------------
// Register budget: four workgroups per CU hold the kernel to 128 registers.  Measured on MI355X (1024 channels x 32
// frames, us per frame; two-kernel pipeline 57.6): two input sub-blocks in flight + the previous block in registers
// 56.4 (42 registers spilled), two in flight + the previous block in the record 56.4 (13 spilled), ONE in flight + the
// record 54.2 (none spilled); three workgroups per CU (168 registers, nothing spilled, 768 channel slots) 60.6.
// Round 5: with the tap pointers laundered at their base and the wave-index offsets re-derived per phase (FRESH_WV) the
// kernel spills 40 SGPRs instead of 85, and the balance tips: the previous block IN REGISTERS (12 VGPRs spilled, 36 B of
// scratch per lane that stay in L2) measures 51.4-51.6 against 53.1-53.3 us per frame interleaved on one box, and the fabric
// traffic falls from 1.153 to 1.077 x the algorithmic bytes (the 16 KiB round trip through the record is gone):
// profiles/r05_ab_prevreg.txt.  (Round 3, 85 spilled SGPRs, two sub-blocks in flight: 56.4 against 54.2 the other way.)
// (Round 5, measured and left off: the /4 decimator's window tail from registers here too, as in rx512_kernel.hpp: 49.78
// against 49.68 us per frame and one more spilled register, HBM traffic 1.075 -> 1.082 x.)
// The kernel's text is fastconv_fused_kernel.inc, compiled twice: as fastconv_fused_kernel<PLAIN>, and as
// fastconv_fused_map_kernel<PLAIN> for calls behind an input map (receiver groups, t41rx_set_input_map), whose channels
// read row a.in_map[ch] of I / Q -- the runs' pre-rolls with it; the output stays [channel].  Two kernels from one text,
// not one body inlined into two: that compiles the unmapped kernel to another instruction stream (commuted operands, a
// few instructions moved), and a template argument for the switch would rename it.
#define T41RX_FUSED_KERNEL fastconv_fused_kernel
#define T41RX_FUSED_MAP false
#include "fastconv_fused_kernel.inc"
#undef T41RX_FUSED_KERNEL
#undef T41RX_FUSED_MAP
#define T41RX_FUSED_KERNEL fastconv_fused_map_kernel
#define T41RX_FUSED_MAP true
#include "fastconv_fused_kernel.inc"
#undef T41RX_FUSED_KERNEL
#undef T41RX_FUSED_MAP

}  // namespace t41
