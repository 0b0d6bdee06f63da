// t41_sdr_amd/csrc/fastconv_fused_kernel.inc -- the text of the one-kernel FFT_LENGTH 4096 chain (described in
// fastconv_kernels.hpp, which includes it inside namespace t41 once per form): T41RX_FUSED_KERNEL names the kernel,
// T41RX_FUSED_MAP says whether its channels read their antenna samples through an input map.
template <bool PLAIN>
__global__ __launch_bounds__((64 * kFcWaves), kFcWavesPerSimd) void T41RX_FUSED_KERNEL(const RxArgs a) {
  constexpr bool MAP = T41RX_FUSED_MAP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = 8, N = 512 * R, D = N / 2, L = 2048;
  constexpr int NWV = kFcWaves, H = 8 / NWV;
  static_assert(NWV == 4 && H == 2, "written for four waves per channel");
  static_assert(NWV * kLdsFloatsPerWave <= 2 * kFcRow * R, "the front end's slices fit in the working array");
  int lane = threadIdx.x & 63;
  int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (re-defined per phase like `lane`, see FRESH_WV)
  const int ch = blockIdx.x;
  if (ch >= a.nchan) return;
  T41RX_CLK_BEGIN();
  cf *A = reinterpret_cast<cf *>(smem);
  constexpr int kArr = fc_arr_floats(R);
  cf *ltw = reinterpret_cast<cf *>(smem + kArr);
  float *AU = smem;
  float *YT = smem + kFcWaves * 2048;
  float *lds = smem + wv * kLdsFloatsPerWave;  // front end: this wave's slice (X | Y1), inside the working array
  constexpr int kX = 0, kY1 = kXFloats;
  float hi_reg = 0.0f, yt_reg = 0.0f;
  float *st = a.state + (size_t)ch * state_floats(N);
  const cf *twN = reinterpret_cast<const cf *>(a.tab4k);
  const cf *maskN = reinterpret_cast<const cf *>(a.tab4k) + (R - 1) * 512;
  const float2 *__restrict__ tab = a.tab;
  const CoefPtr cf0 = (CoefPtr)a.coef;
  const NcoPtr nco = (NcoPtr)(a.nco + ch);
  const float fixed_gain = cf0->sc[kScFixedGain];
  const float2 hp8 = tab[kTabHp8 + lane];
  const float2 hp4 = tab[kTabHp4 + lane];

  for (int i = threadIdx.x; i < 448; i += 64 * NWV) ltw[i] = reinterpret_cast<const cf *>(tab)[kTabTw1 + i];
  if (threadIdx.x < 56) ltw[448 + threadIdx.x] = reinterpret_cast<const cf *>(tab)[kTabTw2 + 64 * (threadIdx.x >> 3) + (threadIdx.x & 7)];
  if (threadIdx.x < 24) hi_reg = st[kStInt1 + threadIdx.x];
  if (threadIdx.x < 8) yt_reg = st[kStInt2 + threadIdx.x];

  // oscillator: phase at the call's start (the copy the host names), rotation per sample, amplitude loop
  const NcoState *ncs_rd = reinterpret_cast<const NcoState *>(st + kStNco) + a.nco_rd;
  NcoState *ncs_wr = reinterpret_cast<NcoState *>(st + kStNco) + (a.nco_rd ^ 1);
  const uint64_t dphi = uniform_u64(nco->phase_inc);
  const uint64_t phase_call = uniform_u64(ncs_rd->phase);
  double osc_r = uniform_f64(ncs_rd->r);
  bool transient = (wv == 0) && fabs(osc_r * osc_r - uniform_f64(nco->r_star_sq)) > 1e-13;
  // gains (Process.cpp:117-134, 165-166); the DC high-pass takes b0 x
  float g_rf = a.g_rf, iq_phase_neg = 0.0f, iq_phase_pos = 0.0f;
  f2 g_iq = splat(1.0f);
  if (!PLAIN) {
    const float gb = a.g_band;
    const bool iq_on = a.iq_corr_on != 0;
    g_iq = f2{iq_on ? gb * a.neg_iq_amp : gb, gb};
    const float ph = iq_on ? a.iq_phase : 0.0f;
    iq_phase_neg = ph < 0.0f ? ph : 0.0f;
    iq_phase_pos = ph > 0.0f ? ph : 0.0f;
  }
  const float g_rf_i = (PLAIN && a.iq_corr_on) ? -g_rf : g_rf;
  const float g_hp = g_rf * (float)kHpB0;
  const float g_hp_i = (PLAIN && a.iq_corr_on) ? -g_hp : g_hp;

  // the overlap-save "previous" block in pass 1's layout, in registers: element k + 512 p, p < 4, k = lane + 64 (wv + 4 h)
  cf prevx[H][R / 2];
#pragma unroll
  for (int h = 0; h < H; ++h)
#pragma unroll
    for (int p = 0; p < R / 2; ++p)
      prevx[h][p] = reinterpret_cast<const cf *>(st + kStOverlap)[lane + 64 * (wv + NWV * h) + 512 * p];
  cf twp[H][R - 1];
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
  // (a.nframes counts 2048-sample segments.)  MAP: the channel's row of I / Q, read once per wave -- a scalar load, ch is
  // the workgroup's; the host has checked the entry (t41rx_set_input_map)
  typedef const __attribute__((address_space(4))) int *MapPtr;
  const size_t in_base = MAP ? (size_t)((MapPtr)a.in_map)[ch] * (size_t)a.in_chan_stride : (size_t)ch * a.nframes * L;
  const float *gIc = a.I + in_base;
  const float *gQc = a.Q + in_base;

  for (int f = 0; f < a.nframes4k; ++f) {
    FRESH_LANE(); FRESH_WV(wv);
    switch ((4 * f) / a.nframes4k) {
      case 0: PRIO(3); break;
      case 1: PRIO(2); break;
      case 2: PRIO(1); break;
      default: PRIO(0); break;
    }
    __syncthreads();  // the previous frame's back end is done with the working array (first frame: the twiddles are staged)
    // =========================== front end: segments 2 wv, 2 wv + 1 of this frame ===========================
    cf ynew[2][2][2];  // [segment][round][even / odd]: /8 outputs m = 128 round + 2 lane + e of the segment
    {
      const int s0 = R * f + 2 * wv;  // first segment of this wave's run, counted from the call's start
      const float *gI = gIc + (size_t)s0 * L, *gQ = gQc + (size_t)s0 * L;
      uint64_t phase0 = phase_call + (uint64_t)s0 * (uint64_t)L * dphi;
      f2 dc2;
      // ---- filter memories at the start of the run
      auto stage_sub = [&](const float4 &rI0, const float4 &rI1, const float4 &rQ0, const float4 &rQ1, cf (&z)[8]) {
        z[0] = cf{rI0.x * g_hp_i, rQ0.x * g_hp};
        z[1] = cf{rI0.y * g_hp_i, rQ0.y * g_hp};
        z[2] = cf{rI0.z * g_hp_i, rQ0.z * g_hp};
        z[3] = cf{rI0.w * g_hp_i, rQ0.w * g_hp};
        z[4] = cf{rI1.x * g_hp_i, rQ1.x * g_hp};
        z[5] = cf{rI1.y * g_hp_i, rQ1.y * g_hp};
        z[6] = cf{rI1.z * g_hp_i, rQ1.z * g_hp};
        z[7] = cf{rI1.w * g_hp_i, rQ1.w * g_hp};
      };
      auto iq_corr = [&](cf (&z)[8]) {
        if (!PLAIN) {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            z[k] *= g_iq;
            z[k].y = fmaf(iq_phase_neg, z[k].x, z[k].y);
            z[k].x = fmaf(iq_phase_pos, z[k].y, z[k].x);
          }
        }
      };
      // mixer for the 8 samples of this lane whose first one has oscillator phase P (Freq_Shift.cpp:94-141 + :42-65)
      auto mix = [&](cf (&z)[8], uint64_t P, float2 t) {
        const uint32_t u = (uint32_t)(P >> 24);
        const float ang = (float)u * (float)(6.283185307179586476925 / 256.0 / 4294967296.0);
        const float a2 = ang * ang;
        const float sn = ang * fmaf(a2, -1.0f / 6.0f, 1.0f);
        const float cs = fmaf(a2, fmaf(a2, 1.0f / 24.0f, -0.5f), 1.0f);
        const cf base = cmul(cf{t.x, t.y}, cf{cs, sn});
        const NcoPtr ncw = fresh_nco(nco);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const cf osc = cmul_s(base, cf{ncw->wk[k][0], ncw->wk[k][1]});
          z[k] = cmulc(z[k], osc);
        }
      };
      // input registers: one sub-block in flight ahead of the one being worked on (see the register budget above).
      // (Element 0 only: the arrays keep the size of the measured two-in-flight form; with plain float4s hipcc schedules
      // the kernel slightly differently, and this form's machine code is the one that was measured.)
      float4 pI0[2], pI1[2], pQ0[2], pQ1[2];
      auto request = [&](const float *pi, const float *pq) {
        const LaneOff lof = fresh_off(8 * lane);
        pI0[0] = ldg_stream(pi, lof);
        pI1[0] = ldg_stream(pi, lof, 4);
        pQ0[0] = ldg_stream(pq, lof);
        pQ1[0] = ldg_stream(pq, lof, 4);
      };
      float dc_carry = 0.0f;
      if (wv == 0) {
        // the frame's first segment: memories from the channel's record (the call's first frame: as the last call
        // left them) or from the hand-over slot where wave 3 left them at the end of the previous frame (two slots
        // in the `mid` scratch, alternating, so that wave 3 of THIS frame never writes what this wave still reads;
        // its stores were drained before the barrier above, and these loads do not look at this CU's L1)
        const float *src = (f == 0) ? st : a.mid + ((size_t)ch * 2 + ((f - 1) & 1)) * 256;
        request(gI, gQ);
        float4 h1 = any_float4(), h2 = any_float4();
        const LaneOff lo4 = fresh_off(4 * lane);
        if (lane < 14) h1 = ldg_stream(src + kStDec1, lo4);
        if (lane < 24) h2 = ldg_stream(src + kStDec2, lo4);
        const float4 dcs = ldg_stream(src + kStMisc);  // (kMiscDc first)
        wave_sync();
        if (lane < 14) *reinterpret_cast<float4 *>(lds + kX + 2 * xpad(2 * lane)) = h1;
        if (lane < 24) *reinterpret_cast<float4 *>(lds + kY1 + y1slot(lane)) = h2;
        wave_sync();
        dc_carry = uniform_f32(dcs.x);
      } else {
        // pre-roll: the 512 samples in front of the run through DC high-pass, mixer and /4 decimator
        request(gI - 512, gQ - 512);
        cf z[8];
        stage_sub(pI0[0], pI1[0], pQ0[0], pQ1[0], z);
        request(gI, gQ);
        f2 dcs = splat(0.0f);
        dc_highpass<8>(z, dcs, lane, hp8.x, hp8.y);  // from rest: 512 samples on, its memory of the start is a1^512
        iq_corr(z);
        {
          const uint64_t P = phase0 - (uint64_t)(511 - 8 * lane) * dphi;
          mix(z, P, ldg2(tab + kTabSinCos, (unsigned)(P >> 56)));
        }
        wave_sync();
        float *xw = lds + kX + 20 * lane;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<float4 *>(xw + 2 * (xpad(28 + 2 * i))) = make_float4(z[2 * i].x, z[2 * i].y, z[2 * i + 1].x, z[2 * i + 1].y);
        wave_sync();
        cf o1[2];
        auto pidx = [](int o) { return xpad(o); };
        fir_pair<kDec1Taps, 1, 5, 18, 6>(xw, pidx, cf0, kCoDec1, o1[0], o1[1]);
        float4 hh = any_float4();
        if (lane < 14) hh = lds4(lds + kX + 2 * xpad(512 + 2 * lane));
        wave_sync();
        if (lane < 14) *reinterpret_cast<float4 *>(lds + kX + 2 * xpad(2 * lane)) = hh;
        if (lane >= 40) *reinterpret_cast<float4 *>(lds + kY1 + y1slot(lane - 40)) = make_float4(o1[0].x, o1[0].y, o1[1].x, o1[1].y);
        wave_sync();
        dc2 = dcs;  // inside a frame both chains of the shared biquad simply run on
      }
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        if (wv == 0 && sg == 0) {
          // Q's DC-block start state = the state after ALL of the frame's I (one shared instance runs over I then Q,
          // Process.cpp:127-128): a1^256 ~ 3e-18, so the frame's last 256 I samples decide it
          const float4 tailF = ldg4(gI + (R * L - 256), fresh_off(4 * lane));
          const float x[4] = {tailF.x * g_rf, tailF.y * g_rf, tailF.z * g_rf, tailF.w * g_rf};
          dc2 = f2{(g_rf_i != g_rf) ? -dc_carry : dc_carry, dc_highpass_end_state<4>(x, hp4.x, hp4.y)};
        }
        float2 osc_tab[4];
        uint64_t osc_p[4];  // (rx512_kernel.hpp: unsigned sample numbers, the sub-block's part of the phase scalar)
        {
          const uint64_t Pl = (uint64_t)(unsigned)(8 * lane + 1) * dphi;
#pragma unroll
          for (int sb = 0; sb < 4; ++sb) {
            osc_p[sb] = (phase0 + (uint64_t)(512 * sb) * dphi) + Pl;
            osc_tab[sb] = ldg2(tab + kTabSinCos, (unsigned)(osc_p[sb] >> 56));
          }
        }
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
#pragma unroll
          for (int hh2 = 0; hh2 < 2; ++hh2) {
            const int sb = 2 * rd + hh2;
            cf z[8];
            stage_sub(pI0[0], pI1[0], pQ0[0], pQ1[0], z);
            // the next sub-block (this segment's, or the run's second segment's)
            if (!(sg == 1 && sb == 3)) request(gI + L * sg + 512 * (sb + 1), gQ + L * sg + 512 * (sb + 1));
            dc_highpass<8>(z, dc2, lane, hp8.x, hp8.y);
            iq_corr(z);
            if (transient) {  // start-up of the oscillator's amplitude loop (Freq_Shift.cpp:130-134), first samples after a reset
              const NcoPtr nt = fresh_nco(nco);
              const double r_star_sq = uniform_f64(nt->r_star_sq);
              const double w_abs = uniform_f64(nt->w_abs);
              const double inv_r = 1.0 / sqrt(r_star_sq);
              double r = osc_r;
              float amp[8];
#pragma unroll
              for (int k = 0; k < 8; ++k) amp[k] = 1.0f;
              for (int g = 0; g < 64; ++g) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                  if (g == lane) amp[k] = (float)(r * inv_r);
                  r = r * (1.95 - r * r) * w_abs;
                }
                if (fabs(r * r - r_star_sq) <= 1e-13) break;
              }
              osc_r = r;
              transient = fabs(osc_r * osc_r - r_star_sq) > 1e-13;
#pragma unroll
              for (int k = 0; k < 8; ++k) z[k] *= splat(amp[k]);
            }
            mix(z, osc_p[sb], osc_tab[sb]);
            wave_sync();
            float *xw = lds + kX + 20 * lane;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              *reinterpret_cast<float4 *>(xw + 2 * (xpad(28 + 2 * i))) = make_float4(z[2 * i].x, z[2 * i].y, z[2 * i + 1].x, z[2 * i + 1].y);
            wave_sync();
            cf o1[2];
            {
              auto pidx = [](int o) { return xpad(o); };
              fir_pair<kDec1Taps, 1, 5, 18, 6>(xw, pidx, cf0, kCoDec1, o1[0], o1[1]);
            }
            {
              float4 hh = any_float4();
              if (lane < 14) hh = lds4(lds + kX + 2 * xpad(512 + 2 * lane));
              wave_sync();
              if (lane < 14) *reinterpret_cast<float4 *>(lds + kX + 2 * xpad(2 * lane)) = hh;
              *reinterpret_cast<float4 *>(lds + kY1 + y1slot(24 + 64 * hh2 + lane)) = make_float4(o1[0].x, o1[0].y, o1[1].x, o1[1].y);
            }
          }
          wave_sync();
          {
            auto planes = [](int o) { return y1slot(o >> 1) / 2; };
            fir_pair<kDec2Taps, 3, 5, 26, 6>(lds + kY1 + 4 * lane, planes, cf0, kCoDec2, ynew[sg][rd][0], ynew[sg][rd][1]);
          }
          {
            float4 hh = any_float4();
            if (lane < 24) hh = lds4(lds + kY1 + y1slot(128 + lane));
            wave_sync();
            if (lane < 24) *reinterpret_cast<float4 *>(lds + kY1 + y1slot(lane)) = hh;
          }
        }
        phase0 += (uint64_t)L * dphi;
      }
      if (wv == NWV - 1) {
        // the frame ends here: the memories the next frame's first segment starts from (and, behind the call's last
        // frame, the channel's state) go to the record; the shared DC biquad ends the frame on Q
        wave_sync();
        float *dst = (f == a.nframes4k - 1) ? st : a.mid + ((size_t)ch * 2 + (f & 1)) * 256;
        if (lane < 14) *reinterpret_cast<float4 *>(dst + kStDec1 + 4 * lane) = lds4(lds + kX + 2 * xpad(2 * lane));
        if (lane < 24) *reinterpret_cast<float4 *>(dst + kStDec2 + 4 * lane) = lds4(lds + kY1 + y1slot(lane));
        if (lane == 0) dst[kStMisc + kMiscDc] = uniform_f32(dc2.y);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // in L2 before the next frame's barrier lets wave 0 read them
      }
    }
    __syncthreads();  // every wave is done with its slice: the array takes the new block in time order
    FRESH_LANE(); FRESH_WV(wv);
    {
      cf *Nb = reinterpret_cast<cf *>(smem);  // new block: sample n = 256 s + m at Nb[n]
#pragma unroll
      for (int sg = 0; sg < 2; ++sg)
#pragma unroll
        for (int rd = 0; rd < 2; ++rd)
          *reinterpret_cast<float4 *>(smem + 2 * (256 * (2 * wv + sg) + 128 * rd + 2 * lane)) =
              make_float4(ynew[sg][rd][0].x, ynew[sg][rd][0].y, ynew[sg][rd][1].x, ynew[sg][rd][1].y);
      __syncthreads();
      cf x1[H][R];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const int k = lane + 64 * (wv + NWV * h);
#pragma unroll
        for (int p = 0; p < R / 2; ++p) {
          x1[h][p] = prevx[h][p];
          x1[h][R / 2 + p] = Nb[k + 512 * p];
        }
      }
      load_twp();
      __syncthreads();  // the new block is in registers everywhere: pass 1 may write the array
      FRESH_LANE(); FRESH_WV(wv);
      // ---- pass 1
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const int k = lane + 64 * (wv + NWV * h);
        cf v[R];
#pragma unroll
        for (int p = 0; p < R; ++p) v[p] = x1[h][p];
#pragma unroll
        for (int p = 0; p < R / 2; ++p) prevx[h][p] = x1[h][R / 2 + p];  // next frame's "previous"
        if (f == a.nframes4k - 1) {
#pragma unroll
          for (int p = R / 2; p < R; ++p) reinterpret_cast<cf *>(st + kStOverlap)[k + 512 * p - D] = v[p];
        }
        dft_r<R, false>(v);
#pragma unroll
        for (int q = 1; q < R; ++q) v[q] = cmul(v[q], twp[h][q - 1]);
#pragma unroll
        for (int q = 0; q < R; ++q) A[k + kFcRow * q] = v[q];
      }
    }
    cf mk[H][8];
    const LaneOff lom = fresh_off(2 * lane);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int q = wv + NWV * h;
#pragma unroll
      for (int r = 0; r < 8; ++r) mk[h][r] = ldg_cf(maskN + 512 * q, lom, 64 * r);
    }
    __syncthreads();
    FRESH_LANE(); FRESH_WV(wv);
    // ---- pass 2: the wave's two rows in lockstep
    {
      const int q0 = wv, q1 = wv + NWV;
      cf v[8], u[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = A[kFcRow * q0 + lane + 64 * r];
#pragma unroll
      for (int r = 0; r < 8; ++r) u[r] = A[kFcRow * q1 + lane + 64 * r];
      float *xv = smem + 2 * kFcRow * q0, *xu = smem + 2 * kFcRow * q1;
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
    }
    load_twp();
    __syncthreads();
    FRESH_LANE(); FRESH_WV(wv);
    // ---- pass 3; fixed gain (DSP_Fn.cpp:494-502); SSB: audio = Re of the valid half
    float y3[H][R / 2];
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
      for (int p = R / 2; p < R; ++p) y3[h][p - R / 2] = fixed_gain * v[p].x;
    }
    {
      float ci[48];
      load_taps<48>(ci, (CFloatPtr)cf0, kCoInt1);
      __syncthreads();
      FRESH_LANE(); FRESH_WV(wv);
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int j = 0; j < R / 2; ++j) AU[24 + lane + 64 * (wv + NWV * h) + 512 * j] = y3[h][j];
      if (threadIdx.x < 24) AU[threadIdx.x] = hi_reg;
      if (threadIdx.x < 8) YT[threadIdx.x] = yt_reg;
      __syncthreads();
      FRESH_LANE(); FRESH_WV(wv);
      if (threadIdx.x < 24) hi_reg = AU[D + threadIdx.x];
      f2 u1[H][4];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const int sg = wv + NWV * h;
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
        if (lane == 63) {
          *reinterpret_cast<float4 *>(YT + 8 * (sg + 1)) = make_float4(0.0f, u1[h][0].y, u1[h][1].x, u1[h][1].y);
          *reinterpret_cast<float4 *>(YT + 8 * (sg + 1) + 4) = make_float4(u1[h][2].x, u1[h][2].y, u1[h][3].x, u1[h][3].y);
        }
      }
      float c4[32];
      load_taps<32>(c4, (CFloatPtr)cf0, kCoInt2);
      __syncthreads();
      FRESH_LANE(); FRESH_WV(wv);
      if (f == a.nframes4k - 1) {
        if (threadIdx.x < 24) st[kStInt1 + threadIdx.x] = hi_reg;
        else if (threadIdx.x >= 64 && threadIdx.x < 72) st[kStInt2 + threadIdx.x - 64] = YT[8 * R + threadIdx.x - 64];
      }
      float *gOf = a.out + ((size_t)ch * a.nframes4k + f) * (size_t)(8 * D);
      float *tr = smem + 2048 * wv;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const int sg = wv + NWV * h;
        float w[15];
        const float x1v[8] = {u1[h][0].x, u1[h][0].y, u1[h][1].x, u1[h][1].y, u1[h][2].x, u1[h][2].y, u1[h][3].x, u1[h][3].y};
        // (the segment's eight history words as two 16-byte reads; [0] is padding and is kept alive on purpose --
        // rx512_kernel.hpp, x2 window: without it the reads are narrowed to ds_read2_b32 at one address register each)
        const float4 ya = lds4(YT + 8 * sg), yb = lds4(YT + 8 * sg + 4);
        asm volatile("" ::"v"(ya.x));
        const float hsv[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const float up = lane_up1(x1v[i + 1]);
          w[i] = (lane == 0) ? hsv[i + 1] : up;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) w[7 + i] = x1v[i];
        wave_sync();
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
        for (int i = 0; i < 8; ++i) {
          const int row = 8 * i + (lane >> 3);
          const float4 t = lds4(tr + 4 * (8 * row + ((lane & 7) ^ (row & 7))));
          stg_stream(gO + 256 * i, lof, t);
        }
      }
      if (threadIdx.x < 8) yt_reg = YT[8 * R + threadIdx.x];
    }
  }
  // the oscillator after the call (the other copy: see rx512_kernel)
  if (threadIdx.x == 0) {
    ncs_wr->phase = phase_call + (uint64_t)a.nframes * (uint64_t)L * dphi;
    ncs_wr->r = osc_r;
  }
  T41RX_CLK_END(ch * NWV + wv);
}
