// t41_sdr_amd/csrc/nrspec_body.inc -- the text of Kim1_NR() / SpectralNoiseReduction() on one channel, one wave: the body of
// nrspec_kernel<KIND> behind its first lines, included once there and twice by nrspec_map_kernel (nr_kernels.hip), once
// per kind under a wave-uniform branch.  The including scope provides the constant KIND (1 or 2), the argument block `a`,
// `lane`, the channel `ch` and the LDS of nrspec_lds.inc.  Text, not a function called by two kernels: an argument
// block handed on by reference compiles to another instruction stream (anr_kernel.inc), and nrspec_kernel<1> / <2> must
// stay the streams they were.
  float *st = a.spec + (size_t)ch * kNrSpecFloats;
  const float *win = a.tab_nr + (KIND == 1 ? kNrTabHann : kNrTabSqrtHann);
  const cf *tab = reinterpret_cast<const cf *>(a.tab);
  cf tw1[7], tw2[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    tw1[q] = tab[kTabTw1 + 64 * q + lane];
    tw2[q] = tab[kTabTw2 + 64 * q + lane];
  }
  // ---- the channel's record -> LDS
  if (KIND == 1) {
    for (int i = lane; i < 3 * 128; i += 64) (&Xs[0][0])[i] = st[kNrX + i];
    for (int i = lane; i < 15 * 128; i += 64) (&Es[0][0])[i] = st[kNrE + i];
  }
  if (lane < 8) {
    GstP[lane] = 0.0f;
    GstP[8 + 128 + lane] = 0.0f;
  }
  for (int i = lane; i < 128; i += 64) {
    if (KIND == 1) {
      Gts1[i] = st[kNrGts1 + i];
      Gts0[i] = st[kNrGts0 + i];
    }
    Gst[i] = st[kNrG + i];
    S[i] = st[kNrLastIn + i];
    Lout[i] = st[kNrLastOut + i];
    Nest[i] = st[kNrNest + i];
    Pslp[i] = st[kNrPslp + i];
    Xt[i] = st[kNrXt + i];
    Hk[i] = st[kNrHk + i];
  }
  float lastX[2] = {0.0f, 0.0f};
  int xp = (int)st[kNrScal + 0], ep = (int)st[kNrScal + 1], first_time_2 = (int)st[kNrScal + 2], init_counter = (int)st[kNrScal + 3];
  const int lo = a.vad_lo, hi = a.vad_hi;
  const float NR_alpha = a.alpha, NR_beta = a.beta, NR_PSI = a.psi;
  __syncthreads();

  // SpectralNoiseReduction()'s per-call constants and statics (Noise.cpp:394-419)
  const float tinc = 0.00533333, tax = 0.0239, tap = 0.05062, psthr = 0.99, pnsaf = 0.01, asnr = 20, psini = 0.5, pspri = 0.5;
  const float ax = expf(-tinc / tax), ap = expf(-tinc / tap);
  const float xih1 = powf(10, (float)asnr / 10.0);
  const float xih1r = 1.0 / (1.0 + xih1) - 1.0;
  const float pfac = (1.0 / pspri - 1.0) * (1.0 + xih1);
  const float snr_prio_min = powf(10, -(float)20 / 20.0);
  const float power_threshold = 0.4;
  const int NR_width = 4;

  if (KIND == 2 && first_time_2 == 1) {  // Noise.cpp:439-450
    for (int i = lane; i < 128; i += 64) {
      S[i] = 0.0;
      Gst[i] = 1.0;
      Hk[i] = 1.0;
      Nest[i] = 0.0;
      Pslp[i] = 0.5;
    }
    first_time_2 = 2;
    __syncthreads();
  }

  float *gio = a.aud + (size_t)ch * a.nframes * 256;
  for (int f = 0; f < a.nframes; ++f) {
    // ---- the block, behind the previous block's second half
#pragma unroll
    for (int q = 0; q < 4; ++q) S[128 + lane + 64 * q] = gio[(size_t)f * 256 + lane + 64 * q];
    __syncthreads();
    // ---- both frames through one transform: z[n] = w[n] (S[n] + j S[128 + n]), zero-interleaved
    cf v[8];
    {
      const int m = lane >> 1;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int n = m + 32 * r;
        const float wn = win[n];
        const cf z = cf{S[n] * wn, S[128 + n] * wn};
        v[r] = (lane & 1) ? cf{0.0f, 0.0f} : z;
      }
    }
    __syncthreads();
    if (lane < 64) {  // the second half becomes NR_last_sample_buffer_L
      S[lane] = S[256 + lane];
      S[64 + lane] = S[320 + lane];
    }
    fft512<false>(v, tw1, tw2, xbuf, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) Zs[lane + 64 * r] = v[r];
    if (lane == 0) Zs[256] = v[0];
    __syncthreads();
    // ---- separate: F0[k] = (Z[k] + conj Z[256-k]) / 2, F1[k] = (Z[k] - conj Z[256-k]) / 2j; bins lane, lane + 64
    cf F[2][2];     // [frame][r]
    float X[2][2];  // squared magnitudes
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int k = lane + 64 * r;
      const cf za = Zs[k], zp = Zs[256 - k];
      F[0][r] = cf{0.5f * (za.x + zp.x), 0.5f * (za.y - zp.y)};
      F[1][r] = cf{0.5f * (za.y + zp.y), -0.5f * (za.x - zp.x)};
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) X[k2][r] = F[k2][r].x * F[k2][r].x + F[k2][r].y * F[k2][r].y;
    }
    const cf z128 = Zs[128];  // F0[128] = Re, F1[128] = Im
    if (KIND == 2) {  // NR_X[bindx][0] as the call's last half-block leaves it (Noise.cpp:478), for the record
      lastX[0] = X[1][0];
      lastX[1] = X[1][1];
    }
    bool proc[2] = {true, true};
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      float G[2] = {0.0f, 0.0f};  // this frame's NR_G for my two bins
      if (KIND == 1) {
        // ---- Kim1_NR(), Noise.cpp:197-257
        const float NR_KIM_K = 1.0;
        const float NR_onemalpha = (1.0 - NR_alpha);
        const float NR_onemtwobeta = (1.0 - (2.0 * NR_beta));
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int i = lane + 64 * r;
          Xs[xp][i] = X[k2][r];
          if (i >= lo && i < hi) {
            float NR_sum = 0.0;
            NR_sum = NR_sum + Xs[0][i];
            NR_sum = NR_sum + Xs[1][i];
            NR_sum = NR_sum + Xs[2][i];
            const float E = NR_sum / (float)3;
            Es[ep][i] = E;
            float M = Es[0][i];
            for (int j = 1; j < 15; ++j)
              if (Es[j][i] < M) M = Es[j][i];
            const float NR_T = X[k2][r] / M;
            const float lambda = (NR_T > NR_PSI) ? M : E;
            float g = (float)(1.0 - (double)(lambda * NR_KIM_K / E));
            if (g < 0.0f) g = 0.0f;
            const float gts = NR_alpha * Gts1[i] + NR_onemalpha * g;
            Gts0[i] = gts;
            Gts1[i] = gts;
          }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int i = lane + 64 * r;
          if (i == 0) G[r] = (NR_onemtwobeta + NR_beta) * Gts0[0] + NR_beta * Gts0[1];
          else if (i == 127) G[r] = NR_beta * Gts0[126] + (NR_onemtwobeta + NR_beta) * Gts0[127];
          else G[r] = NR_beta * Gts0[i - 1] + NR_onemtwobeta * Gts0[i] + NR_beta * Gts0[i + 1];
        }
        xp = (xp + 1 >= 3) ? 0 : xp + 1;
        ep = (ep + 1 >= 15) ? 0 : ep + 1;
      } else {
        // ---- SpectralNoiseReduction(), Noise.cpp:476-601
        if (first_time_2 == 2) {
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            const float ne = (float)((double)Nest[i] + 0.05 * (double)X[k2][r]);
            Nest[i] = ne;
            Xt[i] = psini * ne;
          }
          init_counter++;
          if (init_counter > 19) {
            init_counter = 0;
            first_time_2 = 3;
          }
        }
        proc[k2] = (first_time_2 == 3);
        if (first_time_2 == 3) {
          float post[2], prio[2];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            const float x = X[k2][r];
            float xt = Xt[i];
            float ph1y = (float)(1.0 / (1.0 + (double)(pfac * expf(xih1r * x / xt))));
            const float ps = (float)((double)(ap * Pslp[i]) + (1.0 - (double)ap) * (double)ph1y);
            Pslp[i] = ps;
            if (ps > psthr) ph1y = (float)(1.0 - (double)pnsaf);
            else ph1y = (float)fmin((double)ph1y, 1.0);
            const float xtr = (float)((1.0 - (double)ph1y) * (double)x + (double)(ph1y * xt));
            xt = (float)((double)(ax * xt) + (1.0 - (double)ax) * (double)xtr);
            Xt[i] = xt;
            post[r] = (float)fmax(fmin((double)(x / xt), 1000.0), (double)snr_prio_min);
            prio[r] = (float)fmax((double)(NR_alpha * Hk[i]) + (1.0 - (double)NR_alpha) * fmax((double)post[r] - 1.0, 0.0), 0.0);
          }
          // the gain each bin receives in its own pass of the loop below depends on its two SNRs alone (Noise.cpp:531-535):
          // computed here for both of the lane's bins, so that the bin-by-bin loop only moves values
          float gnew[2], hknew[2];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const float vv = (float)((double)(prio[r] * post[r]) / (1.0 + (double)prio[r]));
            gnew[r] = (float)(1.0 / (double)post[r] * (double)sqrtf((float)(0.7212 * (double)vv + (double)(vv * vv))));
            hknew[r] = post[r] * gnew[r] * gnew[r];
          }
          __syncthreads();
          // pre_power: the same sum in every pass of the loop below
          float pre_part = 0.0f;
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            if (i >= lo && i < hi) pre_part += X[k2][r];
          }
          const float pre_power = wave_sum(pre_part);
          // Round 5.  The loop is serial by construction (every pass sees the gains the previous pass's smoothing left)
          // and the four waves of a SIMD keep its VALU busy: what a pass costs is its VALU instructions.  Round 4 kept
          // the gains in LDS and spent ~140 of them per pass; this form spends ~40:
          //  * the lane's two gains live in registers (Gr); bins 64..127 are left out of the loop when the pass band
          //    ends below bin 64 (wave-uniform: it does for every filter up to 6 kHz);
          //  * a pass that smooths publishes the gains once and requests its whole window in one go from a padded array
          //    (no address clamps), the centred and the upper-edge average are summed from registers in the reference's
          //    order, and s / NN is the correctly rounded quotient from a multiplication and two FMAs (NN is 3, 5, 7 or 9
          //    and 1 / NN is correctly rounded: Markstein's theorem; checked on 64 M quotients per divisor);
          //  * the power ratio only ever decides NN, which changes at 0.4, 0.35, 0.25, 0.15 and 0.05: away from those
          //    (5e-5, bit patterns compared on the scalar unit) post_power x (1 / pre_power) decides, next to one of
          //    them round 4's decision code runs as it was (true quotient, the reference's summation order), so NN is
          //    decided exactly as before;
          //  * the wave sum's six steps are six fused DPP additions.
          // The same additions in the same order as the reference's loops: outputs and records are bit-identical to
          // round 4's (tools/anr_ab_check.py).
          float Gr[2] = {Gst[lane], Gst[64 + lane]};
          const bool r1_live = hi > 64;
          const bool in0 = lane >= lo && lane < hi, in1 = lane + 64 >= lo && lane + 64 < hi;
          const float inv_pre = 1.0f / pre_power;
          for (int i = lo; i < hi; ++i) {  // Noise.cpp:529-588: the musical-noise treatment runs inside this loop
            {
              const bool me = lane == (i & 63);
              if (i >> 6) Gr[1] = me ? gnew[1] : Gr[1];
              else Gr[0] = me ? gnew[0] : Gr[0];
            }
            float post_part = in0 ? Gr[0] * Gr[0] * X[k2][0] : 0.0f;
            if (r1_live) post_part = in1 ? post_part + Gr[1] * Gr[1] * X[k2][1] : post_part;
            const float post_power = wave_sum_fused(post_part);
            int NN;
            // (read into a scalar register by hand: through the builtin the compiler keeps the value in a VGPR and does
            // the ten comparisons below on the VALU)
            unsigned rb;
            asm volatile("s_nop 0\n\tv_readfirstlane_b32 %0, %1" : "=s"(rb) : "v"(post_power * inv_pre));
            if (!nr_ratio_near_edge(rb)) {
              NN = rb > fbits(0.35f) ? 1 : rb > fbits(0.25f) ? 3 : rb > fbits(0.15f) ? 5 : rb > fbits(0.05f) ? 7 : 9;
            } else {
              float power_ratio = post_power / pre_power;
              // The reference adds both sums up bin by bin in float (Noise.cpp:542-546); the tree sums above differ from
              // that by rounding only.  Next to an edge the sums are redone in the reference's order (every lane, the same
              // values through LDS), so NN is decided exactly as the scalar code decides it.
              bool near_edge = false;
#pragma unroll
              for (float b : {0.4f, 0.35f, 0.25f, 0.15f, 0.05f}) near_edge = near_edge || fabsf(power_ratio - b) < 4e-5f;
              if (near_edge) {
                float *Pw = U + 640;  // (free between the transforms: the spectra occupy U[0 .. 520))
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                  const int j = lane + 64 * r;
                  Pw[j] = X[k2][r];
                  Pw[128 + j] = Gr[r] * Gr[r] * X[k2][r];
                }
                __syncthreads();
                float pre_seq = 0.0f, post_seq = 0.0f;
                for (int j = lo; j < hi; ++j) {
                  pre_seq += Pw[j];
                  post_seq += Pw[128 + j];
                }
                power_ratio = post_seq / pre_seq;
                __syncthreads();
              }
              if (power_ratio > power_threshold) {
                power_ratio = 1.0;
                NN = 1;
              } else {
                NN = 1 + 2 * (int)(0.5 + (double)NR_width * (1.0 - (double)(power_ratio / power_threshold)));
              }
            }
            if (NN > 1) {
              // centred average over NN bins; the reference's upper-edge pass (a backward average) overwrites the
              // centred value of the last NN - NN/2 inner bins before the copy back (Noise.cpp:556-584)
              Gst[lane] = Gr[0];
              if (r1_live) Gst[64 + lane] = Gr[1];
              lds_fence();  // (one wave: its LDS operations execute in program order)
              if (NN <= 9) {
                auto smooth = [&](auto nn_tag) {
                  constexpr int N = decltype(nn_tag)::value, H = N / 2;
                  constexpr float rN = 1.0f / (float)N;
#pragma unroll
                  for (int r = 0; r < 2; ++r) {
                    if (r == 1 && !r1_live) continue;
                    const int j = lane + 64 * r;
                    float g[N + H];  // g[t] = NR_G[j - N + 1 + t]
#pragma unroll
                    for (int t = 0; t < N + H; ++t) g[t] = Gst[j - N + 1 + t];
                    float sc = 0.0, sb = 0.0;
#pragma unroll
                    for (int m = -H; m <= H; ++m) sc += g[N - 1 + m];     // m = j - h .. j + h
#pragma unroll
                    for (int m = 0; m > -N; --m) sb += g[N - 1 + m];      // m = j .. j - NN + 1
                    const float sm = (j >= hi - N) ? sb : sc;
                    const float q0 = sm * rN;
                    const float nv = fmaf(fmaf(-q0, (float)N, sm), rN, q0);  // = sm / (float)N, correctly rounded
                    if (j >= lo + H && j < hi - H) Gr[r] = nv;
                  }
                };
                switch (NN) {
                  case 3: smooth(std::integral_constant<int, 3>{}); break;
                  case 5: smooth(std::integral_constant<int, 5>{}); break;
                  case 7: smooth(std::integral_constant<int, 7>{}); break;
                  default: smooth(std::integral_constant<int, 9>{}); break;
                }
              } else {  // (not reachable with NR_width = 4 and a ratio >= 0; kept as the reference's loops)
                Gst[64 + lane] = Gr[1];
                lds_fence();
                const int h = NN / 2;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                  const int j = lane + 64 * r;
                  if (j >= lo + h && j < hi - h) {
                    float sm = 0.0;
                    if (j >= hi - NN) {
                      for (int m = j; m > j - NN; --m) sm += Gst[m];
                    } else {
                      for (int m = j - h; m <= j + h; ++m) sm += Gst[m];
                    }
                    Gr[r] = sm / (float)NN;
                  }
                }
              }
              lds_fence();
            }
          }
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            Gst[i] = Gr[r];
            if (i >= lo && i < hi) Hk[i] = hknew[r];
          }
          __syncthreads();
#pragma unroll
          for (int r = 0; r < 2; ++r) G[r] = Gst[lane + 64 * r] * 1.0f;  // x NR_long_tone_gain (1.0, Noise.cpp:706)
        }
      }
      // ---- this frame's weighted spectrum, conjugate-symmetrised: bin k by (G[k] + G[k-1]) / 2 (bin 0: G[0]; 128: G[127])
      __syncthreads();
      Gb[1 + lane] = G[0];
      Gb[65 + lane] = G[1];
      __syncthreads();
      cf *Wk = k2 ? W1 : W0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int k = lane + 64 * r;
        const float g = (k == 0) ? Gb[1] : 0.5f * (Gb[1 + k] + Gb[k]);
        Wk[k] = (k == 0) ? cf{F[k2][r].x * g, 0.0f} : cf{F[k2][r].x * g, F[k2][r].y * g};
      }
      if (lane == 0) Wk[128] = cf{(k2 ? z128.y : z128.x) * Gb[128], 0.0f};
      __syncthreads();
    }
    // ---- one inverse transform for both frames: V[k] = W0[k] + j W1[k], V[256 - k] = conj W0[k] + j conj W1[k]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = lane + 64 * r;
      const int kk = (k <= 128) ? k : 256 - k;
      const cf a0 = W0[kk], a1 = W1[kk];
      const float sg = (k <= 128) ? 1.0f : -1.0f;
      // a0 (+-conj) + j a1 (+-conj): re = a0.x - sg a1.y, im = sg a0.y + a1.x
      v[r] = cf{a0.x - sg * a1.y, sg * a0.y + a1.x};
      v[r + 4] = v[r];
    }
    fft512<true>(v, tw1, tw2, xbuf, lane);
    if (!(lane & 1)) {
      const int m = lane >> 1;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int n = m + 32 * r;
        const float sw = (KIND == 2) ? win[n] : 1.0f;  // the spectral function windows again after the inverse transform
        Y0[n] = v[r].x * (1.0f / 512.0f) * sw;
        Y1[n] = v[r].y * (1.0f / 512.0f) * sw;
      }
    }
    __syncthreads();
    // ---- overlap-add (Noise.cpp:289-296 / 640-647), Kim: x 30 (Process.cpp:846)
    {
      float o[4];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int i = lane + 64 * q;
        const float l0 = Lout[i];
        float first, l1;
        if (proc[0]) {
          first = Y0[i] + l0;
          l1 = Y0[128 + i];
        } else {
          first = gio[(size_t)f * 256 + i];
          l1 = l0;
        }
        float second, l2;
        if (proc[1]) {
          second = Y1[i] + l1;
          l2 = Y1[128 + i];
        } else {
          second = gio[(size_t)f * 256 + 128 + i];
          l2 = l1;
        }
        Lout[i] = l2;
        o[q] = (KIND == 1) ? first * 30.0f : first;
        o[2 + q] = (KIND == 1) ? second * 30.0f : second;
      }
      gio[(size_t)f * 256 + lane] = o[0];
      gio[(size_t)f * 256 + 64 + lane] = o[1];
      gio[(size_t)f * 256 + 128 + lane] = o[2];
      gio[(size_t)f * 256 + 192 + lane] = o[3];
    }
    __syncthreads();
  }
  // ---- the record back
  if (KIND == 1) {
    for (int i = lane; i < 3 * 128; i += 64) st[kNrX + i] = (&Xs[0][0])[i];
    for (int i = lane; i < 15 * 128; i += 64) st[kNrE + i] = (&Es[0][0])[i];
  } else if (a.nframes > 0) {
    // the spectral function stores NR_X[.][0] every frame and never touches NR_X[.][1..2] or NR_E: what Kim1_NR()'s
    // three-frame average starts from after a live switch of nrOptionSelect from 2 to 1, as in the firmware
    st[kNrX + lane] = lastX[0];
    st[kNrX + 64 + lane] = lastX[1];
  }
  for (int i = lane; i < 128; i += 64) {
    if (KIND == 1) {
      st[kNrGts1 + i] = Gts1[i];
      st[kNrGts0 + i] = Gts0[i];
    }
    st[kNrG + i] = Gst[i];
    st[kNrLastIn + i] = S[i];
    st[kNrLastOut + i] = Lout[i];
    st[kNrNest + i] = Nest[i];
    st[kNrPslp + i] = Pslp[i];
    st[kNrXt + i] = Xt[i];
    st[kNrHk + i] = Hk[i];
  }
  if (lane == 0) {
    st[kNrScal + 0] = (float)xp;
    st[kNrScal + 1] = (float)ep;
    st[kNrScal + 2] = (float)first_time_2;
    st[kNrScal + 3] = (float)init_counter;
  }
