// t41_sdr_amd/csrc/ft8_block.inc -- the text of process_FT8_FFT()'s extract_power() (ft8.cpp:223-256) on a channel's buffer in
// LDS (described in ft8_kernel.hip, which includes it once per kernel): the 1472 bytes of one block to `row`.  It reads the
// including kernel's a.window / a.mag_db / a.tab, sbuf, tw, t and NT, works in its fz, nat and mg, and ends on a barrier; the
// kernel has a barrier between its last write to sbuf and this text.
  for (int ts = 0; ts < 2; ++ts) {
    // window_ft8_dsp_buffer[i] = (q15_t)((float)ft8_dsp_buffer[i + time_sub] * window[i]); point p = samples 2p, 2p + 1
    for (int p = t; p < 1024; p += NT) {
      const float2 wv = reinterpret_cast<const float2 *>(a.window)[p];
      const int re = (int)((float)sbuf[2 * p + 512 * ts] * wv.x), im = (int)((float)sbuf[2 * p + 1 + 512 * ts] * wv.y);
      fz[sw(p)] = pack(Cq{re, im});
    }
    __syncthreads();
    // first stage: inputs >> 2; outputs b and c stored swapped, here and in every stage (arm_radix4_butterfly_q15)
    for (int j = t; j < 256; j += NT) {
      const Cq A = shr(unpack(fz[sw(j)]), 2), B = shr(unpack(fz[sw(j + 256)]), 2);
      const Cq C = shr(unpack(fz[sw(j + 512)]), 2), D = shr(unpack(fz[sw(j + 768)]), 2);
      const Cq R = qadd(A, C), S = qsub(A, C), T = qadd(B, D), U = qsub(B, D);
      fz[sw(j)] = pack(hadd(R, T));
      fz[sw(j + 256)] = pack(twmul(tw[2 * j], qsub(R, T)));
      fz[sw(j + 512)] = pack(twmul(tw[j], Cq{sat16(S.r + U.i), sat16(S.i - U.r)}));      // __QSAX
      fz[sw(j + 768)] = pack(twmul(tw[3 * j], Cq{sat16(S.r - U.i), sat16(S.i + U.r)}));  // __QASX
    }
    __syncthreads();
    // middle stages: n2 = 64, 16, 4; twiddle step 4, 16, 64
#pragma unroll
    for (int lg = 6; lg >= 2; lg -= 2) {
      const int n2 = 1 << lg, mod = 256 >> lg;
      for (int b = t; b < 256; b += NT) {
        const int jj = b & (n2 - 1), i0 = ((b >> lg) << (lg + 2)) + jj, ic = jj * mod;
        const Cq A = unpack(fz[sw(i0)]), B = unpack(fz[sw(i0 + n2)]), C = unpack(fz[sw(i0 + 2 * n2)]), D = unpack(fz[sw(i0 + 3 * n2)]);
        const Cq R = qadd(A, C), S = qsub(A, C), T = qadd(B, D), U = qsub(B, D);
        fz[sw(i0)] = pack(shr(hadd(R, T), 1));
        fz[sw(i0 + n2)] = pack(twmul(tw[2 * ic], hsub(R, T)));
        fz[sw(i0 + 2 * n2)] = pack(twmul(tw[ic], Cq{(S.r + U.i) >> 1, (S.i - U.r) >> 1}));      // __SHSAX
        fz[sw(i0 + 3 * n2)] = pack(twmul(tw[3 * ic], Cq{(S.r - U.i) >> 1, (S.i + U.r) >> 1}));  // __SHASX
      }
      __syncthreads();
    }
    // last stage: four neighbours, one halving; arm_bitreversal_16 folded into the stores
    for (int g = t; g < 256; g += NT) {
      const uint4 v = *reinterpret_cast<const uint4 *>(&fz[sw(4 * g)]);
      const Cq A = unpack(v.x), B = unpack(v.y), C = unpack(v.z), D = unpack(v.w);
      const Cq R = qadd(A, C), S = qsub(A, C), T = qadd(B, D), U = qsub(B, D);
      const int k0 = (int)(__brev((unsigned)(4 * g)) >> 22);  // reversed 10-bit index; + 512, 256, 768 for 4 g + 1, 2, 3
      nat[sw2(k0)] = pack(hadd(R, T));
      nat[sw2(k0 + 512)] = pack(hsub(R, T));
      nat[sw2(k0 + 256)] = pack(Cq{(S.r + U.i) >> 1, (S.i - U.r) >> 1});
      nat[sw2(k0 + 768)] = pack(Cq{(S.r - U.i) >> 1, (S.i + U.r) >> 1});
    }
    __syncthreads();
    // arm_split_rfft_q15 on bins 0 .. 736, arm_shift_q15 by 5, arm_cmplx_mag_squared_q15
    for (int k = t; k < kFt8Bins; k += NT) {
      int re, im;
      const Cq P = unpack(nat[sw2(k)]);
      if (k == 0) {
        re = (P.r + P.i) >> 1;
        im = 0;
      } else {
        const Cq Q = unpack(nat[sw2(1024 - k)]), Ac = unpack(a.tab[kFt8TabA + k]), Bc = unpack(a.tab[kFt8TabB + k]);
        const unsigned outR = (unsigned)(P.r * Ac.r) - (unsigned)(P.i * Ac.i) + (unsigned)(Q.r * Bc.r) + (unsigned)(Q.i * Bc.i);
        const unsigned outI = (unsigned)(Q.r * Bc.i) - (unsigned)(Q.i * Bc.r) + (unsigned)(P.r * Ac.i) + (unsigned)(P.i * Ac.r);
        re = (int)(short)((int)outR >> 16);
        im = (int)(short)((int)outI >> 16);
      }
      re = sat16(re * 32);
      im = sat16(im * 32);
      mg[k] = (unsigned short)(((unsigned)(re * re) + (unsigned)(im * im)) >> 17);  // 0 .. 16384 (the sum in more than 31 bits)
    }
    __syncthreads();
    // the two rows of this time offset: freq_sub 0 / 1, 368 bytes each (ft8.cpp:244-254)
    for (int e = t; e < 2 * kFt8Row; e += NT) {
      const int fs = e >= kFt8Row ? 1 : 0, j = e - kFt8Row * fs;
      const float db = (a.mag_db[mg[2 * j + fs]] + a.mag_db[mg[2 * j + fs + 1]]) / 2;
      const int scaled = (int)db;  // toward zero, saturating, NaN -> 0
      row[2 * kFt8Row * ts + e] = (uint8_t)(scaled < 0 ? 0 : (scaled > 255 ? 255 : scaled));
    }
    __syncthreads();
  }
