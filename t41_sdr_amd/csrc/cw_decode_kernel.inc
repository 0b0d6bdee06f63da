// t41_sdr_amd/csrc/cw_decode_kernel.inc -- the text of cw_decode_kernel, included twice by cw_kernel.hip: T41_STAGE_KERNEL names the kernel,
// T41_STAGE_LIST 0 makes the kernel as it is without a stage map, 1 its list form (t41rx_set_stage_map).  Two kernels
// of one text, not one body shared by two kernels: an argument block handed on by reference compiles to another
// instruction stream, and the form without a map must stay the stream it was.
__global__ __launch_bounds__(64) void T41_STAGE_KERNEL(CwDecodeArgs a) {
#pragma clang fp contract(off)
  constexpr bool LIST = T41_STAGE_LIST != 0;
  using namespace cwd;
  __shared__ int hl[kCwDecGapWords];
  __shared__ int outl[64 * kOutPitch];
  __shared__ unsigned char tree[kCwTreeChars + 3];
  const int lane = threadIdx.x;
  const int ch0 = blockIdx.x * 64;
  const int nlive = min(64, (LIST ? a.nlist : a.nchan) - ch0);
  const bool live = lane < nlive;
  // (the channel in column k of this block: ch0 + k, with a list list[ch0 + k])
  int32_t *w = a.state + (size_t)(LIST ? a.list[ch0 + (live ? lane : 0)] : ch0 + (live ? lane : 0)) * kCwDecWords;
  for (int i = lane; i < kCwTreeChars; i += 64) tree[i] = a.tree[i];

  int st = w[kCwDecState];
  unsigned n = (unsigned)w[kCwDecN];
  int oldTime = w[kCwDecOldTime], signalStart = w[kCwDecSignalStart], signalEnd = w[kCwDecSignalEnd];
  int elapsed = w[kCwDecElapsed], gapLength = w[kCwDecGapLength];
  unsigned ditLength = (unsigned)w[kCwDecDitLength];
  int dahLength = w[kCwDecDahLength], gapAtom = w[kCwDecGapAtom], gapChar = w[kCwDecGapChar];
  float tgm = __int_as_float(w[kCwDecTgm]);
  int aveDit = w[kCwDecAveDit], aveDah = w[kCwDecAveDah], valRef1 = w[kCwDecValRef1], valRef2 = w[kCwDecValRef2];
  int gapRef1 = w[kCwDecGapRef1], valFlag = w[kCwDecValFlag], signalStartOld = w[kCwDecSignalStartOld];
  int dashJump = w[kCwDecDashJump], index = w[kCwDecIndex];
  bool charFlag = w[kCwDecCharFlag] != 0, blankFlag = w[kCwDecBlankFlag] != 0;
  int topGap = w[kCwDecTopGap], topGapOld = w[kCwDecTopGapOld];
  int currentTime = w[kCwDecCurrentTime], interGap = w[kCwDecInterGap], noSignal = w[kCwDecNoSignal];
  __syncthreads();

  for (int f0 = 0; f0 < a.nframes; f0 += kChunk) {
    const int nf = min(kChunk, a.nframes - f0);
    unsigned keys = 0;  // bit k: combinedCoeff > 50 in frame f0 + k (CWProcessing.cpp:365)
    for (int k0 = 0; k0 < nlive; k0 += 8) {  // (8 channels' loads in flight)
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (k0 + j < nlive && lane < nf) ? a.cw[((size_t)(LIST ? a.list[ch0 + k0 + j] : ch0 + k0 + j) * a.nframes + f0 + lane) * 4 + 3] : 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned m = (unsigned)__ballot(v[j] > 50.0f);
        if (lane == k0 + j) keys = m;
      }
    }
    for (int fr = 0; fr < nf; ++fr) {
      const bool key = (keys >> fr) & 1u;
      const int now = (int)((unsigned)a.t0 + (unsigned)(((unsigned long long)n * (unsigned)a.num) / (unsigned)a.den));
      if (n == 0) oldTime = a.t0;  // static long oldTime = millis();
      int ch = 0, ev = 0, evval = 0;  // ev: 1 = DoGapHistogram(evval), 2 = DoSignalHistogram(evval)
      if (st == 0) {
        if (key) {
          signalStart = now;
          st = 1;
          gapLength = sub32(signalStart, signalEnd);
          if (gapLength > 20 && (unsigned)gapLength < (unsigned)(tgm * 3.0f) && sub32(signalStart, oldTime) > 5000) {
            ev = 1;
            evval = gapLength;
            oldTime = signalStart;
          }
        } else {
          noSignal = now;
          interGap = sub32(noSignal, signalEnd);
          if ((double)interGap > (double)ditLength * 1.95 && charFlag)
            st = 5;
          else if ((double)interGap > (double)ditLength * 4.5 && !blankFlag && !charFlag)
            st = 6;
        }
      } else if (st == 1) {
        if (!key) {
          currentTime = now;
          elapsed = sub32(currentTime, signalStart);
          if (elapsed < 20) {
            st = 0;
          } else {
            if (elapsed > 20 && elapsed < kCwHistElements && sub32(currentTime, oldTime) > 5000) {
              ev = 2;
              evval = elapsed;
              oldTime = currentTime;
              // DoSignalHistogram() up to the arrays, :765-789
              if (valFlag == 0) {
                valRef1 = elapsed;
                signalStartOld = now;
                valFlag = 1;
              }
              if ((unsigned)now - (unsigned)signalStartOld > 20u && valFlag == 1) {
                gapRef1 = gapLength;
                valRef2 = elapsed;
                valFlag = 0;
              }
              const float v1 = (float)valRef1, v2 = (float)valRef2, g1 = (float)gapRef1;
              if ((v2 >= v1 * 2.0f && g1 <= v1 * 2.0f) || (v1 >= v2 * 2.0f && g1 <= v2 * 2.0f)) {
                const bool ditFirst = valRef2 >= valRef1;
                const int dit = ditFirst ? valRef1 : valRef2, dah = ditFirst ? valRef2 : valRef1;
                aveDit = (int)(0.9 * (double)aveDit + 0.1 * (double)dit);
                aveDah = (int)(0.9 * (double)aveDah + 0.1 * (double)dah);
              }
              // sqrt() in double, then to float.  The device's f64 sqrt is correctly rounded, as the host's.  (And the
              // float behind it does not hang on the double's last bit: the product N is an integer below 2^30 and a
              // midpoint m between two floats has 25 bits, so N - m^2 is zero or at least 2^-51 of N -- the root is an
              // integer or two double ulps and more away from every midpoint.)
              tgm = (float)sqrt((double)(int)((unsigned)aveDit * (unsigned)aveDah));
            }
            signalEnd = currentTime;
            st = 2;
          }
        }
      } else if (st == 2) {
        if ((double)elapsed > 0.5 * (double)ditLength) {
          dashJump >>= 1;
          index = (index + (elapsed < (int)tgm ? 1 : dashJump)) & 255;
          charFlag = true;
        }
        st = 0;
      } else if (st == 5) {
        ch = index < kCwTreeChars ? (int)tree[index] : (int)'-';  // (past the literal: the tree's own filler)
        index = 0;
        dashJump = 128;
        charFlag = false;
        blankFlag = false;
        st = 0;
      } else if (st == 6) {
        ch = (int)' ';
        blankFlag = true;
        st = 0;
      }
      ++n;
      if (!live) ev = 0;

      // the histogram calls of this frame, one channel at a time, by the whole wave
      unsigned long long pending = __ballot(ev != 0);
      while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        // (wave-uniform by construction; said so, so that the branches and loop bounds below are scalar)
        const int type = __builtin_amdgcn_readfirstlane(__shfl(ev, src)), val = __builtin_amdgcn_readfirstlane(__shfl(evval, src));
        const float t = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(__shfl(tgm, src))));
        int32_t *g = a.state + (size_t)(LIST ? a.list[ch0 + src] : ch0 + src) * kCwDecWords + (type == 1 ? kCwDecOffGap : kCwDecOffSig);
        const int cap = type == 1 ? kCwDecGapWords : kCwDecSigWords;
        __syncthreads();
        for (int k = lane; k < cap; k += 64) hl[k] = g[k];
        __syncthreads();
        bool scaled;
        if (type == 2) {
          // :791-814
          if (lane == 0 && (unsigned)val < (unsigned)cap) hl[val] += 1;
          __syncthreads();
          const int offset = (int)((unsigned)t - 1u);
          int tempDit, dit, tempDah, dah;
          clustered_max(hl, cap, 0, offset, 1, lane, &tempDit, &dit);
          clustered_max(hl, cap, offset, kCwHistElements - offset, 3, lane, &tempDah, &dah);
          scaled = (double)tempDit > kScaleConstant && (double)tempDah > kScaleConstant;
          __syncthreads();
          if (scaled)
            for (int k = lane; k < kCwHistElements; k += 64) hl[k] = (int)(0.8 * (double)hl[k]);
          if (lane == src) {
            ditLength = (unsigned)dit;
            dahLength = dah + offset;
          }
        } else {
          // DoGapHistogram(), :660-698
          scaled = rd(hl, val, cap) > 10;
          __syncthreads();
          if (scaled)
            for (int k = lane; k < kCwHistElements; k += 64) hl[k] = (int)(unsigned)(.8 * (double)(float)hl[k]);
          __syncthreads();
          if (lane == 0 && (unsigned)val < (unsigned)cap) hl[val] += 1;
          __syncthreads();
          int atom = __shfl(gapAtom, src), top = __shfl(topGap, src), chr = 0;
          const int topOld = __shfl(topGapOld, src);
          const bool atomBranch = (float)val <= t;
          if (atomBranch) {
            int cnt, atomIndex;
            clustered_max(hl, cap, 0, (int)(unsigned)t, 1, lane, &cnt, &atomIndex);
            if (atomIndex) atom = atomIndex;
            // :674-684: the highest non-empty word below 2 * gapAtom, counting down from word 750
            const int twice = (int)(2u * (unsigned)atom);
            int found = 0;
            for (int i = 1 + lane; i <= kCwHistElements; i += 64)
              if (hl[i] > 0 && i < twice) found = i;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) found = max(found, __shfl_xor(found, off));
            if (found)
              top = found;
            else if (top > twice)
              top = topOld;  // discard outliers
          } else if ((float)val <= t * 2.0f) {
            int cnt;
            clustered_max(hl, cap, (int)t + 1, (int)(unsigned)(t * 2.0f), 3, lane, &cnt, &chr);
          }
          if (lane == src) {
            gapAtom = atom;
            if (atomBranch) {
              topGap = top;
              topGapOld = top;
            }
            if (chr) gapChar = chr;
          }
        }
        __syncthreads();
        // what changed goes back: words 0 .. 749 after a scaling pass, and the incremented word where that pass did not
        // cover it (no pass, or a gap of 750 ms and more: gapLen runs up to 3 * thresholdGeometricMean)
        if (scaled)
          for (int k = lane; k < kCwHistElements; k += 64) g[k] = hl[k];
        if (lane == 0 && (unsigned)val < (unsigned)cap && (!scaled || val >= kCwHistElements)) g[val] = hl[val];
      }
      outl[lane * kOutPitch + 2 * fr] = ch;
      outl[lane * kOutPitch + 2 * fr + 1] = (int)ditLength;
    }
    __syncthreads();
    for (int kk = 0; kk < nlive; ++kk)
      if (lane < 2 * nf) a.text[((size_t)(LIST ? a.list[ch0 + kk] : ch0 + kk) * a.nframes + f0) * 2 + lane] = outl[kk * kOutPitch + lane];
    __syncthreads();
  }
  if (live) {
    w[kCwDecState] = st;
    w[kCwDecN] = (int)n;
    w[kCwDecOldTime] = oldTime;
    w[kCwDecSignalStart] = signalStart;
    w[kCwDecSignalEnd] = signalEnd;
    w[kCwDecElapsed] = elapsed;
    w[kCwDecGapLength] = gapLength;
    w[kCwDecDitLength] = (int)ditLength;
    w[kCwDecDahLength] = dahLength;
    w[kCwDecGapAtom] = gapAtom;
    w[kCwDecGapChar] = gapChar;
    w[kCwDecTgm] = __float_as_int(tgm);
    w[kCwDecAveDit] = aveDit;
    w[kCwDecAveDah] = aveDah;
    w[kCwDecValRef1] = valRef1;
    w[kCwDecValRef2] = valRef2;
    w[kCwDecGapRef1] = gapRef1;
    w[kCwDecValFlag] = valFlag;
    w[kCwDecSignalStartOld] = signalStartOld;
    w[kCwDecDashJump] = dashJump;
    w[kCwDecIndex] = index;
    w[kCwDecCharFlag] = charFlag ? 1 : 0;
    w[kCwDecBlankFlag] = blankFlag ? 1 : 0;
    w[kCwDecTopGap] = topGap;
    w[kCwDecTopGapOld] = topGapOld;
    w[kCwDecCurrentTime] = currentTime;
    w[kCwDecInterGap] = interGap;
    w[kCwDecNoSignal] = noSignal;
  }
}
