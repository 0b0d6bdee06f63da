// t41_sdr_amd/csrc/nb_kernel.inc -- the text of nb_kernel, included twice by nb_kernel.hip: T41_STAGE_KERNEL names the kernel,
// T41_STAGE_LIST 0 makes the kernel as it is without a stage map, 1 its list form (t41rx_set_stage_map).  Two kernels
// of one text, not one body shared by two kernels: an argument block handed on by reference compiles to another
// instruction stream, and the form without a map must stay the stream it was.
__global__ __launch_bounds__(64) void T41_STAGE_KERNEL(NbArgs a) {
#pragma clang fp contract(off)
  constexpr bool LIST = T41_STAGE_LIST != 0;
  __shared__ __attribute__((aligned(16))) float xs[kRow];  // the block, repaired in place
  __shared__ __attribute__((aligned(16))) float es[kRow];  // prediction error (first arm_fir_f32)
  __shared__ __attribute__((aligned(16))) float ts[kRow];  // matched-filter output (tempsamp)
  __shared__ float rs[16];                                 // R[0 .. 10]
  __shared__ float cs[16];                                 // last_frame_end[0 .. 12]
  const int lane = threadIdx.x;
  const unsigned blk = blockIdx.x;
  if (LIST && blk >= (unsigned)a.nlist * (unsigned)a.nframes) {  // block-uniform, ahead of every barrier
    const int i = 4 * (int)(blk - (unsigned)a.nlist * (unsigned)a.nframes) + (lane >> 4);
    if (i < a.nrest) {
      const size_t c = (size_t)a.rest[i] * kNbCarryPitch + (lane & 15);
      a.carry[(size_t)(a.sel ^ 1) * a.nchan * kNbCarryPitch + c] = a.carry[(size_t)a.sel * a.nchan * kNbCarryPitch + c];
    }
    return;
  }
  const int fr = (int)(blk % (unsigned)a.nframes);
  const int ch = LIST ? a.list[blk / (unsigned)a.nframes] : (int)(blk / (unsigned)a.nframes);
  float *x = a.aud + (LIST ? (size_t)ch * a.nframes + fr : (size_t)blk) * kNbBlock;  // (ch * nframes + fr) * 256

  const float4 xin = reinterpret_cast<const float4 *>(x)[lane];
  *reinterpret_cast<float4 *>(xs + kOff + 4 * lane) = xin;
  if (lane < 3) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    *reinterpret_cast<float4 *>(xs + 4 * lane) = z;
    *reinterpret_cast<float4 *>(es + 4 * lane) = z;
    *reinterpret_cast<float4 *>(xs + kOff + kNbBlock + 4 * lane) = z;
    *reinterpret_cast<float4 *>(ts + kOff + kNbBlock + 4 * lane) = z;
  }
  if (lane < kNbCarry) {
    const float *src = (fr == 0) ? a.carry + ((size_t)a.sel * a.nchan + ch) * kNbCarryPitch
                                 : x - kNbBlock + (kNbBlock - 1 - kNbOrder - kNbPL);  // frame f - 1's x[242 ..]
    cs[lane] = src[lane];
    if (fr == a.nframes - 1)  // this block's input x[242 .. 254] for the next call's frame 0
      a.carry[((size_t)(a.sel ^ 1) * a.nchan + ch) * kNbCarryPitch + lane] = x[kNbBlock - 1 - kNbOrder - kNbPL + lane];
  }
  __syncthreads();

  // R[i] = arm_dot_prod_f32(x, x + i, 256 - i): lane i, one accumulator, ascending n
  {
    const int lag = lane <= kNbOrder ? lane : kNbOrder;
    float r = 0.0f;
    for (int n = 0; n < kNbBlock - lag; ++n) r += xs[kOff + n] * xs[kOff + n + lag];
    if (lane <= kNbOrder) rs[lane] = r;
  }
  __syncthreads();

  // Levinson-Durbin as written (every lane, uniform values)
  float R[kNbOrder + 1], lp[kNbOrder + 1];
#pragma unroll
  for (int i = 0; i <= kNbOrder; ++i) {
    R[i] = rs[i];
    lp[i] = i == 0 ? 1.0f : 0.0f;
  }
  R[0] = (float)((double)R[0] * (1.0 + 1.0e-9));
  float alfa = R[0];
#pragma unroll
  for (int m = 1; m <= kNbOrder; ++m) {
    float s = 0.0f;
#pragma unroll
    for (int u = 1; u < m; ++u) s = s + lp[u] * R[m - u];
    const float k = -(R[m] + s) / alfa;
    float any[kNbOrder + 1];
#pragma unroll
    for (int v = 1; v < m; ++v) any[v] = lp[v] + k * lp[m - v];
#pragma unroll
    for (int w = 1; w < m; ++w) lp[w] = any[w];
    lp[m] = k;
    alfa = alfa * (1.0f - k * k);
  }
  float rl[kNbOrder + 1];
#pragma unroll
  for (int o = 0; o <= kNbOrder; ++o) rl[kNbOrder - o] = lp[o];

  // arm_fir_f32 with pCoeffs = c from a zeroed state: y[n] = sum_j c[j] x[n - 10 + j], j ascending (pCoeffs[0] on the
  // oldest sample).  Lane l: outputs 4 l .. 4 l + 3 from the 16 samples src[4 l - 12 .. 4 l + 3].
  auto fir = [&](const float *src, const float (&c)[kNbOrder + 1], float (&y)[4]) {
#pragma clang fp contract(off)
    float w[16];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 v = *reinterpret_cast<const float4 *>(src + 4 * lane + 4 * t);
      w[4 * t] = v.x;
      w[4 * t + 1] = v.y;
      w[4 * t + 2] = v.z;
      w[4 * t + 3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j <= kNbOrder; ++j) acc += c[j] * w[q + 2 + j];
      y[q] = acc;
    }
  };
  float t4[4];
  fir(xs, rl, t4);  // inverse filter
  *reinterpret_cast<float4 *>(es + kOff + 4 * lane) = make_float4(t4[0], t4[1], t4[2], t4[3]);
  __syncthreads();
  fir(es, lp, t4);  // matched filter
  *reinterpret_cast<float4 *>(ts + kOff + 4 * lane) = make_float4(t4[0], t4[1], t4[2], t4[3]);
  __syncthreads();

  // arm_var_f32 (two-pass: mean, then the squared deviations; / (N - 1)), arm_power_f32(lpcs, 10)
  float sum = 0.0f;
  for (int n = 0; n < kNbBlock; n += 4) {
    const float4 v = *reinterpret_cast<const float4 *>(ts + kOff + n);
    sum += v.x;
    sum += v.y;
    sum += v.z;
    sum += v.w;
  }
  const float mean = sum / (float)kNbBlock;
  float dev = 0.0f;
  for (int n = 0; n < kNbBlock; n += 4) {
    const float4 v = *reinterpret_cast<const float4 *>(ts + kOff + n);
    float d = v.x - mean;
    dev += d * d;
    d = v.y - mean;
    dev += d * d;
    d = v.z - mean;
    dev += d * d;
    d = v.w - mean;
    dev += d * d;
  }
  const float sigma2 = dev / (float)(kNbBlock - 1);
  float lpc_power = 0.0f;
#pragma unroll
  for (int i = 0; i < kNbOrder; ++i) lpc_power += lp[i] * lp[i];
  const float thr = 2.5f * sqrtf(sigma2 * lpc_power);

  // The do-while scan (search_pos = 13 .. 241, skip PL after a hit, at most 20 hits) from one ballot per sample slot:
  // bit l of hit[q] = sample 4 l + q is above the threshold.  A NaN threshold or sample compares false.
  const int first = kNbOrder + kNbPL, last = kNbBlock - kNbBoundary - 1;
  unsigned long long hit[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = 4 * lane + q;
    hit[q] = __ballot(n >= first && n <= last && (t4[q] > thr || t4[q] < -thr));
  }
  if ((hit[0] | hit[1] | hit[2] | hit[3]) == 0ull) return;  // nothing to repair: the scratch keeps its samples

  // repair (negated predictors: lpcs[1..10] backward, reverse_lpcs[0..9] forward)
  float fw[kNbOrder], bw[kNbOrder];
#pragma unroll
  for (int k = 0; k < kNbOrder; ++k) {
    fw[k] = -rl[k];
    bw[k] = -lp[k + 1];
  }
  int cur = first;
  for (int count = 0; count < kNbMaxImpulses; ++count) {
    int sp = kNbBlock;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int l0 = (cur - q + 3) >> 2;  // first lane whose slot-q sample is >= cur
      const unsigned long long m = l0 >= 64 ? 0ull : (hit[q] >> l0) << l0;
      if (m) sp = min(sp, 4 * __builtin_ctzll(m) + q);
    }
    if (sp > last) break;
    cur = sp + kNbPL + 1;
    const int pos = sp - kNbOrder;
    float f[kNbOrder + kNbImpulse], b[kNbOrder + kNbImpulse];
#pragma unroll
    for (int k = 0; k < kNbOrder; ++k) {
      const int i = pos - kNbPL - kNbOrder + k;
      // below the block the reference reads last_frame_end[pos + k] (one sample earlier than x[i] of the previous block)
      f[k] = i < 0 ? cs[min(pos + k, 15)] : xs[kOff + max(i, 0)];
      b[kNbImpulse + k] = xs[kOff + pos + kNbPL + 1 + k];
    }
#pragma unroll
    for (int i = 0; i < kNbImpulse; ++i) {
      float af = 0.0f, ab = 0.0f;
#pragma unroll
      for (int k = 0; k < kNbOrder; ++k) {
        af += fw[k] * f[i + k];
        ab += bw[k] * b[kNbImpulse - i + k];
      }
      f[i + kNbOrder] = af;
      b[kNbImpulse - i - 1] = ab;
    }
    __syncthreads();  // (every lane has read the samples this impulse replaces)
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kNbImpulse; ++i) {
        const float wbw = (float)((double)i / (double)(kNbImpulse - 1));
        const float wfw = (float)((double)(kNbImpulse - 1 - i) / (double)(kNbImpulse - 1));
        xs[kOff + pos - kNbPL + i] = wfw * f[kNbOrder + i] + wbw * b[i];
      }
    }
    __syncthreads();
  }
  // samples 0 .. 239 back (the repairs end at 234; 242 .. 254 are the next frame's carry and stay untouched here)
  if (lane < 60) reinterpret_cast<float4 *>(x)[lane] = *reinterpret_cast<const float4 *>(xs + kOff + 4 * lane);
}
