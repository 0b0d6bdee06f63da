// t41_sdr_amd/csrc/cw_detect_kernel.inc -- the text of cw_detect_kernel, included twice by cw_kernel.hip: T41_STAGE_KERNEL names the kernel,
// T41_STAGE_LIST 0 makes the kernel as it is without a stage map, 1 its list form (t41rx_set_stage_map).  Two kernels
// of one text, not one body shared by two kernels: an argument block handed on by reference compiles to another
// instruction stream, and the form without a map must stay the stream it was.
__global__ __launch_bounds__(64) void T41_STAGE_KERNEL(CwDetectArgs a) {
#pragma clang fp contract(off)
  constexpr bool LIST = T41_STAGE_LIST != 0;
  constexpr int N = kCwBlock, T = kCwFirTaps;
  __shared__ float s[T - 1 + N + 1];  // arm_fir_f32's state: 63 samples of history, then the block
  __shared__ float A[N];              // float_buffer_CW: the filtered block
  __shared__ float B[N];              // sinBuffer
  __shared__ float C[T];              // CW_Filter_Coeffs2
  const int lane = threadIdx.x;
  const unsigned chan = LIST ? (unsigned)a.list[blockIdx.x] : blockIdx.x;
  float *st = a.state + (size_t)chan * kCwStateFloats;
  const float *x = a.aud + (size_t)chan * a.nframes * N;
  float *out = a.out + (size_t)chan * a.nframes * 4;

  C[lane] = a.fir[lane];
#pragma unroll
  for (int m = 0; m < 4; ++m) B[lane + 64 * m] = a.sinb[lane + 64 * m];
  if (lane < T - 1) s[lane] = st[kCwStFir + lane];
  float corrR = st[kCwStCorrR], aveL = st[kCwStAveL], aveR = st[kCwStAveR];

  float nx[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) nx[m] = x[lane + 64 * m];
  for (int f = 0; f < a.nframes; ++f) {
#pragma unroll
    for (int m = 0; m < 4; ++m) s[T - 1 + lane + 64 * m] = nx[m];
    if (f + 1 < a.nframes) {
#pragma unroll
      for (int m = 0; m < 4; ++m) nx[m] = x[(size_t)(f + 1) * N + lane + 64 * m];
    }
    __syncthreads();
    // arm_fir_f32: y[n] = sum_i coeffs[i] * state[n + i], one accumulator in tap order
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < T; ++i) {
      const float c = C[i];
#pragma unroll
      for (int m = 0; m < 4; ++m) y[m] = y[m] + c * s[lane + 64 * m + i];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) A[lane + 64 * m] = y[m];
    const float hist = lane < T - 1 ? s[N + lane] : 0.0f;  // the block's last 63 samples: the next block's history
    __syncthreads();
    if (lane < T - 1) s[lane] = hist;

    // arm_correlate_f32 over the lag pairs, and goertzel_mag's recurrence on the same walk
    float lo[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float q1 = 0.0f, q2 = 0.0f;
#pragma unroll 4
    for (int i = 0; i < N; ++i) {
      const float v = A[i];
      float q0 = a.coeff * q1;
      q0 = q0 - q2;
      q0 = q0 + v;
      q2 = q1;
      q1 = q0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int u = lane + 64 * m;
        const float p = v * B[(i - u - 1) & (N - 1)];
        const float l1 = lo[m] + p, h1 = hi[m] + p;
        lo[m] = i <= u ? l1 : lo[m];
        hi[m] = i <= u ? hi[m] : h1;
      }
    }
    // arm_max_f32 over the 511 lags (pair 255 has no second lag)
    float mx = lo[0];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      mx = lo[m] > mx ? lo[m] : mx;
      if (lane + 64 * m < N - 1) mx = hi[m] > mx ? hi[m] : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float o = __shfl_xor(mx, off);
      mx = o > mx ? o : mx;
    }
    // CWProcessing.cpp:336-357 with float_buffer_R = float_buffer_L: one computation serves both sides
    const float corrL = mx;
    aveL = (float)(.7 * (double)corrL + .3 * (double)aveL);
    const float ave = (corrR + corrL) / 2.0f;  // corrResultR is still the block before's (:339 runs before :348)
    const float re = (q1 - q2 * a.cosine) / 128.0f;
    const float im = (q2 * a.sine) / 128.0f;
    const float g1 = sqrtf(re * re + im * im);
    corrR = corrL;
    aveR = (float)(.7 * (double)corrR + .3 * (double)aveR);
    const float g = (g1 + g1) / 2.0f;
    const float comb = 10.0f * ave * 100.0f * g;
    if (lane < 4) out[(size_t)f * 4 + lane] = lane == 0 ? corrL : lane == 1 ? g : lane == 2 ? ave : comb;
  }
  __syncthreads();
  if (lane < T - 1) st[kCwStFir + lane] = s[lane];
  if (lane == 0) {
    st[kCwStCorrR] = corrR;
    st[kCwStAveL] = aveL;
    st[kCwStAveR] = aveR;
  }
}
