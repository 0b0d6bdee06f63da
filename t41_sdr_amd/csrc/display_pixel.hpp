// t41_sdr_amd/csrc/display_pixel.hpp -- from FFT_spec to the display's integers: log10f_fast() (Utility.cpp:245-258) and
// pixelnew[] (FFT.cpp:157, 245).  Device code of cal_kernel.hip and panadapter_kernel.hip.  The contraction pragma is
// lexical: every function here carries it as its body's first line.
#pragma once
#include <hip/hip_runtime.h>

namespace t41 {

// log10f_fast(), Utility.cpp:245-258, in f32 as written; frexpf(0) = 0 with exponent 0, so log10f_fast(0) is finite
__device__ __forceinline__ float log10f_fast(float X) {
#pragma clang fp contract(off)
  const float t = fabsf(X);
  const float F = __builtin_amdgcn_frexp_mantf(t);
  const int E = __builtin_amdgcn_frexp_expf(t);
  float Y = 1.23149591368684f;
  Y *= F;
  Y += -4.11852516267426f;
  Y *= F;
  Y += 6.02197014179219f;
  Y *= F;
  Y += -3.13396450166353f;
  Y += (float)E;
  return Y * 0.3010299956639812f;
}

// pixelnew[x] = baseOffset + pixel_offset + (int16_t)(dBScale * log10f_fast(FFT_spec[x])): uint16 + int16 + int16 in int,
// stored to an int16; base = baseOffset + pixel_offset
__device__ __forceinline__ short display_pixel(int base, float dBScale, float spec) {
#pragma clang fp contract(off)
  return (short)(base + (int)(short)(int)(dBScale * log10f_fast(spec)));
}

}  // namespace t41
