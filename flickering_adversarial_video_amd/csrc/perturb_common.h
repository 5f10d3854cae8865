// Device helpers shared by the perturbation kernels (attack.hip: the additive pixel model and the capture seams; illum.hip: the
// illumination model): the channel stores / loads of the space-to-depth layouts and the rounding pair that keeps products and sums apart.
#pragma once
#include "flk_internal.h"

template <typename TO, int NCH> __device__ static inline void store_ch(char* dst, const float* v) {
  if constexpr (sizeof(TO) == 4) {
#pragma unroll
    for (int i = 0; i < NCH / 4; ++i) ((float4*)dst)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < NCH / 8; ++i) {
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (bf16_t)v[8 * i + e];
      ((bf16x8*)dst)[i] = o;
    }
  }
}
template <typename TI, int NUSED> __device__ static inline void load_ch(const char* src, float* v) {   // NUSED = 24 | 12
  if constexpr (sizeof(TI) == 4) {
#pragma unroll
    for (int i = 0; i < NUSED / 4; ++i) { const float4 f = ((const float4*)src)[i]; v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w; }
  } else {
    float t[(NUSED + 7) / 8 * 8];
#pragma unroll
    for (int i = 0; i < (NUSED + 7) / 8; ++i) {
      const uint4 u = ((const uint4*)src)[i];
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) { t[8 * i + 2 * k] = __uint_as_float(w[k] << 16); t[8 * i + 2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u); }
    }
#pragma unroll
    for (int i = 0; i < NUSED; ++i) v[i] = t[i];
  }
}

__device__ static inline float clipf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
__device__ static inline int wrap(int t, int T) { t %= T; return t < 0 ? t + T : t; }

// one rounded product / sum: hipcc contracts a * b + c into one fma wherever BOTH operations allow it, and its headers define
// __fmul_rn / __fadd_rn as the plain operators, so the two are spelt out here with contraction switched off for their own operation
__device__ static inline float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ static inline float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
