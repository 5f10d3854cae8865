// Device helpers shared by the perturbation kernels (attack.hip: the additive pixel model and the capture seams; illum.hip: the
// illumination model; stem_grad.hip / stem_fwd.hip: the fused I3D stem): the channel stores / loads of the space-to-depth layouts, the
// rounding pair that keeps products and sums apart, the element model of the additive perturbation (decode, perturbation, clamp,
// 8-bit round trip, gradient pass test and tail), the wave sum, and the unit scheme and statistics fold of the two export kernels.
#pragma once
#include "flk_internal.h"
#include "quant_encode.h"

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

// sum over the 64 lanes of a wave, in lane 0: the shuffle tree 32, 16, .., 1 (one fixed order)
template <typename T> __device__ static inline T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// fold_t -> the space-to-depth layout (the template argument of S2D in attack.hip; 0 -> 2, fold_t 4 is laid out like 1) and the frames
// it folds into one position
__host__ __device__ constexpr int fold_layout(int fold_t) { return (fold_t == 1 || fold_t == 4) ? 1 : fold_t == 3 ? 3 : 2; }
__host__ __device__ constexpr int fold_frames(int fold_t) { return fold_layout(fold_t) == 1 ? 1 : 2; }

// ---- the element of the perturbed clip (flk_apply_args): decode the stored value, add adv_flag * clip(delta) / std of the rolled frame,
// clamp (centred or not), optionally through the 8-bit round trip; for the gradient the inclusive bound test on the same sum and the
// finishing factor under the delta-clamp mask ----------------------------------------------------------------------------------------
// byte i of a run of little-endian words
__device__ static inline uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
// the value of byte `by`: the dialect's scalars, or (x_lut) the per-channel table, channel c
__device__ static inline float decode_scaled(const flk_apply_args& a, uint32_t by) { return (float)by * a.x_scale + a.x_bias; }
__device__ static inline float decode_u8(const flk_apply_args& a, uint32_t by, int c) { return a.x_lut ? a.x_lut[by * 3 + c] : decode_scaled(a, by); }
// the 6 * NP bytes x[b,tx,h, NP * 2 * wg .. , 0..2]: NP = 4 as three aligned 8-byte loads (W % 8 == 0, x 8-byte aligned), NP = 1 as three
// 2-byte loads (x 2-byte aligned)
template <int NP> __device__ static inline void load_bytes(const uint8_t* src, uint32_t* by) {
  if constexpr (NP == 4) {
    const uint2* p = (const uint2*)src;
    const uint2 r0 = p[0], r1 = p[1], r2 = p[2];
    const uint32_t w[6] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y};
#pragma unroll
    for (int k = 0; k < 24; ++k) by[k] = byte_of(w, k);
  } else {
    const uint16_t* p = (const uint16_t*)src;
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
    by[0] = w0 & 255; by[1] = w0 >> 8; by[2] = w1 & 255; by[3] = w1 >> 8; by[4] = w2 & 255; by[5] = w2 >> 8;
  }
}

// the flicker perturbation [T,3] / [B,T,3] added at frame t (before adv_flag): p'[t] = p[(t - shift_p) mod T] (tf.roll), p = clip(delta)/std
// (pert_at of attack.hip is the same over the per-line and dense perturbations: their element of delta, then pert_of)
__device__ static inline int flicker_index(const flk_apply_args& a, int b, int ts, int c) { return (a.delta_per_clip ? b * a.T : 0) * 3 + ts * 3 + c; }
__device__ static inline float pert_of(const flk_apply_args& a, int b, float d, int c) {
  const float dc = a.dclip_dev ? a.dclip_dev[b] : a.dclip;       // (per-clip clamp bound)
  if (dc > 0.f) d = clipf(d, -dc, dc);
  return d * a.inv_std[c];
}
__device__ static inline float flicker_pert(const flk_apply_args& a, int b, int t, int c) {
  return pert_of(a, b, a.delta[flicker_index(a, b, wrap(t - a.shift_p, a.T), c)], c);
}

// value written for a pixel x with perturbation pv (adv_flag included): the clipped sum, or (flk_apply_args.center) the sum minus pv --
// i.e. x itself wherever the clip is inactive.  clamps(): the clamp holds the sum u at a bound
__device__ static inline bool clamps(const flk_apply_args& a, float u) { return u < a.lo || u > a.hi; }
__device__ static inline float applied(const flk_apply_args& a, float x, float pv) {
  const float u = x + pv;
  if (!a.center) return clipf(u, a.lo, a.hi);
  return clamps(a, u) ? clipf(u, a.lo, a.hi) - pv : x;
}
// Quantised apply (flk_apply_args.q_lut, template QUANT of the apply kernels): the value a kernel writes is the one the STORED video
// decodes to -- v = applied(...) encoded to its byte (encode_q of quant_encode.h, the export kernel's quantiser), the byte decoded
// through the table.  NO second clamp: a value the clamp holds at a bound is stored as the level nearest the bound, and a clean forward
// of the stored frames (clamp bounds -inf / +inf) sees that level.  ql: the 768-entry table in LDS (stage_q_lut); c: the value's
// channel.  QUANT = false is the identity: the plain instantiations contain none of this.
template <bool QUANT> __device__ static inline float quantised(const flk_apply_args& a, const float* ql, float v, int c) {
  if constexpr (QUANT) return ql[encode_q(v, a.q_mul[c], a.q_add[c], a.q_levels) * 3 + c];
  else return v;
}
// every thread of the workgroup calls this once, before any early return
__device__ static inline void stage_q_lut(const flk_apply_args& a, float* ql) {
  for (int i = threadIdx.x; i < 768; i += 256) ql[i] = a.q_lut[i];
  __syncthreads();
}
// the value every apply kernel writes (and the export kernel encodes, QUANT = false)
template <bool QUANT> __device__ static inline float perturbed(const flk_apply_args& a, const float* ql, float x, float pv, int c) {
  return quantised<QUANT>(a, ql, applied(a, x, pv), c);
}

// the gradient passes where lo <= x' + adv_flag p' <= hi (both clip gradients are inclusive at the bounds); p: before adv_flag -- the
// product and the sum are one expression here, as the gradient kernels always had it (hipcc contracts them)
__device__ static inline bool passes(const flk_apply_args& a, float x, float p) {
  const float u = x + a.adv_flag * p;
  return u >= a.lo && u <= a.hi;
}
// the tail of every delta gradient: the sum times adv_flag times the channel's factor (in that order), zero where the delta value d
// lies outside its clamp dc (dc <= 0: no clamp)
__device__ static inline bool delta_unclamped(float d, float dc) { return !(dc > 0.f) || (d >= -dc && d <= dc); }
__device__ static inline float delta_grad_out(float d, float dc, float sum, float adv_flag, float factor) {
  return delta_unclamped(d, dc) ? sum * adv_flag * factor : 0.f;
}

// ---- the unit scheme of the 8-bit export kernels: work item = (clip, frame, chunk of 256 units of the DESTINATION frame dst of F
// bytes); unit 0 the bytes in front of dst's first 4-byte boundary (0..3), units 1..nw its aligned words, unit nw + 1 the bytes behind
// the last whole word (0..3).  A thread's unit covers bytes [start, start + cnt) of the frame; (h, w, c) walks their pixels -------------
struct ExportUnit {
  int start, cnt;
  int h, w, c;
  __device__ ExportUnit(const uint8_t* dst, int F, int W, int chunk) : start(0), cnt(0) {
    int head = (4 - (int)((uintptr_t)dst & 3)) & 3;
    if (head > F) head = F;
    const int nw = (F - head) >> 2, tail = (F - head) & 3;
    const int u = chunk * 256 + (int)threadIdx.x;
    if (u == 0) cnt = head;
    else if (u <= nw) { start = head + 4 * (u - 1); cnt = 4; }
    else if (u == nw + 1) { start = head + 4 * nw; cnt = tail; }
    const int pix = start / 3;
    c = start - pix * 3;
    h = pix / W;
    w = pix - h * W;
  }
  __device__ void next(int W) { if (++c == 3) { c = 0; if (++w == W) { w = 0; ++h; } } }
};
// the unit's source bytes: one word where it is whole and aligned, else byte by byte
__device__ static __forceinline__ void export_load_u8(const uint8_t* s, int cnt, uint32_t* by) {
  if (cnt == 4 && ((uintptr_t)s & 3) == 0) {
    const uint32_t v = *(const uint32_t*)s;
    by[0] = v & 255; by[1] = (v >> 8) & 255; by[2] = (v >> 16) & 255; by[3] = v >> 24;
  } else {
    for (int j = 0; j < cnt; ++j) by[j] = s[j];
  }
}
// the 12 sums of a work item (acc[c][0..3]: per channel the sum of d = exported - stored byte, of |d|, the count of d != 0 and the count of
// clamped values; the kernels add to them in place -- as a helper that addition sent acc to scratch memory): reduced in the wave, then through LDS (red: [4][12]), and thread k adds sum k
// to row[k] with one integer atomic (integer sums: exact in any order).  Every thread of the workgroup calls it; red is free again after
__device__ static __forceinline__ void export_stats_fold(const int acc[3][4], int* red, int32_t* row) {
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const int v = wave_sum(acc[k >> 2][k & 3]);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 12 + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    const int s = red[threadIdx.x] + red[12 + threadIdx.x] + red[24 + threadIdx.x] + red[36 + threadIdx.x];
    if (s != 0) atomicAdd(row + threadIdx.x, s);
  }
  __syncthreads();
}
