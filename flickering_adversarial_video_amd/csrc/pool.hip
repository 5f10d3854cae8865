// tf.nn.max_pool3d (SAME) forward and MaxPool3DGrad, channels-last, 16-byte vectorised over channels.
// HBM-bound kernels: one thread = one position x one 16-byte channel group.
//   forward : first maximum in (t,h,w) scan order wins (strict >), padded cells never win
//             (i3d.py:174,189,212,252,398); the winning window index is kept as one byte.
//             Values are compared as numbers: -0.0 == +0.0 (the first of them in scan order wins), a window of -inf only records
//             tap 0.  relu_input: windows whose maximum is <= 0 record 255 ("no cell").  One deviation: the bf16 sortable-key
//             kernel (3x3x3 / 1, SAME pad-before 1) ranks +0.0 above -0.0, so among tied zeros of both signs the first +0.0 wins (see
//             bf16x2_to_keys); every other route, bf16 3x3x3 / 1 at another pad-before included, keeps the rule above.
//             Dispatch: stride-1 SAME windows of >= 8 taps stage a halo box in LDS (maxpool_s1_tiled_fwd; bf16 3x3x3 with pad-before 1
//             takes the sortable-key W-run kernel maxpool_s1_wrun_fwd_bf16); every other geometry takes one thread per
//             output (maxpool_fwd_kernel_k for the I3D windows, maxpool_fwd_kernel for the rest).
//   backward: the three strided I3D geometries take the owner form (maxpool_strided_bwd, both dtypes: every cell written once, fixed
//             order).  Everything else: bf16 takes the scatter form (maxpool_scatter_bwd): a workgroup owns a tile of INPUT cells in
//             LDS and every window that reaches the tile adds its gradient to the cell its saved argmax names, in 32-bit fixed point
//             with integer LDS atomics (order-independent, bitwise reproducible); the fixed-point exponent E depends on the number n
//             of windows that can cover one cell (E = 24 for n <= 64, 23 up to 128, 22 up to 255: n addends never leave an int32).
//             fp32 (the parity mode) takes the gather forms (every input cell scans the windows containing it; fixed summation
//             order): maxpool_s1_tiled_bwd for the LDS-tiled stride-1 windows, maxpool_bwd_kernel otherwise.  There is no switch
//             between the forms.  Optional relu mask of the producing layer (mask > 0) fused in.
//   fused   : flk_maxpool3d_bwd_gemm (bf16) = the scatter form fed by an MFMA product, same fixed point.
//             flk_maxpool3d_fwd_conv1x1 / flk_maxpool3d_bwd_conv1x1 (bf16, 1x3x3 / 1x2x2, 64 -> 64): MaxPool3d_2a with Conv3d_2b_1x1 inside,
//             forward and backward, bitwise the two launches they replace (end of this file).
//   Channel slices: in / out / gout / gin / mask are channels [coff, coff + C) of rows ld wide; nothing outside the slice is written.
#include <stdlib.h>
#include <string.h>
#include "flk_internal.h"
#include "conv_common.h"

// Timing ablations (skip loads / atomics / stores: WRONG results) exist only in -DFLK_ABLATE builds (tools/*_time.py pass it through
// FLK_HIPCC_EXTRA); in the product library the switches are compile-time zeros and the kernels carry no such branch.
#ifdef FLK_ABLATE
#define PF_DBG(bit) (p.dbg & (bit))
#define PG_DBG(bit) (pg.dbg & (bit))
#else
#define PF_DBG(bit) (0)
#define PG_DBG(bit) (0)
#endif

struct PoolKP {
  const char* in; char* out; uint8_t* idx;
  const char* gout; char* gin; const char* mask; const char* add;
  int in_ld, in_coff, out_ld, out_coff, C;
  int gout_ld, gout_coff, gin_ld, gin_coff, mask_ld, mask_coff;
  int B, Ti, Hi, Wi, To, Ho, Wo;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  int relu_input;
};

// position addressing, stated once: linear position of (b, t, h, w) in a [B, T, H, W] grid, and the byte address of channel c of a position
// in a channel slice (channels [coff, coff + C) of rows ld wide).  idx rows are C wide.
__device__ static inline size_t pool_pos(int b, int t, int h, int w, int T, int H, int W) { return (((size_t)(b * T + t) * H + h) * W + w); }
__device__ static inline size_t in_pos(const PoolKP& k, int b, int t, int h, int w) { return pool_pos(b, t, h, w, k.Ti, k.Hi, k.Wi); }
__device__ static inline size_t out_pos(const PoolKP& k, int b, int t, int h, int w) { return pool_pos(b, t, h, w, k.To, k.Ho, k.Wo); }
template <typename T> __device__ static inline size_t slice_off(size_t pos, int ld, int coff, int c) { return (pos * ld + coff + c) * sizeof(T); }
template <typename T> __device__ static inline const char* in_at(const PoolKP& k, size_t pos, int c) { return k.in + slice_off<T>(pos, k.in_ld, k.in_coff, c); }
template <typename T> __device__ static inline char* out_at(const PoolKP& k, size_t pos, int c) { return k.out + slice_off<T>(pos, k.out_ld, k.out_coff, c); }
template <typename T> __device__ static inline const char* gout_at(const PoolKP& k, size_t pos, int c) { return k.gout + slice_off<T>(pos, k.gout_ld, k.gout_coff, c); }
template <typename T> __device__ static inline char* gin_at(const PoolKP& k, size_t pos, int c) { return k.gin + slice_off<T>(pos, k.gin_ld, k.gin_coff, c); }
template <typename T> __device__ static inline const char* mask_at(const PoolKP& k, size_t pos, int c) { return k.mask + slice_off<T>(pos, k.mask_ld, k.mask_coff, c); }
__device__ static inline uint8_t* idx_at(const PoolKP& k, size_t pos, int c) { return k.idx + pos * k.C + c; }

template <typename T> struct PV;
template <> struct PV<bf16_t> {
  static constexpr int EPL = 8;
  __device__ static inline void ld(const char* p, float* f) {
    const uint4 u = *(const uint4*)p;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
  __device__ static inline void st(char* p, const float* f) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16_t)f[i];
    *(bf16x8*)p = v;
  }
  __device__ static inline void ldidx(const uint8_t* p, int* i) {
    const uint2 u = *(const uint2*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) { i[k] = (u.x >> (8 * k)) & 255; i[4 + k] = (u.y >> (8 * k)) & 255; }
  }
  __device__ static inline void stidx(uint8_t* p, const int* i) {
    uint2 u;
    u.x = i[0] | (i[1] << 8) | (i[2] << 16) | (i[3] << 24);
    u.y = i[4] | (i[5] << 8) | (i[6] << 16) | (i[7] << 24);
    *(uint2*)p = u;
  }
};
template <> struct PV<float> {
  static constexpr int EPL = 4;
  __device__ static inline void ld(const char* p, float* f) {
    const float4 u = *(const float4*)p; f[0] = u.x; f[1] = u.y; f[2] = u.z; f[3] = u.w;
  }
  __device__ static inline void st(char* p, const float* f) { *(float4*)p = make_float4(f[0], f[1], f[2], f[3]); }
  __device__ static inline void ldidx(const uint8_t* p, int* i) {
    const uint32_t u = *(const uint32_t*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) i[k] = (u >> (8 * k)) & 255;
  }
  __device__ static inline void stidx(uint8_t* p, const int* i) {
    *(uint32_t*)p = i[0] | (i[1] << 8) | (i[2] << 16) | (i[3] << 24);
  }
};

// The one-thread-per-position kernels.  grid: x = chunks of 256 over (w, channel group) of one row of a [B, Tn, ., Wn] grid (the output
// grid, or the input grid for maxpool_bwd_kernel); y = h; z = b * Tn + t  (32-bit index math only).  live = false: the thread is past the row.
struct PoolTask { bool live; int b, t, h, w, cg; };
template <typename T>
__device__ static inline PoolTask simple_grid_task(const PoolKP& p, int Tn, int Wn) {
  PoolTask k;
  const int ng = p.C / PV<T>::EPL;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  k.live = i < (unsigned)(Wn * ng);
  k.w = i / ng; k.cg = i - k.w * ng;
  k.h = blockIdx.y; k.t = blockIdx.z % Tn; k.b = blockIdx.z / Tn;
  return k;
}

// the end of a forward: a window's maxima and argmax bytes (channels [c, c + EPL) of output position opos)
template <typename T>
__device__ static inline void store_out_idx(const PoolKP& k, size_t opos, int c, const float (&best)[PV<T>::EPL], const int (&bi)[PV<T>::EPL]) {
  PV<T>::st(out_at<T>(k, opos, c), best);
  PV<T>::stidx(idx_at(k, opos, c), bi);
}

// the end of a maskable backward: the gradient of channels [c, c + EPL) of input cell ipos, zeroed where the producing layer's ReLU was
// off (mask <= 0), stored once.  (strided_owner_resolve, which may have loaded the mask operand ahead, keeps this tail written out.)
template <typename T>
__device__ static inline void mask_and_store(const PoolKP& k, size_t ipos, int c, float (&g)[PV<T>::EPL], bool masked) {
  constexpr int EPL = PV<T>::EPL;
  if (masked) {
    float mk[EPL];
    PV<T>::ld(mask_at<T>(k, ipos, c), mk);
#pragma unroll
    for (int e = 0; e < EPL; ++e) g[e] = mk[e] > 0.f ? g[e] : 0.f;
  }
  PV<T>::st(gin_at<T>(k, ipos, c), g);
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const PoolKP p) {
  constexpr int EPL = PV<T>::EPL;
  const PoolTask o = simple_grid_task<T>(p, p.To, p.Wo);
  if (!o.live) return;
  const int ow = o.w, cg = o.cg, oh = o.h, ot = o.t, b = o.b;
  float best[EPL];
  int bi[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) { best[e] = -INFINITY; bi[e] = 0; }
  int tap = 0;
  for (int dt = 0; dt < p.kt; ++dt) {
    const int it = ot * p.st - p.pt + dt;
    for (int dh = 0; dh < p.kh; ++dh) {
      const int ih = oh * p.sh - p.ph + dh;
      for (int dw = 0; dw < p.kw; ++dw, ++tap) {
        const int iw = ow * p.sw - p.pw + dw;
        if ((unsigned)it >= (unsigned)p.Ti || (unsigned)ih >= (unsigned)p.Hi || (unsigned)iw >= (unsigned)p.Wi) continue;
        float v[EPL];
        PV<T>::ld(in_at<T>(p, in_pos(p, b, it, ih, iw), cg * EPL), v);
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (v[e] > best[e]) { best[e] = v[e]; bi[e] = tap; }
      }
    }
  }
  if (p.relu_input) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) bi[e] = best[e] > 0.f ? bi[e] : 255;
  }
  store_out_idx<T>(p, out_pos(p, b, ot, oh, ow), cg * EPL, best, bi);
}

// The window scan of one (position, channel group) over its NT raw 16-byte taps (ok[tap]: the tap is an in-bounds cell): first maximum in
// scan order (strict >), padded cells never win, relu_input turns a maximum <= 0 into 255 ("no cell").  Shared by maxpool_fwd_kernel_k and
// the fused MaxPool3d_2a + Conv3d_2b forward (maxpool133_conv1x1_fwd): one comparison sequence, the same bits.
template <typename T, int NT>
__device__ static inline void pool_window_scan(const uint4 (&raw)[NT], const bool (&ok)[NT], int relu_input, float (&best)[PV<T>::EPL], int (&bi)[PV<T>::EPL]) {
  constexpr int EPL = PV<T>::EPL;
#pragma unroll
  for (int e = 0; e < EPL; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
  for (int tap = 0; tap < NT; ++tap) {
    float v[EPL];
    if constexpr (sizeof(T) == 2) {
      const uint32_t w[4] = {raw[tap].x, raw[tap].y, raw[tap].z, raw[tap].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[2 * k] = __uint_as_float(w[k] << 16); v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u); }
    } else {
      v[0] = __uint_as_float(raw[tap].x); v[1] = __uint_as_float(raw[tap].y); v[2] = __uint_as_float(raw[tap].z); v[3] = __uint_as_float(raw[tap].w);
    }
    if (ok[tap]) {
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        if (v[e] > best[e]) { best[e] = v[e]; bi[e] = tap; }
    }
  }
  if (relu_input) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) bi[e] = best[e] > 0.f ? bi[e] : 255;
  }
}

// The same with the window as template arguments (the I3D pools: 1x3x3, 3x3x3, 2x2x2): the tap loop unrolls and ALL tap loads of a thread
// are requested before the first compare -- with run-time loop bounds hipcc emits load -> wait -> compare per tap, KT*KH*KW exposed memory
// round trips per thread.  Same scan order, same tie rule (strict >), same bits.
template <typename T, int KT, int KH, int KW>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel_k(const PoolKP p) {
  constexpr int EPL = PV<T>::EPL, NT = KT * KH * KW;
  const PoolTask o = simple_grid_task<T>(p, p.To, p.Wo);
  if (!o.live) return;
  const int ow = o.w, cg = o.cg, oh = o.h, ot = o.t, b = o.b;
  uint4 raw[NT];
  bool ok[NT];
#pragma unroll
  for (int dt = 0; dt < KT; ++dt)
#pragma unroll
    for (int dh = 0; dh < KH; ++dh)
#pragma unroll
      for (int dw = 0; dw < KW; ++dw) {
        const int tap = (dt * KH + dh) * KW + dw;
        const int it = ot * p.st - p.pt + dt, ih = oh * p.sh - p.ph + dh, iw = ow * p.sw - p.pw + dw;
        ok[tap] = (unsigned)it < (unsigned)p.Ti && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
        const size_t pos = ok[tap] ? in_pos(p, b, it, ih, iw) : 0;      // (position 0 is always readable)
        raw[tap] = *(const uint4*)in_at<T>(p, pos, cg * EPL);
      }
  float best[EPL];
  int bi[EPL];
  pool_window_scan<T, NT>(raw, ok, p.relu_input, best, bi);
  store_out_idx<T>(p, out_pos(p, b, ot, oh, ow), cg * EPL, best, bi);
}

// the gather form over the INPUT grid
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const PoolKP p) {
  constexpr int EPL = PV<T>::EPL;
  {
    const PoolTask c = simple_grid_task<T>(p, p.Ti, p.Wi);
    if (!c.live) return;
    const int iw = c.w, cg = c.cg, ih = c.h, it = c.t, b = c.b;
    const size_t ipos = in_pos(p, b, it, ih, iw);
    float g[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) g[e] = 0.f;
    if (p.add) PV<T>::ld(p.add + slice_off<T>(ipos, p.gin_ld, p.gin_coff, cg * EPL), g);
    // windows containing this cell: o in [ceil((i+p-k+1)/s), floor((i+p)/s)] per dim; its tap index d = i+p-o*s
    const int ot_lo = max(0, (it + p.pt - p.kt + p.st) / p.st), ot_hi = min(p.To - 1, (it + p.pt) / p.st);
    const int oh_lo = max(0, (ih + p.ph - p.kh + p.sh) / p.sh), oh_hi = min(p.Ho - 1, (ih + p.ph) / p.sh);
    const int ow_lo = max(0, (iw + p.pw - p.kw + p.sw) / p.sw), ow_hi = min(p.Wo - 1, (iw + p.pw) / p.sw);
    for (int ot = ot_lo; ot <= ot_hi; ++ot)
      for (int oh = oh_lo; oh <= oh_hi; ++oh)
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
          const int tap = ((it + p.pt - ot * p.st) * p.kh + (ih + p.ph - oh * p.sh)) * p.kw + (iw + p.pw - ow * p.sw);
          const size_t opos = out_pos(p, b, ot, oh, ow);
          int id[EPL];
          PV<T>::ldidx(idx_at(p, opos, cg * EPL), id);
          bool any = false;
#pragma unroll
          for (int e = 0; e < EPL; ++e) any |= id[e] == tap;
          if (!any) continue;
          float go[EPL];
          PV<T>::ld(gout_at<T>(p, opos, cg * EPL), go);
#pragma unroll
          for (int e = 0; e < EPL; ++e)
            if (id[e] == tap) g[e] += go[e];
        }
    mask_and_store<T>(p, ipos, cg * EPL, g, p.mask != nullptr);
  }
}

// Backward of the STRIDED pools (MaxPool3d_2a/3a/4a/5a, i3d.py:174,189,252,398; window <= 2 * stride; SAME pad-before p < stride per
// dimension: 0 on even sizes, 1 on the odd ones the reference's 90-frame clips produce -- T/2 = 45, 23):
// one thread = one output window x one 16-byte channel group, and it OWNS the stride^3 input cells o*s - p + a, a in [0,s).
// A cell is covered by its own window (tap a) and, where a + s < k, by the previous window of that dimension (tap
// a + s): every thread loads the index bytes and gradients of its <= 8 candidate windows up front (independent loads,
// shared with its neighbours through L1/L2), then resolves its cells in registers in a fixed order -- no atomics,
// no dependent load chains, and each gradient cell is written exactly once (64-byte runs per thread).
// The owner's part once the index bytes id[w] and gradients go[w] of its candidate windows w = (dt * NH + dh) * NW + dw (window o - d per
// dimension; ok[w]: it exists) are in registers: every owned cell sums its candidates in a fixed order and is stored once.  Shared by
// maxpool_strided_bwd (candidates from global memory) and the fused Conv3d_2b data-gradient + MaxPool3d_2a backward
// (maxpool133_conv1x1_bwd: candidates from the LDS tile its GEMM phase wrote, MASKABLE = false): one summation sequence, the same bits.
template <typename T, int KT, int KH, int KW, int ST, int SH, int SW, bool MASKABLE>
__device__ static inline void strided_owner_resolve(const PoolKP& p, int b, int ot, int oh, int ow, int cg,
                                                    const int (&id)[(KT > ST ? 2 : 1) * (KH > SH ? 2 : 1) * (KW > SW ? 2 : 1)][PV<T>::EPL],
                                                    const float (&go)[(KT > ST ? 2 : 1) * (KH > SH ? 2 : 1) * (KW > SW ? 2 : 1)][PV<T>::EPL],
                                                    const bool (&ok)[(KT > ST ? 2 : 1) * (KH > SH ? 2 : 1) * (KW > SW ? 2 : 1)]) {
  constexpr int EPL = PV<T>::EPL;
  constexpr int NT = KT > ST ? 2 : 1, NH = KH > SH ? 2 : 1, NW = KW > SW ? 2 : 1;     // candidate windows per dimension
  // the ReLU-mask operand of every owned cell, requested with the loads above (inside the cell loop each was load -> wait -> store):
  // 1x3x3 / 2 (4 cells) 57.9 -> 54.4 us; with 8 cells the registers cost more than the round trips (3x3x3 / 2: 64.1 -> 67.6 us): not there
  constexpr bool HOIST = MASKABLE && ST * SH * SW <= 4;
  float mk[HOIST ? ST * SH * SW : 1][EPL];
  if (HOIST && p.mask) {
#pragma unroll
    for (int at = 0; at < ST; ++at)
#pragma unroll
      for (int ah = 0; ah < SH; ++ah)
#pragma unroll
        for (int aw = 0; aw < SW; ++aw) {
          const int it = min(max(ot * ST - p.pt + at, 0), p.Ti - 1), ih = min(max(oh * SH - p.ph + ah, 0), p.Hi - 1), iw = min(max(ow * SW - p.pw + aw, 0), p.Wi - 1);
          PV<T>::ld(mask_at<T>(p, in_pos(p, b, it, ih, iw), cg * EPL), mk[(at * SH + ah) * SW + aw]);
        }
  }
#pragma unroll
  for (int at = 0; at < ST; ++at)
#pragma unroll
    for (int ah = 0; ah < SH; ++ah)
#pragma unroll
      for (int aw = 0; aw < SW; ++aw) {
        const int it = ot * ST - p.pt + at, ih = oh * SH - p.ph + ah, iw = ow * SW - p.pw + aw;
        if ((unsigned)it >= (unsigned)p.Ti || (unsigned)ih >= (unsigned)p.Hi || (unsigned)iw >= (unsigned)p.Wi) continue;
        float g[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) g[e] = 0.f;
        // candidates in ascending window order (the order the simple gather kernel uses): previous window first
#pragma unroll
        for (int dt = NT - 1; dt >= 0; --dt)
#pragma unroll
          for (int dh = NH - 1; dh >= 0; --dh)
#pragma unroll
            for (int dw = NW - 1; dw >= 0; --dw) {
              const int tt = at + dt * ST, th = ah + dh * SH, tw = aw + dw * SW;
              if (tt >= KT || th >= KH || tw >= KW) continue;                    // compile-time after unrolling
              const int w = (dt * NH + dh) * NW + dw, tap = (tt * KH + th) * KW + tw;
              if (!ok[w]) continue;
#pragma unroll
              for (int e = 0; e < EPL; ++e) g[e] += id[w][e] == tap ? go[w][e] : 0.f;
            }
        // (mask_and_store written out: through the helper hipcc emits 4 - 16 % more instructions for the six owner kernels and the 1x3x3 one
        // measured 137.4 against 128.9 us on MaxPool3d_3a, DESIGN_LOG.md)
        const size_t ipos = in_pos(p, b, it, ih, iw);
        if (MASKABLE && p.mask) {
          if (!HOIST) PV<T>::ld(mask_at<T>(p, ipos, cg * EPL), mk[0]);
#pragma unroll
          for (int e = 0; e < EPL; ++e) g[e] = mk[HOIST ? (at * SH + ah) * SW + aw : 0][e] > 0.f ? g[e] : 0.f;
        }
        PV<T>::st(gin_at<T>(p, ipos, cg * EPL), g);
      }
}

template <typename T, int KT, int KH, int KW, int ST, int SH, int SW>
__global__ __launch_bounds__(256) void maxpool_strided_bwd(const PoolKP p) {
  constexpr int EPL = PV<T>::EPL;
  constexpr int NT = KT > ST ? 2 : 1, NH = KH > SH ? 2 : 1, NW = KW > SW ? 2 : 1;     // candidate windows per dimension
  static_assert(KT <= 2 * ST && KH <= 2 * SH && KW <= 2 * SW, "a cell may see at most two windows per dimension");
  const PoolTask o = simple_grid_task<T>(p, p.To, p.Wo);
  if (!o.live) return;
  const int ow = o.w, cg = o.cg, oh = o.h, ot = o.t, b = o.b;
  int id[NT * NH * NW][EPL];
  float go[NT * NH * NW][EPL];
  bool ok[NT * NH * NW];
#pragma unroll
  for (int dt = 0; dt < NT; ++dt)
#pragma unroll
    for (int dh = 0; dh < NH; ++dh)
#pragma unroll
      for (int dw = 0; dw < NW; ++dw) {
        const int w = (dt * NH + dh) * NW + dw;
        ok[w] = ot - dt >= 0 && oh - dh >= 0 && ow - dw >= 0;
        const size_t opos = out_pos(p, b, max(ot - dt, 0), max(oh - dh, 0), max(ow - dw, 0));
        PV<T>::ldidx(idx_at(p, opos, cg * EPL), id[w]);
        PV<T>::ld(gout_at<T>(p, opos, cg * EPL), go[w]);
      }
  strided_owner_resolve<T, KT, KH, KW, ST, SH, SW, true>(p, b, ot, oh, ow, cg, id, go, ok);
}

// grid of the one-thread-per-position kernels (simple_grid_task) over the input or the output grid; who: the entry point, for the message
static int simple_grid(const flk_pool_args* a, int epl, bool over_input, const char* who, dim3& grid) {
  const int Tn = over_input ? a->Ti : a->To, Hn = over_input ? a->Hi : a->Ho, Wn = over_input ? a->Wi : a->Wo;
  FLK_REQUIRE(Hn < 65536 && (long)a->B * Tn < 65536, "%s: grid too large", who);
  grid = dim3((unsigned)((Wn * (a->C / epl) + 255) / 256), (unsigned)Hn, (unsigned)(a->B * Tn));
  return FLK_OK;
}

template <typename T, int KT, int KH, int KW, int ST, int SH, int SW>
static int launch_strided_bwd(const PoolKP& kp, const flk_pool_args* a, hipStream_t s) {
  dim3 grid;
  if (int rc = simple_grid(a, PV<T>::EPL, false, "flk_maxpool3d_bwd", grid)) return rc;
  FLK_LAUNCH_KERNEL((maxpool_strided_bwd<T, KT, KH, KW, ST, SH, SW>), grid, dim3(256), 0, s, kp);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// the owner form needs a pad-before below the stride and every input cell inside some window's stride box [o*s - p, o*s - p + s)
static bool strided_owner_ok(const flk_pool_args* a, int kt, int kh, int kw, int st, int sh, int sw) {
  return a->kt == kt && a->kh == kh && a->kw == kw && a->st == st && a->sh == sh && a->sw == sw && a->pt >= 0 && a->pt < st && a->ph >= 0 &&
         a->ph < sh && a->pw >= 0 && a->pw < sw && a->Ti <= a->To * st - a->pt && a->Hi <= a->Ho * sh - a->ph && a->Wi <= a->Wo * sw - a->pw;
}

// ------------------------------------------------------------------------------------------------
// LDS-tiled variants for stride-1 SAME pooling with a window of at least 8 taps, odd or even (the Inception branch-3 pool, i3d.py:212):
// every cell is touched by kt*kh*kw windows, so the simple kernels above read each byte 27x through L1/L2.
// Here a workgroup stages the halo box of ONE 64-byte channel slab once (same 4-plane LDS image as
// conv_igemm.hip) and all window taps are LDS reads.
struct PoolTP {
  PoolKP k;
  int Tt, Ht, Wt, nTt, nTh, nTw, Th, Hh, Wh, P, plane_b, rows, ntiles, nslab;
  int dbg;             // timing experiments only (FLK_PF_DBG, W-run forward): 1 = no halo loads, 2 = no column maxima, 4 = no stores
  int fx_e;            // fixed-point exponent E of the bf16 scatter backward (fixed_point_exponent)
};

__device__ static inline int pplane_off(int c, int plane_b) { return c * plane_b + (c >> 1) * 32; }

// 1-D grid -> (tile, channel slab).  Workgroups are dealt to the 8 XCDs round-robin, so the slabs of ONE tile are put
// on consecutive slots of the SAME XCD: together they touch whole cache lines of every position while those lines
// are still in that XCD's L2 (a slab is only 64 B of a position's row).
// Tile i sits on XCD i % 8 (dealing the tiles to the XCDs in contiguous chunks, as the convolutions do, measured 6.81 against 6.77-6.79 ms
// per step: DESIGN_LOG.md).
__device__ static inline bool tile_slab_of_block(const PoolTP& p, int& tile, int& slab) {
  const int bid = blockIdx.x, xcd = bid & 7, r = bid >> 3;
  slab = r % p.nslab;
  tile = (r / p.nslab) * 8 + xcd;                            // (the host sizes the grid as 8 * ceil(ntiles / 8) * nslab: tile_grid)
  return tile < p.ntiles;
}

// Workgroup -> its tile, the start of every tiled kernel: batch b, the tile's origin (t0, h0, w0) in the grid the kernel tiles (outputs for
// the forwards, input cells for the backwards), channel slab cslab of slabc channels, and this thread's 16-byte chunk of it (channels
// [c0, c0 + slabc / 4); chvalid: the chunk exists, c0 < C).  ok = false: a tail block of the XCD dealing, no tile.  WT: the tile's width
// where it is a compile-time constant (the W-run forward), else p.Wt.
struct PoolTileCtx { bool ok; int b, t0, h0, w0, cslab, c0; bool chvalid; };
template <int WT = 0>
__device__ static inline PoolTileCtx pool_tile(const PoolTP& p, int slabc) {
  PoolTileCtx c;
  int bid;
  c.ok = tile_slab_of_block(p, bid, c.cslab);
  const int tw = bid % p.nTw; bid /= p.nTw;
  const int th = bid % p.nTh; bid /= p.nTh;
  const int tt = bid % p.nTt;
  c.b = bid / p.nTt;
  c.c0 = c.cslab * slabc + (threadIdx.x & 3) * (slabc / 4);
  c.chvalid = c.c0 < p.k.C;
  c.t0 = tt * p.Tt; c.h0 = th * p.Ht; c.w0 = tw * (WT ? WT : p.Wt);
  return c;
}
// x / d for 0 <= x < 2^20 and a small run-time divisor d, inv = 1.0f / d: (x + 0.5) / d is never within 0.5 / d of an integer, so the float
// quotient truncates exactly -- 3 VALU operations instead of the ~40 of a 32-bit integer division (which made the index arithmetic of the
// staging / write-out loops below as expensive as the pooling itself)
__device__ static inline int qdiv(int x, float inv) { return (int)(((float)x + 0.5f) * inv); }
__device__ static inline void split3(int x, int d1, float inv1, int d2, float inv2, int& a, int& b, int& c) {   // x = (a * d1) + b * d2 + c, d1 = (rows of b) * d2
  a = qdiv(x, inv1); const int rem = x - a * d1; b = qdiv(rem, inv2); c = rem - b * d2;
}

template <typename T>
__global__ __launch_bounds__(256, 2) void maxpool_s1_tiled_fwd(const PoolTP p) {
  constexpr int EPL = PV<T>::EPL, SLABC = 4 * EPL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const PoolKP& k = p.k;
  const int tid = threadIdx.x, ch = tid & 3;
  const PoolTileCtx tc = pool_tile(p, SLABC);
  if (!tc.ok) return;
  const int b = tc.b, c0 = tc.c0, ot0 = tc.t0, oh0 = tc.h0, ow0 = tc.w0;
  const bool chvalid = tc.chvalid;
  const int it0 = ot0 - k.pt, ih0 = oh0 - k.ph, iw0 = ow0 - k.pw;
  const int HW = p.Hh * p.Wh;
  // stage the halo (-inf outside the tensor: padded cells never win)
  for (int hp = tid >> 2; hp < p.P; hp += 64) {
    int a, bq, c; split3(hp, HW, 1.0f / (float)HW, p.Wh, 1.0f / (float)p.Wh, a, bq, c);
    const int it = it0 + a, ih = ih0 + bq, iw = iw0 + c;
    float v[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) v[e] = -INFINITY;
    if (chvalid && (unsigned)it < (unsigned)k.Ti && (unsigned)ih < (unsigned)k.Hi && (unsigned)iw < (unsigned)k.Wi)
      PV<T>::ld(in_at<T>(k, in_pos(k, b, it, ih, iw), c0), v);
    PV<T>::st(smem + pplane_off(ch, p.plane_b) + hp * 16, v);
  }
  __syncthreads();
  if (!chvalid) return;
  const int hw = p.Ht * p.Wt;
  for (int r = tid >> 2; r < p.rows; r += 64) {
    int rt, rh, rw; split3(r, hw, 1.0f / (float)hw, p.Wt, 1.0f / (float)p.Wt, rt, rh, rw);
    const int ot = ot0 + rt, oh = oh0 + rh, ow = ow0 + rw;
    if (ot >= k.To || oh >= k.Ho || ow >= k.Wo) continue;
    const char* base = smem + pplane_off(ch, p.plane_b) + ((rt * p.Hh + rh) * p.Wh + rw) * 16;
    float best[EPL];
    int bi[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    int tap = 0;
    for (int dt = 0; dt < k.kt; ++dt)
      for (int dh = 0; dh < k.kh; ++dh)
        for (int dw = 0; dw < k.kw; ++dw, ++tap) {
          float v[EPL];
          PV<T>::ld(base + ((dt * p.Hh + dh) * p.Wh + dw) * 16, v);
#pragma unroll
          for (int e = 0; e < EPL; ++e)
            if (v[e] > best[e]) { best[e] = v[e]; bi[e] = tap; }
        }
    if (k.relu_input) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) bi[e] = best[e] > 0.f ? bi[e] : 255;
    }
    store_out_idx<T>(k, out_pos(k, b, ot, oh, ow), c0, best, bi);
  }
}

// bf16 3x3x3 fast path (the W-run kernel below): the halo holds SORTABLE 16-bit keys (key = bits ^ (sign ? 0xffff : 0x8000): unsigned
// order == float order); one element-tap costs 2 VALU ops: pack (key << 16 | tag), the tag falling with the tap, and v_max_u32 -- the
// larger low byte wins among equal keys, i.e. the FIRST maximum in scan order.  Taps are compile-time so the LDS reads batch.
// DEVIATION from "values compare as numbers": key(-0.0) = 0x7fff < key(+0.0) = 0x8000, so in a window whose maximum is zero a +0.0
// beats an EARLIER -0.0 (the float kernels and torch take the first of the two).  The recorded tap still names an in-bounds cell whose
// value equals the window maximum, and out is a zero; only which of the tied zero cells receives the gradient differs.  Inputs here
// are ReLU outputs (+0.0 only), where the two rules agree.
__device__ static inline uint32_t bf16x2_to_keys(uint32_t w) {
  const uint32_t sign = w & 0x80008000u;                 // per half: 0x8000 if negative
  const uint32_t flip = (sign >> 15) * 0x7fffu;          // 0x7fff for negative halves
  return w ^ (flip | 0x80008000u);                       // negative: ^0xffff, non-negative: ^0x8000
}
__device__ static inline uint32_t keys_to_bf16x2(uint32_t k) {
  const uint32_t neg = (~k) & 0x80008000u;               // original sign set <=> key top bit clear
  const uint32_t flip = (neg >> 15) * 0x7fffu;
  return k ^ (flip | 0x80008000u);
}

// W-run form of the bf16 3x3x3 forward: a thread owns one (t, h) of the tile, 8 channels and the whole run of WT outputs along w.  The
// 9-tap maximum over (dt, dh) of a halo column is computed ONCE and shared by the three outputs whose windows contain it -- (WT+2) * 9
// element-taps per WT outputs instead of WT * 27 (2.1x fewer VALU operations at WT = 7; the pool is VALU-bound).  Tie rule unchanged:
// the column stage tags a candidate with 255 - 3*(3 dt + dh), the combine stage subtracts dw, so the low byte is 255 - tap and the
// larger one (first maximum in scan order) wins among equal keys.
// plane of channel chunk c in the W-run kernel's halo image: 64 bytes of skew per plane.  gfx950 serves a ds_read_b128 / ds_write_b128 16
// lanes at a time (16 x 16 bytes = the 64 banks) and in one pass iff the lanes' 16-byte units differ mod 16; the 16 lanes are 4 (t, h)
// pairs x 4 channel chunks, the pairs' slots one halo row (WT + 2 = 9: odd) apart, so units 4 c + 9 j are all different.  The 32 bytes
// per plane PAIR of pplane_off put chunks 0 / 1 and 2 / 3 on the same banks: rocprofv3 counted SQ_LDS_BANK_CONFLICT = 65 % of this
// kernel's SQ_LDS_IDX_ACTIVE (four passes per read), as many LDS cycles per column as its VALU cycles.
__device__ static inline int wplane_off(int c, int plane_b) { return c * (plane_b + 64); }

// the key epilogue: 8 winners (key << 16 | tag, tag = 27 - tap) -> the bf16 x 8 maxima and the argmax bytes; relu_input: a maximum <= 0
// (key <= 0x8000) clears the tag, and tag 0 -> 255 ("no cell")
__device__ static inline void keys_to_out_idx(uint32_t (&best)[8], int relu_input, uint4& o, uint2& id) {
  o.x = keys_to_bf16x2((best[0] >> 16) | (best[1] & 0xffff0000u));
  o.y = keys_to_bf16x2((best[2] >> 16) | (best[3] & 0xffff0000u));
  o.z = keys_to_bf16x2((best[4] >> 16) | (best[5] & 0xffff0000u));
  o.w = keys_to_bf16x2((best[6] >> 16) | (best[7] & 0xffff0000u));
  if (relu_input) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if ((best[e] >> 16) <= 0x8000u) best[e] &= ~255u;
  }
  uint32_t ix[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { const uint32_t tg = best[e] & 255u; ix[e] = tg ? 27u - tg : 255u; }
  id.x = ix[0] | (ix[1] << 8) | (ix[2] << 16) | (ix[3] << 24);
  id.y = ix[4] | (ix[5] << 8) | (ix[6] << 16) | (ix[7] << 24);
}

template <int WT>
__global__ __launch_bounds__(256, 2) void maxpool_s1_wrun_fwd_bf16(const PoolTP p) {
  constexpr int SLABC = 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const PoolKP& k = p.k;
  const int tid = threadIdx.x, ch = tid & 3;
  const PoolTileCtx tc = pool_tile<WT>(p, SLABC);
  if (!tc.ok) return;
  const int b = tc.b, c0 = tc.c0, ot0 = tc.t0, oh0 = tc.h0, ow0 = tc.w0;
  const bool chvalid = tc.chvalid;
  const int it0 = ot0 - 1, ih0 = oh0 - 1, iw0 = ow0 - 1;
  constexpr int WH = WT + 2;                                   // = p.Wh
  const int HW = p.Hh * WH;
  const float inv_HW = 1.0f / (float)HW;                       // (hp + 0.5) / HW is never within 0.5 / HW of an integer: the float quotient truncates exactly
  // staging, SU halo positions per thread and pass (the whole halo in one pass: P <= 1008): the loads are requested together (as a
  // plain loop hipcc emitted load -> wait -> convert -> ds_write per position: 14 exposed memory round trips per workgroup)
  constexpr int SU = 16;
  for (int hp0 = tid >> 2; hp0 < p.P; hp0 += 64 * SU) {
    uint4 v[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int hp = hp0 + 64 * u;
      const int a = (int)(((float)hp + 0.5f) * inv_HW), rem = hp - a * HW, bq = rem / WH, c = rem - bq * WH;
      const int it = it0 + a, ih = ih0 + bq, iw = iw0 + c;
      v[u] = make_uint4(0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u);     // -inf
      if (hp < p.P && chvalid && (unsigned)it < (unsigned)k.Ti && (unsigned)ih < (unsigned)k.Hi && (unsigned)iw < (unsigned)k.Wi && !PF_DBG(1))
        v[u] = *(const uint4*)in_at<bf16_t>(k, in_pos(k, b, it, ih, iw), c0);
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int hp = hp0 + 64 * u;
      if (hp >= p.P) break;
      uint4 w = v[u];
      w.x = bf16x2_to_keys(w.x); w.y = bf16x2_to_keys(w.y); w.z = bf16x2_to_keys(w.z); w.w = bf16x2_to_keys(w.w);
      *(uint4*)(smem + wplane_off(ch, p.plane_b) + hp * 16) = w;
    }
  }
  __syncthreads();
  if (!chvalid) return;
  const int npairs = p.Tt * p.Ht;
  for (int pr = tid >> 2; pr < npairs; pr += 64) {
    const int rt = qdiv(pr, 1.0f / (float)p.Ht), rh = pr - rt * p.Ht;
    const int ot = ot0 + rt, oh = oh0 + rh;
    if (ot >= k.To || oh >= k.Ho) continue;
    const char* base = smem + wplane_off(ch, p.plane_b) + ((rt * p.Hh + rh) * WH) * 16;
    uint32_t cm[3][8];
    auto colmax = [&](int c, uint32_t (&m)[8]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = 0;
      uint4 tapv[9];                                  // the 9 reads of the column are requested together
#pragma unroll
      for (int dt = 0; dt < 3; ++dt)
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) tapv[dt * 3 + dh] = *(const uint4*)(base + ((dt * p.Hh + dh) * WH + c) * 16);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dt = 0; dt < 3; ++dt)
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
          // tag = 27 - tap of (dt, dh, dw = 0): small enough for an inline constant, so the high-half key is ONE v_and_or_b32
          // (with 255 - tap the mask and the tag were two literals: v_and + v_or)
          const uint32_t tag = 27u - 3u * (uint32_t)(dt * 3 + dh);
          const uint4 v = tapv[dt * 3 + dh];
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            m[2 * i] = max(m[2 * i], (w[i] << 16) | tag);
            m[2 * i + 1] = max(m[2 * i + 1], (w[i] & 0xffff0000u) | tag);
          }
        }
    };
    if PF_DBG(2) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cm[0][e] = cm[1][e] = cm[2][e] = (unsigned)(tid + e) << 8;
    }
    if (!PF_DBG(2)) { colmax(0, cm[0]); colmax(1, cm[1]); }
#pragma unroll
    for (int rw = 0; rw < WT; ++rw) {
      if (!PF_DBG(2)) colmax(rw + 2, cm[(rw + 2) % 3]);
      const int ow = ow0 + rw;
      if (ow >= k.Wo) continue;
      const uint32_t (&l)[8] = cm[rw % 3];
      const uint32_t (&m)[8] = cm[(rw + 1) % 3];
      const uint32_t (&r)[8] = cm[(rw + 2) % 3];
      uint32_t best[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) best[e] = max(max(l[e], m[e] - 1u), r[e] - 2u);
      uint4 o;
      uint2 id;
      keys_to_out_idx(best, k.relu_input, o, id);
      const size_t opos = out_pos(k, b, ot, oh, ow);
      if PF_DBG(4) { if (o.x == 0x12345u && id.x == 0x777u) *(uint2*)idx_at(k, opos, c0) = id; continue; }
      *(uint4*)out_at<bf16_t>(k, opos, c0) = o;
      *(uint2*)idx_at(k, opos, c0) = id;
    }
  }
}

// Host side of pool_tile: the tile fields of tp for tiles t over the input or the output grid and channel slabs of slabc channels.  Returns
// the 1-D grid, 8 * ceil(ntiles / 8) * nslab workgroups (tile_slab_of_block).
static dim3 tile_grid(PoolTP& tp, const flk_pool_args* a, flk_tile t, bool over_input, int slabc) {
  const int Tn = over_input ? a->Ti : a->To, Hn = over_input ? a->Hi : a->Ho, Wn = over_input ? a->Wi : a->Wo;
  tp.Tt = t.Tt; tp.Ht = t.Ht; tp.Wt = t.Wt; tp.rows = t.Tt * t.Ht * t.Wt;
  tp.nTt = (Tn + t.Tt - 1) / t.Tt; tp.nTh = (Hn + t.Ht - 1) / t.Ht; tp.nTw = (Wn + t.Wt - 1) / t.Wt;
  tp.ntiles = a->B * tp.nTt * tp.nTh * tp.nTw; tp.nslab = (a->C + slabc - 1) / slabc;
  return dim3((unsigned)((tp.ntiles + 7) / 8 * 8 * tp.nslab));
}
// the halo box of a stride-1 tile and the size of its LDS plane (16 bytes per position and channel chunk)
static void tile_halo(PoolTP& tp, const flk_pool_args* a) {
  tp.Th = tp.Tt + a->kt - 1; tp.Hh = tp.Ht + a->kh - 1; tp.Wh = tp.Wt + a->kw - 1;
  tp.P = tp.Th * tp.Hh * tp.Wh;
  tp.plane_b = (tp.P * 16 + 255) / 256 * 256;
}

// tile of the W-run kernel: WT outputs along w, (Tt, Ht) with Tt*Ht <= 64 (one (t,h) pair per thread quad) and a halo <= 1008 positions
template <int WT>
static int launch_wrun_fwd(const PoolKP& kp, const flk_pool_args* a, hipStream_t s) {
  PoolTP tp{};
  tp.k = kp;
  int bestT = 1, bestH = 1; double bestScore = -1.0;
  for (int Tt = 1; Tt <= a->To && Tt <= 8; ++Tt)
    for (int Ht = 1; Ht <= a->Ho && Tt * Ht <= 64; ++Ht) {
      const long halo = (long)(Tt + 2) * (Ht + 2) * (WT + 2);
      if (halo > FLK_MAX_HALO) continue;
      const long tiles = (long)((a->To + Tt - 1) / Tt) * ((a->Ho + Ht - 1) / Ht);
      // useful outputs per staged halo position, discounted by idle thread quads (pairs < 64) and ragged edge tiles
      const double eff = (double)a->To * a->Ho / ((double)tiles * Tt * Ht);
      const double score = eff * (double)(Tt * Ht * WT) / (double)halo * (Tt * Ht >= 48 ? 1.0 : (double)(Tt * Ht) / 48.0);
      if (score > bestScore) { bestScore = score; bestT = Tt; bestH = Ht; }
    }
  const dim3 grid = tile_grid(tp, a, flk_tile{bestT, bestH, WT}, false, 32);
  tile_halo(tp, a);                                              // (3x3x3: Tt + 2, Ht + 2, WT + 2)
  const size_t lds = 4 * (size_t)tp.plane_b + 256;               // (wplane_off: 64 bytes of skew per plane)
#ifdef FLK_ABLATE
  tp.dbg = flk_ablate_env("FLK_PF_DBG");
#endif
  static bool attr_set[FLK_MAX_DEVICES] = {};
  if (int rc = flk_raise_lds_limit((const void*)maxpool_s1_wrun_fwd_bf16<WT>, 96 * 1024, attr_set)) return rc;
  FLK_LAUNCH_KERNEL((maxpool_s1_wrun_fwd_bf16<WT>), grid, dim3(256), lds, s, tp);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

template <typename T>
__global__ __launch_bounds__(256, 2) void maxpool_s1_tiled_bwd(const PoolTP p) {
  constexpr int EPL = PV<T>::EPL, SLABC = 4 * EPL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const PoolKP& k = p.k;
  char* const sidx = smem + 4 * p.plane_b + 64;            // [chunk][halo position][EPL bytes]
  const int tid = threadIdx.x, ch = tid & 3;
  const PoolTileCtx tc = pool_tile(p, SLABC);
  if (!tc.ok) return;
  const int b = tc.b, c0 = tc.c0, i_t0 = tc.t0, i_h0 = tc.h0, i_w0 = tc.w0;
  const bool chvalid = tc.chvalid;
  // tile of INPUT cells [i0, i0+tile); windows o with o - pad <= i <= o - pad + k-1  ->  o in [i - (k-1-pad), i + pad]
  const int o_t0 = i_t0 - (k.kt - 1 - k.pt), o_h0 = i_h0 - (k.kh - 1 - k.ph), o_w0 = i_w0 - (k.kw - 1 - k.pw);
  const int HW = p.Hh * p.Wh;
  for (int hp = tid >> 2; hp < p.P; hp += 64) {
    int a, bq, c; split3(hp, HW, 1.0f / (float)HW, p.Wh, 1.0f / (float)p.Wh, a, bq, c);
    const int ot = o_t0 + a, oh = o_h0 + bq, ow = o_w0 + c;
    uint4 g = make_uint4(0, 0, 0, 0);
    int id[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) id[e] = 255;                // never matches a tap
    if (chvalid && (unsigned)ot < (unsigned)k.To && (unsigned)oh < (unsigned)k.Ho && (unsigned)ow < (unsigned)k.Wo) {
      const size_t opos = out_pos(k, b, ot, oh, ow);
      g = *(const uint4*)gout_at<T>(k, opos, c0);
      PV<T>::ldidx(idx_at(k, opos, c0), id);
    }
    *(uint4*)(smem + pplane_off(ch, p.plane_b) + hp * 16) = g;
    PV<T>::stidx((uint8_t*)sidx + ((size_t)ch * p.P + hp) * EPL, id);
  }
  __syncthreads();
  if (!chvalid) return;
  const int hw = p.Ht * p.Wt;
  for (int r = tid >> 2; r < p.rows; r += 64) {
    int rt, rh, rw; split3(r, hw, 1.0f / (float)hw, p.Wt, 1.0f / (float)p.Wt, rt, rh, rw);
    const int it = i_t0 + rt, ih = i_h0 + rh, iw = i_w0 + rw;
    if (it >= k.Ti || ih >= k.Hi || iw >= k.Wi) continue;
    float g[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) g[e] = 0.f;
    // halo offset e (per dim) holds window o = o0 + local + e; this cell is its tap d = i - (o - pad) = k-1-e
    for (int et = 0; et < k.kt; ++et)
      for (int eh = 0; eh < k.kh; ++eh)
        for (int ew = 0; ew < k.kw; ++ew) {
          const int hp = ((rt + et) * p.Hh + rh + eh) * p.Wh + rw + ew;
          const int tap = ((k.kt - 1 - et) * k.kh + (k.kh - 1 - eh)) * k.kw + (k.kw - 1 - ew);
          int id[EPL];
          PV<T>::ldidx((const uint8_t*)sidx + ((size_t)ch * p.P + hp) * EPL, id);
          bool any = false;
#pragma unroll
          for (int e = 0; e < EPL; ++e) any |= id[e] == tap;
          if (!any) continue;
          float go[EPL];
          PV<T>::ld(smem + pplane_off(ch, p.plane_b) + hp * 16, go);
#pragma unroll
          for (int e = 0; e < EPL; ++e)
            if (id[e] == tap) g[e] += go[e];
        }
    mask_and_store<T>(k, in_pos(k, b, it, ih, iw), c0, g, k.mask != nullptr);
  }
}

// Scatter form of the backward (any stride): every OUTPUT window adds its gradient to the cell its argmax points at --
// one LDS atomic per element instead of kt*kh*kw index compares per input cell (the gather form above is VALU-bound).
// A workgroup owns a tile of INPUT cells (accumulators in LDS) and walks the windows that can reach it, reading
// idx / gout straight from global memory.
// ---- the phases the three scatter kernels (maxpool_scatter_bwd, maxpool_scatter_gemm_bwd, maxpool_scatter_gemm_bwd_reg) share ----

// The windows that reach a tile of INPUT cells with origin (i_t0, i_h0, i_w0): o in [ceil((i0 + pad - k + 1) / s),
// floor((i0 + tile - 1 + pad) / s)] per dimension, clipped to the grid -- a box of P = nt * nh * nw windows, walked by a linear index hp.
struct PoolReach {
  int i_t0, i_h0, i_w0, o_t0, o_h0, o_w0, nw, nhw, P;
  float inv_hw, inv_w;
  // window hp (0 <= hp < P) -> its linear output position and its origin relative to the tile's (window o covers cells o * s - pad + d)
  __device__ inline void decode(const PoolKP& k, int b, int hp, size_t& opos, int& lt0, int& lh0, int& lw0) const {
    const int a = (int)(((float)hp + 0.5f) * inv_hw), rem = hp - a * nhw;        // (qdiv: the float quotients truncate exactly)
    const int bq = (int)(((float)rem + 0.5f) * inv_w), c = rem - bq * nw;
    const int ot = o_t0 + a, oh = o_h0 + bq, ow = o_w0 + c;
    opos = out_pos(k, b, ot, oh, ow);
    lt0 = ot * k.st - k.pt - i_t0; lh0 = oh * k.sh - k.ph - i_h0; lw0 = ow * k.sw - k.pw - i_w0;
  }
};
__device__ static inline PoolReach pool_reach(const PoolKP& k, int i_t0, int i_h0, int i_w0, int Tt, int Ht, int Wt) {
  PoolReach r;
  r.i_t0 = i_t0; r.i_h0 = i_h0; r.i_w0 = i_w0;
  r.o_t0 = max(0, (i_t0 + k.pt - k.kt + k.st) / k.st); const int o_t1 = min(k.To - 1, (i_t0 + Tt - 1 + k.pt) / k.st);
  r.o_h0 = max(0, (i_h0 + k.ph - k.kh + k.sh) / k.sh); const int o_h1 = min(k.Ho - 1, (i_h0 + Ht - 1 + k.ph) / k.sh);
  r.o_w0 = max(0, (i_w0 + k.pw - k.kw + k.sw) / k.sw); const int o_w1 = min(k.Wo - 1, (i_w0 + Wt - 1 + k.pw) / k.sw);
  const int nt = max(0, o_t1 - r.o_t0 + 1), nh = max(0, o_h1 - r.o_h0 + 1);
  r.nw = max(0, o_w1 - r.o_w0 + 1);
  r.nhw = nh * r.nw; r.P = nt * r.nhw;
  r.inv_hw = 1.0f / (float)max(r.nhw, 1); r.inv_w = 1.0f / (float)max(r.nw, 1);
  return r;
}

// The bf16 forms accumulate in 32-bit FIXED POINT with a per-workgroup power-of-two scale: ds_add_f32 (and
// ds_cmpst_rtn_b32) run ~10x slower than the integer LDS atomics on gfx950 (measured: 0.28 ms vs 0.12 ms for the
// Mixed_3c pool), and integer sums are associative, so the result does not depend on the order the waves arrive in.
// Scale = 2^E / 2^floor(log2 max|gout|) over the windows this workgroup reads: |v * scale| < 2^(E+1) (a bf16 value times a power
// of two: an integer multiple of 2^(E-7), never rounded up to 2^(E+1)).  A cell receives at most n = ceil(kt/st) * ceil(kh/sh) *
// ceil(kw/sw) addends, and the host picks E = min(24, 30 - ceil(log2 n)) (fixed_point_exponent), so |sum| < n * 2^(E+1) <= 2^31:
// E = 24 for n <= 64 (every I3D pool: 27 addends < 2^30), 23 for n <= 128, 22 for n <= 255.  A bf16 gradient (8 significant bits)
// within 2^-(E-7) of the largest one is represented exactly; every addend is off by at most 2^-(E+1) * max|gout| and a cell by
// less than n * 2^-(E+1) * max|gout| (27 * 2^-25 * max|gout| for 3x3x3 / 1), far below the bf16 rounding of the stored result.
// fp32 mode (the parity mode) keeps exact float atomics.
// Magnitudes travel as fp32 bit patterns (they order like unsigned integers): fx_wave_max is the wave's largest, which lane 0 of every
// wave then publishes with atomicMax into the workgroup's word smax; fx_scale turns that word into the scale and its inverse.
__device__ static inline unsigned fx_wave_max(unsigned mx) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
  return mx;
}
__device__ static inline void fx_scale(unsigned smax, int fx_e, float& scale, float& inv_scale) {
  int ex = (int)(smax >> 23);                                  // biased exponent of the largest magnitude
  ex = min(max(ex, 26), 254);                                  // (inf/nan gradients are not representable; clamp)
  scale = __uint_as_float((unsigned)(127 + fx_e + 127 - ex) << 23);
  inv_scale = __uint_as_float((unsigned)(127 - fx_e - 127 + ex) << 23);
}

// Tap (an argmax byte) of the window whose origin is (lt0, lh0, lw0) relative to the tile: add(cell) with the cell's index in the tile,
// unless the cell lies outside the tile or the byte is 255 ("no cell": it decodes to dt >= kt).  m_khkw / m_kw = magic(kh * kw) /
// magic(kw): tap / d as (tap * m) >> 20.
template <typename F>
__device__ static inline void scatter_tap_cell(const PoolTP& p, int tap, unsigned m_khkw, unsigned m_kw, int lt0, int lh0, int lw0, F add) {
  const PoolKP& k = p.k;
  const int dt = (int)(((unsigned)tap * m_khkw) >> 20), r2 = tap - dt * (k.kh * k.kw);
  const int dh = (int)(((unsigned)r2 * m_kw) >> 20), dw = r2 - dh * k.kw;
  const int lt = lt0 + dt, lh = lh0 + dh, lw = lw0 + dw;
  if ((unsigned)lt < (unsigned)p.Tt && (unsigned)lh < (unsigned)p.Ht && (unsigned)lw < (unsigned)p.Wt && dt < k.kt) add((lt * p.Ht + lh) * p.Wt + lw);
}

// Write the tile: thread = (cell r, 16-byte channel chunk); cells past the tensor's edge are skipped.  Element e of cell r sits at
// acc0[e * es + r] (acc0: this chunk's first accumulator plane), as a fixed-point integer (FIXED) or a float.
template <typename T, bool FIXED, bool MASKABLE>
__device__ static inline void write_tile(const PoolTP& p, const PoolTileCtx& tc, const float* acc0, int es, float inv_scale) {
  constexpr int EPL = PV<T>::EPL;
  const PoolKP& k = p.k;
  const int hw = p.Ht * p.Wt;
  for (int r = threadIdx.x >> 2; r < p.rows; r += 64) {
    int rt, rh, rw; split3(r, hw, 1.0f / (float)hw, p.Wt, 1.0f / (float)p.Wt, rt, rh, rw);
    const int it = tc.t0 + rt, ih = tc.h0 + rh, iw = tc.w0 + rw;
    if (it >= k.Ti || ih >= k.Hi || iw >= k.Wi) continue;
    float g[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) g[e] = FIXED ? (float)(int)__float_as_uint(acc0[e * es + r]) * inv_scale : acc0[e * es + r];
    mask_and_store<T>(k, in_pos(k, tc.b, it, ih, iw), tc.c0, g, MASKABLE && k.mask);
  }
}

template <typename T>
__global__ __launch_bounds__(256, 4) void maxpool_scatter_bwd(const PoolTP p, unsigned m_khkw, unsigned m_kw) {
  constexpr int EPL = PV<T>::EPL, SLABC = 4 * EPL, UNR = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // accumulators [e][chunk][cell], plane stride RS = 16 (mod 64) floats: the 64 lanes of one ds_add_f32 (fixed e; 4
  // chunks x 16 neighbouring cells) fall on 64 different banks instead of the 4-8 a [cell][e] layout would give
  float* const acc = (float*)smem;
  const int RS = p.plane_b;
  const PoolKP& k = p.k;
  const int tid = threadIdx.x, ch = tid & 3;
  const PoolTileCtx tc = pool_tile(p, SLABC);
  if (!tc.ok) return;
  const int b = tc.b, c0 = tc.c0;
  const bool chvalid = tc.chvalid;
  const PoolReach rc = pool_reach(k, tc.t0, tc.h0, tc.w0, p.Tt, p.Ht, p.Wt);
  const int P = rc.P;
  for (int i = tid; i < 4 * RS * EPL; i += 256) acc[i] = 0.f;
  constexpr bool FIXED = sizeof(T) == 2;                     // (fixed point: see fx_scale)
  float scale = 1.f, inv_scale = 1.f;
  if (FIXED) {
    unsigned* const smax = (unsigned*)(acc + 4 * RS * EPL);
    if (tid == 0) *smax = 0u;
    __syncthreads();
    unsigned mx = 0u;
    if (chvalid)
      for (int hp = tid >> 2; hp < P; hp += 64) {
        size_t opos; int lt0, lh0, lw0;
        rc.decode(k, b, hp, opos, lt0, lh0, lw0);
        const uint4 g = *(const uint4*)gout_at<T>(k, opos, c0);
        // largest |bf16| of the 8 packed values, as an fp32 bit pattern
        const unsigned w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = max(mx, max((w[i] << 16) & 0x7fffffffu, w[i] & 0x7fff0000u));
      }
    mx = fx_wave_max(mx);
    if ((tid & 63) == 0) atomicMax(smax, mx);
    __syncthreads();
    fx_scale(*smax, p.fx_e, scale, inv_scale);
  }
  __syncthreads();
  float* const myacc = acc + ch * RS;
  if (chvalid)
    for (int base = tid >> 2; base < P; base += 64 * UNR) {
      int id[UNR][EPL];
      float go[UNR][EPL];
      int lt0[UNR], lh0[UNR], lw0[UNR];
      // all loads of the UNR positions are issued before the first atomic: one memory round trip per UNR positions
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        size_t opos;
        rc.decode(k, b, min(base + u * 64, P - 1), opos, lt0[u], lh0[u], lw0[u]);
        PV<T>::ldidx(idx_at(k, opos, c0), id[u]);
        PV<T>::ld(gout_at<T>(k, opos, c0), go[u]);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (base + u * 64 >= P) break;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          scatter_tap_cell(p, id[u][e], m_khkw, m_kw, lt0[u], lh0[u], lw0[u], [&](int cell) {
            if (FIXED) atomicAdd((unsigned*)&myacc[e * 4 * RS + cell], (unsigned)__float2int_rn(go[u][e] * scale));
            else atomicAdd(&myacc[e * 4 * RS + cell], go[u][e]);
          });
        }
      }
    }
  __syncthreads();
  if (!chvalid) return;
  write_tile<T, FIXED, true>(p, tc, myacc, 4 * RS, inv_scale);
}

// ------------------------------------------------------------------------------------------------
// Branch_3 backward of an Inception block in ONE kernel (i3d.py:211-216 backward; bf16): the data-gradient of the 1x1x1 unit
// (a GEMM with K = 32..128) computed on MFMA inside the pool's scatter backward, instead of  1x1x1 data-gradient -> HBM ->
// scatter  (two dependent launches, 2 x cur_c bytes per position through HBM, and the critical chain of every block's
// backward phase: the two 3x3x3 data-gradients it runs beside are single launches).
//   gin[cell, c] = sum_{windows w whose argmax for channel c is cell} ( sum_k g[w, k] * Wt[k, c] )
// Workgroup = (tile of INPUT cells, slab of 32 channels), as maxpool_scatter_bwd.  A wave takes 16 window positions per pass:
// their g rows are the MFMA B fragments (lane (q, m) loads g[pos m][32 ks + 8 q ..], 16 bytes, straight from global: K-contiguous),
// the slab's weights the A fragments (packed by flk_pool_gemm_weights_create, kept in registers for the whole workgroup), so a lane
// ends up with the 8 values  (position m) x (channels 16 f + 4 q + j)  in fp32 -- never rounded to bf16, never stored -- and adds
// each to the cell its saved argmax names, in 32-bit fixed point with integer LDS atomics exactly like maxpool_scatter_bwd
// (order-independent: bitwise reproducible).  The per-workgroup scale needs max |value| first: the product pass runs twice
// (max, then scatter); its MFMAs are ~1 % of the kernel.
// Fixed-point range with fp32 products: |v * scale| < 2^(E+1) is exact in fp32 (power-of-two scale) and fp32 values of 2^23 and above
// are integers, so __float2int_rn can round a product UP to 2^(E+1) only where 2^(E+1) <= 2^23, i.e. E = 22 (n <= 255 addends of at
// most 2^23: < 2^31).  For E = 23 and 24 an addend is an integer below 2^(E+1), and n <= 2^(30-E) of them stay below 2^31.  The
// error of a cell is below n * 2^-(E+1) * max|product|, as in maxpool_scatter_bwd.
struct PoolGemmP {
  PoolTP t;
  const char* g; int g_ld, g_coff, KS;       // KS = K / 32 k-steps
  const char* wpack;                          // [slab][ks][f = 0,1][64 lanes][16 B]
  int dbg;                                    // timing experiments only (FLK_PG_DBG): 1 = no atomics, 2 = no tile write, 4 = no g loads, 8 = no index loads, 16 = no zeroing
};

// MFMA operands of the two fused forms.  A: the weights of slab cslab, channels [32 cslab, +32), all K (flk_pool_gemm_weights_create's
// packing).  B: the g row of output position opos, lane (q, m) = 16 bytes of position m per k-step.
typedef __bf16 frag8 __attribute__((ext_vector_type(8)));
template <int KS>
__device__ static inline void load_wpack(const char* wpack, int cslab, int lane, frag8 (&af)[KS][2]) {
  const char* wp = wpack + ((size_t)cslab * KS * 2 * 64 + lane) * 16;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int f = 0; f < 2; ++f) af[ks][f] = *(const frag8*)(wp + (size_t)(ks * 2 + f) * 1024);
}
template <int KS>
__device__ static inline void load_g(const PoolGemmP& pg, size_t opos, int q, frag8 (&bf)[KS]) {
  const char* gp = pg.g + slice_off<bf16_t>(opos, pg.g_ld, pg.g_coff, q * 8);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) bf[ks] = *(const frag8*)(gp + ks * 64);
}

template <int KS>
__global__ __launch_bounds__(256, 4) void maxpool_scatter_gemm_bwd(const PoolGemmP pg, unsigned m_khkw, unsigned m_kw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* const acc = (unsigned*)smem;     // [32 channels][RS cells] fixed-point accumulators
  const PoolTP& p = pg.t;
  const PoolKP& k = p.k;
  const int RS = p.plane_b;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, m = lane & 15;
  const PoolTileCtx tc = pool_tile(p, 32);
  if (!tc.ok) return;
  const int b = tc.b, cslab = tc.cslab;
  const PoolReach rc = pool_reach(k, tc.t0, tc.h0, tc.w0, p.Tt, p.Ht, p.Wt);
  const int P = rc.P;
  for (int i = tid; i < 32 * RS; i += 256) acc[i] = 0u;
  unsigned* const smax = acc + 32 * RS;
  if (tid == 0) *smax = 0u;
  frag8 af[KS][2];
  load_wpack<KS>(pg.wpack, cslab, lane, af);
  auto product = [&](size_t opos, f32x4 (&v)[2]) {
    frag8 bf[KS];
    load_g<KS>(pg, opos, q, bf);
    v[0] = f32x4{0.f, 0.f, 0.f, 0.f}; v[1] = v[0];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      v[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][0], bf[ks], v[0], 0, 0, 0);
      v[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][1], bf[ks], v[1], 0, 0, 0);
    }
  };
  __syncthreads();
  // ---- pass 1: the largest |value| this workgroup will add (as an fp32 bit pattern: magnitudes order like unsigned integers) ----
  unsigned mx = 0u;
  for (int base = wave * 16; base < P; base += 64) {
    size_t opos; int lt0, lh0, lw0;
    rc.decode(k, b, min(base + m, P - 1), opos, lt0, lh0, lw0);
    f32x4 v[2];
    product(opos, v);
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int j = 0; j < 4; ++j) mx = max(mx, __float_as_uint(v[f][j]) & 0x7fffffffu);
  }
  mx = fx_wave_max(mx);
  if (lane == 0) atomicMax(smax, mx);
  __syncthreads();
  float scale, inv_scale;
  fx_scale(*smax, p.fx_e, scale, inv_scale);
  // ---- pass 2: the same products, scattered ----
  for (int base = wave * 16; base < P; base += 64) {
    const bool live = base + m < P;
    size_t opos; int lt0, lh0, lw0;
    rc.decode(k, b, min(base + m, P - 1), opos, lt0, lh0, lw0);
    unsigned ib[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) ib[f] = *(const unsigned*)idx_at(k, opos, cslab * 32 + f * 16 + q * 4);
    f32x4 v[2];
    product(opos, v);
    if (!live) continue;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        scatter_tap_cell(p, (int)((ib[f] >> (8 * j)) & 255u), m_khkw, m_kw, lt0, lh0, lw0,
                         [&](int cell) { atomicAdd(&acc[(f * 16 + q * 4 + j) * RS + cell], (unsigned)__float2int_rn(v[f][j] * scale)); });
      }
  }
  __syncthreads();
  if (!tc.chvalid) return;
  write_tile<bf16_t, true, false>(p, tc, (const float*)acc + (tid & 3) * 8 * RS, RS, inv_scale);
}

// The same kernel for tiles reached by at most 64 * NIT windows (the (4,7,7) tiles of the I3D blocks: 486): a wave's NIT passes are
// unrolled, the g rows and index bytes of NB passes are requested together (the loop form above waits for one load round trip per pass and
// per product pass -- 2 x 8 dependent round trips per workgroup: latency-bound, 1 TB/s), and the products and index bytes stay in registers
// between the max pass and the scatter pass: each is loaded and computed ONCE.  That alone changed little: the kernel is VALU-bound on the
// scatter's per-element decode (tap -> (dt,dh,dw), three bound checks, address: ~27 instructions x 8 elements x 8 passes per lane, one wave
// per SIMD and workgroup).  3x3x3 windows only: which taps of a window land inside the tile is a 27-bit mask computed once per window
// (8 elements share it), and a tap's cell offset comes from a 256-entry table in LDS: ~12 instructions per element.
// Measured (Mixed_3c, 8 x 32 x 28 x 28 x 256 channels, K = 64; tools/pool_time.py, FLK_PG_DBG ablations): loop form 192 us, this form
// 161 us; without atomics 137, without the tile write 138, without g loads 145, without index loads 138, without all of them and the
// zeroing 80 us -- what is left is the decode of 486 windows x 32 channels per 196-cell tile (2.48x the cells: the windows that reach a
// tile overlap its neighbours'), ~45 us of VALU time at ~12 instructions per element, plus the per-workgroup chain.  Tried and dropped:
// accumulator plane stride 4 / 20 (mod 64) instead of 16 (no change: the atomics are not bank-bound); the lanes of one atomic on windows 3
// apart, which cannot share an argmax cell (5 % slower: the loads lose locality, same-address serialisation is not the limit either); a
// persistent workgroup per tile that walks over its channel slabs with the decode, masks and g fragments kept and the next slab's
// weights / index bytes prefetched (169 us: 246 VGPRs, two workgroups per CU).
template <int KS, int NIT, int NB>
__global__ __launch_bounds__(256, KS >= 3 ? 2 : 3) void maxpool_scatter_gemm_bwd_reg(const PoolGemmP pg, unsigned m_khkw, unsigned m_kw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* const acc = (unsigned*)smem;     // [32 channels][RS cells] fixed-point accumulators
  const PoolTP& p = pg.t;
  const PoolKP& k = p.k;
  const int RS = p.plane_b;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, m = lane & 15;
  const PoolTileCtx tc = pool_tile(p, 32);
  if (!tc.ok) return;
  const int b = tc.b, cslab = tc.cslab;
  const PoolReach rc = pool_reach(k, tc.t0, tc.h0, tc.w0, p.Tt, p.Ht, p.Wt);
  const int P = rc.P;                                          // <= 64 * NIT (the host checks the tile)
  if (!PG_DBG(16)) for (int i = tid; i < 32 * RS; i += 256) acc[i] = 0u;
  unsigned* const smax = acc + 32 * RS;
  if (tid == 0) *smax = 0u;
  unsigned* const lut = smax + 64;                             // byte offset of tap's cell relative to the window origin's cell
  {
    const int dt = tid / 9, r2 = tid - dt * 9, dh = r2 / 3, dw = r2 - dh * 3;
    lut[tid] = tid < 27 ? (unsigned)(((dt * p.Ht + dh) * p.Wt + dw) * 4) : 0u;
  }
  f32x4 v[NIT][2];
  unsigned ib[NIT][2];
  int org[NIT];                                                // byte offset of the window origin's cell in an accumulator plane (may be negative)
  unsigned okm[NIT];                                           // bit tap = the tap's cell lies inside the tile
  unsigned mx = 0u;
  if (P > 0) {
    frag8 af[KS][2];
    load_wpack<KS>(pg.wpack, cslab, lane, af);
#pragma unroll
    for (int i0 = 0; i0 < NIT; i0 += NB) {
      frag8 bf[NB][KS];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = i0 + u;
        const int hp = wave * 16 + 64 * i + m;
        const bool live = hp < P;
        size_t opos; int lt0, lh0, lw0;
        rc.decode(k, b, min(hp, P - 1), opos, lt0, lh0, lw0);
        org[i] = ((lt0 * p.Ht + lh0) * p.Wt + lw0) * 4;
        // taps d = 0..2 of a dimension with 0 <= l0 + d < n, as 3 bits; the 27-bit mask is their outer product (bit (dt*3 + dh)*3 + dw)
        auto bits3 = [](int l0, int n) { return (7u << min(max(-l0, 0), 3)) & 7u & ((1u << min(max(n - l0, 0), 3)) - 1u); };
        const unsigned bt3 = bits3(lt0, p.Tt), bh3 = bits3(lh0, p.Ht), bw3 = bits3(lw0, p.Wt);
        const unsigned eh = (bh3 & 1u) | ((bh3 & 2u) << 2) | ((bh3 & 4u) << 4);          // spread by 3
        const unsigned et = (bt3 & 1u) | ((bt3 & 2u) << 8) | ((bt3 & 4u) << 16);         // spread by 9
        okm[i] = live ? bw3 * eh * et : 0u;
#pragma unroll
        for (int f = 0; f < 2; ++f) ib[i][f] = PG_DBG(8) ? (unsigned)(m * 0x01010101u) & 0x0f0f0f0fu : *(const unsigned*)idx_at(k, opos, cslab * 32 + f * 16 + q * 4);
        if (PG_DBG(4)) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) bf[u][ks] = af[ks][0];
        } else load_g<KS>(pg, opos, q, bf[u]);
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = i0 + u;
        v[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; v[i][1] = v[i][0];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          v[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][0], bf[u][ks], v[i][0], 0, 0, 0);
          v[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][1], bf[u][ks], v[i][1], 0, 0, 0);
        }
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int j = 0; j < 4; ++j) mx = max(mx, __float_as_uint(v[i][f][j]) & 0x7fffffffu);
      }
    }
  }
  mx = fx_wave_max(mx);
  __syncthreads();                                             // the accumulators and *smax are zero
  if (lane == 0) atomicMax(smax, mx);
  __syncthreads();
  float scale, inv_scale;
  fx_scale(*smax, p.fx_e, scale, inv_scale);
  if (P > 0) {
    // Branch-free: the 8 table reads of a window are requested together, and an element whose cell is outside the tile adds into a
    // dummy word of its own thread instead of being skipped.  (Written as  if (inside) atomicAdd(.. + lut[tap] ..)  hipcc emitted, per
    // element, exec-mask branch -> ds_read_b32 -> s_waitcnt lgkmcnt(0) -> ds_add_u32: 64 exposed LDS round trips per lane.)
    unsigned* const dummy = lut + 256 + tid;
    if (!PG_DBG(1)) {
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        char* const plane0 = (char*)acc + (size_t)(q * 4 * RS) * 4 + org[i];
        unsigned off[2][4];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int j = 0; j < 4; ++j) off[f][j] = lut[(ib[i][f] >> (8 * j)) & 255u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned tap = (ib[i][f] >> (8 * j)) & 255u;             // 255 ("no cell"): bit 31 of the mask, never set
            const bool inside = (okm[i] >> (tap & 31u)) & 1u;
            unsigned* const cell = (unsigned*)(plane0 + (size_t)((f * 16 + j) * RS) * 4 + off[f][j]);
            atomicAdd(inside ? cell : dummy, (unsigned)__float2int_rn(v[i][f][j] * scale));
          }
      }
    }
  }
  __syncthreads();
  if (!tc.chvalid || PG_DBG(2)) return;
  write_tile<bf16_t, true, false>(p, tc, (const float*)acc + (tid & 3) * 8 * RS, RS, inv_scale);
}

// the most windows that reach a (Tt, Ht, Wt) tile of input cells (pool_reach's box at its largest)
static long tile_reach(const flk_pool_args* a, int Tt, int Ht, int Wt) {
  return (long)((Tt + a->kt - 2) / a->st + 1) * ((Ht + a->kh - 2) / a->sh + 1) * ((Wt + a->kw - 2) / a->sw + 1);
}
// x / d as (x * magic(d)) >> 20 for the tap decode (x <= 255: scatter_tap_cell)
static unsigned magic(int d) { return (unsigned)(((1u << 20) + (unsigned)d - 1) / (unsigned)d); }

// input-cell tile for the scatter backward: minimise bytes moved per useful cell (tile writes + the windows read,
// which overlap between neighbouring tiles) plus a fixed per-workgroup cost
// max_reach > 0: only tiles reached by at most that many windows (the register-resident fused Branch_3 backward holds 64 x 8 of them; the
// reference's 90-frame clips -- T/2 = 45 frames in Mixed_3* -- otherwise get 5-frame tiles reached by 567 windows and the slower loop form:
// Mixed_3c 0.249 ms against 0.19 for 1.41 x the positions of the 64-frame clips)
static flk_tile choose_scatter_tile(const flk_pool_args* a, long max_reach = 0) {
  flk_tile best{1, 1, 1};
  double best_cost = 1e300;
  for (int Tt = 1; Tt <= a->Ti && Tt <= 8; ++Tt)
    for (int Ht = 1; Ht <= a->Hi && Tt * Ht <= 256; ++Ht) {
      const int wmax = 256 / (Tt * Ht) < a->Wi ? 256 / (Tt * Ht) : a->Wi;
      for (int Wt = 1; Wt <= wmax; ++Wt) {
        const double tiles = (double)((a->Ti + Tt - 1) / Tt) * ((a->Hi + Ht - 1) / Ht) * ((a->Wi + Wt - 1) / Wt);
        const double outs = (double)tile_reach(a, Tt, Ht, Wt);
        if (max_reach > 0 && outs > (double)max_reach) continue;
        const double passes = (double)(((long)outs + 255) / 256);           // 64 position threads x 4-deep unroll
        const double cost = tiles * (Tt * Ht * Wt * 16.0 + outs * 24.0 + passes * 2048.0 + 2048.0);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = flk_tile{Tt, Ht, Wt}; }
      }
    }
  return best;
}

// fixed-point exponent of the bf16 scatter forms: a cell is covered by at most n = ceil(kt/st) * ceil(kh/sh) * ceil(kw/sw) windows, each
// adding less than 2^(E+1) in magnitude; E = min(24, 30 - ceil(log2 n)) keeps n of them inside an int32 (n <= 255 taps: E >= 22)
static int fixed_point_exponent(const flk_pool_args* a) {
  const int n = ((a->kt + a->st - 1) / a->st) * ((a->kh + a->sh - 1) / a->sh) * ((a->kw + a->sw - 1) / a->sw);
  int lg = 0;
  while ((1 << lg) < n) ++lg;
  return 30 - lg < 24 ? 30 - lg : 24;
}

template <typename T>
static int launch_scatter_bwd(const PoolKP& kp, const flk_pool_args* a, hipStream_t s) {
  constexpr int EPL = PV<T>::EPL;
  PoolTP tp{};
  tp.k = kp;
  tp.fx_e = fixed_point_exponent(a);
  const dim3 grid = tile_grid(tp, a, choose_scatter_tile(a), true, 4 * EPL);
  tp.plane_b = (tp.rows + 47) / 64 * 64 + 16;                         // accumulator plane stride in floats, = 16 (mod 64)
  const size_t lds = (size_t)(4 * tp.plane_b * EPL + 256) * sizeof(float);    // <= 35 KiB (+ one dummy word per thread)
  FLK_LAUNCH_KERNEL(maxpool_scatter_bwd<T>, grid, dim3(256), lds, s, tp, magic(a->kh * a->kw), magic(a->kw));
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// stride-1 pooling whose output grid equals the input grid (SAME; odd or even window) with at least 8 taps: enough reuse to pay for the
// LDS staging
static bool use_tiled(const flk_pool_args* a) {
  return a->st == 1 && a->sh == 1 && a->sw == 1 && a->kt * a->kh * a->kw >= 8 && a->To == a->Ti && a->Ho == a->Hi &&
         a->Wo == a->Wi && a->pt < a->kt && a->ph < a->kh && a->pw < a->kw;
}

template <typename T>
static int launch_tiled(const PoolKP& kp, const flk_pool_args* a, bool bwd, hipStream_t s) {
  PoolTP tp{};
  tp.k = kp;
  constexpr int EPL = PV<T>::EPL;
  const flk_tile t = flk_choose_tile(a->To, a->Ho, a->Wo, a->kt, a->kh, a->kw, 1, 1, 1, 256, 768);   // 2 workgroups per CU
  const dim3 grid = tile_grid(tp, a, t, false, 4 * EPL);       // (To == Ti ..: the same tiles over the input grid for the backward)
  tile_halo(tp, a);
  FLK_REQUIRE(tp.P <= FLK_MAX_HALO, "maxpool tiled: halo %d too large", tp.P);
  const size_t lds = 4 * (size_t)tp.plane_b + 64 + (bwd ? (size_t)4 * tp.P * EPL + 16 : 0);
  static bool attr_fwd[FLK_MAX_DEVICES] = {}, attr_bwd[FLK_MAX_DEVICES] = {};
  if (int rc = flk_raise_lds_limit((const void*)maxpool_s1_tiled_fwd<T>, 96 * 1024, attr_fwd)) return rc;
  if (int rc = flk_raise_lds_limit((const void*)maxpool_s1_tiled_bwd<T>, 96 * 1024, attr_bwd)) return rc;
  if (bwd) FLK_LAUNCH_KERNEL(maxpool_s1_tiled_bwd<T>, grid, dim3(256), lds, s, tp);
  else if (sizeof(T) == 2 && a->kt == 3 && a->kh == 3 && a->kw == 3 && a->pt == 1 && a->ph == 1 && a->pw == 1) {
    return a->Wo % 7 == 0 ? launch_wrun_fwd<7>(kp, a, s) : launch_wrun_fwd<8>(kp, a, s);
  } else FLK_LAUNCH_KERNEL(maxpool_s1_tiled_fwd<T>, grid, dim3(256), lds, s, tp);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

static int check_pool(const flk_pool_args* a) {
  FLK_REQUIRE(a && a->in && a->idx, "flk_maxpool3d: null argument");
  FLK_REQUIRE(a->C % 8 == 0 && a->in_ld % 8 == 0 && a->in_coff % 8 == 0 && a->out_ld % 8 == 0 && a->out_coff % 8 == 0,
              "flk_maxpool3d: channel counts / strides / offsets must be multiples of 8");
  FLK_REQUIRE(a->kt * a->kh * a->kw <= 255 && a->kt > 0 && a->kh > 0 && a->kw > 0, "flk_maxpool3d: window too large");
  FLK_REQUIRE(a->B > 0 && a->To > 0 && a->Ho > 0 && a->Wo > 0 && a->st > 0 && a->sh > 0 && a->sw > 0, "flk_maxpool3d: bad dims");
  // every window must contain at least one in-bounds cell
  FLK_REQUIRE(a->pt < a->kt && a->ph < a->kh && a->pw < a->kw &&
                  (a->To - 1) * a->st - a->pt < a->Ti && (a->Ho - 1) * a->sh - a->ph < a->Hi &&
                  (a->Wo - 1) * a->sw - a->pw < a->Wi, "flk_maxpool3d: a window lies entirely in the padding");
  return FLK_OK;
}

static void fill(PoolKP& kp, const flk_pool_args* a) {
  kp.in = (const char*)a->in; kp.out = (char*)a->out; kp.idx = a->idx;
  kp.in_ld = a->in_ld; kp.in_coff = a->in_coff; kp.out_ld = a->out_ld; kp.out_coff = a->out_coff; kp.C = a->C;
  kp.B = a->B; kp.Ti = a->Ti; kp.Hi = a->Hi; kp.Wi = a->Wi; kp.To = a->To; kp.Ho = a->Ho; kp.Wo = a->Wo;
  kp.kt = a->kt; kp.kh = a->kh; kp.kw = a->kw; kp.st = a->st; kp.sh = a->sh; kp.sw = a->sw;
  kp.pt = a->pt; kp.ph = a->ph; kp.pw = a->pw;
  kp.relu_input = a->relu_input;
}

// one thread per output: the I3D windows take the unrolled kernel (fp32 3x3x3, met only in the parity mode, keeps the generic one)
template <typename T>
static int launch_simple_fwd(const PoolKP& kp, const flk_pool_args* a, hipStream_t s) {
  dim3 grid;
  if (int rc = simple_grid(a, PV<T>::EPL, false, "flk_maxpool3d_fwd", grid)) return rc;
  const int kcode = a->kt * 100 + a->kh * 10 + a->kw;
#define FLK_FWD_K(KT, KH, KW)                                                                               \
  if (kcode == KT * 100 + KH * 10 + KW) {                                                                   \
    FLK_LAUNCH_KERNEL((maxpool_fwd_kernel_k<T, KT, KH, KW>), grid, dim3(256), 0, s, kp);                    \
    FLK_CHECK_HIP(hipGetLastError());                                                                       \
    return FLK_OK;                                                                                          \
  }
  FLK_FWD_K(1, 3, 3)
  if constexpr (sizeof(T) == 2) FLK_FWD_K(3, 3, 3)
  FLK_FWD_K(2, 2, 2)
#undef FLK_FWD_K
  FLK_LAUNCH_KERNEL(maxpool_fwd_kernel<T>, grid, dim3(256), 0, s, kp);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_maxpool3d_fwd(const flk_pool_args* a, int dtype, void* stream) {
  int rc = check_pool(a);
  if (rc) return rc;
  FLK_REQUIRE(a->out, "flk_maxpool3d_fwd: null out");
  PoolKP kp{};
  fill(kp, a);
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "flk_maxpool3d_fwd: bad dtype");
  if (use_tiled(a)) return dtype == FLK_BF16 ? launch_tiled<bf16_t>(kp, a, false, (hipStream_t)stream) : launch_tiled<float>(kp, a, false, (hipStream_t)stream);
  return dtype == FLK_BF16 ? launch_simple_fwd<bf16_t>(kp, a, (hipStream_t)stream) : launch_simple_fwd<float>(kp, a, (hipStream_t)stream);
}

extern "C" int flk_maxpool3d_bwd(const flk_pool_args* a, const void* gout, int gout_ld, int gout_coff,
                                 void* gin, int gin_ld, int gin_coff, const void* mask, int mask_ld, int mask_coff,
                                 int dtype, void* stream) {
  int rc = check_pool(a);
  if (rc) return rc;
  FLK_REQUIRE(gout && gin, "flk_maxpool3d_bwd: null gradient");
  FLK_REQUIRE(gout_ld % 8 == 0 && gout_coff % 8 == 0 && gin_ld % 8 == 0 && gin_coff % 8 == 0 && mask_ld % 8 == 0 && mask_coff % 8 == 0,
              "flk_maxpool3d_bwd: ld/coff must be multiples of 8");
  PoolKP kp{};
  fill(kp, a);
  kp.gout = (const char*)gout; kp.gout_ld = gout_ld; kp.gout_coff = gout_coff;
  kp.gin = (char*)gin; kp.gin_ld = gin_ld; kp.gin_coff = gin_coff;
  kp.mask = (const char*)mask; kp.mask_ld = mask_ld; kp.mask_coff = mask_coff;
  kp.add = nullptr;
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "flk_maxpool3d_bwd: bad dtype");
  {
    hipStream_t s = (hipStream_t)stream;
#define FLK_OWNER(KT, KH, KW, ST, SH, SW)                                                                   \
    if (strided_owner_ok(a, KT, KH, KW, ST, SH, SW))                                                          \
      return dtype == FLK_BF16 ? launch_strided_bwd<bf16_t, KT, KH, KW, ST, SH, SW>(kp, a, s)                 \
                               : launch_strided_bwd<float, KT, KH, KW, ST, SH, SW>(kp, a, s)
    FLK_OWNER(1, 3, 3, 1, 2, 2); FLK_OWNER(3, 3, 3, 2, 2, 2); FLK_OWNER(2, 2, 2, 2, 2, 2);
#undef FLK_OWNER
  }
  // fp32 is the parity mode: it takes the gather form (fixed summation order) so that two fp32 runs are bitwise equal; the scatter
  // form's float LDS atomics are order-dependent in the last ulp, which Adam turns into 1e-4 relative on tiny components.  bf16 takes the
  // scatter form (32-bit fixed-point integer LDS atomics: order-independent, bitwise reproducible as well)
  if (dtype == FLK_BF16) return launch_scatter_bwd<bf16_t>(kp, a, (hipStream_t)stream);
  if (use_tiled(a)) return launch_tiled<float>(kp, a, true, (hipStream_t)stream);
  dim3 grid;
  if (int rc = simple_grid(a, PV<float>::EPL, true, "flk_maxpool3d_bwd", grid)) return rc;
  FLK_LAUNCH_KERNEL(maxpool_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, kp);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}


// ---- fused Branch_3 backward: weights + entry point -----------------------------------------------------------------------------
// wt_kc: fp32 [K][C] = the 1x1x1 unit's weight transposed, batch-norm scale folded in (Wt[k][c] = w[c][k] * scale[k]); K % 32 == 0,
// C % 8 == 0.  Packed as MFMA A fragments per (32-channel slab, 32-wide k-step, half): lane (q, m) holds Wt[32 ks + 8 q + j][32 s + 16 f + m].
extern "C" int flk_pool_gemm_weights_create(const float* wt_kc, int K, int C, void** out_dev) {
  FLK_REQUIRE(wt_kc && out_dev && K > 0 && K % 32 == 0 && K <= 128 && C > 0 && C % 8 == 0, "flk_pool_gemm_weights_create: K must be 32, 64, 96 or 128 and C a multiple of 8 "
              "(got K %d, C %d)", K, C);
  const int nslab = (C + 31) / 32, KS = K / 32;
  std::vector<uint16_t> h((size_t)nslab * KS * 2 * 64 * 8, 0);
  auto bf = [](float f) -> uint16_t {
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  };
  for (int s = 0; s < nslab; ++s)
    for (int ks = 0; ks < KS; ++ks)
      for (int f = 0; f < 2; ++f)
        for (int lane = 0; lane < 64; ++lane) {
          const int q = lane >> 4, m = lane & 15, c = s * 32 + f * 16 + m;
          for (int j = 0; j < 8; ++j) {
            const int kk = ks * 32 + q * 8 + j;
            h[((((size_t)s * KS + ks) * 2 + f) * 64 + lane) * 8 + j] = c < C ? bf(wt_kc[(size_t)kk * C + c]) : 0;
          }
        }
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, h.size() * 2);
  if (e != hipSuccess) { flk_set_error("hipMalloc(%zu): %s", h.size() * 2, hipGetErrorString(e)); return FLK_ENOMEM; }
  e = hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d); flk_set_error("hipMemcpy: %s", hipGetErrorString(e)); return FLK_EHIP; }
  *out_dev = d;
  return FLK_OK;
}
extern "C" int flk_pool_gemm_weights_destroy(void* dev) {
  if (dev) (void)hipFree(dev);
  return FLK_OK;
}

extern "C" int flk_maxpool3d_bwd_gemm(const flk_pool_args* a, const void* g, int g_ld, int g_coff, int K, const void* wpack,
                                      void* gin, int gin_ld, int gin_coff, int dtype, void* stream) {
  int rc = check_pool(a);
  if (rc) return rc;
  FLK_REQUIRE(g && wpack && gin, "flk_maxpool3d_bwd_gemm: null argument");
  FLK_REQUIRE(dtype == FLK_BF16, "flk_maxpool3d_bwd_gemm: bf16 only (fp32, the parity mode, keeps the two-launch gather path)");
  FLK_REQUIRE(K > 0 && K % 32 == 0 && K <= 128, "flk_maxpool3d_bwd_gemm: K must be 32, 64, 96 or 128 (got %d)", K);
  FLK_REQUIRE(g_ld % 8 == 0 && g_coff % 8 == 0 && g_coff + K <= g_ld && gin_ld % 8 == 0 && gin_coff % 8 == 0 && gin_coff + a->C <= gin_ld,
              "flk_maxpool3d_bwd_gemm: bad ld / coff");
  FLK_REQUIRE((size_t)a->B * a->To * a->Ho * a->Wo * (size_t)(g_ld > a->C ? g_ld : a->C) < (1ull << 31), "flk_maxpool3d_bwd_gemm: tensor too large");
  PoolGemmP pg{};
  fill(pg.t.k, a);
  pg.t.k.gin = (char*)gin; pg.t.k.gin_ld = gin_ld; pg.t.k.gin_coff = gin_coff;
  pg.g = (const char*)g; pg.g_ld = g_ld; pg.g_coff = g_coff; pg.KS = K / 32; pg.wpack = (const char*)wpack;
#ifdef FLK_ABLATE
  pg.dbg = flk_ablate_env("FLK_PG_DBG");
#endif
  const char* const reg_env = getenv("FLK_POOL_GEMM_REG");     // (read per call: the tests compare the two forms)
  const bool reg_form = !(reg_env && atoi(reg_env) == 0);
  const bool reg_able = reg_form && a->kt == 3 && a->kh == 3 && a->kw == 3;
  const flk_tile t = choose_scatter_tile(a, reg_able ? 512 : 0);
  PoolTP& tp = pg.t;
  tp.fx_e = fixed_point_exponent(a);
  const dim3 grid = tile_grid(tp, a, t, true, 32);
  { // accumulator plane stride in words: 4 (mod 64) -- the four lane groups q of an atomic (planes 4 q + j) start 16 banks apart
    // (16 (mod 64), the stride of maxpool_scatter_bwd, puts all four on the same banks)
    constexpr int res = 4;
    tp.plane_b = (tp.rows - res + 63) / 64 * 64 + res;
  }
  const size_t lds = (size_t)(32 * tp.plane_b + 64) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  const unsigned m1 = magic(a->kh * a->kw), m2 = magic(a->kw);
  // windows that can reach a tile: at most 64 * 8 -> the register-resident form
  if (reg_able && tile_reach(a, t.Tt, t.Ht, t.Wt) <= 512) {
    const size_t lds_reg = lds + (size_t)(64 + 256 + 256) * sizeof(unsigned);      // + the tap table + one dummy word per thread
    switch (pg.KS) {
      case 1: FLK_LAUNCH_KERNEL((maxpool_scatter_gemm_bwd_reg<1, 8, 4>), grid, dim3(256), lds_reg, s, pg, m1, m2); break;
      case 2: FLK_LAUNCH_KERNEL((maxpool_scatter_gemm_bwd_reg<2, 8, 4>), grid, dim3(256), lds_reg, s, pg, m1, m2); break;
      case 3: FLK_LAUNCH_KERNEL((maxpool_scatter_gemm_bwd_reg<3, 8, 2>), grid, dim3(256), lds_reg, s, pg, m1, m2); break;
      default: FLK_LAUNCH_KERNEL((maxpool_scatter_gemm_bwd_reg<4, 8, 2>), grid, dim3(256), lds_reg, s, pg, m1, m2); break;
    }
    FLK_CHECK_HIP(hipGetLastError());
    return FLK_OK;
  }
  switch (pg.KS) {
    case 1: FLK_LAUNCH_KERNEL(maxpool_scatter_gemm_bwd<1>, grid, dim3(256), lds, s, pg, m1, m2); break;
    case 2: FLK_LAUNCH_KERNEL(maxpool_scatter_gemm_bwd<2>, grid, dim3(256), lds, s, pg, m1, m2); break;
    case 3: FLK_LAUNCH_KERNEL(maxpool_scatter_gemm_bwd<3>, grid, dim3(256), lds, s, pg, m1, m2); break;
    default: FLK_LAUNCH_KERNEL(maxpool_scatter_gemm_bwd<4>, grid, dim3(256), lds, s, pg, m1, m2); break;
  }
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}


// ------------------------------------------------------------------------------------------------------------------------------------
// MaxPool3d_2a_3x3 + Conv3d_2b_1x1 in one kernel per pass (i3d.py:174-180; bf16, window (1,3,3) / stride (1,2,2) over even H, W, 64 -> 64).
// The pooled map has one consumer, the 1x1x1 unit, and so has its gradient: between producer and consumer each is a 64 x 64 GEMM per
// position, 16 MFMAs per 256 positions.  Run inside the pool kernels neither tensor crosses HBM.  Both kernels repeat the arithmetic of the
// launches they replace -- the pool bodies are the shared inlines above, the MFMA instruction, its K order (slab 0, then slab 1) and the
// epilogue (conv_common.h) are conv1x1_dma_kernel's -- so out / idx / gin are bitwise what the two launches write.
struct PoolConvFP {
  PoolKP k;            // the pool; k.out = the pooled map (written only with write_pool)
  ConvKP c;            // the 1x1x1 unit's epilogue operands and output slice; c.w = its packed A fragments [2 slabs][4][64 lanes][16 B]
  unsigned npos;
  int write_pool;
};

// Workgroup = 256 consecutive pooled positions of the flat [B,T,Ho,Wo] grid x all 64 channels.
//   pool phase: a task is (position, 8-channel group), 2048 per tile, 8 per thread, consecutive lanes = consecutive channel groups of a
//               position (maxpool_fwd_kernel_k's order).  The 18 tap loads of two tasks are requested together, then consumed; the index
//               bytes go to global memory, the pooled bf16 x 8 into LDS in conv1x1_dma_kernel's slab layout: [slab][256 positions x 64 B],
//               slot = chunk ^ g[(position >> 2) & 3], g = {0,3,2,1}.
//   GEMM phase: after one barrier, conv1x1_dma_kernel's compute: wave w owns rows [64 w, 64 w + 64), fragments bf / af, slab 0 then slab 1,
//               and its epilogue (finish_store_row_ops: scale and bias in two roundings, ReLU, one 16-byte store per 8 channels).
// LDS: 2 x 16 KiB slabs + 8 KiB weights: three workgroups per CU.
__global__ __launch_bounds__(256, 3) void maxpool133_conv1x1_fwd(const PoolConvFP p) {
  typedef Prec<bf16_t> PR;
  typedef typename PR::frag frag;
  constexpr int EPL = 8, NF = 4, NTAP = 9, TB = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, m = lane & 15;
  const PoolKP& k = p.k;
  const unsigned npos = p.npos, pos0 = blockIdx.x * 256u;
  const int gsw[4] = {0, 3, 2, 1};
  // the unit's A fragments, once per workgroup
  {
    const uint4 w0 = *(const uint4*)(p.c.w + tid * 16), w1 = *(const uint4*)(p.c.w + (tid + 256) * 16);
    *(uint4*)(smem + 32768 + tid * 16) = w0;
    *(uint4*)(smem + 32768 + (tid + 256) * 16) = w1;
  }
  // ---- pool phase ----
  const int cg = tid & 7;
  const unsigned hw = (unsigned)(k.Ho * k.Wo);
#pragma unroll 1
  for (int it0 = 0; it0 < 8; it0 += TB) {
    uint4 raw[TB][NTAP];
    bool ok[TB][NTAP];
    unsigned posv[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      posv[u] = pos0 + (unsigned)((it0 + u) * 32 + (tid >> 3));
      const unsigned pos = posv[u] < npos ? posv[u] : npos - 1;      // rows past the end: a valid window, never stored
      const unsigned bt = pos / hw, rem = pos - bt * hw;               // (kt = st = 1, pt = 0: input frame b * Ti + it = b * To + ot)
      const int oh = (int)(rem / (unsigned)k.Wo), ow = (int)(rem - (unsigned)oh * (unsigned)k.Wo);
#pragma unroll
      for (int dh = 0; dh < 3; ++dh)
#pragma unroll
        for (int dw = 0; dw < 3; ++dw) {
          const int tap = dh * 3 + dw;
          const int ih = oh * 2 - k.ph + dh, iw = ow * 2 - k.pw + dw;
          ok[u][tap] = (unsigned)ih < (unsigned)k.Hi && (unsigned)iw < (unsigned)k.Wi;
          const size_t ipos = ok[u][tap] ? (((size_t)bt * k.Hi + ih) * k.Wi + iw) : 0;      // (position 0 is always readable)
          raw[u][tap] = *(const uint4*)(k.in + (ipos * k.in_ld + k.in_coff + cg * EPL) * 2);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      float best[EPL];
      int bi[EPL];
      pool_window_scan<bf16_t, NTAP>(raw[u], ok[u], k.relu_input, best, bi);
      bf16x8 pv;
#pragma unroll
      for (int e = 0; e < EPL; ++e) pv[e] = (bf16_t)best[e];        // (PV<bf16_t>::st's conversion: exact, the values are bf16 numbers)
      if (posv[u] < npos) {
        PV<bf16_t>::stidx(k.idx + (size_t)posv[u] * k.C + cg * EPL, bi);
        if (p.write_pool) *(bf16x8*)(k.out + ((size_t)posv[u] * k.out_ld + k.out_coff + cg * EPL) * 2) = pv;
      }
      const int pl = (it0 + u) * 32 + (tid >> 3);
      *(bf16x8*)(smem + (cg >> 2) * 16384 + pl * 64 + (((cg & 3) ^ gsw[(pl >> 2) & 3]) * 16)) = pv;
    }
  }
  __syncthreads();
  // ---- GEMM phase: conv1x1_dma_kernel's compute plan ----
  int boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) boff[i] = (64 * wave + 16 * i + m) * 64 + ((q ^ gsw[(m >> 2) & 3]) * 16);
  f32x4 acc[NF][4];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[f][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const char* const sb = smem + s * 16384;
    frag bf[4], af[NF];
#pragma unroll
    for (int i = 0; i < 4; ++i) bf[i] = *(const frag*)(sb + boff[i]);
#pragma unroll
    for (int f = 0; f < NF; ++f) af[f] = *(const frag*)(smem + 32768 + ((s * NF + f) * 64 + lane) * 16);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) PR::mma(af[f], bf[i], acc[f][i]);
  }
  // ---- epilogue (conv1x1_dma_kernel's, no add / mask operand) ----
  constexpr int NG = 4 * NF / EPL;
  const int cbase = q * EPL;
  float4 sc[NG][2], bi[NG][2];
  epi_scale_bias_regs<bf16_t, NG>(p.c, cbase, sc, bi);
  uint4 none[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) none[g] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned pos = pos0 + (unsigned)(64 * wave + 16 * i + m);
    if (pos >= npos) continue;
    float v[NG][EPL];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int e = 0; e < EPL; ++e) v[g][e] = acc[(g * EPL + e) >> 2][i][(g * EPL + e) & 3];
    finish_store_row_ops<bf16_t, NG>(p.c, (size_t)pos, nullptr, cbase, v, sc, bi, none, none);
  }
}

struct PoolConvBP {
  PoolKP k;            // the pool (k.gin = the stem output's gradient)
  const char* w;       // the unit's data-gradient A fragments (batch-norm scale folded in) [2 slabs][4][64 lanes][16 B]
  const char* g;       // gradient of the unit's pre-ReLU output, already masked by its producer
  char* gp;            // the pooled map's gradient, written only when not NULL
  int g_ld, g_coff, gp_ld, gp_coff;
  int Hb, Wb, lgWb, nTh, nTw;
};
constexpr int POOL_CONV_BWD_MAXFRAG = 20;      // position fragments of the largest box with its halo: (8 + 1) x (32 + 1) = 297 positions -> 19

// Workgroup = a box of 1 x Hb x Wb windows (Hb * Wb = 256, Wb a power of two) of one frame, plus the previous row and column: an owned cell
// can be covered by window oh - 1 / ow - 1.
//   GEMM phase: Gp = W2b^T . G2b for the (Hb + 1)(Wb + 1) positions, 16 per fragment, fragments dealt round-robin to the waves.  B fragments
//               straight from global memory (rows are K-contiguous: lane (q, m) = 16 bytes of position m), all of a wave's requested before
//               the first MFMA; K = two 32-channel steps in slab order; each value rounded to bf16 exactly as the stand-alone data-gradient
//               stores it (no scale / bias / ReLU / mask: the pooled map is not a ReLU output) into the LDS tile [position][128 B].
//   pool phase: after one barrier, maxpool_strided_bwd<bf16, 1,3,3, 1,2,2>'s body (strided_owner_resolve) with the candidate gradients read
//               from the tile; the index bytes come from global memory, half of them requested before the GEMM phase.
// Positions outside the frame (the halo of boxes at oh = 0 / ow = 0, boxes cut at the right or bottom edge) compute on position 0's row and
// are never read: ok[] and the window bounds gate them exactly as in the stand-alone kernel.
__global__ __launch_bounds__(256, 3) void maxpool133_conv1x1_bwd(const PoolConvBP p) {
  typedef Prec<bf16_t> PR;
  typedef typename PR::frag frag;
  constexpr int EPL = 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, m = lane & 15;
  const PoolKP& k = p.k;
  int bid = blockIdx.x;
  const int tw = bid % p.nTw; bid /= p.nTw;
  const int th = bid % p.nTh;
  const int bt = bid / p.nTh;                    // b * To + ot
  const int b = bt / k.To, ot = bt - b * k.To;
  const int oh0 = th * p.Hb, ow0 = tw * p.Wb;
  const int Wp = p.Wb + 1, P = (p.Hb + 1) * Wp, nfrag = (P + 15) >> 4;
  const int cg = tid & 7;

  // ---- the index bytes of this thread's 8 (window, channel group) tasks, 4 candidate windows each: requested in two halves ----
  auto task_window = [&](int it, int& wh, int& ww) {
    const int wl = it * 32 + (tid >> 3);
    wh = wl >> p.lgWb; ww = wl & (p.Wb - 1);
    return oh0 + wh < k.Ho && ow0 + ww < k.Wo;
  };
  auto load_idx = [&](int it, uint2 (&r)[4]) {
    int wh, ww;
    if (!task_window(it, wh, ww)) { r[0] = r[1] = r[2] = r[3] = make_uint2(0u, 0u); return; }
    const int oh = oh0 + wh, ow = ow0 + ww;
#pragma unroll
    for (int dh = 0; dh < 2; ++dh)
#pragma unroll
      for (int dw = 0; dw < 2; ++dw) {
        const size_t opos = ((size_t)bt * k.Ho + max(oh - dh, 0)) * k.Wo + max(ow - dw, 0);
        r[dh * 2 + dw] = *(const uint2*)(k.idx + opos * k.C + cg * EPL);
      }
  };
  uint2 ia[4][4];
#pragma unroll
  for (int it = 0; it < 4; ++it) load_idx(it, ia[it]);

  // ---- GEMM phase ----
  {
    frag af[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int f = 0; f < 4; ++f) af[s][f] = *(const frag*)(p.w + ((s * 4 + f) * 64 + lane) * 16);
    constexpr int NJ = POOL_CONV_BWD_MAXFRAG / 4;
    frag bq[NJ][2];
    size_t gpos[NJ];
    bool own[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int fr = wave + 4 * j;
      own[j] = false; gpos[j] = 0;
      if (fr < nfrag) {
        const int pl = fr * 16 + m;
        const int hh = pl / Wp, wp = pl - hh * Wp;
        const int oh = oh0 - 1 + hh, ow = ow0 - 1 + wp;
        const bool inb = pl < P && (unsigned)oh < (unsigned)k.Ho && (unsigned)ow < (unsigned)k.Wo;
        gpos[j] = inb ? ((size_t)bt * k.Ho + oh) * k.Wo + ow : 0;                             // (position 0 is always readable)
        own[j] = inb && hh >= 1 && wp >= 1;                                                 // a window of this box, not its halo
        const char* gp = p.g + (gpos[j] * p.g_ld + p.g_coff + q * EPL) * 2;
        bq[j][0] = *(const frag*)gp;
        bq[j][1] = *(const frag*)(gp + 64);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int fr = wave + 4 * j;
      if (fr < nfrag) {
        f32x4 acc[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int f = 0; f < 4; ++f) PR::mma(af[s][f], bq[j][s], acc[f]);
        const int pl = fr * 16 + m;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          float v[EPL];
#pragma unroll
          for (int e = 0; e < EPL; ++e) v[e] = acc[(g * EPL + e) >> 2][(g * EPL + e) & 3];
          const uint4 r = PR::from_f32(v);
          *(uint4*)(smem + pl * 128 + g * 64 + q * 16) = r;
          if (p.gp && own[j]) *(uint4*)(p.gp + (gpos[j] * p.gp_ld + p.gp_coff + g * 32 + q * EPL) * 2) = r;
        }
      }
    }
  }
  __syncthreads();

  // ---- pool phase ----
  uint2 ib[4][4];
#pragma unroll
  for (int it = 0; it < 4; ++it) load_idx(4 + it, ib[it]);
  auto resolve = [&](int it, const uint2 (&r)[4]) {
    int wh, ww;
    if (!task_window(it, wh, ww)) return;
    const int oh = oh0 + wh, ow = ow0 + ww;
    int id[4][EPL];
    float go[4][EPL];
    bool ok[4];
#pragma unroll
    for (int dh = 0; dh < 2; ++dh)
#pragma unroll
      for (int dw = 0; dw < 2; ++dw) {
        const int w = dh * 2 + dw;
        ok[w] = oh - dh >= 0 && ow - dw >= 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { id[w][e] = (r[w].x >> (8 * e)) & 255; id[w][4 + e] = (r[w].y >> (8 * e)) & 255; }      // (PV<bf16_t>::ldidx)
        const uint4 gv = *(const uint4*)(smem + ((wh + 1 - dh) * Wp + (ww + 1 - dw)) * 128 + cg * 16);
        PR::to_f32(gv, go[w]);
      }
    strided_owner_resolve<bf16_t, 1, 3, 3, 1, 2, 2, false>(k, b, ot, oh, ow, cg, id, go, ok);
  };
#pragma unroll
  for (int it = 0; it < 4; ++it) resolve(it, ia[it]);
#pragma unroll
  for (int it = 0; it < 4; ++it) resolve(4 + it, ib[it]);
}

// why the fused kernels do not take this pool + 1x1x1 pair (a static string), or nullptr when they do
static const char* pool_conv_why_not(const flk_pool_args* a, int cin, int cout, int has_mask, int dtype) {
  if (!a) return "null pool arguments";
  if (dtype != FLK_BF16) return "bf16 only (fp32, the parity mode, keeps the two launches)";
  if (!(a->kt == 1 && a->kh == 3 && a->kw == 3 && a->st == 1 && a->sh == 2 && a->sw == 2)) return "the window must be (1,3,3) with stride (1,2,2)";
  if (!(a->B > 0 && a->To > 0 && a->Ho > 0 && a->Wo > 0)) return "bad dims";
  if (!strided_owner_ok(a, 1, 3, 3, 1, 2, 2)) return "the pool does not fit the owner-form backward";
  if (!(a->To == a->Ti && a->Hi == 2 * a->Ho && a->Wi == 2 * a->Wo && a->ph == 0 && a->pw == 0)) return "H and W must be even (SAME pad-before 0) and To == Ti";
  if (!(a->C == 64 && cin == 64 && cout == 64)) return "C, cin and cout must all be 64 (two 32-channel slabs in, one 64-channel tile out)";
  if (has_mask) return "the 1x1x1 data-gradient must not carry a mask operand";
  if ((size_t)a->B * a->To * a->Ho * a->Wo >= (1ull << 29)) return "too many positions";
  return nullptr;
}
extern "C" int flk_maxpool3d_conv1x1_eligible(const flk_pool_args* a, int cin, int cout, int has_mask, int dtype) {
  return pool_conv_why_not(a, cin, cout, has_mask, dtype) ? 0 : 1;
}
// the unit's packed weights as the kernels index them: [2 slabs][1 tap][4 fragments][64 lanes][16 B]
static int check_pool_conv_weights(const flk_conv_weights* w, const char* who) {
  FLK_REQUIRE(w && w->dev, "%s: null weights", who);
  FLK_REQUIRE(w->dtype == FLK_BF16 && w->kt == 1 && w->kh == 1 && w->kw == 1 && w->cin == 64 && w->cout == 64 && w->nslab == 2 && w->ntaps == 1 &&
                  w->cout_frags == 4 && w->cin_split == 0 && !w->stem4,
              "%s: the weights must be a bf16 1x1x1 64 -> 64 operator of exactly two slabs and four output fragments (nf 2 or 4)", who);
  return FLK_OK;
}

extern "C" int flk_maxpool3d_fwd_conv1x1(const flk_pool_args* a, const flk_conv_weights* w, const float* scale, const float* bias, int relu,
                                         void* out, int out_ld, int out_coff, int write_pool, int dtype, void* stream) {
  FLK_REQUIRE(a && a->in && a->idx && out, "flk_maxpool3d_fwd_conv1x1: null argument");
  if (int rc = check_pool_conv_weights(w, "flk_maxpool3d_fwd_conv1x1")) return rc;
  if (const char* why = pool_conv_why_not(a, w->cin, w->cout, 0, dtype)) { flk_set_error("flk_maxpool3d_fwd_conv1x1: %s", why); return FLK_EINVAL; }
  if (int rc = check_pool(a)) return rc;
  FLK_REQUIRE(a->in_ld % 8 == 0 && a->in_coff % 8 == 0 && a->in_coff + 64 <= a->in_ld && out_ld % 8 == 0 && out_coff % 8 == 0 && out_coff >= 0 &&
                  out_coff + 64 <= out_ld, "flk_maxpool3d_fwd_conv1x1: bad ld / coff");
  FLK_REQUIRE(!write_pool || (a->out && a->out_ld % 8 == 0 && a->out_coff % 8 == 0 && a->out_coff >= 0 && a->out_coff + 64 <= a->out_ld),
              "flk_maxpool3d_fwd_conv1x1: write_pool needs the pooled map's buffer (a->out, ld / coff multiples of 8)");
  PoolConvFP p{};
  fill(p.k, a);
  p.npos = (unsigned)((size_t)a->B * a->To * a->Ho * a->Wo);
  p.write_pool = write_pool ? 1 : 0;
  p.c.w = (const char*)w->dev; p.c.out = (char*)out; p.c.out2 = (char*)out;
  p.c.scale = scale; p.c.bias = bias; p.c.relu = relu ? 1 : 0;
  p.c.out_ld = out_ld; p.c.out_coff = out_coff; p.c.cout = 64; p.c.cout1 = 64; p.c.cin = 64;
  const unsigned grid = (p.npos + 255u) / 256u;
  FLK_LAUNCH_KERNEL(maxpool133_conv1x1_fwd, dim3(grid), dim3(256), 2 * 16384 + 8192, (hipStream_t)stream, p);
  flk_last_kernel_tag = "maxpool133_conv1x1_fwd";
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_maxpool3d_bwd_conv1x1(const flk_pool_args* a, const void* g, int g_ld, int g_coff, const flk_conv_weights* wb,
                                         void* gin, int gin_ld, int gin_coff, void* gpool, int gpool_ld, int gpool_coff, int dtype, void* stream) {
  FLK_REQUIRE(a && a->idx && g && gin, "flk_maxpool3d_bwd_conv1x1: null argument");
  if (int rc = check_pool_conv_weights(wb, "flk_maxpool3d_bwd_conv1x1")) return rc;
  if (const char* why = pool_conv_why_not(a, wb->cout, wb->cin, 0, dtype)) { flk_set_error("flk_maxpool3d_bwd_conv1x1: %s", why); return FLK_EINVAL; }
  if (int rc = check_pool(a)) return rc;
  FLK_REQUIRE(g_ld % 8 == 0 && g_coff % 8 == 0 && g_coff >= 0 && g_coff + 64 <= g_ld && gin_ld % 8 == 0 && gin_coff % 8 == 0 && gin_coff >= 0 &&
                  gin_coff + 64 <= gin_ld, "flk_maxpool3d_bwd_conv1x1: bad ld / coff");
  FLK_REQUIRE(!gpool || (gpool_ld % 8 == 0 && gpool_coff % 8 == 0 && gpool_coff >= 0 && gpool_coff + 64 <= gpool_ld), "flk_maxpool3d_bwd_conv1x1: bad gpool ld / coff");
  PoolConvBP p{};
  fill(p.k, a);
  p.k.in = nullptr; p.k.out = nullptr;
  p.k.gin = (char*)gin; p.k.gin_ld = gin_ld; p.k.gin_coff = gin_coff;
  p.w = (const char*)wb->dev; p.g = (const char*)g; p.g_ld = g_ld; p.g_coff = g_coff;
  p.gp = (char*)gpool; p.gp_ld = gpool_ld; p.gp_coff = gpool_coff;
  // the box: 8 x 32 or 16 x 16 windows, whichever covers the frame in fewer boxes
  const long n832 = (long)((a->Ho + 7) / 8) * ((a->Wo + 31) / 32), n1616 = (long)((a->Ho + 15) / 16) * ((a->Wo + 15) / 16);
  if (n832 <= n1616) { p.Hb = 8; p.Wb = 32; p.lgWb = 5; } else { p.Hb = 16; p.Wb = 16; p.lgWb = 4; }
  p.nTh = (a->Ho + p.Hb - 1) / p.Hb; p.nTw = (a->Wo + p.Wb - 1) / p.Wb;
  const int nfrag = ((p.Hb + 1) * (p.Wb + 1) + 15) / 16;
  FLK_REQUIRE(nfrag <= POOL_CONV_BWD_MAXFRAG, "flk_maxpool3d_bwd_conv1x1: box too large");
  const long grid = (long)a->B * a->To * p.nTh * p.nTw;
  FLK_REQUIRE(grid < (1l << 31), "flk_maxpool3d_bwd_conv1x1: grid too large");
  FLK_LAUNCH_KERNEL(maxpool133_conv1x1_bwd, dim3((unsigned)grid), dim3(256), (size_t)nfrag * 16 * 128, (hipStream_t)stream, p);
  flk_last_kernel_tag = "maxpool133_conv1x1_bwd";
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
