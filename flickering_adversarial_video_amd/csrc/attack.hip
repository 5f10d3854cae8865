// Perturbation kernels (HBM-bound): apply + clip fused with the stem's space-to-depth staging, the
// delta-gradient reduction with the clip masks, and regulariser-gradient + Adam.
//
// Reference maths: kinetics_i3d_utils.py:100-142 (apply), :172-200 (regularisers/metrics),
// i3d_adversarial_main_single_video_npy.py:56-59,79-84 (loss, TF Adam); torch dialect model.py:80-101,
// 198-209, 868.  Closed forms: SURVEY Appendix C.
#include "flk_internal.h"
#include "perturb_common.h"
#include "quant_encode.h"

// Space-to-depth layouts (template FT = flk_apply_args.fold_t, 0 -> 2):
//   FT = 1: fold (h,w) only,   16 channels: (qh*2+qw)*3 + c, 12..15 zero          (VideoResNet stems)
//   FT = 2: fold (t,h,w),      32 channels: (qt*4+qh*2+qw)*3 + c, 24..31 zero
//   FT = 3: fold (t,h,w),      32 channels: (qt*2+qh)*8 + qw*3 + c, 6 and 7 of every 8 zero -- every 16-byte chunk holds
//           ONE (qt,qh) parity, so the structurally zero (tap, parity) chunks of the folded 7x7x7 stem can be skipped
//           (conv_igemm.hip mode 4)
template <int FT> struct S2D {
  static constexpr int F = FT == 1 ? 1 : 2;                 // frames folded into one position
  static constexpr int NCH = 16 * F;
  static constexpr int NUSED = FT == 3 ? 32 : 12 * F;       // leading channels that may be non-zero
  __device__ static constexpr int ch(int qt, int qh, int k) {   // k = qw*3 + c
    return FT == 3 ? (qt * 2 + qh) * 8 + k : (qt * 4 + qh * 2) * 3 + k;
  }
  __device__ static void put(float* v, int qt, int qh, int k, float u) { v[ch(qt, qh, k)] = u; }
};
// fold_t = 4: the (h,w) fold of fold_t = 1 with every value split into TWO bf16 numbers, [B,T,H/2,W/2,32]: channel k = bf16(x_adv),
// channel 16 + k = bf16(x_adv - channel k).  The VideoResNet stems (bf16 plans) read both halves against the same weights, i.e. they
// see the perturbed clip to ~16 mantissa bits at the MFMA cost of the 16 -> 32 channel padding their K step had anyway: rounding
// x + delta/std to ONE bf16 swallows a small flicker perturbation (|delta| = 1e-4 moved the logits with the wrong sign), and the
// centred-clip + position-bias form of the I3D stem is exact only where the clamp bounds are bf16 numbers -- here 5-8 % of the
// values of a clip sit AT a bound, and bf16(bound - p) jumps by a whole ulp for all of them at once (measured: wrong sign at
// |delta| = 5e-4).
struct HiLo {
  static constexpr int F = 1, NCH = 32;
  __device__ static void put(float* v, int, int qh, int k, float u) {
    const float hi = (float)(bf16_t)u;
    v[S2D<1>::ch(0, qh, k)] = hi;                        // (stored again as bf16: exact)
    v[16 + S2D<1>::ch(0, qh, k)] = u - hi;
  }
};

// six consecutive values x[b,t,h,2*w2 .. 2*w2+1, 0..2] (value i is channel i % 3); off = 6*k: a uint8 clip is read with 2-byte loads,
// an fp32 clip with 8-byte loads
__device__ static inline void load6(const flk_apply_args& a, size_t off, float* x) {
  if (a.x_is_u8) {
    uint32_t by[6];
    load_bytes<1>((const uint8_t*)a.x + off, by);
    if (a.x_lut) {                                                      // (the branch hoisted out of decode_u8's loop)
#pragma unroll
      for (int i = 0; i < 6; ++i) x[i] = a.x_lut[by[i] * 3 + i % 3];
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i) x[i] = decode_scaled(a, by[i]);
    }
  } else {
    const float2* p = (const float2*)((const float*)a.x + off);
    const float2 a0 = p[0], a1 = p[1], a2 = p[2];
    x[0] = a0.x; x[1] = a0.y; x[2] = a1.x; x[3] = a1.y; x[4] = a2.x; x[5] = a2.y;
  }
}

// perturbation added at frame t (before adv_flag): flicker_pert's over every form of delta -- the flicker [T,3] / [B,T,3], one value per
// line of a frame (delta_per_line, [Bd,T,H,3]) or per element (delta_dense, [T,H,W,3]); a branch that is uniform over the launch; the
// callers that hoist the three values of a frame take the per-element route for the last two
__device__ static inline float pert_at(const flk_apply_args& a, int b, int t, int h, int w, int c) {
  const int ts = wrap(t - a.shift_p, a.T);
  float d;
  if (a.delta_per_line) d = a.delta[(((size_t)(a.delta_per_clip ? b : 0) * a.T + ts) * a.H + h) * 3 + c];
  else d = a.delta_dense ? a.delta[(((size_t)ts * a.H + h) * a.W + w) * 3 + c] : a.delta[flicker_index(a, b, ts, c)];
  return pert_of(a, b, d, c);
}
// the same with adv_flag: the select keeps the product's rounding apart from the sum that applied() forms
__device__ static inline float adv_pert_at(const flk_apply_args& a, int b, int t, int h, int w, int c) {
  return a.adv_flag != 0.f ? a.adv_flag * pert_at(a, b, t, h, w, c) : 0.f;
}

// ---- apply: one thread = one space-to-depth output position (L::F x 2 x 2 input cells x 3 channels); L = S2D<1|2|3> or HiLo.
// A 1-D grid capped by the host; the workgroups stride over the positions ----
template <typename TO, typename L, bool QUANT>
__global__ __launch_bounds__(256) void apply_s2d_kernel(const flk_apply_args a, char* out) {
  constexpr int FT = L::F, NCH = L::NCH;
  __shared__ float ql[QUANT ? 768 : 1];
  if constexpr (QUANT) stage_q_lut(a, ql);
  const int T2 = a.T / FT, H2 = a.H / 2, W2 = a.W / 2;
  const long total = (long)a.B * T2 * H2 * W2;
  for (long gid = (long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
    long r = gid;
    const int w2 = r % W2; r /= W2;
    const int h2 = r % H2; r /= H2;
    const int t2 = r % T2;
    const int b = r / T2;
    float v[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) v[i] = 0.f;
#pragma unroll
    for (int qt = 0; qt < FT; ++qt) {
      const int t = FT * t2 + qt;
      const int tx = wrap(t - a.shift_x, a.T);      // x'[t] = x[(t - shift_x) mod T]
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        const int h = 2 * h2 + qh;
        float x[6];
        load6(a, ((((size_t)b * a.T + tx) * a.H + h) * a.W + 2 * w2) * 3, x);
#pragma unroll
        for (int qw = 0; qw < 2; ++qw)              // (this nest, not one loop over k = qw*3 + c: DESIGN_LOG.md, the strided legs)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            L::put(v, qt, qh, qw * 3 + c, perturbed<QUANT>(a, ql, x[qw * 3 + c], adv_pert_at(a, b, t, h, 2 * w2 + qw, c), c));
      }
    }
    store_ch<TO, NCH>(out + (size_t)gid * NCH * sizeof(TO), v);
  }
}

// Fast path of the uint8 clips with W % 8 == 0 (fold_t 2 / 3 flicker by scalars: the headline configuration; fold_t 4 through the decode
// table: the input of the bf16 VideoResNet plans read straight from the resident clip): one thread = 4 consecutive output positions of
// one (clip, folded frame, row pair).  It reads its 24 source bytes (8 pixels) of each of the 2 F (frame, row) pairs as three aligned
// 8-byte loads (the strided kernel above issues 2-byte loads) and decodes its position with 32-bit arithmetic from a 3-D grid
// (positions, folded frame, clip).  TABLE: decode through x_lut, staged in LDS once per workgroup (else the scalars; no table is
// reserved).  DENSE: the [T,H,W,3] or per-line [Bd,T,H,3] perturbation, per element; else [T,3] / [B,T,3], the 3 F values evaluated
// once.  Same arithmetic per element as the strided kernel, so the bytes written equal that kernel's.
template <typename TO, typename L, bool TABLE, bool DENSE, bool QUANT>
__global__ __launch_bounds__(256) void apply_s2d_u8x4_kernel(const flk_apply_args a, char* out) {
  constexpr int F = L::F, NCH = L::NCH;
  __shared__ float lut[TABLE ? 768 : 1];
  __shared__ float ql[QUANT ? 768 : 1];
  if constexpr (TABLE)
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = a.x_lut[i];
  if constexpr (QUANT) stage_q_lut(a, ql);        // (its barrier covers lut too)
  else if constexpr (TABLE) __syncthreads();
  const int H2 = a.H / 2, W2 = a.W / 2, WG = W2 / 4;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)(H2 * WG)) return;
  const int h2 = i / WG, wg = i - h2 * WG;
  const int t2 = blockIdx.y, b = blockIdx.z;
  float pv[F][3];
  if constexpr (!DENSE) {
#pragma unroll
    for (int qt = 0; qt < F; ++qt)
#pragma unroll
      for (int c = 0; c < 3; ++c) pv[qt][c] = adv_pert_at(a, b, F * t2 + qt, 0, 0, c);
  }
  uint32_t by[F][2][24];
#pragma unroll
  for (int qt = 0; qt < F; ++qt) {
    const int tx = wrap(F * t2 + qt - a.shift_x, a.T);
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
      load_bytes<4>((const uint8_t*)a.x + ((((size_t)b * a.T + tx) * a.H + 2 * h2 + qh) * a.W + 8 * wg) * 3, by[qt][qh]);
  }
  char* dst = out + ((((size_t)b * (a.T / F) + t2) * H2 + h2) * W2 + 4 * wg) * NCH * sizeof(TO);
#pragma unroll
  for (int j = 0; j < 4; ++j) {                   // output position 4*wg + j: source pixels 2j, 2j+1 of the 8-pixel run
    float v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) v[k] = 0.f;
#pragma unroll
    for (int qt = 0; qt < F; ++qt)
#pragma unroll
      for (int qh = 0; qh < 2; ++qh)
#pragma unroll
        for (int e = 0; e < 6; ++e) {              // byte 6j + e of the 24-byte run: pixel 8wg + 2j + e/3, channel e % 3
          const uint32_t byte = by[qt][qh][6 * j + e];
          float x, p;
          if constexpr (TABLE) x = lut[byte * 3 + e % 3];
          else x = decode_scaled(a, byte);
          if constexpr (DENSE) p = adv_pert_at(a, b, F * t2 + qt, 2 * h2 + qh, 8 * wg + 2 * j + e / 3, e % 3);
          else p = pv[qt][e % 3];
          L::put(v, qt, qh, e, perturbed<QUANT>(a, ql, x, p, e % 3));
        }
    store_ch<TO, NCH>(dst + (size_t)j * NCH * sizeof(TO), v);
  }
}

static int check_apply(const flk_apply_args* a) {
  FLK_REQUIRE(a && a->x && a->delta, "flk_perturb: null argument");
  FLK_REQUIRE(a->fold_t >= 0 && a->fold_t <= 4, "flk_perturb: fold_t must be 0 .. 4");
  FLK_REQUIRE(a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0 && (a->fold_t == 1 || a->fold_t == 4 || a->T % 2 == 0) && a->H % 2 == 0 && a->W % 2 == 0,
              "flk_perturb: H,W (and T when folded) must be positive and even (got %d,%d,%d)", a->T, a->H, a->W);
  FLK_REQUIRE(a->lo <= a->hi, "flk_perturb: lo > hi");
  FLK_REQUIRE(!(a->center && a->delta_dense), "flk_perturb: center = 1 is defined for the flicker perturbation [T,3] only");
  FLK_REQUIRE(!(a->delta_per_clip && a->delta_dense), "flk_perturb: delta_per_clip is defined for the flicker perturbation only");
  FLK_REQUIRE(!a->dclip_dev || a->delta_per_clip, "flk_perturb: dclip_dev (per-clip clamp bounds) needs delta_per_clip");
  FLK_REQUIRE(!(a->delta_per_line && (a->delta_dense || a->center)), "flk_perturb: delta_per_line (one value per line of a frame) excludes delta_dense and center = 1");
  FLK_REQUIRE(!a->delta_per_line || a->fold_t == 1 || a->fold_t == 4, "flk_perturb: delta_per_line is defined for fold_t 1 and 4 (the VideoResNet layouts), got fold_t %d", a->fold_t);
  FLK_REQUIRE(!a->x_lut || (a->x_is_u8 && !a->center), "flk_perturb: x_lut (per-channel decode table) needs a uint8 clip and center = 0");
  FLK_REQUIRE(!a->q_lut || (!a->center && a->q_levels > 0.f), "flk_perturb: q_lut (quantised apply) needs center = 0 and q_levels > 0");
  // load6 reads a uint8 clip with 2-byte loads and an fp32 clip with 8-byte loads (every pixel pair starts at a multiple of 6 values)
  if (a->x_is_u8) FLK_REQUIRE(((size_t)a->x & 1) == 0, "flk_perturb: a uint8 clip must be 2-byte aligned (got %p)", a->x);
  else FLK_REQUIRE(((size_t)a->x & 7) == 0, "flk_perturb: an fp32 clip must be 8-byte aligned (got %p)", a->x);
  return FLK_OK;
}

// the strided kernel: a 1-D grid of at most 16384 workgroups
template <typename TO, typename L>
static int launch_apply(const flk_apply_args* a, void* out, hipStream_t st) {
  const long total = (long)a->B * (a->T / L::F) * (a->H / 2) * (a->W / 2);
  const dim3 grid((unsigned)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256));
  if (a->q_lut) FLK_LAUNCH_KERNEL((apply_s2d_kernel<TO, L, true>), grid, dim3(256), 0, st, *a, (char*)out);
  else FLK_LAUNCH_KERNEL((apply_s2d_kernel<TO, L, false>), grid, dim3(256), 0, st, *a, (char*)out);      // (untouched by the option)
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
// the four-positions kernel: grid (positions of a folded frame / 4 / 256, folded frames, clips)
template <typename TO, typename L, bool TABLE, bool DENSE>
static int launch_apply_u8x4(const flk_apply_args* a, void* out, hipStream_t st) {
  const dim3 grid((unsigned)(((a->H / 2) * (a->W / 8) + 255) / 256), (unsigned)(a->T / L::F), (unsigned)a->B);
  if (a->q_lut) FLK_LAUNCH_KERNEL((apply_s2d_u8x4_kernel<TO, L, TABLE, DENSE, true>), grid, dim3(256), 0, st, *a, (char*)out);
  else FLK_LAUNCH_KERNEL((apply_s2d_u8x4_kernel<TO, L, TABLE, DENSE, false>), grid, dim3(256), 0, st, *a, (char*)out);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
// fold_t 0 .. 3: the layout is a template argument
template <typename TO>
static int dispatch_apply(const flk_apply_args* a, void* out, hipStream_t st) {
  const int ftl = fold_layout(a->fold_t);
  if (ftl != 1 && a->x_is_u8 && !a->x_lut && !a->delta_dense && a->W % 8 == 0 && ((size_t)a->x & 7) == 0 && a->T / 2 < 65536 && a->B < 65536)
    return ftl == 2 ? launch_apply_u8x4<TO, S2D<2>, false, false>(a, out, st) : launch_apply_u8x4<TO, S2D<3>, false, false>(a, out, st);
  return ftl == 1 ? launch_apply<TO, S2D<1>>(a, out, st) : ftl == 2 ? launch_apply<TO, S2D<2>>(a, out, st) : launch_apply<TO, S2D<3>>(a, out, st);
}

extern "C" int flk_perturb_apply_s2d(const flk_apply_args* a, void* out, int dtype, void* stream) {
  int rc = check_apply(a);
  if (rc) return rc;
  FLK_REQUIRE(out, "flk_perturb_apply_s2d: null out");
  FLK_REQUIRE(((size_t)out & 15) == 0, "flk_perturb_apply_s2d: out must be 16-byte aligned (got %p)", out);
  hipStream_t st = (hipStream_t)stream;
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "flk_perturb_apply_s2d: bad dtype");
  if (a->fold_t == 4) {
    FLK_REQUIRE(dtype == FLK_BF16 && !a->center, "flk_perturb_apply_s2d: fold_t = 4 (two bf16 numbers per value) writes bf16, uncentred");
    if (a->x_lut && a->W % 8 == 0 && ((size_t)a->x & 7) == 0 && a->T < 65536 && a->B < 65536)
      return (a->delta_dense || a->delta_per_line) ? launch_apply_u8x4<bf16_t, HiLo, true, true>(a, out, st)
                                                   : launch_apply_u8x4<bf16_t, HiLo, true, false>(a, out, st);
    return launch_apply<bf16_t, HiLo>(a, out, st);
  }
  return dtype == FLK_BF16 ? dispatch_apply<bf16_t>(a, out, st) : dispatch_apply<float>(a, out, st);
}

// ---- 8-bit export: x_adv of the apply kernels encoded to the bytes of a frame (include/flicker_hip.h; encode_q is the quantised
// apply's) ---------------------------------------------------------------------------------------------------------------------------
// One thread = one unit of the destination frame (ExportUnit, perturb_common.h).  A word is built in a register and stored once; the
// source is read as one word / float4 where it is aligned too, else per value.  Workgroups stride over the items, so the bytes do not
// depend on the grid.  STATS: per item the 12 sums are folded by export_stats_fold into stats[b][t][0..11].
template <bool STATS>
__global__ __launch_bounds__(256) void adv_export_u8_kernel(const flk_apply_args a, const flk_export_args e, uint8_t* out, int32_t* stats, int chunks,
                                                            long nitems) {
  flk_apply_args ap = a;          // what pert_at sees: the perturbation's own period
  ap.T = e.delta_T;
  const int F = a.H * a.W * 3;
  __shared__ int red[4 * 12];
  for (long item = blockIdx.x; item < nitems; item += gridDim.x) {
    long r = item;
    const int chunk = (int)(r % chunks); r /= chunks;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    uint8_t* dst = out + (size_t)(e.out_clip_offset + b) * (size_t)e.out_clip_stride + (size_t)t * F;
    ExportUnit un(dst, F, a.W, chunk);
    const int start = un.start, cnt = un.cnt;
    int acc[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    if (cnt > 0) {
      const int tx = wrap(t - a.shift_x, a.T);      // x'[t] = x[(t - shift_x) mod T]
      const size_t soff = ((size_t)b * a.T + tx) * F + start;
      float pvf[3] = {0.f, 0.f, 0.f};
      const bool per_element = a.delta_dense || a.delta_per_line;     // (per line: a unit of four bytes may span two lines)
      if (!per_element) {
#pragma unroll
        for (int k = 0; k < 3; ++k) pvf[k] = adv_pert_at(ap, b, t, 0, 0, k);
      }
      uint32_t by[4] = {0, 0, 0, 0};
      float xs[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.x_is_u8) {
        export_load_u8((const uint8_t*)a.x + soff, cnt, by);
      } else {
        const float* s = (const float*)a.x + soff;
        if (cnt == 4 && ((uintptr_t)s & 15) == 0) {
          const float4 v = *(const float4*)s;
          xs[0] = v.x; xs[1] = v.y; xs[2] = v.z; xs[3] = v.w;
        } else {
          for (int j = 0; j < cnt; ++j) xs[j] = s[j];
        }
      }
      uint32_t packed = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          const int c = un.c;
          const float x = a.x_is_u8 ? decode_u8(a, by[j], c) : xs[j];
          float pv;
          if (per_element) pv = adv_pert_at(ap, b, t, un.h, un.w, c);
          else pv = c == 0 ? pvf[0] : c == 1 ? pvf[1] : pvf[2];
          const float mul = c == 0 ? e.mul[0] : c == 1 ? e.mul[1] : e.mul[2];
          const float add = c == 0 ? e.add[0] : c == 1 ? e.add[1] : e.add[2];
          const int q = encode_q(perturbed<false>(a, nullptr, x, pv, c), mul, add, e.levels);
          if (cnt == 4) packed |= (uint32_t)q << (8 * j);
          else dst[start + j] = (uint8_t)q;
          if constexpr (STATS) {
            // clamped: the sum applied() clamps.  Exactly that sum for adv_flag 0 or 1 (adv_flag * p is then exact, so a contraction at either
            // site changes nothing); for other adv_flag values the two sites may round adv_flag * p + x differently in the last bit
            const int d = q - (a.x_is_u8 ? (int)by[j] : encode_q(x, mul, add, e.levels));
            const int cl = clamps(a, x + pv) ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 3; ++k)
              if (c == k) { acc[k][0] += d; acc[k][1] += d < 0 ? -d : d; acc[k][2] += d != 0; acc[k][3] += cl; }
          }
          un.next(a.W);
        }
      }
      if (cnt == 4) *(uint32_t*)(dst + start) = packed;
    }
    if constexpr (STATS) export_stats_fold(acc, red, stats + ((size_t)b * a.T + t) * 12);
  }
}

// arguments checked by flk_adv_export_u8 (api.cpp)
int flk_adv_export_u8_launch(const flk_apply_args* a, const flk_export_args* e, uint8_t* out, int32_t* stats, hipStream_t stream) {
  flk_export_args ee = *e;
  if (ee.delta_T == 0) ee.delta_T = a->T;
  const int F = a->H * a->W * 3;
  const int chunks = (F / 4 + 2 + 255) / 256;       // units of a frame: at most F / 4 words, a head and a tail
  const long nitems = (long)a->B * a->T * chunks;
  const unsigned grid = (unsigned)(nitems > (1L << 20) ? (1L << 20) : nitems);
  if (stats) {
    FLK_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)a->B * a->T * 12 * sizeof(int32_t), stream));
    FLK_LAUNCH_KERNEL(adv_export_u8_kernel<true>, dim3(grid), dim3(256), 0, stream, *a, ee, out, stats, chunks, nitems);
  } else {
    FLK_LAUNCH_KERNEL(adv_export_u8_kernel<false>, dim3(grid), dim3(256), 0, stream, *a, ee, out, stats, chunks, nitems);
  }
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---- delta gradient --------------------------------------------------------------------------
// stage 1: workgroup (b, t2, chunk of h2 rows) -> partials[wg][qt][c] = sum over its cells of
//          g * 1[lo <= x' + a p' <= hi]      (both clip gradients are inclusive at the bounds)
static inline int grad_nchunk(int B, int T, int H) {
  const int bt = B * (T / 2 > 0 ? T / 2 : 1), H2 = H / 2;
  int n = (1024 + bt - 1) / bt;
  if (n > H2) n = H2;
  if (n < 1) n = 1;
  return n;
}

template <typename TI, int FTL>
__global__ __launch_bounds__(256) void grad_reduce_stage1(const flk_apply_args a, const char* gx, int nchunk, float* partials) {
  constexpr int FT = S2D<FTL>::F, NCH = S2D<FTL>::NCH, NUSED = S2D<FTL>::NUSED;
  const int T2 = a.T / FT, H2 = a.H / 2, W2 = a.W / 2;
  int bid = blockIdx.x;
  const int chunk = bid % nchunk; bid /= nchunk;
  const int t2 = bid % T2;
  const int b = bid / T2;
  const int h_lo = (int)((long)H2 * chunk / nchunk), h_hi = (int)((long)H2 * (chunk + 1) / nchunk);
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int ncell = (h_hi - h_lo) * W2;
  for (int i = threadIdx.x; i < ncell; i += 256) {
    const int h2 = h_lo + i / W2, w2 = i % W2;
    float g[NUSED];
    load_ch<TI, NUSED>(gx + ((((size_t)b * T2 + t2) * H2 + h2) * W2 + w2) * NCH * sizeof(TI), g);
#pragma unroll
    for (int qt = 0; qt < FT; ++qt) {
      const int t = FT * t2 + qt, tx = wrap(t - a.shift_x, a.T);
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        const int h = 2 * h2 + qh;
        float x[6];
        load6(a, ((((size_t)b * a.T + tx) * a.H + h) * a.W + 2 * w2) * 3, x);
#pragma unroll
        for (int qw = 0; qw < 2; ++qw)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (passes(a, x[qw * 3 + c], pert_at(a, b, t, h, 2 * w2 + qw, c))) acc[qt * 3 + c] += g[S2D<FTL>::ch(qt, qh, qw * 3 + c)];
          }
      }
    }
  }
  __shared__ float red[4][6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float v = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6)
    partials[(size_t)blockIdx.x * 6 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// stage 2: thread (t,c) sums partials over (b, chunk) in a fixed order; maps frame t back to the delta
// index it was rolled from; applies adv_flag, 1/std and the delta clip mask.  delta_per_clip: one (t,c) row per clip
// (blockIdx.y = clip), summed over that clip's chunks only -- the order of a batch-1 call with the same chunk count.
__global__ void grad_reduce_stage2(const flk_apply_args a, int nchunk, const float* partials, float* gdelta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.T * 3) return;
  const int FT = fold_frames(a.fold_t);
  const int t = i / 3, c = i % 3, t2 = t / FT, qt = t % FT, T2 = a.T / FT;
  const int b_lo = a.delta_per_clip ? (int)blockIdx.y : 0, b_hi = a.delta_per_clip ? b_lo + 1 : a.B;
  float s = 0.f;
  for (int b = b_lo; b < b_hi; ++b)
    for (int k = 0; k < nchunk; ++k) s += partials[(((size_t)b * T2 + t2) * nchunk + k) * 6 + qt * 3 + c];
  const int ts = wrap(t - a.shift_p, a.T);
  const size_t dbase = a.delta_per_clip ? (size_t)b_lo * a.T * 3 : 0;
  const float d = a.delta[dbase + ts * 3 + c];
  const float dc = a.dclip_dev ? a.dclip_dev[b_lo] : a.dclip;
  gdelta[dbase + ts * 3 + c] = delta_grad_out(d, dc, s, a.adv_flag, a.inv_std[c]);
}

// stage 2 alone, for producers of stage-1 partials outside this file (stem_grad.hip)
int flk_grad_reduce_stage2_launch(const flk_apply_args* a, int nchunk, const float* partials, float* gdelta, hipStream_t s) {
  FLK_LAUNCH_KERNEL(grad_reduce_stage2, dim3((a->T * 3 + 127) / 128, a->delta_per_clip ? a->B : 1), dim3(128), 0, s, *a, nchunk, partials, gdelta);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// dense delta ("L12" baseline, kinetics_i3d_utils.py:308-521): no spatial reduction, sum over the batch.
template <typename TI, int FTL>
__global__ __launch_bounds__(256) void grad_dense_kernel(const flk_apply_args a, const char* gx, float* gdelta) {
  constexpr int FT = S2D<FTL>::F, NCH = S2D<FTL>::NCH, NUSED = S2D<FTL>::NUSED;
  const int T2 = a.T / FT, H2 = a.H / 2, W2 = a.W / 2;
  const long total = (long)T2 * H2 * W2;
  for (long gid = (long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
    long r = gid;
    const int w2 = r % W2; r /= W2;
    const int h2 = r % H2;
    const int t2 = r / H2;
    float acc[NUSED];
#pragma unroll
    for (int k = 0; k < NUSED; ++k) acc[k] = 0.f;
    for (int b = 0; b < a.B; ++b) {
      float g[NUSED];
      load_ch<TI, NUSED>(gx + ((((size_t)b * T2 + t2) * H2 + h2) * W2 + w2) * NCH * sizeof(TI), g);
#pragma unroll
      for (int qt = 0; qt < FT; ++qt) {
        const int t = FT * t2 + qt, tx = wrap(t - a.shift_x, a.T);
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
          float x[6];
          load6(a, ((((size_t)b * a.T + tx) * a.H + 2 * h2 + qh) * a.W + 2 * w2) * 3, x);
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            if (passes(a, x[k], pert_at(a, b, t, 2 * h2 + qh, 2 * w2 + k / 3, k % 3))) acc[S2D<FTL>::ch(qt, qh, k)] += g[S2D<FTL>::ch(qt, qh, k)];
          }
        }
      }
    }
#pragma unroll
    for (int qt = 0; qt < FT; ++qt)
#pragma unroll
      for (int qh = 0; qh < 2; ++qh)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int t = FT * t2 + qt, ts = wrap(t - a.shift_p, a.T), c = k % 3;
          const size_t di = (((size_t)ts * a.H + 2 * h2 + qh) * a.W + 2 * w2 + k / 3) * 3 + c;
          gdelta[di] = delta_grad_out(a.delta[di], a.dclip, acc[S2D<FTL>::ch(qt, qh, k)], a.adv_flag, a.inv_std[c]);
        }
  }
}

// per-line delta (delta_per_line with delta_per_clip; fold_t 1 / 4: the 16-channel gradient): one wave owns one (clip b, frame t, row
// pair h2) of the space-to-depth gradient and produces its 2 lines x 3 channels.  Lane l walks the positions w2 = l, l + 64, ... in
// ascending order (per position pixel 2*w2, then 2*w2 + 1), then the 64 partial sums are folded by the shuffle tree 32, 16, .., 1: one
// fixed order, no atomics, no scratch.  The mask is stage 1's (the same expression); the tail is stage 2's, per line.
template <typename TI>
__global__ __launch_bounds__(256) void grad_lines_kernel(const flk_apply_args a, const char* gx, float* gdelta) {
  const int H2 = a.H / 2, W2 = a.W / 2;
  const long nwork = (long)a.B * a.T * H2;
  const int lane = threadIdx.x & 63;
  for (long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6); item < nwork; item += (long)gridDim.x * 4) {      // uniform over the wave
    long r = item;
    const int h2 = (int)(r % H2); r /= H2;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    const int tx = wrap(t - a.shift_x, a.T);
    float p[2][3];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
#pragma unroll
      for (int c = 0; c < 3; ++c) p[qh][c] = pert_at(a, b, t, 2 * h2 + qh, 0, c);
    float acc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    for (int w2 = lane; w2 < W2; w2 += 64) {
      float g[12];
      load_ch<TI, 12>(gx + ((((size_t)b * a.T + t) * H2 + h2) * W2 + w2) * 16 * sizeof(TI), g);
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        float x[6];
        load6(a, ((((size_t)b * a.T + tx) * a.H + 2 * h2 + qh) * a.W + 2 * w2) * 3, x);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if (passes(a, x[k], p[qh][k % 3])) acc[qh][k % 3] += g[S2D<1>::ch(0, qh, k)];
        }
      }
    }
    const int ts = wrap(t - a.shift_p, a.T);
    const float dc = a.dclip_dev ? a.dclip_dev[b] : a.dclip;
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = wave_sum(acc[qh][c]);
        if (lane == 0) {
          const size_t di = ((((size_t)b * a.T + ts) * a.H) + 2 * h2 + qh) * 3 + c;
          gdelta[di] = delta_grad_out(a.delta[di], dc, v, a.adv_flag, a.inv_std[c]);
        }
      }
  }
}

extern "C" int64_t flk_perturb_grad_scratch_bytes(int B, int T, int H, int W) {
  (void)W;
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return (int64_t)B * T * grad_nchunk(1, T, H) * 6 * sizeof(float);   // covers both fold_t settings and the per-clip chunking (batch-1 chunk count)
}

// (fold_t = 4: the clip went in as two bf16 numbers per value; its gradient comes back in the 16-channel fold_t = 1 layout)
template <typename TI, int FTL>
static int launch_grad_dense(const flk_apply_args* a, const char* gx, float* gdelta, hipStream_t s) {
  const long total = (long)(a->T / S2D<FTL>::F) * (a->H / 2) * (a->W / 2);
  FLK_LAUNCH_KERNEL((grad_dense_kernel<TI, FTL>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, *a, gx, gdelta);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
template <typename TI, int FTL>
static int launch_grad_reduce(const flk_apply_args* a, const char* gx, float* gdelta, float* partials, hipStream_t s) {
  // per-clip perturbations: the chunking (= summation order) of a batch-1 call, so that clip b of a batch follows the same
  // trajectory, bit for bit in fp32, as the same clip attacked alone
  const int nchunk = grad_nchunk(a->delta_per_clip ? 1 : a->B, a->T, a->H);
  const unsigned grid = (unsigned)(a->B * (a->T / S2D<FTL>::F) * nchunk);
  FLK_LAUNCH_KERNEL((grad_reduce_stage1<TI, FTL>), dim3(grid), dim3(256), 0, s, *a, gx, nchunk, partials);
  return flk_grad_reduce_stage2_launch(a, nchunk, partials, gdelta, s);
}
template <typename TI>
static int dispatch_grad(const flk_apply_args* a, const char* gx, float* gdelta, float* partials, hipStream_t s) {
  const int ftl = fold_layout(a->fold_t);
  if (a->delta_per_line) {
    FLK_REQUIRE(a->delta_per_clip, "flk_perturb_grad_reduce: delta_per_line needs delta_per_clip (the gradient comes back per clip, [B,T,H,3])");
    const long waves = (long)a->B * a->T * (a->H / 2);
    const unsigned grid = (unsigned)((waves + 3) / 4 > 262144 ? 262144 : (waves + 3) / 4);
    FLK_LAUNCH_KERNEL(grad_lines_kernel<TI>, dim3(grid), dim3(256), 0, s, *a, gx, gdelta);
    FLK_CHECK_HIP(hipGetLastError());
    return FLK_OK;
  }
  if (a->delta_dense)
    return ftl == 1 ? launch_grad_dense<TI, 1>(a, gx, gdelta, s) : ftl == 2 ? launch_grad_dense<TI, 2>(a, gx, gdelta, s) : launch_grad_dense<TI, 3>(a, gx, gdelta, s);
  FLK_REQUIRE(partials, "flk_perturb_grad_reduce: null scratch");
  return ftl == 1 ? launch_grad_reduce<TI, 1>(a, gx, gdelta, partials, s)
       : ftl == 2 ? launch_grad_reduce<TI, 2>(a, gx, gdelta, partials, s) : launch_grad_reduce<TI, 3>(a, gx, gdelta, partials, s);
}

extern "C" int flk_perturb_grad_reduce(const flk_apply_args* a, const void* gx_s2d, int dtype, float* gdelta,
                                       float* partials, void* stream) {
  int rc = check_apply(a);
  if (rc) return rc;
  FLK_REQUIRE(gx_s2d && gdelta, "flk_perturb_grad_reduce: null argument");
  FLK_REQUIRE(((size_t)gx_s2d & 15) == 0, "flk_perturb_grad_reduce: gx_s2d must be 16-byte aligned (got %p)", gx_s2d);
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "flk_perturb_grad_reduce: bad dtype");
  return dtype == FLK_BF16 ? dispatch_grad<bf16_t>(a, (const char*)gx_s2d, gdelta, partials, (hipStream_t)stream)
                           : dispatch_grad<float>(a, (const char*)gx_s2d, gdelta, partials, (hipStream_t)stream);
}

__global__ void pack_batch_sums_kernel(const float* per_clip, int B, float prob_scale, float* out3) {
  const int k = threadIdx.x;
  if (k >= 3) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += per_clip[b * 4 + k];
  out3[k] = k == 0 ? s : s * prob_scale;
}

extern "C" int flk_pack_batch_sums(const float* per_clip, int B, float prob_scale, float* out3, void* stream) {
  FLK_REQUIRE(per_clip && out3 && B > 0, "flk_pack_batch_sums: bad arguments");
  FLK_LAUNCH_KERNEL(pack_batch_sums_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, per_clip, B, prob_scale, out3);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---- regulariser gradient + Adam / projected sign-gradient step: one workgroup, delta is [T,3] ----------------------------------
__device__ static inline float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ static inline float block_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

constexpr int ADAM_PER = 8;  // 256 threads x 8 >= 3*T  (T <= 682)

// the optimiser that consumes g_tot (template argument of the update kernels: everything up to g_tot is one body)
enum { OPT_ADAM = 0, OPT_PGD = 1 };
// l-infinity PGD: clamp(d - alpha * sgn(g), -eps, +eps).  sgn(0) = 0 (the element stays); a NaN gradient gives a NaN delta like
// torch.sign / torch.clamp do -- hence comparisons instead of fminf / fmaxf, which would swallow it.  alpha * s is exact (+-alpha, 0),
// so the subtraction rounds once whether or not it is contracted to an fma.
__device__ static inline float pgd_step(float d, float g, float alpha, float eps) {
  const float s = g > 0.f ? 1.f : g < 0.f ? -1.f : g;      // g itself where it is +-0 or NaN
  const float n = d - alpha * s;
  return n < -eps ? -eps : n > eps ? eps : n;
}

// blockIdx.x = clip (flk_perturb_reg_adam_batched: B independent perturbations, each with its own Adam state, step counter and
// "still attacking" flag, all on the device -- no host value changes between iterations, so the loop can be replayed as a graph)
// OPT_PGD: m, v are not touched (NULL); the counter is still advanced for active clips (the drivers read it as iterations spent)
template <int OPT>
__global__ __launch_bounds__(256) void reg_adam_kernel(const flk_adam_args a, const float* g_adv, float* delta, float* m, float* v,
                                                       float* scalars, int* steps, const int* active, const float* dyn_dev) {
  __shared__ float sh[4];
  const int T = a.T, N = 3 * T;
  {
    const size_t o = (size_t)blockIdx.x * N;
    g_adv += o; delta += o;
    if constexpr (OPT == OPT_ADAM) { m += o; v += o; }
    if (scalars) scalars += (size_t)blockIdx.x * 8;
  }
  const int step = steps ? steps[blockIdx.x] + 1 : a.step;        // 1-based step of THIS update
  const bool update = !active || active[blockIdx.x] != 0;         // a retired clip keeps its state; its scalars are still reported
  const float dyn = dyn_dev ? dyn_dev[blockIdx.x] : a.dyn_max_norm;
  // value the regulariser sees: raw delta (TF, kinetics_i3d_utils.py:172) or clamp(delta) (torch, model.py:1078)
  auto rv = [&](int t, int c) -> float {
    const float d = delta[wrap(t, T) * 3 + c];
    return a.torch_dialect ? clipf(d, -dyn, dyn) : d;
  };
  float nd[ADAM_PER], nm[ADAM_PER], nv[ADAM_PER];
  float s_norm = 0.f, s_diff = 0.f, s_lap = 0.f, s_abs = 0.f, s_rough = 0.f, s_max = -INFINITY, s_min = INFINITY;
  const float lr_tf = a.lr * sqrtf(1.f - powf(a.adam_b2, (float)step)) / (1.f - powf(a.adam_b1, (float)step));
  const float bc1 = 1.f - powf(a.adam_b1, (float)step), bc2s = sqrtf(1.f - powf(a.adam_b2, (float)step));
#pragma unroll
  for (int k = 0; k < ADAM_PER; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i >= N) continue;
    const int t = i / 3, c = i % 3;
    const float x0 = rv(t, c), xm1 = rv(t - 1, c), xp1 = rv(t + 1, c), xm2 = rv(t - 2, c), xp2 = rv(t + 2, c);
    const float l0 = -2.f * x0 + xm1 + xp1;         // laplacian at t, t-1, t+1
    const float lm = -2.f * xm1 + xm2 + x0;
    const float lp = -2.f * xp1 + x0 + xp2;
    const float df = x0 - xm1;
    s_norm += x0 * x0; s_diff += df * df; s_lap += l0 * l0;
    const float raw = delta[i], rawm1 = delta[wrap(t - 1, T) * 3 + c];
    s_abs += fabsf(raw); s_rough += fabsf(raw - rawm1);
    s_max = fmaxf(s_max, raw); s_min = fminf(s_min, raw);
    float greg = a.beta1 * 2.f * x0 / N + a.beta2 * 2.f * (-l0) / N + a.beta3 * 2.f * (-2.f * l0 + lm + lp) / N;
    if (a.torch_dialect && !(raw >= -dyn && raw <= dyn)) greg = 0.f;   // clamp gradient, inclusive
    const float g = a.g_scale * g_adv[i] + a.beta0 * greg;
    if constexpr (OPT == OPT_PGD) {
      nd[k] = pgd_step(raw, g, a.lr, a.torch_dialect ? dyn : a.pgd_eps);
    } else {
      const float mi = a.adam_b1 * m[i] + (1.f - a.adam_b1) * g;
      const float vi = a.adam_b2 * v[i] + (1.f - a.adam_b2) * g * g;
      nm[k] = mi; nv[k] = vi;
      if (a.torch_dialect) nd[k] = raw - (a.lr / bc1) * mi / (sqrtf(vi) / bc2s + a.adam_eps);   // torch-1.4 Adam
      else nd[k] = raw - lr_tf * mi / (sqrtf(vi) + a.adam_eps);                                   // TF-1.15 AdamOptimizer
    }
  }
  const float t_norm = block_sum(s_norm, sh), t_diff = block_sum(s_diff, sh), t_lap = block_sum(s_lap, sh);
  const float t_abs = block_sum(s_abs, sh), t_rough = block_sum(s_rough, sh);
  const float t_max = block_max(s_max, sh), t_min = -block_max(-s_min, sh);
  __syncthreads();   // every neighbour read of delta is done
  if (update) {
#pragma unroll
    for (int k = 0; k < ADAM_PER; ++k) {
      const int i = threadIdx.x + 256 * k;
      if (i >= N) continue;
      delta[i] = nd[k];
      if constexpr (OPT == OPT_ADAM) { m[i] = nm[k]; v[i] = nv[k]; }
    }
    if (threadIdx.x == 0 && steps) steps[blockIdx.x] = step;
  }
  if (threadIdx.x == 0 && scalars) {
    const float norm = t_norm / N + 1e-12f, diff = t_diff / N + 1e-12f, lap = t_lap / N + 1e-12f;
    scalars[0] = a.beta1 * norm + a.beta2 * diff + a.beta3 * lap;
    scalars[1] = norm; scalars[2] = diff; scalars[3] = lap;
    scalars[4] = t_abs / N; scalars[5] = t_rough / N; scalars[6] = t_max; scalars[7] = t_min;
  }
}

extern "C" int flk_perturb_reg_adam(const flk_adam_args* a, const float* g_adv, float* delta, float* m, float* v,
                                    float* scalars, void* stream) {
  FLK_REQUIRE(a && g_adv && delta && m && v, "flk_perturb_reg_adam: null argument");
  FLK_REQUIRE(a->T > 0 && 3 * a->T <= 256 * ADAM_PER, "flk_perturb_reg_adam: T out of range (%d)", a->T);
  FLK_REQUIRE(a->step >= 1, "flk_perturb_reg_adam: step is 1-based");
  FLK_LAUNCH_KERNEL(reg_adam_kernel<OPT_ADAM>, dim3(1), dim3(256), 0, (hipStream_t)stream, *a, g_adv, delta, m, v, scalars, (int*)nullptr, (const int*)nullptr, (const float*)nullptr);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_perturb_reg_adam_batched(const flk_adam_args* a, int nclip, const float* g_adv, float* delta, float* m, float* v,
                                            int* steps_dev, const int* active_dev, const float* dyn_max_norm_dev, float* scalars, void* stream) {
  FLK_REQUIRE(a && g_adv && delta && m && v && steps_dev, "flk_perturb_reg_adam_batched: null argument");
  FLK_REQUIRE(nclip > 0 && nclip < 65536, "flk_perturb_reg_adam_batched: bad clip count %d", nclip);
  FLK_REQUIRE(a->T > 0 && 3 * a->T <= 256 * ADAM_PER, "flk_perturb_reg_adam_batched: T out of range (%d)", a->T);
  FLK_LAUNCH_KERNEL(reg_adam_kernel<OPT_ADAM>, dim3((unsigned)nclip), dim3(256), 0, (hipStream_t)stream, *a, g_adv, delta, m, v, scalars, steps_dev, active_dev, dyn_max_norm_dev);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_perturb_reg_pgd(const flk_adam_args* a, const float* g_adv, float* delta, float* scalars, void* stream) {
  FLK_REQUIRE(a && g_adv && delta, "flk_perturb_reg_pgd: null argument");
  FLK_REQUIRE(a->T > 0 && 3 * a->T <= 256 * ADAM_PER, "flk_perturb_reg_pgd: T out of range (%d)", a->T);
  const float eps = a->torch_dialect ? a->dyn_max_norm : a->pgd_eps;
  FLK_REQUIRE(eps > 0.f, "flk_perturb_reg_pgd: the l-infinity radius (%s) must be positive (got %g)", a->torch_dialect ? "dyn_max_norm" : "pgd_eps", (double)eps);
  FLK_LAUNCH_KERNEL(reg_adam_kernel<OPT_PGD>, dim3(1), dim3(256), 0, (hipStream_t)stream, *a, g_adv, delta, (float*)nullptr, (float*)nullptr, scalars,
                     (int*)nullptr, (const int*)nullptr, (const float*)nullptr);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_perturb_reg_pgd_batched(const flk_adam_args* a, int nclip, const float* g_adv, float* delta, int* steps_dev,
                                           const int* active_dev, const float* dyn_max_norm_dev, float* scalars, void* stream) {
  FLK_REQUIRE(a && g_adv && delta && steps_dev, "flk_perturb_reg_pgd_batched: null argument");
  FLK_REQUIRE(nclip > 0 && nclip < 65536, "flk_perturb_reg_pgd_batched: bad clip count %d", nclip);
  FLK_REQUIRE(a->T > 0 && 3 * a->T <= 256 * ADAM_PER, "flk_perturb_reg_pgd_batched: T out of range (%d)", a->T);
  const float eps = a->torch_dialect ? a->dyn_max_norm : a->pgd_eps;      // (per-clip radii on the device replace dyn_max_norm)
  FLK_REQUIRE(eps > 0.f || (a->torch_dialect && dyn_max_norm_dev), "flk_perturb_reg_pgd_batched: the l-infinity radius (%s) must be positive (got %g)",
              a->torch_dialect ? "dyn_max_norm" : "pgd_eps", (double)eps);
  FLK_LAUNCH_KERNEL(reg_adam_kernel<OPT_PGD>, dim3((unsigned)nclip), dim3(256), 0, (hipStream_t)stream, *a, g_adv, delta, (float*)nullptr, (float*)nullptr,
                     scalars, steps_dev, active_dev, dyn_max_norm_dev);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---- dense delta: L12 regulariser + Adam / projected sign-gradient step (kinetics_i3d_L12) -----------------------------
// d/d(delta_t) sqrt(mean_{hwc} delta_t^2) = delta_t / (N_f * sqrt(mean_t)),  N_f = H*W*3.
constexpr int DENSE_CHUNKS = 64;     // workgroups per frame in the reduction pass

__global__ __launch_bounds__(256) void dense_frame_stats(const float* delta, int frame_elems, float* part, float clampv) {
  // part[(t*DENSE_CHUNKS + c)*4 + {0,1,2,3}] = {sum clamp(d)^2, sum |d|, sum |d - d_prev_frame|, max |d|} over this chunk
  // (clampv > 0: the regulariser sees the clamped perturbation; the metrics are taken on the raw one, model.py:113-118)
  const int t = blockIdx.y, c = blockIdx.x, T = gridDim.y;
  const float4* d4 = (const float4*)(delta + (size_t)t * frame_elems);
  const float4* p4 = (const float4*)(delta + (size_t)((t + T - 1) % T) * frame_elems);
  const int n4 = frame_elems / 4;
  float sq = 0.f, ab = 0.f, ro = 0.f, mx = 0.f;
  for (int i = c * 256 + threadIdx.x; i < n4; i += DENSE_CHUNKS * 256) {
    const float4 a = d4[i], b = p4[i];
    {
      const float cx = fminf(fmaxf(a.x, -clampv), clampv), cy = fminf(fmaxf(a.y, -clampv), clampv);
      const float cz = fminf(fmaxf(a.z, -clampv), clampv), cw = fminf(fmaxf(a.w, -clampv), clampv);
      sq += cx * cx + cy * cy + cz * cz + cw * cw;
    }
    ab += fabsf(a.x) + fabsf(a.y) + fabsf(a.z) + fabsf(a.w);
    ro += fabsf(a.x - b.x) + fabsf(a.y - b.y) + fabsf(a.z - b.z) + fabsf(a.w - b.w);
    mx = fmaxf(mx, fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))));
  }
  __shared__ float sh[4];
  const float s0 = block_sum(sq, sh), s1 = block_sum(ab, sh), s2 = block_sum(ro, sh), s3 = block_max(mx, sh);
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)t * DENSE_CHUNKS + c) * 4;
    o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
  }
}

__global__ void dense_frame_finish(const float* part, int T, int frame_elems, float* frame_rms, float* scalars) {
  // one thread per frame sums its chunks in a fixed order; thread 0 then folds the frames (T <= 1024)
  __shared__ float s_l12[1024], s_ab[1024], s_ro[1024], s_mx[1024];
  const int t = threadIdx.x;
  float sq = 0.f, ab = 0.f, ro = 0.f, mx = 0.f;
  if (t < T)
    for (int c = 0; c < DENSE_CHUNKS; ++c) {
      const float* o = part + ((size_t)t * DENSE_CHUNKS + c) * 4;
      sq += o[0]; ab += o[1]; ro += o[2]; mx = fmaxf(mx, o[3]);
    }
  const float rms = sqrtf(sq / (float)frame_elems);
  if (t < T) frame_rms[t] = rms;
  s_l12[t] = t < T ? rms : 0.f; s_ab[t] = ab; s_ro[t] = ro; s_mx[t] = mx;
  __syncthreads();
  if (t == 0 && scalars) {
    float l12 = 0.f, a = 0.f, r = 0.f, m = 0.f;
    for (int i = 0; i < T; ++i) { l12 += s_l12[i]; a += s_ab[i]; r += s_ro[i]; m = fmaxf(m, s_mx[i]); }
    const float N = (float)T * (float)frame_elems;
    scalars[0] = l12 + 1e-12f; scalars[1] = a / N; scalars[2] = r / N; scalars[3] = m;
  }
}

// OPT_PGD: streams g_adv and delta in, delta out (16 bytes per lane over the contiguous frame, like the Adam form); m, v NULL
template <int OPT>
__global__ __launch_bounds__(256) void dense_adam_kernel(const flk_dense_adam_args a, int frame_elems, const float* frame_rms,
                                                         const float* g_adv, float* delta, float* m, float* v) {
  const int t = blockIdx.y;
  const float rms = frame_rms[t];
  // sqrt'(0) is unbounded in the reference too (tf.sqrt gradient at 0 -> inf); delta is initialised to 1e-8 for that reason
  const float rcoef = a.beta / ((float)frame_elems * rms);
  const float bc1 = 1.f - powf(a.adam_b1, (float)a.step), bc2s = sqrtf(1.f - powf(a.adam_b2, (float)a.step));
  const float lr_tf = a.lr * bc2s / bc1;
  const size_t base = (size_t)t * frame_elems;
  const int n4 = frame_elems / 4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
    const float4 d = ((const float4*)(delta + base))[i], g4 = ((const float4*)(g_adv + base))[i];
    float4 mm, vv;
    if constexpr (OPT == OPT_ADAM) { mm = ((const float4*)(m + base))[i]; vv = ((const float4*)(v + base))[i]; }
    else mm = vv = make_float4(0.f, 0.f, 0.f, 0.f);
    float dd[4] = {d.x, d.y, d.z, d.w};
    const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
    float mv[4] = {mm.x, mm.y, mm.z, mm.w}, vvv[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // d(L12)/d(delta) through the clamp: passes where |delta| <= dyn_max_norm (torch.clamp gradient, bounds inclusive)
      const float g = a.g_scale * gg[k] + ((a.dyn_max_norm > 0.f && fabsf(dd[k]) > a.dyn_max_norm) ? 0.f : rcoef * dd[k]);
      if constexpr (OPT == OPT_PGD) {
        dd[k] = pgd_step(dd[k], g, a.lr, a.torch_dialect ? a.dyn_max_norm : a.pgd_eps);
      } else {
        mv[k] = a.adam_b1 * mv[k] + (1.f - a.adam_b1) * g;
        vvv[k] = a.adam_b2 * vvv[k] + (1.f - a.adam_b2) * g * g;
        dd[k] = a.torch_dialect ? dd[k] - (a.lr / bc1) * mv[k] / (sqrtf(vvv[k]) / bc2s + a.adam_eps)
                                : dd[k] - lr_tf * mv[k] / (sqrtf(vvv[k]) + a.adam_eps);
      }
    }
    ((float4*)(delta + base))[i] = make_float4(dd[0], dd[1], dd[2], dd[3]);
    if constexpr (OPT == OPT_ADAM) {
      ((float4*)(m + base))[i] = make_float4(mv[0], mv[1], mv[2], mv[3]);
      ((float4*)(v + base))[i] = make_float4(vvv[0], vvv[1], vvv[2], vvv[3]);
    }
  }
}

extern "C" int64_t flk_dense_adam_scratch_bytes(int T, int H, int W) {
  (void)H; (void)W;
  return T > 0 ? (int64_t)(T * DENSE_CHUNKS * 4 + T) * sizeof(float) : 0;
}

extern "C" int flk_perturb_dense_l12_adam(const flk_dense_adam_args* a, const float* g_adv, float* delta, float* m, float* v,
                                          float* scalars, float* scratch, void* stream) {
  FLK_REQUIRE(a && g_adv && delta && m && v && scratch, "flk_perturb_dense_l12_adam: null argument");
  FLK_REQUIRE(a->T > 0 && a->T <= 1024 && a->H > 0 && a->W > 0 && (a->H * a->W * 3) % 4 == 0, "flk_perturb_dense_l12_adam: bad dims");
  FLK_REQUIRE(a->step >= 1, "flk_perturb_dense_l12_adam: step is 1-based");
  FLK_REQUIRE((((size_t)g_adv | (size_t)delta | (size_t)m | (size_t)v) & 15) == 0,
              "flk_perturb_dense_l12_adam: g_adv, delta, m and v must be 16-byte aligned (got %p, %p, %p, %p)", (const void*)g_adv, (void*)delta, (void*)m, (void*)v);
  const int fe = a->H * a->W * 3;
  float* part = scratch;
  float* frame_rms = scratch + (size_t)a->T * DENSE_CHUNKS * 4;
  hipStream_t s = (hipStream_t)stream;
  FLK_LAUNCH_KERNEL(dense_frame_stats, dim3(DENSE_CHUNKS, a->T), dim3(256), 0, s, delta, fe, part,
                     a->dyn_max_norm > 0.f ? a->dyn_max_norm : INFINITY);
  FLK_LAUNCH_KERNEL(dense_frame_finish, dim3(1), dim3(1024), 0, s, part, a->T, fe, frame_rms, scalars);
  FLK_LAUNCH_KERNEL(dense_adam_kernel<OPT_ADAM>, dim3(64, a->T), dim3(256), 0, s, *a, fe, frame_rms, g_adv, delta, m, v);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_perturb_dense_l12_pgd(const flk_dense_adam_args* a, const float* g_adv, float* delta, float* scalars, float* scratch,
                                         void* stream) {
  FLK_REQUIRE(a && g_adv && delta && scratch, "flk_perturb_dense_l12_pgd: null argument");
  FLK_REQUIRE(a->T > 0 && a->T <= 1024 && a->H > 0 && a->W > 0 && (a->H * a->W * 3) % 4 == 0, "flk_perturb_dense_l12_pgd: bad dims");
  const float eps = a->torch_dialect ? a->dyn_max_norm : a->pgd_eps;
  FLK_REQUIRE(eps > 0.f, "flk_perturb_dense_l12_pgd: the l-infinity radius (%s) must be positive (got %g)", a->torch_dialect ? "dyn_max_norm" : "pgd_eps", (double)eps);
  FLK_REQUIRE((((size_t)g_adv | (size_t)delta) & 15) == 0, "flk_perturb_dense_l12_pgd: g_adv and delta must be 16-byte aligned (got %p, %p)",
              (const void*)g_adv, (void*)delta);
  const int fe = a->H * a->W * 3;
  float* part = scratch;
  float* frame_rms = scratch + (size_t)a->T * DENSE_CHUNKS * 4;
  hipStream_t s = (hipStream_t)stream;
  FLK_LAUNCH_KERNEL(dense_frame_stats, dim3(DENSE_CHUNKS, a->T), dim3(256), 0, s, delta, fe, part,
                     a->dyn_max_norm > 0.f ? a->dyn_max_norm : INFINITY);
  FLK_LAUNCH_KERNEL(dense_frame_finish, dim3(1), dim3(1024), 0, s, part, a->T, fe, frame_rms, scalars);
  FLK_LAUNCH_KERNEL(dense_adam_kernel<OPT_PGD>, dim3(64, a->T), dim3(256), 0, s, *a, fe, frame_rms, g_adv, delta, (float*)nullptr, (float*)nullptr);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---- flicker on video time: per-frame rows of a period-P perturbation (include/flicker_hip.h) ------------------------------------
// rows[b*T + t] names the row of the shared delta [P,3] that frame t of clip b carries.  The gather hands the apply / export / gradient
// kernels a per-clip delta [B,T,3] (flk_apply_args.delta_per_clip); the row gradient folds their per-clip gradient back to [P,3].
constexpr int ROWS_MAX_P = (256 * ADAM_PER) / 3;      // 682: what reg_adam_kernel holds
constexpr int ROWS_PIECE = 2048;                      // entries of `rows` staged in LDS at a time (8 KiB)

// one thread = one value of delta_clip; raw values (the clamp and 1/std stay in pert_at); a row outside [0,P) is clamped into it
__global__ __launch_bounds__(256) void flicker_rows_gather_kernel(const float* delta, int P, const int32_t* rows, int n, float* delta_clip) {
  const long total = 3L * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int f = (int)(i / 3), c = (int)(i - 3L * f);
    int r = rows[f];
    r = r < 0 ? 0 : r > P - 1 ? P - 1 : r;
    delta_clip[i] = delta[r * 3 + c];
  }
}

// The fold skeleton of the three transposes below (one thread = one output (row r, channel c) of [P][3]): every entry of `rows` is
// handed to `entry(i, q)` -- i the frame's index, q its row -- in ascending i, so a sum the caller keeps has ONE fixed order whatever
// the grid.  The table is staged in LDS piece by piece by the whole workgroup (one HBM read of `rows` per workgroup, at most 8
// workgroups); all lanes of a wave read the same LDS entry (a broadcast).  EVERY thread of the workgroup calls this and meets every
// barrier; only a `live` one (its output exists) walks the entries.  `entry` sees bad rows too: it must pass over a q outside [0,P).
template <typename Entry>
__device__ static inline void fold_rows(const int32_t* rows, int n, bool live, Entry entry) {
  __shared__ int32_t sh[ROWS_PIECE];
  for (int base = 0; base < n; base += ROWS_PIECE) {
    const int m = n - base < ROWS_PIECE ? n - base : ROWS_PIECE;
    for (int j = threadIdx.x; j < m; j += 256) sh[j] = rows[base + j];
    __syncthreads();
    if (live)
      for (int j = 0; j < m; ++j) entry(base + j, sh[j]);
    __syncthreads();            // sh is refilled by the next piece
  }
}

// the row gradient: the frames that carry row r (inside [0,P), so a bad row matches none) are added in ascending order from +0.  g_clip
// is read only on a hit: 3*n loads over the launch.
__global__ __launch_bounds__(256) void flicker_rows_grad_kernel(const float* g_clip, const int32_t* rows, int n, int P, float* g_rows) {
  const int o = blockIdx.x * 256 + threadIdx.x, r = o / 3, c = o - 3 * r;
  float s = 0.f;
  fold_rows(rows, n, o < 3 * P, [&](int i, int q) {
    if (q == r) s += g_clip[(size_t)i * 3 + c];
  });
  if (o < 3 * P) g_rows[o] = s;
}

// The range checks every entry point of this seam makes, under its own name `who` (one without clips, lines or taps passes 1 for them)
static int check_seam(const char* who, int n, int clip_T, int H, int K, int kmax, int P) {
  FLK_REQUIRE(n >= 1, "%s: n must be >= 1 (got %d)", who, n);
  FLK_REQUIRE(clip_T >= 1 && n % clip_T == 0, "%s: clip_T must be >= 1 and divide n (got clip_T %d, n %d)", who, clip_T, n);
  FLK_REQUIRE(H >= 1, "%s: H (lines of a frame) must be >= 1 (got %d)", who, H);
  FLK_REQUIRE(K >= 1 && K <= kmax, "%s: K (taps of a clip or line) must be 1 .. %d (got %d)", who, kmax, K);
  FLK_REQUIRE(P >= 1 && P <= ROWS_MAX_P, "%s: period P must be 1 .. %d (got %d)", who, ROWS_MAX_P, P);
  return FLK_OK;
}

// the grid of a kernel that strides over `values` outputs: one thread each, at most 1024 workgroups of 256
static inline dim3 strided_grid(long values) {
  const long blocks = (values + 255) / 256;
  return dim3((unsigned)(blocks > 1024 ? 1024 : blocks));
}

// the grid of a fold: one thread per output of [P][3]
static inline dim3 fold_grid(int P) { return dim3((unsigned)((3 * P + 255) / 256)); }

extern "C" int flk_flicker_rows_gather(const float* delta, int P, const int32_t* rows, int n, float* delta_clip, void* stream) {
  FLK_REQUIRE(delta && rows && delta_clip, "flk_flicker_rows_gather: null argument");
  if (int e = check_seam("flk_flicker_rows_gather", n, 1, 1, 1, 1, P)) return e;
  FLK_LAUNCH_KERNEL(flicker_rows_gather_kernel, strided_grid(3L * n), dim3(256), 0, (hipStream_t)stream, delta, P, rows, n, delta_clip);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_flicker_rows_grad(const float* g_clip, const int32_t* rows, int n, int P, float* g_rows, void* stream) {
  FLK_REQUIRE(g_clip && rows && g_rows, "flk_flicker_rows_grad: null argument");
  if (int e = check_seam("flk_flicker_rows_grad", n, 1, 1, 1, 1, P)) return e;
  FLK_LAUNCH_KERNEL(flicker_rows_grad_kernel, fold_grid(P), dim3(256), 0, (hipStream_t)stream, g_clip, rows, n, P, g_rows);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---- capture channel: the flicker as a camera records it (include/flicker_hip.h) -------------------------------------------------------
// Frame i of clip b = i / clip_T records a mix of the K <= 4 consecutive rows rows[i], rows[i] + 1, ... (mod P) of delta, weighted by
// the clip's taps [K] and scaled per channel by its gain [3] (null: none).  A linear map at the per-clip seam of the two kernels above:
// the mix takes the place of the gather, its transpose the place of the row gradient.  Every product and every sum is rounded on its
// own (mul_rn / add_rn of perturb_common.h: nothing contracts to an fma), in one fixed order, so videoresnet_spec.flicker_rows_mix / _mix_grad
// restate both bit for bit; with K = 1, tap 1 and no gain (or gain 1) they are the two kernels above, bit for bit (1 * x = x).
constexpr int ROWS_MIX_MAX_K = 4;

// The tap loop: one value of the mix, channel c of a frame (or line) of clip b whose first row is `r` and whose taps are w[0..K).
// Raw values; a row outside [0,P) is clamped into it; the first product starts the sum (not 0 + product: a -0 stays -0); the gain comes
// last.  The rolling-shutter mix below calls it with each line's own taps.
__device__ static inline float mix_value(const float* delta, int P, int r, int c, const float* w, int K, const float* gain, int b) {
  r = r < 0 ? 0 : r > P - 1 ? P - 1 : r;
  float acc = mul_rn(w[0], delta[r * 3 + c]);
  for (int k = 1; k < K; ++k) {
    r = r + 1 == P ? 0 : r + 1;
    acc = add_rn(acc, mul_rn(w[k], delta[r * 3 + c]));
  }
  return gain ? mul_rn(gain[(size_t)b * 3 + c], acc) : acc;
}

// one thread = one value of delta_clip
__global__ __launch_bounds__(256) void flicker_rows_mix_kernel(const float* delta, int P, const int32_t* rows, int n, int clip_T, const float* taps,
                                                               int K, const float* gain, float* delta_clip) {
  const long total = 3L * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int f = (int)(i / 3), c = (int)(i - 3L * f), b = f / clip_T;
    delta_clip[i] = mix_value(delta, P, rows[f], c, taps + (size_t)b * K, K, gain, b);
  }
}

// The transpose, a fold_rows: frames in ascending i and within a frame taps in ascending k, from +0.  Frame i (row q) reaches row r
// through the taps k = (r - q) mod P, + P, + 2P, ... below K: more than one when P < K, and then all of them are added.  The clip index
// and the frame's place in its clip are carried along over every entry, hit or not (no division per frame: one on a hit alone costs a
// tenth of the kernel's time).  g_clip is read only on a hit.
__global__ __launch_bounds__(256) void flicker_rows_mix_grad_kernel(const float* g_clip, const int32_t* rows, int n, int clip_T, const float* taps,
                                                                    int K, const float* gain, int P, float* g_rows) {
  const int o = blockIdx.x * 256 + threadIdx.x, r = o / 3, c = o - 3 * r;
  float s = 0.f;
  int b = 0, t = 0;
  fold_rows(rows, n, o < 3 * P, [&](int i, int q) {
    if (q >= 0 && q < P) {
      int k = r - q;
      k = k < 0 ? k + P : k;
      if (k < K) {
        const float g = g_clip[(size_t)i * 3 + c];
        for (; k < K; k += P) {
          const float w = taps[(size_t)b * K + k];
          s = add_rn(s, mul_rn(gain ? mul_rn(gain[(size_t)b * 3 + c], w) : w, g));
        }
      }
    }
    if (++t == clip_T) { t = 0; ++b; }
  });
  if (o < 3 * P) g_rows[o] = s;
}

extern "C" int flk_flicker_rows_mix(const float* delta, int P, const int32_t* rows, int n, int clip_T, const float* taps, int K, const float* gain,
                                    float* delta_clip, void* stream) {
  FLK_REQUIRE(delta, "flk_flicker_rows_mix: delta is null");
  FLK_REQUIRE(rows, "flk_flicker_rows_mix: rows is null");
  FLK_REQUIRE(taps, "flk_flicker_rows_mix: taps is null");
  FLK_REQUIRE(delta_clip, "flk_flicker_rows_mix: delta_clip is null");
  if (int e = check_seam("flk_flicker_rows_mix", n, clip_T, 1, K, ROWS_MIX_MAX_K, P)) return e;
  FLK_LAUNCH_KERNEL(flicker_rows_mix_kernel, strided_grid(3L * n), dim3(256), 0, (hipStream_t)stream, delta, P, rows, n, clip_T, taps, K, gain,
                     delta_clip);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_flicker_rows_mix_grad(const float* g_clip, const int32_t* rows, int n, int clip_T, const float* taps, int K, const float* gain,
                                         int P, float* g_rows, void* stream) {
  FLK_REQUIRE(g_clip, "flk_flicker_rows_mix_grad: g_clip is null");
  FLK_REQUIRE(rows, "flk_flicker_rows_mix_grad: rows is null");
  FLK_REQUIRE(taps, "flk_flicker_rows_mix_grad: taps is null");
  FLK_REQUIRE(g_rows, "flk_flicker_rows_mix_grad: g_rows is null");
  if (int e = check_seam("flk_flicker_rows_mix_grad", n, clip_T, 1, K, ROWS_MIX_MAX_K, P)) return e;
  FLK_LAUNCH_KERNEL(flicker_rows_mix_grad_kernel, fold_grid(P), dim3(256), 0, (hipStream_t)stream, g_clip, rows, n, clip_T, taps, K, gain, P, g_rows);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---- rolling shutter: the capture channel per line of a frame (include/flicker_hip.h) ---------------------------------------------------
// Line h of a frame has its own taps [K <= 5] (it starts its exposure later than line 0): the mix writes the per-line perturbation
// [n][H][3] that flk_apply_args.delta_per_line takes; its transpose folds the per-line gradient back to [P][3].  The arithmetic and its
// order are the rows pair's above (mul_rn / add_rn: nothing contracts), so videoresnet_spec.flicker_lines_mix / _mix_grad restate both.
constexpr int LINES_MIX_MAX_K = 5;

// one thread = one output value (frame i, line h, channel c)
__global__ __launch_bounds__(256) void flicker_lines_mix_kernel(const float* delta, int P, const int32_t* rows, int n, int clip_T, int H,
                                                                const float* taps, int K, const float* gain, float* out) {
  const long total = 3L * n * H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long fh = i / 3;
    const int c = (int)(i - 3 * fh), f = (int)(fh / H), h = (int)(fh - (long)f * H), b = f / clip_T;
    out[i] = mix_value(delta, P, rows[f], c, taps + ((size_t)b * H + h) * K, K, gain, b);
  }
}

// transpose, stage 1: one thread = one (frame i, tap k, channel c); the lines of the frame in ascending order, from +0
__global__ __launch_bounds__(256) void flicker_lines_mix_grad_stage1(const float* g_lines, int n, int clip_T, int H, const float* taps, int K,
                                                                     const float* gain, float* sbuf) {
  const long total = 3L * n * K;
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
    const long ik = o / 3;
    const int c = (int)(o - 3 * ik), i = (int)(ik / K), k = (int)(ik - (long)i * K), b = i / clip_T;
    const float* w = taps + (size_t)b * H * K + k;
    const float* g = g_lines + (size_t)i * H * 3 + c;
    const float gn = gain ? gain[(size_t)b * 3 + c] : 1.f;
    float s = 0.f;
    for (int h = 0; h < H; ++h) {
      const float wk = w[(size_t)h * K];
      s = add_rn(s, mul_rn(gain ? mul_rn(gn, wk) : wk, g[(size_t)h * 3]));
    }
    sbuf[o] = s;
  }
}

// transpose, stage 2: flicker_rows_mix_grad_kernel's fold over s[n][K][3] (the coefficients are inside s already): frames ascending,
// taps ascending, from +0
__global__ __launch_bounds__(256) void flicker_lines_mix_grad_stage2(const float* sbuf, const int32_t* rows, int n, int K, int P, float* g_rows) {
  const int o = blockIdx.x * 256 + threadIdx.x, r = o / 3, c = o - 3 * r;
  float s = 0.f;
  fold_rows(rows, n, o < 3 * P, [&](int i, int q) {
    if (q >= 0 && q < P) {
      int k = r - q;
      k = k < 0 ? k + P : k;
      for (; k < K; k += P) s = add_rn(s, sbuf[((size_t)i * K + k) * 3 + c]);
    }
  });
  if (o < 3 * P) g_rows[o] = s;
}

extern "C" int flk_flicker_lines_mix(const float* delta, int P, const int32_t* rows, int n, int clip_T, int H, const float* taps, int K,
                                     const float* gain, float* out, void* stream) {
  FLK_REQUIRE(delta, "flk_flicker_lines_mix: delta is null");
  FLK_REQUIRE(rows, "flk_flicker_lines_mix: rows is null");
  FLK_REQUIRE(taps, "flk_flicker_lines_mix: taps is null");
  FLK_REQUIRE(out, "flk_flicker_lines_mix: out is null");
  if (int e = check_seam("flk_flicker_lines_mix", n, clip_T, H, K, LINES_MIX_MAX_K, P)) return e;
  FLK_LAUNCH_KERNEL(flicker_lines_mix_kernel, strided_grid(3L * n * H), dim3(256), 0, (hipStream_t)stream, delta, P, rows, n, clip_T, H, taps, K, gain,
                     out);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_flicker_lines_mix_grad(const float* g_lines, const int32_t* rows, int n, int clip_T, int H, const float* taps, int K,
                                          const float* gain, int P, float* scratch, float* g_rows, void* stream) {
  FLK_REQUIRE(g_lines, "flk_flicker_lines_mix_grad: g_lines is null");
  FLK_REQUIRE(rows, "flk_flicker_lines_mix_grad: rows is null");
  FLK_REQUIRE(taps, "flk_flicker_lines_mix_grad: taps is null");
  FLK_REQUIRE(scratch, "flk_flicker_lines_mix_grad: scratch is null");
  FLK_REQUIRE(g_rows, "flk_flicker_lines_mix_grad: g_rows is null");
  if (int e = check_seam("flk_flicker_lines_mix_grad", n, clip_T, H, K, LINES_MIX_MAX_K, P)) return e;
  FLK_LAUNCH_KERNEL(flicker_lines_mix_grad_stage1, strided_grid(3L * n * K), dim3(256), 0, (hipStream_t)stream, g_lines, n, clip_T, H, taps, K, gain,
                     scratch);
  FLK_LAUNCH_KERNEL(flicker_lines_mix_grad_stage2, fold_grid(P), dim3(256), 0, (hipStream_t)stream, scratch, rows, n, K, P, g_rows);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---- slope tables of a toned preparation, additive model (flk_flicker_tone_slopes; csrc/prepare.hip resamples them) ----------------
// slope[b][t][v][c] = 1 where the clamp of grad_reduce_stage1 is inactive for source byte v: lo <= u <= hi, u = x_lut[v][c] +
// adv_flag * pert_at(...) -- the same expression; scale[b][t][c] = grad_reduce_stage2's finishing factors adv_flag * inv_std[c], 0 where
// the delta value lies outside its clamp.  One workgroup per (clip, frame), thread v.
__global__ __launch_bounds__(256) void tone_slopes_kernel(const flk_apply_args a, float* slope, float* scale) {
  const int bt = blockIdx.x, b = bt / a.T, t = bt - b * a.T, v = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 3; ++c) slope[((size_t)bt * 256 + v) * 3 + c] = passes(a, a.x_lut[v * 3 + c], pert_at(a, b, t, 0, 0, c)) ? 1.f : 0.f;
  if (v < 3) {
    const float dc = a.dclip_dev ? a.dclip_dev[b] : a.dclip;
    scale[(size_t)bt * 3 + v] = delta_unclamped(a.delta[(size_t)bt * 3 + v], dc) ? a.adv_flag * a.inv_std[v] : 0.f;
  }
}

// arguments already validated (api.cpp: flk_flicker_tone_slopes)
int flk_tone_slopes_launch(const flk_apply_args* a, float* slope, float* scale, hipStream_t stream) {
  FLK_REQUIRE(a->lo <= a->hi, "flk_flicker_tone_slopes: lo > hi");
  FLK_LAUNCH_KERNEL(tone_slopes_kernel, dim3((unsigned)(a->B * a->T)), dim3(256), 0, stream, *a, slope, scale);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
