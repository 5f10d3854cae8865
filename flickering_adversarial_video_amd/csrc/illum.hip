// The flicker as scene illumination (include/flicker_hip.h: flk_illum_*): a lamp multiplies the LINEAR light of a pixel, the camera
// applies its response curve and stores 8 bits.  Per source byte: one lookup of the decode table (linear light), one rounded product
// with the frame's (or line's) factor s = 1 + adv_flag * m, a clamp to [0,1], and one interpolated lookup of the encode table.  Both
// tables live in LDS (dec 3 KB, enc 4 (N + 1) bytes: 16 KB at N = 4096, beside the 3 KB of q_lut), staged once per workgroup, so every
// kernel here runs a CAPPED grid whose workgroups stride over the work: the staging is paid a few times per CU, not once per 256
// positions.  The per-value arithmetic is spelt with mul_rn / add_rn (nothing contracts to an fma): videoresnet_spec.illum_apply_host,
// illum_export_host and illum_grad_host restate it on the host.  The layouts and the two-stage gradient follow csrc/attack.hip; the byte
// loads, the export's unit scheme and statistics fold, the wave sum and the gradient's tail are the helpers of perturb_common.h.
#include "flk_internal.h"
#include "perturb_common.h"

namespace {

constexpr int ILLUM_MAX_N = 16384;
constexpr int ILLUM_GRID_CAP = 1024;           // workgroups per launch: 4 per CU; the tables are staged once per workgroup

// the tables in LDS
struct Curve {
  const float* dec;      // [256][3]
  const float* enc;      // [N + 1]
  int N;
  float Nf;
};

// every thread of the workgroup calls this once, before any early return; dst = dec | (ql) | enc
__device__ inline void stage_tables(const flk_illum_args& m, const float* q_lut, float* dec, float* ql, float* enc) {
  for (int i = threadIdx.x; i < 768; i += 256) dec[i] = m.dec[i];
  if (q_lut)
    for (int i = threadIdx.x; i < 768; i += 256) ql[i] = q_lut[i];
  for (int i = threadIdx.x; i <= m.enc_n; i += 256) enc[i] = m.enc[i];
  __syncthreads();
}

// s = 1 + adv_flag * m, m the clamped delta value of (b, (t - shift_p) mod dT, [h], c); dT: the perturbation's own period
__device__ inline float illum_s(const flk_apply_args& a, int dT, int b, int t, int h, int c) {
  const int ts = wrap(t - a.shift_p, dT);
  const size_t row = (size_t)(a.delta_per_clip ? b : 0) * dT + ts;
  float d = a.delta_per_line ? a.delta[(row * a.H + h) * 3 + c] : a.delta[row * 3 + c];
  const float dc = a.dclip_dev ? a.dclip_dev[b] : a.dclip;
  if (dc > 0.f) d = clipf(d, -dc, dc);
  return add_rn(1.f, mul_rn(a.adv_flag, d));
}

// display value e in [0,1] of byte `by`, channel c, under the factor s; *outside: p left [0,1] (NaN counts as inside: it encodes as 0)
__device__ inline float illum_display(const Curve& cv, uint32_t by, int c, float s, bool* outside = nullptr) {
  const float p = mul_rn(cv.dec[by * 3 + c], s);
  if (outside) *outside = p < 0.f || p > 1.f;
  const float u = fminf(fmaxf(p, 0.f), 1.f);
  const float z = mul_rn(u, cv.Nf);
  int i = (int)z;
  if (i > cv.N - 1) i = cv.N - 1;
  const float f = add_rn(z, -(float)i);
  const float e0 = cv.enc[i], d = add_rn(cv.enc[i + 1], -e0);
  return add_rn(e0, mul_rn(f, d));
}
// the byte a frame stores: q = min(rint(e * 255), 255), NaN -> 0
__device__ inline int illum_byte(float e) {
  const float z = mul_rn(e, 255.f);
  return z >= 0.f ? (int)fminf(rintf(z), 255.f) : 0;
}
// value the network sees
template <bool QUANT> __device__ inline float illum_value(const Curve& cv, const flk_illum_args& m, const float* ql, uint32_t by, int c, float s) {
  const float e = illum_display(cv, by, c, s);
  if constexpr (QUANT) return ql[illum_byte(e) * 3 + c];
  else return add_rn(mul_rn(e, m.out_mul[c]), m.out_add[c]);
}
// d(e)/d(s) = (d * N) * L where 0 <= p <= 1 (false: the clamp is active, no contribution)
__device__ inline bool illum_weight(const Curve& cv, uint32_t by, int c, float s, float* w) {
  const float L = cv.dec[by * 3 + c];
  const float p = mul_rn(L, s);
  if (!(p >= 0.f && p <= 1.f)) return false;
  const float z = mul_rn(p, cv.Nf);
  int i = (int)z;
  if (i > cv.N - 1) i = cv.N - 1;
  const float d = add_rn(cv.enc[i + 1], -cv.enc[i]);
  *w = mul_rn(mul_rn(d, cv.Nf), L);
  return true;
}

// ---- apply: one thread = NP consecutive positions of the (h,w) fold, [B,T,H/2,W/2,16] (channel (qh*2+qw)*3+c) or, HILO (fold_t 4),
// [B,T,H/2,W/2,32] with every value as two bf16 numbers -- the layouts S2D<1> / HiLo of apply_s2d_kernel (attack.hip) ----------
template <typename TO, bool HILO, bool QUANT, int NP>
__global__ __launch_bounds__(256) void illum_apply_kernel(const flk_apply_args a, const flk_illum_args m, char* out) {
  extern __shared__ float smem[];
  float* dec = smem;
  float* ql = smem + 768;
  float* enc = smem + (QUANT ? 1536 : 768);
  stage_tables(m, QUANT ? a.q_lut : nullptr, dec, ql, enc);
  const Curve cv{dec, enc, m.enc_n, (float)m.enc_n};
  constexpr int NCH = HILO ? 32 : 16;
  const int H2 = a.H / 2, W2 = a.W / 2, WG = W2 / NP;
  const long total = (long)a.B * a.T * H2 * WG;
  for (long gid = (long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
    long r = gid;
    const int wg = (int)(r % WG); r /= WG;
    const int h2 = (int)(r % H2); r /= H2;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    const int tx = wrap(t - a.shift_x, a.T);        // x'[t] = x[(t - shift_x) mod T]
    float s[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[0][c] = illum_s(a, a.T, b, t, 2 * h2, c);
      s[1][c] = a.delta_per_line ? illum_s(a, a.T, b, t, 2 * h2 + 1, c) : s[0][c];
    }
    uint32_t by[2][6 * NP];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
      load_bytes<NP>((const uint8_t*)a.x + ((((size_t)b * a.T + tx) * a.H + 2 * h2 + qh) * a.W + (size_t)2 * NP * wg) * 3, by[qh]);
    char* dst = out + ((((size_t)b * a.T + t) * H2 + h2) * W2 + (size_t)NP * wg) * NCH * sizeof(TO);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      float v[NCH];
#pragma unroll
      for (int k = 0; k < NCH; ++k) v[k] = 0.f;
#pragma unroll
      for (int qh = 0; qh < 2; ++qh)
#pragma unroll
        for (int e = 0; e < 6; ++e) {               // pixel 2 * (NP * wg + j) + e / 3, channel e % 3
          const float x = illum_value<QUANT>(cv, m, ql, by[qh][6 * j + e], e % 3, s[qh][e % 3]);
          if constexpr (HILO) {
            const float hi = (float)(bf16_t)x;
            v[qh * 6 + e] = hi;
            v[16 + qh * 6 + e] = x - hi;
          } else {
            v[qh * 6 + e] = x;
          }
        }
      store_ch<TO, NCH>(dst + (size_t)j * NCH * sizeof(TO), v);
    }
  }
}

// ---- export: work item = (clip, frame, chunk of 256 units of the DESTINATION frame), one thread = one unit (ExportUnit,
// perturb_common.h: adv_export_u8_kernel's scheme); workgroups stride over the items ------------------------------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void illum_export_kernel(const flk_apply_args a, const flk_illum_args m, const flk_export_args e, uint8_t* out,
                                                           int32_t* stats, int chunks, long nitems) {
  extern __shared__ float smem[];
  float* dec = smem;
  float* enc = smem + 768;
  int* red = (int*)(enc + m.enc_n + 1);            // [4][12]
  stage_tables(m, nullptr, dec, nullptr, enc);
  const Curve cv{dec, enc, m.enc_n, (float)m.enc_n};
  const int F = a.H * a.W * 3;
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
      const int tx = wrap(t - a.shift_x, a.T);
      const uint8_t* src = (const uint8_t*)a.x + ((size_t)b * a.T + tx) * F + start;
      float sf[3] = {1.f, 1.f, 1.f};
      if (!a.delta_per_line) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sf[k] = illum_s(a, e.delta_T, b, t, 0, k);
      }
      uint32_t by[4] = {0, 0, 0, 0};
      export_load_u8(src, cnt, by);
      uint32_t packed = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          const int c = un.c;
          const float s = a.delta_per_line ? illum_s(a, e.delta_T, b, t, un.h, c) : (c == 0 ? sf[0] : c == 1 ? sf[1] : sf[2]);
          bool outside;
          const int q = illum_byte(illum_display(cv, by[j], c, s, &outside));
          if (cnt == 4) packed |= (uint32_t)q << (8 * j);
          else dst[start + j] = (uint8_t)q;
          if constexpr (STATS) {
            const int d = q - (int)by[j];
#pragma unroll
            for (int k = 0; k < 3; ++k)
              if (c == k) { acc[k][0] += d; acc[k][1] += d < 0 ? -d : d; acc[k][2] += d != 0; acc[k][3] += outside ? 1 : 0; }
          }
          un.next(a.W);
        }
      }
      if (cnt == 4) *(uint32_t*)(dst + start) = packed;
    }
    if constexpr (STATS) export_stats_fold(acc, red, stats + ((size_t)b * a.T + t) * 12);
  }
}

// ---- gradient ------------------------------------------------------------------------------------------------------------------------
// chunks of row pairs per (clip, frame): a function of the shapes only (per-clip perturbations: of ONE clip's, the batch-1 call's)
inline int illum_nchunk(int B, int T, int H) {
  int n = (1024 + B * T - 1) / (B * T);
  if (n > H / 2) n = H / 2;
  return n < 1 ? 1 : n;
}

// stage 1: item (b, t, chunk of row pairs) -> partials[item][c] = the sum of its terms: thread i adds the cells i, i + 256, ... of the
// chunk in ascending order (per cell row 2 h2 then 2 h2 + 1, pixels and channels as stored), the 64 lanes fold by the shuffle tree
// 32, .., 1 and the four waves are added in wave order.  Workgroups stride over the items: the order inside an item does not depend
// on the grid.
template <typename TI>
__global__ __launch_bounds__(256) void illum_grad_stage1(const flk_apply_args a, const flk_illum_args m, const char* gx, int nchunk, long nitems,
                                                         float* partials) {
  extern __shared__ float smem[];
  float* dec = smem;
  float* enc = smem + 768;
  float* red = enc + m.enc_n + 1;                   // [4][3]
  stage_tables(m, nullptr, dec, nullptr, enc);
  const Curve cv{dec, enc, m.enc_n, (float)m.enc_n};
  const int H2 = a.H / 2, W2 = a.W / 2;
  for (long item = blockIdx.x; item < nitems; item += gridDim.x) {
    long r = item;
    const int chunk = (int)(r % nchunk); r /= nchunk;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    const int tx = wrap(t - a.shift_x, a.T);
    const int h_lo = (int)((long)H2 * chunk / nchunk), h_hi = (int)((long)H2 * (chunk + 1) / nchunk);
    float s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = illum_s(a, a.T, b, t, 0, c);
    float acc[3] = {0.f, 0.f, 0.f};
    const int ncell = (h_hi - h_lo) * W2;
    for (int i = threadIdx.x; i < ncell; i += 256) {
      const int h2 = h_lo + i / W2, w2 = i % W2;
      float g[12];
      load_ch<TI, 12>(gx + ((((size_t)b * a.T + t) * H2 + h2) * W2 + w2) * 16 * sizeof(TI), g);
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        uint32_t by[6];
        load_bytes<1>((const uint8_t*)a.x + ((((size_t)b * a.T + tx) * a.H + 2 * h2 + qh) * a.W + 2 * w2) * 3, by);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          float w;
          if (illum_weight(cv, by[k], k % 3, s[k % 3], &w)) acc[k % 3] = add_rn(acc[k % 3], mul_rn(g[qh * 6 + k], w));
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = wave_sum(acc[c]);
      if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 3 + c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) partials[(size_t)item * 3 + threadIdx.x] = red[threadIdx.x] + red[3 + threadIdx.x] + red[6 + threadIdx.x] + red[9 + threadIdx.x];
    __syncthreads();              // red is reused by the next item
  }
}

// the finishing stage: thread (t, c) adds the partials over (b, chunk) in that order (per clip: blockIdx.y = the clip, its chunks only),
// maps frame t back to the delta row it was rolled from, applies adv_flag * out_mul[c] and the delta-clamp mask
__global__ void illum_grad_stage2(const flk_apply_args a, const flk_illum_args m, int nchunk, const float* partials, float* gdelta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.T * 3) return;
  const int t = i / 3, c = i % 3;
  const int b_lo = a.delta_per_clip ? (int)blockIdx.y : 0, b_hi = a.delta_per_clip ? b_lo + 1 : a.B;
  float s = 0.f;
  for (int b = b_lo; b < b_hi; ++b)
    for (int k = 0; k < nchunk; ++k) s += partials[(((size_t)b * a.T + t) * nchunk + k) * 3 + c];
  const int ts = wrap(t - a.shift_p, a.T);
  const size_t di = (a.delta_per_clip ? (size_t)b_lo * a.T * 3 : 0) + (size_t)ts * 3 + c;
  const float dc = a.dclip_dev ? a.dclip_dev[b_lo] : a.dclip;
  gdelta[di] = delta_grad_out(a.delta[di], dc, s, a.adv_flag, m.out_mul[c]);
}

// per line (delta_per_line with delta_per_clip): one wave owns one (clip, frame, row pair) and produces its 2 lines x 3 channels: lane l
// walks the positions l, l + 64, ... in ascending order, then the shuffle tree; the finishing factors per line.  Waves stride over the
// work: no scratch, one fixed order.
template <typename TI>
__global__ __launch_bounds__(256) void illum_grad_lines_kernel(const flk_apply_args a, const flk_illum_args m, const char* gx, float* gdelta) {
  extern __shared__ float smem[];
  float* dec = smem;
  float* enc = smem + 768;
  stage_tables(m, nullptr, dec, nullptr, enc);
  const Curve cv{dec, enc, m.enc_n, (float)m.enc_n};
  const int H2 = a.H / 2, W2 = a.W / 2;
  const long nwork = (long)a.B * a.T * H2;
  const int lane = threadIdx.x & 63;
  for (long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6); item < nwork; item += (long)gridDim.x * 4) {      // uniform over the wave
    long r = item;
    const int h2 = (int)(r % H2); r /= H2;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    const int tx = wrap(t - a.shift_x, a.T);
    float s[2][3];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
#pragma unroll
      for (int c = 0; c < 3; ++c) s[qh][c] = illum_s(a, a.T, b, t, 2 * h2 + qh, c);
    float acc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    for (int w2 = lane; w2 < W2; w2 += 64) {
      float g[12];
      load_ch<TI, 12>(gx + ((((size_t)b * a.T + t) * H2 + h2) * W2 + w2) * 16 * sizeof(TI), g);
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        uint32_t by[6];
        load_bytes<1>((const uint8_t*)a.x + ((((size_t)b * a.T + tx) * a.H + 2 * h2 + qh) * a.W + 2 * w2) * 3, by);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          float w;
          if (illum_weight(cv, by[k], k % 3, s[qh][k % 3], &w)) acc[qh][k % 3] = add_rn(acc[qh][k % 3], mul_rn(g[qh * 6 + k], w));
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
          gdelta[di] = delta_grad_out(a.delta[di], dc, v, a.adv_flag, m.out_mul[c]);
        }
      }
  }
}

// ---- slope tables of a toned preparation (flk_flicker_tone_slopes; csrc/prepare.hip resamples them): slope[b][t][v][c] = the weight
// illum_weight gives source byte v under the frame's factor, 0 where p leaves [0,1]; scale[b][t][c] = illum_grad_stage2's finishing
// factors adv_flag * out_mul[c], 0 where the delta value lies outside its clamp.  Item = (clip, frame), thread v; workgroups stride
__global__ __launch_bounds__(256) void illum_tone_slopes_kernel(const flk_apply_args a, const flk_illum_args m, float* slope, float* scale) {
  extern __shared__ float smem[];
  float* dec = smem;
  float* enc = smem + 768;
  stage_tables(m, nullptr, dec, nullptr, enc);
  const Curve cv{dec, enc, m.enc_n, (float)m.enc_n};
  const int v = threadIdx.x;
  for (int bt = blockIdx.x; bt < a.B * a.T; bt += gridDim.x) {
    const int b = bt / a.T, t = bt - b * a.T;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float w;
      slope[((size_t)bt * 256 + v) * 3 + c] = illum_weight(cv, (uint32_t)v, c, illum_s(a, a.T, b, t, 0, c), &w) ? w : 0.f;
    }
    if (v < 3) {
      const float dc = a.dclip_dev ? a.dclip_dev[b] : a.dclip;
      scale[(size_t)bt * 3 + v] = delta_unclamped(a.delta[(size_t)bt * 3 + v], dc) ? mul_rn(a.adv_flag, m.out_mul[v]) : 0.f;
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// what the three entry points share (who: the entry point's name)
int check_illum(const char* who, const flk_apply_args* a, const flk_illum_args* m) {
  FLK_REQUIRE(a && m, "%s: null argument structure", who);
  FLK_REQUIRE(a->x && a->delta, "%s: null x (clip) or delta", who);
  FLK_REQUIRE(a->x_is_u8 && a->x_lut, "%s: the illumination model takes uint8 clips with their decode table (x_is_u8 = 1, x_lut non-null)", who);
  FLK_REQUIRE(a->center == 0, "%s: center must be 0", who);
  FLK_REQUIRE(!a->delta_dense, "%s: delta_dense is not supported (the flicker [T,3], [B,T,3] or per line [Bd,T,H,3] only)", who);
  FLK_REQUIRE(m->dec && m->enc, "%s: null dec / enc table", who);
  FLK_REQUIRE(m->enc_n >= 2 && m->enc_n <= ILLUM_MAX_N, "%s: enc_n must be 2 .. %d (got %d)", who, ILLUM_MAX_N, m->enc_n);
  FLK_REQUIRE(a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0, "%s: sizes must be positive (got %d,%d,%d,%d)", who, a->B, a->T, a->H, a->W);
  FLK_REQUIRE(!a->dclip_dev || a->delta_per_clip, "%s: dclip_dev (per-clip clamp bounds) needs delta_per_clip", who);
  return FLK_OK;
}
// the folded layouts (apply and gradient)
int check_fold(const char* who, const flk_apply_args* a) {
  FLK_REQUIRE(a->fold_t == 1 || a->fold_t == 4, "%s: fold_t must be 1 or 4 (the VideoResNet layouts), got %d", who, a->fold_t);
  FLK_REQUIRE(a->H % 2 == 0 && a->W % 2 == 0, "%s: H and W must be even (got %d,%d)", who, a->H, a->W);
  FLK_REQUIRE(((size_t)a->x & 1) == 0, "%s: a uint8 clip must be 2-byte aligned (got x = %p)", who, a->x);
  return FLK_OK;
}
inline unsigned capped(long n) { return (unsigned)(n < 1 ? 1 : n > ILLUM_GRID_CAP ? ILLUM_GRID_CAP : n); }

// dynamic LDS above 64 KiB (enc_n near its maximum) needs the kernel's limit raised, once per device
template <auto KERNEL> int raise_lds(int bytes) {
  static bool done[FLK_MAX_DEVICES];
  if (bytes <= 65536) return FLK_OK;
  return flk_raise_lds_limit((const void*)KERNEL, bytes, done);
}

template <typename TO, bool HILO, bool QUANT, int NP>
int launch_apply(const flk_apply_args* a, const flk_illum_args* m, void* out, hipStream_t st) {
  const long total = (long)a->B * a->T * (a->H / 2) * (a->W / 2 / NP);
  const int lds = (768 * (QUANT ? 2 : 1) + m->enc_n + 1) * (int)sizeof(float);
  const int rc = raise_lds<illum_apply_kernel<TO, HILO, QUANT, NP>>(lds);
  if (rc) return rc;
  FLK_LAUNCH_KERNEL((illum_apply_kernel<TO, HILO, QUANT, NP>), dim3(capped((total + 255) / 256)), dim3(256), lds, st, *a, *m, (char*)out);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
template <typename TO, bool HILO>
int dispatch_apply(const flk_apply_args* a, const flk_illum_args* m, void* out, hipStream_t st) {
  const bool fast = a->W % 8 == 0 && ((size_t)a->x & 7) == 0;       // three 8-byte loads per row of four positions
  if (a->q_lut) return fast ? launch_apply<TO, HILO, true, 4>(a, m, out, st) : launch_apply<TO, HILO, true, 1>(a, m, out, st);
  return fast ? launch_apply<TO, HILO, false, 4>(a, m, out, st) : launch_apply<TO, HILO, false, 1>(a, m, out, st);
}

}  // namespace

extern "C" int flk_illum_apply_s2d(const flk_apply_args* a, const flk_illum_args* m, void* out, int dtype, void* stream) {
  static const char* who = "flk_illum_apply_s2d";
  int rc = check_illum(who, a, m);
  if (rc) return rc;
  if ((rc = check_fold(who, a))) return rc;
  FLK_REQUIRE(out, "%s: null out", who);
  FLK_REQUIRE(((size_t)out & 15) == 0, "%s: out must be 16-byte aligned (got %p)", who, out);
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "%s: bad dtype", who);
  FLK_REQUIRE(a->fold_t != 4 || dtype == FLK_BF16, "%s: fold_t = 4 (two bf16 numbers per value) writes bf16", who);
  if (a->adv_flag == 0.f) return flk_perturb_apply_s2d(a, out, dtype, stream);      // the clean clip: the existing kernels, bit for bit
  hipStream_t st = (hipStream_t)stream;
  if (a->fold_t == 4) return dispatch_apply<bf16_t, true>(a, m, out, st);
  if (dtype == FLK_BF16) return dispatch_apply<bf16_t, false>(a, m, out, st);
  return dispatch_apply<float, false>(a, m, out, st);
}

extern "C" int flk_illum_export_u8(const flk_apply_args* a, const flk_illum_args* m, const flk_export_args* e, uint8_t* out, int32_t* stats,
                                   void* stream) {
  static const char* who = "flk_illum_export_u8";
  int rc = check_illum(who, a, m);
  if (rc) return rc;
  FLK_REQUIRE(e, "%s: null export arguments", who);
  FLK_REQUIRE(out, "%s: null out", who);
  FLK_REQUIRE((int64_t)a->H * a->W * 3 <= 0x7fffffff, "%s: a frame of %d x %d is too large", who, a->H, a->W);
  FLK_REQUIRE(e->out_clip_offset >= 0, "%s: negative out_clip_offset", who);
  FLK_REQUIRE(e->out_clip_stride >= (int64_t)a->T * a->H * a->W * 3, "%s: out_clip_stride %lld smaller than the clip", who, (long long)e->out_clip_stride);
  FLK_REQUIRE(e->delta_T >= 0, "%s: negative delta_T", who);
  FLK_REQUIRE(e->delta_T == 0 || !a->delta_per_clip, "%s: delta_T (a period) is defined for the shared perturbation [delta_T,3] (delta_per_line: [delta_T,H,3]) only", who);
  FLK_REQUIRE(!stats || (int64_t)a->H * a->W <= 8388607, "%s: stats need H * W <= 8388607 (255 * H * W must fit an int32), got %d x %d", who, a->H, a->W);
  hipStream_t st = (hipStream_t)stream;
  flk_export_args ee = *e;
  if (ee.delta_T == 0) ee.delta_T = a->T;
  const int F = a->H * a->W * 3;
  const int chunks = (F / 4 + 2 + 255) / 256;       // units of a frame: at most F / 4 words, a head and a tail
  const long nitems = (long)a->B * a->T * chunks;
  const int lds = (768 + m->enc_n + 1 + 48) * (int)sizeof(float);
  if (stats) {
    if ((rc = raise_lds<illum_export_kernel<true>>(lds))) return rc;
    FLK_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)a->B * a->T * 12 * sizeof(int32_t), st));
    FLK_LAUNCH_KERNEL(illum_export_kernel<true>, dim3(capped(nitems)), dim3(256), lds, st, *a, *m, ee, out, stats, chunks, nitems);
  } else {
    if ((rc = raise_lds<illum_export_kernel<false>>(lds))) return rc;
    FLK_LAUNCH_KERNEL(illum_export_kernel<false>, dim3(capped(nitems)), dim3(256), lds, st, *a, *m, ee, out, stats, chunks, nitems);
  }
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

extern "C" int flk_illum_grad_reduce(const flk_apply_args* a, const flk_illum_args* m, const void* gx_s2d, int dtype, float* gdelta, float* partials,
                                     void* stream) {
  static const char* who = "flk_illum_grad_reduce";
  int rc = check_illum(who, a, m);
  if (rc) return rc;
  if ((rc = check_fold(who, a))) return rc;
  FLK_REQUIRE(gx_s2d && gdelta, "%s: null gx_s2d or gdelta", who);
  FLK_REQUIRE(((size_t)gx_s2d & 15) == 0, "%s: gx_s2d must be 16-byte aligned (got %p)", who, gx_s2d);
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "%s: bad dtype", who);
  hipStream_t st = (hipStream_t)stream;
  const bool bf = dtype == FLK_BF16;
  const int lds = (768 + m->enc_n + 1 + 12) * (int)sizeof(float);
  if (a->delta_per_line) {
    FLK_REQUIRE(a->delta_per_clip, "%s: delta_per_line needs delta_per_clip (the gradient comes back per clip, [B,T,H,3])", who);
    const long waves = (long)a->B * a->T * (a->H / 2);
    if (bf) {
      if ((rc = raise_lds<illum_grad_lines_kernel<bf16_t>>(lds))) return rc;
      FLK_LAUNCH_KERNEL(illum_grad_lines_kernel<bf16_t>, dim3(capped((waves + 3) / 4)), dim3(256), lds, st, *a, *m, (const char*)gx_s2d, gdelta);
    } else {
      if ((rc = raise_lds<illum_grad_lines_kernel<float>>(lds))) return rc;
      FLK_LAUNCH_KERNEL(illum_grad_lines_kernel<float>, dim3(capped((waves + 3) / 4)), dim3(256), lds, st, *a, *m, (const char*)gx_s2d, gdelta);
    }
  } else {
    FLK_REQUIRE(partials, "%s: null partials (scratch)", who);
    // per-clip perturbations: the chunking (= summation order) of a batch-1 call
    const int nchunk = illum_nchunk(a->delta_per_clip ? 1 : a->B, a->T, a->H);
    const long nitems = (long)a->B * a->T * nchunk;
    if (bf) {
      if ((rc = raise_lds<illum_grad_stage1<bf16_t>>(lds))) return rc;
      FLK_LAUNCH_KERNEL(illum_grad_stage1<bf16_t>, dim3(capped(nitems)), dim3(256), lds, st, *a, *m, (const char*)gx_s2d, nchunk, nitems, partials);
    } else {
      if ((rc = raise_lds<illum_grad_stage1<float>>(lds))) return rc;
      FLK_LAUNCH_KERNEL(illum_grad_stage1<float>, dim3(capped(nitems)), dim3(256), lds, st, *a, *m, (const char*)gx_s2d, nchunk, nitems, partials);
    }
    FLK_LAUNCH_KERNEL(illum_grad_stage2, dim3((a->T * 3 + 127) / 128, a->delta_per_clip ? a->B : 1), dim3(128), 0, st, *a, *m, nchunk, partials, gdelta);
  }
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// arguments shared with the additive form already validated (api.cpp: flk_flicker_tone_slopes)
int flk_illum_tone_slopes_launch(const flk_apply_args* a, const flk_illum_args* m, float* slope, float* scale, hipStream_t stream) {
  static const char* who = "flk_flicker_tone_slopes";
  int rc = check_illum(who, a, m);
  if (rc) return rc;
  const int lds = (768 + m->enc_n + 1) * (int)sizeof(float);
  if ((rc = raise_lds<illum_tone_slopes_kernel>(lds))) return rc;
  FLK_LAUNCH_KERNEL(illum_tone_slopes_kernel, dim3(capped((long)a->B * a->T)), dim3(256), lds, stream, *a, *m, slope, scale);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
