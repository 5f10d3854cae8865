// Clip preparation on the device: raw uint8 frames [T,Hs,Ws,3] -> the normalised fp32 clip [T,Ho,Wo,3] the VideoResNet engines take.
// One kernel for the reference's get_transforms(train=False) chain (dataset.py:84-123, references/transforms_video.py,
// references/functional_video.py):  ToTensorVideo (/255) -> ResizeVideo(im_scale, keep_ratio; bilinear, align_corners=False) ->
// CenterCropVideo(input_size) -> NormalizeVideo(mean, std).  Only the crop window is computed; the resized image never exists.
//
// Arithmetic (fp32 throughout):
//   v(u8)  = float(u8) / 255.0f                        true division, from a 256-entry table built per workgroup
//   src(d) = max(fma(step, d + 0.5f, -0.5f), 0)         torch's source index AS ITS CPU KERNELS EVALUATE IT: the multiply-subtract is
//                                                       one fused operation there (measured); written with explicit
//                                                       intrinsics so that no compiler flag changes it
//   i0 = min(int(src), in - 1), i1 = min(i0 + 1, in - 1), lambda = clamp(src - i0, 0, 1)
//   out    = ((1-lh) * ((1-lw) v00 + lw v01) + lh * ((1-lw) v10 + lw v11) - mean[c]) / std[c]        true division
// `step` per axis comes from the host (videoresnet_spec.prepare_geometry: the "sizes" or the "scale_factor" rule).
//
// Mapping: workgroup = (`rows` consecutive output rows, frame t, clip).  The two source rows of every output row are staged in LDS
// -- only the byte segment [x0*3, (x0+span)*3) under the crop window, fetched as aligned dwords -- then each thread produces four
// consecutive output floats at a time (one 16-byte store; the output rows of a frame are contiguous).  Memory-bound: per 16-frame
// clip at 240x320 about 2 MB of source bytes under the window are read and 2.4 MB written.
// Every output element is a pure function of its own coordinates: the result does not depend on `rows` or on the grid.
// No atomics, no allocation, no host synchronisation.
//
// Second kernel, further down: clip_prepare_train_kernel, the training transform (a resampled crop box and a flip per clip).
//
// Sampled form of both kernels (flk_clip_prepare_sampled): the clip is cut from a whole resident video on the way.  Output frame t of
// clip k reads source frame idx[k][t] of the view instead of frame t; idx is a device int32 [nclip][T_out] table (8 KB at 64 clips of
// 32 frames: it does not fit the kernel-argument segment, so its pointer travels in the descriptor), the grid's frame dimension is
// T_out, and PrepClipDev.T is the number of source frames: every index read is clamped into [0, T - 1], so no table makes the kernel
// read outside the view.  Addressing only -- one uniform load per workgroup; staging, arithmetic, blend order, flip and box handling
// are the same statements, so a sampled launch gives bit for bit what the plain launch gives on the frames gathered beforehand.
// A frame that a table repeats (jitter step 0, padding with the last frame) is computed again.  Both kernels are templates on their
// descriptor type: the plain instantiations take the descriptor they always took and compile to the code they always were.
#include <math.h>
#include <type_traits>
#include "flk_internal.h"

namespace {

struct PrepClipDev {          // 56 bytes; FLK_PREP_MAX_CLIPS of them travel by value in the kernel argument
  const uint8_t* src;
  long long pitch_t;          // bytes between frames
  int pitch_h;                // bytes between rows
  int T, Hs, Ws;
  float step_h, step_w;
  int crop_i, crop_j;
  int x0, span;               // first source column under the crop window and the number of columns (host-computed, inside [0, Ws))
};

struct PrepLaunch {
  float* out;                 // already offset to the first clip row written
  long long clip_stride;      // floats between clips
  int Ho, Wo, rows, seg_stride, vec;
  float mean[3], std_[3];
  PrepClipDev clip[FLK_PREP_MAX_CLIPS];
};
// what a sampled descriptor adds to its plain one (both kernels)
struct PrepFrameTable {
  const int* idx;             // device int32 [nclip][gridDim.y]: source frame of every output frame
};
struct PrepLaunchSampled : PrepLaunch, PrepFrameTable {};
static_assert(sizeof(PrepLaunchSampled) <= 4096, "the launch descriptor must fit the kernel-argument segment");
template <class L>
constexpr bool prep_sampled = std::is_base_of<PrepFrameTable, L>::value;
// what a toned descriptor adds to its sampled one (both kernels): the clip is prepared from the DELIVERED video -- the source bytes
// after the 8-bit export of a per-frame flicker -- without that video ever being written.  A flicker is uniform over a frame, so
// the delivered frame is the raw frame through a byte -> byte map per (clip, output frame, channel)
struct PrepToneTable {
  const uint8_t* tone;        // device uint8 [nclip][gridDim.y][256][3]: tone[k][t][v][c] = the stored byte of source byte v, channel c
};
struct PrepLaunchToned : PrepLaunchSampled, PrepToneTable {};
static_assert(sizeof(PrepLaunchToned) <= 4096, "the launch descriptor must fit the kernel-argument segment");
template <class L>
constexpr bool prep_toned = std::is_base_of<PrepToneTable, L>::value;
constexpr int kPrepToneBytes = 768;        // one (clip, frame) table, staged in LDS behind everything the untoned kernels keep there

// the source frame of output frame t of the workgroup's clip: t itself, or the table's entry clamped into the view's [0, T - 1]
template <class L>
__device__ __forceinline__ int prep_source_frame(const L& p, int t, int T) {
  if constexpr (prep_sampled<L>) return min(max(p.idx[(size_t)blockIdx.z * gridDim.y + t], 0), T - 1);
  else return t;
}

// torch's area_pixel_compute_source_index (align_corners = False): scale * (dst + 0.5) - 0.5 with the multiply-subtract fused, as the
// vectorised CPU builds of torch evaluate it (separately rounded operations land up to 5.5e-5 away from F.interpolate at 239x317,
// the fused form within 7.2e-7 on every size tried)
__device__ __forceinline__ float prep_src(float step, int d) {
  const float s = __fmaf_rn(step, __fadd_rn((float)d, 0.5f), -0.5f);
  return s < 0.f ? 0.f : s;
}
// the same value on the host (fmaf is exact whatever the host's instruction set)
inline float prep_src_host(float step, int d) {
  const float s = fmaf(step, (float)d + 0.5f, -0.5f);
  return s < 0.f ? 0.f : s;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// toned launches, before phase A: the workgroup's table tone[clip][output frame] into LDS (bytes: no alignment asked of `tone`)
template <class L>
__device__ __forceinline__ void prep_stage_tone(const L& p, int t, uint8_t* tone_lds) {
  if constexpr (prep_toned<L>) {
    const uint8_t* g = p.tone + ((size_t)blockIdx.z * gridDim.y + t) * kPrepToneBytes;
    for (int k = threadIdx.x; k < kPrepToneBytes; k += 256) tone_lds[k] = g[k];
    __syncthreads();
  }
}
// the staged dword `w` of a row segment whose first byte sits `mis` bytes into dword 0, through the tone: byte b of the dword is at
// position 4w + b of the slot and its channel is (position - mis) mod 3.  The up to three bytes in front of the segment and those
// behind it are mapped too (through some channel's column: any byte is in range); no compute loop reads them
__device__ __forceinline__ unsigned prep_tone_dword(const uint8_t* tone_lds, unsigned v, int w, int mis) {
  int ch = (4 * w - mis + 3) % 3;            // mis <= 3: never negative
  unsigned r = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    r |= (unsigned)tone_lds[((v >> (8 * b)) & 255u) * 3 + ch] << (8 * b);
    ch = ch == 2 ? 0 : ch + 1;
  }
  return r;
}

template <class L>
__global__ __launch_bounds__(256) void clip_prepare_kernel(const L p) {
  extern __shared__ unsigned prep_lds[];      // [256] fp32 table u8 / 255 | [2 * rows] segment misalignments | 2 * rows row segments
  const PrepClipDev& c = p.clip[blockIdx.z];
  const int t = blockIdx.y;                   // the output frame
  if (!prep_sampled<L> && t >= c.T) return;         // sampled: the grid's frame dimension is T_out, the same for every clip
  float* tab = (float*)prep_lds;
  int* mis_of = (int*)(prep_lds + 256);
  unsigned* seg = prep_lds + 256 + 2 * p.rows;
  const uint8_t* segb = (const uint8_t*)seg;
  tab[threadIdx.x] = (float)threadIdx.x / 255.0f;
  const int oh0 = blockIdx.x * p.rows;
  const int nrow = min(p.rows, p.Ho - oh0);
  const int ndw = p.seg_stride >> 2;
  const uint8_t* frame = c.src + (long long)prep_source_frame(p, t, c.T) * c.pitch_t;
  const int nbytes = c.span * 3;
  uint8_t* tone_lds = (uint8_t*)(seg + 2 * p.rows * ndw);      // toned launches only: 768 bytes more than the untoned ones ask for
  prep_stage_tone(p, t, tone_lds);
  // ---- stage: slot 2r + s = source row s (0 top, 1 bottom) of output row oh0 + r; columns [x0, x0 + span) ----
  for (int k = threadIdx.x; k < 2 * nrow * ndw; k += 256) {
    const int slot = k / ndw, w = k - slot * ndw;
    int h = min((int)prep_src(c.step_h, c.crop_i + oh0 + (slot >> 1)), c.Hs - 1);
    if (slot & 1) h = min(h + 1, c.Hs - 1);
    const uint8_t* row = frame + (long long)h * c.pitch_h + c.x0 * 3;
    const int mis = (int)((size_t)row & 3);
    if (w == 0) mis_of[slot] = mis;
    // aligned dwords that hold at least one byte of the segment: never beyond the dword of its last byte
    if (4 * w < mis + nbytes) {
      if constexpr (prep_toned<L>) seg[slot * ndw + w] = prep_tone_dword(tone_lds, *(const unsigned*)(row - mis + 4 * w), w, mis);
      else seg[slot * ndw + w] = *(const unsigned*)(row - mis + 4 * w);
    }
  }
  __syncthreads();
  // ---- compute: four consecutive floats of the workgroup's contiguous output run per thread and pass ----
  const int rowlen = p.Wo * 3, nfl = nrow * rowlen;
  float* dst = p.out + (long long)blockIdx.z * p.clip_stride + ((long long)t * p.Ho + oh0) * rowlen;
  for (int e = threadIdx.x * 4; e < nfl; e += 1024) {
    int r = e / rowlen;
    const int rem = e - r * rowlen;
    int ow = rem / 3, ch = rem - ow * 3;
    float lh = 0.f, lw = 0.f;
    const uint8_t *top = segb, *bot = segb;
    int o0 = 0, o1 = 0;
    auto row_state = [&]() {
      const float sh = prep_src(c.step_h, c.crop_i + oh0 + r);
      const int h0 = min((int)sh, c.Hs - 1);
      lh = clamp01(sh - (float)h0);
      top = segb + (2 * r) * p.seg_stride + mis_of[2 * r];
      bot = segb + (2 * r + 1) * p.seg_stride + mis_of[2 * r + 1];
    };
    auto col_state = [&]() {
      const float sw = prep_src(c.step_w, c.crop_j + ow);
      const int i0 = min((int)sw, c.Ws - 1), i1 = min(i0 + 1, c.Ws - 1);
      lw = clamp01(sw - (float)i0);
      o0 = min(max(i0 - c.x0, 0), c.span - 1) * 3;
      o1 = min(max(i1 - c.x0, 0), c.span - 1) * 3;
    };
    row_state();
    col_state();
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = 0.f;
      if (e + j < nfl) {
        const float w0 = 1.f - lw, h0w = 1.f - lh;
        const float a = w0 * tab[top[o0 + ch]] + lw * tab[top[o1 + ch]];
        const float b = w0 * tab[bot[o0 + ch]] + lw * tab[bot[o1 + ch]];
        const float x = h0w * a + lh * b;
        const float mean = ch == 0 ? p.mean[0] : ch == 1 ? p.mean[1] : p.mean[2];
        const float sd = ch == 0 ? p.std_[0] : ch == 1 ? p.std_[1] : p.std_[2];
        v[j] = (x - mean) / sd;
        if (++ch == 3) {
          ch = 0;
          if (++ow == p.Wo) {
            ow = 0;
            ++r;
            if (e + j + 1 < nfl) row_state();
          }
          if (e + j + 1 < nfl) col_state();
        }
      }
    }
    if (p.vec && e + 3 < nfl) {
      *(f32x4*)(dst + e) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < nfl) dst[e + j] = v[j];
    }
  }
}

}  // namespace

// arguments already validated (api.cpp: flk_clip_prepare, flk_clip_prepare_sampled); everything here up to the launch is host arithmetic.
// frame_idx: null for the plain launch, else the device table [nclip][T_out] of the sampled one; tone (with frame_idx only): null, or
// the device tables [nclip][T_out][256][3] of the toned one
int flk_clip_prepare_launch(const flk_prepare_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, float* out,
                            hipStream_t stream) {
  PrepLaunchToned p;
  int max_span = 1, max_T = 1;
  for (int i = 0; i < a->nclip; ++i) {
    const flk_prep_clip& s = a->clips[i];
    PrepClipDev& d = p.clip[i];
    d.src = s.src; d.pitch_t = s.pitch_t; d.pitch_h = (int)s.pitch_h;
    d.T = s.T; d.Hs = s.Hs; d.Ws = s.Ws;
    d.step_h = s.step_h; d.step_w = s.step_w; d.crop_i = s.crop_i; d.crop_j = s.crop_j;
    // columns under the crop window: [i0(first output column), i1(last output column)] with the kernel's own fp32 sequence
    const float s0 = prep_src_host(s.step_w, s.crop_j), s1 = prep_src_host(s.step_w, s.crop_j + a->Wo - 1);
    const int x0 = s0 >= (float)(s.Ws - 1) ? s.Ws - 1 : (int)s0;
    const int l1 = s1 >= (float)(s.Ws - 1) ? s.Ws - 1 : (int)s1;
    const int x1 = l1 + 1 < s.Ws ? l1 + 1 : s.Ws - 1;
    d.x0 = x0; d.span = x1 - x0 + 1;
    if (d.span > max_span) max_span = d.span;
    if (s.T > max_T) max_T = s.T;
  }
  const int seg_stride = (max_span * 3 + 3 + 3) / 4 * 4;       // the segment, up to 3 bytes of misalignment, whole dwords
  int rows = 4;
  while (rows > 1 && (size_t)2 * rows * seg_stride > 48 * 1024) rows >>= 1;
  FLK_REQUIRE((size_t)2 * rows * seg_stride <= 60 * 1024, "flk_clip_prepare: the crop window spans %d source columns, more than one workgroup stages", max_span);
  if (frame_idx) max_T = T_out;                // the grid's frame dimension: output frames
  FLK_REQUIRE(max_T <= 65535, "flk_clip_prepare: more than 65535 frames");
  p.out = out + a->out_clip_offset * a->out_clip_stride;
  p.clip_stride = a->out_clip_stride;
  p.Ho = a->Ho; p.Wo = a->Wo; p.rows = rows; p.seg_stride = seg_stride;
  p.vec = ((size_t)p.out % 16 == 0) && a->out_clip_stride % 4 == 0 && (a->Wo * 3) % 4 == 0;
  for (int k = 0; k < 3; ++k) { p.mean[k] = a->mean[k]; p.std_[k] = a->std[k]; }
  const size_t lds = (size_t)(256 + 2 * rows) * 4 + (size_t)2 * rows * seg_stride;
  const dim3 grid((unsigned)((a->Ho + rows - 1) / rows), (unsigned)max_T, (unsigned)a->nclip);
  if (frame_idx && tone) {
    p.idx = frame_idx;
    p.tone = tone;
    FLK_LAUNCH_KERNEL(clip_prepare_kernel<PrepLaunchToned>, grid, dim3(256), lds + kPrepToneBytes, stream, p);
  } else if (frame_idx) {
    p.idx = frame_idx;
    FLK_LAUNCH_KERNEL(clip_prepare_kernel<PrepLaunchSampled>, grid, dim3(256), lds, stream, static_cast<const PrepLaunchSampled&>(p));
  } else {
    FLK_LAUNCH_KERNEL(clip_prepare_kernel<PrepLaunch>, grid, dim3(256), lds, stream, static_cast<const PrepLaunch&>(p));
  }
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The training transform (dataset.py:105-118): ToTensorVideo -> ResizeVideo -> RandomResizedCropVideo / RandomCropVideo ->
// RandomHorizontalFlipVideo -> NormalizeVideo.  The random draws are the host's (videoresnet_spec.train_crop_params); the kernel takes a
// box (i, j, h, w) in the resized image and a flip per clip.  Two bilinear resamplings fused: neither the resized image nor the
// cropped box reaches HBM.
//
// Arithmetic (fp32):
//   stage 1   R[y, x] = the resized image at (i + y, j + x): clip_prepare_kernel's own sequence before its normalisation -- prep_src, the
//             /255 table, blend along W within the two source rows, then along H; every blend w0 * v0 + w1 * v1 is fma(w0, v0, w1 * v1)
//             (prep_blend), in both stages
//   stage 2   step2 = float(h) / float(Ho) per axis (a float32 division: F.interpolate(size=...)); src = prep_src(step2, d);
//             y0 = min(int(src), h - 1), y1 = min(y0 + 1, h - 1), lambda = clamp(src - y0, 0, 1);
//             v = (1-lh) * ((1-lw) R[y0,x0] + lw R[y0,x1]) + lh * ((1-lw) R[y1,x0] + lw R[y1,x1])
//   flip      output column ow takes the value computed for column Wo - 1 - ow
//   out       (v - mean[c]) / std[c], true division
//
// Layout chosen: workgroup = (`rows` consecutive output rows, frame t, clip), 256 threads, three phases with a barrier between them.
//   A  stage the source-row byte segments under the box (columns [x0, x0 + span), aligned dwords, the misalignment kept per row as
//      clip_prepare_kernel does): two source rows per intermediate row.
//   B  one thread per intermediate pixel: R[y, 0..w) for the workgroup's intermediate rows, float32, into LDS (3 floats per thread at
//      a stride of 3 words: no bank conflicts).
//   C  four consecutive output floats per thread and pass from R, one 16-byte store.
// Intermediate rows: when the rows y0(first output row) .. y1(last output row) of the box are no more than the 2 * rows slots, the
// workgroup computes that contiguous range once (neighbouring output rows share rows whenever the box is resampled by a step below 2:
// at the default sampler's steps of 1.0 .. 1.3 and 3 rows per workgroup about 5 rows instead of 6); otherwise slot 2r + s holds row y_s of output row r.  R[y, x]
// is a pure function of (y, x) and the clip's parameters, so the two forms, any `rows` and any grid give the same bits.
// A box of the output size skips B and the second stage: C then is clip_prepare_kernel's own loop on the staged bytes (the reason is
// written at that loop).
// LDS at 240x320 -> 128x170 with the whole width under the box: 6 slots x (2 x 968 source bytes + 2040 bytes of R) = 24 KB, 6
// workgroups per CU.  No atomics, no allocation, no host synchronisation; all addressing inside [0, Hs) x [0, Ws) of the clip's view.
namespace {

struct PrepTrainClipDev {     // 56 bytes; FLK_PREP_MAX_CLIPS of them travel by value in the kernel argument
  const uint8_t* src;
  long long pitch_t;          // bytes between frames
  int pitch_h;                // bytes between rows
  int T, Hs, Ws;
  float step_h, step_w;       // stage 1: source step per resized pixel
  int i, j, h, w;             // the box in the resized image
};

struct PrepTrainLaunch {
  float* out;                 // already offset to the first clip row written
  long long clip_stride;      // floats between clips
  unsigned long long flips;   // bit k: clip k is flipped along W
  int Ho, Wo, rows, seg_stride, r_stride, vec;       // r_stride: floats between intermediate rows in LDS
  float mean[3], std_[3];
  PrepTrainClipDev clip[FLK_PREP_MAX_CLIPS];
};
static_assert(FLK_PREP_MAX_CLIPS <= 64, "one flip bit per clip");
struct PrepTrainLaunchSampled : PrepTrainLaunch, PrepFrameTable {};
static_assert(sizeof(PrepTrainLaunchSampled) <= 4096, "the launch descriptor must fit the kernel-argument segment");
struct PrepTrainLaunchToned : PrepTrainLaunchSampled, PrepToneTable {};
static_assert(sizeof(PrepTrainLaunchToned) <= 4096, "the launch descriptor must fit the kernel-argument segment");

// source columns under the box: [x0, x0 + span); the same fp32 sequence on the host (LDS sizing) and in the kernel
__host__ __device__ inline void prep_train_span(float step_w, int j, int w, int Ws, int* x0, int* span) {
#ifdef __HIP_DEVICE_COMPILE__
  const float s0 = prep_src(step_w, j), s1 = prep_src(step_w, j + w - 1);
#else
  const float s0 = prep_src_host(step_w, j), s1 = prep_src_host(step_w, j + w - 1);
#endif
  const int a = s0 >= (float)(Ws - 1) ? Ws - 1 : (int)s0;
  const int l = s1 >= (float)(Ws - 1) ? Ws - 1 : (int)s1;
  *x0 = a;
  *span = (l + 1 < Ws ? l + 1 : Ws - 1) - a + 1;
}

// w0 * v0 + w1 * v1 as ONE fixed sequence, fma(w0, v0, w1 * v1).  Left as a plain expression the compiler fuses it one way for some
// of a thread's four unrolled elements and another way for the rest (it does in clip_prepare_kernel): a flipped clip, whose values
// are computed at other positions of the loop, would then not be the unflipped clip reversed.
__device__ __forceinline__ float prep_blend(float w0, float v0, float w1, float v1) {
#pragma clang fp contract(off)
  return __builtin_fmaf(w0, v0, w1 * v1);
}

template <class L>
__global__ __launch_bounds__(256) void clip_prepare_train_kernel(const L p) {
  // [256] fp32 table u8 / 255 | [2 * cap] segment misalignments | 2 * cap source-row segments | cap intermediate rows (cap = 2 * rows)
  extern __shared__ unsigned prep_train_lds[];
  const PrepTrainClipDev& c = p.clip[blockIdx.z];
  const int t = blockIdx.y;                   // the output frame
  if (!prep_sampled<L> && t >= c.T) return;         // sampled: the grid's frame dimension is T_out, the same for every clip
  const int cap = 2 * p.rows;
  float* tab = (float*)prep_train_lds;
  int* mis_of = (int*)(prep_train_lds + 256);
  unsigned* seg = prep_train_lds + 256 + 2 * cap;
  const uint8_t* segb = (const uint8_t*)seg;
  const int ndw = p.seg_stride >> 2;
  float* R = (float*)(seg + 2 * cap * ndw);
  tab[threadIdx.x] = (float)threadIdx.x / 255.0f;
  const int oh0 = blockIdx.x * p.rows;
  const int nrow = min(p.rows, p.Ho - oh0);
  const float step2_h = __fdiv_rn((float)c.h, (float)p.Ho), step2_w = __fdiv_rn((float)c.w, (float)p.Wo);
  const bool flip = (p.flips >> blockIdx.z) & 1ull;
  // ---- the workgroup's intermediate rows (rows of the box): the range [ya, yb] when it fits the slots, else a pair per output row ----
  auto y0_of = [&](int oh) { return min((int)prep_src(step2_h, oh), c.h - 1); };
  // a box of the output size (RandomCropVideo; the evaluation transform's own window): stage 2 is the identity and is not run -- the
  // output rows are the resized rows i + oh themselves, computed straight from the staged bytes (see below)
  const bool direct = c.h == p.Ho && c.w == p.Wo;
  const int ya = direct ? oh0 : y0_of(oh0), yb = direct ? oh0 + nrow - 1 : min(y0_of(oh0 + nrow - 1) + 1, c.h - 1);
  const bool range = yb - ya + 1 <= cap;
  const int ni = range ? yb - ya + 1 : 2 * nrow;
  auto slot_y = [&](int s) {
    if (range) return ya + s;
    const int y = y0_of(oh0 + (s >> 1));
    return (s & 1) ? min(y + 1, c.h - 1) : y;
  };
  int x0, span;
  prep_train_span(c.step_w, c.j, c.w, c.Ws, &x0, &span);
  const uint8_t* frame = c.src + (long long)prep_source_frame(p, t, c.T) * c.pitch_t;
  const int nbytes = span * 3;
  uint8_t* tone_lds = (uint8_t*)(R + cap * p.r_stride);        // toned launches only: 768 bytes more than the untoned ones ask for
  prep_stage_tone(p, t, tone_lds);
  // ---- A: segment 2s + v = source row v (0 top, 1 bottom) of intermediate slot s; columns [x0, x0 + span) ----
  for (int k = threadIdx.x; k < 2 * ni * ndw; k += 256) {
    const int q = k / ndw, w = k - q * ndw;
    int h = min((int)prep_src(c.step_h, c.i + slot_y(q >> 1)), c.Hs - 1);
    if (q & 1) h = min(h + 1, c.Hs - 1);
    const uint8_t* row = frame + (long long)h * c.pitch_h + x0 * 3;
    const int mis = (int)((size_t)row & 3);
    if (w == 0) mis_of[q] = mis;
    // aligned dwords that hold at least one byte of the segment: never beyond the dword of its last byte
    if (4 * w < mis + nbytes) {
      if constexpr (prep_toned<L>) seg[q * ndw + w] = prep_tone_dword(tone_lds, *(const unsigned*)(row - mis + 4 * w), w, mis);
      else seg[q * ndw + w] = *(const unsigned*)(row - mis + 4 * w);
    }
  }
  __syncthreads();
  if (direct) {
    // ---- the evaluation kernel's compute loop on the box's rows: slot r of the range is output row oh0 + r.  This is
    // clip_prepare_kernel's loop statement for statement, on purpose: its blend is written as plain expressions, which the compiler
    // contracts into fused multiply-adds differently for the four unrolled elements, so only the same statements reproduce its bits
    // (the identity tests/test_clip_prepare_train_gpu.py pins).  Every value is computed at its UNFLIPPED position and stored
    // mirrored, so a flipped clip is the unflipped one reversed, bit for bit. ----
    const int rowlen = p.Wo * 3, nfl = nrow * rowlen;
    float* dst = p.out + (long long)blockIdx.z * p.clip_stride + ((long long)t * p.Ho + oh0) * rowlen;
    for (int e = threadIdx.x * 4; e < nfl; e += 1024) {
      int r = e / rowlen;
      const int rem = e - r * rowlen;
      int ow = rem / 3, ch = rem - ow * 3;
      float lh = 0.f, lw = 0.f;
      const uint8_t *top = segb, *bot = segb;
      int o0 = 0, o1 = 0;
      auto row_state = [&]() {
        const float sh = prep_src(c.step_h, c.i + oh0 + r);
        const int h0 = min((int)sh, c.Hs - 1);
        lh = clamp01(sh - (float)h0);
        top = segb + (2 * r) * p.seg_stride + mis_of[2 * r];
        bot = segb + (2 * r + 1) * p.seg_stride + mis_of[2 * r + 1];
      };
      auto col_state = [&]() {
        const float sw = prep_src(c.step_w, c.j + ow);
        const int i0 = min((int)sw, c.Ws - 1), i1 = min(i0 + 1, c.Ws - 1);
        lw = clamp01(sw - (float)i0);
        o0 = min(max(i0 - x0, 0), span - 1) * 3;
        o1 = min(max(i1 - x0, 0), span - 1) * 3;
      };
      row_state();
      col_state();
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = 0.f;
        if (e + j < nfl) {
          const float w0 = 1.f - lw, h0w = 1.f - lh;
          const float a = w0 * tab[top[o0 + ch]] + lw * tab[top[o1 + ch]];
          const float b = w0 * tab[bot[o0 + ch]] + lw * tab[bot[o1 + ch]];
          const float x = h0w * a + lh * b;
          const float mean = ch == 0 ? p.mean[0] : ch == 1 ? p.mean[1] : p.mean[2];
          const float sd = ch == 0 ? p.std_[0] : ch == 1 ? p.std_[1] : p.std_[2];
          v[j] = (x - mean) / sd;
          if (++ch == 3) {
            ch = 0;
            if (++ow == p.Wo) {
              ow = 0;
              ++r;
              if (e + j + 1 < nfl) row_state();
            }
            if (e + j + 1 < nfl) col_state();
          }
        }
      }
      if (flip) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < nfl) {
            const int fr = (e + j) / rowlen, frem = (e + j) - fr * rowlen, fw = frem / 3;
            dst[fr * rowlen + (p.Wo - 1 - fw) * 3 + (frem - fw * 3)] = v[j];
          }
      } else if (p.vec && e + 3 < nfl) {
        *(f32x4*)(dst + e) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < nfl) dst[e + j] = v[j];
      }
    }
    return;
  }
  // ---- B: R[slot][x][ch] = the resized image at (i + y, j + x), one pixel per thread and pass ----
  for (int k = threadIdx.x; k < ni * c.w; k += 256) {
    const int s = k / c.w, x = k - s * c.w;
    const float sh = prep_src(c.step_h, c.i + slot_y(s));
    const float lh = clamp01(sh - (float)min((int)sh, c.Hs - 1));
    const uint8_t* top = segb + (2 * s) * p.seg_stride + mis_of[2 * s];
    const uint8_t* bot = segb + (2 * s + 1) * p.seg_stride + mis_of[2 * s + 1];
    const float sw = prep_src(c.step_w, c.j + x);
    const int i0 = min((int)sw, c.Ws - 1), i1 = min(i0 + 1, c.Ws - 1);
    const float lw = clamp01(sw - (float)i0);
    const int o0 = min(max(i0 - x0, 0), span - 1) * 3;
    const int o1 = min(max(i1 - x0, 0), span - 1) * 3;
    float* r = R + s * p.r_stride + x * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float w0 = 1.f - lw, h0w = 1.f - lh;
      const float a = prep_blend(w0, tab[top[o0 + ch]], lw, tab[top[o1 + ch]]);
      const float b = prep_blend(w0, tab[bot[o0 + ch]], lw, tab[bot[o1 + ch]]);
      r[ch] = prep_blend(h0w, a, lh, b);
    }
  }
  __syncthreads();
  // ---- C: four consecutive floats of the workgroup's contiguous output run per thread and pass ----
  const int rowlen = p.Wo * 3, nfl = nrow * rowlen;
  float* dst = p.out + (long long)blockIdx.z * p.clip_stride + ((long long)t * p.Ho + oh0) * rowlen;
  for (int e = threadIdx.x * 4; e < nfl; e += 1024) {
    int r = e / rowlen;
    const int rem = e - r * rowlen;
    int ow = rem / 3, ch = rem - ow * 3;
    float lh = 0.f, lw = 0.f;
    const float *top = R, *bot = R;
    int o0 = 0, o1 = 0;
    auto row_state = [&]() {
      const float sy = prep_src(step2_h, oh0 + r);
      const int y0 = min((int)sy, c.h - 1), y1 = min(y0 + 1, c.h - 1);
      lh = clamp01(sy - (float)y0);
      top = R + (range ? y0 - ya : 2 * r) * p.r_stride;
      bot = R + (range ? y1 - ya : 2 * r + 1) * p.r_stride;
    };
    auto col_state = [&]() {
      const float sx = prep_src(step2_w, flip ? p.Wo - 1 - ow : ow);
      const int b0 = min((int)sx, c.w - 1), b1 = min(b0 + 1, c.w - 1);
      lw = clamp01(sx - (float)b0);
      o0 = b0 * 3;
      o1 = b1 * 3;
    };
    row_state();
    col_state();
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = 0.f;
      if (e + j < nfl) {
        const float w0 = 1.f - lw, h0w = 1.f - lh;
        const float a = prep_blend(w0, top[o0 + ch], lw, top[o1 + ch]);
        const float b = prep_blend(w0, bot[o0 + ch], lw, bot[o1 + ch]);
        const float x = prep_blend(h0w, a, lh, b);
        const float mean = ch == 0 ? p.mean[0] : ch == 1 ? p.mean[1] : p.mean[2];
        const float sd = ch == 0 ? p.std_[0] : ch == 1 ? p.std_[1] : p.std_[2];
        v[j] = (x - mean) / sd;
        if (++ch == 3) {
          ch = 0;
          if (++ow == p.Wo) {
            ow = 0;
            ++r;
            if (e + j + 1 < nfl) row_state();
          }
          if (e + j + 1 < nfl) col_state();
        }
      }
    }
    if (p.vec && e + 3 < nfl) {
      *(f32x4*)(dst + e) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < nfl) dst[e + j] = v[j];
    }
  }
}

}  // namespace

#ifndef FLK_PREP_TRAIN_ROWS
#define FLK_PREP_TRAIN_ROWS 3       // output rows per workgroup (the result does not depend on it).  3 rows of 112 x 3 floats are 252 four-float
                                    // items, one full pass of the 256 threads in phase C; measured 62.7 us against 65.3 (4 rows) and 82.8 (6 rows)
                                    // per launch of 16 clips of 16 x 240 x 320 (tools/prepare_time.py)
#endif

// arguments already validated (api.cpp: flk_clip_prepare_train, flk_clip_prepare_sampled); everything here up to the launch is host
// arithmetic.  frame_idx: null for the plain launch, else the device table [nclip][T_out] of the sampled one; tone (with frame_idx
// only): null, or the device tables [nclip][T_out][256][3] of the toned one
int flk_clip_prepare_train_launch(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, const uint8_t* tone,
                                  float* out, hipStream_t stream) {
  PrepTrainLaunchToned p;
  int max_span = 1, max_T = 1, max_w = 1;
  p.flips = 0;
  for (int i = 0; i < a->nclip; ++i) {
    const flk_prep_clip& s = a->clips[i];
    const flk_prep_box& b = boxes[i];
    PrepTrainClipDev& d = p.clip[i];
    d.src = s.src; d.pitch_t = s.pitch_t; d.pitch_h = (int)s.pitch_h;
    d.T = s.T; d.Hs = s.Hs; d.Ws = s.Ws;
    d.step_h = s.step_h; d.step_w = s.step_w;
    d.i = b.i; d.j = b.j; d.h = b.h; d.w = b.w;
    if (b.flip) p.flips |= 1ull << i;
    int x0, span;
    prep_train_span(s.step_w, b.j, b.w, s.Ws, &x0, &span);
    if (span > max_span) max_span = span;
    if (b.w > max_w) max_w = b.w;
    if (s.T > max_T) max_T = s.T;
  }
  const size_t seg_stride = ((size_t)max_span * 3 + 3 + 3) / 4 * 4;       // the segment, up to 3 bytes of misalignment, whole dwords
  const size_t r_stride = (size_t)max_w * 3;
  auto lds_of = [&](int rows) { return (size_t)(256 + 4 * rows) * 4 + (size_t)2 * rows * (2 * seg_stride + 4 * r_stride); };
  int rows = FLK_PREP_TRAIN_ROWS;
  while (rows > 1 && lds_of(rows) > 48 * 1024) rows >>= 1;
  FLK_REQUIRE(lds_of(rows) <= 60 * 1024, "flk_clip_prepare_train: a box %d resized columns wide over %d source columns is more than one workgroup stages",
              max_w, max_span);
  if (frame_idx) max_T = T_out;                // the grid's frame dimension: output frames
  FLK_REQUIRE(max_T <= 65535, "flk_clip_prepare_train: more than 65535 frames");
  p.out = out + a->out_clip_offset * a->out_clip_stride;
  p.clip_stride = a->out_clip_stride;
  p.Ho = a->Ho; p.Wo = a->Wo; p.rows = rows; p.seg_stride = (int)seg_stride; p.r_stride = (int)r_stride;
  p.vec = ((size_t)p.out % 16 == 0) && a->out_clip_stride % 4 == 0 && (a->Wo * 3) % 4 == 0;
  for (int k = 0; k < 3; ++k) { p.mean[k] = a->mean[k]; p.std_[k] = a->std[k]; }
  const dim3 grid((unsigned)((a->Ho + rows - 1) / rows), (unsigned)max_T, (unsigned)a->nclip);
  if (frame_idx && tone) {
    p.idx = frame_idx;
    p.tone = tone;
    FLK_LAUNCH_KERNEL(clip_prepare_train_kernel<PrepTrainLaunchToned>, grid, dim3(256), lds_of(rows) + kPrepToneBytes, stream, p);
  } else if (frame_idx) {
    p.idx = frame_idx;
    FLK_LAUNCH_KERNEL(clip_prepare_train_kernel<PrepTrainLaunchSampled>, grid, dim3(256), lds_of(rows), stream,
                      static_cast<const PrepTrainLaunchSampled&>(p));
  } else {
    FLK_LAUNCH_KERNEL(clip_prepare_train_kernel<PrepTrainLaunch>, grid, dim3(256), lds_of(rows), stream, static_cast<const PrepTrainLaunch&>(p));
  }
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The gradient of a toned preparation with respect to the flicker (flk_clip_prepare_grad).  The delivered value of an output pixel
// is the resampling of tone-mapped source bytes; straight through the 8-bit rounding, its derivative with respect to the frame's
// delta value is the SAME resampling of the per-byte slopes slope[k][t][byte][c] (flk_flicker_tone_slopes) -- J(oh, ow, c): the
// indices, taps and lambdas of clip_prepare_train_kernel (prep_src; stage 1 within two source rows then along H; stage 2 on the box;
// a flipped clip pairs g at column ow with J of column Wo - 1 - ow), every blend the fixed prep_blend sequence, no mean and no std.
// The evaluation transform is the box (crop_i, crop_j, Ho, Wo) without a flip; a box of the output size makes stage 2 the identity
// (lambda = 0 exactly: prep_blend(1, v, 0, .) = v), so it is not run.
//   gdelta[k][t][c] = scale[k][t][c] * sum over (oh, ow) of g[k][t][oh][ow][c] * J(oh, ow, c)
// Order (fixed; no atomics; independent of the grid, of the rows a workgroup takes and of the other clips of the call): ONE WAVE per
// (clip, frame, output row) -- lane l adds the rounded products of columns l, l + 64, ... ascending from +0, each sum rounded on its
// own; the 64 lanes fold by the shuffle tree 32, .., 1; partials[k][t][oh][c].  The finishing launch adds a (clip, frame, channel)'s
// rows ascending from +0 and multiplies by scale once.  A clip's result is that of a call holding that clip alone.
// Layout: workgroup = (kPrepGradRows output rows, frame, clip), 4 waves striding over the rows; the 3 KB of slopes of (clip, frame)
// staged in LDS; the source bytes are read in place (all addressing clamped into [0, Hs) x [0, Ws) of the view, the frame index into
// [0, T - 1]): 16 taps of 3 bytes per output pixel at most, neighbours sharing cache lines.
namespace {

constexpr int kPrepGradRows = 16;

struct PrepGradLaunch : PrepFrameTable {
  const float* slope;         // device fp32 [nclip][T_out][256][3]
  const void* gx;             // device [nclip][T_out][Ho/2][Wo/2][16], fp32 or bf16
  float* partials;            // device fp32 [nclip][T_out][Ho][3]
  unsigned long long flips;
  int Ho, Wo;
  PrepTrainClipDev clip[FLK_PREP_MAX_CLIPS];
};
static_assert(sizeof(PrepGradLaunch) <= 4096, "the launch descriptor must fit the kernel-argument segment");

__device__ __forceinline__ float prep_mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float prep_add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
template <typename TI> __device__ __forceinline__ float prep_grad_load(const void* gx, size_t i) {
  if constexpr (sizeof(TI) == 4) return ((const float*)gx)[i];
  else return __uint_as_float((unsigned)((const unsigned short*)gx)[i] << 16);
}

template <typename TI>
__global__ __launch_bounds__(256) void clip_prepare_grad_kernel(const PrepGradLaunch p) {
  __shared__ float S[768];
  const PrepTrainClipDev& c = p.clip[blockIdx.z];
  const int t = blockIdx.y, T_out = gridDim.y;
  const size_t kt = (size_t)blockIdx.z * T_out + t;
  for (int i = threadIdx.x; i < 768; i += 256) S[i] = p.slope[kt * 768 + i];
  __syncthreads();
  const uint8_t* frame = c.src + (long long)prep_source_frame(p, t, c.T) * c.pitch_t;
  const bool flip = (p.flips >> blockIdx.z) & 1ull;
  const bool direct = c.h == p.Ho && c.w == p.Wo;
  const float step2_h = __fdiv_rn((float)c.h, (float)p.Ho), step2_w = __fdiv_rn((float)c.w, (float)p.Wo);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int oh_end = min((int)(blockIdx.x + 1) * kPrepGradRows, p.Ho);
  // R[y, x][0..2] on slopes: the resized image at (i + y, j + x) of the box
  auto resized = [&](int y, int x, float* r) {
    const float sh = prep_src(c.step_h, c.i + y);
    const int h0 = min((int)sh, c.Hs - 1), h1 = min(h0 + 1, c.Hs - 1);
    const float lh = clamp01(sh - (float)h0);
    const float sw = prep_src(c.step_w, c.j + x);
    const int i0 = min((int)sw, c.Ws - 1), i1 = min(i0 + 1, c.Ws - 1);
    const float lw = clamp01(sw - (float)i0);
    const uint8_t* top = frame + (long long)h0 * c.pitch_h;
    const uint8_t* bot = frame + (long long)h1 * c.pitch_h;
    const float w0 = 1.f - lw, h0w = 1.f - lh;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float a = prep_blend(w0, S[top[i0 * 3 + ch] * 3 + ch], lw, S[top[i1 * 3 + ch] * 3 + ch]);
      const float b = prep_blend(w0, S[bot[i0 * 3 + ch] * 3 + ch], lw, S[bot[i1 * 3 + ch] * 3 + ch]);
      r[ch] = prep_blend(h0w, a, lh, b);
    }
  };
  for (int oh = blockIdx.x * kPrepGradRows + wave; oh < oh_end; oh += 4) {      // uniform over the wave
    const float sy = prep_src(step2_h, oh);
    const int y0 = direct ? oh : min((int)sy, c.h - 1), y1 = min(y0 + 1, c.h - 1);
    const float lh2 = clamp01(sy - (float)y0);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int ow = lane; ow < p.Wo; ow += 64) {
      const int oc = flip ? p.Wo - 1 - ow : ow;        // the column whose value the forward stores at ow
      float J[3];
      if (direct) {
        resized(y0, oc, J);
      } else {
        const float sx = prep_src(step2_w, oc);
        const int b0 = min((int)sx, c.w - 1), b1 = min(b0 + 1, c.w - 1);
        const float lw2 = clamp01(sx - (float)b0);
        float r00[3], r01[3], r10[3], r11[3];
        resized(y0, b0, r00);
        resized(y0, b1, r01);
        resized(y1, b0, r10);
        resized(y1, b1, r11);
        const float w0 = 1.f - lw2, h0w = 1.f - lh2;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          J[ch] = prep_blend(h0w, prep_blend(w0, r00[ch], lw2, r01[ch]), lh2, prep_blend(w0, r10[ch], lw2, r11[ch]));
      }
      const size_t gi = (((kt * (p.Ho >> 1) + (oh >> 1)) * (p.Wo >> 1) + (ow >> 1)) << 4) + ((oh & 1) * 2 + (ow & 1)) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] = prep_add_rn(acc[ch], prep_mul_rn(prep_grad_load<TI>(p.gx, gi + ch), J[ch]));
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v = acc[ch];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = prep_add_rn(v, __shfl_down(v, o, 64));
      if (lane == 0) p.partials[(kt * p.Ho + oh) * 3 + ch] = v;
    }
  }
}

// one thread per (clip, frame, channel): its rows ascending from +0, then the finishing factor
__global__ __launch_bounds__(256) void clip_prepare_grad_finish(const float* partials, const float* scale, int n3, int Ho, float* gdelta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n3) return;
  const size_t kt = i / 3;
  const int ch = i - (int)kt * 3;
  float s = 0.f;
  for (int oh = 0; oh < Ho; ++oh) s = prep_add_rn(s, partials[(kt * Ho + oh) * 3 + ch]);
  const float sc = scale[i];
  gdelta[i] = sc == 0.f ? 0.f : prep_mul_rn(s, sc);       // a masked value is +0 whatever the sum is, as in grad_reduce_stage2
}

}  // namespace

// arguments already validated (api.cpp: flk_clip_prepare_grad); boxes null: the evaluation transform's window, unflipped
int flk_clip_prepare_grad_launch(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, const float* slope,
                                 const float* scale, const void* gx_s2d, int dtype, float* gdelta, float* partials, hipStream_t stream) {
  PrepGradLaunch p;
  p.idx = frame_idx;
  p.slope = slope; p.gx = gx_s2d; p.partials = partials;
  p.flips = 0;
  p.Ho = a->Ho; p.Wo = a->Wo;
  for (int i = 0; i < a->nclip; ++i) {
    const flk_prep_clip& s = a->clips[i];
    PrepTrainClipDev& d = p.clip[i];
    d.src = s.src; d.pitch_t = s.pitch_t; d.pitch_h = (int)s.pitch_h;
    d.T = s.T; d.Hs = s.Hs; d.Ws = s.Ws;
    d.step_h = s.step_h; d.step_w = s.step_w;
    if (boxes) {
      d.i = boxes[i].i; d.j = boxes[i].j; d.h = boxes[i].h; d.w = boxes[i].w;
      if (boxes[i].flip) p.flips |= 1ull << i;
    } else {
      d.i = s.crop_i; d.j = s.crop_j; d.h = a->Ho; d.w = a->Wo;
    }
  }
  const dim3 grid((unsigned)((a->Ho + kPrepGradRows - 1) / kPrepGradRows), (unsigned)T_out, (unsigned)a->nclip);
  if (dtype == FLK_BF16) FLK_LAUNCH_KERNEL(clip_prepare_grad_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
  else FLK_LAUNCH_KERNEL(clip_prepare_grad_kernel<float>, grid, dim3(256), 0, stream, p);
  const int n3 = a->nclip * T_out * 3;
  FLK_LAUNCH_KERNEL(clip_prepare_grad_finish, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, stream, (const float*)partials, scale, n3, a->Ho,
                    gdelta);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The transpose of the resampling on images (flk_clip_prepare_grad_image): the gradient with respect to every SOURCE pixel.  The
// resampling is separable, out = A_h V A_w^T, A = S2 S1 per axis; the host (videoresnet_spec.prepare_adjoint_tables) builds both
// composite matrices per clip from the forward's own indices and lambdas and stores them by source index as (first_out, count, w[K])
// -- the outputs that read one source index are a contiguous range.
//   g_src[k][t][y][x][c] = sum over a, b of wh[y][a] * ww[x][b] * g(first_h[y] + a, first_w[x] + b, c)
// Order (fixed; no atomics; independent of the grid and of the other clips): b inner, a outer, both ascending from +0 -- a row sum is
// the chain fma(ww[b], g, .), the pixel the chain fma(wh[a], row, .).  A source pixel no output reads gets +0.
// Layout: workgroup = (256 consecutive pixels of one source row, frame, clip); a thread owns one pixel, its three channels.  The
// row's table entry is uniform over the workgroup; the ranges are clamped into the output image before they address g.
namespace {

struct PrepGradImageClipDev {  // 48 bytes
  float* dst;
  long long pitch_t, pitch_h;  // floats
  int Hs, Ws;
  long long tab_h, tab_w;      // words
};
struct PrepGradImageLaunch {
  const int* tables;
  const void* gx;              // device [nclip][T_out][Ho/2][Wo/2][16], fp32 or bf16
  int Ho, Wo, K, pad_;
  PrepGradImageClipDev clip[FLK_PREP_MAX_CLIPS];
};
static_assert(sizeof(PrepGradImageLaunch) <= 4096, "the launch descriptor must fit the kernel-argument segment");

template <typename TI>
__global__ __launch_bounds__(256) void clip_prepare_grad_image_kernel(const PrepGradImageLaunch p) {
  const PrepGradImageClipDev& c = p.clip[blockIdx.z];
  const int nxb = (c.Ws + 255) >> 8;
  const int y = blockIdx.x / nxb, x = (int)(blockIdx.x - y * nxb) * 256 + (int)threadIdx.x;
  if (y >= c.Hs || x >= c.Ws) return;                     // a clip smaller than the largest of the launch
  const int t = blockIdx.y, E = 2 + p.K;
  const size_t kt = (size_t)blockIdx.z * gridDim.y + t;
  const int* eh = p.tables + c.tab_h + (long long)y * E;
  const int* ew = p.tables + c.tab_w + (long long)x * E;
  const int oh0 = min(max(eh[0], 0), p.Ho), nh = min(max(eh[1], 0), min(p.K, p.Ho - oh0));
  const int ow0 = min(max(ew[0], 0), p.Wo), nw = min(max(ew[1], 0), min(p.K, p.Wo - ow0));
  float acc[3] = {0.f, 0.f, 0.f};
  for (int a = 0; a < nh; ++a) {
    const int oh = oh0 + a;
    float row[3] = {0.f, 0.f, 0.f};
    for (int b = 0; b < nw; ++b) {
      const int ow = ow0 + b;
      const float w = __int_as_float(ew[2 + b]);
      const size_t gi = (((kt * (p.Ho >> 1) + (oh >> 1)) * (p.Wo >> 1) + (ow >> 1)) << 4) + ((oh & 1) * 2 + (ow & 1)) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) row[ch] = fmaf(w, prep_grad_load<TI>(p.gx, gi + ch), row[ch]);
    }
    const float w = __int_as_float(eh[2 + a]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] = fmaf(w, row[ch], acc[ch]);
  }
  float* o = c.dst + (long long)t * c.pitch_t + (long long)y * c.pitch_h + (long long)x * 3;
  o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
}

}  // namespace

// arguments already validated (api.cpp: flk_clip_prepare_grad_image); everything here up to the launch is host arithmetic
int flk_clip_prepare_grad_image_launch(int nclip, const flk_grad_image_clip* clips, int T_out, int Ho, int Wo, int K, const int32_t* tables,
                                       const void* gx_s2d, int dtype, hipStream_t stream) {
  PrepGradImageLaunch p;
  p.tables = tables; p.gx = gx_s2d; p.Ho = Ho; p.Wo = Wo; p.K = K; p.pad_ = 0;
  long long blocks = 1;
  for (int i = 0; i < nclip; ++i) {
    const flk_grad_image_clip& s = clips[i];
    PrepGradImageClipDev& d = p.clip[i];
    d.dst = s.dst; d.pitch_t = s.pitch_t; d.pitch_h = s.pitch_h; d.Hs = s.Hs; d.Ws = s.Ws; d.tab_h = s.tab_h; d.tab_w = s.tab_w;
    const long long n = (long long)s.Hs * ((s.Ws + 255) / 256);
    if (n > blocks) blocks = n;
  }
  FLK_REQUIRE(blocks <= 0x7fffffffLL, "flk_clip_prepare_grad_image: a frame of more than 2^31 row segments");
  const dim3 grid((unsigned)blocks, (unsigned)T_out, (unsigned)nclip);
  if (dtype == FLK_BF16) FLK_LAUNCH_KERNEL(clip_prepare_grad_image_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
  else FLK_LAUNCH_KERNEL(clip_prepare_grad_image_kernel<float>, grid, dim3(256), 0, stream, p);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
