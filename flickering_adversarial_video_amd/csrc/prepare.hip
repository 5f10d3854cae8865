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
#include <math.h>
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
static_assert(sizeof(PrepLaunch) <= 4096, "the launch descriptor must fit the kernel-argument segment");

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

__global__ __launch_bounds__(256) void clip_prepare_kernel(const PrepLaunch p) {
  extern __shared__ unsigned prep_lds[];      // [256] fp32 table u8 / 255 | [2 * rows] segment misalignments | 2 * rows row segments
  const PrepClipDev& c = p.clip[blockIdx.z];
  const int t = blockIdx.y;
  if (t >= c.T) return;
  float* tab = (float*)prep_lds;
  int* mis_of = (int*)(prep_lds + 256);
  unsigned* seg = prep_lds + 256 + 2 * p.rows;
  const uint8_t* segb = (const uint8_t*)seg;
  tab[threadIdx.x] = (float)threadIdx.x / 255.0f;
  const int oh0 = blockIdx.x * p.rows;
  const int nrow = min(p.rows, p.Ho - oh0);
  const int ndw = p.seg_stride >> 2;
  const uint8_t* frame = c.src + (long long)t * c.pitch_t;
  const int nbytes = c.span * 3;
  // ---- stage: slot 2r + s = source row s (0 top, 1 bottom) of output row oh0 + r; columns [x0, x0 + span) ----
  for (int k = threadIdx.x; k < 2 * nrow * ndw; k += 256) {
    const int slot = k / ndw, w = k - slot * ndw;
    int h = min((int)prep_src(c.step_h, c.crop_i + oh0 + (slot >> 1)), c.Hs - 1);
    if (slot & 1) h = min(h + 1, c.Hs - 1);
    const uint8_t* row = frame + (long long)h * c.pitch_h + c.x0 * 3;
    const int mis = (int)((size_t)row & 3);
    if (w == 0) mis_of[slot] = mis;
    // aligned dwords that hold at least one byte of the segment: never beyond the dword of its last byte
    if (4 * w < mis + nbytes) seg[slot * ndw + w] = *(const unsigned*)(row - mis + 4 * w);
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

// arguments already validated (api.cpp: flk_clip_prepare); everything here up to the launch is host arithmetic
int flk_clip_prepare_launch(const flk_prepare_args* a, float* out, hipStream_t stream) {
  PrepLaunch p;
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
  FLK_REQUIRE(max_T <= 65535, "flk_clip_prepare: more than 65535 frames");
  p.out = out + a->out_clip_offset * a->out_clip_stride;
  p.clip_stride = a->out_clip_stride;
  p.Ho = a->Ho; p.Wo = a->Wo; p.rows = rows; p.seg_stride = seg_stride;
  p.vec = ((size_t)p.out % 16 == 0) && a->out_clip_stride % 4 == 0 && (a->Wo * 3) % 4 == 0;
  for (int k = 0; k < 3; ++k) { p.mean[k] = a->mean[k]; p.std_[k] = a->std[k]; }
  const size_t lds = (size_t)(256 + 2 * rows) * 4 + (size_t)2 * rows * seg_stride;
  const dim3 grid((unsigned)((a->Ho + rows - 1) / rows), (unsigned)max_T, (unsigned)a->nclip);
  FLK_LAUNCH_KERNEL(clip_prepare_kernel, grid, dim3(256), lds, stream, p);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
