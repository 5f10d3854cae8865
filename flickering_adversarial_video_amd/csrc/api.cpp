// Error plumbing, version, and host-side packing of convolution weights into MFMA fragment order.
#include <stdarg.h>
#include <string.h>
#include <new>
#include "flk_internal.h"

static thread_local char g_err[1024] = "";
thread_local const char* flk_last_kernel_tag = "";
thread_local hipEvent_t flk_stop_event = nullptr;
thread_local unsigned flk_launch_count = 0;

void flk_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int flk_version(void) { return 100; }
extern "C" const char* flk_last_error(void) { return g_err; }

static inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // keep NaN a NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

int flk_conv_weights_create_impl(const float* w, int kt, int kh, int kw, int cin, int cout,
                                 const float* row_scale, int transpose, int dtype, int nf, int cin_split,
                                 flk_conv_weights** out) {
  FLK_REQUIRE(w && out, "flk_conv_weights_create: null argument");
  FLK_REQUIRE(dtype == FLK_F32 || dtype == FLK_BF16, "flk_conv_weights_create: bad dtype %d", dtype);
  FLK_REQUIRE(nf == 2 || nf == 4 || nf == 8 || (nf == 6 && dtype == FLK_BF16), "flk_conv_weights_create: nf must be 2, 4, 8 (or 6 in bf16: 96-channel tiles) (got %d)", nf);
  FLK_REQUIRE(kt > 0 && kh > 0 && kw > 0 && cin > 0 && cout > 0, "flk_conv_weights_create: bad shape");
  const int ocin = transpose ? cout : cin;    // operator input channels (GEMM K per tap)
  const int ocout = transpose ? cin : cout;   // operator output channels
  const int epl = dtype == FLK_BF16 ? 8 : 4, slabc = 4 * epl;
  const int ntaps = kt * kh * kw;
  FLK_REQUIRE(cin_split >= 0 && cin_split < ocin && cin_split % 8 == 0 && !(cin_split && transpose),
              "flk_conv_weights_create: bad cin_split %d", cin_split);
  const int nslab1 = cin_split ? (cin_split + slabc - 1) / slabc : 0;
  const int nslab = cin_split ? nslab1 + (ocin - cin_split + slabc - 1) / slabc : (ocin + slabc - 1) / slabc;
  const int cout_frags = (ocout + 16 * nf - 1) / (16 * nf) * nf;
  const size_t nelem = (size_t)nslab * ntaps * cout_frags * 64 * epl;
  const size_t bytes = nelem * (dtype == FLK_BF16 ? 2 : 4);
  std::vector<char> host(bytes);
  uint16_t* hb = (uint16_t*)host.data();
  float* hf = (float*)host.data();
  size_t o = 0;
  for (int s = 0; s < nslab; ++s)
    for (int tap = 0; tap < ntaps; ++tap) {
      const int src_tap = transpose ? ntaps - 1 - tap : tap;   // flipping all three axes = reversing the tap index
      for (int F = 0; F < cout_frags; ++F) {
        const int ntile = F / nf, f = F % nf;
        for (int lane = 0; lane < 64; ++lane) {
          const int q = lane >> 4, m = lane & 15;
          // channel owned by accumulator row m = 4q + r of fragment f.  16-byte store group G = f / (epl/4) of lane group q
          // covers channels [G*4*epl + q*epl, +epl): in ONE store instruction the four lane groups q write four consecutive
          // 16-byte pieces (64 contiguous bytes per position).
          const int fpg = epl / 4, G = f / fpg;
          const int co = ntile * 16 * nf + G * 4 * epl + (m >> 2) * epl + (f % fpg) * 4 + (m & 3);
          for (int j = 0; j < epl; ++j, ++o) {
            int ci = s * slabc + q * epl + j;          // position in the (segment-padded) K order -> channel
            bool civalid = ci < ocin;
            if (cin_split) {
              if (s < nslab1) civalid = ci < cin_split;
              else { ci = cin_split + (s - nslab1) * slabc + q * epl + j; civalid = ci < ocin; }
            }
            float v = 0.f;
            if (co < ocout && civalid) {
              // original array is [tap][cin][cout]
              v = transpose ? w[((size_t)src_tap * cin + co) * cout + ci] : w[((size_t)src_tap * cin + ci) * cout + co];
              if (row_scale) v *= row_scale[ci];
            }
            if (dtype == FLK_BF16) hb[o] = f32_to_bf16_rne(v); else hf[o] = v;
          }
        }
      }
    }
  flk_conv_weights* cw = new (std::nothrow) flk_conv_weights();
  if (!cw) { flk_set_error("flk_conv_weights_create: out of host memory"); return FLK_ENOMEM; }
  cw->kt = kt; cw->kh = kh; cw->kw = kw; cw->cin = ocin; cw->cout = ocout;
  cw->dtype = dtype; cw->nf = nf; cw->nslab = nslab; cw->ntaps = ntaps; cw->cout_frags = cout_frags;
  cw->bytes = bytes; cw->cin_split = cin_split; cw->nslab1 = cin_split ? nslab1 : nslab;
  hipError_t e = hipMalloc(&cw->dev, bytes);
  if (e != hipSuccess) { delete cw; flk_set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return FLK_ENOMEM; }
  e = hipMemcpy(cw->dev, host.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(cw->dev); delete cw; flk_set_error("hipMemcpy: %s", hipGetErrorString(e)); return FLK_EHIP; }
  *out = cw;
  return FLK_OK;
}

extern "C" int flk_conv_weights_create(const float* w, int kt, int kh, int kw, int cin, int cout,
                                       const float* row_scale, int transpose, int dtype, int nf,
                                       flk_conv_weights** out) {
  return flk_conv_weights_create_impl(w, kt, kh, kw, cin, cout, row_scale, transpose, dtype, nf, 0, out);
}

extern "C" int flk_conv_weights_create_split(const float* w, int kt, int kh, int kw, int cin, int cout,
                                             const float* row_scale, int cin_split, int dtype, int nf,
                                             flk_conv_weights** out) {
  return flk_conv_weights_create_impl(w, kt, kh, kw, cin, cout, row_scale, 0, dtype, nf, cin_split, out);
}

// Folded 7x7x7/2 stem (fold_t = 3 layout, include/flicker_hip.h): a 4x4x4 convolution over 32 channels = 4 chunks of 8,
// chunk = (qt,qh).  Tap index 3 of an axis only exists for parity 0 (kernel index 2*3+1 = 7 is outside the 7-tap
// window), so for taps with dt == 3 the chunks qt = 1 are zero, for dh == 3 the chunks qh = 1.  The K steps of mode 4
// (conv_igemm.hip) are assembled from the non-zero chunks only, 49 steps instead of 64:
//   class 0 (dt<3, dh<3): one tap, chunks 0..3              class 1 (dt=3): taps (dw, dw+1) x chunks {0,1}
//   class 2 (dh=3): taps (dw, dw+1) x chunks {0,2}           class 3 (dt=3, dh=3): taps dw..dw+3 x chunk 0
// in the order dt, dh, dw.  They are packed as a 49-"tap" convolution over 32 channels whose channel (q*8 + j) of
// step s is (tap, chunk)(s, q) x element j.
extern "C" int flk_conv_weights_create_s2d_stem(const float* w, int cout, int dtype, int nf, flk_conv_weights** out) {
  FLK_REQUIRE(w && out && cout > 0, "flk_conv_weights_create_s2d_stem: bad argument");
  if (dtype != FLK_BF16) return flk_conv_weights_create_impl(w, 4, 4, 4, 32, cout, nullptr, 0, dtype, nf, 0, out);
  auto at = [&](int dt, int dh, int dw, int ch, int co) { return w[((((size_t)dt * 4 + dh) * 4 + dw) * 32 + ch) * cout + co]; };
  for (int dt = 0; dt < 4; ++dt) for (int dh = 0; dh < 4; ++dh) for (int dw = 0; dw < 4; ++dw)
    for (int ch = 0; ch < 32; ++ch) {
      const int qt = ch >> 4, qh = (ch >> 3) & 1;
      if (!((dt == 3 && qt == 1) || (dh == 3 && qh == 1))) continue;
      for (int co = 0; co < cout; ++co)
        FLK_REQUIRE(at(dt, dh, dw, ch, co) == 0.f, "flk_conv_weights_create_s2d_stem: weight (tap %d,%d,%d, channel %d) must be zero", dt, dh, dw, ch);
    }
  std::vector<float> v;
  v.reserve((size_t)49 * 32 * cout);
  for (int dt = 0; dt < 4; ++dt)
    for (int dh = 0; dh < 4; ++dh) {
      const int cls = (dt == 3) + 2 * (dh == 3), wstride = cls == 0 ? 1 : cls == 3 ? 4 : 2;
      for (int dw = 0; dw < 4; dw += wstride)
        for (int q = 0; q < 4; ++q) {
          const int chunk = cls == 0 ? q : cls == 1 ? (q & 1) : cls == 2 ? (q & 1) * 2 : 0;
          const int woff = cls == 0 ? 0 : cls == 3 ? q : (q >> 1);
          for (int j = 0; j < 8; ++j)
            for (int co = 0; co < cout; ++co) v.push_back(at(dt, dh, dw + woff, chunk * 8 + j, co));
        }
    }
  FLK_REQUIRE(v.size() == (size_t)49 * 32 * cout, "flk_conv_weights_create_s2d_stem: internal step count");
  int rc = flk_conv_weights_create_impl(v.data(), 49, 1, 1, 32, cout, nullptr, 0, dtype, nf, 0, out);
  if (rc) return rc;
  (*out)->stem4 = 1;
  (*out)->kt = (*out)->kh = (*out)->kw = 4;      // the operator it implements; ntaps stays 49 (K steps per slab)
  return FLK_OK;
}

extern "C" int flk_conv_weights_destroy(flk_conv_weights* w) {
  if (!w) return FLK_OK;
  if (w->dev) (void)hipFree(w->dev);
  delete w;
  return FLK_OK;
}

// Clip preparation (csrc/prepare.hip): every argument is checked here, on the host, before anything touches the device.
int flk_clip_prepare_launch(const flk_prepare_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, float* out,
                            hipStream_t stream);
int flk_clip_prepare_train_launch(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, const uint8_t* tone,
                                  float* out, hipStream_t stream);

// the checks the entries share; `boxes`: the training transform's crop boxes, which take the place of the centre-crop window;
// `T_out`: frames per clip written by the sampled entry (0: the clip's own T)
static int check_prepare_args(const char* fn, const flk_prepare_args* a, const float* out, const flk_prep_box* boxes, int T_out = 0) {
  FLK_REQUIRE(a && out, "%s: null argument", fn);
  FLK_REQUIRE(a->clips, "%s: null clip list", fn);
  FLK_REQUIRE(a->nclip >= 1 && a->nclip <= FLK_PREP_MAX_CLIPS, "%s: nclip %d outside 1..%d", fn, a->nclip, FLK_PREP_MAX_CLIPS);
  FLK_REQUIRE(a->Ho > 0 && a->Wo > 0, "%s: output size %d x %d", fn, a->Ho, a->Wo);
  for (int k = 0; k < 3; ++k) {
    FLK_REQUIRE(a->std[k] > 0.f && a->std[k] <= 3.4e38f, "%s: std[%d] must be positive", fn, k);
    FLK_REQUIRE(a->mean[k] >= -3.4e38f && a->mean[k] <= 3.4e38f, "%s: mean[%d] is not finite", fn, k);
  }
  FLK_REQUIRE(a->out_clip_offset >= 0, "%s: negative out_clip_offset", fn);
  for (int i = 0; i < a->nclip; ++i) {
    const flk_prep_clip& c = a->clips[i];
    FLK_REQUIRE(c.src, "%s: clip %d: null source", fn, i);
    FLK_REQUIRE(c.T > 0 && c.Hs > 0 && c.Ws > 0, "%s: clip %d: source size %d x %d x %d", fn, i, c.T, c.Hs, c.Ws);
    FLK_REQUIRE(c.pitch_h >= (int64_t)c.Ws * 3 && c.pitch_h <= 0x7fffffff && c.pitch_t > 0,
                "%s: clip %d: pitches (frame %lld, row %lld bytes) must be positive, a row at least 3 * Ws", fn, i, (long long)c.pitch_t, (long long)c.pitch_h);
    FLK_REQUIRE(c.step_h > 0.f && c.step_w > 0.f && c.step_h <= 3.4e38f && c.step_w <= 3.4e38f, "%s: clip %d: steps must be positive and finite", fn, i);
    FLK_REQUIRE(c.Hr > 0 && c.Wr > 0, "%s: clip %d: resized size %d x %d", fn, i, c.Hr, c.Wr);
    if (boxes) {
      const flk_prep_box& b = boxes[i];
      FLK_REQUIRE(b.h >= 1 && b.w >= 1, "%s: clip %d: box size %d x %d", fn, i, b.h, b.w);
      FLK_REQUIRE(b.i >= 0 && b.j >= 0 && (int64_t)b.i + b.h <= c.Hr && (int64_t)b.j + b.w <= c.Wr,
                  "%s: clip %d: box (%d,%d)+%dx%d outside the resized image %d x %d", fn, i, b.i, b.j, b.h, b.w, c.Hr, c.Wr);
      FLK_REQUIRE(b.flip == 0 || b.flip == 1, "%s: clip %d: flip %d is not 0 / 1", fn, i, b.flip);
    } else {
      FLK_REQUIRE(c.crop_i >= 0 && c.crop_j >= 0 && (int64_t)c.crop_i + a->Ho <= c.Hr && (int64_t)c.crop_j + a->Wo <= c.Wr,
                  "%s: clip %d: crop window (%d,%d)+%dx%d outside the resized image %d x %d", fn, i, c.crop_i, c.crop_j, a->Ho, a->Wo, c.Hr, c.Wr);
    }
    FLK_REQUIRE(a->out_clip_stride >= (int64_t)(T_out ? T_out : c.T) * a->Ho * a->Wo * 3, "%s: clip %d: out_clip_stride %lld smaller than the clip", fn, i, (long long)a->out_clip_stride);
  }
  return FLK_OK;
}

extern "C" int flk_clip_prepare(const flk_prepare_args* a, float* out, void* stream) {
  if (int rc = check_prepare_args("flk_clip_prepare", a, out, nullptr)) return rc;
  return flk_clip_prepare_launch(a, nullptr, 0, nullptr, out, (hipStream_t)stream);
}

extern "C" int flk_clip_prepare_train(const flk_prepare_args* a, const flk_prep_box* boxes, float* out, void* stream) {
  FLK_REQUIRE(boxes, "flk_clip_prepare_train: null box list");
  if (int rc = check_prepare_args("flk_clip_prepare_train", a, out, boxes)) return rc;
  return flk_clip_prepare_train_launch(a, boxes, nullptr, 0, nullptr, out, (hipStream_t)stream);
}

extern "C" int flk_clip_prepare_sampled(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, float* out,
                                        void* stream) {
  FLK_REQUIRE(frame_idx, "flk_clip_prepare_sampled: null frame_idx");
  FLK_REQUIRE(T_out >= 1 && T_out <= 65535, "flk_clip_prepare_sampled: T_out %d outside 1..65535", T_out);
  if (int rc = check_prepare_args("flk_clip_prepare_sampled", a, out, boxes, T_out)) return rc;
  if (boxes) return flk_clip_prepare_train_launch(a, boxes, frame_idx, T_out, nullptr, out, (hipStream_t)stream);
  return flk_clip_prepare_launch(a, frame_idx, T_out, nullptr, out, (hipStream_t)stream);
}

extern "C" int flk_clip_prepare_toned(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, const uint8_t* tone,
                                      float* out, void* stream) {
  FLK_REQUIRE(frame_idx, "flk_clip_prepare_toned: null frame_idx");
  FLK_REQUIRE(tone, "flk_clip_prepare_toned: null tone");
  FLK_REQUIRE(T_out >= 1 && T_out <= 65535, "flk_clip_prepare_toned: T_out %d outside 1..65535", T_out);
  if (int rc = check_prepare_args("flk_clip_prepare_toned", a, out, boxes, T_out)) return rc;
  if (boxes) return flk_clip_prepare_train_launch(a, boxes, frame_idx, T_out, tone, out, (hipStream_t)stream);
  return flk_clip_prepare_launch(a, frame_idx, T_out, tone, out, (hipStream_t)stream);
}

// The codec round trip (csrc/codec.hip): every argument is checked here, on the host, before anything touches the device.
void flk_codec_tables_host(int quality, int32_t* qluma, int32_t* qchroma);
int flk_codec_roundtrip_launch(const flk_codec_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, int32_t* stats,
                               hipStream_t stream);

extern "C" int flk_codec_tables(int quality, int32_t* qluma, int32_t* qchroma) {
  FLK_REQUIRE(qluma && qchroma, "flk_codec_tables: null table");
  FLK_REQUIRE(quality >= 1 && quality <= 100, "flk_codec_tables: quality %d outside 1..100", quality);
  flk_codec_tables_host(quality, qluma, qchroma);
  return FLK_OK;
}

// what both codec entries check of the views, the quality and the subsampling.  have_idx: the launch names its own source frames, so
// T_out is not held against the clips' T.  stats_pixels: the largest padded frame stats are taken on (0: no stats asked for)
// need_dst: the entry writes the clips' dst views (flk_codec_grad reads the sources only and leaves dst unused)
static int check_codec_args(const char* fn, const flk_codec_args* a, bool have_idx, int T_out, int64_t stats_pixels, bool need_dst = true) {
  FLK_REQUIRE(a, "%s: null argument", fn);
  FLK_REQUIRE(a->clips, "%s: null clip list", fn);
  FLK_REQUIRE(a->nclip >= 1 && a->nclip <= FLK_PREP_MAX_CLIPS, "%s: nclip %d outside 1..%d", fn, a->nclip, FLK_PREP_MAX_CLIPS);
  FLK_REQUIRE(a->quality >= 1 && a->quality <= 100, "%s: quality %d outside 1..100", fn, a->quality);
  FLK_REQUIRE(a->subsampling == FLK_CODEC_444 || a->subsampling == FLK_CODEC_420, "%s: subsampling %d is neither 444 nor 420", fn, a->subsampling);
  FLK_REQUIRE(T_out >= 1 && T_out <= 65535, "%s: T_out %d outside 1..65535", fn, T_out);
  const int M = a->subsampling == FLK_CODEC_420 ? 16 : 8;
  for (int i = 0; i < a->nclip; ++i) {
    const flk_codec_clip& c = a->clips[i];
    FLK_REQUIRE(c.src && (c.dst || !need_dst), "%s: clip %d: null source or destination", fn, i);
    FLK_REQUIRE(c.T > 0 && c.Hs > 0 && c.Ws > 0, "%s: clip %d: source size %d x %d x %d", fn, i, c.T, c.Hs, c.Ws);
    FLK_REQUIRE(c.Hs <= 0x3fffffff && c.Ws <= 0x1fffffff, "%s: clip %d: frame size %d x %d", fn, i, c.Hs, c.Ws);
    FLK_REQUIRE(c.pitch_h >= (int64_t)c.Ws * 3 && c.pitch_h <= 0x7fffffff && c.pitch_t > 0,
                "%s: clip %d: source pitches (frame %lld, row %lld bytes) must be positive, a row at least 3 * Ws", fn, i, (long long)c.pitch_t,
                (long long)c.pitch_h);
    FLK_REQUIRE(!need_dst || (c.dst_pitch_h >= (int64_t)c.Ws * 3 && c.dst_pitch_h <= 0x7fffffff && c.dst_pitch_t > 0),
                "%s: clip %d: destination pitches (frame %lld, row %lld bytes) must be positive, a row at least 3 * Ws", fn, i,
                (long long)c.dst_pitch_t, (long long)c.dst_pitch_h);
    FLK_REQUIRE(!need_dst || (const uint8_t*)c.dst != c.src, "%s: clip %d: the destination is the source (an MCU reads pixels other workgroups write)", fn, i);
    FLK_REQUIRE(have_idx || T_out <= c.T, "%s: clip %d: T_out %d above its %d frames (no frame_idx)", fn, i, T_out, c.T);
    if (stats_pixels) {
      const int64_t Hp = ((int64_t)c.Hs + M - 1) / M * M, Wp = ((int64_t)c.Ws + M - 1) / M * M;
      FLK_REQUIRE(Hp * Wp <= stats_pixels, "%s: clip %d: stats on a frame of %lld padded pixels (more than %lld)", fn, i, (long long)(Hp * Wp),
                  (long long)stats_pixels);
    }
  }
  return FLK_OK;
}

extern "C" int flk_codec_roundtrip_u8(const flk_codec_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, int32_t* stats,
                                      void* stream) {
  if (int rc = check_codec_args("flk_codec_roundtrip_u8", a, frame_idx != nullptr, T_out, stats ? 5000000 : 0)) return rc;
  return flk_codec_roundtrip_launch(a, frame_idx, T_out, tone, stats, (hipStream_t)stream);
}

// Inter-frame prediction (csrc/codec.hip): closed GOPs over per-clip spans given as host values
int flk_codec_inter_step_host(int quality);
int flk_codec_roundtrip_gop_launch(const flk_codec_args* a, int gop, const int32_t* first, const int32_t* count, int T_max,
                                   const uint8_t* tone, int32_t* stats, hipStream_t stream);

extern "C" int flk_codec_inter_step(int quality, int32_t* qp) {
  FLK_REQUIRE(qp, "flk_codec_inter_step: null result");
  FLK_REQUIRE(quality >= 1 && quality <= 100, "flk_codec_inter_step: quality %d outside 1..100", quality);
  *qp = flk_codec_inter_step_host(quality);
  return FLK_OK;
}

// what the two entries with spans check of them, the views already checked: clip i's span is frames first[i] .. first[i] + count[i] - 1
static int check_codec_spans(const char* fn, const flk_codec_args* a, int gop, const int32_t* first, const int32_t* count, int T_max) {
  for (int i = 0; i < a->nclip; ++i) {
    FLK_REQUIRE(first[i] >= 0 && first[i] % gop == 0, "%s: clip %d: first %d is not a non-negative multiple of gop %d (a span starts on an intra frame)",
                fn, i, first[i], gop);
    FLK_REQUIRE(count[i] >= 1 && count[i] <= T_max, "%s: clip %d: count %d outside 1..T_max %d", fn, i, count[i], T_max);
    FLK_REQUIRE((int64_t)first[i] + count[i] <= a->clips[i].T, "%s: clip %d: span %d + %d beyond its %d frames", fn, i, first[i], count[i],
                a->clips[i].T);
  }
  return FLK_OK;
}

extern "C" int flk_codec_roundtrip_gop_u8(const flk_codec_args* a, int gop, const int32_t* first, const int32_t* count, int T_max,
                                          const uint8_t* tone, int32_t* stats, void* stream) {
  const char* fn = "flk_codec_roundtrip_gop_u8";
  FLK_REQUIRE(first && count, "%s: null first or count", fn);
  FLK_REQUIRE(gop >= 1 && gop <= 65535, "%s: gop %d outside 1..65535", fn, gop);
  // the spans are held against the clips below: to the shared checks the launch has its own source frames (as with a frame_idx)
  // (a P-frame's magnitudes reach 766 per padded pixel, twice an intra frame's: half the frame for the same int32)
  if (int rc = check_codec_args(fn, a, true, T_max, stats ? 2500000 : 0)) return rc;
  if (int rc = check_codec_spans(fn, a, gop, first, count, T_max)) return rc;
  return flk_codec_roundtrip_gop_launch(a, gop, first, count, T_max, tone, stats, (hipStream_t)stream);
}

// Motion-compensated P-frames (csrc/codec.hip): the GOP entry's contract plus the search range, the vectors and the workspace
long long flk_codec_mc_scratch_host(const flk_codec_args* a, int gop, const int32_t* count);
int flk_codec_roundtrip_mc_launch(const flk_codec_args* a, int gop, int search, const int32_t* first, const int32_t* count, int T_max,
                                  const uint8_t* tone, int32_t* stats, int8_t* mv, int mv_stride, void* scratch, hipStream_t stream);

extern "C" int64_t flk_codec_mc_scratch_bytes(const flk_codec_args* a, int gop, const int32_t* count) {
  if (!a || a->nclip > FLK_PREP_MAX_CLIPS) return 0;
  return flk_codec_mc_scratch_host(a, gop, count);
}

extern "C" int flk_codec_roundtrip_mc_u8(const flk_codec_args* a, int gop, int search, const int32_t* first, const int32_t* count, int T_max,
                                         const uint8_t* tone, int32_t* stats, int8_t* mv, int mv_stride, void* scratch, int64_t scratch_bytes,
                                         void* stream) {
  const char* fn = "flk_codec_roundtrip_mc_u8";
  FLK_REQUIRE(first && count, "%s: null first or count", fn);
  FLK_REQUIRE(gop >= 1 && gop <= 65535, "%s: gop %d outside 1..65535", fn, gop);
  FLK_REQUIRE(search >= 0 && search <= 15, "%s: search %d outside 0..15", fn, search);
  if (int rc = check_codec_args(fn, a, true, T_max, stats ? 2500000 : 0)) return rc;
  if (int rc = check_codec_spans(fn, a, gop, first, count, T_max)) return rc;
  const int M = a->subsampling == FLK_CODEC_420 ? 16 : 8;
  for (int i = 0; mv && i < a->nclip; ++i) {
    const int64_t Hp = ((int64_t)a->clips[i].Hs + M - 1) / M * M, Wp = ((int64_t)a->clips[i].Ws + M - 1) / M * M;
    const int64_t mbs = ((Hp + 15) / 16) * ((Wp + 15) / 16);
    FLK_REQUIRE(mv_stride >= mbs, "%s: clip %d: mv_stride %d below its %lld macroblocks", fn, i, mv_stride, (long long)mbs);
  }
  const int64_t need = flk_codec_mc_scratch_host(a, gop, count);
  FLK_REQUIRE(need > 0, "%s: the workspace of these clips cannot be sized (a plane set above 2^36 bytes)", fn);
  FLK_REQUIRE(scratch && ((uintptr_t)scratch & 15) == 0, "%s: null scratch, or one not 16-byte aligned", fn);
  FLK_REQUIRE(scratch_bytes >= need, "%s: scratch of %lld bytes, flk_codec_mc_scratch_bytes asks for %lld", fn, (long long)scratch_bytes,
              (long long)need);
  return flk_codec_roundtrip_mc_launch(a, gop, search, first, count, T_max, tone, stats, mv, mv_stride, scratch, (hipStream_t)stream);
}

// The codec's backward (csrc/codec.hip): flk_codec_roundtrip_u8's contract on the sources, the gradient images packed clip after clip
long long flk_codec_grad_tiles_host(const flk_codec_args* a);
int flk_codec_grad_launch(const flk_codec_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, int mode, const float* g_out,
                          const float* slope, const float* scale, float* gdelta, float* g_in, float* partials, hipStream_t stream);

extern "C" int64_t flk_codec_grad_scratch_bytes(const flk_codec_args* a, int T_out) {
  if (!a || a->nclip > FLK_PREP_MAX_CLIPS || T_out < 1 || T_out > 65535) return 0;
  return (int64_t)flk_codec_grad_tiles_host(a) * a->nclip * T_out * 3 * (int64_t)sizeof(float);
}

extern "C" int flk_codec_grad(const flk_codec_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, int mode, const float* g_out,
                              const float* slope, const float* scale, float* gdelta, float* g_in, float* partials, void* stream) {
  const char* fn = "flk_codec_grad";
  FLK_REQUIRE(mode == FLK_CODEC_GRAD_STE || mode == FLK_CODEC_GRAD_CUBIC, "%s: mode %d is neither FLK_CODEC_GRAD_STE nor FLK_CODEC_GRAD_CUBIC", fn, mode);
  FLK_REQUIRE(slope && scale && gdelta, "%s: null slope, scale or gdelta", fn);
  FLK_REQUIRE(g_out && partials, "%s: null g_out or partials", fn);
  FLK_REQUIRE(g_in != g_out, "%s: g_in is g_out (a block reads gradients other workgroups' pixels wrote)", fn);
  if (int rc = check_codec_args(fn, a, frame_idx != nullptr, T_out, 0, false)) return rc;
  return flk_codec_grad_launch(a, frame_idx, T_out, tone, mode, g_out, slope, scale, gdelta, g_in, partials, (hipStream_t)stream);
}

// The transpose of the resampling on images (csrc/prepare.hip)
int flk_clip_prepare_grad_image_launch(int nclip, const flk_grad_image_clip* clips, int T_out, int Ho, int Wo, int K, const int32_t* tables,
                                       const void* gx_s2d, int dtype, hipStream_t stream);

extern "C" int flk_clip_prepare_grad_image(int nclip, const flk_grad_image_clip* clips, int T_out, int Ho, int Wo, int K, const int32_t* tables,
                                           int64_t table_words, const void* gx_s2d, int dtype, void* stream) {
  static const char* who = "flk_clip_prepare_grad_image";
  FLK_REQUIRE(clips && tables && gx_s2d, "%s: null clips, tables or gx_s2d", who);
  FLK_REQUIRE(nclip >= 1 && nclip <= FLK_PREP_MAX_CLIPS, "%s: nclip %d outside 1..%d", who, nclip, FLK_PREP_MAX_CLIPS);
  FLK_REQUIRE(T_out >= 1 && T_out <= 65535, "%s: T_out %d outside 1..65535", who, T_out);
  FLK_REQUIRE(Ho > 0 && Wo > 0 && Ho % 2 == 0 && Wo % 2 == 0, "%s: Ho and Wo must be positive and even (the folded gradient layout), got %d x %d", who, Ho, Wo);
  FLK_REQUIRE(K >= 1 && K <= Ho + Wo, "%s: K %d outside 1..Ho + Wo", who, K);
  FLK_REQUIRE(((size_t)gx_s2d & 15) == 0, "%s: gx_s2d must be 16-byte aligned (got %p)", who, gx_s2d);
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "%s: bad dtype", who);
  for (int i = 0; i < nclip; ++i) {
    const flk_grad_image_clip& c = clips[i];
    FLK_REQUIRE(c.dst, "%s: clip %d: null destination", who, i);
    FLK_REQUIRE(c.Hs > 0 && c.Ws > 0 && c.Ws <= 0x1fffffff, "%s: clip %d: source size %d x %d", who, i, c.Hs, c.Ws);
    FLK_REQUIRE(c.pitch_h >= (int64_t)c.Ws * 3 && c.pitch_t >= c.pitch_h * (c.Hs - 1) + (int64_t)c.Ws * 3,
                "%s: clip %d: pitches (frame %lld, row %lld floats) must hold a row of 3 * Ws and a frame of Hs rows", who, i, (long long)c.pitch_t,
                (long long)c.pitch_h);
    FLK_REQUIRE(c.tab_h >= 0 && c.tab_w >= 0 && c.tab_h + (int64_t)c.Hs * (2 + K) <= table_words && c.tab_w + (int64_t)c.Ws * (2 + K) <= table_words,
                "%s: clip %d: its tables (rows at word %lld, columns at %lld, %d words an entry) leave the %lld words given", who, i,
                (long long)c.tab_h, (long long)c.tab_w, 2 + K, (long long)table_words);
  }
  return flk_clip_prepare_grad_image_launch(nclip, clips, T_out, Ho, Wo, K, tables, gx_s2d, dtype, (hipStream_t)stream);
}

// The gradient of a toned preparation (csrc/prepare.hip) and the slope tables it resamples (csrc/attack.hip, csrc/illum.hip)
int flk_clip_prepare_grad_launch(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, const float* slope,
                                 const float* scale, const void* gx_s2d, int dtype, float* gdelta, float* partials, hipStream_t stream);
int flk_tone_slopes_launch(const flk_apply_args* a, float* slope, float* scale, hipStream_t stream);
int flk_illum_tone_slopes_launch(const flk_apply_args* a, const flk_illum_args* m, float* slope, float* scale, hipStream_t stream);

extern "C" int64_t flk_clip_prepare_grad_scratch_bytes(int nclip, int T_out, int Ho) {
  if (nclip <= 0 || T_out <= 0 || Ho <= 0) return 0;
  return (int64_t)nclip * T_out * Ho * 3 * (int64_t)sizeof(float);
}

extern "C" int flk_clip_prepare_grad(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, const float* slope,
                                     const float* scale, const void* gx_s2d, int dtype, float* gdelta, float* partials, void* stream) {
  static const char* who = "flk_clip_prepare_grad";
  FLK_REQUIRE(frame_idx, "%s: null frame_idx", who);
  FLK_REQUIRE(slope && scale, "%s: null slope or scale", who);
  FLK_REQUIRE(gx_s2d && gdelta && partials, "%s: null gx_s2d, gdelta or partials", who);
  FLK_REQUIRE(((size_t)gx_s2d & 15) == 0, "%s: gx_s2d must be 16-byte aligned (got %p)", who, gx_s2d);
  FLK_REQUIRE(dtype == FLK_BF16 || dtype == FLK_F32, "%s: bad dtype", who);
  FLK_REQUIRE(T_out >= 1 && T_out <= 65535, "%s: T_out %d outside 1..65535", who, T_out);
  if (int rc = check_prepare_args(who, a, gdelta, boxes, T_out)) return rc;
  FLK_REQUIRE(a->Ho % 2 == 0 && a->Wo % 2 == 0, "%s: Ho and Wo must be even (the folded gradient layout), got %d x %d", who, a->Ho, a->Wo);
  return flk_clip_prepare_grad_launch(a, boxes, frame_idx, T_out, slope, scale, gx_s2d, dtype, gdelta, partials, (hipStream_t)stream);
}

extern "C" int flk_flicker_tone_slopes(const flk_apply_args* a, const flk_illum_args* m, float* slope, float* scale, void* stream) {
  static const char* who = "flk_flicker_tone_slopes";
  FLK_REQUIRE(a, "%s: null argument structure", who);
  FLK_REQUIRE(slope && scale, "%s: null slope or scale", who);
  FLK_REQUIRE(a->x && a->delta, "%s: null x (the ramp clip) or delta", who);
  FLK_REQUIRE(a->x_is_u8 && a->x_lut, "%s: a uint8 clip with its decode table (x_is_u8 = 1, x_lut non-null)", who);
  FLK_REQUIRE(a->B > 0 && a->T > 0, "%s: B and T must be positive (got %d,%d)", who, a->B, a->T);
  FLK_REQUIRE(!a->delta_per_line, "%s: delta_per_line is not supported (a per-line flicker is not a per-frame byte map)", who);
  FLK_REQUIRE(!a->delta_dense, "%s: delta_dense is not supported", who);
  FLK_REQUIRE(a->center == 0, "%s: center must be 0", who);
  FLK_REQUIRE(a->delta_per_clip, "%s: delta_per_clip = 1 (delta is the per-clip [B,T,3] of video time)", who);
  FLK_REQUIRE(a->shift_x == 0 && a->shift_p == 0, "%s: no cyclic rolls (shift_x = shift_p = 0)", who);
  if (m) return flk_illum_tone_slopes_launch(a, m, slope, scale, (hipStream_t)stream);
  return flk_tone_slopes_launch(a, slope, scale, (hipStream_t)stream);
}

// 8-bit export of the adversarial clip (csrc/attack.hip): checked here, on the host, before anything touches the device.
int flk_adv_export_u8_launch(const flk_apply_args* a, const flk_export_args* e, uint8_t* out, int32_t* stats, hipStream_t stream);

extern "C" int flk_adv_export_u8(const flk_apply_args* a, const flk_export_args* e, uint8_t* out, int32_t* stats, void* stream) {
  FLK_REQUIRE(a && e, "flk_adv_export_u8: null argument structure");
  FLK_REQUIRE(a->x && a->delta, "flk_adv_export_u8: null clip or delta");
  FLK_REQUIRE(out, "flk_adv_export_u8: null out");
  FLK_REQUIRE(a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0, "flk_adv_export_u8: sizes must be positive (got %d,%d,%d,%d)", a->B, a->T, a->H, a->W);
  FLK_REQUIRE((int64_t)a->H * a->W * 3 <= 0x7fffffff, "flk_adv_export_u8: a frame of %d x %d is too large", a->H, a->W);
  FLK_REQUIRE(a->center == 0, "flk_adv_export_u8: center must be 0 (the frames hold x_adv itself)");
  FLK_REQUIRE(a->lo <= a->hi, "flk_adv_export_u8: lo > hi");
  FLK_REQUIRE(!(a->delta_per_clip && a->delta_dense), "flk_adv_export_u8: delta_per_clip is defined for the flicker perturbation only");
  FLK_REQUIRE(!a->dclip_dev || a->delta_per_clip, "flk_adv_export_u8: dclip_dev (per-clip clamp bounds) needs delta_per_clip");
  FLK_REQUIRE(!(a->delta_per_line && a->delta_dense), "flk_adv_export_u8: delta_per_line (one value per line of a frame) excludes delta_dense");
  FLK_REQUIRE(!a->x_lut || a->x_is_u8, "flk_adv_export_u8: x_lut (per-channel decode table) needs a uint8 clip");
  FLK_REQUIRE(e->levels > 0.f && e->levels <= 3.4e38f, "flk_adv_export_u8: levels must be positive");
  FLK_REQUIRE(e->out_clip_offset >= 0, "flk_adv_export_u8: negative out_clip_offset");
  FLK_REQUIRE(e->out_clip_stride >= (int64_t)a->T * a->H * a->W * 3, "flk_adv_export_u8: out_clip_stride %lld smaller than the clip",
              (long long)e->out_clip_stride);
  FLK_REQUIRE(e->delta_T >= 0, "flk_adv_export_u8: negative delta_T");
  FLK_REQUIRE(e->delta_T == 0 || !(a->delta_dense || a->delta_per_clip), "flk_adv_export_u8: delta_T (a period) is defined for the shared flicker perturbation [delta_T,3] (delta_per_line: [delta_T,H,3]) only");
  FLK_REQUIRE(!stats || (int64_t)a->H * a->W <= 8388607, "flk_adv_export_u8: stats need H * W <= 8388607 (255 * H * W must fit an int32), got %d x %d", a->H, a->W);
  return flk_adv_export_u8_launch(a, e, out, stats, (hipStream_t)stream);
}
