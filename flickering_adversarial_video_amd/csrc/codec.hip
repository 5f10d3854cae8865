// Lossy intra-frame compression of the delivered video: a JPEG-style round trip (colour transform, chroma subsampling, 8x8 DCT,
// quantisation and back) in ONE kernel, defined in integers only.  The definition is videoresnet_spec.codec_roundtrip_host (DESIGN.md
// 10.8); this file performs the same integer operations, so the two agree bit for bit:
//   tone     (optional) byte -> byte table of the output frame, tone[k][t][v][c]: the 8-bit export of a per-frame flicker
//   colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//            Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16;   Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
//   pad      to whole MCUs (8x8, or 16x16 with 4:2:0) by repeating the last column and row
//   4:2:0    Cb, Cr: (a + b + c + d + 1 + (x & 1)) >> 2 over each 2x2 cell, x the output column
//   DCT      value - 128; the "slow integer" forward transform (13-bit constants; rows, then columns; 8 x the DCT);
//            level = sign * ((|f| + 4 Q) / (8 Q))  (half away from zero);  back: level * Q, columns then rows, + 128, clamp 0..255
//   4:2:0    chroma repeated 2x2
//   colour   R = Y + ((91881 Cr' + 32768) >> 16);  G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16);  B = Y + ((116130 Cb' + 32768) >> 16)
//            (Cb' = Cb - 128, Cr' = Cr - 128), clamp 0..255; crop
// Every intermediate fits an int32 (bounds: DESIGN.md 10.8).  Plain int32 VALU arithmetic, no MFMA: exactness is the contract.
//
// Mapping: workgroup = (tile of kTW columns x TH rows of one output frame of one clip), 192 threads.  TH = 32 (4:4:4) or 64 (4:2:0):
// 192 8x8 blocks per full tile either way, ONE THREAD PER BLOCK -- the 64 values of a block stay in that thread's registers through
// both passes of both transforms, so the transform needs no LDS transposes and no barriers.  The phases, each a helper below that
// the three kernels share (the LDS arrays are the kernel's own and come as pointers; every barrier stands in the kernel):
//   A  stage_rows, load_quant, load_tone: the source row segments under the tile into LDS as aligned dwords (the misalignment of a
//      row kept per row, as clip_prepare_kernel does), the quantisation tables and the frame's tone table
//   B  build_planes: bytes (through the tone) -> Y, Cb, Cr byte planes in LDS, padded by replication, chroma averaged for 4:2:0
//   C  walk_blocks, codec_block: per block forward DCT, quantise, (stats), dequantise, inverse DCT; the reconstructed bytes back into
//      the block's place; stats_to_global
//   D  planes_to_rgb, store_rows: planes -> RGB bytes laid out in LDS as the destination rows lie in memory, then stored: whole
//      aligned dwords inside a row segment, single bytes at its head and tail, so no byte outside the destination view is written
// A block outside the padded image is not computed.  Every output byte is a pure function of its MCU: the result does not depend on
// the tile or the grid.  Stats are integer sums (LDS and global integer atomics): exact in any order.  No allocation, no
// synchronisation with the host.
//
// Inter-frame prediction (codec_gop_kernel below): closed GOPs of one intra frame, coded as above, and P-frames that code
// the residual against the previous frame's reconstruction at zero motion with one flat quantiser step.  A workgroup walks one GOP of
// one tile with the reference planes in LDS.
//
// Motion-compensated P-frames (codec_mc_kernel below): a full-pel block search per 16x16 macroblock in the previous
// reconstruction, which then reaches across tiles: one launch per frame position of the GOP, the planes in a workspace in memory.
//
// The backward of the intra codec (codec_grad_kernel at the end of the file): a surrogate differentiated per frame, its
// constants taken from the integer forward of each block, which is recomputed with the phases A, B and the transform passes above.
#include "flk_internal.h"

namespace {

constexpr int kTW = 128;                       // tile width in pixels
constexpr int kSW = (kTW * 3 + 8) / 4;         // dwords per staged row: the segment plus up to 3 bytes of misalignment, whole dwords
constexpr int kCodecThreads = 192;

template <bool S420>
struct CodecGeo {
  static constexpr int TH = S420 ? 64 : 32;                                // tile rows
  static constexpr int CW = S420 ? kTW / 2 : kTW, CH = S420 ? TH / 2 : TH;  // the chroma planes of a tile
  static constexpr int M = S420 ? 16 : 8;                                  // the MCU
};

struct CodecClipDev {                          // 56 bytes; FLK_PREP_MAX_CLIPS of them travel by value in the kernel argument
  const uint8_t* src;                          // the clip's first frame, or its span's (a multiple of gop: frame t of it is intra iff t % gop == 0)
  uint8_t* dst;
  long long pitch_t, dpitch_t;                 // bytes between frames
  int pitch_h, dpitch_h;                       // bytes between rows
  int count, Hs, Ws;                           // frames of the clip, or of the span
  int ntx;                                     // tiles along W
};
struct CodecMcClipDev : CodecClipDev {         // 64 bytes
  long long ws_off;                            // the clip's plane sets within the workspace: [GOP][2][Y, Cb, Cr]
};
static_assert(sizeof(CodecClipDev) == 56 && sizeof(CodecMcClipDev) == 64, "64 and 48 clips per launch rest on these sizes");
struct CodecLaunch {
  const int* idx;                              // device int32 [nclip][gridDim.y] or null: source frame of every output frame
  const uint8_t* tone;                         // device uint8 [nclip][gridDim.y][256][3] or null
  int* stats;                                  // device int32 [nclip][gridDim.y][2] or null (zeroed by the host entry)
  int pad_;
  unsigned short q[2][64];                     // luma, chroma
  CodecClipDev clip[FLK_PREP_MAX_CLIPS];
};
static_assert(sizeof(CodecLaunch) <= 4096, "the launch descriptor must fit the kernel-argument segment");

constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clamp255(int x) { return min(max(x, 0), 255); }

// one 8-point forward pass in place; UP: the two sums are multiplied by 4 (pass 1), else descaled by 2 bits (pass 2)
template <bool UP, int ODD>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (UP) { d0 = (t10 + t11) * 4; d4 = (t10 - t11) * 4; }
  else { d0 = descale(t10 + t11, 2); d4 = descale(t10 - t11, 2); }
  int z1 = (t12 + t13) * F_0_541;
  d2 = descale(z1 + t13 * F_0_765, ODD);
  d6 = descale(z1 - t12 * F_1_847, ODD);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F_1_175;
  t4 *= F_0_298; t5 *= F_2_053; t6 *= F_3_072; t7 *= F_1_501;
  z1 = -z1 * F_0_899; z2 = -z2 * F_2_562; z3 = -z3 * F_1_961 + z5; z4 = -z4 * F_0_390 + z5;
  d7 = descale(t4 + z1 + z3, ODD);
  d5 = descale(t5 + z2 + z4, ODD);
  d3 = descale(t6 + z2 + z3, ODD);
  d1 = descale(t7 + z1 + z4, ODD);
}

// one 8-point inverse pass in place
template <int SHIFT>
__device__ __forceinline__ void idct8(int& c0, int& c1, int& c2, int& c3, int& c4, int& c5, int& c6, int& c7) {
  int z2 = c2, z3 = c6;
  int z1 = (z2 + z3) * F_0_541;
  int t2 = z1 - z3 * F_1_847, t3 = z1 + z2 * F_0_765;
  int t0 = (c0 + c4) * 8192, t1 = (c0 - c4) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = c7; t1 = c5; t2 = c3; t3 = c1;
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * F_1_175;
  t0 *= F_0_298; t1 *= F_2_053; t2 *= F_3_072; t3 *= F_1_501;
  z1 = -z1 * F_0_899; z2 = -z2 * F_2_562; z3 = -z3 * F_1_961 + z5; z4 = -z4 * F_0_390 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  c0 = descale(t10 + t3, SHIFT); c7 = descale(t10 - t3, SHIFT);
  c1 = descale(t11 + t2, SHIFT); c6 = descale(t11 - t2, SHIFT);
  c2 = descale(t12 + t1, SHIFT); c5 = descale(t12 - t1, SHIFT);
  c3 = descale(t13 + t0, SHIFT); c4 = descale(t13 - t0, SHIFT);
}

struct CodecQuant {
  const int (*qt)[64];                         // luma, chroma: an intra block's table
  const float (*rq)[64];                       // the reciprocals of 8 Q
  int Qp;                                      // a P-frame's flat step
  float rqp;                                   // the reciprocal of 8 Qp
};

// An 8x8 block of a byte plane (8-byte aligned rows `pitch` bytes apart) through the transform pair; `rec` is replaced in place.
// Intra: the block of rec itself, minus 128, quantised by the table qt (rounding offset half a step), plus 128.
// INTER, a P-frame's block: the residual of `cur` against the co-located block of the previous reconstruction `rec`, ONE flat step Qp
// (rounding offset a quarter of a step), added back onto the reference.  The reference bytes are read a second time for that add
// and not kept live: the kernels sit at 256 VGPRs.
// rq / rqp are a first guess of the quotient only: the quotient is corrected to the exact one.
template <bool INTER>
__device__ __forceinline__ void codec_block(const uint8_t* cur, uint8_t* rec, int pitch, const int* qt, const float* rq, int Qp, float rqp,
                                            int& nz, int& mag) {
  auto byte = [](unsigned x, int k) { return (int)((x >> (8 * k)) & 255u); };
  int v[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 w = *(const uint2*)((INTER ? cur : rec) + r * pitch);
    uint2 u = {0u, 0u};
    if constexpr (INTER) u = *(const uint2*)(rec + r * pitch);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[r * 8 + k] = byte(w.x, k) - (INTER ? byte(u.x, k) : 128);
      v[r * 8 + 4 + k] = byte(w.y, k) - (INTER ? byte(u.y, k) : 128);
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct8<true, 11>(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct8<false, 15>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int Q = INTER ? Qp : qt[k], d = Q << 3, f = v[k];
    const int n = abs(f) + (INTER ? d >> 2 : d >> 1);  // < 2^15 (a residual: <= 16320 + 510): exact in fp32
    int lev = (int)((float)n * (INTER ? rqp : rq[k])); // within 1 of n / d
    const int rem = n - lev * d;
    lev += rem >= d ? 1 : (rem < 0 ? -1 : 0);          // the exact quotient
    nz += lev != 0;
    mag += lev;
    v[k] = (f < 0 ? -lev : lev) * Q;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) idct8<11>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    idct8<18>(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7]);
    uint2 u = {0u, 0u};
    if constexpr (INTER) u = *(const uint2*)(rec + r * pitch);
    uint2 w = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w.x |= (unsigned)clamp255(v[r * 8 + k] + (INTER ? byte(u.x, k) : 128)) << (8 * k);
      w.y |= (unsigned)clamp255(v[r * 8 + 4 + k] + (INTER ? byte(u.y, k) : 128)) << (8 * k);
    }
    *(uint2*)(rec + r * pitch) = w;
  }
}

__device__ __forceinline__ void rgb_to_ycc(int R, int G, int B, int& Y, int& Cb, int& Cr) {
  Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
  Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16;
  Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16;
}

// the tile of a workgroup
struct CodecTile {
  int y0, x0;                                  // its first row and column
  int nrows, ncols;                            // its part of the image (>= 1 each)
  int prow, pcol;                              // ... of the padded image: whole MCUs
  int nbytes;                                  // of a row segment
  int Hpad, Wpad;                              // the padded image
};

// tile b of a frame of Hs x Ws with ntx tiles along W; false: b is past the frame's tiles (a clip smaller than the largest of the launch)
template <bool S420>
__device__ __forceinline__ bool codec_tile(int Hs, int Ws, int ntx, unsigned b, CodecTile& g) {
  constexpr int TH = CodecGeo<S420>::TH, M = CodecGeo<S420>::M;
  g.Hpad = (Hs + M - 1) / M * M;
  g.Wpad = (Ws + M - 1) / M * M;
  const int nty = (g.Hpad + TH - 1) / TH;
  if ((int)b >= ntx * nty) return false;
  const int ty = b / ntx, tx = b - ty * ntx;
  g.y0 = ty * TH;
  g.x0 = tx * kTW;
  g.nrows = min(TH, Hs - g.y0);
  g.ncols = min(kTW, Ws - g.x0);
  g.prow = min(TH, g.Hpad - g.y0);
  g.pcol = min(kTW, g.Wpad - g.x0);
  g.nbytes = g.ncols * 3;
  return true;
}

// the tile's segment of row r of a frame whose rows lie pitch_h bytes apart
template <class B>
__device__ __forceinline__ B* tile_row(B* frame, int pitch_h, const CodecTile& g, int r) {
  return frame + (long long)(g.y0 + r) * pitch_h + (long long)g.x0 * 3;
}

struct CodecPlanes {                           // one plane set of a tile in LDS: rows of kTW (Y) and CodecGeo::CW (Cb, Cr) bytes
  uint8_t *Y, *Cb, *Cr;
};

// ---- A: the tables, and the source row segments as aligned dwords ----
__device__ __forceinline__ void load_quant(const unsigned short (&q)[2][64], int (*qt)[64], float (*rq)[64]) {
  const int tid = threadIdx.x;
  if (tid < 128) {
    const int Q = q[tid >> 6][tid & 63];
    qt[tid >> 6][tid & 63] = Q;
    rq[tid >> 6][tid & 63] = 1.0f / (float)(Q << 3);
  }
}

// tone: the launch's tables or null; kt: the frame's row of them
__device__ __forceinline__ void load_tone(const uint8_t* tone, size_t kt, uint8_t* tone_lds) {
  if (tone) {
    const uint8_t* g = tone + kt * 768;
    for (int k = threadIdx.x; k < 768; k += kCodecThreads) tone_lds[k] = g[k];
  }
}

__device__ __forceinline__ void stage_rows(const uint8_t* frame, int pitch_h, const CodecTile& g, unsigned* stage, int* mis_of) {
  for (int k = threadIdx.x; k < g.nrows * kSW; k += kCodecThreads) {
    const int r = k / kSW, w = k - r * kSW;
    const uint8_t* row = tile_row(frame, pitch_h, g, r);
    const int mis = (int)((size_t)row & 3);
    if (w == 0) mis_of[r] = mis;
    if (4 * w < mis + g.nbytes) stage[k] = *(const unsigned*)(row - mis + 4 * w);    // never beyond the dword of the segment's last byte
  }
}

// ---- B: staged bytes (through the tone) -> the plane set o over the padded part of the tile (the last column / row repeated) ----
template <bool S420>
__device__ __forceinline__ void build_planes(const unsigned* stage, const int* mis_of, const uint8_t* tone_lds, bool toned, const CodecTile& g,
                                             const CodecPlanes& o) {
  constexpr int CW = CodecGeo<S420>::CW;
  const int tid = threadIdx.x;
  const uint8_t* sb = (const uint8_t*)stage;
  auto ycc = [&](int r, int col, int& Y, int& Cb, int& Cr) {
    const int rs = min(r, g.nrows - 1), cs = min(col, g.ncols - 1);
    const uint8_t* px = sb + rs * (kSW * 4) + mis_of[rs] + cs * 3;
    int R = px[0], G = px[1], B = px[2];
    if (toned) { R = tone_lds[R * 3]; G = tone_lds[G * 3 + 1]; B = tone_lds[B * 3 + 2]; }
    rgb_to_ycc(R, G, B, Y, Cb, Cr);
  };
  if constexpr (S420) {
    const int qc = g.pcol >> 1;
    for (int k = tid; k < (g.prow >> 1) * qc; k += kCodecThreads) {
      const int r2 = k / qc, c2 = k - r2 * qc;
      int sb_ = 0, sr_ = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int Y, Cb, Cr;
        ycc(2 * r2 + (j >> 1), 2 * c2 + (j & 1), Y, Cb, Cr);
        o.Y[(2 * r2 + (j >> 1)) * kTW + 2 * c2 + (j & 1)] = (uint8_t)Y;
        sb_ += Cb; sr_ += Cr;
      }
      const int bias = 1 + (c2 & 1);                  // x0 / 2 is even: the tile's column parity is the plane's
      o.Cb[r2 * CW + c2] = (uint8_t)((sb_ + bias) >> 2);
      o.Cr[r2 * CW + c2] = (uint8_t)((sr_ + bias) >> 2);
    }
  } else {
    for (int k = tid; k < g.prow * g.pcol; k += kCodecThreads) {
      const int r = k / g.pcol, col = k - r * g.pcol;
      int Y, Cb, Cr;
      ycc(r, col, Y, Cb, Cr);
      o.Y[r * kTW + col] = (uint8_t)Y;
      o.Cb[r * CW + col] = (uint8_t)Cb;
      o.Cr[r * CW + col] = (uint8_t)Cr;
    }
  }
}

// ---- C: one block per thread: luma blocks first, then Cb, then Cr; a block outside the padded image is not computed.  An intra
// frame is transformed in place in `rec`; a P-frame's planes `cur` are coded against `rec`, which becomes the reconstruction.
// Which of the two: F, or at kFrameEither the argument `intra` (uniform over the workgroup).  Stats into red[] ----
enum CodecFrame { kFrameIntra, kFrameP, kFrameEither };

template <bool S420, CodecFrame F>
__device__ __forceinline__ void walk_blocks(bool intra, const CodecPlanes& cur, const CodecPlanes& rec, const CodecTile& g, const CodecQuant& q,
                                            bool stats, int* red) {
  constexpr int TH = CodecGeo<S420>::TH, CW = CodecGeo<S420>::CW, CH = CodecGeo<S420>::CH;
  constexpr int NBY = (TH / 8) * (kTW / 8), NBC = (CH / 8) * (CW / 8);
  const int cprow = S420 ? g.prow >> 1 : g.prow, cpcol = S420 ? g.pcol >> 1 : g.pcol;
  int nz = 0, mag = 0;
  auto block = [&](const uint8_t* c, uint8_t* r, int pitch, int tab) {
    if constexpr (F == kFrameEither) {
      if (intra) codec_block<false>(c, r, pitch, q.qt[tab], q.rq[tab], q.Qp, q.rqp, nz, mag);
      else codec_block<true>(c, r, pitch, q.qt[tab], q.rq[tab], q.Qp, q.rqp, nz, mag);
    } else {
      codec_block<F == kFrameP>(c, r, pitch, q.qt[tab], q.rq[tab], q.Qp, q.rqp, nz, mag);
    }
  };
  for (int b = threadIdx.x; b < NBY + 2 * NBC; b += kCodecThreads) {
    if (b < NBY) {
      const int by = b / (kTW / 8), bx = b - by * (kTW / 8);
      const int o = by * 8 * kTW + bx * 8;
      if (by * 8 < g.prow && bx * 8 < g.pcol) block(cur.Y + o, rec.Y + o, kTW, 0);
    } else {
      const int b2 = b - NBY, pl = b2 / NBC, b3 = b2 - pl * NBC;
      const int by = b3 / (CW / 8), bx = b3 - by * (CW / 8);
      const int o = by * 8 * CW + bx * 8;
      if (by * 8 < cprow && bx * 8 < cpcol) block((pl ? cur.Cr : cur.Cb) + o, (pl ? rec.Cr : rec.Cb) + o, CW, 1);
    }
  }
  if (stats && (nz | mag)) {
    atomicAdd(&red[0], nz);
    atomicAdd(&red[1], mag);
  }
}

// after the barrier that follows walk_blocks: the workgroup's sums into row kt of the launch's stats (integer atomics: exact in any order)
__device__ __forceinline__ void stats_to_global(int* stats, size_t kt, const int* red) {
  const int tid = threadIdx.x;
  if (stats && tid < 2 && red[tid]) atomicAdd(stats + kt * 2 + tid, red[tid]);
}

// ---- D: the plane set s -> RGB bytes in `stage`, laid out as the destination rows lie in memory; after a barrier, stored ----
template <bool S420>
__device__ __forceinline__ void planes_to_rgb(const CodecPlanes& s, const uint8_t* dframe, int dpitch_h, const CodecTile& g, unsigned* stage) {
  constexpr int CW = CodecGeo<S420>::CW;
  uint8_t* ob = (uint8_t*)stage;
  for (int k = threadIdx.x; k < g.nrows * g.ncols; k += kCodecThreads) {
    const int r = k / g.ncols, col = k - r * g.ncols;
    const int dm = (int)((size_t)tile_row(dframe, dpitch_h, g, r) & 3);
    const int Y = s.Y[r * kTW + col];
    const int ci = S420 ? (r >> 1) * CW + (col >> 1) : r * CW + col;
    const int cb = (int)s.Cb[ci] - 128, cr = (int)s.Cr[ci] - 128;
    uint8_t* o = ob + r * (kSW * 4) + dm + col * 3;
    o[0] = (uint8_t)clamp255(Y + ((91881 * cr + 32768) >> 16));
    o[1] = (uint8_t)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    o[2] = (uint8_t)clamp255(Y + ((116130 * cb + 32768) >> 16));
  }
}

// whole aligned dwords inside a row segment, single bytes at its head and tail: no byte outside the destination view is written
__device__ __forceinline__ void store_rows(const unsigned* stage, uint8_t* dframe, int dpitch_h, const CodecTile& g) {
  const uint8_t* ob = (const uint8_t*)stage;
  for (int k = threadIdx.x; k < g.nrows * kSW; k += kCodecThreads) {
    const int r = k / kSW, w = k - r * kSW;
    uint8_t* row = tile_row(dframe, dpitch_h, g, r);
    const int dm = (int)((size_t)row & 3);
    const int lo = dm, hi = dm + g.nbytes;             // the segment's bytes within the aligned run that starts at row - dm
    if (4 * w >= hi || 4 * w + 4 <= lo) continue;
    if (4 * w >= lo && 4 * w + 4 <= hi) {
      *(unsigned*)(row - dm + 4 * w) = stage[k];
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * w + b >= lo && 4 * w + b < hi) (row - dm)[4 * w + b] = ob[k * 4 + b];
    }
  }
}

template <bool S420>
__global__ __launch_bounds__(kCodecThreads) void codec_roundtrip_kernel(const CodecLaunch p) {
  using G = CodecGeo<S420>;
  __shared__ unsigned stage[G::TH * kSW];              // source row segments (A, B), then the destination's (D)
  __shared__ __attribute__((aligned(8))) uint8_t Yp[G::TH * kTW];
  __shared__ __attribute__((aligned(8))) uint8_t Cbp[G::CH * G::CW];
  __shared__ __attribute__((aligned(8))) uint8_t Crp[G::CH * G::CW];
  __shared__ uint8_t tone_lds[768];
  __shared__ int mis_of[G::TH];
  __shared__ int qt[2][64];
  __shared__ float rq[2][64];
  __shared__ int red[2];

  const CodecClipDev& c = p.clip[blockIdx.z];
  CodecTile g;
  if (!codec_tile<S420>(c.Hs, c.Ws, c.ntx, blockIdx.x, g)) return;         // uniform over the workgroup
  const int t = blockIdx.y, tid = threadIdx.x;
  const size_t kt = (size_t)blockIdx.z * gridDim.y + t;
  const int fsrc = p.idx ? min(max(p.idx[kt], 0), c.count - 1) : min(t, c.count - 1);
  const CodecPlanes set = {Yp, Cbp, Crp};

  // A
  load_quant(p.q, qt, rq);
  if (tid < 2) red[tid] = 0;
  load_tone(p.tone, kt, tone_lds);
  stage_rows(c.src + (long long)fsrc * c.pitch_t, c.pitch_h, g, stage, mis_of);
  __syncthreads();
  // B
  build_planes<S420>(stage, mis_of, tone_lds, p.tone != nullptr, g, set);
  __syncthreads();
  // C: in place
  walk_blocks<S420, kFrameIntra>(true, set, set, g, {qt, rq, 0, 0.0f}, p.stats != nullptr, red);
  __syncthreads();
  stats_to_global(p.stats, kt, red);
  // D
  uint8_t* dframe = c.dst + (long long)t * c.dpitch_t;
  planes_to_rgb<S420>(set, dframe, c.dpitch_h, g, stage);
  __syncthreads();
  store_rows(stage, dframe, c.dpitch_h, g);
}

// ---- inter-frame prediction: closed GOPs of one intra frame and zero-motion P-frames ----
struct CodecGopLaunch {
  const uint8_t* tone;                         // device uint8 [nclip][T_max][256][3] or null
  int* stats;                                  // device int32 [nclip][T_max][2] or null (zeroed by the host entry)
  int gop, T_max;
  int qp, pad_;                                // the P-frames' step
  unsigned short q[2][64];
  CodecClipDev clip[FLK_PREP_MAX_CLIPS];       // the span's first frame is folded into src
};
static_assert(sizeof(CodecGopLaunch) <= 4096, "the launch descriptor must fit the kernel-argument segment");

// Workgroup = (tile, GOP of the span, clip): it walks its GOP's frames in order, the reconstructed planes of the previous frame kept in
// LDS (plane set 1; set 0 takes a P-frame's own planes).  Zero motion: an output byte depends on its own MCU's history within the GOP
// alone, so there is no workspace in memory and no dependency between workgroups.  Per frame the phases are those of
// codec_roundtrip_kernel; C reads set 0 and set 1 and writes set 1.
template <bool S420>
__global__ __launch_bounds__(kCodecThreads) void codec_gop_kernel(const CodecGopLaunch p) {
  using G = CodecGeo<S420>;
  __shared__ unsigned stage[G::TH * kSW];
  __shared__ __attribute__((aligned(8))) uint8_t Yp[2][G::TH * kTW];
  __shared__ __attribute__((aligned(8))) uint8_t Cbp[2][G::CH * G::CW];
  __shared__ __attribute__((aligned(8))) uint8_t Crp[2][G::CH * G::CW];
  __shared__ uint8_t tone_lds[768];
  __shared__ int mis_of[G::TH];
  __shared__ int qt[2][64];
  __shared__ float rq[2][64];
  __shared__ int red[2];

  const CodecClipDev& c = p.clip[blockIdx.z];
  CodecTile g;
  const int t0 = (int)blockIdx.y * p.gop;              // gridDim.y * gop <= 65535 + gop: no overflow
  if (!codec_tile<S420>(c.Hs, c.Ws, c.ntx, blockIdx.x, g) || t0 >= c.count) return;          // uniform over the workgroup
  const int t1 = min(t0 + p.gop, c.count);
  const int tid = threadIdx.x;
  const CodecQuant quant = {qt, rq, p.qp, 1.0f / (float)(p.qp << 3)};
  const CodecPlanes own = {Yp[0], Cbp[0], Crp[0]}, rec = {Yp[1], Cbp[1], Crp[1]};

  load_quant(p.q, qt, rq);
  for (int t = t0; t < t1; ++t) {
    const bool intra = t == t0;
    const size_t kt = (size_t)blockIdx.z * p.T_max + t;
    if (tid < 2) red[tid] = 0;
    load_tone(p.tone, kt, tone_lds);
    stage_rows(c.src + (long long)t * c.pitch_t, c.pitch_h, g, stage, mis_of);
    __syncthreads();
    build_planes<S420>(stage, mis_of, tone_lds, p.tone != nullptr, g, intra ? rec : own);     // an intra frame is transformed in place in set 1
    __syncthreads();
    walk_blocks<S420, kFrameEither>(intra, own, rec, g, quant, p.stats != nullptr, red);      // every thread keeps its blocks through the GOP
    __syncthreads();
    stats_to_global(p.stats, kt, red);
    uint8_t* dframe = c.dst + (long long)t * c.dpitch_t;
    planes_to_rgb<S420>(rec, dframe, c.dpitch_h, g, stage);
    __syncthreads();
    store_rows(stage, dframe, c.dpitch_h, g);
    __syncthreads();                                   // the next frame stages into what this one stored from
  }
}

// ---- motion-compensated P-frames: a block search per 16x16 macroblock ----
// With vectors a block's reference comes from neighbouring tiles, so a workgroup can no longer walk its GOP alone.  ONE LAUNCH PER
// FRAME POSITION j within the GOP: workgroup = (tile, GOP of the span, clip) handles frame j of its GOP, and the reconstructed padded
// planes travel through a caller-supplied workspace, two plane sets per (clip, GOP), written at parity j & 1 and read at the other.
// Launches depend on each other by stream order alone: no grid barrier, no flags.  Position 0 is the intra path plus the plane store.
constexpr int kMcMaxClips = 48;                // clips per launch: the descriptors are 64 bytes here (the workspace offset)
constexpr int kMaxSearch = 15;
constexpr int kHaloX = 16;                     // columns staged left and right of the tile: whole dwords, >= kMaxSearch
constexpr int kHP = kTW + 2 * kHaloX;          // bytes per staged reference row
static_assert(kHaloX % 4 == 0 && kHaloX >= kMaxSearch && kHP % 4 == 0, "reference rows are staged as aligned dwords");

struct CodecMcLaunch {
  const uint8_t* tone;                         // device uint8 [nclip][T_max][256][3] or null; rows of the whole call, clip0 the launch's first
  int* stats;                                  // device int32 [nclip][T_max][2] or null (zeroed by the host entry)
  signed char* mv;                             // device int8 [nclip][T_max][mv_stride][2] or null (zeroed by the host entry)
  uint8_t* ws;
  int gop, T_max, qp, j;                       // j: the frame position within the GOP this launch codes
  int search, mv_stride, clip0, pad_;
  unsigned short q[2][64];
  CodecMcClipDev clip[kMcMaxClips];
};
static_assert(sizeof(CodecMcLaunch) <= 4096, "the launch descriptor must fit the kernel-argument segment");

__host__ __device__ inline long long mc_set_bytes(long long Hpad, long long Wpad, bool s420) {
  return s420 ? Hpad * Wpad + 2 * (Hpad / 2) * (Wpad / 2) : 3 * Hpad * Wpad;             // a multiple of 64: every plane starts dword-aligned
}

// the vector of a macroblock's winning key SAD * 1024 + rank: rank 0 is (0, 0), rank 1 + (dy + R)(2R + 1) + (dx + R) the others
__device__ __forceinline__ void mc_vector(unsigned key, int R, int& dy, int& dx) {
  const int rank = (int)(key & 1023u), n = 2 * R + 1, k = max(rank - 1, 0), row = k / n;
  dy = rank ? row - R : 0;
  dx = rank ? k - row * n - R : 0;
}

// INTRA: frame position 0 (codec_roundtrip_kernel's phases, then the planes stored).  Otherwise a P-frame: A and B fill plane set 0
// with the frame's own planes; H stages the luma reference under the tile plus a halo (kHaloX columns, `search` rows, coordinates
// clamped into the plane) where the source rows were; S searches the tile's macroblocks, candidates spread over the threads and
// folded by an integer min of SAD * 1024 + rank, which is the serial first-strictly-smaller rule whatever the mapping; P builds the
// prediction in set 1 (luma from the halo, chroma from the workspace); C turns set 1 into the reconstruction; D stores it.
template <bool S420, bool INTRA>
__global__ __launch_bounds__(kCodecThreads) void codec_mc_kernel(const CodecMcLaunch p) {
  using G = CodecGeo<S420>;
  constexpr int TH = G::TH, CW = G::CW, CH = G::CH;
  constexpr int NS = INTRA ? 1 : 2, S1 = NS - 1;       // S1: the set that ends as the reconstruction
  constexpr int NMB = (TH / 16) * (kTW / 16);
  static_assert((TH + 2 * kMaxSearch) * kHP <= TH * kSW * 4, "the staged reference takes the place of the staged source rows");
  __shared__ unsigned stage[TH * kSW];
  __shared__ __attribute__((aligned(16))) uint8_t Yp[NS][TH * kTW];
  __shared__ __attribute__((aligned(8))) uint8_t Cbp[NS][CH * CW];
  __shared__ __attribute__((aligned(8))) uint8_t Crp[NS][CH * CW];
  __shared__ uint8_t tone_lds[768];
  __shared__ int mis_of[TH];
  __shared__ int qt[2][64];
  __shared__ float rq[2][64];
  __shared__ int red[2];
  __shared__ unsigned best[NMB];
  __shared__ int mvl[NMB][2];

  const CodecMcClipDev& c = p.clip[blockIdx.z];
  CodecTile g;
  const int t = (int)blockIdx.y * p.gop + p.j;         // gridDim.y * gop <= 65535 + gop: no overflow
  if (!codec_tile<S420>(c.Hs, c.Ws, c.ntx, blockIdx.x, g) || t >= c.count) return;           // uniform over the workgroup
  const int y0 = g.y0, x0 = g.x0, prow = g.prow, pcol = g.pcol, Hpad = g.Hpad, Wpad = g.Wpad;
  const int cprow = S420 ? prow >> 1 : prow, cpcol = S420 ? pcol >> 1 : pcol;
  const int tid = threadIdx.x;
  const size_t kt = (size_t)(p.clip0 + blockIdx.z) * p.T_max + t;
  const CodecPlanes own = {Yp[0], Cbp[0], Crp[0]}, rec = {Yp[S1], Cbp[S1], Crp[S1]};
  // the two plane sets of this (clip, GOP): this launch writes set j & 1 and reads the other
  const int Hc = S420 ? Hpad >> 1 : Hpad, Wc = S420 ? Wpad >> 1 : Wpad;
  const long long ysz = (long long)Hpad * Wpad, csz = (long long)Hc * Wc, setsz = ysz + 2 * csz;
  uint8_t* wsg = p.ws + c.ws_off + (long long)blockIdx.y * 2 * setsz;
  uint8_t* wcur = wsg + (p.j & 1) * setsz;
  const uint8_t* wref = wsg + ((p.j & 1) ^ 1) * setsz;

  // ---- A, and B: the frame's own planes into set 0 ----
  if constexpr (INTRA) load_quant(p.q, qt, rq);
  if (tid < 2) red[tid] = 0;
  if (tid < NMB) best[tid] = 0xffffffffu;
  load_tone(p.tone, kt, tone_lds);
  stage_rows(c.src + (long long)t * c.pitch_t, c.pitch_h, g, stage, mis_of);
  __syncthreads();
  build_planes<S420>(stage, mis_of, tone_lds, p.tone != nullptr, g, own);
  __syncthreads();

  if constexpr (!INTRA) {
    const int R = p.search;
    const int mbx = (pcol + 15) >> 4, nmb = ((prow + 15) >> 4) * mbx;
    // ---- H: reference luma rows y0 - R .. y0 + prow + R - 1, columns x0 - kHaloX .. as aligned dwords; outside the plane the edge sample ----
    {
      const int d0 = (kHaloX - R) >> 2, nd = ((kHaloX + pcol + R + 3) >> 2) - d0;            // the dwords of a row the search can touch
      for (int k = tid; k < (prow + 2 * R) * nd; k += kCodecThreads) {
        const int hr = k / nd, hd = d0 + (k - hr * nd);
        const uint8_t* row = wref + (long long)min(max(y0 - R + hr, 0), Hpad - 1) * Wpad;
        const int gx = x0 - kHaloX + 4 * hd;           // a multiple of 4, as Wpad is: a dword is inside the plane or outside it, whole
        stage[hr * (kHP / 4) + hd] = gx < 0 ? row[0] * 0x01010101u : gx >= Wpad ? row[Wpad - 1] * 0x01010101u : *(const unsigned*)(row + gx);
      }
    }
    __syncthreads();

    // ---- S: one work item = (macroblock, dy, group of the four dx whose reference rows start in one dword): the five dwords of a
    // reference row are read once for four candidates, whose byte shifts are then constants.  The zero vector's two ranks hold one
    // SAD, so its candidate is keyed with rank 0 and the other rank, which can never win, is not made ----
    {
      const int n = 2 * R + 1, g0 = (kHaloX - R) >> 2, ng = ((kHaloX + R) >> 2) - g0 + 1, per = n * ng;
      for (int it = tid; it < nmb * per; it += kCodecThreads) {
        const int mb = it / per, k = it - mb * per, dyi = k / ng, g = g0 + (k - dyi * ng);
        const int my = mb / mbx, mx = mb - my * mbx;
        const int mbh = min(16, prow - my * 16);       // 16, or 8 where a 4:4:4 plane ends on half a macroblock
        const bool wide = pcol - mx * 16 >= 16;
        const uint8_t* cu = Yp[0] + my * 16 * kTW + mx * 16;
        const unsigned* h = stage + (my * 16 + dyi) * (kHP / 4) + mx * 4 + g;              // row y + dy of the plane is staged row y + dy + R
        unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int r0 = 0; r0 < mbh; r0 += 8) {
#pragma unroll
          for (int rr = 0; rr < 8; ++rr) {
            const uint4 cw = *(const uint4*)(cu + (r0 + rr) * kTW);
            const unsigned* hr = h + (r0 + rr) * (kHP / 4);
            const unsigned a0 = hr[0], a1 = hr[1], a2 = hr[2], a3 = hr[3], a4 = hr[4];   // hr[4]: still inside the staged row (g <= 7)
            s0 = __builtin_amdgcn_sad_u8(cw.x, a0, s0);
            s1 = __builtin_amdgcn_sad_u8(cw.x, __builtin_amdgcn_alignbyte(a1, a0, 1), s1);
            s2 = __builtin_amdgcn_sad_u8(cw.x, __builtin_amdgcn_alignbyte(a1, a0, 2), s2);
            s3 = __builtin_amdgcn_sad_u8(cw.x, __builtin_amdgcn_alignbyte(a1, a0, 3), s3);
            s0 = __builtin_amdgcn_sad_u8(cw.y, a1, s0);
            s1 = __builtin_amdgcn_sad_u8(cw.y, __builtin_amdgcn_alignbyte(a2, a1, 1), s1);
            s2 = __builtin_amdgcn_sad_u8(cw.y, __builtin_amdgcn_alignbyte(a2, a1, 2), s2);
            s3 = __builtin_amdgcn_sad_u8(cw.y, __builtin_amdgcn_alignbyte(a2, a1, 3), s3);
            if (wide) {
              s0 = __builtin_amdgcn_sad_u8(cw.z, a2, s0);
              s1 = __builtin_amdgcn_sad_u8(cw.z, __builtin_amdgcn_alignbyte(a3, a2, 1), s1);
              s2 = __builtin_amdgcn_sad_u8(cw.z, __builtin_amdgcn_alignbyte(a3, a2, 2), s2);
              s3 = __builtin_amdgcn_sad_u8(cw.z, __builtin_amdgcn_alignbyte(a3, a2, 3), s3);
              s0 = __builtin_amdgcn_sad_u8(cw.w, a3, s0);
              s1 = __builtin_amdgcn_sad_u8(cw.w, __builtin_amdgcn_alignbyte(a4, a3, 1), s1);
              s2 = __builtin_amdgcn_sad_u8(cw.w, __builtin_amdgcn_alignbyte(a4, a3, 2), s2);
              s3 = __builtin_amdgcn_sad_u8(cw.w, __builtin_amdgcn_alignbyte(a4, a3, 3), s3);
            }
          }
        }
        const unsigned sads[4] = {s0, s1, s2, s3};
        unsigned key = 0xffffffffu;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int dx = 4 * g + s - kHaloX;           // the group's first and last may hold dx outside the range: not candidates
          const unsigned rank = dyi == R && dx == 0 ? 0u : (unsigned)(1 + dyi * n + dx + R);
          if (dx >= -R && dx <= R) key = min(key, sads[s] * 1024u + rank);
        }
        atomicMin(&best[mb], key);
      }
    }
    __syncthreads();
    if (tid < nmb) {
      int dy, dx;
      mc_vector(best[tid], R, dy, dx);
      mvl[tid][0] = dy; mvl[tid][1] = dx;
      if (p.mv) {
        const int my = tid / mbx, mx = tid - my * mbx;
        signed char* o = p.mv + (kt * p.mv_stride + (size_t)((y0 >> 4) + my) * ((Wpad + 15) >> 4) + (x0 >> 4) + mx) * 2;
        o[0] = (signed char)dy; o[1] = (signed char)dx;
      }
    }
    __syncthreads();

    // ---- P: the prediction into set 1: luma from the staged reference, chroma from the workspace with clamped coordinates ----
    {
      const int qd = pcol >> 2;
      for (int k = tid; k < prow * qd; k += kCodecThreads) {
        const int r = k / qd, col = (k - r * qd) * 4;
        const int mb = (r >> 4) * mbx + (col >> 4);
        const int off = (r + mvl[mb][0] + R) * kHP + col + mvl[mb][1] + kHaloX;
        const unsigned* h = stage + (off >> 2);
        *(unsigned*)(Yp[1] + r * kTW + col) = __builtin_amdgcn_alignbyte(h[1], h[0], (unsigned)off & 3u);
      }
      const uint8_t* rcb = wref + ysz;
      const uint8_t* rcr = rcb + csz;
      const int cy0 = S420 ? y0 >> 1 : y0, cx0 = S420 ? x0 >> 1 : x0;
      for (int k = tid; k < cprow * cpcol; k += kCodecThreads) {
        const int r = k / cpcol, col = k - r * cpcol;
        const int mb = S420 ? (r >> 3) * mbx + (col >> 3) : (r >> 4) * mbx + (col >> 4);
        const int dy = mvl[mb][0], dx = mvl[mb][1];
        if constexpr (S420) {
          const int ya = min(max(cy0 + r + (dy >> 1), 0), Hc - 1), yb = min(max(cy0 + r + (dy >> 1) + 1, 0), Hc - 1);
          const int xa = min(max(cx0 + col + (dx >> 1), 0), Wc - 1), xb = min(max(cx0 + col + (dx >> 1) + 1, 0), Wc - 1);
          const bool hy = dy & 1, hx = dx & 1;
          auto half = [&](const uint8_t* pl) -> int {
            const int a = pl[(long long)ya * Wc + xa];
            if (hy && hx) return (a + pl[(long long)ya * Wc + xb] + pl[(long long)yb * Wc + xa] + pl[(long long)yb * Wc + xb] + 2) >> 2;
            if (hx) return (a + pl[(long long)ya * Wc + xb] + 1) >> 1;
            if (hy) return (a + pl[(long long)yb * Wc + xa] + 1) >> 1;
            return a;
          };
          Cbp[1][r * CW + col] = (uint8_t)half(rcb);
          Crp[1][r * CW + col] = (uint8_t)half(rcr);
        } else {
          const long long o = (long long)min(max(cy0 + r + dy, 0), Hc - 1) * Wc + min(max(cx0 + col + dx, 0), Wc - 1);
          Cbp[1][r * CW + col] = rcb[o];
          Crp[1][r * CW + col] = rcr[o];
        }
      }
    }
    __syncthreads();
  }

  // ---- C: set S1 becomes the reconstruction ----
  walk_blocks<S420, INTRA ? kFrameIntra : kFrameP>(INTRA, own, rec, g, {qt, rq, p.qp, 1.0f / (float)(p.qp << 3)}, p.stats != nullptr, red);
  __syncthreads();
  stats_to_global(p.stats, kt, red);

  // ---- D: the reconstruction to the workspace (whole dwords of the padded planes), and as RGB bytes to the destination ----
  {
    const int qd = pcol >> 2, cqd = cpcol >> 2;
    for (int k = tid; k < prow * qd; k += kCodecThreads) {
      const int r = k / qd, col = (k - r * qd) * 4;
      *(unsigned*)(wcur + (long long)(y0 + r) * Wpad + x0 + col) = *(const unsigned*)(Yp[S1] + r * kTW + col);
    }
    const int cy0 = S420 ? y0 >> 1 : y0, cx0 = S420 ? x0 >> 1 : x0;
    for (int k = tid; k < cprow * cqd; k += kCodecThreads) {
      const int r = k / cqd, col = (k - r * cqd) * 4;
      const long long o = ysz + (long long)(cy0 + r) * Wc + cx0 + col;
      *(unsigned*)(wcur + o) = *(const unsigned*)(Cbp[S1] + r * CW + col);
      *(unsigned*)(wcur + csz + o) = *(const unsigned*)(Crp[S1] + r * CW + col);
    }
  }
  uint8_t* dframe = c.dst + (long long)t * c.dpitch_t;
  planes_to_rgb<S420>(rec, dframe, c.dpitch_h, g, stage);
  __syncthreads();
  store_rows(stage, dframe, c.dpitch_h, g);
}

}  // namespace

// the two quantisation tables at `quality` (1..100): ITU T.81 Annex K under the IJG scaling rule, row-major
void flk_codec_tables_host(int quality, int32_t* qluma, int32_t* qchroma) {
  static const unsigned char base_l[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                           14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  static const unsigned char base_c[32] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                           24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99};
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int k = 0; k < 64; ++k) {
    const int l = (base_l[k] * s + 50) / 100, ch = ((k < 32 ? base_c[k] : 99) * s + 50) / 100;
    qluma[k] = l < 1 ? 1 : l > 255 ? 255 : l;
    qchroma[k] = ch < 1 ? 1 : ch > 255 ? 255 : ch;
  }
}

// the P-frames' quantiser step at `quality` (1..100): MPEG-2's flat non-intra 16 under the IJG scaling rule
int flk_codec_inter_step_host(int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int q = (16 * s + 50) / 100;
  return q < 1 ? 1 : q > 255 ? 255 : q;
}

// the q[2][64] of a launch descriptor
static void fill_quant(int quality, unsigned short (*q)[64]) {
  int32_t ql[64], qc[64];
  flk_codec_tables_host(quality, ql, qc);
  for (int k = 0; k < 64; ++k) { q[0][k] = (unsigned short)ql[k]; q[1][k] = (unsigned short)qc[k]; }
}

static long long padded(long long n, bool s420) { return s420 ? (n + 15) / 16 * 16 : (n + 7) / 8 * 8; }    // to whole MCUs

// the descriptor of the `count` frames of clip s from its frame `first`; returns the number of tiles of one of its frames
static long long fill_clip(CodecClipDev& d, const flk_codec_clip& s, int first, int count, bool s420) {
  d.src = s.src + (long long)first * s.pitch_t; d.dst = s.dst; d.pitch_t = s.pitch_t; d.dpitch_t = s.dst_pitch_t;
  d.pitch_h = (int)s.pitch_h; d.dpitch_h = (int)s.dst_pitch_h;
  d.count = count; d.Hs = s.Hs; d.Ws = s.Ws;
  d.ntx = (int)((padded(s.Ws, s420) + kTW - 1) / kTW);
  const int TH = s420 ? 64 : 32;
  return d.ntx * ((padded(s.Hs, s420) + TH - 1) / TH);
}

static long long max_of(long long a, long long b) { return a > b ? a : b; }

// arguments already validated (api.cpp: flk_codec_roundtrip_u8); everything here up to the launch is host arithmetic
int flk_codec_roundtrip_launch(const flk_codec_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, int32_t* stats,
                               hipStream_t stream) {
  CodecLaunch p;
  const bool s420 = a->subsampling == FLK_CODEC_420;
  p.idx = frame_idx; p.tone = tone; p.stats = stats; p.pad_ = 0;
  fill_quant(a->quality, p.q);
  long long max_tiles = 1;
  for (int i = 0; i < a->nclip; ++i) max_tiles = max_of(max_tiles, fill_clip(p.clip[i], a->clips[i], 0, a->clips[i].T, s420));
  FLK_REQUIRE(max_tiles <= 0x7fffffffLL, "flk_codec_roundtrip_u8: a frame of more than 2^31 tiles");
  if (stats) FLK_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)a->nclip * T_out * 2 * sizeof(int32_t), stream));
  const dim3 grid((unsigned)max_tiles, (unsigned)T_out, (unsigned)a->nclip);
  if (s420) FLK_LAUNCH_KERNEL(codec_roundtrip_kernel<true>, grid, dim3(kCodecThreads), 0, stream, p);
  else FLK_LAUNCH_KERNEL(codec_roundtrip_kernel<false>, grid, dim3(kCodecThreads), 0, stream, p);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// arguments already validated (api.cpp: flk_codec_roundtrip_gop_u8); everything here up to the launch is host arithmetic
int flk_codec_roundtrip_gop_launch(const flk_codec_args* a, int gop, const int32_t* first, const int32_t* count, int T_max,
                                   const uint8_t* tone, int32_t* stats, hipStream_t stream) {
  CodecGopLaunch p;
  const bool s420 = a->subsampling == FLK_CODEC_420;
  p.tone = tone; p.stats = stats; p.gop = gop; p.T_max = T_max; p.qp = flk_codec_inter_step_host(a->quality); p.pad_ = 0;
  fill_quant(a->quality, p.q);
  long long max_tiles = 1, max_gops = 1;
  for (int i = 0; i < a->nclip; ++i) {
    max_tiles = max_of(max_tiles, fill_clip(p.clip[i], a->clips[i], first[i], count[i], s420));
    max_gops = max_of(max_gops, (count[i] + gop - 1) / gop);                // count <= 65535: no overflow
  }
  FLK_REQUIRE(max_tiles <= 0x7fffffffLL, "flk_codec_roundtrip_gop_u8: a frame of more than 2^31 tiles");
  if (stats) FLK_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)a->nclip * T_max * 2 * sizeof(int32_t), stream));
  const dim3 grid((unsigned)max_tiles, (unsigned)max_gops, (unsigned)a->nclip);
  if (s420) FLK_LAUNCH_KERNEL(codec_gop_kernel<true>, grid, dim3(kCodecThreads), 0, stream, p);
  else FLK_LAUNCH_KERNEL(codec_gop_kernel<false>, grid, dim3(kCodecThreads), 0, stream, p);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}

// the workspace of flk_codec_roundtrip_mc_u8: two plane sets per (clip, GOP of its span); 0 where the arguments are not a launch's
long long flk_codec_mc_scratch_host(const flk_codec_args* a, int gop, const int32_t* count) {
  if (!a || !a->clips || !count || a->nclip < 1 || gop < 1 || gop > 65535) return 0;
  if (a->subsampling != FLK_CODEC_420 && a->subsampling != FLK_CODEC_444) return 0;
  const bool s420 = a->subsampling == FLK_CODEC_420;
  long long total = 0;
  for (int i = 0; i < a->nclip; ++i) {
    const flk_codec_clip& s = a->clips[i];
    if (s.Hs < 1 || s.Ws < 1 || count[i] < 1 || count[i] > 65535) return 0;
    const long long Hpad = padded(s.Hs, s420), Wpad = padded(s.Ws, s420);
    if (Hpad > (1LL << 34) / Wpad) return 0;           // a plane set of more than 2^36 bytes: no such workspace, and no overflow below
    total += (long long)((count[i] + gop - 1) / gop) * 2 * mc_set_bytes(Hpad, Wpad, s420);
    if (total > (1LL << 60)) return 0;
  }
  return total;
}

// arguments already validated (api.cpp: flk_codec_roundtrip_mc_u8); everything here up to the first launch is host arithmetic.  One
// launch per frame position of the GOP and kMcMaxClips clips; positions follow each other on the stream, which is all the ordering
// the reference planes need.
int flk_codec_roundtrip_mc_launch(const flk_codec_args* a, int gop, int search, const int32_t* first, const int32_t* count, int T_max,
                                  const uint8_t* tone, int32_t* stats, int8_t* mv, int mv_stride, void* scratch, hipStream_t stream) {
  const bool s420 = a->subsampling == FLK_CODEC_420;
  CodecMcLaunch p;
  p.tone = tone; p.stats = stats; p.mv = (signed char*)mv; p.ws = (uint8_t*)scratch;
  p.gop = gop; p.T_max = T_max; p.qp = flk_codec_inter_step_host(a->quality); p.search = search; p.mv_stride = mv_stride; p.pad_ = 0;
  fill_quant(a->quality, p.q);
  if (stats) FLK_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)a->nclip * T_max * 2 * sizeof(int32_t), stream));
  if (mv) FLK_CHECK_HIP(hipMemsetAsync(mv, 0, (size_t)a->nclip * T_max * mv_stride * 2, stream));
  long long ws_off = 0;
  for (int c0 = 0; c0 < a->nclip; c0 += kMcMaxClips) {
    const int n = a->nclip - c0 < kMcMaxClips ? a->nclip - c0 : kMcMaxClips;
    long long max_tiles = 1, max_gops = 1, max_count = 1;
    for (int i = 0; i < n; ++i) {
      const flk_codec_clip& s = a->clips[c0 + i];
      const int cnt = count[c0 + i], gops = (cnt + gop - 1) / gop;
      max_tiles = max_of(max_tiles, fill_clip(p.clip[i], s, first[c0 + i], cnt, s420));
      max_gops = max_of(max_gops, gops);
      max_count = max_of(max_count, cnt);
      p.clip[i].ws_off = ws_off;
      ws_off += (long long)gops * 2 * mc_set_bytes(padded(s.Hs, s420), padded(s.Ws, s420), s420);
    }
    FLK_REQUIRE(max_tiles <= 0x7fffffffLL, "flk_codec_roundtrip_mc_u8: a frame of more than 2^31 tiles");
    p.clip0 = c0;
    const dim3 grid((unsigned)max_tiles, (unsigned)max_gops, (unsigned)n);
    for (int j = 0; j < gop && j < max_count; ++j) {
      p.j = j;
      if (j == 0) {
        if (s420) FLK_LAUNCH_KERNEL((codec_mc_kernel<true, true>), grid, dim3(kCodecThreads), 0, stream, p);
        else FLK_LAUNCH_KERNEL((codec_mc_kernel<false, true>), grid, dim3(kCodecThreads), 0, stream, p);
      } else {
        if (s420) FLK_LAUNCH_KERNEL((codec_mc_kernel<true, false>), grid, dim3(kCodecThreads), 0, stream, p);
        else FLK_LAUNCH_KERNEL((codec_mc_kernel<false, false>), grid, dim3(kCodecThreads), 0, stream, p);
      }
      FLK_CHECK_HIP(hipGetLastError());
    }
  }
  return FLK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The codec's backward (flk_codec_grad; videoresnet_spec.codec_grad_host is the definition in float64).  The forward
// stays the integer codec above; the backward differentiates a surrogate of it, per frame, whose constants come from the integer
// forward of each block, recomputed here and not stored:
//   colour   the derivative of the fixed-point definitions: the integer constants over 2^16 (dyadic, exact in fp32); rounding: 1
//   clamps   the plane clamp after the inverse transform and the RGB clamp pass the gradient where the UNCLAMPED integer lies in 0..255
//   pad      the transpose of the replication: the padded pixels' gradients are added onto the last row and column
//   4:2:0    the box mean gives 1/4 to each of its four pixels; the replication on decode sums its four pixels
//   DCT      the orthonormal 8x8 DCT-II matrix C in fp32 (kDct): G = C g C^T is the transpose of the inverse, C^T G C of the forward
//            (the forward's x 8 and the quantiser's 8 Q cancel)
//   quant    per coefficient f with level lev: r = (f - lev * 8 Q) / (8 Q) in [-1/2, 1/2] from the integers; the factor d is 1
//            (FLK_CODEC_GRAD_STE) or 3 r^2 (FLK_CODEC_GRAD_CUBIC: the rounding u -> round(u) + (u - round(u))^3)
// g_out [Hs][Ws][3] -> RGB mask, M_dec^T, chroma 2x2 sum, plane mask, C . C^T, x d, C^T . C, chroma 1/4 spread, padding fold, M_enc^T
// -> g_in [Hs][Ws][3];   gdelta[k][t][c] = scale[k][t][c] * sum over pixels of g_in(p, c) * slope[k][t][v(p, c)][c], v the SOURCE byte.
// Mapping: the forward's tiling and its phases A and B unchanged; every thread owns exactly one 8x8 block of the tile (192 blocks), so
// what the integer forward of a block leaves for its backward -- the remainders f - lev * 8 Q, two int16 to a register, and the 64
// bits of the plane mask -- stays in that thread's registers across the barriers:
//   C1  codec_grad_block_forward: the block's integer forward; the reconstruction in place (the RGB mask reads all three planes)
//   D1  per pixel: unclamped RGB from the reconstruction, g_out through the mask and M_dec^T into the fp32 gradient planes (4:2:0:
//       one thread per chroma sample, its four pixels in the order of build_planes)
//   C2  codec_grad_block: the block's gradient through mask, C . C^T, d, C^T . C, in place
//   E   per image pixel: spread, fold (rows outer, columns inner, ascending from +0), M_enc^T, optional g_in store, times the slope of
//       its source byte; a thread adds its pixels k = tid, tid + 192, .. ascending from +0; lanes fold by the shuffle tree 32 .. 1, the
//       three waves ascending from +0: partials[k][t][tile][c].  The finishing launch adds a frame's tiles ascending from +0 and
//       multiplies by scale (a zero scale writes +0).  No atomics: repeats are bitwise equal, a clip's result is that of a call with
//       it alone (the tile sums do not see the grid).
// The gradient planes are fp32 in LDS, BLOCK-MAJOR: block b at b * kGB floats, kGB = 64 + 4 -- a thread reads its block as sixteen
// 16-byte accesses whose lanes lie 272 bytes apart (4 banks on from lane to lane: sixteen lanes cover the 64 banks once), where a
// row-major plane would put lanes 32 bytes apart, two to a bank.
namespace {

constexpr int kGB = 68;                        // floats between the blocks of a gradient plane

struct CodecGradLaunch {
  const int* idx;                              // device int32 [nclip][gridDim.y] or null
  const uint8_t* tone;                         // device uint8 [nclip][gridDim.y][256][3] or null
  const float* slope;                          // device fp32 [nclip][gridDim.y][256][3]
  float* partials;                             // device fp32 [nclip][gridDim.y][max_tiles][3]
  const float* g_out;                          // the packed gradient images; a clip's dst is its first frame IN g_out, its pitches floats
  float* g_in;                                 // packed as g_out, or null
  int mode, max_tiles;
  unsigned short q[2][64];
  CodecClipDev clip[FLK_PREP_MAX_CLIPS];
};
static_assert(sizeof(CodecGradLaunch) <= 4096, "the launch descriptor must fit the kernel-argument segment");

// one 8-point pass in place with the fp32 orthonormal DCT-II matrix C[u][x] = a(u) cos((2 x + 1) u pi / 16) (a(0) = sqrt(1/8), else
// 1/2; float64 values rounded once): y = C x, or with T y = C^T x; every output the chain fma(c7, x7, .. fma(c1, x1, c0 * x0))
template <bool T>
__device__ __forceinline__ void dct8f(float& x0, float& x1, float& x2, float& x3, float& x4, float& x5, float& x6, float& x7) {
  constexpr float C[8][8] = {
      {0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f},
      {0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f},
      {0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f},
      {0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f},
      {0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f},
      {0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f},
      {0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f},
      {0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f}};
  const float x[8] = {x0, x1, x2, x3, x4, x5, x6, x7};
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float s = (T ? C[0][j] : C[j][0]) * x[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s = fmaf(T ? C[i][j] : C[j][i], x[i], s);
    y[j] = s;
  }
  x0 = y[0]; x1 = y[1]; x2 = y[2]; x3 = y[3]; x4 = y[4]; x5 = y[5]; x6 = y[6]; x7 = y[7];
}

// The integer forward of one intra block, as codec_block<false> runs it, for the backward: `rec` (8-byte aligned rows `pitch` bytes
// apart) is replaced by its reconstruction in place.  Left for codec_grad_block: rem, per coefficient f - lev * 8 Q with lev signed
// (in [-4 Q, 4 Q], |.| <= 1020: two int16 to a register), and keep, bit 8 r + c set where the reconstruction of pixel (r, c) BEFORE its
// clamp lies in 0..255.
__device__ __forceinline__ void codec_grad_block_forward(uint8_t* rec, int pitch, const int* qt, const float* rq, unsigned (&rem)[32],
                                                         unsigned long long& keep) {
  auto byte = [](unsigned x, int k) { return (int)((x >> (8 * k)) & 255u); };
  int v[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 w = *(const uint2*)(rec + r * pitch);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[r * 8 + k] = byte(w.x, k) - 128;
      v[r * 8 + 4 + k] = byte(w.y, k) - 128;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct8<true, 11>(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct8<false, 15>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int Q = qt[k], d = Q << 3, f = v[k];
    const int n = abs(f) + (d >> 1);
    int lev = (int)((float)n * rq[k]);                 // within 1 of n / d
    const int over = n - lev * d;
    lev += over >= d ? 1 : (over < 0 ? -1 : 0);        // the exact quotient
    const int sl = f < 0 ? -lev : lev;
    const unsigned rm = (unsigned)(f - sl * d) & 0xffffu;
    if (k & 1) rem[k >> 1] |= rm << 16;
    else rem[k >> 1] = rm;
    v[k] = sl * Q;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) idct8<11>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
  keep = 0ull;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    idct8<18>(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7]);
    uint2 w = {0u, 0u};
    unsigned bits = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int o = v[r * 8 + k] + 128;
      bits |= ((unsigned)o <= 255u ? 1u : 0u) << k;
      if (k < 4) w.x |= (unsigned)clamp255(o) << (8 * k);
      else w.y |= (unsigned)clamp255(o) << (8 * (k - 4));
    }
    keep |= (unsigned long long)bits << (8 * r);
    *(uint2*)(rec + r * pitch) = w;
  }
}

// The backward of one intra block, in place on its 64 gradients g (block-major, 16-byte aligned): plane mask, G = C g C^T, times the
// quantiser's factor d (1, or 3 r^2 with r = rem / (8 Q): rq holds the reciprocals), C^T G C.  The unit a reverse walk of a GOP calls.
__device__ __forceinline__ void codec_grad_block(float* g, const unsigned (&rem)[32], unsigned long long keep, const float* rq, bool cubic) {
  float v[64];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float4 w = *(const float4*)(g + 4 * k);
    v[4 * k] = (keep >> (4 * k)) & 1ull ? w.x : 0.f;
    v[4 * k + 1] = (keep >> (4 * k + 1)) & 1ull ? w.y : 0.f;
    v[4 * k + 2] = (keep >> (4 * k + 2)) & 1ull ? w.z : 0.f;
    v[4 * k + 3] = (keep >> (4 * k + 3)) & 1ull ? w.w : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) dct8f<false>(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c) dct8f<false>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
  if (cubic) {
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const int rm = (int)(short)(k & 1 ? rem[k >> 1] >> 16 : rem[k >> 1] & 0xffffu);
      const float r = (float)rm * rq[k];
      v[k] *= 3.f * (r * r);
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) dct8f<true>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
  for (int r = 0; r < 8; ++r) dct8f<true>(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7]);
#pragma unroll
  for (int k = 0; k < 16; ++k) *(float4*)(g + 4 * k) = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}

// pixel (r, col) of a block-major gradient plane of `bw` blocks to the row
__device__ __forceinline__ int grad_at(int r, int col, int bw) { return ((r >> 3) * bw + (col >> 3)) * kGB + (r & 7) * 8 + (col & 7); }

// the derivatives of the two colour transforms: the integer constants over 2^16
constexpr float kCs = 1.0f / 65536.0f;
constexpr float kDecRCr = 91881 * kCs, kDecGCb = -22554 * kCs, kDecGCr = -46802 * kCs, kDecBCb = 116130 * kCs;
constexpr float kEncYR = 19595 * kCs, kEncYG = 38470 * kCs, kEncYB = 7471 * kCs;
constexpr float kEncCbR = -11059 * kCs, kEncCbG = -21709 * kCs, kEncCbB = 32768 * kCs;
constexpr float kEncCrR = 32768 * kCs, kEncCrG = -27439 * kCs, kEncCrB = -5329 * kCs;

template <bool S420>
struct CodecGradLds {                          // byte offsets into the dynamic LDS of codec_grad_kernel
  using G = CodecGeo<S420>;
  static constexpr int NBY = (G::TH / 8) * (kTW / 8), NBC = (G::CH / 8) * (G::CW / 8);
  static constexpr int stage = 0;
  static constexpr int Yp = stage + G::TH * kSW * 4;
  static constexpr int Cbp = Yp + G::TH * kTW;
  static constexpr int Crp = Cbp + G::CH * G::CW;
  static constexpr int gY = Crp + G::CH * G::CW;
  static constexpr int gCb = gY + NBY * kGB * 4;
  static constexpr int gCr = gCb + NBC * kGB * 4;
  static constexpr int slope = gCr + NBC * kGB * 4;
  static constexpr int tone = slope + 768 * 4;
  static constexpr int mis = tone + 768;
  static constexpr int qt = mis + G::TH * 4;
  static constexpr int rq = qt + 128 * 4;
  static constexpr int wsum = rq + 128 * 4;
  static constexpr int bytes = wsum + 16 * 4;
  static_assert(NBY + 2 * NBC == kCodecThreads, "one block per thread: its remainders and mask stay in registers across the barriers");
  static_assert(Yp % 16 == 0 && Cbp % 8 == 0 && Crp % 8 == 0 && gY % 16 == 0 && gCb % 16 == 0 && gCr % 16 == 0 && slope % 4 == 0 && mis % 4 == 0,
                "alignment of the LDS arrays");
  static_assert(bytes <= 160 * 1024, "the LDS of a CU");
};

template <bool S420>
__global__ __launch_bounds__(kCodecThreads) void codec_grad_kernel(const CodecGradLaunch p) {
  using G = CodecGeo<S420>;
  using L = CodecGradLds<S420>;
  constexpr int CW = G::CW, NBY = L::NBY, NBC = L::NBC;
  extern __shared__ __attribute__((aligned(16))) char codec_grad_lds[];
  unsigned* stage = (unsigned*)(codec_grad_lds + L::stage);
  uint8_t* Yp = (uint8_t*)(codec_grad_lds + L::Yp);
  uint8_t* Cbp = (uint8_t*)(codec_grad_lds + L::Cbp);
  uint8_t* Crp = (uint8_t*)(codec_grad_lds + L::Crp);
  float* gY = (float*)(codec_grad_lds + L::gY);
  float* gCb = (float*)(codec_grad_lds + L::gCb);
  float* gCr = (float*)(codec_grad_lds + L::gCr);
  float* slope_lds = (float*)(codec_grad_lds + L::slope);
  uint8_t* tone_lds = (uint8_t*)(codec_grad_lds + L::tone);
  int* mis_of = (int*)(codec_grad_lds + L::mis);
  int (*qt)[64] = (int (*)[64])(codec_grad_lds + L::qt);
  float (*rq)[64] = (float (*)[64])(codec_grad_lds + L::rq);
  float* wsum = (float*)(codec_grad_lds + L::wsum);

  const CodecClipDev& c = p.clip[blockIdx.z];
  CodecTile g;
  if (!codec_tile<S420>(c.Hs, c.Ws, c.ntx, blockIdx.x, g)) return;         // uniform over the workgroup
  const int t = blockIdx.y, tid = threadIdx.x;
  const size_t kt = (size_t)blockIdx.z * gridDim.y + t;
  const int fsrc = p.idx ? min(max(p.idx[kt], 0), c.count - 1) : min(t, c.count - 1);
  const CodecPlanes set = {Yp, Cbp, Crp};
  const int cprow = S420 ? g.prow >> 1 : g.prow, cpcol = S420 ? g.pcol >> 1 : g.pcol;

  // A
  load_quant(p.q, qt, rq);
  load_tone(p.tone, kt, tone_lds);
  for (int k = tid; k < 768; k += kCodecThreads) slope_lds[k] = p.slope[kt * 768 + k];
  stage_rows(c.src + (long long)fsrc * c.pitch_t, c.pitch_h, g, stage, mis_of);
  __syncthreads();
  // B
  build_planes<S420>(stage, mis_of, tone_lds, p.tone != nullptr, g, set);
  __syncthreads();

  // C1: this thread's block (walk_blocks' numbering: luma, then Cb, then Cr); one outside the padded image is not computed
  unsigned rem[32];
  unsigned long long keep = 0ull;
  float* gblk;
  bool live;
  int tab;
  {
    uint8_t* blk;
    int pitch;
    if (tid < NBY) {
      const int by = tid / (kTW / 8), bx = tid - by * (kTW / 8);
      blk = Yp + by * 8 * kTW + bx * 8; pitch = kTW; tab = 0;
      gblk = gY + tid * kGB;
      live = by * 8 < g.prow && bx * 8 < g.pcol;
    } else {
      const int b2 = tid - NBY, pl = b2 / NBC, b3 = b2 - pl * NBC;
      const int by = b3 / (CW / 8), bx = b3 - by * (CW / 8);
      blk = (pl ? Crp : Cbp) + by * 8 * CW + bx * 8; pitch = CW; tab = 1;
      gblk = (pl ? gCr : gCb) + b3 * kGB;
      live = by * 8 < cprow && bx * 8 < cpcol;
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) rem[k] = 0u;
    if (live) codec_grad_block_forward(blk, pitch, qt[tab], rq[tab], rem, keep);
  }
  __syncthreads();

  // D1: g_out through the RGB mask and M_dec^T into the gradient planes; a padded pixel has no output, hence no gradient
  {
    const float* gframe = (const float*)c.dst + (long long)t * c.dpitch_t;
    auto pixel = [&](int r, int col, float& gy, float& gcb, float& gcr) {
      gy = gcb = gcr = 0.f;
      if (r < g.nrows && col < g.ncols) {
        const int Y = Yp[r * kTW + col];
        const int ci = S420 ? (r >> 1) * CW + (col >> 1) : r * CW + col;
        const int cb = (int)Cbp[ci] - 128, cr = (int)Crp[ci] - 128;
        const int R = Y + ((91881 * cr + 32768) >> 16), Gn = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), B = Y + ((116130 * cb + 32768) >> 16);
        const float* go = gframe + (long long)(g.y0 + r) * c.dpitch_h + (long long)(g.x0 + col) * 3;
        const float gr = (unsigned)R <= 255u ? go[0] : 0.f, gg = (unsigned)Gn <= 255u ? go[1] : 0.f, gb = (unsigned)B <= 255u ? go[2] : 0.f;
        gy = (gr + gg) + gb;
        gcb = fmaf(kDecBCb, gb, kDecGCb * gg);
        gcr = fmaf(kDecGCr, gg, kDecRCr * gr);
      }
    };
    if constexpr (S420) {
      const int qc = g.pcol >> 1;
      for (int k = tid; k < (g.prow >> 1) * qc; k += kCodecThreads) {
        const int r2 = k / qc, c2 = k - r2 * qc;
        float sb = 0.f, sr = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float gy, gcb, gcr;
          pixel(2 * r2 + (j >> 1), 2 * c2 + (j & 1), gy, gcb, gcr);
          gY[grad_at(2 * r2 + (j >> 1), 2 * c2 + (j & 1), kTW / 8)] = gy;
          sb += gcb; sr += gcr;
        }
        gCb[grad_at(r2, c2, CW / 8)] = sb;
        gCr[grad_at(r2, c2, CW / 8)] = sr;
      }
    } else {
      for (int k = tid; k < g.prow * g.pcol; k += kCodecThreads) {
        const int r = k / g.pcol, col = k - r * g.pcol;
        float gy, gcb, gcr;
        pixel(r, col, gy, gcb, gcr);
        const int o = grad_at(r, col, kTW / 8);
        gY[o] = gy; gCb[o] = gcb; gCr[o] = gcr;
      }
    }
  }
  __syncthreads();

  // C2
  if (live) codec_grad_block(gblk, rem, keep, rq[tab], p.mode == FLK_CODEC_GRAD_CUBIC);
  __syncthreads();

  // E: spread, fold, M_enc^T, the slope of the source byte
  float acc[3] = {0.f, 0.f, 0.f};
  {
    const uint8_t* sb = (const uint8_t*)stage;
    float* iframe = p.g_in ? p.g_in + (((const float*)c.dst - p.g_out) + (long long)t * c.dpitch_t) : nullptr;
    for (int k = tid; k < g.nrows * g.ncols; k += kCodecThreads) {
      const int r = k / g.ncols, col = k - r * g.ncols;
      const int r1 = r == g.nrows - 1 ? g.prow : r + 1, c1 = col == g.ncols - 1 ? g.pcol : col + 1;     // the last row / column takes the padding's
      float gy = 0.f, gcb = 0.f, gcr = 0.f;
      for (int rr = r; rr < r1; ++rr)
        for (int cc = col; cc < c1; ++cc) {
          gy += gY[grad_at(rr, cc, kTW / 8)];
          const int o = S420 ? grad_at(rr >> 1, cc >> 1, CW / 8) : grad_at(rr, cc, CW / 8);
          gcb += S420 ? 0.25f * gCb[o] : gCb[o];
          gcr += S420 ? 0.25f * gCr[o] : gCr[o];
        }
      float gi[3];
      gi[0] = fmaf(kEncCrR, gcr, fmaf(kEncCbR, gcb, kEncYR * gy));
      gi[1] = fmaf(kEncCrG, gcr, fmaf(kEncCbG, gcb, kEncYG * gy));
      gi[2] = fmaf(kEncCrB, gcr, fmaf(kEncCbB, gcb, kEncYB * gy));
      const uint8_t* px = sb + r * (kSW * 4) + mis_of[r] + col * 3;
      float* io = iframe ? iframe + (long long)(g.y0 + r) * c.dpitch_h + (long long)(g.x0 + col) * 3 : nullptr;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (io) io[ch] = gi[ch];
        acc[ch] = fmaf(gi[ch], slope_lds[px[ch] * 3 + ch], acc[ch]);
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v = acc[ch];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) wsum[(tid >> 6) * 3 + ch] = v;
  }
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kCodecThreads / 64; ++w) s += wsum[w * 3 + tid];
    p.partials[(kt * p.max_tiles + blockIdx.x) * 3 + tid] = s;
  }
}

// one thread per (clip, frame, channel): the frame's tiles ascending from +0, then the finishing factor
__global__ __launch_bounds__(256) void codec_grad_finish(const CodecGradLaunch p, const float* scale, int T_out, int n3, bool s420, float* gdelta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n3) return;
  const int kt = i / 3, ch = i - kt * 3;
  const CodecClipDev& c = p.clip[kt / T_out];
  const int M = s420 ? 16 : 8, TH = s420 ? 64 : 32;
  const int ntiles = c.ntx * (((c.Hs + M - 1) / M * M + TH - 1) / TH);
  float s = 0.f;
  for (int b = 0; b < ntiles; ++b) s += p.partials[((size_t)kt * p.max_tiles + b) * 3 + ch];
  const float sc = scale[i];
  gdelta[i] = sc == 0.f ? 0.f : s * sc;
}

}  // namespace

// the tiles of the largest frame of a call: what partials holds per (clip, frame); 0 where the arguments are not a launch's
long long flk_codec_grad_tiles_host(const flk_codec_args* a) {
  if (!a || !a->clips || a->nclip < 1 || (a->subsampling != FLK_CODEC_420 && a->subsampling != FLK_CODEC_444)) return 0;
  const bool s420 = a->subsampling == FLK_CODEC_420;
  long long max_tiles = 0;
  for (int i = 0; i < a->nclip; ++i) {
    const flk_codec_clip& s = a->clips[i];
    if (s.Hs < 1 || s.Ws < 1) return 0;
    const long long ntx = (padded(s.Ws, s420) + kTW - 1) / kTW, TH = s420 ? 64 : 32;
    max_tiles = max_of(max_tiles, ntx * ((padded(s.Hs, s420) + TH - 1) / TH));
  }
  return max_tiles;
}

// arguments already validated (api.cpp: flk_codec_grad); everything here up to the first launch is host arithmetic.  Clip k's images
// lie in g_out (and g_in) behind those of the clips before it, [T_out][Hs][Ws][3] fp32 each
int flk_codec_grad_launch(const flk_codec_args* a, const int32_t* frame_idx, int T_out, const uint8_t* tone, int mode, const float* g_out,
                          const float* slope, const float* scale, float* gdelta, float* g_in, float* partials, hipStream_t stream) {
  CodecGradLaunch p;
  const bool s420 = a->subsampling == FLK_CODEC_420;
  p.idx = frame_idx; p.tone = tone; p.slope = slope; p.partials = partials; p.g_out = g_out; p.g_in = g_in; p.mode = mode;
  fill_quant(a->quality, p.q);
  long long max_tiles = 1, off = 0;
  for (int i = 0; i < a->nclip; ++i) {
    const flk_codec_clip& s = a->clips[i];
    max_tiles = max_of(max_tiles, fill_clip(p.clip[i], s, 0, s.T, s420));
    p.clip[i].dst = (uint8_t*)(g_out + off);
    p.clip[i].dpitch_h = s.Ws * 3;
    p.clip[i].dpitch_t = (long long)s.Hs * s.Ws * 3;
    off += (long long)T_out * s.Hs * s.Ws * 3;
  }
  FLK_REQUIRE(max_tiles <= 0x7fffffffLL, "flk_codec_grad: a frame of more than 2^31 tiles");
  p.max_tiles = (int)max_tiles;
  const dim3 grid((unsigned)max_tiles, (unsigned)T_out, (unsigned)a->nclip);
  if (s420) {
    static bool done[FLK_MAX_DEVICES];
    if (int rc = flk_raise_lds_limit((const void*)codec_grad_kernel<true>, CodecGradLds<true>::bytes, done)) return rc;
    FLK_LAUNCH_KERNEL(codec_grad_kernel<true>, grid, dim3(kCodecThreads), CodecGradLds<true>::bytes, stream, p);
  } else {
    static bool done[FLK_MAX_DEVICES];
    if (int rc = flk_raise_lds_limit((const void*)codec_grad_kernel<false>, CodecGradLds<false>::bytes, done)) return rc;
    FLK_LAUNCH_KERNEL(codec_grad_kernel<false>, grid, dim3(kCodecThreads), CodecGradLds<false>::bytes, stream, p);
  }
  const int n3 = a->nclip * T_out * 3;
  FLK_LAUNCH_KERNEL(codec_grad_finish, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, stream, p, scale, T_out, n3, s420, gdelta);
  FLK_CHECK_HIP(hipGetLastError());
  return FLK_OK;
}
