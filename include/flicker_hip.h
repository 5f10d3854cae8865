/* flicker_hip.h -- C ABI of libflicker_hip.so (MI355X / gfx950 flickering-attack hot path).
 *
 * The reference (roiponytch/Flickering_Adversarial_Video) has no FFI / operator layer: its hot path is
 * framework ops (TF-1.15 Conv3D / MaxPool3D / ... and torch-1.4 aten::conv3d / ...) reached from
 * Python objects.  This header is the boundary a maintainer binds instead; every
 * entry point cites the reference code it replaces.  See INTEGRATION.md for the ctypes binding.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every function returns 0 (FLK_OK) or a negative
 *     FLK_E* code; flk_last_error() returns a thread-local message for the last failure.
 *   - the CALLER owns every tensor: functions take raw device pointers, PODs and a hipStream_t
 *     (passed as void*); everything is asynchronous on that stream, there are no hidden syncs.
 *   - tensors are channels-last ("NDHWC") as the I3D maths is specified (i3d.py); `ld` is the
 *     channel stride between consecutive positions (>= C), `coff` a channel offset into the buffer
 *     (so Inception branches write slices of one concat buffer -- tf.concat, i3d.py:219, is elided).
 *   - dtype: FLK_F32 = fp32 storage + exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): the parity mode;
 *            FLK_BF16 = bf16 storage + bf16 MFMA with fp32 accumulation: the performance mode.
 *     BN scale/bias, losses, delta, Adam state and all reductions are fp32 in both modes.
 *   - a flk_net is bound to one device and is not thread-safe; distinct nets are independent.
 */
#ifndef FLICKER_HIP_H
#define FLICKER_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FLK_OK 0
#define FLK_EINVAL (-1)   /* bad argument / unsupported shape */
#define FLK_EHIP (-2)     /* a HIP runtime call failed */
#define FLK_ENOMEM (-3)
#define FLK_ESTATE (-4)   /* call order violated (e.g. backward before forward) */

#define FLK_F32 0
#define FLK_BF16 1

int flk_version(void);
const char* flk_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Per-op entry points (kernel-level parity tests call these).
 * ------------------------------------------------------------------------------------------- */

/* Packed weights for one convolution: built once on the host, resident on the device.
 * w_dhwio: fp32 host array [kt][kh][kw][cin][cout] (TF checkpoint layout, i3d.py:61-65).
 * row_scale (optional, len cout for transpose=1): folded into the weights (BN scale for dgrad).
 * transpose=1 builds the data-gradient operator (taps flipped, cin<->cout swapped), i.e. what
 * Conv3DBackpropInputV2 / aten::conv3d backward-input applies.  nf = output-channel fragments per
 * workgroup tile (2, 4 or 8 -> 32/64/128 channels). */
typedef struct flk_conv_weights flk_conv_weights;
int flk_conv_weights_create(const float* w_dhwio, int kt, int kh, int kw, int cin, int cout,
                            const float* row_scale, int transpose, int dtype, int nf,
                            flk_conv_weights** out);
/* Same, for an operator whose INPUT channels come from two tensors (flk_conv_args.in / .in2): channels [0,cin_split)
 * and [cin_split,cin) are each padded to a whole 64-byte slab in the packed K order.  w_dhwio is the plain
 * [kt][kh][kw][cin][cout] array (no transpose option: build the data-gradient operator explicitly). */
int flk_conv_weights_create_split(const float* w_dhwio, int kt, int kh, int kw, int cin, int cout,
                                  const float* row_scale, int cin_split, int dtype, int nf,
                                  flk_conv_weights** out);
/* Launch-layout autotuning (speed only: the arithmetic per output does not depend on the layout).  While switched on
 * (per host thread), every flk_conv3d call with a geometry not seen before times its candidate layouts on its own
 * operands, SYNCHRONISING the stream, and remembers the fastest in the weights object; later calls reuse it.
 * flk_net_autotune runs one forward + backward of a finalized network in that mode. */
int flk_conv_set_autotune(int on);

/* Weights of the folded 7x7x7 / stride-2 I3D stem (Conv3d_1a_7x7, i3d.py:168-170) as a 4x4x4 convolution over the
 * fold_t = 3 space-to-depth clip (flk_perturb_apply_s2d): w_folded is [4,4,4,32,cout] with channel
 * (qt*2+qh)*8 + qw*3 + c.  Tap index 3 of an axis exists for parity 0 only, so whole 8-channel chunks are structurally
 * zero (checked); in bf16 the K loop is assembled from the non-zero chunks only (49 steps instead of 64).  Use with
 * flk_conv3d(kt = kh = kw = 4, cin = 32, stride 1). */
int flk_conv_weights_create_s2d_stem(const float* w_folded, int cout, int dtype, int nf, flk_conv_weights** out);
int flk_conv_weights_destroy(flk_conv_weights* w);

/* Generic 3-D convolution as implicit GEMM on MFMA, LDS-staged T x H x W halo tiles.
 * Replaces snt.Conv3D + snt.BatchNorm(inference) + relu (Unit3D, i3d.py:51-71) and, with a
 * transposed weight set, Conv3DBackpropInputV2 + ReluGrad; also aten::conv3d(+BatchNorm3d+ReLU
 * +residual) of torchvision VideoResNet (model.py:421).
 *   out[pos, coff_out + n] = epilogue( sum_{tap,c} in[pos*stride - pad + tap, coff_in + c] * W )
 *   epilogue: v = acc*scale[n] + bias[n];  v += add[pos,n];  relu;  v = mask[pos,n] > 0 ? v : 0
 * (each stage optional).  Logical output grid (To,Ho,Wo) maps to physical output positions
 * o*ostride + ooffset inside (OT,OH,OW): stride-1 everywhere except the parity-decomposed
 * data-gradient of strided convolutions. */
typedef struct {
  const void* in; int in_ld, in_coff, cin;
  int B, Ti, Hi, Wi;
  int kt, kh, kw;          /* tap box */
  int st, sh, sw;          /* input step per logical output step */
  int pt, ph, pw;          /* padding BEFORE (TF SAME puts the extra pad after, i3d.py:64) */
  int To, Ho, Wo;          /* logical output grid */
  void* out; int out_ld, out_coff, cout;
  int OT, OH, OW;          /* physical output dims */
  int ost, osh, osw, oot, ooh, oow;
  const float* scale; const float* bias;       /* per output channel or NULL */
  const void* add; int add_ld, add_coff;       /* NULL or tensor with the physical output geometry */
  const void* mask; int mask_ld, mask_coff;    /* NULL or tensor with the physical output geometry */
  int relu;
  /* optional second segments (fused Inception 1x1x1 convolutions: i3d.py:197-207 share one input):
   * in2 != NULL : input channels [cin1, cin) are read from in2[:, in2_coff + (c - cin1)] (weights packed with
   *               flk_conv_weights_create_split(cin_split = cin1));
   * out2 != NULL: output channels [cout1, cout) are written to out2[:, out2_coff + (n - cout1)] (cout1 % 8 == 0). */
  const void* in2; int in2_ld, in2_coff, cin1;
  void* out2; int out2_ld, out2_coff, cout1;
  /* optional position-class bias (the exact perturbation path of the I3D stem, flk_stem_delta_bias): fp32 [To][4][4][cout], added
   * after scale / bias; row = (ot, class(oh), class(ow)) with class(o) = 0 for o == 0, 2 for o == n-2, 3 for o == n-1, else 1 */
  const float* pos_bias;
  /* optional workspace for deterministic split-K (launches with too few output tiles to fill the chip: the input-channel slabs are
   * divided over up to 8 slices, each writes fp32 partial sums here, a second launch adds them in slice order and runs the
   * epilogue -- bitwise reproducible).  NULL: never split.  Size: flk_conv_splitk_bytes (0 = this convolution is never split).
   * Two convolutions that may run concurrently need separate workspaces. */
  void* splitk_ws; int64_t splitk_ws_bytes;
  int64_t pos_bias_bstride;  /* elements between the position-class tables of consecutive clips (per-clip perturbations); 0: one table */
} flk_conv_args;
int flk_conv3d(const flk_conv_args* a, const flk_conv_weights* w, int dtype, void* stream);
int64_t flk_conv_splitk_bytes(const flk_conv_args* a, const flk_conv_weights* w);
/* n <= 3 multi-tap convolutions in ONE grid (bf16): an Inception block's Branch_1 and Branch_2 3x3x3 units (i3d.py:201-209), forward or
 * data-gradient, which the reference's graph runs as independent ops.  Member i is computed exactly as flk_conv3d(a[i], w[i]) would with
 * direct-A weights and (w[i]'s nf) / nfw waves along the channels -- bitwise the same outputs -- but its workgroups share the launch: no
 * second stream, no fork / join, and the short member fills the tail of the long one.  nfw (2 or 4) = channel fragments per wave, the
 * one template argument the members share; every w[i] must have been packed with nf in {nfw, 2 nfw, 4 nfw}.  ring != 0: the members
 * take the LDS weight ring instead (the large launches' path): all packed with nf == nfw (4 or 8), 256-row tiles.  Longest K loops first. */
int flk_conv3d_group(const flk_conv_args* const* a, const flk_conv_weights* const* w, int n, int nfw, int ring, int dtype, void* stream);
/* n <= 3 convolutions of 3x3x3 or 1x3x3 taps, stride 1, bf16, weights packed with nf = 4 (i3d.py:183-186 Conv3d_2c_3x3; 200-209 / 229-238
 * Branch_1 and Branch_2 of the Mixed_3* blocks; the 3x3x3 layers of r3d_18 / mc3_18 and the (1,3,3) spatial halves of r2plus1d_18's layer1
 * units; forward and data-gradient) in ONE persistent launch with wave-specialised producers (csrc/conv_pc.hip: one 512-thread workgroup per
 * CU; four consumer waves that only read fragments and issue MFMAs, two waves streaming the weights by LDS-DMA, two staging the next halo).
 * Bitwise the outputs of flk_conv3d.  Members in the order given, longest K loops first.
 * flk_conv3d_pc_why_not: NULL when flk_conv3d_pc takes the convolution, else the reason (a static string). */
int flk_conv3d_pc(const flk_conv_args* const* a, const flk_conv_weights* const* w, int n, int dtype, void* stream);
const char* flk_conv3d_pc_why_not(const flk_conv_args* a, const flk_conv_weights* w, int dtype);
/* 1 when flk_conv3d / flk_conv3d_group send these convolutions to flk_conv3d_pc: eligible, plannable, a modelled efficiency (useful share of
 * busiest workgroup x workgroups) >= 0.65 and a busiest workgroup of >= 150 K steps; the environment variables FLK_PC_MIN_EFF / FLK_PC_MIN_STEPS
 * override the two bounds (read once).  0 otherwise; never sets flk_last_error. */
int flk_conv3d_pc_worthwhile(const flk_conv_args* const* a, const flk_conv_weights* const* w, int n, int dtype);
/* the same decision from the geometries alone (no weights, no device), with the launch behind it: member 0's tile (tile3[3] = Tt, Ht, Wt), the
 * position fragments per consumer wave, the modelled efficiency and the K steps of the busiest workgroup; returns 1 / 0 or a negative FLK_E* */
int flk_conv3d_pc_query(const flk_conv_args* const* a, int n, int dtype, int* tile3, int* ni, double* eff, double* steps);
/* the validation and planning of flk_conv3d_group without the launch (FLK_OK / the error the launch would return): plan builders call it
 * once per group when the plan is built */
int flk_conv3d_group_check(const flk_conv_args* const* a, const flk_conv_weights* const* w, int n, int nfw, int ring, int dtype);
/* the (waves along the channels, weight path: 0 LDS ring / 5 LDS ring with the weights a row of taps ahead / 1 direct A / ...) flk_conv3d's heuristics choose for this geometry when the
 * weights are packed at `nf` (force_da: -1 heuristic, 0 ring, 1 direct A): lets a plan builder pick the packing of a grouped launch's
 * members before any weights exist.  No device work. */
int flk_conv_layout_query(const flk_conv_args* a, int nf, int dtype, int force_da, int* wn_out, int* mode_out);
/* Everything the planner decides for one launch, from the geometry and the packing alone (no weights, no device work): the plan of
 * flk_conv3d(a, weights packed at nf / dtype) under a requested layout.  route: 0 the halo kernel (conv_igemm_kernel), 1 the LDS-DMA ring
 * over whole-T tiles (conv_t3_dma_kernel), 2 its form with 16-frame temporal tiles, 3 the 1x1x1 LDS-DMA ring (conv1x1_dma_kernel).  mode is
 * the planner's weight path (0 ring, 1 direct A, 2 direct A of a 1x1x1, 3 ring of a 1x1x1, 4 folded stem, 5 ring with the weights a row of
 * taps ahead), template_mode the MODE argument of the conv_igemm_kernel instance the dispatch launches (planner mode 5 runs template 6, the
 * ring write behind the barrier, on tiles of at most 64 channels); both describe the halo kernel and are what a forced halo launch would
 * take when route != 0.  nf / wn: channel fragments of the workgroup tile and waves along the channels as they will really run (a request
 * the planner clamps -- direct A on 96-channel tiles, more waves than the tile has fragment pairs -- is reported clamped).  ksplit: split-K
 * slices (1 = none); tile / rows / halo: output positions per workgroup and the cells of its input halo; wgs: workgroups. */
typedef struct {
  int route, nf, wn, mode, template_mode, ksplit;
  int Tt, Ht, Wt, rows, halo;
  int64_t wgs;
} flk_conv_plan_info;
/* stem4: the folded-stem packing (flk_conv_weights_create_s2d_stem; bf16 packs K steps, fp32 is the generic 4x4x4 packing); cin_split: 0 or
 * the first segment's channels of a two-segment packing (a->in2 / a->cin1 must agree); wn / da: the requested layout (0 / -1 = heuristic,
 * wn 1 / 2 / 4 waves along the channels, da 0 LDS ring / 1 direct A); splitk: plan as if a->splitk_ws were given (!= 0) or not (0). */
int flk_conv_plan_query(const flk_conv_args* a, int nf, int dtype, int stem4, int cin_split, int wn, int da, int splitk, flk_conv_plan_info* out);
/* the same for flk_conv3d_group(a, weights packed at nf[i], n, nfw, ring): members[i] as group_plan plans member i, *body_mode the MODE
 * argument of the conv_igemm_group_kernel<NFW = nfw, MODE> instance (1 direct A; ring groups: 0, or 5 / 6 when EVERY member is planned
 * for the row-ahead ring) */
int flk_conv_group_plan_query(const flk_conv_args* const* a, const int* nf, int n, int nfw, int ring, int dtype, int* body_mode,
                              flk_conv_plan_info* members);
/* the layouts {wn, da} the autotuner times for weights packed at nf / dtype, in its order, the heuristic {0, -1} first (the folded stem is
 * never tuned: that one only); at most cap are written, the count is returned */
int flk_conv_layout_candidates(int nf, int dtype, int stem4, int* wn, int* da, int cap);
/* flk_conv3d with the layout {wn, da} given by the caller: exactly the launch the autotuner times for that candidate and a tuned entry
 * replays (not the producer / consumer kernel; {0, -1} is the heuristic's own launch, every other layout runs the halo kernel).  A
 * layout that is not in flk_conv_layout_candidates for these weights is refused (FLK_EINVAL) before anything is launched. */
int flk_conv3d_layout(const flk_conv_args* a, const flk_conv_weights* w, int dtype, int wn, int da, void* stream);

/* tf.nn.max_pool3d SAME (i3d.py:174,189,212,252,398): padded cells never win; argmax = FIRST
 * maximum in (t,h,w) scan order (strict >), stored as a uint8 window index (tap = (dt*kh + dh)*kw + dw) for the backward pass.
 * Values are compared as numbers: -0.0 and +0.0 tie and the first of them wins; a window that holds only -inf records tap 0 and
 * out = -inf.  One deviation: the bf16 kernels of the 3x3x3 / 1 window order values by an integer key in which +0.0 ranks above -0.0,
 * so among tied zeros of both signs they record the first +0.0 (still an in-bounds cell whose value equals the window maximum).  in / out / gout / gin / mask are channel slices
 * [coff, coff + C) of rows ld channels wide (all multiples of 8); channels outside a slice are never written.
 * MaxPool3DGrad: the strided I3D windows (1x3x3 / 1x2x2, 3x3x3 / 2, 2x2x2 / 2) take an owner form in both dtypes (every cell written
 * once, fixed order).  Every other geometry: fp32 takes a gather form (fixed summation order, bitwise reproducible); bf16 takes an
 * LDS scatter that sums in 32-bit fixed point with integer atomics (order-independent, bitwise reproducible as well).  Its scale is
 * 2^E / 2^floor(log2 max|gout|) per workgroup with E = min(24, 30 - ceil(log2 n)), n = ceil(kt/st) * ceil(kh/sh) * ceil(kw/sw) the
 * number of windows that can cover one cell (E = 24 for n <= 64: every I3D pool), so n addends never leave an int32 for any
 * accepted window (<= 255 taps); the sum of a cell is within n * 2^-(E+1) * max|gout| of exact before its one rounding to bf16.
 * A gradient that a -inf window sends to a padded cell is dropped.  Optional relu-mask like flk_conv3d.  There is no environment
 * switch between the forms. */
typedef struct {
  const void* in; int in_ld, in_coff; int C;
  int B, Ti, Hi, Wi;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  int To, Ho, Wo;
  void* out; int out_ld, out_coff;
  uint8_t* idx;            /* [B,To,Ho,Wo,C]; 255 = "no cell" */
  int relu_input;          /* forward only.  1: the input is a ReLU output whose gradient is masked by (input > 0)
                              anyway -> windows whose maximum is <= 0 record "no cell", so the backward pass needs no
                              mask tensor (pass mask = NULL): identical result, ~40 % less traffic */
} flk_pool_args;
int flk_maxpool3d_fwd(const flk_pool_args* a, int dtype, void* stream);
/* gin[pos,c] = sum_{windows containing pos with argmax == pos} gout[window,c];
 * then masked by mask[pos,c] > 0 if mask != NULL.  a->in/out describe the FORWARD tensors'
 * geometry: gout has the `out` geometry (ld/coff given here), gin the `in` geometry. */
int flk_maxpool3d_bwd(const flk_pool_args* a, const void* gout, int gout_ld, int gout_coff,
                      void* gin, int gin_ld, int gin_coff,
                      const void* mask, int mask_ld, int mask_coff, int dtype, void* stream);

/* Branch_3 backward of an Inception block in ONE kernel (i3d.py:211-216 backward; bf16 only): the data-gradient of the 1x1x1 unit that
 * follows the stride-1 3x3x3 max-pool is computed on MFMA inside the pool's scatter backward,
 *   gin[cell, c] = sum_{windows w whose saved argmax for channel c is cell} ( sum_k g[w, k] * Wt[k, c] ),
 * instead of flk_conv3d (transposed 1x1x1) -> HBM -> flk_maxpool3d_bwd.  `a` describes the FORWARD pool (a->C = C channels, a->idx its
 * argmax bytes); g: [B,To,Ho,Wo,g_ld] gradient of the unit's pre-ReLU output (K = 32, 64, 96 or 128 channels at g_coff); wpack: from
 * flk_pool_gemm_weights_create(Wt [K][C] = unit weight transposed x batch-norm scale).  Products stay in fp32 (no bf16 rounding of the
 * intermediate), the scatter sums in 32-bit fixed point like flk_maxpool3d_bwd (same window-dependent exponent E, any window the pool
 * accepts; FLK_POOL_GEMM_REG=0 selects the loop form where the register form would run): bitwise reproducible. */
int flk_pool_gemm_weights_create(const float* wt_kc, int K, int C, void** out_dev);
int flk_pool_gemm_weights_destroy(void* dev);
int flk_maxpool3d_bwd_gemm(const flk_pool_args* a, const void* g, int g_ld, int g_coff, int K, const void* wpack,
                           void* gin, int gin_ld, int gin_coff, int dtype, void* stream);

/* MaxPool3d_2a_3x3 with Conv3d_2b_1x1 inside (i3d.py:174-180), one kernel per pass, bf16 only.  The pooled map and its gradient each have
 * one consumer -- the 1x1x1 unit and its data-gradient -- so run inside the pool kernels neither crosses HBM.
 *
 * flk_maxpool3d_conv1x1_eligible: host-only (no device work, never sets flk_last_error).  1 when the two entry points below take the pair:
 * dtype bf16; window (1,3,3), stride (1,2,2) over even H and W (SAME pad-before 0) and passing the owner-form backward's conditions;
 * a->C == cin == cout == 64 (exactly two 32-channel slabs); has_mask == 0 (the unit's data-gradient carries no ReLU mask: the pooled map
 * is not a ReLU output).  0 otherwise.  Only the geometry fields of `a` are read.
 *
 * flk_maxpool3d_fwd_conv1x1: out[pos, out_coff + n] = epilogue(sum_c maxpool(in)[pos, c] * W[c, n]) with flk_conv3d's epilogue
 * (scale, bias, relu; each optional); a->idx receives the argmax bytes.  w: the unit's forward weights (flk_conv_weights_create, 1x1x1,
 * 64 -> 64, nf 2 or 4).  write_pool != 0: the pooled map is also written to a->out (else a->out is not touched and may be NULL).
 * out and idx -- and a->out where written -- are BITWISE what flk_maxpool3d_fwd followed by flk_conv3d write.
 *
 * flk_maxpool3d_bwd_conv1x1: gin = MaxPool3DGrad(idx, Gp) with Gp[pos, c] = bf16(sum_k g[pos, g_coff + k] * Wb[k, c]); wb: the unit's
 * data-gradient weights (transpose = 1, batch-norm scale folded in).  gpool != NULL: Gp is also written there.  gin -- and gpool -- are
 * BITWISE what flk_conv3d (data-gradient, no mask) followed by flk_maxpool3d_bwd write.  No atomics, every cell written once.
 *
 * Both entry points return FLK_EINVAL with the reason for anything the query refuses. */
int flk_maxpool3d_conv1x1_eligible(const flk_pool_args* a, int cin, int cout, int has_mask, int dtype);
int flk_maxpool3d_fwd_conv1x1(const flk_pool_args* a, const flk_conv_weights* w, const float* scale, const float* bias, int relu,
                              void* out, int out_ld, int out_coff, int write_pool, int dtype, void* stream);
int flk_maxpool3d_bwd_conv1x1(const flk_pool_args* a, const void* g, int g_ld, int g_coff, const flk_conv_weights* wb,
                              void* gin, int gin_ld, int gin_coff, void* gpool, int gpool_ld, int gpool_coff, int dtype, void* stream);

/* Perturbation apply fused with the stem's space-to-depth staging.
 * kinetics_i3d_utils.py:100-142:  x_adv = clip(x + a * clip(delta[t,c], +-dclip), lo, hi)
 * model.py:80-101 (torch dialect): same with delta/std[c] and scalar clamp bounds.
 * x: uint8 (x = u8*x_scale + x_bias, the TFRecord path pre_process_rgb_flow.py:226-234, or x = x_lut[u8][c]) or fp32,
 *    [B,T,H,W,3]; delta: fp32 [T,3] (flicker), [T,H,W,3] (dense, "L12" baseline) or [Bd,T,H,3] (per line: delta_per_line).
 * out: [B,T/2,H/2,W/2,32] of dtype: channel (qt*4+qh*2+qw)*3+c, channels 24..31 zero -- the
 * 7x7x7/2 stem (i3d.py:169) then runs as a 4x4x4/1 convolution on MFMA.  T,H,W must be even.
 * Pointer contract (flk_perturb_apply_s2d and flk_perturb_grad_reduce; FLK_EINVAL naming the alignment, before any GPU call): a uint8
 * clip x is 2-byte aligned and an fp32 clip 8-byte aligned (the kernels read a pixel pair at a time); out and gx_s2d are 16-byte
 * aligned.  A uint8 clip that is not 8-byte aligned is served by the generic kernels instead of the 8-byte-load fast paths (fold_t 2 / 3
 * flicker, fold_t 4 with x_lut): same bits, more load instructions.  delta, gdelta, partials and the tables are read and written
 * one float at a time (4-byte aligned, as any float array is). */
typedef struct {
  const void* x; int x_is_u8; float x_scale, x_bias;
  const float* delta; int delta_dense;
  float dclip;               /* 0.4 (TF) or dynamic_max_norm (torch); <=0 disables */
  float inv_std[3];          /* 1 (TF) or 1/DEFAULT_STD (torch) */
  float lo, hi;              /* -1,1 (TF) or -1.73488, 2.49020 (torch) */
  float adv_flag;            /* 0 -> clean input */
  int shift_x, shift_p;      /* cyclic temporal rolls (kinetics_i3d_utils.py:115-137), 0 = off */
  int B, T, H, W;
  int fold_t;                /* 0/2: fold (t,h,w) parities -> [B,T/2,H/2,W/2,32], channel (qt*4+qh*2+qw)*3+c, 24..31 zero
                                (I3D stem, stride 2x2x2);
                                3: the same fold with chunk-aligned channels (qt*2+qh)*8 + qw*3+c, 6 and 7 of every 8
                                zero (one (qt,qh) parity per 16-byte chunk: flk_conv_weights_create_s2d_stem);
                                1: fold (h,w) only -> [B,T,H/2,W/2,16], channel (qh*2+qw)*3+c, 12..15 zero
                                (VideoResNet stems, stride 1x2x2);
                                4 (bf16 output only): the fold of 1 with every value as TWO bf16 numbers -> [B,T,H/2,W/2,32]: channel k =
                                bf16(x_adv), channel 16 + k = bf16(x_adv - channel k) -- the input of the VideoResNet stems in bf16
                                plans (both halves against the same weights: the perturbed clip to ~16 bits at no extra MFMA work;
                                one bf16 per value swallows |delta| < 1e-3 / std).  Gradients come back in the layout of 1. */
  int center;                /* 1 (flicker delta only): write x' = x_adv - a*p' instead of x_adv, i.e. the CLEAN value wherever the
                                clip is inactive (exactly representable in bf16 for uint8 clips) -- the perturbation then reaches the stem
                                through flk_conv_args.pos_bias in fp32 (flk_stem_delta_bias) instead of being rounded away with the
                                bf16 input: |delta| < 2^-9 is below half a bf16 ulp of a pixel value near +-1 */
  int delta_per_clip;        /* 1 (flicker delta only): delta is [B,T,3] and clip b is perturbed by ITS OWN delta[b] -- B independent
                                single-video attacks (i3d_adversarial_main_single_video_npy.py:103-337, model.py:791-982) advancing in
                                one batch; the delta-gradient then comes back per clip, [B,T,3].  0: one delta [T,3] shared by the batch */
  int delta_per_line;        /* 1 (VideoResNet layouts, fold_t 1 and 4, and flk_adv_export_u8): the perturbation has one value PER LINE of a frame --
                                delta is fp32 [Bd,T,H,3], Bd = B with delta_per_clip, else 1 -- what a rolling-shutter camera records of a
                                flickering emitter (flk_flicker_lines_mix makes it).  The value added at (b,t,h,w,c) is that of
                                (b or 0, (t - shift_p) mod T, h, c), through the same clamp (dclip / dclip_dev) and 1/std as any other value.
                                flk_adv_export_u8 with delta_T = P (Bd = 1): delta is [P,H,3], frame t takes row (t - shift_p) mod P.
                                flk_perturb_grad_reduce (with delta_per_clip only): gdelta comes back fp32 [B,T,H,3], entry (b,ts,h,c) the
                                masked sum of the input gradient over w ONLY (one wave per (b, t, row pair), lanes stride over W/2, sums
                                added per lane in ascending w, then the 64 lanes folded by a fixed shuffle tree: no atomics, one fixed
                                order; `partials` is not used), times adv_flag * inv_std[c], zero where that delta value lies outside its clamp.
                                FLK_EINVAL before any GPU call: with delta_dense or center = 1; fold_t 0, 2, 3; the gradient without
                                delta_per_clip; delta_T with delta_per_clip; every I3D-only entry point (flk_stem_fwd_u8, flk_stem_delta_grad*,
                                flk_stem_delta_bias, flk_net_backward_delta).  0: today's behaviour, bit for bit.  (The field fills the four
                                bytes of padding behind delta_per_clip: no other field moves, the struct keeps its size, and a
                                zero-initialised struct keeps its meaning) */
  const float* dclip_dev;    /* delta_per_clip only, or NULL: per-clip clamp bounds [B] on the device replacing `dclip` -- the torch loop grows a
                                video's bound by 1.3 when it restarts (model.py:1061-1066), independently per video */
  const float* q_lut;        /* NULL = off.  Quantised apply (8-bit straight-through): fp32 [256][3] on the device, byte v of channel c decodes
                                to q_lut[v * 3 + c].  Every value flk_perturb_apply_s2d writes becomes the value the STORED video holds:
                                  x_adv = the value written today (center = 0);   q = the encode of flk_export_args on x_adv with q_mul[c],
                                  q_add[c], q_levels (the same device function: each operation rounded on its own, half to even,
                                  saturating, NaN -> 0);   x_q = q_lut[q * 3 + c]
                                and x_q goes through the fold, the bf16 rounding and the split of fold_t = 4 as x_adv does, whatever adv_flag
                                is.  So a quantised apply is, bit for bit, the clean apply (adv_flag = 0, lo = -inf, hi = +inf: what a clean
                                forward uses) of the bytes flk_adv_export_u8 writes for the same arguments, decoded through x_lut = q_lut
                                (TF: x_scale / x_bias).  x_q is NOT clamped again: a value the clamp holds at lo or hi is stored as the
                                level nearest the bound (the torch dialect's bounds are byte values of one channel only), and the stored
                                video decodes to that level, up to half a level outside [lo, hi].
                                FLK_EINVAL before any GPU call with center != 0 or q_levels <= 0.  Of the I3D-only entry points
                                flk_stem_fwd_u8 takes it in the TF dialect (its quantised instantiation: see there) and the others
                                refuse it as they refuse x_lut -- flk_net_forward_apply / flk_net_backward_delta route such arguments
                                themselves.  flk_adv_export_u8 ignores the four fields: it already is the quantiser.
                                Gradient: the straight-through estimator d(x_q)/d(u) := 1[lo <= u <= hi], u = x + a p' -- exactly the mask
                                flk_perturb_grad_reduce computes from x, delta and the clamp bounds; its kernels do not read the four
                                fields and give the same bits with and without them.  (The four fields sit in front of x_lut, which
                                stays the struct's last field; a zero-initialised struct keeps its meaning) */
  float q_mul[3], q_add[3], q_levels;   /* the encode of flk_export_args: mul, add, levels (torch: std, mean, 255; TF: 1, 1, 128) */
  const float* x_lut;        /* uint8 x only, or NULL: per-channel decode table fp32 [256][3] on the device, x = x_lut[u8 * 3 + c], replacing
                                x_scale / x_bias -- the VideoResNet decode (u8 / 255 - mean[c]) / std[c] (dataset.py:28-29), whose float32
                                value no scalar multiply-add reproduces bit for bit (videoresnet_spec.u8_decode_table).  Refused with
                                center = 1 and by the I3D-only entry points (flk_stem_fwd_u8, flk_stem_delta_grad*, flk_stem_delta_bias) */
} flk_apply_args;
int flk_perturb_apply_s2d(const flk_apply_args* a, void* out, int dtype, void* stream);

/* The adversarial clip as 8-bit frames: what a file or a display can hold (model.py:103-112 de-normalises the perturbed clip to [0,1]
 * on the host; a video is that times 255, rounded).  Per value of x_adv -- the value flk_perturb_apply_s2d writes in fp32, computed by
 * the same device functions: every source form (uint8 through x_lut or x_scale / x_bias, fp32), flicker / per-clip / dense delta, dclip
 * and dclip_dev, shift_x and shift_p, adv_flag, lo and hi -- each operation rounded separately (no contraction):
 *   y = x_adv * mul[c] + add[c];   z = y * levels;   q = z >= 0 ? min(rint(z), 255) : 0        (rint: half to even; NaN -> 0)
 * torch dialect: mul = std, add = mean, levels = 255 (inverse of (u8/255 - mean)/std); TF dialect: mul = 1, add = 1, levels = 128
 * (inverse of u8/128 - 1).  out: uint8 [B,T,H,W,3], plain layout; clip b at out + (out_clip_offset + b) * out_clip_stride BYTES, so a
 * call can fill rows of a batch buffer.  a->fold_t and a->q_lut / q_mul / q_add / q_levels are ignored (this IS the quantiser: the encode
 * is e's), a->center must be 0, T, H and W may be any positive numbers.  One
 * launch, no allocation, no synchronisation; 4-byte stores wherever the destination is aligned, bytes at the heads and tails of a
 * frame; the result does not depend on the launch geometry.
 * delta_T (0: a->T; flicker delta [delta_T,3] only): frame t takes row (t - shift_p) mod delta_T -- a universal flicker of period
 * delta_T laid over a clip or a whole video of any length, at its own resolution.
 * stats (NULL, or int32 [B][T][3][4], zeroed here by one hipMemsetAsync): per (clip, frame, channel) the sums over the frame of
 * q - q_clean, |q - q_clean|, [q != q_clean] and [the lo / hi clamp was active], q_clean = the source byte (uint8 x) or the encoding
 * of the unperturbed x (fp32 x).  Integer sums: exact in any order.  Entry 0 / (H*W) is the flicker the frames carry, in levels.
 * FLK_EINVAL before any GPU call: null a / e / x / delta / out, non-positive sizes, center != 0, levels <= 0, out_clip_stride smaller
 * than a clip, delta_T with a dense or per-clip delta, stats with H*W > 8388607 (255*H*W must fit an int32). */
typedef struct {
  float mul[3], add[3];
  float levels;
  int delta_T;
  int64_t out_clip_offset;   /* first clip row of `out` written */
  int64_t out_clip_stride;   /* bytes between clip rows of `out` (>= T*H*W*3) */
} flk_export_args;
int flk_adv_export_u8(const flk_apply_args* a, const flk_export_args* e, uint8_t* out, int32_t* stats, void* stream);

/* d(loss)/d(delta): reduce the stem's input gradient (space-to-depth layout, from flk_conv3d) over
 * (B,H,W) with the clip masks of flk_perturb_apply_s2d.  gdelta: fp32 [T,3]
 * (flicker; deterministic two-stage reduction) or [T,H,W,3] (dense).  `partials` is caller scratch
 * of flk_perturb_grad_scratch_bytes(). */
int64_t flk_perturb_grad_scratch_bytes(int B, int T, int H, int W);
int flk_perturb_grad_reduce(const flk_apply_args* a, const void* gx_s2d, int dtype,
                            float* gdelta, float* partials, void* stream);

/* Flicker on VIDEO time: a shared flicker perturbation delta [P,3] of period P (independent of the clip length T) laid over clips
 * whose frames name their rows.  rows: DEVICE int32 [n], n = B*T clip-major -- rows[b*T + t] is the row of delta that frame t of clip b
 * carries; for a clip cut from a video it is (frame number - phase) mod P, the rule flk_adv_export_u8 applies to a whole video with
 * delta_T = P and shift_p = phase (videoresnet_spec.flicker_rows states it on the host).  Both kernels feed the per-clip-delta path the
 * apply, export and gradient kernels already have (flk_apply_args.delta_per_clip); none of those kernels knows about the table.
 *   flk_flicker_rows_gather: delta_clip[i][c] = delta[rows[i]][c], fp32 [n][3] -- RAW values: the clamp and 1/std stay in the apply.  A
 *     row outside [0,P) is clamped into it (wrong data, never a wild read: the rule of flk_clip_prepare_sampled).
 *   flk_flicker_rows_grad:   g_rows[r][c] = sum of g_clip[i][c] over the i with rows[i] == r, fp32 [P][3], added in ASCENDING i starting
 *     from +0; a row no frame carries is written as 0 and an entry of rows outside [0,P) contributes nothing.  g_clip [n][3] is what
 *     flk_perturb_grad_reduce writes with the per-clip arguments the clips were applied with: its stage 2 has applied adv_flag, 1/std
 *     and the delta-clamp mask per (b,t) already, which is right here because all frames that share a row share its delta value.
 *     Every element of g_rows is written exactly once, by one thread; no atomics; the table is staged in LDS in pieces.
 * One launch each, no allocation, no synchronisation; the results do not depend on the launch geometry.
 * FLK_EINVAL before any GPU call: null pointers, n < 1, P outside 1..682 (3*P values are what flk_perturb_reg_adam holds). */
int flk_flicker_rows_gather(const float* delta, int P, const int32_t* rows, int n, float* delta_clip, void* stream);
int flk_flicker_rows_grad(const float* g_clip, const int32_t* rows, int n, int P, float* g_rows, void* stream);

/* Capture channel: the flicker as a CAMERA records it.  Frame i integrates the emitter over an exposure window that starts a sub-frame
 * phase after its own row, so it records a convex mix of K = 1..4 consecutive rows of delta, and the emitter / white balance / ambient
 * light scale each channel by a gain.  Frame i belongs to clip b = i / clip_T (n % clip_T == 0); taps: DEVICE fp32 [n/clip_T][K], one
 * row per clip (videoresnet_spec.capture_taps makes one; rows padded with 0 to a common K); gain: DEVICE fp32 [n/clip_T][3], or null
 * for none.  A linear map at the same seam as the pair above -- the mix in the gather's place, its transpose in the row gradient's:
 *   flk_flicker_rows_mix:      r0 = clamp(rows[i], 0, P-1);  acc = taps[b][0] * delta[r0][c];
 *                              for k = 1 .. K-1: acc = acc + taps[b][k] * delta[(r0 + k) mod P][c];
 *                              delta_clip[i][c] = gain ? gain[b][c] * acc : acc.            RAW values, as the gather's.
 *   flk_flicker_rows_mix_grad: g_rows[r][c] = the sum, from +0, over the frames i ASCENDING and within a frame the taps k ASCENDING with
 *                              (rows[i] + k) mod P == r, of (gain ? gain[b][c] * taps[b][k] : taps[b][k]) * g_clip[i][c].  P < K is legal
 *                              (a frame then reaches one row through two taps: both are added); entries of rows outside [0,P) are
 *                              skipped; a row nothing reaches is written as 0.  One thread per output, no atomics, rows staged in LDS.
 * Every product and every sum is rounded to fp32 on its own (no fused multiply-add), in that one order: videoresnet_spec.flicker_rows_mix
 * and flicker_rows_mix_grad restate both on the host bit for bit.  With K = 1, taps = 1 and gain null or all ones the two launches give the
 * bits of flk_flicker_rows_gather / flk_flicker_rows_grad.  One launch each, no allocation, no synchronisation.
 * FLK_EINVAL before any GPU call: a null delta / g_clip, rows, taps or output, n < 1, clip_T < 1 or n % clip_T != 0, K outside 1..4,
 * P outside 1..682. */
int flk_flicker_rows_mix(const float* delta, int P, const int32_t* rows, int n, int clip_T, const float* taps, int K, const float* gain,
                         float* delta_clip, void* stream);
int flk_flicker_rows_mix_grad(const float* g_clip, const int32_t* rows, int n, int clip_T, const float* taps, int K, const float* gain, int P,
                              float* g_rows, void* stream);

/* Rolling shutter: the capture channel per LINE of a frame.  Line h of a frame of H lines starts its exposure later than line 0, so it
 * has taps of its own (videoresnet_spec.capture_line_taps: the rule of capture_taps with psi_h = phi + (rho * h) / H in phi's place,
 * K = 1..5), and a frame that carries row r records on line h  gain[c] * sum_k w_k(h) * delta[(r + k) mod P][c]: horizontal bands.
 * taps: DEVICE fp32 [n/clip_T][H][K], one table per clip (lines padded with 0 to a common K); gain: DEVICE fp32 [n/clip_T][3] or null.
 *   flk_flicker_lines_mix:      out[i][h][c], fp32 [n][H][3] -- the per-line perturbation flk_apply_args.delta_per_line takes, RAW values.
 *                               One thread per output value; the arithmetic of flk_flicker_rows_mix with the line's taps:
 *                               r0 = clamp(rows[i], 0, P-1);  acc = taps[b][h][0] * delta[r0][c];
 *                               for k = 1 .. K-1: acc = acc + taps[b][h][k] * delta[(r0 + k) mod P][c];   out = gain ? gain[b][c] * acc : acc.
 *   flk_flicker_lines_mix_grad: the transpose, g_lines fp32 [n][H][3] -> g_rows fp32 [P][3], in two launches and ONE fixed order:
 *                               stage 1  s[i][k][c] = the sum, from +0, over the lines h ASCENDING of
 *                                        (gain ? gain[b][c] * taps[b][h][k] : taps[b][h][k]) * g_lines[i][h][c]      (one thread per (i,k,c));
 *                               stage 2  g_rows[r][c] = the sum, from +0, over the frames i ASCENDING and within a frame the taps k ASCENDING
 *                                        with (rows[i] + k) mod P == r, of s[i][k][c] -- the fold of flk_flicker_rows_mix_grad: P < K legal
 *                                        (both taps added), entries of rows outside [0,P) skipped, a row nothing reaches written as 0;
 *                                        one thread per output, rows staged in LDS in pieces.  No atomics.
 *                               scratch: DEVICE fp32 [n][K][3] (s), the caller's.
 * Every product and every sum is rounded to fp32 on its own (no fused multiply-add): videoresnet_spec.flicker_lines_mix and
 * flicker_lines_mix_grad restate both on the host bit for bit.  With the same taps on every line the mix gives the bits of
 * flk_flicker_rows_mix on every line.  No allocation, no synchronisation; the results do not depend on the launch geometry.
 * FLK_EINVAL before any GPU call: a null delta / g_lines, rows, taps, scratch or output, n < 1, clip_T < 1 or n % clip_T != 0, H < 1,
 * K outside 1..5, P outside 1..682. */
int flk_flicker_lines_mix(const float* delta, int P, const int32_t* rows, int n, int clip_T, int H, const float* taps, int K, const float* gain,
                          float* out, void* stream);
int flk_flicker_lines_mix_grad(const float* g_lines, const int32_t* rows, int n, int clip_T, int H, const float* taps, int K, const float* gain,
                               int P, float* scratch, float* g_rows, void* stream);

/* The flicker as SCENE ILLUMINATION (csrc/illum.hip): a second pixel model beside the additive one of flk_perturb_apply_s2d.  A lamp
 * multiplies the linear light of a pixel, the camera then applies its response curve and stores 8 bits; both curves are TABLES, so the
 * kernels equal a numpy float32 restatement bit for bit (videoresnet_spec.illum_apply_host / illum_export_host / illum_grad_host), the
 * slope the gradient uses is exact, and a measured camera curve can be supplied.  Per source byte v of channel c at (b,t,h,w), every
 * product and every sum rounded to fp32 on its own (no fused multiply-add):
 *   m = clamp(delta value of (b, (t - shift_p) mod T, [h], c), +-dclip)     dclip / dclip_dev as flk_apply_args; inv_std is NOT applied:
 *                                                                          m is a relative modulation of the light
 *   L = dec[v * 3 + c]                                                      linear light in [0,1]
 *   s = 1 + adv_flag * m;   p = L * s;   u = min(max(p, 0), 1)
 *   z = u * N;   i = min(int(z), N - 1);   f = z - i;   d = enc[i + 1] - enc[i];   e = enc[i] + f * d       display value in [0,1]
 *   plain:      x_adv = e * out_mul[c] + out_add[c]                         (torch dialect: 1 / std, -mean / std)
 *   quantised:  q = min(rint(e * 255), 255) (NaN -> 0);   x_adv = q_lut[q * 3 + c]      (a->q_lut != NULL; q_mul / q_add / q_levels unused)
 *   export:     the byte q
 * dec: DEVICE fp32 [256][3]; enc: DEVICE fp32 [enc_n + 1], non-decreasing, N = enc_n in 2..16384 (both staged in LDS by every kernel).
 * `a` is read as by the additive entry points, except: lo, hi, x_scale, x_bias, inv_std and the encode fields are not used; the clip is
 * uint8 with x_lut given (x_lut itself is read only by the adv_flag = 0 delegation below); delta is the shared [T,3], the per-clip
 * [B,T,3] or the per-line [Bd,T,H,3] form.
 *   flk_illum_apply_s2d:   x_adv in the layouts of fold_t 1 (fp32 / bf16, 16 channels) and 4 (bf16, hi | lo), as flk_perturb_apply_s2d
 *                          lays out its values; adv_flag == 0 is DELEGATED to flk_perturb_apply_s2d(a): the clean clip, bit for bit.
 *   flk_illum_export_u8:   the bytes q, out / e->out_clip_offset / out_clip_stride / delta_T as flk_adv_export_u8 (T, H, W any positive
 *                          numbers; e->mul / add / levels unused); stats as there with q_clean = the source byte and the fourth sum
 *                          counting the values with p outside [0,1].
 *   flk_illum_grad_reduce: d(loss)/d(m), straight-through under quantisation: per output the sum over its pixels of
 *                          gx * ((d * N) * L) * 1[0 <= p <= 1] (the weight two rounded products, the term a third, terms added in one
 *                          fixed order, fp32, no atomics), then once per output  * adv_flag * out_mul[c], zero where the delta value lies
 *                          outside its clamp.  gx_s2d: the 16-channel gradient of fold_t 1 (also for fold_t 4), fp32 or bf16.  gdelta:
 *                          [T,3], [B,T,3] or (per line, needs delta_per_clip) [B,T,H,3].  partials: scratch of
 *                          flk_perturb_grad_scratch_bytes (unused per line).  The chunking depends on the shapes only, and per clip it
 *                          is the batch-1 call's: a per-clip result equals the batch-1 call on that clip, bit for bit.
 * No allocation, no synchronisation; results do not depend on the launch geometry.
 * FLK_EINVAL before any GPU call, naming the field: null a / m / x / delta / out; an fp32 clip or a null x_lut; center != 0; delta_dense;
 * fold_t other than 1 and 4 (apply and gradient; fold_t 4 writes bf16 only); null dec / enc; enc_n outside 2..16384; dclip_dev without
 * delta_per_clip; the per-line gradient without delta_per_clip; the pointer-alignment contract of flk_perturb_apply_s2d (x 2-byte,
 * out and gx_s2d 16-byte aligned); for the export what flk_adv_export_u8 refuses of the fields it shares. */
typedef struct { const float* dec; const float* enc; int enc_n; float out_mul[3], out_add[3]; } flk_illum_args;
int flk_illum_apply_s2d(const flk_apply_args* a, const flk_illum_args* m, void* out, int dtype, void* stream);
int flk_illum_export_u8(const flk_apply_args* a, const flk_illum_args* m, const flk_export_args* e, uint8_t* out, int32_t* stats, void* stream);
int flk_illum_grad_reduce(const flk_apply_args* a, const flk_illum_args* m, const void* gx_s2d, int dtype, float* gdelta, float* partials,
                          void* stream);

/* Fused form of (stem data-gradient + flk_perturb_grad_reduce) for the flickering perturbation of I3D: d(loss)/d(delta[t,c]) straight
 * from G = d(loss)/d(pre-ReLU output of Conv3d_1a_7x7) (bf16 [B,T/2,H/2,W/2,g_ld], 64 channels) -- replaces Conv3DBackpropInputV2 of
 * i3d.py:169 and the clip_by_value / reduce_sum gradients of kinetics_i3d_utils.py:100-142 with ONE MFMA kernel in the weight-gradient
 * form (csrc/stem_grad.hip): the per-pixel gradient is never materialised.  `a` are the arguments the clip was applied with (its
 * clip / roll / 1/std semantics define the mask); wf_dev comes from flk_stem_delta_grad_weights_create (the canonical
 * [7,7,7,3,64] stem weights x the folded batch-norm scale, fp32); scratch: flk_stem_delta_grad_scratch_bytes() of caller scratch
 * (stage-1 partials + the de-interleaved clip mask, 768 bytes per clip row).  Two launches: the mask pre-pass (HBM-bound;
 * mask_done != 0 skips it when flk_stem_delta_grad_mask already ran for the same arguments) and the GEMM.
 * Deterministic (fixed summation order); bf16 gradients only -- the fp32 parity mode keeps the two-kernel path.
 * Pointer contract (flk_stem_delta_grad and flk_stem_delta_grad_mask; FLK_EINVAL naming the alignment, before any GPU call -- a refused
 * flk_stem_delta_grad launches nothing, not even the mask pre-pass): a uint8 clip x is 4-byte aligned and an fp32 clip 16-byte aligned
 * (the mask pre-pass reads a row of the clip as dwords / float4: stricter than flk_perturb_apply_s2d asks); G, wf_dev and scratch are
 * 16-byte aligned (G and the mask inside the scratch move by 16-byte LDS-DMA pieces -- with g_ld % 8 == 0 every piece of G is aligned
 * when its base is -- and the weights are read as float4); gdelta is 4-byte aligned.  delta, dclip_dev and the stage-1 partials at the head of the
 * scratch are read and written one float at a time.  g_ld >= 64, g_ld % 8 == 0; channels [64, g_ld) of G are never read.
 * flk_stem_delta_grad_chunks (host only: no device work, callable without a GPU): how flk_stem_delta_grad cuts the work of a batch of B
 * clips of T frames x H rows -- one workgroup per (clip, frame pair, chunk of output rows): *nchunk chunks of *rows_per_chunk output
 * rows (H/2 in all), the last chunk H/2 - (*nchunk - 1) * *rows_per_chunk rows.  per_clip != 0: for per-clip perturbations
 * (flk_apply_args.delta_per_clip), whose chunking is that of a batch-1 call whatever B is -- a per-clip result equals the batch-1 call
 * on that clip, bit for bit.  The rule depends on the sizes only.  (flk_net_backward_delta may run the GEMM per half of the batch: its
 * chunking is then that of B/2 clips.)  FLK_EINVAL: null outputs, and the sizes flk_stem_delta_grad refuses (B < 1, T or H odd or < 2). */
int64_t flk_stem_delta_grad_scratch_bytes(int B, int T, int H);
int flk_stem_delta_grad_chunks(int B, int T, int H, int per_clip, int* nchunk, int* rows_per_chunk);
int flk_stem_delta_grad_weights_create(const float* w7_dhwio, const float* bn_scale, float** out_dev);
int flk_stem_delta_grad_weights_destroy(float* dev);
int flk_stem_delta_grad_mask(const flk_apply_args* a, float* scratch, void* stream);   /* step 1 alone (clip mask; needs x and delta only) */
int flk_stem_delta_grad(const flk_apply_args* a, const void* G, int g_ld, const float* wf_dev, float* gdelta,
                        float* scratch, int mask_done, void* stream);

/* Exact perturbation path of the folded I3D stem in bf16 mode.  conv(x') + sum over the taps inside the clip of W * a*p'[t,c] equals
 * conv(x_adv) wherever the clip is inactive (x' from flk_perturb_apply_s2d with center = 1); the second term depends on the output
 * frame and on which taps fall outside the frame only: a [T/2][4][4][64] table, added in the stem's epilogue (flk_conv_args.pos_bias).
 * weights: [7][4][4][3][64] = bn_scale * (sums of the canonical [7,7,7,3,64] stem weights over the in-frame (kh, kw) of each class). */
int flk_stem_delta_bias_weights_create(const float* w7_dhwio, const float* bn_scale, float** out_dev);
int flk_stem_delta_bias(const flk_apply_args* a, const float* sums_dev, float* table_out, void* stream);

/* Conv3d_1a_7x7 (i3d.py:168-170: 7x7x7 / 2 SAME, 3 -> 64, batch norm + ReLU) computed straight from the uint8 clip with the flickering
 * perturbation applied on the way in (kinetics_i3d_utils.py:100-142) -- ONE kernel (csrc/stem_fwd.hip) in place of
 * flk_perturb_apply_s2d + flk_conv3d over the space-to-depth tensor: K packed along the pixel row (37 MFMA K steps instead of 49),
 * the applied clip never written to HBM.  `a`: uint8 clip [B,T,224,224,3], flicker perturbation, center = 1 (the value fed to the
 * convolution is clamp(x, lo - p, hi - p) = clip(x + p, lo, hi) - p; the perturbation's own contribution comes from pos_bias =
 * flk_stem_delta_bias's table, per clip when pos_bias_bstride != 0, or NULL).  weights: flk_stem_fwd_u8_weights_create from the
 * canonical [7,7,7,3,64] array (destroy with flk_conv_weights_destroy); bn_scale / bn_bias: fp32 [64];
 * out: bf16 [B,T/2,112,112,out_ld], channels [0,64).  bf16 only (the fp32 parity mode keeps the two-kernel path).
 * Quantised stem (a->q_lut != NULL, a->center = 0): the value fed to the convolution is the one the STORED video holds,
 *   x = u8 * x_scale + x_bias;  u = clip(x + p, lo, hi);  q = the encode of flk_export_args on u (the device function flk_adv_export_u8
 *   uses);  v = q * x_scale + x_bias
 * -- the TF dialect only: q_mul = q_add = 1, q_levels = 128, x_scale = 1/128, x_bias = -1, where v = (q - 128) / 128 has eight
 * significant bits and is exact in bf16, so nothing is left for the centred clip to protect and the perturbation contributes nothing
 * through pos_bias (pass NULL, or the all-zero table).  q_lut only SELECTS the mode here: its contents are not read (the decode is the two
 * scalars).  The output is, bit for bit, that of the plain call on the bytes flk_adv_export_u8 writes for the same arguments, with
 * adv_flag = 0.  Positions outside the clip (SAME padding) stay zero.  FLK_EINVAL before any GPU call, naming the field: q_lut with
 * center != 0, with delta_dense, with another encode (q_levels, q_mul, q_add) or another decode (x_scale, x_bias); center = 0 without q_lut.
 * Gradient: straight through the clip mask -- flk_stem_delta_grad on the same arguments with q_lut cleared. */
int flk_stem_fwd_u8_weights_create(const float* w7_dhwio, flk_conv_weights** out);
int flk_stem_fwd_u8(const flk_apply_args* a, const flk_conv_weights* w, const float* bn_scale, const float* bn_bias,
                    const float* pos_bias, int64_t pos_bias_bstride, void* out, int out_ld, void* stream);

/* Clip preparation: raw decoded frames -> the normalised clip the VideoResNet engines take.  ONE kernel (csrc/prepare.hip) for the
 * reference's get_transforms(train=False) (dataset.py:84-123; references/transforms_video.py, references/functional_video.py), which
 * its attack scripts apply to every video (r2plus1d_main_universal_attack.py:169-170):
 *   ToTensorVideo (/255) -> ResizeVideo(im_scale, keep_ratio: bilinear, align_corners=False) -> CenterCropVideo -> NormalizeVideo
 * all in fp32, the interpolation between the /255 and the normalisation.  Only the crop window is computed.  Per axis
 *   src(d) = max(fma(step, d + 0.5f, -0.5f), 0) (the multiply-subtract fused, as torch's CPU kernels evaluate it: DESIGN.md 5.2.2),
 *   i0 = int(src), i1 = min(i0 + 1, in - 1), lambda = src - i0;   blend along W within each of the two rows, then along H;
 *   out = (v - mean[c]) / std[c] (true division).
 * The host supplies the geometry (videoresnet_spec.prepare_geometry is where the rules are written down): the resized size
 * (Hr, Wr) = floor(in * scale), scale = im_scale / min(Hs, Ws); the per-axis step -- float(in) / float(out) (F.interpolate(size=...),
 * also what the reference's pinned torch 1.4.0 did with its scale_factor) or float(1 / scale) (current torch given scale_factor);
 * the crop offsets round((Hr - Ho) / 2.0), round half to even.
 * One launch for up to FLK_PREP_MAX_CLIPS clips, which may differ in source resolution and pitches.  Clip k of the call is written
 * to out + (out_clip_offset + k) * out_clip_stride as [T][Ho][Wo][3] fp32, so a call can fill rows of a batch buffer.
 * No allocation, no synchronisation, no atomics; the result does not depend on the launch geometry.
 * FLK_EINVAL (before any GPU call): null pointers, nclip outside 1..FLK_PREP_MAX_CLIPS, non-positive sizes / pitches / steps, a crop
 * window outside the resized image, std <= 0, out_clip_stride smaller than a clip. */
#define FLK_PREP_MAX_CLIPS 64
typedef struct {
  const uint8_t* src;        /* device: uint8 [T][Hs][Ws][3], the 3 bytes of a pixel adjacent */
  int T, Hs, Ws;
  int64_t pitch_t, pitch_h;  /* bytes between consecutive frames / rows (a view into a longer or wider video is fine) */
  int Hr, Wr;                /* size of the resized image (never materialised): the bounds of the crop window */
  float step_h, step_w;      /* source step per resized pixel */
  int crop_i, crop_j;        /* top-left corner of the crop window in the resized image */
} flk_prep_clip;
typedef struct {
  int nclip;
  int Ho, Wo;                /* crop = output size */
  float mean[3], std[3];     /* dataset.py:28-29 as fp32 */
  int64_t out_clip_offset;   /* first clip row of `out` this call writes */
  int64_t out_clip_stride;   /* floats between clip rows of `out` (>= T*Ho*Wo*3) */
  const flk_prep_clip* clips; /* HOST array [nclip]; copied into the kernel argument */
} flk_prepare_args;
int flk_clip_prepare(const flk_prepare_args* a, float* out, void* stream);

/* The training transform on the device (csrc/prepare.hip, clip_prepare_train_kernel): the reference's get_transforms(train=True)
 * (dataset.py:105-118):
 *   ToTensorVideo -> ResizeVideo(im_scale, keep_ratio) -> RandomResizedCropVideo(input_size, scale, ratio) | RandomCropVideo(input_size)
 *   -> RandomHorizontalFlipVideo(p) -> NormalizeVideo
 * with the random draws made by the host (videoresnet_spec.train_crop_params draws them in the reference's order): per clip a box
 * (i, j, h, w) in the RESIZED image and a flip.  Two bilinear resamplings fused in one kernel, fp32 throughout:
 *   stage 1  R[y, x] = the resized image at (i + y, j + x), exactly as flk_clip_prepare computes a value before its normalisation
 *            (same source index, same /255, same blend order, the clip's step_h / step_w);
 *   stage 2  the box resampled to Ho x Wo as F.interpolate(size=(Ho, Wo), bilinear, align_corners=False) does: per axis
 *            step2 = float(h) / float(Ho) (a float32 division), src(d) = max(fma(step2, d + 0.5f, -0.5f), 0), y0 = min(int(src), h - 1),
 *            y1 = min(y0 + 1, h - 1), lambda = clamp(src - y0, 0, 1);
 *            v = (1-lh) * ((1-lw) R[y0,x0] + lw R[y0,x1]) + lh * ((1-lw) R[y1,x0] + lw R[y1,x1]);
 *   flip     output column ow takes the value computed for column Wo - 1 - ow when the clip's flip is set;
 *   out      (v - mean[c]) / std[c], true division.
 * A box of Ho x Wo (RandomCropVideo) makes stage 2 the identity: with the box at (crop_i, crop_j) and no flip the output is bitwise
 * flk_clip_prepare's.  `a` as for flk_clip_prepare, crop_i / crop_j ignored; boxes: HOST array [a->nclip].  One launch for up to
 * FLK_PREP_MAX_CLIPS clips of differing resolution, pitches, boxes and flips; rows of a batch buffer are written as by flk_clip_prepare.
 * No allocation, no synchronisation, no atomics; the result does not depend on the launch geometry.
 * FLK_EINVAL (before any GPU call): everything flk_clip_prepare refuses except the crop window, a null `boxes`, h < 1 or w < 1, a box
 * outside Hr x Wr, a flip that is not 0 / 1; and a box too wide for one workgroup to stage (never truncated). */
typedef struct { int i, j, h, w; int flip; } flk_prep_box;   /* box in the RESIZED image; flip 0/1 */
int flk_clip_prepare_train(const flk_prepare_args* a, const flk_prep_box* boxes /* HOST [nclip] */, float* out, void* stream);

/* Either transform through a frame-index table: the clips are cut from whole resident videos on the way (the temporal sampling of the
 * reference's VideoDataset, dataset.py:500-586; videoresnet_spec.sample_frame_indices draws the tables as the reference does).
 * Output frame t of clip k is computed from source frame frame_idx[k * T_out + t] of clips[k] instead of frame t; nothing else differs,
 * so the result is bitwise what flk_clip_prepare (boxes NULL) or flk_clip_prepare_train (boxes given) writes for the frames gathered
 * beforehand, and with the identity table what they write for the view itself.  A frame the table repeats is computed again.
 * `a` as for those calls, except: clips[k].T is the number of SOURCE frames in the view (any positive count), clip k is written as
 * [T_out][Ho][Wo][3] and out_clip_stride >= T_out*Ho*Wo*3.  frame_idx: DEVICE int32 [nclip][T_out], read by the kernel when it runs;
 * its validity is the caller's: the kernel clamps every index it reads into [0, clips[k].T - 1], so a bad table gives wrong frames
 * but never a read outside the view (ops.prepare_clips refuses such a table before it launches).
 * No allocation, no synchronisation, no atomics; the result does not depend on the launch geometry.
 * FLK_EINVAL (before any GPU call): everything flk_clip_prepare (boxes NULL) / flk_clip_prepare_train (boxes given) refuses, a null
 * frame_idx, T_out outside 1..65535. */
int flk_clip_prepare_sampled(const flk_prepare_args* a, const flk_prep_box* boxes /* HOST [nclip], or NULL: the evaluation transform */,
                             const int32_t* frame_idx /* DEVICE [nclip][T_out] */, int T_out, float* out, void* stream);

/* Training on the DELIVERED video at its native resolution.  A per-frame flicker is uniform over a frame, so the delivered frame -- the
 * raw frame after the 8-bit export of the flicker (flk_adv_export_u8 / flk_illum_export_u8) -- is the raw frame through a byte -> byte
 * map per (clip, frame, channel), the TONE TABLE: tone[k][t][v][c], uint8 [nclip][T_out][256][3], the byte the export writes for source
 * byte v of channel c under the delta row of output frame t of clip k.  It is made by the export launch itself on a constant ramp clip
 * (uint8 [n][T][16][16][3], pixel p holding level p in its three channels) with the per-clip delta [n][T][3] of video time
 * (flk_flicker_rows_gather / flk_flicker_rows_mix), so it equals the export of a whole video bit for bit; there is no kernel of its own.
 *
 * flk_clip_prepare_toned: flk_clip_prepare_sampled on the delivered video, which is never written.  The workgroup of (clip k, output
 *   frame t) stages tone[k][t] (768 bytes) in LDS and maps every source byte as it stages the row segments; everything after that is
 *   the sampled kernels' own statements, so the result is bit for bit what flk_clip_prepare_sampled writes for the exported video:
 *   both transforms (two-stage and box-of-the-output-size paths, flips), clips of differing resolution, tables that repeat frames.
 *   With the identity table (tone[v] = v) it is bit for bit the untoned launch.  tone: DEVICE, any alignment.
 *   FLK_EINVAL (before any GPU call): everything flk_clip_prepare_sampled refuses, a null tone.
 *
 * flk_flicker_tone_slopes: the straight-through derivative of the display value of source byte v with respect to the frame's delta
 *   value, before its finishing factors -- slope fp32 [B][T][256][3] -- and those factors, scale fp32 [B][T][3].  `a` is the apply
 *   description of the ramp: uint8 through x_lut, delta_per_clip (delta [B][T][3]), no rolls; m NULL: the additive model.
 *     additive:      slope = 1 where lo <= u <= hi, u = x_lut[v][c] + adv_flag * p (p the clamped delta value times inv_std[c]: the
 *                    mask expression of flk_perturb_grad_reduce), else 0;            scale = adv_flag * inv_std[c]
 *     illumination:  slope = (d * N) * L of flk_illum_grad_reduce (two rounded products), 0 where p leaves [0,1];
 *                                                                                    scale = adv_flag * out_mul[c]
 *   scale is 0 where the delta value lies outside its clamp (dclip / dclip_dev).  One launch.
 *   FLK_EINVAL (before any GPU call): null a / slope / scale / x / delta, an fp32 clip or a null x_lut, delta_per_line, delta_dense,
 *   center = 1, delta_per_clip = 0, a roll; with m what flk_illum_grad_reduce refuses of m.
 *
 * flk_clip_prepare_grad: d(loss)/d(delta_clip) through the resampling of a toned preparation,
 *     gdelta[k][t][c] = scale[k][t][c] * sum over output pixels (oh, ow) of g(k,t,oh,ow,c) * J(oh,ow,c)        fp32 [nclip][T_out][3]
 *   J: the forward's own resampling run on slopes instead of pixel values -- the same source indices, taps and lambdas, the one- or
 *   two-stage blend (a box of the output size skips stage 2), every blend the fixed sequence fma(w0, v0, w1 * v1), every tap read
 *   through slope[k][t][byte][c]; no mean, no std; a flipped clip pairs g at column ow with J of column Wo - 1 - ow.  boxes NULL: the
 *   evaluation transform (the box (crop_i, crop_j, Ho, Wo), no flip).  g: gx_s2d, the layout flk_perturb_grad_reduce reads for fold_t 1,
 *   [nclip][T_out][Ho/2][Wo/2][16] fp32 or bf16, channel ((oh & 1) * 2 + (ow & 1)) * 3 + c; row k belongs to clip k of the call
 *   (out_clip_offset is not used).  Every product g * J and every sum is rounded to fp32 on its own, in ONE order that does not depend
 *   on the grid, on the rows a workgroup takes or on the other clips: one wave per (clip, frame, output row), lane l adds columns l,
 *   l + 64, ... ascending from +0, the lanes fold by the shuffle tree 32 .. 1 (partials [nclip][T_out][Ho][3]); a finishing launch adds
 *   the rows ascending from +0 and multiplies by scale (a zero scale writes +0 whatever the sum is).  No atomics: repeats are bitwise equal, and a clip's result is that of a call
 *   holding that clip alone.  partials: flk_clip_prepare_grad_scratch_bytes(nclip, T_out, Ho) of caller scratch.  Two launches.
 *   FLK_EINVAL (before any launch): null pointers, gx_s2d not 16-byte aligned, a bad dtype, odd Ho / Wo, and everything
 *   flk_clip_prepare_toned refuses of a / boxes / frame_idx / T_out (out_clip_stride as there). */
int flk_clip_prepare_toned(const flk_prepare_args* a, const flk_prep_box* boxes /* HOST [nclip], or NULL: the evaluation transform */,
                           const int32_t* frame_idx /* DEVICE [nclip][T_out] */, int T_out, const uint8_t* tone /* DEVICE [nclip][T_out][256][3] */,
                           float* out, void* stream);
int flk_flicker_tone_slopes(const flk_apply_args* a, const flk_illum_args* m /* NULL: additive */, float* slope /* [B,T,256,3] */,
                            float* scale /* [B,T,3] */, void* stream);
int64_t flk_clip_prepare_grad_scratch_bytes(int nclip, int T_out, int Ho);
int flk_clip_prepare_grad(const flk_prepare_args* a, const flk_prep_box* boxes, const int32_t* frame_idx, int T_out, const float* slope,
                          const float* scale, const void* gx_s2d, int dtype, float* gdelta /* fp32 [nclip,T_out,3] */, float* partials,
                          void* stream);

/* The transpose of the resampling on IMAGES (csrc/prepare.hip, clip_prepare_grad_image_kernel): the gradient with respect to every
 * source pixel, where flk_clip_prepare_grad pushes per-byte slopes forward.  The resampling is separable, out = A_h V A_w^T with
 * A = S2 S1 per axis (flip included along W); videoresnet_spec.prepare_adjoint_tables builds both composite matrices per clip from
 * the forward's own indices and lambdas in float64, rounds them once to fp32 and stores them BY SOURCE INDEX: entry y of a table is
 * 2 + K 32-bit words (first_out, count, w[K] fp32) -- the outputs that read a source index are a contiguous range, both stages
 * being monotone; K is the largest count of the call.
 *   g_src[k][t][y][x][c] = sum over a < count_h[y], b < count_w[x] of wh[y][a] * ww[x][b] * g(first_h[y] + a, first_w[x] + b, c)
 * with b inner and a outer, both ascending from +0: row sums fma(ww[b], g, .), then fma(wh[a], row, .).  g: the gx_s2d layout of
 * flk_clip_prepare_grad (fp32 or bf16), row k of it clip k of the call.  g_src: fp32, clip k at clips[k].dst as [T_out][Hs][Ws][3]
 * with pitches in floats; a source pixel no output reads gets +0.  tables: DEVICE, table_words words; every range read from it is
 * clamped into the output image, so a bad table gives wrong sums but no read outside g.  One launch, no atomics, one fixed order: a
 * clip's result is that of a call holding it alone.
 * FLK_EINVAL (before any GPU call): null pointers, nclip outside 1..FLK_PREP_MAX_CLIPS, T_out outside 1..65535, odd or non-positive
 * Ho / Wo, K outside 1..Ho + Wo, gx_s2d not 16-byte aligned, a bad dtype, non-positive sizes, pitches that do not hold a row / a
 * frame, tables that leave table_words. */
typedef struct {
  float* dst;                /* device: fp32 [T_out][Hs][Ws][3] */
  int64_t pitch_t, pitch_h;  /* FLOATS between consecutive frames / rows */
  int Hs, Ws;
  int64_t tab_h, tab_w;      /* word offsets of the clip's row and column tables: Hs and Ws entries of 2 + K words */
} flk_grad_image_clip;
int flk_clip_prepare_grad_image(int nclip, const flk_grad_image_clip* clips /* HOST [nclip] */, int T_out, int Ho, int Wo, int K,
                                const int32_t* tables /* DEVICE */, int64_t table_words, const void* gx_s2d, int dtype, void* stream);

/* Lossy intra-frame compression of the delivered video (csrc/codec.hip): a JPEG-style round trip -- colour transform, chroma
 * subsampling, 8x8 DCT, quantisation and back -- as ONE kernel with an exact integer definition, which
 * videoresnet_spec.codec_roundtrip_host restates in numpy bit for bit (DESIGN.md 10.8 has every constant and rounding rule).  It is
 * exactly MJPEG and the I-frame path of a block codec minus the (lossless) entropy coder.  Per output frame, uint8 [Hs][Ws][3]:
 *   tone (optional byte -> byte table, as flk_clip_prepare_toned takes it) -> RGB to YCbCr (JFIF full range, 16-bit fixed point) ->
 *   pad to whole MCUs by repeating the last column and row (8x8; 16x16 with 4:2:0) -> 4:2:0 only: Cb, Cr as 2x2 box means,
 *   (a + b + c + d + 1 + (x & 1)) >> 2, x the output column -> minus 128, forward 8x8 "slow integer" DCT (13-bit constants, two passes) ->
 *   level = the coefficient / (8 Q), half away from zero -> level * Q, inverse DCT, plus 128, clamp to 0..255 -> chroma repeated 2x2 ->
 *   YCbCr to RGB (16-bit fixed point, clamped) -> crop.
 * flk_codec_tables (host only; no device work): Q = clamp((base * s + 50) / 100, 1, 255) of the two base tables of ITU T.81 Annex K
 *   (luminance, chrominance; row-major), s = 5000 / quality for quality < 50, else 200 - 2 quality (integer division): the tables a
 *   JPEG encoder writes at that quality.
 * flk_codec_roundtrip_u8: one launch for up to FLK_PREP_MAX_CLIPS clips of differing resolution and pitches.  Output frame t of clip k
 *   is made from source frame frame_idx[k * T_out + t] of clips[k] (DEVICE int32 [nclip][T_out]; every index read is clamped into
 *   [0, clips[k].T - 1], the rule of flk_clip_prepare_sampled), or from frame t when frame_idx is null (then T_out <= clips[k].T),
 *   and written to clips[k].dst + t * dst_pitch_t as rows dst_pitch_h bytes apart.  No byte outside the Hs x Ws x 3 views is written.
 *   tone: DEVICE uint8 [nclip][T_out][256][3], any alignment, or null.  stats: DEVICE int32 [nclip][T_out][2] or null, zeroed here by
 *   one hipMemsetAsync: per frame the number of non-zero quantised coefficients and the sum of their magnitudes (a proxy for the bit
 *   rate; integer sums, exact in any order).  A frame a table repeats is computed again.  No allocation, no synchronisation; the
 *   result does not depend on the launch geometry.
 *   FLK_EINVAL (before any GPU call): null a / clips / src / dst, nclip outside 1..FLK_PREP_MAX_CLIPS, non-positive sizes or pitches,
 *   a row pitch smaller than 3 * Ws (or above 2^31 - 1), quality outside 1..100, a subsampling other than FLK_CODEC_444 /
 *   FLK_CODEC_420, T_out outside 1..65535 (or above a clip's T without frame_idx), dst == src, stats on frames of more than 5000000
 *   padded pixels (the sum of magnitudes is at most 386 per pixel: it must fit an int32). */
#define FLK_CODEC_444 444
#define FLK_CODEC_420 420
typedef struct {
  const uint8_t* src;        /* device: uint8 [T][Hs][Ws][3], the 3 bytes of a pixel adjacent */
  int T, Hs, Ws;
  int64_t pitch_t, pitch_h;  /* bytes between consecutive source frames / rows */
  uint8_t* dst;              /* device: uint8 [T_out][Hs][Ws][3] */
  int64_t dst_pitch_t, dst_pitch_h;
} flk_codec_clip;
typedef struct {
  int nclip;
  int quality;               /* 1..100, the IJG scale */
  int subsampling;           /* FLK_CODEC_444 or FLK_CODEC_420 */
  const flk_codec_clip* clips; /* HOST array [nclip]; copied into the kernel argument */
} flk_codec_args;
int flk_codec_tables(int quality, int32_t* qluma /* [64] */, int32_t* qchroma /* [64] */);
int flk_codec_roundtrip_u8(const flk_codec_args* a, const int32_t* frame_idx /* DEVICE [nclip][T_out] or NULL */, int T_out,
                           const uint8_t* tone /* DEVICE [nclip][T_out][256][3] or NULL */, int32_t* stats /* DEVICE [nclip][T_out][2] or NULL */,
                           void* stream);

/* The codec's backward (csrc/codec.hip, codec_grad_kernel; videoresnet_spec.codec_grad_host is the definition in
 * float64).  The forward stays the integer codec; the backward differentiates a surrogate of it per frame, whose constants the kernel
 * takes from the integer forward of each block, recomputed and not stored: colour transforms by their integer constants over 2^16;
 * the plane clamp and the RGB clamp pass the gradient where the UNCLAMPED integer lies in 0..255; the padding folds onto the last
 * row and column; the 4:2:0 box mean gives 1/4 to each pixel, the replication sums; the DCT pair is the orthonormal 8x8 matrix C in
 * fp32 (G = C g C^T, then C^T G C); the quantiser's factor per coefficient f of level lev, r = (f - lev * 8 Q) / (8 Q):
 *   FLK_CODEC_GRAD_STE    d = 1
 *   FLK_CODEC_GRAD_CUBIC  d = 3 r^2  (the rounding u -> round(u) + (u - round(u))^3: 0 at a bin centre, 3/4 at a bin edge)
 * g_out: DEVICE fp32, d(loss)/d(decoded RGB), the clips packed one after the other, clip k as [T_out][Hs_k][Ws_k][3]; g_in: the same
 * layout or NULL, d(loss)/d(the codec's input frame).  gdelta[k][t][c] = scale[k][t][c] * sum over pixels of g_in(p, c) *
 * slope[k][t][v(p, c)][c], v the SOURCE byte before the tone table; slope fp32 [nclip][T_out][256][3] and scale fp32 [nclip][T_out][3]
 * as flk_flicker_tone_slopes writes them.  a, frame_idx, T_out and tone as flk_codec_roundtrip_u8 takes them, clips[k].dst and its
 * pitches unused.  One workgroup per tile of the forward's tiling; per-tile sums in partials (flk_codec_grad_scratch_bytes(a, T_out)
 * of caller scratch; 0 for arguments the call would refuse), a finishing launch adds a frame's tiles ascending from +0 and multiplies
 * by scale (a zero scale writes +0).  No atomics: repeats are bitwise equal and a clip's result is that of a call holding it alone.
 * FLK_EINVAL (before any GPU call): what flk_codec_roundtrip_u8 refuses of a / T_out (but for dst), a mode other than the two, null
 * slope / scale / gdelta / g_out / partials, g_in == g_out. */
#define FLK_CODEC_GRAD_STE 1
#define FLK_CODEC_GRAD_CUBIC 2
int64_t flk_codec_grad_scratch_bytes(const flk_codec_args* a, int T_out);
int flk_codec_grad(const flk_codec_args* a, const int32_t* frame_idx /* DEVICE [nclip][T_out] or NULL */, int T_out,
                   const uint8_t* tone /* DEVICE [nclip][T_out][256][3] or NULL */, int mode, const float* g_out, const float* slope,
                   const float* scale, float* gdelta /* fp32 [nclip][T_out][3] */, float* g_in /* optional */, float* partials, void* stream);

/* Inter-frame prediction in the codec (csrc/codec.hip; videoresnet_spec.codec_roundtrip_host(gop=, first_frame=) is
 * the definition, bit for bit): closed GOPs of `gop` frames.  Video frame n is an intra frame iff n % gop == 0, coded as
 * flk_codec_roundtrip_u8 codes it; every other frame is a P-frame predicted at ZERO MOTION from the previous frame's reconstructed
 * padded planes ref -- per plane (Y, Cb, Cr) and 8x8 block: r = cur - ref (no -128), the same forward transform,
 * level = sign * ((|f| + 2 Qp) / (8 Qp)) (a rounding offset of 1/4 step), rec = clamp(ref + idct(level * Qp), 0, 255), ref <- rec.
 * flk_codec_inter_step (host only): Qp = clamp((16 * s + 50) / 100, 1, 255), s the IJG scale of `quality` -- one step for all 64
 *   positions and all three planes (MPEG-2's flat default non-intra matrix under the rule of flk_codec_tables).
 * flk_codec_roundtrip_gop_u8: one launch for up to FLK_PREP_MAX_CLIPS clips.  Clip k's span is the count[k] video frames from
 *   first[k] (HOST arrays; first[k] a multiple of gop, so every span starts on an intra frame); output frame t is video frame
 *   first[k] + t, written at clips[k].dst + t * dst_pitch_t.  tone / stats rows are [k][t], T_max rows per clip; rows at or past
 *   count[k] are not read / stay zero.  A workgroup walks one GOP of one tile with the reference planes in LDS: no workspace, no
 *   allocation, no synchronisation; the result does not depend on the launch geometry.  gop == 1 is allowed (every frame intra).
 *   FLK_EINVAL (before any GPU call): what flk_codec_roundtrip_u8 refuses of a / clips / quality / subsampling, stats on frames of
 *   more than 2500000 padded pixels (a P-frame's magnitudes reach 766 per pixel, twice an intra frame's), null first or
 *   count, gop outside 1..65535, T_max outside 1..65535, first[k] < 0 or not a multiple of gop, count[k] < 1, count[k] > T_max,
 *   first[k] + count[k] > clips[k].T. */
int flk_codec_inter_step(int quality, int32_t* qp);
int flk_codec_roundtrip_gop_u8(const flk_codec_args* a, int gop, const int32_t* first /* HOST [nclip] */,
                               const int32_t* count /* HOST [nclip] */, int T_max,
                               const uint8_t* tone /* DEVICE [nclip][T_max][256][3] or NULL */,
                               int32_t* stats /* DEVICE [nclip][T_max][2] or NULL */, void* stream);

/* Motion-compensated P-frames (csrc/codec.hip; videoresnet_spec.codec_roundtrip_host(gop=, first_frame=, search=) is
 * the definition, bit for bit).  As flk_codec_roundtrip_gop_u8, but a P-frame's padded luma plane is cut into 16x16 macroblocks from
 * the top-left corner (at 4:4:4 the last column or row may be 8 wide or high) and each is predicted from the previous reconstruction
 * displaced by the full-pel vector (dy, dx), |dy|, |dx| <= search, of least SAD = sum |cur_Y[y][x] - ref_Y[clamp(y + dy)][clamp(x + dx)]|;
 * among equal SADs the first in the order (0, 0), then dy = -search..search (outer), dx = -search..search (inner) -- the minimum of
 * SAD * 1024 + rank.  Chroma takes the same vector at 4:4:4 and half of it at half-pel precision at 4:2:0 (iy = dy >> 1, hy = dy & 1;
 * a, (a + b + 1) >> 1 or (a + b + c + d + 2) >> 2), every read clamped into the plane.  The residual against that prediction is coded
 * as at zero motion.  search == 0 is allowed: zero vectors, the bytes of flk_codec_roundtrip_gop_u8 through this path.
 * One launch per frame position within the GOP (min(gop, the longest count) of them, times ceil(nclip / 48)); the reconstructed
 * planes travel through `scratch`, two plane sets per (clip, GOP), and the launches are ordered by the stream alone.
 * flk_codec_mc_scratch_bytes: the bytes of scratch the call with the same a / gop / count needs; 0 for arguments it would refuse.
 * mv: DEVICE int8 [nclip][T_max][mv_stride][2] or null, zeroed here: (dy, dx) of clip k's macroblock (my, mx) of output frame t at
 *   [k][t][my * MBx_k + mx], MBx_k = ceil(padded width / 16); intra frames and rows at or past count[k] stay zero.
 * FLK_EINVAL (before any GPU call): what flk_codec_roundtrip_gop_u8 refuses, search outside 0..15, a null scratch, one not 16-byte
 *   aligned or smaller than flk_codec_mc_scratch_bytes, mv_stride below a clip's macroblock count (with mv). */
int64_t flk_codec_mc_scratch_bytes(const flk_codec_args* a, int gop, const int32_t* count /* HOST [nclip] */);
int flk_codec_roundtrip_mc_u8(const flk_codec_args* a, int gop, int search, const int32_t* first /* HOST [nclip] */,
                              const int32_t* count /* HOST [nclip] */, int T_max,
                              const uint8_t* tone /* DEVICE [nclip][T_max][256][3] or NULL */,
                              int32_t* stats /* DEVICE [nclip][T_max][2] or NULL */,
                              int8_t* mv /* DEVICE [nclip][T_max][mv_stride][2] or NULL */, int mv_stride, void* scratch,
                              int64_t scratch_bytes, void* stream);

/* Tail of the data-parallel payload (flickering_adversarial_video_amd/parallel.py; replaces the per-iteration
 * reduce_sum / reduce_mean fetches of i3d_adversarial_main_single_video_npy.py:213-217): from the per-clip
 * outputs of flk_softmax_adv_loss ([B,4] = loss, p_label, p_max_other, argmax)
 *   out3 = { sum_b loss_b, prob_scale * sum_b p_label, prob_scale * sum_b p_max_other }   (fixed summation order). */
int flk_pack_batch_sums(const float* per_clip, int B, float prob_scale, float* out3, void* stream);

/* Regulariser gradient + Adam on delta (flicker, [T,3] time-major; the torch dialect's [3,T] is
 * transposed by the host wrapper).  TF dialect: kinetics_i3d_utils.py:177-186 +
 * i3d_adversarial_main_single_video_npy.py:56-59,79-84 (regulariser on the RAW delta, TF Adam).
 * torch dialect: model.py:198-209 (regulariser on the CLAMPED delta, torch Adam, model.py:868).
 * g_adv is the (all-reduced) adversarial-loss gradient.  Writes scalars[8] =
 * {reg_total, norm, diff, lap, thickness, roughness, max, min} of the PRE-update delta. */
typedef struct {
  int T;
  int torch_dialect;
  float beta0;               /* TF: LAMBDA; torch: lambda_ */
  float beta1, beta2, beta3; /* TF: b1*norm + b2*diff + b3*lap; torch: b1*norm + (1-b1)(diff+lap) */
  float dyn_max_norm;        /* torch clamp bound for the regulariser */
  float g_scale;             /* multiplies g_adv (1/(global batch) for mean losses) */
  float lr, adam_b1, adam_b2, adam_eps;
  int step;                  /* 1-based Adam step of THIS update */
  float pgd_eps;             /* flk_perturb_reg_pgd* only, TF dialect: the l-infinity radius (torch dialect: dyn_max_norm is the radius) */
} flk_adam_args;
int flk_perturb_reg_adam(const flk_adam_args* a, const float* g_adv, float* delta, float* m, float* v,
                         float* scalars, void* stream);
/* The same update for nclip INDEPENDENT perturbations (delta, m, v, g_adv: [nclip,T,3]; scalars: [nclip,8]) -- single-video attacks
 * batched (i3d_adversarial_main_single_video_npy.py:103-337; model.py:791-982 fit_many_videos): clip b takes Adam step
 * steps_dev[b] + 1 (a->step is ignored) and the counter is advanced on the device; clips with active_dev[b] == 0 (already
 * adversarial: retired) keep delta / m / v / counter, their scalars are still written.  active_dev may be NULL (all active);
 * dyn_max_norm_dev (torch dialect) may be NULL (a->dyn_max_norm for every clip) or hold one clamp bound per clip.
 * Per clip the arithmetic is exactly flk_perturb_reg_adam's. */
int flk_perturb_reg_adam_batched(const flk_adam_args* a, int nclip, const float* g_adv, float* delta, float* m, float* v,
                                 int* steps_dev, const int* active_dev, const float* dyn_max_norm_dev, float* scalars, void* stream);

/* Regulariser gradient + projected sign-gradient (l-infinity PGD) step on the flicker delta: the update BASELINE.json's north star
 * names beside Adam (the reference optimises with Adam only, i3d_adversarial_main_single_video_npy.py:79-84 / model.py:868; this is
 * the baseline attack its comparisons are run against).  g_tot = g_scale * g_adv + beta0 * d(reg)/d(delta) is formed by the SAME
 * code as flk_perturb_reg_adam (TF dialect: regulariser of the raw delta; torch dialect: of the clamped one, zero outside the clamp), then
 *   delta' = clamp(delta - lr * sgn(g_tot), -eps, +eps)      in fp32; sgn(0) = 0 (the element does not move); NaN stays NaN
 * with eps = dyn_max_norm (torch dialect: the clamp of model.py:1078, so the restart schedule of model.py:1061-1066 widens the
 * projection with it) or pgd_eps (TF dialect; 0.4 = the apply clip of kinetics_i3d_utils.py:104 makes raw and clipped delta
 * coincide); eps <= 0 is FLK_EINVAL.  No optimiser state; adam_b1 / adam_b2 / adam_eps / step are ignored.  scalars[8] as
 * flk_perturb_reg_adam writes them (bitwise, for the same delta).  One launch, deterministic. */
int flk_perturb_reg_pgd(const flk_adam_args* a, const float* g_adv, float* delta, float* scalars, void* stream);
/* The same step for nclip INDEPENDENT perturbations (delta, g_adv: [nclip,T,3]; scalars: [nclip,8]), the sibling of
 * flk_perturb_reg_adam_batched: clips with active_dev[b] == 0 keep delta and counter (scalars still written); steps_dev[b] is advanced
 * for active clips ("iterations spent on this video" -- it does not enter the arithmetic); dyn_max_norm_dev (torch dialect) holds
 * one radius per clip or is NULL.  Per clip the arithmetic is exactly flk_perturb_reg_pgd's. */
int flk_perturb_reg_pgd_batched(const flk_adam_args* a, int nclip, const float* g_adv, float* delta, int* steps_dev,
                                const int* active_dev, const float* dyn_max_norm_dev, float* scalars, void* stream);

/* Dense-delta ("sparse adversarial perturbations" baseline, kinetics_i3d_L12, kinetics_i3d_utils.py:308-521): delta is
 * [T,H,W,3] (init 1e-8, no +-0.4 clip), regulariser L12 = sum_t sqrt(mean_{hwc} delta_t^2) + 1e-12 (:409; torch dialect
 * model.py:211-214), loss = adv + beta1 * L12 (i3d_adversarial_main_universal.py:129-133), TF or torch Adam.
 * Two HBM-bound passes: per-frame sum of squares (deterministic two-stage reduction into frame_sq[T], fp32), then the
 * fused gradient + Adam update streaming delta, m, v, g_adv once (5 fp32 streams = 193 MB at T=64).
 * scalars[4] = {L12, thickness, roughness, max|delta|} of the PRE-update delta.  scratch: flk_dense_adam_scratch_bytes().
 * Pointer contract: g_adv, delta, m and v (flk_perturb_dense_l12_pgd: g_adv and delta) are 16-byte aligned -- the kernels stream them
 * four floats at a time; anything else is FLK_EINVAL naming the alignment, before any GPU call. */
typedef struct {
  int T, H, W;
  int torch_dialect;
  float beta;                /* weight of L12 in the loss */
  float g_scale;
  float lr, adam_b1, adam_b2, adam_eps;
  int step;
  float dyn_max_norm;        /* > 0 (torch dialect): L12 is taken on clamp(delta, +-dyn_max_norm), as Losses receives the CLAMPED
                              * perturbation (model.py:1078,211-214); its gradient vanishes where |delta| > dyn_max_norm.  0: raw delta */
  float pgd_eps;             /* flk_perturb_dense_l12_pgd only, TF dialect: the l-infinity radius (torch dialect: dyn_max_norm) */
} flk_dense_adam_args;
int64_t flk_dense_adam_scratch_bytes(int T, int H, int W);
int flk_perturb_dense_l12_adam(const flk_dense_adam_args* a, const float* g_adv, float* delta, float* m, float* v,
                               float* scalars, float* scratch, void* stream);
/* The dense delta under the projected sign-gradient step (the standard l-infinity video PGD attack next to the kinetics_i3d_L12
 * baseline, kinetics_i3d_utils.py:308-521): the two reduction passes of flk_perturb_dense_l12_adam, then ONE streaming pass
 *   delta' = clamp(delta - lr * sgn(g_scale * g_adv + d(beta * L12)/d(delta)), -eps, +eps)
 * reading g_adv and delta and writing delta (3 fp32 streams = 115 MB at T=64; no m, v).  eps = dyn_max_norm (torch dialect) or
 * pgd_eps (TF dialect: this form has no apply clip, kinetics_i3d_utils.py:333, so the radius is required); eps <= 0 is FLK_EINVAL.
 * sgn(0) = 0, NaN stays NaN.  scalars[4] and scratch as flk_perturb_dense_l12_adam; adam_b1 / adam_b2 / adam_eps / step are ignored. */
int flk_perturb_dense_l12_pgd(const flk_dense_adam_args* a, const float* g_adv, float* delta, float* scalars, float* scratch,
                              void* stream);

/* Classifier head (csrc/head.hip): time-weighted average pool + linear layer, and its gradient.  What every flk_net runs between its
 * last activation and the loss head (I3D Logits endpoint, i3d.py:459-474; VideoResNet avgpool + fc), callable on its own.
 *   feat[b,c]   = sum_{t,p} wt[t] * y[b,t,p,coff+c]                  (p over the HW positions of frame t)
 *   logits[b,n] = bias[n] + sum_c feat[b,c] * W[c,n]                 (bias == NULL: no bias)
 *   dfeat[b,c]  = sum_n dlogits[b,n] * W[c,n]
 *   gy[b,t,p,gcoff+c] = wt[t] * dfeat[b,c], and 0 where use_mask and not y[b,t,p,coff+c] > 0 (-0.0, +0.0, negatives and NaN give 0;
 *                       denormals and +inf pass).  Channels of gy outside [gcoff, gcoff+C) are not written.
 * All pointers are DEVICE pointers.  y: [B,Tn,HW,ld] and gy: [B,Tn,HW,gld] of `dtype` (FLK_F32 / FLK_BF16), channels innermost;
 * wt: fp32 [Tn]; W: fp32 [C,N]; bias: fp32 [N] or NULL; feat, dfeat: fp32 [B,C]; logits, dlogits: fp32 [B,N].  All arithmetic is
 * fp32 in a fixed order: no atomics, results bitwise repeatable and row b independent of the other rows of the batch; bf16 gy is
 * the fp32 product rounded to nearest even once.
 * Limits: B, C, Tn, HW, N >= 1; B <= 65535; N <= 1024; forward: C <= 2048, any coff >= 0 with coff + C <= ld; backward: C, ld, coff,
 * gld, gcoff multiples of EPL = 4 (fp32) / 8 (bf16), gcoff + C <= gld, B*Tn*HW*(C/EPL) < 2^31, gy 16-byte aligned, and with use_mask y
 * 16-byte aligned (use_mask == 0: y is not read and may be NULL).  FLK_EINVAL naming the argument and its value otherwise, before any
 * GPU call.  Two launches each. */
int flk_head_forward(const void* y, int ld, int coff, int C, int B, int Tn, int HW, const float* wt, const float* W,
                     const float* bias, int N, float* feat, float* logits, int dtype, void* stream);
int flk_head_backward(const void* y, int ld, int coff, void* gy, int gld, int gcoff, int C, int B, int Tn, int HW,
                      const float* wt, const float* W, int N, const float* dlogits, float* dfeat, int use_mask, int dtype,
                      void* stream);

/* Loss head: softmax + adversarial loss + d(loss)/d(logits) (kinetics_i3d_utils.py:152-169,253-307;
 * model.py:177-250).  per_clip[b*4..] = {loss_b, label_prob, max_non_label_prob, argmax}. */
typedef struct {
  int B, C;
  int torch_dialect, improve_loss, use_logits, targeted;
  float margin;
  float mean_scale;          /* CE variants are means: 1/(global batch) */
} flk_loss_args;
int flk_softmax_adv_loss(const flk_loss_args* a, const float* logits, const int64_t* labels,
                         float* softmax, float* dlogits, float* per_clip, void* stream);
/* The same loss on a VIDEO's aggregated logits -- the quantity the reference's evaluate(num_samples) decides on (model.py:1227-1317: the
 * argmax of the summed logits of a video's clips).  logits holds a->B = V*G clip rows, video-major and clip-minor; one workgroup per
 * video forms, in fp32 and strictly in clip order,
 *   z[v][j] = scale * (((l[vG+0][j] + l[vG+1][j]) + l[vG+2][j]) + ...)          (scale = 1: the sum; 1/G: the mean, same argmax)
 * and applies flk_softmax_adv_loss's arithmetic (same code) to z[v] with labels[v]; a->mean_scale is 1/(global number of VIDEOS).
 * Outputs: softmax [V,C] of z and video_logits [V,C] = z (either may be NULL), per_video [V,4] = {loss_v, label_prob, max_non_label_prob,
 * argmax} of z, and dlogits [V*G,C] with dlogits[vG+g][j] = scale * d(loss_v)/dz[v][j] for every clip g of the video.
 * With G = 1 and scale = 1 every output is bitwise flk_softmax_adv_loss's (finite logits).  NaN logits and labels outside [0,C) end in a
 * NaN loss and NaN gradient rows for that video alone (flk_softmax_adv_loss reports a loss of 0 beside the NaN gradient for NaN logits
 * under the improve-loss variants; this entry reports NaN in every variant).  FLK_EINVAL: G < 1, a->B % G != 0, scale <= 0, and everything
 * flk_softmax_adv_loss refuses. */
int flk_softmax_adv_loss_video(const flk_loss_args* a, int G, float scale, const float* logits, const int64_t* labels,
                               float* softmax, float* video_logits, float* dlogits, float* per_video, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-network plan: the victim classifier forward + backward-to-input as one call
 * (replaces sess.run([train_op, ...]) of i3d_adversarial_main_single_video_npy.py:213-217 and
 * model([x,True]) + loss.backward() of model.py:1073-1101).  Weights are handed over once,
 * packed on the host and kept resident (never re-broadcast, cf. nn.DataParallel model.py:576).
 * ------------------------------------------------------------------------------------------- */
typedef struct flk_net flk_net;
#define FLK_NET_I3D 0
#define FLK_NET_R2PLUS1D_18 1
#define FLK_NET_R3D_18 2
#define FLK_NET_MC3_18 3
#define FLK_NET_R2PLUS1D_34 4                /* R(2+1)D-34 (IG65M / Kinetics, ig65m-pytorch): blocks 3-4-6-3, BN eps 1e-3 */

int flk_net_create(int arch, int dtype, int B, int T, int H, int W, int device, flk_net** out);
int flk_net_destroy(flk_net* n);
/* name = checkpoint variable name (kinetics_i3d_utils.py:41-62 for I3D; torchvision state_dict keys
 * for VideoResNet); data = fp32 host array in the checkpoint's own layout. */
int flk_net_set_weight(flk_net* n, const char* name, const float* data, int64_t numel);
int flk_net_finalize(flk_net* n);                 /* pack + upload; plan buffers */
int64_t flk_net_workspace_bytes(const flk_net* n);
/* x_s2d: output of flk_perturb_apply_s2d (I3D) ; logits: fp32 [B,num_classes] */
int flk_net_forward(flk_net* n, const void* x_in, float* logits, int save_for_backward, void* stream);
/* forward of a clip applied with flk_apply_args.center = 1 (I3D plan in bf16: flk_net_has_forward_flicker): computes the stem's
 * position-class bias table of `a` (flk_stem_delta_bias) and runs the plan with it */
int flk_net_has_forward_flicker(const flk_net* n);
int flk_net_forward_flicker(flk_net* n, const void* x_in, const flk_apply_args* a, float* logits, void* stream);
/* apply + forward in one call: the plan launches flk_perturb_apply_s2d itself, per batch slice on the stream that slice's stem
 * convolution runs on (I3D at bs >= 4: the two half-batches -- the second half's apply overlaps the first half's stem), writing the
 * space-to-depth clip into x_s2d_out; with a->center = 1 (flk_net_has_forward_flicker) the position-class bias path is taken.
 * a->fold_t must be the plan's layout, flk_net_input_fold(): 3 for I3D; VideoResNet plans 1 in fp32 (16 channels) and 4 in bf16 (32 channels:
 * every value as two bf16 numbers, [hi(16) | lo(16)]).  Same logits as apply followed by flk_net_forward[_flicker].
 * x_s2d_out is SCRATCH: when the stem reads the uint8 clip itself (I3D plan in bf16, a->x_is_u8 with a->center = 1 -- the default
 * engine path) it is left untouched, so a caller that needs the space-to-depth tensor calls flk_perturb_apply_s2d itself.
 * Quantised arguments (a->q_lut, a->center = 0: the plan sees the STORED clip): on the I3D plan in bf16 at 224 x 224, a uint8 clip with a
 * flicker delta in the TF dialect goes to the quantised instantiation of flk_stem_fwd_u8 -- half-batch streams and per-clip slices as in
 * the plain mode, x_s2d_out untouched; every other plan or clip (fp32 plans, an fp32 clip, FLK_STEM_U8=0, the torch encode) takes the
 * quantised flk_perturb_apply_s2d into x_s2d_out and the folded stem. */
int flk_net_forward_apply(flk_net* n, const flk_apply_args* a, void* x_s2d_out, float* logits, void* stream);
/* dlogits fp32 [B,C] -> gradient w.r.t. the network input: dtype of x_in; layout of x_in for I3D ([B,T/2,H/2,W/2,32]); VideoResNet plans ALWAYS
 * [B,T,H/2,W/2,16] -- the gradient of x_adv -- also where the bf16 input has 32 channels (hi | lo) */
int flk_net_backward(flk_net* n, const float* dlogits, void* gx_in, void* stream);
/* backward straight to the flickering perturbation: the plan without the stem's data-gradient, then flk_stem_delta_grad on the
 * stem's output gradient.  gdelta fp32 [T,3]; scratch: flk_stem_delta_grad_scratch_bytes(B, T, H).  I3D in bf16 only
 * (flk_net_has_backward_delta() tells); `a` = the flk_apply_args the clip of this forward pass was applied with.  Quantised arguments
 * (a->q_lut with a->center = 0; also flk_net_prepare_backward_delta): the straight-through gradient -- the clip mask of the same arguments,
 * the same bits as without q_lut; center != 0 with q_lut is FLK_EINVAL. */
int flk_net_has_backward_delta(const flk_net* n);
int flk_net_backward_delta(flk_net* n, const float* dlogits, const flk_apply_args* a, float* gdelta, float* scratch, void* stream);
/* optional, before the forward pass of the same iteration: start the clip-mask pre-pass of the coming flk_net_backward_delta(a, scratch)
 * on the plan's own side stream (the mask depends on the clip and on delta only: kinetics_i3d_utils.py:100-142's clip_by_value
 * gradient), so that it runs beside the stem instead of beside the first kernels of the backward pass.  Same `a` contents and same
 * `scratch` as the backward call, which otherwise computes the mask itself. */
int flk_net_prepare_backward_delta(flk_net* n, const flk_apply_args* a, float* scratch, void* stream);
/* per-layer HIP-event timing of the next forward/backward (bench.py roofline leg).  While enabled the plan runs serially on
 * the caller's stream (normally independent Inception branches run on parallel streams; FLK_SINGLE_STREAM=1 disables that). */
int flk_net_profile(flk_net* n, int enable);
/* one serial forward + backward with flk_conv_set_autotune(1): tunes the launch layout of every convolution of the plan on
 * its real operands (x_in / dlogits as for forward / backward; synchronises the stream) */
int flk_net_autotune(flk_net* n, const void* x_in, float* logits, const float* dlogits, void* gx_in, void* stream);
int flk_net_profile_read(flk_net* n, char* json_out, int64_t cap);
/* the input tensor flk_net_forward reads (it cannot check the buffer it is given): elements, channels per folded position
 * (I3D 32; VideoResNet 16 in fp32, 32 in bf16) and the flk_apply_args.fold_t that produces it (3 / 1 / 4) */
int64_t flk_net_input_numel(const flk_net* n);
int flk_net_input_channels(const flk_net* n);
int flk_net_input_fold(const flk_net* n);
int flk_net_num_classes(const flk_net* n);
/* debugging / parity: copy a named activation (fp32, NDHWC) to the host */
int flk_net_get_activation(flk_net* n, const char* name, float* host_out, int64_t cap_numel, int64_t* dims5);

/* ---- data-parallel exchange: RCCL over xGMI behind the C ABI -------------------------------------------------
 * Replaces nn.DataParallel's gather of the perturbation gradient (model.py:576-578) / the dead tf.distribute.MirroredStrategy of
 * i3d_adversarial_main_universal.py:309-312: one process per GPU, ONE in-place sum all-reduce per attack iteration of the
 * (T*3 + 3)-float payload [d(sum adv)/d(delta) | sum adv | sum p_min | sum p_max] (or of the dense gradient), issued on the
 * caller's stream.  Rank 0 obtains a 128-byte id with flk_comm_unique_id and hands it to the other ranks by any side channel
 * (the Python host uses its torch.distributed process group); every rank then calls flk_comm_create.  RCCL is loaded at run time. */
typedef struct flk_comm flk_comm;
int flk_comm_unique_id(void* id128_out);
int flk_comm_create(const void* id128, int rank, int world, int device, flk_comm** out);
int flk_allreduce_sum_f32(flk_comm* c, float* buf, int64_t n, void* stream);
int flk_comm_destroy(flk_comm* c);

#ifdef __cplusplus
}
#endif
#endif
