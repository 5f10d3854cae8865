"""Thin host-side wrappers over the C ABI (include/flicker_hip.h): torch tensors are used for device
memory and streams only; every computation happens in libflicker_hip.so."""
import ctypes as C
import functools
import json
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import (FLK_BF16, FLK_F32, FLK_NET_I3D, FLK_PREP_MAX_CLIPS, AdamArgs, ApplyArgs, ConvArgs, DenseAdamArgs, ExportArgs, IllumArgs, LossArgs, PoolArgs, PrepareArgs, PrepBox,
                   PrepClip, check, dtype_code, load, ptr, stream_ptr, torch_dtype)
from .videoresnet_spec import DEFAULT_MEAN, DEFAULT_STD, prepare_geometry


def same_pad(n, k, s):
    """TF SAME: (out, pad_before); the extra pad goes after."""
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return out, tot // 2


class _HandleOwner:
    """owns ``self.handle``, an object of the library that ``_destroy`` (the name of a C function) frees -- once, when the owner goes"""
    _destroy = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                getattr(load(), self._destroy)(self.handle)
                self.handle = None
        except Exception:      # interpreter shutdown
            pass


class ConvWeights(_HandleOwner):
    """Packed weights of one convolution operator (flk_conv_weights)."""
    _destroy = "flk_conv_weights_destroy"

    def __init__(self, w_dhwio, dtype, nf, row_scale=None, transpose=False, cin_split=0):
        w = np.ascontiguousarray(w_dhwio, dtype=np.float32)
        assert w.ndim == 5
        self.kt, self.kh, self.kw, cin, cout = w.shape
        self.cin, self.cout = (cout, cin) if transpose else (cin, cout)
        self.dtype, self.nf = dtype_code(dtype), nf
        rs = None if row_scale is None else np.ascontiguousarray(row_scale, dtype=np.float32)
        h = C.c_void_p()
        if cin_split:
            assert not transpose
            check(load().flk_conv_weights_create_split(ptr(w), self.kt, self.kh, self.kw, cin, cout, ptr(rs), cin_split,
                                                       self.dtype, nf, C.byref(h)))
        else:
            check(load().flk_conv_weights_create(ptr(w), self.kt, self.kh, self.kw, cin, cout, ptr(rs), int(transpose),
                                                 self.dtype, nf, C.byref(h)))
        self.cin_split = cin_split
        self.handle = h

    @classmethod
    def s2d_stem(cls, w_folded, dtype, nf):
        """folded 7x7x7/2 stem: [4,4,4,32,cout] in the fold_t = 3 channel order (flk_conv_weights_create_s2d_stem)"""
        w = np.ascontiguousarray(w_folded, dtype=np.float32)
        assert w.shape[:4] == (4, 4, 4, 32)
        self = cls.__new__(cls)
        self.kt = self.kh = self.kw = 4
        self.cin, self.cout = 32, w.shape[4]
        self.dtype, self.nf, self.cin_split = dtype_code(dtype), nf, 0
        h = C.c_void_p()
        check(load().flk_conv_weights_create_s2d_stem(ptr(w), self.cout, self.dtype, nf, C.byref(h)))
        self.handle = h
        return self


def conv3d(x, w, **kw):
    """x: [B,T,H,W,ld] channels-last; returns / fills out [B,OT,OH,OW,ld_out].  pad = pad-before per dim
    (default: TF SAME).  out_grid = logical output grid (default: SAME output size).  Keywords: conv3d_args."""
    a, out = conv3d_args(x, w, **kw)
    check(load().flk_conv3d(C.byref(a), w.handle, dtype_code(x.dtype), stream_ptr()))
    return out


def conv3d_layout(x, w, wn, da, **kw):
    """conv3d with the launch layout {wn, da} of the caller (flk_conv3d_layout): one of conv_layout_candidates(w.nf, x.dtype), (0, -1)
    being the heuristic's own launch; never the producer / consumer kernel"""
    a, out = conv3d_args(x, w, **kw)
    check(load().flk_conv3d_layout(C.byref(a), w.handle, dtype_code(x.dtype), wn, da, stream_ptr()))
    return out


def conv_layout_candidates(nf, dtype, stem4=False):
    """[(wn, da)]: the layouts the autotuner times for weights packed at nf / dtype, the heuristic (0, -1) first (no device work)"""
    wn, da = (C.c_int * 8)(), (C.c_int * 8)()
    n = load().flk_conv_layout_candidates(nf, dtype_code(dtype), int(stem4), wn, da, 8)
    assert 0 < n <= 8
    return [(wn[i], da[i]) for i in range(n)]


_PLAN_ROUTES = ("halo", "t3", "t3_tiled", "dma1x1")


def _plan_dict(p):
    return dict(route=_PLAN_ROUTES[p.route], nf=p.nf, wn=p.wn, mode=p.mode, template_mode=p.template_mode, ksplit=p.ksplit,
                tile=(p.Tt, p.Ht, p.Wt), rows=p.rows, halo=p.halo, wgs=p.wgs)


def conv_plan_query(a, nf, dtype, *, stem4=False, cin_split=0, wn=0, da=-1, splitk=False):
    """what the planner decides for flk_conv3d(a, weights packed at nf / dtype) under the requested layout (flk_conv_plan_query; no
    weights, no device work): dict(route, nf, wn, mode, template_mode, ksplit, tile, rows, halo, wgs)"""
    p = _lib.ConvPlanInfo()
    check(load().flk_conv_plan_query(C.byref(a), nf, dtype_code(dtype), int(stem4), cin_split, wn, da, int(splitk), C.byref(p)))
    return _plan_dict(p)


def conv_group_plan_query(args, nfs, nfw, ring, dtype):
    """(body mode, [member plans]) of flk_conv3d_group over the flk_conv_args `args` with weights packed at `nfs` (no device work)"""
    n = len(args)
    ap = (C.POINTER(ConvArgs) * n)(*[C.pointer(a) for a in args])
    body, plans = C.c_int(), (_lib.ConvPlanInfo * n)()
    check(load().flk_conv_group_plan_query(ap, (C.c_int * n)(*nfs), n, nfw, int(ring), dtype_code(dtype), C.byref(body), plans))
    return body.value, [_plan_dict(p) for p in plans]


def conv3d_group(members, nfw, ring=False):
    """members: [(x, w, kwargs)] -- up to three multi-tap bf16 convolutions in ONE launch (flk_conv3d_group); returns their outputs.
    ring: the members take the LDS weight ring (all packed with nf == nfw) instead of direct-A weights"""
    built = [conv3d_args(x, w, **kw) for x, w, kw in members]
    n = len(built)
    ap = (C.POINTER(ConvArgs) * n)(*[C.pointer(a) for a, _ in built])
    wp = (C.c_void_p * n)(*[w.handle for _, w, _ in members])
    check(load().flk_conv3d_group(ap, wp, n, nfw, int(ring), dtype_code(members[0][0].dtype), stream_ptr()))
    return [o for _, o in built]


def conv3d_pc(members):
    """members: [(x, w, kwargs)] -- up to three 3x3x3 or 1x3x3 stride-1 bf16 convolutions (weights packed with nf = 4) in ONE persistent
    launch of the producer / consumer kernel (flk_conv3d_pc); returns their outputs.  Bitwise the outputs of conv3d."""
    built = [conv3d_args(x, w, **kw) for x, w, kw in members]
    n = len(built)
    ap = (C.POINTER(ConvArgs) * n)(*[C.pointer(a) for a, _ in built])
    wp = (C.c_void_p * n)(*[w.handle for _, w, _ in members])
    check(load().flk_conv3d_pc(ap, wp, n, dtype_code(members[0][0].dtype), stream_ptr()))
    return [o for _, o in built]


def conv3d_args(x, w, *, in_coff=0, cin=None, stride=(1, 1, 1), pad=None, out=None, out_coff=0, out_grid=None,
                out_stride=(1, 1, 1), out_offset=(0, 0, 0), scale=None, bias=None, add=None, add_coff=0, mask=None,
                mask_coff=0, relu=False, in2=None, in2_coff=0, out2=None, out2_coff=0, cout1=0, splitk=False, pos_bias=None):
    """the flk_conv_args of conv3d(x, w, ...) and the output tensor it will fill"""
    B, Ti, Hi, Wi, in_ld = x.shape
    cin = w.cin if cin is None else cin
    k = (w.kt, w.kh, w.kw)
    if pad is None:
        pad = tuple(same_pad(n, kk, s)[1] for n, kk, s in zip((Ti, Hi, Wi), k, stride))
    if out_grid is None:
        out_grid = tuple(same_pad(n, kk, s)[0] for n, kk, s in zip((Ti, Hi, Wi), k, stride))
    if out is None:
        phys = tuple((g - 1) * os_ + oo + 1 for g, os_, oo in zip(out_grid, out_stride, out_offset))
        out = torch.zeros((B, *phys, w.cout + out_coff), dtype=x.dtype, device=x.device)
    a = ConvArgs()
    a.in_, a.in_ld, a.in_coff, a.cin = ptr(x), in_ld, in_coff, cin
    a.B, a.Ti, a.Hi, a.Wi = B, Ti, Hi, Wi
    a.kt, a.kh, a.kw = k
    a.st, a.sh, a.sw = stride
    a.pt, a.ph, a.pw = pad
    a.To, a.Ho, a.Wo = out_grid
    a.out, a.out_ld, a.out_coff, a.cout = ptr(out), out.shape[4], out_coff, w.cout
    a.OT, a.OH, a.OW = out.shape[1:4]
    a.ost, a.osh, a.osw = out_stride
    a.oot, a.ooh, a.oow = out_offset
    a.scale, a.bias = ptr(scale), ptr(bias)
    if add is not None:
        a.add, a.add_ld, a.add_coff = ptr(add), add.shape[4], add_coff
    if mask is not None:
        a.mask, a.mask_ld, a.mask_coff = ptr(mask), mask.shape[4], mask_coff
    a.relu = int(relu)
    if pos_bias is not None:     # fp32 [1 or B, To, 4, 4, cout] position-class bias (flk_stem_delta_bias)
        a.pos_bias = ptr(pos_bias)
        a.pos_bias_bstride = pos_bias[0].numel() if pos_bias.shape[0] > 1 else 0
    if in2 is not None:
        a.in2, a.in2_ld, a.in2_coff, a.cin1 = ptr(in2), in2.shape[4], in2_coff, w.cin_split
    if out2 is not None:
        a.out2, a.out2_ld, a.out2_coff, a.cout1 = ptr(out2), out2.shape[4], out2_coff, cout1
    if splitk:           # workspace for deterministic split-K (used only where the launch would leave most CUs idle)
        nbytes = load().flk_conv_splitk_bytes(C.byref(a), w.handle)
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            a.splitk_ws, a.splitk_ws_bytes = ptr(ws), nbytes
            a._keepalive = ws
    return a, out


def _pool_args(x, C_, k, s, pad, out, idx, in_coff=0, out_coff=0):
    B, Ti, Hi, Wi, ld = x.shape
    a = PoolArgs()
    a.in_, a.in_ld, a.in_coff, a.C = ptr(x), ld, in_coff, C_
    a.B, a.Ti, a.Hi, a.Wi = B, Ti, Hi, Wi
    a.kt, a.kh, a.kw = k
    a.st, a.sh, a.sw = s
    a.pt, a.ph, a.pw = pad
    a.To, a.Ho, a.Wo = out.shape[1:4]
    a.out, a.out_ld, a.out_coff = ptr(out), out.shape[4], out_coff
    a.idx = ptr(idx)
    return a


def maxpool3d(x, k, s, C_=None, relu_input=False, *, in_coff=0, out=None, out_coff=0):
    """tf.nn.max_pool3d SAME of channels [in_coff, in_coff + C_) of x.  Returns (out, idx uint8, ctx) with ctx for maxpool3d_bwd.
    out: a [B,To,Ho,Wo,ld] buffer whose channels [out_coff, out_coff + C_) are filled (default: a fresh [.., C_] tensor)."""
    B, Ti, Hi, Wi, ld = x.shape
    C_ = ld - in_coff if C_ is None else C_
    og, pad = zip(*(same_pad(n, kk, ss) for n, kk, ss in zip((Ti, Hi, Wi), k, s)))
    if out is None:
        out = torch.empty((B, *og, C_ + out_coff), dtype=x.dtype, device=x.device)
    assert tuple(out.shape[:4]) == (B, *og) and out.dtype == x.dtype and in_coff + C_ <= ld and out_coff + C_ <= out.shape[4]
    idx = torch.empty((B, *og, C_), dtype=torch.uint8, device=x.device)
    a = _pool_args(x, C_, k, s, pad, out, idx, in_coff, out_coff)
    a.relu_input = int(relu_input)
    check(load().flk_maxpool3d_fwd(C.byref(a), dtype_code(x.dtype), stream_ptr()))
    return out, idx, (x, C_, k, s, pad, out, idx, in_coff, out_coff)


def maxpool3d_bwd(ctx, gout, mask=None, *, gout_coff=0, gin=None, gin_coff=0, mask_coff=0):
    """MaxPool3DGrad: gout[..., gout_coff:gout_coff+C_] scattered by ctx's argmax bytes into gin[..., gin_coff:gin_coff+C_] (default: a
    fresh [.., C_] tensor), masked by mask[..., mask_coff:mask_coff+C_] > 0 if a mask is given."""
    x, C_, k, s, pad, out, idx, in_coff, out_coff = ctx
    if gin is None:
        gin = torch.empty((*x.shape[:4], C_ + gin_coff), dtype=x.dtype, device=x.device)
    assert gin.shape[:4] == x.shape[:4] and gin.dtype == x.dtype and gin_coff + C_ <= gin.shape[4] and gout_coff + C_ <= gout.shape[4]
    assert mask is None or mask_coff + C_ <= mask.shape[4]
    a = _pool_args(x, C_, k, s, pad, out, idx, in_coff, out_coff)
    check(load().flk_maxpool3d_bwd(C.byref(a), ptr(gout), gout.shape[4], gout_coff, ptr(gin), gin.shape[4], gin_coff, ptr(mask),
                                   0 if mask is None else mask.shape[4], mask_coff, dtype_code(x.dtype), stream_ptr()))
    return gin


class PoolGemmWeights(_HandleOwner):
    """MFMA-packed Wt [K][C] (a 1x1x1 unit's weight transposed x batch-norm scale) for maxpool3d_bwd_gemm"""
    _destroy = "flk_pool_gemm_weights_destroy"

    def __init__(self, wt_kc):
        w = np.ascontiguousarray(wt_kc, dtype=np.float32)
        self.K, self.C = w.shape
        self.handle = C.c_void_p()
        check(load().flk_pool_gemm_weights_create(w.ctypes.data_as(C.c_void_p), self.K, self.C, C.byref(self.handle)))


def maxpool3d_bwd_gemm(ctx, g, weights, g_coff=0, *, gin=None, gin_coff=0):
    """Branch_3 backward in one kernel (bf16): gin[..., gin_coff:gin_coff+C_] = MaxPool3DGrad(idx, g[..., g_coff:g_coff+K] @ Wt); ctx from
    maxpool3d"""
    x, C_, k, s, pad, out, idx, in_coff, out_coff = ctx
    assert x.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and weights.C == C_
    if gin is None:
        gin = torch.empty((*x.shape[:4], C_ + gin_coff), dtype=x.dtype, device=x.device)
    assert gin.shape[:4] == x.shape[:4] and gin.dtype == x.dtype and gin_coff + C_ <= gin.shape[4]
    a = _pool_args(x, C_, k, s, pad, out, idx, in_coff, out_coff)
    check(load().flk_maxpool3d_bwd_gemm(C.byref(a), ptr(g), g.shape[4], g_coff, weights.K, weights.handle, ptr(gin), gin.shape[4], gin_coff,
                                        dtype_code(x.dtype), stream_ptr()))
    return gin


def maxpool3d_conv1x1_eligible(shape, C_, cin, cout, dtype, *, k=(1, 3, 3), s=(1, 2, 2), has_mask=False):
    """host-only: do the fused MaxPool3d_2a + Conv3d_2b kernels take a k / s SAME pool over C_ channels of a [B,T,H,W] grid followed by a
    1x1x1 cin -> cout unit?  (flk_maxpool3d_conv1x1_eligible; no GPU needed)"""
    B, Ti, Hi, Wi = shape
    a = PoolArgs()
    a.C = C_
    a.B, a.Ti, a.Hi, a.Wi = B, Ti, Hi, Wi
    a.kt, a.kh, a.kw = k
    a.st, a.sh, a.sw = s
    (a.To, a.pt), (a.Ho, a.ph), (a.Wo, a.pw) = (same_pad(n, kk, ss) for n, kk, ss in zip((Ti, Hi, Wi), k, s))
    return bool(load().flk_maxpool3d_conv1x1_eligible(C.byref(a), cin, cout, int(has_mask), dtype_code(dtype)))


def maxpool3d_conv1x1(x, w, *, scale=None, bias=None, relu=False, relu_input=False, in_coff=0, out=None, out_coff=0, pool_out=None,
                      pool_out_coff=0):
    """(1,3,3) / (1,2,2) SAME max-pool of channels [in_coff, in_coff + 64) of x followed by the 1x1x1 unit w (64 -> 64) in ONE kernel
    (flk_maxpool3d_fwd_conv1x1).  Returns (out, idx, ctx): out[..., out_coff:out_coff+64] the unit's output, idx the pool's argmax bytes,
    ctx for maxpool3d_bwd / maxpool3d_bwd_conv1x1.  pool_out: a buffer whose channels [pool_out_coff, +64) also receive the pooled map."""
    B, Ti, Hi, Wi, ld = x.shape
    k, s = (1, 3, 3), (1, 2, 2)
    og, pad = zip(*(same_pad(n, kk, ss) for n, kk, ss in zip((Ti, Hi, Wi), k, s)))
    if out is None:
        out = torch.empty((B, *og, 64 + out_coff), dtype=x.dtype, device=x.device)
    idx = torch.empty((B, *og, 64), dtype=torch.uint8, device=x.device)
    assert tuple(out.shape[:4]) == (B, *og) and out.dtype == x.dtype
    assert pool_out is None or (tuple(pool_out.shape[:4]) == (B, *og) and pool_out.dtype == x.dtype)
    a = _pool_args(x, 64, k, s, pad, out if pool_out is None else pool_out, idx, in_coff, pool_out_coff)
    if pool_out is None:
        a.out, a.out_ld, a.out_coff = None, 64, 0
    a.relu_input = int(relu_input)
    check(load().flk_maxpool3d_fwd_conv1x1(C.byref(a), w.handle, ptr(scale), ptr(bias), int(relu), ptr(out), out.shape[4], out_coff,
                                           int(pool_out is not None), dtype_code(x.dtype), stream_ptr()))
    return out, idx, (x, 64, k, s, pad, out if pool_out is None else pool_out, idx, in_coff, pool_out_coff)


def maxpool3d_bwd_conv1x1(ctx, g, wb, *, g_coff=0, gin=None, gin_coff=0, gpool=None, gpool_coff=0):
    """the 1x1x1 unit's data-gradient (wb: its transposed weights, 64 -> 64, no mask) followed by the (1,3,3) / (1,2,2) MaxPool3DGrad in ONE
    kernel (flk_maxpool3d_bwd_conv1x1): g[..., g_coff:g_coff+64] -> gin[..., gin_coff:gin_coff+64].  gpool: a buffer whose channels
    [gpool_coff, +64) also receive the pooled map's gradient.  ctx from maxpool3d or maxpool3d_conv1x1."""
    x, C_, k, s, pad, out, idx, in_coff, out_coff = ctx
    if gin is None:
        gin = torch.empty((*x.shape[:4], C_ + gin_coff), dtype=x.dtype, device=x.device)
    assert gin.shape[:4] == x.shape[:4] and gin.dtype == x.dtype and g.shape[:4] == idx.shape[:4]
    assert gpool is None or (gpool.shape[:4] == idx.shape[:4] and gpool.dtype == x.dtype)
    a = _pool_args(x, C_, k, s, pad, out, idx, in_coff, out_coff)
    check(load().flk_maxpool3d_bwd_conv1x1(C.byref(a), ptr(g), g.shape[4], g_coff, wb.handle, ptr(gin), gin.shape[4], gin_coff, ptr(gpool),
                                           0 if gpool is None else gpool.shape[4], gpool_coff, dtype_code(x.dtype), stream_ptr()))
    return gin


I3D_FOLD = 3   # space-to-depth layout the I3D plan (flk_net, FLK_NET_I3D) expects: chunk-aligned (t,h,w) fold


def quant_table_host(dialect):
    """fp32 [256,3]: what byte v of channel c decodes to in a dialect of EXPORT_DIALECTS -- torch: videoresnet_spec.u8_decode_table
    ((v / 255 - mean) / std); TF: v / 128 - 1 (exact in float32)"""
    if dialect not in EXPORT_DIALECTS:
        raise ValueError(f"dialect must be one of {sorted(EXPORT_DIALECTS)}, got {dialect!r}")
    if dialect == "torch":
        from .videoresnet_spec import u8_decode_table
        return u8_decode_table()
    return np.ascontiguousarray(np.repeat((np.arange(256, dtype=np.float32) / np.float32(128.0) - np.float32(1.0))[:, None], 3, axis=1))


_QUANT_TABLES = {}


def quant_table(dialect, device):
    """``quant_table_host(dialect)`` on ``device`` (flk_apply_args.q_lut): one copy per device -- the torch dialect's is the decode table
    the uint8 clips already go through (torch_attack.decode_table)"""
    if dialect not in EXPORT_DIALECTS:
        raise ValueError(f"dialect must be one of {sorted(EXPORT_DIALECTS)}, got {dialect!r}")
    if dialect == "torch":
        from .torch_attack import decode_table
        return decode_table(device)
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _QUANT_TABLES:
        _QUANT_TABLES[key] = torch.from_numpy(quant_table_host("tf")).to(torch.device(dev.type, key[1]))
    return _QUANT_TABLES[key]


def make_apply_args(x, delta, *, dialect="tf", dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0, inv_std=(1.0, 1.0, 1.0),
                    lo=-1.0, hi=1.0, fold_t=2, center=False, dclip_dev=None, x_lut=None, quantise=None, q_lut=None, per_line=False):
    """x: uint8 or fp32 [B,T,H,W,3] on the GPU; delta fp32 [T,3] (flicker, shared by the batch), [B,T,3] (one flicker perturbation PER
    CLIP: independent single-video attacks advancing in one batch) or [T,H,W,3] (dense).  per_line=True (fold_t 1 and 4, no centre):
    delta is fp32 [T,H,3] or [B,T,H,3] -- one value per LINE of a frame (flk_apply_args.delta_per_line, ``flicker_lines_mix`` makes it);
    named by the keyword because a 4-D delta means dense.  x_lut: fp32 [256,3] on the device (uint8 x
    only): byte v of channel c decodes to x_lut[v, c] (videoresnet_spec.u8_decode_table) instead of the dialect's scalar decode.
    quantise: None, or the dialect ("torch" | "tf") of EXPORT_DIALECTS whose 8-bit round trip the apply kernels put every value through
    (flk_apply_args.q_lut: the clip the network sees is the STORED video; the gradient is the straight-through estimator, which the
    gradient kernels already compute).  q_lut: its decode table, fp32 [256,3] on the device (default: ``quant_table``)."""
    if quantise is not None:
        if quantise not in EXPORT_DIALECTS:
            raise ValueError(f"quantise must be None or one of {sorted(EXPORT_DIALECTS)}, got {quantise!r}")
        if center:
            raise ValueError("quantise: the centred clip (center=True) carries the perturbation in the stem's position bias -- there is no "
                             "per-pixel value to round")
        if q_lut is None:
            q_lut = quant_table(quantise, x.device)
        if not (torch.is_tensor(q_lut) and q_lut.dtype == torch.float32 and tuple(q_lut.shape) == (256, 3) and q_lut.is_contiguous() and q_lut.is_cuda):
            raise ValueError("q_lut: fp32 [256,3] on the device")
    elif q_lut is not None:
        raise ValueError("q_lut without quantise: name the dialect whose encode goes with the table")
    assert x_lut is None or not center, "x_lut: uint8 clips, center = False"
    a = _fill_apply_args(x, delta, dialect, dclip, adv_flag, shift_x, shift_p, inv_std, lo, hi, dclip_dev, x_lut, per_line)
    B, T, H, W = a.B, a.T, a.H, a.W
    if per_line:
        if tuple(delta.shape) not in ((T, H, 3), (B, T, H, 3)):
            raise ValueError(f"per_line: delta must be fp32 [{T},{H},3] or [{B},{T},{H},3], got {tuple(delta.shape)}")
        if center or fold_t not in (1, 4):
            raise ValueError(f"per_line: fold_t 1 or 4 without center (the VideoResNet layouts), got fold_t {fold_t}, center {center}")
    else:
        assert tuple(delta.shape) in ((T, 3), (B, T, 3), (T, H, W, 3)), delta.shape
    assert not (a.delta_per_clip and (shift_x or shift_p)), "per-clip perturbations: cyclic rolls are drawn per run in the reference; not batched"
    a.fold_t = fold_t
    a.center = int(center)      # write x_adv - a*p' (the clean value where the clip is inactive); see Net.forward_flicker
    if quantise is not None:    # the encode of make_export_args(quantise), the decode of q_lut
        mul, add, levels = EXPORT_DIALECTS[quantise]
        a.q_lut, a.q_mul, a.q_add, a.q_levels = ptr(q_lut), (C.c_float * 3)(*mul), (C.c_float * 3)(*add), levels
        a._keepalive += (q_lut,)
    return a


def _fill_apply_args(x, delta, dialect, dclip, adv_flag, shift_x, shift_p, inv_std, lo, hi, dclip_dev, x_lut, per_line):
    """the flk_apply_args that ``make_apply_args`` and ``make_export_apply_args`` share: the clip, its decode, the perturbation (its rank
    names the form; the caller checks the shape) and the scalars of the pixel model.  The fold, ``center``, the quantiser and
    the period stay with the callers."""
    B, T, H, W, c3 = x.shape
    assert c3 == 3 and x.is_contiguous() and delta.is_contiguous() and delta.dtype == torch.float32
    assert x.dtype in (torch.uint8, torch.float32)
    if x_lut is not None:
        assert x.dtype == torch.uint8, "x_lut: uint8 clips, center = False"
        assert x_lut.dtype == torch.float32 and tuple(x_lut.shape) == (256, 3) and x_lut.is_contiguous() and x_lut.is_cuda, "x_lut: fp32 [256,3] on the device"
    # the torch dialect's clips are normalised per channel: a uint8 clip without its table would be read as values 0..255
    assert not (dialect == "torch" and x.dtype == torch.uint8 and x_lut is None), "torch dialect: a uint8 clip needs x_lut (its decode table)"
    a = ApplyArgs()
    a.x, a.x_is_u8 = ptr(x), int(x.dtype == torch.uint8)
    # TFRecord path: x = u8/128 - 1 (pre_process_rgb_flow.py:226-234)
    a.x_scale, a.x_bias = (1.0 / 128.0, -1.0) if dialect == "tf" else (1.0, 0.0)
    a.delta = ptr(delta)
    if per_line:
        a.delta_dense, a.delta_per_clip, a.delta_per_line = 0, int(delta.dim() == 4), 1
    else:
        a.delta_dense, a.delta_per_clip = int(delta.dim() == 4), int(delta.dim() == 3)
    a.dclip = float(dclip)
    a.inv_std = (C.c_float * 3)(*inv_std)
    a.lo, a.hi, a.adv_flag = float(lo), float(hi), float(adv_flag)
    a.shift_x, a.shift_p = int(shift_x), int(shift_p)
    a.B, a.T, a.H, a.W = B, T, H, W
    if dclip_dev is not None:   # per-clip clamp bounds (fp32 [B] on the device), per-clip perturbations only
        assert a.delta_per_clip and dclip_dev.dtype == torch.float32 and dclip_dev.shape == (B,) and dclip_dev.is_cuda
    a.dclip_dev, a.x_lut = ptr(dclip_dev), ptr(x_lut)
    a._keepalive = (x, delta, dclip_dev, x_lut)   # the struct holds raw pointers only
    return a


def perturb_apply_s2d(args, dtype, out=None):
    if out is None:
        ft = 1 if args.fold_t in (1, 4) else 2
        out = torch.empty((args.B, args.T // ft, args.H // 2, args.W // 2, 32 if args.fold_t == 4 else 16 * ft), dtype=torch_dtype(dtype_code(dtype)),
                          device="cuda")
    check(load().flk_perturb_apply_s2d(C.byref(args), ptr(out), dtype_code(dtype), stream_ptr()))
    return out


# 8-bit export (flk_adv_export_u8): dialect -> (mul[3], add[3], levels), the inverse of the dialect's decode
EXPORT_DIALECTS = {"torch": (DEFAULT_STD, DEFAULT_MEAN, 255.0),          # inverse of (u8 / 255 - mean) / std
                   "tf": ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 128.0)}      # inverse of u8 / 128 - 1


def make_export_args(dialect, out_clip_stride, out_offset=0, delta_T=0):
    """flk_export_args of a dialect: clip b of the call goes to row ``out_offset + b`` of a buffer whose rows are ``out_clip_stride``
    bytes apart; ``delta_T``: the period of a flicker perturbation [delta_T,3] laid over a longer (or shorter) clip, 0 = the clip's T"""
    if dialect not in EXPORT_DIALECTS:
        raise ValueError(f"dialect must be one of {sorted(EXPORT_DIALECTS)}, got {dialect!r}")
    mul, add, levels = EXPORT_DIALECTS[dialect]
    e = ExportArgs()
    e.mul, e.add, e.levels = (C.c_float * 3)(*mul), (C.c_float * 3)(*add), levels
    e.delta_T, e.out_clip_offset, e.out_clip_stride = int(delta_T), int(out_offset), int(out_clip_stride)
    return e


def make_export_apply_args(x, delta, *, dialect="tf", dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0, inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0,
                           dclip_dev=None, x_lut=None, delta_T=0, per_line=False):
    """the flk_apply_args of an 8-bit export: ``make_apply_args`` without a fold (T, H and W may be odd) and, with ``delta_T``, with a
    flicker perturbation [delta_T,3] whose length is its period instead of the clip's T.  (The fields are filled by the filler ``make_apply_args``
    uses, ``_fill_apply_args``; only the fold, ``center`` and the shape rule of ``delta`` differ, and there is no
    ``quantise``: the export is the quantiser itself, and ``make_apply_args(quantise=dialect)`` applies the clip these bytes decode to.)  The period is
    remembered on the result (``_delta_T``): ``export_adversarial_u8`` takes it from there.  per_line=True: delta is fp32 [T,H,3], [B,T,H,3]
    or, with ``delta_T``, [delta_T,H,3] -- one value per line of a frame (flk_apply_args.delta_per_line)."""
    B, T, H, W, _ = x.shape
    assert x.is_cuda and delta.is_cuda and min(B, T, H, W) > 0
    a = _fill_apply_args(x, delta, dialect, dclip, adv_flag, shift_x, shift_p, inv_std, lo, hi, dclip_dev, x_lut, per_line)
    if per_line:
        want = ((int(delta_T), H, 3),) if delta_T else ((T, H, 3), (B, T, H, 3))
        if tuple(delta.shape) not in want:
            raise ValueError(f"per_line (delta_T = {delta_T}): delta must be fp32 {' or '.join(str(list(w)) for w in want)}, got {tuple(delta.shape)}")
    elif delta_T:
        assert tuple(delta.shape) == (int(delta_T), 3), f"delta_T = {delta_T}: the perturbation must be [{delta_T},3], got {tuple(delta.shape)}"
    else:
        assert tuple(delta.shape) in ((T, 3), (B, T, 3), (T, H, W, 3)), delta.shape
    a._delta_T = int(delta_T)                     # the kernel must wrap by the length delta really has
    return a


def export_adversarial_u8(args, dialect="tf", out=None, out_offset=0, stats=False, delta_T=None):
    """the perturbed clip of ``args`` (make_export_apply_args, or make_apply_args: the fold is ignored) as uint8 frames [B,T,H,W,3] in one
    launch (flk_adv_export_u8).  ``out``: a contiguous CUDA uint8 buffer [>= out_offset + B, T, H, W, 3] whose rows ``out_offset ...`` are
    written (the others are left alone); without it a tensor [B,T,H,W,3] is allocated.  Returns the rows written; with ``stats`` also the
    int32 [B,T,3,4] table of per (clip, frame, channel) sums: q - q_clean, |q - q_clean|, [q != q_clean], [clamp active].
    ``delta_T``: the period the arguments were built with (default); naming another one is an error -- the kernel would read past a
    perturbation of ``delta_T`` rows."""
    return _export_u8("export_adversarial_u8", args, dialect, out, out_offset, stats, delta_T,
                      lambda e, out, st: load().flk_adv_export_u8(C.byref(args), C.byref(e), ptr(out), ptr(st), stream_ptr()))


def _export_u8(what, args, dialect, out, out_offset, stats, delta_T, launch):
    """the host half of the two 8-bit exports (``what`` names the caller in a refusal): the period must be the one ``args`` were built
    with, ``out`` is allocated or checked, ``launch(export_args, out, stats_table)`` runs the kernel; returns the rows written, with
    ``stats`` also the table"""
    B, T, H, W = args.B, args.T, args.H, args.W
    built = getattr(args, "_delta_T", 0)
    if delta_T is None:
        delta_T = built
    if int(delta_T) != built:
        raise ValueError(f"{what}: delta_T = {delta_T}, but the arguments were built for delta_T = {built}")
    dev = args._keepalive[0].device
    if out is None:
        out = torch.empty((out_offset + B, T, H, W, 3), dtype=torch.uint8, device=dev)
    if (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != 5
            or tuple(out.shape[1:]) != (T, H, W, 3) or out_offset < 0 or out.shape[0] < out_offset + B):
        desc = f"{tuple(out.shape)} {out.dtype}" if torch.is_tensor(out) else type(out).__name__
        raise ValueError(f"{what}: out must be a contiguous CUDA uint8 tensor [>= {out_offset + B},{T},{H},{W},3], got {desc}")
    e = make_export_args(dialect, T * H * W * 3, out_offset, delta_T)
    st = torch.empty((B, T, 3, 4), dtype=torch.int32, device=dev) if stats else None
    check(launch(e, out, st))
    rows = out[out_offset:out_offset + B]
    return (rows, st) if stats else rows


def encode_u8_host(v, dialect):
    """numpy float32 restatement of the encode of flk_adv_export_u8 (one rounded operation per step): fp32 [...,3] -> uint8"""
    from . import i3d_spec, videoresnet_spec
    return {"torch": videoresnet_spec.encode_u8, "tf": i3d_spec.encode_u8}[dialect](v)


def export_adversarial_u8_host(x, delta, *, dialect="tf", dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0, inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0,
                               dclip_clip=None, x_lut=None, delta_T=0, stats=False):
    """the host A/B route of ``export_adversarial_u8``: the same arithmetic in numpy float32, one rounded operation per step (exact for
    adv_flag 0 / 1, where no contraction can change the apply).  x: uint8 or fp32 [B,T,H,W,3]; delta: [T,3], [B,T,3], [T,H,W,3] or, with
    ``delta_T``, [delta_T,3]; ``dclip_clip``: per-clip clamp bounds [B]; ``x_lut``: fp32 [256,3].  Returns the frames uint8 [B,T,H,W,3]
    and, with ``stats``, the int64 [B,T,3,4] sums of flk_adv_export_u8."""
    x, d = np.asarray(x), np.asarray(delta, dtype=np.float32)
    B, T = x.shape[:2]
    f32 = np.float32
    if x.dtype == np.uint8:
        xf = np.asarray(x_lut, f32)[x, np.arange(3)] if x_lut is not None else \
            (x.astype(f32) * (f32(1.0 / 128.0) if dialect == "tf" else f32(1.0)) + (f32(-1.0) if dialect == "tf" else f32(0.0))).astype(f32)
    else:
        xf = x.astype(f32)
    xf, xsrc = np.roll(xf, shift_x, axis=1), np.roll(x, shift_x, axis=1)         # x'[t] = x[(t - shift_x) mod T]
    rows = (np.arange(T) - shift_p) % (int(delta_T) or T)                        # p'[t] = p[(t - shift_p) mod period]
    p = d[rows] if d.ndim == 4 else d[:, rows][:, :, None, None, :] if d.ndim == 3 else d[rows][None, :, None, None, :]
    dc = np.asarray(dclip_clip, f32).reshape(B, 1, 1, 1, 1) if dclip_clip is not None else f32(dclip)
    if dclip_clip is not None or dclip > 0:
        p = np.minimum(np.maximum(p, -dc), dc)
    p = (p * np.array(inv_std, f32)).astype(f32)
    pv = f32(adv_flag) * p if adv_flag != 0 else np.zeros_like(p)
    u = (xf + pv).astype(f32)
    q = encode_u8_host(np.minimum(np.maximum(u, f32(lo)), f32(hi)), dialect)
    if not stats:
        return q
    qc = xsrc if x.dtype == np.uint8 else encode_u8_host(xf, dialect)
    dq = q.astype(np.int64) - qc.astype(np.int64)
    active = (u < f32(lo)) | (u > f32(hi))
    st = np.stack([dq.sum((2, 3)), np.abs(dq).sum((2, 3)), (dq != 0).sum((2, 3)), active.sum((2, 3))], axis=-1)
    return q, st.astype(np.int64)


def perturb_apply_quantised_host(x, delta, *, dialect="tf", dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0, inv_std=(1.0, 1.0, 1.0), lo=-1.0,
                                 hi=1.0, dclip_clip=None, x_lut=None, delta_T=0):
    """the host A/B route of a quantised apply (``make_apply_args(quantise=dialect)``), unfolded: numpy float32 [B,T,H,W,3], the bytes of
    ``export_adversarial_u8_host`` (same keywords) decoded through ``quant_table_host(dialect)`` -- what a clean forward of the stored
    video sees (no second clamp: a value held at lo / hi is stored as the level nearest the bound and comes back as that level)"""
    q = export_adversarial_u8_host(x, delta, dialect=dialect, dclip=dclip, adv_flag=adv_flag, shift_x=shift_x, shift_p=shift_p, inv_std=inv_std,
                                   lo=lo, hi=hi, dclip_clip=dclip_clip, x_lut=x_lut, delta_T=delta_T)
    return np.ascontiguousarray(quant_table_host(dialect)[q, np.arange(3)], dtype=np.float32)


def _grad_shape(args):
    """the shape of d(loss)/d(delta) for the delta of ``args``: per line [B,T,H,3] (the gradient kernels take per-clip lines only),
    dense [T,H,W,3], per clip [B,T,3], shared [T,3]"""
    return (args.B, args.T, args.H, 3) if args.delta_per_line else (args.T, args.H, args.W, 3) if args.delta_dense else \
        (args.B, args.T, 3) if args.delta_per_clip else (args.T, 3)


def perturb_grad_reduce(args, gx_s2d, gdelta=None, scratch=None):
    if gdelta is None:
        gdelta = torch.empty(_grad_shape(args), dtype=torch.float32, device="cuda")
    if scratch is None and not args.delta_dense and not args.delta_per_line:
        n = load().flk_perturb_grad_scratch_bytes(args.B, args.T, args.H, args.W)
        scratch = torch.empty(n // 4, dtype=torch.float32, device="cuda")
    check(load().flk_perturb_grad_reduce(C.byref(args), ptr(gx_s2d), dtype_code(gx_s2d.dtype), ptr(gdelta), ptr(scratch), stream_ptr()))
    return gdelta


# ---- the flicker as scene illumination (flk_illum_*): a second pixel model beside the additive one ----------------------------------
def make_illum_args(tables, device="cuda", out_mul=None, out_add=None):
    """flk_illum_args of a pair of camera tables (``videoresnet_spec.illum_tables``: dec float32 [256,3], enc float32 [N+1]; numpy
    arrays are copied to ``device``, CUDA tensors are taken as they are).  ``out_mul`` / ``out_add``: the affine map from a display
    value in [0,1] to the network's input (default: the torch dialect's 1 / std and -mean / std)."""
    from .videoresnet_spec import ILLUM_MAX_N, illum_out_affine
    dec, enc = tables
    dec = dec if torch.is_tensor(dec) else torch.from_numpy(np.ascontiguousarray(dec)).to(device)
    enc = enc if torch.is_tensor(enc) else torch.from_numpy(np.ascontiguousarray(enc)).to(device)
    if not (dec.dtype == torch.float32 and tuple(dec.shape) == (256, 3) and dec.is_contiguous() and enc.dtype == torch.float32 and enc.dim() == 1
            and 3 <= enc.shape[0] <= ILLUM_MAX_N + 1 and enc.is_contiguous() and dec.device == enc.device):
        raise ValueError(f"make_illum_args: dec fp32 [256,3] and enc fp32 [N+1] (N in 2..{ILLUM_MAX_N}) on one device, got {tuple(dec.shape)} {dec.dtype} "
                         f"and {tuple(enc.shape)} {enc.dtype}")
    mul0, add0 = illum_out_affine()
    m = IllumArgs()
    m.dec, m.enc, m.enc_n = ptr(dec), ptr(enc), int(enc.shape[0]) - 1
    m.out_mul = (C.c_float * 3)(*(mul0 if out_mul is None else out_mul))
    m.out_add = (C.c_float * 3)(*(add0 if out_add is None else out_add))
    m._keepalive = (dec, enc)      # the struct holds raw pointers only
    return m


def illum_apply_s2d(args, illum, dtype, out=None):
    """the clip of ``args`` (make_apply_args: uint8 with x_lut, fold_t 1 or 4; dclip = the largest relative modulation) lit by its
    flicker, in the folded layout of ``perturb_apply_s2d`` (flk_illum_apply_s2d)"""
    if out is None:
        out = torch.empty((args.B, args.T, args.H // 2, args.W // 2, 32 if args.fold_t == 4 else 16), dtype=torch_dtype(dtype_code(dtype)),
                          device=args._keepalive[0].device)
    check(load().flk_illum_apply_s2d(C.byref(args), C.byref(illum), ptr(out), dtype_code(dtype), stream_ptr()))
    return out


def illum_export_u8(args, illum, out=None, out_offset=0, stats=False, delta_T=None):
    """the bytes a camera stores of the clip of ``args`` (make_export_apply_args, or make_apply_args) lit by its flicker
    (flk_illum_export_u8); ``out`` / ``out_offset`` / ``stats`` / ``delta_T`` as ``export_adversarial_u8``"""
    # (the encode fields of the "torch" dialect are not read: the tables are the encode)
    return _export_u8("illum_export_u8", args, "torch", out, out_offset, stats, delta_T,
                      lambda e, out, st: load().flk_illum_export_u8(C.byref(args), C.byref(illum), C.byref(e), ptr(out), ptr(st), stream_ptr()))


def illum_grad_reduce(args, illum, gx_s2d, gdelta=None, scratch=None):
    """d(loss)/d(delta) under the illumination model from the 16-channel input gradient (flk_illum_grad_reduce): fp32 in the shape of
    the delta of ``args`` -- [T,3], [B,T,3] or, per line (per-clip only), [B,T,H,3]"""
    dev = args._keepalive[0].device
    if gdelta is None:
        gdelta = torch.empty(_grad_shape(args), dtype=torch.float32, device=dev)
    if scratch is None and not args.delta_per_line:
        scratch = torch.empty(load().flk_perturb_grad_scratch_bytes(args.B, args.T, args.H, args.W) // 4, dtype=torch.float32, device=dev)
    check(load().flk_illum_grad_reduce(C.byref(args), C.byref(illum), ptr(gx_s2d), dtype_code(gx_s2d.dtype), ptr(gdelta), ptr(scratch), stream_ptr()))
    return gdelta


# ---- training on the delivered video: tone tables and their slopes (flk_clip_prepare_toned / flk_clip_prepare_grad take them) -------
def tone_ramp(n, T, device="cuda"):
    """the constant ramp clip the tone tables are exported from: uint8 ``[n,T,16,16,3]``, pixel p of every frame holding level p in its
    three channels -- a clip that holds every (byte, channel) once per frame"""
    ramp = torch.arange(256, dtype=torch.uint8, device=device).view(1, 1, 16, 16, 1)
    return ramp.expand(int(n), int(T), 16, 16, 3).contiguous()


def _check_ramp_args(what, args):
    if (args.H, args.W) != (16, 16) or not args.x_is_u8 or not args.delta_per_clip or args.delta_per_line or args.delta_dense:
        raise ValueError(f"{what}: args must describe the ramp clip (tone_ramp: uint8 [n,T,16,16,3]) with a per-clip delta [n,T,3]")


def flicker_tone_tables(args, illum=None, out=None, dialect="torch"):
    """The tone tables of a batch of clips: uint8 ``[n,T,256,3]``, ``tone[k,t,v,c]`` = the byte the export kernel of the pixel model
    writes for source byte ``v`` of channel ``c`` under the delta row of frame ``t`` of clip ``k``.  No kernel of its own: the existing
    export launch (``export_adversarial_u8`` in ``dialect``; with ``illum`` -- ``make_illum_args`` -- ``illum_export_u8``) run on the ramp,
    so the table equals the export of a whole video bit for bit.  ``args``: ``make_export_apply_args(tone_ramp(n, T), delta_clip, ...)``
    with the per-clip delta ``[n,T,3]`` of video time (``flicker_rows_gather`` / ``flicker_rows_mix``).  ``out``: the buffer to fill."""
    _check_ramp_args("flicker_tone_tables", args)
    B, T = args.B, args.T
    dev = args._keepalive[0].device
    if out is None:
        out = torch.empty((B, T, 256, 3), dtype=torch.uint8, device=dev)
    _check_tone("flicker_tone_tables", "out", out, torch.uint8, (B, T, 256, 3), dev)
    frames = out.view(B, T, 16, 16, 3)
    if illum is not None:
        illum_export_u8(args, illum, out=frames)
    else:
        export_adversarial_u8(args, dialect, out=frames)
    return out


def flicker_tone_slopes(args, illum=None, slope=None, scale=None):
    """``(slope, scale)`` of the tone tables of ``args`` (as for ``flicker_tone_tables``; flk_flicker_tone_slopes): ``slope`` fp32
    ``[n,T,256,3]``, the straight-through derivative of the display value of source byte v with respect to the frame's delta value --
    additive: 1 where the clamp to [lo, hi] is inactive, else 0; illumination (``illum``): the weight ``(d * N) * L`` of
    ``illum_grad_reduce``, 0 where the lit value leaves [0,1] -- and ``scale`` fp32 ``[n,T,3]``, the finishing factors
    (``adv_flag * inv_std[c]`` / ``adv_flag * out_mul[c]``; 0 where the delta value lies outside its clamp).  ``prepare_clips_grad``
    resamples them."""
    _check_ramp_args("flicker_tone_slopes", args)
    B, T = args.B, args.T
    dev = args._keepalive[0].device
    if slope is None:
        slope = torch.empty((B, T, 256, 3), dtype=torch.float32, device=dev)
    if scale is None:
        scale = torch.empty((B, T, 3), dtype=torch.float32, device=dev)
    _check_tone("flicker_tone_slopes", "slope", slope, torch.float32, (B, T, 256, 3), dev)
    _check_tone("flicker_tone_slopes", "scale", scale, torch.float32, (B, T, 3), dev)
    check(load().flk_flicker_tone_slopes(C.byref(args), C.byref(illum) if illum is not None else None, ptr(slope), ptr(scale), stream_ptr()))
    return slope, scale


FLICKER_MAX_PERIOD = 682     # 3 * P values are what flk_perturb_reg_adam holds (256 threads x 8)


def _check_rows(what, rows, P, rows_host):
    """the device table of flk_flicker_rows_*: int32, contiguous, on the device, any shape (n = its element count).  ``rows_host``: the
    host copy it was uploaded from -- same shape, every entry inside [0,P) (the kernels clamp / skip a bad entry; here it is refused)"""
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or not 1 <= P <= FLICKER_MAX_PERIOD:
        raise ValueError(f"{what}: the period must be an integer in 1..{FLICKER_MAX_PERIOD}, got {P!r}")
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() >= 1):
        desc = f"{tuple(rows.shape)} {rows.dtype} on {rows.device}" if torch.is_tensor(rows) else type(rows).__name__
        raise ValueError(f"{what}: rows must be a non-empty contiguous int32 tensor on the device, got {desc}")
    if rows_host is not None:
        h = np.asarray(rows_host)
        if tuple(h.shape) != tuple(rows.shape) or h.dtype.kind not in "iu":
            raise ValueError(f"{what}: rows_host must be the integer table {tuple(rows.shape)} the device rows were uploaded from, got {h.shape} {h.dtype}")
        if h.min() < 0 or h.max() >= P:
            raise ValueError(f"{what}: rows must lie in [0,{P}), got {int(h.min())} .. {int(h.max())}")


def _check_f32(what, name, t, shape, like):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.device == like.device):
        desc = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor {tuple(shape)} on {like.device}, got {desc}")


def _check_delta(what, delta, rows, rows_host):
    """the shared perturbation of flk_flicker_*: fp32 [P,3], contiguous on the device of ``rows``, which ``_check_rows`` checks against
    its period -> P"""
    if not (torch.is_tensor(delta) and delta.dim() == 2 and delta.shape[1] == 3):
        raise ValueError(f"{what}: delta must be fp32 [P,3] on the device")
    P = int(delta.shape[0])
    _check_rows(what, rows, P, rows_host)
    _check_f32(what, "delta", delta, (P, 3), rows)
    return P


def _out_f32(what, out, shape, like):
    """``out``, the buffer a call fills: allocated on the device of ``like`` when None, checked (``_check_f32``) when given"""
    if out is None:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=like.device)
    _check_f32(what, "out", out, shape, like)
    return out


def _check_tables(what, rows, taps, gain, kmax, per_line=False):
    """the channel tables of flk_flicker_rows_mix* and, ``per_line``, flk_flicker_lines_mix*: ``rows`` [B,clip_T] (or [clip_T]: one clip),
    fp32 ``taps`` [B,K] -- per line [B,H,K] -- with K in 1..kmax and fp32 ``gain`` [B,3] or None, contiguous on rows' device
    -> (clip_T, K), per line (clip_T, H, K)"""
    if rows.dim() not in (1, 2):
        raise ValueError(f"{what}: rows must be [clips,clip_T] (or [clip_T] for one clip), got {tuple(rows.shape)}")
    nb, clip_T = (1, int(rows.shape[0])) if rows.dim() == 1 else (int(rows.shape[0]), int(rows.shape[1]))
    if not (torch.is_tensor(taps) and taps.dim() == (3 if per_line else 2) and min(taps.shape[1:]) >= 1 and taps.shape[-1] <= kmax):
        desc = f"{tuple(taps.shape)}" if torch.is_tensor(taps) else type(taps).__name__
        form = f"[{nb},H,K] with K in 1..{kmax} (one table per clip)" if per_line else f"[{nb},K] with K in 1..{kmax} (one row per clip)"
        raise ValueError(f"{what}: taps must be fp32 {form}, got {desc}")
    dims = tuple(int(v) for v in taps.shape[1:])
    _check_f32(what, "taps", taps, (nb, *dims), rows)
    if gain is not None:
        _check_f32(what, "gain", gain, (nb, 3), rows)
    return (clip_T, *dims)


def flicker_rows_gather(delta, rows, out=None, rows_host=None):
    """delta_clip[..., c] = delta[rows[...], c] (flk_flicker_rows_gather, one launch): the shared flicker perturbation ``delta`` fp32 [P,3]
    spread over the frames of a batch by their ``rows`` (int32 on the device, e.g. [B,T]; videoresnet_spec.flicker_rows makes the table)
    -> fp32 ``rows.shape + (3,)``, the per-clip perturbation ``make_apply_args`` takes.  Raw values.  ``out``: the buffer to fill."""
    what = "flicker_rows_gather"
    P = _check_delta(what, delta, rows, rows_host)
    out = _out_f32(what, out, (*rows.shape, 3), rows)
    check(load().flk_flicker_rows_gather(ptr(delta), P, ptr(rows), rows.numel(), ptr(out), stream_ptr()))
    return out


def flicker_rows_grad(g_clip, rows, period, out=None, rows_host=None):
    """g_rows[r, c] = the sum of g_clip[i, c] over the frames i with rows[i] == r (flk_flicker_rows_grad, one launch): the per-clip gradient
    of ``perturb_grad_reduce`` (fp32 ``rows.shape + (3,)``) folded back onto the rows of the shared perturbation -> fp32 [period,3].
    fp32 additions in ascending frame order from +0; a row no frame carries is 0.  ``out``: the buffer to fill."""
    what = "flicker_rows_grad"
    _check_rows(what, rows, period, rows_host)
    _check_f32(what, "g_clip", g_clip, (*rows.shape, 3), rows)
    P = int(period)
    out = _out_f32(what, out, (P, 3), rows)
    check(load().flk_flicker_rows_grad(ptr(g_clip), ptr(rows), rows.numel(), P, ptr(out), stream_ptr()))
    return out


FLICKER_MIX_MAX_TAPS = 4      # rows of the perturbation one captured frame mixes (flk_flicker_rows_mix's K)


def flicker_rows_mix(delta, rows, taps, gain=None, out=None, rows_host=None):
    """the flicker as a camera records it (flk_flicker_rows_mix, one launch, in ``flicker_rows_gather``'s place): frame t of clip b takes
    ``gain[b] * sum_k taps[b,k] * delta[(rows[b,t] + k) mod P]`` -- ``delta`` fp32 [P,3], ``rows`` int32 [B,clip_T] on the device, ``taps``
    fp32 [B,K] (K <= 4, videoresnet_spec.capture_taps / CaptureChannel.tables), ``gain`` fp32 [B,3] or None -> fp32 ``rows.shape + (3,)``.
    Raw values; every product and sum rounded on its own (videoresnet_spec.flicker_rows_mix restates it bit for bit)."""
    what = "flicker_rows_mix"
    P = _check_delta(what, delta, rows, rows_host)
    clip_T, K = _check_tables(what, rows, taps, gain, FLICKER_MIX_MAX_TAPS)
    out = _out_f32(what, out, (*rows.shape, 3), rows)
    check(load().flk_flicker_rows_mix(ptr(delta), P, ptr(rows), rows.numel(), clip_T, ptr(taps), K, ptr(gain), ptr(out), stream_ptr()))
    return out


def flicker_rows_mix_grad(g_clip, rows, period, taps, gain=None, out=None, rows_host=None):
    """the transpose of ``flicker_rows_mix`` (flk_flicker_rows_mix_grad, one launch, in ``flicker_rows_grad``'s place): the per-clip
    gradient fp32 ``rows.shape + (3,)`` folded onto the rows of the shared perturbation through the same tables -> fp32 [period,3].
    One fixed order (frames ascending, taps ascending, from +0), no atomics; a row nothing reaches is 0."""
    what = "flicker_rows_mix_grad"
    _check_rows(what, rows, period, rows_host)
    _check_f32(what, "g_clip", g_clip, (*rows.shape, 3), rows)
    clip_T, K = _check_tables(what, rows, taps, gain, FLICKER_MIX_MAX_TAPS)
    P = int(period)
    out = _out_f32(what, out, (P, 3), rows)
    check(load().flk_flicker_rows_mix_grad(ptr(g_clip), ptr(rows), rows.numel(), clip_T, ptr(taps), K, ptr(gain), P, ptr(out), stream_ptr()))
    return out


FLICKER_LINES_MAX_TAPS = 5    # rows of the perturbation one LINE of a rolling-shutter frame mixes (flk_flicker_lines_mix's K)


def flicker_lines_mix(delta, rows, taps, gain=None, out=None, rows_host=None):
    """the flicker as a ROLLING-SHUTTER camera records it (flk_flicker_lines_mix, one launch): line h of frame t of clip b takes
    ``gain[b] * sum_k taps[b,h,k] * delta[(rows[b,t] + k) mod P]`` -- ``delta`` fp32 [P,3], ``rows`` int32 [B,clip_T] on the device, ``taps``
    fp32 [B,H,K] (K <= 5; videoresnet_spec.capture_line_taps / CaptureChannel.line_tables), ``gain`` fp32 [B,3] or None -> fp32
    ``rows.shape + (H,3)``, the per-line perturbation ``make_apply_args(per_line=True)`` takes.  Raw values; every product and sum rounded
    on its own (videoresnet_spec.flicker_lines_mix restates it bit for bit)."""
    what = "flicker_lines_mix"
    P = _check_delta(what, delta, rows, rows_host)
    clip_T, H, K = _check_tables(what, rows, taps, gain, FLICKER_LINES_MAX_TAPS, per_line=True)
    out = _out_f32(what, out, (*rows.shape, H, 3), rows)
    check(load().flk_flicker_lines_mix(ptr(delta), P, ptr(rows), rows.numel(), clip_T, H, ptr(taps), K, ptr(gain), ptr(out), stream_ptr()))
    return out


def flicker_lines_mix_grad(g_lines, rows, period, taps, gain=None, out=None, rows_host=None, scratch=None):
    """the transpose of ``flicker_lines_mix`` (flk_flicker_lines_mix_grad, two launches): the per-line gradient fp32 ``rows.shape + (H,3)``
    (``perturb_grad_reduce`` of per-line arguments) folded onto the rows of the shared perturbation through the same tables -> fp32
    [period,3].  One fixed order (per frame and tap the lines ascending from +0; then frames ascending, taps ascending, from +0), no
    atomics.  ``scratch``: fp32 with at least ``rows.numel() * K * 3`` elements on the device (allocated when None)."""
    what = "flicker_lines_mix_grad"
    _check_rows(what, rows, period, rows_host)
    clip_T, H, K = _check_tables(what, rows, taps, gain, FLICKER_LINES_MAX_TAPS, per_line=True)
    _check_f32(what, "g_lines", g_lines, (*rows.shape, H, 3), rows)
    P = int(period)
    out = _out_f32(what, out, (P, 3), rows)
    need = rows.numel() * K * 3
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=rows.device)
    if not (torch.is_tensor(scratch) and scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.device == rows.device and scratch.numel() >= need):
        raise ValueError(f"{what}: scratch must be a contiguous fp32 tensor of at least {need} elements on {rows.device}")
    check(load().flk_flicker_lines_mix_grad(ptr(g_lines), ptr(rows), rows.numel(), clip_T, H, ptr(taps), K, ptr(gain), P, ptr(scratch), ptr(out),
                                            stream_ptr()))
    return out


class StemDeltaGradWeights(_HandleOwner):
    """fp32 weights of flk_stem_delta_grad: canonical stem weights [7,7,7,3,64] x folded batch-norm scale [64]"""
    _destroy = "flk_stem_delta_grad_weights_destroy"

    def __init__(self, w7_dhwio, bn_scale):
        w = np.ascontiguousarray(w7_dhwio, dtype=np.float32)
        sc = np.ascontiguousarray(bn_scale, dtype=np.float32)
        assert w.shape == (7, 7, 7, 3, 64) and sc.shape == (64,)
        h = C.c_void_p()
        check(load().flk_stem_delta_grad_weights_create(ptr(w), ptr(sc), C.byref(h)))
        self.handle = h


def stem_delta_grad_chunks(B, T, H, per_clip=False):
    """(nchunk, rows_per_chunk): how flk_stem_delta_grad cuts the H/2 output rows of each (clip, frame pair) of a [B,T,H,224,3] batch
    (flk_stem_delta_grad_chunks; host only, needs no GPU).  per_clip: the chunking of per-clip perturbations (the batch-1 call's)"""
    n, rows = C.c_int(), C.c_int()
    check(load().flk_stem_delta_grad_chunks(int(B), int(T), int(H), int(bool(per_clip)), C.byref(n), C.byref(rows)))
    return n.value, rows.value


def stem_delta_grad(args, G, weights, gdelta=None, scratch=None):
    """G: bf16 [B,T/2,H/2,W/2,ld] gradient of the stem's pre-ReLU output; returns d(loss)/d(delta) [T,3]"""
    assert G.dtype == torch.bfloat16 and G.is_contiguous() and G.dim() == 5
    if gdelta is None:
        gdelta = torch.empty((args.T, 3), dtype=torch.float32, device="cuda")
    if scratch is None:
        scratch = torch.empty(max(1, load().flk_stem_delta_grad_scratch_bytes(args.B, args.T, args.H) // 4), dtype=torch.float32, device="cuda")
    check(load().flk_stem_delta_grad(C.byref(args), ptr(G), G.shape[4], weights.handle, ptr(gdelta), ptr(scratch), 0, stream_ptr()))
    return gdelta


class StemFwdU8Weights(_HandleOwner):
    """MFMA fragments of flk_stem_fwd_u8 from the canonical stem weights [7,7,7,3,64] (37 K steps x 2 column parities)"""
    _destroy = "flk_conv_weights_destroy"

    def __init__(self, w7_dhwio):
        w = np.ascontiguousarray(w7_dhwio, dtype=np.float32)
        assert w.shape == (7, 7, 7, 3, 64)
        h = C.c_void_p()
        check(load().flk_stem_fwd_u8_weights_create(ptr(w), C.byref(h)))
        self.handle = h


def stem_delta_bias_table(args, w7_dhwio, bn_scale):
    """position-class bias table of the stem for the perturbation of `args` (flk_stem_delta_bias): fp32 [1 or B, T/2, 4, 4, 64]"""
    w = np.ascontiguousarray(w7_dhwio, dtype=np.float32)
    sc = np.ascontiguousarray(bn_scale, dtype=np.float32)
    h = C.c_void_p()
    check(load().flk_stem_delta_bias_weights_create(ptr(w), ptr(sc), C.byref(h)))
    try:
        tab = torch.zeros((args.B if args.delta_per_clip else 1, args.T // 2, 4, 4, 64), dtype=torch.float32, device="cuda")
        check(load().flk_stem_delta_bias(C.byref(args), h, ptr(tab), stream_ptr()))
        torch.cuda.synchronize()
    finally:
        load().flk_stem_delta_grad_weights_destroy(h)
    return tab


def stem_fwd_u8(args, weights, bn_scale, bn_bias, pos_bias=None, out=None):
    """Conv3d_1a_7x7 + batch norm + ReLU straight from the uint8 clip of `args` (center = 1): bf16 [B,T/2,112,112,64]"""
    assert bn_scale.dtype == torch.float32 and bn_bias.dtype == torch.float32 and bn_scale.is_cuda and bn_bias.is_cuda
    if out is None:
        out = torch.empty((args.B, args.T // 2, 112, 112, 64), dtype=torch.bfloat16, device="cuda")
    bstride = 0
    if pos_bias is not None:
        assert pos_bias.dtype == torch.float32 and pos_bias.is_contiguous() and pos_bias.shape[1:] == (args.T // 2, 4, 4, 64)
        bstride = pos_bias[0].numel() if pos_bias.shape[0] > 1 else 0
    check(load().flk_stem_fwd_u8(C.byref(args), weights.handle, ptr(bn_scale), ptr(bn_bias), ptr(pos_bias), bstride, ptr(out),
                                 out.shape[4], stream_ptr()))
    return out


def _flicker_opt_args(T, dialect, betas, dyn_max_norm, g_scale, lr, *, adam=(0.0, 0.0, 0.0), step=0, eps=0.0):
    """flk_adam_args of a flicker delta [T,3] (or [B,T,3]): the regulariser weights ``betas`` (beta0..beta3) and the step size; an Adam
    step names ``adam`` (b1, b2, eps) and, unbatched, its ``step``; a projected sign-gradient step names its radius ``eps``"""
    a = AdamArgs()
    a.T = T
    a.torch_dialect = int(dialect == "torch")
    a.beta0, a.beta1, a.beta2, a.beta3 = betas
    a.dyn_max_norm, a.g_scale, a.lr = dyn_max_norm, g_scale, lr
    a.adam_b1, a.adam_b2, a.adam_eps = adam
    a.step, a.pgd_eps = int(step), float(eps)
    return a


def perturb_reg_adam(g_adv, delta, m, v, step, *, dialect="tf", beta0=1.0, beta1=0.5, beta2=0.5, beta3=0.5,
                     dyn_max_norm=0.0, g_scale=1.0, lr=1e-3, adam=(0.9, 0.999, 1e-8), scalars=None):
    a = _flicker_opt_args(delta.shape[0], dialect, (beta0, beta1, beta2, beta3), dyn_max_norm, g_scale, lr, adam=adam, step=step)
    if scalars is None:
        scalars = torch.empty(8, dtype=torch.float32, device="cuda")
    check(load().flk_perturb_reg_adam(C.byref(a), ptr(g_adv), ptr(delta), ptr(m), ptr(v), ptr(scalars), stream_ptr()))
    return scalars


def perturb_reg_adam_batched(g_adv, delta, m, v, steps, active=None, *, dialect="tf", beta0=1.0, beta1=0.5, beta2=0.5, beta3=0.5,
                             dyn_max_norm=0.0, g_scale=1.0, lr=1e-3, adam=(0.9, 0.999, 1e-8), scalars=None, dyn_max_norm_dev=None):
    """B independent perturbations [B,T,3], each with its own Adam state and DEVICE step counter ``steps`` (int32 [B], advanced by the
    kernel); clips with ``active[b] == 0`` are frozen.  Returns scalars [B,8] of the pre-update perturbations."""
    B, T, _ = delta.shape
    assert steps.dtype == torch.int32 and steps.shape == (B,) and steps.is_cuda and (active is None or (active.dtype == torch.int32 and active.shape == (B,)))
    for t in (g_adv, delta, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == B * T * 3
    a = _flicker_opt_args(T, dialect, (beta0, beta1, beta2, beta3), dyn_max_norm, g_scale, lr, adam=adam)
    if scalars is None:
        scalars = torch.empty((B, 8), dtype=torch.float32, device="cuda")
    assert dyn_max_norm_dev is None or (dyn_max_norm_dev.dtype == torch.float32 and dyn_max_norm_dev.shape == (B,) and dyn_max_norm_dev.is_cuda)
    check(load().flk_perturb_reg_adam_batched(C.byref(a), B, ptr(g_adv), ptr(delta), ptr(m), ptr(v), ptr(steps), ptr(active),
                                              ptr(dyn_max_norm_dev), ptr(scalars), stream_ptr()))
    return scalars


def _dense_opt_args(delta, dialect, beta, g_scale, lr, dyn_max_norm, scalars, scratch, *, adam=(0.0, 0.0, 0.0), step=0, eps=0.0):
    """(flk_dense_adam_args of a dense delta [T,H,W,3], scalars, scratch), the two buffers allocated when None; an Adam step names
    ``adam`` (b1, b2, eps) and its ``step``, a projected sign-gradient step its radius ``eps``"""
    T, H, W, _ = delta.shape
    a = DenseAdamArgs()
    a.T, a.H, a.W, a.torch_dialect = T, H, W, int(dialect == "torch")
    a.beta, a.g_scale, a.lr = beta, g_scale, lr
    a.adam_b1, a.adam_b2, a.adam_eps = adam
    a.step = int(step)
    a.dyn_max_norm, a.pgd_eps = float(dyn_max_norm), float(eps)
    if scalars is None:
        scalars = torch.empty(4, dtype=torch.float32, device="cuda")
    if scratch is None:
        scratch = torch.empty(load().flk_dense_adam_scratch_bytes(T, H, W) // 4, dtype=torch.float32, device="cuda")
    return a, scalars, scratch


def perturb_dense_l12_adam(g_adv, delta, m, v, step, *, dialect="tf", beta=1.0, g_scale=1.0, lr=1e-3, adam=(0.9, 0.999, 1e-8),
                           scalars=None, scratch=None, dyn_max_norm=0.0):
    """dense delta [T,H,W,3]: L12 regulariser gradient + Adam (kinetics_i3d_L12); returns scalars {L12, thickness, roughness, max}.
    dyn_max_norm > 0 (torch dialect): L12 of the clamped perturbation, as Losses receives it (model.py:1078)"""
    a, scalars, scratch = _dense_opt_args(delta, dialect, beta, g_scale, lr, dyn_max_norm, scalars, scratch, adam=adam, step=step)
    check(load().flk_perturb_dense_l12_adam(C.byref(a), ptr(g_adv), ptr(delta), ptr(m), ptr(v), ptr(scalars), ptr(scratch), stream_ptr()))
    return scalars


def perturb_reg_pgd(g_adv, delta, *, dialect="tf", beta0=1.0, beta1=0.5, beta2=0.5, beta3=0.5, dyn_max_norm=0.0, g_scale=1.0, lr=1e-3,
                    eps=0.0, scalars=None):
    """projected sign-gradient step on the flicker delta [T,3]: delta <- clamp(delta - lr * sgn(g_tot), +-radius), g_tot formed as
    perturb_reg_adam forms it.  Radius: ``eps`` (TF dialect) or ``dyn_max_norm`` (torch dialect).  Returns the 8 scalars of the
    pre-update delta."""
    a = _flicker_opt_args(delta.shape[0], dialect, (beta0, beta1, beta2, beta3), dyn_max_norm, g_scale, lr, eps=eps)
    if scalars is None:
        scalars = torch.empty(8, dtype=torch.float32, device="cuda")
    check(load().flk_perturb_reg_pgd(C.byref(a), ptr(g_adv), ptr(delta), ptr(scalars), stream_ptr()))
    return scalars


def perturb_reg_pgd_batched(g_adv, delta, steps, active=None, *, dialect="tf", beta0=1.0, beta1=0.5, beta2=0.5, beta3=0.5, dyn_max_norm=0.0,
                            g_scale=1.0, lr=1e-3, eps=0.0, scalars=None, dyn_max_norm_dev=None):
    """B independent perturbations [B,T,3] under the projected sign-gradient step; ``steps`` (int32 [B]) is advanced for the clips with
    ``active[b] != 0``, the others are frozen.  Returns scalars [B,8] of the pre-update perturbations."""
    B, T, _ = delta.shape
    assert steps.dtype == torch.int32 and steps.shape == (B,) and steps.is_cuda and (active is None or (active.dtype == torch.int32 and active.shape == (B,)))
    for t in (g_adv, delta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == B * T * 3
    a = _flicker_opt_args(T, dialect, (beta0, beta1, beta2, beta3), dyn_max_norm, g_scale, lr, eps=eps)
    if scalars is None:
        scalars = torch.empty((B, 8), dtype=torch.float32, device="cuda")
    assert dyn_max_norm_dev is None or (dyn_max_norm_dev.dtype == torch.float32 and dyn_max_norm_dev.shape == (B,) and dyn_max_norm_dev.is_cuda)
    check(load().flk_perturb_reg_pgd_batched(C.byref(a), B, ptr(g_adv), ptr(delta), ptr(steps), ptr(active), ptr(dyn_max_norm_dev),
                                             ptr(scalars), stream_ptr()))
    return scalars


def perturb_dense_l12_pgd(g_adv, delta, *, dialect="tf", beta=1.0, g_scale=1.0, lr=1e-3, eps=0.0, scalars=None, scratch=None, dyn_max_norm=0.0):
    """dense delta [T,H,W,3]: L12 regulariser gradient + projected sign-gradient step; radius ``eps`` (TF dialect, required) or
    ``dyn_max_norm`` (torch dialect).  Returns scalars {L12, thickness, roughness, max} of the pre-update delta."""
    a, scalars, scratch = _dense_opt_args(delta, dialect, beta, g_scale, lr, dyn_max_norm, scalars, scratch, eps=eps)
    check(load().flk_perturb_dense_l12_pgd(C.byref(a), ptr(g_adv), ptr(delta), ptr(scalars), ptr(scratch), stream_ptr()))
    return scalars


def prepare_clips(frames, out=None, out_offset=0, im_scale=128, input_size=112, mean=DEFAULT_MEAN, std=DEFAULT_STD, rule="sizes", boxes=None,
                  flips=None, frame_idx=None, tone=None):
    """Raw decoded frames -> normalised clips on the device (flk_clip_prepare): the reference's evaluation transform
    ``ToTensorVideo -> ResizeVideo(im_scale) -> CenterCropVideo(input_size) -> NormalizeVideo(mean, std)`` (dataset.py:84-123) in one
    kernel launch per ``FLK_PREP_MAX_CLIPS`` clips.

    ``frames``: a CUDA uint8 tensor ``[N,T,H,W,3]`` or a list of ``[T,H,W,3]`` tensors whose ``H x W`` may differ (same ``T``).  Views
    are read in place when a pixel's three bytes and a row's pixels are adjacent (frames sliced out of a longer video are).
    ``out``: fp32 ``[>= out_offset + N, T, Ho, Wo, 3]`` contiguous; clip k goes to ``out[out_offset + k]``, other rows are left alone.
    Without ``out`` a tensor ``[N,T,Ho,Wo,3]`` is allocated.  Returns the rows written.
    ``rule``: ``"sizes"`` (default: the arithmetic of torch 1.4.0, which the reference pins) or ``"scale_factor"`` (current torch);
    see ``videoresnet_spec.prepare_geometry``.
    ``boxes`` and ``flips`` (both or neither; sequences of length N): the training transform instead (flk_clip_prepare_train; dataset.py:105-118) --
    clip k's box ``(i, j, h, w)`` of its resized image is resampled to ``input_size`` (RandomResizedCropVideo; RandomCropVideo when the
    box has that size) and mirrored along W when ``flips[k]``; ``videoresnet_spec.train_crop_params`` draws them as the reference does.
    ``frame_idx``: cut the clips from whole videos on the way (flk_clip_prepare_sampled; the temporal sampling of dataset.py:500-586).
    ``frames`` is then a list of videos ``[N_k,H_k,W_k,3]`` whose lengths and resolutions may differ -- the same tensor may be listed
    several times, once per clip cut from it -- and ``frame_idx`` holds one row of ``T_out`` frame numbers per clip (host integers: nested
    lists, an array or a CPU tensor ``[N, T_out]``; ``videoresnet_spec.sample_frame_indices`` draws them as the reference does).  Frame t of
    clip k is prepared from ``frames[k][frame_idx[k][t]]``: bitwise what the call without ``frame_idx`` gives on ``frames[k][frame_idx[k]]``,
    without that gathered copy.  Every index is checked against its video here, before anything is launched; the table is uploaded once
    per call as one int32 tensor.  ``out`` rows are ``[T_out,Ho,Wo,3]``; ``boxes`` / ``flips``, ``out`` / ``out_offset``, views and long
    lists work as without it.
    ``tone`` (with ``frame_idx``): prepare the clips of the DELIVERED videos (flk_clip_prepare_toned) -- a CUDA uint8 tensor
    ``[N,T_out,256,3]``, ``tone[k,t,v,c]`` the byte that source byte ``v`` of channel ``c`` is stored as in output frame ``t`` of clip ``k``
    (``flicker_tone_tables``): bitwise the call without ``tone`` on the videos after their 8-bit export, which are never written."""
    plan, out, n = prepare_clips_plan(frames, out, out_offset, im_scale, input_size, mean, std, rule, boxes, flips, frame_idx)
    if tone is not None:
        if frame_idx is None:
            raise ValueError("prepare_clips: tone needs frame_idx (the tables belong to the frames of whole videos)")
        T_out = plan[0]._frame_idx.shape[1]
        _check_tone("prepare_clips", "tone", tone, torch.uint8, (n, T_out, 256, 3), out.device)
        for j, a in enumerate(plan):
            check(load().flk_clip_prepare_toned(C.byref(a), a._boxes, ptr(a._frame_idx), T_out, ptr(tone[j * FLK_PREP_MAX_CLIPS:]), ptr(out),
                                                stream_ptr()))
        return out[out_offset:out_offset + n]
    for a in plan:
        if a._frame_idx is not None:
            check(load().flk_clip_prepare_sampled(C.byref(a), a._boxes, ptr(a._frame_idx), a._frame_idx.shape[1], ptr(out), stream_ptr()))
        elif a._boxes is None:
            check(load().flk_clip_prepare(C.byref(a), ptr(out), stream_ptr()))
        else:
            check(load().flk_clip_prepare_train(C.byref(a), a._boxes, ptr(out), stream_ptr()))
    return out[out_offset:out_offset + n]


def _check_tone(what, name, t, dtype, shape, device):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == device):
        desc = f"{tuple(t.shape)} {t.dtype} {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor {list(shape)} on {device}, got {desc}")


def prepare_clips_grad(frames, gx_s2d, slope, scale, im_scale=128, input_size=112, rule="sizes", boxes=None, flips=None, frame_idx=None, gdelta=None,
                       scratch=None):
    """d(loss)/d(delta_clip) through the resampling of a toned preparation (flk_clip_prepare_grad): fp32 ``[N,T_out,3]``.  ``frames``,
    ``im_scale`` / ``input_size`` / ``rule``, ``boxes`` / ``flips`` and ``frame_idx`` (required) exactly as the ``prepare_clips(tone=)`` call
    whose clips went into the network; ``gx_s2d``: the input gradient ``[N,T_out,Ho/2,Wo/2,16]`` (fp32 or bf16, the layout
    ``perturb_grad_reduce`` reads); ``slope`` fp32 ``[N,T_out,256,3]`` and ``scale`` fp32 ``[N,T_out,3]`` from ``flicker_tone_slopes``.
    ``gdelta``: the result's buffer; ``scratch``: fp32, ``flk_clip_prepare_grad_scratch_bytes`` / 4 elements per launch.  One fixed
    summation order: repeats are bitwise equal and a clip's rows are those of a call with that clip alone."""
    if frame_idx is None:
        raise ValueError("prepare_clips_grad: frame_idx is required (the clips are cut from whole videos)")
    if not torch.is_tensor(gx_s2d) or not gx_s2d.is_cuda:
        raise ValueError("prepare_clips_grad: gx_s2d must be a CUDA tensor")
    dev = gx_s2d.device
    Ho, Wo = (int(input_size), int(input_size)) if np.isscalar(input_size) else (int(input_size[0]), int(input_size[1]))
    if Ho % 2 or Wo % 2:
        raise ValueError(f"prepare_clips_grad: the output size must be even (the folded gradient layout), got {Ho} x {Wo}")
    plan, _, n = prepare_clips_plan(frames, None, 0, im_scale, (Ho, Wo), DEFAULT_MEAN, DEFAULT_STD, rule, boxes, flips, frame_idx, need_out=False)
    T_out = plan[0]._frame_idx.shape[1]
    if gx_s2d.dtype not in (torch.float32, torch.bfloat16) or tuple(gx_s2d.shape) != (n, T_out, Ho // 2, Wo // 2, 16) or not gx_s2d.is_contiguous():
        raise ValueError(f"prepare_clips_grad: gx_s2d must be a contiguous fp32 or bf16 tensor [{n},{T_out},{Ho // 2},{Wo // 2},16], got "
                         f"{tuple(gx_s2d.shape)} {gx_s2d.dtype}")
    _check_tone("prepare_clips_grad", "slope", slope, torch.float32, (n, T_out, 256, 3), dev)
    _check_tone("prepare_clips_grad", "scale", scale, torch.float32, (n, T_out, 3), dev)
    if gdelta is None:
        gdelta = torch.empty((n, T_out, 3), dtype=torch.float32, device=dev)
    _check_tone("prepare_clips_grad", "gdelta", gdelta, torch.float32, (n, T_out, 3), dev)
    need = int(load().flk_clip_prepare_grad_scratch_bytes(min(n, FLK_PREP_MAX_CLIPS), T_out, Ho)) // 4
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    if not (torch.is_tensor(scratch) and scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.device == dev and scratch.numel() >= need):
        raise ValueError(f"prepare_clips_grad: scratch must be a contiguous fp32 tensor of at least {need} elements on {dev}")
    for j, a in enumerate(plan):
        f = j * FLK_PREP_MAX_CLIPS
        check(load().flk_clip_prepare_grad(C.byref(a), a._boxes, ptr(a._frame_idx), T_out, ptr(slope[f:]), ptr(scale[f:]), ptr(gx_s2d[f:]),
                                           dtype_code(gx_s2d.dtype), ptr(gdelta[f:]), ptr(scratch), stream_ptr()))
    return gdelta


_prep_geometry = functools.lru_cache(maxsize=512)(prepare_geometry)


def prepare_clips_plan(frames, out=None, out_offset=0, im_scale=128, input_size=112, mean=DEFAULT_MEAN, std=DEFAULT_STD, rule="sizes", boxes=None,
                       flips=None, frame_idx=None, need_out=True):
    """the host half of ``prepare_clips``: ``([flk_prepare_args per launch], out, N)`` -- every check and every descriptor, no GPU call.
    (A caller that repeats one preparation, such as a timing loop, launches the arguments itself.)  With ``boxes`` / ``flips`` each
    launch's ``_boxes`` is its flk_prep_box array (None otherwise); with ``frame_idx`` its ``_frame_idx`` is its rows of the uploaded int32
    table (None otherwise) -- the upload is the one thing here that touches the device, after every check has passed.
    ``need_out=False`` (``prepare_clips_grad``, which writes no clips): no output buffer is made or checked, ``out`` comes back as given."""
    if (boxes is None) != (flips is None):
        raise ValueError("prepare_clips: boxes and flips go together, got only " + ("boxes" if flips is None else "flips"))
    Ho, Wo = (int(input_size), int(input_size)) if np.isscalar(input_size) else (int(input_size[0]), int(input_size[1]))
    clips = list(frames) if isinstance(frames, (list, tuple)) else [frames]        # a 5-d tensor is one group of equal clips
    if not clips or (torch.is_tensor(clips[0]) and clips[0].dim() == 5 and clips[0].shape[0] == 0):
        raise ValueError("prepare_clips: no clips")
    if boxes is not None:                      # one box and one flip per clip: checked before anything else looks at the clips
        boxes, flips = list(boxes), list(flips)
        n = sum(int(x.shape[0]) if torch.is_tensor(x) and x.dim() == 5 and not isinstance(frames, (list, tuple)) else 1 for x in clips)
        if len(boxes) != n or len(flips) != n:
            raise ValueError(f"prepare_clips: {n} clips, {len(boxes)} boxes and {len(flips)} flips")
    table = None
    if frame_idx is not None:
        if not isinstance(frames, (list, tuple)):
            raise ValueError("prepare_clips: with frame_idx, frames is a list of whole videos [N_k,H_k,W_k,3], one entry per clip")
        rows = frame_idx.numpy() if torch.is_tensor(frame_idx) and not frame_idx.is_cuda else frame_idx
        if torch.is_tensor(rows):
            raise ValueError("prepare_clips: frame_idx must be host integers (it is checked against the videos before anything is launched)")
        rows = [np.asarray(r) for r in rows]
        if len(rows) != len(clips):
            raise ValueError(f"prepare_clips: {len(clips)} clips and {len(rows)} rows of frame_idx")
        if any(r.ndim != 1 or r.shape != rows[0].shape for r in rows) or rows[0].size < 1:
            raise ValueError(f"prepare_clips: the rows of frame_idx must be equally long, at least one frame each; got lengths "
                             f"{[tuple(r.shape) for r in rows][:8]}")
        if any(r.dtype.kind not in "iu" for r in rows):
            raise ValueError(f"prepare_clips: frame_idx must hold integers, got {sorted({str(r.dtype) for r in rows})}")
        if rows[0].size > 65535:
            raise ValueError(f"prepare_clips: {rows[0].size} frames per clip, more than 65535")
        table = np.stack(rows).astype(np.int64)
    keep, descs, T = [], [], None
    for k, x in enumerate(clips):
        group = torch.is_tensor(x) and x.dim() == 5 and not isinstance(frames, (list, tuple))
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.uint8 or x.dim() != (5 if group else 4) or x.shape[-1] != 3:
            desc = f"{tuple(x.shape)} {x.dtype} {x.device}" if torch.is_tensor(x) else type(x).__name__
            raise ValueError(f"prepare_clips: {'frames' if group else f'clip {k}'} must be a CUDA uint8 tensor [{'N,' if group else ''}T,H,W,3], got {desc}")
        Tk, Hs, Ws = (int(v) for v in x.shape[-4:-1])
        if table is not None:                  # a whole video: its length bounds the clip's row of the table, the clip is T_out long
            if Tk < 1 or table[k].min() < 0 or table[k].max() >= Tk:
                raise ValueError(f"prepare_clips: clip {k}: frame_idx holds {int(table[k].min())} .. {int(table[k].max())}, the video has {Tk} frames")
            T = table.shape[1]
        else:
            T = Tk if T is None else T
            if Tk != T:
                raise ValueError(f"prepare_clips: clip {k} has {Tk} frames, clip 0 has {T}")
        # read in place when a pixel's bytes and a row's pixels are adjacent; anything else is copied once
        if x.stride(-1) != 1 or x.stride(-2) != 3 or x.stride(-3) < 3 * Ws or (Tk > 1 and x.stride(-4) <= 0) or (group and x.stride(0) < 0):
            x = x.contiguous()
        keep.append(x)
        Hr, Wr, sh, sw, ci, cj = _prep_geometry(Hs, Ws, im_scale, (Ho, Wo), rule)
        base, nstride = x.data_ptr(), (x.stride(0) if group else 0)
        for j in range(x.shape[0] if group else 1):
            d = PrepClip()
            d.src, d.T, d.Hs, d.Ws = base + j * nstride, Tk, Hs, Ws
            d.pitch_t, d.pitch_h = max(int(x.stride(-4)), 1), int(x.stride(-3))
            d.Hr, d.Wr, d.step_h, d.step_w, d.crop_i, d.crop_j = Hr, Wr, sh, sw, ci, cj
            descs.append(d)
    n = len(descs)
    if boxes is not None:
        for k, (b, d) in enumerate(zip(boxes, descs)):
            if len(b) != 4 or min(b[2], b[3]) < 1 or min(b[0], b[1]) < 0 or b[0] + b[2] > d.Hr or b[1] + b[3] > d.Wr:
                raise ValueError(f"prepare_clips: clip {k}: box {tuple(b)} is not (i, j, h, w) inside the resized image {d.Hr} x {d.Wr}")
    if out is None and need_out:
        out = torch.empty((out_offset + n, T, Ho, Wo, 3), dtype=torch.float32, device=keep[0].device)
    if need_out and (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 5
            or tuple(out.shape[1:]) != (T, Ho, Wo, 3) or out_offset < 0 or out.shape[0] < out_offset + n):
        desc = f"{tuple(out.shape)} {out.dtype}" if torch.is_tensor(out) else type(out).__name__
        raise ValueError(f"prepare_clips: out must be a contiguous CUDA float32 tensor [>= {out_offset + n},{T},{Ho},{Wo},3], got {desc}")
    if table is not None:                      # one upload per call; each launch takes its rows
        table = torch.from_numpy(table.astype(np.int32)).to(keep[0].device)
    plan = []
    for first in range(0, n, FLK_PREP_MAX_CLIPS):
        part = descs[first:first + FLK_PREP_MAX_CLIPS]
        arr = (PrepClip * len(part))(*part)
        a = PrepareArgs()
        a.nclip, a.Ho, a.Wo = len(part), Ho, Wo
        a.mean, a.std = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        a.out_clip_offset, a.out_clip_stride = out_offset + first, T * Ho * Wo * 3
        a.clips = arr
        a._keepalive = (arr, keep, table)   # the struct holds raw pointers only
        a._boxes = None
        a._frame_idx = None if table is None else table[first:first + len(part)]
        if boxes is not None:
            a._boxes = (PrepBox * len(part))(*[PrepBox(int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(bool(f)))
                                               for b, f in zip(boxes[first:first + len(part)], flips[first:first + len(part)])])
        plan.append(a)
    return plan, out, n


def codec_tables(quality):
    """flk_codec_tables: the luma and chroma quantisation tables at ``quality`` as the library makes them, int32 ``[64]`` each (host)"""
    ql, qc = (C.c_int32 * 64)(), (C.c_int32 * 64)()
    check(load().flk_codec_tables(int(quality), ql, qc))
    return np.asarray(ql[:], np.int32), np.asarray(qc[:], np.int32)


def codec_inter_step(quality):
    """flk_codec_inter_step: the P-frames' quantiser step at ``quality`` as the library makes it (host)"""
    qp = C.c_int32()
    check(load().flk_codec_inter_step(int(quality), C.byref(qp)))
    return int(qp.value)


_codec_mc_scratch = {}      # device -> the reused uint8 workspace of flk_codec_roundtrip_mc_u8 (grown, never shrunk)


def codec_roundtrip(videos, codec, frame_idx=None, tone=None, out=None, stats=False, spans=None, motion=False):
    """The delivered videos after lossy intra-frame compression (flk_codec_roundtrip_u8; ``videoresnet_spec.codec_roundtrip_host`` is
    its definition, bit for bit): one kernel launch per ``FLK_PREP_MAX_CLIPS`` videos.

    ``videos``: a list of CUDA uint8 ``[N_k,H_k,W_k,3]`` whose lengths and resolutions may differ; views are read in place when a
    pixel's bytes and a row's pixels are adjacent.  ``codec``: a ``videoresnet_spec.Codec``.  Returns the list of compressed videos,
    uint8 ``[N_k,H_k,W_k,3]``; with ``stats`` also a list of int32 ``[N_k,2]`` (per frame: non-zero quantised coefficients, the sum
    of their magnitudes).
    ``frame_idx``: host integers ``[len(videos), T_out]`` (as ``prepare_clips`` takes them, checked against the videos here): only
    the listed frames are compressed, output ``k`` is ``[T_out,H_k,W_k,3]`` -- bitwise the call on ``videos[k][frame_idx[k]]``.
    ``tone``: CUDA uint8 ``[len(videos), T, 256, 3]`` (``flicker_tone_tables``), T the common output length: every frame goes through
    its byte -> byte table first -- bitwise the call on the exported videos, which are never written.
    ``out``: a list of uint8 tensors to fill, which may be views with row and frame pitches of their own; bytes outside them are
    not touched.  Everything is refused before any device call.
    A codec with ``gop`` > 1 (flk_codec_roundtrip_gop_u8: closed GOPs of zero-motion P-frames, whose frames depend on their
    predecessors) takes no ``frame_idx`` but ``spans``: host integers ``[len(videos), 2]`` of (first, count), first a multiple of
    ``gop``; the default is the whole video, ``(0, N_k)``.  Output ``k`` is ``[count_k,H_k,W_k,3]``, video frames first .. first +
    count - 1 -- bitwise those frames of the whole video's result; ``stats`` are ``[count_k,2]``; ``tone`` is
    ``[len(videos), max count (or more), 256, 3]``, row t the table of video frame first_k + t (rows past a video's count are not read).
    A codec with ``search`` > 0 (flk_codec_roundtrip_mc_u8: motion-compensated P-frames) takes the same arguments
    and is launched once per frame position of the GOP, its reconstructed planes travelling through a workspace kept per device and
    reused from call to call.  ``motion`` (a codec with ``gop`` > 1 only): also return, last, the list of the vectors, int8
    ``[count_k, MBy_k, MBx_k, 2]`` as (dy, dx) per 16 x 16 macroblock of the padded luma plane -- zeros on intra frames and at ``search`` 0,
    which then goes through the same entry."""
    from .videoresnet_spec import Codec
    what = "codec_roundtrip"
    if not isinstance(codec, Codec):
        raise ValueError(f"{what}: codec must be a videoresnet_spec.Codec, got {type(codec).__name__}")
    if not isinstance(videos, (list, tuple)) or not videos:
        raise ValueError(f"{what}: videos must be a non-empty list of CUDA uint8 tensors [N,H,W,3]")
    vids = list(videos)
    for k, v in enumerate(vids):
        if not torch.is_tensor(v) or not v.is_cuda or v.dtype != torch.uint8 or v.dim() != 4 or v.shape[-1] != 3 or min(v.shape) < 1:
            desc = f"{tuple(v.shape)} {v.dtype} {v.device}" if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"{what}: video {k} must be a CUDA uint8 tensor [N,H,W,3], got {desc}")
    n, dev = len(vids), vids[0].device
    table = None
    gop = codec.gop
    if motion and gop == 1:
        raise ValueError(f"{what}: motion vectors go with a codec of gop > 1 (an intra-frame codec has no P-frames)")
    if gop > 1 and frame_idx is not None:
        raise ValueError(f"{what}: a codec with gop {gop} predicts every frame from the one before it: give spans=(first, count) per video, not "
                         f"frame_idx")
    if spans is not None:
        if gop == 1:
            raise ValueError(f"{what}: spans go with a codec of gop > 1 (an intra-frame codec takes frame_idx)")
        sp = spans.numpy() if torch.is_tensor(spans) and not spans.is_cuda else spans
        if torch.is_tensor(sp):
            raise ValueError(f"{what}: spans must be host integers (they are checked against the videos before anything is launched)")
        sp = np.asarray(sp)
        if sp.shape != (n, 2) or sp.dtype.kind not in "iu":
            raise ValueError(f"{what}: spans must be integers [{n}, 2] of (first, count), got {sp.shape} {sp.dtype}")
        sp = sp.astype(np.int64)
        for k, v in enumerate(vids):
            f, cnt = int(sp[k, 0]), int(sp[k, 1])
            if f < 0 or f % gop or cnt < 1 or f + cnt > v.shape[0]:
                raise ValueError(f"{what}: video {k}: span (first {f}, count {cnt}) must start on a multiple of gop {gop} and lie inside its "
                                 f"{v.shape[0]} frames")
    elif gop > 1:
        sp = np.asarray([(0, int(v.shape[0])) for v in vids], np.int64)
    if frame_idx is not None:
        rows = frame_idx.numpy() if torch.is_tensor(frame_idx) and not frame_idx.is_cuda else frame_idx
        if torch.is_tensor(rows):
            raise ValueError(f"{what}: frame_idx must be host integers (it is checked against the videos before anything is launched)")
        rows = [np.asarray(r) for r in rows]
        if len(rows) != n or any(r.ndim != 1 or r.shape != rows[0].shape or r.dtype.kind not in "iu" for r in rows) or not 1 <= rows[0].size <= 65535:
            raise ValueError(f"{what}: frame_idx must hold {n} equally long rows of 1..65535 integers")
        table = np.stack(rows).astype(np.int64)
        for k, v in enumerate(vids):
            if table[k].min() < 0 or table[k].max() >= v.shape[0]:
                raise ValueError(f"{what}: video {k}: frame_idx holds {int(table[k].min())} .. {int(table[k].max())}, the video has {v.shape[0]} frames")
    lens = [int(sp[k, 1]) if gop > 1 else int(v.shape[0]) if table is None else table.shape[1] for k, v in enumerate(vids)]
    if max(lens) > 65535:
        raise ValueError(f"{what}: {max(lens)} frames in one video, more than 65535 (cut it, or give {'spans' if gop > 1 else 'frame_idx'})")
    if tone is not None and gop > 1:               # rows past the longest span (a caller's buffer made in whole pieces) are allowed, and not read
        more = torch.is_tensor(tone) and tone.dim() == 4 and max(lens) < tone.shape[1] <= 65535
        _check_tone(what, "tone", tone, torch.uint8, (n, tone.shape[1] if more else max(lens), 256, 3), dev)
    elif tone is not None:
        if len(set(lens)) != 1:
            raise ValueError(f"{what}: tone needs one output length for every video (give frame_idx), got lengths {sorted(set(lens))}")
        _check_tone(what, "tone", tone, torch.uint8, (n, lens[0], 256, 3), dev)
    if out is None:
        outs = [torch.empty((lens[k], v.shape[1], v.shape[2], 3), dtype=torch.uint8, device=dev) for k, v in enumerate(vids)]
    else:
        outs = list(out) if isinstance(out, (list, tuple)) else None
        if outs is None or len(outs) != n:
            raise ValueError(f"{what}: out must be a list of {n} uint8 tensors")
    keep = []
    for k, (v, o) in enumerate(zip(vids, outs)):
        shape = (lens[k], int(v.shape[1]), int(v.shape[2]), 3)
        if (not torch.is_tensor(o) or not o.is_cuda or o.dtype != torch.uint8 or tuple(o.shape) != shape or o.device != dev or o.stride(-1) != 1
                or o.stride(-2) != 3 or o.stride(-3) < 3 * shape[2] or (shape[0] > 1 and o.stride(0) < o.stride(-3) * shape[1])):
            desc = f"{tuple(o.shape)} {o.dtype} strides {o.stride()}" if torch.is_tensor(o) else type(o).__name__
            raise ValueError(f"{what}: out[{k}] must be a CUDA uint8 tensor {list(shape)} with adjacent pixel bytes and pixels, rows and frames not "
                             f"overlapping, got {desc}")
        if v.stride(-1) != 1 or v.stride(-2) != 3 or v.stride(-3) < 3 * shape[2] or (v.shape[0] > 1 and v.stride(0) <= 0):
            v = v.contiguous()
        keep.append(v)
        lo_s, hi_s = v.data_ptr(), v.data_ptr() + (v.shape[0] - 1) * max(v.stride(0), 0) + (shape[1] - 1) * v.stride(1) + 3 * shape[2]
        lo_d, hi_d = o.data_ptr(), o.data_ptr() + (shape[0] - 1) * max(o.stride(0), 0) + (shape[1] - 1) * o.stride(1) + 3 * shape[2]
        if lo_s < hi_d and lo_d < hi_s:
            raise ValueError(f"{what}: out[{k}] overlaps its source (an MCU reads pixels that other workgroups write)")
    st_out, mv_out = [None] * n, [None] * n
    sub = _lib.FLK_CODEC_420 if codec.subsampling == "420" else _lib.FLK_CODEC_444

    def clip_array(part):
        arr = (_lib.CodecClip * len(part))()
        for d, k in zip(arr, part):
            v, o = keep[k], outs[k]
            d.src, d.T, d.Hs, d.Ws = v.data_ptr(), int(v.shape[0]), int(v.shape[1]), int(v.shape[2])
            d.pitch_t, d.pitch_h = max(int(v.stride(0)), 1), int(v.stride(1))
            d.dst, d.dst_pitch_t, d.dst_pitch_h = o.data_ptr(), max(int(o.stride(0)), 1), int(o.stride(1))
        a = _lib.CodecArgs()
        a.nclip, a.quality, a.subsampling, a.clips = len(part), codec.quality, sub, arr
        return a, arr

    if gop > 1:                                 # one launch per FLK_PREP_MAX_CLIPS consecutive videos; every launch has the rows of max count
        T_max = max(lens) if tone is None else int(tone.shape[1])
        for first in range(0, n, FLK_PREP_MAX_CLIPS):
            part = list(range(first, min(first + FLK_PREP_MAX_CLIPS, n)))
            a, arr = clip_array(part)
            firsts, counts = ((C.c_int32 * len(part))(*[int(sp[k, j]) for k in part]) for j in (0, 1))
            st = torch.empty((len(part), T_max, 2), dtype=torch.int32, device=dev) if stats else None
            tn = None if tone is None else ptr(tone[first:])
            if codec.search > 0 or motion:
                m = 8 if codec.subsampling == "444" else 16
                mbs = [(-(-int(vids[k].shape[1]) // m) * m + 15) // 16 for k in part], [(-(-int(vids[k].shape[2]) // m) * m + 15) // 16 for k in part]
                stride = max(y * x for y, x in zip(*mbs))
                mv = torch.empty((len(part), T_max, stride, 2), dtype=torch.int8, device=dev) if motion else None
                need = int(load().flk_codec_mc_scratch_bytes(C.byref(a), gop, counts))
                if need <= 0:
                    raise ValueError(f"{what}: the workspace of these videos cannot be sized")
                ws = _codec_mc_scratch.get(dev)
                if ws is None or ws.numel() < need:        # the stream orders a later call's launches after this one's: reuse is safe
                    ws = _codec_mc_scratch[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
                check(load().flk_codec_roundtrip_mc_u8(C.byref(a), gop, codec.search, firsts, counts, T_max, tn, ptr(st), ptr(mv), stride, ptr(ws),
                                                       ws.numel(), stream_ptr()))
                if motion:
                    for j, k in enumerate(part):
                        mv_out[k] = mv[j, :lens[k], :mbs[0][j] * mbs[1][j]].reshape(lens[k], mbs[0][j], mbs[1][j], 2)
            else:
                check(load().flk_codec_roundtrip_gop_u8(C.byref(a), gop, firsts, counts, T_max, tn, ptr(st), stream_ptr()))
            if stats:
                for j, k in enumerate(part):
                    st_out[k] = st[j, :lens[k]]
        res = (outs,) + ((st_out,) if stats else ()) + ((mv_out,) if motion else ())
        return res if len(res) > 1 else outs
    tab_dev = None if table is None else torch.from_numpy(table.astype(np.int32)).to(dev)
    groups = {}
    for k in range(n):                          # one launch has one output length: videos of equal length share launches
        groups.setdefault(lens[k], []).append(k)
    if table is not None or tone is not None:
        assert len(groups) == 1
    for T_out, members in groups.items():
        for first in range(0, len(members), FLK_PREP_MAX_CLIPS):
            part = members[first:first + FLK_PREP_MAX_CLIPS]
            a, arr = clip_array(part)
            st = torch.empty((len(part), T_out, 2), dtype=torch.int32, device=dev) if stats else None
            # with a table or a tone the launch's members are consecutive videos: its rows of the tables start at part[0]
            check(load().flk_codec_roundtrip_u8(C.byref(a), None if tab_dev is None else ptr(tab_dev[part[0]:]), T_out,
                                                None if tone is None else ptr(tone[part[0]:]), ptr(st), stream_ptr()))
            if stats:
                for j, k in enumerate(part):
                    st_out[k] = st[j]
    return (outs, st_out) if stats else outs


def _packed_images(what, name, t, shapes, dev):
    """the packed fp32 gradient images of a call as ONE flat tensor and its per-clip views: ``t`` is that flat tensor, or the list of
    ``[T_out,H_k,W_k,3]`` tensors -- taken in place when they lie one after the other in memory (views of one buffer), copied into
    one buffer otherwise"""
    sizes = [int(np.prod(s)) for s in shapes]
    ends = np.cumsum(sizes)
    if isinstance(t, (list, tuple)):
        if len(t) != len(shapes) or any(not torch.is_tensor(v) or v.dtype != torch.float32 or tuple(v.shape) != tuple(s) or v.device != dev
                                        for v, s in zip(t, shapes)):
            raise ValueError(f"{what}: {name} must be a list of fp32 tensors {[list(s) for s in shapes][:4]}.. on {dev}")
        packed = all(v.is_contiguous() and v.data_ptr() == t[0].data_ptr() + 4 * (e - n) for v, n, e in zip(t, sizes, ends))
        if packed:                              # one flat tensor over the same memory
            t = torch.as_strided(t[0], (int(ends[-1]),), (1,))
        else:
            t = torch.cat([v.reshape(-1) for v in t])
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous() and t.device == dev and t.numel() >= ends[-1]):
        raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor of {int(ends[-1])} elements on {dev} (the clips' images packed one "
                         f"after the other), or the list of them")
    return t, [t[e - n:e].view(*s) for s, n, e in zip(shapes, sizes, ends)]


def prepare_clips_grad_image(frames, gx_s2d, im_scale=128, input_size=112, rule="sizes", boxes=None, flips=None, frame_idx=None, out=None):
    """The transpose of the resampling on images (flk_clip_prepare_grad_image): the gradient with respect to every SOURCE pixel of the
    frames the clips were prepared from -- a list of fp32 ``[T_out,H_k,W_k,3]``.  ``frames`` (a list of videos ``[N_k,H_k,W_k,3]``, of
    which the resolutions are read), ``im_scale`` / ``input_size`` / ``rule``, ``boxes`` / ``flips`` and ``frame_idx`` (required: it
    gives T_out; output frame t has its own image whatever source frame it names) as the ``prepare_clips`` call whose clips went into
    the network; ``gx_s2d`` as ``prepare_clips_grad`` takes it.  ``out``: the list of images to write, which may be views with row and
    frame pitches (in whole floats) of their own.  The composite matrices come from ``videoresnet_spec.prepare_adjoint_tables``, one
    upload per call.  One fixed summation order: repeats are bitwise equal and a clip's images are those of a call with it alone."""
    from .videoresnet_spec import prepare_adjoint_tables
    what = "prepare_clips_grad_image"
    if frame_idx is None:
        raise ValueError(f"{what}: frame_idx is required (the clips are cut from whole videos)")
    if not torch.is_tensor(gx_s2d) or not gx_s2d.is_cuda:
        raise ValueError(f"{what}: gx_s2d must be a CUDA tensor")
    if not isinstance(frames, (list, tuple)) or not frames or any(not torch.is_tensor(v) or v.dim() != 4 or v.shape[-1] != 3 for v in frames):
        raise ValueError(f"{what}: frames must be a non-empty list of videos [N,H,W,3]")
    dev, n = gx_s2d.device, len(frames)
    Ho, Wo = (int(input_size), int(input_size)) if np.isscalar(input_size) else (int(input_size[0]), int(input_size[1]))
    if Ho % 2 or Wo % 2:
        raise ValueError(f"{what}: the output size must be even (the folded gradient layout), got {Ho} x {Wo}")
    rows = np.asarray(frame_idx.numpy() if torch.is_tensor(frame_idx) else frame_idx)
    if rows.ndim != 2 or rows.shape[0] != n or not 1 <= rows.shape[1] <= 65535:
        raise ValueError(f"{what}: frame_idx must hold {n} equally long rows of 1..65535 integers, got {rows.shape}")
    T_out = rows.shape[1]
    if gx_s2d.dtype not in (torch.float32, torch.bfloat16) or tuple(gx_s2d.shape) != (n, T_out, Ho // 2, Wo // 2, 16) or not gx_s2d.is_contiguous():
        raise ValueError(f"{what}: gx_s2d must be a contiguous fp32 or bf16 tensor [{n},{T_out},{Ho // 2},{Wo // 2},16], got "
                         f"{tuple(gx_s2d.shape)} {gx_s2d.dtype}")
    sizes = [(int(v.shape[1]), int(v.shape[2])) for v in frames]
    if out is None:
        out = [torch.empty((T_out, h, w, 3), dtype=torch.float32, device=dev) for h, w in sizes]
    out = list(out)
    for k, (o, (h, w)) in enumerate(zip(out, sizes)):
        if (len(out) != n or not torch.is_tensor(o) or o.dtype != torch.float32 or tuple(o.shape) != (T_out, h, w, 3) or o.device != dev or o.stride(3) != 1
                or o.stride(2) != 3 or o.stride(1) < 3 * w or (T_out > 1 and o.stride(0) < o.stride(1) * (h - 1) + 3 * w)):
            raise ValueError(f"{what}: out[{k}] must be an fp32 tensor {[T_out, h, w, 3]} on {dev} with adjacent channels and pixels, rows and "
                             f"frames not overlapping")
    for first in range(0, n, FLK_PREP_MAX_CLIPS):
        part = range(first, min(first + FLK_PREP_MAX_CLIPS, n))
        words, offsets, K = prepare_adjoint_tables([sizes[k] for k in part], None if boxes is None else [boxes[k] for k in part],
                                                   None if flips is None else [flips[k] for k in part], im_scale, (Ho, Wo), rule)
        tab = torch.from_numpy(words).to(dev)
        arr = (_lib.GradImageClip * len(part))()
        for d, k, (th, tw) in zip(arr, part, offsets):
            o = out[k]
            d.dst, d.pitch_t, d.pitch_h = o.data_ptr(), max(int(o.stride(0)), 1), int(o.stride(1))
            d.Hs, d.Ws, d.tab_h, d.tab_w = sizes[k][0], sizes[k][1], th, tw
        check(load().flk_clip_prepare_grad_image(len(part), arr, T_out, Ho, Wo, K, ptr(tab), tab.numel(), ptr(gx_s2d[first:]),
                                                 dtype_code(gx_s2d.dtype), stream_ptr()))
    return out


CODEC_GRAD_MODES = {"ste": _lib.FLK_CODEC_GRAD_STE, "cubic": _lib.FLK_CODEC_GRAD_CUBIC}


def codec_grad(videos, codec, g_out, slope, scale, mode, frame_idx=None, tone=None, gdelta=None, g_in=None, scratch=None):
    """The backward of the intra codec (flk_codec_grad; ``videoresnet_spec.codec_grad_host`` is its definition): fp32 ``[n,T_out,3]``,
    d(loss)/d(delta_clip) through the surrogate of ``codec_roundtrip(videos, codec, frame_idx=, tone=)``.  ``videos``, ``codec`` (gop 1),
    ``frame_idx`` and ``tone`` as that call took them; ``g_out``: d(loss)/d(decoded frames), the list of fp32 ``[T_out,H_k,W_k,3]``
    (``prepare_clips_grad_image`` writes it) or one flat fp32 tensor holding them one after the other; ``slope`` / ``scale`` from
    ``flicker_tone_slopes``; ``mode``: "ste" or "cubic".  ``g_in``: True, or a flat fp32 buffer: also return, second, the list of
    gradients with respect to the codec's input frames.  ``scratch``: fp32, flk_codec_grad_scratch_bytes / 4 elements per launch.
    One launch pair per ``FLK_PREP_MAX_CLIPS`` videos; one fixed summation order."""
    from .videoresnet_spec import Codec
    what = "codec_grad"
    if not isinstance(codec, Codec) or codec.gop != 1:
        raise ValueError(f"{what}: codec must be an intra-frame videoresnet_spec.Codec (gop 1), got {codec!r}")
    if mode not in CODEC_GRAD_MODES:
        raise ValueError(f"{what}: mode must be one of {tuple(CODEC_GRAD_MODES)}, got {mode!r}")
    if not isinstance(videos, (list, tuple)) or not videos:
        raise ValueError(f"{what}: videos must be a non-empty list of CUDA uint8 tensors [N,H,W,3]")
    vids = []
    for k, v in enumerate(videos):
        if not torch.is_tensor(v) or not v.is_cuda or v.dtype != torch.uint8 or v.dim() != 4 or v.shape[-1] != 3 or min(v.shape) < 1:
            desc = f"{tuple(v.shape)} {v.dtype} {v.device}" if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"{what}: video {k} must be a CUDA uint8 tensor [N,H,W,3], got {desc}")
        if v.stride(-1) != 1 or v.stride(-2) != 3 or v.stride(-3) < 3 * v.shape[2] or (v.shape[0] > 1 and v.stride(0) <= 0):
            v = v.contiguous()
        vids.append(v)
    n, dev = len(vids), vids[0].device
    table = None
    if frame_idx is not None:
        table = np.asarray(frame_idx.numpy() if torch.is_tensor(frame_idx) else frame_idx)
        if table.ndim != 2 or table.shape[0] != n or table.dtype.kind not in "iu" or not 1 <= table.shape[1] <= 65535:
            raise ValueError(f"{what}: frame_idx must hold {n} equally long rows of 1..65535 integers")
        for k, v in enumerate(vids):
            if table[k].min() < 0 or table[k].max() >= v.shape[0]:
                raise ValueError(f"{what}: video {k}: frame_idx holds {int(table[k].min())} .. {int(table[k].max())}, the video has {v.shape[0]} frames")
        T_out = table.shape[1]
    else:
        if len({int(v.shape[0]) for v in vids}) != 1 or vids[0].shape[0] > 65535:
            raise ValueError(f"{what}: without frame_idx the videos have one length, at most 65535 frames")
        T_out = int(vids[0].shape[0])
    if tone is not None:
        _check_tone(what, "tone", tone, torch.uint8, (n, T_out, 256, 3), dev)
    _check_tone(what, "slope", slope, torch.float32, (n, T_out, 256, 3), dev)
    _check_tone(what, "scale", scale, torch.float32, (n, T_out, 3), dev)
    if gdelta is None:
        gdelta = torch.empty((n, T_out, 3), dtype=torch.float32, device=dev)
    _check_tone(what, "gdelta", gdelta, torch.float32, (n, T_out, 3), dev)
    shapes = [(T_out, int(v.shape[1]), int(v.shape[2]), 3) for v in vids]
    flat, _ = _packed_images(what, "g_out", g_out, shapes, dev)
    gin_flat = gin_views = None
    if g_in is not None and g_in is not False:
        if g_in is True:
            g_in = torch.empty(sum(int(np.prod(s)) for s in shapes), dtype=torch.float32, device=dev)
        if not torch.is_tensor(g_in):
            raise ValueError(f"{what}: g_in must be True or one flat fp32 buffer")
        gin_flat, gin_views = _packed_images(what, "g_in", g_in, shapes, dev)
    tab_dev = None if table is None else torch.from_numpy(table.astype(np.int32)).to(dev)
    sub = _lib.FLK_CODEC_420 if codec.subsampling == "420" else _lib.FLK_CODEC_444
    off = 0
    for first in range(0, n, FLK_PREP_MAX_CLIPS):
        part = range(first, min(first + FLK_PREP_MAX_CLIPS, n))
        arr = (_lib.CodecClip * len(part))()
        for d, k in zip(arr, part):
            v = vids[k]
            d.src, d.T, d.Hs, d.Ws = v.data_ptr(), int(v.shape[0]), int(v.shape[1]), int(v.shape[2])
            d.pitch_t, d.pitch_h = max(int(v.stride(0)), 1), int(v.stride(1))
        a = _lib.CodecArgs()
        a.nclip, a.quality, a.subsampling, a.clips = len(part), codec.quality, sub, arr
        need = int(load().flk_codec_grad_scratch_bytes(C.byref(a), T_out)) // 4
        if need <= 0:
            raise ValueError(f"{what}: the scratch of these videos cannot be sized")
        ws = torch.empty(need, dtype=torch.float32, device=dev) if scratch is None else scratch
        if not (torch.is_tensor(ws) and ws.dtype == torch.float32 and ws.is_contiguous() and ws.device == dev and ws.numel() >= need):
            raise ValueError(f"{what}: scratch must be a contiguous fp32 tensor of at least {need} elements on {dev}")
        check(load().flk_codec_grad(C.byref(a), None if tab_dev is None else ptr(tab_dev[first:]), T_out, None if tone is None else ptr(tone[first:]),
                                    CODEC_GRAD_MODES[mode], C.c_void_p(flat.data_ptr() + 4 * off), ptr(slope[first:]), ptr(scale[first:]), ptr(gdelta[first:]),
                                    None if gin_flat is None else C.c_void_p(gin_flat.data_ptr() + 4 * off), ptr(ws), stream_ptr()))
        off += sum(int(np.prod(shapes[k])) for k in part)
    return gdelta if gin_views is None else (gdelta, gin_views)


def _head_check(y, wt, W, C_, coff):
    assert y.dim() == 4 and y.is_contiguous() and y.is_cuda and y.dtype in (torch.float32, torch.bfloat16)
    B, Tn, HW, ld = y.shape
    C_ = ld - coff if C_ is None else C_
    assert 0 <= coff and coff + C_ <= ld
    assert wt.dtype == torch.float32 and wt.is_contiguous() and wt.is_cuda and tuple(wt.shape) == (Tn,)
    assert W.dtype == torch.float32 and W.is_contiguous() and W.is_cuda and W.dim() == 2 and W.shape[0] == C_
    return B, Tn, HW, ld, C_, W.shape[1]


def head_forward(y, wt, W, bias, *, C=None, coff=0):
    """the classifier head (flk_head_forward) on channels [coff, coff + C) of y [B,Tn,HW,ld] (fp32 / bf16): frame weights wt [Tn], fc weight
    W [C,N], bias [N] or None -> (feat [B,C], logits [B,N]), fp32"""
    B, Tn, HW, ld, C_, N = _head_check(y, wt, W, C, coff)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.is_cuda and tuple(bias.shape) == (N,))
    feat = torch.empty((B, C_), dtype=torch.float32, device=y.device)
    logits = torch.empty((B, N), dtype=torch.float32, device=y.device)
    check(load().flk_head_forward(ptr(y), ld, coff, C_, B, Tn, HW, ptr(wt), ptr(W), ptr(bias), N, ptr(feat), ptr(logits), dtype_code(y.dtype),
                                  stream_ptr()))
    return feat, logits


def head_backward(y, wt, W, dlogits, *, gy=None, C=None, coff=0, gcoff=0, use_mask=True):
    """the head's gradient (flk_head_backward): dlogits [B,N] -> (gy, dfeat [B,C]); channels [gcoff, gcoff + C) of gy [B,Tn,HW,gld] (default: a
    fresh [.., gcoff + C] tensor of y's dtype) receive wt[t] * dfeat, zero where use_mask and not y > 0; its other channels are left alone"""
    B, Tn, HW, ld, C_, N = _head_check(y, wt, W, C, coff)
    assert dlogits.dtype == torch.float32 and dlogits.is_contiguous() and dlogits.is_cuda and tuple(dlogits.shape) == (B, N)
    if gy is None:
        gy = torch.empty((B, Tn, HW, gcoff + C_), dtype=y.dtype, device=y.device)
    assert tuple(gy.shape[:3]) == (B, Tn, HW) and gy.dim() == 4 and gy.dtype == y.dtype and gy.is_contiguous() and gy.is_cuda
    assert 0 <= gcoff and gcoff + C_ <= gy.shape[3]
    dfeat = torch.empty((B, C_), dtype=torch.float32, device=y.device)
    check(load().flk_head_backward(ptr(y), ld, coff, ptr(gy), gy.shape[3], gcoff, C_, B, Tn, HW, ptr(wt), ptr(W), N, ptr(dlogits), ptr(dfeat),
                                   int(bool(use_mask)), dtype_code(y.dtype), stream_ptr()))
    return gy, dfeat


def pack_batch_sums(per_clip, prob_scale, out3):
    """out3 = [sum loss_b, prob_scale * sum p_label, prob_scale * sum p_max_other] from softmax_adv_loss's per-clip table"""
    assert per_clip.dtype == torch.float32 and per_clip.is_contiguous() and per_clip.shape[1] == 4 and out3.dtype == torch.float32
    check(load().flk_pack_batch_sums(ptr(per_clip), per_clip.shape[0], float(prob_scale), ptr(out3), stream_ptr()))
    return out3


_labels_ok = {}      # id(LIVE label tensor object) -> (weakref to it, _version, num_classes) it was range-checked at


def _labels_memo_get(labels):
    ent = _labels_ok.get(id(labels))
    return (ent[1], ent[2]) if ent is not None and ent[0]() is labels else None


def mark_labels_validated(labels, num_classes):
    """Record that ``labels`` (a CUDA tensor) was range-checked where it originated, on the host (the dataset driver checks the
    numpy labels of every record batch before the copy): check_labels then skips its device read-back for this tensor object.
    The entry is removed when the tensor object dies (weakref callback), so a recycled id / address can never inherit it."""
    key = id(labels)
    _labels_ok[key] = (weakref.ref(labels, lambda _r, k=key: _labels_ok.pop(k, None)), labels._version, num_classes)
    return labels


def check_labels(labels, batch, num_classes):
    """labels must be a contiguous CUDA int64 tensor of shape (batch,) with 0 <= label < num_classes: anything else would hand the
    loss kernel a host pointer (GPU memory fault), a wrong stride or an out-of-range class index.  Device / dtype / shape are checked
    on every call (free).  The range check reads min / max back from the device (two syncs) ONCE per live tensor object and
    version: the memo is keyed on the identity of the LIVE tensor object (weak reference) -- not on its address, which the caching allocator recycles for
    the next batch's labels -- so an entry dies with its tensor and an in-place write invalidates it.  A loop that reuses its label
    tensor pays the read-back once; a loop that builds labels per batch validates them on the host and says so
    (mark_labels_validated).  Independently, the kernel clamps a bad index and poisons that clip's outputs with NaN (head.hip)."""
    if not torch.is_tensor(labels) or not labels.is_cuda or labels.dtype != torch.int64 or tuple(labels.shape) != (batch,):
        desc = f"{tuple(labels.shape)} {labels.dtype} {labels.device}" if torch.is_tensor(labels) else type(labels).__name__
        raise ValueError(f"labels must be a CUDA int64 tensor of shape ({batch},), got {desc}")
    if not labels.is_contiguous():
        raise ValueError("labels must be contiguous")
    if _labels_memo_get(labels) != (labels._version, num_classes):
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= num_classes:
            raise ValueError(f"labels must lie in [0, {num_classes}), got [{lo}, {hi}]")
        mark_labels_validated(labels, num_classes)
    return labels


def softmax_adv_loss(logits, labels, *, dialect="tf", improve_loss=True, use_logits=False, targeted=False, margin=0.05,
                     mean_scale=1.0, out=None):
    """out: optional (softmax, dlogits, per_clip) buffers to write into"""
    B, Cn = logits.shape
    a = LossArgs()
    a.B, a.C = B, Cn
    a.torch_dialect, a.improve_loss, a.use_logits, a.targeted = int(dialect == "torch"), int(improve_loss), int(use_logits), int(targeted)
    a.margin, a.mean_scale = margin, mean_scale
    if out is None:
        sm = torch.empty_like(logits)
        dl = torch.empty_like(logits)
        pc = torch.empty((B, 4), dtype=torch.float32, device=logits.device)
    else:
        sm, dl, pc = out
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    check_labels(labels, B, Cn)
    check(load().flk_softmax_adv_loss(C.byref(a), ptr(logits), ptr(labels), ptr(sm), ptr(dl), ptr(pc), stream_ptr()))
    return sm, dl, pc


VIDEO_REDUCES = ("mean", "sum")


def video_scale(clips_per_video, reduce):
    """the factor on a video's summed clip logits: "sum" = 1 (the reference's evaluate), "mean" = 1/G (same argmax; the margin and CE
    hyper-parameters stay on the scale of one clip's logits)"""
    if reduce not in VIDEO_REDUCES:
        raise ValueError(f"reduce must be one of {VIDEO_REDUCES}, got {reduce!r}")
    if int(clips_per_video) < 1:
        raise ValueError(f"clips_per_video must be >= 1, got {clips_per_video!r}")
    return 1.0 if reduce == "sum" else 1.0 / int(clips_per_video)


def softmax_adv_loss_video(logits, labels, clips_per_video, *, reduce="mean", dialect="tf", improve_loss=True, use_logits=False,
                           targeted=False, margin=0.05, mean_scale=1.0, out=None):
    """the loss head on a video's aggregated logits (flk_softmax_adv_loss_video): ``logits`` [B = V*G, C] video-major and clip-minor,
    ``labels`` [V] -> (softmax [V,C], dlogits [B,C], per_video [V,4], video_logits [V,C]).  out: optional buffers, in that order"""
    B, Cn = logits.shape
    G = int(clips_per_video)
    scale = video_scale(G, reduce)
    if B % G:
        raise ValueError(f"{B} clips are not a multiple of clips_per_video = {G}")
    V = B // G
    check_labels(labels, V, Cn)
    a = LossArgs()
    a.B, a.C = B, Cn
    a.torch_dialect, a.improve_loss, a.use_logits, a.targeted = int(dialect == "torch"), int(improve_loss), int(use_logits), int(targeted)
    a.margin, a.mean_scale = margin, mean_scale
    if out is None:
        sm = torch.empty((V, Cn), dtype=torch.float32, device=logits.device)
        dl = torch.empty_like(logits)
        pv = torch.empty((V, 4), dtype=torch.float32, device=logits.device)
        vl = torch.empty((V, Cn), dtype=torch.float32, device=logits.device)
    else:
        sm, dl, pv, vl = out
        assert tuple(sm.shape) == (V, Cn) and tuple(dl.shape) == (B, Cn) and tuple(pv.shape) == (V, 4) and tuple(vl.shape) == (V, Cn)
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda for t in (sm, dl, pv, vl))
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.is_cuda
    check(load().flk_softmax_adv_loss_video(C.byref(a), G, scale, ptr(logits), ptr(labels), ptr(sm), ptr(vl), ptr(dl), ptr(pv), stream_ptr()))
    return sm, dl, pv, vl


class Net(_HandleOwner):
    """flk_net: whole-network forward + backward-to-input plan with resident packed weights."""
    _destroy = "flk_net_destroy"

    def __init__(self, arch, dtype, B, T, H, W, weights, device=0):
        self.dtype = dtype_code(dtype)
        self.B, self.T, self.H, self.W = B, T, H, W
        h = C.c_void_p()
        check(load().flk_net_create(arch, self.dtype, B, T, H, W, device, C.byref(h)))
        self.handle = h
        for name, arr in weights.items():
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            check(load().flk_net_set_weight(h, name.encode(), ptr(arr), arr.size))
        check(load().flk_net_finalize(h))
        self.num_classes = load().flk_net_num_classes(h)
        self.input_numel = load().flk_net_input_numel(h)
        # VideoResNet plans: channels of the (h,w)-folded input tensor -- 16, or 32 in bf16 (two bf16 numbers per value, fold_t = 4);
        # the input GRADIENT always has the 16-channel layout
        self.input_channels = load().flk_net_input_channels(h)
        self.input_fold = load().flk_net_input_fold(h)
        self.grad_numel = self.input_numel if arch == FLK_NET_I3D else self.input_numel // self.input_channels * 16
        self.workspace_bytes = load().flk_net_workspace_bytes(h)

    def forward(self, x_in, logits=None):
        if logits is None:
            logits = torch.empty((self.B, self.num_classes), dtype=torch.float32, device="cuda")
        assert x_in.numel() == self.input_numel and x_in.is_contiguous()
        check(load().flk_net_forward(self.handle, ptr(x_in), ptr(logits), 1, stream_ptr()))
        return logits

    @property
    def has_forward_flicker(self):
        """the exact perturbation path of the stem is available: I3D plan, bf16 (FLK_STEM_CENTER=0 switches it off)"""
        return bool(load().flk_net_has_forward_flicker(self.handle))

    def forward_flicker(self, x_in, apply_args, logits=None):
        """forward of a clip applied with ``center=True``: the perturbation enters the stem in fp32 through its epilogue"""
        if logits is None:
            logits = torch.empty((self.B, self.num_classes), dtype=torch.float32, device="cuda")
        assert x_in.numel() == self.input_numel and x_in.is_contiguous() and apply_args.center == 1
        check(load().flk_net_forward_flicker(self.handle, ptr(x_in), C.byref(apply_args), ptr(logits), stream_ptr()))
        return logits

    def forward_apply(self, apply_args, x_s2d, logits=None):
        """perturbation apply + forward in one call: the plan applies each batch slice on the stream its stem convolution runs on
        (x_s2d is scratch: it receives the space-to-depth clip unless the stem reads the uint8 clip itself -- the bf16 I3D plan with a
        centred uint8 clip -- in which case it is left untouched; call perturb_apply_s2d when the tensor itself is needed)"""
        if logits is None:
            logits = torch.empty((self.B, self.num_classes), dtype=torch.float32, device=x_s2d.device)
        assert x_s2d.is_contiguous() and x_s2d.numel() == self.input_numel and dtype_code(x_s2d.dtype) == self.dtype
        check(load().flk_net_forward_apply(self.handle, C.byref(apply_args), ptr(x_s2d), ptr(logits), stream_ptr()))
        return logits

    def backward(self, dlogits, gx=None):
        if gx is None:
            gx = torch.empty(self.grad_numel, dtype=torch_dtype(self.dtype), device="cuda")
        check(load().flk_net_backward(self.handle, ptr(dlogits), ptr(gx), stream_ptr()))
        return gx

    @property
    def has_backward_delta(self):
        """the fused stem delta-gradient (csrc/stem_grad.hip) is available: I3D plan, bf16 (FLK_STEM_FUSED=0 switches it off)"""
        return bool(load().flk_net_has_backward_delta(self.handle))

    def prepare_backward_delta(self, apply_args, scratch):
        """start the clip-mask pre-pass of the coming backward_delta(…, apply_args, …, scratch) now (beside the forward pass)"""
        check(load().flk_net_prepare_backward_delta(self.handle, C.byref(apply_args), ptr(scratch), stream_ptr()))

    def backward_delta(self, dlogits, apply_args, gdelta, scratch):
        """backward straight to the flickering perturbation [T,3]: no per-pixel input gradient is materialised"""
        assert gdelta.dtype == torch.float32 and gdelta.is_contiguous() and gdelta.numel() == 3 * self.T * (self.B if apply_args.delta_per_clip else 1)
        assert scratch.numel() * 4 >= load().flk_stem_delta_grad_scratch_bytes(self.B, self.T, self.H)
        check(load().flk_net_backward_delta(self.handle, ptr(dlogits), C.byref(apply_args), ptr(gdelta), ptr(scratch), stream_ptr()))
        return gdelta

    def autotune(self, x, logits, dlogits, gx):
        """tune the launch layout of every convolution of the plan on these operands (one serial forward + backward)"""
        check(load().flk_net_autotune(self.handle, ptr(x), ptr(logits), ptr(dlogits), ptr(gx), stream_ptr()))

    def profile(self, enable):
        check(load().flk_net_profile(self.handle, int(enable)))

    def profile_read(self):
        buf = C.create_string_buffer(1 << 20)
        check(load().flk_net_profile_read(self.handle, buf, len(buf)))
        return json.loads(buf.value.decode())

    def activation(self, name):
        dims = (C.c_int64 * 5)()
        check(load().flk_net_get_activation(self.handle, name.encode(), None, 0, dims))
        out = np.empty(tuple(dims), dtype=np.float32)
        check(load().flk_net_get_activation(self.handle, name.encode(), ptr(out), out.size, dims))
        return out
