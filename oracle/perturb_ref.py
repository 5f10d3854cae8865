"""Bit-faithful numpy restatement of the perturbation apply and its delta-gradient (TEST INFRASTRUCTURE, see oracle/__init__.py).

oracle/attack_math.py states the mathematics in torch so that autograd supplies gradients; its fp32 sums have an order of their own.
This module evaluates what csrc/attack.hip evaluates, in float32, ONE operation at a time and in the kernel's order, so that

* ``apply_ref`` is the value the apply kernels write, and
* ``delta_grad_ref`` takes its pass mask from that same float32 ``u = x' + a p'`` and sums ``g * mask`` in int64 (integer-valued g)
  or float64 -- with integer g every fp32 partial sum of the kernels is an integer below 2^24, so their result does not depend on the
  summation order and must EQUAL this one.

Where it is bit-exact: adv_flag = 1 (a fused multiply-add cannot change x + 1 * p) and a decode without rounding -- the TF
``u8 / 128 - 1``, a table, or an fp32 clip.  Layouts are the plain ones: clips and gradients [B,T,H,W,3]; delta [T,3] (flicker),
[B,T,3] (one per clip) or [T,H,W,3] (dense).  Checked against attack_math + autograd by tests/test_perturb_ref_cpu.py."""
import numpy as np

F32 = np.float32


def decode(x, x_scale=1.0 / 128.0, x_bias=-1.0, x_lut=None):
    """the clip as the kernels see it (load6): fp32 as it is; uint8 through the table x_lut[v, c] or as v * x_scale + x_bias"""
    x = np.asarray(x)
    if x.dtype == np.float32:
        return x
    assert x.dtype == np.uint8 and x.shape[-1] == 3
    if x_lut is not None:
        lut = np.asarray(x_lut, dtype=F32)
        assert lut.shape == (256, 3)
        return lut[x, np.arange(3)]
    return (x.astype(F32) * F32(x_scale)).astype(F32) + F32(x_bias)


def _kind(x, delta):
    B, T, H, W, _ = x.shape
    if delta.shape == (T, 3):
        return "flicker"
    if delta.shape == (B, T, 3):
        return "per_clip"
    assert delta.shape == (T, H, W, 3), delta.shape
    return "dense"


def _bounds(kind, B, dclip, dclip_dev):
    """clamp bound of delta broadcast against it: a scalar, or one per clip (dclip_dev, per-clip deltas only)"""
    if dclip_dev is not None:
        assert kind == "per_clip"
        return np.asarray(dclip_dev, dtype=F32).reshape(B, 1, 1)
    return F32(dclip)


def perturbation(x_shape, delta, dclip=0.4, inv_std=(1.0, 1.0, 1.0), shift_p=0, dclip_dev=None):
    """p'[.., t, ..] = p[(t - shift_p) mod T], p = clamp(delta, +-dclip) * inv_std[c] (pert_at), broadcastable to [B,T,H,W,3]"""
    B, T, H, W, _ = x_shape
    delta = np.asarray(delta, dtype=F32)
    kind = {(T, 3): "flicker", (B, T, 3): "per_clip"}.get(delta.shape, "dense")
    dc = _bounds(kind, B, dclip, dclip_dev)
    d = np.where(dc > 0, np.minimum(np.maximum(delta, -dc), dc), delta).astype(F32)
    p = (d * np.asarray(inv_std, dtype=F32)).astype(F32)
    axis = 1 if kind == "per_clip" else 0
    p = np.roll(p, shift_p, axis=axis)
    if kind == "flicker":
        return p.reshape(1, T, 1, 1, 3)
    if kind == "per_clip":
        return p.reshape(B, T, 1, 1, 3)
    return p.reshape(1, T, H, W, 3)


def clamp_input(x, delta, *, dclip=0.4, inv_std=(1.0, 1.0, 1.0), adv_flag=1.0, shift_x=0, shift_p=0, x_scale=1.0 / 128.0, x_bias=-1.0,
                x_lut=None, dclip_dev=None):
    """u = x' + adv_flag * p' in float32: the number both the apply and the gradient kernels compare with lo and hi"""
    xd = decode(x, x_scale, x_bias, x_lut)
    assert xd.ndim == 5 and xd.shape[-1] == 3
    _kind(xd, np.asarray(delta))
    xr = np.roll(xd, shift_x, axis=1)                                   # x'[t] = x[(t - shift_x) mod T]
    if F32(adv_flag) == 0:
        return xr
    pv = (F32(adv_flag) * perturbation(xd.shape, delta, dclip, inv_std, shift_p, dclip_dev)).astype(F32)
    return (xr + pv).astype(F32)


def apply_ref(x, delta, *, lo=-1.0, hi=1.0, **kw):
    """x_adv = clamp(x' + adv_flag * p', lo, hi), float32 [B,T,H,W,3]; keywords of ``clamp_input``"""
    u = clamp_input(x, delta, **kw)
    return np.minimum(np.maximum(u, F32(lo)), F32(hi)).astype(F32)


def pass_mask(x, delta, *, lo=-1.0, hi=1.0, **kw):
    """1[lo <= u <= hi], both bounds inclusive (the gradient of both clamps), bool [B,T,H,W,3]"""
    u = clamp_input(x, delta, **kw)
    return (u >= F32(lo)) & (u <= F32(hi))


def delta_grad_ref(x, delta, g, *, lo=-1.0, hi=1.0, dclip=0.4, inv_std=(1.0, 1.0, 1.0), adv_flag=1.0, shift_p=0, dclip_dev=None, **kw):
    """d(loss)/d(delta) for the clip gradient g [B,T,H,W,3] (plain layout): sum of g * mask over (b,h,w) (flicker), over b (dense) or over
    (h,w) per clip ([B,T,3]); frame t goes back to the delta row (t - shift_p) mod T it was rolled from; rows with |delta| > dclip are
    zero; the sum -- rounded to float32 -- times float32(adv_flag), then times float32(inv_std[c]).  float32, the shape of delta."""
    delta = np.asarray(delta, dtype=F32)
    g = np.asarray(g)
    mask = pass_mask(x, delta, lo=lo, hi=hi, dclip=dclip, inv_std=inv_std, adv_flag=adv_flag, shift_p=shift_p, dclip_dev=dclip_dev, **kw)
    B, T, H, W, _ = mask.shape
    assert g.shape == mask.shape
    kind = _kind(mask, delta)
    integral = bool(np.all(g == np.rint(g)))
    gm = np.where(mask, g.astype(np.int64 if integral else np.float64), 0)
    if kind == "flicker":
        s, axis = gm.sum(axis=(0, 2, 3)), 0
    elif kind == "per_clip":
        s, axis = gm.sum(axis=(2, 3)), 1
    else:
        s, axis = gm.sum(axis=0), 0
    s = np.roll(s, -shift_p, axis=axis)                                 # row ts takes frame ts + shift_p
    dc = _bounds(kind, B, dclip, dclip_dev)
    keep = ~(dc > 0) | ((delta >= -dc) & (delta <= dc))
    out = (s.astype(F32) * F32(adv_flag)).astype(F32)
    out = (out * np.asarray(inv_std, dtype=F32)).astype(F32)
    return np.where(keep, out, F32(0)).astype(F32)
