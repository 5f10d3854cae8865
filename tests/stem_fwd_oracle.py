"""The CPU oracle of the stem computed straight from the uint8 clip (csrc/stem_fwd.hip: flk_stem_fwd_u8), shared by test_stem_fwd_gpu.py
and test_stem_fwd_edges_gpu.py.

The kernel's model (i3d.py:168-170, kinetics_i3d_utils.py:100-142):
    x'[t] = decode(clip)[(t - shift_x) mod T]            decode: u8 * x_scale + x_bias
    p'[t] = adv_flag * (clamp(delta, +-dclip) * inv_std)[(t - shift_p) mod T]          (no clamp with dclip <= 0; 0 with adv_flag = 0)
    xc    = clamp(x', lo - p', hi - p')                  = clip(x' + p', lo, hi) - p', staged as bf16
    y     = relu(conv7(xc, bf16(w)) * bn_scale + bn_bias + conv7(p' inside the frame, fp32(w * bn_scale)))
conv7 = 7x7x7 / 2, TF SAME (2 before, 3 after), 3 -> 64.  The last term is what the position-class table of flk_stem_delta_bias holds.

`staged_operands` evaluates the first three lines in numpy, in fp32 operation by operation as the kernel does (or in float64);
`stem_oracle` the last one in the dtype it is given; `stem_bound_ratio` holds a kernel output to the float64 oracle ON THE KERNEL'S OWN
OPERANDS, element by element, under conv_bound.bf16_bound_ratio.

The table term's error (TABLE_ERR).  One table entry is sum_{kt, c} p'[t, c] * S[kt, c] with S[kt, c] = sum_{kh, kw inside} fp32(w * scale):
the host sums up to 49 of these rounded products in fp32 one after the other (48 additions, relative error <= gamma_48 on sum |w * scale|),
the kernel multiplies and adds up to 21 terms (a dot product of length 21, fused or not: gamma_21), and the epilogue's addition of the
entry rounds once more: (48 + 21 + 1) u < 72 * 2^-24 of A = the same table on |p'| and |fp32(w * scale)| (gamma_n = n u / (1 - n u),
u = 2^-24; the second-order terms are what 72 leaves over 70).  The products fp32(w * scale) themselves are the oracle's operands too.  The
epilogue's other roundings -- fma(acc, scale, bias), then + entry: 2 u (|scale| S + |bias|) -- sit inside bf16_bound_ratio's
2^-22 |bias| and the half of n_K 2^-23 |scale| S that fp32 accumulation (gamma_{n_K}) does not use."""
import numpy as np
import torch
import torch.nn.functional as F

from conv_bound import bf16_bound_ratio

N_K = 37 * 32                   # the multiply-accumulates the kernel executes per output value (1029 taps + zero-weight slots)
TABLE_ERR = 72 * 2.0 ** -24


def f32(v):
    """the value a float takes as an fp32 kernel argument"""
    return float(np.float32(v))


def staged_operands(xu, delta, *, dtype=np.float32, dclip=0.4, dclip_dev=None, adv_flag=1.0, shift_x=0, shift_p=0,
                    inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0, x_scale=1.0 / 128, x_bias=-1.0):
    """(x', xc, p') of the model above as numpy arrays of `dtype`: x', xc [B,T,224,224,3], p' [B or 1, T, 3].  xu uint8 [B,T,224,224,3],
    delta fp32 [T,3] or [B,T,3], dclip_dev fp32 [B] or None (numpy).  Every scalar enters as the fp32 value the kernel receives.  In fp32
    each operation rounds once, in the kernel's order: d * inv_std, adv_flag * that, lo - p', hi - p', the median of three.  (The
    decode is u8 * x_scale + x_bias in two roundings; the kernel may fuse them, so fp32 callers use decodes that are exact.)"""
    f = np.dtype(dtype).type
    T = xu.shape[1]
    x = xu.astype(dtype) * f(f32(x_scale)) + f(f32(x_bias))
    if shift_x % T:
        x = np.roll(x, shift_x, axis=1)
    d = delta.astype(dtype).reshape(-1, T, 3)
    dc = (np.full(1, f32(dclip), np.float32) if dclip_dev is None else dclip_dev).astype(dtype).reshape(-1, 1, 1)
    d = np.where(dc > 0, np.clip(d, -dc, dc), d)
    p = d * np.array([f32(s) for s in inv_std], dtype)
    p = f(f32(adv_flag)) * np.roll(p, shift_p, axis=1) if adv_flag != 0 else np.zeros_like(p)
    lo_p, hi_p = f(f32(lo)) - p, f(f32(hi)) - p
    xc = np.minimum(np.maximum(x, lo_p[:, :, None, None, :]), hi_p[:, :, None, None, :])
    return x, xc, p


def conv7(inp, w):
    """7x7x7 / 2, TF SAME on even sizes: inp [B,T,H,W,3], w [7,7,7,3,64] (torch, one dtype) -> [B,T/2,H/2,W/2,64]"""
    y = F.conv3d(F.pad(inp.permute(0, 4, 1, 2, 3), (2, 3, 2, 3, 2, 3)), w.permute(4, 3, 0, 1, 2).contiguous(), stride=2)
    return y.permute(0, 2, 3, 4, 1)


_EDGE = torch.tensor([0] + [1] * 109 + [6, 7])


def conv7_frames(p, w):
    """conv7 of the clip whose frame t is the constant p[b, t, c] over its 224 x 224 pixels: [B,T/2,112,112,64].  The convolution is
    translation invariant, so a 16 x 16 frame has every kind of output row there is -- row 0, the interior rows 1..5, rows 6 and 7 of its
    8 are rows 0, 1..109, 110 and 111 of the 112 (the same along w).  Which taps an edge row loses is decided by conv3d, not here."""
    B, T, _ = p.shape
    small = conv7(p[:, :, None, None, :].expand(B, T, 16, 16, 3).contiguous(), w)
    if small.dtype == torch.float64:
        tol = 1e-13 * float(small.abs().max())
        assert float((small[:, :, 1:6] - small[:, :, 1:2]).abs().max()) <= tol and float((small[:, :, :, 1:6] - small[:, :, :, 1:2]).abs().max()) <= tol
    return small[:, :, _EDGE][:, :, :, _EDGE]


def stem_oracle(xc, p, w_clip, w_pert, scale, bias, dtype=torch.float64):
    """relu(conv7(xc, w_clip) * scale + bias + conv7(p inside the frame, w_pert)) evaluated in `dtype` (torch tensors; xc [B,T,224,224,3],
    p [B or 1, T, 3]): w_clip the weights the clip term multiplies, w_pert = fp32(w * scale) those of the perturbation term"""
    y = conv7(xc.to(dtype), w_clip.to(dtype)) * scale.to(dtype) + bias.to(dtype)
    return torch.relu(y + conv7_frames(p.to(dtype), w_pert.to(dtype)))


def kernel_operands(xu, delta, w7, scale, **kw):
    """what the kernel multiplies, as torch tensors: (bf16(xc) as fp32, p' fp32, bf16(w) as fp32, fp32(w * scale)) -- xc and p' by
    `staged_operands` in fp32.  xu, delta, w7, scale: torch CPU tensors"""
    dev = kw.pop("dclip_dev", None)
    _, xc, p = staged_operands(xu.numpy(), delta.numpy(), dtype=np.float32, dclip_dev=None if dev is None else dev.numpy(), **kw)
    return torch.from_numpy(xc).bfloat16().float(), torch.from_numpy(p), w7.bfloat16().float(), w7 * scale


def stem_bound_ratio(got, xc, p, w_clip, w_pert, scale, bias, ref=None):
    """asserts every element of the kernel output `got` (bf16 [B,T/2,112,112,>= 64], CPU) within the derived bound of the float64 oracle
    on the operands of `kernel_operands`:  |y - r| <= 2^-8 |r| + (1 + 2^-8) (n_K 2^-23 |scale| S + 2^-22 |bias| + TABLE_ERR A),
    S = conv7(|xc|, |w_clip|), A = conv7(|p| inside the frame, |w_pert|).  Returns (worst ratio, the oracle)."""
    if ref is None:
        ref = stem_oracle(xc, p, w_clip, w_pert, scale, bias)
    S = conv7(xc.abs().double(), w_clip.abs().double())
    A = conv7_frames(p.abs().double(), w_pert.abs().double())
    worst = 0.0
    for b in range(ref.shape[0]):        # bias_err is per element: one clip per call
        r, _ = bf16_bound_ratio(got[b:b + 1, ..., :64], ref[b:b + 1], S[b:b + 1], N_K, scale=scale, bias=bias,
                                bias_err=TABLE_ERR * A[b if A.shape[0] > 1 else 0])
        worst = max(worst, r)
    return worst, ref
