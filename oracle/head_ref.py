"""The classifier head (csrc/head.hip: flk_head_forward / flk_head_backward) restated in float64: a time-weighted average pool, a
linear layer, and their gradient masked by the producer's ReLU.  Plain torch; the tests compare the HIP kernels with this and
this with torch's own pooling / convolution / autograd (tests/test_head_contract_cpu.py).

    feat[b,c]   = sum_{t,p} wt[t] * y[b,t,p,c]
    logits[b,n] = bias[n] + sum_c feat[b,c] * W[c,n]
    dfeat[b,c]  = sum_n dlogits[b,n] * W[c,n]
    gy[b,t,p,c] = wt[t] * dfeat[b,c] where y[b,t,p,c] > 0 (or everywhere without the mask), else 0

Every function also returns the sum of the ABSOLUTE values of the terms of each sum it forms: the rounding-error bounds of the GPU
tests (n * 2^-24 * sum|terms|, the standard bound of recursive summation in any order) need them."""
import torch

F64 = torch.float64


def _f64(x):
    return torch.as_tensor(x).to(F64)


def pool_ref(y, wt):
    """y [B,Tn,HW,C], wt [Tn] -> (feat [B,C], sum|wt * y| [B,C]), float64"""
    y, wt = _f64(y), _f64(wt)
    w = wt.view(1, -1, 1, 1)
    return (w * y).sum(dim=(1, 2)), (w * y).abs().sum(dim=(1, 2))


def fc_ref(feat, W, bias):
    """feat [B,C], W [C,N], bias [N] or None -> (logits [B,N], |bias| + sum_c |feat * W| [B,N]), float64"""
    feat, W = _f64(feat), _f64(W)
    logits, mag = feat @ W, feat.abs() @ W.abs()
    if bias is not None:
        logits, mag = logits + _f64(bias), mag + _f64(bias).abs()
    return logits, mag


def head_forward_ref(y, wt, W, bias):
    """y: the activation already converted from its storage dtype (any float dtype; taken as float64).
    -> (feat, logits, sum|wt * y|, |bias| + sum|feat * W|)"""
    feat, feat_mag = pool_ref(y, wt)
    logits, logits_mag = fc_ref(feat, W, bias)
    return feat, logits, feat_mag, logits_mag


def fc_bwd_ref(dlogits, W):
    """dlogits [B,N], W [C,N] -> (dfeat [B,C], sum_n |dlogits * W| [B,C]), float64"""
    dlogits, W = _f64(dlogits), _f64(W)
    return dlogits @ W.t(), dlogits.abs() @ W.abs().t()


def pool_bwd_ref(y, wt, dfeat, use_mask):
    """gy [B,Tn,HW,C] = wt[t] * dfeat[b,c], zero where use_mask and not y > 0: the mask is a comparison, so -0.0, +0.0, negatives and NaN
    give zero, denormals and +inf pass (and inf never multiplies anything).  With use_mask false y gives the shape alone."""
    wt, dfeat = _f64(wt), _f64(dfeat)
    B, Tn, HW, C = y.shape
    g = (wt.view(1, Tn, 1, 1) * dfeat.view(B, 1, 1, C)).expand(B, Tn, HW, C)
    if use_mask:
        g = torch.where(y > 0, g, torch.zeros((), dtype=F64))
    return g.contiguous()


def head_backward_ref(y, wt, W, dlogits, use_mask):
    """-> (dfeat, gy, sum|dlogits * W|)"""
    dfeat, dfeat_mag = fc_bwd_ref(dlogits, W)
    return dfeat, pool_bwd_ref(y, wt, dfeat, use_mask), dfeat_mag


def i3d_time_weights(Tn):
    """I3D Logits: avg_pool3d 2x7x7 VALID stride 1 over a [Tn,7,7] grid, then the mean over its T' = Tn - 1 output frames.  Frame t lies
    in the windows starting at t - 1 and at t, those of them that exist: wt[t] = coverage / (2 * 7 * 7 * T')."""
    if Tn < 2:
        raise ValueError(f"the 2-frame pool needs Tn >= 2, got {Tn}")
    Tp = Tn - 1
    cover = torch.tensor([(1 if t - 1 >= 0 else 0) + (1 if t <= Tp - 1 else 0) for t in range(Tn)], dtype=F64)
    return cover / (2 * 7 * 7 * Tp)


def videoresnet_time_weights(Tn, HW):
    """AdaptiveAvgPool3d(1): the plain mean over all Tn * HW positions"""
    return torch.full((Tn,), 1.0 / (Tn * HW), dtype=F64)
