"""The derived error bound of a bf16 convolution output against a high-precision reference on the same bf16 operands, shared by the
kernel-level convolution tests (test_conv_pc_scale_gpu.py, test_conv_instances_gpu.py) -- one bf16 output rounding plus fp32
accumulation on both sides:
    |y - r| <= 2^-8 |r| + (1 + 2^-8) E,   E = n_K 2^-23 |s| S + 2^-22 (|b| + |add|)
with S the same operator on |x| and |w|, n_K = taps x cin, s / b the epilogue's scale and bias (1 / 0 without)."""
import torch


def bf16_bound_ratio(y, r, S, nK, *, scale=None, bias=None, add=None, bias_err=None, against=None):
    """worst |y - r| / bound over y [B, ..., cout] against the reference r (the epilogue applied: scale, bias, + add, ReLU, mask) with S
    the operator on |x|, |w| (no epilogue); asserts the bound on every element.  scale / bias: the epilogue's per-channel vectors; add:
    the residual operand [B, ..., cout]; bias_err: a bound on how far the bias the kernel used may be from `bias` (added to E).
    against: compare y with these values instead of r (another launch's output of the same convolution); the bound is still built from r.
    Returns (worst ratio, clip it occurred in)."""
    s = scale.double().abs() if scale is not None else 1.0
    b_abs = bias.double().abs() if bias is not None else 0.0
    worst, where = 0.0, None
    for b in range(r.shape[0]):         # float64, one clip at a time
        rb, yb = r[b].double(), y[b].double()
        cb = rb if against is None else against[b].double()
        E = nK * 2.0 ** -23 * s * S[b].double() + 2.0 ** -22 * (b_abs + (add[b].double().abs() if add is not None else 0.0))
        if bias_err is not None:
            E = E + bias_err.double()
        bound = 2.0 ** -8 * rb.abs() + (1 + 2.0 ** -8) * E
        err = (yb - cb).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{int(bad.sum())} elements outside the bound, the first at clip {b} {i}: y {float(yb[i])}, "
                                 f"{'r' if against is None else 'compared with'} {float(cb[i])}, bound {float(bound[i])}")
        rw = float(torch.where(bound > 0, err / bound, torch.zeros((), dtype=torch.float64)).max())
        if where is None or rw > worst:
            worst, where = rw, b
    return worst, where
