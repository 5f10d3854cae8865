"""Max-pool kernels (csrc/pool.hip) at their edges (GPU): every dispatch family of flk_maxpool3d_fwd / _bwd / _bwd_gemm against a plain
float64 restatement on the CPU (torch max_pool3d with indices + an explicit scatter), on signed data, zero-sign ties, -inf windows,
channel slices of wider buffers, ragged and degenerate tiles, geometries outside the I3D ones, and the operating range of the bf16
fixed-point backward.

What is asserted, and where the bounds come from (nothing here is measured):
  * out and the argmax bytes idx are EXACT (max-pooling selects, it does not compute): first maximum in (t,h,w) scan order, values
    compared as numbers (-0.0 == +0.0; the bf16 key kernels deviate on zero signs, see test_zero_sign_ties), padded cells never win, a
    window of -inf records tap 0, relu_input records 255 where max <= 0.
  * fp32 backward: the existing fp32 tolerance of tests/test_kernels_gpu.py (summation order only).
  * bf16 backward, fixed-point forms (scatter, fused): a cell is the sum of at most n = prod ceil(k/s) addends, each rounded to a
    multiple of 2^-E * 2^floor(log2 max|gout|), E = min(24, 30 - ceil(log2 n)): |sum - exact| <= delta = n * 2^-(E+1) * max|gout|
    (the kernel's documented error), then ONE round-to-nearest to bf16 (relative 2^-8):  |got - ref| <= delta + 2^-8 (|ref| + delta).
  * bf16 backward, owner form (the strided I3D pools; a plain fp32 sum of <= 8 addends in fixed order): the same shape of bound with
    delta = (n - 1) * 2^-24 * sum|addends| (standard recursive-summation bound).
The fused Branch_3 backward is always fed g and Wt made of small integers and powers of two, so that every product and K-sum is exact in
fp32 in any order and the bounds above apply to it unchanged."""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
FORMS = pytest.mark.parametrize("form", ["reg", "loop"])
INF = float("inf")
GMAX = 1.9921875          # bf16 0x3FFF: the largest mantissa


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale)


def q(x, dtype):
    """round to the storage dtype (bf16 mode) and back to fp32"""
    return x.to(dtype).float()


def tol(dtype, ref):
    s = float(ref.abs().max()) + 1e-12
    return (1e-4, 1e-5 * s) if dtype == torch.float32 else (1e-2, 1e-2 * s)


def cl(x):   # NCDHW -> NDHWC
    return x.permute(0, 2, 3, 4, 1).contiguous()


def cf(x):   # NDHWC -> NCDHW
    return x.permute(0, 4, 1, 2, 3).contiguous()


def dev(x, dtype):
    return x.to(dtype).cuda()


def bits(x):
    """bit pattern of a float tensor (compares -0.0 != +0.0, unlike ==)"""
    return x.detach().cpu().contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def same(n, k, s):
    """TF SAME: (out, pad before, pad after)"""
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return out, tot // 2, tot - tot // 2


def cover(k, s):
    """the largest number of windows that contain one cell"""
    return math.prod(-(-kk // ss) for kk, ss in zip(k, s))


def fx_e(n):
    return min(24, 30 - math.ceil(math.log2(n))) if n > 1 else 24


class Ref:
    """float64 max-pool (SAME, -inf padding) of x [B,T,H,W,C]: .out [B,To,Ho,Wo,C] float64, .tap uint8 (the expected idx), .bwd(gout).
    pad_before: an explicit pad-before per dimension instead of SAME's (stride 1: the output grid is the input grid and the pad-after is
    k - 1 - pad_before)"""

    def __init__(self, x, k, s, relu_input=False, pad_before=None):
        B, T, H, W, C = x.shape
        g = [same(n, kk, ss) for n, kk, ss in zip((T, H, W), k, s)]
        if pad_before is not None:
            assert tuple(s) == (1, 1, 1)
            g = [(n, pb, kk - 1 - pb) for n, kk, pb in zip((T, H, W), k, pad_before)]
        self.shape, self.pb = (B, T, H, W, C), [a[1] for a in g]
        xp = F.pad(cf(x).double(), [g[2][1], g[2][2], g[1][1], g[1][2], g[0][1], g[0][2]], value=-INF)
        y, fi = F.max_pool3d(xp, k, s, return_indices=True)
        self.xp = xp
        assert tuple(y.shape[2:]) == tuple(a[0] for a in g)
        self.pshape = tuple(xp.shape[2:])
        Tp, Hp, Wp = self.pshape
        it, ih, iw = fi // (Hp * Wp), fi // Wp % Hp, fi % Wp
        ot = torch.arange(y.shape[2]).view(1, 1, -1, 1, 1) * s[0]
        oh = torch.arange(y.shape[3]).view(1, 1, 1, -1, 1) * s[1]
        ow = torch.arange(y.shape[4]).view(1, 1, 1, 1, -1) * s[2]
        tap = ((it - ot) * k[1] + (ih - oh)) * k[2] + (iw - ow)
        assert int(tap.min()) >= 0 and int(tap.max()) < k[0] * k[1] * k[2]
        if relu_input:
            tap = torch.where(y <= 0, torch.full_like(tap, 255), tap)
        self.fi, self.live = fi, tap != 255
        self.out, self.tap = cl(y), cl(tap).to(torch.uint8)

    def bwd(self, gout, mask=None):
        """gout [B,To,Ho,Wo,C] scattered to the argmax cells in float64; gradient that lands on a padded cell is dropped"""
        B, T, H, W, C = self.shape
        Tp, Hp, Wp = self.pshape
        g = torch.where(self.live, cf(gout).double(), torch.zeros((), dtype=torch.float64))
        buf = torch.zeros((B, C, Tp * Hp * Wp), dtype=torch.float64)
        buf.scatter_add_(2, self.fi.reshape(B, C, -1), g.reshape(B, C, -1))
        p = self.pb
        r = cl(buf.view(B, C, Tp, Hp, Wp)[:, :, p[0]:p[0] + T, p[1]:p[1] + H, p[2]:p[2] + W])
        return r if mask is None else torch.where(mask > 0, r, torch.zeros_like(r))


def check_fwd(out, idx, ref, bitwise=True):
    o = out.float().cpu()
    if bitwise:
        assert torch.equal(bits(o), bits(ref.out.float())), "out differs from the reference"
    else:
        assert torch.equal(o.double(), ref.out), "out differs in value from the reference"
    bad = (idx.cpu() != ref.tap).nonzero()
    assert len(bad) == 0, f"{len(bad)} argmax bytes differ, first at {bad[0].tolist()}: got {int(idx.cpu()[tuple(bad[0])])}, want {int(ref.tap[tuple(bad[0])])}"


OWNER = {((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2))}


def check_bwd(got, ref, gout, k, s, dtype, mask=None, fused=False):
    """gout: the gradient the reference was fed (for the fused form: the exact float64 product)"""
    want = ref.bwd(gout, mask)
    got = got.float().cpu()
    if dtype == F32:
        r, a = tol(dtype, want)
        torch.testing.assert_close(got, want.float(), rtol=r, atol=a)
        return
    n = cover(k, s)
    if (tuple(k), tuple(s)) in OWNER and not fused:
        acc = (n - 1) * 2.0 ** -24 * ref.bwd(gout.abs(), mask)
    else:
        acc = torch.full_like(want, n * 2.0 ** -(fx_e(n) + 1) * float(gout.abs().max()))
    bound = acc + 2.0 ** -8 * (want.abs() + acc)
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"k={k} s={s} n={n}: max |got - ref| = {float(err.max()):.3e}, max err / bound = {ratio:.3f}")
    bad = (err > bound).nonzero()
    assert len(bad) == 0, f"{len(bad)} cells beyond the bound; first {bad[0].tolist()}: got {float(got[tuple(bad[0])])}, want {float(want[tuple(bad[0])])}"


def exact_gw(pos_shape, K, C, seed):
    """g (small integers) and Wt (+-powers of two): every product and K-sum is exact in fp32 in any order (|sum| <= 128 * 4, steps of 2^-3)"""
    rng = np.random.default_rng(seed)
    g = torch.from_numpy(rng.integers(-4, 5, (*pos_shape, K)).astype(np.float32))
    wt = torch.from_numpy((rng.choice([-1.0, 1.0], (K, C)) * 2.0 ** rng.integers(-3, 1, (K, C))).astype(np.float32))
    return g, wt


def set_form(monkeypatch, form):
    if form == "loop":
        monkeypatch.setenv("FLK_POOL_GEMM_REG", "0")
    else:
        monkeypatch.delenv("FLK_POOL_GEMM_REG", raising=False)


# name -> (window, stride, extents).  The four I3D pools (the stride-1 one at a W that is a multiple of 7 and one that is not: the two
# W-run widths), 1x3x3 / 1, and geometries no network here uses but the ABI accepts: stride above the window (uncovered cells), an even
# window at stride 1 (LDS-tiled route), 125 taps, mixed strides, and windows flat in one or two dimensions.
GEOS = {
    "2a": ((1, 3, 3), (1, 2, 2), (3, 15, 13)),
    "4a": ((3, 3, 3), (2, 2, 2), (5, 7, 9)),
    "5a": ((2, 2, 2), (2, 2, 2), (4, 7, 6)),
    "b3_w7": ((3, 3, 3), (1, 1, 1), (3, 7, 14)),
    "b3_w8": ((3, 3, 3), (1, 1, 1), (5, 13, 30)),
    "133_s1": ((1, 3, 3), (1, 1, 1), (3, 9, 9)),
    "111_s2": ((1, 1, 1), (2, 2, 2), (5, 7, 9)),
    "222_s1": ((2, 2, 2), (1, 1, 1), (4, 9, 10)),
    "555_s1": ((5, 5, 5), (1, 1, 1), (6, 11, 12)),
    "333_s122": ((3, 3, 3), (1, 2, 2), (4, 15, 13)),
    "231_s121": ((2, 3, 1), (1, 2, 1), (5, 9, 8)),
    "311_s211": ((3, 1, 1), (2, 1, 1), (9, 6, 8)),
}
OTHER = ["111_s2", "222_s1", "555_s1", "333_s122", "231_s121", "311_s211"]
GEO = pytest.mark.parametrize("geo", list(GEOS))


def make_input(kind, shape, dtype, seed):
    x = rnd(shape, seed)
    if kind == "relu_input":        # zeros, positives and negatives: windows whose maximum is exactly 0, above it and below it
        x = torch.where(x.abs() < 1.2, torch.zeros_like(x), x)
    elif kind == "all_negative":
        x = -x.abs() - 0.25
    elif kind == "zero_signs":       # {-1, -0.0, +0.0}: many windows hold a -0.0 earlier in scan order than a +0.0
        c = torch.from_numpy(np.random.default_rng(seed).integers(0, 3, shape))
        x = torch.where(c == 0, torch.tensor(-1.0), torch.where(c == 1, torch.tensor(-0.0), torch.tensor(0.0)))
    return q(x, dtype)


@functools.lru_cache(maxsize=None)
def case(geo, dtype, kind, B=2, C=24):
    """input and float64 reference of one (geometry, dtype, data kind), computed once and shared (treat as read-only)"""
    k, s, dims = GEOS[geo]
    x = make_input(kind, (B, *dims, C), dtype, 100 + list(GEOS).index(geo))
    return x, Ref(x, k, s, relu_input=kind in ("relu_input", "all_negative"))


# ---- A / F: out and idx against the reference on signed data, every geometry ---------------------------------------------------------

@DTYPES
@GEO
@pytest.mark.parametrize("kind", ["signed", "relu_input", "all_negative"])
def test_forward_out_and_idx_exact(ops, geo, dtype, kind):
    k, s, _ = GEOS[geo]
    x, ref = case(geo, dtype, kind)
    out, idx, _ = ops.maxpool3d(dev(x, dtype), k, s, relu_input=kind != "signed")
    check_fwd(out, idx, ref)
    if kind == "all_negative":
        assert bool((idx == 255).all())


@DTYPES
@GEO
def test_backward_signed_data(ops, geo, dtype):
    """MaxPool3DGrad of N(0,1) gradients on signed data, with and without the fused mask; cells no window covers come back exactly 0"""
    k, s, dims = GEOS[geo]
    x, ref = case(geo, dtype, "signed")
    _, idx, ctx = ops.maxpool3d(dev(x, dtype), k, s)
    assert torch.equal(idx.cpu(), ref.tap)
    g = q(rnd(tuple(ref.out.shape), 7), dtype)
    gin = ops.maxpool3d_bwd(ctx, dev(g, dtype))
    check_bwd(gin, ref, g, k, s, dtype)
    check_bwd(ops.maxpool3d_bwd(ctx, dev(g, dtype), mask=dev(x, dtype)), ref, g, k, s, dtype, mask=x)
    covered = ref.bwd(torch.ones_like(g)) > 0
    if geo == "111_s2":
        assert float(covered.double().mean()) < 0.2              # stride above the window: most cells lie in no window
    assert bool((gin.float().cpu()[~covered] == 0).all())


@DTYPES
@pytest.mark.parametrize("geo", ["b3_w8", "4a", "333_s122"])
def test_minus_inf_windows(ops, geo, dtype):
    """whole windows of -inf: out = -inf, tap 0; their gradient is dropped where tap 0 is a padded cell (the corner windows)"""
    k, s, dims = GEOS[geo]
    x = q(rnd((2, *dims, 24), 55), dtype)
    x[:, :3, :5, :5, :] = -INF
    ref = Ref(x, k, s)
    dead = ref.out == -INF
    assert int(dead.sum()) >= 8 * 24 and bool((ref.tap[dead] == 0).all())
    out, idx, ctx = ops.maxpool3d(dev(x, dtype), k, s)
    check_fwd(out, idx, ref)
    g = q(rnd(tuple(ref.out.shape), 56), dtype)
    check_bwd(ops.maxpool3d_bwd(ctx, dev(g, dtype)), ref, g, k, s, dtype)
    out, idx, _ = ops.maxpool3d(dev(x, dtype), k, s, relu_input=True)
    check_fwd(out, idx, Ref(x, k, s, relu_input=True))


# ---- B: zero-sign ties ---------------------------------------------------------------------------------------------------------------

KEY_KERNEL_GEOS = ("b3_w7", "b3_w8")     # in bf16 these take the sortable-key forwards, which rank +0.0 above -0.0 (documented deviation)


def repointed(ref, idx, k, s):
    """(a copy of ref whose argmax cells are the ones the taps idx [B,To,Ho,Wo,C] name, which of them lie inside the unpadded input)"""
    tap = cf(idx.cpu().long())
    Tp, Hp, Wp = ref.pshape
    (T, H, W), p = ref.shape[1:4], ref.pb
    ot = torch.arange(tap.shape[2]).view(1, 1, -1, 1, 1) * s[0]
    oh = torch.arange(tap.shape[3]).view(1, 1, 1, -1, 1) * s[1]
    ow = torch.arange(tap.shape[4]).view(1, 1, 1, 1, -1) * s[2]
    it, ih, iw = ot + tap // (k[1] * k[2]), oh + tap // k[2] % k[1], ow + tap % k[2]
    inside = (it >= p[0]) & (it < p[0] + T) & (ih >= p[1]) & (ih < p[1] + H) & (iw >= p[2]) & (iw < p[2] + W)
    r = copy.copy(ref)
    r.fi, r.tap = (it * Hp + ih) * Wp + iw, idx.cpu()
    return r, inside


@DTYPES
@GEO
def test_zero_sign_ties(ops, geo, dtype):
    """-0.0 and +0.0 are the same number: the FIRST of them in scan order is the argmax (the reference's taps, exactly), in every float
    kernel.  The bf16 key kernels (KEY_KERNEL_GEOS) order values as integers with +0.0 above -0.0; they are pinned to the weaker rule
    pool.hip documents: the recorded tap names an in-bounds cell whose value equals the window maximum, and the backward sends each
    gradient to exactly that cell.  Either zero sign is accepted in out."""
    k, s, _ = GEOS[geo]
    x, ref = case(geo, dtype, "zero_signs")
    if k[0] * k[1] * k[2] > 1:
        # the case this test is about is in the data: windows whose first maximum is a -0.0 and which hold a +0.0 later in scan order
        first = ref.xp.flatten(2).gather(2, ref.fi.flatten(2)).view_as(ref.fi)
        holds_pos_zero = F.max_pool3d(((ref.xp == 0) & ~torch.signbit(ref.xp)).double(), k, s) > 0
        assert int(((first == 0) & torch.signbit(first) & holds_pos_zero).sum()) > 100
        assert int(((ref.out == 0) & (ref.tap > 0)).sum()) > 0
    out, idx, ctx = ops.maxpool3d(dev(x, dtype), k, s)
    if dtype == BF16 and geo in KEY_KERNEL_GEOS:
        assert torch.equal(out.float().cpu().double(), ref.out), "out differs in value from the reference"
        assert int(idx.max()) < k[0] * k[1] * k[2]
        ref, inside = repointed(ref, idx, k, s)
        assert bool(inside.all()), "a recorded tap names a padded cell"
        named = ref.xp.flatten(2).gather(2, ref.fi.flatten(2)).view_as(ref.fi)
        assert torch.equal(cl(named), ref.out), "a recorded tap names a cell whose value is not the window maximum"
    else:
        check_fwd(out, idx, ref, bitwise=False)
    g = q(rnd(tuple(ref.out.shape), 8), dtype)
    check_bwd(ops.maxpool3d_bwd(ctx, dev(g, dtype)), ref, g, k, s, dtype)


# ---- C: channel slices of wider buffers, slab tails ------------------------------------------------------------------------------------

SENT = 7.0
IN_OFF, OUT_OFF, GOUT_OFF, GIN_OFF, MASK_OFF = 8, 16, 24, 32, 40


def widen(t, coff, extra, seed):
    """t as channels [coff, coff + C) of a buffer `extra` channels wider, random elsewhere"""
    w = rnd((*t.shape[:4], t.shape[4] + extra), seed)
    w[..., coff:coff + t.shape[4]] = t
    return w


def assert_slice(buf, coff, C_, contiguous, what):
    """(i) nothing outside the slice was written, (ii) the slice is bitwise the contiguous call's result"""
    b = buf.cpu()
    assert bool((b[..., :coff].float() == SENT).all()) and bool((b[..., coff + C_:].float() == SENT).all()), f"{what}: wrote outside its slice"
    assert torch.equal(bits(b[..., coff:coff + C_]), bits(contiguous)), f"{what}: slice differs from the contiguous call"


# forward families: _k (2a, 5a, bf16 4a), generic (311_s211, fp32 4a), LDS-tiled (fp32 b3_*), W-run 7 / 8 (bf16 b3_w7 / b3_w8).
# bf16 3x3x3 / 1 with a pad-before other than 1, which SAME padding (all the wrappers compute) never gives, takes the LDS-tiled float
# forward maxpool_s1_tiled_fwd<bf16_t> like every other tiled window: test_explicit_pad_before calls the C ABI with such pads.
# backward families: owner (2a, 4a, 5a), gather (fp32 311_s211 / 333_s122), tiled gather (fp32 b3_*), scatter (every other bf16 one)
@DTYPES
@pytest.mark.parametrize("C_", [8, 40, 72])
@pytest.mark.parametrize("geo", ["2a", "4a", "5a", "b3_w7", "b3_w8", "311_s211", "333_s122"])
def test_channel_slices(ops, geo, dtype, C_):
    k, s, dims = GEOS[geo]
    B = 2
    x = make_input("relu_input", (B, *dims, C_), dtype, 61)
    ref = Ref(x, k, s)
    g = q(rnd(tuple(ref.out.shape), 62), dtype)
    xd, gd = dev(x, dtype), dev(g, dtype)
    # contiguous calls, against the reference
    out, idx, ctx = ops.maxpool3d(xd, k, s)
    check_fwd(out, idx, ref)
    gin = ops.maxpool3d_bwd(ctx, gd)
    gin_m = ops.maxpool3d_bwd(ctx, gd, mask=xd)
    check_bwd(gin, ref, g, k, s, dtype)
    check_bwd(gin_m, ref, g, k, s, dtype, mask=x)
    # the same through slices of wider buffers at five different offsets
    xw = dev(widen(x, IN_OFF, 24, 63), dtype)
    outw = torch.full((*out.shape[:4], C_ + 40), SENT, dtype=dtype, device="cuda")
    out2, idx2, ctx2 = ops.maxpool3d(xw, k, s, C_, in_coff=IN_OFF, out=outw, out_coff=OUT_OFF)
    assert out2 is outw and torch.equal(idx2, idx)
    assert_slice(outw, OUT_OFF, C_, out, "out")
    gw = dev(widen(g, GOUT_OFF, 32, 64), dtype)
    mw = dev(widen(x, MASK_OFF, 48, 65), dtype)
    for mask, want in ((None, gin), (mw, gin_m)):
        ginw = torch.full((*x.shape[:4], C_ + 48), SENT, dtype=dtype, device="cuda")
        ops.maxpool3d_bwd(ctx2, gw, mask=mask, gout_coff=GOUT_OFF, gin=ginw, gin_coff=GIN_OFF, mask_coff=MASK_OFF)
        assert_slice(ginw, GIN_OFF, C_, want, "gin")


@FORMS
@pytest.mark.parametrize("C_,K", [(72, 32), (40, 96)])
def test_channel_slices_fused(ops, C_, K, form, monkeypatch):
    set_form(monkeypatch, form)
    k, s, dims = (3, 3, 3), (1, 1, 1), (4, 7, 9)
    B = 2
    x = make_input("relu_input", (B, *dims, C_), BF16, 66)
    ref = Ref(x, k, s)
    g, wt = exact_gw((B, *dims), K, C_, 67)
    wp = ops.PoolGemmWeights(wt.numpy())
    gpl = g.double() @ wt.double()
    _, idx, ctx = ops.maxpool3d(dev(x, BF16), k, s)
    assert torch.equal(idx.cpu(), ref.tap)
    gin = ops.maxpool3d_bwd_gemm(ctx, dev(g, BF16), wp)
    check_bwd(gin, ref, gpl, k, s, BF16, fused=True)
    xw = dev(widen(x, IN_OFF, 24, 68), BF16)
    _, idx2, ctx2 = ops.maxpool3d(xw, k, s, C_, in_coff=IN_OFF)
    assert torch.equal(idx2, idx)
    ginw = torch.full((*x.shape[:4], C_ + 48), SENT, dtype=BF16, device="cuda")
    ops.maxpool3d_bwd_gemm(ctx2, dev(widen(g, GOUT_OFF, 32, 69), BF16), wp, g_coff=GOUT_OFF, gin=ginw, gin_coff=GIN_OFF)
    assert_slice(ginw, GIN_OFF, C_, gin, "fused gin")


# ---- D: many ragged tiles, degenerate extents ------------------------------------------------------------------------------------------

def fwd_bwd_fused(ops, dtype, k, s, B, dims, C_, seed, monkeypatch, fused):
    x = make_input("relu_input", (B, *dims, C_), dtype, seed)
    ref = Ref(x, k, s)
    out, idx, ctx = ops.maxpool3d(dev(x, dtype), k, s)
    check_fwd(out, idx, ref)
    g = q(rnd(tuple(ref.out.shape), seed + 1), dtype)
    check_bwd(ops.maxpool3d_bwd(ctx, dev(g, dtype)), ref, g, k, s, dtype)
    if fused and dtype == BF16:
        gk, wt = exact_gw(tuple(ref.out.shape[:4]), 32, C_, seed + 2)             # g has the OUT geometry
        wp = ops.PoolGemmWeights(wt.numpy())
        gpl = gk.double() @ wt.double()
        for form in ("reg", "loop"):
            set_form(monkeypatch, form)
            check_bwd(ops.maxpool3d_bwd_gemm(ctx, dev(gk, BF16), wp), ref, gpl, k, s, BF16, fused=True)


@DTYPES
@pytest.mark.parametrize("k,s,dims", [((3, 3, 3), (1, 1, 1), (11, 29, 31)), ((3, 3, 3), (2, 2, 2), (23, 29, 31))], ids=["branch3", "owner_4a"])
def test_many_ragged_tiles(ops, dtype, k, s, dims, monkeypatch):
    """prime extents above every tile edge: ragged edge tiles in every dimension for every tile chooser, far more than 8 tiles (the
    8-way dealing of tiles to XCDs and its idle tail blocks), a full channel slab plus a one-chunk tail; in bf16 also the fused
    backward in both forms -- for owner_4a that is flk_maxpool3d_bwd_gemm on a STRIDED window (g in the out geometry, n = 8)"""
    fwd_bwd_fused(ops, dtype, k, s, 3, dims, 40, 71, monkeypatch, fused=True)


@DTYPES
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 2), (2, 1, 9), (1, 8, 1)], ids=lambda d: "x".join(map(str, d)))
def test_tiny_extents(ops, dtype, dims, monkeypatch):
    """3x3x3 / 1 windows that are mostly padding, W below the W-run width"""
    fwd_bwd_fused(ops, dtype, (3, 3, 3), (1, 1, 1), 2, dims, 40, 75, monkeypatch, fused=True)


# ---- E: the bf16 fixed-point backward --------------------------------------------------------------------------------------------------

def run_bwd(ops, ctx, kind, gout, monkeypatch, wp=None):
    """kind: scatter | reg | loop.  gout: the window gradient (scatter) or the g rows of the fused product"""
    if kind == "scatter":
        return ops.maxpool3d_bwd(ctx, dev(gout, BF16))
    set_form(monkeypatch, kind)
    return ops.maxpool3d_bwd_gemm(ctx, dev(gout, BF16), wp)


def peaks_input(k, dims, C_, seed):
    """2.0 on the lattice t,h,w = k//2 (mod k), uniform [0, 0.5) elsewhere: every window holds exactly one peak and every peak receives
    all k^3 windows"""
    x = torch.from_numpy(np.random.default_rng(seed).uniform(0, 0.5, (1, *dims, C_)).astype(np.float32))
    t, h, w = (torch.arange(n) % kk == kk // 2 for n, kk in zip(dims, k))
    peak = (t.view(-1, 1, 1) & h.view(1, -1, 1) & w.view(1, 1, -1)).view(1, *dims, 1).expand_as(x)
    return q(torch.where(peak, torch.tensor(2.0), x), BF16), peak


EXACT = pytest.mark.parametrize("k,dims,npeaks,kind", [((3, 3, 3), (6, 9, 9), 18, "scatter"), ((3, 3, 3), (6, 9, 9), 18, "reg"),
                                                       ((3, 3, 3), (6, 9, 9), 18, "loop"), ((5, 5, 5), (5, 10, 10), 4, "scatter"),
                                                       ((5, 5, 5), (5, 10, 10), 4, "loop")],
                                 ids=["333-scatter", "333-reg", "333-loop", "555-scatter", "555-loop"])


@EXACT
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["pos", "neg"])
def test_fixed_point_exact_worst_case(ops, k, dims, npeaks, kind, sign, monkeypatch):
    """every covering window of a cell sends it the largest-mantissa gradient with the same sign: n * 1.9921875 * 2^E must not leave the
    int32 accumulator (n = 27: 2^30 headroom; n = 125 needs E = 23), and every addend is exact, so gin is bitwise bf16(n * 1.9921875)
    (249 for n = 125) at the peaks and exactly 0 elsewhere"""
    C_, n, s = 40, k[0] * k[1] * k[2], (1, 1, 1)
    x, peak = peaks_input(k, dims, C_, 81)
    assert int(peak[..., 0].sum()) == npeaks
    _, idx, ctx = ops.maxpool3d(dev(x, BF16), k, s)
    ref = Ref(x, k, s)
    assert torch.equal(idx.cpu(), ref.tap)
    assert torch.equal(ref.bwd(torch.ones_like(ref.out)), torch.where(peak, float(n), 0.0).double())
    if kind == "scatter":
        gout, wp, chscale = torch.full(tuple(ref.out.shape), sign * GMAX), None, torch.ones(C_)
    else:   # g = 128, 64, .., 1 in eight of the K rows, Wt = 2^-7 * 2^e(c) there: the product is +-255/128 * 2^e(c), exact
        K = 32
        gout = torch.zeros((*ref.out.shape[:4], K))
        gout[..., 3:11] = sign * 2.0 ** torch.arange(7, -1, -1)
        chscale = 2.0 ** torch.tensor([0, -1, -2, 3]).repeat(C_ // 4).float()
        wt = rnd((K, C_), 82)
        wt[3:11] = 2.0 ** -7 * chscale
        wp = ops.PoolGemmWeights(q(wt, BF16).numpy())
    gin = run_bwd(ops, ctx, kind, gout, monkeypatch, wp)
    want = (torch.where(peak, torch.tensor(float(n) * sign * GMAX).to(BF16).float(), torch.tensor(0.0)) * chscale).to(BF16)
    if n == 125:
        assert float(want.float().abs().max()) == 249.0 * float(chscale.max())
    got = gin.cpu()
    print(f"n={n} {kind}: got at a peak {float(got[0, k[0] // 2, k[1] // 2, k[2] // 2, 0])}, want {float(want[0, k[0] // 2, k[1] // 2, k[2] // 2, 0])}")
    assert torch.equal(got.float(), want.float())                 # (== : the sign of a zero is not pinned)
    assert torch.equal(bits(got)[peak], bits(want)[peak])


MIXED = pytest.mark.parametrize("k,dims,kind", [((3, 3, 3), (4, 9, 10), "scatter"), ((3, 3, 3), (4, 9, 10), "reg"), ((3, 3, 3), (4, 9, 10), "loop"),
                                                ((5, 5, 5), (5, 10, 10), "scatter"), ((5, 5, 5), (5, 10, 10), "loop")],
                                 ids=["333-scatter", "333-reg", "333-loop", "555-scatter", "555-loop"])


def mixed_case(ops, k, dims, kind, seed, C_=40, B=2):
    """post-ReLU input (ties, shared argmax cells), its context and reference, and for the fused kinds exact-product g / weights"""
    x = torch.relu(q(rnd((B, *dims, C_), seed), BF16))
    ref = Ref(x, k, (1, 1, 1))
    _, idx, ctx = ops.maxpool3d(dev(x, BF16), k, (1, 1, 1))
    assert torch.equal(idx.cpu(), ref.tap)
    if kind == "scatter":
        return ctx, ref, None, None
    g, wt = exact_gw((B, *dims), 32, C_, seed + 1)
    return ctx, ref, g, wt


@MIXED
def test_fixed_point_mixed_magnitudes(ops, k, dims, kind, monkeypatch):
    """gout = +-2^u, u uniform in [-20, 0]: the small gradients sit far below the workgroup's scale and must still arrive within the
    documented n * 2^-(E+1) * max|gout| (a scale of 2^16 instead of 2^24 loses them)"""
    ctx, ref, g, wt = mixed_case(ops, k, dims, kind, 85)
    if kind == "scatter":
        rng = np.random.default_rng(86)
        gout = torch.from_numpy((rng.choice([-1.0, 1.0], tuple(ref.out.shape)) * 2.0 ** rng.integers(-20, 1, tuple(ref.out.shape))).astype(np.float32))
        check_bwd(run_bwd(ops, ctx, kind, gout, monkeypatch), ref, gout, k, (1, 1, 1), BF16)
    else:   # rows scaled by 2^u: the products stay exact and span the same 20 octaves
        u = torch.from_numpy(np.random.default_rng(86).integers(-20, 1, (*ref.out.shape[:4], 1))).float()
        g = g * 2.0 ** u
        check_bwd(run_bwd(ops, ctx, kind, g, monkeypatch, ops.PoolGemmWeights(wt.numpy())), ref, g.double() @ wt.double(), k, (1, 1, 1), BF16, fused=True)


@pytest.mark.parametrize("kind", ["scatter", "reg", "loop"])
def test_fixed_point_scale_invariance(ops, kind, monkeypatch):
    """a power-of-two factor on the gradient only shifts the workgroup's exponent: bwd(gout * 2^e) is bitwise bwd(gout) * 2^e over the
    whole bf16 exponent range the clamps (26 / 254) leave; zero gradients give zeros; one non-zero element arrives alone and exact"""
    k, s = (3, 3, 3), (1, 1, 1)
    ctx, ref, g, wt = mixed_case(ops, k, (4, 9, 10), kind, 88)
    wp = None if kind == "scatter" else ops.PoolGemmWeights(wt.numpy())
    if kind == "scatter":   # bf16 magnitudes in [2^-6, 2), random sign
        rng = np.random.default_rng(89)
        shp = tuple(ref.out.shape)
        g = torch.from_numpy((rng.choice([-1.0, 1.0], shp) * (1 + rng.integers(0, 128, shp) / 128.0) * 2.0 ** rng.integers(-6, 1, shp)).astype(np.float32))
        assert torch.equal(q(g, BF16), g)
    r0 = run_bwd(ops, ctx, kind, g, monkeypatch, wp).float().cpu()
    assert float(r0.abs().max()) > 0
    for e in (-100, -40, 40, 100):
        ge = torch.ldexp(g, torch.tensor(e))
        assert torch.equal(q(ge, BF16), ge)
        re = run_bwd(ops, ctx, kind, ge, monkeypatch, wp).float().cpu()
        want = torch.ldexp(r0, torch.tensor(e))
        assert torch.equal(re, want), f"e={e}: {int((re != want).sum())} cells differ"
    assert bool((run_bwd(ops, ctx, kind, torch.zeros_like(g), monkeypatch, wp).float() == 0).all())
    # a single non-zero element: it (for the fused kinds its product row 3 * Wt[7, :], +-3 * 2^j) arrives unrounded, everything else is 0
    one = torch.zeros_like(g)
    if kind == "scatter":
        one[1, 2, 4, 5, 13] = -1.2578125
        want = ref.bwd(one)
    else:
        one[1, 2, 4, 5, 7] = 3.0
        want = ref.bwd(one.double() @ wt.double())
        assert torch.equal(want.to(BF16).double(), want)
    assert float(want.abs().max()) > 0
    assert torch.equal(run_bwd(ops, ctx, kind, one, monkeypatch, wp).float().cpu().double(), want)


# ---- G: relu_input through the fused backward ------------------------------------------------------------------------------------------

@FORMS
def test_relu_input_fused(ops, form, monkeypatch):
    """ctx recorded with relu_input (255 = "no cell" where the window maximum is <= 0): the fused backward equals, bit for bit, the one
    without relu_input masked by x > 0 -- 255 must be dropped by the register form's 27-bit mask as by the loop form's decode"""
    set_form(monkeypatch, form)
    k, s, B, dims, C_, K = (3, 3, 3), (1, 1, 1), 2, (4, 7, 9), 40, 64
    x = torch.relu(q(rnd((B, *dims, C_), 91) - 1.5, BF16))
    ref = Ref(x, k, s, relu_input=True)
    assert float((ref.tap == 255).double().mean()) > 0.05           # many all-zero windows
    _, idx, ctx = ops.maxpool3d(dev(x, BF16), k, s)
    _, idx_r, ctx_r = ops.maxpool3d(dev(x, BF16), k, s, relu_input=True)
    assert torch.equal(idx_r.cpu(), ref.tap)
    g, wt = exact_gw((B, *dims), K, C_, 92)
    wp = ops.PoolGemmWeights(wt.numpy())
    plain = ops.maxpool3d_bwd_gemm(ctx, dev(g, BF16), wp).cpu()
    got = ops.maxpool3d_bwd_gemm(ctx_r, dev(g, BF16), wp).cpu()
    assert torch.equal(got.float(), torch.where(x > 0, plain.float(), torch.tensor(0.0)))
    assert torch.equal(bits(got)[x > 0], bits(plain)[x > 0])
    check_bwd(got, Ref(x, k, s), g.double() @ wt.double(), k, s, BF16, mask=x, fused=True)


# ---- H: explicit pad-before (the C ABI accepts any pad below the window; SAME gives 1 for 3x3x3 / 1) --------------------------------------

PADS = [(0, 0, 0), (2, 2, 2), (0, 2, 1)]


@functools.lru_cache(maxsize=None)
def pad_case(pad, dtype, kind):
    """as case(): 3x3x3 / 1 over B = 2, (3, 7, 9), C = 24 (a slab tail) with the reference at pad-before `pad` (read-only)"""
    x = make_input(kind, (2, 3, 7, 9, 24), dtype, 120 + PADS.index(pad))
    return x, Ref(x, (3, 3, 3), (1, 1, 1), relu_input=kind == "relu_input", pad_before=pad)


@DTYPES
@pytest.mark.parametrize("pad", PADS, ids=lambda p: "pad" + "".join(map(str, p)))
@pytest.mark.parametrize("kind", ["signed", "relu_input"])
def test_explicit_pad_before(ops, pad, dtype, kind):
    """flk_maxpool3d_fwd / _bwd called with a pad-before no wrapper computes (To, Ho, Wo = Ti, Hi, Wi): the LDS-tiled forward of both
    dtypes and the fp32 tiled backward at a window origin other than i - 1, the bf16 scatter backward at the same pads.  Neither data
    kind holds a -0.0, so out and idx are bit for bit the reference's under either tie rule."""
    k, s = (3, 3, 3), (1, 1, 1)
    x, ref = pad_case(pad, dtype, kind)
    xd = dev(x, dtype)
    out = torch.empty_like(xd)
    idx = torch.empty(tuple(xd.shape), dtype=torch.uint8, device="cuda")
    a = ops._pool_args(xd, 24, k, s, pad, out, idx)
    a.relu_input = int(kind == "relu_input")
    ops.check(ops.load().flk_maxpool3d_fwd(ctypes.byref(a), ops.dtype_code(dtype), ops.stream_ptr()))
    check_fwd(out, idx, ref)
    ctx = (xd, 24, k, s, pad, out, idx, 0, 0)                       # maxpool3d's context: _pool_args + load().flk_maxpool3d_bwd
    g = q(rnd(tuple(ref.out.shape), 9), dtype)
    check_bwd(ops.maxpool3d_bwd(ctx, dev(g, dtype)), ref, g, k, s, dtype)
    check_bwd(ops.maxpool3d_bwd(ctx, dev(g, dtype), mask=xd), ref, g, k, s, dtype, mask=x)
