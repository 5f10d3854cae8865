"""The classifier head (flk_head_forward / flk_head_backward, include/flicker_hip.h) on a machine without a GPU:
  * oracle/head_ref.py IS the operation: its float64 sums against torch's own avg_pool3d -> 1x1x1 convolution -> mean over T' (I3D
    Logits, i3d.py:459-474) and AdaptiveAvgPool3d(1) + Linear (VideoResNet), and its gradient against torch.autograd times the ReLU mask;
  * every refusal of the two entry points: FLK_EINVAL with a message naming the argument, before any GPU call.  Fake pointers, as in
    tests/test_perturb_contract_cpu.py: each call is valid in everything but the one argument under test and NO call here passes a fully
    valid argument set -- nothing is ever launched;
  * the exact data of tests/test_head_edges_gpu.py is exact: on every case every sum the kernels form is computed in float32 in ascending
    and in descending order and equals the float64 value bit for bit, and the reason it must (all terms multiples of one grain, the sum
    of their magnitudes below 2^24 grains, so every partial sum in ANY order is representable) is asserted as well.  The GPU test's zero
    tolerance then rests on the reference alone."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as hc
from oracle import head_ref

GOOD = 0x10000            # 16-byte aligned, never dereferenced
EINVAL = -1
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- the oracle is the operation ---------------------------------------------------------------------------------------------------------
def rnd64(*shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))


def channels_last(x):
    """[B,C,Tn,H,W] -> the head's [B,Tn,HW,C]"""
    B, Cn, Tn, H, W = x.shape
    return x.permute(0, 2, 3, 4, 1).reshape(B, Tn, H * W, Cn)


def i3d_logits_torch(x, W, bias):
    p = F.avg_pool3d(x, (2, 7, 7), stride=1)
    z = F.conv3d(p, W.t().reshape(W.shape[1], W.shape[0], 1, 1, 1), bias)
    return z.squeeze(4).squeeze(3).mean(dim=2)


def vrn_logits_torch(x, W, bias):
    return F.linear(torch.nn.AdaptiveAvgPool3d(1)(x).flatten(1), W.t(), bias)


def check_against_torch(x, wt, W, bias, dl, logits_torch):
    x = x.clone().requires_grad_(True)
    want = logits_torch(x, W, bias)
    (gx,) = torch.autograd.grad(want, x, grad_outputs=dl)
    y = channels_last(x.detach())
    feat, logits, feat_mag, logits_mag = head_ref.head_forward_ref(y, wt, W, bias)
    assert logits.dtype == F64 and feat.dtype == F64
    assert torch.allclose(logits, want, rtol=1e-12, atol=1e-12 * float(logits_mag.max()))
    assert (feat.abs() <= feat_mag * (1 + 1e-12)).all() and (logits.abs() <= logits_mag * (1 + 1e-12)).all()
    for use_mask in (False, True):
        dfeat, gy, dfeat_mag = head_ref.head_backward_ref(y, wt, W, dl, use_mask)
        g_want = channels_last(gx * (x.detach() > 0) if use_mask else gx)
        assert gy.dtype == F64 and torch.allclose(gy, g_want, rtol=1e-12, atol=1e-12 * float(g_want.abs().max()))
        assert (dfeat.abs() <= dfeat_mag * (1 + 1e-12)).all()


@pytest.mark.parametrize("Tn", [2, 3, 8])
def test_oracle_is_the_i3d_logits_endpoint(Tn):
    B, Cn, N = 2, 24, 7
    wt = head_ref.i3d_time_weights(Tn)
    assert abs(float(wt.sum()) * 49 - 1) < 1e-15
    check_against_torch(rnd64(B, Cn, Tn, 7, 7, seed=Tn), wt, rnd64(Cn, N, seed=10 + Tn), rnd64(N, seed=20 + Tn), rnd64(B, N, seed=30 + Tn),
                        i3d_logits_torch)


@pytest.mark.parametrize("Tn,H,W_", [(1, 7, 7), (2, 7, 7), (4, 14, 14), (3, 5, 2)])
def test_oracle_is_the_videoresnet_head(Tn, H, W_):
    B, Cn, N = 2, 24, 7
    check_against_torch(rnd64(B, Cn, Tn, H, W_, seed=Tn), head_ref.videoresnet_time_weights(Tn, H * W_), rnd64(Cn, N, seed=11 + Tn),
                        rnd64(N, seed=21 + Tn), rnd64(B, N, seed=31 + Tn), vrn_logits_torch)


def test_i3d_time_weights_are_the_plan_s():
    """the plan's own fp32 weights (csrc/net.cpp: (float)cover / (2 * 49 * T') in float) are these rounded to fp32 once"""
    for Tn in (2, 3, 8, 9, 16):
        w = head_ref.i3d_time_weights(Tn)
        cover = [1] + [2] * (Tn - 2) + [1]
        want = np.array(cover, np.float32) / (np.float32(2.0) * np.float32(49.0) * np.float32(Tn - 1))
        assert want.dtype == np.float32 and np.array_equal(w.to(torch.float32).numpy(), want)
    with pytest.raises(ValueError):
        head_ref.i3d_time_weights(1)


def test_oracle_mask_is_a_comparison():
    """-0.0, +0.0, negatives and NaN give zero; the smallest denormal and +inf pass, and inf multiplies nothing"""
    vals = [0.0, -0.0, -1.0, float("nan"), float("-inf"), 5e-324, float("inf"), 2.0]
    y = torch.tensor(vals, dtype=F64).view(1, 1, len(vals), 1)
    wt, W, dl = torch.tensor([0.5]), torch.tensor([[3.0]]), torch.tensor([[2.0]])
    dfeat, gy, _ = head_ref.head_backward_ref(y, wt, W, dl, True)
    assert dfeat.item() == 6.0 and gy.flatten().tolist() == [0, 0, 0, 0, 0, 3.0, 3.0, 3.0]
    assert head_ref.head_backward_ref(y, wt, W, dl, False)[1].flatten().tolist() == [3.0] * len(vals)


# ---- every refusal -----------------------------------------------------------------------------------------------------------------------
def refused(lib, rc, *words):
    msg = lib.flk_last_error().decode()
    assert rc == EINVAL, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def fwd(lib, *, y=GOOD, ld=None, coff=0, Cn=64, B=2, Tn=2, HW=3, wt=GOOD, W=GOOD, bias=GOOD, N=5, feat=GOOD, logits=GOOD, dtype=0):
    ld = Cn + coff if ld is None else ld
    return lib.flk_head_forward(C.c_void_p(y), ld, coff, Cn, B, Tn, HW, C.c_void_p(wt), C.c_void_p(W), C.c_void_p(bias), N, C.c_void_p(feat),
                                C.c_void_p(logits), dtype, None)


def bwd(lib, *, y=GOOD, ld=None, coff=0, gy=GOOD, gld=None, gcoff=0, Cn=64, B=2, Tn=2, HW=3, wt=GOOD, W=GOOD, N=5, dlogits=GOOD, dfeat=GOOD,
        use_mask=1, dtype=0):
    ld = Cn + coff if ld is None else ld
    gld = Cn + gcoff if gld is None else gld
    return lib.flk_head_backward(C.c_void_p(y), ld, coff, C.c_void_p(gy), gld, gcoff, Cn, B, Tn, HW, C.c_void_p(wt), C.c_void_p(W), N,
                                 C.c_void_p(dlogits), C.c_void_p(dfeat), use_mask, dtype, None)


def test_null_arguments_are_refused(lib):
    for name in ("y", "wt", "W", "feat", "logits"):            # bias may be null: no bias
        refused(lib, fwd(lib, **{name: 0}), "flk_head_forward", "null")
    for name in ("y", "gy", "wt", "W", "dlogits", "dfeat"):    # y may be null only without the mask
        refused(lib, bwd(lib, **{name: 0}), "flk_head_backward", "null")


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_extents_are_refused_by_name(lib, dtype):
    for call, what in ((fwd, "flk_head_forward"), (bwd, "flk_head_backward")):
        for name in ("B", "Tn", "HW", "N"):
            for bad in (0, -1):
                refused(lib, call(lib, dtype=dtype, **{name: bad}), what, f"{name} must be >= 1", str(bad))
        for bad in (0, -8):
            refused(lib, call(lib, dtype=dtype, Cn=bad, ld=64), what, "C must be >= 1", str(bad))
        refused(lib, call(lib, dtype=dtype, N=1025), what, "N must be <= 1024", "1025")
        refused(lib, call(lib, dtype=dtype, B=65536), what, "B must be <= 65535", "65536")
        refused(lib, call(lib, dtype=dtype, Tn=1 << 16, HW=1 << 15), what, "Tn * HW", str(1 << 31))
        refused(lib, call(lib, dtype=dtype, Cn=64, coff=8, ld=64), what, "ld = 64", "coff")
        refused(lib, call(lib, dtype=dtype, Cn=64, coff=-8, ld=64), what, "ld = 64", "-8")
        refused(lib, call(lib, dtype=7), what, "dtype", "7")
    refused(lib, fwd(lib, dtype=dtype, Cn=2049), "flk_head_forward", "C must be <= 2048", "2049")
    refused(lib, fwd(lib, dtype=dtype, Cn=2056), "flk_head_forward", "C must be <= 2048", "2056")
    refused(lib, bwd(lib, dtype=dtype, Cn=64, gcoff=16, gld=72), "flk_head_backward", "gld = 72", "gcoff")


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_backward_refuses_what_is_no_multiple_of_the_16_byte_group(lib, dtype):
    e = 8 if dtype else 4
    h = e // 2
    mult = f"must be a multiple of {e}"
    refused(lib, bwd(lib, dtype=dtype, Cn=64 + h), f"C = {64 + h}", mult)
    refused(lib, bwd(lib, dtype=dtype, Cn=h), f"C = {h}", mult)
    refused(lib, bwd(lib, dtype=dtype, ld=64 + h), f"ld = {64 + h}", mult)
    refused(lib, bwd(lib, dtype=dtype, coff=h, ld=64 + e), f"coff = {h}", mult)
    refused(lib, bwd(lib, dtype=dtype, gld=64 + h), f"gld = {64 + h}", mult)
    refused(lib, bwd(lib, dtype=dtype, gcoff=h, gld=64 + e), f"gcoff = {h}", mult)
    if dtype:                                      # multiples of 4 that fp32 takes are refused in bf16
        for kw in (dict(Cn=68), dict(ld=68), dict(coff=4, ld=72), dict(gld=68), dict(gcoff=4, gld=72)):
            refused(lib, bwd(lib, dtype=1, **kw), mult)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_backward_refuses_misaligned_pointers(lib, dtype):
    for off in (2, 4, 8, 12):
        refused(lib, bwd(lib, dtype=dtype, y=GOOD + off), "y = ", "16-byte aligned", "use_mask")
        refused(lib, bwd(lib, dtype=dtype, gy=GOOD + off), "gy = ", "16-byte aligned")
        refused(lib, bwd(lib, dtype=dtype, gy=GOOD + off, use_mask=0), "gy = ", "16-byte aligned")


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_backward_refuses_a_group_count_past_31_bits(lib, dtype):
    e = 8 if dtype else 4
    B, Tn, HW, Cn = 64, 256, 256, 512 * e              # 2^22 positions x 512 groups = 2^31
    refused(lib, bwd(lib, dtype=dtype, B=B, Tn=Tn, HW=HW, Cn=Cn), "overflow", str(1 << 31))
    refused(lib, bwd(lib, dtype=dtype, B=B + 1, Tn=Tn, HW=HW, Cn=Cn), "overflow", str((B + 1) * Tn * HW * 512))


# ---- the exact data is exact -------------------------------------------------------------------------------------------------------------
EXACT_CASES = (hc.SMALL_CASES + [hc.BIAS_NONE_CASE, hc.SLICE_CASE, hc.MASK_CASE] + hc.GRID_CASES[hc.F32] + hc.GRID_CASES[hc.BF16])


def seq_sum(term, n, start=None):
    """float32 recursive sums of term(0) .. term(n-1), ascending and descending; start: the fp32 value the sum begins from (added FIRST
    ascending, LAST descending)"""
    zero = np.zeros_like(term(0), dtype=np.float32)
    up = zero.copy() if start is None else start.astype(np.float32).copy()
    for i in range(n):
        up = up + term(i)
    down = zero.copy()
    for i in reversed(range(n)):
        down = down + term(i)
    if start is not None:
        down = down + start.astype(np.float32)
    assert up.dtype == np.float32 and down.dtype == np.float32
    return up, down


def same_bits(got32, want64):
    """the float32 array, converted, IS the float64 one (numbers compared; the sign of a zero is not a number)"""
    return np.array_equal(got32.astype(np.float64), want64.numpy())


@pytest.mark.parametrize("case", EXACT_CASES, ids=hc.case_id)
def test_exact_data_is_exact_in_any_order(case):
    B, Tn, HW, Cn, N = case
    d = hc.exact_data(case)
    y, wt, W, bias, dl = d["y"], d["wt"], d["W"], d["bias"], d["dlogits"]
    assert torch.equal(y.to(torch.bfloat16).float(), y)                         # bf16 storage changes nothing
    assert (y == 0).any() and (torch.signbit(y) & (y == 0)).any() and (y < 0).any() and (y > 0).any()
    assert len(set(wt[:8].tolist())) == min(Tn, 8)
    feat, logits, feat_mag, logits_mag = head_ref.head_forward_ref(y, wt, W, bias)
    dfeat, gy, dfeat_mag = head_ref.head_backward_ref(y, wt, W, dl, True)
    # why it is exact: every term is a whole number of grains and the magnitudes sum to fewer than 2^24 of them
    grain = hc.FEAT_GRAIN
    for v in (wt.double().view(1, Tn, 1, 1) * y.double() / grain, feat / grain, logits / grain, dfeat, gy / grain):
        assert torch.equal(v, v.round())
    assert float(feat_mag.max()) / grain < 2 ** 24 and float(logits_mag.max()) / grain < 2 ** 24 and float(dfeat_mag.max()) < 2 ** 24
    # and it is: float32 sums in two orders
    yn, wn, Wn, bn, dn = (t.numpy() for t in (y.reshape(B, Tn * HW, Cn), wt, W, bias, dl))
    for got in seq_sum(lambda i: wn[i // HW] * yn[:, i, :], Tn * HW):
        assert same_bits(got, feat)
    f32 = feat.to(torch.float32).numpy()
    for got in seq_sum(lambda c: f32[:, c, None] * Wn[None, c, :], Cn, start=np.broadcast_to(bn, (B, N))):
        assert same_bits(got, logits)
    for got in seq_sum(lambda n: dn[:, n, None] * Wn[None, :, n], N):
        assert same_bits(got, dfeat)
    g32 = wn[None, :, None, None] * dfeat.to(torch.float32).numpy()[:, None, None, :]
    assert g32.dtype == np.float32
    assert same_bits(np.where(y.numpy() > 0, np.broadcast_to(g32, y.shape), np.float32(0)), gy)
