"""oracle/perturb_ref.py (the bit-faithful numpy restatement the GPU edge tests compare the kernels with) against the mathematics it
restates: oracle/attack_math.py's tf_apply / torch_apply and autograd through them.  Small shapes, no GPU: flicker, dense and per-clip
perturbations, cyclic shifts, both dialects, uint8 (scalar decode and table) and fp32 clips.

TF dialect: inv_std = 1, so both sides do the same float32 operations per element and the applied clip is EQUAL; with an integer clip
gradient the delta-gradient is a sum of integers below 2^24 on both sides and EQUAL too.  torch dialect: attack_math divides by std where
the kernels (and perturb_ref) multiply by float32(1/std) -- one rounding apart, so 1e-6 there (the tolerance of
test_apply_and_grad_torch_dialect_golden)."""
import numpy as np
import pytest
import torch

from oracle import attack_math as am
from oracle import perturb_ref as pr

B, T, H, W = 2, 6, 4, 6


def clip_u8(seed):
    return np.random.default_rng(seed).integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)


def int_grad(seed, shape=(B, T, H, W, 3)):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float32)


def make_delta(seed, shape):
    return np.random.default_rng(seed).uniform(-0.6, 0.6, shape).astype(np.float32)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32in"])
@pytest.mark.parametrize("dense", [False, True], ids=["flicker", "dense"])
@pytest.mark.parametrize("shifts", [(0, 0), (3, 5), (-2, T + 1)], ids=["plain", "cyclic", "cyclic-neg"])
def test_tf_dialect_equals_attack_math(u8, dense, shifts):
    xu = clip_u8(1)
    x = xu.astype(np.float32) / np.float32(128) - np.float32(1) if u8 else np.random.default_rng(2).uniform(-1, 1, xu.shape).astype(np.float32)
    d = make_delta(3, (T, H, W, 3) if dense else (T, 3))
    sx, sp = shifts
    kw = dict(dclip=0.0 if dense else 0.4, shift_x=sx, shift_p=sp)
    dt = torch.from_numpy(d.reshape(T, H, W, 3) if dense else d.reshape(T, 1, 1, 3)).requires_grad_(True)
    xa = am.tf_apply(torch.from_numpy(x), dt, 1.0, sx, float(sx != 0), sp, float(sp != 0), clip_delta=not dense)
    got = pr.apply_ref(xu if u8 else x, d, **kw)
    assert got.dtype == np.float32 and np.array_equal(got, xa.detach().numpy())
    g = int_grad(4)
    (gref,) = torch.autograd.grad(xa, dt, torch.from_numpy(g), retain_graph=True)
    gd = pr.delta_grad_ref(xu if u8 else x, d, g, **kw)
    assert gd.dtype == np.float32 and gd.shape == d.shape
    assert np.array_equal(gd, gref.numpy().reshape(d.shape))
    # the case says something: the clamp is active and inactive, delta rows beyond the bound exist and carry no gradient
    share = pr.pass_mask(xu if u8 else x, d, **kw).mean()
    assert 0.3 < share < 0.98
    if not dense:
        beyond = np.abs(d) > np.float32(0.4)
        assert beyond.any() and not gd[beyond].any() and gd[~beyond].any()
    # a float gradient goes through float64 sums: autograd's float32 sums agree to their own rounding
    gf = np.random.default_rng(5).standard_normal(g.shape).astype(np.float32)
    (gref,) = torch.autograd.grad(xa, dt, torch.from_numpy(gf))
    np.testing.assert_allclose(pr.delta_grad_ref(xu if u8 else x, d, gf, **kw), gref.numpy().reshape(d.shape), rtol=1e-5, atol=1e-5)


def test_adv_flag_zero_and_scaled():
    xu, d = clip_u8(1), make_delta(3, (T, 3))
    clean = pr.apply_ref(xu, d, adv_flag=0.0, shift_x=2)
    assert np.array_equal(clean, np.roll(xu.astype(np.float32) / 128 - 1, 2, axis=1))
    x = torch.from_numpy(xu).float() / 128 - 1
    dt = torch.from_numpy(d.reshape(T, 1, 1, 3)).requires_grad_(True)
    xa = am.tf_apply(x, dt, 0.5)
    np.testing.assert_allclose(pr.apply_ref(xu, d, adv_flag=0.5), xa.detach().numpy(), rtol=0, atol=1e-7)
    g = int_grad(4)
    (gref,) = torch.autograd.grad(xa, dt, torch.from_numpy(g))
    np.testing.assert_allclose(pr.delta_grad_ref(xu, d, g, adv_flag=0.5), gref.numpy().reshape(T, 3), rtol=1e-6, atol=0)


def test_per_clip_is_each_clip_alone():
    xu = clip_u8(6)
    d = make_delta(7, (B, T, 3))
    g = int_grad(8)
    got, gd = pr.apply_ref(xu, d), pr.delta_grad_ref(xu, d, g)
    assert gd.shape == (B, T, 3)
    for b in range(B):
        dt = torch.from_numpy(d[b].reshape(T, 1, 1, 3)).requires_grad_(True)
        xa = am.tf_apply(torch.from_numpy(xu[b:b + 1]).float() / 128 - 1, dt)
        assert np.array_equal(got[b:b + 1], xa.detach().numpy())
        (gref,) = torch.autograd.grad(xa, dt, torch.from_numpy(g[b:b + 1]))
        assert np.array_equal(gd[b], gref.numpy().reshape(T, 3))
    # one clamp bound per clip
    bounds = np.array([0.2, 0.5], np.float32)
    got, gd = pr.apply_ref(xu, d, dclip_dev=bounds), pr.delta_grad_ref(xu, d, g, dclip_dev=bounds)
    for b in range(B):
        assert np.array_equal(got[b:b + 1], pr.apply_ref(xu[b:b + 1], d[b], dclip=float(bounds[b])))
        assert np.array_equal(gd[b], pr.delta_grad_ref(xu[b:b + 1], d[b], g[b:b + 1], dclip=float(bounds[b])))
        assert (np.abs(d[b]) > bounds[b]).any() and not gd[b][np.abs(d[b]) > bounds[b]].any()


@pytest.mark.parametrize("src", ["f32in", "u8-table"])
@pytest.mark.parametrize("dense", [False, True], ids=["flicker", "dense"])
@pytest.mark.parametrize("shift", [0, 4])
def test_torch_dialect_vs_attack_math(src, dense, shift):
    """Perturbation.forward (model.py:80-101): delta / std, scalar bounds, the perturbation alone is rolled"""
    from flickering_adversarial_video_amd.videoresnet_spec import u8_decode_table
    xu = clip_u8(9)
    lut = u8_decode_table()
    x = lut[xu, np.arange(3)] if src == "u8-table" else np.random.default_rng(10).uniform(-2, 2.6, xu.shape).astype(np.float32)
    dyn = 0.2
    d = (make_delta(11, (T, H, W, 3) if dense else (T, 3)) * 0.5).astype(np.float32)          # U(-0.3, 0.3) against 0.2
    kw = dict(dclip=dyn, inv_std=tuple(1.0 / s for s in am.DEFAULT_STD), lo=am.TORCH_MIN_VALUE, hi=am.TORCH_MAX_VALUE, shift_p=shift)
    clip = xu if src == "u8-table" else x
    if src == "u8-table":
        kw["x_lut"] = lut
    d64 = torch.from_numpy(d.reshape(T, H, W, 3) if dense else d.reshape(T, 1, 1, 3)).double().permute(3, 0, 1, 2).contiguous().requires_grad_(True)
    xa = am.torch_apply(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), d64, dyn, True, shift, shift != 0)
    got = pr.apply_ref(clip, d, **kw)
    np.testing.assert_allclose(got, xa.detach().permute(0, 2, 3, 4, 1).numpy(), rtol=1e-6, atol=1e-6)
    g = int_grad(12)
    (gref,) = torch.autograd.grad(xa, d64, torch.from_numpy(g).double().permute(0, 4, 1, 2, 3))
    gd = pr.delta_grad_ref(clip, d, g, **kw)
    np.testing.assert_allclose(gd, gref.permute(1, 2, 3, 0).numpy().reshape(d.shape), rtol=1e-6, atol=0)
    assert 0.3 < pr.pass_mask(clip, d, **kw).mean() < 0.98 and (np.abs(d) > dyn).any() and not gd[np.abs(d) > dyn].any()


def test_decode_forms():
    xu = clip_u8(13)
    assert np.array_equal(pr.decode(xu), xu.astype(np.float32) / 128 - 1)
    lut = np.random.default_rng(14).standard_normal((256, 3)).astype(np.float32)
    dec = pr.decode(xu, x_lut=lut)
    for c in range(3):
        assert np.array_equal(dec[..., c], lut[xu[..., c], c])
    xf = dec.copy()
    assert pr.decode(xf) is xf
