"""Strided convolutions and their data-gradients at odd extents (GPU): the four strided geometries of the VideoResNet plans with
torch's symmetric padding -- 3x3x3 / 2, (1,3,3) / (1,2,2), (3,1,1) / (2,1,1) and the 1x1x1 strided downsample -- at kernel level,
and whole plans at clip sizes whose strided layers see odd extents, unequal class grids and empty classes.

Kernel level: forward against torch-CPU ``F.conv3d(stride, padding)``; the data-gradient as the plan runs it -- one stride-1
``flk_conv3d`` per parity class (oracle/strided_dgrad.py, shown equal to autograd in tests/test_conv_strided_cpu.py) over a 1- or
2-tap box, writing the sub-lattice o * stride + class of ONE shared gradient buffer through out_stride / out_offset -- against torch
autograd.  Inputs and weights are pre-rounded to the storage dtype and the tolerances are those of tests/test_kernels_gpu.py
(``tol``; twice that where a row_scale is folded into the weights, as in its test_conv_data_gradient).

Whole plans: tests/test_videoresnet_gpu.py bounds a backward link for all but a counted fraction of its elements, because two
implementations decide some ReLUs differently; at tiny extents one flipped unit is percent of a tensor.  Here the weights are
settled on the clip (oracle/fixtures.py::settled_videoresnet_weights: no ReLU input within 0.04 of its tensor's maximum of zero), so
every element of every endpoint and gradient buffer is bounded."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures, strided_dgrad

pytestmark = pytest.mark.gpu


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


# The smallest extents at which each edge exists.  232 = r2plus1d's 230 mid-planes padded to 8: a partial 16-channel output fragment
# forward and a partial K slab in the data-gradient (B), the reverse in C.
GEO = {
    "A": ((3, 3, 3), (2, 2, 2), (1, 1, 1), 64, 128),
    "B": ((1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 232),
    "C": ((3, 1, 1), (2, 1, 1), (1, 0, 0), 232, 128),
    "D222": ((1, 1, 1), (2, 2, 2), (0, 0, 0), 64, 128),
    "D122": ((1, 1, 1), (1, 2, 2), (0, 0, 0), 64, 128),
}
EXT = {
    "A": [(5, 9, 7),      # all odd: the eight classes have unequal grids
          (4, 8, 6),      # even: the classes read past the end of G
          (1, 5, 3)],     # T = 1 leaves the odd-t classes empty
    "B": [(3, 9, 7), (2, 8, 6)],
    "C": [(5, 5, 3), (4, 4, 4), (1, 3, 3)],
    "D222": [(5, 9, 7), (4, 8, 6)],
    "D122": [(5, 9, 7), (4, 8, 6)],
}
# (geometry, extents, B, nf): B = 2 on the first extent of each geometry; nf = 4 everywhere, A also with 32- and 128-channel tiles
CASES = [(g, d, 2 if i == 0 else 1, nf) for g in GEO for i, d in enumerate(EXT[g]) for nf in ((4, 2, 8) if g == "A" else (4,))]
CASE_IDS = [f"{g}_{'x'.join(map(str, d))}_B{B}_nf{nf}" for g, d, B, nf in CASES]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
EACH_CASE = pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
SENTINEL = 7.0      # exactly representable in bf16


@DTYPES
@EACH_CASE
def test_strided_forward(ops, case, dtype):
    """the strided convolution with torch's symmetric padding and the epilogue of a block's last unit: relu(conv * scale + bias + add)"""
    geo, dims, B, nf = case
    k, s, pad, cin, cout = GEO[geo]
    og = strided_dgrad.out_dims(k, s, pad, dims)
    x = q(rnd((B, *dims, cin), 1), dtype)
    w = q(rnd((*k, cin, cout), 2, (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5), dtype)
    scale, bias = rnd((cout,), 3).abs() + 0.5, rnd((cout,), 4) * 0.1
    add = q(rnd((B, *og, cout), 5), dtype)
    conv = F.conv3d(cf(x), w.permute(4, 3, 0, 1, 2).contiguous(), None, s, pad)
    ref = torch.relu(cl(conv) * scale + bias + add)
    pw = ops.ConvWeights(w.numpy(), dtype, nf)
    out = ops.conv3d(x.to(dtype).cuda(), pw, stride=s, pad=pad, out_grid=og, scale=scale.cuda(), bias=bias.cuda(), add=add.to(dtype).cuda(), relu=True)
    assert tuple(out.shape) == tuple(ref.shape)
    r, a = tol(dtype, ref)
    err = float((out.float().cpu() - ref).abs().max() / ref.abs().max())
    print(f"[{geo} {dims} B{B} nf{nf} {dtype}] forward: max err {err:.2e} of the maximum")
    torch.testing.assert_close(out.float().cpu(), ref, rtol=r, atol=a)


@functools.lru_cache(maxsize=None)
def dgrad_case(case, dtype):
    """one data-gradient case: output gradient g, BN scale, the class operators and torch autograd's gradient (computed once)"""
    geo, dims, B, nf = case
    k, s, pad, cin, cout = GEO[geo]
    og = strided_dgrad.out_dims(k, s, pad, dims)
    w = q(rnd((*k, cin, cout), 11, 0.05), dtype)
    a_scale = rnd((cout,), 12).abs() + 0.5
    g = q(rnd((B, *og, cout), 13), dtype)
    x = torch.zeros((B, cin, *dims), requires_grad=True)
    y = F.conv3d(x, w.permute(4, 3, 0, 1, 2).contiguous(), None, s, pad) * a_scale.view(1, -1, 1, 1, 1)
    (gx_ref,) = torch.autograd.grad(y, x, cf(g))
    classes = strided_dgrad.classes(k, s, pad, dims, w.numpy())
    owned = torch.zeros(dims, dtype=torch.bool)
    for c in classes:
        o = c["offset"]
        owned[o[0]::s[0], o[1]::s[1], o[2]::s[2]] = True
    return dict(g=g, a_scale=a_scale, classes=classes, gx_ref=cl(gx_ref), owned=owned, s=s, cin=cin, cout=cout, dims=dims, B=B, nf=nf)


def run_classes(ops, c, dtype, gdev, weights, out, **kw):
    """the plan's launch list: one stride-1 flk_conv3d per class into the shared buffer `out`"""
    for cls, pw in zip(c["classes"], weights):
        ops.conv3d(gdev, pw, pad=cls["pad"], out_grid=cls["grid"], out_stride=c["s"], out_offset=cls["offset"], out=out, **kw)
    torch.cuda.synchronize()
    return out


def class_weights(ops, c, dtype):
    return [ops.ConvWeights(cls["w"], dtype, c["nf"], row_scale=c["a_scale"].numpy(), transpose=False) for cls in c["classes"]]


@DTYPES
@EACH_CASE
def test_strided_data_gradient(ops, case, dtype):
    """the classes' union == autograd.grad(conv * a_scale) (BN scale folded through row_scale) in a slice of a wider buffer; every
    channel outside the slice and every cell no class owns (the downsample: `downsample/zero`'s memset owns those) keeps the
    sentinel bit for bit; the same launch list twice gives the same bits; and no class is ever split over K -- a split launch's
    workspace is indexed by PHYSICAL output cells (the header's "logical == physical output grid" condition)"""
    from flickering_adversarial_video_amd._lib import load
    c = dgrad_case(case, dtype)
    cin, coff, ld = c["cin"], 8, c["cin"] + 24
    gdev = c["g"].to(dtype).cuda()
    weights = class_weights(ops, c, dtype)
    fresh = lambda: torch.full((c["B"], *c["dims"], ld), SENTINEL, dtype=dtype, device="cuda")
    out = run_classes(ops, c, dtype, gdev, weights, fresh(), out_coff=coff)
    o = out.float().cpu()
    owned, ref = c["owned"], c["gx_ref"]
    assert bool(owned.all()) == (case[0][0] != "D")
    r, a = tol(dtype, ref)
    got = o[..., coff:coff + cin]
    err = float((got[:, owned] - ref[:, owned]).abs().max() / ref.abs().max())
    print(f"[{case} {dtype}] data-gradient over {len(weights)} classes: max err {err:.2e} of the maximum")
    # bf16: a * W is rounded once more when folded
    torch.testing.assert_close(got[:, owned], ref[:, owned], rtol=r * 2, atol=a * 2)
    assert bool((o[..., :coff] == SENTINEL).all()) and bool((o[..., coff + cin:] == SENTINEL).all())
    assert bool((o[:, ~owned] == SENTINEL).all())
    assert bool((ref[:, ~owned] == 0).all())                 # ... and the gradient there is zero: what the memset writes
    # determinism: the same launch list again gives the same bits
    assert torch.equal(out, run_classes(ops, c, dtype, gdev, weights, fresh(), out_coff=coff)), "second run differs"
    # a split-K request changes nothing: no workspace is planned, and the launches give the same bits again
    assert torch.equal(out, run_classes(ops, c, dtype, gdev, weights, fresh(), out_coff=coff, splitk=True)), "splitk=True run differs"
    for cls, pw in zip(c["classes"], weights):
        args, _ = ops.conv3d_args(gdev, pw, pad=cls["pad"], out_grid=cls["grid"], out_stride=c["s"], out_offset=cls["offset"], out=out,
                                  out_coff=coff, splitk=True)
        assert max(c["s"]) > 1 and load().flk_conv_splitk_bytes(C.byref(args), pw.handle) == 0 and args.splitk_ws_bytes == 0


@DTYPES
@EACH_CASE
def test_strided_data_gradient_epilogue(ops, case, dtype):
    """the epilogue as emit_gen_bwd uses it on a block's first unit: the output slice holds the shortcut gradient S and is passed as
    `add` too (accumulation in place), with the ReLU mask of the block's input: where(mask > 0, gx + S, 0)"""
    c = dgrad_case(case, dtype)
    cin, coff, ld = c["cin"], 8, c["cin"] + 24
    shape = (c["B"], *c["dims"])
    S = q(rnd((*shape, cin), 14), dtype)
    mask = q(rnd((*shape, cin + 16), 15), dtype)             # its own ld and coff (16)
    buf = torch.full((*shape, ld), SENTINEL, dtype=dtype)
    buf[..., coff:coff + cin] = S.to(dtype)
    out = buf.cuda()
    run_classes(ops, c, dtype, c["g"].to(dtype).cuda(), class_weights(ops, c, dtype), out, out_coff=coff, add=out, add_coff=coff,
                mask=mask.to(dtype).cuda(), mask_coff=16)
    o = out.float().cpu()
    owned = c["owned"]
    ref = torch.where(mask[..., 16:16 + cin] > 0, c["gx_ref"] + S, torch.zeros_like(S))
    r, a = tol(dtype, ref)
    got = o[..., coff:coff + cin]
    err = float((got[:, owned] - ref[:, owned]).abs().max() / ref.abs().max())
    print(f"[{case} {dtype}] data-gradient + shortcut + mask: max err {err:.2e} of the maximum")
    torch.testing.assert_close(got[:, owned], ref[:, owned], rtol=r * 2, atol=a * 2)
    assert bool((o[..., :coff] == SENTINEL).all()) and bool((o[..., coff + cin:] == SENTINEL).all())
    assert torch.equal(got[:, ~owned], S[:, ~owned])          # cells no class owns keep what they held


# ---- whole plans at odd extents ----
PLAN_ARCHS = ["r3d_18", "mc3_18", "r2plus1d_18"]


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


# (T, HW, B): (5, 36) runs the strided layers over (5,18,18), (3,9,9) and (2,5,5) -- even to odd, odd to odd, T 5 -> 3 -> 2 -> 1;
# (3, 20) ends with a temporal stride 2 over T = 1 (an empty class) and a 1x2x2 head
PLAN_CASES = [(5, 36, 1), (3, 20, 2)]
# bf16: rel-L2 of EVERY gradient buffer against the fp64 oracle with bf16-rounded convolution weights, as measured on an MI355X (the
# fp32 plans: 5.5e-7 ... 6.9e-7 on the same buffers).  The test asserts twice a buffer's own measured value, capped by the
# whole-network test's BWD_L2: the bound of a late layer is not widened by the error the early ones have accumulated.
BWD_L2_CAP = 8e-2
GRAD_BUFFERS = ["grad:stem"] + [f"grad:layer{l}.{b}" for l in (1, 2, 3, 4) for b in (0, 1)] + ["d(adv)/d(delta)"]
BF16_GRAD_L2 = {   # (arch, T): stem, layer1.0, layer1.1, layer2.0, layer2.1, layer3.0, layer3.1, layer4.0, layer4.1, delta
    ("r3d_18", 5): (7.66e-3, 7.43e-3, 7.30e-3, 5.77e-3, 5.46e-3, 4.22e-3, 3.92e-3, 2.38e-3, 1.71e-3, 4.66e-3),
    ("r3d_18", 3): (7.32e-3, 6.97e-3, 6.71e-3, 5.68e-3, 5.55e-3, 4.45e-3, 3.98e-3, 2.13e-3, 1.55e-3, 2.02e-3),
    ("mc3_18", 5): (5.70e-3, 5.40e-3, 5.13e-3, 5.00e-3, 4.70e-3, 4.32e-3, 4.02e-3, 2.37e-3, 1.68e-3, 2.14e-3),
    ("mc3_18", 3): (6.05e-3, 5.82e-3, 5.63e-3, 5.25e-3, 5.06e-3, 4.29e-3, 3.96e-3, 2.47e-3, 1.86e-3, 3.32e-3),
    ("r2plus1d_18", 5): (5.97e-3, 5.94e-3, 5.89e-3, 4.76e-3, 4.75e-3, 3.72e-3, 3.72e-3, 1.97e-3, 1.64e-3, 1.24e-2),
    ("r2plus1d_18", 3): (7.68e-3, 7.59e-3, 7.63e-3, 5.32e-3, 5.31e-3, 4.19e-3, 4.13e-3, 2.31e-3, 1.76e-3, 1.20e-2),
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("size", PLAN_CASES, ids=[f"T{t}_HW{hw}_B{b}" for t, hw, b in PLAN_CASES])
@pytest.mark.parametrize("arch", PLAN_ARCHS)
def test_videoresnet_odd_extents(arch, size, dtype):
    """forward endpoints, logits, every gradient buffer and d(adv)/d(delta) of one attack iteration against the fp64 oracle on the
    settled fixture: fp32 within 1e-3 of each tensor's maximum for EVERY element (the two torch oracles agree to 1e-6 on it)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    T, HW, B = size
    f32 = dtype == "f32"
    W, x_cl, delta = fixtures.settled_case(arch, T, HW, B)
    ref = fixtures.videoresnet_attack_pass(W, x_cl, delta, arch, torch.float64, bf16_conv_weights=not f32)
    eng = FlickerVideoResNet(arch, W, batch_size=B, sample_length=T, image_size=HW, dtype=dtype, l_inf_pert_norm=0.2)
    eng.pert_model.init_perturbation(delta.numpy())
    crit = Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)
    res = eng.step(x_cl.cuda(), ref["label"].cuda(), crit, update=False)
    hip = lambda n: torch.from_numpy(eng.net.activation(n)).permute(0, 4, 1, 2, 3).contiguous()
    fails = []
    for name, want in ref["ep"].items():
        e = rel_err(hip(name), want)
        print(f"[{arch} {size} {dtype}] {name}: max err {e:.3e} of the maximum")
        if not e < (1e-3 if f32 else 8e-2):
            fails.append((name, e))
    e = rel_err(eng._logits.cpu(), ref["logits"])
    print(f"[{arch} {size} {dtype}] logits: max err {e:.3e} of the maximum; adv loss {float(res['adv_loss']):.6f} (oracle {ref['adv']:.6f})")
    if not e < (1e-3 if f32 else 5e-2):
        fails.append(("logits", e))
    if f32 and float(res["adv_loss"]) != pytest.approx(ref["adv"], rel=1e-3, abs=1e-5):
        fails.append(("adv_loss", float(res["adv_loss"]), ref["adv"]))
    g_hip = eng._red[:3 * T].view(T, 3).cpu().t().reshape(3, T, 1, 1)
    grads = [("grad:" + n, hip("grad:" + n), want) for n, want in ref["ge"].items()] + [("d(adv)/d(delta)", g_hip, ref["g"])]
    assert [n for n, _, _ in grads] == GRAD_BUFFERS
    measured = dict(zip(GRAD_BUFFERS, BF16_GRAD_L2[(arch, T)]))
    worst_l2 = 0.0
    for name, got, want in grads:
        l2_bound = min(2 * measured[name], BWD_L2_CAP)
        e = rel_err(got, want)
        l2 = float((got.double() - want.double()).norm() / want.double().norm())
        worst_l2 = max(worst_l2, l2)
        print(f"[{arch} {size} {dtype}] {name}: max err {e:.3e} of the maximum, rel-L2 {l2:.3e}" + ("" if f32 else f" (bound {l2_bound:.2e})"))
        if not (e < 1e-3 if f32 else l2 < l2_bound):
            fails.append((name, e, l2))
    print(f"[{arch} {size} {dtype}] worst gradient rel-L2 {worst_l2:.3e}")
    assert not fails, fails
    assert float(g_hip[:, 2].abs().max()) == 0              # the frame whose delta lies beyond the clamp
    del eng
