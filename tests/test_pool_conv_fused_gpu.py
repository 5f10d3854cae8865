"""MaxPool3d_2a_3x3 with Conv3d_2b_1x1 inside (csrc/pool.hip: flk_maxpool3d_fwd_conv1x1 / flk_maxpool3d_bwd_conv1x1) against the two launches
they replace (GPU).  Nothing here is approximate: the fused kernels run the pool bodies, the MFMA instruction, the K order and the epilogue
of the stand-alone kernels, so every comparison is torch.equal on the stored bits.

Kernel level: the smallest (B,T,H,W) grids where the tiling can go wrong -- the forward tiles 256 consecutive pooled positions of the flat
[B,T,Ho,Wo] grid, the backward boxes of 8 x 32 or 16 x 16 windows of one frame plus the previous row and column:
    (1,1,4,4)    4 pooled positions   one partial tile
    (1,2,12,12)  72                   small partial tile
    (1,1,32,32)  256                  one exact tile
    (1,1,34,30)  255                  one short of a tile; a 16 x 16 box cut at both edges
    (1,1,32,34)  272                  a second tile of 16; an 8 x 32 box cut at the right
    (2,3,20,20)  600                  three tiles, the last partial, tiles crossing frame and clip boundaries
and two more for the backward boxes: (1,1,40,72) -- 3 x 2 boxes of 8 x 32, one with oh0 > 0 and ow0 > 0, cut at both edges -- and
(1,1,64,32) -- two 16 x 16 boxes, the second at oh0 = 16.  Every grid has boxes at oh = 0 and ow = 0.
Inputs: non-negative small integers with relu_input (many exact ties, all-zero windows -> index 255) and a signed variant with both zero
signs; a batch-norm scale with negative entries; random weights; a gradient containing zeros; every tensor also as channels [16, 80) of a
96-wide buffer whose other columns hold a sentinel that must survive; both request flags (pooled map / its gradient written or not).

Plan level: the I3D bf16 plan at B = 1 and B = 4 (the half-batch split), T = 16, built with FLK_POOL_CONV_FUSED = 0 and = 1 on the same clip,
labels and perturbation: logits, the perturbation's gradient and the endpoints around the fused pair -- the lazily filled pooled map and its
gradient included -- are bitwise equal, and the per-launch profile lists the two fused operators against the four old ones."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
K, S = (1, 3, 3), (1, 2, 2)
SENT = -7.0
CASES = [(1, 1, 4, 4), (1, 2, 12, 12), (1, 1, 32, 32), (1, 1, 34, 30), (1, 1, 32, 34), (2, 3, 20, 20), (1, 1, 40, 72), (1, 1, 64, 32)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


@pytest.fixture(scope="module")
def unit(ops):
    """the 1x1x1 unit: random weights, a batch-norm scale with negative entries, a bias; forward and data-gradient operators"""
    rng = np.random.default_rng(7)
    w = (rng.standard_normal((1, 1, 1, 64, 64)) * 0.2).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, 64).astype(np.float32) * np.where(rng.random(64) < 0.3, -1.0, 1.0).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32) * 0.5
    wf = ops.ConvWeights(w, BF16, 4)
    wb = ops.ConvWeights(w, BF16, 4, row_scale=scale, transpose=True)
    return wf, wb, torch.from_numpy(scale).cuda(), torch.from_numpy(bias).cuda()


def wide(t, sliced):
    """t [..., 64] as it is, or as channels [16, 80) of a 96-wide buffer filled with the sentinel; returns (buffer, coff)"""
    if not sliced:
        return t.contiguous(), 0
    buf = torch.full((*t.shape[:4], 96), SENT, dtype=t.dtype, device=t.device)
    buf[..., 16:80] = t
    return buf, 16


def blank(shape4, sliced, device="cuda"):
    return torch.full((*shape4, 96 if sliced else 64), SENT, dtype=BF16, device=device), (16 if sliced else 0)


def inner(buf, coff):
    return buf[..., coff:coff + 64]


def outside_untouched(buf, coff):
    if buf.shape[4] == 64:
        return True
    return bool((buf[..., :coff] == SENT).all()) and bool((buf[..., coff + 64:] == SENT).all())


def make_input(shape, variant, seed):
    rng = np.random.default_rng(seed)
    B, T, H, W = shape
    if variant == "relu":       # a ReLU output: small non-negative integers, about half of them zero
        x = rng.integers(0, 4, (B, T, H, W, 64)).astype(np.float32) * (rng.random((B, T, H, W, 64)) < 0.5)
        if H >= 6 and W >= 6:
            x[:, :, 0:5, 0:5, :32] = 0.0          # whole windows of zeros: relu_input records 255
    else:                       # signed, with zeros of both signs
        x = rng.integers(-3, 4, (B, T, H, W, 64)).astype(np.float32)
        x = np.where((x == 0) & (rng.random(x.shape) < 0.5), np.float32(-0.0), x)
        if H >= 6 and W >= 6:
            x[:, :, 0:5, 0:5, :16] = np.where(rng.random((B, T, 5, 5, 16)) < 0.5, np.float32(-0.0), np.float32(0.0))
    return torch.from_numpy(x.astype(np.float32)).to(BF16).cuda()


@pytest.mark.parametrize("write", [False, True], ids=["nowrite", "write"])
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("variant", ["relu", "signed"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_fused_equals_two_launches(ops, unit, shape, variant, sliced, write):
    wf, wb, scale, bias = unit
    B, T, H, W = shape
    og = (B, T, -(-H // 2), -(-W // 2))
    relu_input = variant == "relu"
    x, xc = wide(make_input(shape, variant, seed=sum(shape)), sliced)

    # ---- forward: pool -> 1x1x1 unit (scale, bias, ReLU) ----
    p_ref, pc = blank(og, sliced)
    _, idx_ref, ctx_ref = ops.maxpool3d(x, K, S, C_=64, relu_input=relu_input, in_coff=xc, out=p_ref, out_coff=pc)
    o_ref, oc = blank(og, sliced)
    ops.conv3d(p_ref, wf, in_coff=pc, cin=64, scale=scale, bias=bias, relu=True, out=o_ref, out_coff=oc)

    o_got, _ = blank(og, sliced)
    p_got, _ = blank(og, sliced)
    _, idx_got, ctx_got = ops.maxpool3d_conv1x1(x, wf, scale=scale, bias=bias, relu=True, relu_input=relu_input, in_coff=xc, out=o_got,
                                                out_coff=oc, pool_out=p_got if write else None, pool_out_coff=pc)
    torch.cuda.synchronize()
    assert torch.equal(idx_got, idx_ref)
    assert torch.equal(o_got.view(torch.int16), o_ref.view(torch.int16))          # bits, sentinel columns included
    assert outside_untouched(o_got, oc)
    if relu_input and H >= 6:
        assert bool((idx_ref == 255).any())
    if write:
        assert torch.equal(p_got.view(torch.int16), p_ref.view(torch.int16))
    else:
        assert bool((p_got == SENT).all())                                         # not touched without the flag

    # ---- backward: 1x1x1 data-gradient (no mask) -> pool backward ----
    rng = np.random.default_rng(11 + sum(shape))
    g = rng.standard_normal((*og, 64)).astype(np.float32) * (rng.random((*og, 64)) < 0.7)
    g, gc = wide(torch.from_numpy(g.astype(np.float32)).to(BF16).cuda(), sliced)
    gp_ref, gpc = blank(og, sliced)
    ops.conv3d(g, wb, in_coff=gc, cin=64, out=gp_ref, out_coff=gpc)
    gin_ref, gic = blank(shape, sliced)
    ops.maxpool3d_bwd(ctx_ref, gp_ref, gout_coff=gpc, gin=gin_ref, gin_coff=gic)

    gin_got, _ = blank(shape, sliced)
    gp_got, _ = blank(og, sliced)
    ops.maxpool3d_bwd_conv1x1(ctx_got, g, wb, g_coff=gc, gin=gin_got, gin_coff=gic, gpool=gp_got if write else None, gpool_coff=gpc)
    torch.cuda.synchronize()
    assert torch.equal(gin_got.view(torch.int16), gin_ref.view(torch.int16))
    assert outside_untouched(gin_got, gic)
    assert bool((inner(gin_ref, gic) != 0).any())
    if write:
        assert torch.equal(gp_got.view(torch.int16), gp_ref.view(torch.int16))
    else:
        assert bool((gp_got == SENT).all())


def test_entry_points_refuse_what_the_query_refuses(ops, unit):
    """fp32, another window and another channel count are errors with a reason, not a silent fall-back"""
    from flickering_adversarial_video_amd._lib import FlickerHipError
    wf, wb, scale, bias = unit
    x = torch.zeros((1, 1, 8, 8, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(FlickerHipError, match="bf16"):
        ops.maxpool3d_conv1x1(x, wf)
    x = torch.zeros((1, 1, 9, 8, 64), dtype=BF16, device="cuda")
    with pytest.raises(FlickerHipError, match="even"):
        ops.maxpool3d_conv1x1(x, wf)
    w8 = ops.ConvWeights(np.zeros((1, 1, 1, 64, 128), np.float32), BF16, 8)
    x = torch.zeros((1, 1, 8, 8, 64), dtype=BF16, device="cuda")
    with pytest.raises(FlickerHipError, match="64"):
        ops.maxpool3d_conv1x1(x, w8)


# ---- plan level ---------------------------------------------------------------------------------------------------------------------
T = 16
ENDPOINTS = ["Conv3d_2b_1x1", "grad:Conv3d_2b_1x1", "grad:Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "grad:MaxPool3d_2a_3x3"]
FUSED_OPS = {"MaxPool3d_2a_3x3+Conv3d_2b_1x1", "Conv3d_2b_1x1/dgrad+MaxPool3d_2a_3x3/grad"}
OLD_OPS = {"MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2b_1x1/dgrad", "MaxPool3d_2a_3x3/grad"}


def run_plan(B, switch, monkeypatch, labels=None):
    from flickering_adversarial_video_amd import i3d_spec
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    monkeypatch.setenv("FLK_POOL_CONV_FUSED", switch)
    eng = FlickerI3D(i3d_spec.synthetic_i3d_weights(42), batch_size=B, frames=T, dtype="bf16")
    xu = torch.from_numpy(i3d_spec.synthetic_clip_u8(B, T, seed=77)).cuda()
    eng.perturbation.copy_(torch.from_numpy(np.random.default_rng(5).uniform(-0.1, 0.1, (T, 1, 1, 3)).astype(np.float32)))
    if labels is None:      # the clean prediction (the loss has a gradient there); the second plan gets the first one's labels
        labels = eng.logits(xu, adv_flag=0.0).argmax(-1).clone()
    eng.step(xu, labels, update=False)
    torch.cuda.synchronize()
    out = {"logits": eng._logits.detach().cpu().numpy().copy(), "delta_gradient": eng.delta_gradient().detach().cpu().numpy().copy()}
    for name in ENDPOINTS:
        out[name] = eng.net.activation(name)
    eng.net.profile(True)
    eng.step(xu, labels, update=False)
    torch.cuda.synchronize()
    names = {r["name"]: r["kernel"] for r in eng.net.profile_read()}
    eng.net.profile(False)
    del eng
    return out, names, labels


@pytest.mark.parametrize("B", [1, 4])
def test_plan_fused_equals_four_operators(B, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    old, old_names, labels = run_plan(B, "0", monkeypatch)
    new, new_names, _ = run_plan(B, "1", monkeypatch, labels)
    assert OLD_OPS <= set(old_names) and not (FUSED_OPS & set(old_names)), sorted(old_names)
    assert FUSED_OPS <= set(new_names) and not (OLD_OPS & set(new_names)), sorted(new_names)
    assert new_names["MaxPool3d_2a_3x3+Conv3d_2b_1x1"] == "maxpool133_conv1x1_fwd"
    assert new_names["Conv3d_2b_1x1/dgrad+MaxPool3d_2a_3x3/grad"] == "maxpool133_conv1x1_bwd"
    for name in ["logits", "delta_gradient"] + ENDPOINTS:
        a, b = old[name], new[name]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        assert np.any(a != 0), name
