"""The quantised instantiation of the uint8 stem (csrc/stem_fwd.hip, QUANT: flk_apply_args.q_lut with center = 0) through
flk_stem_fwd_u8, on the GPU.

What it must compute: per staged byte, x = u8 / 128 - 1; u = clip(x + p, lo, hi); q = the export's encode of u; v = q / 128 - 1 -- the
value the STORED video holds, exact in bf16.  So its output is, value for value, the plain instantiation run on the stored bytes
(i3d_spec.quantised_stem_bytes) with adv_flag = 0: with no position-class table, and with the all-zero table flk_stem_delta_bias computes
for adv_flag = 0 (the route FlickerI3D.quantised_logits takes).  On a dyadic fixture (the recipe and the weights of
test_stem_fwd_edges_gpu.py) nothing rounds before the bf16 store and the output is the float64 oracle of stem_fwd_oracle.py on those
bytes, rounded once.

Each case asserts on the numpy restatement alone, before the GPU is touched, that it can fail: the stored bytes differ from the source
on 10..90 % of the values, the saturation at 0 / 255 is active on >= 1 %, one (frame, channel) sits on a rounding tie (an entry of delta
whose perturbation is an odd multiple of 1/256: every pixel of it is a tie), one is below half a level, and the plain centred staged
clip differs from the quantised staged clip on >= 10 % of the values -- a kernel that ignored q_lut would fail.  (The clean case,
adv_flag = 0, has nothing to differ by: its output is the clean one.)

The gradient.  The straight-through estimator is the clip mask the plain kernels build; the public entry points flk_stem_delta_grad /
flk_stem_delta_grad_mask keep refusing q_lut (tests/test_quant_apply_cpu.py pins that) and the plan clears it before it calls them:
flk_net_backward_delta with q_lut is bitwise the call without it, for shared and per-clip delta (test_plan_gradient_...)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stem_fwd_oracle as so
from flickering_adversarial_video_amd import i3d_spec

pytestmark = pytest.mark.gpu

FLK_EINVAL = -1
NAN_BITS = 0x7FC1
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int16)


CASES = {
    "T2_both_borders": dict(B=1, T=2, kw=dict(dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0)),
    "T10_partial_tile": dict(B=1, T=10, kw=dict(dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0)),
    "per_clip_dclip_dev": dict(B=2, T=4, per_clip=True, dclip_dev=(0.4, 0.23), kw=dict(dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0)),
    "rolls": dict(B=1, T=8, kw=dict(dclip=0.4, adv_flag=1.0, shift_x=-3, shift_p=13)),
    "half_flag": dict(B=1, T=4, kw=dict(dclip=0.4, adv_flag=0.5, shift_x=0, shift_p=0)),
    "clean": dict(B=1, T=4, kw=dict(dclip=0.4, adv_flag=0.0, shift_x=0, shift_p=0), clean=True),
}


@functools.lru_cache(maxsize=None)
def general_weights():
    rng = np.random.default_rng(317)
    w7 = torch.from_numpy((rng.standard_normal((7, 7, 7, 3, 64)) * (2.0 / 1029) ** 0.5).astype(F32))
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, 64).astype(F32))
    bias = torch.from_numpy(rng.uniform(-0.3, 0.3, 64).astype(F32))
    return w7, scale, bias


def perturbation(delta, B, T, kw, dev):
    """p'[b or 0, t, c] in float32 as the kernel forms it (TF dialect: inv_std = 1)"""
    _, _, p = so.staged_operands(np.zeros((B, T, 224, 224, 3), np.uint8)[:, :, :1, :1], delta, dtype=F32, dclip_dev=dev, dclip=kw["dclip"],
                                 adv_flag=kw["adv_flag"], shift_p=kw["shift_p"])
    return p


def make_case(name):
    """fixture of a case + the numpy-only assertions that it can fail"""
    c = CASES[name]
    B, T, kw = c["B"], c["T"], dict(c["kw"])
    rng = np.random.default_rng(2000 + sorted(CASES).index(name))
    xu = rng.integers(0, 256, (B, T, 224, 224, 3), dtype=np.uint8)
    nd = (B, T, 3) if c.get("per_clip") else (T, 3)
    delta = rng.uniform(-0.5, 0.5, nd).astype(F32)
    flat = delta.reshape(-1)
    sub = rng.permutation(flat.size)[:max(1, flat.size // 4)]               # a quarter of the entries below half a level
    flat[sub] = rng.uniform(-0.003, 0.003, sub.size).astype(F32)
    flag = kw["adv_flag"] or 1.0
    tie = [i for i in range(flat.size) if i not in set(sub.tolist())][0]
    flat[tie] = F32(3.0 / 256.0 / flag)                                      # a rounding tie on every pixel of that (frame, channel)
    dev = np.asarray(c["dclip_dev"], F32) if "dclip_dev" in c else None
    stored = i3d_spec.quantised_stem_bytes(xu, delta, dclip_dev=dev, **kw)
    src = np.roll(xu, kw["shift_x"], axis=1)
    if c.get("clean"):
        assert np.array_equal(stored, src)
        return xu, delta, dev, kw, stored
    p = perturbation(delta, B, T, kw, dev)                                   # [B or 1, T, 3]
    differ = float((stored != src).mean())
    assert 0.10 <= differ <= 0.90, differ
    u = (src.astype(F32) * F32(1.0 / 128.0) + F32(-1.0)) + p[:, :, None, None, :]
    sat = float(((u < -1.0) | (u > 1.0 - 1.0 / 128.0)).mean())
    assert sat >= 0.01, sat
    k256 = p.astype(np.float64) * 256
    assert bool(((k256 == np.rint(k256)) & (np.rint(k256) % 2 == 1)).any()), "no (frame, channel) on a rounding tie"
    assert bool(((np.abs(p) * 128 < 0.5) & (p != 0)).any()), "no sub-level (frame, channel)"
    _, xc, _ = so.staged_operands(xu, delta, dtype=F32, dclip_dev=dev, **kw)
    plain_staged = torch.from_numpy(xc).bfloat16().float().numpy()
    quant_staged = stored.astype(F32) * F32(1.0 / 128.0) + F32(-1.0)
    staged_differ = float((plain_staged != quant_staged).mean())
    assert staged_differ >= 0.10, staged_differ
    print(f"[{name}] stored != source on {differ:.1%}, saturation active on {sat:.1%}, plain staged != quantised staged on {staged_differ:.1%}")
    return xu, delta, dev, kw, stored


def quant_args(ops, x, delta, dev, kw):
    return ops.make_apply_args(x, delta, fold_t=ops.I3D_FOLD, quantise="tf", center=False, dclip_dev=None if dev is None else torch.from_numpy(dev).cuda(), **kw)


def fresh_out(B, T):
    out = torch.empty((B, T // 2, 112, 112, 64), dtype=torch.bfloat16, device="cuda")
    out.view(torch.int16).fill_(NAN_BITS)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_quant_stem_is_the_plain_stem_on_the_stored_bytes(ops, name):
    xu, delta, dev, kw, stored = make_case(name)
    B, T = xu.shape[:2]
    w7, scale, bias = general_weights()
    w = ops.StemFwdU8Weights(w7.numpy())
    sg, bg = scale.cuda(), bias.cuda()
    xg, dg = torch.from_numpy(xu).cuda(), torch.from_numpy(delta).cuda()
    got = ops.stem_fwd_u8(quant_args(ops, xg, dg, dev, kw), w, sg, bg, None, out=fresh_out(B, T))
    # the plain instantiation on the stored bytes (already rolled), adv_flag = 0: no table, and the all-zero table of flk_stem_delta_bias
    zero = torch.zeros((T, 3), dtype=torch.float32, device="cuda")
    plain = ops.make_apply_args(torch.from_numpy(stored).cuda(), zero, fold_t=ops.I3D_FOLD, center=True, dclip=0.0, adv_flag=0.0)
    want = ops.stem_fwd_u8(plain, w, sg, bg, None, out=fresh_out(B, T))
    tab = ops.stem_delta_bias_table(plain, w7.numpy(), scale.numpy())
    assert not bool(tab.view(torch.int32).any()), "the table of adv_flag = 0 is not all +0"
    want_tab = ops.stem_fwd_u8(plain, w, sg, bg, tab, out=fresh_out(B, T))
    torch.cuda.synchronize()
    assert not bool((bits(want) == NAN_BITS).any())
    assert torch.equal(bits(want_tab), bits(want))
    differ = bits(got) != bits(want)
    if bool(differ.any()):
        i = tuple(int(v) for v in differ.nonzero()[0])
        raise AssertionError(f"{int(differ.sum())} of {differ.numel()} outputs differ from the plain stem on the stored bytes, the first at {i}: "
                             f"quantised {float(got.cpu()[i])}, plain {float(want.cpu()[i])}")
    if not CASES[name].get("clean"):
        # ... and the quantiser is not a no-op here: the plain centred stem of the same arguments gives other bits
        pc = ops.make_apply_args(xg, dg, fold_t=ops.I3D_FOLD, center=True, dclip_dev=None if dev is None else torch.from_numpy(dev).cuda(), **kw)
        other = ops.stem_fwd_u8(pc, w, sg, bg, ops.stem_delta_bias_table(pc, w7.numpy(), scale.numpy()), out=fresh_out(B, T))
        torch.cuda.synchronize()
        assert float((bits(other) != bits(got)).float().mean()) > 0.10


def test_clean_case_is_the_clean_output(ops):
    xu, delta, dev, kw, stored = make_case("clean")
    w7, scale, bias = general_weights()
    w = ops.StemFwdU8Weights(w7.numpy())
    xg, dg = torch.from_numpy(xu).cuda(), torch.from_numpy(delta).cuda()
    got = ops.stem_fwd_u8(quant_args(ops, xg, dg, dev, kw), w, scale.cuda(), bias.cuda(), None)
    clean = ops.make_apply_args(xg, dg, fold_t=ops.I3D_FOLD, center=True, dclip=0.4, adv_flag=0.0)
    want = ops.stem_fwd_u8(clean, w, scale.cuda(), bias.cuda(), None)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))


def test_dyadic_fixture_is_the_float64_oracle_on_the_stored_bytes(ops):
    """the recipe of test_stem_fwd_edges_gpu.exact_case: clip bytes multiples of 32, delta multiples of 1/64 within +-0.5 (beyond
    dclip = 0.375), that module's integer weights / dyadic scale and bias.  The stored value is k/128, |k| <= 128; products are m/128
    with |m| <= 512 and any partial sum of the 1029 taps stays below 2^24 / 128: nothing rounds before the bf16 store."""
    import test_stem_fwd_edges_gpu as edges
    B, T = 1, 10
    rng = np.random.default_rng(1234)
    xu = (rng.integers(0, 8, (B, T, 224, 224, 3)) * 32).astype(np.uint8)
    delta = (rng.integers(-32, 33, (T, 3)) / 64).astype(F32)
    delta[0] = (3.0 / 256.0, -0.5, 0.5)                                      # a tie; two entries beyond dclip
    kw = dict(dclip=0.375, adv_flag=1.0, shift_x=2, shift_p=-1)
    stored = i3d_spec.quantised_stem_bytes(xu, delta, **kw)
    differ = float((stored != np.roll(xu, 2, axis=1)).mean())
    assert 0.10 <= differ <= 0.98, differ
    assert float(((stored == 0) & (np.roll(xu, 2, axis=1) != 0)).mean()) >= 0.01              # the clamp at -1 is active
    v = stored.astype(np.float64) / 128 - 1
    w7, scale, bias = edges.dyadic_weights()
    w_pert = w7 * scale
    vt, pz = torch.from_numpy(v), torch.zeros((1, T, 3), dtype=torch.float64)
    ref = so.stem_oracle(vt, pz, w7, w_pert, scale, bias, torch.float64)
    ref32 = so.stem_oracle(vt, pz, w7, w_pert, scale, bias, torch.float32)
    assert torch.equal(ref32.double(), ref)                                  # fp32 evaluates the oracle exactly: no order can show
    assert float((ref != 0).float().mean()) >= 0.25
    want = ref.float().bfloat16()
    a = ops.make_apply_args(torch.from_numpy(xu).cuda(), torch.from_numpy(delta).cuda(), fold_t=ops.I3D_FOLD, quantise="tf", center=False, **kw)
    got = ops.stem_fwd_u8(a, ops.StemFwdU8Weights(w7.numpy()), scale.cuda(), bias.cuda(), None, out=fresh_out(B, T))
    torch.cuda.synchronize()
    differ = bits(got) != bits(want)
    assert not bool(differ.any()), f"{int(differ.sum())} of {differ.numel()} outputs differ from the float64 oracle on the stored bytes"


REFUSALS = {
    # name: (what differs from a valid quantised call, what flk_last_error() must name)
    "center_1": (dict(center=1), "center"),
    "q_levels_255": (dict(q_levels=255.0), "q_levels"),
    "x_scale_256": (dict(x_scale=1.0 / 256.0), "x_scale"),
    "dense_delta": (dict(dense=True), "delta_dense"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refuses(ops, name):
    from flickering_adversarial_video_amd._lib import ptr, stream_ptr
    lib = ops.load()
    how, field = REFUSALS[name]
    B, T = 1, 2
    x = torch.zeros((B, T, 224, 224, 3), dtype=torch.uint8, device="cuda")
    delta = torch.zeros((T, 224, 224, 3) if how.get("dense") else (T, 3), dtype=torch.float32, device="cuda")
    a = ops.make_apply_args(x, delta, fold_t=ops.I3D_FOLD, quantise="tf", center=False)
    assert a.q_lut and a.q_levels == 128.0 and a.delta_dense == int(bool(how.get("dense")))
    for k in ("center", "q_levels", "x_scale"):
        if k in how:
            setattr(a, k, how[k])
    w7, scale, bias = general_weights()
    w = ops.StemFwdU8Weights(w7.numpy())
    sg, bg = scale.cuda(), bias.cuda()
    out = fresh_out(B, T)
    torch.cuda.synchronize()
    rc = lib.flk_stem_fwd_u8(C.byref(a), w.handle, ptr(sg), ptr(bg), None, 0, ptr(out), 64, stream_ptr())
    msg = lib.flk_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    assert rc == FLK_EINVAL, (rc, msg)
    assert "flk_stem_fwd_u8" in msg and field in msg, msg
    assert bool((bits(out) == NAN_BITS).all()), "a refused call wrote to the output"


# ---- the gradient: straight through the clip mask, through the plan ------------------------------------------------------------------
@pytest.mark.parametrize("per_clip", [False, True], ids=["shared", "per_clip"])
def test_plan_gradient_with_q_lut_is_the_gradient_without(ops, per_clip):
    """flk_net_prepare_backward_delta / flk_net_backward_delta accept quantised arguments (center = 0) and give, bit for bit, the
    delta-gradient of the same arguments without q_lut -- same forward pass, same dlogits.  T = 16, the smallest clip the I3D plan
    admits, at its 224 x 224; clamp active on 10..90 % of the values."""
    from flickering_adversarial_video_amd._lib import FLK_NET_I3D
    B, T = 2, 16
    rng = np.random.default_rng(77)
    xu = rng.integers(0, 256, (B, T, 224, 224, 3), dtype=np.uint8)
    xu[:, :, :60] //= 4                                                      # dark and bright bands: the clamp is active there
    xu[:, :, -60:] = 255 - (255 - xu[:, :, -60:]) // 4
    delta = rng.uniform(-0.4, 0.4, (B, T, 3) if per_clip else (T, 3)).astype(F32)
    u = (xu.astype(F32) / 128 - 1) + delta.reshape(-1, T, 3)[:, :, None, None, :]
    active = float(((u < -1) | (u > 1)).mean())
    assert 0.10 <= active <= 0.90, active
    net = ops.Net(FLK_NET_I3D, "bf16", B, T, 224, 224, i3d_spec.synthetic_i3d_weights(42))
    assert net.has_backward_delta
    xg, dg = torch.from_numpy(xu).cuda(), torch.from_numpy(delta).cuda()
    aq = ops.make_apply_args(xg, dg, fold_t=ops.I3D_FOLD, quantise="tf", center=False)
    ap = ops.make_apply_args(xg, dg, fold_t=ops.I3D_FOLD, center=False)
    xs2d = torch.empty((B, T // 2, 112, 112, 32), dtype=torch.bfloat16, device="cuda")
    logits = net.forward_apply(aq, xs2d)
    dl = torch.from_numpy(rng.standard_normal(tuple(logits.shape)).astype(F32) * 1e-2).cuda()
    scratch = torch.empty(max(1, ops.load().flk_stem_delta_grad_scratch_bytes(B, T, 224) // 4), dtype=torch.float32, device="cuda")
    grads = []
    for a, prepare in ((aq, False), (ap, False), (aq, True)):
        g = torch.full((B, T, 3) if per_clip else (T, 3), float("nan"), dtype=torch.float32, device="cuda")
        net.forward_apply(aq, xs2d, logits)                                  # the same forward pass in front of every backward
        if prepare:
            net.prepare_backward_delta(a, scratch)
        net.backward_delta(dl, a, g, scratch)
        torch.cuda.synchronize()
        grads.append(g.cpu())
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    assert torch.equal(grads[2].view(torch.int32), grads[1].view(torch.int32))
    # center = 1 with q_lut is refused, naming both
    aq.center = 1
    with pytest.raises(Exception, match="q_lut"):
        net.backward_delta(dl, aq, torch.empty_like(grads[0]).cuda(), scratch)
