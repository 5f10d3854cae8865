"""The stem computed straight from the uint8 clip (csrc/stem_fwd.hip: flk_stem_fwd_u8, with the position-class table of
flk_stem_delta_bias) bit for bit where its arithmetic is exact, per element where it rounds, and at what it refuses (GPU).
The oracle is tests/stem_fwd_oracle.py.

1. Exact cases (test_exact).  A dyadic fixture: clip bytes are multiples of 32 (x a multiple of 1/4, or of 1/8 under the second
decode), delta multiples of 1/64 within +-0.5 (1/16 where inv_std and adv_flag divide further), dclip / lo / hi dyadic and inside the
value range, integer weights in [-4, 4], bn_scale from {0.5, 1, 2}, bn_bias multiples of 1/4.  Every staged value is then k/128 with
|k| < 256 (bf16-exact), every product m/128 with |m| < 1024, and every partial sum of ANY grouping stays below 2^24 / 128 in size: for
the clip term at most 1029 * 2 * 4 = 8232, times scale 2, plus bias 2, plus a table entry of at most 21 * 0.75 * 49 * 8 = 6174 --
23 000 * 128 < 2^22.  Nothing rounds before the bf16 store, so summation order, FMA contraction and MFMA grouping cannot show, and the
kernel must equal the float64 oracle, rounded once to bf16, BIT FOR BIT.  Each case asserts on the reference alone, before the GPU is
touched: the staged values are k/128 with |k| < 256 and the same in fp32 and float64; the oracle evaluated in fp32 equals the float64
one exactly; the clamp is active on 10..90 % of the values (the clean case is exempt); at least 25 % of the outputs are nonzero.

2. Rounding cases (test_rounding).  General values; the oracle is float64 on the kernel's own operands and every element is held to
stem_fwd_oracle.stem_bound_ratio (conv_bound.bf16_bound_ratio with n_K = 37 * 32 and the table term's 72 * 2^-24, both derived
there).  The TF decode u8 / 128 - 1 is kept: x is exact, so the staged value has one fp32 evaluation whatever the compiler fuses.

3. Refusals (test_refuses): FLK_EINVAL, the field named in flk_last_error(), a poisoned output untouched.

Measured on an MI355X: every exact case bitwise equal; worst |y - r| / bound of the rounding cases:
    shared_T10 0.849   per_clip 0.860        (test_stem_fwd_gpu.py: shared 0.854, per_clip_T10 0.845, rolled 0.832, clean 0.820)
The CPU stand-in -- torch fp32 convolution, one bf16 rounding -- gives 0.849 and 0.860 on the same two fixtures: almost all of it is
the output rounding.  The same stand-in with its output truncated to bf16 leaves 49 273 and 27 820 elements outside the bound.
The exact cases cannot see a wrong rounding of the STAGED value (it is bf16-exact by construction); the rounding cases do."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stem_fwd_oracle as so

pytestmark = pytest.mark.gpu

FLK_EINVAL = -1                   # include/flicker_hip.h
NAN_BITS = 0x7FC1                 # a quiet bf16 NaN no arithmetic produces


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int16)


# ---- 1. exact cases -------------------------------------------------------------------------------------------------------------------
# name -> geometry, what make_apply_args gets (kw), the decode set on the struct, the denominator of delta
EXACT = {
    "clean_T2": dict(B=1, T=2, kw=dict(adv_flag=0.0, dclip=0.375, lo=-0.75, hi=0.875), table=False, clamp_share=False),
    "shared_T10": dict(B=1, T=10, kw=dict(dclip=0.375, lo=-0.75, hi=0.875)),
    "per_clip_dclip_dev": dict(B=2, T=4, per_clip=True, dclip_dev=(0.375, 0.125), kw=dict(dclip=0.5, lo=-0.75, hi=0.875)),
    "rolls": dict(B=1, T=8, kw=dict(dclip=0.375, lo=-0.75, hi=0.875, shift_x=-3, shift_p=8 + 5)),
    "scaled": dict(B=1, T=6, den=16, decode=(1.0 / 256, -0.5),
                   kw=dict(dclip=0.375, lo=-0.25, hi=0.1875, inv_std=(0.5, 2.0, 4.0), adv_flag=0.5)),
    "no_dclip": dict(B=1, T=6, kw=dict(dclip=0.0, lo=-0.75, hi=0.875)),
    "wide_out_embedded": dict(B=2, T=4, kw=dict(dclip=0.375, lo=-0.75, hi=0.875), embedded=True),
}


@functools.lru_cache(maxsize=None)
def dyadic_weights():
    rng = np.random.default_rng(29)
    w7 = torch.from_numpy(rng.integers(-4, 5, (7, 7, 7, 3, 64)).astype(np.float32))
    scale = torch.from_numpy(rng.choice(np.array([0.5, 1.0, 2.0], np.float32), 64))
    bias = torch.from_numpy((rng.integers(-8, 9, 64) / 4).astype(np.float32))
    return w7, scale, bias


def exact_case(name):
    """the fixture of a case and the bits its output must have; asserts the case's preconditions (CPU only)"""
    c = EXACT[name]
    B, T, den = c["B"], c["T"], c.get("den", 64)
    rng = np.random.default_rng(1000 + sorted(EXACT).index(name))
    xu = torch.from_numpy((rng.integers(0, 8, (B, T, 224, 224, 3)) * 32).astype(np.uint8))
    delta = torch.from_numpy((rng.integers(-den // 2, den // 2 + 1, (B, T, 3) if c.get("per_clip") else (T, 3)) / den).astype(np.float32))
    dev = torch.tensor(c["dclip_dev"], dtype=torch.float32) if "dclip_dev" in c else None
    w7, scale, bias = dyadic_weights()
    kw = dict(c["kw"])
    if "decode" in c:
        kw["x_scale"], kw["x_bias"] = c["decode"]
    if kw["dclip"] > 0 and dev is None and kw.get("adv_flag", 1.0) != 0:
        assert float(delta.abs().max()) > kw["dclip"]                  # some entries beyond the clamp of delta
    np_dev = None if dev is None else dev.numpy()
    x, xc, p = so.staged_operands(xu.numpy(), delta.numpy(), dtype=np.float64, dclip_dev=np_dev, **kw)
    _, xc32, p32 = so.staged_operands(xu.numpy(), delta.numpy(), dtype=np.float32, dclip_dev=np_dev, **kw)
    # every staged value is k/128, |k| < 256: bf16-exact; the fp32 evaluation of the operands is the float64 one
    k = xc * 128
    assert np.array_equal(k, np.rint(k)) and float(np.abs(k).max()) < 256
    assert np.array_equal(xc32.astype(np.float64), xc) and np.array_equal(p32.astype(np.float64), p)
    xct, pt = torch.from_numpy(xc), torch.from_numpy(p)
    assert torch.equal(xct.float().bfloat16().double(), xct)
    active = float((xc != x).mean())
    if c.get("clamp_share", True):
        assert 0.10 <= active <= 0.90, active
    w_pert = w7 * scale
    assert torch.equal(w7.bfloat16().float(), w7) and torch.equal(w_pert.double(), w7.double() * scale.double())
    ref = so.stem_oracle(xct, pt, w7, w_pert, scale, bias, torch.float64)
    ref32 = so.stem_oracle(xct, pt, w7, w_pert, scale, bias, torch.float32)
    assert torch.equal(ref32.double(), ref)                              # fp32 evaluates the oracle exactly (and holds its values)
    nonzero = float((ref != 0).float().mean())
    assert nonzero >= 0.25, nonzero
    want = ref.float().bfloat16()                                        # the one rounding
    print(f"[{name}] clamp active on {active:.1%} of the values, {nonzero:.1%} of the outputs nonzero, "
          f"{int(torch.unique(bits(want)).numel())} distinct bf16 values, {float((want.double() != ref).float().mean()):.1%} of them rounded")
    return xu, delta, dev, kw, want


@pytest.mark.parametrize("name", list(EXACT))
def test_exact(ops, name):
    c = EXACT[name]
    B, T = c["B"], c["T"]
    To = T // 2
    xu, delta, dev, kw, want = exact_case(name)
    w7, scale, bias = dyadic_weights()
    decode = (kw.pop("x_scale", None), kw.pop("x_bias", None))

    n = xu.numel()
    if c.get("embedded"):
        # the clip as a view at a nonzero offset that is a multiple of 8, not of 16, inside a buffer of byte 255 -- a value the clip
        # never holds (<= 224), so a read outside the clip changes result bits
        off = 4096 + 24
        xbuf = torch.full((n + 2 * off,), 255, dtype=torch.uint8, device="cuda")
        xg = xbuf[off:off + n].view(xu.shape)
        xg.copy_(xu)
        assert xg.data_ptr() % 16 == 8 and xg.is_contiguous()
        # the output as the first 64 of 96 channels of a NaN-filled buffer with one guard row of 112 positions before and after
        ld, guard = 96, 112 * 96
        m = B * To * 112 * 112 * ld
        obuf = torch.empty((m + 2 * guard,), dtype=torch.bfloat16, device="cuda")
        obuf.view(torch.int16).fill_(NAN_BITS)
        out = obuf[guard:guard + m].view(B, To, 112, 112, ld)
    else:
        xbuf = obuf = None
        xg = xu.cuda()
        out = torch.empty((B, To, 112, 112, 64), dtype=torch.bfloat16, device="cuda")
        out.view(torch.int16).fill_(NAN_BITS)

    dg = delta.cuda()
    a = ops.make_apply_args(xg, dg, fold_t=ops.I3D_FOLD, center=True, dclip_dev=None if dev is None else dev.cuda(), **kw)
    if decode[0] is not None:
        a.x_scale, a.x_bias = decode
    assert a.delta_per_clip == int(bool(c.get("per_clip")))
    tab = ops.stem_delta_bias_table(a, w7.numpy(), scale.numpy()) if c.get("table", True) else None
    if c.get("per_clip"):
        assert tab.shape[0] == B                                         # one table per clip: pos_bias_bstride != 0
    w = ops.StemFwdU8Weights(w7.numpy())
    sg, bg = scale.cuda(), bias.cuda()
    ops.stem_fwd_u8(a, w, sg, bg, tab, out=out)
    torch.cuda.synchronize()
    got = out.cpu()
    differ = bits(got[..., :64]) != bits(want)
    if bool(differ.any()):
        i = tuple(int(v) for v in differ.nonzero()[0])
        raise AssertionError(f"{int(differ.sum())} of {differ.numel()} outputs differ from the float64 oracle, the first at {i}: "
                             f"kernel {float(got[i])}, oracle {float(want[i])}")
    if c.get("embedded"):
        assert bool((bits(got[..., 64:]) == NAN_BITS).all()), "channels 64..95 were written"
        ob = bits(obuf)
        assert bool((ob[:guard] == NAN_BITS).all()) and bool((ob[-guard:] == NAN_BITS).all()), "a guard row was written"
        xb = xbuf.cpu()
        assert bool((xb[:off] == 255).all()) and bool((xb[off + n:] == 255).all())
    # a second run gives the same bits
    out2 = torch.empty_like(out)
    out2.view(torch.int16).fill_(NAN_BITS)
    ops.stem_fwd_u8(a, w, sg, bg, tab, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(bits(out2), bits(got))


# ---- 2. rounding cases ----------------------------------------------------------------------------------------------------------------
ROUNDING = {
    "shared_T10": dict(B=1, T=10, per_clip=False, dclip_dev=None),
    "per_clip": dict(B=2, T=4, per_clip=True, dclip_dev=(0.4, 0.23)),
}


@pytest.mark.parametrize("name", list(ROUNDING))
def test_rounding(ops, name):
    c = ROUNDING[name]
    B, T = c["B"], c["T"]
    rng = np.random.default_rng(211 + B)
    xu = torch.from_numpy(rng.integers(0, 256, (B, T, 224, 224, 3), dtype=np.uint8))
    xu[:, :, :8] = 0                      # saturated bands: the clip to [lo, hi] is active there
    xu[:, :, -8:] = 255
    delta = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, T, 3) if c["per_clip"] else (T, 3)).astype(np.float32))
    w7 = torch.from_numpy((rng.standard_normal((7, 7, 7, 3, 64)) * (2.0 / 1029) ** 0.5).astype(np.float32))
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, 64).astype(np.float32))
    bias = torch.from_numpy(rng.uniform(-0.3, 0.3, 64).astype(np.float32))
    dev = None if c["dclip_dev"] is None else torch.tensor(c["dclip_dev"], dtype=torch.float32)
    kw = dict(dclip=0.4, lo=-0.9, hi=0.95, inv_std=(1.0 / 0.9, 1.0 / 1.1, 1.0 / 0.7))
    xc, p, w_clip, w_pert = so.kernel_operands(xu, delta, w7, scale, dclip_dev=dev, **kw)
    active = float((xc != xu.float() / 128 - 1).float().mean())
    assert 0.02 < active < 0.9, active                                   # the clamp matters, and not everywhere

    a = ops.make_apply_args(xu.cuda(), delta.cuda(), fold_t=ops.I3D_FOLD, center=True, dclip_dev=None if dev is None else dev.cuda(), **kw)
    tab = ops.stem_delta_bias_table(a, w7.numpy(), scale.numpy())
    out = ops.stem_fwd_u8(a, ops.StemFwdU8Weights(w7.numpy()), scale.cuda(), bias.cuda(), tab)
    torch.cuda.synchronize()
    got = out.cpu()
    ref = so.stem_oracle(xc, p, w_clip, w_pert, scale, bias)
    s = float(ref.abs().max())
    print(f"[{name}] clamp active on {active:.1%}; max abs err / output scale = {float((got.double() - ref).abs().max()) / s:.2e} (scale {s:.3f})")
    worst, _ = so.stem_bound_ratio(got, xc, p, w_clip, w_pert, scale, bias, ref=ref)
    print(f"[{name}] worst |y - r| / derived bound = {worst:.3f}")


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def _folded(w7):
    wf = np.zeros((4, 4, 4, 32, 64), np.float32)
    for kt in range(7):
        for kh in range(7):
            for kw in range(7):
                ch = ((kt & 1) * 2 + (kh & 1)) * 8 + (kw & 1) * 3
                wf[kt >> 1, kh >> 1, kw >> 1, ch:ch + 3] = w7[kt, kh, kw]
    return wf


REFUSALS = {
    # name: (what differs from a valid call, what flk_last_error() must name)
    "H_222": (dict(shape=(1, 2, 222, 224, 3)), "224"),
    "W_222": (dict(shape=(1, 2, 224, 222, 3)), "224"),
    "odd_T": (dict(shape=(1, 3, 224, 224, 3)), "even T"),
    "fp32_clip": (dict(xdtype=torch.float32), "uint8"),
    "center_0": (dict(center=False), "center"),
    "dense_delta": (dict(dense=True), "flicker"),
    "lo_above_hi": (dict(lo=0.5, hi=-0.5), "lo > hi"),
    "out_ld_60": (dict(out_ld=60), "out_ld"),
    "out_ld_68": (dict(out_ld=68), "out_ld"),
    "clip_offset_4": (dict(offset=4), "8-byte aligned"),
    "s2d_stem_weights": (dict(folded=True), "weights"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refuses(ops, name):
    from flickering_adversarial_video_amd._lib import ptr, stream_ptr
    lib = ops.load()
    how, field = REFUSALS[name]
    shape = how.get("shape", (1, 2, 224, 224, 3))
    B, T, H, Wd, _ = shape
    n = int(np.prod(shape))
    off = how.get("offset", 0)
    xbuf = torch.zeros((n + 8,), dtype=how.get("xdtype", torch.uint8), device="cuda")
    x = xbuf[off:off + n].view(shape)
    delta = torch.zeros((T, H, Wd, 3) if how.get("dense") else (T, 3), dtype=torch.float32, device="cuda")
    a = ops.make_apply_args(x, delta, fold_t=ops.I3D_FOLD, center=how.get("center", True), lo=how.get("lo", -1.0), hi=how.get("hi", 1.0))
    w7, scale, bias = dyadic_weights()
    w = ops.ConvWeights.s2d_stem(_folded(w7.numpy()), torch.bfloat16, 4) if how.get("folded") else ops.StemFwdU8Weights(w7.numpy())
    sg, bg = scale.cuda(), bias.cuda()
    out = torch.empty((B * max(T // 2, 1) * 112 * 112 * 96,), dtype=torch.bfloat16, device="cuda")
    out.view(torch.int16).fill_(NAN_BITS)
    torch.cuda.synchronize()
    rc = lib.flk_stem_fwd_u8(C.byref(a), w.handle, ptr(sg), ptr(bg), None, 0, ptr(out), how.get("out_ld", 64), stream_ptr())
    msg = lib.flk_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    assert rc == FLK_EINVAL, (rc, msg)
    assert "flk_stem_fwd_u8" in msg and field in msg, msg
    assert bool((bits(out) == NAN_BITS).all()), "a refused call wrote to the output"
