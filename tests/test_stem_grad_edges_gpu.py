"""The fused stem delta-gradient (csrc/stem_grad.hip: flk_stem_delta_grad) at the chunkings it really runs, and at its edges (GPU).

Every case first asserts, through the host-only query flk_stem_delta_grad_chunks, the chunking it claims to cover (the query's own
values are pinned in tests/test_stem_grad_contract_cpu.py), then holds the kernel to the reference of
tests/test_kernels_gpu.py::test_stem_delta_grad_fused: fp64 on the CPU,
    x_adv = clamp(roll(x) + adv_flag * roll(clamp(delta, +-dclip) * inv_std), lo, hi),   y = conv3d(x_adv, W * bn_scale), TF SAME, stride 2,
    ref   = autograd.grad(y, delta, grad_outputs = G)          (delta [T,3], or [B,T,3] for per-clip perturbations)
with G bf16 on both sides and the weights fp32.  The clip keeps that test's construction (columns [:20] = 0 and [200:] = 255, delta from
+-0.5 so that some entries lie beyond dclip): the mask is neither all-pass nor trivial.

Bound: max|got - ref| / max|ref| < 2e-5 per case (per clip row for per-clip perturbations) -- the bar test_stem_delta_grad_fused holds this
kernel to; nothing here is a new measurement.  With a dense random G one missing 8-position group moves an entry by ~1e-2 of its size,
and in `sparse_seams` a dropped or doubled group is the whole signal.  Bitwise claims: g_ld = 128 with NaN in channels 64..127 against
g_ld = 64; a per-clip row against the batch-1 call on that clip; mask pre-pass + mask_done = 1 against the one-call form; run to run.

The scalars the kernel receives as fp32 (dclip, inv_std, lo, hi) enter the reference as those fp32 values.  A pixel whose clip mask is
decided by less than 1e-5 -- where the kernel's fp32 sum x + p and the fp64 one may legitimately fall on different sides of lo / hi --
is replaced in the INPUT (by mid-range) before either side sees it; with these seeds that is a handful of pixels of the fp32 clip.

Measured on an MI355X, max|got - ref| / max|ref|:
    one_chunk_long 1.38e-07   two_chunks_T90 1.44e-07   uneven_tail_oddB 6.85e-08   smallest H=2 1.20e-07, H=4 8.09e-08
    f32_torch_adv_half 1.00e-07   gld_128_nan 1.87e-07   sparse_seams 8.66e-08   per_clip 1.75e-07 (worst clip row)
(two runs, the same figures: the kernel is deterministic); every bitwise claim held."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-5
W = 224


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def stem_weights():
    rng = np.random.default_rng(17)
    w7 = (rng.standard_normal((7, 7, 7, 3, 64)) * 0.05).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, 64).astype(np.float32)
    return w7, scale


@pytest.fixture(scope="module")
def wts(ops):
    return ops.StemDeltaGradWeights(*stem_weights())


def f32(v):
    """the value a float takes as an fp32 kernel argument"""
    return float(np.float32(v))


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def perturbation(delta, dclip, inv_std, adv, sp):
    """adv_flag * roll(clamp(delta, +-dclip) * inv_std) in the dtype of delta (fp64): [1 or B, T, 3].  dclip: a float, or fp32 [B]"""
    T = delta.shape[-2]
    bound = dclip.double().view(-1, 1, 1) if torch.is_tensor(dclip) else torch.tensor(f32(dclip), dtype=torch.float64)
    p = torch.clamp(delta, min=-bound, max=bound) * torch.tensor([f32(s) for s in inv_std], dtype=torch.float64)
    p = p.view(-1, T, 3)
    return adv * (torch.roll(p, sp, 1) if sp else p)


def decode(x):
    return x.double() / 128 - 1 if x.dtype == torch.uint8 else x.double()


def settle(x, delta, *, dclip, inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0, adv=1.0, sx=0, sp=0):
    """replace (in place) the pixels of the clip whose mask is decided by less than 1e-5; returns how many"""
    p = perturbation(delta.double(), dclip, inv_std, adv, sp)
    xf = decode(x)
    u = (torch.roll(xf, sx, 1) if sx else xf) + p.view(-1, x.shape[1], 1, 1, 3)
    bad = (u - f32(lo)).abs_() < 1e-5
    bad |= u.sub_(f32(hi)).abs_() < 1e-5
    if sx:
        bad = torch.roll(bad, -sx, 1)
    x[bad] = 128 if x.dtype == torch.uint8 else 0.0
    return int(bad.sum())


def reference(x, delta, G, *, dclip, inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0, adv=1.0, sx=0, sp=0, forward_conv=False):
    """fp64 d(loss)/d(delta), the shape of delta: the reference of test_stem_delta_grad_fused.  forward_conv: literally that test's
    graph, autograd.grad(conv3d(x_adv), delta, grad_outputs = G).  Default: the convolution is linear in x_adv, so the same gradient is
    autograd.grad(<x_adv, conv_transpose3d(G)>, delta) -- the transposed convolution autograd runs for the form above, without paying
    for the forward convolution (half the time at the two large cases); test_smallest and test_uneven_tail_oddB hold the two forms together."""
    w7, scale = stem_weights()
    T, H = x.shape[1:3]
    d = delta.double().requires_grad_(True)
    p = perturbation(d, dclip, inv_std, adv, sp)
    xf = decode(x)
    xa = ((torch.roll(xf, sx, 1) if sx else xf) + p.view(-1, T, 1, 1, 3)).clamp(f32(lo), f32(hi))
    wt = torch.from_numpy(w7 * scale).double().permute(4, 3, 0, 1, 2).contiguous()           # [co, c, kt, kh, kw]
    Gd = G[..., :64].double().permute(0, 4, 1, 2, 3)                                          # [B,64,To,Ho,Wo]
    if forward_conv:
        xp = F.pad(xa.permute(0, 4, 1, 2, 3), (2, 3, 2, 3, 2, 3))                             # TF SAME for k 7, s 2 on even sizes
        y = F.conv3d(xp, wt, None, stride=2)
        (ref,) = torch.autograd.grad(y, d, grad_outputs=Gd)
    else:
        gx = F.conv_transpose3d(Gd, wt, None, stride=2)[:, :, 2:2 + T, 2:2 + H, 2:2 + W]      # the gradient of the padded clip, pad 2 in front cut off
        (ref,) = torch.autograd.grad((xa * gx.permute(0, 2, 3, 4, 1)).sum(), d)
    return ref


def assert_reference_forms_agree(x, delta, G, **kw):
    a, b = reference(x, delta, G, **kw), reference(x, delta, G, forward_conv=True, **kw)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def clip_u8(rng, B, T, H):
    xu = torch.from_numpy(rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8))
    xu[:, :, :, :20] = 0                            # dark / bright bands: pixels that saturate as soon as delta has the right sign
    xu[:, :, :, 200:] = 255
    return xu


def dense_G(rng, B, T, H):
    To, Ho = T // 2, H // 2
    G = torch.from_numpy(rng.standard_normal((B, To, Ho, W // 2, 64)).astype(np.float32)).to(torch.bfloat16)
    if Ho >= 12:                                    # some structure: zero rows, one strong row
        G[:, :, 5:9] = 0
        G[:, :, Ho - 4] *= 8
    return G


def flicker(rng, *shape):
    return torch.from_numpy(rng.uniform(-0.5, 0.5, shape).astype(np.float32))       # some entries beyond the clamp


def assert_chunking(ops, B, T, H, want, per_clip=False):
    """want = (nchunk, rows per chunk, rows of the last chunk)"""
    n, rows = ops.stem_delta_grad_chunks(B, T, H, per_clip)
    assert (n, rows, H // 2 - (n - 1) * rows) == want, (n, rows)


def compare(name, got, ref):
    got = got.detach().cpu().double()
    scale = ref.abs().amax(dim=(-2, -1), keepdim=True)                # one [T,3] (per clip row for [B,T,3])
    assert bool((scale > 0).all()) and bool(torch.isfinite(got).all())
    err = float(((got - ref).abs() / scale).max())
    print(f"[{name}] fused stem delta-gradient: max-rel {err:.2e} (|ref| max {float(ref.abs().max()):.3e})")
    assert err < TOL
    return err


def run_dense(ops, wts, name, B, T, H, want, seed):
    """a dense random G on a uint8 clip, TF dialect: chunking, bound, exact zeros of the clamped entries"""
    assert_chunking(ops, B, T, H, want)
    rng = np.random.default_rng(seed)
    x, delta, G = clip_u8(rng, B, T, H), flicker(rng, T, 3), dense_G(rng, B, T, H)
    settle(x, delta, dclip=0.4)
    args = ops.make_apply_args(x.cuda(), delta.cuda(), dialect="tf", dclip=0.4, fold_t=ops.I3D_FOLD)
    got = ops.stem_delta_grad(args, G.cuda(), wts).cpu()
    compare(name, got, reference(x, delta, G, dclip=0.4))
    if B * T * H <= 3 * 6 * 38:
        assert_reference_forms_agree(x, delta, G, dclip=0.4)
    clipped = delta.abs() > f32(0.4)
    if clipped.any():
        assert float(got[clipped].abs().max()) == 0.0


def test_one_chunk_long(ops, wts):
    """the product chunking of bs 8 x T 64: ONE chunk per (clip, frame pair).  24 output rows = 336 groups = 84 K steps, 53 mask rows: the G
    buffers repeat every 4 steps, a row of 14 groups spans 3.5 steps, the 16-slot ring covers 8 output rows = 28 steps -- 84 steps run
    three full periods of every phase the 392-step loop of H = 224 has"""
    run_dense(ops, wts, "one_chunk_long", 8, 64, 48, (1, 24, 24), 101)


def test_two_chunks_T90(ops, wts):
    """the product chunking of the reference's T = 90 at bs 8: two chunks, odd To = 45, and an odd row count -- 13 rows = 182 groups, so
    the last K step is half padding"""
    run_dense(ops, wts, "two_chunks_T90", 8, 90, 52, (2, 13, 13), 102)


def test_uneven_tail_oddB(ops, wts):
    """19 output rows in 10 chunks of 2: the last chunk has ONE row; odd batch"""
    run_dense(ops, wts, "uneven_tail_oddB", 3, 6, 38, (10, 2, 1), 103)


@pytest.mark.parametrize("H,want", [(2, (1, 1, 1)), (4, (2, 1, 1))], ids=["H2", "H4"])
def test_smallest(ops, wts, H, want):
    """To = 1: one of the four G planes exists; Ho = 1, 2: most mask rows of a window come from the zero page; nsteps = 4 is fewer K steps
    than the producer's look-ahead reaches"""
    run_dense(ops, wts, f"smallest H={H}", 1, 2, H, want, 104 + H)


def test_f32_torch_adv_half(ops, wts):
    """the fp32 mask path and both rolls at a new shape; adv_flag = 0.5 enters the mask AND the scale of the result"""
    from oracle import attack_math as am
    B, T, H = 3, 6, 38
    assert_chunking(ops, B, T, H, (10, 2, 1))
    rng = np.random.default_rng(110)
    x = torch.from_numpy(rng.uniform(-2.2, 2.9, (B, T, H, W, 3)).astype(np.float32))          # beyond [lo, hi] on both sides
    delta, G = flicker(rng, T, 3), dense_G(rng, B, T, H)
    kw = dict(dclip=0.2, inv_std=tuple(1.0 / s for s in am.DEFAULT_STD), lo=am.TORCH_MIN_VALUE, hi=am.TORCH_MAX_VALUE)
    n = settle(x, delta, adv=0.5, sx=2, sp=5, **kw)
    print(f"[f32_torch_adv_half] {n} of {x.numel()} pixels within 1e-5 of a clip bound replaced")
    assert n < 100
    args = ops.make_apply_args(x.cuda(), delta.cuda(), dialect="torch", adv_flag=0.5, shift_x=2, shift_p=5, fold_t=ops.I3D_FOLD, **kw)
    got = ops.stem_delta_grad(args, G.cuda(), wts).cpu()
    compare("f32_torch_adv_half", got, reference(x, delta, G, adv=0.5, sx=2, sp=5, **kw))
    assert_reference_forms_agree(x, delta, G, adv=0.5, sx=2, sp=5, **kw)
    clipped = delta.abs() > f32(0.2)
    assert clipped.any() and float(got[clipped].abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def case_2_8_36():
    rng = np.random.default_rng(120)
    x, delta, G = clip_u8(rng, 2, 8, 36), flicker(rng, 8, 3), dense_G(rng, 2, 8, 36)
    settle(x, delta, dclip=0.4)
    return x, delta, G


def test_gld_128_nan(ops, wts):
    """g_ld != 64: G as the first 64 of 128 channels, the others all NaN -- nothing beyond channel 63 may be read"""
    B, T, H = 2, 8, 36
    assert_chunking(ops, B, T, H, (9, 2, 2))
    x, delta, G = case_2_8_36()
    G128 = torch.cat([G, torch.full_like(G, float("nan"))], -1).contiguous()
    assert G128.shape[-1] == 128 and bool(torch.isnan(G128[..., 64:]).all())
    args = ops.make_apply_args(x.cuda(), delta.cuda(), dialect="tf", dclip=0.4, fold_t=ops.I3D_FOLD)
    g64 = ops.stem_delta_grad(args, G.cuda(), wts).cpu()
    g128 = ops.stem_delta_grad(args, G128.cuda(), wts).cpu()
    assert bool(torch.isfinite(g128).all())
    assert torch.equal(bits(g128), bits(g64))
    compare("gld_128_nan", g128, reference(x, delta, G, dclip=0.4))


def test_sparse_seams(ops, wts):
    """G zero except at 24 positions on chunk seams and frame edges (oh), 8-group seams (ow), the first and last output frame, both
    clips -- each with a random 64-vector: a dropped or doubled group at a seam is the whole signal"""
    B, T, H = 2, 8, 224
    assert_chunking(ops, B, T, H, (16, 7, 7))
    To = T // 2
    rng = np.random.default_rng(130)
    x, delta = clip_u8(rng, B, T, H), flicker(rng, T, 3)
    settle(x, delta, dclip=0.4)
    G = torch.zeros((B, To, H // 2, W // 2, 64), dtype=torch.bfloat16)
    pos = [(i % 2, (0, To - 1)[(i // 2) % 2], oh, ow) for i, (oh, ow) in enumerate((oh, ow) for oh in (0, 6, 7, 13, 111) for ow in (0, 7, 8, 111))]
    pos += [(1, To - 1, 0, 0), (0, 0, 111, 111), (1, 0, 7, 8), (0, To - 1, 6, 7)]         # seams in the other clip / output frame too
    assert len(set(pos)) == 24
    for b, ot, oh, ow in pos:
        G[b, ot, oh, ow] = torch.from_numpy(rng.standard_normal(64).astype(np.float32)).to(torch.bfloat16)
    args = ops.make_apply_args(x.cuda(), delta.cuda(), dialect="tf", dclip=0.4, fold_t=ops.I3D_FOLD)
    got = ops.stem_delta_grad(args, G.cuda(), wts).cpu()
    compare("sparse_seams", got, reference(x, delta, G, dclip=0.4))
    clipped = delta.abs() > f32(0.4)
    assert clipped.any() and float(got[clipped].abs().max()) == 0.0


def test_per_clip(ops, wts):
    """per-clip perturbations (delta [B,T,3], per-clip clamp bounds on the device): (a) each clip row against the fp64 reference;
    (b) row b BITWISE the batch-1 call on clip b with delta[b] and dclip = dclip_dev[b] -- per clip the chunking is the batch-1 call's;
    (c) entries beyond that clip's bound are exactly 0, at least one in each clip"""
    B, T, H = 3, 8, 36
    assert_chunking(ops, B, T, H, (9, 2, 2), per_clip=True)
    assert ops.stem_delta_grad_chunks(B, T, H, True) == ops.stem_delta_grad_chunks(1, T, H, False)
    rng = np.random.default_rng(140)
    x, delta, G = clip_u8(rng, B, T, H), flicker(rng, B, T, 3), dense_G(rng, B, T, H)
    bounds = torch.tensor([0.4, 0.2, 0.45], dtype=torch.float32)
    settle(x, delta, dclip=bounds)
    xd, Gd = x.cuda(), G.cuda()
    args = ops.make_apply_args(xd, delta.cuda(), dialect="tf", dclip=0.4, dclip_dev=bounds.cuda(), fold_t=ops.I3D_FOLD)
    assert args.delta_per_clip == 1
    got = torch.empty((B, T, 3), dtype=torch.float32, device="cuda")
    ops.stem_delta_grad(args, Gd, wts, gdelta=got)
    got = got.cpu()
    compare("per_clip", got, reference(x, delta, G, dclip=bounds))
    assert_reference_forms_agree(x, delta, G, dclip=bounds)
    for b in range(B):
        a1 = ops.make_apply_args(xd[b:b + 1].contiguous(), delta[b].contiguous().cuda(), dialect="tf", dclip=float(bounds[b]), fold_t=ops.I3D_FOLD)
        assert a1.delta_per_clip == 0 and a1.B == 1
        one = ops.stem_delta_grad(a1, Gd[b:b + 1].contiguous(), wts).cpu()
        assert torch.equal(bits(got[b]), bits(one)), b
        clipped = delta[b].abs() > bounds[b]
        assert clipped.any() and float(got[b][clipped].abs().max()) == 0.0
        assert float(got[b][~clipped].abs().min()) > 0.0


def test_mask_done(ops, wts):
    """flk_stem_delta_grad_mask, then flk_stem_delta_grad(..., mask_done = 1): bitwise the one-call form; the one-call form run to run"""
    from flickering_adversarial_video_amd._lib import check, ptr, stream_ptr
    lib = ops.load()
    B, T, H = 2, 8, 36
    x, delta, G = case_2_8_36()
    Gd = G.cuda()
    args = ops.make_apply_args(x.cuda(), delta.cuda(), dialect="tf", dclip=0.4, fold_t=ops.I3D_FOLD)
    nfl = lib.flk_stem_delta_grad_scratch_bytes(B, T, H) // 4

    def run(split):
        scratch = torch.full((nfl,), float("nan"), dtype=torch.float32, device="cuda")       # nothing left over from another run
        gd = torch.full((T, 3), float("nan"), dtype=torch.float32, device="cuda")
        if split:
            check(lib.flk_stem_delta_grad_mask(C.byref(args), ptr(scratch), stream_ptr()))
        check(lib.flk_stem_delta_grad(C.byref(args), ptr(Gd), 64, wts.handle, ptr(gd), ptr(scratch), int(split), stream_ptr()))
        return gd.cpu()

    one, again, two = run(False), run(False), run(True)
    assert bool(torch.isfinite(one).all()) and float(one.abs().max()) > 0.0
    assert torch.equal(bits(one), bits(again))
    assert torch.equal(bits(one), bits(two))
    assert torch.equal(bits(one), bits(ops.stem_delta_grad(args, Gd, wts)))
