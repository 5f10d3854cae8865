"""The perturbation kernels of csrc/attack.hip where their loops iterate: chunk seams and second trips of the delta-gradient reduction,
the dense gradient, the apply kernel beyond its grid cap, the dense L12 update where both stride loops run, the one-workgroup flicker
update at the edges of T, and clips that are not 8-byte aligned.

A and B are EXACT: the clip gradient holds integers in [-8, 8], so every fp32 partial sum of the kernels is an integer below 2^24 and
the result cannot depend on the summation order; it must equal oracle/perturb_ref.py (numpy, int64 sums, the pass mask taken from the
same float32 u = x' + p' the kernels compare with the bounds -- itself checked by tests/test_perturb_ref_cpu.py).  Each of those
tests first asserts, from the reference alone, the conditions that make it meaningful: the pass share lies in (0.5, 0.95), at least
one delta row is zeroed by the delta clip, and sum |g| per output stays below 2^24."""
import numpy as np
import pytest
import torch

from oracle import attack_math as am
from oracle import perturb_ref as pr

pytestmark = pytest.mark.gpu

TORCH_KW = dict(inv_std=tuple(1.0 / s for s in am.DEFAULT_STD), lo=am.TORCH_MIN_VALUE, hi=am.TORCH_MAX_VALUE)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


# ---- layouts (s2d, s2d_aligned, un_s2d: tests/test_attack_gpu.py) -------------------------------------------------------------------
def s2d(x):
    """[B,T,H,W,3] -> [B,T/2,H/2,W/2,32], channel (qt*4+qh*2+qw)*3+c, 24..31 zero (include/flicker_hip.h)"""
    B, T, H, W, _ = x.shape
    y = x.reshape(B, T // 2, 2, H // 2, 2, W // 2, 2, 3).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B, T // 2, H // 2, W // 2, 24)
    return torch.cat([y, torch.zeros(*y.shape[:4], 8, dtype=x.dtype)], -1)


def s2d_aligned(x):
    """fold_t = 3: channel (qt*2+qh)*8 + qw*3 + c, 6 and 7 of every 8 zero (one (qt,qh) parity per 16-byte chunk)"""
    B, T, H, W, _ = x.shape
    y = x.reshape(B, T // 2, 2, H // 2, 2, W // 2, 2, 3).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B, T // 2, H // 2, W // 2, 4, 6)
    return torch.cat([y, torch.zeros(*y.shape[:5], 2, dtype=x.dtype)], -1).reshape(B, T // 2, H // 2, W // 2, 32)


def s2d_hw(x):
    """fold_t = 1 (and the gradient layout of fold_t = 4): [B,T,H/2,W/2,16], channel (qh*2+qw)*3+c, 12..15 zero"""
    B, T, H, W, _ = x.shape
    y = x.reshape(B, T, H // 2, 2, W // 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, T, H // 2, W // 2, 12)
    return torch.cat([y, torch.zeros(*y.shape[:4], 4, dtype=x.dtype)], -1)


def fold(x, fold_t):
    return {1: s2d_hw, 4: s2d_hw, 2: s2d, 3: s2d_aligned}[fold_t](x)


def decode_table():
    from flickering_adversarial_video_amd.videoresnet_spec import u8_decode_table
    return u8_decode_table()


# ---- A. delta gradient, exact -------------------------------------------------------------------------------------------------------
def grad_nchunk(B, T, H):
    """csrc/attack.hip grad_nchunk, restated: workgroups per (clip, folded frame) of stage 1 (rows H/2 split as H2*k/n)"""
    bt, H2 = B * max(T // 2, 1), H // 2
    return max(1, min((1024 + bt - 1) // bt, H2))


def seams(B, T, H, W, per_clip=False):
    n, H2, W2 = grad_nchunk(1 if per_clip else B, T, H), H // 2, W // 2
    rows = [H2 * (k + 1) // n - H2 * k // n for k in range(n)]
    return n, rows, sorted({r * W2 for r in rows})


def grad_inputs(shape, seed, per_clip=False):
    B, T, H, W = shape
    rng = np.random.default_rng(seed)
    xu = rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    g = rng.integers(-8, 9, (B, T, H, W, 3)).astype(np.float32)
    d = rng.uniform(-0.6, 0.6, (B, T, 3) if per_clip else (T, 3)).astype(np.float32)
    return xu, g, d


def meaningful(x, d, g, kw, what):
    """the conditions of an exact gradient test, from the reference alone; returns the reference gradient"""
    mask = pr.pass_mask(x, d, **kw)
    share = float(mask.mean())
    dense = d.ndim == 4
    axes = (0,) if dense else (2, 3) if d.ndim == 3 else (0, 2, 3)
    worst = float(np.abs(g).sum(axis=axes).max())
    dc = kw.get("dclip_dev")
    dc = np.asarray(dc, np.float32).reshape(-1, 1, 1) if dc is not None else np.float32(kw.get("dclip", 0.4))
    zeroed = float(((dc > 0) & (np.abs(d) > dc)).mean())
    print(f"{what}: pass share {share:.3f}, max sum|g| per output {worst:.0f}, {zeroed:.1%} of the delta rows zeroed")
    assert 0.5 < share < 0.95 and worst < 2 ** 24
    assert zeroed > 0 or not np.any(dc > 0)
    return torch.from_numpy(pr.delta_grad_ref(x, d, g, **kw))


def check_grad(ops, x_dev, d, g, fold_ts, ref, make_kw, what):
    for ft in fold_ts:
        args = ops.make_apply_args(x_dev, torch.from_numpy(d).cuda(), fold_t=ft, **make_kw)
        gl = fold(torch.from_numpy(g), ft)
        for gdev in (gl.cuda(), gl.bfloat16().cuda()):          # integers up to 8 are bf16 numbers
            got = ops.perturb_grad_reduce(args, gdev).cpu()
            bad = int((got != ref).sum())
            assert torch.equal(got, ref), f"{what} fold_t {ft} {gdev.dtype}: {bad} of {ref.numel()} outputs differ, max {float((got - ref).abs().max())}"


def test_grad_seams_fold2_fold3_u8(ops):
    """(3,100,44,180), shifts (3, 5): 7 chunks of 3,3,3,3,3,3,4 row pairs -> 270 / 360 cells per workgroup (two trips, ragged waves)"""
    shape = (3, 100, 44, 180)
    assert seams(*shape) == (7, [3, 3, 3, 3, 3, 3, 4], [270, 360])
    xu, g, d = grad_inputs(shape, 11)
    kw = dict(dclip=0.4, shift_x=3, shift_p=5)
    ref = meaningful(xu, d, g, kw, "A1")
    check_grad(ops, torch.from_numpy(xu).cuda(), d, g, (2, 3), ref, kw, "A1")


def test_grad_seams_fold2_w_not_multiple_of_8(ops):
    """(2,172,22,260), shifts (-3, T+5): 6 chunks of 1,2,2,2,2,2 row pairs -> 130 / 260 cells; W % 8 != 0"""
    shape = (2, 172, 22, 260)
    assert seams(*shape) == (6, [1, 2, 2, 2, 2, 2], [130, 260]) and shape[3] % 8
    xu, g, d = grad_inputs(shape, 12)
    kw = dict(dclip=0.4, shift_x=-3, shift_p=shape[1] + 5)
    ref = meaningful(xu, d, g, kw, "A2")
    check_grad(ops, torch.from_numpy(xu).cuda(), d, g, (2,), ref, kw, "A2")


@pytest.mark.parametrize("src", ["f32in", "u8-table"])
def test_grad_seams_fold1_fold4_torch_dialect(ops, src):
    """(4,64,22,260), torch dialect: 8 uneven chunks (1,1,2,1,1,2,1,2 row pairs); an fp32 clip, and a uint8 clip through x_lut"""
    shape = (4, 64, 22, 260)
    assert seams(*shape) == (8, [1, 1, 2, 1, 1, 2, 1, 2], [130, 260])
    xu, g, d = grad_inputs(shape, 13)
    lut = decode_table()
    kw = dict(dclip=0.4, **TORCH_KW)
    if src == "u8-table":
        x, x_dev, mk = xu, torch.from_numpy(xu).cuda(), dict(kw, dialect="torch", x_lut=torch.from_numpy(lut).cuda())
        kw = dict(kw, x_lut=lut)
    else:
        x = lut[xu, np.arange(3)]                                   # the same values as an fp32 clip
        x_dev, mk = torch.from_numpy(x).cuda(), dict(kw, dialect="torch")
    ref = meaningful(x, d, g, kw, f"A3 {src}")
    check_grad(ops, x_dev, d, g, (1, 4), ref, mk, f"A3 {src}")


def test_grad_seams_per_clip(ops):
    """(3,100,112,40), delta [B,T,3] with one clamp bound per clip: the chunking of a batch-1 call, 21 chunks over 56 row pairs"""
    shape = (3, 100, 112, 40)
    n, rows, cells = seams(*shape, per_clip=True)
    assert n == 21 and sum(rows) == 56 and sorted(set(rows)) == [2, 3]
    xu, g, d = grad_inputs(shape, 14, per_clip=True)
    bounds = np.array([0.4, 0.3, 0.5], np.float32)
    ref = meaningful(xu, d, g, dict(dclip_dev=bounds), "A4")
    check_grad(ops, torch.from_numpy(xu).cuda(), d, g, (1,), ref, dict(dclip_dev=torch.from_numpy(bounds).cuda()), "A4")


@pytest.mark.parametrize("shape", [(1, 1, 8, 8), (2, 5, 6, 10)], ids=["T1", "T5"])
def test_grad_degenerate_T(ops, shape):
    """fold_t = 1 at T = 1 and at an odd T: grad_nchunk's T / 2 is 0 resp. rounds down; shifts fold onto the clip"""
    xu, g, d = grad_inputs(shape, 15 + shape[1])
    d[0, 0] = 0.55                                                  # a zeroed row at every size
    kw = dict(dclip=0.4, shift_x=2, shift_p=-1)
    ref = meaningful(xu, d, g, kw, f"A5 {shape}")
    check_grad(ops, torch.from_numpy(xu).cuda(), d, g, (1,), ref, kw, f"A5 {shape}")


def test_grad_nchunk_restatement_is_the_librarys(ops):
    """flk_perturb_grad_scratch_bytes = B * T * grad_nchunk(1, T, H) * 6 floats: the restatement above is what the library computes"""
    from flickering_adversarial_video_amd import _lib
    for B, T, H, W in ((3, 100, 44, 180), (2, 172, 22, 260), (4, 64, 22, 260), (3, 100, 112, 40), (1, 1, 8, 8), (2, 5, 6, 10), (8, 64, 224, 224)):
        assert _lib.load().flk_perturb_grad_scratch_bytes(B, T, H, W) == B * T * grad_nchunk(1, T, H) * 6 * 4
    assert grad_nchunk(8, 64, 224) == 4                             # the workload: 4 chunks of 28 row pairs x 112 cells


# ---- B. dense gradient, exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dclip", [0.0, 0.4])
def test_dense_grad_exact(ops, dclip):
    B, T, H, W = 3, 6, 10, 14
    rng = np.random.default_rng(21)
    xu = rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    g = rng.integers(-8, 9, (B, T, H, W, 3)).astype(np.float32)
    d = rng.uniform(-0.6, 0.6, (T, H, W, 3)).astype(np.float32)
    kw = dict(dclip=dclip, shift_x=1, shift_p=4)
    ref = meaningful(xu, d, g, kw, f"B dclip {dclip}")
    check_grad(ops, torch.from_numpy(xu).cuda(), d, g, (1, 2, 3), ref, kw, f"B dclip {dclip}")


# ---- C. apply beyond the grid cap ---------------------------------------------------------------------------------------------------
def test_apply_strides_beyond_the_grid_cap(ops):
    """apply_s2d_kernel caps its grid at 16384 workgroups and strides over the rest: (4,33,360,360), fold_t = 1, is 4,276,800
    positions against 16384 * 256 = 4,194,304.  bf16 output against the reference rounded to bf16, atol = 0"""
    B, T, H, W = 4, 33, 360, 360
    assert B * T * (H // 2) * (W // 2) > 16384 * 256
    rng = np.random.default_rng(31)
    xu = rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    d = rng.uniform(-0.6, 0.6, (T, 3)).astype(np.float32)
    args = ops.make_apply_args(torch.from_numpy(xu).cuda(), torch.from_numpy(d).cuda(), dclip=0.4, fold_t=1)
    out = ops.perturb_apply_s2d(args, torch.bfloat16)
    want = s2d_hw(torch.from_numpy(pr.apply_ref(xu, d, dclip=0.4)).bfloat16())
    assert tuple(out.shape) == tuple(want.shape)
    got = out.cpu()
    tail = got.reshape(-1, 16)[16384 * 256:]
    assert tail.numel() > 0 and bool(tail[:, :12].float().abs().sum() > 0)         # the strided part was written
    torch.testing.assert_close(got.float(), want.float(), rtol=0, atol=0)


# ---- D. dense L12 Adam / PGD where both stride loops iterate ------------------------------------------------------------------------
def dense_update(xp, d, g, m, v, step, *, dialect, beta, dyn, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, pgd_eps=None):
    """the update formula of dense_adam_kernel in the precision ``xp`` (np.float32 | np.float64), every constant cast to it:
    g_tot = g + beta * d / (N_f * rms_t) where |d| <= dyn (or dyn = 0), rms_t = sqrt(mean clamp(d_t)^2); then Adam (TF-1.15 or
    torch-1.4 form) or, pgd_eps given, clamp(d - lr * sgn(g_tot), +-pgd_eps).  Returns (d', m', v', g_tot)"""
    c = xp
    d, g, m, v = d.astype(c), g.astype(c), m.astype(c), v.astype(c)
    fe = c(d[0].size)
    dcl = np.clip(d, -c(dyn), c(dyn)) if dyn > 0 else d
    rms = np.sqrt((dcl * dcl).reshape(d.shape[0], -1).sum(1, dtype=c) / fe).astype(c)
    rcoef = (c(beta) / (fe * rms)).astype(c).reshape(-1, 1, 1, 1)
    reg = (rcoef * d).astype(c)
    if dyn > 0:
        reg = np.where(np.abs(d) > c(dyn), c(0), reg)
    gt = (g + reg).astype(c)
    if pgd_eps is not None:
        return np.clip(d - c(lr) * np.sign(gt), -c(pgd_eps), c(pgd_eps)).astype(c), m, v, gt
    m = (c(b1) * m + (c(1) - c(b1)) * gt).astype(c)
    v = (c(b2) * v + (c(1) - c(b2)) * gt * gt).astype(c)
    bc1, bc2s = c(1) - c(b1) ** c(step), np.sqrt(c(1) - c(b2) ** c(step)).astype(c)
    if dialect == "torch":
        dn = d - (c(lr) / bc1) * m / (np.sqrt(v) / bc2s + c(eps))
    else:
        dn = d - (c(lr) * bc2s / bc1) * m / (np.sqrt(v) + c(eps))
    return dn.astype(c), m, v, gt


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("HW", [(2, 2), (36, 38), (150, 150)], ids=["n4=3", "n4=1026", "n4=16875"])
def test_dense_l12_update_where_the_stride_loops_iterate(ops, HW, T):
    """dense_frame_stats / dense_adam_kernel run 64 workgroups of 256 float4 lanes per frame: n4 = 3 leaves one wave of chunk 0 live,
    n4 = 1026 fills chunks 0-3 and gives chunk 4 two lanes, n4 = 16875 sends chunks 0 and 1 on a second trip.
    Scalars: delta holds multiples of 1/8 in [-3/8, 3/8] (no all-zero frame), so the three per-frame sums are exact in fp32 in any
    order; what is left is the division, the square root and the T-term sum: (T + 2) * 2^-24 < rtol = 1e-6 against fp64; max |d| is exact.
    Updated delta (two Adam steps in both dialects, one PGD step in both): the bound is MEASURED on the CPU, never against the kernel --
    the update formula (dense_update) evaluated in numpy float32 and in float64, largest difference over the steps, times 4 (powf and
    the operation order of the kernel).  Measured over the six cases: Adam 1.3e-8 .. 4.9e-8 -> bound 5.0e-8 .. 1.9e-7; PGD
    2.0e-9 .. 1.3e-8 -> bound 8.1e-9 .. 5.2e-8 (both printed per case, beside the kernel's own distance from fp64).  The fp32 and fp64 evaluations must agree on every sign of g_tot (asserted), so the PGD
    figure is one rounding of d - lr, not a flipped step."""
    H, W = HW
    n4 = H * W * 3 // 4
    assert H * W * 3 % 4 == 0 and n4 == {(2, 2): 3, (36, 38): 1026, (150, 150): 16875}[HW]
    rng = np.random.default_rng(41 + n4 + T)
    d0 = (rng.integers(-3, 4, (T, H, W, 3)) / 8.0).astype(np.float32)
    d0[:, 0, 0, 0] = 0.375                                           # no all-zero frame
    fe = H * W * 3
    d64 = d0.astype(np.float64)
    rms = np.sqrt((d64 ** 2).reshape(T, -1).mean(1))
    want_sc = [rms.sum() + 1e-12, np.abs(d64).mean(), np.abs(d64 - np.roll(d64, 1, 0)).mean(), np.abs(d64).max()]
    # g_adv on the scale of the regulariser gradient, so that both terms of g_tot matter
    gs = [(rng.standard_normal(d0.shape) * 0.7 / (fe * rms.mean()) * 0.2).astype(np.float32) for _ in range(2)]
    for dialect, dyn in (("tf", 0.0), ("torch", 0.25)):
        if dyn > 0:                                                  # the regulariser sees the clamped delta
            want_sc[0] = np.sqrt((np.clip(d64, -dyn, dyn) ** 2).reshape(T, -1).mean(1)).sum() + 1e-12
        # Adam, two steps
        s32 = (d0, np.zeros_like(d0), np.zeros_like(d0))
        s64 = tuple(a.astype(np.float64) for a in s32)
        dg, mg, vg = (torch.from_numpy(a.copy()).cuda() for a in s32)
        measured, errs = 0.0, []
        for step in (1, 2):
            g = gs[step - 1]
            sc = ops.perturb_dense_l12_adam(torch.from_numpy(g).cuda(), dg, mg, vg, step, dialect=dialect, beta=0.7, dyn_max_norm=dyn).cpu().numpy()
            if step == 1:
                np.testing.assert_allclose(sc, want_sc, rtol=1e-6, atol=0)
                assert sc[3] == np.float32(0.375)
            *s32, gt32 = dense_update(np.float32, s32[0], g, s32[1], s32[2], step, dialect=dialect, beta=0.7, dyn=dyn)
            *s64, gt64 = dense_update(np.float64, s64[0], g, s64[1], s64[2], step, dialect=dialect, beta=0.7, dyn=dyn)
            assert np.array_equal(np.sign(gt32), np.sign(gt64))
            measured = max(measured, float(np.abs(s32[0].astype(np.float64) - s64[0]).max()))
            errs.append(float(np.abs(dg.cpu().numpy().astype(np.float64) - s64[0]).max()))
        bound = 4 * measured
        print(f"n4={n4} T={T} {dialect} Adam: fp32-vs-fp64 formula {measured:.2e} -> bound {bound:.2e}; kernel vs fp64 per step {['%.2e' % e for e in errs]}")
        assert 0 < measured < 1e-6 and max(errs) <= bound
        # PGD, one step; the radius lies inside the range of delta
        radius = dict(eps=0.3) if dialect == "tf" else {}
        dyn_p = dyn if dialect == "torch" else 0.0
        p32, _, _, gt32 = dense_update(np.float32, d0, gs[0], d0, d0, 1, dialect=dialect, beta=0.7, dyn=dyn_p, pgd_eps=0.3 if dialect == "tf" else dyn)
        p64, _, _, gt64 = dense_update(np.float64, d0, gs[0], d0, d0, 1, dialect=dialect, beta=0.7, dyn=dyn_p, pgd_eps=0.3 if dialect == "tf" else dyn)
        assert np.array_equal(np.sign(gt32), np.sign(gt64)) and not np.any(gt64 == 0)
        measured = float(np.abs(p32.astype(np.float64) - p64).max())
        dg = torch.from_numpy(d0.copy()).cuda()
        sc = ops.perturb_dense_l12_pgd(torch.from_numpy(gs[0]).cuda(), dg, dialect=dialect, beta=0.7, dyn_max_norm=dyn_p, **radius).cpu().numpy()
        np.testing.assert_allclose(sc, want_sc, rtol=1e-6, atol=0)
        err = float(np.abs(dg.cpu().numpy().astype(np.float64) - p64).max())
        print(f"n4={n4} T={T} {dialect} PGD: fp32-vs-fp64 formula {measured:.2e} -> bound {4 * measured:.2e}; kernel vs fp64 {err:.2e}")
        assert 0 < measured < 1e-6 and err <= 4 * measured
        assert float(dg.abs().max()) <= float(np.float32(0.3 if dialect == "tf" else dyn)) and int((np.abs(d0) > 0.3).sum()) > 0


# ---- E. the one-workgroup flicker update at the edges of T --------------------------------------------------------------------------
EDGE_T = [1, 2, 3, 4, 85, 86, 171, 682]     # wrap(t +- 2, T) folding onto itself; 3T = 255 / 258 round the 256-thread seam; all 8 trips
ALPHA = 1e-3
KERNEL_TAU = 1e-5                           # tests/test_pgd_gpu.py, THE SIGN RULE, kernel level


def reg64(d, dialect, b0, b1, b2, b3, dyn):
    """(b0 * reg, {norm, diff, lap, thickness, roughness}) in fp64 for a [T,3] delta, through oracle.attack_math: the TF regulariser
    on the raw delta, the torch one on the clamped delta (beta2 = beta3 = 1 - beta1); the metrics on the raw delta in both"""
    dv = d.reshape(-1, 1, 1, 3)
    if dialect == "tf":
        _, reg = am.tf_total_loss(0.0, dv, 1.0, b1, b2, b3)
        parts = am.tf_regularizers(dv)
    else:
        assert b2 == b3 == 1 - b1
        dc = dv.clamp(-dyn, dyn)
        reg = am.torch_flicker_reg(dc.permute(3, 0, 1, 2), b1)
        parts = am.tf_regularizers(dc)
    raw = am.tf_regularizers(dv)
    return b0 * reg, [reg, parts["norm"], parts["diff"], parts["lap"], raw["thickness"], raw["roughness"]]


def flicker_inputs(Tn, dialect, seed):
    """tests/test_pgd_gpu.py flicker_inputs with the three planted out-of-bound entries folded into [0, T): they exist at T = 1 too"""
    rng = np.random.default_rng(seed)
    d = torch.from_numpy(rng.uniform(-0.25, 0.25, (Tn, 3)).astype(np.float32))
    d[1 % Tn, 0], d[5 % Tn, 2], d[(Tn - 2) % Tn, 1] = 0.47, -0.52, 0.41
    hp = dict(dialect=dialect, beta0=1.3, beta1=0.4, beta2=0.6, beta3=0.6, lr=ALPHA)
    eps = 0.4 if dialect == "tf" else 0.2
    hp.update(dict(eps=eps) if dialect == "tf" else dict(dyn_max_norm=eps))
    dv = d.double().clone().requires_grad_(True)
    (reg,) = torch.autograd.grad(reg64(dv, dialect, hp["beta0"], hp["beta1"], hp["beta2"], hp["beta3"], eps)[0], dv)
    g = torch.from_numpy((rng.standard_normal((Tn, 3)) * max(float(reg.abs().mean()), 1e-3)).astype(np.float32))
    return d, g, reg, eps, hp


@pytest.mark.parametrize("dialect", ["tf", "torch"])
@pytest.mark.parametrize("Tn", EDGE_T)
def test_reg_adam_at_the_edges_of_T(ops, Tn, dialect):
    """three Adam steps against fp64 (regulariser and its gradient through oracle.attack_math + autograd, am.tf_adam_step /
    am.torch_adam_step), at the tolerances of test_reg_adam_tf: scalars rtol 2e-5, delta rtol 1e-4 / atol 2e-7"""
    rng = np.random.default_rng(500 + Tn)
    d, _, _, dyn, hp = flicker_inputs(Tn, dialect, seed=200 + Tn)
    hp = {k: v for k, v in hp.items() if k != "eps"}
    betas = (hp["beta0"], hp["beta1"], hp["beta2"], hp["beta3"])
    d64, m64, v64 = d.double(), torch.zeros(Tn, 3, dtype=torch.float64), torch.zeros(Tn, 3, dtype=torch.float64)
    dg, mg, vg = d.clone().cuda(), torch.zeros(Tn, 3).cuda(), torch.zeros(Tn, 3).cuda()
    for step in range(1, 4):
        gadv = torch.from_numpy(rng.standard_normal((Tn, 3)).astype(np.float32) * (1e-9 if step == 2 else 1e-2))
        dv = d64.clone().requires_grad_(True)
        total, parts = reg64(dv, dialect, *betas, dyn)
        (g,) = torch.autograd.grad((gadv.double() * dv).sum() + total, dv)
        sc = ops.perturb_reg_adam(gadv.cuda(), dg, mg, vg, step, **hp).cpu()
        np.testing.assert_allclose(sc.numpy()[:6], [float(p) for p in parts], rtol=2e-5)
        assert sc[6].item() == pytest.approx(d64.max().item()) and sc[7].item() == pytest.approx(d64.min().item())
        d64, m64, v64 = (am.tf_adam_step if dialect == "tf" else am.torch_adam_step)(d64, g, m64, v64, step)
        torch.testing.assert_close(dg.cpu().double(), d64, rtol=1e-4, atol=2e-7)


@pytest.mark.parametrize("dialect", ["tf", "torch"])
@pytest.mark.parametrize("Tn", EDGE_T)
def test_reg_pgd_at_the_edges_of_T(ops, Tn, dialect):
    """test_reg_pgd_kernel at the edges of T: the kernel-level sign rule with its cap of zero elements left out, asserted from the
    fp64 restatement before the GPU result is looked at; 1e-7 absolute; scalars bitwise those of flk_perturb_reg_adam"""
    d, g, reg, eps, hp = flicker_inputs(Tn, dialect, seed=300 + Tn)
    out = int(((g.double() + reg).abs() < KERNEL_TAU * (g.double().abs() + reg.abs())).sum())
    print(f"T={Tn} {dialect}: {out} of {d.numel()} elements left out by the kernel-level rule; {int((d.abs() > eps).sum())} beyond the bound")
    assert out == 0, "cap: the flicker forms leave nothing out"
    assert int((d.abs() > eps).sum()) >= 3
    want = (d.double() - ALPHA * torch.sign(g.double() + reg)).clamp(-eps, eps)
    dg = d.clone().cuda()
    sc = ops.perturb_reg_pgd(g.cuda(), dg, **hp).cpu()
    err = float((dg.cpu().double() - want).abs().max())
    print(f"  max |delta' - restatement| = {err:.2e}")
    assert err <= 1e-7
    assert float(dg.abs().max()) <= float(np.float32(eps))
    hp_adam = {k: v for k, v in hp.items() if k != "eps"}
    da = d.clone().cuda()
    sc_adam = ops.perturb_reg_adam(g.cuda(), da, torch.zeros_like(da), torch.zeros_like(da), 1, **hp_adam).cpu()
    assert torch.equal(sc, sc_adam)


@pytest.mark.parametrize("dialect", ["tf", "torch"])
def test_batched_updates_at_T_682_equal_the_one_clip_kernels(ops, dialect):
    """reg_adam_batched and reg_pgd_batched at the documented maximum T = 682 (all eight trips of every thread), 3 clips, one of them
    frozen: bit for bit the one-clip kernels on each slice; the frozen clip keeps delta, moments and counter, its scalars are written"""
    B, Tn = 3, 682
    rng = np.random.default_rng(61)
    d = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, Tn, 3)).astype(np.float32)).cuda()
    g = torch.from_numpy((rng.standard_normal((B, Tn, 3)) * 5e-3).astype(np.float32)).cuda()
    m0 = torch.from_numpy((rng.standard_normal((B, Tn, 3)) * 1e-3).astype(np.float32)).cuda()
    v0 = torch.from_numpy((rng.random((B, Tn, 3)) * 1e-5).astype(np.float32)).cuda()
    active = torch.tensor([1, 0, 1], dtype=torch.int32).cuda()
    start = [0, 4, 8]
    hp = dict(dialect=dialect, beta0=1.3, beta1=0.4, beta2=0.6, beta3=0.6, lr=ALPHA, dyn_max_norm=0.2 if dialect == "torch" else 0.0)
    # Adam
    d2, m2, v2, steps = d.clone(), m0.clone(), v0.clone(), torch.tensor(start, dtype=torch.int32).cuda()
    sc = ops.perturb_reg_adam_batched(g, d2, m2, v2, steps, active, **hp)
    assert steps.tolist() == [1, 4, 9]
    for b in range(B):
        d1, m1, v1 = d[b].clone(), m0[b].clone(), v0[b].clone()
        sc1 = ops.perturb_reg_adam(g[b].contiguous(), d1, m1, v1, start[b] + 1, **hp)
        assert torch.equal(sc[b], sc1), b
        if int(active[b]):
            assert torch.equal(d2[b], d1) and torch.equal(m2[b], m1) and torch.equal(v2[b], v1) and not torch.equal(d2[b], d[b]), b
        else:
            assert torch.equal(d2[b], d[b]) and torch.equal(m2[b], m0[b]) and torch.equal(v2[b], v0[b]), b
    # PGD
    radius = dict(eps=0.25) if dialect == "tf" else {}
    d2, steps = d.clone(), torch.tensor(start, dtype=torch.int32).cuda()
    sc = ops.perturb_reg_pgd_batched(g, d2, steps, active, **hp, **radius)
    assert steps.tolist() == [1, 4, 9]
    for b in range(B):
        d1 = d[b].clone()
        sc1 = ops.perturb_reg_pgd(g[b].contiguous(), d1, **hp, **radius)
        assert torch.equal(sc[b], sc1), b
        if int(active[b]):
            assert torch.equal(d2[b], d1) and not torch.equal(d2[b], d[b]), b
        else:
            assert torch.equal(d2[b], d[b]), b


# ---- pointer contract: a uint8 clip that is not 8-byte aligned ----------------------------------------------------------------------
SMALL, TWO_WORKGROUPS = (2, 8, 12, 16), (2, 4, 44, 104)


@pytest.mark.parametrize("offset,shape", [pytest.param(2, SMALL, id="2"), pytest.param(4, SMALL, id="4"),
                                          pytest.param(2, TWO_WORKGROUPS, id="2-two-workgroups")])
def test_u8_clip_at_an_offset_equals_its_aligned_copy(ops, offset, shape):
    """a contiguous uint8 view `offset` bytes into a larger buffer (what a slice of a batch buffer or a loader hands over): the fast
    paths that read 8 bytes at a time (fold_t 2 / 3 flicker; fold_t 4 with x_lut: flicker, dense and per line) must not take it -- the
    strided kernels serve it, and output and gradient equal, bit for bit, those of an aligned copy of the same bytes.  Every case with
    and without the 8-bit round trip (q_lut); the gradient does not read the quantiser and is compared once per case.
    (2,8,12,16) is 6 x 2 = 12 live threads of one workgroup of the four-positions kernel; (2,4,44,104) is 22 x 13 = 286: its grid is
    (2, T', B) and the second workgroup has 30 live threads.  Pass share of the reference, asserted first: 0.85 - 0.86 (TF flicker),
    0.67 - 0.69 (torch flicker through the table), 0.70 (torch dense), 0.70 - 0.71 (torch per line)"""
    B, T, H, W = shape
    n = B * T * H * W * 3
    assert ((H // 2) * (W // 8) + 255) // 256 == (2 if shape == TWO_WORKGROUPS else 1)
    rng = np.random.default_rng(71 if shape == SMALL else 72)
    buf = torch.from_numpy(rng.integers(0, 256, n + 16, dtype=np.uint8)).cuda()
    view = buf[offset:offset + n].view(B, T, H, W, 3)
    copy = view.clone()
    assert view.is_contiguous() and view.data_ptr() % 8 == offset and copy.data_ptr() % 16 == 0 and torch.equal(view, copy)
    g = torch.from_numpy(rng.integers(-8, 9, (B, T, H, W, 3)).astype(np.float32))
    d = torch.from_numpy(rng.uniform(-0.6, 0.6, (T, 3)).astype(np.float32)).cuda()
    dd = torch.from_numpy(rng.uniform(-0.6, 0.6, (T, H, W, 3)).astype(np.float32)).cuda()
    dl = torch.from_numpy(rng.uniform(-0.6, 0.6, (B, T, H, 3)).astype(np.float32)).cuda()
    lut_np = decode_table()
    lut = torch.from_numpy(lut_np).cuda()
    tf_shifted, tf, torch_kw = dict(dclip=0.4, shift_x=1, shift_p=3), dict(dclip=0.4), dict(dclip=0.4, dialect="torch", x_lut=lut, **TORCH_KW)
    cases = [("fold_t 2", d, dict(fold_t=2, **tf_shifted), torch.float32),
             ("fold_t 2 bf16", d, dict(fold_t=2, **tf), torch.bfloat16),
             ("fold_t 3", d, dict(fold_t=3, **tf), torch.bfloat16),
             ("fold_t 3 f32", d, dict(fold_t=3, **tf), torch.float32),
             ("fold_t 4 flicker", d, dict(fold_t=4, **torch_kw), torch.bfloat16),
             ("fold_t 4 dense", dd, dict(fold_t=4, **torch_kw), torch.bfloat16),
             ("fold_t 4 per line", dl, dict(fold_t=4, per_line=True, **torch_kw), torch.bfloat16)]
    # the reference's pass share: neither everything nor nothing is clamped in any of the four models
    xc, ref_torch = copy.cpu().numpy(), dict(dclip=0.4, x_lut=lut_np, **TORCH_KW)
    lines = [np.ascontiguousarray(np.broadcast_to(dl[b].cpu().numpy()[:, :, None, :], (T, H, W, 3))) for b in range(B)]
    shares = {"TF flicker, rolled": pr.pass_mask(xc, d.cpu().numpy(), **tf_shifted).mean(), "TF flicker": pr.pass_mask(xc, d.cpu().numpy(), **tf).mean(),
              "torch flicker": pr.pass_mask(xc, d.cpu().numpy(), **ref_torch).mean(), "torch dense": pr.pass_mask(xc, dd.cpu().numpy(), **ref_torch).mean(),
              "torch per line": np.mean([pr.pass_mask(xc[b:b + 1], lines[b], **ref_torch).mean() for b in range(B)])}
    print({k: round(float(v), 3) for k, v in shares.items()})
    assert all(0.5 < float(v) < 0.95 for v in shares.values()), shares
    for what, delta, kw, dt in cases:
        for quantise in (None, "torch" if kw.get("dialect") == "torch" else "tf"):
            a_view, a_copy = ops.make_apply_args(view, delta, quantise=quantise, **kw), ops.make_apply_args(copy, delta, quantise=quantise, **kw)
            o_view, o_copy = ops.perturb_apply_s2d(a_view, dt), ops.perturb_apply_s2d(a_copy, dt)
            assert float(o_copy.float().abs().sum()) > 0 and torch.equal(o_view, o_copy), (what, quantise)
        gl = fold(g, kw["fold_t"]).cuda()
        g_view, g_copy = ops.perturb_grad_reduce(a_view, gl), ops.perturb_grad_reduce(a_copy, gl)
        assert float(g_copy.abs().sum()) > 0 and torch.equal(g_view, g_copy), what
    # the aligned copy of the TF cases is what the reference says (so "equal" is not "equally wrong")
    ref = pr.apply_ref(copy.cpu().numpy(), d.cpu().numpy(), dclip=0.4, shift_x=1, shift_p=3)
    got = ops.perturb_apply_s2d(ops.make_apply_args(view, d, fold_t=2, dclip=0.4, shift_x=1, shift_p=3), torch.float32).cpu()
    assert torch.equal(got, s2d(torch.from_numpy(ref)))
