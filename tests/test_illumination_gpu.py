"""The flicker as scene illumination on the GPU (csrc/illum.hip: flk_illum_apply_s2d / flk_illum_export_u8 / flk_illum_grad_reduce): the
apply and the export BITWISE the numpy float32 restatements of videoresnet_spec, the bf16 / fold-4 / quantised forms bitwise the existing
clean apply run on those results, the identities between the delta forms, saturation, and the gradient -- exact on dyadic tables, within
its rounding bound of the float64 restatement on the sRGB tables, reproducible, per clip the batch-1 call."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
INF = float("inf")
DCLIP = 0.3


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def clip_u8(B, T, H, W, seed):
    """random bytes with a row of 0 and a row of 255 planted and every byte value present"""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    u8[:, :, 0] = 0
    u8[:, :, 1] = 255
    if u8[:, :, 2:].size >= 256:
        free = u8[:, :, 2:].reshape(-1)
        free[:256] = np.arange(256, dtype=np.uint8)
        u8[:, :, 2:] = free.reshape(u8[:, :, 2:].shape)
    return u8


def on_device(u8, offset=0):
    """the clip on the device, `offset` bytes past an allocation's start (allocations are at least 256-byte aligned)"""
    buf = torch.empty(u8.size + offset, dtype=torch.uint8, device="cuda")
    x = buf[offset:].view(u8.shape)
    x.copy_(torch.from_numpy(u8))
    assert x.is_contiguous() and x.data_ptr() % 8 == offset % 8
    return x


def fold1(x):
    """[B,T,H,W,3] -> the 16-channel (h,w) fold [B,T,H/2,W/2,16], channel (qh*2+qw)*3+c, 12..15 zero (data movement only)"""
    x = torch.as_tensor(x)
    B, T, H, W, _ = x.shape
    f = x.reshape(B, T, H // 2, 2, W // 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, T, H // 2, W // 2, 12)
    return torch.cat([f, torch.zeros(f.shape[:4] + (4,), dtype=f.dtype)], dim=4).contiguous()


def unfold1(f):
    B, T, H2, W2 = f.shape[:4]
    return f[..., :12].reshape(B, T, H2, W2, 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, T, 2 * H2, 2 * W2, 3).contiguous()


@pytest.fixture(scope="module")
def env():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import decode_table
    tables = {r: vs.illum_tables(r) for r in vs.ILLUM_RESPONSES}
    return dict(ops=ops, vs=vs, lut=decode_table("cuda"), lut_host=vs.u8_decode_table(), tables=tables,
                illum={r: ops.make_illum_args(t) for r, t in tables.items()})


def make_delta(kind, B, T, H, seed, amp=0.4):
    """(host delta, keywords of make_apply_args, keywords of the restatements); amplitudes beyond DCLIP: the delta clamp is hit"""
    rng = np.random.default_rng(seed)
    if kind == "shared":
        return rng.uniform(-amp, amp, (T, 3)).astype(np.float32), dict(shift_x=1, shift_p=2), dict(shift_x=1, shift_p=2)
    if kind == "per_clip":
        bounds = np.linspace(0.15, DCLIP, B).astype(np.float32)
        return rng.uniform(-amp, amp, (B, T, 3)).astype(np.float32), dict(dclip_dev=torch.from_numpy(bounds).cuda()), dict(dclip_clip=bounds)
    if kind == "lines":
        return rng.uniform(-amp, amp, (T, H, 3)).astype(np.float32), dict(per_line=True, shift_x=1, shift_p=2), dict(per_line=True, shift_x=1, shift_p=2)
    assert kind == "lines_per_clip"
    return rng.uniform(-amp, amp, (B, T, H, 3)).astype(np.float32), dict(per_line=True), dict(per_line=True)


def apply_args(env, x, d_dev, fold_t=1, quantise=None, adv_flag=1.0, dclip=DCLIP, **kw):
    vs = env["vs"]
    lo = float(np.max((0.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    hi = float(np.min((1.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    return env["ops"].make_apply_args(x, d_dev, dialect="torch", dclip=dclip, adv_flag=adv_flag, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo,
                                      hi=hi, fold_t=fold_t, x_lut=env["lut"], quantise=quantise, **kw)


def clean_apply(env, x, dtype, fold_t):
    """the existing clean apply (adv_flag = 0, no clamp) of an fp32 clip or of uint8 frames decoded through x_lut"""
    ops = env["ops"]
    zero = torch.zeros((x.shape[1], 3), dtype=F32, device="cuda")
    a = ops.make_apply_args(x, zero, dialect="torch", dclip=0.0, adv_flag=0.0, lo=-INF, hi=INF, fold_t=fold_t, x_lut=env["lut"] if x.dtype == torch.uint8 else None)
    return ops.perturb_apply_s2d(a, dtype)


KINDS = ("shared", "per_clip", "lines", "lines_per_clip")


# ---- apply -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "2-byte"])
@pytest.mark.parametrize("response", ["srgb", "linear"])
def test_apply_is_the_restatement_and_its_bf16_forms_the_clean_apply_of_it(env, kind, offset, response):
    ops, vs = env["ops"], env["vs"]
    B, T, H, W = 2, 4, 16, 16
    u8 = clip_u8(B, T, H, W, seed=3)
    x = on_device(u8, offset)              # offset 2: 2-byte but not 8-byte aligned -> the 2-byte-load instantiations
    d, kw, hkw = make_delta(kind, B, T, H, seed=5)
    dd = torch.from_numpy(d).cuda()
    want = vs.illum_apply_host(u8, d, env["tables"][response], dclip=DCLIP, **hkw)
    got = ops.illum_apply_s2d(apply_args(env, x, dd, fold_t=1, **kw), env["illum"][response], F32)
    assert same_bits(got, fold1(want))
    xf = torch.from_numpy(want).cuda()
    assert same_bits(ops.illum_apply_s2d(apply_args(env, x, dd, fold_t=1, **kw), env["illum"][response], BF16), clean_apply(env, xf, BF16, 1))
    assert same_bits(ops.illum_apply_s2d(apply_args(env, x, dd, fold_t=4, **kw), env["illum"][response], BF16), clean_apply(env, xf, BF16, 4))
    # the modulation does something: more than a tenth of the values moved off the round trip
    clean = vs.illum_apply_host(u8, np.zeros_like(d), env["tables"][response], dclip=DCLIP, **hkw)
    assert (want != clean).mean() > 0.1


# ---- export and quantised apply ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_export_is_the_restatement_and_the_quantised_apply_the_clean_apply_of_its_bytes(env, kind):
    ops, vs = env["ops"], env["vs"]
    B, T, H, W = 2, 4, 16, 16
    u8 = clip_u8(B, T, H, W, seed=7)
    d, kw, hkw = make_delta(kind, B, T, H, seed=9)
    dd = torch.from_numpy(d).cuda()
    for offset in (0, 2):
        x = on_device(u8, offset)
        want, want_st = vs.illum_export_host(u8, d, env["tables"]["srgb"], dclip=DCLIP, stats=True, **hkw)
        got, st = ops.illum_export_u8(apply_args(env, x, dd, **kw), env["illum"]["srgb"], stats=True)
        assert same_bits(got, want) and np.array_equal(st.cpu().numpy().astype(np.int64), want_st)
        assert want_st[..., 2].sum() > 0.1 * u8.size and want_st[..., 3].sum() > 0          # bytes moved; the [0,1] clamp was hit
        for dtype, fold_t in ((F32, 1), (BF16, 1), (BF16, 4)):
            q = ops.illum_apply_s2d(apply_args(env, x, dd, fold_t=fold_t, quantise="torch", **kw), env["illum"]["srgb"], dtype)
            assert same_bits(q, clean_apply(env, got.contiguous(), dtype, fold_t))


@pytest.mark.parametrize("per_line", [False, True], ids=["frame", "lines"])
def test_export_of_odd_frames_with_a_period_and_a_row_offset(env, per_line):
    ops, vs = env["ops"], env["vs"]
    B, T, H, W, P = 2, 3, 5, 7, 2
    u8 = clip_u8(B, T, H, W, seed=11)
    x = on_device(u8)
    rng = np.random.default_rng(13)
    for delta_T in (0, P):
        d = rng.uniform(-0.4, 0.4, ((delta_T or T,) + ((H, 3) if per_line else (3,)))).astype(np.float32)
        a = ops.make_export_apply_args(x, torch.from_numpy(d).cuda(), dialect="torch", dclip=DCLIP, shift_x=1, shift_p=2, x_lut=env["lut"], delta_T=delta_T,
                                       per_line=per_line)
        want, want_st = vs.illum_export_host(u8, d, env["tables"]["srgb"], dclip=DCLIP, shift_x=1, shift_p=2, delta_T=delta_T, per_line=per_line, stats=True)
        out = torch.full((B + 2, T, H, W, 3), 77, dtype=torch.uint8, device="cuda")
        rows, st = ops.illum_export_u8(a, env["illum"]["srgb"], out=out, out_offset=1, stats=True)
        assert same_bits(rows, want) and np.array_equal(st.cpu().numpy().astype(np.int64), want_st)
        assert bool((out[0] == 77).all()) and bool((out[B + 1] == 77).all())               # the other rows are left alone
        assert same_bits(ops.illum_export_u8(a, env["illum"]["srgb"]), want)                # without stats: the other instantiation


# ---- identities --------------------------------------------------------------------------------------------------------------------
def test_identities_between_the_forms(env):
    ops = env["ops"]
    B, T, H, W = 2, 4, 16, 16
    u8 = clip_u8(B, T, H, W, seed=15)
    x = on_device(u8)
    il = env["illum"]["srgb"]
    rng = np.random.default_rng(17)
    d = torch.from_numpy(rng.uniform(-0.4, 0.4, (T, 3)).astype(np.float32)).cuda()
    zero = torch.zeros((T, 3), dtype=F32, device="cuda")
    for dtype, fold_t in ((F32, 1), (BF16, 1), (BF16, 4)):
        clean = clean_apply(env, x, dtype, fold_t)
        # no modulation, quantised: the stored video is the source video
        assert same_bits(ops.illum_apply_s2d(apply_args(env, x, zero, fold_t=fold_t, quantise="torch"), il, dtype), clean)
        # adv_flag = 0: the existing apply with the same arguments, plain and quantised
        for quantise in (None, "torch"):
            a0 = apply_args(env, x, d, fold_t=fold_t, quantise=quantise, adv_flag=0.0)
            assert same_bits(ops.illum_apply_s2d(a0, il, dtype), ops.perturb_apply_s2d(a0, dtype))
        shared = ops.illum_apply_s2d(apply_args(env, x, d, fold_t=fold_t), il, dtype)
        per_clip = d[None].expand(B, T, 3).contiguous()
        assert same_bits(ops.illum_apply_s2d(apply_args(env, x, per_clip, fold_t=fold_t), il, dtype), shared)              # equal clips
        lines = per_clip[:, :, None, :].expand(B, T, H, 3).contiguous()
        assert same_bits(ops.illum_apply_s2d(apply_args(env, x, lines, fold_t=fold_t, per_line=True), il, dtype), shared)    # equal lines
    assert same_bits(ops.illum_export_u8(apply_args(env, x, zero), il), u8)
    e = ops.illum_export_u8(apply_args(env, x, d), il)
    assert same_bits(ops.illum_export_u8(apply_args(env, x, d[None].expand(B, T, 3).contiguous()), il), e)
    assert same_bits(ops.illum_export_u8(apply_args(env, x, d[None, :, None, :].expand(B, T, H, 3).contiguous(), per_line=True), il), e)


def test_saturated_and_black_bytes_do_not_move_and_carry_no_gradient(env):
    ops = env["ops"]
    B, T, H, W = 2, 4, 16, 16
    u8 = np.zeros((B, T, H, W, 3), np.uint8)
    u8[:, :, ::2] = 255
    x = on_device(u8)
    d = torch.full((T, 3), 0.25, dtype=F32, device="cuda")               # m > 0: 255 * (1 + m) leaves the range, 0 * anything is 0
    for il in env["illum"].values():
        a = apply_args(env, x, d)
        assert same_bits(ops.illum_export_u8(a, il), u8)
        assert same_bits(ops.illum_apply_s2d(apply_args(env, x, d, quantise="torch"), il, F32), clean_apply(env, x, F32, 1))
        gx = torch.from_numpy(np.random.default_rng(19).standard_normal((B, T, H // 2, W // 2, 16)).astype(np.float32)).cuda()
        g = ops.illum_grad_reduce(a, il, gx)
        assert bool((g == 0).all())
        lines = d[None, :, None, :].expand(B, T, H, 3).contiguous()
        assert bool((ops.illum_grad_reduce(apply_args(env, x, lines, per_line=True), il, gx) == 0).all())


# ---- gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS[:2] + KINDS[3:])
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gradient_is_exact_on_dyadic_tables(env, kind, gdtype):
    """dec = v / 256, enc = the identity on N = 256 segments, modulations that are multiples of 1/4 and small integer gradients: every
    weight, product and partial sum is a dyadic number far inside 24 bits, so the kernels must give the int64 sums exactly"""
    ops = env["ops"]
    B, T, H, W = 2, 4, 16, 16
    dec = np.ascontiguousarray(np.repeat((np.arange(256) / 256.0).astype(np.float32)[:, None], 3, axis=1))
    enc = (np.arange(257) / 256.0).astype(np.float32)
    il = ops.make_illum_args((dec, enc), out_mul=(1.0, 1.0, 1.0), out_add=(0.0, 0.0, 0.0))
    u8 = clip_u8(B, T, H, W, seed=21)
    rng = np.random.default_rng(23)
    shape = {"shared": (T, 3), "per_clip": (B, T, 3), "lines_per_clip": (B, T, H, 3)}[kind]
    d = (rng.integers(-2, 3, shape) / 4.0).astype(np.float32)            # -0.5 .. 0.5; the clamp at 0.25 masks the +-0.5 entries
    d.reshape(-1)[:3] = (0.5, 0.25, -0.25)
    kw = dict(per_line=True) if kind == "lines_per_clip" else dict(shift_x=1, shift_p=2) if kind == "shared" else {}
    g = rng.integers(-4, 5, (B, T, H, W, 3)).astype(np.int64)
    gx = fold1(torch.from_numpy(g.astype(np.float32))).to(gdtype).cuda()
    got = ops.illum_grad_reduce(apply_args(env, on_device(u8), torch.from_numpy(d).cuda(), dclip=0.25, **kw), il, gx).cpu().numpy()
    # int64 reference: s = (4 + m4) / 4, m4 = 4 * clamp(d, +-0.25); p = v * (4 + m4) / 1024, live where p <= 1; weight = L = v / 256
    sx, sp = kw.get("shift_x", 0), kw.get("shift_p", 0)
    rows = (np.arange(T) - sp) % T
    m4 = np.clip(np.round(d * 4).astype(np.int64), -1, 1)
    dm = (m4[rows] if kind == "shared" else m4[:, rows]).reshape({"shared": (1, T, 1, 1, 3), "per_clip": (B, T, 1, 1, 3), "lines_per_clip": (B, T, H, 1, 3)}[kind])
    v = np.roll(u8, sx, axis=1).astype(np.int64)
    live = v * (4 + dm) <= 1024
    assert not live.all()
    terms = np.where(live, g * v, 0)
    axes = {"shared": (0, 2, 3), "per_clip": (2, 3), "lines_per_clip": (3,)}[kind]
    by_t = terms.sum(axes)
    want = np.zeros(shape, np.int64)
    if kind == "shared":
        want[rows] = by_t
    else:
        want[:, rows] = by_t
    want = np.where(np.abs(d) <= 0.25, want, 0)
    assert np.abs(want).max() > 0 and (want == 0).any()
    assert np.array_equal(got.astype(np.float64) * 256.0, want.astype(np.float64))


@pytest.mark.parametrize("kind", KINDS[:2] + KINDS[3:])
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gradient_against_float64_reproducible_and_per_clip_the_batch_1_call(env, kind, gdtype):
    ops, vs = env["ops"], env["vs"]
    B, T, H, W = 2, 4, 16, 16
    u8 = clip_u8(B, T, H, W, seed=25)
    d, kw, hkw = make_delta(kind, B, T, H, seed=27)
    dd = torch.from_numpy(d).cuda()
    g = torch.from_numpy(np.random.default_rng(29).standard_normal((B, T, H, W, 3)).astype(np.float32)).to(gdtype)
    gx = fold1(g).cuda()
    for fold_t, offset in ((1, 0), (4, 2)):        # (the gradient of fold_t 4 comes back in the layout of 1)
        x = on_device(u8, offset)
        got = ops.illum_grad_reduce(apply_args(env, x, dd, fold_t=fold_t, **kw), env["illum"]["srgb"], gx)
        ref, mag, n = vs.illum_grad_host(u8, d, env["tables"]["srgb"], g.to(F32).numpy(), dclip=DCLIP, bound=True, **hkw)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        print(f"{kind} fold {fold_t}: max err / bound = {(err / np.maximum(n * U * mag, 1e-300)).max():.3g}, n = {n}")
        assert (err <= n * U * mag).all() and np.abs(ref).max() > 0 and (ref == 0).any()      # (zeros: delta values outside their clamp)
        assert same_bits(ops.illum_grad_reduce(apply_args(env, x, dd, fold_t=fold_t, **kw), env["illum"]["srgb"], gx), got)
        if kind != "shared":
            for b in range(B):
                kb = dict(kw)
                if "dclip_dev" in kb:
                    kb["dclip_dev"] = kb["dclip_dev"][b:b + 1].clone()
                one = ops.illum_grad_reduce(apply_args(env, on_device(u8[b:b + 1], offset), dd[b:b + 1].clone(), fold_t=fold_t, **kb), env["illum"]["srgb"],
                                            gx[b:b + 1].clone())
                assert same_bits(one[0], got[b])


# ---- where the loops iterate -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large(env):
    """2 clips of 9 x 480 x 512.  Every kernel of illum.hip runs at most 1024 workgroups that stride over the work, so each loop needs
    more work than one pass holds: the apply 2*9*240*64 = 276480 four-position groups (> 1024 * 256 threads; the 2-byte route four
    times as many items); the export 2*9*720 = 12960 chunk items (> 1024); the gradient's stage 1 2*9*57 = 1026 items (> 1024) of
    4 or 5 row pairs * 256 cells (> 256 threads), stage 2 sums 2 * 57 partials; the per-line gradient 2*9*240 = 4320 waves (> 4 * 1024)
    of 256 positions (> 64 lanes).  The restatements are computed once, here."""
    vs = env["vs"]
    B, T, H, W = 2, 9, 480, 512
    u8 = np.random.default_rng(31).integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    d = np.random.default_rng(33).uniform(-0.4, 0.4, (T, 3)).astype(np.float32)
    t = env["tables"]["srgb"]
    return dict(u8=u8, d=d, apply=vs.illum_apply_host(u8, d, t, dclip=DCLIP, shift_x=1, shift_p=2),
                export=vs.illum_export_host(u8, d, t, dclip=DCLIP, shift_x=1, shift_p=2, stats=True))


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "2-byte"])
def test_large_apply_and_export(env, large, offset):
    ops = env["ops"]
    x, dd = on_device(large["u8"], offset), torch.from_numpy(large["d"]).cuda()
    a = apply_args(env, x, dd, shift_x=1, shift_p=2)
    got = ops.illum_apply_s2d(a, env["illum"]["srgb"], F32)
    assert same_bits(unfold1(got), large["apply"]) and bool((got[..., 12:] == 0).all())
    q, st = ops.illum_export_u8(a, env["illum"]["srgb"], stats=True)
    assert same_bits(q, large["export"][0]) and np.array_equal(st.cpu().numpy().astype(np.int64), large["export"][1])
    if offset == 0:
        qa = ops.illum_apply_s2d(apply_args(env, x, dd, fold_t=4, quantise="torch", shift_x=1, shift_p=2), env["illum"]["srgb"], BF16)
        assert same_bits(qa, clean_apply(env, q.contiguous(), BF16, 4))


def test_large_gradients(env, large):
    ops, vs = env["ops"], env["vs"]
    u8, d = large["u8"], large["d"]
    B, T, H, W = u8.shape[:4]
    x = on_device(u8)
    g = torch.from_numpy(np.random.default_rng(35).standard_normal((B, T, H, W, 3)).astype(np.float32)).to(BF16)
    gx = fold1(g).cuda()
    got = ops.illum_grad_reduce(apply_args(env, x, torch.from_numpy(d).cuda(), shift_x=1, shift_p=2), env["illum"]["srgb"], gx)
    ref, mag, n = vs.illum_grad_host(u8, d, env["tables"]["srgb"], g.to(F32).numpy(), dclip=DCLIP, shift_x=1, shift_p=2, bound=True)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= n * U * mag).all() and np.abs(ref).max() > 0
    lines = np.ascontiguousarray(np.broadcast_to(d[None, :, None, :], (B, T, H, 3)))
    got = ops.illum_grad_reduce(apply_args(env, x, torch.from_numpy(lines).cuda(), per_line=True), env["illum"]["srgb"], gx)
    ref, mag, n = vs.illum_grad_host(u8, lines, env["tables"]["srgb"], g.to(F32).numpy(), dclip=DCLIP, per_line=True, bound=True)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= n * U * mag).all() and np.abs(ref).max() > 0


def test_the_longest_encode_table(env):
    """N = 16384: the tables no longer fit 64 KiB of LDS beside q_lut, the launch raises the kernel's limit"""
    ops, vs = env["ops"], env["vs"]
    B, T, H, W = 2, 4, 16, 16
    dec = env["tables"]["srgb"][0]
    g = np.arange(16385, dtype=np.float64) / 16384
    enc = np.where(g <= 0.0031308, 12.92 * g, 1.055 * g ** (1.0 / 2.4) - 0.055).clip(0, 1).astype(np.float32)
    tables = vs.illum_tables((dec, enc))
    il = ops.make_illum_args(tables)
    u8 = clip_u8(B, T, H, W, seed=37)
    x = on_device(u8)
    d = np.random.default_rng(39).uniform(-0.3, 0.3, (T, 3)).astype(np.float32)
    a = apply_args(env, x, torch.from_numpy(d).cuda())
    want = vs.illum_export_host(u8, d, tables, dclip=DCLIP)
    assert same_bits(ops.illum_export_u8(a, il), want)
    assert same_bits(ops.illum_apply_s2d(a, il, F32), fold1(vs.illum_apply_host(u8, d, tables, dclip=DCLIP)))
    q = ops.illum_apply_s2d(apply_args(env, x, torch.from_numpy(d).cuda(), fold_t=4, quantise="torch"), il, BF16)
    assert same_bits(q, clean_apply(env, torch.from_numpy(want).cuda(), BF16, 4))
    gx = torch.from_numpy(np.random.default_rng(41).standard_normal((B, T, H, W, 3)).astype(np.float32))
    got = ops.illum_grad_reduce(a, il, fold1(gx).cuda())
    ref, mag, n = vs.illum_grad_host(u8, d, tables, gx.numpy(), dclip=DCLIP, bound=True)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= n * U * mag).all()


# ---- engines ---------------------------------------------------------------------------------------------------------------------
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HW, NFRAMES = 8, 64, 37
FIXED = {"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}
FIXED_RS = dict(FIXED, readout=0.8)
_ENGINES = {}


def engine(key, **kw):
    """r3d_18 on synthetic weights, 2 clips of 8 x 64 x 64, bf16; one per ``key``"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    if key not in _ENGINES:
        kw = dict(dict(batch_size=2, sample_length=T, image_size=HW, dtype="bf16", l_inf_pert_norm=0.2, optimizer="adam"), **kw)
        _ENGINES[key] = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), **kw)
    return _ENGINES[key]


def set_delta(eng, seed, amp=0.1):
    p = eng.pert_model.perturbation
    p.copy_(torch.from_numpy(np.random.default_rng(seed).uniform(-amp, amp, tuple(p.shape)).astype(np.float32)))


def criterion():
    from flickering_adversarial_video_amd.torch_attack import Losses
    return Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)


def clips_dev(seed):
    return torch.from_numpy(clip_u8(2, T, HW, HW, seed)).cuda()


def test_engine_steps_on_the_stored_video_and_its_payload_is_the_new_reduce():
    from flickering_adversarial_video_amd import ops
    eng = engine("clip", flicker_model="illumination", quantise_train=True)
    assert eng.illumination and eng.pert_model.illumination and eng.pert_model.illum.enc_n == 4096
    x = clips_dev(43)
    set_delta(eng, 45)
    got = eng.logits(x, True).clone()
    frames = eng.adversarial_frames(x)
    assert same_bits(got, eng.logits(frames, False)) and same_bits(got, eng.quantised_logits(x))
    assert not same_bits(frames, x) and not same_bits(got, eng.logits(x, False))
    # Perturbation.forward and export_u8 follow the model: the unfolded quantised clip decodes the exported frames
    lut = env_lut()
    assert same_bits(eng.pert_model.forward([x, True], quantise=True), lut[frames.long(), torch.arange(3, device="cuda")])
    assert same_bits(eng.pert_model.export_u8(x), frames) and same_bits(eng.pert_model.export_u8(x, adversarial=False), x)
    with pytest.raises(ValueError, match="uint8 clips"):
        eng.logits(lut[x.long(), torch.arange(3, device="cuda")].contiguous(), True)
    # the step: forward on the folded tensor, backward, illum_grad_reduce -- the payload is that reduce of the engine's own _gx
    lab = eng.logits(x, False).argmax(1).clone()
    res = eng.step(x, lab, criterion(), update=False)
    assert bool(torch.isfinite(res["softmax"]).all())
    a = eng.pert_model.apply_args(x, True, fold_t=eng.net.input_fold, quantise=True)
    want = ops.illum_grad_reduce(a, eng.pert_model.illum, eng._gx)
    pay = eng._red[:3 * T].view(T, 3)
    assert same_bits(pay, want) and float(pay.abs().max()) > 0 and bool(torch.isfinite(pay).all())
    assert not same_bits(pay, ops.perturb_grad_reduce(a, eng._gx))                     # ... and not the additive model's
    before = eng.pert_model.perturbation.clone()
    for _ in range(2):
        res = eng.step(x, lab, criterion(), lr=1e-2, update=True)
    assert not same_bits(eng.pert_model.perturbation, before) and bool(torch.isfinite(eng.pert_model.perturbation).all()) and np.isfinite(float(res["adv_loss"]))


def env_lut():
    from flickering_adversarial_video_amd.torch_attack import decode_table
    return decode_table("cuda")


def test_the_step_sees_the_lit_video_a_rolling_shutter_records():
    """video time, the fixed capture channel with a readout of 0.8: the clips cut from a video and lit line by line are bit for bit the
    clips cut from the video exported through that channel; the payload is the per-line illum_grad_reduce followed by the transpose"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    P = 5
    ch = vs.CaptureChannel(subframe=FIXED["subframe"], exposure=FIXED["exposure"], gain=FIXED["gain"], gain_mode="per_channel", readout=0.8)
    eng = engine("video", flicker_model="illumination", flicker_time="video", flicker_period=P, capture=ch, clips_per_video=2, video_reduce="sum",
                 im_scale=HW, quantise_train=True)
    u8 = np.random.default_rng(47).integers(0, 256, (NFRAMES, HW, HW, 3)).astype(np.uint8)
    u8[:, :2], u8[:, 2:4] = 0, 255
    video = torch.from_numpy(u8).cuda()
    table = vs.sample_frame_indices(NFRAMES, T, sample_step=2, num_samples=2)
    idx = torch.from_numpy(table).cuda()
    clips = video[idx].contiguous()
    eng.set_frame_numbers(table)
    set_delta(eng, 49)
    for phase in (3, 0):
        got = eng.logits(clips, True, phases=phase, capture=FIXED_RS).clone()
        assert same_bits(got, eng.logits(eng.export_video(video, phase=phase, capture=FIXED_RS)[idx].contiguous(), False))
        assert not same_bits(got, eng.logits(clips, True, phases=phase, capture=FIXED))            # the readout matters
    assert not same_bits(eng.export_video(video), video)
    lab = eng.video_logits(eng.logits(clips, False)).argmax(1).clone()
    res = eng.step(clips, lab, criterion(), update=False)
    stepped, pay = res["video_logits"].clone(), eng._red[:3 * P].view(P, 3).clone()
    lc = eng.last_capture
    assert lc["readout"].tolist() == [0.8] and tuple(eng._g_lines.shape) == (2, T, HW, 3)
    a = eng.pert_model.apply_args(clips, True, fold_t=eng.net.input_fold, quantise=True, phases=0, capture=FIXED_RS)
    assert a.delta_per_line == 1 and same_bits(eng._g_lines, ops.illum_grad_reduce(a, eng.pert_model.illum, eng._gx))
    want = ops.flicker_lines_mix_grad(eng._g_lines, eng.pert_model.rows_dev, P, torch.from_numpy(lc["taps"]).cuda(), torch.from_numpy(lc["gain_rows"]).cuda())
    assert same_bits(pay, want) and float(pay.abs().max()) > 0
    ev = eng.evaluate_videos([video], lab, num_samples=2, quantise="video", capture=ch, capture_draws=1)
    assert ev["capture_video_logits"].shape == (1, 1, 400) and np.isfinite(ev["capture_video_logits"]).all()
    with pytest.raises(ValueError, match="quantise='video'"):
        eng.evaluate_videos([video], lab, num_samples=2, adversarial=True)
    assert bool(torch.isfinite(stepped).all())


def test_additive_is_the_engine_without_the_argument():
    a, b = engine("add_a", flicker_model="additive"), engine("add_b")
    assert not a.illumination and not b.illumination and a.pert_model._illum is None
    x = clips_dev(51)
    outs = []
    for e in (a, b):
        set_delta(e, 53, amp=0.05)
        lab = e.logits(x, False).argmax(1).clone()
        got = []
        for _ in range(3):
            r = e.step(x, lab, criterion(), lr=1e-2, update=True)
            got += [r["softmax"].clone(), r["adv_loss"].clone().reshape(1), e._red.clone()]
        outs.append(got + [e.pert_model.perturbation.clone(), e.adversarial_frames(x), e.logits(x, True).clone()])
    assert all(same_bits(p, q) for p, q in zip(*outs))


def test_per_clip_engine_with_pgd_steps_under_illumination():
    from flickering_adversarial_video_amd import ops
    eng = engine("per_clip", flicker_model="illumination", response="linear", per_clip=True, optimizer="pgd")
    x = clips_dev(55)
    set_delta(eng, 57)
    lab = eng.logits(x, False).argmax(1).clone()
    res = eng.step(x, lab, criterion(), update=False)
    a = eng.pert_model.apply_args(x, True, fold_t=eng.net.input_fold)
    assert a.delta_per_clip == 1 and same_bits(eng._gclip, ops.illum_grad_reduce(a, eng.pert_model.illum, eng._gx))
    before = eng.pert_model.perturbation.clone()
    eng.step(x, lab, criterion(), lr=1e-2, update=True)
    p = eng.pert_model.perturbation
    assert not same_bits(p, before) and bool(torch.isfinite(p).all()) and float(p.abs().max()) <= 0.2 and bool(torch.isfinite(res["adv_loss"]).all())


# ---- scripts -----------------------------------------------------------------------------------------------------------------------
def test_single_video_script_with_the_illumination_model(tmp_path):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    Ts = 8
    u8 = vs.synthetic_clip_u8(2, Ts, seed=6)
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=1, sample_length=Ts, dtype="f32")
    lab = [int(eng.logits(torch.from_numpy(u8[i:i + 1]).cuda(), False).argmax()) for i in range(2)]
    del eng
    np.savez(tmp_path / "v.npz", clips=u8, labels=np.array(lab), names=np.array(["clipA", "clipB"]))
    (tmp_path / "labels.txt").write_text("\n".join(f"class {i}" for i in range(400)))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_statistics_single_video_attack.py"), "--videos-npz", str(tmp_path / "v.npz"),
           "--label-map", str(tmp_path / "labels.txt"), "--results-root", str(tmp_path / "res"), "--base-model", "r3d_18", "--dtype", "f32",
           "--n-iter", "3", "--restart-after", "40", "--flicker-model", "illumination", "--quantise-train", "--save-adversarial-u8"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(glob.glob(str(tmp_path / "res" / "r3d_18" / "single_video_attack" / "flickering" / "*" / "*.npy")))
    assert [os.path.basename(f) for f in files] == [f"clipA_@class_{lab[0]}.npy", f"clipB_@class_{lab[1]}.npy"]
    ra = np.load(files[0], allow_pickle=True).tolist()
    assert len(ra["loss/total"]) >= 3 and ra["perturbation"][0].shape == (3, Ts, 1, 1) and np.isfinite(ra["loss/total"]).all()
    assert ra["adv_video_u8"].dtype == np.uint8 and ra["adv_video_u8"].shape == (1, Ts, 112, 112, 3)
    # the frames saved are the illumination export of the clip under the final perturbation
    final = np.ascontiguousarray(np.asarray(ra["perturbation"][-1], np.float32).reshape(3, Ts).T)
    want = vs.illum_export_host(u8[:1], final, vs.illum_tables("srgb"), dclip=float(np.abs(final).max()) + 1.0)
    assert np.array_equal(ra["adv_video_u8"], want)


def test_universal_script_with_the_illumination_model(tmp_path):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    Ts, N = 8, 4
    u8 = np.random.default_rng(3).integers(0, 256, (N, Ts, 112, 112, 3), dtype=np.uint8)
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=2, sample_length=Ts, dtype="f32")
    labels = np.concatenate([eng.logits(torch.from_numpy(u8[i:i + 2]).cuda(), False).argmax(1).cpu().numpy() for i in (0, 2)])
    del eng
    np.savez(tmp_path / "train.npz", clips=u8, labels=labels)
    np.savez(tmp_path / "val.npz", clips=u8[:2], labels=labels[:2])
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_universal_attack.py"), "--train-npz", str(tmp_path / "train.npz"),
           "--val-npz", str(tmp_path / "val.npz"), "--results-root", str(tmp_path / "results"), "--base-model", "r3d_18", "--batch-size", "2",
           "--dtype", "f32", "--epochs", "1", "--flicker-model", "illumination", "--response", "linear"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    dest = glob.glob(str(tmp_path / "results" / "r3d_18" / "generalization" / "universal" / "val_test" / "all_cls_shuffle_flickering" / "t_4_v_2_*"))
    assert len(dest) == 1
    res = np.load(os.path.join(dest[0], "r3d_18_001.npy"), allow_pickle=True)
    p = res[-1]["valid/perturbation"]
    assert p.shape == (3, Ts, 1, 1) and np.isfinite(p).all() and np.abs(p).max() > 1e-5 and 0.0 <= res[-1]["valid/fooling_ratio"] <= 1.0
