"""The rolling shutter on the GPU: the lines mix and its transpose (flk_flicker_lines_mix / flk_flicker_lines_mix_grad) against their
numpy float32 restatements, bit for bit, at the sizes where their loops can go wrong; the per-line perturbation
(flk_apply_args.delta_per_line) in the apply, export and gradient kernels against the per-clip and dense forms those kernels already
have and against numpy; an engine whose channel has a readout steps on the logits of the video ``export_video(capture=)`` delivers,
folds its per-line gradient through the same tables, and is today's engine when the channel has none."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
T, HW, NFRAMES = 8, 64, 37
FIXED = {"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}      # the fixed channel of test_capture_gpu.py
FIXED_RS = dict(FIXED, readout=0.8)


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def line_tables(nb, H, K, seed, gain=True):
    """random taps (not normalised: the kernels take any) and gains, one table per clip"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (nb, H, K)).astype(np.float32), (rng.uniform(0.5, 1.5, (nb, 3)).astype(np.float32) if gain else None)


def edge_rows(P, nb, clip_T, seed):
    """random rows that contain P-1 and, outside the period, -1 and P (clamped by the mix, skipped by its gradient)"""
    rows = np.random.default_rng(seed).integers(0, P, (nb, clip_T)).astype(np.int32)
    flat = rows.reshape(-1)
    flat[0] = P - 1
    if flat.shape[0] >= 3:
        flat[1], flat[-1] = -1, P
    return rows


# ---- the mix and its transpose -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("P", [1, 2, 5, 682])
def test_mix_and_transpose_are_the_restatements(P, K):
    """P < K, rows -1 and P, a -0 entry, H = 1 / 6 / 112; with equal taps on every line the mix is flk_flicker_rows_mix on every line"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    delta = np.random.default_rng(P + K).standard_normal((P, 3)).astype(np.float32)
    delta[0, 0], delta[P - 1, 2] = -0.0, -0.0
    for H, clip_T, nb in ((1, 1, 5), (6, 3, 4), (112, 8, 2)):
        rows = edge_rows(P, nb, clip_T, seed=clip_T)
        taps, gain = line_tables(nb, H, K, seed=P * K + clip_T)
        taps[0, 0, 0] = 1.0                                             # ... so that a -0 of delta reaches the output of a K = 1 table
        g = np.random.default_rng(H + K).standard_normal((nb, clip_T, H, 3)).astype(np.float32)
        for gn in (gain, None):
            got = ops.flicker_lines_mix(dev(delta), dev(rows), dev(taps), dev(gn))
            assert tuple(got.shape) == (nb, clip_T, H, 3) and same_bits(got, vs.flicker_lines_mix(delta, rows, clip_T, taps, gn))
            out = torch.full((P, 3), np.nan, device="cuda")
            back = ops.flicker_lines_mix_grad(dev(g), dev(rows), P, dev(taps), dev(gn), out=out)
            assert back is out and same_bits(back, vs.flicker_lines_mix_grad(g, rows, clip_T, taps, gn, P))
        if K <= 4:                                                      # (the per-frame kernel takes up to 4 taps)
            flat = np.ascontiguousarray(taps[:, 0, :])
            same = ops.flicker_lines_mix(dev(delta), dev(rows), dev(np.ascontiguousarray(np.repeat(flat[:, None, :], H, axis=1))), dev(gain))
            frame = ops.flicker_rows_mix(dev(delta), dev(rows), dev(flat), dev(gain))
            assert same_bits(same, frame[:, :, None, :].expand(nb, clip_T, H, 3).contiguous())
    if K == 1:                                                          # -0 kept: the first product starts the sum
        one = ops.flicker_lines_mix(dev(delta), dev(np.zeros((1, 1), np.int32)), torch.ones((1, 2, 1), device="cuda"))
        assert bool(torch.signbit(one[0, 0, 1, 0])) and float(one[0, 0, 1, 0]) == 0.0


def test_mix_grid_stride_loop_iterates():
    """3 n H = 268 800 values > 1024 workgroups x 256 threads: threads of the capped grid take a second value"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    P, K, nb, clip_T, H = 5, 3, 100, 8, 112
    assert 3 * nb * clip_T * H > 1024 * 256
    delta = np.random.default_rng(1).standard_normal((P, 3)).astype(np.float32)
    rows = edge_rows(P, nb, clip_T, seed=2)
    taps, gain = line_tables(nb, H, K, seed=3)
    assert same_bits(ops.flicker_lines_mix(dev(delta), dev(rows), dev(taps), dev(gain)), vs.flicker_lines_mix(delta, rows, clip_T, taps, gain))


# (n, clip_T): the last entry of the first LDS piece of stage 2 (2048 entries), one entry into the second; clips of 7 frames that straddle
# the piece boundary (2051 = 293 x 7).  (P, K): 8 workgroups; a second workgroup with 2 live threads (3 * 86 = 258); the period below the taps
@pytest.mark.parametrize("P,K", [(682, 3), (86, 5), (2, 5), (3, 4)])
@pytest.mark.parametrize("n,clip_T", [(2048, 1), (2049, 1), (2051, 7)])
def test_transpose_across_the_staging_boundary(n, clip_T, P, K):
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    nb, H = n // clip_T, 2
    rows = edge_rows(P, nb, clip_T, seed=n + P)
    g = np.random.default_rng(n + K).standard_normal((nb, clip_T, H, 3)).astype(np.float32)
    taps, gain = line_tables(nb, H, K, seed=n * K + P)
    got = ops.flicker_lines_mix_grad(dev(g), dev(rows), P, dev(taps), dev(gain))
    assert tuple(got.shape) == (P, 3) and same_bits(got, vs.flicker_lines_mix_grad(g, rows, clip_T, taps, gain, P))
    # the scratch may be larger than stage 1 needs, and what it held does not matter
    big = torch.full((n * K * 3 + 7,), np.nan, device="cuda")
    assert same_bits(ops.flicker_lines_mix_grad(dev(g), dev(rows), P, dev(taps), dev(gain), scratch=big), got)


def test_transpose_unhit_rows_skipped_rows_and_exact_integers():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    rng = np.random.default_rng(5)
    rows = rng.choice(np.array([1, 4, -1, 9], np.int32), (3, 8)).astype(np.int32)        # K = 2 reaches rows 1, 2, 4, 5 of 9; -1 and 9 are no rows
    H = 6
    g = rng.integers(-8, 9, (3, 8, H, 3)).astype(np.float32)
    taps = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), (3, H, 2)).astype(np.float32)      # powers of two: every product and sum exact
    gain = rng.choice(np.array([0.5, 1.0, 4.0], np.float32), (3, 3)).astype(np.float32)
    out = torch.full((9, 3), np.nan, device="cuda")
    got = ops.flicker_lines_mix_grad(dev(g), dev(rows), 9, dev(taps), dev(gain), out=out).cpu().numpy()
    assert same_bits(got, vs.flicker_lines_mix_grad(g, rows, 8, taps, gain, 9))
    assert np.array_equal(got[[0, 3, 6, 7, 8]].view(np.uint32), np.zeros((5, 3), np.uint32))
    exact = np.zeros((9, 3), np.int64)                                  # in units of 1/8
    for i, r in enumerate(rows.reshape(-1)):
        if 0 <= r < 9:
            b = i // 8
            for k in range(2):
                coef = (8 * gain[b].astype(np.float64)[None, :] * taps[b, :, k].astype(np.float64)[:, None])
                exact[(r + k) % 9] += np.rint(coef * g.reshape(-1, H, 3)[i]).astype(np.int64).sum(0)
    assert np.array_equal(got.astype(np.float64) * 8, exact.astype(np.float64)) and np.abs(exact).max() > 0
    g_in = g.copy()
    g_in[(rows < 0) | (rows >= 9)] = np.nan                            # what a skipped frame holds never reaches an output
    assert same_bits(ops.flicker_lines_mix_grad(dev(g_in), dev(rows), 9, dev(taps), dev(gain)), got)


def test_argument_discipline():
    from flickering_adversarial_video_amd import ops
    delta, rows = torch.zeros((5, 3), device="cuda"), torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    g, taps, gain = torch.ones((2, 8, 4, 3), device="cuda"), torch.ones((2, 4, 2), device="cuda"), torch.ones((2, 3), device="cuda")
    for what, call in (("int32", lambda: ops.flicker_lines_mix(delta, rows.long(), taps)), ("delta", lambda: ops.flicker_lines_mix(delta.double(), rows, taps)),
                       ("taps", lambda: ops.flicker_lines_mix(delta, rows, taps[:, 0])), ("taps", lambda: ops.flicker_lines_mix(delta, rows, taps.cpu())),
                       ("taps", lambda: ops.flicker_lines_mix(delta, rows, torch.ones((2, 4, 6), device="cuda"))),
                       ("taps", lambda: ops.flicker_lines_mix_grad(g, rows, 5, torch.ones((3, 4, 2), device="cuda"))),
                       ("gain", lambda: ops.flicker_lines_mix(delta, rows, taps, gain[:, :2])),
                       ("out", lambda: ops.flicker_lines_mix(delta, rows, taps, out=torch.zeros((2, 8, 3), device="cuda"))),
                       ("g_lines", lambda: ops.flicker_lines_mix_grad(g[:, :, :2], rows, 5, taps)),
                       ("scratch", lambda: ops.flicker_lines_mix_grad(g, rows, 5, taps, scratch=torch.zeros(10, device="cuda"))),
                       ("period", lambda: ops.flicker_lines_mix_grad(g, rows, 683, taps)),
                       (r"rows must lie in \[0,5\)", lambda: ops.flicker_lines_mix(delta, rows, taps, rows_host=np.full((2, 8), 5, np.int32)))):
        with pytest.raises(ValueError, match=what):
            call()


# ---- the per-line perturbation in the apply, export and gradient kernels --------------------------------------------------------------
def torch_kw():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    mean, std = np.array(vs.DEFAULT_MEAN), np.array(vs.DEFAULT_STD)
    # (dclip 0.11: a delta held at the clamp then moves a byte value by 28.05 levels -- 0.1 would be 25.5, a rounding tie of the encode)
    return dict(dialect="torch", dclip=0.11, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=float(np.max((0.0 - mean) / std)),
                hi=float(np.min((1.0 - mean) / std)))


def clip_u8(B, Tc, H, W, seed):
    u8 = np.random.default_rng(seed).integers(0, 256, (B, Tc, H, W, 3)).astype(np.uint8)
    u8[:, :, 0], u8[:, :, 1] = 0, 255                                   # lines on which the lo / hi clamp is active
    return u8


def unfold(folded, B, Tc, H, W):
    return folded[..., :12].reshape(B, Tc, H // 2, W // 2, 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, Tc, H, W, 3).contiguous()


def applied_host(x, d_lines, kw, shift_p=0):
    """numpy float32 restatement of applied(x, pert) per element for a per-line perturbation [Bd,T,H,3] (adv_flag 1)"""
    f32 = np.float32
    d = np.roll(d_lines, shift_p, axis=1)                               # p'[t] = p[(t - shift_p) mod T]
    p = (np.minimum(np.maximum(d, f32(-kw["dclip"])), f32(kw["dclip"])) * np.array(kw["inv_std"], f32)).astype(f32)
    u = (x + p[:, :, :, None, :]).astype(f32)
    return np.minimum(np.maximum(u, f32(kw["lo"])), f32(kw["hi"]))


APPLY_SHAPES = [(2, 3, 6, 8), (1, 2, 10, 40), (2, 2, 6, 260)]           # W/2 = 4, 20, 130; H/2 = 3, 5, 3; W % 8 != 0 leaves the uint8 fast path


@pytest.mark.parametrize("fold_t", [1, 4])
@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_per_line_apply(shape, fold_t):
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import decode_table
    B, Tc, H, W = shape
    kw, rng = torch_kw(), np.random.default_rng(sum(shape))
    u8 = clip_u8(B, Tc, H, W, seed=W)
    xf = vs.normalize_u8(u8)
    lut = decode_table("cuda")
    out_dtype = torch.bfloat16 if fold_t == 4 else torch.float32
    d_clip = rng.uniform(-0.15, 0.15, (B, Tc, 3)).astype(np.float32)          # some values outside dclip
    d_lines = rng.uniform(-0.15, 0.15, (B, Tc, H, 3)).astype(np.float32)
    for x, xkw in ((dev(xf), {}), (dev(u8), dict(x_lut=lut))):
        for quant in (None, "torch"):
            def run(delta, **more):
                return ops.perturb_apply_s2d(ops.make_apply_args(x, dev(delta), fold_t=fold_t, quantise=quant, **xkw, **kw, **more), out_dtype)

            # every line of delta holds the same [B,T,3] values: bitwise the per-clip apply; one shared [T,3] with a roll: the shared apply
            same = np.ascontiguousarray(np.broadcast_to(d_clip[:, :, None, :], (B, Tc, H, 3)))
            assert same_bits(run(same, per_line=True), run(d_clip))
            assert same_bits(run(same[0], per_line=True, shift_p=1), run(d_clip[0], shift_p=1))
            # distinct lines: bitwise the dense apply of the lines spread over w (clip by clip: a dense delta is shared by the batch)
            got = run(d_lines, per_line=True)
            for b in range(B):
                dense = np.ascontiguousarray(np.broadcast_to(d_lines[b][:, :, None, :], (Tc, H, W, 3)))
                xb = x[b:b + 1].contiguous()
                want = ops.perturb_apply_s2d(ops.make_apply_args(xb, dev(dense), fold_t=fold_t, quantise=quant, **xkw, **kw), out_dtype)
                assert same_bits(got[b:b + 1], want)
            shared = run(d_lines[0], per_line=True, shift_p=1)           # [T,H,3] shared by the batch, rolled
            if fold_t == 1:                                              # ... and the numpy restatement, per element
                want = applied_host(xf, d_lines, kw)
                want1 = applied_host(xf, d_lines[:1], kw, shift_p=1)
                if quant:
                    want, want1 = (ops.quant_table_host("torch")[ops.encode_u8_host(w, "torch"), np.arange(3)] for w in (want, want1))
                assert same_bits(unfold(got, B, Tc, H, W), want) and same_bits(unfold(shared, B, Tc, H, W), want1)
                assert float(got[..., 12:].abs().max()) == 0.0


GRAD_SHAPES = [(2, 2, 6, 8), (1, 3, 10, 128), (2, 2, 6, 260)]           # W/2 = 4, 64, 130: below a wave, exactly one, two strides and a tail


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_per_line_gradient(shape):
    from flickering_adversarial_video_amd import ops
    B, Tc, H, W = shape
    rng = np.random.default_rng(sum(shape))
    kw = dict(dialect="tf", dclip=0.25, inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0, fold_t=1)
    x = (rng.integers(-12, 13, (B, Tc, H, W, 3)) / 8.0).astype(np.float32)          # eighths: x + p is exact, and lands ON the bounds too
    d_lines = (rng.integers(-4, 5, (B, Tc, H, 3)) / 8.0).astype(np.float32)         # some outside dclip = 0.25
    d_lines[0, 0, 0], d_lines[0, 0, 1] = (0.25, -0.25, 0.375), (-0.375, 0.25, 0.0)  # at the bound (kept), outside (zeroed)
    gi = rng.integers(-8, 9, (B, Tc, H, W, 3))
    folded = np.zeros((B, Tc, H // 2, W // 2, 16), np.float32)
    folded[..., :12] = gi.reshape(B, Tc, H // 2, 2, W // 2, 2, 3).transpose(0, 1, 2, 4, 3, 5, 6).reshape(B, Tc, H // 2, W // 2, 12)
    folded[..., 12:] = 99.0                                             # the padding channels are never read into a sum

    def expected(d):
        u = x + np.clip(d, -0.25, 0.25)[:, :, :, None, :]
        mask = (u >= -1.0) & (u <= 1.0)
        assert (u == 1.0).any() and (u == -1.0).any() and (u > 1.0).any() and (u < -1.0).any()
        s = (gi * mask).sum(3)                                          # int64 [B,T,H,3]: over w only
        return np.where(np.abs(d) <= 0.25, s, 0)

    a = ops.make_apply_args(dev(x), dev(d_lines), per_line=True, **kw)
    want = expected(d_lines)
    for gx in (dev(folded), dev(folded).to(torch.bfloat16)):
        out = torch.full((B, Tc, H, 3), np.nan, device="cuda")
        got = ops.perturb_grad_reduce(a, gx, out)
        assert got is out and np.array_equal(got.cpu().numpy().astype(np.int64), want) and bool(torch.isfinite(got).all())
    assert (want[np.abs(d_lines) > 0.25] == 0).all() and np.abs(want).max() > 0
    # every line holds its frame's [B,T,3] values: summed over H it is the per-clip gradient, exactly
    d_clip = (rng.integers(-3, 4, (B, Tc, 3)) / 8.0).astype(np.float32)
    same = np.ascontiguousarray(np.broadcast_to(d_clip[:, :, None, :], (B, Tc, H, 3)))
    lines = ops.perturb_grad_reduce(ops.make_apply_args(dev(x), dev(same), per_line=True, **kw), dev(folded))
    clip = ops.perturb_grad_reduce(ops.make_apply_args(dev(x), dev(d_clip), **kw), dev(folded))
    assert tuple(clip.shape) == (B, Tc, 3) and np.array_equal(lines.cpu().numpy().astype(np.float64).sum(2), clip.cpu().numpy().astype(np.float64))
    assert np.array_equal(lines.cpu().numpy().astype(np.int64), expected(same))
    # a float gradient: W addends per output, each within one rounding -- (W + 2) * 2^-24 * sum |g| of float64
    gf = rng.standard_normal((B, Tc, H, W, 3)).astype(np.float32)
    ff = np.zeros_like(folded)
    ff[..., :12] = gf.reshape(B, Tc, H // 2, 2, W // 2, 2, 3).transpose(0, 1, 2, 4, 3, 5, 6).reshape(B, Tc, H // 2, W // 2, 12)
    got = ops.perturb_grad_reduce(a, dev(ff)).cpu().numpy().astype(np.float64)
    u = x + np.clip(d_lines, -0.25, 0.25)[:, :, :, None, :]
    mask = ((u >= -1.0) & (u <= 1.0)) & (np.abs(d_lines) <= 0.25)[:, :, :, None, :]
    ref, mag = (gf.astype(np.float64) * mask).sum(3), (np.abs(gf.astype(np.float64)) * mask).sum(3)
    assert (np.abs(got - ref) <= (W + 2) * U * mag).all() and np.abs(ref).max() > 1


def test_per_line_export():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import decode_table
    kw, rng = torch_kw(), np.random.default_rng(7)
    lut = decode_table("cuda")
    # odd sizes, a period shorter than the clip, a roll: frame t takes row (t - 2) mod 3 of [3,H,3]; bitwise (frames and statistics) the
    # dense export of those rows spread over w, and the encode of the numpy restatement
    B, Tc, H, W, P = 1, 5, 7, 9, 3
    u8 = clip_u8(B, Tc, H, W, seed=3)
    xf = vs.normalize_u8(u8)
    d = rng.uniform(-0.15, 0.15, (P, H, 3)).astype(np.float32)
    per_frame = d[(np.arange(Tc) - 2) % P]                               # [T,H,3]
    dense = np.ascontiguousarray(np.broadcast_to(per_frame[:, :, None, :], (Tc, H, W, 3)))
    for x, xkw in ((dev(u8), dict(x_lut=lut)), (dev(xf), {})):
        got, st = ops.export_adversarial_u8(ops.make_export_apply_args(x, dev(d), shift_p=2, delta_T=P, per_line=True, **xkw, **kw), "torch", stats=True)
        want, wst = ops.export_adversarial_u8(ops.make_export_apply_args(x, dev(dense), **xkw, **kw), "torch", stats=True)
        assert tuple(got.shape) == (B, Tc, H, W, 3) and same_bits(got, want) and same_bits(st, wst) and int(st[..., 2].sum()) > 0
        assert same_bits(got, ops.encode_u8_host(applied_host(xf, per_frame[None], kw), "torch"))
    # even sizes, one perturbation per clip: the encode of what the fp32 apply writes
    B, Tc, H, W = 2, 4, 6, 8
    u8 = clip_u8(B, Tc, H, W, seed=5)
    dl = rng.uniform(-0.15, 0.15, (B, Tc, H, 3)).astype(np.float32)
    for x, xkw in ((dev(u8), dict(x_lut=lut)), (dev(vs.normalize_u8(u8)), {})):
        frames, st = ops.export_adversarial_u8(ops.make_export_apply_args(x, dev(dl), per_line=True, **xkw, **kw), "torch", stats=True)
        applied = ops.perturb_apply_s2d(ops.make_apply_args(x, dev(dl), fold_t=1, per_line=True, **xkw, **kw), torch.float32)
        assert same_bits(frames, ops.encode_u8_host(unfold(applied, B, Tc, H, W).cpu().numpy(), "torch")) and tuple(st.shape) == (B, Tc, 3, 4)
    with pytest.raises(ValueError, match="per_line"):
        ops.make_export_apply_args(x, dev(dl), per_line=True, delta_T=3, **xkw, **kw)


# ---- engines ---------------------------------------------------------------------------------------------------------------------
_ENGINES = {}
VIDEO_KW = dict(flicker_time="video", clips_per_video=2, video_reduce="sum", im_scale=HW, quantise_train=True)      # one video of two clips per batch


def channel(**kw):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    return vs.CaptureChannel(**kw)


def fixed_channel(**kw):
    """the distribution that has one channel: FIXED (``readout=0.8``: FIXED_RS)"""
    return channel(subframe=FIXED["subframe"], exposure=FIXED["exposure"], gain=FIXED["gain"], gain_mode="per_channel", **kw)


def engine(key, **kw):
    """r3d_18 on synthetic weights, 2 clips of 8 x 64 x 64, bf16; one per ``key``"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    if key not in _ENGINES:
        kw = dict(dict(batch_size=2, sample_length=T, image_size=HW, dtype="bf16", l_inf_pert_norm=0.2, optimizer="adam"), **kw)
        _ENGINES[key] = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), **kw)
    eng = _ENGINES[key]
    eng.set_frame_numbers(None)
    eng.pert_model.cyclic_pert = False
    return eng


def set_delta(eng, seed, amp=0.05):
    p = eng.pert_model.perturbation
    p.copy_(torch.from_numpy(np.random.default_rng(seed).uniform(-amp, amp, tuple(p.shape)).astype(np.float32)))


def criterion():
    from flickering_adversarial_video_amd.torch_attack import Losses
    return Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)


def video_u8(seed=11):
    u8 = np.random.default_rng(seed).integers(0, 256, (NFRAMES, HW, HW, 3)).astype(np.uint8)
    u8[:, :2] = 0
    u8[:, 2:4] = 255
    return torch.from_numpy(u8).cuda()


def table_of(sample_step=2, num_samples=2):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    return vs.sample_frame_indices(NFRAMES, T, sample_step=sample_step, num_samples=num_samples)


@pytest.mark.parametrize("P", [8, 5])
def test_the_step_sees_the_video_a_rolling_shutter_records(P):
    """clips cut from a video and perturbed line by line through a channel with a readout are bit for bit the clips cut from the video
    exported through that channel -- at a non-zero phase, with a step between the frames; the readout matters; a readout of 0 is none"""
    eng = engine(("fixed", P), flicker_period=P, capture=fixed_channel(readout=0.8), **VIDEO_KW)
    video, table = video_u8(), table_of(sample_step=2)
    assert any(int(t[0]) % P for t in table) and int(table[0, 1] - table[0, 0]) == 2
    idx = torch.from_numpy(table).cuda()
    clips = video[idx]
    eng.set_frame_numbers(table)
    set_delta(eng, 23)
    for phase in (3, 1):
        got = eng.logits(clips, True, phases=phase, capture=FIXED_RS).clone()
        assert same_bits(got, eng.logits(eng.export_video(video, phase=phase, capture=FIXED_RS)[idx], False))
        lc = eng.last_capture
        assert lc["taps"].shape == (2, HW, 3) and lc["readout"].tolist() == [0.8] and same_bits(eng.pert_model.taps_dev, lc["taps"])
        # the same channel without its readout reproduces neither
        frame = eng.logits(clips, True, phases=phase, capture=FIXED).clone()
        assert not same_bits(frame, got) and eng.last_capture["taps"].shape == (2, 2)
        assert not same_bits(eng.logits(eng.export_video(video, phase=phase, capture=FIXED)[idx], False), got)
        # ... and with a readout of 0 every line has the frame's taps: bit for bit the logits of the channel without one
        assert same_bits(eng.logits(clips, True, phases=phase, capture=dict(FIXED, readout=0.0)), frame)
        assert same_bits(eng.export_video(video, phase=phase, capture=dict(FIXED, readout=0.0)), eng.export_video(video, phase=phase, capture=FIXED))
    assert same_bits(eng.quantised_logits(clips, capture=FIXED_RS), eng.logits(clips, True, phases=0, capture=FIXED_RS).clone())


def test_video_level_verdict_and_the_payload():
    """the step's video logits under a fixed rolling-shutter channel are those evaluate_videos(quantise="video", capture=) gives the video
    exported through it; its payload is flicker_lines_mix_grad of the per-line gradient on last_capture's tables"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    ch = fixed_channel(readout=0.8)
    eng = engine("verdict", capture=ch, **VIDEO_KW)
    P = eng.P
    video = video_u8(seed=29)
    x = eng.prepare_videos([video], train=False, num_samples=2).clone()
    table = np.concatenate(eng.last_sampling)
    lab = eng.video_logits(eng.logits(x, False)).argmax(1).clone()
    set_delta(eng, 31)
    res = eng.step(x, lab, criterion(), update=False)
    stepped, got = res["video_logits"].clone(), eng._red[:3 * P].view(P, 3).clone()
    lc, rows = eng.last_capture, eng.pert_model.rows_host
    assert lc["readout"].tolist() == [0.8] and lc["taps"].shape == (2, HW, 3) and lc["gain_rows"].shape == (2, 3)
    assert np.array_equal(lc["taps"][0], vs.capture_line_taps(0.3, 1.5, 0.8, HW)) and np.array_equal(lc["taps"][0], lc["taps"][1])
    assert tuple(eng._g_lines.shape) == (2, T, HW, 3)
    want = ops.flicker_lines_mix_grad(eng._g_lines, eng.pert_model.rows_dev, P, dev(lc["taps"]), dev(lc["gain_rows"]), rows_host=rows)
    assert same_bits(got, want) and float(got.abs().max()) > 0 and bool(torch.isfinite(got).all())
    assert same_bits(want, vs.flicker_lines_mix_grad(eng._g_lines.cpu().numpy(), rows, T, lc["taps"], lc["gain_rows"], P))
    ev = eng.evaluate_videos([video], lab, num_samples=2, quantise="video", capture=ch, capture_draws=1)
    assert same_bits(stepped, ev["capture_video_logits"][0]) and ev["capture_draws"][0]["readout"].tolist() == [0.8]
    assert not same_bits(ev["video_logits"], stepped)
    # the frame-level channel (no readout) gives the video other logits
    ev0 = eng.evaluate_videos([video], lab, num_samples=2, quantise="video", capture=fixed_channel(), capture_draws=1)
    assert not same_bits(ev0["capture_video_logits"][0], stepped)
    for q in (None, "clip"):                                            # the other two routes of evaluate_videos take the readout too
        evq = eng.evaluate_videos([video], lab, num_samples=2, adversarial=True, quantise=q, capture=ch, capture_draws=1)
        assert same_bits(evq["capture_video_logits"][0], stepped)
    assert eng.pert_model.frame_numbers.tolist() == table.tolist()


def test_readout_none_is_the_engine_without_the_argument():
    kw = dict(subframe=(0, 1), exposure=(0.5, 2), gain=(0.7, 1.0), gain_mode="per_channel", seed=5)
    a, b = engine("off_a", flicker_period=5, capture=channel(readout=None, **kw), **VIDEO_KW), engine("off_b", flicker_period=5, capture=channel(**kw), **VIDEO_KW)
    video, table = video_u8(seed=37), table_of(sample_step=1)
    x = video[torch.from_numpy(table).cuda()]
    outs = []
    for e in (a, b):
        e.set_frame_numbers(table)
        set_delta(e, 41)
        lab = e.video_logits(e.logits(x, False)).argmax(1).clone()
        got = []
        for _ in range(3):
            r = e.step(x, lab, criterion(), lr=1e-2, update=True)
            got += [r["softmax"].clone(), r["adv_loss"].clone().reshape(1)]
            assert set(e.last_capture) == {"subframe", "exposure", "gain", "taps", "gain_rows"} and e.last_capture["taps"].ndim == 2
        outs.append(got + [e.pert_model.perturbation.clone()])
        assert getattr(e, "_g_lines", None) is None and e.pert_model._delta_lines is None
    assert all(same_bits(p, q) for p, q in zip(*outs)) and not same_bits(outs[0][-1], dev(np.zeros((5, 3), np.float32)))


def test_training_draws_a_readout_per_video_and_step():
    ch = channel(subframe=(0, 1), exposure=(0.5, 2), readout=(0, 1), seed=9)
    eng = engine("draws", batch_size=4, capture=ch, **VIDEO_KW)           # two videos of two clips
    video = video_u8(seed=59)
    x = eng.prepare_videos([video, video[:30]], num_samples=2).clone()
    set_delta(eng, 61)
    lab = eng.video_logits(eng.logits(x, False)).argmax(1).clone()
    seen = []
    for _ in range(2):
        before = eng.pert_model.perturbation.clone()
        eng.step(x, lab, criterion(), lr=1e-2, update=True)
        lc = eng.last_capture
        assert lc["readout"].shape == (2,) and lc["taps"].shape[:2] == (4, HW) and lc["taps"].shape[2] <= 5
        assert np.array_equal(lc["taps"][0], lc["taps"][1]) and not np.array_equal(lc["taps"][0], lc["taps"][2])      # the G clips share one
        assert same_bits(eng.pert_model.taps_dev, lc["taps"]) and same_bits(eng.pert_model.gain_dev, lc["gain_rows"])
        assert not same_bits(before, eng.pert_model.perturbation) and bool(torch.isfinite(eng.pert_model.perturbation).all())
        seen.append(lc["readout"].copy())
    assert not np.array_equal(seen[0], seen[1])
