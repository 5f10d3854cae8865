"""The codec-aware backward on the host: the float64 restatements the kernels are held against -- the transpose of the
resampling (``prepare_adjoint_matrices`` / ``prepare_grad_image_host``), the factors and masks of the integer forward
(``codec_quant_slopes_host``) and the linear chain (``codec_grad_host``) -- and every refusal that needs no device."""
import argparse
import ctypes as C

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

U24 = 2.0 ** -24


def _box(Hs, Ws, kind, im_scale=128):
    Hr, Wr = vs.prepare_geometry(Hs, Ws, im_scale, 112)[:2]
    return {"eval": None, "up": (3, 5, 60, 70), "down": (0, 0, Hr, Wr), "size": (2, 3, 112, 112)}[kind]


# ---- the transpose of the resampling ----
@pytest.mark.parametrize("rule", vs.RESIZE_RULES)
@pytest.mark.parametrize("size", [(37, 53), (240, 320)])
@pytest.mark.parametrize("kind,flip", [("eval", False), ("up", False), ("up", True), ("down", False), ("down", True), ("size", True)])
def test_grad_image_is_the_adjoint_of_the_resampling(size, kind, flip, rule):
    """sum g . prepare_resample_host(V) = sum V . prepare_grad_image_host(g): float64 noise plus the ONE float32 rounding of every
    composite weight (each of the two matrices carries a relative 2^-24, so the pairing moves by at most 2 * 2^-24 of its magnitude)"""
    Hs, Ws = size
    rng = np.random.default_rng(Hs + len(kind) + flip)
    box = _box(Hs, Ws, kind)
    V, g = rng.standard_normal((Hs, Ws, 3)), rng.standard_normal((112, 112, 3))
    kw = dict(box=box, flip=flip, im_scale=128, input_size=112, rule=rule)
    lhs = (g * vs.prepare_resample_host(V, **kw)).sum()
    back, mag, n = vs.prepare_grad_image_host(g, Hs, Ws, bound=True, **kw)
    rhs = (V * back).sum()
    pairing = (np.abs(V) * mag).sum()
    assert abs(lhs - rhs) <= (2 * U24 + 1e-12) * pairing, (lhs, rhs, pairing)
    assert n >= 2 and mag.min() >= 0


def test_adjoint_tables_restate_the_matrices_and_a_box_of_the_output_size_is_one_stage():
    Hs, Ws = 37, 53
    box = _box(Hs, Ws, "size")
    A_h, A_w = vs.prepare_adjoint_matrices(Hs, Ws, box, True)
    Hr, Wr, step_h, step_w, _, _ = vs.prepare_geometry(Hs, Ws, 128, 112)
    i0, i1, lam = vs._prep_axis(step_h, box[0] + np.arange(112), Hs)
    one = np.zeros((112, Hs), np.float32)
    np.add.at(one, (np.arange(112), i0), np.float32(1.0) - lam)
    np.add.at(one, (np.arange(112), i1), lam)
    assert np.array_equal(A_h, one), "a box of the output size: stage 1's own float32 weights, no second stage"
    assert (A_h != 0).sum(1).max() <= 2 and (A_w != 0).sum(1).max() <= 2
    # the tables of two clips of one call, against the matrices column by column
    sizes, boxes, flips = [(37, 53), (64, 48)], [_box(37, 53, "up"), _box(64, 48, "down")], [True, False]
    words, offsets, K = vs.prepare_adjoint_tables(sizes, boxes, flips)
    assert words.dtype == np.int32 and K >= 2
    for (Hs, Ws), box, flip, (th, tw) in zip(sizes, boxes, flips, offsets):
        for A, off, n in zip(vs.prepare_adjoint_matrices(Hs, Ws, box, flip), (th, tw), (Hs, Ws)):
            e = words[off:off + n * (2 + K)].reshape(n, 2 + K)
            dense = np.zeros_like(A)
            for s in range(n):
                first, cnt = int(e[s, 0]), int(e[s, 1])
                assert 0 <= cnt <= K and first + cnt <= A.shape[0]
                dense[first:first + cnt, s] = e[s, 2:2 + cnt].view(np.float32)
                assert not e[s, 2 + cnt:].any()
            assert np.array_equal(dense, A)
    assert offsets[1][0] == (37 + 53) * (2 + K)
    with pytest.raises(ValueError, match="go together"):
        vs.prepare_adjoint_tables(sizes, boxes, None)
    with pytest.raises(ValueError, match="outside the resized image"):
        vs.prepare_adjoint_matrices(37, 53, (0, 0, 500, 500))
    with pytest.raises(ValueError, match="must be"):
        vs.prepare_grad_image_host(np.zeros((8, 8, 3)), 37, 53)


# ---- the linear chain against autograd ----
def _torch_chain(g_out, d, keep, rgb_mask, s420):
    """the same chain written forwards in torch float64 and differentiated: pad, mean, matrices, repeat, with d and the masks constants"""
    import torch
    import torch.nn.functional as F
    N, H, W, _ = g_out.shape
    Hp, Wp = d[0].shape[1:]
    Cm = torch.from_numpy(vs.codec_dct_matrix().astype(np.float64))
    enc, dec = torch.from_numpy(vs._CODEC_ENC), torch.from_numpy(vs._CODEC_DEC)
    x = torch.zeros((N, H, W, 3), dtype=torch.float64, requires_grad=True)
    p = F.pad(x.permute(0, 3, 1, 2), (0, Wp - W, 0, Hp - H), mode="replicate").permute(0, 2, 3, 1) @ enc.T          # [N,Hp,Wp,(Y,Cb,Cr)]
    planes = [p[..., 0], p[..., 1], p[..., 2]]
    if s420:
        planes[1:] = [F.avg_pool2d(q[:, None], 2)[:, 0] for q in planes[1:]]
    rec = []
    for q, dd, kk in zip(planes, d, keep):
        n, hp, wp = q.shape
        blocks = lambda a: a.reshape(n, hp // 8, 8, wp // 8, 8).permute(0, 1, 3, 2, 4)
        coef = (Cm @ blocks(q) @ Cm.T) * blocks(torch.from_numpy(dd))
        back = (Cm.T @ coef @ Cm).permute(0, 1, 3, 2, 4).reshape(n, hp, wp)
        rec.append(back * torch.from_numpy(kk.astype(np.float64)))
    if s420:
        rec[1:] = [q.repeat_interleave(2, 1).repeat_interleave(2, 2) for q in rec[1:]]
    out = (torch.stack(rec, -1) @ dec.T)[:, :H, :W] * torch.from_numpy(rgb_mask.astype(np.float64))
    (out * torch.from_numpy(g_out)).sum().backward()
    return x.grad.numpy()


@pytest.mark.parametrize("mode", vs.CODEC_GRAD_MODES)
@pytest.mark.parametrize("sub", vs.CODEC_SUBSAMPLINGS)
@pytest.mark.parametrize("size", [(8, 8), (17, 23), (40, 56)])
def test_chain_is_the_autograd_of_the_surrogate(size, sub, mode):
    H, W = size
    rng = np.random.default_rng(H * W)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    frames[1, : H // 2] = np.where(rng.random((H // 2, W, 1)) < 0.5, 0, 255)          # saturated content: both clamps fire
    tone = np.stack([np.arange(256, dtype=np.uint8)[:, None].repeat(3, 1), (255 - np.arange(256, dtype=np.uint8))[:, None].repeat(3, 1)])
    g = rng.standard_normal((2, H, W, 3))
    consts = vs.codec_quant_slopes_host(frames, 50, sub, tone, mode)
    d, keep, rgb_mask = consts
    assert not rgb_mask.all() and (mode == "ste" or d[0].max() <= 0.75)
    got = vs.codec_grad_host(frames, 50, sub, tone, mode, g, consts=consts)["g_in"]
    want = _torch_chain(g, d, keep, rgb_mask, sub == "420")
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


# ---- the factors ----
def _grey(level, H=16, W=16):
    return np.full((1, H, W, 3), level, np.uint8)


def test_quantiser_factor_at_a_bin_centre_and_at_a_bin_edge():
    """a flat grey 4:4:4 frame at quality 50: luma DC f = 64 * (Y - 128), 8 Q = 128 -- level 130 sits on a bin centre, 131 on an edge"""
    ql, _ = vs.codec_tables(50)
    assert ql[0] == 16
    for level, r in ((130, 0.0), (131, -0.5)):
        x = _grey(level).astype(np.int64)
        Y = (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 32768) >> 16
        _, lev, f, _ = vs._codec_plane_parts(Y, ql, np.int64)
        assert (Y == level).all() and (f[..., 0, 0] == 64 * (level - 128)).all()          # the fixed-point luma of a grey is the grey
        assert ((f[..., 0, 0] - lev[..., 0, 0] * 128) / 128 == r).all()
        d, keep, rgb = vs.codec_quant_slopes_host(_grey(level), 50, "444", None, "cubic")
        assert (d[0][:, ::8, ::8] == 3 * r * r).all() and all(k.all() for k in keep) and rgb.all()
        assert (vs.codec_quant_slopes_host(_grey(level), 50, "444", None, "ste")[0][0] == 1).all()


def test_cubic_passes_nothing_at_a_bin_centre_and_ste_is_the_identity_route():
    frame = _grey(130)
    rng = np.random.default_rng(3)
    g = np.repeat(np.repeat(rng.standard_normal((1, 2, 2, 3)), 8, 1), 8, 2)             # constant per block: only the DC terms carry it
    luma_only = g[..., 1:2] * np.array([46802 / 91881, 1.0, 22554 / 116130])            # M_dec^T sends it to the luma plane alone
    delta = np.zeros((1, 1, 3), np.float32)
    slope, scale = vs.tone_slopes_host(delta)
    cubic = vs.codec_grad_host(frame, 50, "444", None, "cubic", g, slope[0], scale[0])
    assert (cubic["gdelta"] == 0).all() and np.abs(cubic["g_in"]).max() <= 1e-15 * np.abs(g).max()
    # level 131: the DC terms pass at 3/4
    edge = vs.codec_grad_host(_grey(131), 50, "444", None, "cubic", luma_only, slope[0], scale[0])
    ste131 = vs.codec_grad_host(_grey(131), 50, "444", None, "ste", luma_only, slope[0], scale[0])
    assert np.abs(ste131["gdelta"]).min() > 0 and np.allclose(edge["gdelta"], 0.75 * ste131["gdelta"], rtol=1e-9, atol=0)
    # straight through the quantiser, nothing clamped, whole blocks: the chain is M_enc^T M_dec^T, the identity up to the 16-bit
    # constants of the two colour transforms -- the identity route's payload within that
    ste = vs.codec_grad_host(frame, 50, "444", None, "ste", g, slope[0], scale[0], bound=True)
    identity = (g * slope[0][0][frame[0], np.arange(3)]).sum((1, 2)) * scale[0]
    colour = np.abs(vs._CODEC_DEC @ vs._CODEC_ENC - np.eye(3)).max()
    assert colour < 1e-4
    assert np.abs(ste["gdelta"] - identity).max() <= 3 * colour * ste["gdelta_mag"].max()
    assert ste["gdelta_roundings"] > ste["g_in_roundings"] > 56


@pytest.mark.parametrize("sub", vs.CODEC_SUBSAMPLINGS)
def test_saturated_content_zeroes_the_masked_pixels(sub):
    """black / white pixels ring past 0 and 255 after quantisation: where the unclamped value leaves 0..255 the gradient is dropped"""
    frame = np.where(np.random.default_rng(5).random((1, 16, 16, 3)) < 0.5, 0, 255).astype(np.uint8)      # saturated colours
    d, keep, rgb = vs.codec_quant_slopes_host(frame, 10, sub, None, "ste")
    assert not rgb.all() and not keep[0].all()
    g = np.ones((1, 16, 16, 3))
    only = np.where(rgb, 0.0, g)                                                       # gradient on the masked outputs alone
    res = vs.codec_grad_host(frame, 10, sub, None, "ste", only, bound=True)
    assert (res["g_in"] == 0).all() and (res["g_in_mag"] == 0).all()
    # a gradient on one plane-masked luma sample reaches nothing through luma
    y, x = np.argwhere(~keep[0][0])[0]
    consts = (d, keep, np.ones_like(rgb))
    lum = np.zeros((1, 16, 16, 3))
    lum[0, y, x] = 1.0
    full = vs.codec_grad_host(frame, 10, sub, None, "ste", lum, consts=consts)["g_in"]
    open_ = vs.codec_grad_host(frame, 10, sub, None, "ste", lum, consts=(d, tuple(np.ones_like(k) for k in keep), np.ones_like(rgb)))["g_in"]
    assert np.abs(full).sum() < np.abs(open_).sum()


# ---- refusals ----
def test_host_refusals():
    f, g = np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 8, 8, 3))
    with pytest.raises(ValueError, match="one of"):
        vs.codec_grad_host(f, 50, "444", None, "identity", g)
    with pytest.raises(ValueError, match="g_out"):
        vs.codec_grad_host(f, 50, "444", None, "ste", g[:, :4])
    with pytest.raises(ValueError, match="uint8"):
        vs.codec_quant_slopes_host(f.astype(np.float32), 50, "444")
    with pytest.raises(ValueError, match="tone"):
        vs.codec_quant_slopes_host(f, 50, "444", np.zeros((2, 256, 3), np.uint8))
    with pytest.raises(ValueError, match="slope"):
        vs.codec_grad_host(f, 50, "444", None, "ste", g, np.zeros((1, 256)), np.zeros((1, 3)))


def test_engine_refusals():
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    W = vs.synthetic_weights("r3d_18", 42)
    kw = dict(batch_size=2, sample_length=8, image_size=32, im_scale=36, flicker_time="video", train_delivered=True)
    with pytest.raises(ValueError, match="give codec="):
        FlickerVideoResNet("r3d_18", W, codec_grad="cubic", **kw)
    with pytest.raises(ValueError, match="intra codec"):
        FlickerVideoResNet("r3d_18", W, codec=vs.Codec(75, "420", gop=4), codec_grad="ste", **kw)
    with pytest.raises(ValueError, match="intra codec"):
        FlickerVideoResNet("r3d_18", W, codec=vs.Codec(75, "420", gop=4, search=3), codec_grad="cubic", **kw)
    with pytest.raises(ValueError, match="one of"):
        FlickerVideoResNet("r3d_18", W, codec=vs.Codec(75, "420"), codec_grad="soft", **kw)


def test_script_option():
    def parse(argv, train_delivered=True, used=True):
        ap = argparse.ArgumentParser()
        vs.add_codec_arguments(ap)
        a = ap.parse_args(argv)
        a.train_delivered = train_delivered
        a.codec = vs.codec_from_arguments(ap, a, used)
        return a
    a = parse(["--codec-quality", "60", "--codec-grad", "cubic"])
    assert a.codec == vs.Codec(60, "420") and a.codec_grad == "cubic"
    assert parse(["--codec-quality", "60"]).codec_grad is None
    for argv, td in ((["--codec-grad", "ste"], True), (["--codec-quality", "60", "--codec-gop", "4", "--codec-grad", "ste"], True),
                     (["--codec-quality", "60", "--codec-grad", "ste"], False), (["--codec-quality", "60", "--codec-grad", "soft"], True)):
        with pytest.raises(SystemExit):
            parse(argv, td)


def test_argument_refusals_of_the_entries():
    """every refusal of the two new entries is made on the host, before any device call"""
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    p = C.c_void_p(4096)
    clip = _lib.CodecClip()
    clip.src, clip.T, clip.Hs, clip.Ws, clip.pitch_t, clip.pitch_h = 4096, 2, 8, 8, 192, 24
    a = _lib.CodecArgs()
    a.nclip, a.quality, a.subsampling, a.clips = 1, 50, _lib.FLK_CODEC_444, (_lib.CodecClip * 1)(clip)

    def grad(args=a, T_out=2, mode=_lib.FLK_CODEC_GRAD_STE, g_out=p, slope=p, scale=p, gdelta=p, g_in=None, partials=p):
        return lib.flk_codec_grad(C.byref(args), None, T_out, None, mode, g_out, slope, scale, gdelta, g_in, partials, None), lib.flk_last_error()

    assert lib.flk_codec_grad_scratch_bytes(C.byref(a), 2) == 1 * 2 * 1 * 3 * 4
    assert lib.flk_codec_grad_scratch_bytes(C.byref(a), 0) == 0
    for kw, word in ((dict(mode=0), b"mode"), (dict(mode=3), b"mode"), (dict(slope=None), b"slope"), (dict(scale=None), b"slope"),
                     (dict(gdelta=None), b"slope"), (dict(g_out=None), b"g_out"), (dict(partials=None), b"g_out"), (dict(g_in=p), b"g_in"),
                     (dict(T_out=3), b"T_out"), (dict(T_out=0), b"T_out")):
        rc, msg = grad(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    bad = _lib.CodecArgs()
    bad.nclip, bad.quality, bad.subsampling, bad.clips = 1, 0, _lib.FLK_CODEC_444, a.clips
    assert grad(args=bad)[0] == -1 and b"quality" in lib.flk_last_error()
    bad.quality, bad.subsampling = 50, 422
    assert grad(args=bad)[0] == -1 and b"subsampling" in lib.flk_last_error()

    ic = _lib.GradImageClip()
    ic.dst, ic.pitch_t, ic.pitch_h, ic.Hs, ic.Ws, ic.tab_h, ic.tab_w = 4096, 8 * 24, 24, 8, 8, 0, 8 * 4
    arr = (_lib.GradImageClip * 1)(ic)

    def image(n=1, clips=arr, T_out=2, Ho=16, Wo=16, K=2, tables=p, words=64, gx=p, dtype=_lib.FLK_F32):
        return lib.flk_clip_prepare_grad_image(n, clips, T_out, Ho, Wo, K, tables, words, gx, dtype, None), lib.flk_last_error()

    for kw, word in ((dict(n=0), b"nclip"), (dict(n=65), b"nclip"), (dict(T_out=0), b"T_out"), (dict(Ho=15), b"even"), (dict(K=0), b"K"),
                     (dict(tables=None), b"null"), (dict(gx=None), b"null"), (dict(gx=C.c_void_p(4100)), b"aligned"), (dict(dtype=7), b"dtype"),
                     (dict(words=63), b"tables")):
        rc, msg = image(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    ic.pitch_h = 23
    assert image(clips=(_lib.GradImageClip * 1)(ic))[0] == -1 and b"pitches" in lib.flk_last_error()
