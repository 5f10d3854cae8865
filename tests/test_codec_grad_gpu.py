"""The codec-aware backward on the GPU: the transpose of the resampling on images (flk_clip_prepare_grad_image) and the
codec's own transpose (flk_codec_grad) per element within the rounding bounds of their float64 restatements, reproducible bit for bit
and per clip the call with that clip alone; the seam with flk_clip_prepare_grad where no clamp fires; and the engine under
``codec_grad`` "ste" / "cubic" against "identity"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
GEOM = dict(im_scale=16, input_size=12)


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def fold1(x):
    """[B,T,H,W,3] -> the 16-channel (h,w) fold [B,T,H/2,W/2,16], channel (qh*2+qw)*3+c, 12..15 zero (data movement only)"""
    x = torch.as_tensor(x)
    B, T, H, W, _ = x.shape
    f = x.reshape(B, T, H // 2, 2, W // 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, T, H // 2, W // 2, 12)
    return torch.cat([f, torch.zeros(f.shape[:4] + (4,), dtype=f.dtype)], dim=4).contiguous()


def unfold1(f):
    """the inverse of fold1 on the host, float64"""
    f = f.detach().float().cpu().numpy().astype(np.float64)
    B, T, H2, W2, _ = f.shape
    return f[..., :12].reshape(B, T, H2, W2, 2, 2, 3).transpose(0, 1, 2, 4, 3, 5, 6).reshape(B, T, 2 * H2, 2 * W2, 3)


def check(got, want, mag, n, what):
    """per element: |device - float64| <= roundings * 2^-24 * magnitude"""
    err, bound = np.abs(np.asarray(got, np.float64) - want), n * U * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.4f} (roundings {n})")
    assert (err <= bound).all(), (what, float(err.max()), float(bound.max()), worst)


@pytest.fixture(scope="module")
def env():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    return dict(ops=ops, vs=vs)


# ---- the transpose of the resampling on images ---------------------------------------------------------------------------------
SIZES = [(37, 53), (64, 48)]                                   # resized 16 x 22 and 21 x 16 under GEOM
IMAGE_TF = {"eval": dict(boxes=None, flips=None),
            "up_flip": dict(boxes=[(1, 2, 7, 9), (2, 1, 8, 6)], flips=[True, True]),                 # boxes smaller than 12 x 12: upscaled
            "down": dict(boxes=[(0, 0, 16, 22), (0, 0, 21, 16)], flips=[False, False])}              # the whole resized image: downscaled
IDX = np.array([[0, 0, 2], [1, 2, 2]])                         # a table with repeats: every output frame has its own image


@pytest.fixture(scope="module")
def image_case():
    rng = np.random.default_rng(7)
    videos = [torch.from_numpy(rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)).cuda() for h, w in SIZES]
    g = rng.standard_normal((2, 3, 12, 12, 3)).astype(np.float32)
    return dict(videos=videos, g={F32: fold1(g).cuda(), BF16: fold1(g).to(BF16).cuda()})


@pytest.mark.parametrize("gdtype", [F32, BF16])
@pytest.mark.parametrize("tf", list(IMAGE_TF))
def test_grad_image_within_its_rounding_bound_of_the_restatement(env, image_case, tf, gdtype):
    ops, vs = env["ops"], env["vs"]
    kw, gx = IMAGE_TF[tf], image_case["g"][gdtype]
    got = ops.prepare_clips_grad_image(image_case["videos"], gx, frame_idx=IDX, **GEOM, **kw)
    again = ops.prepare_clips_grad_image(image_case["videos"], gx, frame_idx=IDX, **GEOM, **kw)
    g = unfold1(gx)
    for k, (Hs, Ws) in enumerate(SIZES):
        assert tuple(got[k].shape) == (3, Hs, Ws, 3) and same_bits(got[k], again[k])                 # repeats
        box, flip = (kw["boxes"][k], kw["flips"][k]) if kw["boxes"] else (None, False)
        for t in range(3):
            want, mag, n = vs.prepare_grad_image_host(g[k, t], Hs, Ws, box, flip, bound=True, **GEOM)
            check(got[k][t].cpu().numpy(), want, mag, n, f"grad image {tf} {gdtype} clip {k} frame {t}")
        unread = vs.prepare_grad_image_host(np.ones((12, 12, 3)), Hs, Ws, box, flip, bound=True, **GEOM)[1] == 0
        assert (got[k].cpu().numpy()[:, unread] == 0).all() and (tf != "eval" or unread.any())         # pixels no output reads: +0
        alone = ops.prepare_clips_grad_image([image_case["videos"][k]], gx[k:k + 1].contiguous(), frame_idx=IDX[k:k + 1], **GEOM,
                                             **(dict(boxes=[box], flips=[flip]) if kw["boxes"] else {}))
        assert same_bits(got[k], alone[0])                                                           # a clip alone: its rows of the batch call


def test_grad_image_into_pitched_views(env, image_case):
    ops = env["ops"]
    gx, kw = image_case["g"][F32], IMAGE_TF["up_flip"]
    dense = ops.prepare_clips_grad_image(image_case["videos"], gx, frame_idx=IDX, **GEOM, **kw)
    bufs = [torch.full((3, h + 2, w + 3, 3), -7.0, dtype=F32, device="cuda") for h, w in SIZES]
    views = [b[:, 1:1 + h, 2:2 + w] for b, (h, w) in zip(bufs, SIZES)]
    out = ops.prepare_clips_grad_image(image_case["videos"], gx, frame_idx=IDX, out=views, **GEOM, **kw)
    for b, v, d, (h, w) in zip(bufs, out, dense, SIZES):
        assert same_bits(v.contiguous(), d)
        b[:, 1:1 + h, 2:2 + w] = -7.0
        assert bool((b == -7.0).all())                                                               # nothing outside the views was written
    with pytest.raises(ValueError, match="frame_idx"):
        ops.prepare_clips_grad_image(image_case["videos"], gx, **GEOM)
    with pytest.raises(ValueError, match="gx_s2d"):
        ops.prepare_clips_grad_image(image_case["videos"], gx[:1], frame_idx=IDX, **GEOM)
    with pytest.raises(ValueError, match="out"):
        ops.prepare_clips_grad_image(image_case["videos"], gx, frame_idx=IDX, out=[d[:, :4] for d in dense], **GEOM)


# ---- the codec's transpose ---------------------------------------------------------------------------------------------------
def contents(H, W, seed):
    """four frames: random, flat grey, saturated colours, smooth"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([128 + 90 * np.sin(yy / 5.0 + c) * np.cos(xx / 7.0) for c in range(3)], -1)
    return np.stack([rng.integers(0, 256, (H, W, 3)), np.full((H, W, 3), 130), np.where(rng.random((H, W, 3)) < 0.5, 0, 255), smooth]).astype(np.uint8)


def codec_case(vs, sub, seed=0):
    """three clips -- 8 x 8, 17 x 23 (partial MCUs in both axes) and one spanning two workgroup tiles in both directions -- of four
    frames each; a frame table with repeats; a tone table that is not the identity; random slopes; scales with zeros"""
    th = vs.CODEC_TILE_H[sub]
    sizes = [(8, 8), (17, 23), (th + 8, vs.CODEC_TILE_W + 8)]
    rng = np.random.default_rng(31 + seed)
    hosts = [contents(h, w, 5 + k) for k, (h, w) in enumerate(sizes)]
    idx = np.array([[0, 1, 2, 3, 2], [3, 3, 0, 1, 2], [2, 0, 1, 3, 0]])
    ramp = np.arange(256)
    tone = np.stack([np.stack([np.stack([np.clip((ramp * (0.7 + 0.1 * c) + 10 * t + 3 * k).round(), 0, 255) for c in range(3)], -1)
                               for t in range(5)]) for k in range(3)]).astype(np.uint8)
    slope = rng.uniform(0.0, 2.0, (3, 5, 256, 3)).astype(np.float32)
    scale = rng.uniform(-4.0, 4.0, (3, 5, 3)).astype(np.float32)
    scale[0, 1], scale[2, 3, 1] = 0.0, 0.0
    g = [rng.standard_normal((5, h, w, 3)).astype(np.float32) for h, w in sizes]
    return dict(sizes=sizes, hosts=hosts, idx=idx, tone=tone, slope=slope, scale=scale, g=g)


def run_codec_grad(ops, vs, case, sub, mode, quality, want_gin=True):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.codec_grad([dev(h) for h in case["hosts"]], vs.Codec(quality, sub), [dev(g) for g in case["g"]], dev(case["slope"]), dev(case["scale"]),
                          mode, frame_idx=case["idx"], tone=dev(case["tone"]), g_in=want_gin)


@pytest.mark.parametrize("quality", [10, 50, 75, 100])
@pytest.mark.parametrize("mode", ["ste", "cubic"])
@pytest.mark.parametrize("sub", ["444", "420"])
def test_codec_grad_within_its_rounding_bound_of_the_restatement(env, sub, mode, quality):
    ops, vs = env["ops"], env["vs"]
    case = codec_case(vs, sub)
    gdelta, g_in = run_codec_grad(ops, vs, case, sub, mode, quality)
    again, g_in2 = run_codec_grad(ops, vs, case, sub, mode, quality)
    assert same_bits(gdelta, again) and all(same_bits(p, q) for p, q in zip(g_in, g_in2))           # repeats
    assert same_bits(gdelta, run_codec_grad(ops, vs, case, sub, mode, quality, want_gin=False))      # the optional store changes nothing
    gd = gdelta.cpu().numpy()
    clamped = 0
    for k in range(3):
        frames = case["hosts"][k][case["idx"][k]]
        consts = vs.codec_quant_slopes_host(frames, quality, sub, case["tone"][k], mode)
        clamped += int((~consts[2]).sum()) + int((~consts[1][0]).sum())
        res = vs.codec_grad_host(frames, quality, sub, case["tone"][k], mode, case["g"][k], case["slope"][k], case["scale"][k], bound=True, consts=consts)
        what = f"codec grad {sub} {mode} q{quality} clip {k}"
        check(g_in[k].cpu().numpy(), res["g_in"], res["g_in_mag"], res["g_in_roundings"], what + " g_in")
        check(gd[k], res["gdelta"], res["gdelta_mag"], res["gdelta_roundings"], what + " gdelta")
        assert np.abs(res["gdelta"]).max() > 0
    assert clamped > 0                                                                               # both clamps fire somewhere in the case
    zero = case["scale"] == 0
    assert zero.any() and (gd[zero] == 0).all() and not np.signbit(gd[zero]).any()                   # a zero scale writes +0


def test_codec_grad_of_more_than_64_clips(env):
    """70 clips through ops.codec_grad: two launch pairs; the second one's clips are those of a call holding them alone"""
    ops, vs = env["ops"], env["vs"]
    rng = np.random.default_rng(2)
    sizes = [(8, 8) if k % 3 else (17, 23) for k in range(70)]
    hosts = [rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8) for h, w in sizes]
    g = [rng.standard_normal((2, h, w, 3)).astype(np.float32) for h, w in sizes]
    slope, scale = rng.uniform(0, 2, (70, 2, 256, 3)).astype(np.float32), rng.uniform(-2, 2, (70, 2, 3)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()
    vids, gs, sl, sc = [dev(h) for h in hosts], [dev(x) for x in g], dev(slope), dev(scale)
    codec = vs.Codec(50, "420")
    got = ops.codec_grad(vids, codec, gs, sl, sc, "cubic")
    assert tuple(got.shape) == (70, 2, 3)
    assert same_bits(got[64:], ops.codec_grad(vids[64:], codec, gs[64:], sl[64:].contiguous(), sc[64:].contiguous(), "cubic"))
    flat = torch.cat([x.reshape(-1) for x in gs])
    assert same_bits(got, ops.codec_grad(vids, codec, flat, sl, sc, "cubic"))                        # the images given packed already
    for k in (0, 1, 63, 64, 69):
        res = vs.codec_grad_host(hosts[k], 50, "420", None, "cubic", g[k], slope[k], scale[k], bound=True)
        check(got[k].cpu().numpy(), res["gdelta"], res["gdelta_mag"], res["gdelta_roundings"], f"70 clips: clip {k}")
    # the image transpose of the same 70 clips: its second launch's clips are those of a call holding them alone
    gx = fold1(rng.standard_normal((70, 2, 12, 12, 3)).astype(np.float32)).cuda()
    table = np.broadcast_to(np.arange(2), (70, 2))
    images = ops.prepare_clips_grad_image(vids, gx, frame_idx=table, **GEOM)
    alone = ops.prepare_clips_grad_image(vids[64:], gx[64:].contiguous(), frame_idx=table[64:], **GEOM)
    assert len(images) == 70 and all(same_bits(p, q) for p, q in zip(images[64:], alone))
    want, mag, n = vs.prepare_grad_image_host(unfold1(gx[69:])[0, 1], *sizes[69], bound=True, **GEOM)
    check(images[69][1].cpu().numpy(), want, mag, n, "70 clips: image of clip 69")
    with pytest.raises(ValueError, match="intra-frame"):
        ops.codec_grad(vids[:1], vs.Codec(50, "420", gop=4), gs[:1], sl[:1].contiguous(), sc[:1].contiguous(), "ste")
    with pytest.raises(ValueError, match="mode"):
        ops.codec_grad(vids[:1], codec, gs[:1], sl[:1].contiguous(), sc[:1].contiguous(), "identity")
    with pytest.raises(ValueError, match="g_out"):
        ops.codec_grad(vids[:2], codec, gs[:1], sl[:2].contiguous(), sc[:2].contiguous(), "ste")


# ---- the seam with flk_clip_prepare_grad ----------------------------------------------------------------------------------------
def test_seam_with_the_prepare_gradient_where_no_clamp_fires(env):
    """ste, 4:4:4, quality 100, smooth mid-range content and a small delta: the restatement's masks are all ones, so the codec's
    transpose is the identity up to the two colour matrices and the image transpose followed by flk_codec_grad must give
    flk_clip_prepare_grad's gdelta -- within the sum of the bounds of the routes: the codec chain's, the image transpose's carried
    through the chain, and the prepare gradient's ((n + 16) roundings, as tests/test_delivered_gpu.py holds it)"""
    ops, vs = env["ops"], env["vs"]
    from flickering_adversarial_video_amd.torch_attack import decode_table
    rng = np.random.default_rng(9)
    Hs, Ws, T = 40, 56, 3
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    host = np.stack([np.stack([128 + 40 * np.sin(yy / 9.0 + t + c) * np.cos(xx / 11.0) for c in range(3)], -1) for t in range(T)]).round().astype(np.uint8)
    video, idx = torch.from_numpy(host).cuda(), np.arange(T)[None]
    delta = rng.uniform(-0.05, 0.05, (1, T, 3)).astype(np.float32)
    lo, hi = vs.additive_bounds()
    a = ops.make_export_apply_args(ops.tone_ramp(1, T), torch.from_numpy(delta).cuda(), x_lut=decode_table("cuda"), dialect="torch", dclip=0.6,
                                   inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo, hi=hi)
    tone = ops.flicker_tone_tables(a, None)
    slope, scale = ops.flicker_tone_slopes(a, None)
    consts = vs.codec_quant_slopes_host(host, 100, "444", tone[0].cpu().numpy(), "ste")
    assert all(k.all() for k in consts[1]) and consts[2].all() and all((d == 1).all() for d in consts[0])
    g = rng.standard_normal((1, T, 12, 12, 3)).astype(np.float32)
    gx = fold1(g).cuda()
    images = ops.prepare_clips_grad_image([video], gx, frame_idx=idx, **GEOM)
    got = ops.codec_grad([video], vs.Codec(100, "444"), images, slope, scale, "ste", frame_idx=idx, tone=tone)[0].cpu().numpy()
    ref = ops.prepare_clips_grad([video], gx, slope, scale, frame_idx=idx, **GEOM)[0].cpu().numpy()
    hs, hsc = slope[0].cpu().numpy(), scale[0].cpu().numpy()
    img = images[0].cpu().numpy().astype(np.float64)
    chain = vs.codec_grad_host(host, 100, "444", tone[0].cpu().numpy(), "ste", img, hs, hsc, bound=True, consts=consts)
    img_mag = np.stack([vs.prepare_grad_image_host(g[0, t], Hs, Ws, bound=True, **GEOM)[1] for t in range(T)])
    n_img = vs.prepare_grad_image_host(g[0, 0], Hs, Ws, bound=True, **GEOM)[2]
    carried = vs.codec_grad_host(host, 100, "444", tone[0].cpu().numpy(), "ste", img_mag, hs, hsc, bound=True, consts=consts)["gdelta_mag"]
    _, mag_b, n_b = vs.prepare_grad_host(host, idx[0], g[0], hs, hsc, bound=True, **GEOM)
    bound = U * (chain["gdelta_roundings"] * chain["gdelta_mag"] + n_img * carried + (n_b + 16) * mag_b)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(f"seam: worst error / bound = {float((err / bound).max()):.4f}; |gdelta| up to {float(np.abs(ref).max()):.4g}")
    assert np.abs(ref).max() > 0 and (err <= bound).all(), (err, bound)


# ---- engine ------------------------------------------------------------------------------------------------------------------------
T, HW = 8, 64
FIXED = {"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}
CODEC = dict(quality=60, subsampling="420")
_ENGINES = {}


def engine(**kw):
    """mc3_18 on synthetic weights, 8 frames of 64 x 64, bf16, flicker on video time, trained on the delivered, compressed video"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    kw = dict(dict(batch_size=2, sample_length=T, image_size=HW, im_scale=HW, dtype="bf16", l_inf_pert_norm=0.2, flicker_time="video", flicker_period=5,
                   train_delivered=True, codec=vs.Codec(**CODEC)), **kw)
    key = tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _ENGINES:
        _ENGINES[key] = FlickerVideoResNet("mc3_18", vs.synthetic_weights("mc3_18", 42), **kw)
    eng = _ENGINES[key]
    rng = np.random.default_rng(13 + eng.P)
    eng.pert_model.init_perturbation(rng.uniform(-0.25, 0.25, (3, eng.P, 1, 1)).astype(np.float32))      # beyond the bound of 0.2 too
    eng.pert_model.dynamic_max_norm = eng.pert_model.max_norm
    return eng


def criterion():
    from flickering_adversarial_video_amd.torch_attack import Losses
    return Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)


@pytest.fixture(scope="module")
def raw():
    """two raw videos of differing length and resolution, neither a whole number of 16 x 16 MCUs: 20 x 72 x 100 and 14 x 90 x 82"""
    rng = np.random.default_rng(17)
    vids = []
    for n, h, w in ((20, 72, 100), (14, 90, 82)):
        yy, xx = np.mgrid[0:h, 0:w]
        v = np.stack([np.stack([128 + 80 * np.sin(yy / 6.0 + 0.3 * t + c) * np.cos(xx / 8.0 - 0.2 * t) for c in range(3)], -1) for t in range(n)])
        v = np.clip(v + rng.normal(0, 6, v.shape), 0, 255).astype(np.uint8)
        v[:, :2], v[:, 2:4] = 0, 255
        vids.append(torch.from_numpy(v).cuda())
    return vids


def clean_labels(eng, videos):
    return torch.from_numpy(eng.evaluate_videos(videos, np.zeros(len(videos), np.int64), num_samples=1)["video_preds"]).cuda()


def host_clip_gradient(vs, ops, eng, raw, mode, model):
    """the host chain on the engine's own input gradient: float64 [B,T,3] with its bound"""
    pm = eng.pert_model
    rows = np.concatenate(eng.last_sampling)
    slope, scale = (x.cpu().numpy() for x in (eng._slope[:2], eng._scale[:2]))
    tone = eng._tone[:2].cpu().numpy()
    g = unfold1(eng._gx)
    want, bound = np.zeros((2, T, 3)), np.zeros((2, T, 3))
    for k, v in enumerate(raw):
        Hs, Ws = int(v.shape[1]), int(v.shape[2])
        parts = [vs.prepare_grad_image_host(g[k, t], Hs, Ws, bound=True, im_scale=HW, input_size=HW) for t in range(T)]
        img, img_mag, n_img = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), parts[0][2]
        frames = v.cpu().numpy()[rows[k]]
        consts = vs.codec_quant_slopes_host(frames, CODEC["quality"], CODEC["subsampling"], tone[k], mode)
        res = vs.codec_grad_host(frames, CODEC["quality"], CODEC["subsampling"], tone[k], mode, img, slope[k], scale[k], bound=True, consts=consts)
        carried = vs.codec_grad_host(frames, CODEC["quality"], CODEC["subsampling"], tone[k], mode, img_mag, slope[k], scale[k], bound=True, consts=consts)
        want[k] = res["gdelta"]
        bound[k] = U * (res["gdelta_roundings"] * carried["gdelta_mag"] + n_img * carried["gdelta_mag"])
    return want, bound


@pytest.mark.parametrize("model", ["additive", "illumination"])
def test_engine_payload_is_the_host_chain_on_its_input_gradient(env, raw, model):
    ops, vs = env["ops"], env["vs"]
    ident = engine(flicker_model=model)
    labels = clean_labels(ident, raw)
    ident.step_videos(raw, labels, criterion(), update=False, train=False)
    logits, payload = ident._logits.clone(), ident._red[:15].clone()
    for mode in (("ste", "cubic") if model == "additive" else ("cubic",)):
        eng = engine(flicker_model=model, codec_grad=mode)
        eng.step_videos(raw, labels, criterion(), update=False, train=False)
        assert same_bits(eng._logits, logits)                                                        # the forward is the same integer codec
        assert float(eng._red[:15].abs().max()) > 0 and not same_bits(eng._red[:15], payload)        # ... the backward is not
        want, bound = host_clip_gradient(vs, ops, eng, raw, mode, model)
        got = eng._g_clip.cpu().numpy().astype(np.float64)
        worst = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
        print(f"engine {model} {mode}: per-clip gradient worst error / bound = {worst:.4f}")
        assert (np.abs(got - want) <= bound).all()
        pm = eng.pert_model
        assert same_bits(eng._red[:15].view(5, 3), ops.flicker_rows_grad(eng._g_clip, pm.rows_dev, 5))
        rows = pm.rows_dev.cpu().numpy()
        fold, fold_bound = np.zeros((5, 3)), np.zeros((5, 3))
        np.add.at(fold, rows.reshape(-1), want.reshape(-1, 3))
        np.add.at(fold_bound, rows.reshape(-1), (bound + 2 * T * U * np.abs(want)).reshape(-1, 3))
        assert (np.abs(eng._red[:15].view(5, 3).cpu().numpy() - fold) <= fold_bound).all()           # the [P,3] payload: the host chain, folded


def test_engine_through_a_fixed_capture_channel(env, raw):
    ops, vs = env["ops"], env["vs"]
    ch = vs.CaptureChannel(subframe=FIXED["subframe"], exposure=FIXED["exposure"], gain=FIXED["gain"], gain_mode="per_channel")
    ident, eng = engine(capture=ch), engine(capture=ch, codec_grad="cubic")
    labels = clean_labels(ident, raw)
    ident.step_videos(raw, labels, criterion(), update=False, train=False)
    eng.step_videos(raw, labels, criterion(), update=False, train=False)
    assert same_bits(eng._logits, ident._logits) and not same_bits(eng._red[:15], ident._red[:15])
    want, bound = host_clip_gradient(vs, ops, eng, raw, "cubic", "additive")
    assert (np.abs(eng._g_clip.cpu().numpy() - want) <= bound).all()
    pm = eng.pert_model
    assert same_bits(eng._red[:15].view(5, 3), ops.flicker_rows_mix_grad(eng._g_clip, pm.rows_dev, 5, pm.taps_dev, pm.gain_dev))


def test_identity_is_the_engine_built_without_the_keyword(raw):
    """three updating steps: the engine given codec_grad="identity" is, bit for bit, the one never handed the keyword"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    common = dict(batch_size=2, sample_length=T, image_size=HW, im_scale=HW, dtype="bf16", l_inf_pert_norm=0.2, flicker_time="video", flicker_period=5,
                  train_delivered=True, codec=vs.Codec(**CODEC), optimizer="pgd")
    W = vs.synthetic_weights("mc3_18", 42)
    outs = []
    for kw in ({}, {"codec_grad": "identity"}):
        eng = FlickerVideoResNet("mc3_18", W, **common, **kw)
        labels = clean_labels(eng, raw)
        for _ in range(3):
            eng.step_videos(raw, labels, criterion(), lr=1e-2, update=True, train=True)
        outs.append((eng._logits.clone(), eng.pert_model.perturbation.clone(), eng._red.clone()))
        assert not hasattr(eng, "_g_img")
    assert all(same_bits(p, q) for p, q in zip(*outs))
