"""The codec round trip on the GPU: flk_codec_roundtrip_u8 BITWISE its numpy integer restatement (videoresnet_spec.codec_roundtrip_host)
over sizes, qualities, subsamplings, contents, views, clip tables, frame tables and tone tables; then the engine: export, evaluation and
the delivered-video training forward through the codec, and the identity step_videos(train=False) == evaluate_videos(quantise="video",
codec=)."""
import numpy as np
import pytest
import torch

import codec_mc_cases as cases

pytestmark = pytest.mark.gpu
SUBS = ("444", "420")
QUALITIES = (1, 50, 75, 95, 100)
SIZES = ((8, 8), (16, 16), (1, 1), (17, 23), (24, 40), (33, 16), (48, 200))


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def smooth(N, H, W, seed):
    """smooth luminance and chroma plus noise, a different phase per frame"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for n in range(N):
        img = np.stack([128 + 70 * np.sin(xx / 9. + n) + 40 * np.cos(yy / 5.), 120 + 60 * np.cos(xx / 13. + yy / 7. - n),
                        100 + 80 * np.sin(yy / 11. + 2 * n) - 30 * np.cos(xx / 4.)], -1) + rng.normal(0, 8, (H, W, 3))
        out.append(np.clip(np.rint(img), 0, 255))
    return np.stack(out).astype(np.uint8)


def checker(N, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.broadcast_to(np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1), (N, H, W, 3)).copy()


@pytest.fixture(scope="module")
def env():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    return dict(ops=ops, vs=vs)


_WANT = {}


def want(vs, x, q, sub, key=None):
    """the restatement's result (and stats), computed once per fixture and setting and left unchanged"""
    k = (key, q, sub) if key is not None else None
    if k is None or k not in _WANT:
        res = vs.codec_roundtrip_host(x, q, sub, stats=True)
        if k is None:
            return res
        _WANT[k] = res
    return _WANT[k]


# ---- kernel == restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_is_the_restatement(env, size, sub):
    """every size of the list (one MCU, a 1 x 1 frame, odd sizes, a multiple of 8 but not of 16, two tiles wide) at every quality: one
    launch holds the size's frames at one setting; outputs and stats bit for bit"""
    ops, vs = env["ops"], env["vs"]
    H, W = size
    N = 3 if H * W < 2000 else 2
    x = smooth(N, H, W, seed=H * 1000 + W)
    xd = torch.from_numpy(x).cuda()
    for q in QUALITIES:
        (got,), (st,) = ops.codec_roundtrip([xd], vs.Codec(q, sub), stats=True)
        exp, exp_st = want(vs, x, q, sub)
        assert same_bits(got, exp), (size, q, sub, int(np.abs(got.cpu().numpy().astype(int) - exp.astype(int)).max()))
        assert same_bits(st, exp_st), (size, q, sub, st.cpu().numpy(), exp_st)
    assert exp_st[:, 0].min() > 0                                                  # quality 100: every frame has non-zero levels


def test_native_size(env):
    ops, vs = env["ops"], env["vs"]
    x = smooth(2, 240, 320, seed=5)
    (got,), (st,) = ops.codec_roundtrip([torch.from_numpy(x).cuda()], vs.Codec(75, "420"), stats=True)
    exp, exp_st = vs.codec_roundtrip_host(x, 75, "420", stats=True)
    assert same_bits(got, exp) and same_bits(st, exp_st)
    assert not same_bits(got, x)


@pytest.mark.parametrize("sub", SUBS)
def test_extreme_contents(env, sub):
    """the 0 / 255 checkerboard (saturation on both sides, the largest AC energy), independent 0 / 255 per channel, all-0 and all-255"""
    ops, vs = env["ops"], env["vs"]
    rng = np.random.RandomState(3)
    x = np.concatenate([checker(1, 33, 40), rng.choice(np.array([0, 255], np.uint8), (1, 33, 40, 3)), np.zeros((1, 33, 40, 3), np.uint8),
                        np.full((1, 33, 40, 3), 255, np.uint8)])
    xd = torch.from_numpy(x).cuda()
    for q in (1, 25, 75, 100):
        (got,), (st,) = ops.codec_roundtrip([xd], vs.Codec(q, sub), stats=True)
        exp, exp_st = vs.codec_roundtrip_host(x, q, sub, stats=True)
        assert same_bits(got, exp) and same_bits(st, exp_st), (q, sub)
    assert same_bits(got[2], x[2]) and same_bits(got[3], x[3])                     # black and white are fixed points at quality 100


# ---- views ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub,geom", cases.VIEW_GEOMETRIES, ids=cases.VIEW_IDS)
def test_source_and_destination_views(env, sub, geom):
    """the source a view of a wider and longer video, starting 0..3 bytes off a 4-byte boundary; the destination a view with pitches of
    its own, also off alignment: the result is the contiguous call's and no byte outside the destination view changes.  "seams": a
    view of several tiles, the last ones partial (codec_mc_cases.check_views_across_tile_seams)"""
    ops, vs = env["ops"], env["vs"]
    if geom == "seams":
        return cases.check_views_across_tile_seams(ops, vs, sub)
    codec = vs.Codec(60, sub)
    big = smooth(5, 30, 150, seed=11)
    for off in (0, 1, 2, 3):
        buf = torch.empty(big.size + 8, dtype=torch.uint8, device="cuda")
        whole = buf[off:off + big.size].view(big.shape)
        whole.copy_(torch.from_numpy(big))
        src = whole[1:4, 3:22, 5:42]                                               # 3 x 19 x 37 inside 5 x 30 x 150
        assert src.data_ptr() % 4 == (off + 1 * 30 * 450 + 3 * 450 + 15) % 4
        exp, _ = vs.codec_roundtrip_host(big[1:4, 3:22, 5:42], 60, sub, stats=True)
        assert same_bits(ops.codec_roundtrip([src], codec)[0], exp), off
        dbuf = torch.full((4 * 25 * 50 * 3 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        dwhole = dbuf[off + 1:off + 1 + 4 * 25 * 50 * 3].view(4, 25, 50, 3)
        dst = dwhole[1:4, 2:21, 7:44]
        before = dbuf.clone()
        out = ops.codec_roundtrip([src], codec, out=[dst])
        assert out[0].data_ptr() == dst.data_ptr() and same_bits(dst, exp), off
        mask = torch.zeros_like(dwhole, dtype=torch.bool)
        mask[1:4, 2:21, 7:44] = True
        assert bool((dwhole[~mask] == 0xA5).all()) and same_bits(dbuf[:off + 1], before[:off + 1]) and same_bits(dbuf[-7 + off:], before[-7 + off:])


def test_refused_before_launch(env):
    ops, vs = env["ops"], env["vs"]
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="overlaps"):
        ops.codec_roundtrip([x], vs.Codec(), out=[x])
    with pytest.raises(ValueError, match="out"):
        ops.codec_roundtrip([x], vs.Codec(), out=[torch.zeros((2, 8, 9, 3), dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError, match="frame_idx"):
        ops.codec_roundtrip([x], vs.Codec(), frame_idx=[[0, 2]])
    with pytest.raises(ValueError, match="tone"):
        ops.codec_roundtrip([x], vs.Codec(), tone=torch.zeros((1, 3, 256, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="Codec"):
        ops.codec_roundtrip([x], 75)


# ---- clip tables ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(env):
    """clips of differing length and resolution, the second one byte off alignment"""
    hosts = [smooth(3, 17, 23, 21), smooth(2, 48, 200, 22), smooth(3, 24, 40, 23), smooth(3, 1, 1, 24), checker(2, 33, 16)]
    devs = []
    for k, h in enumerate(hosts):
        buf = torch.empty(h.size + 4, dtype=torch.uint8, device="cuda")
        v = buf[k % 4:k % 4 + h.size].view(h.shape)
        v.copy_(torch.from_numpy(h))
        devs.append(v)
    return hosts, devs


@pytest.mark.parametrize("sub", SUBS)
def test_several_clips_of_differing_resolution_in_one_call(env, mixed, sub):
    ops, vs = env["ops"], env["vs"]
    hosts, devs = mixed
    codec = vs.Codec(75, sub)
    outs, sts = ops.codec_roundtrip(devs, codec, stats=True)
    for k, (h, d) in enumerate(zip(hosts, devs)):
        exp, exp_st = want(vs, h, 75, sub, key=("mixed", k))
        assert same_bits(outs[k], exp) and same_bits(sts[k], exp_st), k
        (one,), (one_st,) = ops.codec_roundtrip([d], codec, stats=True)
        assert same_bits(one, outs[k]) and same_bits(one_st, sts[k]), k
    # equal lengths: ONE launch holds the three 3-frame clips of differing resolution
    idx = [0, 2, 3]
    outs3 = ops.codec_roundtrip([devs[k] for k in idx], codec)
    assert all(same_bits(o, outs[k]) for o, k in zip(outs3, idx))


def test_more_than_64_clips(env):
    ops, vs = env["ops"], env["vs"]
    rng = np.random.RandomState(9)
    hosts = [smooth(2, 9 + (k % 3), 11 + (k % 5), 100 + k) for k in range(70)]
    outs = ops.codec_roundtrip([torch.from_numpy(h).cuda() for h in hosts], vs.Codec(50, "420"))
    assert len(outs) == 70
    for k in (0, 1, 31, 63, 64, 65, 69):
        assert same_bits(outs[k], vs.codec_roundtrip_host(hosts[k], 50, "420")), k
    idx = rng.randint(0, 2, (70, 3))
    outs = ops.codec_roundtrip([torch.from_numpy(h).cuda() for h in hosts], vs.Codec(50, "420"), frame_idx=idx)
    for k in (0, 63, 64, 69):
        assert same_bits(outs[k], vs.codec_roundtrip_host(hosts[k][idx[k]], 50, "420")), k


# ---- frame tables and tone tables ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_frame_idx_is_the_launch_on_gathered_frames(env, sub):
    ops, vs = env["ops"], env["vs"]
    hosts = [smooth(7, 17, 23, 31), smooth(4, 24, 40, 32)]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    idx = np.array([[6, 0, 0, 3, 3, 3], [1, 3, 3, 0, 2, 2]])
    codec = vs.Codec(75, sub)
    outs, sts = ops.codec_roundtrip(devs, codec, frame_idx=idx, stats=True)
    gathered = ops.codec_roundtrip([d[torch.as_tensor(r, device="cuda")].contiguous() for d, r in zip(devs, idx)], codec)
    for k in range(2):
        assert tuple(outs[k].shape) == (6,) + hosts[k].shape[1:]
        assert same_bits(outs[k], gathered[k])
        exp, exp_st = vs.codec_roundtrip_host(hosts[k][idx[k]], 75, sub, stats=True)
        assert same_bits(outs[k], exp) and same_bits(sts[k], exp_st)
    assert same_bits(outs[0][1], outs[0][2]) and same_bits(outs[0][3], outs[0][5])      # repeated frames: computed again, equal


@pytest.mark.parametrize("model", ["additive", "illumination"])
@pytest.mark.parametrize("sub", SUBS)
def test_tone_is_the_launch_on_the_exported_video(env, sub, model):
    ops, vs = env["ops"], env["vs"]
    from flickering_adversarial_video_amd.torch_attack import decode_table
    lo, hi = vs.additive_bounds()
    kw = dict(dialect="torch", dclip=0.6, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo, hi=hi)
    illum = ops.make_illum_args(vs.illum_tables("srgb")) if model == "illumination" else None
    lut = decode_table("cuda")
    rng = np.random.default_rng(41)
    hosts = [smooth(6, 17, 23, 41), smooth(6, 24, 40, 42)]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    delta = torch.from_numpy(rng.uniform(-0.8, 0.8, (2, 6, 3)).astype(np.float32)).cuda()        # beyond the clamp too
    tone = ops.flicker_tone_tables(ops.make_export_apply_args(ops.tone_ramp(2, 6), delta, x_lut=lut, **kw), illum)
    codec = vs.Codec(75, sub)
    got = ops.codec_roundtrip(devs, codec, tone=tone)
    exported = []
    for k, d in enumerate(devs):
        a = ops.make_export_apply_args(d[None].contiguous(), delta[k:k + 1].contiguous(), x_lut=lut, **kw)
        exported.append((ops.illum_export_u8(a, illum) if illum is not None else ops.export_adversarial_u8(a, "torch"))[0])
    plain = ops.codec_roundtrip(exported, codec)
    for k in range(2):
        assert same_bits(got[k], plain[k]), k
        assert same_bits(got[k], vs.codec_roundtrip_host(hosts[k], 75, sub, tone=tone[k].cpu().numpy())), k
        assert not same_bits(exported[k], devs[k])
    # with a frame table as well: the tone of OUTPUT frame t on source frame idx[t]
    idx = np.array([[5, 5, 0, 2, 2, 1], [0, 1, 1, 4, 3, 3]])
    got = ops.codec_roundtrip(devs, codec, frame_idx=idx, tone=tone)
    for k in range(2):
        assert same_bits(got[k], vs.codec_roundtrip_host(hosts[k][idx[k]], 75, sub, tone=tone[k].cpu().numpy())), k
    ident = torch.arange(256, dtype=torch.uint8, device="cuda").view(1, 1, 256, 1).expand(2, 6, 256, 3).contiguous()
    assert all(same_bits(p, q) for p, q in zip(ops.codec_roundtrip(devs, codec, tone=ident), ops.codec_roundtrip(devs, codec)))


# ---- engine --------------------------------------------------------------------------------------------------------------------
T, HW = 8, 64
FIXED = {"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}
_ENGINES = {}


def engine(**kw):
    """mc3_18 on synthetic weights, 8 frames of 64 x 64, bf16, flicker on video time; one engine per setting for the module"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    kw = dict(dict(batch_size=2, sample_length=T, image_size=HW, im_scale=HW, dtype="bf16", l_inf_pert_norm=0.2, flicker_time="video"), **kw)
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
    vids = [smooth(20, 72, 100, 51), smooth(14, 90, 82, 52)]
    for v in vids:
        v[:, :2], v[:, 2:4] = 0, 255
    return [torch.from_numpy(v).cuda() for v in vids]


def clean_labels(eng, videos, num_samples=1):
    return torch.from_numpy(eng.evaluate_videos(videos, np.zeros(len(videos), np.int64), num_samples=num_samples)["video_preds"]).cuda()


CODEC = dict(quality=60, subsampling="420")


def test_export_video_through_the_codec(env, raw):
    ops, vs = env["ops"], env["vs"]
    eng = engine(flicker_period=5)
    codec = vs.Codec(**CODEC)
    plain, st = eng.export_video(raw[0], phase=2, stats=True)
    got, st2 = eng.export_video(raw[0], phase=2, stats=True, codec=codec)
    assert same_bits(got, ops.codec_roundtrip([plain], codec)[0]) and same_bits(st, st2)
    assert same_bits(eng.export_video(raw[0], phase=2, codec=codec), got) and not same_bits(got, plain)
    assert same_bits(eng.export_video(raw[0], phase=2, capture=FIXED, codec=codec),
                     ops.codec_roundtrip([eng.export_video(raw[0], phase=2, capture=FIXED)], codec)[0])
    with pytest.raises(ValueError, match="Codec"):
        eng.export_video(raw[0], codec=(60, "420"))


def test_evaluate_videos_through_the_codec_is_the_chain_by_hand(env, raw):
    ops, vs = env["ops"], env["vs"]
    eng = engine(flicker_period=5)
    codec = vs.Codec(**CODEC)
    labels = clean_labels(eng, raw, 2).cpu().numpy()
    ev = eng.evaluate_videos(raw, labels, num_samples=2, quantise="video", codec=codec)
    rows = np.concatenate(eng.last_sampling)
    stored, stats = ops.codec_roundtrip([eng.export_video(v) for v in raw], codec, stats=True)
    parts = []
    for first in (0, 2):
        x = ops.prepare_clips([stored[k // 2] for k in range(first, first + 2)], im_scale=HW, input_size=(HW, HW), frame_idx=rows[first:first + 2])
        parts.append(eng.logits(x, False).cpu().clone())
    assert same_bits(ev["clip_logits"], torch.cat(parts))
    assert len(ev["codec_stats"]) == 2 and all(same_bits(a, b) for a, b in zip(ev["codec_stats"], stats))
    plain = eng.evaluate_videos(raw, labels, num_samples=2, quantise="video")
    assert not same_bits(ev["clip_logits"], plain["clip_logits"]) and same_bits(ev["clean_clip_logits"], plain["clean_clip_logits"])
    assert set(ev) == set(plain) | {"codec_stats"}
    # through capture draws as well: every draw's exported videos are compressed
    ch = vs.CaptureChannel(subframe=(0.0, 1.0), exposure=(0.5, 2.0), gain=(0.5, 1.0), seed=3)
    evc = eng.evaluate_videos(raw, labels, num_samples=1, quantise="video", capture=ch, capture_draws=1, codec=codec)
    d = evc["capture_draws"][0]
    exp = [eng.export_video(v, capture={k: (d[k][i] if k == "gain" else float(d[k][i])) for k in d}, codec=codec) for i, v in enumerate(raw)]
    x = ops.prepare_clips(exp, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling))
    assert same_bits(evc["capture_clip_logits"][0], eng.logits(x, False))


def test_evaluate_videos_without_a_codec_is_unchanged(raw):
    """codec=None: the keys and values of an engine that was never handed the keyword"""
    eng = engine(flicker_period=5)
    labels = clean_labels(eng, raw).cpu().numpy()
    a = eng.evaluate_videos(raw, labels, num_samples=2, quantise="video", codec=None)
    b = eng.evaluate_videos(raw, labels, num_samples=2, quantise="video")
    assert set(a) == set(b) and "codec_stats" not in a
    for k in a:
        if k == "realised_flicker":
            assert all(same_bits(p, q) for p, q in zip(a[k], b[k]))
        elif isinstance(a[k], np.ndarray):
            assert same_bits(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


@pytest.mark.parametrize("model", ["additive", "illumination"])
@pytest.mark.parametrize("P", [5, 8])
def test_step_videos_scores_what_evaluate_videos_scores_through_the_codec(env, raw, P, model):
    vs = env["vs"]
    codec = vs.Codec(**CODEC)
    eng = engine(flicker_period=P, flicker_model=model, train_delivered=True, codec=codec)
    labels = clean_labels(eng, raw)
    r = eng.step_videos(raw, labels, criterion(), update=False, train=False)
    logits, argmax = eng._logits.clone(), r["argmax"].clone()
    ev = eng.evaluate_videos(raw, labels.cpu().numpy(), num_samples=1, quantise="video", codec=codec)
    assert same_bits(logits, ev["clip_logits"])
    assert np.array_equal(argmax.cpu().numpy().astype(np.int64), ev["clip_preds"])
    plain = eng.evaluate_videos(raw, labels.cpu().numpy(), num_samples=1, quantise="video")
    assert not same_bits(logits, plain["clip_logits"]) and not same_bits(logits, ev["clean_clip_logits"])


def test_step_videos_through_a_fixed_capture_channel_and_the_codec(env, raw):
    ops, vs = env["ops"], env["vs"]
    codec = vs.Codec(**CODEC)
    ch = vs.CaptureChannel(subframe=FIXED["subframe"], exposure=FIXED["exposure"], gain=FIXED["gain"], gain_mode="per_channel")
    eng = engine(flicker_period=8, train_delivered=True, capture=ch, codec=codec)
    labels = clean_labels(eng, raw)
    eng.step_videos(raw, labels, criterion(), update=False, train=False)
    logits = eng._logits.clone()
    exported = [eng.export_video(v, capture=FIXED, codec=codec) for v in raw]
    x = ops.prepare_clips(exported, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling))
    assert same_bits(logits, eng.logits(x, False))
    uncompressed = [eng.export_video(v, capture=FIXED) for v in raw]
    assert not same_bits(logits, eng.logits(ops.prepare_clips(uncompressed, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling)), False))


def test_step_videos_trains_through_the_codec_straight_through(env, raw):
    """update=True for a few steps: the perturbation moves.  The backward is the train_delivered one on the source videos (the codec's
    Jacobian taken as the identity): handed the input gradient of the codec step, the no-codec chain of slopes, resampling and row fold
    reproduces the codec step's payload bit for bit -- the same launches on the same inputs"""
    ops, vs = env["ops"], env["vs"]
    eng = engine(flicker_period=5, train_delivered=True, optimizer="pgd", codec=vs.Codec(**CODEC))
    labels = clean_labels(eng, raw)
    before = eng.pert_model.perturbation.clone()
    r = eng.step_videos(raw, labels, criterion(), update=False, train=False)
    pm = eng.pert_model
    a = pm.export_args(ops.tone_ramp(2, T), True, shift_p=0)
    slope, scale = ops.flicker_tone_slopes(a, None)
    g_clip = ops.prepare_clips_grad(raw, eng._gx, slope, scale, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling))
    expect = ops.flicker_rows_grad(g_clip, pm.rows_dev, 5)
    assert float(expect.abs().max()) > 0 and same_bits(eng._red[:15].view(5, 3), expect)
    for _ in range(3):
        r = eng.step_videos(raw, labels, criterion(), lr=1e-2, update=True, train=True)
        assert np.isfinite(float(r["loss"]))
    assert not same_bits(before, eng.pert_model.perturbation)


def test_refusals(env, raw):
    vs = env["vs"]
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    W = vs.synthetic_weights("mc3_18", 42)
    kw = dict(batch_size=2, sample_length=T, image_size=HW, dtype="bf16", flicker_time="video")
    with pytest.raises(ValueError, match="train_delivered"):
        FlickerVideoResNet("mc3_18", W, codec=vs.Codec(), **kw)
    with pytest.raises(ValueError, match="Codec"):
        FlickerVideoResNet("mc3_18", W, train_delivered=True, codec=75, **kw)
    eng = engine(flicker_period=5)
    labels = np.zeros(2, np.int64)
    for quantise in ("clip", None):
        with pytest.raises(ValueError, match="quantise='video'"):
            eng.evaluate_videos(raw, labels, num_samples=1, quantise=quantise, codec=vs.Codec())
    for q, s in ((0, "420"), (101, "420"), (75, "422"), (75, "411")):
        with pytest.raises(ValueError):
            vs.Codec(q, s)


def test_universal_script_trains_delivered_through_the_codec(tmp_path):
    """one --train-delivered --codec-quality run of the universal script on a tiny raw whole-video file finishes and writes its results"""
    import glob
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(1)
    vids = {f"video_{k:05d}": rng.integers(0, 256, (12 + k, 72, 96, 3)).astype(np.uint8) for k in range(2)}
    path = str(tmp_path / "raw.npz")
    np.savez(path, labels=np.array([1, 2], np.int64), **vids)
    base = [sys.executable, os.path.join(root, "scripts", "r2plus1d_main_universal_attack.py"), "--train-npz", path, "--val-npz", path, "--base-model", "r3d_18",
            "--batch-size", "2", "--sample-length", "8", "--image-size", "64", "--im-scale", "64", "--epochs", "1", "--flicker-time", "video",
            "--flicker-period", "5"]
    r = subprocess.run(base + ["--train-delivered", "--codec-quality", "60", "--eval-quantised", "video", "--results-root", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "epoch 1" in r.stdout and "Codec(quality=60" in r.stdout
    files = glob.glob(str(tmp_path / "out" / "**" / "video_eval_quantised.npz"), recursive=True)
    assert len(files) == 1
    ev = np.load(files[0])
    assert int(ev["codec_quality"]) == 60 and str(ev["codec_subsampling"]) == "420" and ev["codec_stats"].shape == (12 + 13, 2)
    bad = subprocess.run(base + ["--codec-quality", "60", "--results-root", str(tmp_path / "out2")], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--codec-quality" in bad.stderr
    bad = subprocess.run(base + ["--train-delivered", "--codec-subsampling", "444", "--results-root", str(tmp_path / "out3")], capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode != 0 and "--codec-quality" in bad.stderr
