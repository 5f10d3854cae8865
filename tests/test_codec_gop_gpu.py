"""Inter-frame prediction in the codec on the GPU: flk_codec_roundtrip_gop_u8 BITWISE its numpy integer restatement
(videoresnet_spec.codec_roundtrip_host(gop=, first_frame=)) over subsamplings, qualities, GOP lengths, frame sizes, spans, tone tables,
views and contents; then the engine: export, evaluation and the delivered-video training forward through a codec with GOPs, and the
identity step_videos(train=False) == evaluate_videos(quantise="video", codec=)."""
import numpy as np
import pytest
import torch

import codec_mc_cases as cases

pytestmark = pytest.mark.gpu
SUBS = ("444", "420")
QUALITIES = (1, 50, 75, 100)
# one MCU; one 4:2:0 MCU; no whole MCU and less than one tile; 2 x 2 tiles at 4:2:0; 2 x 2 tiles at 4:4:4
SIZES = ((8, 8), (16, 16), (90, 82), (66, 130), (34, 130))


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def moving(N, H, W, seed):
    """smooth luminance and chroma plus noise, drifting from frame to frame: P-frames with small and with large residuals"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for n in range(N):
        img = np.stack([128 + 70 * np.sin(xx / 9. + n / 3.) + 40 * np.cos(yy / 5.), 120 + 60 * np.cos(xx / 13. + yy / 7. - n / 4.),
                        100 + 80 * np.sin(yy / 11. + n / 5.) - 30 * np.cos(xx / 4.)], -1) + rng.normal(0, 6, (H, W, 3))
        out.append(np.clip(np.rint(img), 0, 255))
    return np.stack(out).astype(np.uint8)


def checker(H, W, inverse=False):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat(((((yy + xx + int(inverse)) & 1)) * 255).astype(np.uint8)[..., None], 3, -1)


@pytest.fixture(scope="module")
def env():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    return dict(ops=ops, vs=vs)


# ---- kernel == restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_is_the_restatement(env, size, sub):
    """videos of N = 1 and N = 7 frames in one launch per (quality, gop), gop in {2, 3, N, N + 5}: a lone intra frame, whole and cut
    GOPs, one GOP that is the video, a GOP longer than the video; outputs and stats bit for bit"""
    ops, vs = env["ops"], env["vs"]
    H, W = size
    hosts = [moving(1, H, W, seed=H + W), moving(7, H, W, seed=H * 1000 + W)]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    p_levels = 0
    for q in QUALITIES:
        for gop in (1, 2, 3, 6, 7, 12):                           # {2, 3, N, N + 5} of N = 1 (gop 1: the intra entry) and of N = 7
            outs, sts = ops.codec_roundtrip(devs, vs.Codec(q, sub, gop=gop), stats=True)
            for h, o, st in zip(hosts, outs, sts):
                exp, exp_st = vs.codec_roundtrip_host(h, q, sub, stats=True, gop=gop)
                assert same_bits(o, exp), (size, q, sub, gop, len(h), int(np.abs(o.cpu().numpy().astype(int) - exp.astype(int)).max()))
                assert same_bits(st, exp_st), (size, q, sub, gop, st.cpu().numpy(), exp_st)
                p_levels += int(exp_st[1:2, 0].sum())
    assert p_levels > 0                                           # P-frames with levels were among them


@pytest.mark.parametrize("sub", SUBS)
def test_gop_1_is_the_intra_launch(env, sub):
    ops, vs = env["ops"], env["vs"]
    x = torch.from_numpy(moving(5, 33, 40, seed=3)).cuda()
    for q in (50, 100):
        (a,), (sa,) = ops.codec_roundtrip([x], vs.Codec(q, sub), stats=True)
        (b,), (sb,) = ops.codec_roundtrip([x], vs.Codec(q, sub, gop=1), stats=True)
        assert same_bits(a, b) and same_bits(sa, sb)
        assert same_bits(ops.codec_roundtrip([x], vs.Codec(q, sub, gop=1), frame_idx=[[4, 0, 0]])[0], ops.codec_roundtrip([x], vs.Codec(q, sub), frame_idx=[[4, 0, 0]])[0])


def test_the_gop_entry_at_gop_1_is_the_intra_entry(env):
    """the wrapper sends gop 1 to flk_codec_roundtrip_u8; the GOP entry itself takes it too (every frame an intra frame), spans included"""
    import ctypes as C
    from flickering_adversarial_video_amd import _lib
    ops, vs = env["ops"], env["vs"]
    host = moving(5, 33, 40, seed=4)
    x = torch.from_numpy(host).cuda()
    out = torch.zeros((3, 33, 40, 3), dtype=torch.uint8, device="cuda")
    st = torch.empty((1, 3, 2), dtype=torch.int32, device="cuda")
    arr = (_lib.CodecClip * 1)()
    d = arr[0]
    d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = x.data_ptr(), 5, 33, 40, x.stride(0), x.stride(1)
    d.dst, d.dst_pitch_t, d.dst_pitch_h = out.data_ptr(), out.stride(0), out.stride(1)
    a = _lib.CodecArgs()
    a.nclip, a.quality, a.subsampling, a.clips = 1, 50, _lib.FLK_CODEC_420, arr
    _lib.check(_lib.load().flk_codec_roundtrip_gop_u8(C.byref(a), 1, (C.c_int32 * 1)(2), (C.c_int32 * 1)(3), 3, None, _lib.ptr(st), _lib.stream_ptr()))
    exp, exp_st = vs.codec_roundtrip_host(host[2:5], 50, "420", stats=True)
    assert same_bits(out, exp) and same_bits(st[0], exp_st)


@pytest.mark.parametrize("sub", SUBS)
def test_extreme_contents_and_determinism(env, sub):
    """the largest residuals: the 0 / 255 checkerboard against its inverse, flat 0 against flat 255, independent 0 / 255 per channel;
    gop 4 over 6 frames at every quality of the overflow check; two runs give equal bytes"""
    ops, vs = env["ops"], env["vs"]
    rng = np.random.RandomState(5)
    H, W = 24, 32
    hosts = [np.stack([checker(H, W, n & 1) for n in range(6)]), np.stack([np.full((H, W, 3), 255 * (n & 1), np.uint8) for n in range(6)]),
             rng.choice(np.array([0, 255], np.uint8), (6, H, W, 3))]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    for q in (1, 25, 50, 75, 100):
        codec = vs.Codec(q, sub, gop=4)
        outs, sts = ops.codec_roundtrip(devs, codec, stats=True)
        again, sts2 = ops.codec_roundtrip(devs, codec, stats=True)
        for k, h in enumerate(hosts):
            exp, exp_st = vs.codec_roundtrip_host(h, q, sub, stats=True, gop=4)
            assert same_bits(outs[k], exp) and same_bits(sts[k], exp_st), (q, sub, k)
            assert same_bits(outs[k], again[k]) and same_bits(sts[k], sts2[k])
    assert same_bits(outs[1], hosts[1])                           # quality 100: black <-> white is reproduced


# ---- spans, clip tables, tone tables -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    """three videos of differing resolution and length"""
    return [moving(11, 17, 23, 21), moving(9, 48, 200, 22), moving(14, 40, 24, 23)]


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("gop", [2, 3])
def test_one_launch_of_three_videos_with_their_own_spans(env, three, sub, gop):
    """firsts 0, gop and 2 gop, differing counts; the second video has fewer GOPs than the grid; tone tables of max count rows and
    stats: every output is the whole toned video's result, sliced"""
    ops, vs = env["ops"], env["vs"]
    devs = [torch.from_numpy(h).cuda() for h in three]
    spans = np.array([[0, 11], [gop, 2], [2 * gop, 7]])
    rng = np.random.RandomState(gop)
    tone = rng.randint(0, 256, (3, 11, 256, 3)).astype(np.uint8)
    tone[..., :] = np.sort(tone, axis=2)                          # monotone byte maps, as a flicker's are
    codec = vs.Codec(50, sub, gop=gop)
    outs, sts = ops.codec_roundtrip(devs, codec, spans=spans, tone=torch.from_numpy(tone).cuda(), stats=True)
    plain = ops.codec_roundtrip(devs, codec, spans=spans)
    for k, (h, (first, count)) in enumerate(zip(three, spans)):
        assert tuple(outs[k].shape) == (count,) + h.shape[1:] and tuple(sts[k].shape) == (count, 2)
        exp, exp_st = vs.codec_roundtrip_host(h[first:first + count], 50, sub, tone=tone[k, :count], stats=True, gop=gop, first_frame=int(first))
        assert same_bits(outs[k], exp) and same_bits(sts[k], exp_st), k
        whole = vs.codec_roundtrip_host(h, 50, sub, gop=gop)
        assert same_bits(plain[k], whole[first:first + count]), k
        assert not same_bits(plain[k], outs[k])
    # the default span is the whole video
    for k, o in enumerate(ops.codec_roundtrip(devs, codec)):
        assert same_bits(o, vs.codec_roundtrip_host(three[k], 50, sub, gop=gop)), k


def test_more_than_64_videos(env):
    ops, vs = env["ops"], env["vs"]
    hosts = [moving(3, 8, 8, 100 + k) for k in range(70)]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    tone = np.sort(np.random.RandomState(1).randint(0, 256, (70, 3, 256, 3)).astype(np.uint8), axis=2)
    codec = vs.Codec(75, "420", gop=2)
    outs, sts = ops.codec_roundtrip(devs, codec, tone=torch.from_numpy(tone).cuda(), stats=True)
    assert len(outs) == 70
    for k in (0, 1, 31, 63, 64, 65, 69):
        exp, exp_st = vs.codec_roundtrip_host(hosts[k], 75, "420", tone=tone[k], stats=True, gop=2)
        assert same_bits(outs[k], exp) and same_bits(sts[k], exp_st), k


@pytest.mark.parametrize("sub,geom", cases.VIEW_GEOMETRIES, ids=cases.VIEW_IDS)
def test_source_and_destination_views(env, sub, geom):
    """the source a view of a wider and longer video one byte off a 4-byte boundary, the span inside it; the destination a view with
    pitches of its own, also off alignment: the result is the restatement's and no byte outside the destination view changes.
    "seams": a view of several tiles, the last ones partial (codec_mc_cases.check_views_across_tile_seams)"""
    ops, vs = env["ops"], env["vs"]
    if geom == "seams":
        return cases.check_views_across_tile_seams(ops, vs, sub, gop=3)
    codec = vs.Codec(60, sub, gop=3)
    big = moving(9, 30, 150, seed=11)
    buf = torch.empty(big.size + 8, dtype=torch.uint8, device="cuda")
    whole = buf[1:1 + big.size].view(big.shape)
    whole.copy_(torch.from_numpy(big))
    src = whole[1:9, 3:22, 5:42]                                                   # 8 x 19 x 37 inside 9 x 30 x 150
    assert src.data_ptr() % 4 != 0
    exp = vs.codec_roundtrip_host(big[1:9, 3:22, 5:42][3:8], 60, sub, gop=3, first_frame=3)
    assert same_bits(ops.codec_roundtrip([src], codec, spans=[[3, 5]])[0], exp)
    n = 6 * 25 * 50 * 3
    dbuf = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    dwhole = dbuf[2:2 + n].view(6, 25, 50, 3)
    dst = dwhole[1:6, 2:21, 7:44]
    assert dst.data_ptr() % 4 != 0
    before = dbuf.clone()
    out = ops.codec_roundtrip([src], codec, spans=[[3, 5]], out=[dst])
    assert out[0].data_ptr() == dst.data_ptr() and same_bits(dst, exp)
    mask = torch.zeros_like(dwhole, dtype=torch.bool)
    mask[1:6, 2:21, 7:44] = True
    assert bool((dwhole[~mask] == 0xA5).all()) and same_bits(dbuf[:2], before[:2]) and same_bits(dbuf[2 + n:], before[2 + n:])


def test_refused_before_launch(env):
    ops, vs = env["ops"], env["vs"]
    x = torch.zeros((6, 8, 8, 3), dtype=torch.uint8, device="cuda")
    codec = vs.Codec(gop=3)
    with pytest.raises(ValueError, match="spans"):
        ops.codec_roundtrip([x], codec, frame_idx=[[0, 1]])
    with pytest.raises(ValueError, match="spans"):
        ops.codec_roundtrip([x], vs.Codec(), spans=[[0, 6]])
    for bad in ([[1, 2]], [[3, 4]], [[0, 0]], [[-3, 2]], [[0, 7]], [[0, 6], [0, 6]], [0, 6], [[0.0, 6.0]]):
        with pytest.raises(ValueError, match="span"):
            ops.codec_roundtrip([x], codec, spans=bad)
    with pytest.raises(ValueError, match="spans"):
        ops.codec_roundtrip([x], codec, spans=torch.tensor([[0, 6]], device="cuda"))
    with pytest.raises(ValueError, match="tone"):
        ops.codec_roundtrip([x], codec, spans=[[3, 2]], tone=torch.zeros((1, 1, 256, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        ops.codec_roundtrip([x], codec, spans=[[3, 2]], out=[torch.zeros((6, 8, 8, 3), dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError, match="overlaps"):
        ops.codec_roundtrip([x], codec, out=[x])


# ---- engine --------------------------------------------------------------------------------------------------------------------
T, HW, GOP = 8, 64, 4
FIXED = {"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}
CODEC = dict(quality=60, subsampling="420", gop=GOP)
_ENGINES = {}


def engine(**kw):
    """mc3_18 on synthetic weights, 8 frames of 64 x 64, bf16, flicker on video time; one engine per setting for the module"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    kw = dict(dict(batch_size=2, sample_length=T, image_size=HW, im_scale=HW, dtype="bf16", l_inf_pert_norm=0.2, flicker_time="video", flicker_period=8), **kw)
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
    """two raw videos of differing length and resolution, neither a whole number of 16 x 16 MCUs: 24 x 72 x 100, whose evaluation
    clip starts on a GOP boundary (frame 8), and 27 x 90 x 82, whose clip does not (frame 10: two lead-in frames)"""
    vids = [moving(24, 72, 100, 51), moving(27, 90, 82, 52)]
    for v in vids:
        v[:, :2], v[:, 2:4] = 0, 255
    return [torch.from_numpy(v).cuda() for v in vids]


def clean_labels(eng, videos, num_samples=1):
    return torch.from_numpy(eng.evaluate_videos(videos, np.zeros(len(videos), np.int64), num_samples=num_samples)["video_preds"]).cuda()


@pytest.mark.parametrize("model", ["additive", "illumination"])
def test_export_video_through_the_gop_codec_is_the_restatement(env, raw, model):
    ops, vs = env["ops"], env["vs"]
    eng = engine(flicker_model=model)
    codec = vs.Codec(**CODEC)
    plain = eng.export_video(raw[1], phase=2)
    got = eng.export_video(raw[1], phase=2, codec=codec)
    assert same_bits(got, vs.codec_roundtrip_host(plain.cpu().numpy(), 60, "420", gop=GOP))
    assert not same_bits(got, eng.export_video(raw[1], phase=2, codec=vs.Codec(60, "420")))
    assert same_bits(eng.export_video(raw[0], phase=2, capture=FIXED, codec=codec),
                     ops.codec_roundtrip([eng.export_video(raw[0], phase=2, capture=FIXED)], codec)[0])


def test_evaluate_videos_through_the_gop_codec_is_the_chain_by_hand(env, raw):
    ops, vs = env["ops"], env["vs"]
    eng = engine()
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
    intra = eng.evaluate_videos(raw, labels, num_samples=2, quantise="video", codec=vs.Codec(60, "420"))
    assert not same_bits(ev["clip_logits"], intra["clip_logits"]) and same_bits(ev["clean_clip_logits"], intra["clean_clip_logits"])


@pytest.mark.parametrize("model", ["additive", "illumination"])
def test_step_videos_scores_what_evaluate_videos_scores_through_the_gop_codec(env, raw, model):
    vs = env["vs"]
    codec = vs.Codec(**CODEC)
    eng = engine(flicker_model=model, train_delivered=True, codec=codec)
    labels = clean_labels(eng, raw)
    r = eng.step_videos(raw, labels, criterion(), update=False, train=False)
    logits, argmax = eng._logits.clone(), r["argmax"].clone()
    firsts = np.concatenate(eng.last_sampling)[:, 0]
    assert firsts[0] % GOP == 0 and firsts[1] % GOP != 0           # one clip on a GOP boundary, one with lead-in frames
    ev = eng.evaluate_videos(raw, labels.cpu().numpy(), num_samples=1, quantise="video", codec=codec)
    assert same_bits(logits, ev["clip_logits"])
    assert np.array_equal(argmax.cpu().numpy().astype(np.int64), ev["clip_preds"])
    intra = eng.evaluate_videos(raw, labels.cpu().numpy(), num_samples=1, quantise="video", codec=vs.Codec(60, "420"))
    assert not same_bits(logits, intra["clip_logits"]) and not same_bits(logits, ev["clean_clip_logits"])


def test_step_videos_through_a_fixed_capture_channel_and_the_gop_codec(env, raw):
    ops, vs = env["ops"], env["vs"]
    codec = vs.Codec(**CODEC)
    ch = vs.CaptureChannel(subframe=FIXED["subframe"], exposure=FIXED["exposure"], gain=FIXED["gain"], gain_mode="per_channel")
    eng = engine(train_delivered=True, capture=ch, codec=codec)
    labels = clean_labels(eng, raw)
    eng.step_videos(raw, labels, criterion(), update=False, train=False)
    logits = eng._logits.clone()
    rows = np.concatenate(eng.last_sampling)
    assert (rows[:, 0] % GOP != 0).any()
    exported = [eng.export_video(v, capture=FIXED, codec=codec) for v in raw]
    assert same_bits(logits, eng.logits(ops.prepare_clips(exported, im_scale=HW, input_size=(HW, HW), frame_idx=rows), False))
    uncaptured = [eng.export_video(v, codec=codec) for v in raw]
    assert not same_bits(logits, eng.logits(ops.prepare_clips(uncaptured, im_scale=HW, input_size=(HW, HW), frame_idx=rows), False))


def test_step_videos_trains_through_the_gop_codec_straight_through(env, raw):
    """the backward is the train_delivered one on the source clip frames (rec ~ cur for a P-frame as for an intra frame): handed the
    input gradient of the GOP step, the no-codec chain of slopes, resampling and row fold reproduces the step's payload bit for bit;
    and with update=True the perturbation moves"""
    ops, vs = env["ops"], env["vs"]
    eng = engine(train_delivered=True, optimizer="pgd", codec=vs.Codec(**CODEC))
    labels = clean_labels(eng, raw)
    before = eng.pert_model.perturbation.clone()
    eng.step_videos(raw, labels, criterion(), update=False, train=False)
    pm = eng.pert_model
    a = pm.export_args(ops.tone_ramp(2, T), True, shift_p=0)
    slope, scale = ops.flicker_tone_slopes(a, None)
    g_clip = ops.prepare_clips_grad(raw, eng._gx, slope, scale, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling))
    expect = ops.flicker_rows_grad(g_clip, pm.rows_dev, 8)
    assert float(expect.abs().max()) > 0 and same_bits(eng._red[:24].view(8, 3), expect)
    for _ in range(3):
        r = eng.step_videos(raw, labels, criterion(), lr=1e-2, update=True, train=True)
        assert np.isfinite(float(r["loss"]))
    assert not same_bits(before, eng.pert_model.perturbation)


def test_a_gop_engine_refuses_what_train_delivered_refuses(env):
    vs = env["vs"]
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    W = vs.synthetic_weights("mc3_18", 42)
    kw = dict(batch_size=2, sample_length=T, image_size=HW, dtype="bf16")
    codec = vs.Codec(**CODEC)
    with pytest.raises(ValueError, match="train_delivered"):
        FlickerVideoResNet("mc3_18", W, flicker_time="video", codec=codec, **kw)
    with pytest.raises(ValueError, match="train_delivered"):
        FlickerVideoResNet("mc3_18", W, flicker_time="clip", train_delivered=True, codec=codec, **kw)
    with pytest.raises(ValueError, match="one shared perturbation"):
        FlickerVideoResNet("mc3_18", W, flicker_time="video", train_delivered=True, per_clip=True, codec=codec, **kw)
    with pytest.raises(ValueError, match="readout"):
        FlickerVideoResNet("mc3_18", W, flicker_time="video", train_delivered=True, codec=codec,
                           capture=vs.CaptureChannel(readout=(0.5, 0.5)), **kw)
    eng = engine()
    with pytest.raises(ValueError, match="quantise='video'"):
        eng.evaluate_videos([torch.zeros((12, 64, 64, 3), dtype=torch.uint8, device="cuda")] * 2, np.zeros(2, np.int64), num_samples=1, quantise="clip", codec=codec)
    with pytest.raises(ValueError, match="train_delivered"):
        eng.step_videos([], None, criterion())
