"""Motion-compensated P-frames on the GPU: flk_codec_roundtrip_mc_u8 BITWISE its numpy integer restatement
(videoresnet_spec.codec_roundtrip_host(gop=, first_frame=, search=, motion=)) -- frames, stats and vectors -- over subsamplings,
qualities, GOP lengths, search ranges, frame sizes, spans, tone tables, views and contents (tests/codec_mc_cases.py; their coverage is
checked in tests/test_codec_mc_cpu.py); then the engine: export, evaluation and the delivered-video training forward through such a
codec, and the identity step_videos(train=False) == evaluate_videos(quantise="video", codec=)."""
import ctypes as C

import numpy as np
import pytest
import torch

import codec_mc_cases as cases

pytestmark = pytest.mark.gpu
SUBS = cases.SUBS


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


@pytest.fixture(scope="module")
def env():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    return dict(ops=ops, vs=vs)


# ---- kernel == restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_is_the_restatement(env, size, sub):
    """videos of 1 and of 7 frames in one call per case: frames, stats and vectors bit for bit.  The cases hold search 1, 4, 7, 15 (7 and
    15 on every content kind), gop 2, 3, 7, 12, qualities 1, 50, 75, 100"""
    ops, vs = env["ops"], env["vs"]
    moved = 0
    for content, q, gop, R in cases.COMBOS:
        hosts = cases.case_videos(content, size, R)
        outs, sts, mvs = ops.codec_roundtrip([torch.from_numpy(h).cuda() for h in hosts], vs.Codec(q, sub, gop=gop, search=R), stats=True, motion=True)
        for h, o, st, mv in zip(hosts, outs, sts, mvs):
            exp, exp_st, exp_mv = vs.codec_roundtrip_host(h, q, sub, stats=True, gop=gop, search=R, motion=True)
            what = (size, sub, content, q, gop, R, len(h))
            assert same_bits(mv, exp_mv), (what, np.argwhere(mv.cpu().numpy() != exp_mv)[:4])
            assert same_bits(o, exp), (what, int(np.abs(o.cpu().numpy().astype(int) - exp.astype(int)).max()))
            assert same_bits(st, exp_st), (what, st.cpu().numpy(), exp_st)
            moved += int(np.abs(exp_mv).sum())
    assert moved > 0


@pytest.mark.parametrize("sub", SUBS)
def test_search_0_through_the_new_entry_is_the_gop_entry(env, sub):
    """ops sends search 0 to flk_codec_roundtrip_gop_u8; with motion=True it goes through the new entry: the same bytes, zero vectors.
    And the new entry called directly at search 0"""
    from flickering_adversarial_video_amd import _lib
    ops, vs = env["ops"], env["vs"]
    host = cases.moving(7, 40, 150, seed=4)
    x = torch.from_numpy(host).cuda()
    for q, gop in ((50, 3), (100, 7)):
        (a,), (sa,) = ops.codec_roundtrip([x], vs.Codec(q, sub, gop=gop), stats=True)
        (b,), (sb,), (mv,) = ops.codec_roundtrip([x], vs.Codec(q, sub, gop=gop), stats=True, motion=True)
        assert same_bits(a, b) and same_bits(sa, sb) and tuple(mv.shape[:1] + mv.shape[3:]) == (7, 2) and not bool(mv.any())
    out = torch.zeros((4, 40, 150, 3), dtype=torch.uint8, device="cuda")
    st = torch.empty((1, 4, 2), dtype=torch.int32, device="cuda")
    arr = (_lib.CodecClip * 1)()
    d = arr[0]
    d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = x.data_ptr(), 7, 40, 150, x.stride(0), x.stride(1)
    d.dst, d.dst_pitch_t, d.dst_pitch_h = out.data_ptr(), out.stride(0), out.stride(1)
    a = _lib.CodecArgs()
    a.nclip, a.quality, a.subsampling, a.clips = 1, 50, int(sub), arr
    first, count = (C.c_int32 * 1)(3), (C.c_int32 * 1)(4)
    need = _lib.load().flk_codec_mc_scratch_bytes(C.byref(a), 3, count)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().flk_codec_roundtrip_mc_u8(C.byref(a), 3, 0, first, count, 4, None, _lib.ptr(st), None, 0, _lib.ptr(ws), need, _lib.stream_ptr()))
    ref = torch.zeros_like(out)
    st2 = torch.empty_like(st)
    d.dst = ref.data_ptr()
    got = out
    _lib.check(_lib.load().flk_codec_roundtrip_gop_u8(C.byref(a), 3, first, count, 4, None, _lib.ptr(st2), _lib.stream_ptr()))
    assert same_bits(got, ref) and same_bits(st, st2) and same_bits(ref, vs.codec_roundtrip_host(host[3:7], 50, sub, gop=3, first_frame=3))


# ---- spans, clip tables, tone tables -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    """three videos of differing resolution and length, the second more than one tile wide"""
    return [cases.moving(11, 17, 23, 21), cases.pan(9, 48, 200, 2, -5, seed=22), cases.moving(14, 40, 24, 23)]


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("gop", [2, 3])
def test_one_call_of_three_videos_with_their_own_spans(env, three, sub, gop):
    """firsts 0, gop and 2 gop, differing counts, tone tables of max count rows, stats and vectors: every output is the single-video
    call's and the whole video's result, sliced"""
    ops, vs = env["ops"], env["vs"]
    devs = [torch.from_numpy(h).cuda() for h in three]
    spans = np.array([[0, 11], [gop, 2], [2 * gop, 7]])
    tone = np.sort(np.random.RandomState(gop).randint(0, 256, (3, 11, 256, 3)).astype(np.uint8), axis=2)          # monotone byte maps
    tone_dev = torch.from_numpy(tone).cuda()
    codec = vs.Codec(50, sub, gop=gop, search=6)
    outs, sts, mvs = ops.codec_roundtrip(devs, codec, spans=spans, tone=tone_dev, stats=True, motion=True)
    plain, pmv = ops.codec_roundtrip(devs, codec, spans=spans, motion=True)
    for k, (h, (first, count)) in enumerate(zip(three, spans)):
        exp, exp_st, exp_mv = vs.codec_roundtrip_host(h[first:first + count], 50, sub, tone=tone[k, :count], stats=True, gop=gop, first_frame=int(first),
                                                      search=6, motion=True)
        assert tuple(outs[k].shape) == (count,) + h.shape[1:] and tuple(sts[k].shape) == (count, 2) and tuple(mvs[k].shape) == exp_mv.shape
        assert same_bits(outs[k], exp) and same_bits(sts[k], exp_st) and same_bits(mvs[k], exp_mv), k
        (o1,), (s1,), (m1,) = ops.codec_roundtrip([devs[k]], codec, spans=spans[k:k + 1], tone=tone_dev[k:k + 1, :count], stats=True, motion=True)
        assert same_bits(o1, outs[k]) and same_bits(s1, sts[k]) and same_bits(m1, mvs[k]), k
        whole, wmv = vs.codec_roundtrip_host(h, 50, sub, gop=gop, search=6, motion=True)
        assert same_bits(plain[k], whole[first:first + count]) and same_bits(pmv[k], wmv[first:first + count]), k
        assert not same_bits(plain[k], outs[k])
    for k, o in enumerate(ops.codec_roundtrip(devs, codec)):     # the default span is the whole video
        assert same_bits(o, vs.codec_roundtrip_host(three[k], 50, sub, gop=gop, search=6)), k


def test_more_videos_than_one_launch_takes(env):
    """70 videos: ops splits at 64, the entry at 48 clips a launch; every clip keeps its tone rows, stats rows, vectors and workspace"""
    ops, vs = env["ops"], env["vs"]
    hosts = [cases.moving(3, 16, 24, 100 + k) for k in range(70)]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    tone = np.sort(np.random.RandomState(1).randint(0, 256, (70, 3, 256, 3)).astype(np.uint8), axis=2)
    codec = vs.Codec(75, "420", gop=3, search=3)
    outs, sts, mvs = ops.codec_roundtrip(devs, codec, tone=torch.from_numpy(tone).cuda(), stats=True, motion=True)
    assert len(outs) == 70
    for k in (0, 1, 47, 48, 49, 63, 64, 65, 69):
        exp, exp_st, exp_mv = vs.codec_roundtrip_host(hosts[k], 75, "420", tone=tone[k], stats=True, gop=3, search=3, motion=True)
        assert same_bits(outs[k], exp) and same_bits(sts[k], exp_st) and same_bits(mvs[k], exp_mv), k


@pytest.mark.parametrize("sub,geom", cases.VIEW_GEOMETRIES, ids=cases.VIEW_IDS)
def test_source_and_destination_views(env, sub, geom):
    """the source a view of a wider and longer video one byte off a 4-byte boundary, the span inside it; the destination a view with
    pitches of its own, also off alignment: the result is the restatement's and no byte outside the destination view changes.
    "seams": a view of several tiles, the last ones partial (codec_mc_cases.check_views_across_tile_seams)"""
    ops, vs = env["ops"], env["vs"]
    if geom == "seams":
        return cases.check_views_across_tile_seams(ops, vs, sub, gop=3, search=4)
    codec = vs.Codec(60, sub, gop=3, search=5)
    big = cases.moving(9, 30, 150, seed=11)
    buf = torch.empty(big.size + 8, dtype=torch.uint8, device="cuda")
    whole = buf[1:1 + big.size].view(big.shape)
    whole.copy_(torch.from_numpy(big))
    src = whole[1:9, 3:22, 5:42]                                                   # 8 x 19 x 37 inside 9 x 30 x 150
    assert src.data_ptr() % 4 != 0
    exp = vs.codec_roundtrip_host(big[1:9, 3:22, 5:42][3:8], 60, sub, gop=3, first_frame=3, search=5)
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


def test_repeats_and_a_reused_workspace(env):
    """two calls give equal bytes; a call on other (larger, then smaller) videos in between, which reuses the workspace, changes nothing"""
    ops, vs = env["ops"], env["vs"]
    codec = vs.Codec(50, "420", gop=4, search=7)
    x = torch.from_numpy(cases.pan(6, 66, 130, -3, 2)).cuda()
    a, sa, ma = ops.codec_roundtrip([x], codec, stats=True, motion=True)
    b, sb, mb = ops.codec_roundtrip([x], codec, stats=True, motion=True)
    assert same_bits(a[0], b[0]) and same_bits(sa[0], sb[0]) and same_bits(ma[0], mb[0])
    ops.codec_roundtrip([torch.from_numpy(cases.moving(9, 90, 140, 5)).cuda()], vs.Codec(90, "444", gop=2, search=2))
    ops.codec_roundtrip([torch.from_numpy(cases.moving(3, 16, 16, 6)).cuda()], codec)
    c, sc, mc = ops.codec_roundtrip([x], codec, stats=True, motion=True)
    assert same_bits(a[0], c[0]) and same_bits(sa[0], sc[0]) and same_bits(ma[0], mc[0])
    assert ops._codec_mc_scratch[x.device].numel() >= 5 * 2 * (96 * 144 * 3)


def test_refused_before_launch(env):
    from flickering_adversarial_video_amd import _lib
    ops, vs = env["ops"], env["vs"]
    x = torch.zeros((6, 8, 8, 3), dtype=torch.uint8, device="cuda")
    codec = vs.Codec(gop=3, search=7)
    with pytest.raises(ValueError, match="spans"):
        ops.codec_roundtrip([x], codec, frame_idx=[[0, 1]])
    with pytest.raises(ValueError, match="motion"):
        ops.codec_roundtrip([x], vs.Codec(), motion=True)
    for bad in ([[1, 2]], [[3, 4]], [[0, 0]], [[-3, 2]], [[0, 7]], [[0, 6], [0, 6]]):
        with pytest.raises(ValueError, match="span"):
            ops.codec_roundtrip([x], codec, spans=bad)
    with pytest.raises(ValueError, match="tone"):
        ops.codec_roundtrip([x], codec, spans=[[3, 2]], tone=torch.zeros((1, 1, 256, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="overlaps"):
        ops.codec_roundtrip([x], codec, out=[x])
    # the entry itself, with real pointers: a scratch too small, a bad search, an mv_stride too small -- nothing is written
    out = torch.full((6, 8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    arr = (_lib.CodecClip * 1)()
    d = arr[0]
    d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = x.data_ptr(), 6, 8, 8, x.stride(0), x.stride(1)
    d.dst, d.dst_pitch_t, d.dst_pitch_h = out.data_ptr(), out.stride(0), out.stride(1)
    a = _lib.CodecArgs()
    a.nclip, a.quality, a.subsampling, a.clips = 1, 50, 420, arr
    first, count = (C.c_int32 * 1)(0), (C.c_int32 * 1)(6)
    lib = _lib.load()
    need = lib.flk_codec_mc_scratch_bytes(C.byref(a), 3, count)
    assert need == 2 * 2 * (256 + 128)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    mv = torch.zeros((1, 6, 1, 2), dtype=torch.int8, device="cuda")
    for kw in (dict(nbytes=need - 1), dict(search=16), dict(stride=0), dict(scratch=None)):
        rc = lib.flk_codec_roundtrip_mc_u8(C.byref(a), 3, kw.get("search", 7), first, count, 6, None, None, _lib.ptr(mv), kw.get("stride", 1),
                                           _lib.ptr(ws) if "scratch" not in kw else None, kw.get("nbytes", need), _lib.stream_ptr())
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and not bool(ws.any())
    _lib.check(lib.flk_codec_roundtrip_mc_u8(C.byref(a), 3, 7, first, count, 6, None, None, _lib.ptr(mv), 1, _lib.ptr(ws), need, _lib.stream_ptr()))
    assert same_bits(out, vs.codec_roundtrip_host(x.cpu().numpy(), 50, "420", gop=3, search=7))


# ---- engine --------------------------------------------------------------------------------------------------------------------
T, HW, GOP = 8, 64, 4
CODEC = dict(quality=75, subsampling="420", gop=GOP, search=7)
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
    eng.pert_model.init_perturbation(rng.uniform(-0.25, 0.25, (3, eng.P, 1, 1)).astype(np.float32))
    eng.pert_model.dynamic_max_norm = eng.pert_model.max_norm
    return eng


def criterion():
    from flickering_adversarial_video_amd.torch_attack import Losses
    return Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)


@pytest.fixture(scope="module")
def raw():
    """the small raw videos of the GOP tests, panning here: 24 x 72 x 100, whose evaluation clip starts on a GOP boundary (frame 8), and
    27 x 90 x 82, whose clip does not (frame 10: two lead-in frames)"""
    vids = [cases.pan(24, 72, 100, 1, -2, seed=51), cases.pan(27, 90, 82, -2, 3, seed=52)]
    for v in vids:
        v[:, :2], v[:, 2:4] = 0, 255
    return [torch.from_numpy(v).cuda() for v in vids]


def clean_labels(eng, videos, num_samples=1):
    return torch.from_numpy(eng.evaluate_videos(videos, np.zeros(len(videos), np.int64), num_samples=num_samples)["video_preds"]).cuda()


@pytest.mark.parametrize("model", ["additive", "illumination"])
def test_export_video_through_the_mc_codec_is_the_restatement(env, raw, model):
    vs = env["vs"]
    eng = engine(flicker_model=model)
    codec = vs.Codec(**CODEC)
    plain = eng.export_video(raw[1], phase=2)
    got = eng.export_video(raw[1], phase=2, codec=codec)
    assert same_bits(got, vs.codec_roundtrip_host(plain.cpu().numpy(), 75, "420", gop=GOP, search=7))
    assert not same_bits(got, eng.export_video(raw[1], phase=2, codec=vs.Codec(75, "420", gop=GOP)))


@pytest.mark.parametrize("model", ["additive", "illumination"])
def test_step_videos_scores_what_evaluate_videos_scores_through_the_mc_codec(env, raw, model):
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
    zero = eng.evaluate_videos(raw, labels.cpu().numpy(), num_samples=1, quantise="video", codec=vs.Codec(75, "420", gop=GOP))
    assert not same_bits(logits, zero["clip_logits"]) and not same_bits(logits, ev["clean_clip_logits"])


def test_step_videos_trains_through_the_mc_codec(env, raw):
    """the backward is the straight-through one of the zero-motion codec; with update=True the perturbation moves"""
    vs = env["vs"]
    eng = engine(train_delivered=True, optimizer="pgd", codec=vs.Codec(**CODEC))
    labels = clean_labels(eng, raw)
    before = eng.pert_model.perturbation.clone()
    for _ in range(3):
        r = eng.step_videos(raw, labels, criterion(), lr=1e-2, update=True, train=True)
        assert np.isfinite(float(r["loss"]))
    assert not same_bits(before, eng.pert_model.perturbation)
