"""Training on the delivered video at its native resolution, on the GPU: the toned preparation (flk_clip_prepare_toned) BITWISE the
sampled preparation of the exported video on every path, the tone tables bitwise their host restatement, the gradient through the
resampling (flk_clip_prepare_grad) exact where every number is dyadic and within its rounding bound of the float64 restatement where
not, reproducible and per clip the call with that clip alone; and the engine's ``step_videos`` against ``evaluate_videos`` / ``export_video``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
GEOM = dict(im_scale=16, input_size=12)
DCLIP = 0.6


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def on_device(u8, offset=0):
    """the array on the device, `offset` bytes past an allocation's start (allocations are at least 256-byte aligned)"""
    buf = torch.empty(u8.size + offset, dtype=torch.uint8, device="cuda")
    x = buf[offset:].view(u8.shape)
    x.copy_(torch.from_numpy(u8))
    assert x.is_contiguous() and x.data_ptr() % 4 == offset % 4
    return x


def fold1(x):
    """[B,T,H,W,3] -> the 16-channel (h,w) fold [B,T,H/2,W/2,16], channel (qh*2+qw)*3+c, 12..15 zero (data movement only)"""
    x = torch.as_tensor(x)
    B, T, H, W, _ = x.shape
    f = x.reshape(B, T, H // 2, 2, W // 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, T, H // 2, W // 2, 12)
    return torch.cat([f, torch.zeros(f.shape[:4] + (4,), dtype=f.dtype)], dim=4).contiguous()


@pytest.fixture(scope="module")
def env():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import decode_table
    lo, hi = vs.additive_bounds()
    tables = vs.illum_tables("srgb")
    return dict(ops=ops, vs=vs, lut=decode_table("cuda"), tables=tables, illum=ops.make_illum_args(tables),
                kw=dict(dialect="torch", dclip=DCLIP, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo, hi=hi))


def export_args(env, x, delta, **over):
    return env["ops"].make_export_apply_args(x, delta, x_lut=env["lut"], **{**env["kw"], **over})


def tone_of(env, delta, model, **over):
    """the tone tables of the per-clip delta [n,T,3] (device) under a pixel model"""
    ops = env["ops"]
    n, T = delta.shape[:2]
    a = export_args(env, ops.tone_ramp(n, T), delta, **over)
    return ops.flicker_tone_tables(a, env["illum"] if model == "illumination" else None), a


def exported_clips(env, videos, idx, delta, model):
    """export_video's arithmetic on the frames each clip is cut from: clip k's gathered frames [T_out,H,W,3] exported under its own delta rows"""
    ops = env["ops"]
    out = []
    for k, v in enumerate(videos):
        frames = v[torch.as_tensor(idx[k], device="cuda")].contiguous()[None]
        a = export_args(env, frames, delta[k:k + 1].contiguous())
        out.append((ops.illum_export_u8(a, env["illum"]) if model == "illumination" else ops.export_adversarial_u8(a, "torch"))[0])
    return out


@pytest.fixture(scope="module")
def small(env):
    """two videos in one call: 20 frames of 24 x 32 (steps 1.5 / 1.5238) and 9 frames of 32 x 48 (step 2.0), both views starting one byte
    past a 4-byte boundary (a nonzero staging misalignment); frame tables that repeat and pad frames; deltas that clamp"""
    rng = np.random.default_rng(101)
    hosts = [rng.integers(0, 256, (20, 24, 32, 3), dtype=np.uint8), rng.integers(0, 256, (9, 32, 48, 3), dtype=np.uint8)]
    videos = [on_device(h, 1) for h in hosts]
    assert all(v.data_ptr() % 4 == 1 for v in videos)
    idx = np.array([[0, 0, 3, 5, 5, 10, 19, 19], [2, 4, 6, 8, 8, 8, 8, 8]])
    delta = rng.uniform(-0.8, 0.8, (2, 8, 3)).astype(np.float32)                      # beyond DCLIP too: the delta clamp is hit
    delta[0, 2] = 0.0
    return dict(hosts=hosts, videos=videos, idx=idx, delta=delta, delta_dev=torch.from_numpy(delta).cuda())


TRANSFORMS = {"eval": dict(boxes=None, flips=None),
              "box_flip": dict(boxes=[(1, 2, 9, 13), (2, 3, 11, 17)], flips=[True, True]),          # resampled boxes (16 x 21 and 16 x 24 resized)
              "direct_flip": dict(boxes=[(2, 3, 12, 12), (1, 5, 12, 12)], flips=[True, True]),      # boxes of the output size
              "box_mixed": dict(boxes=[(0, 0, 16, 21), (3, 1, 7, 20)], flips=[False, True])}


# ---- toned prepare -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["additive", "illumination"])
@pytest.mark.parametrize("tf", list(TRANSFORMS))
def test_toned_prepare_is_the_prepare_of_the_exported_video(env, small, model, tf):
    ops, vs = env["ops"], env["vs"]
    tone, _ = tone_of(env, small["delta_dev"], model)
    got = ops.prepare_clips(small["videos"], frame_idx=small["idx"], tone=tone, **GEOM, **TRANSFORMS[tf])
    exp = exported_clips(env, small["videos"], small["idx"], small["delta_dev"], model)
    want = ops.prepare_clips(exp, frame_idx=np.broadcast_to(np.arange(8), (2, 8)), **GEOM, **TRANSFORMS[tf])
    assert same_bits(got, want)
    if model == "additive":                             # the deltas really clamp: counted by the host restatement of the export
        for k in range(2):
            _, st = ops.export_adversarial_u8_host(small["hosts"][k][small["idx"][k]][None], small["delta"][k:k + 1], x_lut=vs.u8_decode_table(),
                                                   stats=True, **env["kw"])
            assert st[..., 3].sum() > 0
    assert not same_bits(got, ops.prepare_clips(small["videos"], frame_idx=small["idx"], **GEOM, **TRANSFORMS[tf]))


@pytest.mark.parametrize("tf", ["eval", "box_flip"])
def test_toned_prepare_wide_enough_for_several_staging_passes(env, tf):
    """one 4-frame 240 x 320 video at 128 / 112: a row segment of about 850 bytes, 8 (6) slots of 2 x 214 dwords: 7 passes of 256 threads"""
    ops = env["ops"]
    rng = np.random.default_rng(7)
    video = on_device(rng.integers(0, 256, (4, 240, 320, 3), dtype=np.uint8), 1)
    idx = np.array([[3, 0, 0, 2, 1]])
    delta = torch.from_numpy(rng.uniform(-0.5, 0.5, (1, 5, 3)).astype(np.float32)).cuda()
    kw = dict(boxes=[(7, 20, 100, 131)], flips=[True]) if tf == "box_flip" else {}
    tone, _ = tone_of(env, delta, "additive")
    got = ops.prepare_clips([video], frame_idx=idx, tone=tone, im_scale=128, input_size=112, **kw)
    exp = exported_clips(env, [video], idx, delta, "additive")
    assert same_bits(got, ops.prepare_clips(exp, frame_idx=np.arange(5)[None], im_scale=128, input_size=112, **kw))


@pytest.mark.parametrize("tf", list(TRANSFORMS))
def test_identity_tone_is_the_untoned_launch(env, small, tf):
    ops = env["ops"]
    ident = torch.arange(256, dtype=torch.uint8, device="cuda").view(1, 1, 256, 1).expand(2, 8, 256, 3).contiguous()
    got = ops.prepare_clips(small["videos"], frame_idx=small["idx"], tone=ident, **GEOM, **TRANSFORMS[tf])
    assert same_bits(got, ops.prepare_clips(small["videos"], frame_idx=small["idx"], **GEOM, **TRANSFORMS[tf]))


@pytest.mark.parametrize("model", ["additive", "illumination"])
def test_tone_tables_are_the_export_of_the_ramp(env, small, model):
    ops, vs = env["ops"], env["vs"]
    tone, a = tone_of(env, small["delta_dev"], model)
    il = env["illum"] if model == "illumination" else None
    ramp_export = ops.illum_export_u8(a, il) if il is not None else ops.export_adversarial_u8(a, "torch")
    assert same_bits(tone.view(2, 8, 16, 16, 3), ramp_export)
    host = vs.tone_tables_host(small["delta"], env["tables"] if il is not None else None, dclip=DCLIP)
    assert same_bits(tone, host)
    with pytest.raises(ValueError, match="tone"):
        ops.prepare_clips(small["videos"], frame_idx=small["idx"], tone=tone[:1], **GEOM)
    with pytest.raises(ValueError, match="frame_idx"):
        ops.prepare_clips([v[:8] for v in small["videos"]], tone=tone, **GEOM)


# ---- gradient: exact ---------------------------------------------------------------------------------------------------------------
def slopes_of(env, delta, model, illum=None, **over):
    ops = env["ops"]
    n, T = delta.shape[:2]
    a = export_args(env, ops.tone_ramp(n, T), delta, **over)
    return ops.flicker_tone_slopes(a, (illum or env["illum"]) if model == "illumination" else None)


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("model", ["additive", "illumination"])
def test_gradient_is_exact_on_dyadic_numbers(env, model, gdtype, flip):
    """a 32 x 32 source (step 2.0: every stage-1 lambda is 0.5) and a 6 x 6 box on the 12 x 12 output (step 0.5: stage-2 lambdas 0.25 /
    0.75): J is a multiple of 1/64 of a slope.  Additive slopes are 0 / 1; illumination slopes on dec = v / 256, the identity enc and
    N = 256 are v / 256 with bytes that are multiples of 4 below 196 (6 bits, never clamped).  With g an integer in -8..8 every product,
    lane sum, wave sum and row sum has at most 6 + 6 + 4 + 8 = 24 bits: the kernel must give the exact sums."""
    ops, vs = env["ops"], env["vs"]
    rng = np.random.default_rng(55)
    illum, tables, over = None, None, {}
    if model == "illumination":
        host = (rng.integers(0, 49, (5, 32, 32, 3)) * 4).astype(np.uint8)
        dec = np.ascontiguousarray(np.repeat((np.arange(256) / 256.0).astype(np.float32)[:, None], 3, axis=1))
        tables = (dec, (np.arange(257) / 256.0).astype(np.float32))
        illum = ops.make_illum_args(tables, out_mul=(1.0, 1.0, 1.0), out_add=(0.0, 0.0, 0.0))
        delta = (rng.integers(-1, 2, (1, 4, 3)) * 0.25).astype(np.float32)
        over = dict(dclip=0.25)
    else:
        host = rng.integers(0, 256, (5, 32, 32, 3), dtype=np.uint8)
        delta = rng.uniform(-0.5, 0.5, (1, 4, 3)).astype(np.float32)
    video, idx = on_device(host, 1), np.array([[4, 0, 0, 2]])
    box = (3, 5, 6, 6)
    slope, scale = slopes_of(env, torch.from_numpy(delta).cuda(), model, illum, **over)
    hs, hsc = vs.tone_slopes_host(delta, tables, dclip=over.get("dclip", DCLIP), out_mul=(1.0, 1.0, 1.0) if tables else None)
    assert same_bits(slope, hs) and same_bits(scale, hsc)
    if model == "additive":
        assert 0 < float(slope.sum()) < slope.numel()
    g = rng.integers(-8, 9, (1, 4, 12, 12, 3))
    gx = fold1(torch.from_numpy(g.astype(np.float32))).to(gdtype).cuda()
    got = ops.prepare_clips_grad([video], gx, slope, scale, boxes=[box], flips=[flip], frame_idx=idx, **GEOM).cpu().numpy()
    want = np.zeros((4, 3), np.int64)
    for t, f in enumerate(idx[0]):
        J = vs.prepare_resample_host(hs[0, t][host[f], np.arange(3)].astype(np.float64) * 256.0, box, flip, **GEOM) * 64.0
        assert np.array_equal(J, np.rint(J))
        want[t] = (g[0, t] * J.astype(np.int64)).sum((0, 1))
    assert np.abs(want).max() > 0
    expect = (want.astype(np.float64) / (256.0 * 64.0)).astype(np.float32) * hsc[0]           # the sums are exact; one rounded product with scale
    assert same_bits(got[0], expect.astype(np.float32))


@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gradient_of_a_pure_crop_is_perturb_grad_reduce_on_the_cropped_clip(env, gdtype):
    """a 16 x 16 source at im_scale 16 / input_size 12: step 1, the evaluation transform is the crop [2:14, 2:14] and J is the slope of the
    pixel itself -- the masked sum flk_perturb_grad_reduce takes on the cropped uint8 clip, exactly (integer gradients)"""
    ops = env["ops"]
    rng = np.random.default_rng(77)
    host = rng.integers(0, 256, (6, 16, 16, 3), dtype=np.uint8)
    video, idx = on_device(host, 1), np.array([[5, 1, 1, 0], [0, 2, 3, 3]])
    delta = torch.from_numpy(rng.uniform(-0.8, 0.8, (2, 4, 3)).astype(np.float32)).cuda()
    slope, scale = slopes_of(env, delta, "additive")
    gx = fold1(torch.from_numpy(rng.integers(-8, 9, (2, 4, 12, 12, 3)).astype(np.float32))).to(gdtype).cuda()
    got = ops.prepare_clips_grad([video, video], gx, slope, scale, frame_idx=idx, **GEOM)
    crop = torch.stack([video[torch.as_tensor(r, device="cuda")][:, 2:14, 2:14] for r in idx]).contiguous()
    a = ops.make_apply_args(crop, delta, fold_t=1, x_lut=env["lut"], **env["kw"])
    want = ops.perturb_grad_reduce(a, gx)
    assert float(want.abs().max()) > 0 and bool((want == 0).any())                   # some delta values lie outside DCLIP: exact zeros
    assert same_bits(got, want)


# ---- gradient: general -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general(env, small):
    """the non-dyadic cases above: random fp32 gradients for the two clips, shared by the tests below"""
    g = np.random.default_rng(91).standard_normal((2, 8, 12, 12, 3)).astype(np.float32)
    return dict(g=g, gx=fold1(torch.from_numpy(g)).cuda())


@pytest.mark.parametrize("model", ["additive", "illumination"])
@pytest.mark.parametrize("tf", list(TRANSFORMS))
def test_gradient_within_its_rounding_bound_of_the_float64_restatement(env, small, general, model, tf):
    """|GPU - float64| <= (n + 16) * 2^-24 * sum|g * J| per output, n = 144 terms: sequential summation plus at most 16 roundings per term
    (the float64 restatement takes the same float32 slopes, factors, indices and lambdas)"""
    ops, vs = env["ops"], env["vs"]
    slope, scale = slopes_of(env, small["delta_dev"], model)
    kw = TRANSFORMS[tf]
    got = ops.prepare_clips_grad(small["videos"], general["gx"], slope, scale, frame_idx=small["idx"], **GEOM, **kw)
    assert same_bits(got, ops.prepare_clips_grad(small["videos"], general["gx"], slope, scale, frame_idx=small["idx"], **GEOM, **kw))   # repeats
    hs, hsc = slope.cpu().numpy(), scale.cpu().numpy()
    worst = 0.0
    for k in range(2):
        box, flip = (kw["boxes"][k], kw["flips"][k]) if kw["boxes"] else (None, False)
        want, mag, n = vs.prepare_grad_host(small["hosts"][k], small["idx"][k], general["g"][k], hs[k], hsc[k], box, flip, bound=True, **GEOM)
        err = np.abs(got[k].cpu().numpy().astype(np.float64) - want)
        bound = (n + 16) * U * mag
        print(f"delivered gradient {model} {tf} clip {k}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
        assert (err <= bound).all(), (err.max(), bound.max())
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        alone = ops.prepare_clips_grad([small["videos"][k]], general["gx"][k:k + 1].contiguous(), slope[k:k + 1].contiguous(),
                                       scale[k:k + 1].contiguous(), frame_idx=small["idx"][k:k + 1], **GEOM,
                                       **(dict(boxes=[box], flips=[flip]) if kw["boxes"] else {}))
        assert same_bits(got[k:k + 1], alone)                                         # each clip's rows: the call with that clip alone
        outside = np.abs(small["delta"][k]) > DCLIP
        assert outside.any() and (got[k].cpu().numpy()[outside] == 0).all() and (want[outside] == 0).all()
    assert worst <= 1.0


# ---- engine ----------------------------------------------------------------------------------------------------------------------------
T, HW = 8, 64
FIXED = {"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}
_ENGINES = {}


def engine(**kw):
    """r3d_18 on synthetic weights, 8 frames of 64 x 64, bf16, flicker on video time; one engine per setting for the module"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    kw = dict(dict(batch_size=2, sample_length=T, image_size=HW, im_scale=HW, dtype="bf16", l_inf_pert_norm=0.2, flicker_time="video"), **kw)
    key = tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _ENGINES:
        _ENGINES[key] = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), **kw)
    eng = _ENGINES[key]
    P = eng.P
    rng = np.random.default_rng(13 + P)
    eng.pert_model.init_perturbation(rng.uniform(-0.25, 0.25, (3, P, 1, 1)).astype(np.float32))      # beyond the bound of 0.2 too
    eng.pert_model.dynamic_max_norm = eng.pert_model.max_norm
    return eng


def criterion():
    from flickering_adversarial_video_amd.torch_attack import Losses
    return Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)


@pytest.fixture(scope="module")
def raw():
    """two raw videos of differing length and resolution: 20 x 72 x 96 and 14 x 80 x 80, the clamp bounds reached"""
    rng = np.random.default_rng(17)
    vids = []
    for shape in ((20, 72, 96, 3), (14, 80, 80, 3)):
        u8 = rng.integers(0, 256, shape).astype(np.uint8)
        u8[:, :2], u8[:, 2:4] = 0, 255
        vids.append(torch.from_numpy(u8).cuda())
    return vids


def clean_labels(eng, videos, num_samples=1):
    return torch.from_numpy(eng.evaluate_videos(videos, np.zeros(len(videos), np.int64), num_samples=num_samples)["video_preds"]).cuda()


@pytest.mark.parametrize("model", ["additive", "illumination"])
@pytest.mark.parametrize("P", [5, 8])
def test_step_videos_scores_what_evaluate_videos_scores(raw, P, model):
    eng = engine(flicker_period=P, flicker_model=model, train_delivered=True)
    labels = clean_labels(eng, raw)
    r = eng.step_videos(raw, labels, criterion(), update=False, train=False)
    logits, argmax = eng._logits.clone(), r["argmax"].clone()
    ev = eng.evaluate_videos(raw, labels.cpu().numpy(), num_samples=1, quantise="video")
    assert same_bits(logits, ev["clip_logits"])
    assert np.array_equal(argmax.cpu().numpy().astype(np.int64), ev["clip_preds"])
    assert not same_bits(logits, ev["clean_clip_logits"])
    # the step's payload: the engine's own input gradient through the slopes, the resampling and the row fold
    from flickering_adversarial_video_amd import ops
    pm = eng.pert_model
    a = pm.export_args(ops.tone_ramp(2, T), True, shift_p=0)
    slope, scale = ops.flicker_tone_slopes(a, pm.illum if model == "illumination" else None)
    g_clip = ops.prepare_clips_grad(raw, eng._gx, slope, scale, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling))
    want = ops.flicker_rows_grad(g_clip, pm.rows_dev, P)
    assert float(want.abs().max()) > 0
    assert same_bits(eng._red[:3 * P].view(P, 3), want)


def test_step_videos_video_loss_on_the_clips_of_one_video(raw):
    eng = engine(flicker_period=5, train_delivered=True, clips_per_video=2, video_reduce="sum")
    video = [raw[0]]
    labels = clean_labels(eng, video, 2)
    r = eng.step_videos(video, labels, criterion(), update=False, train=False)
    vl = r["video_logits"].clone()
    ev = eng.evaluate_videos(video, labels.cpu().numpy(), num_samples=2, quantise="video")
    assert same_bits(vl, ev["video_logits"])


def test_step_videos_training_transform_and_phase(raw):
    """train=True on an engine with augment, shifted sampling and a cyclic perturbation: the logits are those of the clips cut, with the
    step's own tables, boxes and flips, from the videos exported at the phases the step drew"""
    from flickering_adversarial_video_amd import ops
    eng = engine(flicker_period=5, train_delivered=True, cyclic_pert=True, augment={"seed": 3}, sampling={"random_shift": True, "seed": 5})
    labels = clean_labels(eng, raw)
    eng.step_videos(raw, labels, criterion(), update=False, train=True)
    logits = eng._logits.clone()
    aug, rows, phases = eng.last_augment, np.concatenate(eng.last_sampling), eng.last_phases
    assert any(tuple(b[2:]) != (HW, HW) for b in aug["boxes"]) and len(phases) == 2
    exported = [eng.export_video(v, phase=int(ph)) for v, ph in zip(raw, phases)]
    x = ops.prepare_clips(exported, im_scale=HW, input_size=(HW, HW), boxes=aug["boxes"], flips=aug["flips"], frame_idx=rows)
    assert same_bits(logits, eng.logits(x, False))


def test_step_videos_through_a_fixed_capture_channel(raw):
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    ch = vs.CaptureChannel(subframe=FIXED["subframe"], exposure=FIXED["exposure"], gain=FIXED["gain"], gain_mode="per_channel")
    eng = engine(flicker_period=8, train_delivered=True, capture=ch)
    labels = clean_labels(eng, raw)
    eng.step_videos(raw, labels, criterion(), update=False, train=False)
    logits = eng._logits.clone()
    exported = [eng.export_video(v, capture=FIXED) for v in raw]
    x = ops.prepare_clips(exported, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling))
    assert same_bits(logits, eng.logits(x, False))
    no_channel = [eng.export_video(v) for v in raw]
    assert not same_bits(logits, eng.logits(ops.prepare_clips(no_channel, im_scale=HW, input_size=(HW, HW), frame_idx=np.concatenate(eng.last_sampling)), False))


def test_step_videos_updates_and_train_an_epoch_routes_through_it(raw):
    eng = engine(flicker_period=5, train_delivered=True, optimizer="pgd")
    from flickering_adversarial_video_amd.torch_attack import Adversarial_metrics
    labels = clean_labels(eng, raw)
    before = eng.pert_model.perturbation.clone()
    r = eng.step_videos(raw, labels, criterion(), lr=1e-2, update=True, train=True)
    assert np.isfinite(float(r["loss"])) and not same_bits(before, eng.pert_model.perturbation)
    loaders = {"train": [(raw, labels, None)], "valid": [(raw, labels, None)]}
    res = eng.train_an_epoch(loaders, criterion(), Adversarial_metrics(), lr=1e-2)
    assert np.isfinite(res["train/loss"]) and np.isfinite(res["valid/loss"]) and res["valid/flicker_period"] == 5
    with pytest.raises(ValueError, match="whole uint8 videos"):
        eng.train_an_epoch({"train": [(torch.zeros((2, T, HW, HW, 3), dtype=torch.uint8, device="cuda"), labels, None)], "valid": []},
                           criterion(), Adversarial_metrics(), lr=1e-2)


def test_engines_without_train_delivered_step_alike(raw):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    common = dict(batch_size=2, sample_length=T, image_size=HW, im_scale=HW, dtype="bf16", l_inf_pert_norm=0.2, flicker_time="video", flicker_period=5)
    W = vs.synthetic_weights("r3d_18", 42)
    a, b = FlickerVideoResNet("r3d_18", W, **common), FlickerVideoResNet("r3d_18", W, train_delivered=False, **common)
    outs = []
    for eng in (a, b):
        x = eng.prepare_videos(raw)
        labels = eng.logits(x, False).argmax(1)
        for _ in range(2):
            eng.step(x, labels, criterion(), lr=1e-2)
        outs.append((eng._logits.clone(), eng.pert_model.perturbation.clone(), eng._red.clone()))
        with pytest.raises(ValueError, match="train_delivered"):
            eng.step_videos(raw, labels, criterion())
    assert all(same_bits(p, q) for p, q in zip(*outs))


def test_train_delivered_refusals():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    W = vs.synthetic_weights("r3d_18", 42)
    kw = dict(batch_size=2, sample_length=T, image_size=HW, dtype="bf16", train_delivered=True)
    with pytest.raises(ValueError, match="readout"):
        FlickerVideoResNet("r3d_18", W, flicker_time="video", capture=vs.CaptureChannel(readout=(0.5, 0.9)), **kw)
    with pytest.raises(ValueError):
        FlickerVideoResNet("r3d_18", W, flicker_time="video", per_clip=True, **kw)
    with pytest.raises(ValueError, match="train_delivered"):
        FlickerVideoResNet("r3d_18", W, flicker_time="clip", **kw)
    with pytest.raises(ValueError, match="train_delivered"):
        FlickerVideoResNet("r3d_18", W, attack_type="L12", **kw)


def test_universal_script_trains_delivered(tmp_path):
    """one --train-delivered run of the universal script on a tiny raw whole-video file finishes and writes its results"""
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
            "--batch-size", "2", "--sample-length", "8", "--image-size", "64", "--im-scale", "64", "--epochs", "1", "--train-delivered"]
    r = subprocess.run(base + ["--flicker-time", "video", "--flicker-period", "5", "--results-root", str(tmp_path / "out")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "epoch 1" in r.stdout
    assert glob.glob(str(tmp_path / "out" / "**" / "*.npy"), recursive=True)
    bad = subprocess.run(base + ["--flicker-time", "clip", "--results-root", str(tmp_path / "out2")], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--train-delivered" in bad.stderr
