"""``evaluate_videos`` where its packing is not one video per batch: three raw videos of differing length and resolution, three clips
each, batches of two -- nine clips in five batches, the middle video straddling a batch boundary (clips 3 | 4 5) and the last batch
padded -- under ``quantise``, ``capture`` and ``codec`` on a video-time engine.  Every comparison is BITWISE.  The delivered-video cases
are compared with a CLEAN ``evaluate_videos`` over the exported videos: both calls share one packing, so nothing is assumed about the
rows of a batch being independent.  The clip-level cases restate the packing by hand."""
import numpy as np
import pytest
import torch

from test_codec_gpu import same_bits, smooth

pytestmark = pytest.mark.gpu
T, HW, B, S, V, P = 8, 64, 2, 3, 3, 5
CODEC = dict(quality=60, subsampling="420")
CHANNEL = dict(subframe=(0.0, 1.0), exposure=(0.5, 2.0), gain=(0.5, 1.0), gain_mode="per_channel")
_CACHE = {}


@pytest.fixture(scope="module")
def setup():
    """the engine (r3d_18 on synthetic weights, flicker of period 5 on video time, a perturbation beyond its bound too), the videos
    (20 x 72 x 100, 14 x 90 x 82, 11 x 66 x 120: none a whole number of 16 x 16 MCUs) and labels: the clean verdicts, one of them wrong"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=B, sample_length=T, image_size=HW, im_scale=HW, dtype="bf16",
                             l_inf_pert_norm=0.2, flicker_time="video", flicker_period=P)
    eng.pert_model.init_perturbation(np.random.default_rng(18).uniform(-0.25, 0.25, (3, P, 1, 1)).astype(np.float32))
    vids = [smooth(20, 72, 100, 51), smooth(14, 90, 82, 52), smooth(11, 66, 120, 53)]
    for v in vids:
        v[:, :2], v[:, 2:4] = 0, 255
    vids = [torch.from_numpy(v).cuda() for v in vids]
    labels = eng.evaluate_videos(vids, np.zeros(V, np.int64), num_samples=S)["video_preds"].copy()
    labels[2] = (labels[2] + 1) % eng.num_classes
    assert V * S == 9 and (V * S) % B == 1 and S % B == 1            # a padded last batch; video 1 holds clips 3 | 4 5
    return eng, vids, labels


def codec_of(env_codec):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    return vs.Codec(**CODEC) if env_codec else None


def marked(eng):
    """frame numbers of the caller's own, set before a call: the call must leave them as they are"""
    table = np.arange(B * T, dtype=np.int64).reshape(B, T) * 3 + 1
    eng.set_frame_numbers(table)
    return table


def evaluated(setup, quantise, with_codec=False):
    """the call without ``capture``, made once per setting and left unchanged"""
    eng, vids, labels = setup
    key = (quantise, with_codec)
    if key not in _CACHE:
        table = marked(eng)
        _CACHE[key] = eng.evaluate_videos(vids, labels, num_samples=S, adversarial=True, quantise=quantise, codec=codec_of(with_codec))
        assert np.array_equal(eng.pert_model.frame_numbers, table)
    return _CACHE[key]


def same_value(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_value(p, q) for p, q in zip(a, b))
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return same_bits(a, b)
    return type(a) is type(b) and (a == b or (a != a and b != b))


def one_channel(draw, v):
    return {k: (draw[k][v] if k == "gain" else float(draw[k][v])) for k in draw}


@pytest.mark.parametrize("with_codec", [False, True], ids=["plain", "codec"])
def test_quantise_video_is_the_clean_evaluation_of_the_exported_videos(setup, with_codec):
    from flickering_adversarial_video_amd import ops
    eng, vids, labels = setup
    codec = codec_of(with_codec)
    ev = evaluated(setup, "video", with_codec)
    pairs = [eng.export_video(v, stats=True) for v in vids]
    clean = eng.evaluate_videos([eng.export_video(v, codec=codec) for v in vids], labels, num_samples=S)
    assert ev["clip_logits"].shape == (V * S, eng.num_classes) and same_bits(ev["clip_logits"], clean["clip_logits"])
    assert same_bits(ev["video_logits"], clean["video_logits"]) and np.array_equal(ev["video_preds"], clean["video_preds"])
    assert not same_bits(ev["clip_logits"], ev["clean_clip_logits"])
    assert len(ev["realised_flicker"]) == V
    for v, (got, (_, st)) in enumerate(zip(ev["realised_flicker"], pairs)):
        assert same_bits(got, st[:, :, 0].cpu().numpy() / float(vids[v].shape[1] * vids[v].shape[2])), v
    if with_codec:
        _, stats = ops.codec_roundtrip([p[0] for p in pairs], codec, stats=True)
        assert len(ev["codec_stats"]) == V and all(same_bits(a, b) for a, b in zip(ev["codec_stats"], stats))
        assert not same_bits(ev["clip_logits"], evaluated(setup, "video", False)["clip_logits"])
    else:
        assert "codec_stats" not in ev


@pytest.mark.parametrize("with_codec", [False, True], ids=["plain", "codec"])
def test_quantise_video_capture_draws_are_the_clean_evaluations_of_their_exports(setup, with_codec):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    eng, vids, labels = setup
    codec = codec_of(with_codec)
    ch, twin = vs.CaptureChannel(seed=7, **CHANNEL), vs.CaptureChannel(seed=7, **CHANNEL)
    table = marked(eng)
    ev = eng.evaluate_videos(vids, labels, num_samples=S, quantise="video", capture=ch, capture_draws=2, codec=codec)
    assert np.array_equal(eng.pert_model.frame_numbers, table)
    assert same_value(ev["capture_draws"], [twin.draw(V), twin.draw(V)]) and same_value(ch.draw(V), twin.draw(V))
    assert ev["capture_clip_logits"].shape == (2, V * S, eng.num_classes)
    for j, d in enumerate(ev["capture_draws"]):
        exported = [eng.export_video(v, capture=one_channel(d, i), codec=codec) for i, v in enumerate(vids)]
        clean = eng.evaluate_videos(exported, labels, num_samples=S)
        assert same_bits(ev["capture_clip_logits"][j], clean["clip_logits"]), j
        assert same_bits(ev["capture_video_logits"][j], clean["video_logits"]), j
    assert not same_bits(ev["capture_clip_logits"][0], ev["capture_clip_logits"][1])
    assert not same_bits(ev["capture_clip_logits"][0], ev["clip_logits"])
    plain = evaluated(setup, "video", with_codec)
    rest = {k for k in ev if not k.startswith("capture_")}
    assert rest == set(plain) and all(same_value(ev[k], plain[k]) for k in rest)


@pytest.mark.parametrize("quantise", [None, "clip"], ids=["adversarial", "clip"])
def test_clip_level_scoring_is_the_packing_by_hand(setup, quantise):
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    eng, vids, labels = setup
    ch, twin = vs.CaptureChannel(seed=9, **CHANNEL), vs.CaptureChannel(seed=9, **CHANNEL)
    table = marked(eng)
    ev = eng.evaluate_videos(vids, labels, num_samples=S, adversarial=True, quantise=quantise, capture=ch, capture_draws=1)
    assert np.array_equal(eng.pert_model.frame_numbers, table)
    assert same_value(ev["capture_draws"], [twin.draw(V)]) and same_value(ch.draw(V), twin.draw(V))
    d = ev["capture_draws"][0]
    rows = np.concatenate(eng.last_sampling)
    assert rows.shape == (V * S, T)
    adv, cap, flick = [], [], []
    for first in range(0, V * S, B):
        ks = [min(first + b, V * S - 1) for b in range(B)]
        n = min(B, V * S - first)
        x = ops.prepare_clips([vids[k // S] for k in ks], im_scale=HW, input_size=(HW, HW), frame_idx=rows[ks])
        eng.set_frame_numbers(rows[ks])
        per_clip = {k: d[k][np.asarray(ks) // S] for k in d}
        if quantise == "clip":
            frames, st = eng.adversarial_frames(x, stats=True)
            adv.append(eng.logits(frames, False)[:n].cpu().clone())
            flick.append(st[:n, :, :, 0].cpu().numpy() / float(HW * HW))
            cap.append(eng.logits(eng.adversarial_frames(x, capture=per_clip), False)[:n].cpu().clone())
        else:
            adv.append(eng.logits(x, True, phases=0)[:n].cpu().clone())
            cap.append(eng.logits(x, True, phases=0, capture=per_clip)[:n].cpu().clone())
    assert same_bits(ev["clip_logits"], torch.cat(adv)) and same_bits(ev["capture_clip_logits"][0], torch.cat(cap))
    assert not same_bits(ev["clip_logits"], ev["capture_clip_logits"][0])
    if quantise == "clip":
        assert same_bits(ev["realised_flicker"], np.concatenate(flick))
    plain = evaluated(setup, quantise)
    rest = {k for k in ev if not k.startswith("capture_")}
    assert rest == set(plain) and all(same_value(ev[k], plain[k]) for k in rest)
