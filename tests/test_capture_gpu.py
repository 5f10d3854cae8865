"""The capture channel on the GPU: the two kernels that record a period-P flicker through a camera's exposure window and colour gain and
fold the per-clip gradient back (flk_flicker_rows_mix / flk_flicker_rows_mix_grad) against their numpy float32 restatements, bit for bit,
at the sizes where their loops can go wrong; at the identity channel they are the gather and the row gradient; an engine built with
``capture`` steps on the logits of the video ``export_video(capture=)`` delivers, folds its gradient through the same tables, and is
today's engine when the feature is off; ``evaluate_videos`` scores the attack over random captures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T, HW, NFRAMES = 8, 64, 37
FIXED = {"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def channel_tables(nb, K, seed, gain=True):
    """random taps (not normalised: the kernels take any) and gains, one row per clip"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (nb, K)).astype(np.float32), (rng.uniform(0.5, 1.5, (nb, 3)).astype(np.float32) if gain else None)


def edge_rows(P, nb, clip_T, seed):
    """random rows that contain P-1 and, outside the period, -1 and P (clamped by the mix, skipped by its gradient)"""
    rows = np.random.default_rng(seed).integers(0, P, (nb, clip_T)).astype(np.int32)
    flat = rows.reshape(-1)
    flat[0] = P - 1
    if flat.shape[0] >= 3:
        flat[1], flat[-1] = -1, P
    return rows


# ---- the mix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("P", [1, 2, 3, 5, 682])
def test_mix_is_the_restatement(P, K):
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    delta = np.random.default_rng(P + K).standard_normal((P, 3)).astype(np.float32)
    delta[0, 0], delta[P - 1, 2] = -0.0, -0.0
    for clip_T, nb in ((1, 5), (3, 4), (8, 3)):
        rows = edge_rows(P, nb, clip_T, seed=clip_T)
        taps, gain = channel_tables(nb, K, seed=P * K + clip_T)
        taps[0, 0] = 1.0                                                # ... so that a -0 of delta reaches the output of a K = 1 clip
        got = ops.flicker_rows_mix(dev(delta), dev(rows), dev(taps), dev(gain))
        assert tuple(got.shape) == (nb, clip_T, 3) and same_bits(got, vs.flicker_rows_mix(delta, rows, clip_T, taps, gain))
        plain = ops.flicker_rows_mix(dev(delta), dev(rows), dev(taps))
        assert same_bits(plain, vs.flicker_rows_mix(delta, rows, clip_T, taps, None))
        assert same_bits(plain, ops.flicker_rows_mix(dev(delta), dev(rows), dev(taps), torch.ones((nb, 3), device="cuda")))      # gain 1 = no gain
        out = torch.full((nb, clip_T, 3), 7.0, device="cuda")
        assert ops.flicker_rows_mix(dev(delta), dev(rows), dev(taps), dev(gain), out=out) is out and same_bits(out, got)
    if K == 1:                                                          # -0 kept: the first product starts the sum
        one = ops.flicker_rows_mix(dev(delta), dev(np.zeros((1, 1), np.int32)), torch.ones((1, 1), device="cuda"))
        assert bool(torch.signbit(one[0, 0, 0])) and float(one[0, 0, 0]) == 0.0


def test_mix_grid_stride_loop_iterates():
    """3n = 270 000 values > 1024 workgroups x 256 threads: every thread of the capped grid takes a second value"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    P, K, nb, clip_T = 5, 3, 30000, 3
    assert 3 * nb * clip_T > 1024 * 256
    delta = np.random.default_rng(1).standard_normal((P, 3)).astype(np.float32)
    rows = edge_rows(P, nb, clip_T, seed=2)
    taps, gain = channel_tables(nb, K, seed=3)
    got = ops.flicker_rows_mix(dev(delta), dev(rows), dev(taps), dev(gain))
    assert same_bits(got, vs.flicker_rows_mix(delta, rows, clip_T, taps, gain))


# ---- its transpose -----------------------------------------------------------------------------------------------------------------
# (n, clip_T): one frame; the last entry of the first LDS piece (2048 entries), a full piece, one entry into the second; clips of 7
# frames that straddle the piece boundary (2051 = 293 x 7), and three pieces (4102 = 586 x 7)
GRAD_N = [(1, 1), (2047, 1), (2048, 1), (2049, 1), (2051, 7), (4102, 7)]
# (P, K): 8 workgroups; two workgroups, the second with 2 live threads (3 * 86 = 258); the period shorter than the taps
GRAD_PK = [(682, 3), (86, 2), (86, 1), (1, 4), (2, 4), (3, 4)]


@pytest.mark.parametrize("P,K", GRAD_PK, ids=[f"P{p}_K{k}" for p, k in GRAD_PK])
@pytest.mark.parametrize("n,clip_T", GRAD_N, ids=[f"n{n}_T{t}" for n, t in GRAD_N])
def test_mix_gradient_is_the_restatement(n, clip_T, P, K):
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    nb = n // clip_T
    rows = edge_rows(P, nb, clip_T, seed=n + P)
    g = np.random.default_rng(n + K).standard_normal((nb, clip_T, 3)).astype(np.float32)
    taps, gain = channel_tables(nb, K, seed=n * K + P)
    for gn in (gain, None):
        want = vs.flicker_rows_mix_grad(g, rows, clip_T, taps, gn, P)
        out = torch.full((P, 3), np.nan, device="cuda")
        got = ops.flicker_rows_mix_grad(dev(g), dev(rows), P, dev(taps), None if gn is None else dev(gn), out=out)
        assert got is out and tuple(got.shape) == (P, 3) and same_bits(got, want)
        assert same_bits(ops.flicker_rows_mix_grad(dev(g), dev(rows), P, dev(taps), None if gn is None else dev(gn)), got)      # a second call


def test_mix_gradient_unhit_rows_are_zero_and_bad_rows_are_skipped():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    rng = np.random.default_rng(5)
    rows = rng.choice(np.array([1, 4, -1, 9], np.int32), (3, 8)).astype(np.int32)        # K = 2 reaches rows 1, 2, 4, 5 of 9; -1 and 9 are no rows
    g = rng.standard_normal((3, 8, 3)).astype(np.float32)
    taps, gain = channel_tables(3, 2, seed=6)
    out = torch.full((9, 3), np.nan, device="cuda")
    got = ops.flicker_rows_mix_grad(dev(g), dev(rows), 9, dev(taps), dev(gain), out=out).cpu().numpy()
    assert same_bits(got, vs.flicker_rows_mix_grad(g, rows, 8, taps, gain, 9))
    assert np.array_equal(got[[0, 3, 6, 7, 8]].view(np.uint32), np.zeros((5, 3), np.uint32)) and np.abs(got[[1, 2, 4, 5]]).min() > 0
    g_in = g.copy()
    g_in[(rows < 0) | (rows >= 9)] = np.nan                            # what a skipped frame holds never reaches a sum
    assert same_bits(ops.flicker_rows_mix_grad(dev(g_in), dev(rows), 9, dev(taps), dev(gain)), got)


@pytest.mark.parametrize("P,B,Tc", [(1, 1, 1), (5, 2, 8), (7, 3, 8), (682, 64, 32), (3, 3, 683)], ids=lambda v: str(v))
def test_identity_channel_is_the_gather_and_the_row_gradient(P, B, Tc):
    from flickering_adversarial_video_amd import ops
    rng = np.random.default_rng(P + B)
    delta, g = dev(rng.standard_normal((P, 3)).astype(np.float32)), dev(rng.standard_normal((B, Tc, 3)).astype(np.float32))
    delta[0, 1] = -0.0
    rows = dev(rng.integers(0, P, (B, Tc)).astype(np.int32))
    one, ones = torch.ones((B, 1), device="cuda"), torch.ones((B, 3), device="cuda")
    for gain in (None, ones):
        assert same_bits(ops.flicker_rows_mix(delta, rows, one, gain), ops.flicker_rows_gather(delta, rows))
        assert same_bits(ops.flicker_rows_mix_grad(g, rows, P, one, gain), ops.flicker_rows_grad(g, rows, P))


def test_argument_discipline():
    from flickering_adversarial_video_amd import ops
    delta, rows = torch.zeros((5, 3), device="cuda"), torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    g, taps, gain = torch.ones((2, 8, 3), device="cuda"), torch.ones((2, 2), device="cuda"), torch.ones((2, 3), device="cuda")
    bad_rows = np.array([[0, 5] * 4] * 2, np.int32)
    for what, call in (("int32", lambda: ops.flicker_rows_mix(delta, rows.long(), taps)), ("int32", lambda: ops.flicker_rows_mix(delta, rows.cpu(), taps)),
                       ("int32", lambda: ops.flicker_rows_mix_grad(torch.ones((8, 2, 3), device="cuda"), rows.t(), 5, taps)),
                       ("delta", lambda: ops.flicker_rows_mix(delta.double(), rows, taps)), ("delta", lambda: ops.flicker_rows_mix(delta.t(), rows, taps)),
                       ("taps", lambda: ops.flicker_rows_mix(delta, rows, taps.double())), ("taps", lambda: ops.flicker_rows_mix(delta, rows, taps.cpu())),
                       ("taps", lambda: ops.flicker_rows_mix(delta, rows, torch.ones((2, 4), device="cuda")[:, :2])),
                       ("taps", lambda: ops.flicker_rows_mix(delta, rows, torch.ones((2, 5), device="cuda"))),
                       ("taps", lambda: ops.flicker_rows_mix_grad(g, rows, 5, torch.ones((2, 5), device="cuda"))),
                       ("taps", lambda: ops.flicker_rows_mix(delta, rows, torch.ones((3, 2), device="cuda"))),
                       ("taps", lambda: ops.flicker_rows_mix(delta, rows, torch.ones((2, 0), device="cuda"))),
                       ("gain", lambda: ops.flicker_rows_mix(delta, rows, taps, gain[:, :2])), ("gain", lambda: ops.flicker_rows_mix(delta, rows, taps, gain.cpu())),
                       ("gain", lambda: ops.flicker_rows_mix_grad(g, rows, 5, taps, gain.double())),
                       ("out", lambda: ops.flicker_rows_mix(delta, rows, taps, out=torch.zeros((2, 8, 2), device="cuda"))),
                       ("out", lambda: ops.flicker_rows_mix_grad(g, rows, 5, taps, out=torch.zeros((4, 3), device="cuda"))),
                       ("g_clip", lambda: ops.flicker_rows_mix_grad(g[:, :4], rows, 5, taps)), ("g_clip", lambda: ops.flicker_rows_mix_grad(g.cpu(), rows, 5, taps)),
                       ("period", lambda: ops.flicker_rows_mix_grad(g, rows, 683, taps)), ("period", lambda: ops.flicker_rows_mix_grad(g, rows, 0, taps)),
                       ("period", lambda: ops.flicker_rows_mix(torch.zeros((683, 3), device="cuda"), rows, taps)),
                       (r"rows must lie in \[0,5\)", lambda: ops.flicker_rows_mix(delta, rows, taps, rows_host=bad_rows)),
                       (r"rows must lie in \[0,5\)", lambda: ops.flicker_rows_mix_grad(g, rows, 5, taps, rows_host=bad_rows))):
        with pytest.raises(ValueError, match=what):
            call()


# ---- engines ---------------------------------------------------------------------------------------------------------------------
_ENGINES = {}
VIDEO_KW = dict(flicker_time="video", clips_per_video=2, video_reduce="sum", im_scale=HW, quantise_train=True)      # one video of two clips per batch


def channel(**kw):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    return vs.CaptureChannel(**kw)


def fixed_channel():
    """the distribution that has one channel: FIXED"""
    return channel(subframe=FIXED["subframe"], exposure=FIXED["exposure"], gain=FIXED["gain"], gain_mode="per_channel")


def engine(key, **kw):
    """r3d_18 on synthetic weights, 2 clips of 8 x 64 x 64, bf16: the smallest engine the video-time tests use; one per ``key``"""
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
def test_the_step_sees_the_captured_video(P):
    """clips cut from a video, perturbed through a capture channel by their frame numbers' rows and the 8-bit round trip, are bit for
    bit the clips cut from the video exported through that channel -- at a non-zero phase, with a step between the frames"""
    eng = engine(("fixed", P), flicker_period=P, capture=fixed_channel(), **VIDEO_KW)
    video, table = video_u8(), table_of(sample_step=2)
    assert any(int(t[0]) % P for t in table) and int(table[0, 1] - table[0, 0]) == 2          # a clip off the period's grid, a step between frames
    idx = torch.from_numpy(table).cuda()
    clips = video[idx]
    eng.set_frame_numbers(table)
    set_delta(eng, 23)
    for phase in (3, 1):
        got = eng.logits(clips, True, phases=phase, capture=FIXED).clone()
        assert same_bits(got, eng.logits(eng.export_video(video, phase=phase, capture=FIXED)[idx], False))
        # without the channel the same engine gives other logits, and so does the export
        plain = eng.logits(clips, True, phases=phase).clone()
        assert not same_bits(plain, got) and same_bits(plain, eng.logits(eng.export_video(video, phase=phase)[idx], False))
    lc = eng.last_capture
    assert lc["taps"].shape == (2, 2) and np.array_equal(lc["gain_rows"], np.array([[0.9, 0.8, 0.7]] * 2, np.float32))
    assert same_bits(eng.quantised_logits(clips, capture=FIXED), eng.logits(clips, True, phases=0, capture=FIXED).clone())


def test_video_level_verdict_is_the_captured_videos():
    """the step's video logits under a fixed channel are those evaluate_videos(quantise="video", capture=) gives the video exported
    through it"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    ch = fixed_channel()
    eng = engine("verdict", capture=ch, **VIDEO_KW)
    video = video_u8(seed=29)
    x = eng.prepare_videos([video], train=False, num_samples=2).clone()
    table = np.concatenate(eng.last_sampling)
    assert same_bits(x, vs.normalize_u8(video.cpu().numpy()[table]))
    lab = eng.video_logits(eng.logits(x, False)).argmax(1).clone()
    set_delta(eng, 31)
    res = eng.step(x, lab, criterion(), update=False)
    stepped = res["video_logits"].clone()
    assert eng.last_capture["subframe"].tolist() == [0.3] and eng.last_capture["exposure"].tolist() == [1.5]
    assert np.array_equal(eng.last_capture["gain"], np.array([FIXED["gain"]], np.float32))
    ev = eng.evaluate_videos([video], lab, num_samples=2, quantise="video", capture=ch, capture_draws=1)
    assert same_bits(stepped, ev["capture_video_logits"][0])
    # the same engine without the channel reproduces neither
    assert not same_bits(ev["video_logits"], stepped)
    assert not same_bits(eng.evaluate_videos([video], lab, num_samples=2, quantise="video")["video_logits"], stepped)
    assert eng.pert_model.frame_numbers.tolist() == table.tolist()


def test_gradient_is_the_mix_gradient_of_the_per_clip_gradient():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    P = 5
    eng = engine(("grad", P), flicker_period=P, capture=channel(subframe=0.3, exposure=1.5, gain=(0.7, 0.9), gain_mode="per_channel"), **VIDEO_KW)
    ident = engine(("ident", P), flicker_period=P, capture=channel(subframe=0.0), **VIDEO_KW)
    plain = engine(("plain", P), flicker_period=P, **VIDEO_KW)
    video, table = video_u8(), table_of(sample_step=1)
    x = video[torch.from_numpy(table).cuda()]
    for e in (eng, ident, plain):
        e.set_frame_numbers(table)
        set_delta(e, 19)
    lab = plain.video_logits(plain.logits(x, False)).argmax(1).clone()
    eng.step(x, lab, criterion(), update=False)
    got = eng._red[:3 * P].view(P, 3).clone()
    lc, rows = eng.last_capture, eng.pert_model.rows_host
    assert lc["taps"].shape == (2, 2) and lc["gain_rows"].shape == (2, 3) and np.array_equal(lc["gain_rows"][0], lc["gain_rows"][1])
    assert np.array_equal(lc["gain_rows"][0], lc["gain"][0]) and len(set(lc["gain"][0].tolist())) == 3
    want = ops.flicker_rows_mix_grad(eng._g_clip, eng.pert_model.rows_dev, P, dev(lc["taps"]), dev(lc["gain_rows"]), rows_host=rows)
    assert same_bits(got, want) and float(got.abs().max()) > 0 and bool(torch.isfinite(got).all())
    assert same_bits(want, vs.flicker_rows_mix_grad(eng._g_clip.cpu().numpy(), rows, T, lc["taps"], lc["gain_rows"], P))
    # the identity channel (sub-frame phase 0, exposure 1, gain 1): the payload of an engine built without capture
    ident.step(x, lab, criterion(), update=False)
    plain.step(x, lab, criterion(), update=False)
    assert ident.last_capture["taps"].tolist() == [[1.0], [1.0]] and plain.last_capture is None
    assert same_bits(ident._red, plain._red) and not same_bits(got, plain._red[:3 * P].view(P, 3))


def test_capture_none_is_the_engine_without_the_argument():
    a, b = engine("off_a", flicker_period=5, capture=None, **VIDEO_KW), engine("off_b", flicker_period=5, **VIDEO_KW)
    video, table = video_u8(seed=37), table_of(sample_step=1)
    x = video[torch.from_numpy(table).cuda()]
    outs = []
    for e in (a, b):
        e.set_frame_numbers(table)
        set_delta(e, 41)
        e.adam_m.zero_(); e.adam_v.zero_()
        e.adam_t = 0
        lab = e.video_logits(e.logits(x, False)).argmax(1).clone()
        got = []
        for _ in range(3):
            r = e.step(x, lab, criterion(), lr=1e-2, update=True)
            got += [r["softmax"].clone(), r["adv_loss"].clone().reshape(1)]
        outs.append(got + [e.pert_model.perturbation.clone()])
        assert e.last_capture is None and e.pert_model.taps_dev is None
    assert all(same_bits(p, q) for p, q in zip(*outs)) and not same_bits(outs[0][-1], dev(np.zeros((5, 3), np.float32)))


def test_evaluate_videos_over_capture_draws():
    ch = channel(subframe=(0, 1), exposure=(0.5, 2), gain=(0.7, 1.0), gain_mode="per_channel", seed=5)
    eng = engine("eval", capture=ch, **VIDEO_KW)
    videos = [video_u8(seed=43), video_u8(seed=47)[:29]]
    set_delta(eng, 53)
    lab = eng.evaluate_videos(videos, np.zeros(2, np.int64), num_samples=2)["video_preds"]      # every video counts towards the ratio
    base = eng.evaluate_videos(videos, lab, num_samples=2, adversarial=True)
    state = ch._rng.bit_generator.state
    assert eng.evaluate_videos(videos, lab, num_samples=2, adversarial=True).keys() == base.keys() and ch._rng.bit_generator.state == state
    assert not any(k.startswith("capture") for k in base)              # without capture: today's keys
    ev = eng.evaluate_videos(videos, lab, num_samples=2, adversarial=True, capture=ch, capture_draws=2)
    assert set(ev) - set(base) == {"capture_draws", "capture_clip_logits", "capture_video_logits", "capture_video_fooling_ratios",
                                   "capture_video_fooling_ratio_mean", "capture_video_fooling_ratio_min"}
    assert all(same_bits(ev[k], base[k]) if isinstance(base[k], np.ndarray) else ev[k] == base[k] or base[k] != base[k] for k in base)
    C = eng.num_classes
    assert ev["capture_video_logits"].shape == (2, 2, C) and ev["capture_clip_logits"].shape == (2, 4, C) and ev["capture_video_fooling_ratios"].shape == (2,)
    draws = ev["capture_draws"]
    assert len(draws) == 2 and all(d["subframe"].shape == (2,) and d["exposure"].shape == (2,) and d["gain"].shape == (2, 3) for d in draws)
    assert not np.array_equal(draws[0]["subframe"], draws[1]["subframe"])
    r = ev["capture_video_fooling_ratios"]
    assert not np.isnan(r).any()
    if True:
        assert ev["capture_video_fooling_ratio_mean"] == float(r.mean()) and ev["capture_video_fooling_ratio_min"] == float(r.min())
    # draw j, video v: its two clips (one batch of the engine) are logits(x, True, phases=0, capture=<video v's channel of draw j>)
    for j, d in enumerate(draws):
        for v, video in enumerate(videos):
            x = eng.prepare_videos([video], num_samples=2).clone()
            one = {k: d[k][v:v + 1] for k in d}
            assert same_bits(eng.logits(x, True, phases=0, capture=one), ev["capture_clip_logits"][j, 2 * v:2 * v + 2])
        assert same_bits(ev["capture_video_logits"][j], ev["capture_clip_logits"][j][0::2] + ev["capture_clip_logits"][j][1::2])
        assert not same_bits(ev["capture_clip_logits"][j], base["clip_logits"])
    for q in ("clip", "video"):
        evq = eng.evaluate_videos(videos[:1], lab[:1], num_samples=2, quantise=q, capture=ch, capture_draws=1)
        assert evq["capture_video_logits"].shape == (1, 1, C) and not same_bits(evq["capture_video_logits"][0], evq["video_logits"])
    with pytest.raises(ValueError, match="capture"):
        eng.evaluate_videos(videos, lab, num_samples=2, capture=ch)     # a clean evaluation has no flicker to capture
    with pytest.raises(ValueError, match="capture_draws"):
        eng.evaluate_videos(videos, lab, num_samples=2, adversarial=True, capture=ch, capture_draws=0)


def test_training_forwards_draw_one_channel_per_video():
    ch = channel(subframe=(0, 1), exposure=(0.5, 2), seed=9)
    eng = engine("draws", batch_size=4, capture=ch, **VIDEO_KW)           # two videos of two clips
    video = video_u8(seed=59)
    x = eng.prepare_videos([video, video[:30]], num_samples=2).clone()
    set_delta(eng, 61)
    lab = eng.video_logits(eng.logits(x, False)).argmax(1).clone()
    assert eng.last_capture is None                                     # a clean forward draws nothing
    seen = []
    for _ in range(2):
        eng.step(x, lab, criterion(), update=False)
        lc = eng.last_capture
        assert lc["subframe"].shape == (2,) and lc["taps"].shape[0] == 4 and lc["gain_rows"].shape == (4, 3)
        assert np.array_equal(lc["taps"][0], lc["taps"][1]) and np.array_equal(lc["taps"][2], lc["taps"][3])          # the G clips share one
        assert not np.array_equal(lc["taps"][0], lc["taps"][2]) and lc["subframe"][0] != lc["subframe"][1]
        assert same_bits(eng.pert_model.taps_dev, lc["taps"]) and same_bits(eng.pert_model.gain_dev, lc["gain_rows"])
        seen.append(lc["subframe"].copy())
    assert not np.array_equal(seen[0], seen[1])
    # evaluation and export without a channel leave the generator alone
    state = ch._rng.bit_generator.state
    eng.evaluate_videos([video], lab[:1].cpu().numpy(), num_samples=2, adversarial=True)
    eng.export_video(video)
    eng.logits(x, True, phases=0)
    assert ch._rng.bit_generator.state == state
    eng.logits(x, True, phases=0, capture="draw")
    assert ch._rng.bit_generator.state != state
    with pytest.raises(ValueError, match="draw"):
        engine("off_b", flicker_period=5, **VIDEO_KW).logits(x[:2], True, capture="draw")
