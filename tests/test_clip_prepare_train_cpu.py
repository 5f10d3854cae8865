"""The training transform without a GPU: the host sampler (videoresnet_spec.train_crop_params) against the boxes and flips the reference's
own classes drew (tests/golden/clip_prepare_train_golden.npz), the host A/B route (videoresnet_spec.prepare_host_train, the scripts'
``--prepare host --train-transforms train``) against the fixture bit for bit, flk_clip_prepare_train's argument validation, and the
ValueErrors of the Python surface that need no device."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_prepare_train_golden as gold  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return gold.load_cases()


def test_fixture_covers_the_cases(cases):
    assert [(c["H"], c["W"], c["rseed"]) for c in cases] == [(H, W, s) for H, W in gold.SIZES for s in gold.SEEDS]
    assert {c["flip"] for c in cases} == {False, True}
    assert all(c["out"].shape == (gold.T, 112, 112, 3) and c["out"].dtype == np.float32 for c in cases)
    # boxes that enlarge one axis and shrink the other are among them
    assert any((c["box"][2] - 112) * (c["box"][3] - 112) < 0 for c in cases)
    here = os.path.dirname(gold.OUT)
    assert os.path.getsize(gold.OUT) <= os.path.getsize(os.path.join(here, "clip_prepare_golden.npz"))
    names = {r["name"] for r in gold.load_sampler_records()}
    assert {"fallback_227x128", "randomcrop_128x170", "randomcrop_112x112", "seq_128x170", "seq_227x128", "seq_128x128", "seq_127x169", "seq_128x171"} == names


def test_exact_restatement_at_the_centre_crop_is_the_evaluation_restatement(cases):
    """restate_train_fp64 on the evaluation transform's own window, no flip: stage 2 is the identity, the value is restate_fp64's"""
    import make_prepare_golden as gold_eval
    for c in cases[::3]:
        for rule in ("sizes", "scale_factor"):
            i, j = int(round((c["Hr"] - 112) / 2.0)), int(round((c["Wr"] - 112) / 2.0))
            a = gold.restate_train_fp64(c["frames"], (i, j, 112, 112), False, rule)
            assert np.array_equal(a, gold_eval.restate_fp64(c["frames"], rule)), (c["name"], rule)


def test_sampler_reproduces_the_reference_draws(cases):
    """random.Random(s) through train_crop_params = the reference's classes under random.seed(s): every box, every flip, and the state
    the generator is left in (the next draw)"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    for c in cases:
        rng = random.Random(c["rseed"])
        assert (c["Hr"], c["Wr"]) == vs.prepare_geometry(c["H"], c["W"], rule="scale_factor")[:2]
        got = vs.train_crop_params(c["Hr"], c["Wr"], rng=rng)
        assert got == c["box"] + (c["flip"],), (c["name"], got)
        assert rng.random() == c["next"], c["name"]
    for r in gold.load_sampler_records():
        rng = random.Random(r["seed"])
        for k, want in enumerate(r["draws"]):
            got = vs.train_crop_params(r["Hr"], r["Wr"], input_size=112, scales=r["scales"], rng=rng)
            assert [int(v) for v in got] == [int(v) for v in want], (r["name"], k, got, want)
        assert rng.random() == r["next"], r["name"]


def test_sampler_spelled_out_cases():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    recs = {r["name"]: r for r in gold.load_sampler_records()}
    # scale 1.0: w = round(sqrt(A r)) <= 128 and h = round(sqrt(A / r)) <= 227 cannot both hold for r in [3/4, 4/3] -> the central fallback,
    # in_ratio 128 / 227 = 0.564 < 3/4: w = 128, h = round(128 / 0.75) = 171, i = (227 - 171) // 2
    assert all(tuple(d[:4]) == (28, 0, 171, 128) for d in recs["fallback_227x128"]["draws"])
    assert all(tuple(d[2:4]) == (112, 112) for d in recs["randomcrop_128x170"]["draws"])
    assert all(tuple(d[:4]) == (0, 0, 112, 112) for d in recs["randomcrop_112x112"]["draws"])
    # the three fallback branches and the draw counts, on a generator whose consumption is counted
    class Counting(random.Random):
        n = 0

        def random(self):
            self.n += 1
            return super().random()
    # (a box of 1.2 times the image's area never fits: ten failures whatever the aspect ratio)
    for Hr, Wr, want in ((227, 128, (28, 0, 171, 128)), (128, 227, (0, 28, 128, 171)), (128, 128, (0, 0, 128, 128)), (120, 150, (0, 0, 120, 150))):
        rng = Counting(5)
        got = vs.train_crop_params(Hr, Wr, scales=(1.2, 1.2), rng=rng)
        assert got[:4] == want, (Hr, Wr, got)
        assert rng.n == 21                                  # 10 attempts of two uniforms, then the flip
    rng = Counting(5)
    assert vs.train_crop_params(112, 112, scales=None, flip_ratio=0.0, rng=rng) == (0, 0, 112, 112, False) and rng.n == 1   # the flip draw only, made even at p = 0
    with pytest.raises(ValueError):
        vs.train_crop_params(100, 200, scales=None)
    assert isinstance(vs.train_crop_params(128, 170)[4], bool)                          # no generator given: a fresh one


def test_host_route_reproduces_the_fixture_bitwise(cases):
    """``--prepare host --train-transforms train`` with --resize-rule scale_factor is the reference's torch calls on the recorded box:
    anything but equal bits is a wiring error"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    for c in cases:
        got = vs.prepare_host_train(c["frames"], c["box"], c["flip"], rule="scale_factor")
        assert got.dtype == torch.float32 and tuple(got.shape) == c["out"].shape
        assert np.array_equal(got.numpy().view(np.uint32), c["out"].view(np.uint32)), c["name"]


def test_host_route_identity_box_and_flip(cases):
    """the evaluation transform's window without a flip is prepare_host bit for bit under both rules; a flip reverses W; bad arguments"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    c = cases[0]
    for rule in vs.RESIZE_RULES:
        Hr, Wr, _, _, ci, cj = vs.prepare_geometry(c["H"], c["W"], rule=rule)
        a = vs.prepare_host_train(c["frames"], (ci, cj, 112, 112), False, rule=rule)
        assert torch.equal(a, vs.prepare_host(c["frames"], rule=rule))
        assert torch.equal(vs.prepare_host_train(c["frames"], (ci, cj, 112, 112), True, rule=rule), a.flip(2))
    assert torch.equal(vs.prepare_host_train(c["frames"], c["box"], True, input_size=(96, 128)),
                       vs.prepare_host_train(c["frames"], c["box"], False, input_size=(96, 128)).flip(2))
    for bad in ((0, 0, 0, 5), (-1, 0, 5, 5), (0, 0, 129, 5), (0, 166, 5, 5)):
        with pytest.raises(ValueError):
            vs.prepare_host_train(c["frames"], bad, False)
    with pytest.raises(ValueError):
        vs.prepare_host_train(c["frames"], c["box"], False, rule="nearest")
    with pytest.raises(ValueError):
        vs.prepare_host_train(c["frames"].astype(np.float32), c["box"], False)


def _valid_args(Hs=240, Ws=320):
    from flickering_adversarial_video_amd import _lib, videoresnet_spec as vs
    clip = _lib.PrepClip()
    clip.src, clip.T, clip.Hs, clip.Ws, clip.pitch_t, clip.pitch_h = 64, 2, Hs, Ws, Hs * Ws * 3, Ws * 3
    clip.Hr, clip.Wr, clip.step_h, clip.step_w, clip.crop_i, clip.crop_j = vs.prepare_geometry(Hs, Ws)
    arr = (_lib.PrepClip * 1)(clip)
    a = _lib.PrepareArgs()
    a.nclip, a.Ho, a.Wo = 1, 112, 112
    a.mean, a.std = (C.c_float * 3)(*vs.DEFAULT_MEAN), (C.c_float * 3)(*vs.DEFAULT_STD)
    a.out_clip_offset, a.out_clip_stride = 0, 2 * 112 * 112 * 3
    a.clips = arr
    boxes = (_lib.PrepBox * 1)(_lib.PrepBox(5, 8, 121, 160, 1))
    return a, arr, boxes


def test_argument_validation_without_gpu():
    """every invalid argument is FLK_EINVAL with a message, decided on the host before any GPU call (there is no GPU here)"""
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    out = C.c_void_p(64)

    def rc(mut=None, a_null=False, out_null=False, boxes_null=False):
        a, arr, boxes = _valid_args()
        if mut:
            mut(a, arr[0], boxes[0])
        r = lib.flk_clip_prepare_train(None if a_null else C.byref(a), None if boxes_null else boxes, None if out_null else out, None)
        assert r == 0 or len(lib.flk_last_error()) > 0
        return r

    def bad(mut, word, **kw):
        assert rc(mut, **kw) == -1 and word in lib.flk_last_error(), (word, lib.flk_last_error())

    # what flk_clip_prepare checks
    bad(None, b"null", a_null=True)
    bad(None, b"null", out_null=True)
    bad(lambda a, c, b: setattr(a, "clips", C.POINTER(_lib.PrepClip)()), b"null")
    bad(lambda a, c, b: setattr(c, "src", None), b"null")
    for n in (0, -1, _lib.FLK_PREP_MAX_CLIPS + 1):
        bad(lambda a, c, b: setattr(a, "nclip", n), b"nclip")
    for field in ("T", "Hs", "Ws", "Hr", "Wr", "pitch_t", "pitch_h"):
        for v in (0, -3):
            assert rc(lambda a, c, b: setattr(c, field, v)) == -1, field
    bad(lambda a, c, b: setattr(c, "pitch_h", 320 * 3 - 1), b"pitch")
    for field in ("Ho", "Wo"):
        bad(lambda a, c, b: setattr(a, field, 0), b"output size")
    for field in ("step_h", "step_w"):
        for v in (0.0, -1.875, float("nan"), float("inf")):
            bad(lambda a, c, b: setattr(c, field, v), b"step")
    for k in range(3):
        for v in (0.0, -0.2, float("nan")):
            def mut(a, c, b, k=k, v=v):
                a.std[k] = v
            bad(mut, b"std")
    bad(lambda a, c, b: setattr(a, "out_clip_stride", 2 * 112 * 112 * 3 - 1), b"out_clip_stride")
    assert rc(lambda a, c, b: setattr(a, "out_clip_offset", -1)) == -1
    # the new entry's own
    bad(None, b"null box", boxes_null=True)
    for field in ("h", "w"):
        for v in (0, -4):
            bad(lambda a, c, b: setattr(b, field, v), b"box size")
    for field, v in (("i", -1), ("j", -1), ("i", 128 - 121 + 1), ("j", 170 - 160 + 1), ("h", 129), ("w", 171)):
        bad(lambda a, c, b: setattr(b, field, v), b"outside the resized image")
    bad(lambda a, c, b: setattr(c, "Hr", 125), b"outside the resized image")
    for v in (2, -1):
        bad(lambda a, c, b: setattr(b, "flip", v), b"flip")
    # crop_i / crop_j are ignored by this entry: values flk_clip_prepare refuses are not what the call fails on
    def crop_out_and_flip(a, c, b):
        c.crop_i, c.crop_j, b.flip = -5, 4000, 2
    bad(crop_out_and_flip, b"flip")
    assert b"crop window" not in lib.flk_last_error()


def test_a_box_too_wide_to_stage_is_refused_without_gpu():
    """a box whose source rows and intermediate rows do not fit one workgroup's LDS is an error with a message, never truncated: decided
    on the host before the launch"""
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    a, arr, boxes = _valid_args(Hs=4000, Ws=16000)
    boxes[0].i, boxes[0].j, boxes[0].h, boxes[0].w = 0, 0, arr[0].Hr, arr[0].Wr           # 128 x 512 over 16000 source columns
    assert lib.flk_clip_prepare_train(C.byref(a), boxes, C.c_void_p(64), None) == -1
    assert b"stages" in lib.flk_last_error()


def test_python_surface_value_errors_without_gpu():
    from flickering_adversarial_video_amd import ops
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    x = torch.zeros((2, 1, 120, 160, 3), dtype=torch.uint8)
    box = (0, 0, 100, 100)
    with pytest.raises(ValueError, match="go together"):
        ops.prepare_clips(x, boxes=[box, box])
    with pytest.raises(ValueError, match="go together"):
        ops.prepare_clips(x, flips=[0, 1])
    with pytest.raises(ValueError, match="2 clips, 1 boxes and 2 flips"):
        ops.prepare_clips(x, boxes=[box], flips=[0, 1])
    with pytest.raises(ValueError, match="2 clips, 2 boxes and 3 flips"):
        ops.prepare_clips([x[0], x[1]], boxes=[box, box], flips=[0, 1, 0])
    # the engine: a malformed augment is refused before the device is looked for; train=True needs augment
    for aug in ({"scale": (0.6, 1.0)}, {"scales": (1.0, 0.6)}, {"scales": 0.6}, {"ratio": None}, {"flip_ratio": 1.5}, [0.6, 1.0]):
        with pytest.raises(ValueError, match="augment"):
            FlickerVideoResNet("r3d_18", {}, augment=aug)
    assert FlickerVideoResNet._check_augment(None) is None
    assert FlickerVideoResNet._check_augment({"scales": None, "seed": 4}) == {"scales": None, "ratio": (3 / 4, 4 / 3), "flip_ratio": 0.5, "seed": 4}
    eng = FlickerVideoResNet.__new__(FlickerVideoResNet)
    eng.augment, eng.T = None, 1
    with pytest.raises(ValueError, match="augment"):
        eng.prepare(x, train=True)


def test_script_keeps_raw_training_clips_for_the_host_training_transform(tmp_path, cases):
    """--prepare host --train-transforms train: the training clips stay raw at load time (every batch is prepared with fresh draws), the
    validation clips are prepared once as before"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import r2plus1d_main_universal_attack as uni
    c = cases[0]
    clips = np.stack([c["frames"], c["frames"][:, ::-1]])
    np.savez(tmp_path / "raw.npz", clips=clips, labels=np.array([1, 2]))
    x, y = uni.load_clips(str(tmp_path / "raw.npz"), prepare="host", keep_raw=True)
    assert x.dtype == np.uint8 and x.shape == clips.shape and list(y) == [1, 2]
    x, _ = uni.load_clips(str(tmp_path / "raw.npz"), prepare="host")
    assert x.dtype == np.float32 and x.shape == (2, gold.T, 112, 112, 3)
