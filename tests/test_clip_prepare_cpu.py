"""Clip preparation without a GPU: the host geometry (videoresnet_spec.prepare_geometry) against the sizes the reference's own transform
produced (tests/golden/clip_prepare_golden.npz), the host A/B route (videoresnet_spec.prepare_host, the scripts' ``--prepare host``)
against the fixture bit for bit, and flk_clip_prepare's argument validation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_prepare_golden as gold  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return gold.load_cases()


def test_fixture_covers_the_sizes(cases):
    assert sorted({(c["H"], c["W"]) for c in cases}) == sorted(gold.SIZES) and len(cases) == 2 * len(gold.SIZES)
    assert {c["kind"] for c in cases} == {"noise", "ramp"}
    assert all(c["out"].shape == (gold.T, 112, 112, 3) and c["out"].dtype == np.float32 for c in cases)


def test_prepare_geometry_matches_the_reference_sizes(cases):
    """resized sizes as the reference's ResizeVideo produced them, crop offsets by Python's round -- for every size and both rules"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    for c in cases:
        for rule in vs.RESIZE_RULES:
            Hr, Wr, sh, sw, ci, cj = vs.prepare_geometry(c["H"], c["W"], rule=rule)
            assert (Hr, Wr) == (c["Hr"], c["Wr"]), c["name"]
            assert (ci, cj) == (int(round((Hr - 112) / 2.0)), int(round((Wr - 112) / 2.0)))
            scale = 128 / min(c["H"], c["W"])
            want = (np.float32(c["H"]) / np.float32(Hr), np.float32(c["W"]) / np.float32(Wr)) if rule == "sizes" else (np.float32(1.0 / scale),) * 2
            assert (np.float32(sh), np.float32(sw)) == want and sh == float(want[0]) and sw == float(want[1])
    # the spelled-out cases: 4:3 at 240 lines; portrait; the half-way crop offset 29.5 -> 30 (round half to even: 30, not 29.5 -> 29)
    assert vs.prepare_geometry(240, 320)[:2] + vs.prepare_geometry(240, 320)[4:] == (128, 170, 8, 29)
    assert vs.prepare_geometry(480, 270)[:2] + vs.prepare_geometry(480, 270)[4:] == (227, 128, 58, 8)       # 57.5 -> 58
    assert vs.prepare_geometry(128, 171)[:2] + vs.prepare_geometry(128, 171)[4:] == (128, 171, 8, 30)       # 29.5 -> 30
    assert vs.prepare_geometry(130, 171, im_scale=130, input_size=113)[4:] == (8, 29)                        # 8.5 -> 8, 29.0
    assert vs.prepare_geometry(239, 317)[:2] == (127, 169)                                                   # 239 * (128 / 239) < 128 in doubles
    # the two rules agree where in * scale is an integer, and only there
    for H, W, same in ((256, 340, True), (128, 171, True), (240, 320, False), (239, 317, False)):
        assert (vs.prepare_geometry(H, W, rule="sizes") == vs.prepare_geometry(H, W, rule="scale_factor")) == same


def test_prepare_geometry_refuses_a_resized_image_smaller_than_the_crop():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    with pytest.raises(ValueError):
        vs.prepare_geometry(240, 320, im_scale=100, input_size=112)         # 100 x 133 < 112
    with pytest.raises(ValueError):
        vs.prepare_geometry(480, 270, im_scale=128, input_size=(112, 130))  # 227 x 128: too narrow
    with pytest.raises(ValueError):
        vs.prepare_geometry(240, 320, rule="nearest")
    assert vs.prepare_geometry(240, 320, im_scale=112, input_size=112)[:2] == (112, 149)


def test_host_route_reproduces_the_fixture_bitwise(cases):
    """``--prepare host`` with --resize-rule scale_factor is the reference's four torch calls: anything but equal bits is a wiring error"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    for c in cases:
        got = vs.prepare_host(c["frames"], rule="scale_factor")
        assert got.dtype == torch.float32 and tuple(got.shape) == c["out"].shape
        assert np.array_equal(got.numpy().view(np.uint32), c["out"].view(np.uint32)), c["name"]


def test_host_route_sizes_rule_is_interpolate_with_sizes(cases):
    """rule="sizes": F.interpolate(size=(Hr, Wr)) between the /255 and the normalisation (torch, not reference text); equal to the other
    rule exactly where the steps coincide"""
    import torch.nn.functional as F
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    for c in cases:
        x = torch.from_numpy(c["frames"])
        v = F.interpolate(x.float().permute(3, 0, 1, 2) / 255.0, size=(c["Hr"], c["Wr"]), mode="bilinear", align_corners=False)
        i, j = int(round((c["Hr"] - 112) / 2.0)), int(round((c["Wr"] - 112) / 2.0))
        v = v[..., i:i + 112, j:j + 112].clone()
        v.sub_(torch.tensor(vs.DEFAULT_MEAN)[:, None, None, None]).div_(torch.tensor(vs.DEFAULT_STD)[:, None, None, None])
        got = vs.prepare_host(c["frames"], rule="sizes")
        assert torch.equal(got, v.permute(1, 2, 3, 0))
        if (c["H"], c["W"]) in ((256, 340), (128, 171)):
            assert np.array_equal(got.numpy(), c["out"]), c["name"]


def test_script_host_route_is_the_package_route(tmp_path, cases):
    """the scripts' --prepare host: per clip videoresnet_spec.prepare_host, stacked"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import r2plus1d_main_universal_attack as uni
    c = next(c for c in cases if c["name"] == "240x320_noise")
    clips = np.stack([c["frames"], c["frames"][:, ::-1]])                     # [2,T,240,320,3]
    assert uni.engine_size(clips) == (112, True) and uni.engine_size(clips, image_size=240) == (240, True)
    assert uni.engine_size(np.zeros((1, 2, 64, 64, 3), np.uint8)) == (64, False)             # square clips: the engine takes their size, as before
    assert uni.engine_size(np.zeros((1, 2, 64, 64, 3), np.uint8), prepare="device") == (112, True)
    assert uni.engine_size(np.zeros((1, 2, 240, 320, 3), np.float32)) == (240, False)        # float32 files are normalised clips already
    np.savez(tmp_path / "raw.npz", clips=clips, labels=np.array([1, 2]))
    x, y = uni.load_clips(str(tmp_path / "raw.npz"), prepare="host", rule="scale_factor")
    assert x.dtype == np.float32 and x.shape == (2, gold.T, 112, 112, 3) and np.array_equal(x[0], c["out"]) and list(y) == [1, 2]
    xr, _ = uni.load_clips(str(tmp_path / "raw.npz"))                           # default: the raw frames stay uint8 for the device route
    assert xr.dtype == np.uint8 and xr.shape == clips.shape


def _valid_args():
    from flickering_adversarial_video_amd import _lib, videoresnet_spec as vs
    clip = _lib.PrepClip()
    clip.src, clip.T, clip.Hs, clip.Ws, clip.pitch_t, clip.pitch_h = 64, 2, 240, 320, 240 * 320 * 3, 320 * 3
    clip.Hr, clip.Wr, clip.step_h, clip.step_w, clip.crop_i, clip.crop_j = vs.prepare_geometry(240, 320)
    arr = (_lib.PrepClip * 1)(clip)
    a = _lib.PrepareArgs()
    a.nclip, a.Ho, a.Wo = 1, 112, 112
    a.mean, a.std = (C.c_float * 3)(*vs.DEFAULT_MEAN), (C.c_float * 3)(*vs.DEFAULT_STD)
    a.out_clip_offset, a.out_clip_stride = 0, 2 * 112 * 112 * 3
    a.clips = arr
    return a, arr


def test_argument_validation_without_gpu():
    """every invalid argument is FLK_EINVAL with a message, decided on the host before any GPU call (there is no GPU here)"""
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    out = C.c_void_p(64)

    def rc(mut=None, a_null=False, out_null=False):
        a, arr = _valid_args()
        if mut:
            mut(a, arr[0])
        return lib.flk_clip_prepare(None if a_null else C.byref(a), None if out_null else out, None)

    assert rc(a_null=True) == -1 and b"null" in lib.flk_last_error()
    assert rc(out_null=True) == -1 and b"null" in lib.flk_last_error()
    assert rc(lambda a, c: setattr(a, "clips", C.POINTER(_lib.PrepClip)())) == -1 and b"null" in lib.flk_last_error()
    assert rc(lambda a, c: setattr(c, "src", None)) == -1 and b"null" in lib.flk_last_error()
    for n in (0, -1, _lib.FLK_PREP_MAX_CLIPS + 1):
        assert rc(lambda a, c: setattr(a, "nclip", n)) == -1 and b"nclip" in lib.flk_last_error()
    for field in ("T", "Hs", "Ws", "Hr", "Wr", "pitch_t", "pitch_h"):
        for bad in (0, -3):
            assert rc(lambda a, c: setattr(c, field, bad)) == -1, field
    assert rc(lambda a, c: setattr(c, "pitch_h", 320 * 3 - 1)) == -1 and b"pitch" in lib.flk_last_error()
    for field in ("Ho", "Wo"):
        assert rc(lambda a, c: setattr(a, field, 0)) == -1 and b"output size" in lib.flk_last_error()
    for field in ("step_h", "step_w"):
        for bad in (0.0, -1.875, float("nan"), float("inf")):
            assert rc(lambda a, c: setattr(c, field, bad)) == -1 and b"step" in lib.flk_last_error(), (field, bad)
    for field, bad in (("crop_i", -1), ("crop_j", -1), ("crop_i", 128 - 112 + 1), ("crop_j", 170 - 112 + 1)):
        assert rc(lambda a, c: setattr(c, field, bad)) == -1 and b"crop window" in lib.flk_last_error(), (field, bad)
    assert rc(lambda a, c: setattr(c, "Hr", 111)) == -1 and b"crop window" in lib.flk_last_error()
    for k in range(3):
        for bad in (0.0, -0.2, float("nan")):
            def mut(a, c, k=k, bad=bad):
                a.std[k] = bad
            assert rc(mut) == -1 and b"std" in lib.flk_last_error()
    assert rc(lambda a, c: setattr(a, "out_clip_stride", 2 * 112 * 112 * 3 - 1)) == -1 and b"out_clip_stride" in lib.flk_last_error()
    assert rc(lambda a, c: setattr(a, "out_clip_offset", -1)) == -1


def test_prepare_source_is_not_an_inline_asm_load_source():
    from flickering_adversarial_video_amd import build
    assert "prepare.hip" in build.SOURCES and "prepare.hip" not in build.ASM_LOAD_SOURCES
