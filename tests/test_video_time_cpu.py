"""Flicker on video time, the host side: the rule that gives every frame its row (videoresnet_spec.flicker_rows) against tables written
out by hand and against the whole-video export's own wording, the engine constructor's refusals (raised before anything touches a
device), and the two new entry points in the header, the built library and the ctypes table alike."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(*a, **kw):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    return vs.flicker_rows(*a, **kw)


def test_consecutive_frames_are_a_roll_of_the_period():
    """T = P = 8: a clip cut at offset o carries the rows rolled by o mod 8"""
    assert rows(np.arange(0, 8), 8).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert rows(np.arange(13, 21), 8).tolist() == [5, 6, 7, 0, 1, 2, 3, 4]
    assert rows(np.arange(29, 37), 8).tolist() == [5, 6, 7, 0, 1, 2, 3, 4]
    assert rows(np.arange(16, 24), 8).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    table = np.stack([np.arange(0, 8), np.arange(13, 21), np.arange(29, 37)])
    assert rows(table, 8).tolist() == [[0, 1, 2, 3, 4, 5, 6, 7], [5, 6, 7, 0, 1, 2, 3, 4], [5, 6, 7, 0, 1, 2, 3, 4]]


def test_period_independent_of_the_clip_length():
    """T = 8 frames under a shorter and a longer period: rows repeat inside the clip (P = 5) or some are never carried (P = 12)"""
    assert rows(np.arange(13, 21), 5).tolist() == [3, 4, 0, 1, 2, 3, 4, 0]
    assert rows(np.arange(0, 8), 5).tolist() == [0, 1, 2, 3, 4, 0, 1, 2]
    assert rows(np.arange(13, 21), 12).tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert rows(np.arange(7, 15), 12).tolist() == [7, 8, 9, 10, 11, 0, 1, 2]


def test_sample_step_jitter_and_padding_are_no_roll():
    # sample_step = 3 from frame 2: 2, 5, 8, ... -- under P = 8 not a roll of 0..7
    assert rows(2 + 3 * np.arange(8), 8).tolist() == [2, 5, 0, 3, 6, 1, 4, 7]
    assert rows(2 + 3 * np.arange(8), 5).tolist() == [2, 0, 3, 1, 4, 2, 0, 3]
    # temporal jitter: steps of 0 repeat a frame, and with it its row
    assert rows(np.array([4, 4, 6, 7, 7, 7, 9, 11]), 8).tolist() == [4, 4, 6, 7, 7, 7, 1, 3]
    # a video of 5 frames padded to a clip of 8 with its last frame
    assert rows(np.array([0, 1, 2, 3, 4, 4, 4, 4]), 8).tolist() == [0, 1, 2, 3, 4, 4, 4, 4]
    assert rows(np.array([0, 1, 2, 3, 4, 4, 4, 4]), 3).tolist() == [0, 1, 2, 0, 1, 1, 1, 1]


def test_phases_of_any_sign_and_per_clip():
    n = np.arange(13, 21)
    assert rows(n, 8, 3).tolist() == [2, 3, 4, 5, 6, 7, 0, 1]
    assert rows(n, 8, -3).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]            # (13 + 3) mod 8 = 0
    assert rows(n, 8, 19).tolist() == rows(n, 8, 3).tolist()              # a phase beyond the period is the phase mod the period
    assert rows(n, 8, -13).tolist() == rows(n, 8, 3).tolist()
    assert rows(np.arange(0, 8), 5, 7).tolist() == [3, 4, 0, 1, 2, 3, 4, 0]
    assert rows(np.arange(0, 3), 5, -100).tolist() == [0, 1, 2]
    table = np.stack([np.arange(0, 8), np.arange(13, 21)])
    got = rows(table, 8, np.array([2, -3]))
    assert got.tolist() == [[6, 7, 0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6, 7]]
    with pytest.raises(ValueError, match="one per clip"):
        rows(table, 8, np.array([1, 2, 3]))
    with pytest.raises(ValueError, match="period"):
        rows(table, 0)
    with pytest.raises(ValueError, match="integers"):
        rows(table.astype(np.float32), 8)


def test_dtype_and_range():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    rng = np.random.RandomState(3)
    for P in (1, 5, 8, 12, 682):
        for kw in (dict(sample_step=1), dict(sample_step=3), dict(sample_step=2, temporal_jitter=True, random_shift=True)):
            table = vs.sample_frame_indices(37, 8, num_samples=4, rng=rng, **kw)
            for phase in (0, 5, -7, 1000, np.array([0, -1, 3, 700])):
                r = vs.flicker_rows(table, P, phase)
                assert r.dtype == np.int32 and r.shape == table.shape and r.min() >= 0 and r.max() < P
    assert vs.flicker_rows(np.int32(9), 4).shape == () and int(vs.flicker_rows(np.int32(9), 4)) == 1


@pytest.mark.parametrize("P,phase", [(8, 0), (5, 3), (12, -5), (7, 40), (1, 2)])
def test_agrees_with_the_export_rule(P, phase):
    """flk_adv_export_u8 with delta_T = P and shift_p = phase: "frame t takes row (t - shift_p) mod delta_T" -- the mathematical mod,
    0 <= row < P, written here without numpy's own mod; the same table is what ops.export_adversarial_u8_host indexes with"""
    for n in range(40):
        want = n - phase
        while want < 0:
            want += P
        while want >= P:
            want -= P
        assert int(rows(np.int64(n), P, phase)) == want
    assert rows(np.arange(40), P, phase).tolist() == ((np.arange(40) - phase) % P).tolist()
    hdr = open(os.path.join(ROOT, "include", "flicker_hip.h")).read()
    assert "frame t takes row (t - shift_p) mod delta_T" in hdr
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    assert "shift_p = phase" in vs.flicker_rows.__doc__ and "delta_T = period" in vs.flicker_rows.__doc__


def test_constructor_refusals_touch_no_device():
    """every refusal names its reason and comes before the weights are looked at or a device is asked for (weights = None would fail there)"""
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, check_flicker_time
    kw = dict(batch_size=2, sample_length=8, image_size=64)
    with pytest.raises(ValueError, match="flicker_time must be one of"):
        FlickerVideoResNet("r3d_18", None, flicker_time="frame", **kw)
    with pytest.raises(ValueError, match="flicker_period needs flicker_time='video'"):
        FlickerVideoResNet("r3d_18", None, flicker_period=5, **kw)
    for bad in (0, 683, -1, 2.5, True):
        with pytest.raises(ValueError, match="flicker_period must be an integer in 1..682"):
            FlickerVideoResNet("r3d_18", None, flicker_time="video", flicker_period=bad, **kw)
    with pytest.raises(ValueError, match="one shared perturbation only"):
        FlickerVideoResNet("r3d_18", None, flicker_time="video", attack_type="L12", **kw)
    with pytest.raises(ValueError, match="one shared perturbation only"):
        FlickerVideoResNet("r3d_18", None, flicker_time="video", per_clip=True, **kw)
    assert check_flicker_time("clip", None, 8) == 8 and check_flicker_time("video", None, 8) == 8
    assert check_flicker_time("video", 5, 8) == 5 and check_flicker_time("video", 682, 8) == 682


def test_the_two_entry_points_in_header_library_and_binding():
    import ctypes as C
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flicker_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(flk_[a-z0-9_]+)\s*\(", src))
    for name in ("flk_flicker_rows_gather", "flk_flicker_rows_grad"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    # FLK_EINVAL with a reason, before any GPU call (there is no GPU here): null pointers, n < 1, P outside 1..682
    p = C.c_void_p(8)
    assert lib.flk_flicker_rows_gather(None, 5, p, 4, p, None) == -1 and b"null" in lib.flk_last_error()
    assert lib.flk_flicker_rows_gather(p, 5, None, 4, p, None) == -1 and lib.flk_flicker_rows_gather(p, 5, p, 4, None, None) == -1
    assert lib.flk_flicker_rows_gather(p, 5, p, 0, p, None) == -1 and b"n must be" in lib.flk_last_error()
    assert lib.flk_flicker_rows_gather(p, 0, p, 4, p, None) == -1 and b"period" in lib.flk_last_error()
    assert lib.flk_flicker_rows_gather(p, 683, p, 4, p, None) == -1 and b"period" in lib.flk_last_error()
    assert lib.flk_flicker_rows_grad(None, p, 4, 5, p, None) == -1 and b"null" in lib.flk_last_error()
    assert lib.flk_flicker_rows_grad(p, None, 4, 5, p, None) == -1 and lib.flk_flicker_rows_grad(p, p, 4, 5, None, None) == -1
    assert lib.flk_flicker_rows_grad(p, p, -1, 5, p, None) == -1 and b"n must be" in lib.flk_last_error()
    assert lib.flk_flicker_rows_grad(p, p, 4, 0, p, None) == -1 and lib.flk_flicker_rows_grad(p, p, 4, 683, p, None) == -1
    assert b"period" in lib.flk_last_error()
