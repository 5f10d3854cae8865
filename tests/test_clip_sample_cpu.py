"""Temporal sampling on the host (videoresnet_spec.sample_frame_indices) against index tables recorded from the reference's own
``VideoDataset._sample_indices`` / ``_get_frames`` (tests/golden/clip_sample_golden.npz, written by tests/golden/make_sample_golden.py).
No GPU."""
import os
import sys

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_sample_golden import FIELDS, load_cases  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return load_cases()


def _kwargs(c):
    return {f: c[f] for f in FIELDS if f != "seed"}


def test_fixture_covers_what_it_should(cases):
    assert len(cases) >= 300
    assert {c["sample_step"] for c in cases} >= {1, 2, 4}
    assert {c["num_samples"] for c in cases} >= {1, 3, 10}
    assert {(c["temporal_jitter"], c["random_shift"]) for c in cases} == {(a, b) for a in (False, True) for b in (False, True)}
    rel = {np.sign(c["num_frames"] - c["presample_length"]) for c in cases}
    assert rel == {-1, 0, 1}
    assert any(c["num_frames"] == c["presample_length"] + 1 for c in cases)
    assert any(c["num_frames"] > 9 * c["presample_length"] for c in cases)
    assert any(c["num_frames"] == 1 for c in cases)
    # the train split: a jitter step of 2 with presample_length left at sample_length
    assert any(c["sample_step"] == 2 and c["presample_length"] == c["sample_length"] and c["temporal_jitter"] for c in cases)


def test_tables_and_generator_state_match_the_reference(cases):
    for c in cases:
        rng = np.random.RandomState(c["seed"])
        got = vs.sample_frame_indices(rng=rng, **_kwargs(c))
        assert got.dtype == np.int64 and got.shape == (c["num_samples"], c["sample_length"]), c
        assert np.array_equal(got, c["table"]), (c, got.tolist())
        assert rng.random_sample() == c["next"], {f: c[f] for f in FIELDS}          # the same number of draws, in the same order


def test_indices_within_range(cases):
    for c in cases:
        got = vs.sample_frame_indices(rng=np.random.RandomState(c["seed"] + 7), **_kwargs(c))
        assert got.min() >= 0 and got.max() < c["num_frames"], c
        assert (np.diff(got, axis=1) >= 0).all(), c
    rng = np.random.RandomState(3)
    for _ in range(200):
        N, T, step, S = int(rng.randint(1, 300)), int(rng.randint(1, 33)), int(rng.randint(1, 5)), int(rng.randint(1, 11))
        got = vs.sample_frame_indices(N, T, step, S, bool(rng.randint(2)), bool(rng.randint(2)), rng=rng)
        assert got.shape == (S, T) and got.min() >= 0 and got.max() < N


def test_presample_length_defaults_to_length_times_step():
    a = vs.sample_frame_indices(100, 8, 2, 3, rng=np.random.RandomState(0))
    b = vs.sample_frame_indices(100, 8, 2, 3, presample_length=16, rng=np.random.RandomState(0))
    assert np.array_equal(a, b)
    # uniform offsets int(d/2 + d*x), d = (100 - 16 + 1) / 3
    d = 85 / 3
    assert a[:, 0].tolist() == [int(d / 2 + d * x) for x in range(3)]
    assert np.array_equal(a[0], a[0, 0] + 2 * np.arange(8))


def test_bad_sampler_arguments_raise():
    for kw in (dict(num_frames=0, sample_length=8), dict(num_frames=10, sample_length=0), dict(num_frames=10, sample_length=8, sample_step=0),
               dict(num_frames=10, sample_length=8, num_samples=0), dict(num_frames=10, sample_length=8, presample_length=0)):
        with pytest.raises(ValueError):
            vs.sample_frame_indices(**kw)


def test_split_sampling_is_the_references_train_test_split(cases):
    s = {"sample_step": 1, "temporal_jitter": True, "temporal_jitter_step": 2, "random_shift": True}
    tr, te = vs.split_sampling(s, 8, train=True), vs.split_sampling(s, 8, train=False)
    assert tr == dict(sample_length=8, sample_step=2, temporal_jitter=True, random_shift=True, presample_length=8)
    assert te == dict(sample_length=8, sample_step=1, temporal_jitter=False, random_shift=False, presample_length=8)
    s = {"sample_step": 2}
    assert vs.split_sampling(s, 16, train=True) == dict(sample_length=16, sample_step=2, temporal_jitter=False, random_shift=False, presample_length=32)
    # a recorded train-split case through the helper
    c = next(c for c in cases if c["sample_step"] == 2 and c["presample_length"] == c["sample_length"] == 8 and c["random_shift"] and c["num_frames"] == 300
             and c["num_samples"] == 3)
    kw = vs.split_sampling({"temporal_jitter": True, "random_shift": True}, 8, train=True)
    got = vs.sample_frame_indices(300, num_samples=3, rng=np.random.RandomState(c["seed"]), **kw)
    assert np.array_equal(got, c["table"])


def test_defaults_are_the_reference_scripts_settings():
    assert vs.check_sampling(None) == {"sample_step": 1, "temporal_jitter": False, "temporal_jitter_step": 2, "random_shift": False, "seed": 0}
    assert vs.check_sampling({"seed": 5})["seed"] == 5


@pytest.mark.parametrize("bad", [
    [1, 2], "step", {"step": 2}, {"sample_step": 0}, {"sample_step": 1.5}, {"sample_step": True}, {"temporal_jitter_step": -1},
    {"temporal_jitter": 1}, {"random_shift": "yes"}, {"seed": -1}, {"seed": 1.0}, {"seed": 2 ** 32}, {"seed": None},
])
def test_malformed_sampling_dicts_raise(bad):
    with pytest.raises(ValueError):
        vs.check_sampling(bad)
