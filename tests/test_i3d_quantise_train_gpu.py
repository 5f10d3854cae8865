"""FlickerI3D(quantise_train=True): the I3D engines train and score on the STORED clip (GPU).

Every forward that applies the perturbation sees the 8-bit frames ``adversarial_inputs_u8`` holds, decoded again: in bf16 on a uint8
clip the stem stages the stored byte itself (csrc/stem_fwd.hip, QUANT -- the space-to-depth tensor is not written), on every other plan
or clip the quantised apply feeds the folded stem.  The references are the plain engine on the exported frames (what
``quantised_logits`` has always computed) and, where the perturbation is zero or a whole number of levels inside the value range, the
plain engine itself.  synthetic_i3d_weights, T = 16 (the smallest clip the topology admits), B = 1 and 2, bf16 and f32.

Per-clip trajectories are compared in f32: a batch-2 and a batch-1 bf16 plan differ in launch layout (test_per_clip_gpu.py), in f32 a
clip's arithmetic does not depend on the batch."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16
HP = dict(lr=1e-3, beta0=1.0, beta1=0.5, beta2=0.5, beta3=0.5)


def same_bits(a, b):
    a, b = (t.detach().cpu() for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


@functools.lru_cache(maxsize=None)
def weights():
    from flickering_adversarial_video_amd import i3d_spec
    return i3d_spec.synthetic_i3d_weights(42)


def engine(dtype, B, quant, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    return FlickerI3D(weights(), batch_size=B, frames=T, dtype=dtype, quantise_train=quant, **kw)


@functools.lru_cache(maxsize=None)
def clip(B, lo=0, hi=256):
    return torch.from_numpy(np.random.default_rng(97 + B).integers(lo, hi, (B, T, 224, 224, 3), dtype=np.uint8)).cuda()


def mixed_delta(seed):
    """entries of many levels (some beyond the +-0.4 clamp), a quarter below half a level, one rounding tie"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-0.5, 0.5, (T, 3)).astype(np.float32)
    d.reshape(-1)[rng.permutation(3 * T)[:12]] = rng.uniform(-0.003, 0.003, 12).astype(np.float32)
    d[0, 0] = 3.0 / 256.0
    return d


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_logits_are_those_of_the_exported_frames(dtype, B):
    eq, ep = engine(dtype, B, True), engine(dtype, B, False)
    x = clip(B)
    for e in (eq, ep):
        e.reset_perturbation(mixed_delta(5))
    poison = float("nan")
    for flag, cyclic in ((1.0, 1), (1.0, 0), (0.5, 0)):
        eq._xs2d.fill_(poison)
        lq = eq.logits(x, flag, cyclic).clone()
        sx = eq._last_shifts[0]                                              # the roll eng_q drew
        assert cyclic or sx == 0
        if dtype == "bf16":
            # the in-stem route: the space-to-depth tensor is neither written nor read
            assert bool(torch.isnan(eq._xs2d.float()).all())
        frames = ep._export_u8(x, flag, sx, 0, 0.4)
        share = float((frames != torch.roll(x, sx, 1)).float().mean())
        assert 0.10 <= share <= 0.95, share
        want = ep.logits(frames, 0.0, 0).clone()
        assert same_bits(lq, want), (flag, cyclic)
        assert not same_bits(lq, ep.logits(x, flag, 0))                      # ... which the float clip's logits are not
    # __call__ and a fractional adv_flag go the same way
    assert same_bits(eq(x, adv_flag=1, cyclic=0), torch.softmax(ep.logits(ep._export_u8(x, 1.0, 0, 0, 0.4), 0.0, 0), -1))
    if dtype == "bf16":
        # an fp32 clip takes the quantised apply + the folded stem: the logits of the same frames given as fp32 values
        x32 = x.float() / 128 - 1
        frames = ep._export_u8(x, 1.0, 0, 0, 0.4)
        assert torch.equal(ep._export_u8(x32, 1.0, 0, 0, 0.4), frames)
        eq._xs2d.fill_(poison)
        l32 = eq.logits(x32, 1.0, 0).clone()
        assert not bool(torch.isnan(eq._xs2d.float()).any())
        assert same_bits(l32, ep.logits(frames.float() / 128 - 1, 0.0, 0))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_zero_perturbation_step_is_the_plain_step(dtype, B):
    eq, ep = engine(dtype, B, True), engine(dtype, B, False)
    x = clip(B)
    lab = ep.logits(x, 0.0, 0).argmax(-1).clone()
    rq, rp = eq.step(x, lab, update=False, **HP), ep.step(x, lab, update=False, **HP)
    assert same_bits(rq["softmax"], rp["softmax"]) and same_bits(rq["_argmax_f"], rp["_argmax_f"])
    assert same_bits(eq.delta_gradient(), ep.delta_gradient()) and float(eq.delta_gradient().abs().max()) > 0
    assert torch.equal(rq["argmax"], rp["argmax"]) and same_bits(rq["label_prob"], rp["label_prob"])


@pytest.mark.parametrize("B", [1, 2])
def test_whole_level_perturbation_f32_is_the_plain_engine(B):
    """delta = k/128, clip bytes in 40..215 and |k| <= 30: no clamp is active, x + p is exact and already a level -- quantising changes
    nothing, so the quantised and the plain f32 engines agree bit for bit in logits and delta-gradient"""
    eq, ep = engine("f32", B, True), engine("f32", B, False)
    x = clip(B, 40, 216)
    d = np.random.default_rng(61).integers(-30, 31, (T, 3)).astype(np.float32) / np.float32(128.0)
    assert float(np.abs(d).max()) > 0
    lab = ep.logits(x, 0.0, 0).argmax(-1).clone()
    for e in (eq, ep):
        e.reset_perturbation(d)
        e.step(x, lab, update=False, **HP)
    assert same_bits(eq._logits, ep._logits) and same_bits(eq.delta_gradient(), ep.delta_gradient())
    assert not same_bits(eq._logits, ep.logits(x, 0.0, 0))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_sub_level_perturbation_reaches_no_frame_but_has_a_gradient(dtype):
    eq, ep = engine(dtype, 1, True), engine(dtype, 1, False)
    x = clip(1)
    clean = ep.logits(x, 0.0, 0).clone()
    lab = clean.argmax(-1).clone()
    d = 1e-3 * np.where(np.random.default_rng(59).random((T, 3)) < 0.5, -1.0, 1.0)
    for e in (eq, ep):
        e.reset_perturbation(d)
    eq.step(x, lab, update=False, **HP)
    assert same_bits(eq._logits, clean)                                      # an eighth of a level moves no stored byte
    g = eq.delta_gradient()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0         # ... and the straight-through gradient is there
    assert not same_bits(ep.logits(x, 1.0, 0), clean)                        # the float clip of the plain engine moves the logits


@pytest.mark.parametrize("optimizer", ["adam", "pgd"])
@pytest.mark.parametrize("dtype,B", [("bf16", 1), ("bf16", 2), ("f32", 1)])
def test_twenty_steps_stay_on_the_stored_clip(dtype, B, optimizer):
    eq = engine(dtype, B, True, optimizer=optimizer)
    x = clip(B)
    lab = eq.logits(x, 0.0, 0).argmax(-1).clone()
    lr = 2.0 / 128 if optimizer == "pgd" else 5e-3                           # steps of whole levels: the stored frames move
    for it in range(20):
        before = eq.quantised_logits(x).clone()
        eq.step(x, lab, **dict(HP, lr=lr))
        assert same_bits(eq._logits, before), it                             # the step scored the stored clip, at no extra forward pass
        assert same_bits(eq.logits(x, 1.0), eq.quantised_logits(x)), it
    assert not torch.equal(eq.adversarial_inputs_u8, x)


@pytest.mark.parametrize("optimizer", ["adam", "pgd"])
def test_per_clip_trajectories_are_those_of_single_runs_f32(optimizer):
    B = 2
    eB, e1 = engine("f32", B, True, optimizer=optimizer, per_clip_delta=True), engine("f32", 1, True, optimizer=optimizer)
    x = clip(B)
    lab = eB.logits(x, 0.0).argmax(-1).clone()
    lr = 2.0 / 128 if optimizer == "pgd" else 5e-3
    singles = []
    for b in range(B):
        e1.reset_perturbation()
        tr = []
        for it in range(20):
            e1.step(x[b:b + 1].contiguous(), lab[b:b + 1].contiguous(), **dict(HP, lr=lr))
            tr.append((e1._logits.clone(), e1.delta_gradient().clone(), e1.eps_rgb.clone()))
        singles.append(tr)
    for it in range(20):
        eB.step(x, lab, **dict(HP, lr=lr))
        for b in range(B):
            lg, g, d = singles[b][it]
            assert same_bits(eB._logits[b], lg[0]) and same_bits(eB.delta_gradient()[b], g) and same_bits(eB.eps_rgb[b], d), (it, b)
        assert same_bits(eB.logits(x, 1.0), eB.quantised_logits(x)), it
    assert not torch.equal(eB.adversarial_inputs_u8, x)


def test_dense_is_refused():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D, FlickerI3DInference
    for cls in (FlickerI3D, FlickerI3DInference):
        with pytest.raises(ValueError, match="quantise_train"):
            cls(weights(), batch_size=1, frames=T, dense_delta=True, quantise_train=True)


def test_inference_engine_scores_the_stored_clip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3DInference
    x = clip(1)
    iq = FlickerI3DInference(weights(), batch_size=1, frames=T, dtype="bf16", quantise_train=True)
    ip = FlickerI3DInference(weights(), batch_size=1, frames=T, dtype="bf16")
    for e in (iq, ip):
        e.set_perturbation(mixed_delta(7))
    assert same_bits(iq(x, adv_flag=1), ip(x, adv_flag=1, quantise=True))
    assert not same_bits(iq(x, adv_flag=1), ip(x, adv_flag=1))


# ---- the single-video script ---------------------------------------------------------------------------------------------------------
def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("quantise_train", [True, None], ids=["QUANTISE_TRAIN", "absent"])
def test_single_video_script(tmp_path, quantise_train):
    from flickering_adversarial_video_amd import config as cfgmod, i3d_spec
    c = i3d_spec.synthetic_clip_u8(1, T, seed=71).astype(np.float32) / 128 - 1
    eng = engine("f32", 1, False)
    cls_id = int(eng(torch.from_numpy(c).cuda(), adv_flag=0).argmax())
    (tmp_path / "npy").mkdir()
    (tmp_path / "labels.txt").write_text("\n".join(f"class {i}" for i in range(400)))
    np.save(tmp_path / "npy" / f"rgb_0001@class_{cls_id}.npy", c)
    cfg = open(os.path.join(ROOT, "run_config.yml")).read()
    cfg = cfg.replace("'data/label_map.txt'", f"'{tmp_path}/labels.txt'").replace("NPY_PATH: 'data/videos_for_tests/npy/'", f"NPY_PATH: '{tmp_path}/npy/'", 1)
    cfg = cfg.replace("PKL_RESULT_PATH: 'result/videos_for_tests/npy/'", f"PKL_RESULT_PATH: '{tmp_path}/out/'")
    assert cfg.count("    QUANTISE_TRAIN: False") == 3
    if quantise_train:
        cfg = cfg.replace("QUANTISE_TRAIN: False", "QUANTISE_TRAIN: True", 1).replace("SAVE_ADV_U8: False", "SAVE_ADV_U8: True", 1)
    else:
        cfg = "\n".join(line for line in cfg.split("\n") if "QUANTISE_TRAIN" not in line)       # a config from before the key
    (tmp_path / "cfg.yml").write_text(cfg)
    _run([sys.executable, os.path.join(ROOT, "scripts", "i3d_adversarial_main_single_video_npy.py"), str(tmp_path / "cfg.yml"),
          "--max-steps", "3", "--frames", str(T), "--dtype", "f32"])
    outs = os.listdir(tmp_path / "out")
    assert len(outs) == 1
    res = pickle.load(open(tmp_path / "out" / outs[0], "rb"))
    if not quantise_train:
        assert set(res) == set(cfgmod.RESULT_KEYS)                           # today's keys
        return
    assert set(res) == set(cfgmod.RESULT_KEYS) | {"adv_video_u8", "quantised_pred", "quantised_is_adversarial"}
    final = res["softmax"][-1]                                               # the verification that ended the loop
    assert res["quantised_pred"] == int(final.argmax())
    assert res["quantised_is_adversarial"] == (int(final.argmax()) != cls_id)
    # ... and it IS the verdict on the stored frames: a plain engine on the saved bytes gives that softmax, bit for bit
    frames = torch.from_numpy(res["adv_video_u8"]).cuda()
    assert same_bits(eng(frames, adv_flag=0)[0], torch.from_numpy(final))
