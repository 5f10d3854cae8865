"""The quantised uint8 stem, host side (no GPU): i3d_spec.quantised_stem_bytes is the encode of the float restatement of
clip(x + p, -1, 1); what the bytes decode to is k/128 with |k| <= 128 -- eight significant bits, exact in bf16 (the argument the stem's
QUANT instantiation rests on); the QUANTISE_TRAIN key of run_config.yml."""
import os

import numpy as np
import pytest
import torch

from flickering_adversarial_video_amd import config as cfgmod, i3d_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def float_restatement(xu, delta, *, dclip, adv_flag, shift_x, shift_p, dclip_dev=None):
    """clip(x' + p', -1, 1) written out frame by frame with explicit indices (no np.roll): float32, one rounding per operation"""
    B, T = xu.shape[:2]
    d = np.asarray(delta, F32).reshape(-1, T, 3)
    out = np.empty(xu.shape, F32)
    for b in range(B):
        bound = F32(dclip_dev[b]) if dclip_dev is not None else F32(dclip)
        for t in range(T):
            x = xu[b, (t - shift_x) % T].astype(F32) * F32(1.0 / 128.0) + F32(-1.0)
            row = d[b if d.shape[0] > 1 else 0, (t - shift_p) % T]
            if bound > 0:
                row = np.minimum(np.maximum(row, -bound), bound)
            p = F32(adv_flag) * row if adv_flag != 0 else np.zeros(3, F32)
            out[b, t] = np.minimum(np.maximum((x + p).astype(F32), F32(-1.0)), F32(1.0))
    return out


CASES = {
    "shared": dict(B=1, T=6, kw=dict(dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0)),
    "rolled": dict(B=1, T=8, kw=dict(dclip=0.4, adv_flag=1.0, shift_x=-3, shift_p=13)),
    "half_flag": dict(B=1, T=4, kw=dict(dclip=0.4, adv_flag=0.5, shift_x=0, shift_p=0)),
    "no_dclip": dict(B=1, T=4, kw=dict(dclip=0.0, adv_flag=1.0, shift_x=0, shift_p=0)),
    "per_clip": dict(B=2, T=4, per_clip=True, dclip_dev=(0.4, 0.05), kw=dict(dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0)),
    "clean": dict(B=1, T=4, kw=dict(dclip=0.4, adv_flag=0.0, shift_x=0, shift_p=0)),
}


def fixture(name, hw=24):
    c = CASES[name]
    B, T = c["B"], c["T"]
    rng = np.random.default_rng(500 + sorted(CASES).index(name))
    xu = rng.integers(0, 256, (B, T, hw, hw, 3), dtype=np.uint8)
    delta = rng.uniform(-0.6, 0.6, (B, T, 3) if c.get("per_clip") else (T, 3)).astype(F32)
    delta.reshape(-1, 3)[0] = (3.0 / 256.0, -5.0 / 256.0, 1e-3)            # two rounding ties and a sub-level entry
    dev = np.asarray(c["dclip_dev"], F32) if "dclip_dev" in c else None
    return xu, delta, dev, dict(c["kw"])


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_are_the_encode_of_the_float_restatement(name):
    xu, delta, dev, kw = fixture(name)
    got = i3d_spec.quantised_stem_bytes(xu, delta, dclip_dev=dev, **kw)
    want = i3d_spec.encode_u8(float_restatement(xu, delta, dclip_dev=dev, **kw))
    assert got.dtype == np.uint8 and got.shape == xu.shape
    assert np.array_equal(got, want)
    if kw["adv_flag"] == 0:
        assert np.array_equal(got, np.roll(xu, kw["shift_x"], axis=1))       # the clean clip is its own stored form
    else:
        changed = float((got != np.roll(xu, kw["shift_x"], axis=1)).mean())
        assert 0.10 <= changed <= 0.999, changed


def test_ties_round_half_to_even_and_saturate():
    # x + p = (k + 1/2) / 128 exactly: delta an odd multiple of 1/256 puts every pixel of the (frame, channel) on a tie
    xu = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16, 1).repeat(2, 1).repeat(3, 4)
    delta = np.array([[3.0 / 256.0, -3.0 / 256.0, 1.0 / 256.0], [0.0, 0.0, 0.0]], F32)
    q = i3d_spec.quantised_stem_bytes(xu, delta, dclip=0.4, adv_flag=1.0, shift_x=0, shift_p=0).astype(np.int64)
    k = np.arange(256).reshape(16, 16)
    for c, half in enumerate((1.5, -1.5, 0.5)):
        want = np.clip(np.rint(np.clip(k + half, 0, 256)), 0, 255)          # np.rint: half to even; 256 has no byte
        assert np.array_equal(q[0, 0, :, :, c], want.astype(np.int64)), c
        assert np.all(q[0, 0, :, :, c][(k + half > 0) & (k + half < 255)] % 2 == 0)    # every tie went to the even level
    assert np.array_equal(q[0, 1], xu[0, 1].astype(np.int64))                # delta = 0: the source bytes


def test_every_decoded_value_is_exact_in_bf16():
    q = np.arange(256, dtype=np.uint8)
    v = q.astype(F32) * F32(1.0 / 128.0) + F32(-1.0)                          # the decode the stem applies to the stored byte
    k = v.astype(np.float64) * 128
    assert np.array_equal(k, np.rint(k)) and np.array_equal(k, q.astype(np.float64) - 128) and float(np.abs(k).max()) <= 128
    t = torch.from_numpy(v)
    assert torch.equal(t.bfloat16().float(), t)                               # the round trip through bf16 changes nothing
    # ... and it is the TF table of the generic quantised apply
    from flickering_adversarial_video_amd import ops
    assert np.array_equal(ops.quant_table_host("tf"), np.repeat(v[:, None], 3, axis=1))
    # the bytes of a perturbed clip decode to such values only
    xu, delta, dev, kw = fixture("shared")
    vq = i3d_spec.quantised_stem_bytes(xu, delta, **kw).astype(F32) * F32(1.0 / 128.0) + F32(-1.0)
    tq = torch.from_numpy(vq)
    assert torch.equal(tq.bfloat16().float(), tq) and float(np.abs(vq * 128).max()) <= 128


def test_quantise_train_config_key(tmp_path):
    shipped = cfgmod.load_config(os.path.join(ROOT, "run_config.yml"))
    for sec in cfgmod.ATTACK_SECTIONS:
        assert shipped[sec].QUANTISE_TRAIN is False and "EVAL_QUANTISED" in shipped[sec]
    assert cfgmod.DEFAULT_ATTACK["QUANTISE_TRAIN"] is False
    base = "DATA:\n    LABEL_MAP_PATH: 'x'\nSINGLE_VIDEO_ATTACK:\n    BETA_1: 0.1\n"
    p = tmp_path / "c.yml"
    p.write_text(base)
    assert cfgmod.load_config(str(p)).SINGLE_VIDEO_ATTACK.QUANTISE_TRAIN is False            # absent: off
    p.write_text(base + "    QUANTISE_TRAIN: True\n")
    assert cfgmod.load_config(str(p)).SINGLE_VIDEO_ATTACK.QUANTISE_TRAIN is True
    for bad in ("'tf'", "1", "'yes'"):
        p.write_text(base + f"    QUANTISE_TRAIN: {bad}\n")
        with pytest.raises(ValueError, match="QUANTISE_TRAIN"):
            cfgmod.load_config(str(p))


def test_dense_engine_refuses_quantise_train_before_it_needs_a_device():
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D, FlickerI3DInference
    import inspect
    for cls in (FlickerI3D, FlickerI3DInference):
        assert inspect.signature(cls.__init__).parameters["quantise_train"].default is False
        with pytest.raises(ValueError, match="quantise_train"):
            cls({}, dense_delta=True, quantise_train=True)
