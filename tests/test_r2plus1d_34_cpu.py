"""R(2+1)D-34 on the host side (no GPU): the 34-layer table against a hand-written expectation of the upstream network
(moabitcoin/ig65m-pytorch models.py), the (base_model, sample_length, num_classes) resolver against the reference's MODELS table
(utils_cv/action_recognition/model.py:46-56, 373, 418-441), and the state_dict loader on 34-layer checkpoints."""
import numpy as np
import pytest
import torch

from flickering_adversarial_video_amd import videoresnet_spec as vs


def test_r2plus1d_34_table():
    t = vs.conv_table("r2plus1d_34")
    shapes = {pre: (co, ci, *k) for pre, co, ci, k, _ in t}
    assert len(t) == len(shapes) == 2 + 4 * (3 + 4 + 6 + 3) + 3 == 69
    assert shapes["stem.0"] == (45, 3, 1, 7, 7) and shapes["stem.3"] == (64, 45, 3, 1, 1)
    assert shapes["layer2.0.conv1.0.0"] == (230, 64, 1, 3, 3)          # torchvision's formula
    assert shapes["layer2.0.conv2.0.0"] == (288, 128, 1, 3, 3)         # the Caffe2 midplanes
    assert shapes["layer3.0.conv2.0.0"] == (576, 256, 1, 3, 3)
    assert shapes["layer4.0.conv2.0.0"] == (1152, 512, 1, 3, 3)
    assert shapes["layer4.0.conv2.0.3"] == (512, 1152, 3, 1, 1)
    assert shapes["layer3.0.conv1.0.0"] == (460, 128, 1, 3, 3) and shapes["layer4.0.conv1.0.0"] == (921, 256, 1, 3, 3)
    assert shapes["layer1.2.conv2.0.0"] == (144, 64, 1, 3, 3) and shapes["layer3.5.conv1.0.3"] == (256, 576, 3, 1, 1)
    blocks = sorted({pre.rsplit(".", 3)[0] if "conv" in pre else pre.rsplit(".", 2)[0] for pre in shapes if pre.startswith("layer")})
    assert blocks == sorted(f"layer{li}.{bi}" for li, n in zip(range(1, 5), (3, 4, 6, 3)) for bi in range(n))
    assert sorted(p for p in shapes if "downsample" in p) == ["layer2.0.downsample.0", "layer3.0.downsample.0", "layer4.0.downsample.0"]
    assert "layer5.0.conv1.0.0" not in shapes and "layer1.3.conv1.0.0" not in shapes and "layer4.3.conv1.0.0" not in shapes
    # the 18-layer tables are untouched
    assert len(vs.conv_table("r2plus1d_18")) == 37 and len(vs.conv_table("r3d_18")) == 20 and len(vs.conv_table("mc3_18")) == 20


REFERENCE_MODELS = {"r2plus1d_34_32_ig65m": 359, "r2plus1d_34_32_kinetics": 400, "r2plus1d_34_8_ig65m": 487, "r2plus1d_34_8_kinetics": 400,
                    "mc3_18": 400, "r2plus1d_18": 400, "r3d_18": 400}


def test_resolver_matches_reference_models():
    for base in ("ig65m", "kinetics"):
        for T in (8, 32):
            name = f"r2plus1d_34_{T}_{base}"
            assert vs.resolve_model(base, T) == ("r2plus1d_34", name, REFERENCE_MODELS[name])
            assert vs.resolve_model(base, T, 51) == ("r2plus1d_34", name, 51)           # a replaced fc head
    for name, n in REFERENCE_MODELS.items():
        arch = "r2plus1d_34" if name.startswith("r2plus1d_34") else name
        assert vs.resolve_model(name, 16) == (arch, name, n)
        assert arch in vs.ARCHS
    for T in (1, 4, 16, 64, None):
        with pytest.raises(ValueError):
            vs.resolve_model("ig65m", T)
        with pytest.raises(ValueError):
            vs.resolve_model("kinetics", T)
    with pytest.raises(ValueError):
        vs.resolve_model("r2plus1d_50", 8)


def test_load_weights_34_layer_state_dict(tmp_path):
    W = vs.synthetic_weights("r2plus1d_34", 3, num_classes=359)
    sd = {"module." + k: torch.from_numpy(v) for k, v in W.items()}
    sd["module.stem.1.num_batches_tracked"] = torch.tensor(0)
    torch.save(sd, tmp_path / "r2plus1d_34_32_ig65m.pth")
    got = vs.load_weights(tmp_path / "r2plus1d_34_32_ig65m.pth", "r2plus1d_34")
    assert set(got) == set(W) and got["fc.weight"].shape == (359, 512) and got["fc.bias"].shape == (359,)
    assert all(np.array_equal(got[k], W[k]) for k in W)
    # the same checkpoint is not an 18-layer one
    with pytest.raises(ValueError):
        vs.load_weights(tmp_path / "r2plus1d_34_32_ig65m.pth", "r2plus1d_18")


def test_load_weights_refuses_formula_midplanes(tmp_path):
    """torchvision's own 34-layer shapes (230 midplanes in layer2.0.conv2) are not the IG65M / Kinetics checkpoints'"""
    W = vs.synthetic_weights("r2plus1d_34", 3, num_classes=400)
    rng = np.random.default_rng(0)
    W["layer2.0.conv2.0.0.weight"] = rng.standard_normal((230, 128, 1, 3, 3)).astype(np.float32)
    W["layer2.0.conv2.0.3.weight"] = rng.standard_normal((128, 230, 3, 1, 1)).astype(np.float32)
    for s in (".weight", ".bias", ".running_mean", ".running_var"):
        W["layer2.0.conv2.0.1" + s] = np.ones(230, np.float32)
    torch.save({k: torch.from_numpy(v) for k, v in W.items()}, tmp_path / "formula.pth")
    with pytest.raises(ValueError, match="layer2.0.conv2"):
        vs.load_weights(tmp_path / "formula.pth", "r2plus1d_34")
