"""Projected sign-gradient (PGD) optimiser: what can be checked without a device -- argument validation of the three entry points
through the C ABI, the OPTIMIZER / PGD_EPS configuration keys, the optimiser keyword of the engines and the checkpoint contents."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _flicker_args(T=16, torch_dialect=0, eps=0.4, dyn=0.0):
    from flickering_adversarial_video_amd import _lib
    a = _lib.AdamArgs()
    a.T, a.torch_dialect, a.beta0, a.beta1, a.beta2, a.beta3 = T, torch_dialect, 1.0, 0.5, 0.5, 0.5
    a.g_scale, a.lr, a.pgd_eps, a.dyn_max_norm = 1.0, 1e-3, eps, dyn
    return a


def test_flicker_entry_points_validate_their_arguments(lib):
    p = C.c_void_p(8)                                   # never dereferenced: validation fails first
    a = _flicker_args()
    assert lib.flk_perturb_reg_pgd(None, p, p, p, None) == -1 and b"null" in lib.flk_last_error()
    assert lib.flk_perturb_reg_pgd(C.byref(a), None, p, p, None) == -1 and b"null" in lib.flk_last_error()
    assert lib.flk_perturb_reg_pgd(C.byref(a), p, None, p, None) == -1 and b"null" in lib.flk_last_error()
    for T in (0, -3, 683):                              # 3*T <= 2048
        assert lib.flk_perturb_reg_pgd(C.byref(_flicker_args(T=T)), p, p, p, None) == -1
        assert b"T out of range" in lib.flk_last_error()
        assert lib.flk_perturb_reg_pgd_batched(C.byref(_flicker_args(T=T)), 2, p, p, p, None, None, p, None) == -1
        assert b"T out of range" in lib.flk_last_error()
    for eps in (0.0, -0.1):                             # TF dialect: pgd_eps is the radius
        assert lib.flk_perturb_reg_pgd(C.byref(_flicker_args(eps=eps)), p, p, p, None) == -1 and b"pgd_eps" in lib.flk_last_error()
        assert lib.flk_perturb_reg_pgd_batched(C.byref(_flicker_args(eps=eps)), 2, p, p, p, None, None, p, None) == -1
        assert b"pgd_eps" in lib.flk_last_error()
    # torch dialect: the clamp bound is the radius (pgd_eps is not looked at)
    assert lib.flk_perturb_reg_pgd(C.byref(_flicker_args(torch_dialect=1, eps=0.4, dyn=0.0)), p, p, p, None) == -1
    assert b"dyn_max_norm" in lib.flk_last_error()
    assert lib.flk_perturb_reg_pgd_batched(C.byref(a), 2, p, p, None, None, None, p, None) == -1 and b"null" in lib.flk_last_error()
    for n in (0, 65536):
        assert lib.flk_perturb_reg_pgd_batched(C.byref(a), n, p, p, p, None, None, p, None) == -1 and b"clip count" in lib.flk_last_error()


def test_dense_entry_point_validates_its_arguments(lib):
    from flickering_adversarial_video_amd import _lib
    p = C.c_void_p(8)

    def args(T=16, H=224, W=224, torch_dialect=0, eps=0.05, dyn=0.0):
        a = _lib.DenseAdamArgs()
        a.T, a.H, a.W, a.torch_dialect, a.beta, a.g_scale, a.lr, a.pgd_eps, a.dyn_max_norm = T, H, W, torch_dialect, 1.0, 1.0, 1e-3, eps, dyn
        return a
    assert lib.flk_perturb_dense_l12_pgd(None, p, p, p, p, None) == -1 and b"null" in lib.flk_last_error()
    assert lib.flk_perturb_dense_l12_pgd(C.byref(args()), p, p, p, None, None) == -1 and b"null" in lib.flk_last_error()
    assert lib.flk_perturb_dense_l12_pgd(C.byref(args(T=1025)), p, p, p, p, None) == -1 and b"bad dims" in lib.flk_last_error()
    assert lib.flk_perturb_dense_l12_pgd(C.byref(args(T=0)), p, p, p, p, None) == -1 and b"bad dims" in lib.flk_last_error()
    assert lib.flk_perturb_dense_l12_pgd(C.byref(args(H=3, W=3)), p, p, p, p, None) == -1 and b"bad dims" in lib.flk_last_error()
    for eps in (0.0, -1.0):                             # the dense TF form has no apply clip: the radius is required
        assert lib.flk_perturb_dense_l12_pgd(C.byref(args(eps=eps)), p, p, p, p, None) == -1
        msg = lib.flk_last_error()
        assert b"flk_perturb_dense_l12_pgd" in msg and b"pgd_eps" in msg and b"positive" in msg
    assert lib.flk_perturb_dense_l12_pgd(C.byref(args(torch_dialect=1, eps=0.05, dyn=0.0)), p, p, p, p, None) == -1
    assert b"dyn_max_norm" in lib.flk_last_error()


def test_argument_structs_keep_their_layout():
    """the radius is a TRAILING field: every field the Adam entry points read keeps its offset"""
    from flickering_adversarial_video_amd import _lib
    assert _lib.AdamArgs.step.offset == 48 and _lib.AdamArgs.pgd_eps.offset == 52 and C.sizeof(_lib.AdamArgs) == 56
    assert _lib.DenseAdamArgs.dyn_max_norm.offset == 44 and _lib.DenseAdamArgs.pgd_eps.offset == 48 and C.sizeof(_lib.DenseAdamArgs) == 52


def test_optimizer_key_defaults_to_adam(tmp_path):
    from flickering_adversarial_video_amd import config as cfgmod
    p = tmp_path / "c.yml"
    p.write_text("DATA:\n    LABEL_MAP_PATH: 'x'\nSINGLE_VIDEO_ATTACK:\n    BETA_1: 0.1\nUNIVERSAL_ATTACK:\n    OPTIMIZER: 'pgd'\n    PGD_EPS: 0.1\n")
    cfg = cfgmod.load_config(str(p))
    assert cfg.SINGLE_VIDEO_ATTACK.OPTIMIZER == "adam" and cfg.SINGLE_VIDEO_ATTACK.PGD_EPS is None
    assert cfg.UNIVERSAL_ATTACK.OPTIMIZER == "pgd" and cfg.UNIVERSAL_ATTACK.PGD_EPS == 0.1
    assert "CLASS_GEN_ATTACK" not in cfg                # absent sections stay absent
    p.write_text("CLASS_GEN_ATTACK:\n    OPTIMIZER: 'sgd'\n")
    with pytest.raises(ValueError, match="OPTIMIZER"):
        cfgmod.load_config(str(p))
    shipped = cfgmod.load_config(os.path.join(ROOT, "run_config.yml"))
    for sec in cfgmod.ATTACK_SECTIONS:
        assert shipped[sec].OPTIMIZER == "adam"


def test_unknown_optimizer_raises_before_anything_else():
    import inspect
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D, check_optimizer
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, VideoLearnerAdversarial
    assert check_optimizer("adam") == "adam" and check_optimizer("pgd") == "pgd"
    for bad in ("sgd", "PGD", None, ""):
        with pytest.raises(ValueError, match="optimizer"):
            check_optimizer(bad)
        with pytest.raises(ValueError, match="optimizer"):
            FlickerI3D({}, optimizer=bad)
        with pytest.raises(ValueError, match="optimizer"):
            FlickerVideoResNet("r2plus1d_18", {}, optimizer=bad)
    for cls in (FlickerI3D, FlickerVideoResNet, VideoLearnerAdversarial):
        assert inspect.signature(cls.__init__).parameters["optimizer"].default == "adam"
    assert inspect.signature(FlickerI3D.__init__).parameters["pgd_eps"].default is None


def _fake_engine(optimizer):
    d = torch.arange(48, dtype=torch.float32).reshape(16, 1, 1, 3) * 1e-3
    eng = types.SimpleNamespace(optimizer=optimizer, perturbation=d, adam_t=7)
    eng.adam_m, eng.adam_v = (None, None) if optimizer == "pgd" else (torch.ones(16, 3), torch.full((16, 3), 2.0))
    return eng


def test_pgd_checkpoints_carry_no_moments_and_mismatched_resumes_are_refused():
    from flickering_adversarial_video_amd import i3d_dataset_attack as da
    t = da.checkpoint_tensors(_fake_engine("pgd"), 30)
    assert set(t) == {"RGB/eps", "pgd_steps"} and int(t["pgd_steps"]) == 30
    np.testing.assert_array_equal(t["RGB/eps"], _fake_engine("pgd").perturbation.numpy())
    t = da.checkpoint_tensors(_fake_engine("adam"), 30)
    assert set(t) == {"RGB/eps", "RGB/eps/Adam", "RGB/eps/Adam_1", "beta1_power", "beta2_power"}       # unchanged under Adam
    for ck_opt, eng_opt in (("adam", "pgd"), ("pgd", "adam")):
        with pytest.raises(ValueError) as e:
            da.check_checkpoint_optimizer(_fake_engine(eng_opt), ck_opt, "model_step_00030")
        assert f"OPTIMIZER: {ck_opt}" in str(e.value) and f"OPTIMIZER: {eng_opt}" in str(e.value)
    for opt in ("adam", "pgd"):
        da.check_checkpoint_optimizer(_fake_engine(opt), opt, "x")
        da.check_checkpoint_optimizer(_fake_engine(opt), None, "x")        # a bare perturbation resumes under either
