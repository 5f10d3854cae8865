"""The pointer contract of the perturbation entry points (include/flicker_hip.h), on a machine without a GPU: every refusal is FLK_EINVAL
with a message naming the alignment, and it comes BEFORE any GPU call.  Fake pointers, as in tests/test_video_time_cpu.py: each call
is valid in everything but the one pointer (or size) under test, and no call here passes a fully valid argument set -- nothing is
ever launched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = 0x10000            # 16-byte aligned, never dereferenced
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def p(addr):
    return C.c_void_p(addr)


def apply_args(x, u8, fold_t=2, dense=False, lut=False):
    from flickering_adversarial_video_amd import _lib
    a = _lib.ApplyArgs()
    a.x, a.x_is_u8, a.x_scale, a.x_bias = x, int(u8), 1.0 / 128.0, -1.0
    a.delta, a.delta_dense, a.dclip = GOOD, int(dense), 0.4
    a.inv_std = (C.c_float * 3)(1.0, 1.0, 1.0)
    a.lo, a.hi, a.adv_flag = -1.0, 1.0, 1.0
    a.B, a.T, a.H, a.W, a.fold_t = 2, 8, 12, 16, fold_t
    if lut:
        a.x_lut = GOOD
    return a


def refused(lib, rc, *words):
    msg = lib.flk_last_error().decode()
    assert rc == EINVAL, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("fold_t", [1, 2, 3, 4])
@pytest.mark.parametrize("dense", [False, True], ids=["flicker", "dense"])
def test_apply_and_grad_refuse_a_misaligned_clip(lib, fold_t, dense):
    from flickering_adversarial_video_amd import _lib
    dt = _lib.FLK_BF16 if fold_t == 4 else _lib.FLK_F32
    for off in (1, 3, 7):              # uint8: odd addresses
        a = apply_args(GOOD + off, True, fold_t, dense, lut=fold_t == 4)
        refused(lib, lib.flk_perturb_apply_s2d(C.byref(a), p(GOOD), dt, None), "uint8 clip", "2-byte aligned")
        refused(lib, lib.flk_perturb_grad_reduce(C.byref(a), p(GOOD), _lib.FLK_F32, p(GOOD), p(GOOD), None), "uint8 clip", "2-byte aligned")
    for off in (4, 12, 2):             # fp32: anything that is no multiple of 8
        a = apply_args(GOOD + off, False, fold_t, dense)
        refused(lib, lib.flk_perturb_apply_s2d(C.byref(a), p(GOOD), dt, None), "fp32 clip", "8-byte aligned")
        refused(lib, lib.flk_perturb_grad_reduce(C.byref(a), p(GOOD), _lib.FLK_F32, p(GOOD), p(GOOD), None), "fp32 clip", "8-byte aligned")


@pytest.mark.parametrize("fold_t", [1, 2, 3, 4])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32in"])
def test_apply_out_and_gradient_in_are_16_byte_aligned(lib, fold_t, u8):
    from flickering_adversarial_video_amd import _lib
    a = apply_args(GOOD, u8, fold_t, lut=u8 and fold_t == 4)
    for off in (2, 4, 8):
        for dt in ((_lib.FLK_BF16,) if fold_t == 4 else (_lib.FLK_BF16, _lib.FLK_F32)):
            refused(lib, lib.flk_perturb_apply_s2d(C.byref(a), p(GOOD + off), dt, None), "out", "16-byte aligned")
        for dt in (_lib.FLK_BF16, _lib.FLK_F32):
            refused(lib, lib.flk_perturb_grad_reduce(C.byref(a), p(GOOD + off), dt, p(GOOD), p(GOOD), None), "gx_s2d", "16-byte aligned")


def dense_args(pgd):
    from flickering_adversarial_video_amd import _lib
    a = _lib.DenseAdamArgs()
    a.T, a.H, a.W, a.torch_dialect = 3, 4, 6, 0
    a.beta, a.g_scale, a.lr, a.adam_b1, a.adam_b2, a.adam_eps, a.step = 1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1
    a.pgd_eps = 0.4 if pgd else 0.0
    return a


def test_dense_update_streams_are_16_byte_aligned(lib):
    a = dense_args(False)
    for k in range(4):                 # g_adv, delta, m, v: one of them off, the others fine
        for off in (4, 8, 12):
            ptrs = [p(GOOD + (off if j == k else 0)) for j in range(4)]
            refused(lib, lib.flk_perturb_dense_l12_adam(C.byref(a), *ptrs, p(GOOD), p(GOOD), None), "g_adv, delta, m and v", "16-byte aligned")
    a = dense_args(True)
    for k in range(2):
        for off in (4, 8, 12):
            ptrs = [p(GOOD + (off if j == k else 0)) for j in range(2)]
            refused(lib, lib.flk_perturb_dense_l12_pgd(C.byref(a), *ptrs, p(GOOD), p(GOOD), None), "g_adv and delta", "16-byte aligned")


def test_flicker_updates_refuse_T_683(lib):
    """256 threads x 8 values hold 3 * T <= 2048: T = 682 is the last size the four one-workgroup update kernels take"""
    from flickering_adversarial_video_amd import _lib
    a = _lib.AdamArgs()
    a.T, a.torch_dialect = 683, 0
    a.beta0, a.beta1, a.beta2, a.beta3, a.g_scale, a.lr = 1.0, 0.5, 0.5, 0.5, 1.0, 1e-3
    a.adam_b1, a.adam_b2, a.adam_eps, a.step, a.pgd_eps = 0.9, 0.999, 1e-8, 1, 0.4
    g = p(GOOD)
    refused(lib, lib.flk_perturb_reg_adam(C.byref(a), g, g, g, g, g, None), "T out of range (683)")
    refused(lib, lib.flk_perturb_reg_adam_batched(C.byref(a), 3, g, g, g, g, g, None, None, g, None), "T out of range (683)")
    refused(lib, lib.flk_perturb_reg_pgd(C.byref(a), g, g, g, None), "T out of range (683)")
    refused(lib, lib.flk_perturb_reg_pgd_batched(C.byref(a), 3, g, g, g, None, None, g, None), "T out of range (683)")
    a.T = 0
    refused(lib, lib.flk_perturb_reg_adam(C.byref(a), g, g, g, g, g, None), "T out of range (0)")


def test_header_states_the_contract():
    hdr = re.sub(r"\s+\*?\s*", " ", open(os.path.join(ROOT, "include", "flicker_hip.h")).read())
    assert "a uint8 clip x is 2-byte aligned and an fp32 clip 8-byte aligned" in hdr
    assert "out and gx_s2d are 16-byte aligned" in hdr
    assert "g_adv, delta, m and v (flk_perturb_dense_l12_pgd: g_adv and delta) are 16-byte aligned" in hdr
