"""uint8 VideoResNet clips, host side: the decode table is the scripts' float32 normalisation, the C ABI of flk_apply_args.x_lut
matches ctypes, and every entry point that cannot honour the table refuses it before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_table_is_the_float32_host_normalisation():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    t = vs.u8_decode_table()
    mean, std = np.array(vs.DEFAULT_MEAN, np.float32), np.array(vs.DEFAULT_STD, np.float32)
    ref = (np.arange(256, dtype=np.uint8).astype(np.float32)[:, None] / 255.0 - mean) / std
    assert t.dtype == np.float32 and t.shape == (256, 3) and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t.view(np.uint32), ref.astype(np.float32).view(np.uint32))
    for seed in (1234, 5):
        u8 = vs.synthetic_clip_u8(2, 4, 6, 8, seed=seed)
        x = vs.synthetic_clip(2, 4, 6, 8, seed=seed)
        assert u8.dtype == np.uint8 and np.array_equal(x.view(np.uint32), t[u8, np.arange(3)].view(np.uint32))
        assert np.array_equal(vs.normalize_u8(u8).view(np.uint32), x.view(np.uint32))


def test_apply_args_layout_matches_the_header(tmp_path):
    from flickering_adversarial_video_amd import _lib
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flicker_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(flk_apply_args), offsetof(flk_apply_args, x_lut), '
                   'offsetof(flk_apply_args, dclip_dev)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    size, off_lut, off_dclip = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.ApplyArgs) == size
    assert _lib.ApplyArgs.x_lut.offset == off_lut and _lib.ApplyArgs.dclip_dev.offset == off_dclip
    assert _lib.ApplyArgs._fields_[-1][0] == "x_lut"


def test_make_apply_args_needs_a_table_for_uint8_torch_clips():
    import torch
    from flickering_adversarial_video_amd import ops
    xu = torch.zeros((1, 2, 4, 4, 3), dtype=torch.uint8)
    d = torch.zeros((2, 3), dtype=torch.float32)
    with pytest.raises(AssertionError, match="x_lut"):
        ops.make_apply_args(xu, d, dialect="torch")
    with pytest.raises(AssertionError, match="x_lut"):           # the table decodes uint8 clips only
        ops.make_apply_args(xu.float(), d, dialect="torch", x_lut=torch.zeros((256, 3)))
    a = ops.make_apply_args(xu, d, dialect="tf")                  # the I3D decode is unchanged: no table
    assert a.x_is_u8 == 1 and not a.x_lut


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_entry_points_refuse_the_table_where_it_has_no_meaning(lib):
    """host-side validation only: every call returns FLK_EINVAL before it touches a device pointer"""
    from flickering_adversarial_video_amd import _lib
    fake = C.c_void_p(256)

    def args(**kw):
        a = _lib.ApplyArgs()
        a.x, a.x_is_u8, a.delta, a.x_lut = fake, 1, fake, fake
        a.inv_std = (C.c_float * 3)(1.0, 1.0, 1.0)
        a.lo, a.hi, a.adv_flag = -1.0, 1.0, 1.0
        a.B, a.T, a.H, a.W, a.fold_t = 1, 16, 224, 224, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad in (args(x_is_u8=0), args(center=1, fold_t=3)):
        assert lib.flk_perturb_apply_s2d(C.byref(bad), fake, _lib.FLK_F32, None) == -1 and b"x_lut" in lib.flk_last_error()
        assert lib.flk_perturb_grad_reduce(C.byref(bad), fake, _lib.FLK_F32, fake, fake, None) == -1 and b"x_lut" in lib.flk_last_error()
    a = args(fold_t=3)
    assert lib.flk_stem_delta_grad_mask(C.byref(a), fake, None) == -1 and b"x_lut" in lib.flk_last_error()
    assert lib.flk_stem_delta_grad(C.byref(a), fake, 64, fake, fake, fake, 0, None) == -1 and b"x_lut" in lib.flk_last_error()
    assert lib.flk_stem_delta_bias(C.byref(a), fake, fake, None) == -1 and b"x_lut" in lib.flk_last_error()
    a.center = 1
    assert lib.flk_stem_fwd_u8(C.byref(a), fake, fake, fake, None, 0, fake, 64, None) == -1 and b"x_lut" in lib.flk_last_error()
