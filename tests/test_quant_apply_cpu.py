"""The quantised apply (flk_apply_args.q_lut), host side: ops.perturb_apply_quantised_host is the decode of the exported bytes, whole
levels move whole bytes and a sub-level perturbation moves none; make_apply_args refuses what has no meaning; the C ABI holds the four
fields and flk_perturb_apply_s2d / the I3D-only entry points refuse them before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clip_u8(B, T, H, W, seed):
    """random bytes with rows of 0 and of 255 planted, and every byte value present: the clamp bounds are hit"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    u8 = vs.synthetic_clip_u8(B, T, H, W, seed=seed)
    u8[:, :, :2] = 0
    u8[:, :, 2:4] = 255
    free = u8[:, :, 4:].reshape(-1)                  # (a copy: the rows below the planted ones)
    free[:256] = np.arange(256, dtype=np.uint8)
    u8[:, :, 4:] = free.reshape(u8[:, :, 4:].shape)
    assert len(np.unique(u8)) == 256
    return u8


def torch_kw():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    lo = float(np.max((0.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    hi = float(np.min((1.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    return dict(dialect="torch", dclip=0.2, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo, hi=hi)


TF_KW = dict(dialect="tf", dclip=0.4, inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clamp(v, kw):
    return np.minimum(np.maximum(v, np.float32(kw["lo"])), np.float32(kw["hi"])).astype(np.float32)


def test_host_route_is_the_decode_of_the_exported_bytes():
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    B, T, H, W = 2, 4, 10, 16
    u8 = clip_u8(B, T, H, W, seed=3)
    rng = np.random.default_rng(5)
    tf_table = (np.arange(256, dtype=np.float32) / np.float32(128.0) - np.float32(1.0))[:, None].repeat(3, 1)
    assert np.array_equal(bits(ops.quant_table_host("tf")), bits(tf_table))
    assert np.array_equal(bits(ops.quant_table_host("torch")), bits(vs.u8_decode_table()))
    with pytest.raises(ValueError, match="dialect"):
        ops.quant_table_host("jpeg")
    sources = [(vs.normalize_u8(u8), torch_kw(), {}), (u8, torch_kw(), dict(x_lut=vs.u8_decode_table())), (u8, dict(TF_KW), {})]
    bounds = np.linspace(0.15, 0.25, B).astype(np.float32)
    perts = [(rng.uniform(-0.2, 0.2, (T, 3)).astype(np.float32), {}),
             (rng.uniform(-0.2, 0.2, (B, T, 3)).astype(np.float32), dict(dclip_clip=bounds)),
             (rng.uniform(-0.2, 0.2, (T, H, W, 3)).astype(np.float32), dict(shift_x=1, shift_p=3))]
    for x, kw, lut in sources:
        table = ops.quant_table_host(kw["dialect"])
        for d, extra in perts:
            got = ops.perturb_apply_quantised_host(x, d, adv_flag=1.0, **kw, **lut, **extra)
            q = ops.export_adversarial_u8_host(x, d, adv_flag=1.0, **kw, **lut, **extra)
            assert got.dtype == np.float32 and got.shape == (B, T, H, W, 3)
            assert np.array_equal(bits(got), bits(table[q, np.arange(3)]))
            assert q.min() == 0 and q.max() == 255                   # both ends of the byte range are reached
            # the round trip is idempotent: the bytes of the quantised clip are the bytes
            assert np.array_equal(ops.encode_u8_host(got, kw["dialect"]), q)


def test_whole_levels_move_whole_bytes():
    """delta = k / 255 on bytes 30..200, k in -20..20 (every k, one per (clip, frame, channel)): exactly table[byte + k]"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    B, T, H, W = 2, 8, 6, 8
    rng = np.random.default_rng(7)
    u8 = rng.integers(30, 201, (B, T, H, W, 3)).astype(np.uint8)
    k = np.concatenate([np.arange(-20, 21), rng.integers(-20, 21, B * T * 3 - 41)])
    k = rng.permutation(k).reshape(B, T, 3)
    d = (k / 255.0).astype(np.float32)
    table = vs.u8_decode_table()
    want = table[(u8.astype(np.int64) + k[:, :, None, None, :]), np.arange(3)]
    for x, lut in ((u8, dict(x_lut=table)), (vs.normalize_u8(u8), {})):
        got = ops.perturb_apply_quantised_host(x, d, adv_flag=1.0, **torch_kw(), **lut)
        assert np.array_equal(bits(got), bits(want))


def test_a_sub_level_perturbation_moves_no_byte():
    """|delta| = 1e-4 (0.0255 levels) on a uint8 clip of every byte value: the quantised clip is the clean clip.  TF dialect: everywhere --
    its clamp bounds are byte values (-1 is byte 0; byte 255 is below +1).  Torch dialect: wherever the clean value lies inside
    [lo, hi].  Outside (bytes 0..9 / 234..255, depending on the channel) the attack's clamp moves the value to a bound with ANY delta, and
    a bound is a byte value of one channel only: the stored byte is the level nearest the bound, not the clean byte -- there the
    quantised clip is the decode of the exported bytes (test_host_route_is_the_decode_of_the_exported_bytes), what a stored video holds."""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    B, T, H, W = 1, 4, 10, 16
    u8 = clip_u8(B, T, H, W, seed=11)
    d = (1e-4 * np.where(np.random.default_rng(13).random((T, 3)) < 0.5, -1.0, 1.0)).astype(np.float32)
    tf_clean = (u8.astype(np.float32) / np.float32(128.0) - np.float32(1.0)).astype(np.float32)
    got = ops.perturb_apply_quantised_host(u8, d, adv_flag=1.0, **TF_KW)
    assert np.array_equal(bits(got), bits(tf_clean))
    kw = torch_kw()
    clean = vs.normalize_u8(u8)
    got = ops.perturb_apply_quantised_host(u8, d, adv_flag=1.0, x_lut=vs.u8_decode_table(), **kw)
    inside = (clean >= np.float32(kw["lo"])) & (clean <= np.float32(kw["hi"]))
    assert 0.5 < inside.mean() < 1.0
    assert np.array_equal(bits(got)[inside], bits(clean)[inside])
    # the float clip the optimiser saw before differs from the clean clip at most values
    assert (bits(clamp(clean + (d * np.array(kw["inv_std"], np.float32))[None, :, None, None, :], kw)) != bits(clean)).mean() > 0.5


def test_make_apply_args_refuses_quantise_with_center_and_unknown_dialects():
    import torch
    from flickering_adversarial_video_amd import ops
    xu = torch.zeros((1, 2, 4, 4, 3), dtype=torch.uint8)
    d = torch.zeros((2, 3), dtype=torch.float32)
    for dialect in ("torch", "tf"):
        with pytest.raises(ValueError, match="center"):
            ops.make_apply_args(xu, d, dialect="tf", quantise=dialect, center=True)
    with pytest.raises(ValueError, match="quantise"):
        ops.make_apply_args(xu, d, dialect="tf", quantise="jpeg")
    with pytest.raises(ValueError, match="quantise"):          # a table alone names no encode
        ops.make_apply_args(xu, d, dialect="tf", q_lut=torch.zeros((256, 3)))
    with pytest.raises(ValueError, match="q_lut"):             # the table lives on the device
        ops.make_apply_args(xu, d, dialect="tf", quantise="tf", q_lut=torch.zeros((256, 3)))
    a = ops.make_apply_args(xu, d, dialect="tf")                # off by default: the fields are zero
    assert not a.q_lut and a.q_levels == 0.0 and tuple(a.q_mul) == (0.0, 0.0, 0.0)


def test_apply_args_layout_holds_the_quantiser_fields(tmp_path):
    from flickering_adversarial_video_amd import _lib
    names = ("dclip_dev", "q_lut", "q_mul", "q_add", "q_levels", "x_lut")
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flicker_hip.h"\n'
                   'int main(void) { printf("%zu' + " %zu" * len(names) + '\\n", sizeof(flk_apply_args), '
                   + ", ".join(f"offsetof(flk_apply_args, {n})" for n in names) + '); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    size, *offs = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.ApplyArgs) == size
    assert [getattr(_lib.ApplyArgs, n).offset for n in names] == offs
    assert [f[0] for f in _lib.ApplyArgs._fields_[-6:]] == list(names)            # behind dclip_dev, in the header's order; x_lut stays last
    assert offs[1] == offs[0] + 8 and offs[2] == offs[1] + 8 and offs[3] == offs[2] + 12 and offs[4] == offs[3] + 12
    assert offs[5] == offs[4] + 8 and size == offs[5] + 8                           # q_levels, 4 bytes of padding, the x_lut pointer


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_entry_points_refuse_a_quantiser_they_cannot_honour(lib):
    """host-side validation only: every call returns FLK_EINVAL before it touches a device pointer"""
    from flickering_adversarial_video_amd import _lib
    fake = C.c_void_p(256)

    def args(**kw):
        a = _lib.ApplyArgs()
        a.x, a.x_is_u8, a.delta, a.q_lut = fake, 1, fake, fake
        a.x_scale, a.x_bias = 1.0 / 128.0, -1.0
        a.inv_std = (C.c_float * 3)(1.0, 1.0, 1.0)
        a.q_mul, a.q_add, a.q_levels = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(1.0, 1.0, 1.0), 128.0
        a.lo, a.hi, a.adv_flag = -1.0, 1.0, 1.0
        a.B, a.T, a.H, a.W, a.fold_t = 1, 16, 224, 224, 3
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad in (args(center=1), args(q_levels=0.0), args(q_levels=-255.0)):
        assert lib.flk_perturb_apply_s2d(C.byref(bad), fake, _lib.FLK_F32, None) == -1 and b"q_lut" in lib.flk_last_error()
        assert lib.flk_perturb_apply_s2d(C.byref(bad), fake, _lib.FLK_BF16, None) == -1 and b"q_lut" in lib.flk_last_error()
    a = args()
    assert lib.flk_stem_delta_grad_mask(C.byref(a), fake, None) == -1 and b"q_lut" in lib.flk_last_error()
    assert lib.flk_stem_delta_grad(C.byref(a), fake, 64, fake, fake, fake, 0, None) == -1 and b"q_lut" in lib.flk_last_error()
    assert lib.flk_stem_delta_bias(C.byref(a), fake, fake, None) == -1 and b"q_lut" in lib.flk_last_error()
    a.center = 1
    assert lib.flk_stem_fwd_u8(C.byref(a), fake, fake, fake, None, 0, fake, 64, None) == -1 and b"q_lut" in lib.flk_last_error()
