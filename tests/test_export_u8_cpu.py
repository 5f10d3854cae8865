"""The 8-bit export on the host (no GPU): the numpy restatement of flk_adv_export_u8's encode (videoresnet_spec.encode_u8, i3d_spec.encode_u8,
ops.export_adversarial_u8_host) round-trips every byte, realises integer levels exactly, agrees with the reference's own float64
de-normalisation except at ties, and the entry point refuses bad arguments before any device call."""
import ctypes as C

import numpy as np
import pytest


def test_encode_round_trips_every_byte():
    from flickering_adversarial_video_amd import i3d_spec, videoresnet_spec as vs
    q = vs.encode_u8(vs.u8_decode_table())
    assert q.dtype == np.uint8 and q.shape == (256, 3)
    assert np.array_equal(q, np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1))          # all 768 entries
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal(i3d_spec.encode_u8(v / np.float32(128.0) - np.float32(1.0)), np.arange(256, dtype=np.uint8))


def test_encode_saturates_and_sends_nan_to_zero():
    from flickering_adversarial_video_amd import i3d_spec, videoresnet_spec as vs
    x = np.array([np.nan, -np.inf, np.inf, -5.0, 5.0, 1.0], np.float32)
    assert i3d_spec.encode_u8(x).tolist() == [0, 0, 255, 0, 255, 255]
    x[5] = 3.0                                  # (3 * std + mean) * 255 > 255 in every channel
    assert vs.encode_u8(np.stack([x, x, x], -1)).tolist() == [[v] * 3 for v in (0, 0, 255, 0, 255, 255)]
    # ties go to the even level: z = 0.5, 1.5, 2.5 exactly (TF dialect: y * 128 is exact)
    z = np.array([0.5, 1.5, 2.5, 254.5], np.float32)
    assert i3d_spec.encode_u8(z / np.float32(128.0) - np.float32(1.0)).tolist() == [0, 2, 2, 254]


def test_integer_levels_are_realised_exactly():
    """bytes 30..200, delta = k / 255 for every k in -20..20, torch dialect, max_norm 0.1, the scalar clamp: the frames hold byte + k"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    bytes_ = np.arange(30, 201, dtype=np.uint8)
    x = np.repeat(bytes_[:, None], 3, axis=1).reshape(1, 1, 1, -1, 3)                                # [1,1,1,171,3]
    lo = float(np.max((0.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    hi = float(np.min((1.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    lut = vs.u8_decode_table()
    for k in range(-20, 21):
        d = np.full((1, 3), np.float32(k) / np.float32(255.0), np.float32)
        q, st = ops.export_adversarial_u8_host(x, d, dialect="torch", dclip=0.1, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo, hi=hi,
                                               x_lut=lut, stats=True)
        assert np.array_equal(q.astype(np.int64), x.astype(np.int64) + k), k
        assert (st[0, 0, :, 0] == k * 171).all() and (st[0, 0, :, 1] == abs(k) * 171).all()
        assert (st[0, 0, :, 2] == (171 if k else 0)).all() and (st[0, 0, :, 3] == 0).all()


@pytest.mark.parametrize("case", ["flk01", "flk02", "dense02"])
def test_encode_agrees_with_the_reference_de_normalisation(golden, case):
    """the reference's own float64 ``convert_adversarial_video_zero_one`` of its perturbed clip, times 255 and rounded, against the float32
    encode: a byte may differ by one level, only within 1e-3 of a tie, in at most 3 of the 6144 values (here: 1 / 0 / 0)"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    xadv = np.transpose(golden[f"pert_{case}_xadv"], (0, 2, 3, 4, 1))                                # NCDHW -> [B,T,H,W,3]
    z = 255.0 * golden[f"pert_{case}_zero_one"]
    assert xadv.shape == z.shape and z.size == 6144
    q = vs.encode_u8(xadv).astype(np.int64)
    ref = np.clip(np.rint(z), 0, 255).astype(np.int64)
    diff = q != ref
    print(case, "values that differ:", int(diff.sum()), "distance from a tie:", np.abs(np.abs(z - np.floor(z)) - 0.5)[diff])
    assert np.abs(q - ref).max() <= 1
    assert (np.abs(np.abs(z - np.floor(z)) - 0.5)[diff] < 1e-3).all()
    assert diff.sum() <= 3


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    """every refusal of flk_adv_export_u8 is FLK_EINVAL with a message, decided on the host (no device work)"""
    from flickering_adversarial_video_amd import _lib

    def args(**kw):
        a, e = _lib.ApplyArgs(), _lib.ExportArgs()
        a.x, a.delta = 8, 8                   # never dereferenced: every case below is refused on the host
        a.B, a.T, a.H, a.W = 2, 3, 5, 7
        a.lo, a.hi, a.adv_flag = -1.0, 1.0, 1.0
        e.mul, e.add, e.levels = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(1, 1, 1), 128.0
        e.out_clip_stride = 3 * 5 * 7 * 3
        for k, v in kw.items():
            setattr(e if hasattr(e, k) else a, k, v)
        return a, e

    def refused(word, out=C.c_void_p(8), stats=None, null_a=False, null_e=False, **kw):
        a, e = args(**kw)
        rc = lib.flk_adv_export_u8(None if null_a else C.byref(a), None if null_e else C.byref(e), out, stats, None)
        msg = lib.flk_last_error()
        assert rc == -1 and word in msg, (kw, rc, msg)

    refused(b"null", null_a=True)
    refused(b"null", null_e=True)
    refused(b"null", x=None)
    refused(b"null", delta=None)
    refused(b"null out", out=None)
    for dim in ("B", "T", "H", "W"):
        refused(b"positive", **{dim: 0})
        refused(b"positive", **{dim: -4})
    refused(b"center", center=1)
    refused(b"levels", levels=0.0)
    refused(b"levels", levels=-255.0)
    refused(b"out_clip_stride", out_clip_stride=3 * 5 * 7 * 3 - 1)
    refused(b"delta_T", delta_T=4, delta_dense=1)
    refused(b"delta_T", delta_T=4, delta_per_clip=1)
    refused(b"stats", stats=C.c_void_p(8), H=4096, W=2048, out_clip_stride=1 << 60)
    refused(b"stats", stats=C.c_void_p(8), H=1, W=8388608, out_clip_stride=1 << 60)
    refused(b"too large", H=65536, W=16384, out_clip_stride=1 << 60)
