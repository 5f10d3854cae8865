"""Inter-frame prediction in the codec without a GPU: the numpy integer restatement with GOPs of zero-motion P-frames
(videoresnet_spec.codec_roundtrip_host(gop=, first_frame=), the definition of flk_codec_roundtrip_gop_u8), the flicker facts it was
built for, ``Codec(gop=)`` and ``--codec-gop``, and the argument contract of the new ABI entries (nothing here launches anything)."""
import argparse
import ctypes as C

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

SUBS = ("444", "420")


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def moving(N, H, W, seed):
    """smooth luminance and chroma plus noise, a different phase per frame"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for n in range(N):
        img = np.stack([128 + 70 * np.sin(xx / 9. + n / 3.) + 40 * np.cos(yy / 5.), 120 + 60 * np.cos(xx / 13. + yy / 7. - n / 4.),
                        100 + 80 * np.sin(yy / 11. + n / 5.) - 30 * np.cos(xx / 4.)], -1) + rng.normal(0, 6, (H, W, 3))
        out.append(np.clip(np.rint(img), 0, 255))
    return np.stack(out).astype(np.uint8)


def checker(H, W, inverse=False):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat(((((yy + xx + int(inverse)) & 1)) * 255).astype(np.uint8)[..., None], 3, -1)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_gop_1_is_the_intra_codec(sub):
    for (H, W), q in (((8, 8), 1), ((17, 23), 50), ((33, 40), 75), ((16, 48), 100)):
        x = moving(4, H, W, seed=H)
        o, st = vs.codec_roundtrip_host(x, q, sub, stats=True)
        o1, st1 = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=1)
        assert o1.dtype == np.uint8 and st1.dtype == np.int32 and (o == o1).all() and (st == st1).all(), (H, W, q)
        o3, st3 = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=1, first_frame=3)
        assert (o == o3).all() and (st == st3).all()


@pytest.mark.parametrize("sub", SUBS)
def test_intra_frames_gop_isolation_and_spans(sub):
    gop, q = 3, 60
    x = moving(8, 24, 40, seed=7)
    o, st = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=gop)
    intra, intra_st = vs.codec_roundtrip_host(x, q, sub, stats=True)
    for n in range(8):
        if n % gop == 0:                                        # an intra frame is the intra call on that frame alone
            assert (o[n] == intra[n]).all() and (st[n] == intra_st[n]).all(), n
            assert (o[n] == vs.codec_roundtrip_host(x[n], q, sub)).all()
    assert any((o[n] != intra[n]).any() for n in range(8) if n % gop)              # a P-frame is not
    # a source frame changes no output byte of any other GOP (and none before it in its own)
    y = x.copy()
    y[4] = 255 - y[4]
    o2 = vs.codec_roundtrip_host(y, q, sub, gop=gop)
    assert (o2[:4] == o[:4]).all() and (o2[6:] == o[6:]).all() and (o2[4] != o[4]).any() and (o2[5] != o[5]).any()
    # a span that starts on an intra frame is the whole video's result, sliced
    for k, count in ((1, 5), (2, 2), (1, 1)):
        so, sst = vs.codec_roundtrip_host(x[k * gop:k * gop + count], q, sub, stats=True, gop=gop, first_frame=k * gop)
        assert (so == o[k * gop:k * gop + count]).all() and (sst == st[k * gop:k * gop + count]).all(), (k, count)
    for bad in (1, 2, 4, -3, True, 1.0):
        with pytest.raises(ValueError, match="first_frame"):
            vs.codec_roundtrip_host(x[:2], q, sub, gop=gop, first_frame=bad)
    for bad in (0, -1, 65536, 2.0, True):
        with pytest.raises(ValueError, match="gop"):
            vs.codec_roundtrip_host(x[:2], q, sub, gop=bad)
    # a tone table per frame: the call on the toned frames
    tone = np.random.RandomState(1).randint(0, 256, (8, 256, 3)).astype(np.uint8)
    toned = np.stack([np.stack([tone[n, :, c][x[n, :, :, c]] for c in range(3)], -1) for n in range(8)])
    assert (vs.codec_roundtrip_host(x, q, sub, tone=tone, gop=gop) == vs.codec_roundtrip_host(toned, q, sub, gop=gop)).all()


def test_a_plane_equal_to_its_reference_has_no_levels():
    rng = np.random.RandomState(2)
    ref = rng.randint(0, 256, (1, 16, 24)).astype(np.int32)
    for qp in (1, 8, 255):
        rec, lev = vs._codec_plane_inter(ref.copy(), ref, qp, np.int32)
        assert (lev == 0).all() and (rec == ref).all()
    # so a still video that its intra frame reproduces (a flat grey on the luma DC grid) costs nothing after it
    x = np.full((5, 17, 23, 3), 160, np.uint8)
    for sub in SUBS:
        o, st = vs.codec_roundtrip_host(x, 50, sub, stats=True, gop=5)
        assert (st[1:] == 0).all() and st[0, 0] > 0 and (o == x).all()


def test_inter_step():
    assert [vs.codec_inter_step(q) for q in (1, 25, 50, 75, 100)] == [255, 32, 16, 8, 1]
    for bad in (0, 101, 50.0):
        with pytest.raises(ValueError):
            vs.codec_inter_step(bad)


@pytest.mark.parametrize("sub", SUBS)
def test_int32_is_enough_at_the_extremes(sub):
    """the largest residuals there are -- a 0 / 255 checkerboard against its inverse, flat 0 against flat 255, independent 0 / 255 per
    channel -- in int32 and int64 side by side, gop 4 over 6 frames: equal, so nothing wraps; and the clamps saturate"""
    rng = np.random.RandomState(5)
    H, W = 24, 32
    videos = {"checker": np.stack([checker(H, W, n & 1) for n in range(6)]),
              "flat": np.stack([np.full((H, W, 3), 255 * (n & 1), np.uint8) for n in range(6)]),
              "random": rng.choice(np.array([0, 255], np.uint8), (6, H, W, 3))}
    for name, x in videos.items():
        for q in (1, 25, 50, 75, 100):
            o32, s32 = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=4)
            o64, s64 = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=4, _dtype=np.int64)
            assert (o32 == o64).all() and (s32 == s64).all(), (name, q)
    o = vs.codec_roundtrip_host(videos["flat"], 100, sub, gop=4)
    assert (o == videos["flat"]).all()                           # step 1: flat black <-> white is reproduced, 0 and 255 reached, no wrap
    o = vs.codec_roundtrip_host(videos["checker"], 100, "444", gop=4).astype(int)
    assert np.abs(o - videos["checker"].astype(int)).max() <= 2 and o.min() == 0 and o.max() == 255
    # the forward transform of the largest residual: |f| <= 8 * 8 * 255 = 16320, so |f| + 2 Qp < 2^15
    r = np.full((1, 1, 1, 8, 8), 255, np.int32)
    f = vs._fdct_1d(vs._fdct_1d(r, -2, 11).swapaxes(-1, -2), 2, 15)
    assert int(np.abs(f).max()) == 16320 and 16320 + 2 * 255 < 2 ** 15


# ---- what the model is for: the inter-frame quantiser decides whether a flicker arrives ------------------------------------------
def flicker_video(d, N=9, grey=128):
    """flat grey whose intra frame (frame 0) carries the grey itself and whose P-frames carry grey +d, -d, +d, ...: a flicker of +-d
    levels about what the reference holds"""
    x = np.full((N, 16, 16, 3), grey, np.int64)
    x[1::2] += d
    x[2::2] -= d
    return x.astype(np.uint8)


@pytest.mark.parametrize("sub", SUBS)
def test_flicker_of_one_level_is_erased_at_quality_50_and_survives_at_75(sub):
    x = flicker_video(1)
    o, st = vs.codec_roundtrip_host(x, 50, sub, stats=True, gop=9)
    assert vs.codec_inter_step(50) == 16
    assert (st[1:] == 0).all() and (o == 128).all()              # zero levels in every P-frame: the reconstruction never moves
    # wherever the flicker stands against the intra frame, it is gone from the second P-frame on
    y = np.full((9, 16, 16, 3), 128, np.int64)
    y[0::2] -= 1
    y[1::2] += 1
    o, st = vs.codec_roundtrip_host(y.astype(np.uint8), 50, sub, stats=True, gop=9)
    assert (st[2:] == 0).all() and (o[2:] == o[1]).all()
    # the intra model does not see this: every frame carries its own DC there
    assert {int(v) for v in vs.codec_roundtrip_host(x, 50, sub)[:, 0, 0, 0]} == {126, 128, 130}
    o, st = vs.codec_roundtrip_host(x, 75, sub, stats=True, gop=9)
    assert vs.codec_inter_step(75) == 8
    assert (st[1:, 0] > 0).all() and (o == x).all()              # quality 75: every P-frame has levels, the flicker arrives whole


@pytest.mark.parametrize("sub", SUBS)
def test_flicker_of_two_levels_survives_at_quality_50(sub):
    x = flicker_video(2)
    o, st = vs.codec_roundtrip_host(x, 50, sub, stats=True, gop=9)
    assert (st[1:, 0] > 0).all() and (o == x).all()


# ---- Codec and the scripts' options ---------------------------------------------------------------------------------------------
def test_codec_value_semantics():
    c = vs.Codec(60, "444", gop=12)
    assert (c.quality, c.subsampling, c.gop) == (60, "444", 12) and vs.Codec().gop == 1 and vs.Codec(60, "444", 12) == c
    assert c != vs.Codec(60, "444") and c != vs.Codec(60, "444", gop=11) and vs.Codec(60, "444", gop=1) == vs.Codec(60, "444")
    assert hash(c) == hash(vs.Codec(60, "444", gop=12)) and len({c, vs.Codec(60, "444"), vs.Codec(60, "444", gop=1)}) == 2
    assert repr(c) == "Codec(quality=60, subsampling='444', gop=12)" and repr(vs.Codec(60, "444")) == "Codec(quality=60, subsampling='444')"
    assert eval(repr(c), {"Codec": vs.Codec}) == c
    with pytest.raises(AttributeError):
        c.gop = 2
    for bad in (0, -1, 65536, 2.5, True, None, "4"):
        with pytest.raises(ValueError, match="gop"):
            vs.Codec(75, "420", gop=bad)
    assert vs.Codec(75, "420", gop=65535).gop == 65535 and vs.Codec(75, "420", gop=np.int64(4)).gop == 4


def test_codec_gop_option(capsys):
    def parse(argv, used=True):
        ap = argparse.ArgumentParser()
        vs.add_codec_arguments(ap)
        a = ap.parse_args(argv)
        return vs.codec_from_arguments(ap, a, used)

    assert parse([]) is None
    assert parse(["--codec-quality", "60"]) == vs.Codec(60, "420") and parse(["--codec-quality", "60"]).gop == 1
    assert parse(["--codec-quality", "60", "--codec-gop", "12"]) == vs.Codec(60, "420", gop=12)
    assert parse(["--codec-quality", "60", "--codec-subsampling", "444", "--codec-gop", "1"]) == vs.Codec(60, "444")
    for argv, word in ((["--codec-gop", "12"], "--codec-gop needs --codec-quality"), (["--codec-quality", "60", "--codec-gop", "0"], "gop"),
                       (["--codec-quality", "60", "--codec-gop", "70000"], "gop"), (["--codec-quality", "60", "--codec-gop", "x"], "--codec-gop")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err, argv
    with pytest.raises(SystemExit):
        parse(["--codec-quality", "60", "--codec-gop", "4"], used=False)


# ---- the ABI (fake pointers, nothing launched) ------------------------------------------------------------------------------------
def test_inter_step_equals_the_library_at_every_quality(lib):
    for q in range(1, 101):
        qp = C.c_int32(-1)
        assert lib.flk_codec_inter_step(q, C.byref(qp)) == 0 and qp.value == vs.codec_inter_step(q), q
        assert 1 <= qp.value <= 255
    for bad in (0, 101, -3):
        assert lib.flk_codec_inter_step(bad, C.byref(C.c_int32())) == -1 and b"quality" in lib.flk_last_error()
    assert lib.flk_codec_inter_step(50, None) == -1


def test_gop_argument_contract_without_gpu(lib):
    from flickering_adversarial_video_amd import _lib

    def make(n=1):
        arr = (_lib.CodecClip * max(n, 1))()
        for d in arr:
            d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = 0x10000, 12, 24, 40, 24 * 120, 120
            d.dst, d.dst_pitch_t, d.dst_pitch_h = 0x90000, 24 * 120, 120
        a = _lib.CodecArgs()
        a.nclip, a.quality, a.subsampling, a.clips = n, 75, _lib.FLK_CODEC_420, arr
        a._keep = arr
        return a, arr

    def call(a, gop=4, first=(4,), count=(8,), T_max=8, tone=None, stats=None):
        f = None if first is None else (C.c_int32 * len(first))(*first)
        c = None if count is None else (C.c_int32 * len(count))(*count)
        return lib.flk_codec_roundtrip_gop_u8(C.byref(a) if a is not None else None, gop, f, c, T_max, tone, stats, None)

    def refused(word, a=None, **kw):
        a = make()[0] if a is None else a
        assert call(a, **kw) == -1 and word in lib.flk_last_error(), (kw, lib.flk_last_error())

    assert call(None) == -1
    refused(b"null first", first=None)
    refused(b"null first", count=None)
    for gop in (0, -1, 65536):
        refused(b"gop", gop=gop)
    for first in (-4, 1, 2, 3, 5, 6):
        refused(b"first", first=(first,), count=(1,))
    refused(b"first", gop=5, first=(4,), count=(1,))
    for count in (0, -1):
        refused(b"count", count=(count,))
    refused(b"count", count=(8,), T_max=7)                       # count > T_max
    refused(b"beyond", first=(8,), count=(5,))                   # first + count > T
    refused(b"beyond", first=(12,), count=(1,))
    refused(b"beyond", first=(0,), count=(13,), T_max=13)
    for T_max in (0, -1, 65536):
        refused(b"T_out", T_max=T_max)
    a, arr = make(2)
    assert call(a, first=(0, 4), count=(8, 9), T_max=9) == -1 and b"clip 1" in lib.flk_last_error() and b"beyond" in lib.flk_last_error()
    for n in (0, -1, 65):
        a, arr = make()
        a.nclip = n
        refused(b"nclip", a)
    for q in (0, 101):
        a, arr = make()
        a.quality = q
        refused(b"quality", a)
    a, arr = make()
    a.subsampling = 422
    refused(b"subsampling", a)
    a, arr = make()
    a.clips = C.POINTER(_lib.CodecClip)()
    refused(b"null clip list", a)
    for field, value, word in (("src", None, b"null"), ("dst", None, b"null"), ("T", 0, b"size"), ("Hs", 0, b"size"), ("pitch_h", 119, b"source pitches"),
                               ("pitch_t", 0, b"source pitches"), ("dst_pitch_h", 119, b"destination pitches"),
                               ("dst_pitch_t", 0, b"destination pitches"), ("dst", 0x10000, b"destination is the source")):
        a, arr = make(2)
        setattr(arr[1], field, value)
        assert call(a, first=(4, 4), count=(8, 8)) == -1 and word in lib.flk_last_error(), (field, lib.flk_last_error())
        assert b"clip 1" in lib.flk_last_error() and b"flk_codec_roundtrip_gop_u8" in lib.flk_last_error()
    a, arr = make()
    arr[0].Hs, arr[0].Ws, arr[0].pitch_h, arr[0].dst_pitch_h = 1600, 1600, 4800, 4800            # 2 560 000 pixels: above the GOP entry's bound
    refused(b"stats", a, stats=C.c_void_p(0x200000))


def test_python_wrapper_refuses_before_touching_a_device():
    torch = pytest.importorskip("torch")
    from flickering_adversarial_video_amd import ops
    host = torch.zeros((6, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.codec_roundtrip([host], vs.Codec(gop=3))
    assert ops.codec_inter_step(50) == 16
