"""Motion-compensated P-frames in the codec without a GPU: the numpy integer restatement
(videoresnet_spec.codec_roundtrip_host(gop=, search=, motion=) and codec_motion_search, the definition of flk_codec_roundtrip_mc_u8), the
tie rule of the search, what the search is for (a flicker on moving content), ``Codec(search=)`` and ``--codec-search``, the coverage
of the GPU test's fixtures, and the argument contract of the new ABI entries (nothing here launches anything)."""
import argparse
import ctypes as C

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

import codec_mc_cases as cases

SUBS = cases.SUBS


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_search_0_is_the_zero_motion_codec(sub):
    for (H, W), q, gop in (((8, 8), 1, 2), ((17, 23), 50, 3), ((33, 40), 75, 7), ((16, 48), 100, 4)):
        x = cases.moving(7, H, W, seed=H)
        o, st = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=gop)
        o0, st0, mv = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=gop, search=0, motion=True)
        m = 8 if sub == "444" else 16
        Hp, Wp = -(-H // m) * m, -(-W // m) * m
        assert (o == o0).all() and (st == st0).all() and mv.dtype == np.int8 and mv.shape == (7, -(-Hp // 16), -(-Wp // 16), 2) and not mv.any()
        assert (vs.codec_roundtrip_host(x, q, sub, gop=gop, search=0) == o).all()


@pytest.mark.parametrize("sub", SUBS)
def test_intra_frames_spans_and_returns(sub):
    gop, q, R = 3, 60, 5
    x = cases.moving(8, 24, 40, seed=7)
    o, st, mv = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=gop, search=R, motion=True)
    o2, mv2 = vs.codec_roundtrip_host(x, q, sub, gop=gop, search=R, motion=True)
    assert (o == o2).all() and (mv == mv2).all() and (vs.codec_roundtrip_host(x, q, sub, gop=gop, search=R) == o).all()
    intra, intra_st = vs.codec_roundtrip_host(x, q, sub, stats=True)
    for n in range(0, 8, gop):                                     # an intra frame is the intra call on that frame, with zero vectors
        assert (o[n] == intra[n]).all() and (st[n] == intra_st[n]).all() and not mv[n].any()
    assert mv.any() and np.abs(mv).max() <= R
    for k, count in ((1, 5), (2, 2), (1, 1)):                      # a span that starts on an intra frame is the whole video's result, sliced
        so, sst, smv = vs.codec_roundtrip_host(x[k * gop:k * gop + count], q, sub, stats=True, gop=gop, first_frame=k * gop, search=R, motion=True)
        assert (so == o[k * gop:k * gop + count]).all() and (sst == st[k * gop:k * gop + count]).all() and (smv == mv[k * gop:k * gop + count]).all()
    one, mv1 = vs.codec_roundtrip_host(x[0], q, sub, gop=gop, search=R, motion=True)            # a single frame
    assert (one == o[0]).all() and mv1.shape == mv.shape[1:]
    for bad in (-1, 16, 2.0, True, None):
        with pytest.raises(ValueError, match="search"):
            vs.codec_roundtrip_host(x[:2], q, sub, gop=gop, search=bad)
    with pytest.raises(ValueError, match="needs gop > 1"):
        vs.codec_roundtrip_host(x[:2], q, sub, search=3)


def test_prediction_is_the_definition_pixel_by_pixel():
    """_codec_mc_predict against loops written from the definition: full-pel luma, 4:4:4 chroma with the same vector, 4:2:0 chroma with
    half the vector (arithmetic shift, the three averaging rules), every read clamped"""
    rng = np.random.RandomState(3)
    Hp, Wp = 32, 48
    Y, Cb, Cr = (rng.randint(0, 256, (Hp, Wp)).astype(np.int32) for _ in range(3))
    cb2, cr2 = (rng.randint(0, 256, (Hp // 2, Wp // 2)).astype(np.int32) for _ in range(2))
    mv = np.array([[(-3, 3), (0, 0), (15, -15)], [(2, -1), (-1, -1), (7, 8)]], np.int8)
    cl = lambda v, n: min(max(v, 0), n - 1)
    pY, pCb, pCr = vs._codec_mc_predict((Y, Cb, Cr), mv, False)
    qY, qCb, qCr = vs._codec_mc_predict((Y, cb2, cr2), mv, True)
    assert (pY == qY).all()
    for y in range(Hp):
        for x in range(Wp):
            dy, dx = (int(v) for v in mv[y // 16, x // 16])
            assert pY[y, x] == Y[cl(y + dy, Hp), cl(x + dx, Wp)] and pCb[y, x] == Cb[cl(y + dy, Hp), cl(x + dx, Wp)] and pCr[y, x] == Cr[cl(y + dy, Hp), cl(x + dx, Wp)]
    Hc, Wc = Hp // 2, Wp // 2
    for y in range(Hc):
        for x in range(Wc):
            dy, dx = (int(v) for v in mv[y // 8, x // 8])
            iy, hy, ix, hx = dy >> 1, dy & 1, dx >> 1, dx & 1
            for p, q in ((cb2, qCb), (cr2, qCr)):
                a, b, c, d = (p[cl(y + iy + j, Hc), cl(x + ix + i, Wc)] for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)))
                want = (a + b + c + d + 2) >> 2 if hy and hx else (a + b + 1) >> 1 if hx else (a + c + 1) >> 1 if hy else a
                assert q[y, x] == want, (y, x, dy, dx)
    assert (-3 >> 1, -3 & 1) == (-2, 1)                            # -3 is -2 + 1/2


# ---- the tie rule ---------------------------------------------------------------------------------------------------------------
def test_search_serial_rule_is_the_key_minimum():
    """codec_motion_search against the serial rule as the definition words it: (0, 0) first, then dy outer, dx inner, replace only if
    strictly smaller; macroblocks of 16 and of 8 at the plane's end"""
    rng = np.random.RandomState(9)
    Hp, Wp, R = 24, 40, 3
    ref = rng.randint(0, 256, (Hp, Wp))
    cur = np.roll(ref, (2, -1), (0, 1))
    cur[:8] = 77                                                   # and a part where nothing matches well
    got = vs.codec_motion_search(cur, ref, R)
    assert got.shape == (2, 3, 2) and got.dtype == np.int8
    cl = lambda v, n: min(max(v, 0), n - 1)
    for my in range(2):
        for mx in range(3):
            def sad(dy, dx):
                return sum(abs(int(cur[y, x]) - int(ref[cl(y + dy, Hp), cl(x + dx, Wp)]))
                           for y in range(my * 16, min(my * 16 + 16, Hp)) for x in range(mx * 16, min(mx * 16 + 16, Wp)))
            best, vec = sad(0, 0), (0, 0)
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    s = sad(dy, dx)
                    if s < best:
                        best, vec = s, (dy, dx)
            assert tuple(got[my, mx]) == vec, (my, mx)


def test_tie_rule_flat_and_stripes():
    for R in (0, 1, 7, 15):                                        # every candidate ties: the zero vector, visited first, stays
        assert not vs.codec_motion_search(np.full((24, 40), 9), np.full((24, 40), 200), R).any()
    Hp, Wp = 64, 96
    x = np.arange(Wp)
    ref = np.broadcast_to(64 + 128 * ((x % 8) < 4), (Hp, Wp))
    cur = np.broadcast_to(64 + 128 * (((x + 3) % 8) < 4), (Hp, Wp))
    mv = vs.codec_motion_search(cur, ref, 7)
    # SAD 0 at dx = 3 and -5 for every dy: the first visited is dy = -7, dx = -5; the zero vector (SAD > 0) does not hold its place
    assert (mv[:, 1:] == (-7, -5)).all()
    assert (mv[:, 0] != (-7, -5)).any(axis=-1).all()               # the left column reads clamped samples at dx = -5: another winner
    for bad in (np.zeros((4, 4)), np.zeros((2, 4, 4), int), np.full((4, 4), 256)):
        with pytest.raises(ValueError):
            vs.codec_motion_search(bad, bad, 2)
    with pytest.raises(ValueError):
        vs.codec_motion_search(np.zeros((4, 4), int), np.zeros((4, 8), int), 2)
    for bad in (-1, 16, True, 1.0):
        with pytest.raises(ValueError, match="search"):
            vs.codec_motion_search(ref, ref, bad)


@pytest.mark.parametrize("sub", SUBS)
def test_stripes_through_the_whole_codec(sub):
    """at quality 75 the reconstruction keeps the stripes sharp enough for the same winner in every interior macroblock"""
    _, mv = vs.codec_roundtrip_host(cases.stripes(4, 64, 96), 75, sub, gop=4, search=7, motion=True)
    assert (mv[1:, :, 1:] == (-7, -5)).all()


# ---- pans -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("q", [50, 75, 90])
def test_the_search_finds_a_pan(q, sub):
    for v in ((0, 2), (1, -3), (-3, 3), (4, -4)):
        x = cases.pan(6, 72, 104, *v)
        _, s0 = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=6)
        _, s1, mv = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=6, search=4, motion=True)
        assert (mv[1:, 1:-1, 1:-1] == v).all(), (q, sub, v)         # every interior macroblock of every P-frame
        print(f"q {q} {sub} pan {v}: P-frame levels {int(s0[1:, 0].sum())} at zero motion, {int(s1[1:, 0].sum())} with search 4")
        assert (s1[1:, 0] < s0[1:, 0]).all()


# ---- what the model is for ------------------------------------------------------------------------------------------------------
def arrived(x, q, sub, R, gop=6):
    """the fraction of a +-1 flicker on the P-frames that arrives: mean over P-frames of the delivered difference to the unflickered
    run, in the flicker's direction"""
    f = x.astype(int)
    sign = np.where(np.arange(len(x)) % 2 == 1, 1, -1)
    sign[0] = 0
    f += sign[:, None, None, None]
    a = vs.codec_roundtrip_host(x, q, sub, gop=gop, search=R).astype(int)
    b = vs.codec_roundtrip_host(np.clip(f, 0, 255).astype(np.uint8), q, sub, gop=gop, search=R).astype(int)
    return float(((b - a) * sign[:, None, None, None])[1:].mean())


@pytest.mark.parametrize("sub", SUBS)
def test_flicker_on_a_panning_clip_arrives_whole_only_without_compensation(sub):
    """quality 50, +-1 on the P-frames: at least 0.85 arrives at zero motion, at most 0.70 with search 4.  Measured on this texture, 4:4:4 /
    4:2:0: pan (0, 2) 0.930 / 0.932 and 0.516 / 0.532; (1, -3) 0.858 / 0.850 and 0.529 / 0.550; (-3, 3) 0.917 / 0.919 and 0.571 / 0.635.
    The fraction is a statistic of a small clip and moves with the texture sample"""
    for v in ((0, 2), (1, -3), (-3, 3)):
        x = cases.pan(6, 72, 104, *v)
        zero, comp = arrived(x, 50, sub, 0), arrived(x, 50, sub, 4)
        print(f"q 50 {sub} pan {v}: arrived {zero:.3f} at zero motion, {comp:.3f} with search 4")
        assert zero >= 0.85 and comp <= 0.70, (sub, v, zero, comp)


@pytest.mark.parametrize("sub", SUBS)
def test_flicker_on_flat_grey_is_still_erased(sub):
    x = np.full((9, 16, 16, 3), 128, np.int64)
    x[1::2] += 1
    x[2::2] -= 1
    o, st, mv = vs.codec_roundtrip_host(x.astype(np.uint8), 50, sub, stats=True, gop=9, search=7, motion=True)
    assert (st[1:] == 0).all() and (o == 128).all() and not mv.any()


# ---- int32 is enough ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_int32_is_enough_at_the_extremes(sub):
    """the prediction is made of bytes, so the bounds of the zero-motion P-frame hold: int64 beside int32 on its saturated contents"""
    rng = np.random.RandomState(5)
    H, W = 24, 32
    yy, xx = np.mgrid[0:H, 0:W]
    checker = lambda inv: np.repeat(((((yy + xx + inv) & 1)) * 255).astype(np.uint8)[..., None], 3, -1)
    videos = {"checker": np.stack([checker(n & 1) for n in range(6)]), "flat": np.stack([np.full((H, W, 3), 255 * (n & 1), np.uint8) for n in range(6)]),
              "random": rng.choice(np.array([0, 255], np.uint8), (6, H, W, 3))}
    for name, x in videos.items():
        for q in (1, 25, 50, 75, 100):
            r32 = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=4, search=7, motion=True)
            r64 = vs.codec_roundtrip_host(x, q, sub, stats=True, gop=4, search=7, motion=True, _dtype=np.int64)
            assert all((a == b).all() for a, b in zip(r32, r64)), (name, q)
    # the checkerboard against its inverse is found one pixel aside: the search turns the largest residual into none
    _, st, mv = vs.codec_roundtrip_host(videos["checker"], 100, "444", stats=True, gop=4, search=7, motion=True)
    assert mv[1].any()


# ---- the GPU test's fixtures ----------------------------------------------------------------------------------------------------
def test_gpu_fixtures_cover_what_the_kernel_can_get_wrong():
    """over the cases tests/test_codec_mc_gpu.py runs, the restated vectors hold the zero vector, both signs of both components, odd
    and even components, a component of magnitude R, and chosen blocks whose reads are clamped at each of the four plane edges"""
    seen = set()
    for size in cases.SIZES:
        for sub in SUBS:
            for content, q, gop, R in cases.COMBOS:
                _, mv = vs.codec_roundtrip_host(cases.case_videos(content, size, R)[1], q, sub, gop=gop, search=R, motion=True)
                m = 8 if sub == "444" else 16
                Hp, Wp = -(-size[0] // m) * m, -(-size[1] // m) * m
                dy, dx = mv[..., 0].astype(int), mv[..., 1].astype(int)
                seen |= {"zero"} if ((dy == 0) & (dx == 0))[1:].any() else set()
                for name, v in (("dy", dy), ("dx", dx)):
                    seen |= {f"{name}{w}" for w, hit in (("<0", v < 0), (">0", v > 0), (" odd", v % 2 == 1), (" even", (v % 2 == 0) & (v != 0))) if hit.any()}
                    seen |= {"magnitude R"} if (np.abs(v) == R).any() else set()
                seen |= {"top"} if (dy[:, 0] < 0).any() else set()
                seen |= {"left"} if (dx[:, :, 0] < 0).any() else set()
                y_end = np.minimum(np.arange(mv.shape[1]) * 16 + 16, Hp)[None, :, None]
                x_end = np.minimum(np.arange(mv.shape[2]) * 16 + 16, Wp)[None, None, :]
                seen |= {"bottom"} if (y_end - 1 + dy > Hp - 1).any() else set()
                seen |= {"right"} if (x_end - 1 + dx > Wp - 1).any() else set()
    want = {"zero", "dy<0", "dy>0", "dx<0", "dx>0", "dy odd", "dy even", "dx odd", "dx even", "magnitude R", "top", "left", "bottom", "right"}
    assert seen == want, want - seen


# ---- Codec and the scripts' options ---------------------------------------------------------------------------------------------
def test_codec_value_semantics():
    c = vs.Codec(60, "444", gop=12, search=7)
    assert (c.quality, c.subsampling, c.gop, c.search) == (60, "444", 12, 7) and vs.Codec().search == 0 and vs.Codec(gop=4).search == 0
    assert vs.Codec(60, "444", 12, 7) == c and c != vs.Codec(60, "444", gop=12) and c != vs.Codec(60, "444", gop=12, search=6)
    assert vs.Codec(60, "444", gop=12, search=0) == vs.Codec(60, "444", gop=12)
    assert hash(c) == hash(vs.Codec(60, "444", gop=12, search=7)) and len({c, vs.Codec(60, "444", gop=12), vs.Codec(60, "444", gop=12, search=0)}) == 2
    assert repr(c) == "Codec(quality=60, subsampling='444', gop=12, search=7)" and eval(repr(c), {"Codec": vs.Codec}) == c
    assert repr(vs.Codec(60, "444", gop=12)) == "Codec(quality=60, subsampling='444', gop=12)"
    assert repr(vs.Codec(60, "444")) == "Codec(quality=60, subsampling='444')"
    with pytest.raises(AttributeError):
        c.search = 2
    for bad in (-1, 16, 2.5, True, None, "4"):
        with pytest.raises(ValueError, match="search"):
            vs.Codec(75, "420", gop=4, search=bad)
    for gop in (1,):
        with pytest.raises(ValueError, match="needs gop > 1"):
            vs.Codec(75, "420", gop=gop, search=1)
    with pytest.raises(ValueError, match="needs gop > 1"):
        vs.Codec(75, "420", search=7)
    assert vs.Codec(75, "420", gop=2, search=15).search == 15 and vs.Codec(75, "420", gop=2, search=np.int64(4)).search == 4
    assert vs.check_codec_search(7) == 7 and vs.check_codec_search(0, gop=1) == 0 and vs.check_codec_search(3, gop=2) == 3


def test_codec_search_option(capsys):
    def parse(argv, used=True):
        ap = argparse.ArgumentParser()
        vs.add_codec_arguments(ap)
        a = ap.parse_args(argv)
        return vs.codec_from_arguments(ap, a, used)

    assert parse(["--codec-quality", "60", "--codec-gop", "12"]) == vs.Codec(60, "420", gop=12)
    assert parse(["--codec-quality", "60", "--codec-gop", "12", "--codec-search", "7"]) == vs.Codec(60, "420", gop=12, search=7)
    assert parse(["--codec-quality", "60", "--codec-search", "0"]) == vs.Codec(60, "420")
    for argv, word in ((["--codec-search", "7"], "--codec-search needs --codec-quality"), (["--codec-quality", "60", "--codec-search", "7"], "gop > 1"),
                       (["--codec-quality", "60", "--codec-gop", "4", "--codec-search", "16"], "search"),
                       (["--codec-quality", "60", "--codec-gop", "4", "--codec-search", "x"], "--codec-search")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err, argv


# ---- the ABI (fake pointers, nothing launched) ------------------------------------------------------------------------------------
def make_args(n=1, sub=420, Hs=24, Ws=40):
    from flickering_adversarial_video_amd import _lib
    arr = (_lib.CodecClip * max(n, 1))()
    for d in arr:
        d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = 0x10000, 12, Hs, Ws, Hs * Ws * 3, Ws * 3
        d.dst, d.dst_pitch_t, d.dst_pitch_h = 0x900000, Hs * Ws * 3, Ws * 3
    a = _lib.CodecArgs()
    a.nclip, a.quality, a.subsampling, a.clips = n, 75, sub, arr
    a._keep = arr
    return a, arr


def ints(*v):
    return (C.c_int32 * len(v))(*v)


def test_scratch_bytes(lib):
    a, _ = make_args()                                             # 24 x 40 -> 32 x 48 at 4:2:0: 1536 + 2 * 384 bytes a set
    assert lib.flk_codec_mc_scratch_bytes(C.byref(a), 4, ints(8)) == 2 * 2 * 2304
    assert lib.flk_codec_mc_scratch_bytes(C.byref(a), 4, ints(9)) == 3 * 2 * 2304
    assert lib.flk_codec_mc_scratch_bytes(C.byref(a), 12, ints(1)) == 2 * 2304
    a, _ = make_args(sub=444)                                      # 24 x 40 stays: three planes of 960
    assert lib.flk_codec_mc_scratch_bytes(C.byref(a), 4, ints(8)) == 2 * 2 * 2880
    a, arr = make_args(2)
    arr[1].Hs, arr[1].Ws = 90, 82                                  # 96 x 96
    assert lib.flk_codec_mc_scratch_bytes(C.byref(a), 3, ints(7, 2)) == 3 * 2 * 2304 + 1 * 2 * (9216 + 2 * 2304)
    for bad in (lambda: lib.flk_codec_mc_scratch_bytes(None, 4, ints(8)), lambda: lib.flk_codec_mc_scratch_bytes(C.byref(a), 0, ints(7, 2)),
                lambda: lib.flk_codec_mc_scratch_bytes(C.byref(a), 3, None), lambda: lib.flk_codec_mc_scratch_bytes(C.byref(a), 3, ints(7, 0))):
        assert bad() == 0
    a.subsampling = 422
    assert lib.flk_codec_mc_scratch_bytes(C.byref(a), 3, ints(7, 2)) == 0


def test_mc_argument_contract_without_gpu(lib):
    WS, BIG = C.c_void_p(0x4000000), 1 << 30

    def call(a, gop=4, search=7, first=(4,), count=(8,), T_max=8, tone=None, stats=None, mv=None, mv_stride=0, scratch=WS, scratch_bytes=BIG):
        f = None if first is None else ints(*first)
        c = None if count is None else ints(*count)
        return lib.flk_codec_roundtrip_mc_u8(C.byref(a) if a is not None else None, gop, search, f, c, T_max, tone, stats, mv, mv_stride, scratch,
                                             scratch_bytes, None)

    def refused(word, a=None, **kw):
        a = make_args()[0] if a is None else a
        assert call(a, **kw) == -1 and word in lib.flk_last_error(), (kw, lib.flk_last_error())
        assert b"flk_codec_roundtrip_mc_u8" in lib.flk_last_error()

    assert call(None) == -1
    for search in (-1, 16, 100):
        refused(b"search", search=search)
    refused(b"scratch", scratch=None)
    refused(b"scratch", scratch=C.c_void_p(0x4000004))             # not 16-byte aligned
    need = 2 * 2 * 2304
    refused(b"scratch", scratch_bytes=need - 1)
    refused(b"scratch", scratch_bytes=0)
    refused(b"mv_stride", mv=C.c_void_p(0x5000000), mv_stride=5)    # 32 x 48 padded: 2 x 3 macroblocks
    refused(b"mv_stride", mv=C.c_void_p(0x5000000), mv_stride=0)
    a, arr = make_args(2)
    arr[1].Hs, arr[1].Ws, arr[1].pitch_h, arr[1].dst_pitch_h, arr[1].pitch_t, arr[1].dst_pitch_t = 90, 82, 246, 246, 90 * 246, 90 * 246
    assert call(a, first=(4, 4), count=(8, 8), mv=C.c_void_p(0x5000000), mv_stride=35) == -1 and b"clip 1" in lib.flk_last_error()
    # everything the GOP entry refuses
    refused(b"null first", first=None)
    refused(b"null first", count=None)
    for gop in (0, -1, 65536):
        refused(b"gop", gop=gop)
    for first in (-4, 1, 2, 3, 5, 6):
        refused(b"first", first=(first,), count=(1,))
    for count in (0, -1):
        refused(b"count", count=(count,))
    refused(b"count", count=(8,), T_max=7)
    refused(b"beyond", first=(8,), count=(5,))
    for T_max in (0, -1, 65536):
        refused(b"T_out", T_max=T_max)
    for n in (0, -1, 65):
        a, arr = make_args()
        a.nclip = n
        refused(b"nclip", a)
    for q in (0, 101):
        a, arr = make_args()
        a.quality = q
        refused(b"quality", a)
    a, arr = make_args()
    a.subsampling = 422
    refused(b"subsampling", a)
    for field, value, word in (("src", None, b"null"), ("dst", None, b"null"), ("T", 0, b"size"), ("Hs", 0, b"size"), ("pitch_h", 119, b"source pitches"),
                               ("pitch_t", 0, b"source pitches"), ("dst_pitch_h", 119, b"destination pitches"),
                               ("dst_pitch_t", 0, b"destination pitches"), ("dst", 0x10000, b"destination is the source")):
        a, arr = make_args(2)
        setattr(arr[1], field, value)
        assert call(a, first=(4, 4), count=(8, 8)) == -1 and word in lib.flk_last_error() and b"clip 1" in lib.flk_last_error(), (field, lib.flk_last_error())
    a, arr = make_args(Hs=1600, Ws=1600)                           # 2 560 000 pixels: above the bound stats are taken on
    refused(b"stats", a, stats=C.c_void_p(0x200000))


def test_python_wrapper_refuses_before_touching_a_device():
    torch = pytest.importorskip("torch")
    from flickering_adversarial_video_amd import ops
    host = torch.zeros((6, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.codec_roundtrip([host], vs.Codec(gop=3, search=7), motion=True)
