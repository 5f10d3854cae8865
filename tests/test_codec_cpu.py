"""The codec round trip without a GPU: the quantisation tables (restatement == library == a real JPEG encoder), the properties of the
numpy integer restatement (videoresnet_spec.codec_roundtrip_host, the kernel's definition), its closeness to Pillow's own JPEG round
trip, and the argument contract of flk_codec_roundtrip_u8 / ops.codec_roundtrip (nothing here launches anything)."""
import ctypes as C
import io

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

SUBS = ("444", "420")


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def smooth_frame(H=64, W=96, seed=0):
    """smooth luminance and chroma plus mild noise, inside 30..225 (nothing saturates)"""
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.RandomState(seed)
    img = np.stack([128 + 60 * np.sin(xx / 17.) + 40 * np.cos(yy / 11.), 120 + 50 * np.cos(xx / 23. + yy / 13.),
                    100 + 70 * np.sin(yy / 19.) - 20 * np.cos(xx / 7.)], -1) + rng.normal(0, 6, (H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


# ---- tables -------------------------------------------------------------------------------------------------------------------
def test_tables_equal_the_library_at_every_quality(lib):
    for q in range(1, 101):
        ql, qc = (C.c_int32 * 64)(), (C.c_int32 * 64)()
        assert lib.flk_codec_tables(q, ql, qc) == 0
        sl, sc = vs.codec_tables(q)
        assert sl.dtype == np.int32 and sl.shape == (64,)
        assert list(ql) == sl.tolist() and list(qc) == sc.tolist(), q
        assert 1 <= min(sl.min(), sc.min()) and max(sl.max(), sc.max()) <= 255
    assert vs.codec_tables(50)[0].tolist() == list(vs.CODEC_BASE_LUMA) and vs.codec_tables(50)[1].tolist() == list(vs.CODEC_BASE_CHROMA)
    assert set(vs.codec_tables(100)[0].tolist()) == {1}
    for bad in (0, 101, -3):
        assert lib.flk_codec_tables(bad, (C.c_int32 * 64)(), (C.c_int32 * 64)()) == -1 and b"quality" in lib.flk_last_error()
        with pytest.raises(ValueError):
            vs.codec_tables(bad)
    assert lib.flk_codec_tables(50, None, (C.c_int32 * 64)()) == -1


# zig-zag scan of an 8x8 block (ITU T.81 figure A.6): position in the scan -> row-major index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def test_tables_equal_the_ones_pillow_writes():
    """a JPEG written by Pillow at quality q carries exactly codec_tables(q).  Pillow hands the tables back either row-major or in the
    file's zig-zag order, depending on its version: which one is read off the (asymmetric) base table at quality 50, once"""
    pytest.importorskip("PIL")
    from PIL import Image

    def written(q):
        b = io.BytesIO()
        Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, "JPEG", quality=q, subsampling=0)
        b.seek(0)
        t = Image.open(b).quantization
        return list(t[0]), list(t[1])

    base = list(vs.CODEC_BASE_LUMA)
    got = written(50)[0]
    natural = got == base
    assert natural or got == [base[i] for i in ZIGZAG]

    def row_major(t):
        if natural:
            return t
        out = [0] * 64
        for pos, i in enumerate(ZIGZAG):
            out[i] = t[pos]
        return out

    for q in range(1, 101):
        pl, pc = written(q)
        sl, sc = vs.codec_tables(q)
        assert row_major(pl) == sl.tolist() and row_major(pc) == sc.tolist(), q


# ---- properties of the restatement ---------------------------------------------------------------------------------------------
def test_constant_frames():
    """What holds of a constant frame.  It has no AC energy, so the round trip returns a CONSTANT frame at every quality; its value is the
    input's only where the DC step divides it -- 8 (v - 128) is a multiple of Q_dc -- so mid-grey (all coefficients 0) is a fixed point at
    every quality, every grey level is one at quality 100 (Q = 1; a grey converts to Y = v, Cb = Cr = 128 exactly), and a grey v
    elsewhere comes back as a grey within Q_dc / 16 + 1 of v (half a DC step, in pixels, and the inverse's rounding)."""
    for sub in SUBS:
        for q in range(1, 101):
            g = np.full((2, 9, 13, 3), 128, np.uint8)
            assert (vs.codec_roundtrip_host(g, q, sub) == g).all(), (q, sub)
            c = np.empty((1, 9, 13, 3), np.uint8)
            c[...] = (77, 200, 31)
            o = vs.codec_roundtrip_host(c, q, sub)
            assert (o == o[:, :1, :1]).all(), (q, sub)
            v = (q * 37) % 256
            o = vs.codec_roundtrip_host(np.full((17, 23, 3), v, np.uint8), q, sub).astype(int)
            assert (o == o[0, 0, 0]).all() and abs(int(o[0, 0, 0]) - v) <= vs.codec_tables(q)[0][0] / 16 + 1, (q, sub, v, o[0, 0])
        greys = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None, None], 8, 1).repeat(8, 2).repeat(3, 3)
        assert (vs.codec_roundtrip_host(greys, 100, sub) == greys).all()


def test_quality_100_error_bound_on_a_smooth_frame():
    """quality 100, 4:4:4: Q = 1 everywhere, so only roundings remain.  Per plane: the colour transform rounds by <= 0.51; each of the 64
    coefficients is off by <= 0.5 (its rounding to a level) + 0.25 (the forward integer transform, accurate to 2 of its 1/8 units), an
    error vector of norm <= 8 * 0.75 = 6, which an orthonormal inverse spreads to at most 6 on one pixel; the inverse integer
    transform adds <= 1 (its peak error) -- 7.51 per plane.  The worst channel is B = Y + 1.772 Cb: 2.772 * 7.51 + 0.51 < 22."""
    x = smooth_frame()
    o = vs.codec_roundtrip_host(x, 100, "444")
    err = np.abs(o.astype(int) - x.astype(int))
    print("quality 100 4:4:4 smooth frame: max byte error", err.max(), "mean", err.mean())
    assert err.max() <= 22


def test_second_round_trip_changes_few_bytes():
    """measured, not asserted: the share of bytes a second round trip at the same settings changes (recorded in DESIGN.md 10.8)"""
    x = smooth_frame()
    for q in (50, 75, 100):
        for sub in SUBS:
            o = vs.codec_roundtrip_host(x, q, sub)
            o2 = vs.codec_roundtrip_host(o, q, sub)
            print(f"q {q} {sub}: second round trip changes {(o2 != o).mean():.4f} of the bytes, max {np.abs(o2.astype(int) - o.astype(int)).max()}")
            assert o2.shape == o.shape and o2.dtype == np.uint8


def test_odd_sizes_single_frames_and_stats():
    rng = np.random.RandomState(1)
    for shape in ((1, 1), (1, 9), (7, 1), (17, 23), (8, 8), (16, 16), (24, 40), (33, 16)):
        x = rng.randint(0, 256, (2,) + shape + (3,)).astype(np.uint8)
        for sub in SUBS:
            o, st = vs.codec_roundtrip_host(x, 75, sub, stats=True)
            assert o.shape == x.shape and o.dtype == np.uint8 and st.shape == (2, 2) and st.dtype == np.int32
            assert (st[:, 1] >= st[:, 0]).all() and (st[:, 0] >= 0).all()
            one = vs.codec_roundtrip_host(x[1], 75, sub)
            assert one.shape == x.shape[1:] and (one == o[1]).all()               # frames are independent; a single frame is taken too
    # a 1 x 1 frame is its colour replicated over one MCU: the constant-frame result
    p = np.array([[[3, 250, 100]]], np.uint8)
    for sub in SUBS:
        assert (vs.codec_roundtrip_host(p, 90, sub) == vs.codec_roundtrip_host(np.broadcast_to(p, (16, 16, 3)).copy(), 90, sub)[:1, :1]).all()
    # the tone table is applied first
    x = rng.randint(0, 256, (2, 9, 12, 3)).astype(np.uint8)
    tone = rng.randint(0, 256, (2, 256, 3)).astype(np.uint8)
    toned = np.stack([np.stack([tone[n, :, c][x[n, ..., c]] for c in range(3)], -1) for n in range(2)])
    assert (vs.codec_roundtrip_host(x, 60, "420", tone=tone) == vs.codec_roundtrip_host(toned, 60, "420")).all()
    ident = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    assert (vs.codec_roundtrip_host(x, 60, "420", tone=ident) == vs.codec_roundtrip_host(x, 60, "420")).all()


def test_checkerboard_saturates_without_wrap_and_fits_int32():
    """the 0 / 255 checkerboard carries the largest AC energy a frame can: coarse quantisation overshoots 0..255 and the clamps hold it
    (no wrap-around: every output byte lies within the reach of the quantisation error of its source byte at quality 100, and the int32
    run equals the int64 run at every quality, i.e. no intermediate left an int32)"""
    rng = np.random.RandomState(2)
    extreme = rng.choice(np.array([0, 255], np.uint8), (17, 23, 3))            # independent per channel: saturated chroma as well
    for x in (checkerboard(17, 23), checkerboard(16, 16), extreme):
        for sub in SUBS:
            for q in (1, 5, 25, 50, 75, 95, 100):
                o32, s32 = vs.codec_roundtrip_host(x, q, sub, stats=True)
                o64, s64 = vs.codec_roundtrip_host(x, q, sub, stats=True, _dtype=np.int64)
                assert (o32 == o64).all() and (s32 == s64).all(), (q, sub)
        o = vs.codec_roundtrip_host(x, 100, "444").astype(int)
        assert np.abs(o - x.astype(int)).max() <= 22                            # (the quality-100 bound above): a wrapped byte is ~255 off


# ---- closeness to a real JPEG round trip ---------------------------------------------------------------------------------------
# mean / max absolute difference to Pillow's round trip of smooth_frame(), measured once: 4:4:4 is bit equal;
# 4:2:0 differs because Pillow's decoder interpolates the chroma ("fancy upsampling") where this codec replicates it
PILLOW_420_MEAN = {50: 1.3095, 75: 1.2549}


@pytest.mark.parametrize("q", [50, 75])
def test_close_to_pillow(q):
    pytest.importorskip("PIL")
    from PIL import Image
    x = smooth_frame()
    for sub, pil_sub in (("444", 0), ("420", 2)):
        b = io.BytesIO()
        Image.fromarray(x).save(b, "JPEG", quality=q, subsampling=pil_sub)
        b.seek(0)
        pil = np.asarray(Image.open(b).convert("RGB")).astype(int)
        loss = np.abs(pil - x.astype(int)).mean()
        assert loss >= 1.0, (q, sub, loss)                                      # the fixture is one the codec really changes
        d = np.abs(vs.codec_roundtrip_host(x, q, sub).astype(int) - pil)
        print(f"q {q} {sub}: |restatement - Pillow| mean {d.mean():.4f} max {d.max()}; |Pillow - source| mean {loss:.4f}")
        assert d.mean() < loss, (q, sub)
        if sub == "444":
            assert d.max() == 0                                                 # the recommended arithmetic is the encoder's and decoder's own
        else:
            assert d.mean() <= PILLOW_420_MEAN[q] + 0.25


# ---- argument contract (fake pointers, nothing launched) -----------------------------------------------------------------------
def test_argument_contract_without_gpu(lib):
    from flickering_adversarial_video_amd import _lib

    def make(n=1, **over):
        arr = (_lib.CodecClip * max(n, 1))()
        for d in arr:
            d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = 0x10000, 4, 24, 40, 24 * 120, 120
            d.dst, d.dst_pitch_t, d.dst_pitch_h = 0x90000, 24 * 120, 120
        a = _lib.CodecArgs()
        a.nclip, a.quality, a.subsampling, a.clips = n, 75, _lib.FLK_CODEC_420, arr
        a._keep = arr
        return a, arr

    def call(a, idx=None, T_out=4, tone=None, stats=None):
        return lib.flk_codec_roundtrip_u8(C.byref(a) if a is not None else None, idx, T_out, tone, stats, None)

    assert call(None) == -1
    a, arr = make()
    a.clips = C.POINTER(_lib.CodecClip)()
    assert call(a) == -1 and b"null clip list" in lib.flk_last_error()
    for n in (0, -1, 65):
        a, arr = make()
        a.nclip = n
        assert call(a) == -1 and b"nclip" in lib.flk_last_error()
    for q in (0, 101, -5):
        a, arr = make()
        a.quality = q
        assert call(a) == -1 and b"quality" in lib.flk_last_error()
    for s in (0, 422, 411, 1):
        a, arr = make()
        a.subsampling = s
        assert call(a) == -1 and b"subsampling" in lib.flk_last_error()
    for T_out in (0, -1, 65536):
        a, arr = make()
        assert call(a, T_out=T_out) == -1 and b"T_out" in lib.flk_last_error()
    a, arr = make()
    assert call(a, T_out=5) == -1 and b"T_out" in lib.flk_last_error()         # more frames than the view, no frame table
    for field, value, word in (("src", None, b"null"), ("dst", None, b"null"), ("T", 0, b"size"), ("Hs", 0, b"size"), ("Ws", -2, b"size"),
                               ("pitch_h", 119, b"source pitches"), ("pitch_h", 0, b"source pitches"), ("pitch_t", 0, b"source pitches"),
                               ("pitch_t", -8, b"source pitches"), ("dst_pitch_h", 119, b"destination pitches"),
                               ("dst_pitch_h", -120, b"destination pitches"), ("dst_pitch_t", 0, b"destination pitches"),
                               ("dst", 0x10000, b"destination is the source")):
        a, arr = make(2)
        setattr(arr[1], field, value)
        assert call(a) == -1 and word in lib.flk_last_error(), (field, lib.flk_last_error())
        assert b"clip 1" in lib.flk_last_error()
    a, arr = make()
    arr[0].Hs, arr[0].Ws, arr[0].pitch_h, arr[0].dst_pitch_h = 2400, 2400, 7200, 7200
    assert call(a, stats=C.c_void_p(0x200000)) == -1 and b"stats" in lib.flk_last_error()


def test_python_wrapper_refuses_before_touching_a_device():
    torch = pytest.importorskip("torch")
    from flickering_adversarial_video_amd import ops
    host = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="Codec"):
        ops.codec_roundtrip([host], (75, "420"))
    with pytest.raises(ValueError, match="non-empty list"):
        ops.codec_roundtrip([], vs.Codec())
    with pytest.raises(ValueError, match="non-empty list"):
        ops.codec_roundtrip(host, vs.Codec())
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.codec_roundtrip([host], vs.Codec())
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.codec_roundtrip([np.zeros((2, 8, 8, 3), np.uint8)], vs.Codec())
    for q, s in ((0, "420"), (101, "444"), (75.0, "420"), (True, "420"), (75, "422"), (75, None)):
        with pytest.raises(ValueError):
            vs.Codec(q, s)
    c = vs.Codec()
    assert (c.quality, c.subsampling) == (75, "420") and vs.Codec(60, 444).subsampling == "444" and c == vs.Codec(75, "420")
    with pytest.raises(AttributeError):
        c.quality = 10
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((0, 4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            vs.codec_roundtrip_host(bad, 75, "420")
