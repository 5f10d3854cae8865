"""Training on the delivered video at its native resolution, on a machine without a GPU: the host restatements of the tone tables
(videoresnet_spec.tone_tables_host), their slopes and the gradient through the resampling (prepare_grad_host), and every refusal of the
three new entry points flk_clip_prepare_toned / flk_flicker_tone_slopes / flk_clip_prepare_grad -- FLK_EINVAL before any GPU call, with
fake pointers as in tests/test_stem_grad_contract_cpu.py: every call is valid in everything but the one thing under test, and no call
here passes a fully valid argument set, so nothing is ever launched."""
import ctypes as C
import math

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

GOOD = 0x10000            # 16-byte aligned, never dereferenced
EINVAL = -1
F32, BF16 = 0, 1


# ---- tone tables ---------------------------------------------------------------------------------------------------------------------
def all_levels_clip(n, T, seed):
    """uint8 [n,T,16,16,3]: every frame holds all 256 levels in every channel, in an order of its own"""
    rng = np.random.default_rng(seed)
    x = np.empty((n, T, 256, 3), np.uint8)
    for idx in np.ndindex(n, T, 3):
        x[idx[0], idx[1], :, idx[2]] = rng.permutation(256)
    return x.reshape(n, T, 16, 16, 3)


def through_tone(tone, x):
    """the clip x [n,T,H,W,3] mapped byte by byte through tone [n,T,256,3]"""
    n, T = x.shape[:2]
    k, t = np.arange(n)[:, None, None, None, None], np.arange(T)[None, :, None, None, None]
    return tone[k, t, x, np.arange(3)]


def clamp_range_in_bytes():
    """the bytes that lie inside the additive clamp in every channel: DESIGN.md section 10's table (lo and hi in levels per channel)"""
    lo, hi = vs.additive_bounds()
    mean, std = np.array(vs.DEFAULT_MEAN), np.array(vs.DEFAULT_STD)
    lo_levels, hi_levels = (lo * std + mean) * 255.0, (hi * std + mean) * 255.0
    return int(math.ceil(lo_levels.max())), int(math.floor(hi_levels.min()))


@pytest.mark.parametrize("amp", [0.0, 0.05, 0.6], ids=["zero", "small", "clamping"])
def test_tone_tables_additive_are_the_export_of_every_level(amp):
    from flickering_adversarial_video_amd import ops
    n, T = 2, 5
    rng = np.random.default_rng(3)
    delta = (rng.uniform(-1, 1, (n, T, 3)) * amp).astype(np.float32)
    tone = vs.tone_tables_host(delta, dclip=0.5)
    assert tone.shape == (n, T, 256, 3) and tone.dtype == np.uint8
    x = all_levels_clip(n, T, 11)
    lo, hi = vs.additive_bounds()
    want = ops.export_adversarial_u8_host(x, delta, dialect="torch", dclip=0.5, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo, hi=hi,
                                          x_lut=vs.u8_decode_table())
    assert np.array_equal(through_tone(tone, x), want)
    if amp == 0.0:
        b0, b1 = clamp_range_in_bytes()
        assert (b0, b1) == (10, 233)                                     # what the table of section 10 states
        ident = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], tone.shape)
        assert np.array_equal(tone[:, :, b0:b1 + 1], ident[:, :, b0:b1 + 1])
        assert not np.array_equal(tone, ident)                           # outside the range the clamp moves bytes even at delta = 0


@pytest.mark.parametrize("response", ["srgb", "linear"])
def test_tone_tables_illumination_are_the_export_of_every_level(response):
    n, T = 2, 4
    tables = vs.illum_tables(response)
    rng = np.random.default_rng(5)
    delta = rng.uniform(-0.3, 0.3, (n, T, 3)).astype(np.float32)
    tone = vs.tone_tables_host(delta, tables, dclip=0.2)
    x = all_levels_clip(n, T, 12)
    assert np.array_equal(through_tone(tone, x), vs.illum_export_host(x, delta, tables, dclip=0.2))
    ident = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], tone.shape)
    assert np.array_equal(vs.tone_tables_host(np.zeros_like(delta), tables), ident)      # no modulation: every byte comes back


def test_tone_slopes_host_masks_and_factors():
    n, T = 1, 3
    delta = np.array([[[0.0, 0.3, -0.3], [0.7, 0.0, 0.0], [0.1, -0.1, 0.2]]], np.float32)
    slope, scale = vs.tone_slopes_host(delta, dclip=0.5)
    assert slope.shape == (n, T, 256, 3) and scale.shape == (n, T, 3) and set(np.unique(slope)) <= {0.0, 1.0}
    inv_std = np.array([1.0 / s for s in vs.DEFAULT_STD]).astype(np.float32)
    assert np.array_equal(scale[0, 0], inv_std) and scale[0, 1, 0] == 0.0 and np.array_equal(scale[0, 1, 1:], inv_std[1:])
    b0, b1 = clamp_range_in_bytes()
    assert slope[0, 0, b0:b1 + 1, 0].all() and not slope[0, 0, :b0, 0].any()             # delta = 0: the clamp table itself
    assert slope[0, 0, :, 1].sum() < slope[0, 0, :, 0].sum()                             # +0.3 pushes bright bytes over the bound
    tables = vs.illum_tables("srgb")
    s2, sc2 = vs.tone_slopes_host(delta, tables, dclip=0.5)
    assert np.array_equal(sc2[0, 0], vs.illum_out_affine()[0]) and sc2[0, 1, 0] == 0.0
    assert (s2[0, 0, 1:, 0] > 0).all() and s2[0, 0, 255, 1] == 0.0                       # byte 255 lit by +0.3 leaves [0,1]


# ---- the gradient through the resampling against central differences of the unquantised chain ---------------------------------------
def chain(video, idx, delta, tables, box, flip, geom):
    """decode -> +delta or *(1 + m) -> curve -> resample -> normalise, float64, no clamp and no rounding: [T_out,Ho,Wo,3]"""
    mean, std = np.array(vs.DEFAULT_MEAN), np.array(vs.DEFAULT_STD)
    out = []
    for t, f in enumerate(idx):
        by = video[f]
        if tables is None:
            e = by / 255.0 + delta[t]                                    # the additive delta in display units: (delta / std) * std
        else:
            dec, enc = (np.asarray(a, np.float64) for a in tables)
            N = enc.shape[0] - 1
            z = dec[by, np.arange(3)] * (1.0 + delta[t]) * N
            i = np.minimum(np.floor(z).astype(np.int64), N - 1)
            e = enc[i] + (z - i) * (enc[i + 1] - enc[i])
        out.append((vs.prepare_resample_host(e, box, flip, **geom) - mean) / std)
    return np.stack(out)


GEOM = dict(im_scale=16, input_size=12, rule="sizes")
GRAD_CASES = [("eval", None, False), ("box_flip", (1, 2, 9, 13), True), ("direct_flip", (2, 3, 12, 12), True), ("box", (0, 0, 16, 21), False)]


@pytest.mark.parametrize("model", ["additive", "illumination"])
@pytest.mark.parametrize("name,box,flip", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_prepare_grad_host_is_the_derivative_of_the_unquantised_chain(model, name, box, flip):
    rng = np.random.default_rng(21)
    video = rng.integers(40, 200, (7, 24, 32, 3)).astype(np.uint8)     # away from the clamp edges of both models
    idx = np.array([0, 2, 2, 5, 6, 6])
    tables = vs.illum_tables("srgb") if model == "illumination" else None
    delta = rng.uniform(-0.05, 0.05, (idx.size, 3)).astype(np.float32)
    gx = rng.standard_normal((idx.size, 12, 12, 3))
    slope, scale = vs.tone_slopes_host(delta[None], tables, dclip=0.2)
    got = vs.prepare_grad_host(video, idx, gx, slope[0], scale[0], box, flip, **GEOM)
    h = 1e-7
    want = np.zeros_like(got)
    for t in range(idx.size):
        for c in range(3):
            dp, dm = delta.astype(np.float64), delta.astype(np.float64)
            dp[t, c] += h
            dm[t, c] -= h
            want[t, c] = ((chain(video, idx, dp, tables, box, flip, GEOM) - chain(video, idx, dm, tables, box, flip, GEOM)) * gx).sum() / (2 * h)
    # the slopes and factors are float32 numbers (1.2e-7 relative); the difference quotient of a piecewise-linear chain is exact up to
    # float64 rounding of the loss (1e-16 * |loss| / h, about 1e-7 here) and the rare value whose segment the step crosses
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())


def test_prepare_grad_host_zero_outside_the_delta_clamp():
    rng = np.random.default_rng(2)
    video = rng.integers(0, 256, (3, 24, 32, 3)).astype(np.uint8)
    delta = np.array([[[0.3, 0.0, 0.0], [0.0, 0.0, -0.3]]], np.float32)
    slope, scale = vs.tone_slopes_host(delta, dclip=0.2)
    g = vs.prepare_grad_host(video, [0, 2], rng.standard_normal((2, 12, 12, 3)), slope[0], scale[0], **GEOM)
    assert g[0, 0] == 0.0 and g[1, 2] == 0.0 and (g[0, 1:] != 0).all()


# ---- refusals of the three entry points ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def p(addr):
    return C.c_void_p(addr)


def refused(lib, rc, *words):
    msg = lib.flk_last_error().decode()
    assert rc == EINVAL, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def prep_args(nclip=2, T_out=8, Ho=12, Wo=12):
    from flickering_adversarial_video_amd import _lib
    clips = (_lib.PrepClip * max(nclip, 1))()
    for c in clips:
        c.src, c.T, c.Hs, c.Ws, c.pitch_t, c.pitch_h = GOOD, 20, 24, 32, 24 * 32 * 3, 32 * 3
        c.Hr, c.Wr, c.step_h, c.step_w, c.crop_i, c.crop_j = 16, 21, 1.5, 1.5238, 2, 4
    a = _lib.PrepareArgs()
    a.nclip, a.Ho, a.Wo = nclip, Ho, Wo
    a.mean, a.std = (C.c_float * 3)(*vs.DEFAULT_MEAN), (C.c_float * 3)(*vs.DEFAULT_STD)
    a.out_clip_offset, a.out_clip_stride = 0, T_out * Ho * Wo * 3
    a.clips = clips
    a._keep = clips
    return a


def boxes_of(n, **kw):
    from flickering_adversarial_video_amd import _lib
    b = (_lib.PrepBox * n)()
    for x in b:
        x.i, x.j, x.h, x.w, x.flip = 1, 2, 9, 13, 1
        for k, v in kw.items():
            setattr(x, k, v)
    return b


def shared_prepare_refusals():
    """(name, mutate(args), boxes or None, T_out, words): everything flk_clip_prepare_sampled refuses of a / boxes / T_out"""
    def setc(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a.clips[1], k, v)
        return f

    def seta(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a, k, v)
        return f
    return [
        ("nclip0", seta(nclip=0), None, 8, ("nclip",)), ("nclip65", seta(nclip=65), None, 8, ("nclip",)),
        ("Ho0", seta(Ho=0), None, 8, ("output size",)), ("Wo_neg", seta(Wo=-2), None, 8, ("output size",)),
        ("std0", seta(std=(C.c_float * 3)(0.2, 0.0, 0.2)), None, 8, ("std[1]",)),
        ("mean_inf", seta(mean=(C.c_float * 3)(0.4, 0.4, float("inf"))), None, 8, ("mean[2]",)),
        ("offset_neg", seta(out_clip_offset=-1), None, 8, ("out_clip_offset",)),
        ("stride_small", seta(out_clip_stride=8 * 12 * 12 * 3 - 1), None, 8, ("out_clip_stride",)),
        ("src_null", setc(src=None), None, 8, ("clip 1", "null source")),
        ("T0", setc(T=0), None, 8, ("clip 1", "source size")), ("Hs0", setc(Hs=0), None, 8, ("source size",)),
        ("pitch_h_small", setc(pitch_h=95), None, 8, ("pitches",)), ("pitch_t0", setc(pitch_t=0), None, 8, ("pitches",)),
        ("step0", setc(step_h=0.0), None, 8, ("steps",)), ("step_inf", setc(step_w=float("inf")), None, 8, ("steps",)),
        ("Hr0", setc(Hr=0), None, 8, ("resized size",)),
        ("crop_outside", setc(crop_i=5), None, 8, ("crop window",)), ("crop_neg", setc(crop_j=-1), None, 8, ("crop window",)),
        ("box_h0", None, dict(h=0), 8, ("box size",)), ("box_outside", None, dict(i=8), 8, ("outside the resized image",)),
        ("box_neg", None, dict(j=-1), 8, ("outside the resized image",)), ("flip2", None, dict(flip=2), 8, ("flip",)),
        ("T_out0", None, None, 0, ("T_out",)), ("T_out_big", None, None, 65536, ("T_out",)),
    ]


SHARED = shared_prepare_refusals()


@pytest.mark.parametrize("case", SHARED, ids=[c[0] for c in SHARED])
def test_toned_and_grad_refuse_what_the_sampled_launch_refuses(lib, case):
    _, mutate, box_kw, T_out, words = case
    a = prep_args()
    if mutate:
        mutate(a)
    boxes = boxes_of(2, **box_kw) if box_kw is not None else None
    refused(lib, lib.flk_clip_prepare_toned(C.byref(a), boxes, p(GOOD), T_out, p(GOOD), p(GOOD), None), "flk_clip_prepare_toned", *words)
    refused(lib, lib.flk_clip_prepare_grad(C.byref(a), boxes, p(GOOD), T_out, p(GOOD), p(GOOD), p(GOOD), F32, p(GOOD), p(GOOD), None),
            "flk_clip_prepare_grad", *words)


def test_toned_refuses_null_pointers(lib):
    a = prep_args()
    refused(lib, lib.flk_clip_prepare_toned(None, None, p(GOOD), 8, p(GOOD), p(GOOD), None), "null argument")
    refused(lib, lib.flk_clip_prepare_toned(C.byref(a), None, None, 8, p(GOOD), p(GOOD), None), "null frame_idx")
    refused(lib, lib.flk_clip_prepare_toned(C.byref(a), None, p(GOOD), 8, None, p(GOOD), None), "null tone")
    refused(lib, lib.flk_clip_prepare_toned(C.byref(a), None, p(GOOD), 8, p(GOOD), None, None), "null argument")
    a.clips = C.POINTER(type(a._keep[0]))()
    refused(lib, lib.flk_clip_prepare_toned(C.byref(a), None, p(GOOD), 8, p(GOOD), p(GOOD), None), "null clip list")


def test_grad_refusals_of_its_own(lib):
    a = prep_args()

    def grad(a_=a, boxes=None, idx=GOOD, T_out=8, slope=GOOD, scale=GOOD, gx=GOOD, dtype=F32, gdelta=GOOD, partials=GOOD):
        return lib.flk_clip_prepare_grad(C.byref(a_) if a_ is not None else None, boxes, p(idx), T_out, p(slope), p(scale), p(gx), dtype, p(gdelta),
                                         p(partials), None)
    refused(lib, grad(a_=None), "null argument")
    refused(lib, grad(idx=None), "null frame_idx")
    refused(lib, grad(slope=None), "null slope or scale")
    refused(lib, grad(scale=None), "null slope or scale")
    for k in ("gx", "gdelta", "partials"):
        refused(lib, grad(**{k: None}), "null gx_s2d, gdelta or partials")
    for off in (2, 4, 8):
        refused(lib, grad(gx=GOOD + off), "gx_s2d must be 16-byte aligned")
    for dt in (-1, 2, 7):
        refused(lib, grad(dtype=dt), "bad dtype")
    for Ho, Wo in ((11, 12), (12, 11), (13, 13)):
        b = prep_args(Ho=Ho, Wo=Wo)
        for c in b._keep:                                              # keep the crop window inside the resized image
            c.crop_i, c.crop_j = 0, 0
        refused(lib, grad(a_=b), "Ho and Wo must be even")
        refused(lib, grad(a_=b, dtype=BF16), "Ho and Wo must be even")
    assert lib.flk_clip_prepare_grad_scratch_bytes(2, 8, 12) == 2 * 8 * 12 * 3 * 4
    assert lib.flk_clip_prepare_grad_scratch_bytes(0, 8, 12) == 0


def ramp_args(**kw):
    from flickering_adversarial_video_amd import _lib
    a = _lib.ApplyArgs()
    a.x, a.x_is_u8, a.x_scale, a.x_bias = GOOD, 1, 1.0, 0.0
    a.delta, a.delta_dense, a.dclip, a.delta_per_clip = GOOD, 0, 0.2, 1
    a.inv_std = (C.c_float * 3)(*[1.0 / s for s in vs.DEFAULT_STD])
    a.lo, a.hi, a.adv_flag = -1.7, 2.4, 1.0
    a.B, a.T, a.H, a.W, a.fold_t = 2, 8, 16, 16, 1
    a.x_lut = GOOD
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def illum_args(**kw):
    from flickering_adversarial_video_amd import _lib
    m = _lib.IllumArgs()
    m.dec, m.enc, m.enc_n = GOOD, GOOD, 4096
    for k, v in kw.items():
        setattr(m, k, v)
    return m


SLOPE_REFUSALS = [
    ("x_null", dict(x=None), ("null x",)), ("delta_null", dict(delta=None), ("null x",)),
    ("fp32_clip", dict(x_is_u8=0), ("uint8 clip",)), ("no_table", dict(x_lut=None), ("x_lut",)),
    ("B0", dict(B=0), ("positive",)), ("T_neg", dict(T=-1), ("positive",)),
    ("per_line", dict(delta_per_line=1), ("delta_per_line",)), ("dense", dict(delta_dense=1), ("delta_dense",)),
    ("center", dict(center=1), ("center",)), ("shared_delta", dict(delta_per_clip=0), ("delta_per_clip",)),
    ("shift_x", dict(shift_x=1), ("rolls",)), ("shift_p", dict(shift_p=3), ("rolls",)),
]


@pytest.mark.parametrize("illum", [False, True], ids=["additive", "illumination"])
@pytest.mark.parametrize("case", SLOPE_REFUSALS, ids=[c[0] for c in SLOPE_REFUSALS])
def test_tone_slopes_refusals(lib, case, illum):
    _, kw, words = case
    a = ramp_args(**kw)
    m = illum_args() if illum else None
    refused(lib, lib.flk_flicker_tone_slopes(C.byref(a), C.byref(m) if m is not None else None, p(GOOD), p(GOOD), None), "flk_flicker_tone_slopes", *words)


def test_tone_slopes_refuses_null_outputs_and_bad_tables(lib):
    a = ramp_args()
    refused(lib, lib.flk_flicker_tone_slopes(None, None, p(GOOD), p(GOOD), None), "null argument structure")
    refused(lib, lib.flk_flicker_tone_slopes(C.byref(a), None, None, p(GOOD), None), "null slope or scale")
    refused(lib, lib.flk_flicker_tone_slopes(C.byref(a), None, p(GOOD), None, None), "null slope or scale")
    refused(lib, lib.flk_flicker_tone_slopes(C.byref(ramp_args(lo=1.0, hi=-1.0)), None, p(GOOD), p(GOOD), None), "lo > hi")
    for kw, word in ((dict(dec=None), "null dec / enc"), (dict(enc=None), "null dec / enc"), (dict(enc_n=1), "enc_n"), (dict(enc_n=16385), "enc_n")):
        m = illum_args(**kw)
        refused(lib, lib.flk_flicker_tone_slopes(C.byref(a), C.byref(m), p(GOOD), p(GOOD), None), "flk_flicker_tone_slopes", word)


# ---- scripts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script,flag", [("r2plus1d_main_universal_attack.py", ("--train-npz", "--val-npz")),
                                         ("r2plus1d_main_statistics_single_video_attack.py", ("--videos-npz",))])
def test_scripts_refuse_train_delivered_on_files_of_clips(tmp_path, script, flag):
    """clips at the engine's size have no native resolution to flicker at: refused before anything touches a GPU, pointing to --quantise-train"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "clips.npz")
    np.savez(path, clips=np.zeros((2, 8, 64, 64, 3), np.uint8), labels=np.array([0, 1], np.int64))
    files = [x for f in flag for x in (f, path)]
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", script), *files, "--train-delivered", "--flicker-time", "video",
                        "--results-root", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--train-delivered" in r.stderr and "--quantise-train" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "out"))
