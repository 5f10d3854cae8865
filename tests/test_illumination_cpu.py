"""The flicker as scene illumination, the host side: the camera tables (videoresnet_spec.illum_tables) give every byte back under no
modulation; the restatements' derivative against central differences in float64; the identities between the delta forms; the C ABI of
flk_illum_args and the three entry points, and every argument they refuse -- none of which needs a GPU."""
import argparse
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                  # the unit roundoff of float32
LEVELS = np.ascontiguousarray(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1).reshape(1, 1, 16, 16, 3))


# ---- the tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("response", vs.ILLUM_RESPONSES)
def test_every_level_re_encodes_to_itself(response):
    dec, enc = vs.illum_tables(response)
    assert dec.dtype == np.float32 and dec.shape == (256, 3) and enc.dtype == np.float32 and enc.shape == (vs.ILLUM_N + 1,)
    assert dec[0].tolist() == [0, 0, 0] and dec[255].tolist() == [1, 1, 1] and enc[0] == 0 and enc[-1] == 1 and (np.diff(enc) >= 0).all()
    zero = np.zeros((1, 3), np.float32)
    assert np.array_equal(vs.illum_export_host(LEVELS, zero, (dec, enc)), LEVELS)
    e = vs._illum_display(LEVELS, np.float32(1.0), dec, enc)[0]
    err = np.abs(e.astype(np.float64) * 255.0 - LEVELS).max()
    print(f"{response}: largest round-trip error {err:.4g} of a level")
    assert err < 0.01                      # far from the 0.5 at which a level would move
    # and the quantised apply under no modulation is the decode table itself
    lut = vs.u8_decode_table()
    assert np.array_equal(vs.illum_apply_host(LEVELS, zero, (dec, enc), q_lut=lut), lut[LEVELS, np.arange(3)])


def test_user_tables():
    dec, enc = vs.illum_tables("srgb")
    d2, e2 = vs.illum_tables((dec, enc[::4]))                   # a coarser table of the same curve still round-trips: N = 1024
    assert e2.shape == (1025,) and np.array_equal(d2, dec)
    with pytest.raises(ValueError, match="does not give every byte back"):
        vs.illum_tables((dec, vs.illum_tables("linear")[1]))     # sRGB decode, linear encode: not a round trip
    with pytest.raises(ValueError, match="does not give every byte back"):
        vs.illum_tables((dec, enc[::512]))                       # 8 segments cannot carry 256 levels
    with pytest.raises(ValueError, match="non-decreasing"):
        vs.illum_tables((dec, enc[::-1]))
    with pytest.raises(ValueError, match=r"\[0,1\]"):
        vs.illum_tables((dec * 2, enc))
    for bad in ((dec[:, :2], enc), (dec, enc[:2]), (dec, np.zeros(vs.ILLUM_MAX_N + 2, np.float32)), (dec, enc.reshape(1, -1))):
        with pytest.raises(ValueError, match="dec must be"):
            vs.illum_tables(bad)
    for bad in ("gamma", 3, None):
        with pytest.raises(ValueError, match="response must be"):
            vs.illum_tables(bad)


# ---- the restatements --------------------------------------------------------------------------------------------------------------
def display64(L, s, enc):
    """the model in float64 on the float32 tables: interpolated display value of linear light L under the factor s"""
    N = enc.shape[0] - 1
    z = np.clip(L * s, 0.0, 1.0) * N
    i = np.minimum(z.astype(np.int64), N - 1)
    e = enc.astype(np.float64)
    return e[i] + (z - i) * (e[i + 1] - e[i])


@pytest.mark.parametrize("response", vs.ILLUM_RESPONSES)
def test_derivative_is_the_central_difference(response):
    """one pixel per clip, so every output of illum_grad_host is one term: gx * (d N) L * adv_flag * out_mul.  Points are kept only where
    the +-h neighbourhood stays inside one table segment and strictly inside the [0,1] clamp; there the map is linear in m, so the
    central difference in float64 is its slope up to float64 rounding, and the restatement's weight is that slope up to its two
    float32 products and the float32 difference d (3 roundings)."""
    dec, enc = tables = vs.illum_tables(response)
    N = enc.shape[0] - 1
    rng = np.random.default_rng(1)
    B = 4096
    x = rng.integers(1, 256, (B, 1, 1, 1, 3), dtype=np.uint8)
    m = rng.uniform(-0.25, 0.25, (B, 1, 3)).astype(np.float32)
    mul, add = vs.illum_out_affine()
    g = vs.illum_grad_host(x, m, tables, np.ones(x.shape), dclip=0.3)
    L = dec[x.reshape(B, 3), np.arange(3)].astype(np.float64)
    s = (np.float32(1.0) + m.reshape(B, 3)).astype(np.float64)           # the factor the restatement used (float32)
    z = (L.astype(np.float32) * s.astype(np.float32)).astype(np.float64) * N
    h = 0.05 / (L * N)                                                    # moves z by +-0.05 of a segment
    frac = z - np.floor(z)
    keep = (frac > 0.1) & (frac < 0.9) & (z > 0.2) & (z < N - 0.2)
    assert keep.mean() > 0.5
    f = lambda sv: display64(L, sv, enc) * mul.astype(np.float64) + add.astype(np.float64)
    cd = (f(s + h) - f(s - h)) / (2 * h)
    got = g.reshape(B, 3)
    rel = np.abs(got - cd)[keep] / np.abs(cd)[keep]
    print(f"{response}: {keep.sum()} points, largest relative difference {rel.max():.3g}")
    assert (np.abs(cd)[keep] > 0).all() and rel.max() <= 4 * U


def test_gradient_sums_roll_clamp_and_saturation():
    tables = vs.illum_tables("srgb")
    rng = np.random.default_rng(2)
    B, T, H, W = 2, 4, 6, 8
    x = rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    gx = rng.standard_normal(x.shape)
    d = rng.uniform(-0.4, 0.4, (T, 3)).astype(np.float32)
    g, mag, n = vs.illum_grad_host(x, d, tables, gx, dclip=0.3, shift_x=1, shift_p=2, bound=True)
    assert g.shape == (T, 3) and n == B * H * W and (mag >= np.abs(g)).all()
    assert ((g == 0) == (np.abs(d) > 0.3)).all() and (np.abs(d) > 0.3).any()          # zero exactly where delta lies outside its clamp
    # the shared form is the sum of the per-clip form over equal clips, and that the sum of the per-line form over its lines
    pc = vs.illum_grad_host(np.roll(x, 1, axis=1), np.ascontiguousarray(np.broadcast_to(np.roll(d, 2, axis=0), (B, T, 3))), tables, gx, dclip=0.3)
    assert np.allclose(np.roll(pc.sum(0), -2, axis=0), g, rtol=1e-12, atol=1e-12)
    pl = vs.illum_grad_host(np.roll(x, 1, axis=1), np.ascontiguousarray(np.broadcast_to(np.roll(d, 2, axis=0)[None, :, None, :], (B, T, H, 3))), tables, gx,
                            dclip=0.3, per_line=True)
    assert pl.shape == (B, T, H, 3) and np.allclose(pl.sum(2), pc, rtol=1e-12, atol=1e-12)
    # saturated and black bytes: unchanged output, no gradient
    sat = np.zeros((1, 2, 2, 2, 3), np.uint8)
    sat[:, :, 0] = 255
    up = np.full((2, 3), 0.25, np.float32)
    assert np.array_equal(vs.illum_export_host(sat, up, tables, dclip=0.3), sat)
    assert (vs.illum_grad_host(sat, up, tables, np.ones(sat.shape), dclip=0.3) == 0).all()
    with pytest.raises(ValueError, match="per-clip"):
        vs.illum_grad_host(x, np.zeros((T, H, 3), np.float32), tables, gx, per_line=True)


def test_forms_agree_and_the_consequences_the_model_is_for():
    dec, enc = tables = vs.illum_tables("srgb")
    rng = np.random.default_rng(3)
    B, T, H, W = 2, 3, 5, 7
    x = rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    d = rng.uniform(-0.3, 0.3, (T, 3)).astype(np.float32)
    q, st = vs.illum_export_host(x, d, tables, dclip=0.25, shift_x=1, shift_p=2, stats=True)
    per_clip = np.ascontiguousarray(np.broadcast_to(np.roll(d, 2, axis=0), (B, T, 3)))
    assert np.array_equal(vs.illum_export_host(np.roll(x, 1, axis=1), per_clip, tables, dclip=0.25), q)
    lines = np.ascontiguousarray(np.broadcast_to(d[:, None, :], (T, H, 3)))
    assert np.array_equal(vs.illum_export_host(x, lines, tables, dclip=0.25, shift_x=1, shift_p=2, per_line=True), q)
    assert np.array_equal(vs.illum_export_host(x, d[:2], tables, dclip=0.25, delta_T=2)[:, 2], vs.illum_export_host(x, d[[0, 1, 0]], tables, dclip=0.25)[:, 2])
    src = np.roll(x, 1, axis=1).astype(np.int64)
    assert st.shape == (B, T, 3, 4) and np.array_equal(st[..., 0], (q.astype(np.int64) - src).sum((2, 3)))
    # the quantised apply decodes the exported bytes; the plain apply is the affine map of the display value
    lut = vs.u8_decode_table()
    assert np.array_equal(vs.illum_apply_host(x, d, tables, dclip=0.25, shift_x=1, shift_p=2, q_lut=lut), lut[q, np.arange(3)])
    plain = vs.illum_apply_host(x, d, tables, dclip=0.25, shift_x=1, shift_p=2)
    assert np.abs(vs.encode_u8(plain).astype(np.int64) - q).max() <= 1                 # (a second rounding chain: at most the neighbouring level)
    # +10 % light: a dark pixel barely moves, a mid-grey one moves by several levels, 255 does not move at all
    grey = np.array([8, 128, 255], np.uint8).reshape(1, 1, 1, 3, 1).repeat(3, axis=4)
    moved = vs.illum_export_host(grey, np.full((1, 3), 0.1, np.float32), tables).astype(np.int64) - grey
    assert moved[0, 0, 0, 0, 0] <= 1 and moved[0, 0, 0, 1, 0] >= 4 and moved[0, 0, 0, 2, 0] == 0
    with pytest.raises(ValueError, match="uint8"):
        vs.illum_export_host(x.astype(np.float32), d, tables)
    with pytest.raises(ValueError, match="delta is"):
        vs.illum_export_host(x, np.zeros((T + 1, 3), np.float32), tables)
    with pytest.raises(ValueError, match="adv_flag = 0"):
        vs.illum_apply_host(x, d, tables, adv_flag=0.0)


# ---- the C ABI and the argument checks, without a GPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


NEW = ("flk_illum_apply_s2d", "flk_illum_export_u8", "flk_illum_grad_reduce")


def test_header_library_and_binding_agree(lib, tmp_path):
    from flickering_adversarial_video_amd import _lib, build
    assert "illum.hip" in build.SOURCES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flicker_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(flk_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert [len(_lib._SIGS[n][1]) for n in NEW] == [5, 6, 7]
    names = ("dec", "enc", "enc_n", "out_mul", "out_add")
    prog = tmp_path / "abi.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flicker_hip.h"\n'
                    'int main(void) { printf("%zu %zu' + " %zu" * len(names) + '\\n", sizeof(flk_illum_args), sizeof(flk_apply_args), '
                    + ", ".join(f"offsetof(flk_illum_args, {n})" for n in names) + '); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True, capture_output=True)
    size, apply_size, *offs = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.IllumArgs) == size == 48 and [getattr(_lib.IllumArgs, n).offset for n in names] == offs == [0, 8, 16, 20, 32]
    assert C.sizeof(_lib.ApplyArgs) == apply_size                # the model came in a struct of its own: flk_apply_args did not grow


def test_entry_points_refuse_what_they_do_not_support(lib):
    from flickering_adversarial_video_amd import _lib
    fake = C.c_void_p(4096)

    def args(**kw):
        a = _lib.ApplyArgs()
        a.x, a.x_is_u8, a.x_lut, a.delta = fake, 1, fake, fake
        a.B, a.T, a.H, a.W, a.fold_t, a.adv_flag, a.dclip = 2, 4, 6, 8, 1, 1.0, 0.2
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def illum(**kw):
        m = _lib.IllumArgs()
        m.dec, m.enc, m.enc_n = fake, fake, 4096
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    e = _lib.ExportArgs()
    e.out_clip_stride = 2 * 4 * 6 * 8 * 3

    def apply(a, m=None, out=fake):
        return lib.flk_illum_apply_s2d(C.byref(a), C.byref(m or illum()), out, _lib.FLK_BF16 if a.fold_t == 4 else _lib.FLK_F32, None)

    def export(a, m=None, out=fake):
        return lib.flk_illum_export_u8(C.byref(a), C.byref(m or illum()), C.byref(e), out, None, None)

    def reduce(a, m=None, out=fake):
        return lib.flk_illum_grad_reduce(C.byref(a), C.byref(m or illum()), out, _lib.FLK_F32, fake, fake, None)

    # FLK_EINVAL naming the field, before any GPU call (there is no GPU here: a call that got past its checks would return FLK_EHIP, -2)
    for call in (apply, export, reduce):
        for kw, name in ((dict(x_is_u8=0), b"x_is_u8"), (dict(x_lut=None), b"x_lut"), (dict(center=1), b"center"), (dict(delta_dense=1), b"delta_dense"),
                         (dict(x=None), b"null x"), (dict(delta=None), b"delta"), (dict(B=0), b"sizes"), (dict(dclip_dev=fake), b"dclip_dev")):
            assert call(args(**kw)) == -1 and name in lib.flk_last_error(), (call.__name__, kw, lib.flk_last_error())
        for kw, name in ((dict(dec=None), b"dec"), (dict(enc=None), b"enc"), (dict(enc_n=1), b"enc_n"), (dict(enc_n=0), b"enc_n"), (dict(enc_n=-5), b"enc_n"),
                         (dict(enc_n=16385), b"enc_n")):
            assert call(args(), illum(**kw)) == -1 and name in lib.flk_last_error(), (call.__name__, kw, lib.flk_last_error())
        assert call(args(), out=None) == -1 and b"null" in lib.flk_last_error()
    assert lib.flk_illum_apply_s2d(None, C.byref(illum()), fake, 0, None) == -1 and lib.flk_illum_apply_s2d(C.byref(args()), None, fake, 0, None) == -1
    for call in (apply, reduce):
        for fold_t in (0, 2, 3):
            assert call(args(fold_t=fold_t)) == -1 and b"fold_t" in lib.flk_last_error()
        assert call(args(x=C.c_void_p(4097))) == -1 and b"2-byte aligned" in lib.flk_last_error()
        assert call(args(), out=C.c_void_p(4104)) == -1 and b"16-byte aligned" in lib.flk_last_error()
        assert call(args(H=5)) == -1 and b"even" in lib.flk_last_error()
    assert lib.flk_illum_apply_s2d(C.byref(args(fold_t=4)), C.byref(illum()), fake, _lib.FLK_F32, None) == -1 and b"fold_t = 4" in lib.flk_last_error()
    assert reduce(args(delta_per_line=1)) == -1 and b"delta_per_line needs delta_per_clip" in lib.flk_last_error()
    assert lib.flk_illum_grad_reduce(C.byref(args()), C.byref(illum()), fake, _lib.FLK_F32, fake, None, None) == -1 and b"partials" in lib.flk_last_error()
    e.delta_T = 3
    assert export(args(delta_per_clip=1)) == -1 and b"delta_T" in lib.flk_last_error()
    e.delta_T, e.out_clip_stride = 0, 7
    assert export(args()) == -1 and b"out_clip_stride" in lib.flk_last_error()
    # what passes every check reaches the device, which is not there
    e.out_clip_stride = 2 * 4 * 6 * 8 * 3
    import torch
    if not torch.cuda.is_available():
        assert apply(args()) == -2 and export(args(H=5, W=7, fold_t=0)) in (-1, -2)


# ---- the engine's and the scripts' arguments -------------------------------------------------------------------------------------------
def test_flicker_model_arguments():
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, check_flicker_model
    assert check_flicker_model("additive") is None and check_flicker_model("additive", "no such curve") is None
    dec, enc = check_flicker_model("illumination", "linear")
    assert np.array_equal(enc, vs.illum_tables("linear")[1]) and vs.FLICKER_MODELS == ("additive", "illumination")
    kw = dict(batch_size=2, sample_length=8, image_size=64)
    with pytest.raises(ValueError, match="flicker_model must be one of"):
        FlickerVideoResNet("r3d_18", None, flicker_model="lamp", **kw)
    with pytest.raises(ValueError, match="response must be"):
        FlickerVideoResNet("r3d_18", None, flicker_model="illumination", response="gamma", **kw)
    with pytest.raises(ValueError, match="flickering attack only"):
        FlickerVideoResNet("r3d_18", None, flicker_model="illumination", attack_type="L12", **kw)
    with pytest.raises(ValueError, match="flickering attack only"):
        check_flicker_model("illumination", dense=True)
    ap = argparse.ArgumentParser()
    vs.add_flicker_model_arguments(ap)
    a = ap.parse_args([])
    assert (a.flicker_model, a.response) == ("additive", "srgb")
    a = ap.parse_args(["--flicker-model", "illumination", "--response", "linear"])
    assert (a.flicker_model, a.response) == ("illumination", "linear")
    with pytest.raises(SystemExit):
        ap.parse_args(["--flicker-model", "lamp"])


def test_make_illum_args_checks_its_tables():
    import torch
    from flickering_adversarial_video_amd import ops
    dec, enc = vs.illum_tables("srgb")
    m = ops.make_illum_args((torch.from_numpy(dec), torch.from_numpy(enc)))
    mul, add = vs.illum_out_affine()
    assert m.enc_n == 4096 and list(m.out_mul) == mul.tolist() and list(m.out_add) == add.tolist()
    assert list(ops.make_illum_args((dec, enc), device="cpu", out_mul=(1, 2, 3), out_add=(0, 0, 0)).out_mul) == [1, 2, 3]
    for bad in ((dec[:, :2], enc), (dec, enc[:2]), (dec.astype(np.float64), enc), (dec, np.zeros(16386, np.float32))):
        with pytest.raises(ValueError, match="make_illum_args"):
            ops.make_illum_args(bad, device="cpu")
