"""The rolling shutter, the host side: the taps every LINE of a camera frame gives the rows of the flicker
(videoresnet_spec.capture_line_taps) against capture_taps line by line; the channel's readout draw, which leaves every earlier value of a
seed alone; the numpy float32 restatements of the two kernels (flicker_lines_mix / flicker_lines_mix_grad) against the per-frame pair,
against float64 within the bound their own roundings allow, and against each other as transposes; the C ABI of the new field and entry
points, and their argument checks -- none of which needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                  # the unit roundoff of float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def psi_of(phi, rho, H):
    return phi + (rho * np.arange(H, dtype=np.float64)) / H


# ---- capture_line_taps -------------------------------------------------------------------------------------------------------------
def test_line_taps_are_capture_taps_line_by_line():
    rng = np.random.default_rng(0)
    below = 0
    for _ in range(400):
        phi, e, rho, H = rng.uniform(0, 1), rng.uniform(0, 3), rng.uniform(0, 1), int(rng.integers(1, 130))
        w = vs.capture_line_taps(phi, e, rho, H)
        psi = psi_of(phi, rho, H)
        assert w.dtype == np.float32 and w.shape == (H, max(1, int(np.ceil(psi.max() + e)))) and 1 <= w.shape[1] <= 5 and (w >= 0).all()
        assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
        for h in np.flatnonzero(psi < 1):
            t = vs.capture_taps(psi[h], e)
            assert np.array_equal(bits(w[h, :len(t)]), bits(t)) and (w[h, len(t):] == 0).all()
            below += 1
    assert below > 1000


def test_no_readout_gives_every_line_the_frames_taps():
    for phi, e in ((0.0, 1.0), (0.3, 1.5), (0.9, 3.0), (0.25, 0.0), (np.nextafter(1.0, 0.0), 2.0)):
        t = vs.capture_taps(phi, e)
        w = vs.capture_line_taps(phi, e, 0.0, 7)
        assert w.shape == (7, len(t)) and all(np.array_equal(bits(w[h]), bits(t)) for h in range(7))


def test_line_taps_never_need_more_than_five_rows():
    w = vs.capture_line_taps(np.nextafter(1.0, 0.0), 3.0, 1.0, 112)
    assert w.shape == (112, 5) and np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    assert w[0, 4] == 0 and w[111, 4] > 0 and w[111, 0] == 0          # the last line has left row 0 and reached row 4


def test_line_taps_of_an_instantaneous_sample():
    w = vs.capture_line_taps(0.5, 0.0, 1.0, 4)                         # psi = .5, .75, 1, 1.25: tap floor(psi) is 1
    assert w.tolist() == [[1, 0], [1, 0], [0, 1], [0, 1]]
    assert vs.capture_line_taps(0.2, 0.0, 0.5, 9).tolist() == [[1]] * 9
    assert vs.capture_line_taps(0.0, 0.0, 1.0, 1).tolist() == [[1]]


@pytest.mark.parametrize("args,what", [((1.0, 1, 0.5, 4), "sub-frame"), ((-0.1, 1, 0.5, 4), "sub-frame"), ((np.nan, 1, 0.5, 4), "sub-frame"),
                                       ((0.5, 3.01, 0.5, 4), "exposure"), ((0.5, -1, 0.5, 4), "exposure"), ((0.5, np.inf, 0.5, 4), "exposure"),
                                       ((0.5, 1, -0.01, 4), "readout"), ((0.5, 1, 1.01, 4), "readout"), ((0.5, 1, np.nan, 4), "readout"),
                                       ((0.5, 1, np.inf, 4), "readout"), ((0.5, 1, 0.5, 0), "lines"), ((0.5, 1, 0.5, -3), "lines"),
                                       ((0.5, 1, 0.5, 2.0), "lines"), ((0.5, 1, 0.5, True), "lines"), (("a", 1, 0.5, 4), "numbers"),
                                       ((0.5, 1, None, 4), "numbers")])
def test_line_taps_refusals(args, what):
    with pytest.raises(ValueError, match=what):
        vs.capture_line_taps(*args)


# ---- CaptureChannel ----------------------------------------------------------------------------------------------------------------
def test_channel_without_readout_draws_what_it_drew():
    kw = dict(subframe=(0.0, 1.0), exposure=(0.5, 2.0), gain=(0.8, 1.2), gain_mode="per_channel", seed=7)
    a, b = vs.CaptureChannel(**kw), vs.CaptureChannel(readout=None, **kw)
    assert a.readout is None and b.readout is None
    rng = np.random.default_rng(7)
    for _ in range(2):
        d, e = a.draw(3), b.draw(3)
        assert set(d) == set(e) == {"subframe", "exposure", "gain"}
        assert np.array_equal(d["subframe"], rng.uniform(0.0, 1.0, 3)) and np.array_equal(d["exposure"], rng.uniform(0.5, 2.0, 3))
        assert np.array_equal(d["gain"], rng.uniform(0.8, 1.2, (3, 3)).astype(np.float32))
        assert all(np.array_equal(d[k], e[k]) for k in d)
    with pytest.raises(ValueError, match="tables"):                    # tables still takes the three keys only
        vs.CaptureChannel.tables(dict(a.draw(1), readout=np.zeros(1)), 1)


def test_readouts_are_drawn_after_the_gains():
    kw = dict(subframe=(0.0, 1.0), exposure=(0.5, 2.0), gain=(0.8, 1.2), seed=11)
    plain, rolling = vs.CaptureChannel(**kw), vs.CaptureChannel(readout=(0.2, 0.9), **kw)
    rng = np.random.default_rng(11)
    d0, d = plain.draw(4), rolling.draw(4)
    assert list(d) == ["subframe", "exposure", "gain", "readout"]
    assert all(np.array_equal(d0[k], d[k]) for k in d0)               # the first three entries of the draw are unchanged
    rng.uniform(0, 1, 4), rng.uniform(0.5, 2, 4), rng.uniform(0.8, 1.2, 4)
    assert np.array_equal(d["readout"], rng.uniform(0.2, 0.9, 4)) and d["readout"].dtype == np.float64
    assert (d["readout"] >= 0.2).all() and (d["readout"] <= 0.9).all()
    assert vs.CaptureChannel(readout=0.8).draw(3)["readout"].tolist() == [0.8] * 3          # a number fixes it (the draw is still made)
    assert vs.CaptureChannel(readout=(0, 1)).readout == (0.0, 1.0)
    for bad in ((-0.1, 0.5), (0.5, 1.1), (0.6, 0.4), np.nan, (0, 0.5, 1)):
        with pytest.raises(ValueError, match="readout"):
            vs.CaptureChannel(readout=bad)


def test_line_tables_shapes_padding_and_the_clips_of_a_video():
    draw = {"subframe": np.array([0.0, 0.25, 0.9]), "exposure": np.array([1.0, 1.0, 3.0]), "readout": np.array([0.0, 0.5, 1.0]),
            "gain": np.array([[1, 1, 1], [0.9, 0.8, 0.7], [0.5, 0.5, 0.5]], np.float32)}
    taps, gain = vs.CaptureChannel.line_tables(draw, 2, 6)
    assert taps.dtype == np.float32 and gain.dtype == np.float32 and taps.shape == (6, 6, 5) and gain.shape == (6, 3)
    for v in range(3):
        w = vs.capture_line_taps(draw["subframe"][v], draw["exposure"][v], draw["readout"][v], 6)
        for g in range(2):                                             # the G clips of a video share its channel
            assert np.array_equal(bits(taps[2 * v + g, :, :w.shape[1]]), bits(w)) and (taps[2 * v + g, :, w.shape[1]:] == 0).all()
            assert np.array_equal(gain[2 * v + g], draw["gain"][v])
    assert taps[0].tolist() == [[1, 0, 0, 0, 0]] * 6
    t1, g1 = vs.CaptureChannel.line_tables({"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7), "readout": 0.8}, 1, 10)      # one channel
    assert np.array_equal(t1, vs.capture_line_taps(0.3, 1.5, 0.8, 10)[None]) and np.array_equal(g1, np.array([[0.9, 0.8, 0.7]], np.float32))
    no_readout = {k: draw[k] for k in ("subframe", "exposure", "gain")}
    for bad in (no_readout, dict(draw, extra=1), dict(draw, readout=np.zeros(2)), [1, 2]):
        with pytest.raises(ValueError, match="line_tables"):
            vs.CaptureChannel.line_tables(bad, 1, 6)
    with pytest.raises(ValueError, match="clips per video"):
        vs.CaptureChannel.line_tables(draw, 0, 6)
    with pytest.raises(ValueError, match="lines"):
        vs.CaptureChannel.line_tables(draw, 1, 0)
    with pytest.raises(ValueError, match="readout"):
        vs.CaptureChannel.line_tables(dict(draw, readout=np.array([0.0, 0.5, 1.5])), 1, 6)


# ---- the restatements --------------------------------------------------------------------------------------------------------------
def line_tables(nb, H, K, seed, gain=True):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (nb, H, K)).astype(np.float32), (rng.uniform(0.5, 1.5, (nb, 3)).astype(np.float32) if gain else None)


def test_equal_taps_on_every_line_are_the_frame_mix_on_every_line():
    rng = np.random.default_rng(1)
    for P, K, H in ((5, 4, 6), (2, 3, 1), (1, 4, 9), (7, 1, 3)):
        delta = rng.standard_normal((P, 3)).astype(np.float32)
        delta[0, 0] = -0.0
        rows = rng.integers(-1, P + 1, (3, 4)).astype(np.int32)
        taps = rng.uniform(0, 1, (3, K)).astype(np.float32)
        gain = rng.uniform(0.5, 1.5, (3, 3)).astype(np.float32)
        for gn in (gain, None):
            got = vs.flicker_lines_mix(delta, rows, 4, np.ascontiguousarray(np.repeat(taps[:, None, :], H, axis=1)), gn)
            want = vs.flicker_rows_mix(delta, rows, 4, taps, gn)
            assert got.shape == (3, 4, H, 3) and np.array_equal(bits(got), bits(np.broadcast_to(want[:, :, None, :], got.shape)))


def test_orders_are_the_stated_ones():
    """against scalar float32 loops: the mix per line as flicker_rows_mix; the gradient in its two stages"""
    rng = np.random.default_rng(2)
    for P, K, H in ((5, 5, 3), (2, 5, 2), (1, 3, 4), (3, 4, 1)):
        delta = rng.standard_normal((P, 3)).astype(np.float32)
        rows = rng.integers(0, P, (2, 3)).astype(np.int32)
        taps, gain = line_tables(2, H, K, seed=P)
        g = rng.standard_normal((2, 3, H, 3)).astype(np.float32)
        mix, grad = vs.flicker_lines_mix(delta, rows, 3, taps, gain), vs.flicker_lines_mix_grad(g, rows, 3, taps, gain, P)
        want = np.zeros((P, 3), np.float32)
        for i in range(6):
            b, t = divmod(i, 3)
            for c in range(3):
                for h in range(H):
                    acc = np.float32(taps[b, h, 0] * delta[rows[b, t], c])
                    for k in range(1, K):
                        acc = np.float32(acc + np.float32(taps[b, h, k] * delta[(rows[b, t] + k) % P, c]))
                    assert bits(mix[b, t, h, c]) == bits(np.float32(gain[b, c] * acc))
            for k in range(K):
                for c in range(3):
                    s = np.float32(0)
                    for h in range(H):
                        s = np.float32(s + np.float32(np.float32(gain[b, c] * taps[b, h, k]) * g[b, t, h, c]))
                    r = (rows[b, t] + k) % P
                    want[r, c] = np.float32(want[r, c] + s)
        assert np.array_equal(bits(grad), bits(want))


def mix64(delta, rows, clip_T, taps, gain):
    P = delta.shape[0]
    r0 = np.clip(rows.reshape(-1).astype(np.int64), 0, P - 1)
    b = np.arange(r0.shape[0]) // clip_T
    out = np.zeros((r0.shape[0], taps.shape[1], 3))
    mag = np.zeros_like(out)
    for k in range(taps.shape[2]):
        term = taps[b, :, k].astype(np.float64)[:, :, None] * delta[(r0 + k) % P].astype(np.float64)[:, None, :]
        term = term * (1.0 if gain is None else gain[b].astype(np.float64)[:, None, :])
        out, mag = out + term, mag + np.abs(term)
    return out.reshape(rows.shape + out.shape[1:]), mag.reshape(rows.shape + out.shape[1:])


def grad64(g, rows, clip_T, taps, gain, P):
    """the transpose in float64, the magnitudes of its terms, and the number of addends of every output (terms: one per line and hit)"""
    H, K = taps.shape[1:]
    out, mag, hits = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 1), np.int64)
    g, r = g.reshape(-1, H, 3).astype(np.float64), rows.reshape(-1)
    for i in range(r.shape[0]):
        if 0 <= r[i] < P:
            b = i // clip_T
            for k in range(K):
                term = taps[b, :, k].astype(np.float64)[:, None] * (1.0 if gain is None else gain[b].astype(np.float64)) * g[i]
                out[(r[i] + k) % P] += term.sum(0)
                mag[(r[i] + k) % P] += np.abs(term).sum(0)
                hits[(r[i] + k) % P] += H
    return out, mag, hits


@pytest.mark.parametrize("P,K,H,nb,clip_T", [(5, 5, 6, 4, 8), (2, 4, 3, 3, 3), (1, 5, 7, 2, 5), (682, 3, 4, 3, 16), (8, 2, 112, 6, 7)])
@pytest.mark.parametrize("with_gain", [False, True], ids=["nogain", "gain"])
def test_restatements_against_float64_and_as_transposes(P, K, H, nb, clip_T, with_gain):
    rng = np.random.default_rng(P * 10 + K)
    delta = rng.standard_normal((P, 3)).astype(np.float32)
    rows = rng.integers(0, P, (nb, clip_T)).astype(np.int32)
    g = rng.standard_normal((nb, clip_T, H, 3)).astype(np.float32)
    taps, gain = line_tables(nb, H, K, seed=P + K, gain=with_gain)
    m, gr = vs.flicker_lines_mix(delta, rows, clip_T, taps, gain), vs.flicker_lines_mix_grad(g, rows, clip_T, taps, gain, P)
    assert m.dtype == np.float32 and m.shape == (nb, clip_T, H, 3) and gr.dtype == np.float32 and gr.shape == (P, 3)
    # every output: (addends + K + 2) roundings of relative size 2^-24 at most, on the scale of the sum of the terms' magnitudes
    m64, m_mag = mix64(delta, rows, clip_T, taps, gain)
    assert (np.abs(m.astype(np.float64) - m64) <= (K + K + 2) * U * m_mag).all()
    g64, g_mag, hits = grad64(g, rows, clip_T, taps, gain, P)
    assert (np.abs(gr.astype(np.float64) - g64) <= (hits + K + 2) * U * g_mag).all()
    # adjoint identity <mix(delta), g> = <delta, mix_grad(g)>: both sides are sums of the same terms, each side off by its own bound
    lhs, rhs = (m.astype(np.float64) * g).sum(), (delta.astype(np.float64) * gr).sum()
    bound = ((K + K + 2) * U * m_mag * np.abs(g)).sum() + ((hits + K + 2) * U * g_mag * np.abs(delta)).sum()
    assert abs(lhs - rhs) <= bound and bound < 1e-2 * max(1.0, np.abs(m64 * g).sum())


def test_bad_rows_unhit_rows_and_refusals():
    delta = np.arange(9, dtype=np.float32).reshape(3, 3)
    taps, gain = line_tables(1, 2, 2, seed=4)
    bad = np.array([[-1, 3, 7, -9, 2, 0]], np.int32)
    assert np.array_equal(bits(vs.flicker_lines_mix(delta, bad, 6, taps, gain)), bits(vs.flicker_lines_mix(delta, np.clip(bad, 0, 2), 6, taps, gain)))
    g = np.random.default_rng(5).standard_normal((1, 6, 2, 3)).astype(np.float32)
    g_skipped = g.copy()
    g_skipped[0, :4] = 0
    assert np.array_equal(vs.flicker_lines_mix_grad(g, bad, 6, taps, gain, 3), vs.flicker_lines_mix_grad(g_skipped, np.clip(bad, 0, 2), 6, taps, gain, 3))
    out = vs.flicker_lines_mix_grad(g[:, :1], np.array([[1]], np.int32), 1, np.ones((1, 2, 1), np.float32), None, 4)
    assert np.array_equal(bits(out[[0, 2, 3]]), np.zeros((3, 3), np.uint32)) and np.abs(out[1]).min() > 0
    d, r, t = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32), np.ones((2, 5, 2), np.float32)
    for call in (lambda: vs.flicker_lines_mix(d.astype(np.float64), r, 3, t), lambda: vs.flicker_lines_mix(d, r.astype(np.float32), 3, t),
                 lambda: vs.flicker_lines_mix(d, r, 4, t), lambda: vs.flicker_lines_mix(d, r, 3, np.ones((2, 5, 6), np.float32)),
                 lambda: vs.flicker_lines_mix(d, r, 3, np.ones((2, 2), np.float32)), lambda: vs.flicker_lines_mix(d, r, 3, np.ones((3, 5, 2), np.float32)),
                 lambda: vs.flicker_lines_mix(d, r, 3, t, np.ones((2, 2), np.float32)),
                 lambda: vs.flicker_lines_mix_grad(np.zeros((2, 3, 4, 3), np.float32), r, 3, t, None, 4),
                 lambda: vs.flicker_lines_mix_grad(np.zeros((2, 3, 5, 3), np.float32), r, 3, t, None, 0)):
        with pytest.raises(ValueError):
            call()


# ---- the C ABI and the argument checks, without a GPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_header_library_and_binding_agree(lib, tmp_path):
    from flickering_adversarial_video_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flicker_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(flk_[a-z0-9_]+)\s*\(", src))
    for name in ("flk_flicker_lines_mix", "flk_flicker_lines_mix_grad"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert len(_lib._SIGS["flk_flicker_lines_mix"][1]) == 11 and len(_lib._SIGS["flk_flicker_lines_mix_grad"][1]) == 12
    # the new field: same offset in the header and the binding; no other field moved and the struct kept its size (it fills padding)
    names = ("delta_per_clip", "delta_per_line", "dclip_dev", "x_lut")
    prog = tmp_path / "abi.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flicker_hip.h"\n'
                    'int main(void) { printf("%zu' + " %zu" * len(names) + '\\n", sizeof(flk_apply_args), '
                    + ", ".join(f"offsetof(flk_apply_args, {n})" for n in names) + '); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True, capture_output=True)
    size, *offs = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(_lib.ApplyArgs) == size and [getattr(_lib.ApplyArgs, n).offset for n in names] == offs
    assert offs[1] == offs[0] + 4 and offs[2] == offs[1] + 4 and size == offs[3] + 8
    assert _lib.ApplyArgs().delta_per_line == 0


def test_mix_entry_points_refuse_bad_arguments(lib):
    p = C.c_void_p(8)

    def mix(delta=p, P=5, rows=p, n=6, clip_T=3, H=4, taps=p, K=2, gain=None, out=p):
        return lib.flk_flicker_lines_mix(delta, P, rows, n, clip_T, H, taps, K, gain, out, None)

    def grad(g=p, rows=p, n=6, clip_T=3, H=4, taps=p, K=2, gain=None, P=5, scratch=p, out=p):
        return lib.flk_flicker_lines_mix_grad(g, rows, n, clip_T, H, taps, K, gain, P, scratch, out, None)

    # FLK_EINVAL with a reason that names the argument, before any GPU call (there is no GPU here)
    for call, nulls in ((mix, dict(delta=b"delta", rows=b"rows", taps=b"taps", out=b"out")),
                        (grad, dict(g=b"g_lines", rows=b"rows", taps=b"taps", scratch=b"scratch", out=b"g_rows"))):
        for arg, name in nulls.items():
            assert call(**{arg: None}) == -1 and name in lib.flk_last_error() and b"null" in lib.flk_last_error()
        for kw, name in ((dict(n=0), b"n must be"), (dict(n=-3), b"n must be"), (dict(n=7), b"clip_T"), (dict(clip_T=0), b"clip_T"),
                         (dict(clip_T=4), b"clip_T"), (dict(K=0), b"K "), (dict(K=6), b"K "), (dict(K=-1), b"K "), (dict(H=0), b"H "),
                         (dict(H=-2), b"H "), (dict(P=0), b"period"), (dict(P=683), b"period")):
            assert call(**kw) == -1 and name in lib.flk_last_error(), (kw, lib.flk_last_error())


def test_per_line_arguments_are_refused_where_they_have_no_meaning(lib):
    from flickering_adversarial_video_amd import _lib
    fake = C.c_void_p(4096)

    def args(**kw):
        a = _lib.ApplyArgs()
        a.x, a.x_is_u8, a.delta, a.delta_per_line, a.delta_per_clip = fake, 0, fake, 1, 1
        a.B, a.T, a.H, a.W, a.fold_t, a.lo, a.hi, a.adv_flag = 2, 4, 6, 8, 1, -1.0, 1.0, 1.0
        a.inv_std = (C.c_float * 3)(1, 1, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def apply(a):
        return lib.flk_perturb_apply_s2d(C.byref(a), fake, _lib.FLK_BF16 if a.fold_t == 4 else _lib.FLK_F32, None)

    def reduce(a):
        return lib.flk_perturb_grad_reduce(C.byref(a), fake, _lib.FLK_F32, fake, fake, None)

    # FLK_EINVAL naming the field, before any GPU call (there is no GPU here: a call that got past its checks would return FLK_EHIP, -2)
    for call in (apply, reduce):
        for kw in (dict(delta_dense=1, delta_per_clip=0), dict(center=1), dict(fold_t=0), dict(fold_t=2), dict(fold_t=3)):
            assert call(args(**kw)) == -1 and b"delta_per_line" in lib.flk_last_error(), (call.__name__, kw, lib.flk_last_error())
    assert reduce(args(delta_per_clip=0)) == -1 and b"delta_per_line needs delta_per_clip" in lib.flk_last_error()
    # the I3D-only entry points
    i3d = args(x_is_u8=1, center=1, fold_t=3, H=224, W=224, delta_per_clip=0)
    assert lib.flk_stem_delta_grad_mask(C.byref(i3d), fake, None) == -1 and b"delta_per_line" in lib.flk_last_error()
    assert lib.flk_stem_delta_grad(C.byref(i3d), fake, 64, fake, fake, fake, 0, None) == -1 and b"delta_per_line" in lib.flk_last_error()
    assert lib.flk_stem_delta_bias(C.byref(i3d), fake, fake, None) == -1 and b"delta_per_line" in lib.flk_last_error()
    assert lib.flk_stem_fwd_u8(C.byref(i3d), fake, fake, fake, None, 0, fake, 64, None) == -1 and b"delta_per_line" in lib.flk_last_error()
    # the export: with a dense delta; a period with per-clip perturbations
    e = _lib.ExportArgs()
    e.mul, e.add, e.levels, e.out_clip_stride = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(1, 1, 1), 128.0, 2 * 4 * 6 * 8 * 3
    assert lib.flk_adv_export_u8(C.byref(args(delta_dense=1, delta_per_clip=0)), C.byref(e), fake, None, None) == -1 and b"delta_per_line" in lib.flk_last_error()
    e.delta_T = 3
    assert lib.flk_adv_export_u8(C.byref(args()), C.byref(e), fake, None, None) == -1 and b"delta_T" in lib.flk_last_error()


def test_make_apply_args_names_the_per_line_form_by_keyword():
    import torch
    from flickering_adversarial_video_amd import ops
    x = torch.zeros((2, 4, 6, 8, 3))
    a = ops.make_apply_args(x, torch.zeros((2, 4, 6, 3)), fold_t=1, per_line=True)
    assert (a.delta_per_line, a.delta_per_clip, a.delta_dense) == (1, 1, 0)
    a = ops.make_apply_args(x, torch.zeros((4, 6, 3)), fold_t=4, per_line=True)
    assert (a.delta_per_line, a.delta_per_clip, a.delta_dense) == (1, 0, 0)
    a = ops.make_apply_args(x, torch.zeros((4, 6, 8, 3)), fold_t=1)                       # a 4-D delta without the keyword still means dense
    assert (a.delta_per_line, a.delta_per_clip, a.delta_dense) == (0, 0, 1)
    for bad in (dict(delta=torch.zeros((4, 3))), dict(delta=torch.zeros((4, 6, 8, 3))), dict(delta=torch.zeros((4, 6, 3)), fold_t=2),
                dict(delta=torch.zeros((4, 6, 3)), fold_t=1, center=True)):
        with pytest.raises(ValueError, match="per_line"):
            ops.make_apply_args(x, bad.pop("delta"), per_line=True, **dict(dict(fold_t=1), **bad))


def test_scripts_take_the_readout_option():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--flicker-time", default="clip")
    vs.add_capture_arguments(ap)
    a = ap.parse_args(["--flicker-time", "video", "--capture-readout", "0.2", "0.9"])
    ch = vs.capture_from_arguments(ap, a)
    assert ch.readout == (0.2, 0.9) and ch.subframe == (0.0, 0.0) and "readout" in ch.draw(1)
    a = ap.parse_args(["--flicker-time", "video", "--capture-subframe", "0", "1"])
    assert vs.capture_from_arguments(ap, a).readout is None and ap.parse_args([]).capture_readout is None
    for argv in (["--capture-readout", "0", "1"], ["--flicker-time", "video", "--capture-readout", "0", "2"]):
        with pytest.raises(SystemExit):
            vs.capture_from_arguments(ap, ap.parse_args(argv))
