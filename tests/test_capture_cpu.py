"""The capture channel, the host side: the taps a camera frame gives the rows of the flicker (videoresnet_spec.capture_taps) against
tables written by hand; the numpy float32 restatements of the two kernels (flicker_rows_mix / flicker_rows_mix_grad) against float64 within
the bound their own roundings allow, and against each other as transposes; the distribution the channels are drawn from
(CaptureChannel); the two C entry points' argument checks and the constructors' refusals, none of which needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from flickering_adversarial_video_amd import videoresnet_spec as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                  # the unit roundoff of float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- capture_taps ----------------------------------------------------------------------------------------------------------------
BY_HAND = [((0, 1), [1]), ((0.25, 1), [.75, .25]), ((0.5, 0.5), [1]), ((0.75, 0.5), [.5, .5]), ((0.5, 2), [.25, .5, .25]),
           ((0.9, 3), [0.1 / 3, 1 / 3, 1 / 3, 0.9 / 3]), ((0, 0), [1]), ((0.4, 0), [1]), ((0.999, 0), [1]), ((0, 3), [1 / 3, 1 / 3, 1 / 3]),
           ((0.3, 1.5), [0.7 / 1.5, 0.8 / 1.5])]


@pytest.mark.parametrize("args,want", BY_HAND, ids=[f"phi{a}_e{b}" for (a, b), _ in BY_HAND])
def test_taps_against_tables_written_by_hand(args, want):
    w = vs.capture_taps(*args)
    assert w.dtype == np.float32 and w.shape == (len(want),)
    assert np.array_equal(w, np.asarray(want, np.float64).astype(np.float32)) or np.abs(w.astype(np.float64) - want).max() <= U
    assert (w >= 0).all() and abs(w.astype(np.float64).sum() - 1.0) <= len(want) * U


def test_taps_are_a_convex_mix_everywhere():
    rng = np.random.default_rng(0)
    for phi, e in zip(rng.uniform(0, 1, 300), rng.uniform(0, 3, 300)):
        w = vs.capture_taps(phi, e)
        assert w.shape == (max(1, int(np.ceil(phi + e))),) and 1 <= w.shape[0] <= 4 and (w >= 0).all()
        assert abs(w.astype(np.float64).sum() - 1.0) <= w.shape[0] * U


@pytest.mark.parametrize("phi,e,what", [(1.0, 1, "sub-frame"), (-0.1, 1, "sub-frame"), (np.nan, 1, "sub-frame"), (np.inf, 1, "sub-frame"),
                                        (0.5, -0.1, "exposure"), (0.5, 3.01, "exposure"), (0.5, np.nan, "exposure"), (0.5, np.inf, "exposure"),
                                        ("a", 1, "numbers"), (0.5, None, "numbers")])
def test_taps_refusals(phi, e, what):
    with pytest.raises(ValueError, match=what):
        vs.capture_taps(phi, e)


# ---- the restatements --------------------------------------------------------------------------------------------------------------
def tables(nb, K, seed, gain=True):
    rng = np.random.default_rng(seed)
    taps = rng.uniform(0, 1, (nb, K)).astype(np.float32)
    return taps, (rng.uniform(0.5, 1.5, (nb, 3)).astype(np.float32) if gain else None)


def mix64(delta, rows, clip_T, taps, gain):
    """the mix in float64, and the sum of the magnitudes of its addends (the scale of its rounding error)"""
    P = delta.shape[0]
    r0 = np.clip(rows.reshape(-1).astype(np.int64), 0, P - 1)
    b = np.arange(r0.shape[0]) // clip_T
    out, mag = np.zeros((r0.shape[0], 3)), np.zeros((r0.shape[0], 3))
    for k in range(taps.shape[1]):
        term = taps[b, k].astype(np.float64)[:, None] * delta[(r0 + k) % P].astype(np.float64) * (1.0 if gain is None else gain[b].astype(np.float64))
        out, mag = out + term, mag + np.abs(term)
    return out.reshape(rows.shape + (3,)), mag.reshape(rows.shape + (3,))


def grad64(g, rows, clip_T, taps, gain, P):
    """the transpose in float64, the magnitudes, and the number of addends (hits) of every output"""
    out, mag, hits = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 1), np.int64)
    g, r = g.reshape(-1, 3).astype(np.float64), rows.reshape(-1)
    for i in range(r.shape[0]):
        if 0 <= r[i] < P:
            b = i // clip_T
            for k in range(taps.shape[1]):
                term = float(taps[b, k]) * (1.0 if gain is None else gain[b].astype(np.float64)) * g[i]
                out[(r[i] + k) % P] += term
                mag[(r[i] + k) % P] += np.abs(term)
                hits[(r[i] + k) % P] += 1
    return out, mag, hits


def test_one_tap_of_one_is_the_gather_and_the_ordered_sum():
    rng = np.random.default_rng(1)
    delta = rng.standard_normal((5, 3)).astype(np.float32)
    rows = rng.integers(0, 5, (4, 8)).astype(np.int32)
    g = rng.standard_normal((4, 8, 3)).astype(np.float32)
    one = np.ones((4, 1), np.float32)
    for gain in (None, np.ones((4, 3), np.float32)):
        assert np.array_equal(bits(vs.flicker_rows_mix(delta, rows, 8, one, gain)), bits(delta[rows]))
        want = np.zeros((5, 3), np.float32)
        np.add.at(want, rows.reshape(-1), g.reshape(-1, 3))           # unbuffered: added in ascending i
        assert np.array_equal(bits(vs.flicker_rows_mix_grad(g, rows, 8, one, gain, 5)), bits(want))
    loop = np.zeros((5, 3), np.float32)
    for i, r in enumerate(rows.reshape(-1)):
        loop[r] = loop[r] + g.reshape(-1, 3)[i]
    assert np.array_equal(bits(want), bits(loop))


def test_order_of_the_forward_is_the_stated_one():
    """acc = w0 * d0, then + w1 * d1, ..., then gain * acc, each rounded: against a scalar float32 loop"""
    rng = np.random.default_rng(2)
    for P, K in [(5, 4), (2, 4), (1, 3), (7, 2)]:
        delta = rng.standard_normal((P, 3)).astype(np.float32)
        rows = rng.integers(0, P, (3, 4)).astype(np.int32)
        taps, gain = tables(3, K, seed=P)
        got = vs.flicker_rows_mix(delta, rows, 4, taps, gain)
        for b in range(3):
            for t in range(4):
                for c in range(3):
                    acc = np.float32(taps[b, 0] * delta[rows[b, t], c])
                    for k in range(1, K):
                        acc = np.float32(acc + np.float32(taps[b, k] * delta[(rows[b, t] + k) % P, c]))
                    assert bits(got[b, t, c]) == bits(np.float32(gain[b, c] * acc))


def test_order_of_the_gradient_is_the_stated_one():
    """frames ascending, taps ascending, from +0, (gain * tap) * g: against a scalar float32 loop -- also with P < K, where one frame
    reaches a row through two taps"""
    rng = np.random.default_rng(3)
    for P, K in [(5, 4), (2, 4), (1, 4), (3, 4), (7, 2)]:
        rows = rng.integers(0, P, (3, 4)).astype(np.int32)
        g = rng.standard_normal((3, 4, 3)).astype(np.float32)
        taps, gain = tables(3, K, seed=10 + P)
        got = vs.flicker_rows_mix_grad(g, rows, 4, taps, gain, P)
        want = np.zeros((P, 3), np.float32)
        for i in range(12):
            b = i // 4
            for k in range(K):
                for c in range(3):
                    r = (rows.reshape(-1)[i] + k) % P
                    want[r, c] = np.float32(want[r, c] + np.float32(np.float32(gain[b, c] * taps[b, k]) * g.reshape(-1, 3)[i, c]))
        assert np.array_equal(bits(got), bits(want))
        if P < K:                                                     # P = 1: all K taps land on the one row
            assert grad64(g, rows, 4, taps, gain, P)[2].min() >= 12 * (K // P)


def test_minus_zero_is_kept_and_bad_rows_are_clamped_or_skipped():
    delta = np.array([[-0.0, 0.0, 1.0], [2.0, -0.0, -3.0], [4.0, 5.0, -0.0]], np.float32)
    rows = np.array([[0, 1, 2]], np.int32)
    got = vs.flicker_rows_mix(delta, rows, 3, np.ones((1, 1), np.float32), None)
    assert np.array_equal(bits(got[0]), bits(delta)) and np.signbit(got[0, 0, 0]) and not np.signbit(got[0, 0, 1])
    # a second tap of 0 adds +0: a -0 sum becomes +0 there, as IEEE addition has it -- which is why K = 1 tables carry no padding
    two = vs.flicker_rows_mix(delta, rows, 3, np.array([[1.0, 0.0]], np.float32), None)
    assert not np.signbit(two[0, 0, 0]) and np.array_equal(two, delta[None])
    # rows outside [0,P): the forward clamps them, the gradient skips them
    bad = np.array([[-1, 3, 7, -9, 2, 0]], np.int32)
    taps, gain = tables(1, 2, seed=4)
    assert np.array_equal(bits(vs.flicker_rows_mix(delta, bad, 6, taps, gain)), bits(vs.flicker_rows_mix(delta, np.clip(bad, 0, 2), 6, taps, gain)))
    g = np.random.default_rng(5).standard_normal((1, 6, 3)).astype(np.float32)
    g_skipped = g.copy()
    g_skipped[0, :4] = 0
    assert np.array_equal(vs.flicker_rows_mix_grad(g, bad, 6, taps, gain, 3), vs.flicker_rows_mix_grad(g_skipped, np.clip(bad, 0, 2), 6, taps, gain, 3))
    # unhit rows stay +0
    out = vs.flicker_rows_mix_grad(g[:, :1], np.array([[1]], np.int32), 1, np.ones((1, 1), np.float32), None, 4)
    assert np.array_equal(bits(out[[0, 2, 3]]), np.zeros((3, 3), np.uint32)) and np.array_equal(bits(out[1]), bits(g[0, 0]))


@pytest.mark.parametrize("P,K,nb,clip_T", [(5, 4, 6, 8), (2, 4, 3, 3), (1, 4, 2, 5), (682, 3, 4, 16), (8, 2, 300, 7)])
@pytest.mark.parametrize("with_gain", [False, True], ids=["nogain", "gain"])
def test_restatements_against_float64_and_as_transposes(P, K, nb, clip_T, with_gain):
    rng = np.random.default_rng(P * 10 + K)
    delta = rng.standard_normal((P, 3)).astype(np.float32)
    rows = rng.integers(0, P, (nb, clip_T)).astype(np.int32)
    g = rng.standard_normal((nb, clip_T, 3)).astype(np.float32)
    taps, gain = tables(nb, K, seed=P + K, gain=with_gain)
    m, gr = vs.flicker_rows_mix(delta, rows, clip_T, taps, gain), vs.flicker_rows_mix_grad(g, rows, clip_T, taps, gain, P)
    assert m.dtype == np.float32 and m.shape == (nb, clip_T, 3) and gr.dtype == np.float32 and gr.shape == (P, 3)
    # every output: (addends + K + 2) roundings of relative size 2^-24 at most, on the scale of the sum of the addends' magnitudes
    m64, m_mag = mix64(delta, rows, clip_T, taps, gain)
    assert (np.abs(m.astype(np.float64) - m64) <= (K + K + 2) * U * m_mag).all()
    g64, g_mag, hits = grad64(g, rows, clip_T, taps, gain, P)
    assert (np.abs(gr.astype(np.float64) - g64) <= (hits + K + 2) * U * g_mag).all()
    # adjoint identity <mix(delta), g> = <delta, mix_grad(g)>: both sides are sums of the same n*K*3 terms, each side off by its own bound
    lhs, rhs = (m.astype(np.float64) * g).sum(), (delta.astype(np.float64) * gr).sum()
    bound = ((K + K + 2) * U * m_mag * np.abs(g)).sum() + ((hits + K + 2) * U * g_mag * np.abs(delta)).sum()
    assert abs(lhs - rhs) <= bound and bound < 1e-3 * max(1.0, np.abs(m64 * g).sum())


def test_restatement_refusals():
    d, r, t = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32), np.ones((2, 2), np.float32)
    for bad in (lambda: vs.flicker_rows_mix(d.astype(np.float64), r, 3, t), lambda: vs.flicker_rows_mix(d, r.astype(np.float32), 3, t),
                lambda: vs.flicker_rows_mix(d, r, 4, t), lambda: vs.flicker_rows_mix(d, r, 3, np.ones((2, 5), np.float32)),
                lambda: vs.flicker_rows_mix(d, r, 3, np.ones((3, 2), np.float32)), lambda: vs.flicker_rows_mix(d, r, 3, t, np.ones((2, 2), np.float32)),
                lambda: vs.flicker_rows_mix_grad(np.zeros((2, 3, 2), np.float32), r, 3, t, None, 4),
                lambda: vs.flicker_rows_mix_grad(np.zeros((2, 3, 3), np.float32), r, 3, t, None, 0)):
        with pytest.raises(ValueError):
            bad()


# ---- CaptureChannel ----------------------------------------------------------------------------------------------------------------
def test_channel_draws_in_the_documented_order():
    kw = dict(subframe=(0.0, 1.0), exposure=(0.5, 2.0), gain=(0.8, 1.2), seed=7)
    a, b = vs.CaptureChannel(**kw), vs.CaptureChannel(**kw)
    d1, d2 = a.draw(3), a.draw(3)
    e1, e2 = b.draw(3), b.draw(3)
    for k in ("subframe", "exposure", "gain"):
        assert np.array_equal(d1[k], e1[k]) and np.array_equal(d2[k], e2[k]) and not np.array_equal(d1[k], d2[k])
    assert d1["subframe"].shape == (3,) and d1["exposure"].shape == (3,) and d1["gain"].shape == (3, 3) and d1["gain"].dtype == np.float32
    # the subframes, then the exposures, then the gains, from default_rng(seed)
    rng = np.random.default_rng(7)
    assert np.array_equal(d1["subframe"], rng.uniform(0.0, 1.0, 3)) and np.array_equal(d1["exposure"], rng.uniform(0.5, 2.0, 3))
    assert np.array_equal(d1["gain"], np.repeat(rng.uniform(0.8, 1.2, 3)[:, None], 3, 1).astype(np.float32))
    assert (d1["gain"][:, 0] == d1["gain"][:, 1]).all()              # "common": one gain for the three channels
    pc = vs.CaptureChannel(gain=(0.8, 1.2), gain_mode="per_channel", seed=7).draw(2)
    rng = np.random.default_rng(7)
    rng.uniform(0, 1, 2), rng.uniform(1, 1, 2)
    assert np.array_equal(pc["gain"], rng.uniform(0.8, 1.2, (2, 3)).astype(np.float32)) and (pc["gain"][:, 0] != pc["gain"][:, 1]).all()
    assert vs.CaptureChannel(seed=1).draw(4)["subframe"].tolist() != vs.CaptureChannel(seed=2).draw(4)["subframe"].tolist()


def test_channel_fixed_bounds_scalars_and_the_default():
    d = vs.CaptureChannel(subframe=0.3, exposure=(1.5, 1.5), gain=0.9).draw(4)
    assert d["subframe"].tolist() == [0.3] * 4 and d["exposure"].tolist() == [1.5] * 4 and np.array_equal(d["gain"], np.full((4, 3), 0.9, np.float32))
    d = vs.CaptureChannel().draw(1000)                                # sub-frame phase anywhere, exposure one row, gain 1
    assert (d["subframe"] >= 0).all() and (d["subframe"] < 1).all() and d["subframe"].min() < 0.05 and d["subframe"].max() > 0.95
    assert (d["exposure"] == 1).all() and (d["gain"] == 1).all()
    rgb = vs.CaptureChannel(subframe=0.3, exposure=1.5, gain=(0.9, 0.8, 0.7), gain_mode="per_channel")      # a known colour cast: three fixed gains
    assert np.array_equal(rgb.draw(2)["gain"], np.array([[0.9, 0.8, 0.7]] * 2, np.float32))
    with pytest.raises(ValueError, match="per_channel"):
        vs.CaptureChannel(gain=(0.9, 0.8, 0.7))
    taps, gain = vs.CaptureChannel.tables(vs.CaptureChannel(subframe=0.0).draw(2), 3)      # the identity channel: one tap of 1, no padding
    assert np.array_equal(taps, np.ones((6, 1), np.float32)) and np.array_equal(gain, np.ones((6, 3), np.float32))
    for bad in (dict(subframe=(0.5, 0.2)), dict(subframe=(0, 1.5)), dict(subframe=1.0), dict(exposure=(0, 3.5)), dict(exposure=-1), dict(gain=(-1, 1)),
                dict(gain=(1, np.inf)), dict(gain_mode="rgb"), dict(seed=0.5), dict(subframe=(0, 0.5, 1)), dict(exposure=np.nan)):
        with pytest.raises(ValueError, match="CaptureChannel"):
            vs.CaptureChannel(**bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="draw"):
            vs.CaptureChannel().draw(bad)


def test_channel_tables_share_a_videos_channel_and_pad_with_zeros():
    draw = {"subframe": np.array([0.0, 0.25, 0.9]), "exposure": np.array([1.0, 1.0, 3.0]),
            "gain": np.array([[1, 1, 1], [0.9, 0.8, 0.7], [0.5, 0.5, 0.5]], np.float32)}
    taps, gain = vs.CaptureChannel.tables(draw, 2)
    assert taps.dtype == np.float32 and gain.dtype == np.float32 and taps.shape == (6, 4) and gain.shape == (6, 3)
    for v in range(3):
        w = vs.capture_taps(draw["subframe"][v], draw["exposure"][v])
        for g in range(2):                                             # the G clips of a video share its channel
            assert np.array_equal(taps[2 * v + g, :len(w)], w) and (taps[2 * v + g, len(w):] == 0).all()
            assert np.array_equal(gain[2 * v + g], draw["gain"][v])
    assert taps[0].tolist() == [1, 0, 0, 0] and taps[2].tolist() == [0.75, 0.25, 0, 0] and (taps[4] > 0).all()
    # one channel: scalars and gain [3]
    t1, g1 = vs.CaptureChannel.tables({"subframe": 0.3, "exposure": 1.5, "gain": (0.9, 0.8, 0.7)}, 1)
    assert np.array_equal(t1, vs.capture_taps(0.3, 1.5)[None]) and np.array_equal(g1, np.array([[0.9, 0.8, 0.7]], np.float32))
    for bad in (dict(draw, extra=1), {"subframe": np.zeros(2), "exposure": np.ones(3), "gain": np.ones((2, 3))},
                {"subframe": np.zeros(2), "exposure": np.ones(2), "gain": np.ones((2, 2))}, [1, 2]):
        with pytest.raises(ValueError, match="tables"):
            vs.CaptureChannel.tables(bad, 1)
    with pytest.raises(ValueError, match="clips per video"):
        vs.CaptureChannel.tables(draw, 0)
    with pytest.raises(ValueError, match="sub-frame"):                 # a channel outside the model is refused where its taps are made
        vs.CaptureChannel.tables({"subframe": 1.0, "exposure": 1.0, "gain": (1, 1, 1)}, 1)


# ---- the C entry points and the constructors, without a GPU ---------------------------------------------------------------------------
def test_the_two_entry_points_in_header_library_and_binding():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flicker_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(flk_[a-z0-9_]+)\s*\(", src))
    for name in ("flk_flicker_rows_mix", "flk_flicker_rows_mix_grad"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    p = C.c_void_p(8)

    def mix(delta=p, P=5, rows=p, n=6, clip_T=3, taps=p, K=2, gain=None, out=p):
        return lib.flk_flicker_rows_mix(delta, P, rows, n, clip_T, taps, K, gain, out, None)

    def grad(g=p, rows=p, n=6, clip_T=3, taps=p, K=2, gain=None, P=5, out=p):
        return lib.flk_flicker_rows_mix_grad(g, rows, n, clip_T, taps, K, gain, P, out, None)

    # FLK_EINVAL with a reason that names the argument, before any GPU call (there is no GPU here)
    for call, nulls in ((mix, dict(delta=b"delta", rows=b"rows", taps=b"taps", out=b"delta_clip")),
                        (grad, dict(g=b"g_clip", rows=b"rows", taps=b"taps", out=b"g_rows"))):
        for arg, name in nulls.items():
            assert call(**{arg: None}) == -1 and name in lib.flk_last_error() and b"null" in lib.flk_last_error()
        for kw, name in ((dict(n=0), b"n must be"), (dict(n=-3), b"n must be"), (dict(n=7), b"clip_T"), (dict(clip_T=0), b"clip_T"),
                         (dict(clip_T=4), b"clip_T"), (dict(K=0), b"K "), (dict(K=5), b"K "), (dict(K=-1), b"K "), (dict(P=0), b"period"),
                         (dict(P=683), b"period")):
            assert call(**kw) == -1 and name in lib.flk_last_error(), (kw, lib.flk_last_error())


def test_constructor_refusals_touch_no_device():
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, check_flicker_time
    ch = vs.CaptureChannel()
    kw = dict(batch_size=2, sample_length=8, image_size=64)
    assert check_flicker_time("video", 5, 8, capture=ch) == 5 and check_flicker_time("video", None, 8, capture=None) == 8
    for bad in (dict(), dict(flicker_time="clip"), dict(flicker_time="video", attack_type="L12"), dict(flicker_time="video", per_clip=True),
                dict(attack_type="L12"), dict(per_clip=True)):
        with pytest.raises(ValueError, match="capture needs flicker_time='video'"):
            FlickerVideoResNet("r3d_18", None, capture=ch, **bad, **kw)
    with pytest.raises(ValueError, match="capture needs flicker_time='video'"):
        check_flicker_time("clip", None, 8, capture=ch)
    with pytest.raises(ValueError, match="CaptureChannel"):
        FlickerVideoResNet("r3d_18", None, flicker_time="video", capture={"subframe": 0.3}, **kw)


@pytest.mark.parametrize("script,files", [("r2plus1d_main_statistics_single_video_attack.py", ["--videos-npz"]),
                                          ("r2plus1d_main_universal_attack.py", ["--train-npz", "--val-npz"])])
def test_scripts_refuse_the_channel_off_video_time(script, files, tmp_path):
    """any --capture-* option without --flicker-time video is an argparse error (exit status 2), before a device is asked for"""
    import subprocess
    import sys
    import textwrap
    np.savez(tmp_path / "v.npz", labels=np.zeros(1, np.int64), video_00000=np.zeros((12, 8, 8, 3), np.uint8))
    path = os.path.join(ROOT, "scripts", script)
    base = [a for f in files for a in (f, str(tmp_path / "v.npz"))]
    # one interpreter for all the cases of a script: its main() under each argument list
    cases = [["--capture-subframe", "0", "1"], ["--capture-exposure", "0.5", "2"], ["--capture-gain", "0.8", "1"], ["--capture-gain-mode", "common"],
             ["--capture-seed", "3"], ["--eval-capture-draws", "4"], ["--flicker-time", "video", "--capture-exposure", "0.5", "4"]]
    code = textwrap.dedent(f"""
        import contextlib, io, runpy, sys
        for case in {cases!r}:
            sys.argv = [{path!r}] + {base!r} + case
            err = io.StringIO()
            try:
                with contextlib.redirect_stderr(err):
                    runpy.run_path({path!r}, run_name="__main__")
                print("RAN", case)
            except SystemExit as e:
                print("EXIT", e.code, err.getvalue().strip().splitlines()[-1])
        """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("EXIT", "RAN"))]
    assert r.returncode == 0 and len(lines) == len(cases), r.stdout + r.stderr
    for line in lines[:-1]:
        assert line.startswith("EXIT 2") and "needs --flicker-time video" in line, line
    assert lines[-1].startswith("EXIT 2") and "exposure" in lines[-1], lines[-1]
