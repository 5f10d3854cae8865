"""Projected sign-gradient (l-infinity PGD) optimiser on the GPU: the three kernels against the CPU restatement (oracle.attack_math +
torch.sign / clamp, fp64), the engines under ``optimizer="pgd"`` against fp64 oracle trajectories, per-clip and data-parallel modes,
and the scripts.

THE SIGN RULE.  A sign is discontinuous, so an element whose reference gradient has no defined sign at fp32 accuracy may be left out
of a comparison.  What may be left out is fixed from the fp64 restatement ALONE, and its cap is asserted BEFORE the GPU result is looked
at; a test whose cap is exceeded fails, it never passes on what is left.
* kernel level (the gradient is an input; only the sum g_scale * g_adv + reg can cancel): element i is left out when
  |g_tot64_i| < 1e-5 * (|g_scale * g_adv_i| + |reg64_i|) -- about 100 fp32 ulps of the terms.  Cap: flicker forms 0 elements, dense
  form 1e-4 of the elements.
* engine level, flicker (the gradient comes from the network): element i is left out when |g64_i| < 1e-4 * max|g64| (the engines' fp32
  delta-gradient is within 1e-3 relative of the fp64 oracle by the north-star tests, measured 3e-6).  Cap: 0 elements.
* engine level, dense: the dense gradient is heavy-tailed (84 % of its elements lie under 1e-4 * max|g64| on the I3D fixture), so the
  max-normalised rule is not used; see test_dense_i3d_engine.
Everywhere else the step is quantised (every element moves by exactly alpha or not at all), so results are compared to 1e-7 (kernels:
one fp32 rounding of delta - alpha) or 1e-6 (engines, accumulated over the steps) ABSOLUTE."""
import functools
import glob
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import attack_math as am
from oracle import i3d_ref
from oracle import videoresnet_ref as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16
ALPHA = 1e-3
BETAS = (1.0, 0.5, 0.5, 0.5)
KERNEL_TAU, ENGINE_TAU = 1e-5, 1e-4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


def pgd_ref(d, g, alpha, eps):
    """the step under test, restated: clamp(delta - alpha * sgn(g), -eps, +eps)"""
    return (d - alpha * torch.sign(g)).clamp(-eps, eps)


def kernel_left_out(g_adv64, reg64):
    """kernel-level sign rule: True where the fp64 sum cancels to within ~100 fp32 ulps of its terms"""
    return (g_adv64 + reg64).abs() < KERNEL_TAU * (g_adv64.abs() + reg64.abs())


# ---- kernel level -------------------------------------------------------------------------------------------------------------------
def flicker_reg_grad64(d, dialect, b0, b1, b2, b3, dyn):
    """b0 * d(reg)/d(delta) in fp64 for a [T,3] delta: the TF regulariser on the raw delta (kinetics_i3d_utils.py:172-186), the torch
    one on the clamped delta, through the clamp (model.py:198-209,1078)"""
    dv = d.double().clone().requires_grad_(True)
    if dialect == "tf":
        _, reg = am.tf_total_loss(0.0, dv.reshape(-1, 1, 1, 3), b0, b1, b2, b3)
    else:
        assert b2 == b3 == 1 - b1
        reg = am.torch_flicker_reg(dv.t().reshape(3, -1, 1, 1).clamp(-dyn, dyn), b1)
    (g,) = torch.autograd.grad(b0 * reg, dv)
    return g


def flicker_inputs(Tn, dialect, seed):
    rng = np.random.default_rng(seed)
    d = torch.from_numpy(rng.uniform(-0.25, 0.25, (Tn, 3)).astype(np.float32))
    d[1, 0], d[5, 2], d[Tn - 2, 1] = 0.47, -0.52, 0.41          # beyond both bounds (0.4 / 0.2): the projection returns them
    hp = dict(dialect=dialect, beta0=1.3, beta1=0.4, beta2=0.6, beta3=0.6, lr=ALPHA)
    eps = 0.4 if dialect == "tf" else 0.2                        # torch: many elements of U(+-0.25) lie beyond the clamp as well
    hp.update(dict(eps=eps) if dialect == "tf" else dict(dyn_max_norm=eps))
    reg = flicker_reg_grad64(d, dialect, hp["beta0"], hp["beta1"], hp["beta2"], hp["beta3"], eps)
    # g_adv on the scale of the regulariser gradient: neither term of g_tot dominates
    g = torch.from_numpy((rng.standard_normal((Tn, 3)) * float(reg.abs().mean())).astype(np.float32))
    return d, g, reg, eps, hp


@pytest.mark.parametrize("dialect", ["tf", "torch"])
@pytest.mark.parametrize("Tn", [16, 64, 90])
def test_reg_pgd_kernel(ops, Tn, dialect):
    """flk_perturb_reg_pgd against the restatement, elements beyond the clamp bound included; scalars bitwise those of
    flk_perturb_reg_adam for the same delta"""
    d, g, reg, eps, hp = flicker_inputs(Tn, dialect, seed=100 + Tn)
    out = int(kernel_left_out(g.double(), reg).sum())
    print(f"T={Tn} {dialect}: {out} of {d.numel()} elements left out by the kernel-level rule; "
          f"{int((d.abs() > eps).sum())} beyond the bound; mean|g_adv| / mean|reg| = {float(g.abs().mean() / reg.abs().mean()):.2f}")
    assert out == 0, "cap: the flicker forms leave nothing out"
    want = pgd_ref(d.double(), g.double() + reg, ALPHA, eps)
    dg = d.clone().cuda()
    sc = ops.perturb_reg_pgd(g.cuda(), dg, **hp).cpu()
    err = float((dg.cpu().double() - want).abs().max())
    print(f"  max |delta' - restatement| = {err:.2e}")
    assert err <= 1e-7
    assert float(dg.abs().max()) <= float(np.float32(eps))           # (the kernel's radius is the fp32 number)
    hp_adam = {k: v for k, v in hp.items() if k != "eps"}
    da = d.clone().cuda()
    sc_adam = ops.perturb_reg_adam(g.cuda(), da, torch.zeros_like(da), torch.zeros_like(da), 1, **hp_adam).cpu()
    assert torch.equal(sc, sc_adam)


@pytest.mark.parametrize("dialect", ["tf", "torch"])
def test_reg_pgd_sign_of_zero_and_nan(ops, dialect):
    """sgn(0) = 0: with beta0 = 0 the elements whose gradient is exactly zero (+0 or -0) are bitwise unchanged and the others move by
    exactly alpha (the fp32 difference); a NaN gradient gives a NaN delta, as torch.sign does"""
    Tn = 64
    rng = np.random.default_rng(7)
    d = torch.from_numpy(rng.uniform(-0.1, 0.1, (Tn, 3)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((Tn, 3)).astype(np.float32))
    zero = torch.from_numpy(rng.random((Tn, 3)) < 0.2)
    g[zero] = 0.0
    g[3, 1] = -0.0
    zero[3, 1] = True
    g[10, 2] = float("nan")
    zero[10, 2] = False
    kw = dict(eps=0.4) if dialect == "tf" else dict(dyn_max_norm=0.2)
    dg = d.clone().cuda()
    ops.perturb_reg_pgd(g.cuda(), dg, dialect=dialect, beta0=0.0, lr=ALPHA, **kw)
    got = dg.cpu()
    assert int(zero.sum()) > 20 and torch.equal(got[zero], d[zero])
    assert torch.isnan(got[10, 2]) and int(torch.isnan(got).sum()) == 1
    moved = ~zero
    moved[10, 2] = False
    want = d - torch.tensor(ALPHA, dtype=torch.float32) * torch.sign(g)          # fp32 arithmetic: one rounding
    assert torch.equal(got[moved], want[moved]) and bool((got[moved] != d[moved]).all())


@pytest.mark.parametrize("dialect", ["tf", "torch"])
def test_reg_pgd_batched_equals_the_one_clip_kernel(ops, dialect):
    """nclip = 5, mixed active flags, per-clip radii (torch dialect): every clip bitwise the single-clip entry point on its slice;
    inactive clips bitwise untouched, their counters not advanced, their scalars still written"""
    B, Tn = 5, 16
    rng = np.random.default_rng(31)
    d = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, Tn, 3)).astype(np.float32)).cuda()
    g = torch.from_numpy((rng.standard_normal((B, Tn, 3)) * 5e-3).astype(np.float32)).cuda()
    active = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32).cuda()
    steps = torch.tensor([0, 4, 8, 2, 7], dtype=torch.int32).cuda()
    bounds = [0.2, 0.1, 0.26, 0.15, 0.3]
    hp = dict(dialect=dialect, beta0=1.3, beta1=0.4, beta2=0.6, beta3=0.6, lr=ALPHA)
    d2 = d.clone()
    if dialect == "torch":
        sc = ops.perturb_reg_pgd_batched(g, d2, steps, active, dyn_max_norm_dev=torch.tensor(bounds).cuda(), **hp)
    else:
        sc = ops.perturb_reg_pgd_batched(g, d2, steps, active, eps=0.25, **hp)
    assert steps.tolist() == [1, 4, 9, 3, 7]
    for b in range(B):
        d1 = d[b].clone()
        sc1 = ops.perturb_reg_pgd(g[b].contiguous(), d1, **hp, **(dict(dyn_max_norm=bounds[b]) if dialect == "torch" else dict(eps=0.25)))
        assert torch.equal(sc[b], sc1), b
        if int(active[b]):
            assert torch.equal(d2[b], d1) and not torch.equal(d2[b], d[b]), b
        else:
            assert torch.equal(d2[b], d[b]), b
    # active = NULL: every clip is updated
    d3, st3 = d.clone(), torch.zeros(B, dtype=torch.int32).cuda()
    ops.perturb_reg_pgd_batched(g, d3, st3, None, **hp, **(dict(dyn_max_norm=0.2) if dialect == "torch" else dict(eps=0.25)))
    assert st3.tolist() == [1] * B and bool((d3 != d).flatten(1).any(1).all())


DENSE_SHAPE = (16, 224, 224, 3)


def dense_l12_grad64(d, beta, dialect, dyn):
    """beta * d(L12)/d(delta) in fp64: on the raw delta (kinetics_i3d_utils.py:409) or, torch dialect, on the clamped one (model.py:211-214)"""
    dv = d.double().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(beta * am.tf_l12(dv if dialect == "tf" else dv.clamp(-dyn, dyn)), dv)
    return g


@pytest.mark.parametrize("dialect", ["tf", "torch"])
def test_dense_l12_pgd_kernel(ops, dialect):
    """flk_perturb_dense_l12_pgd at [16,224,224,3].  beta = 0 with planted zeros: exact on every element.  beta = 1, delta ~ U(+-0.05),
    g_adv ~ 1e-5 N(0,1) (both terms matter), seed 11: the kernel-level rule leaves out ~8e-6 of the elements (cap 1e-4), the rest
    equals the restatement to 1e-7.  The radius (0.04) lies inside the range of delta: the projection is active."""
    rng = np.random.default_rng(11)
    d = torch.from_numpy(rng.uniform(-0.05, 0.05, DENSE_SHAPE).astype(np.float32))
    g = torch.from_numpy((1e-5 * rng.standard_normal(DENSE_SHAPE)).astype(np.float32))
    eps = 0.04
    kw = dict(dialect=dialect, lr=ALPHA, **(dict(eps=eps) if dialect == "tf" else dict(dyn_max_norm=eps)))
    # beta = 0
    g0 = g.clone()
    zero = torch.from_numpy(rng.random(DENSE_SHAPE) < 0.057)
    g0[zero] = 0.0
    dg = d.clone().cuda()
    ops.perturb_dense_l12_pgd(g0.cuda(), dg, beta=0.0, **kw)
    e32 = torch.tensor(eps, dtype=torch.float32)
    want = torch.minimum(torch.maximum(d - torch.tensor(ALPHA, dtype=torch.float32) * torch.sign(g0), -e32), e32)
    assert torch.equal(dg.cpu(), want)
    inside = zero & (d.abs() <= eps)
    assert torch.equal(dg.cpu()[inside], d[inside]) and int(inside.sum()) > 100000
    # beta = 1
    reg = dense_l12_grad64(d, 1.0, dialect, eps)
    out = kernel_left_out(g.double(), reg)
    n_out = int(out.sum())
    print(f"{dialect}: {n_out} of {d.numel()} elements left out ({n_out / d.numel():.1e}); mean|g_adv| / mean|reg| = "
          f"{float(g.abs().mean() / reg.abs().mean()):.2f}")
    assert n_out <= 1e-4 * d.numel(), "cap of the dense form"
    want = pgd_ref(d.double(), g.double() + reg, ALPHA, eps)
    dg = d.clone().cuda()
    sc = ops.perturb_dense_l12_pgd(g.cuda(), dg, beta=1.0, **kw).cpu()
    err = (dg.cpu().double() - want).abs()
    print(f"  max |delta' - restatement| outside the left-out set = {float(err[~out].max()):.2e}; sign flips inside it: {int((err[out] > 1e-7).sum())}")
    assert float(err[~out].max()) <= 1e-7
    da = d.clone().cuda()
    kw_adam = {k: v for k, v in kw.items() if k != "eps"}
    sc_adam = ops.perturb_dense_l12_adam(g.cuda(), da, torch.zeros_like(da), torch.zeros_like(da), 1, beta=1.0, **kw_adam).cpu()
    assert torch.equal(sc, sc_adam)


# ---- engine level: I3D ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def i3d_fixture():
    from flickering_adversarial_video_amd import i3d_spec
    from oracle import fixtures
    xu = torch.from_numpy(i3d_spec.synthetic_clip_u8(1, T, seed=1234))
    W = fixtures.coherent_i3d_weights(xu, seed=5, label=233)
    return W, {k: torch.from_numpy(v).double() for k, v in W.items()}, xu


def i3d_pgd_trajectory(W64, xu, steps, eps=0.4, d0=None):
    """the single-video loop (i3d_adversarial_main_single_video_npy.py:211-217) under the projected sign-gradient step, fp64, from
    delta = 0: per step the pre-update delta, the gradient of the total loss, its adversarial part, the loss terms and the new delta"""
    x = xu.double() / 128 - 1
    label = i3d_ref.i3d_logits(x, W64).argmax(-1)
    d = torch.zeros(T, 1, 1, 3, dtype=torch.float64) if d0 is None else d0.double().clone()
    out = []
    for _ in range(steps):
        dv = d.clone().requires_grad_(True)
        lg = i3d_ref.i3d_logits(am.tf_apply(x, dv), W64)
        adv, _, _ = am.tf_improve_adversarial_loss(lg, label, 0.05, False, False)
        total, reg = am.tf_total_loss(adv, dv, *BETAS)
        (g_reg,) = torch.autograd.grad(BETAS[0] * reg, dv, retain_graph=True)
        (g,) = torch.autograd.grad(total, dv)
        new = pgd_ref(d, g, ALPHA, eps)
        out.append(dict(before=d.clone(), g=g.clone(), g_adv=g - g_reg, adv=adv.item(), total=total.item(), logits=lg.detach(), delta=new.clone()))
        d = new
    return label, out


@functools.lru_cache(maxsize=None)
def i3d_single_clip_trajectory():
    W, W64, xu = i3d_fixture()
    return i3d_pgd_trajectory(W64, xu, 6)


def assert_flicker_cap(traj, what):
    """engine-level sign rule, flicker: nothing may lie under 1e-4 * max|g64|"""
    for it, s in enumerate(traj):
        ratio = float(s["g"].abs().min() / s["g"].abs().max())
        print(f"{what} step {it + 1}: min|g64| / max|g64| = {ratio:.1e}")
        assert int((s["g"].abs() < ENGINE_TAU * s["g"].abs().max()).sum()) == 0, f"{what}: the fixture leaves elements out at step {it + 1}"


def test_i3d_engine_fp32_trajectory():
    """I3D fp32, 6 free-running PGD steps from delta = 0 on the well-conditioned fixture (eps 0.4, betas (1, .5, .5, .5)): the
    perturbation equals the fp64 oracle's to 1e-6 absolute at every step, adversarial and total loss within 1e-3, same iteration-to-fool"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    W, W64, xu = i3d_fixture()
    label, t64 = i3d_single_clip_trajectory()
    assert int(label) == 233
    assert_flicker_cap(t64, "I3D")
    eng = FlickerI3D(W, batch_size=1, frames=T, dtype="f32", optimizer="pgd")
    assert eng.adam_m is None and eng.adam_v is None and eng.pgd_eps == 0.4
    fooled = {"hip": None, "oracle": None}
    for it, s in enumerate(t64):
        res = eng.step(xu.cuda(), label.cuda(), lr=ALPHA, beta0=BETAS[0], beta1=BETAS[1], beta2=BETAS[2], beta3=BETAS[3], margin=0.05).host()
        err = float((eng.perturbation.cpu().double() - s["delta"]).abs().max())
        print(f"iter {it + 1}: adv {res['adv_loss']:.7f} (oracle {s['adv']:.7f}), total {res['total_loss']:.7f} (oracle {s['total']:.7f}), max |delta - oracle| {err:.2e}")
        assert err <= 1e-6
        assert res["adv_loss"] == pytest.approx(s["adv"], rel=1e-3, abs=1e-7) and res["total_loss"] == pytest.approx(s["total"], rel=1e-3, abs=1e-7)
        for k, lg in (("hip", eng._logits.cpu()), ("oracle", s["logits"])):
            if fooled[k] is None and int(lg.argmax()) != int(label):
                fooled[k] = it
    assert fooled["hip"] == fooled["oracle"]
    eng.reset_perturbation()
    assert float(eng.perturbation.abs().max()) == 0 and eng.adam_m is None


def test_i3d_engine_bf16_moves_in_the_oracles_direction():
    """bf16: no bound is fixed in advance.  The bf16 engine's delta-gradient error against the fp64 oracle is MEASURED under the
    existing Adam path (eng.delta_gradient() at the oracle's first 4 states, max-abs error over max|g64|); tau_bf16 = twice that
    (margin for launch-layout differences between runs).  Under PGD every element with |g64| >= tau_bf16 * max|g64| must then move in
    the oracle's direction at each of 4 teacher-forced steps (the oracle's delta is loaded before each step: PGD has no other state).
    Condition, from the oracle alone: at most 12 of the 48 elements lie under tau_bf16 * max|g64| at any step.
    Measured on MI355X: see DESIGN.md (projected sign-gradient optimiser)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    W, W64, xu = i3d_fixture()
    label, t64 = i3d_single_clip_trajectory()
    t64 = t64[:4]
    hp = dict(lr=ALPHA, beta0=BETAS[0], beta1=BETAS[1], beta2=BETAS[2], beta3=BETAS[3], margin=0.05)
    eng = FlickerI3D(W, batch_size=1, frames=T, dtype="bf16")
    errs = []
    for s in t64:
        eng.reset_perturbation(s["before"].float().numpy())
        eng.step(xu.cuda(), label.cuda(), update=False, **hp)
        errs.append(float((eng.delta_gradient().cpu().double().reshape(T, 1, 1, 3) - s["g_adv"]).abs().max() / s["g_adv"].abs().max()))
    del eng
    tau = 2 * max(errs)
    left = [int((s["g"].abs() < tau * s["g"].abs().max()).sum()) for s in t64]
    print(f"bf16 delta-gradient error under the Adam path, per state: {['%.2e' % e for e in errs]}; tau_bf16 = {tau:.2e}; left out per step: {left} of 48")
    assert max(left) <= 12, f"tau_bf16 = {tau:.2e} leaves out {left} of 48 elements: the bf16 gradient is too coarse for this fixture"
    eng = FlickerI3D(W, batch_size=1, frames=T, dtype="bf16", optimizer="pgd")
    for it, s in enumerate(t64):
        eng.reset_perturbation(s["before"].float().numpy())
        before = eng.perturbation.cpu().clone()
        eng.step(xu.cuda(), label.cuda(), **hp)
        moved = torch.sign(before.double() - eng.perturbation.cpu().double())
        keep = s["g"].abs() >= tau * s["g"].abs().max()
        wrong = int((moved[keep] != torch.sign(s["g"])[keep]).sum())
        print(f"step {it + 1}: {int(keep.sum())} elements compared, {wrong} moved against the oracle")
        assert wrong == 0


def test_dense_i3d_engine():
    """dense I3D, fp32, beta = 0 and beta = 1, 2 steps each.  (a) Wiring, every element: delta' equals clamp(delta - alpha *
    sgn(g_tot), +-eps) recomputed in fp64 from the engine's OWN dense gradient of that step (eng._gdense) and the pre-update delta, under
    the kernel-level rule and its dense cap.  (b) Against the fp64 oracle (evaluated at the engine's pre-update delta), on the part of
    the gradient that has a sign: over the elements with |g64| >= 1e-3 * max|g64| the moved direction sgn(delta - delta') equals
    sgn(g64) without exception; that set must hold at least 5 % of the elements (asserted from the oracle first)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    W, W64, xu = i3d_fixture()
    x64 = xu.double() / 128 - 1
    label = torch.tensor([233])
    eps = 0.05
    eng = FlickerI3D(W, batch_size=1, frames=T, dtype="f32", dense_delta=True, optimizer="pgd", pgd_eps=eps)
    assert eng.adam_m is None
    with pytest.raises(ValueError, match="pgd_eps"):
        FlickerI3D(W, batch_size=1, frames=T, dtype="f32", dense_delta=True, optimizer="pgd")
    for beta in (0.0, 1.0):
        eng.reset_perturbation()
        for it in range(2):
            before = eng.perturbation.cpu().clone()
            dv = before.double().clone().requires_grad_(True)
            lg = i3d_ref.i3d_logits(am.tf_apply(x64, dv, clip_delta=False), W64)
            adv, _, _ = am.tf_improve_adversarial_loss(lg, label, 0.05, False, False)
            (g64,) = torch.autograd.grad(adv + beta * am.tf_l12(dv), dv)
            keep = g64.abs() >= 1e-3 * g64.abs().max()
            frac = float(keep.double().mean())
            print(f"beta {beta} step {it + 1}: {frac:.1%} of the elements have |g64| >= 1e-3 max|g64|; {float((g64 == 0).double().mean()):.1%} are exactly zero")
            assert frac >= 0.05
            eng.step(xu.cuda(), label.cuda(), lr=ALPHA, beta0=1.0, beta1=beta, margin=0.05)
            after = eng.perturbation.cpu()
            # (a) wiring
            g_adv = eng._gdense.cpu().double()
            reg = dense_l12_grad64(before, beta, "tf", 0.0) if beta else torch.zeros_like(g_adv)
            out = kernel_left_out(g_adv, reg) if beta else torch.zeros_like(keep)
            assert int(out.sum()) <= 1e-4 * out.numel()
            err = (after.double() - pgd_ref(before.double(), g_adv + reg, ALPHA, eps)).abs()
            print(f"  (a) {int(out.sum())} left out; max error elsewhere {float(err[~out].max()):.2e}")
            assert float(err[~out].max()) <= 1e-7
            # (b) direction
            wrong = int((torch.sign(before.double() - after.double())[keep] != torch.sign(g64)[keep]).sum())
            print(f"  (b) {int(keep.sum())} elements compared with the oracle, {wrong} moved against it")
            assert wrong == 0


HP = dict(lr=ALPHA, beta0=1.0, beta1=0.5, beta2=0.5, beta3=0.5, margin=0.05)


def test_per_clip_i3d_pgd_is_bitwise_the_single_runs():
    """B = 3 clips under PGD in per-clip mode vs each clip attacked alone (fp32): logits, gradient, perturbation and scalars bitwise
    equal; a retired clip stops moving and its counter stops; reset_clip restarts delta and counter only"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import i3d_spec
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    B = 3
    W = i3d_spec.synthetic_i3d_weights(42)
    xu = torch.from_numpy(i3d_spec.synthetic_clip_u8(B, T, seed=21)).cuda()
    engB = FlickerI3D(W, batch_size=B, frames=T, dtype="f32", per_clip_delta=True, optimizer="pgd")
    eng1 = FlickerI3D(W, batch_size=1, frames=T, dtype="f32", optimizer="pgd")
    assert engB.adam_m is None
    labels = engB.logits(xu, adv_flag=0.0).argmax(-1).clone()
    singles = []
    for b in range(B):
        eng1.reset_perturbation()
        tr = []
        for it in range(4):
            r = eng1.step(xu[b:b + 1].contiguous(), labels[b:b + 1].contiguous(), **HP)
            tr.append(dict(logits=eng1._logits.clone(), g=eng1.delta_gradient().clone(), d=eng1.eps_rgb.clone(), reg=r["reg_loss"].clone()))
        singles.append(tr)
    for it in range(4):
        if it == 2:
            engB.active[1] = 0
            frozen = engB.eps_rgb[1].clone()
        r = engB.step(xu, labels, **HP)
        for b in range(B):
            s = singles[b][it]
            if b == 1 and it >= 2:
                assert torch.equal(engB.eps_rgb[1], frozen) and int(engB.adam_steps[1]) == 2
                continue
            assert torch.equal(engB._logits[b], s["logits"][0]) and torch.equal(engB.delta_gradient()[b], s["g"]), (it, b)
            assert torch.equal(engB.eps_rgb[b], s["d"]) and torch.equal(r["reg_loss"][b], s["reg"].reshape(())), (it, b)
            assert int(engB.adam_steps[b]) == it + 1
    engB.reset_clip(1)
    assert int(engB.active[1]) == 1 and int(engB.adam_steps[1]) == 0 and float(engB.eps_rgb[1].abs().max()) == 0
    engB.step(xu, labels, **HP)
    assert torch.equal(engB.eps_rgb[1], singles[1][0]["d"])


# ---- engine level: VideoResNet ------------------------------------------------------------------------------------------------------
VT, VHW = 16, 112


def test_r2plus1d_engine_fp32_trajectory():
    """r2plus1d_18 fp32 on the fixture of test_videoresnet_attack_trajectory_well_conditioned (eps = l_inf_pert_norm 0.2, the same
    Losses settings), 4 free-running PGD steps from delta = 0 -- not 6: at step 5 one element of the oracle gradient falls under the
    engine-level bound (5.9e-5 of the maximum).  Same assertions as the I3D trajectory."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    from oracle import fixtures
    arch, steps = "r2plus1d_18", 4
    x_cl = torch.from_numpy(vs.synthetic_clip(1, VT, VHW, VHW, seed=5))
    x = x_cl.permute(0, 4, 1, 2, 3).contiguous()
    W = fixtures.coherent_videoresnet_weights(vs.synthetic_weights(arch, 42), x, arch, label=233)
    W64 = {k: torch.from_numpy(v).double() for k, v in W.items()}
    xd = x.double()
    label = vr.videoresnet_logits(xd, W64, arch).argmax(-1)
    assert int(label) == 233
    d = torch.zeros(3, VT, 1, 1, dtype=torch.float64)
    t64 = []
    for _ in range(steps):
        dv = d.clone().requires_grad_(True)
        logits = vr.videoresnet_logits(am.torch_apply(xd, dv, 0.2), W64, arch)
        loss, adv, reg = am.torch_losses(label, logits, torch.softmax(logits, 1), dv.clamp(-0.2, 0.2), 0.5, 1.0, 0.05, True, True, "flickering")
        (g,) = torch.autograd.grad(loss, dv)
        d = pgd_ref(d, g, ALPHA, 0.2)
        t64.append(dict(g=g.clone(), adv=adv.item(), total=loss.item(), logits=logits.detach(), delta=d.clone()))
    assert_flicker_cap(t64, arch)
    eng = FlickerVideoResNet(arch, W, batch_size=1, sample_length=VT, image_size=VHW, dtype="f32", l_inf_pert_norm=0.2, optimizer="pgd")
    assert eng.adam_m is None and eng.adam_v is None
    eng.pert_model.init_perturbation(np.zeros((3, VT, 1, 1), np.float32))
    crit = Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)
    fooled = {"hip": None, "oracle": None}
    for it, s in enumerate(t64):
        res = eng.step(x_cl.cuda(), label.cuda(), crit, lr=ALPHA).host()
        delta = eng.pert_model.perturbation.cpu().t().reshape(3, VT, 1, 1)
        err = float((delta.double() - s["delta"]).abs().max())
        print(f"iter {it + 1}: adv {float(res['adv_loss']):.7f} (oracle {s['adv']:.7f}), total {float(res['loss']):.7f} (oracle {s['total']:.7f}), "
              f"max |delta - oracle| {err:.2e}")
        assert err <= 1e-6
        assert float(res["adv_loss"]) == pytest.approx(s["adv"], rel=1e-3, abs=1e-7) and float(res["loss"]) == pytest.approx(s["total"], rel=1e-3, abs=1e-7)
        for k, lg in (("hip", eng._logits.cpu()), ("oracle", s["logits"])):
            if fooled[k] is None and int(lg.argmax()) != int(label):
                fooled[k] = it
    assert fooled["hip"] == fooled["oracle"]


def test_per_clip_r2plus1d_pgd_is_bitwise_the_single_runs():
    """r2plus1d_18 fp32: 3 clips with 3 perturbations and 3 clamp bounds (= PGD radii; the restart schedule grows them per video,
    model.py:1061-1066) in one per-clip batch vs each clip alone, 4 PGD iterations: logits, loss terms and perturbation bitwise equal"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    B, Tn, HW, arch = 3, 8, 64, "r2plus1d_18"
    W = vs.synthetic_weights(arch, 42)
    mk = lambda b, pc: FlickerVideoResNet(arch, W, batch_size=b, sample_length=Tn, image_size=HW, dtype="f32", l_inf_pert_norm=0.2, per_clip=pc,
                                          optimizer="pgd")
    engB, eng1 = mk(B, True), mk(1, False)
    assert engB.adam_m is None
    x = torch.from_numpy(vs.synthetic_clip(B, Tn, HW, HW, seed=3)).cuda()
    labels = engB.logits(x).argmax(-1).clone()
    rng = np.random.default_rng(6)
    d0 = [rng.uniform(-0.25, 0.25, (3, Tn, 1, 1)).astype(np.float32) for _ in range(B)]
    bounds = [0.2, 0.1, 0.26]
    crit = Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)
    singles = []
    for b in range(B):
        eng1.pert_model.init_perturbation(d0[b])
        eng1.pert_model.dynamic_max_norm = bounds[b]
        tr = []
        for it in range(4):
            r = eng1.step(x[b:b + 1].contiguous(), labels[b:b + 1].contiguous(), crit, lr=ALPHA)
            tr.append((eng1._logits.clone(), r["adv_loss"].clone(), r["reg_loss"].clone(), eng1.pert_model.perturbation.clone()))
        assert float(eng1.pert_model.perturbation.abs().max()) <= float(np.float32(bounds[b]))
        singles.append(tr)
    for b in range(B):
        engB.pert_model.init_clip(b, d0[b], max_norm=bounds[b])
    for it in range(4):
        r = engB.step(x, labels, crit, lr=ALPHA)
        for b in range(B):
            lg, adv, reg, d = singles[b][it]
            assert torch.equal(engB._logits[b], lg[0]) and torch.equal(r["adv_loss"][b], adv.reshape(())) and torch.equal(r["reg_loss"][b], reg.reshape(())), (it, b)
            assert torch.equal(engB.pert_model.perturbation[b], d), (it, b)
    assert engB.adam_steps.tolist() == [4, 4, 4]


@pytest.mark.parametrize("family", ["i3d", "r2plus1d_18"])
def test_adam_keyword_is_bitwise_the_default_engine(family):
    """optimizer="adam" is the engine built without the keyword: 3 bf16 steps, perturbation, moments and logits bitwise equal"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    runs = []
    for kw in (dict(), dict(optimizer="adam")):
        if family == "i3d":
            from flickering_adversarial_video_amd import i3d_spec
            from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
            xu = torch.from_numpy(i3d_spec.synthetic_clip_u8(1, T, seed=1234)).cuda()
            eng = FlickerI3D(i3d_spec.synthetic_i3d_weights(42), batch_size=1, frames=T, dtype="bf16", **kw)
            label = eng.logits(xu, adv_flag=0.0).argmax(-1).clone()
            for _ in range(3):
                eng.step(xu, label, **HP)
            runs.append((eng.eps_rgb.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng._logits.clone(), eng.adam_t))
        else:
            from flickering_adversarial_video_amd import videoresnet_spec as vs
            from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
            x = torch.from_numpy(vs.synthetic_clip(1, 8, 64, 64, seed=3)).cuda()
            eng = FlickerVideoResNet(family, vs.synthetic_weights(family, 42), batch_size=1, sample_length=8, image_size=64, dtype="bf16",
                                     l_inf_pert_norm=0.2, **kw)
            eng.pert_model.init_perturbation(np.zeros((3, 8, 1, 1), np.float32))
            label = eng.logits(x).argmax(-1).clone()
            crit = Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)
            for _ in range(3):
                eng.step(x, label, crit, lr=ALPHA)
            runs.append((eng.pert_model.perturbation.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng._logits.clone(), eng.adam_t))
        del eng
    for a, b in zip(*runs):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert float(runs[0][0].abs().max()) > 0


# ---- data-parallel ------------------------------------------------------------------------------------------------------------------
DP_STEPS = 2


def _dp_data():
    from flickering_adversarial_video_amd import i3d_spec
    W, W64, xu = i3d_fixture()
    x2 = torch.cat([xu, torch.from_numpy(i3d_spec.synthetic_clip_u8(1, T, seed=4321))])
    return W, W64, x2


def _dp_run(eng, x, labels):
    deltas = []
    for _ in range(DP_STEPS):
        eng.step(x, labels, **HP)
        deltas.append(eng.perturbation.cpu().numpy().copy())
    return deltas


def _dp_worker(rk, world, port, labels, q):
    import torch.distributed as dist
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rk, world_size=world)
    try:
        W, _, x2 = _dp_data()
        eng = FlickerI3D(W, batch_size=1, frames=T, dtype="f32", device=0, optimizer="pgd")
        assert eng.world == world
        q.put((rk, _dp_run(eng, x2[rk:rk + 1].cuda(), labels[rk:rk + 1].cuda())))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_under_pgd():
    """two data-parallel ranks x one clip against one process x two clips (the arrangement of tests/test_dp_gpu.py) under PGD on the
    well-conditioned weights: the sign is taken after the all-reduce, so the replicas stay bitwise identical; against the single
    process -- and the fp64 oracle of the two-clip batch -- the perturbation is equal to 1e-6 under the flicker engine-level rule
    (its cap of 0 left-out elements asserted from the oracle first)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import torch.multiprocessing as mp
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    W, W64, x2 = _dp_data()
    labels, t64 = i3d_pgd_trajectory(W64, x2, DP_STEPS)
    assert labels.tolist() == [233, 233]
    assert_flicker_cap(t64, "I3D, two clips")
    eng = FlickerI3D(W, batch_size=2, frames=T, dtype="f32", device=0, optimizer="pgd")
    ref = _dp_run(eng, x2.cuda(), labels.cuda())
    del eng
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(rk, 2, port, labels, q)) for rk in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for it in range(DP_STEPS):
        np.testing.assert_array_equal(got[0][it], got[1][it])                 # replicas: bitwise
        np.testing.assert_allclose(got[0][it], ref[it], rtol=0, atol=1e-6)
        np.testing.assert_allclose(ref[it], t64[it]["delta"].numpy(), rtol=0, atol=1e-6)


# ---- scripts ------------------------------------------------------------------------------------------------------------------------
def test_class_gen_script_under_pgd(tmp_path):
    """OPTIMIZER: pgd in CLASS_GEN_ATTACK on the tiny configuration of tests/test_scripts_gpu.py: the script finishes, res.pkl keeps
    its keys, checkpoints carry no moments, the run resumes, and a resume under the other optimiser is refused naming both"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import i3d_spec, tf_checkpoint, tfrecord_io as tio
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    Tn, B = 16, 2
    (tmp_path / "rec").mkdir()
    u8 = i3d_spec.synthetic_clip_u8(5, Tn + 2, seed=9)
    eng = FlickerI3D(i3d_spec.synthetic_i3d_weights(42), batch_size=1, frames=Tn, dtype="f32")
    labels = [int(eng(torch.from_numpy(u8[i:i + 1, -Tn:]).cuda(), adv_flag=0).argmax()) for i in range(5)]
    del eng
    tio.write_records(str(tmp_path / "rec" / "a.tfrecords"), [tio.make_example(u8[i], labels[i]) for i in range(5)], with_payload_crc=False)
    (tmp_path / "labels.txt").write_text("\n".join(f"class {i}" for i in range(400)))
    cfg = open(os.path.join(ROOT, "run_config.yml")).read().replace("'data/label_map.txt'", f"'{tmp_path}/labels.txt'")
    cfg = cfg.replace("['data/kinetics/database/tfrecord/test/hula hooping']", f"['{tmp_path}/rec']")
    cfg = cfg.replace("PKL_RESULT_PATH: 'result/generalization/model_gen_one_class/'", f"PKL_RESULT_PATH: '{tmp_path}/out/'")
    cfg = cfg.replace("BATCH_SIZE: 8\n    MAX_NUM_STEP: 10000\n    TARGETED_ATTACK: False\n    TARGETED_CLASS: 'javelin throw'",
                      f"BATCH_SIZE: {B}\n    MAX_NUM_STEP: 10000\n    TARGETED_ATTACK: False\n    TARGETED_CLASS: 'javelin throw'", 1)
    head, tail = cfg.split("CLASS_GEN_ATTACK:")
    sec, rest = tail.split("UNIVERSAL_ATTACK:")
    pgd_cfg = head + "CLASS_GEN_ATTACK:" + sec.replace("OPTIMIZER: 'adam'", "OPTIMIZER: 'pgd' ").replace("PGD_EPS: 0.4", "PGD_EPS: 0.3") + "UNIVERSAL_ATTACK:" + rest
    assert pgd_cfg.count("OPTIMIZER: 'pgd'") == 1 and "PGD_EPS: 0.3" in pgd_cfg
    (tmp_path / "pgd.yml").write_text(pgd_cfg)
    (tmp_path / "adam.yml").write_text(cfg)
    script = os.path.join(ROOT, "scripts", "i3d_adversarial_main_single_class_gen.py")
    tailargs = ["--frames", str(Tn), "--dtype", "f32", "--no-weights-in-checkpoint"]
    r = subprocess.run([sys.executable, script, str(tmp_path / "pgd.yml")] + tailargs + ["--max-steps", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Step: 00003" in r.stdout and "fool_rate" in r.stdout
    ck = tf_checkpoint.read_bundle(str(tmp_path / "out" / "model_step_00003"), verify_crc=True)
    assert set(ck) == {"RGB/eps", "pgd_steps"} and int(ck["pgd_steps"]) == 3
    # 3 sign steps of 1e-3 from zero: every element is a multiple of alpha within [-3, 3] alpha
    q = ck["RGB/eps"] / np.float32(ALPHA)
    assert ck["RGB/eps"].shape == (Tn, 1, 1, 3) and np.abs(q).max() <= 3 + 1e-3 and np.abs(q - np.round(q)).max() < 1e-3 and np.abs(q).max() >= 1
    res = pickle.load(open(tmp_path / "out" / "res.pkl", "rb"))
    assert set(res) == {"total_loss_l", "adv_loss_l", "reg_loss_l", "norm_reg_loss_l", "diff_norm_reg_loss_l", "perturbation", "total_steps",
                        "beta_1", "beta_2", "fatness", "smoothness", "fool_rate"}
    assert res["total_steps"] == 3 and len(res["total_loss_l"]) == 3 and np.isfinite(res["total_loss_l"]).all()
    r = subprocess.run([sys.executable, script, str(tmp_path / "pgd.yml")] + tailargs + ["--max-steps", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resumed from" in r.stdout and "at step 3" in r.stdout and os.path.exists(tmp_path / "out" / "model_step_00005.index")
    r = subprocess.run([sys.executable, script, str(tmp_path / "adam.yml")] + tailargs + ["--max-steps", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "OPTIMIZER: pgd" in r.stderr and "OPTIMIZER: adam" in r.stderr and "cannot be resumed" in r.stderr


def test_r2plus1d_statistics_script_under_pgd(tmp_path):
    """--optimizer pgd on the single-video statistics script (tiny configuration of tests/test_scripts_gpu.py): it finishes and the
    result files carry the usual keys; the perturbation stays inside the clamp bound"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    Tn = 8
    norm = vs.synthetic_clip(1, Tn, seed=6)
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=1, sample_length=Tn, dtype="f32")
    lab = [int(eng.logits(torch.from_numpy(norm[:1]).cuda(), False).argmax())]
    del eng
    np.savez(tmp_path / "v.npz", clips=norm, labels=np.array(lab), names=np.array(["clipA"]))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_statistics_single_video_attack.py"), "--videos-npz", str(tmp_path / "v.npz"),
           "--results-root", str(tmp_path / "res"), "--base-model", "r3d_18", "--dtype", "f32", "--n-iter", "3", "--restart-after", "40",
           "--optimizer", "pgd", "--reset-optimizer-per-video"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    files = glob.glob(str(tmp_path / "res" / "r3d_18" / "single_video_attack" / "flickering" / "*" / "*.npy"))
    assert len(files) == 1
    ra = np.load(files[0], allow_pickle=True).tolist()
    assert set(ra) == {"loss/total", "loss/adv_loss", "loss/reg_loss", "perturbation/thickness", "perturbation/roughness", "perturbation/inf_norm",
                       "perturbation", "prob_clean_input", "label", "is_adversarial", "max_prob", "correct_cls_prob", "restarts"}
    assert len(ra["loss/total"]) >= 3 and ra["perturbation"][0].shape == (3, Tn, 1, 1) and np.isfinite(ra["loss/total"]).all()
    assert ra["perturbation/inf_norm"] <= 0.2 * 1.3 ** 4 + 1e-6
    r = subprocess.run(cmd[:cmd.index("--optimizer")] + ["--optimizer", "sgd"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "invalid choice" in r.stderr
