"""R(2+1)D-34 victims and 32-frame temporal convolutions on the GPU.

- conv_t3_dma_kernel over 16-frame temporal tiles (T = 32 / 48): forward with the full epilogue and data-gradient with the ReLU mask
  against torch-CPU conv3d / its autograd, bitwise against the halo kernel, and the launch seen to take the ring (FLK_CONV_DBG).
- The R(2+1)D-34 plan (and r2plus1d_18 with a replaced fc head) against a CPU restatement of the upstream network written out here
  (moabitcoin/ig65m-pytorch models.py: torchvision VideoResNet(BasicBlock, [Conv2Plus1D] * 4, [3, 4, 6, 3], R2Plus1dStem), midplanes
  288 / 576 / 1152 in layer{2,3,4}[0].conv2, BatchNorm3d eps 1e-3), with test_videoresnet_gpu.py's method and tolerances.
- The statistics script with --base-model ig65m."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import attack_math as am

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale)


def q(x):
    return x.to(torch.bfloat16).float()


def tol(ref):
    s = float(ref.abs().max()) + 1e-12
    return 1e-2, 1e-2 * s


def conv_t(x_cl, w_dhwio):
    """torch-CPU (3,1,1) convolution, pad 1 in t: x [B,T,H,W,C] fp32, w [3,1,1,Cin,Cout] -> [B,T,H,W,Cout]"""
    y = F.conv3d(x_cl.permute(0, 4, 1, 2, 3), w_dhwio.permute(4, 3, 0, 1, 2), padding=(1, 0, 0))
    return y.permute(0, 2, 3, 4, 1).contiguous()


T3_TILED = [
    # name, B, T, H, W, cin (real), cout, nf -- two / three 16-frame tiles per clip, several clips per launch
    ("T32_144_64_nf4", 2, 32, 8, 8, 144, 64, 4),        # layer1's temporal half: interior tiles fetch frames t0 - 1 / t0 + 16
    ("T48_64_144_ragged", 3, 48, 6, 8, 64, 144, 4),     # three tiles in t, 3 chunks per frame, 2.25 channel tiles
    ("T32_45_64_stem3", 2, 32, 12, 12, 45, 64, 4),      # stem.3: 45 channels padded to 48 like the plan (a half slab of zeros)
    ("T32_288_128_nf8", 2, 32, 8, 8, 288, 128, 8),      # nf = 8
]


def _t3_operands(case):
    _, B, T, H, W, cin, cout, nf = case
    cp = (cin + 7) // 8 * 8
    x = torch.zeros((B, T, H, W, cp))
    x[..., :cin] = q(rnd((B, T, H, W, cin), 71))
    w = torch.zeros((3, 1, 1, cp, cout))
    w[..., :cin, :] = q(rnd((3, 1, 1, cin, cout), 72, (2.0 / (3 * cin)) ** 0.5))
    sc, bi = rnd((cout,), 73).abs() + 0.5, rnd((cout,), 74, 0.1)
    add = q(rnd((B, T, H, W, cout), 75))
    a_scale = rnd((cout,), 76).abs() + 0.5
    g = q(rnd((B, T, H, W, cout), 77))
    mask = q(rnd((B, T, H, W, cp), 78))
    return x, w, sc, bi, add, a_scale, g, mask


def _t3_run(ops, case, nf_fwd=None):
    """forward (scale, bias, residual, ReLU) and masked data-gradient through ops.conv3d; nf_fwd overrides the forward's weight tiles"""
    _, B, T, H, W, cin, cout, nf = case
    x, w, sc, bi, add, a_scale, g, mask = _t3_operands(case)
    bf = torch.bfloat16
    out = ops.conv3d(x.to(bf).cuda(), ops.ConvWeights(w.numpy(), "bf16", nf_fwd or nf), scale=sc.cuda(), bias=bi.cuda(), add=add.to(bf).cuda(), relu=True)
    nfb = 8 if w.shape[3] >= 128 else 4
    pwb = ops.ConvWeights(w.numpy(), "bf16", nf_fwd or nfb, row_scale=a_scale.numpy(), transpose=True)
    gx = ops.conv3d(g.to(bf).cuda(), pwb, pad=(1, 0, 0), out_grid=(T, H, W), mask=mask.to(bf).cuda())
    torch.cuda.synchronize()
    return out, gx


@pytest.mark.parametrize("case", T3_TILED, ids=[c[0] for c in T3_TILED])
def test_conv_temporal_dma_tiled(ops, case):
    """The ring over 16-frame temporal tiles: halo frames fetched inside the clip, zeros at the clip edges, never across clips"""
    x, w, sc, bi, add, a_scale, g, mask = _t3_operands(case)
    out, gx = _t3_run(ops, case)
    ref = torch.relu(conv_t(x, w) * sc + bi + add)
    r, a = tol(ref)
    torch.testing.assert_close(out.float().cpu(), ref, rtol=r, atol=a)
    xz = torch.zeros_like(x, requires_grad=True)
    (gx_ref,) = torch.autograd.grad(conv_t(xz, w) * a_scale, xz, g)
    gx_ref = gx_ref * (mask > 0)
    r, a = tol(gx_ref)
    torch.testing.assert_close(gx.float().cpu(), gx_ref, rtol=r * 2, atol=a * 2)
    # weights in 32-channel tiles (nf = 2) are outside the ring's route: the halo kernel, the same (slab, tap) K order -- the same bits
    out_h, gx_h = _t3_run(ops, case, nf_fwd=2)
    assert torch.equal(out_h, out)
    assert torch.equal(gx_h, gx)


_DBG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from flickering_adversarial_video_amd import ops
import test_r2plus1d_34_gpu as t
for case in t.T3_TILED:
    print("case", case[0], file=sys.stderr, flush=True)
    t._t3_run(ops, case)
"""


def test_conv_temporal_dma_tiled_takes_the_ring(ops):
    """Every T3_TILED launch (forward and data-gradient) runs conv_t3_dma_kernel: its FLK_CONV_DBG line, in a fresh process"""
    env = dict(os.environ, FLK_CONV_DBG="1")
    r = subprocess.run([sys.executable, "-c", _DBG_CHILD, ROOT, os.path.dirname(os.path.abspath(__file__))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    chunks = r.stderr.split("case ")[1:]
    assert len(chunks) == len(T3_TILED)
    for c in chunks:
        hits = [ln for ln in c.splitlines() if "whole-T tiles (16-frame temporal tiles)" in ln]
        assert len(hits) == 2, c


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU restatement of the upstream networks (NCDHW)

def _bn(x, W, p, eps):
    return F.batch_norm(x, W[p + ".running_mean"], W[p + ".running_var"], W[p + ".weight"], W[p + ".bias"], False, 0.0, eps)


def _conv2plus1d(x, W, p, s, eps):
    x = F.relu(_bn(F.conv3d(x, W[p + ".0.weight"], stride=(1, s, s), padding=(0, 1, 1)), W, p + ".1", eps))
    return F.conv3d(x, W[p + ".3.weight"], stride=(s, 1, 1), padding=(1, 0, 0))


def r_stem(x, W, eps):
    x = F.relu(_bn(F.conv3d(x, W["stem.0.weight"], stride=(1, 2, 2), padding=(0, 3, 3)), W, "stem.1", eps))
    return F.relu(_bn(F.conv3d(x, W["stem.3.weight"], padding=(1, 0, 0)), W, "stem.4", eps))


def r_block(x, W, pre, s, eps):
    h = F.relu(_bn(_conv2plus1d(x, W, pre + ".conv1.0", s, eps), W, pre + ".conv1.1", eps))
    h = _bn(_conv2plus1d(h, W, pre + ".conv2.0", 1, eps), W, pre + ".conv2.1", eps)
    sc = _bn(F.conv3d(x, W[pre + ".downsample.0.weight"], stride=s), W, pre + ".downsample.1", eps) if s != 1 else x
    return F.relu(h + sc)


def r_blocks(depth):
    return [(f"layer{li}.{bi}", 2 if li > 1 and bi == 0 else 1)
            for li, n in enumerate((3, 4, 6, 3) if depth == 34 else (2, 2, 2, 2), 1) for bi in range(n)]


def r_logits(x, W, depth, eps):
    h = r_stem(x, W, eps)
    ep = {"stem": h}
    for pre, s in r_blocks(depth):
        h = ep[pre] = r_block(h, W, pre, s, eps)
    return F.linear(h.mean(dim=(2, 3, 4)), W["fc.weight"], W["fc.bias"]), ep


def victim_weights(arch, ncls, seed=42):
    """seeded synthetic weights; the residual branches of the 34-layer net damped (its 16 blocks would otherwise grow the activations
    ~1.5x each: logits O(1e3), every softmax saturated)"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    W = vs.synthetic_weights(arch, seed, num_classes=ncls)
    if arch == "r2plus1d_34":
        for k in list(W):
            if k.endswith(".conv2.1.weight") or k.endswith(".conv2.1.bias"):
                W[k] = (W[k] * 0.3).astype(np.float32)
    return W


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


NET_CASES = [
    # base_model, arch, B, T, HW, classes
    ("r2plus1d_34_32_ig65m", "r2plus1d_34", 2, 32, 56, 359),
    ("r2plus1d_34_8_ig65m", "r2plus1d_34", 1, 8, 112, 487),      # layer4 at T = 1
]


@pytest.mark.parametrize("case", NET_CASES, ids=[f"{c[0]}_bs{c[2]}_{c[3]}x{c[4]}" for c in NET_CASES])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_r2plus1d_34_forward_backward(case, dtype):
    """Logits, endpoints and the delta-gradient of the R(2+1)D-34 plan against the restatement; backward link by link (each block's
    backward fed with the HIP path's own output gradient, evaluated on its own input endpoint)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    base, arch, B, T, HW, ncls = case
    torch.set_num_threads(16)
    f32 = dtype == "f32"
    W = victim_weights(arch, ncls)
    x_cl = torch.from_numpy(vs.synthetic_clip(B, T, HW, HW, seed=5))
    rng = np.random.default_rng(2)
    delta = torch.from_numpy(rng.uniform(-0.05, 0.05, (3, T, 1, 1)).astype(np.float32))
    Wt = {k: torch.from_numpy(v) for k, v in W.items()}
    with torch.no_grad():
        ref_logits, ref_ep = r_logits(am.torch_apply(x_cl.permute(0, 4, 1, 2, 3).contiguous(), delta, 0.2), Wt, 34, 1e-3)
    label = ref_logits.argmax(-1)
    eng = FlickerVideoResNet(base, W, batch_size=B, sample_length=T, image_size=HW, dtype=dtype, l_inf_pert_norm=0.2)
    assert eng.num_classes == ncls and eng.model_name == base
    eng.pert_model.init_perturbation(delta.numpy())
    crit = Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)
    eng.step(x_cl.cuda(), label.cuda(), crit, update=False)
    for name, ref in ref_ep.items():
        e = rel_err(torch.from_numpy(eng.net.activation(name)), ref.permute(0, 2, 3, 4, 1))
        assert e < (1e-3 if f32 else 8e-2), f"{name}: {e:.3e}"
    e = rel_err(eng._logits.cpu(), ref_logits)
    print(f"[{base} {dtype}] logits max rel err {e:.3e}")
    assert e < (1e-3 if f32 else 5e-2)
    # ---- backward, link by link: delta -> stem -> layer1.0 -> ... -> layer4.2 -> logits ----
    Wd = {k: (torch.from_numpy(v).to(torch.bfloat16).double() if (not f32 and v.ndim == 5) else torch.from_numpy(v).double()) for k, v in W.items()}
    FWD_TOL, BWD_TOL, BWD_FRAC, BWD_L2 = (1e-4, 1e-3, 3e-3, 1e-2) if f32 else (3e-2, 5e-2, 2e-2, 8e-2)
    hip_act = lambda n: torch.from_numpy(eng.net.activation(n)).permute(0, 4, 1, 2, 3).contiguous().double()
    links = [("stem", lambda x: r_stem(x, Wd, 1e-3))]
    links += [(pre, lambda x, pre=pre, s=s: r_block(x, Wd, pre, s, 1e-3)) for pre, s in r_blocks(34)]
    links.append(("logits", lambda x: F.linear(x.mean(dim=(2, 3, 4)), Wd["fc.weight"], Wd["fc.bias"])))
    d0 = delta.double().clone().requires_grad_(True)
    xa = am.torch_apply(x_cl.double().permute(0, 4, 1, 2, 3).contiguous(), d0, 0.2)
    hi16 = xa.detach().to(torch.bfloat16).double()
    prev_name, prev = "delta", (hi16 + (xa.detach() - hi16).to(torch.bfloat16).double() + (xa - xa.detach())) if not f32 else xa
    for name, fn in links:
        out = fn(prev)
        got_f, got_g = (eng._logits.cpu().double(), eng._dl.cpu().double()) if name == "logits" else (hip_act(name), hip_act("grad:" + name))
        e_f = rel_err(out.detach(), got_f)
        assert e_f < FWD_TOL, f"forward link {prev_name} -> {name}: {e_f:.3e}"
        if prev_name == "delta":
            (g_ref,) = torch.autograd.grad(out, d0, grad_outputs=got_g)
            g_hip = eng._red[:3 * T].view(T, 3).cpu().t().reshape(3, T, 1, 1).double()
            assert rel_err(g_hip, g_ref) < (1e-3 if f32 else 3e-2), f"d(adv)/d(delta) link: {rel_err(g_hip, g_ref):.3e}"
        else:
            (g_ref,) = torch.autograd.grad(out, prev, grad_outputs=got_g)
            g_ref = torch.where(prev > 0, g_ref, torch.zeros_like(g_ref))
            g_hip = hip_act("grad:" + prev_name)
            e_l2, frac = rel_l2(g_hip, g_ref), float(((g_hip - g_ref).abs() > BWD_TOL * g_ref.abs().max()).double().mean())
            assert frac <= BWD_FRAC and e_l2 < BWD_L2, f"backward link {name} -> {prev_name}: rel-L2 {e_l2:.2e}, beyond {frac:.2e}"
        prev_name = name
        if name != "logits":
            prev = hip_act(name).requires_grad_(True)
    del eng


def test_r2plus1d_34_full_size_forward():
    """One 32 x 112 x 112 clip (the IG65M 32-frame model's input) in bf16: logits against the fp32 restatement"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    torch.set_num_threads(16)
    W = victim_weights("r2plus1d_34", 359)
    x_cl = torch.from_numpy(vs.synthetic_clip(1, 32, 112, 112, seed=9))
    with torch.no_grad():
        ref, _ = r_logits(x_cl.permute(0, 4, 1, 2, 3).contiguous(), {k: torch.from_numpy(v) for k, v in W.items()}, 34, 1e-3)
    eng = FlickerVideoResNet("ig65m", W, batch_size=1, sample_length=32, image_size=112, dtype="bf16")
    assert eng.model_name == "r2plus1d_34_32_ig65m"
    got = eng.logits(x_cl.cuda(), adversarial=False).cpu()
    e = rel_err(got, ref)
    print(f"[r2plus1d_34 32x112x112 bf16] logits max rel err {e:.3e}")
    assert e < 5e-2 and torch.equal(got.argmax(-1), ref.argmax(-1))


def test_r2plus1d_18_fine_tuned_head():
    """r2plus1d_18 with a replaced 51-class fc (an HMDB51 victim, model.py:436-437): the plan takes the class count from the weights;
    a num_classes that disagrees is refused"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    W = victim_weights("r2plus1d_18", 51)
    x_cl = torch.from_numpy(vs.synthetic_clip(2, 8, 112, 112, seed=11))
    with torch.no_grad():
        ref, _ = r_logits(x_cl.permute(0, 4, 1, 2, 3).contiguous(), {k: torch.from_numpy(v) for k, v in W.items()}, 18, 1e-5)
    eng = FlickerVideoResNet("r2plus1d_18", W, batch_size=2, sample_length=8, image_size=112, dtype="f32", num_classes=51)
    got = eng.logits(x_cl.cuda(), adversarial=False).cpu()
    assert got.shape == (2, 51)
    assert rel_err(got, ref) < 1e-3
    del eng
    with pytest.raises(ValueError, match="disagrees"):
        FlickerVideoResNet("r2plus1d_18", W, batch_size=1, sample_length=8, image_size=112, dtype="f32", num_classes=400)


def test_statistics_script_ig65m(tmp_path):
    """r2plus1d_main_statistics_single_video_attack.py --base-model ig65m on two 8-frame videos: R(2+1)D-34 (r2plus1d_34_8_ig65m,
    487 classes from the weights), a few iterations"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import glob
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    torch.set_num_threads(16)
    clips = vs.synthetic_clip(2, 8, seed=6)
    W = {k: torch.from_numpy(v) for k, v in vs.synthetic_weights("r2plus1d_34", 42, num_classes=487).items()}     # the script's stand-in
    with torch.no_grad():
        lg, _ = r_logits(torch.from_numpy(clips).permute(0, 4, 1, 2, 3).contiguous(), W, 34, 1e-3)
    lab = [int(lg[0].argmax()), (int(lg[1].argmax()) + 1) % 487]              # second clip "misclassified": no attack, None result
    np.savez(tmp_path / "v.npz", clips=clips, labels=np.array(lab), names=np.array(["clipA", "clipB"]))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_statistics_single_video_attack.py"), "--videos-npz", str(tmp_path / "v.npz"),
           "--results-root", str(tmp_path / "res"), "--base-model", "ig65m", "--dtype", "f32", "--n-iter", "3", "--restart-after", "40"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clipA:" in r.stdout and "clipB: clean clip misclassified" in r.stdout
    files = sorted(glob.glob(str(tmp_path / "res" / "r2plus1d_34_8_ig65m" / "single_video_attack" / "flickering" / "*" / "*.npy")))
    assert [os.path.basename(f) for f in files] == [f"clipA_@{lab[0]}.npy", f"clipB_@{lab[1]}.npy"]     # (no --label-map: class ids)
    ra = np.load(files[0], allow_pickle=True).tolist()
    assert ra["prob_clean_input"].shape == (1, 487) and len(ra["loss/total"]) >= 3
