"""Synthetic fixtures for the parity tests -- TEST INFRASTRUCTURE, see oracle/__init__.py.

``coherent_i3d_weights``: a WELL-CONDITIONED InceptionI3d weight set for asserting the learned perturbation at the north-star
1e-3.  Why it is needed (measured, tests/test_i3d_gpu.py): on seeded He-normal (random-sign) weights two fp32 implementations of
the same forward pass disagree on ~10-30 of the ~3e7 ReLU / max-pool decisions of a 16-frame clip (units within fp32 rounding of
a tie: 4 ReLU + 23 pool flips between torch-CPU fp32 and fp64 on a smooth clip, 1 + 7 on a noise clip).  With random-sign weights
d(loss)/d(delta) is a random-sign sum over N units per layer, so ONE flipped unit moves it by ~1/sqrt(N) (1e-3 for the 4e5-unit
Mixed_4 layers): the torch-CPU fp32 oracle itself reproduces the fp64 gradient only to 2e-3...6e-3, whatever the clip (smooth or
noise), and Adam carries that into delta.  That is a property of the random-sign fixture, not of the path.

Here every convolution weight is >= 0 (|He-normal|), so all paths contribute to the gradient with the same sign and a flipped
decision moves it by ~1/N; batch-norm statistics are calibrated on the fixture clip itself (per-channel mean / variance of the
convolution output, like real BN statistics), which keeps about half of the units of every layer switched off -- the ReLU and
max-pool masks are as non-trivial as on the random fixture.  The logits layer favours one class so that the clean prediction has
a comfortable margin.  Measured: torch-CPU fp32 reproduces the fp64 delta after 6 Adam steps to 3e-6.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from . import i3d_ref

P = i3d_ref.PREFIX


def coherent_i3d_weights(xu, seed=5, label=233, num_classes=400):
    """xu: uint8 clip [1,T,224,224,3] the statistics are calibrated on.  Returns {checkpoint variable name: float32 array}."""
    rng = np.random.default_rng(seed)
    W = {}
    cout_of = {name: co for name, _, _, _, co in i3d_ref.unit_names()}
    x = (xu.double() / 128 - 1).permute(0, 4, 1, 2, 3).contiguous()

    def unit(x, name, k, s=(1, 1, 1)):
        cin, cout = x.shape[1], cout_of[name]
        w = np.abs(rng.standard_normal((*k, cin, cout))).astype(np.float32) * np.float32(np.sqrt(2.0 / (k[0] * k[1] * k[2] * cin)))
        W[P + name + "/conv_3d/w"] = w
        y = F.conv3d(i3d_ref._pad3(x, k, s, 0.0), torch.from_numpy(w).double().permute(4, 3, 0, 1, 2).contiguous(), None, stride=s)
        shp = (1, 1, 1, 1, cout)
        mean = y.mean(dim=(0, 2, 3, 4)).numpy().astype(np.float32).reshape(shp)
        var = np.maximum(y.var(dim=(0, 2, 3, 4), unbiased=False).numpy(), 1e-6).astype(np.float32).reshape(shp)
        beta = (rng.standard_normal(cout) * 0.3).astype(np.float32).reshape(shp)
        W[P + name + "/batch_norm/moving_mean"], W[P + name + "/batch_norm/moving_variance"], W[P + name + "/batch_norm/beta"] = mean, var, beta
        m, v, b = (torch.from_numpy(a).double().reshape(1, -1, 1, 1, 1) for a in (mean, var, beta))
        return F.relu((y - m) * torch.rsqrt(v + i3d_ref.BN_EPS) + b)

    x = unit(x, "Conv3d_1a_7x7", (7, 7, 7), (2, 2, 2))
    x = i3d_ref.maxpool_same(x, (1, 3, 3), (1, 2, 2))
    x = unit(x, "Conv3d_2b_1x1", (1, 1, 1))
    x = unit(x, "Conv3d_2c_3x3", (3, 3, 3))
    x = i3d_ref.maxpool_same(x, (1, 3, 3), (1, 2, 2))
    for name, spec in i3d_ref.MIXED:
        if name.startswith("MaxPool"):
            x = i3d_ref.maxpool_same(x, *spec)
            continue
        b0 = unit(x, name + "/Branch_0/Conv3d_0a_1x1", (1, 1, 1))
        b1 = unit(unit(x, name + "/Branch_1/Conv3d_0a_1x1", (1, 1, 1)), name + "/Branch_1/Conv3d_0b_3x3", (3, 3, 3))
        b2 = unit(unit(x, name + "/Branch_2/Conv3d_0a_1x1", (1, 1, 1)), name + "/Branch_2/" + i3d_ref.b2_3x3_name(name), (3, 3, 3))
        b3 = unit(i3d_ref.maxpool_same(x, (3, 3, 3), (1, 1, 1)), name + "/Branch_3/Conv3d_0b_1x1", (1, 1, 1))
        x = torch.cat([b0, b1, b2, b3], 1)
    wfc = np.abs(rng.standard_normal((x.shape[1], num_classes))).astype(np.float32) * np.float32(0.002)
    wfc[:, label] += np.float32(0.02)
    W[P + "Logits/Conv3d_0c_1x1/conv_3d/w"] = wfc.reshape(1, 1, 1, x.shape[1], num_classes)
    W[P + "Logits/Conv3d_0c_1x1/conv_3d/b"] = np.zeros(num_classes, np.float32)
    return W


def coherent_videoresnet_weights(W_base, x_ncdhw, arch, label=233, seed=5):
    """Well-conditioned VideoResNet weights (same idea as coherent_i3d_weights) from a base weight dict of the right shapes
    (torchvision state_dict names): every convolution weight becomes |w|, BatchNorm gamma = 1 with a small random beta and running
    statistics calibrated on the fixture clip (one oracle forward pass in which every BatchNorm records the mean / variance of its
    own input), fc >= 0 favouring ``label``.  x_ncdhw: the normalised clip [1,3,T,H,W] (float64)."""
    from . import videoresnet_ref as vr
    rng = np.random.default_rng(seed)
    W = {}
    for k, v in W_base.items():
        v = np.asarray(v, np.float32)
        if v.ndim == 5:
            W[k] = np.abs(v)
        elif k.endswith(".weight") and v.ndim == 1:
            W[k] = np.ones_like(v)                                   # BatchNorm gamma
        elif k.endswith(".bias") and not k.startswith("fc."):
            W[k] = (rng.standard_normal(v.shape) * 0.3).astype(np.float32)   # BatchNorm beta
        else:
            W[k] = v.copy()
    Wt = {k: torch.from_numpy(v).double() for k, v in W.items()}
    orig_bn = vr.bn

    def calibrating_bn(x, Wd, pre):
        Wd[pre + ".running_mean"] = x.mean(dim=(0, 2, 3, 4))
        Wd[pre + ".running_var"] = x.var(dim=(0, 2, 3, 4), unbiased=False).clamp_min(1e-6)
        return orig_bn(x, Wd, pre)

    vr.bn = calibrating_bn
    try:
        with torch.no_grad():
            vr.videoresnet_logits(x_ncdhw.double(), Wt, arch)
    finally:
        vr.bn = orig_bn
    for k in W:
        if k.endswith("running_mean") or k.endswith("running_var"):
            W[k] = Wt[k].numpy().astype(np.float32)
    C, F_ = W["fc.weight"].shape
    wfc = np.abs(rng.standard_normal((C, F_))).astype(np.float32) * np.float32(0.002)
    wfc[label] += np.float32(0.02)
    W["fc.weight"], W["fc.bias"] = wfc, np.zeros(C, np.float32)
    return W


def videoresnet_relu_inputs(x, W, arch, visit=None):
    """Walk a VideoResNet forward (the structure of videoresnet_ref.videoresnet_logits; x NCDHW, W a dict of tensors of x's dtype)
    and hand every ReLU's input to ``visit(name, pre_fn, bn, ds_bn)``: ``pre_fn()`` evaluates the pre-activation from W as it is NOW
    (so a visitor may change the batch norm ``bn`` -- and ``ds_bn``, the downsample's, at a block's last ReLU -- and evaluate
    again) and the visitor returns the pre-activation the walk continues from.  Without a visitor: returns [(name, pre)]."""
    from . import videoresnet_ref as vr
    seen = []

    def record(name, pre_fn, bn, ds_bn):
        seen.append((name, pre_fn()))
        return seen[-1][1]

    visit = visit or record
    if arch == "r2plus1d_18":
        y = F.relu(visit("stem.1", lambda: vr.bn(F.conv3d(x, W["stem.0.weight"], None, (1, 2, 2), (0, 3, 3)), W, "stem.1"), "stem.1", None))
        y = F.relu(visit("stem.4", lambda y=y: vr.bn(F.conv3d(y, W["stem.3.weight"], None, 1, (1, 0, 0)), W, "stem.4"), "stem.4", None))
    else:
        y = F.relu(visit("stem.1", lambda: vr.bn(F.conv3d(x, W["stem.0.weight"], None, (1, 2, 2), (1, 3, 3)), W, "stem.1"), "stem.1", None))

    def unit(inp, pre, kind, stride, bnp, shortcut=None, ds_bn=None):
        """conv_builder + the block's batch norm (+ shortcut); (2+1)D units hold a ReLU of their own in the middle"""
        if kind == "2plus1d":
            mid = F.relu(visit(pre + ".0.1", lambda: vr.bn(F.conv3d(inp, W[pre + ".0.0.weight"], None, (1, stride, stride), (0, 1, 1)), W, pre + ".0.1"),
                               pre + ".0.1", None))
            conv = lambda: F.conv3d(mid, W[pre + ".0.3.weight"], None, (stride, 1, 1), (1, 0, 0))
        else:
            conv = lambda: vr.conv_unit(inp, W, pre + ".0", kind, stride)
        if shortcut is None:
            return visit(bnp, lambda: vr.bn(conv(), W, bnp), bnp, None)
        return visit(bnp, lambda: vr.bn(conv(), W, bnp) + shortcut(), bnp, ds_bn)

    for name, kind, stride, has_ds in vr.blocks(arch):
        h1 = F.relu(unit(y, name + ".conv1", kind, stride, name + ".conv1.1"))
        if has_ds:
            shortcut = lambda y=y, name=name, kind=kind, stride=stride: vr.bn(
                F.conv3d(y, W[name + ".downsample.0.weight"], None, vr.ds_stride(kind, stride)), W, name + ".downsample.1")
        else:
            shortcut = lambda y=y: y
        y = F.relu(unit(h1, name + ".conv2", kind, 1, name + ".conv2.1", shortcut, name + ".downsample.1" if has_ds else None))
    return seen


SETTLED_MARGIN = 0.05


def settled_videoresnet_weights(arch, x_adv, seed=42):
    """VideoResNet weights on which NO ReLU can flip for the clip ``x_adv`` (the perturbed, normalised clip, NCDHW): every ReLU input
    is at least SETTLED_MARGIN of its tensor's maximum, so the network is affine around the clip and two implementations of it differ
    by rounding alone -- whole-plan tests at tiny extents, where one flipped unit would be percent of a tensor, can then bound every
    element.  From videoresnet_spec.synthetic_weights(arch, seed), walking forward in fp64; at every batch norm that feeds a ReLU, in
    order: its weight and bias are divided by max|its output| (at a block's last batch norm the downsample's by max|its output| as
    well, the ReLU's input being their sum), and where min(pre) < m * max|pre| (m = SETTLED_MARGIN) its bias is raised by
    (m * max|pre| - min(pre)) / (1 - m) * 1.01.  Returns {state_dict name: float32 array}."""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    W = {k: torch.from_numpy(np.asarray(v)).double() for k, v in vs.synthetic_weights(arch, seed).items()}
    m = SETTLED_MARGIN

    def rescale(bn, by):
        W[bn + ".weight"] = W[bn + ".weight"] / by
        W[bn + ".bias"] = W[bn + ".bias"] / by

    def settle(name, pre_fn, bn, ds_bn):
        pre = pre_fn()
        if name.endswith(".conv2.1"):    # a block's last batch norm: pre = its output + the shortcut (identity or downsample batch norm)
            keep = W[bn + ".weight"], W[bn + ".bias"]
            W[bn + ".weight"], W[bn + ".bias"] = torch.zeros_like(keep[0]), torch.zeros_like(keep[1])
            short = pre_fn()             # (with its weight and bias at zero the batch norm's output is zero)
            W[bn + ".weight"], W[bn + ".bias"] = keep
            rescale(bn, (pre - short).abs().max())
            if ds_bn is not None:
                rescale(ds_bn, short.abs().max())
        else:
            rescale(bn, pre.abs().max())
        pre = pre_fn()
        lo, top = float(pre.min()), float(pre.abs().max())
        if lo < m * top:
            W[bn + ".bias"] = W[bn + ".bias"] + (m * top - lo) / (1 - m) * 1.01
            pre = pre_fn()
        return pre

    with torch.no_grad():
        videoresnet_relu_inputs(x_adv.double(), W, arch, settle)
    return {k: v.numpy().astype(np.float32) for k, v in W.items()}


@functools.lru_cache(maxsize=2)      # (a weight set is 50-130 MB: the cases of one fixture run back to back, no more are kept)
def settled_case(arch, T, HW, B=1):
    """one odd-extent plan case: (settled weights, clip [B,T,HW,HW,3] fp32 channels-last, delta [3,T,1,1] fp32) -- the clip and delta of
    tests/test_videoresnet_gpu.py::test_videoresnet_forward_backward at the case's size, the weights settled on the perturbed clip"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from . import attack_math as am
    x_cl = torch.from_numpy(vs.synthetic_clip(B, T, HW, HW, seed=5))
    delta = torch.from_numpy(np.random.default_rng(2).uniform(-0.05, 0.05, (3, T, 1, 1)).astype(np.float32))
    delta[:, 2] = 0.25                                      # beyond dynamic_max_norm = 0.2: no gradient through the clamp
    x_adv = am.torch_apply(x_cl.double().permute(0, 4, 1, 2, 3).contiguous(), delta.double(), 0.2)
    return settled_videoresnet_weights(arch, x_adv), x_cl, delta


def videoresnet_attack_pass(W, x_cl, delta, arch, dt, bf16_conv_weights=False):
    """oracle of one attack iteration in dtype ``dt``: forward, adversarial loss (improve loss on logits, as the engine's Losses) and its
    gradient at every named endpoint and at delta; ``bf16_conv_weights``: the convolution weights rounded to bf16 first"""
    from . import attack_math as am
    from . import videoresnet_ref as vr
    Wd = {k: (torch.from_numpy(v).to(torch.bfloat16).to(dt) if (bf16_conv_weights and v.ndim == 5) else torch.from_numpy(v).to(dt)) for k, v in W.items()}
    x = x_cl.to(dt).permute(0, 4, 1, 2, 3).contiguous()
    d = delta.to(dt).clone().requires_grad_(True)
    logits, ep = vr.videoresnet_logits(am.torch_apply(x, d, 0.2), Wd, arch, return_endpoints=True)
    label = logits.argmax(-1)
    _, adv, _ = am.torch_losses(label, logits, torch.softmax(logits, 1), d.clamp(-0.2, 0.2), 0.5, 1.0, 0.05, True, True, "flickering")
    names = [n for n in ep if n != "stem.mid"]
    g, *ge = torch.autograd.grad(adv, [d] + [ep[n] for n in names])
    return dict(logits=logits.detach(), ep={k: v.detach() for k, v in ep.items()}, adv=adv.item(), label=label, g=g, ge=dict(zip(names, ge)))
