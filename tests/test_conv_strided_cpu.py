"""The data-gradient of the strided VideoResNet convolutions as parity classes (oracle/strided_dgrad.py), and the settled fixture of
the odd-extent plan tests (oracle/fixtures.py::settled_videoresnet_weights) -- both shown to be what they claim on the CPU, in fp64,
before tests/test_conv_strided_gpu.py drives the HIP kernels with them.

flk_conv3d's contract is emulated here in torch: a stride-1 convolution with pad-before, zeros outside the input, a logical output
grid, and a scatter of that grid to the cells o * out_stride + out_offset of the output buffer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import attack_math as am
from oracle import fixtures, strided_dgrad
from oracle import videoresnet_ref as vr

# name -> kernel, stride, torch's symmetric padding: every strided convolution of the r3d_18 / mc3_18 / r2plus1d_18 / 34 plans
GEOMETRIES = {
    "a_3x3x3_s2": ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
    "b_1x3x3_s122": ((1, 3, 3), (1, 2, 2), (0, 1, 1)),
    "c_3x1x1_s211": ((3, 1, 1), (2, 1, 1), (1, 0, 0)),
    "d_1x1x1_s2": ((1, 1, 1), (2, 2, 2), (0, 0, 0)),
    "e_1x1x1_s122": ((1, 1, 1), (1, 2, 2), (0, 0, 0)),
}
CLASS_COUNTS = {"a_3x3x3_s2": 8, "b_1x3x3_s122": 4, "c_3x1x1_s211": 2, "d_1x1x1_s2": 1, "e_1x1x1_s122": 1}
EXTENTS = [(5, 9, 7), (4, 8, 6), (1, 5, 3), (2, 3, 2)]


def conv_contract(g, wd, pad, grid):
    """flk_conv3d on the CPU: g [B,C,T,H,W], wd DHWIO; stride 1, pad-before ``pad``, zeros wherever a tap falls outside g, the
    logical output grid ``grid`` -> [B,C',*grid]"""
    k = wd.shape[:3]
    pads = []
    for i in (2, 1, 0):
        after = grid[i] - 1 + k[i] - pad[i] - g.shape[2 + i]
        pads += [pad[i], max(after, 0)]
    y = F.conv3d(F.pad(g, pads), wd.permute(4, 3, 0, 1, 2).contiguous())
    return y[:, :, :grid[0], :grid[1], :grid[2]]


def scatter_classes(gx, cls, val, s):
    """write a class's logical grid to its cells o * s + offset of gx [B,C,T,H,W]"""
    o = cls["offset"]
    gx[:, :, o[0]::s[0], o[1]::s[1], o[2]::s[2]] = val


@pytest.mark.parametrize("dims", EXTENTS, ids=["x".join(map(str, d)) for d in EXTENTS])
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_class_union_is_the_data_gradient(geo, dims):
    """the union of the class operators == torch autograd of the strided convolution, to 1e-12 in fp64"""
    k, s, pad = GEOMETRIES[geo]
    rng = np.random.default_rng(3)
    B, cin, cout = 2, 5, 7
    w = torch.from_numpy(rng.standard_normal((*k, cin, cout)))                     # DHWIO, fp64
    x = torch.zeros((B, cin, *dims), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, w.permute(4, 3, 0, 1, 2).contiguous(), None, s, pad)
    assert tuple(y.shape[2:]) == strided_dgrad.out_dims(k, s, pad, dims)
    g = torch.from_numpy(rng.standard_normal(tuple(y.shape)))
    (ref,) = torch.autograd.grad(y, x, g)
    # every class of the stride box, empty grids included, is counted by the all-axes-long extent
    full = strided_dgrad.classes(k, s, pad, tuple(2 * ss for ss in s))
    assert len(full) == CLASS_COUNTS[geo]
    cls = strided_dgrad.classes(k, s, pad, dims, w.numpy())
    empty_grids = sum(1 for c in full if any(c["offset"][i] >= dims[i] for i in range(3)))
    assert len(cls) == CLASS_COUNTS[geo] - empty_grids
    got = torch.zeros_like(ref)
    owned = torch.zeros(dims, dtype=torch.int64)
    for c in cls:
        assert min(c["pad"]) >= 0
        assert c["w"].shape == (*(len(t) for t in c["taps"]), cout, cin) and max(c["w"].shape[:3]) <= 2
        assert c["grid"] == tuple(len(range(c["offset"][i], dims[i], s[i])) for i in range(3))
        scatter_classes(got, c, conv_contract(g, torch.from_numpy(c["w"]), c["pad"], c["grid"]), s)
        o = c["offset"]
        owned[o[0]::s[0], o[1]::s[1], o[2]::s[2]] += 1
    assert int(owned.max()) == 1                                                   # the classes' cells are disjoint
    assert bool((ref[:, :, owned == 0] == 0).all())                                # cells no class owns get no gradient from the layer
    if geo[0] in "abc":
        assert int(owned.min()) == 1
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err < 1e-12, err


# ---- the settled fixture of the odd-extent plan tests ----
# (T, HW, B): the cases of tests/test_conv_strided_gpu.py::test_videoresnet_odd_extents, with their batch sizes -- the fixture is
# settled on the whole batch
PLAN_CASES = [(5, 36, 1), (3, 20, 2)]
PLAN_ARCHS = ["r3d_18", "mc3_18", "r2plus1d_18"]


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.mark.parametrize("size", PLAN_CASES, ids=[f"T{t}_HW{hw}_B{b}" for t, hw, b in PLAN_CASES])
@pytest.mark.parametrize("arch", PLAN_ARCHS)
def test_settled_fixture_cannot_flip(arch, size):
    """after rounding the weights to fp32 every ReLU input keeps a margin of 0.04 of its tensor's maximum, and the two torch oracles
    (fp32, fp64) agree on every gradient to 1e-5 (measured 1.1e-6): nothing between them for a test to absorb.  The walk the
    fixture is settled on is the network the oracle runs: its last activation is the oracle's last endpoint, bit for bit."""
    T, HW, B = size
    W, x_cl, delta = fixtures.settled_case(arch, T, HW, B)
    Wd = {k: torch.from_numpy(v).double() for k, v in W.items()}
    x_adv = am.torch_apply(x_cl.double().permute(0, 4, 1, 2, 3).contiguous(), delta.double(), 0.2)
    with torch.no_grad():
        sites = fixtures.videoresnet_relu_inputs(x_adv, Wd, arch)
        _, ep = vr.videoresnet_logits(x_adv, Wd, arch, return_endpoints=True)
    assert len(sites) == {"r3d_18": 17, "mc3_18": 17, "r2plus1d_18": 34}[arch]
    assert torch.equal(torch.relu(sites[-1][1]), ep["layer4.1"])
    for name, pre in sites:
        margin = float(pre.min() / pre.abs().max())
        assert margin >= 0.04, (name, margin)
    r32, r64 = (fixtures.videoresnet_attack_pass(W, x_cl, delta, arch, dt) for dt in (torch.float32, torch.float64))
    assert torch.equal(r32["label"], r64["label"]) and r64["adv"] > 0
    worst = max([rel_err(r32["g"], r64["g"])] + [rel_err(r32["ge"][n], r64["ge"][n]) for n in r64["ge"]])
    print(f"[{arch} T{T} HW{HW} B{B}] fp32 vs fp64 oracle: gradients {worst:.2e}, logits {rel_err(r32['logits'], r64['logits']):.2e}, adv {r64['adv']:.3f}")
    assert worst < 1e-5
    assert float(r64["g"][:, 2].abs().max()) == 0
