"""flk_conv3d_pc (csrc/conv_pc.hip) at the sizes the plans launch it: workgroups that run SEVERAL items in a row (halo images alternating
by slab parity, the next item's first slab staged under the current one, the weight ring and its slot carried across items, member
state kept while the member does not change, halo cell offsets cached per position tile, scale / bias areas alternating by item parity,
late-starting workgroups), the <8> instance, a tail in the last XCD's chunk and a launch of three members.  The cases and their schedule
are tests/test_conv_pc_schedule_cpu.py's PC_SCALE_CASES; each case here first asserts that the device plans that schedule.

Per case, every output element against torch-CPU fp32 on the same bf16 operands (data-gradients with the folded weights exactly as the
packer rounds them, bf16(W x scale)) within a derived bound -- one bf16 output rounding plus fp32 accumulation on both sides:
    |y - r| <= 2^-8 |r| + (1 + 2^-8) E,   E = n_K 2^-23 |s| S + 2^-22 (|b| + |add|)
with S the same operator on |x| and |w|, n_K = taps x cin, s / b the epilogue's scale and bias (1 / 0 without).  Then bitwise against
conv_igemm_kernel (flk_conv3d with FLK_CONV_PC=0, read once per process: ONE child process computes those outputs for the module from
the same seeds and packed weights); outputs poisoned before the launch (NaN in the channels it writes, a finite sentinel elsewhere:
no NaN may survive, the sentinel channels must keep their bits); and a second launch gives the same bits."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_bound import bf16_bound_ratio
from test_conv_pc_schedule_cpu import PC_SCALE_CASES, pc_schedule

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENTINEL = -1536.0          # exact in bf16
EDGE = 8                    # sentinel channels in front of and behind the members' output slices

# epilogue of each member: fwd = scale, bias, ReLU (Unit3D); fwd_add = scale, bias, + residual, ReLU (VideoResNet conv2); dgrad = transposed
# weights x BN scale, ReLU mask of the layer's input; dgrad_add = the same accumulated onto another gradient (+ add, then the mask)
EPILOGUES = {"mc3_l1_fwd_residual": ["fwd_add"], "three_members": ["fwd", "fwd_add", "dgrad_add"]}


def epilogues(case):
    name, members, dgrad = case[0], case[5], case[6]
    return EPILOGUES.get(name, ["dgrad" if dgrad else "fwd"] * len(members))


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(scale))


def bf(x):
    return x.to(torch.bfloat16).float()


def ref_conv(x, w, kt):
    """torch-CPU fp32 'same' stride-1 convolution; x [B, T, H, W, C] channels-last, w [kt, 3, 3, cin, cout]"""
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w.permute(4, 3, 0, 1, 2).contiguous(), padding=((kt - 1) // 2, 1, 1))
    return y.permute(0, 2, 3, 4, 1)


def make_case(case):
    """The case's operands on the host, from its seeds alone (the child process rebuilds the same): the bf16-rounded input, add and mask
    tensors (channels-last, fp32 values), and per member the operator's weights as the kernel multiplies them, the weights as given to
    the packer, and its epilogue."""
    idx = [c[0] for c in PC_SCALE_CASES].index(case[0])
    _, B, T, H, W, members, _, _ = case
    kinds = epilogues(case)
    seed = 1000 * (idx + 1)
    ci_tot = sum(m[0] for m in members)
    co_tot = EDGE + sum(m[1] for m in members) + EDGE
    x = bf(rnd((B, T, H, W, ci_tot), seed))
    add = bf(rnd((B, T, H, W, co_tot), seed + 1)) if any(k.endswith("_add") for k in kinds) else None
    mask = bf(rnd((B, T, H, W, co_tot), seed + 2)) if any(k.startswith("dgrad") for k in kinds) else None
    ms, in_off, out_off = [], 0, EDGE
    for i, ((cin, cout, kt), kind) in enumerate(zip(members, kinds)):
        s = seed + 10 * (i + 1)
        m = dict(cin=cin, cout=cout, kt=kt, kind=kind, in_off=in_off, out_off=out_off)
        if kind.startswith("dgrad"):
            # the data-gradient of a forward layer cout -> cin with batch-norm scale sc: G (cin channels) -> gx (cout channels).  The packer
            # flips the taps, swaps the channel axes and rounds W x sc to bf16 in one step (api.cpp): so does the operator here
            w_fwd = bf(rnd((kt, 3, 3, cout, cin), s, (2.0 / (9 * kt * cout)) ** 0.5))
            sc = rnd((cin,), s + 1).abs() + 0.5
            m.update(pack=dict(w=w_fwd, transpose=True, row_scale=sc),
                     w=bf(w_fwd.flip(0, 1, 2).permute(0, 1, 2, 4, 3) * sc.view(1, 1, 1, cin, 1)), scale=None, bias=None)
        else:
            w = bf(rnd((kt, 3, 3, cin, cout), s, (2.0 / (9 * kt * cin)) ** 0.5))
            m.update(pack=dict(w=w, transpose=False, row_scale=None), w=w, scale=rnd((cout,), s + 1).abs() + 0.5, bias=rnd((cout,), s + 2, 0.1))
        ms.append(m)
        in_off += cin
        out_off += cout
    return dict(x=x, add=add, mask=mask, members=ms, co_tot=co_tot)


def pack(ops, m):
    p = m["pack"]
    rs = None if p["row_scale"] is None else p["row_scale"].numpy()
    return ops.ConvWeights(p["w"].numpy(), torch.bfloat16, 4, row_scale=rs, transpose=p["transpose"])


def poisoned(h):
    """the output buffer: NaN in every channel a member writes, the sentinel in the others"""
    x = h["x"]
    out = torch.full((*x.shape[:4], h["co_tot"]), SENTINEL, dtype=torch.bfloat16, device="cuda")
    for m in h["members"]:
        out[..., m["out_off"]:m["out_off"] + m["cout"]] = float("nan")
    return out


def launch_members(ops, h, dev, weights, out):
    """(x, weights, conv3d keywords) of every member, writing into `out`"""
    xg, addg, maskg = dev
    mem = []
    for m, pw in zip(h["members"], weights):
        kw = dict(in_coff=m["in_off"], cin=m["cin"], out=out, out_coff=m["out_off"])
        if m["kind"].startswith("fwd"):
            kw.update(scale=m["scale"].cuda(), bias=m["bias"].cuda(), relu=True)
        else:
            kw.update(mask=maskg, mask_coff=m["out_off"])
        if m["kind"].endswith("_add"):
            kw.update(add=addg, add_coff=m["out_off"])
        mem.append((xg, pw, kw))
    return mem


def to_device(h):
    return tuple(None if t is None else t.to(torch.bfloat16).cuda() for t in (h["x"], h["add"], h["mask"]))


def igemm_child(outdir):
    """Run in a fresh process with FLK_CONV_PC=0: every case's members through flk_conv3d -- conv_igemm_kernel -- into a poisoned buffer,
    saved as outdir/<case>.pt"""
    assert os.environ.get("FLK_CONV_PC") == "0"
    from flickering_adversarial_video_amd import ops
    for case in PC_SCALE_CASES:
        h = make_case(case)
        weights = [pack(ops, m) for m in h["members"]]
        out = poisoned(h)
        for xg, pw, kw in launch_members(ops, h, to_device(h), weights, out):
            ops.conv3d(xg, pw, **kw)
        torch.cuda.synchronize()
        torch.save(out.cpu(), os.path.join(outdir, case[0] + ".pt"))
        print(f"conv_igemm outputs of {case[0]} saved", flush=True)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    torch.set_num_threads(16)
    return o


@pytest.fixture(scope="module")
def igemm_outputs(ops, tmp_path_factory):
    """conv_igemm_kernel's outputs of every case, computed once by one child process.  The child runs with FLK_CONV_DBG, under which
    every conv_igemm_kernel launch prints its layout ('conv kt x 3 x 3 ...') and every persistent launch 'pc launch ...': its log must show
    one conv_igemm_kernel launch per member and no persistent one -- the bitwise comparison is between two kernels, not one with itself"""
    d = tmp_path_factory.mktemp("conv_igemm")
    env = dict(os.environ, FLK_CONV_PC="0", FLK_CONV_DBG="1")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_conv_pc_scale_gpu as t; t.igemm_child({str(d)!r})"
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"conv_igemm child failed ({r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = r.stderr.splitlines()
    assert not [ln for ln in lines if ln.startswith("pc ")], "the child ran the persistent kernel"
    launches = [ln for ln in lines if re.match(r"conv [13]x3x3 s111 ", ln)]
    assert len(launches) == sum(len(c[5]) for c in PC_SCALE_CASES), launches
    print(f"\n[pc scale] conv_igemm child: {time.time() - t0:.1f} s")
    return d


def bound_ratio(y, x, w, kt, *, scale=None, bias=None, add=None, mask=None, relu=False, bias_err=None):
    """worst |y - r| / bound of a convolution's output (y fp32 [B, T, H, W, cout]) against the fp32 oracle of x [.., cin] and the
    operator's weights w [kt, 3, 3, cin, cout]; the epilogue in the kernel's order: scale, bias, + add, ReLU, mask (> 0).  Asserts the
    bound on every element (conv_bound.bf16_bound_ratio).  bias_err: a bound on how far the bias the kernel used may be from `bias` (added to E)."""
    r = ref_conv(x, w, kt)
    S = ref_conv(x.abs(), w.abs(), kt)
    if scale is not None:
        r = r * scale + bias
    if add is not None:
        r = r + add
    if relu:
        r = torch.relu(r)
    if mask is not None:
        r = torch.where(mask > 0, r, torch.zeros(()))
    return bf16_bound_ratio(y, r, S, 9 * kt * x.shape[-1], scale=scale, bias=bias, add=add, bias_err=bias_err)


def member_bound_ratio(y, h, m):
    """bound_ratio of one member of a case (y: its output slice)"""
    sl = slice(m["out_off"], m["out_off"] + m["cout"])
    kind = m["kind"]
    return bound_ratio(y, h["x"][..., m["in_off"]:m["in_off"] + m["cin"]], m["w"], m["kt"], scale=m["scale"], bias=m["bias"],
                       add=h["add"][..., sl] if kind.endswith("_add") else None,
                       mask=h["mask"][..., sl] if kind.startswith("dgrad") else None, relu=kind.startswith("fwd"))


@pytest.mark.parametrize("case", PC_SCALE_CASES, ids=[c[0] for c in PC_SCALE_CASES])
def test_conv_pc_at_launch_size(ops, igemm_outputs, case):
    import ctypes as C
    from flickering_adversarial_video_amd._lib import FLK_BF16, load
    name, B, T, H, W, members, _, want = case
    t0 = time.time()
    # 1. the case is what it claims: routed to the persistent kernel, with the schedule of the table on this device
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = pc_schedule(B, T, H, W, members, cus)
    assert s["rc"] == 1 and s["members"][0]["tile"] == want["tile"] and s["ni"] == want["ni"], (cus, s)
    assert (s["per_xcd"], s["busiest"]) == (want["per_xcd"], want["busiest"]), (cus, s)
    h = make_case(case)
    weights = [pack(ops, m) for m in h["members"]]
    dev = to_device(h)
    out = poisoned(h)
    mem = launch_members(ops, h, dev, weights, out)
    built = [ops.conv3d_args(xg, pw, **kw)[0] for xg, pw, kw in mem]
    ap = (C.POINTER(ops.ConvArgs) * len(built))(*[C.pointer(a) for a in built])
    wp = (C.c_void_p * len(built))(*[pw.handle for _, pw, _ in mem])
    assert load().flk_conv3d_pc_worthwhile(ap, wp, len(built), FLK_BF16) == 1      # flk_conv3d (one member) / flk_conv3d_group (two) route here
    # 2. the launch, a second one into another poisoned buffer
    ops.conv3d_pc(mem)
    again = poisoned(h)
    ops.conv3d_pc(launch_members(ops, h, dev, weights, again))
    torch.cuda.synchronize()
    y = out.cpu()
    assert torch.equal(again.cpu().view(torch.int16), y.view(torch.int16)), "a second launch gave other bits"
    del again, dev
    # 3. poison: every written element was written, the channels no member owns kept their bits
    owned = torch.zeros(h["co_tot"], dtype=torch.bool)
    for m in h["members"]:
        owned[m["out_off"]:m["out_off"] + m["cout"]] = True
    assert not bool(torch.isnan(y[..., owned]).any()), "an output element was never stored"
    sentinel = torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16)
    assert bool((y[..., ~owned].view(torch.int16) == sentinel).all()), "a store reached a channel outside the members' slices"
    # 4. bitwise conv_igemm_kernel (flk_conv3d, FLK_CONV_PC=0, same packed weights)
    path = os.path.join(igemm_outputs, name + ".pt")
    ref_bits = torch.load(path)
    os.remove(path)             # (up to 235 MB a case: not left behind in pytest's temporary directories)
    assert torch.equal(ref_bits.view(torch.int16), y.view(torch.int16)), "not bitwise the conv_igemm_kernel outputs"
    del ref_bits
    # 5. every element against the fp32 oracle within the derived bound
    yf = y.float()
    for i, m in enumerate(h["members"]):
        worst, b = member_bound_ratio(yf[..., m["out_off"]:m["out_off"] + m["cout"]], h, m)
        print(f"[pc scale] {name} member {i} ({m['cin']} -> {m['cout']}, {m['kt']}x3x3, {m['kind']}): worst |y - r| / bound {worst:.3f} (clip {b})")
    print(f"[pc scale] {name}: {s['per_xcd']} items per XCD on {s['slots']} workgroups, busiest {s['busiest']} items, NI {s['ni']}; "
          f"{time.time() - t0:.1f} s")


def test_i3d_bs8_conv_pc_layers_on_plan_buffers(ops):
    """The layers the I3D bf16 plan sends to the persistent kernel at the headline batch (bs 8, 64 x 224 x 224), checked on the plan's
    own buffers after one step(update=False), each within the bound of the kernel-level cases above.  What net.cpp feeds them:
      * Conv3d_2c_3x3 forward (emit_conv_fwd, per half batch): Conv3d_2c_3x3 = relu(conv(Conv3d_2b_1x1, bf16(W)) x s + b);
      * its data-gradient (emit_conv_bwd): grad:Conv3d_2b_1x1 = [Conv3d_2b_1x1 > 0] x conv(grad:Conv3d_2c_3x3, bf16(flip(W^T) x s)) -- the
        mask is the ReLU OUTPUT of Conv3d_2b (> 0 exactly where its ReLU passed), the incoming gradient the buffer as the pool backward
        left it; weights folded and rounded once, as the packer does (pack: row_scale = the layer's BN scale);
      * Mixed_3b / 3c Branch_1 + Branch_2 forward (one group launch): mid:<block> = [Branch_1/Conv3d_0a | Branch_2/Conv3d_0a] (the fused
        1x1x1's ReLU outputs) -> <block>[c0 : c0 + c1b] and [c0 + c1b : c0 + c1b + c2b];
      * their data-gradient (one group launch): grad:<block> at those slices -> gradmid:<block>, masked by mid:<block> > 0.
    s = 1 / sqrt(var + 1e-3) and b = beta - mean s are computed in fp32 on the host by make_unit3d.  s is reproduced exactly here (a
    correctly rounded sqrt and division, as sqrtf and the host's division); b may differ, since the host compiler may fuse mean s into the subtraction (one
    rounding instead of two): E carries 2^-23 (|mean s| + |b|) for it."""
    from flickering_adversarial_video_amd import i3d_spec
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    B, T = 8, 64
    Wts = i3d_spec.synthetic_i3d_weights(42)
    xu = torch.from_numpy(i3d_spec.synthetic_clip_u8(B, T, seed=1234))
    eng = FlickerI3D(Wts, batch_size=B, frames=T, dtype="bf16")
    labels = eng.logits(xu.cuda(), adv_flag=0.0).argmax(-1).clone()
    eng.step(xu.cuda(), labels, update=False)
    torch.cuda.synchronize()
    act = lambda n: torch.from_numpy(eng.net.activation(n))            # [B, T, H, W, C], the bf16 values in fp32

    def unit(name):
        pre = "RGB/inception_i3d/" + name
        w = torch.from_numpy(Wts[pre + "/conv_3d/w"])
        beta, mean, var = (torch.from_numpy(Wts[pre + "/batch_norm/" + k]).reshape(-1) for k in ("beta", "moving_mean", "moving_variance"))
        # 1.0f / sqrtf(var + 1e-3f), each step correctly rounded to fp32 (through float64: exact for sqrt and division; torch's CPU sqrt
        # is not correctly rounded)
        q = np.sqrt((var + 1e-3).double().numpy()).astype(np.float32)
        s = torch.from_numpy((1.0 / q.astype(np.float64)).astype(np.float32))
        b = beta - mean * s
        return w, s, b, 2.0 ** -23 * ((mean.double() * s.double()).abs() + b.double().abs())

    def fwd(name, y, x):
        w, s, b, berr = unit(name)
        return bound_ratio(y, x, bf(w), 3, scale=s, bias=b, relu=True, bias_err=berr)

    def dgrad(name, y, g, mask):
        w, s, _, _ = unit(name)
        return bound_ratio(y, g, bf(w.flip(0, 1, 2).permute(0, 1, 2, 4, 3) * s.view(1, 1, 1, -1, 1)), 3, mask=mask)

    report = []
    a2b = act("Conv3d_2b_1x1")
    report.append(("Conv3d_2c_3x3 forward", fwd("Conv3d_2c_3x3", act("Conv3d_2c_3x3"), a2b)))
    report.append(("Conv3d_2c_3x3 data-gradient", dgrad("Conv3d_2c_3x3", act("grad:Conv3d_2b_1x1"), act("grad:Conv3d_2c_3x3"), a2b)))
    del a2b
    for bn, (c0, c1a, c1b, c2a, c2b) in (("Mixed_3b", (64, 96, 128, 16, 32)), ("Mixed_3c", (128, 128, 192, 32, 96))):
        mid, out, gout, gmid = act("mid:" + bn), act(bn), act("grad:" + bn), act("gradmid:" + bn)
        assert mid.shape[-1] == c1a + c2a and gmid.shape[-1] == c1a + c2a and out.shape[-1] >= c0 + c1b + c2b
        for br, sl_in, sl_out in (("Branch_1", slice(0, c1a), slice(c0, c0 + c1b)), ("Branch_2", slice(c1a, c1a + c2a), slice(c0 + c1b, c0 + c1b + c2b))):
            name = f"{bn}/{br}/Conv3d_0b_3x3"
            report.append((name + " forward", fwd(name, out[..., sl_out], mid[..., sl_in])))
            report.append((name + " data-gradient", dgrad(name, gmid[..., sl_in], gout[..., sl_out], mid[..., sl_in])))
        del mid, out, gout, gmid
    for what, (worst, clip) in report:
        print(f"[pc plan bs 8] {what:<45s} worst |y - r| / bound {worst:.3f} (clip {clip})")
