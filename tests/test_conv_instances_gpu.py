"""Every compiled convolution kernel instance, run once per case of tests/conv_instance_cases.py against a float64 oracle.

tests/test_conv_instances_cpu.py proves (without a GPU) which instantiation each case runs and that every instantiation of the library has
a case; here the cases are launched through flk_conv3d_layout -- the launch the autotuner times for a candidate layout {wn, da} and a
tuned entry replays -- so a layout that is wrong only at, say, two waves along the channels is compared with something whether or not it
ever wins a timing.

Per (geometry, dtype, epilogue) the oracle is computed once: torch-CPU float64 on the same rounded operands (data-gradient forms with the
folded weights rounded as the packer rounds them, dtype(W x scale)).  Epilogues: full = scale, bias, + add, ReLU, mask; bare = none;
dgrad = transposed pack with row_scale, plus the mask.  Then, for every packing nf and every candidate layout:
  * the output buffer is poisoned (NaN in the channels the launch writes, a finite sentinel in the EDGE channels on both sides): no NaN
    survives, the sentinels keep their bits;
  * every element is within the bound -- bf16: conv_bound.bf16_bound_ratio (|y - r| <= 2^-8 |r| + (1 + 2^-8) E); fp32: test_kernels_gpu.tol
    (1e-4 relative + 1e-5 of the maximum);
  * a second launch gives the same bits;
  * LAYOUT INVARIANCE, the autotuner's contract: every candidate gives the bits of the heuristic's launch at the same packing, in both
    dtypes.  Across packings equality is asserted where the suite already claims it (bf16 3x3x3: test_conv_ring_weights_a_row_ahead) and
    printed elsewhere.
The LDS-DMA routes (whole-T ring, its tiled form, the 1x1x1 ring) must be bitwise the forced halo-kernel launch; split-K, at every
candidate layout, within the bound of the oracle and of the one-slice launch and bitwise the heuristic's split launch; every member of a grouped launch bitwise its own forced-layout single launch."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_instance_cases as cc
from conv_bound import bf16_bound_ratio
from test_kernels_gpu import fold_stem, tol

pytestmark = pytest.mark.gpu

SENTINEL = -1536.0          # exact in bf16
EDGE = cc.EDGE
TD = {"bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    torch.set_num_threads(16)
    return o


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(scale))


def ref_conv64(x, w, stride, pad, og):
    """float64 convolution with explicit pad-before (zero padding behind as far as the output grid needs); x [B, T, H, W, cin],
    w [kt, kh, kw, cin, cout] -> [B, *og, cout]"""
    xc = x.double().permute(0, 4, 1, 2, 3)
    k = w.shape[:3]
    pads = []
    for i in (2, 1, 0):
        after = (og[i] - 1) * stride[i] + k[i] - pad[i] - xc.shape[2 + i]
        pads += [pad[i], max(after, 0)]
    y = F.conv3d(F.pad(xc, pads), w.double().permute(4, 3, 0, 1, 2).contiguous(), stride=stride)
    return y.permute(0, 2, 3, 4, 1)[:, :og[0], :og[1], :og[2]].contiguous()


def wide(t, ld, off, seed):
    """t [..., c] at channel offset off of a buffer [..., ld] whose other channels hold large finite values (a read outside the slice shows)"""
    buf = rnd((*t.shape[:-1], ld), seed, 64.0).to(t.dtype)
    buf[..., off:off + t.shape[-1]] = t
    return buf


def make_problem(geo, dtype, epi, cout, seed, pad=None):
    """host operands (rounded to dtype, as fp32 values), what the packer gets, and the float64 reference r with S = the operator on |x|, |w|"""
    B, T, H, W, cin, k, s = geo
    td = TD[dtype]
    q = lambda t: t.to(td).float()
    og, spad = zip(*(cc.same_pad(n, kk, ss) for n, kk, ss in zip((T, H, W), k, s)))
    pad = spad if pad is None else pad
    taps = k[0] * k[1] * k[2]
    x = q(rnd((B, T, H, W, cin), seed))
    p = dict(geo=geo, dtype=dtype, epi=epi, cout=cout, x=x, og=og, pad=pad, scale=None, bias=None, add=None, mask=None, relu=False, nK=taps * cin)
    oshape = (B, *og, cout)
    if epi == "dgrad":
        # the data-gradient of a forward layer cout -> cin with scale sc: the packer flips the taps, swaps the channel axes and rounds
        # W x sc to the storage type in one step (api.cpp); so does the operator here
        w_fwd = q(rnd((*k, cout, cin), seed + 1, (2.0 / (taps * cout)) ** 0.5))
        sc = rnd((cin,), seed + 2).abs() + 0.5
        p.update(pack=dict(w=w_fwd, transpose=True, row_scale=sc), w=q(w_fwd.flip(0, 1, 2).permute(0, 1, 2, 4, 3) * sc.view(1, 1, 1, cin, 1)),
                 mask=q(rnd(oshape, seed + 6)))
    else:
        w = q(rnd((*k, cin, cout), seed + 1, (2.0 / (taps * cin)) ** 0.5))
        p.update(pack=dict(w=w, transpose=False, row_scale=None), w=w)
        if epi == "full":
            p.update(scale=rnd((cout,), seed + 3).abs() + 0.5, bias=rnd((cout,), seed + 4, 0.1), add=q(rnd(oshape, seed + 5)),
                     mask=q(rnd(oshape, seed + 6)), relu=True)
    r = ref_conv64(x, p["w"], s, pad, og)
    p["S"] = ref_conv64(x.abs(), p["w"].abs(), s, pad, og)
    if p["scale"] is not None:
        r = r * p["scale"].double() + p["bias"].double()
    if p["add"] is not None:
        r = r + p["add"].double()
    if p["relu"]:
        r = torch.relu(r)
    if p["mask"] is not None:
        r = torch.where(p["mask"] > 0, r, torch.zeros((), dtype=torch.float64))
    p["r"] = r
    return p


def pack(ops, p, nf):
    pk = p["pack"]
    rs = None if pk["row_scale"] is None else pk["row_scale"].numpy()
    return ops.ConvWeights(pk["w"].numpy(), TD[p["dtype"]], nf, row_scale=rs, transpose=pk["transpose"])


def device_operands(p, in_ld=None, in_off=EDGE, xbuf=None):
    """the launch's keywords except `out`: the input slice inside a wider buffer, add / mask at channel offset EDGE of wider buffers"""
    td = TD[p["dtype"]]
    cin = p["geo"][4]
    if xbuf is None:
        xbuf = wide(p["x"], cin + 2 * EDGE if in_ld is None else in_ld, in_off, 901).to(td).cuda()
    kw = dict(in_coff=in_off, cin=cin, stride=p["geo"][6], pad=p["pad"], out_grid=p["og"], relu=p["relu"])
    if p["scale"] is not None:
        kw.update(scale=p["scale"].cuda(), bias=p["bias"].cuda())
    if p["add"] is not None:
        kw.update(add=wide(p["add"], p["cout"] + 2 * EDGE, EDGE, 902).to(td).cuda(), add_coff=EDGE)
    if p["mask"] is not None:
        kw.update(mask=wide(p["mask"], p["cout"] + 2 * EDGE, EDGE, 903).to(td).cuda(), mask_coff=EDGE)
    return xbuf, kw


def poisoned(p, ld=None, owned=None):
    """the output buffer: NaN in the channels the launch writes ([EDGE, EDGE + cout) unless `owned` lists slices), the sentinel elsewhere"""
    ld = p["cout"] + 2 * EDGE if ld is None else ld
    out = torch.full((p["geo"][0], *p["og"], ld), SENTINEL, dtype=TD[p["dtype"]], device="cuda")
    for a, b in ([(EDGE, EDGE + p["cout"])] if owned is None else owned):
        out[..., a:b] = float("nan")
    return out


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_output(y, p, off=EDGE, others_owned=()):
    """y: the whole output buffer on the host.  Poison, then every element of the slice [off, off + cout) against the reference.  Returns
    (list of failures, worst |y - r| / bound)"""
    fails = []
    cout = p["cout"]
    owned = torch.zeros(y.shape[-1], dtype=torch.bool)
    for a, b in [(off, off + cout), *others_owned]:
        owned[a:b] = True
    ys = y[..., off:off + cout].float()
    if bool(torch.isnan(ys).any()):
        fails.append(f"{int(torch.isnan(ys).sum())} output elements never stored")
    sentinel = bits(torch.tensor(SENTINEL, dtype=y.dtype))
    if not bool((bits(y[..., ~owned].contiguous()) == sentinel).all()):
        fails.append("a store reached a channel outside the output slice")
    worst = float("nan")
    if p["dtype"] == "bf16":
        try:
            worst, _ = bf16_bound_ratio(ys, p["r"], p["S"], p["nK"], scale=p["scale"], bias=p["bias"], add=p["add"])
        except AssertionError as e:
            fails.append(str(e))
    else:
        rt, at = tol(torch.float32, p["r"])
        bound = rt * p["r"].abs() + at
        err = (ys.double() - p["r"]).abs()
        bad = ~(err <= bound)
        worst = float((err / bound).max())
        if bool(bad.any()):
            i = tuple(int(v) for v in bad.nonzero()[0])
            fails.append(f"{int(bad.sum())} elements outside the fp32 tolerance, the first at {i}: y {float(ys[i])}, r {float(p['r'][i])}")
    return fails, worst


def run_layouts(ops, p, nf, xbuf, kw, pw=None, splitk=False):
    """every candidate layout of the packing, twice each: {layout: output buffer on the host}, failures"""
    pw = pack(ops, p, nf) if pw is None else pw
    outs, fails, worst = {}, [], {}
    for lay in ops.conv_layout_candidates(nf, p["dtype"], stem4=bool(p.get("stem4"))):
        out, again = poisoned(p), poisoned(p)
        ops.conv3d_layout(xbuf, pw, lay[0], lay[1], out=out, out_coff=EDGE, splitk=splitk, **kw)
        ops.conv3d_layout(xbuf, pw, lay[0], lay[1], out=again, out_coff=EDGE, splitk=splitk, **kw)
        torch.cuda.synchronize()
        y = out.cpu()
        if not torch.equal(bits(again.cpu()), bits(y)):
            fails.append(f"nf {nf} layout {lay}: a second launch gave other bits")
        f, worst[lay] = check_output(y, p)
        fails += [f"nf {nf} layout {lay}: {m}" for m in f]
        outs[lay] = y
    return outs, fails, worst, pw


HALO_PROBLEMS = [(g, dt, epi) for g in cc.GEOMETRIES for dt in cc.NFS for epi in cc.EPILOGUES]


@pytest.mark.parametrize("g,dtype,epi", HALO_PROBLEMS, ids=["-".join(c) for c in HALO_PROBLEMS])
def test_conv_igemm_instances(ops, g, dtype, epi):
    """the conv_igemm_kernel cases of one (geometry, dtype, epilogue): all packings, all candidate layouts"""
    geo = cc.GEOMETRIES[g]
    p = make_problem(geo, dtype, epi, cc.COUT, 100 * (1 + list(cc.GEOMETRIES).index(g)))
    xbuf, kw = device_operands(p)
    fails, by_nf = [], {}
    for nf in cc.NFS[dtype]:
        # the case is the one the CPU test reasons about: same geometry, same strides and offsets, and it plans as pinned
        pw = pack(ops, p, nf)
        a, _ = ops.conv3d_args(xbuf, pw, out=poisoned(p), out_coff=EDGE, **kw)
        ga = cc.geometry_args(geo)
        for f in ("B", "Ti", "Hi", "Wi", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw", "To", "Ho", "Wo", "OT", "OH", "OW", "cin", "cout",
                  "in_ld", "in_coff", "out_ld", "out_coff"):
            assert getattr(a, f) == getattr(ga, f), (f, getattr(a, f), getattr(ga, f))
        for lay, want in cc.HALO_EXPECT[(g, dtype, nf)].items():
            pl = ops.conv_plan_query(a, nf, dtype, wn=lay[0], da=lay[1])
            assert (pl["route"], pl["wn"], pl["template_mode"]) == ("halo", *want), (nf, lay, pl)
        outs, f, worst, _ = run_layouts(ops, p, nf, xbuf, kw, pw=pw)
        fails += f
        by_nf[nf] = outs
        heur = outs[(0, -1)]
        for lay, y in outs.items():
            if not torch.equal(bits(y), bits(heur)):
                n = int((bits(y) != bits(heur)).sum())
                fails.append(f"nf {nf}: layout {lay} differs from the heuristic's launch in {n} elements (the autotuner's contract: speed only)")
        print(f"[instances] {g} {dtype} {epi} nf {nf}: worst |y - r| / bound " + ", ".join(f"{lay} {w:.3f}" for lay, w in worst.items()))
    # across packings: claimed for the bf16 3x3x3 ring kernels at nf 4 / 6 / 8 (test_conv_ring_weights_a_row_ahead); printed elsewhere
    nfs = list(by_nf)
    for nf in nfs[1:]:
        same = torch.equal(bits(by_nf[nf][(1, 0)]), bits(by_nf[nfs[0]][(1, 0)]))
        print(f"[instances] {g} {dtype} {epi}: ring launch at nf {nf} bitwise the one at nf {nfs[0]}: {same}")
    if g == "k333" and dtype == "bf16":
        for nf in (6, 8):
            if not torch.equal(bits(by_nf[nf][(1, 0)]), bits(by_nf[4][(1, 0)])):
                fails.append(f"the row-ahead ring at nf {nf} differs from nf 4")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("epi", ["full", "bare"])
def test_folded_stem_instances(ops, epi):
    """mode 4 at nf 2 / 4 / 8: the folded 7x7x7 stem as a 4x4x4 convolution over one 32-channel slab, against the float64 4x4x4 convolution of
    the same folded tensors (that the folding itself is right: test_kernels_gpu.test_conv_folded_stem)"""
    B, T, H, W, cout = cc.STEM
    geo = (B, T, H, W, 32, (4, 4, 4), (1, 1, 1))
    p = make_problem(geo, "bf16", epi, cout, 4000, pad=(1, 1, 1))
    wf = fold_stem(rnd((7, 7, 7, 3, cout), 4001, (2.0 / 1029) ** 0.5)).to(torch.bfloat16).float()
    p.update(w=wf, stem4=True, nK=49 * 32)
    r = ref_conv64(p["x"], wf, (1, 1, 1), (1, 1, 1), p["og"])
    p["S"] = ref_conv64(p["x"].abs(), wf.abs(), (1, 1, 1), (1, 1, 1), p["og"])
    if epi == "full":
        r = torch.relu(r * p["scale"].double() + p["bias"].double() + p["add"].double())
        r = torch.where(p["mask"] > 0, r, torch.zeros((), dtype=torch.float64))
    p["r"] = r
    xbuf, kw = device_operands(p, in_ld=32, in_off=0)
    fails, first = [], None
    for nf in cc.STEM_NFS:
        pw = ops.ConvWeights.s2d_stem(wf.numpy(), torch.bfloat16, nf)
        a, _ = ops.conv3d_args(xbuf, pw, out=poisoned(p), out_coff=EDGE, **kw)
        pl = ops.conv_plan_query(a, nf, "bf16", stem4=True)
        assert (pl["route"], pl["wn"], pl["template_mode"]) == ("halo", *cc.STEM_EXPECT[nf][(0, -1)]), pl
        outs, f, worst, _ = run_layouts(ops, p, nf, xbuf, kw, pw=pw)
        fails += f
        y = outs[(0, -1)]
        first = y if first is None else first
        print(f"[instances] stem {epi} nf {nf}: worst |y - r| / bound {worst[(0, -1)]:.3f}; bitwise nf {cc.STEM_NFS[0]}: {torch.equal(bits(y), bits(first))}")
        out = poisoned(p)
        with pytest.raises(ops._lib.FlickerHipError, match="not a layout the autotuner times"):
            ops.conv3d_layout(xbuf, pw, 1, 0, out=out, out_coff=EDGE, **kw)         # the folded stem is never tuned
    assert not fails, "\n".join(fails)


def test_forced_layout_refuses_non_candidates_before_any_launch(ops):
    p = make_problem(cc.GEOMETRIES["k111_short"], "bf16", "bare", cc.COUT, 5000)
    xbuf, kw = device_operands(p)
    for nf, bad in ((4, (4, 1)), (6, (1, 1)), (8, (1, 1)), (2, (2, 1)), (4, (2, 0)), (4, (3, 1)), (4, (0, 1))):
        pw = pack(ops, p, nf)
        out = poisoned(p)
        before = bits(out).clone()
        with pytest.raises(ops._lib.FlickerHipError, match="not a layout the autotuner times"):
            ops.conv3d_layout(xbuf, pw, bad[0], bad[1], out=out, out_coff=EDGE, **kw)
        torch.cuda.synchronize()
        assert torch.equal(bits(out), before), "a refused layout wrote to the output"


ROUTES = [(n, epi) for n in cc.ROUTE_CASES for epi in cc.EPILOGUES]


@pytest.mark.parametrize("name,epi", ROUTES, ids=["-".join(c) for c in ROUTES])
def test_dma_routes_bitwise_the_halo_kernel(ops, name, epi):
    """a geometry the heuristic sends to an LDS-DMA ring kernel: within the bound, and bitwise the forced halo-kernel launch {1, 0}"""
    geo, nf, route = cc.ROUTE_CASES[name]
    p = make_problem(geo, "bf16", epi, cc.COUT, 6000 + 10 * list(cc.ROUTE_CASES).index(name))
    xbuf, kw = device_operands(p)
    pw = pack(ops, p, nf)
    a, _ = ops.conv3d_args(xbuf, pw, out=poisoned(p), out_coff=EDGE, **kw)
    assert ops.conv_plan_query(a, nf, "bf16")["route"] == route
    assert ops.conv_plan_query(a, nf, "bf16", wn=1, da=0)["route"] == "halo"
    fails, outs = [], {}
    for lay in ((0, -1), (1, 0)):
        out, again = poisoned(p), poisoned(p)
        ops.conv3d_layout(xbuf, pw, lay[0], lay[1], out=out, out_coff=EDGE, **kw)
        ops.conv3d_layout(xbuf, pw, lay[0], lay[1], out=again, out_coff=EDGE, **kw)
        torch.cuda.synchronize()
        outs[lay] = out.cpu()
        if not torch.equal(bits(again.cpu()), bits(outs[lay])):
            fails.append(f"layout {lay}: a second launch gave other bits")
        f, worst = check_output(outs[lay], p)
        fails += [f"layout {lay}: {m}" for m in f]
        print(f"[instances] {name} {epi} layout {lay}: worst |y - r| / bound {worst:.3f}")
    if not torch.equal(bits(outs[(0, -1)]), bits(outs[(1, 0)])):
        fails.append(f"the {route} kernel is not bitwise the halo kernel ({int((bits(outs[(0, -1)]) != bits(outs[(1, 0)])).sum())} elements differ)")
    assert not fails, "\n".join(fails)


SPLITK = [(n, epi) for n in cc.SPLITK_CASES for epi in cc.EPILOGUES]


@pytest.mark.parametrize("name,epi", SPLITK, ids=["-".join(c) for c in SPLITK])
def test_splitk_instances(ops, name, epi):
    """conv_splitk_finish_kernel<T> behind every layout a tuning call launches when the caller gives a workspace (the direct-A kernels
    write partial sums too): each candidate splits as pinned, is within the bound, bitwise the heuristic's split launch, and every element
    is within the bound of the one-slice launch (no workspace) as well -- |y_split - y_one| <= the case's bound built from the oracle"""
    geo, dtype, nf, row = cc.SPLITK_CASES[name]
    p = make_problem(geo, dtype, epi, cc.COUT, 7000)
    xbuf, kw = device_operands(p)
    pw = pack(ops, p, nf)
    a, _ = ops.conv3d_args(xbuf, pw, out=poisoned(p), out_coff=EDGE, splitk=True, **kw)
    assert a.splitk_ws
    for lay, want in row.items():
        pl = ops.conv_plan_query(a, nf, dtype, wn=lay[0], da=lay[1], splitk=True)
        assert (pl["route"], pl["wn"], pl["template_mode"], pl["ksplit"]) == ("halo", *want), (lay, pl)
    outs, fails, worst, _ = run_layouts(ops, p, nf, xbuf, kw, pw=pw, splitk=True)
    assert list(outs) == list(row)
    print(f"[instances] {name} {epi} split-K: worst |y - r| / bound " + ", ".join(f"{lay} {w:.3f}" for lay, w in worst.items()))
    one = poisoned(p)
    ops.conv3d_layout(xbuf, pw, 0, -1, out=one, out_coff=EDGE, **kw)
    torch.cuda.synchronize()
    one = one.cpu()
    f, w1 = check_output(one, p)
    fails += [f"one slice: {m}" for m in f]
    y1 = one[..., EDGE:EDGE + p["cout"]].float()
    for lay, y in outs.items():
        if not torch.equal(bits(y), bits(outs[(0, -1)])):
            n = int((bits(y) != bits(outs[(0, -1)])).sum())
            fails.append(f"split-K layout {lay} differs from the heuristic's split launch in {n} elements (the autotuner's contract: speed only)")
        ys = y[..., EDGE:EDGE + p["cout"]].float()
        if dtype == "bf16":
            try:
                bf16_bound_ratio(ys, p["r"], p["S"], p["nK"], scale=p["scale"], bias=p["bias"], add=p["add"], against=y1)
            except AssertionError as e:
                fails.append(f"split-K layout {lay} against the one-slice launch: {e}")
        else:
            rt, at = tol(torch.float32, p["r"])
            bad = ~((ys.double() - y1.double()).abs() <= rt * p["r"].abs() + at)
            if bool(bad.any()):
                fails.append(f"split-K layout {lay}: {int(bad.sum())} elements outside the fp32 tolerance of the one-slice launch")
    assert not fails, "\n".join(fails)


GROUPS = [(n, epis) for n in cc.GROUP_CASES for epis in (("full", "dgrad"), ("bare", "bare"))]


@pytest.mark.parametrize("name,epis", GROUPS, ids=[f"{n}-{'+'.join(e)}" for n, e in GROUPS])
def test_group_instances(ops, name, epis):
    """one grouped launch per conv_igemm_group_kernel<bf16, NFW, MODE>: planned as pinned, every member within the bound and bitwise its own
    forced-layout single launch (the ring at wn 1 for ring groups, direct A at the member's wave count otherwise); once with a full and a
    data-gradient epilogue, once with no epilogue operand at all"""
    from flickering_adversarial_video_amd._lib import FLK_BF16, load
    case = cc.GROUP_CASES[name]
    B, T, H, W, members, nfw, ring, body, want = case
    cin_tot = sum(m[0] for m in members)
    out_ld = sum(m[1] for m in members) + 2 * EDGE
    probs, offs, in_off, out_off = [], [], EDGE, EDGE
    for i, (cin, cout, nf, k) in enumerate(members):
        probs.append(make_problem((B, T, H, W, cin, k, (1, 1, 1)), "bf16", epis[i], cout, 8000 + 100 * i))
        offs.append((in_off, out_off))
        in_off += cin
        out_off += cout
    xbuf = wide(torch.cat([p["x"] for p in probs], -1), cin_tot + 2 * EDGE, EDGE, 904).to(torch.bfloat16).cuda()      # guard channels around the slices
    owned = [(o, o + p["cout"]) for p, (_, o) in zip(probs, offs)]
    weights = [pack(ops, p, m[2]) for p, m in zip(probs, members)]

    def member_kw(i, out):
        p, (ioff, ooff) = probs[i], offs[i]
        _, kw = device_operands(p, xbuf=xbuf)
        kw.update(in_coff=ioff, out=out, out_coff=ooff)
        return kw

    def launch_group():
        out = poisoned(probs[0], ld=out_ld, owned=owned)
        mem = [(xbuf, weights[i], member_kw(i, out)) for i in range(len(members))]
        built = [ops.conv3d_args(x_, w_, **kw_)[0] for x_, w_, kw_ in mem]
        ap = (C.POINTER(ops.ConvArgs) * len(built))(*[C.pointer(a) for a in built])
        wp = (C.c_void_p * len(built))(*[w_.handle for w_ in weights])
        assert load().flk_conv3d_pc_worthwhile(ap, wp, len(built), FLK_BF16) == 0          # (not the producer / consumer kernel)
        got_body, plans = ops.conv_group_plan_query(built, [m[2] for m in members], nfw, ring, "bf16")
        assert got_body == body and [(pl["wn"], pl["mode"]) for pl in plans] == want, (got_body, plans)
        for a, ga in zip(built, (cc.group_member_args(case, i) for i in range(len(members)))):
            assert (a.in_ld, a.in_coff, a.out_ld, a.out_coff, a.cin, a.cout) == (ga.in_ld, ga.in_coff, ga.out_ld, ga.out_coff, ga.cin, ga.cout)
        ops.conv3d_group(mem, nfw, ring=ring)
        torch.cuda.synchronize()
        return out.cpu()

    y = launch_group()
    fails = []
    if not torch.equal(bits(launch_group()), bits(y)):
        fails.append("a second launch gave other bits")
    single = poisoned(probs[0], ld=out_ld, owned=owned)
    keep = [member_kw(i, single) for i in range(len(members))]
    for i, (wn, _) in enumerate(want):
        ops.conv3d_layout(xbuf, weights[i], wn, 0 if ring else 1, **keep[i])
    torch.cuda.synchronize()
    ys = single.cpu()
    for i, (p, (_, ooff)) in enumerate(zip(probs, offs)):
        f, worst = check_output(y, p, off=ooff, others_owned=owned)
        fails += [f"member {i}: {m}" for m in f]
        sl = slice(ooff, ooff + p["cout"])
        if not torch.equal(bits(y[..., sl].contiguous()), bits(ys[..., sl].contiguous())):
            fails.append(f"member {i} is not bitwise its forced-layout single launch")
        print(f"[instances] group {name} member {i}: worst |y - r| / bound {worst:.3f}")
    assert not fails, "\n".join(fails)
