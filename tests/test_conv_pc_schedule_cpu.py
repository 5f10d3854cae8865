"""The persistent producer / consumer kernel's schedule at the launch sizes the plans make (csrc/conv_pc.hip), on the host: per member
its position tiles and XCD chunk, the items per XCD, the workgroups per XCD (`slots`) and the items of the busiest workgroup.  Every
launch of PC_SCALE_CASES gives its workgroups several items in a row -- the path on which the halo images alternate, the weight ring
carries over and member state is kept across items -- and the <8> instance, a tail in the last XCD's chunk and a third member are in the
list.  pc_schedule() is the one model of that schedule; tests/test_conv_pc_scale_gpu.py runs these cases on the GPU and asserts the
same numbers from the device's CU count.  No GPU here: flk_conv3d_pc_query plans on the host (256 CUs without a device)."""
import ctypes as C

import pytest

PC_ROW = 9          # K steps per frame of taps (conv_pc.hip)

# name, B, T, H, W (the shared output grid), members [(cin, cout, kt)] in launch order, data-gradient form,
# expected schedule at 256 CUs: member 0's tile, NI, items per XCD, items of the busiest workgroup, position tiles per member
PC_SCALE_CASES = [
    # the launches the plans make (I3D bf16 at bs 8 runs its stem segment per half batch: Conv3d_2c at 4 clips)
    ("conv2c_fwd", 4, 32, 56, 56, [(64, 192, 3)], False, dict(tile=(8, 7, 8), ni=7, per_xcd=336, busiest=11)),
    ("conv2c_dgrad", 4, 32, 56, 56, [(192, 64, 3)], True, dict(tile=(8, 7, 8), ni=7, per_xcd=112, busiest=4)),
    ("conv2c_fwd_t90", 4, 45, 56, 56, [(64, 192, 3)], False, dict(tile=(9, 7, 7), ni=7, per_xcd=480, busiest=15)),
    ("mixed3c_fwd", 8, 32, 28, 28, [(128, 192, 3), (32, 96, 3)], False, dict(tile=(8, 4, 14), ni=7, per_xcd=280, busiest=9)),
    ("mixed3c_dgrad", 8, 32, 28, 28, [(192, 128, 3), (96, 32, 3)], True, dict(tile=(8, 4, 14), ni=7, per_xcd=168, busiest=6)),
    ("mixed3b_dgrad", 8, 32, 28, 28, [(128, 96, 3), (32, 16, 3)], True, dict(tile=(8, 4, 14), ni=7, per_xcd=168, busiest=6)),
    ("mixed4f_dgrad", 8, 16, 14, 14, [(320, 160, 3), (128, 32, 3)], True, dict(tile=(8, 7, 7), ni=7, per_xcd=32, busiest=1)),
    ("r2plus1d_l1_133_fwd", 8, 16, 56, 56, [(64, 144, 1)], False, dict(tile=(1, 8, 56), ni=7, per_xcd=336, busiest=11)),
    ("r2plus1d_l1_133_dgrad", 8, 16, 56, 56, [(144, 64, 1)], True, dict(tile=(1, 8, 56), ni=7, per_xcd=112, busiest=4)),
    ("mc3_l1_fwd_residual", 16, 16, 56, 56, [(64, 64, 3)], False, dict(tile=(8, 7, 8), ni=7, per_xcd=224, busiest=7)),
    # synthetic: conv_pc_kernel<8> with several items per workgroup and 495 position tiles (the last XCD's chunk has a tail)
    ("ni8_tail", 3, 30, 54, 50, [(64, 192, 3)], False, dict(tile=(10, 5, 10), ni=8, per_xcd=186, busiest=6)),
    # synthetic: three members (PcIter's m = 2 branch), 3x3x3 and 1x3x3 taps, 2 / 1 / 3 slabs, 2 / 1 / 1 channel tiles; epilogues
    # scale-bias-ReLU, scale-bias-add-ReLU (the residual form) and add-mask
    ("three_members", 3, 25, 42, 46, [(64, 128, 3), (32, 64, 1), (96, 40, 3)], False, dict(tile=(5, 6, 16), ni=8, per_xcd=158, busiest=5)),
]


def conv_args(B, T, H, W, cin, cout, kt, in_ld=None, out_ld=None):
    """flk_conv_args of a stride-1 3x3 (kt = 3: 3x3x3; 1: 1x3x3) 'same' convolution on B x T x H x W, no pointers"""
    from flickering_adversarial_video_amd import _lib
    a = _lib.ConvArgs()
    a.B, a.Ti, a.Hi, a.Wi = B, T, H, W
    a.To, a.Ho, a.Wo, a.OT, a.OH, a.OW = T, H, W, T, H, W
    a.kt, a.kh, a.kw = kt, 3, 3
    a.st = a.sh = a.sw = a.ost = a.osh = a.osw = 1
    a.pt, a.ph, a.pw = (kt - 1) // 2, 1, 1
    a.cin, a.cout, a.in_ld, a.out_ld = cin, cout, in_ld or cin, out_ld or cout
    return a


def pc_query(args):
    """flk_conv3d_pc_query of the members in this order: (route 1 / 0 / FLK_E*, member 0's tile, NI, modelled efficiency, busiest K steps)"""
    from flickering_adversarial_video_amd import _lib
    ap = (C.POINTER(_lib.ConvArgs) * len(args))(*[C.pointer(a) for a in args])
    tile, ni, eff, steps = (C.c_int * 3)(), C.c_int(), C.c_double(), C.c_double()
    rc = _lib.load().flk_conv3d_pc_query(ap, len(args), _lib.FLK_BF16, tile, C.byref(ni), C.byref(eff), C.byref(steps))
    return rc, tuple(tile), ni.value, eff.value, steps.value


def pc_schedule(B, T, H, W, members, cus):
    """The schedule flk_conv3d_pc runs for these members (in launch order) on a device of `cus` CUs.  Tile and NI come from
    flk_conv3d_pc_query; it reports member 0's tile, so a member with other taps along T is queried at the front of the same group.
    The rest is conv_pc.hip's host arithmetic (pc_tile, pc_geometry): per member position tiles, an XCD chunk of ceil(tiles / 8)
    of them with all their channel tiles (the last XCD's chunk skips the `tail`), slots = min(CUs / 8, items per XCD), slot j walking
    the XCD-local items j, j + slots, ... -- and the planner's own cost model over that walk, to be checked against the query's."""
    def args(order):
        return [conv_args(B, T, H, W, *members[i]) for i in order]
    n = len(members)
    rc, _, ni, eff, steps = pc_query(args(range(n)))
    tiles = {}
    for i, (_, _, kt) in enumerate(members):
        if kt not in tiles:
            order = [i] + [j for j in range(n) if j != i]
            q = pc_query(args(order))
            assert q[2] == ni and q[4] == steps, ("the planner's choice depends on the member order", q, steps)
            tiles[kt] = q[1]
    mem = []
    for cin, cout, kt in members:
        Tt, Ht, Wt = tiles[kt]
        ptiles = B * -(-T // Tt) * -(-H // Ht) * -(-W // Wt)
        chunk = -(-ptiles // 8)
        ntile = -(-cout // 64)
        mem.append(dict(tile=(Tt, Ht, Wt), rows=Tt * Ht * Wt, ptiles=ptiles, chunk=chunk, tail=8 * chunk - ptiles, ntile=ntile,
                        nslab=-(-cin // 32), kt=kt, cnt=chunk * ntile))
    per_xcd = sum(m["cnt"] for m in mem)
    slots = max(1, min(cus // 8, per_xcd))
    cost = []
    for q in range(per_xcd):
        r, mi = q, 0
        while mi + 1 < n and r >= mem[mi]["cnt"]:
            r -= mem[mi]["cnt"]
            mi += 1
        cost.append((mem[mi]["nslab"] * PC_ROW * mem[mi]["kt"] + 7) * (ni / 8.0))
    model_steps = max(sum(cost[j::slots]) for j in range(slots))
    useful = sum(B * T * H * W / 512.0 * m["ntile"] * m["nslab"] * PC_ROW * m["kt"] / 8.0 for m in mem)
    return dict(rc=rc, ni=ni, members=mem, per_xcd=per_xcd, slots=slots, busiest=-(-per_xcd // slots), grid=8 * slots,
                steps=steps, eff=eff, model_steps=model_steps, model_eff=useful / (model_steps * slots))


def held_slab_skips(s, slots=None):
    """Slab stagings the halo waves would skip in schedule s (pc_schedule's) -- conv_pc.hip's begin_slab replayed per workgroup: the
    workgroup's slabs in item order, slab g staged into image g & 1, skipped when that image still holds the same (member, position
    tile, slab).  slots: workgroups per XCD other than the schedule's (what a smaller device would run)."""
    mem, slots = s["members"], slots or s["slots"]
    skips = 0
    for xcd in range(8):
        for slot in range(slots):
            held, g = [None, None], 0
            for q in range(slot, s["per_xcd"], slots):
                r, mi = q, 0
                while mi + 1 < len(mem) and r >= mem[mi]["cnt"]:
                    r -= mem[mi]["cnt"]
                    mi += 1
                pt = xcd * mem[mi]["chunk"] + r // mem[mi]["ntile"]
                if pt >= mem[mi]["ptiles"]:
                    continue                    # tail of the last XCD's chunk
                for sl in range(mem[mi]["nslab"]):
                    tag = (mi, pt, sl)
                    skips += held[g & 1] == tag and sl < 8
                    held[g & 1] = tag
                    g += 1
    return skips


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("case", PC_SCALE_CASES, ids=[c[0] for c in PC_SCALE_CASES])
def test_pc_schedule_at_launch_sizes_without_gpu(lib, case):
    """Each case is routed to the persistent kernel, plans the tile and NI its comment claims, and its busiest workgroup runs the items the
    table claims -- several for every case but Mixed_4f's (one round).  The schedule model reproduces the planner's own figures (busiest
    workgroup's K steps, efficiency) exactly, so it is the schedule flk_conv3d_pc launches, not a second guess of it."""
    name, B, T, H, W, members, _, want = case
    s = pc_schedule(B, T, H, W, members, 256)
    assert s["rc"] == 1, (name, s)
    assert s["members"][0]["tile"] == want["tile"] and s["ni"] == want["ni"], (name, s)
    assert (s["per_xcd"], s["busiest"]) == (want["per_xcd"], want["busiest"]), (name, s)
    assert s["model_steps"] == pytest.approx(s["steps"], rel=1e-12) and s["model_eff"] == pytest.approx(s["eff"], rel=1e-12), (name, s)
    assert s["slots"] == 32 and all(m["rows"] <= 64 * s["ni"] for m in s["members"])
    if name != "mixed4f_dgrad":
        assert s["busiest"] >= 4, (name, s)
    # the held-slab skip of the halo waves never fires at 256 CUs: a workgroup's next item is on another position tile
    assert held_slab_skips(s) == 0, name
    if name == "conv2c_fwd":
        assert held_slab_skips(s, slots=2) > 0        # (it would with fewer workgroups per XCD than channel tiles per position tile)
    if name == "ni8_tail":
        assert s["ni"] == 8 and s["members"][0]["ptiles"] % 8 != 0 and s["members"][0]["tail"] > 0, s
    if name == "three_members":
        kts = [m["kt"] for m in s["members"]]
        assert len(s["members"]) == 3 and kts == [3, 1, 3] and len({m["tile"] for m in s["members"]}) == 2, s
        assert len({(m["nslab"], m["ntile"]) for m in s["members"]}) == 3, s
