"""Which compiled convolution kernel every case of tests/conv_instance_cases.py runs -- decided on the host, checked here without a GPU.

csrc/conv_igemm.hip is compiled into some sixty kernels (conv_igemm_kernel<T, NF, WN, MODE>, its grouped form, the two LDS-DMA rings, the
split-K finish) and conv_plan picks one from the geometry.  The instantiation set is read from the built library's kernel symbol names;
flk_conv_plan_query / flk_conv_group_plan_query (conv_plan and group_plan themselves, no device work) say where a case lands:
  (a) every case lands on an instantiation that exists, and on the one the table pins for it;
  (b) every instantiation in the library is hit by at least one case -- a new instantiation without a case fails here, and so does one
      that no argument can reach (dead code: remove the instantiation);
  (c) per (geometry, packing) the table's layouts are exactly the candidate list the autotuner times, so every layout a tuning call
      launches on the caller's operands is a case of tests/test_conv_instances_gpu.py;
and every case has the shape the table's docstring promises (tiles, partial channel tile, partial K slab, offsets)."""
import ctypes as C

import pytest

import conv_instance_cases as cc


@pytest.fixture(scope="module")
def ops():
    from flickering_adversarial_video_amd import build, ops as o
    build.build(verbose=False)
    return o


@pytest.fixture(scope="module")
def instances():
    from flickering_adversarial_video_amd import build
    return cc.library_instances(build.build(verbose=False))


def planned_instances(ops):
    """{instantiation: [case ids]} over the whole table, each case asserted against its pin on the way"""
    hit = {}

    def add(inst, case):
        hit.setdefault(inst, []).append(case)

    for g, dt, nf, lay, want in cc.halo_cases():
        p = ops.conv_plan_query(cc.geometry_args(cc.GEOMETRIES[g]), nf, dt, wn=lay[0], da=lay[1])
        assert (p["route"], p["nf"], p["ksplit"]) == ("halo", nf, 1), (g, dt, nf, lay, p)
        assert (p["wn"], p["template_mode"]) == want, (g, dt, nf, lay, p)
        add(("conv_igemm_kernel", dt, nf, *want), (g, dt, nf, lay))
    for nf, row in cc.STEM_EXPECT.items():
        for lay, want in row.items():
            p = ops.conv_plan_query(cc.stem_args(), nf, "bf16", stem4=True, wn=lay[0], da=lay[1])
            assert (p["route"], p["wn"], p["template_mode"], p["mode"]) == ("halo", *want, 4), (nf, p)
            add(("conv_igemm_kernel", "bf16", nf, *want), ("stem", nf, lay))
    for name, (geo, nf, route) in cc.ROUTE_CASES.items():
        a = cc.geometry_args(geo)
        p = ops.conv_plan_query(a, nf, "bf16")
        assert p["route"] == route and p["nf"] == nf, (name, p)
        add((cc.ROUTE_KERNEL[route], None, nf, *((2, int(route == "t3_tiled")) if route.startswith("t3") else (3,))), name)
        h = ops.conv_plan_query(a, nf, "bf16", wn=1, da=0)           # the forced halo launch the GPU test compares the route with
        assert (h["route"], h["wn"], h["template_mode"]) == ("halo", 1, 0), (name, h)
        add(("conv_igemm_kernel", "bf16", nf, 1, 0), name + "/halo")
    for name, (geo, dt, nf, row) in cc.SPLITK_CASES.items():
        a = cc.geometry_args(geo)
        for lay, want in row.items():
            p = ops.conv_plan_query(a, nf, dt, wn=lay[0], da=lay[1], splitk=True)
            assert (p["route"], p["wn"], p["template_mode"], p["ksplit"]) == ("halo", *want) and want[2] > 1, (name, lay, p)
            add(("conv_splitk_finish_kernel", dt), (name, lay))
            add(("conv_igemm_kernel", dt, nf, *want[:2]), (name, lay))
        assert ops.conv_plan_query(a, nf, dt)["ksplit"] == 1, name       # no workspace, no split
    for name, case in cc.GROUP_CASES.items():
        members, nfw, ring, body, want = case[4:]
        args = [cc.group_member_args(case, i) for i in range(len(members))]
        got_body, plans = ops.conv_group_plan_query(args, [m[2] for m in members], nfw, ring, "bf16")
        assert got_body == body, (name, got_body, plans)
        assert [(p["wn"], p["mode"]) for p in plans] == want, (name, plans)
        add(("conv_igemm_group_kernel", "bf16", nfw, body), name)
    return hit


def test_every_case_lands_on_its_pinned_instantiation_and_it_exists(ops, instances):
    hit = planned_instances(ops)
    missing = {inst: cases[:3] for inst, cases in hit.items() if inst not in instances}
    assert not missing, f"cases planned for kernels the library does not contain: {missing}"


def test_every_instantiation_in_the_library_is_hit_by_a_case(ops, instances):
    assert len(instances) >= 40, sorted(instances)            # (the symbol scan itself found the library's kernels)
    counts = {}
    for inst in instances:
        counts[inst[0]] = counts.get(inst[0], 0) + 1
    print("\ninstantiations in the library:", sum(counts.values()), counts)
    hit = planned_instances(ops)
    orphans = sorted(i for i in instances if i not in hit)
    assert not orphans, f"instantiations without a case (add one to tests/conv_instance_cases.py, or remove dead instantiations): {orphans}"


def test_case_table_holds_exactly_the_autotuner_candidates(ops):
    """(c), and the table is the full product: every geometry at every packing of both dtypes, every candidate layout of that packing"""
    rows = set(cc.HALO_EXPECT)
    assert rows == {(g, dt, nf) for g in cc.GEOMETRIES for dt, nfs in cc.NFS.items() for nf in nfs}, "a (geometry, dtype, nf) row is missing"
    for (g, dt, nf), row in cc.HALO_EXPECT.items():
        assert list(row) == ops.conv_layout_candidates(nf, dt), (g, dt, nf)
    for nf, row in cc.STEM_EXPECT.items():
        assert list(row) == ops.conv_layout_candidates(nf, "bf16", stem4=True) == [(0, -1)], nf
    for name, (_, dt, nf, row) in cc.SPLITK_CASES.items():
        assert list(row) == ops.conv_layout_candidates(nf, dt), name
    assert set(cc.STEM_EXPECT) == set(cc.STEM_NFS)


def test_cases_have_the_promised_shape(ops):
    for g, dt, nf, lay, _ in cc.halo_cases():
        a = cc.geometry_args(cc.GEOMETRIES[g])
        p = ops.conv_plan_query(a, nf, dt, wn=lay[0], da=lay[1])
        og = (a.To, a.Ho, a.Wo)
        ntiles = [-(-o // t) for o, t in zip(og, p["tile"])]
        axes, partial = cc.TILING.get(g, cc.TILING_DEFAULT)
        assert a.B == 2 and sum(n >= 2 for n in ntiles) >= axes, (g, dt, nf, lay, p)
        assert not partial or any(o % t for o, t in zip(og, p["tile"])), (g, dt, nf, lay, p)
        assert a.cout % 16 == 8 and a.cout % (16 * nf) and a.cout > 16 * nf, (g, nf)          # a partial channel tile behind a full one
        assert a.cin % (32 if dt == "bf16" else 16) and a.in_coff > 0 and a.out_coff > 0 and a.in_ld > a.in_coff + a.cin, (g, dt)
    for nf in cc.STEM_NFS:
        a = cc.stem_args()
        p = ops.conv_plan_query(a, nf, "bf16", stem4=True)
        ntiles = [-(-o // t) for o, t in zip((a.To, a.Ho, a.Wo), p["tile"])]
        assert a.B == 2 and sum(n >= 2 for n in ntiles) >= 2 and a.cout % 16 == 8 and a.cout > 16 * nf, (nf, p)


def test_modes_select_themselves_as_documented(ops):
    """the rules the case table leans on, from the planner itself: the row-ahead ring needs kw = 3 and a halo above 256 cells at wn = 1;
    one tap with a halo of at most 256 cells is a '1x1x1' (ring: mode 3 from 4 K slabs, mode 0 below; direct A: mode 2)"""
    for g, dt, nf, lay, (wn, tmode) in cc.halo_cases():
        geo = cc.GEOMETRIES[g]
        p = ops.conv_plan_query(cc.geometry_args(geo), nf, dt, wn=lay[0], da=lay[1])
        one_tap = geo[5] == (1, 1, 1) and p["halo"] <= 256
        slabs = -(-geo[4] // (32 if dt == "bf16" else 16))
        if p["mode"] == 5:
            assert dt == "bf16" and geo[5][2] == 3 and p["halo"] > 256 and wn == 1 and tmode == (6 if nf <= 4 else 5), (g, dt, nf, lay, p)
        elif p["mode"] in (2, 3):
            assert one_tap and (p["mode"] == 2 or slabs >= 4), (g, dt, nf, lay, p)
        elif p["mode"] == 0:
            assert wn == 1 and (not one_tap or slabs < 4) and not (dt == "bf16" and geo[5][2] == 3 and p["halo"] > 256), (g, dt, nf, lay, p)
        else:
            assert p["mode"] == 1 and not one_tap, (g, dt, nf, lay, p)


def test_plan_query_reports_clamped_requests_as_they_run(ops):
    a = cc.geometry_args(cc.GEOMETRIES["k333"])
    p = ops.conv_plan_query(a, 6, "bf16", wn=1, da=1)             # 96-channel tiles have no direct-A kernels
    assert (p["wn"], p["mode"], p["template_mode"]) == (1, 5, 5), p
    p = ops.conv_plan_query(a, 6, "bf16", wn=4, da=1)             # ... and one wave layout
    assert (p["wn"], p["mode"]) == (1, 5), p
    p = ops.conv_plan_query(a, 4, "bf16", wn=4, da=1)             # two fragments per wave at least in bf16: wn <= 2 at nf 4
    assert (p["wn"], p["mode"]) == (2, 1), p
    p = ops.conv_plan_query(a, 8, "bf16", wn=1, da=1)             # direct A holds at most four fragments per wave
    assert (p["wn"], p["mode"], p["template_mode"]) == (1, 5, 5), p
    p = ops.conv_plan_query(a, 2, "bf16", wn=1, da=0)
    assert (p["mode"], p["template_mode"]) == (5, 6), p           # planner mode 5 runs template 6 on narrow tiles


def test_layout_candidates_and_host_side_refusals(ops):
    """the candidate family (ring at wn 1; direct A wherever a wave keeps 2..4 fragments in bf16, 1..4 in fp32; never on 96-channel tiles),
    and the null checks of the new entries (no device work).  flk_conv3d_layout's refusal of a layout outside the list needs a weights
    object: tests/test_conv_instances_gpu.py"""
    from flickering_adversarial_video_amd import _lib
    lib = _lib.load()
    a = cc.geometry_args(cc.GEOMETRIES["k333"])
    assert lib.flk_conv3d_layout(C.byref(a), None, _lib.FLK_BF16, 1, 0, None) == -1 and b"null argument" in lib.flk_last_error()
    assert lib.flk_conv_plan_query(None, 4, _lib.FLK_BF16, 0, 0, 0, -1, 0, None) == -1
    for nf, dt in ((2, "bf16"), (4, "bf16"), (6, "bf16"), (8, "bf16"), (2, "f32"), (4, "f32"), (8, "f32")):
        cands = ops.conv_layout_candidates(nf, dt)
        assert cands[0] == (0, -1) and (1, 0) in cands and len(set(cands)) == len(cands)
        for wn, da in cands[1:]:
            nfw = nf // wn
            assert da == 0 and wn == 1 or da == 1 and nf != 6 and nfw <= 4 and (dt == "f32" or nfw >= 2), (nf, dt, wn, da)
