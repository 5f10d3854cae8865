"""The case table of tests/test_conv_instances_cpu.py (planning only, no GPU) and tests/test_conv_instances_gpu.py (every case launched
against the float64 oracle): one case per (geometry, dtype, packing nf, requested launch layout {wn, da}), with the kernel instantiation
the planner sends it to PINNED here.  A retuned heuristic, a new instantiation or a removed one shows up as a change of this table.

Geometries are the smallest at which an instance can still go wrong: two clips, at least two position tiles along two axes with a
partial last tile, cout % 16 == 8 (neither a multiple of a channel tile nor of a 16-channel fragment), cin = 40 or 104 (no multiple of
a K slab: 32 channels in bf16, 16 in fp32), the operands at channel offset EDGE inside wider buffers.

The instantiation set itself is read from the built library's kernel symbol names (library_instances)."""
import re

EDGE = 8            # channels in front of and behind the slices a case reads / writes
COUT = 136          # 8 full 16-channel fragments + half of one: a partial channel tile at every packing (32 / 64 / 96 / 128 channels)
NFS = {"bf16": (2, 4, 6, 8), "f32": (2, 4, 8)}
ROUTE_KERNEL = {"halo": "conv_igemm_kernel", "t3": "conv_t3_dma_kernel", "t3_tiled": "conv_t3_dma_kernel", "dma1x1": "conv1x1_dma_kernel"}

# name: (B, T, H, W of the input, cin, k, stride).  TF SAME padding, the output grid that goes with it.
GEOMETRIES = {
    # 3-tap rows over a halo of more than 256 cells at wn = 1: the row-ahead ring (planner mode 5 -> template 5 / 6) in bf16, the plain ring
    # in fp32, direct-A (mode 1) at every wave layout
    "k333": (2, 6, 11, 12, 40, (3, 3, 3), (1, 1, 1)),
    # one tap, 2 (bf16) / 3 (fp32) K slabs: ring mode 0, direct-A mode 2
    "k111_short": (2, 2, 11, 41, 40, (1, 1, 1), (1, 1, 1)),
    # one tap, 4 (bf16) / 7 (fp32) K slabs: ring mode 3, direct-A mode 2
    "k111_long": (2, 2, 11, 41, 104, (1, 1, 1), (1, 1, 1)),
    # strided spatial taps (the spatial half of a strided (2+1)D unit): row-ahead ring / direct-A over a strided halo
    "k133_s122": (2, 2, 33, 37, 40, (1, 3, 3), (1, 2, 2)),
    # strided temporal taps: kw = 1, so the plain multi-tap ring (mode 0) in bf16 as well
    "k311_s211": (2, 5, 14, 23, 40, (3, 1, 1), (2, 1, 1)),
    # the strided 1x1x1 downsample: one tap over a halo with holes
    "k111_s222": (2, 5, 13, 15, 104, (1, 1, 1), (2, 2, 2)),
    # the same over a halo of more than 256 cells: no longer a "1x1x1" to the planner, the multi-tap kernels (mode 0 / 1) run it with one tap
    "k111_s222_wide": (2, 3, 33, 33, 104, (1, 1, 1), (2, 2, 2)),
    # a strided one-tap form whose tiles the chooser does split: temporal stride only, the halo stays below 256 cells -- the strided
    # mode 2 / 3 instances over two tiled axes with a ragged last tile, at every layout
    "k111_s211": (2, 3, 17, 17, 104, (1, 1, 1), (2, 1, 1)),
    # even taps, generic packing (what the fp32 folded stem runs): mode 0 / 1
    "k444": (2, 2, 17, 22, 40, (4, 4, 4), (1, 1, 1)),
}
EPILOGUES = ("full", "bare", "dgrad")      # scale, bias, add, ReLU, mask | nothing | transposed pack x row_scale, mask

# the folded stem (bf16 mode 4: 4x4x4 taps over ONE 32-channel slab, K steps from the non-zero chunks): B, T, H, W of the folded clip, cout
STEM = (2, 3, 13, 13, COUT)
STEM_NFS = (2, 4, 8)


def same_pad(n, k, s):
    out = -(-n // s)
    return out, max((out - 1) * s + k - n, 0) // 2


def geometry_args(geo, cout=COUT):
    """flk_conv_args of a geometry with the buffers' strides and offsets of the GPU test and no pointers: all that planning reads"""
    from flickering_adversarial_video_amd import _lib
    B, T, H, W, cin, k, s = geo
    a = _lib.ConvArgs()
    a.B, a.Ti, a.Hi, a.Wi = B, T, H, W
    a.kt, a.kh, a.kw = k
    a.st, a.sh, a.sw = s
    og, pad = zip(*(same_pad(n, kk, ss) for n, kk, ss in zip((T, H, W), k, s)))
    a.pt, a.ph, a.pw = pad
    a.To, a.Ho, a.Wo = a.OT, a.OH, a.OW = og
    a.ost = a.osh = a.osw = 1
    a.cin, a.in_ld, a.in_coff = cin, cin + 2 * EDGE, EDGE
    a.cout, a.out_ld, a.out_coff = cout, cout + 2 * EDGE, EDGE
    return a


def stem_args():
    B, T, H, W, cout = STEM
    a = geometry_args((B, T, H, W, 32, (4, 4, 4), (1, 1, 1)), cout)
    a.in_ld, a.in_coff = 32, 0              # (the stem reads the whole folded clip)
    a.pt = a.ph = a.pw = 1
    return a


# ---- the pinned table ------------------------------------------------------------------------------------------------------------------
# (geometry, dtype, nf): {(wn, da) requested: (wn, template MODE) of the conv_igemm_kernel<dtype, nf, wn, MODE> it runs}; the keys of a row
# are, in order, the autotuner's candidate list for that packing ((0, -1) = the heuristic's own choice)
HALO_EXPECT = {
    ('k333', 'bf16', 2): {(0, -1): (1, 6), (1, 0): (1, 6), (1, 1): (1, 1)},
    ('k333', 'bf16', 4): {(0, -1): (2, 1), (1, 0): (1, 6), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k333', 'bf16', 6): {(0, -1): (1, 5), (1, 0): (1, 5)},
    ('k333', 'bf16', 8): {(0, -1): (4, 1), (1, 0): (1, 5), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k333', 'f32', 2): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k333', 'f32', 4): {(0, -1): (4, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k333', 'f32', 8): {(0, -1): (4, 1), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k111_short', 'bf16', 2): {(0, -1): (1, 0), (1, 0): (1, 0), (1, 1): (1, 2)},
    ('k111_short', 'bf16', 4): {(0, -1): (2, 2), (1, 0): (1, 0), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_short', 'bf16', 6): {(0, -1): (1, 0), (1, 0): (1, 0)},
    ('k111_short', 'bf16', 8): {(0, -1): (4, 2), (1, 0): (1, 0), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_short', 'f32', 2): {(0, -1): (2, 2), (1, 0): (1, 0), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_short', 'f32', 4): {(0, -1): (4, 2), (1, 0): (1, 0), (1, 1): (1, 2), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_short', 'f32', 8): {(0, -1): (4, 2), (1, 0): (1, 0), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_long', 'bf16', 2): {(0, -1): (1, 3), (1, 0): (1, 3), (1, 1): (1, 2)},
    ('k111_long', 'bf16', 4): {(0, -1): (2, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_long', 'bf16', 6): {(0, -1): (1, 3), (1, 0): (1, 3)},
    ('k111_long', 'bf16', 8): {(0, -1): (4, 2), (1, 0): (1, 3), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_long', 'f32', 2): {(0, -1): (2, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_long', 'f32', 4): {(0, -1): (4, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_long', 'f32', 8): {(0, -1): (4, 2), (1, 0): (1, 3), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k133_s122', 'bf16', 2): {(0, -1): (1, 6), (1, 0): (1, 6), (1, 1): (1, 1)},
    ('k133_s122', 'bf16', 4): {(0, -1): (2, 1), (1, 0): (1, 6), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k133_s122', 'bf16', 6): {(0, -1): (1, 5), (1, 0): (1, 5)},
    ('k133_s122', 'bf16', 8): {(0, -1): (4, 1), (1, 0): (1, 5), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k133_s122', 'f32', 2): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k133_s122', 'f32', 4): {(0, -1): (4, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k133_s122', 'f32', 8): {(0, -1): (4, 1), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k311_s211', 'bf16', 2): {(0, -1): (1, 0), (1, 0): (1, 0), (1, 1): (1, 1)},
    ('k311_s211', 'bf16', 4): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k311_s211', 'bf16', 6): {(0, -1): (1, 0), (1, 0): (1, 0)},
    ('k311_s211', 'bf16', 8): {(0, -1): (4, 1), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k311_s211', 'f32', 2): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k311_s211', 'f32', 4): {(0, -1): (4, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k311_s211', 'f32', 8): {(0, -1): (4, 1), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k111_s222', 'bf16', 2): {(0, -1): (1, 3), (1, 0): (1, 3), (1, 1): (1, 2)},
    ('k111_s222', 'bf16', 4): {(0, -1): (2, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_s222', 'bf16', 6): {(0, -1): (1, 3), (1, 0): (1, 3)},
    ('k111_s222', 'bf16', 8): {(0, -1): (4, 2), (1, 0): (1, 3), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_s222', 'f32', 2): {(0, -1): (2, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_s222', 'f32', 4): {(0, -1): (4, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_s222', 'f32', 8): {(0, -1): (4, 2), (1, 0): (1, 3), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_s222_wide', 'bf16', 2): {(0, -1): (1, 0), (1, 0): (1, 0), (1, 1): (1, 1)},
    ('k111_s222_wide', 'bf16', 4): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k111_s222_wide', 'bf16', 6): {(0, -1): (1, 0), (1, 0): (1, 0)},
    ('k111_s222_wide', 'bf16', 8): {(0, -1): (4, 2), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 2)},
    ('k111_s222_wide', 'f32', 2): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k111_s222_wide', 'f32', 4): {(0, -1): (4, 2), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1), (4, 1): (4, 2)},
    ('k111_s222_wide', 'f32', 8): {(0, -1): (4, 2), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 2)},
    ('k111_s211', 'bf16', 2): {(0, -1): (1, 3), (1, 0): (1, 3), (1, 1): (1, 2)},
    ('k111_s211', 'bf16', 4): {(0, -1): (2, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_s211', 'bf16', 6): {(0, -1): (1, 3), (1, 0): (1, 3)},
    ('k111_s211', 'bf16', 8): {(0, -1): (4, 2), (1, 0): (1, 3), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_s211', 'f32', 2): {(0, -1): (2, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2)},
    ('k111_s211', 'f32', 4): {(0, -1): (4, 2), (1, 0): (1, 3), (1, 1): (1, 2), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k111_s211', 'f32', 8): {(0, -1): (4, 2), (1, 0): (1, 3), (2, 1): (2, 2), (4, 1): (4, 2)},
    ('k444', 'bf16', 2): {(0, -1): (1, 0), (1, 0): (1, 0), (1, 1): (1, 1)},
    ('k444', 'bf16', 4): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k444', 'bf16', 6): {(0, -1): (1, 0), (1, 0): (1, 0)},
    ('k444', 'bf16', 8): {(0, -1): (4, 1), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k444', 'f32', 2): {(0, -1): (2, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1)},
    ('k444', 'f32', 4): {(0, -1): (4, 1), (1, 0): (1, 0), (1, 1): (1, 1), (2, 1): (2, 1), (4, 1): (4, 1)},
    ('k444', 'f32', 8): {(0, -1): (4, 1), (1, 0): (1, 0), (2, 1): (2, 1), (4, 1): (4, 1)},
}
# tiling of the position grid every case must show: (axes with >= 2 tiles, a partial last tile on one of them).  The strided one-tap forms
# are the exception -- the tile chooser weighs the halo against ONE tap and never splits a row of such a grid, at four waves along the
# channels it takes single rows: their tiles split T (and H in the wide form) only, and the wide form's single-row tiles are all whole.
# k111_s211 is the strided one-tap geometry that meets the rule at every layout.
TILING = {"k111_s222": (1, False), "k111_s222_wide": (2, False)}
TILING_DEFAULT = (2, True)
STEM_EXPECT = {nf: {(0, -1): (1, 4)} for nf in STEM_NFS}


def halo_cases():
    """[(geometry name, dtype, nf, (wn, da), (wn, template mode))] of every pinned conv_igemm_kernel case"""
    return [(g, dt, nf, lay, exp) for (g, dt, nf), row in HALO_EXPECT.items() for lay, exp in row.items()]


# ---- routes beside the halo kernel (they need >= 2048 positions) --------------------------------------------------------------------------
# name: (geometry, nf, route, requested layout); T3: (3,1,1) taps, stride 1, T in {2, 4, 8, 16} or a multiple of 16 (tiled), H * W % 16 == 0
ROUTE_CASES = {
    "t3_nf4": ((2, 8, 8, 16, 72, (3, 1, 1), (1, 1, 1)), 4, "t3"),
    "t3_nf8": ((2, 16, 8, 8, 72, (3, 1, 1), (1, 1, 1)), 8, "t3"),
    "t3_tiled_nf4": ((2, 32, 4, 8, 72, (3, 1, 1), (1, 1, 1)), 4, "t3_tiled"),
    "t3_tiled_nf8": ((2, 32, 4, 8, 72, (3, 1, 1), (1, 1, 1)), 8, "t3_tiled"),
    "dma1x1_nf4": ((2, 3, 19, 19, 72, (1, 1, 1), (1, 1, 1)), 4, "dma1x1"),
    "dma1x1_nf6": ((2, 3, 19, 19, 72, (1, 1, 1), (1, 1, 1)), 6, "dma1x1"),
    "dma1x1_nf8": ((2, 3, 19, 19, 72, (1, 1, 1), (1, 1, 1)), 8, "dma1x1"),
}
# split-K (a workspace is given, few output tiles, >= 4 K slabs of a multi-tap convolution): (geometry, dtype, nf, {layout requested:
# (wn, template MODE, slices)}).  A tuning call on a launch with a workspace times the same candidate list, and every candidate keeps the
# split: the direct-A kernels write partial sums too.  The rows are the autotuner's candidate list of the packing, in order.
SPLITK_CASES = {
    "splitk_bf16": ((2, 3, 7, 9, 136, (3, 3, 3), (1, 1, 1)), "bf16", 4,
                    {(0, -1): (1, 6, 5), (1, 0): (1, 6, 5), (1, 1): (1, 1, 5), (2, 1): (2, 1, 5)}),
    "splitk_f32": ((2, 3, 7, 9, 72, (3, 3, 3), (1, 1, 1)), "f32", 4,
                   {(0, -1): (1, 0, 5), (1, 0): (1, 0, 5), (1, 1): (1, 1, 5), (2, 1): (2, 1, 5), (4, 1): (4, 1, 5)}),
}

# ---- grouped launches: one per conv_igemm_group_kernel<bf16, NFW, MODE> ---------------------------------------------------------------------
# name: (B, T, H, W, [(cin, cout, nf, taps)], nfw, ring, body MODE, [(wn, planner mode) of each member]).  A ring group runs the row-ahead
# body only when EVERY member is planned for it (3-tap rows, large halo): the "plain" groups pair such a member with (3,1,1) taps, and the
# mode-0 body then runs both
K3, KT = (3, 3, 3), (3, 1, 1)
GROUP_CASES = {
    "direct_nfw2": (2, 3, 7, 9, [(72, 136, 8, K3), (40, 40, 2, K3)], 2, False, 1, [(4, 1), (1, 1)]),
    "direct_nfw4": (2, 3, 7, 9, [(72, 136, 8, K3), (40, 72, 4, K3)], 4, False, 1, [(2, 1), (1, 1)]),
    "ring_nfw4_plain": (2, 5, 9, 11, [(72, 136, 4, K3), (40, 72, 4, KT)], 4, True, 0, [(1, 5), (1, 0)]),
    "ring_nfw8_plain": (2, 5, 9, 11, [(72, 136, 8, K3), (40, 72, 8, KT)], 8, True, 0, [(1, 5), (1, 0)]),
    "ring_nfw4_row_ahead": (2, 5, 9, 11, [(72, 136, 4, K3), (40, 72, 4, K3)], 4, True, 6, [(1, 5), (1, 5)]),
    "ring_nfw8_row_ahead": (2, 5, 9, 11, [(72, 136, 8, K3), (40, 72, 8, K3)], 8, True, 5, [(1, 5), (1, 5)]),
}


def group_member_args(case, i):
    """member i of a grouped case: its channel slice of the shared input buffer, its slice of the shared output buffer (EDGE guard
    channels in front of and behind the members' slices in both)"""
    B, T, H, W, members = case[:5]
    cin, cout, _, k = members[i]
    a = geometry_args((B, T, H, W, cin, k, (1, 1, 1)), cout)
    a.in_ld, a.in_coff = sum(m[0] for m in members) + 2 * EDGE, EDGE + sum(m[0] for m in members[:i])
    a.out_ld, a.out_coff = sum(m[1] for m in members) + 2 * EDGE, EDGE + sum(m[1] for m in members[:i])
    return a


# ---- the instantiations of the built library -------------------------------------------------------------------------------------------------
_DT = {b"DF16b": "bf16", b"f": "f32"}
_SYM = re.compile(rb"_Z\d+(conv_igemm_kernel|conv_igemm_group_kernel|conv1x1_dma_kernel|conv_t3_dma_kernel|conv_splitk_finish_kernel)"
                  rb"I((?:DF16b|f)?)((?:L[ib]\d+E)*)Ev\d+Conv(?:Group)?KP")


def library_instances(path):
    """{(kernel, dtype or None, template integers...)} from the kernel symbol names in the built library, e.g.
    _Z17conv_igemm_kernelIDF16bLi4ELi1ELi6EEv6ConvKP -> ('conv_igemm_kernel', 'bf16', 4, 1, 6)"""
    blob = open(path, "rb").read()
    found = set()
    for m in _SYM.finditer(blob):
        ints = tuple(int(v) for v in re.findall(rb"L[ib](\d+)E", m.group(3)))
        found.add((m.group(1).decode(), _DT.get(m.group(2)), *ints))
    return found
