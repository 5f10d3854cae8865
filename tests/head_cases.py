"""Shapes and data of the classifier-head tests, shared by tests/test_head_contract_cpu.py (which proves the exact data exact) and
tests/test_head_edges_gpu.py (which relies on that for its zero tolerance).

A case is (B, Tn, HW, C, N).  Each list names the seam of csrc/head.hip its shapes are the smallest to reach:
  head_pool_kernel      4 position groups; the unrolled loop takes 8 positions per group while i + 28 < npos, the tail one
  head_fc_kernel        64 classes x 16 channel groups per workgroup; unrolled over 128 channels while c + 112 < C; sf[2048]
  head_fc_bwd_kernel    16 channels x 16 lanes per workgroup; sd[1024] filled 256 at a time
  head_pool_bwd_kernel  one thread per 16-byte group, at most 8192 x 256 threads, grid-stride beyond"""
import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16


def epl(dtype):
    """elements per 16-byte group"""
    return 8 if dtype == BF16 else 4


# (Tn, HW) with npos = Tn * HW in {1, 3, 4, 5, 28, 29, 32, 33, 36, 61, 64, 65}: each npos once as a single frame or as one position per frame
# and, where it factors, with frame boundaries inside the unrolled group of 32 positions (HW = 3, 7, 13) and inside the tail
POOL_SEAMS = [(1, 1), (1, 3), (3, 1), (4, 1), (1, 4), (5, 1), (4, 7), (1, 29), (29, 1), (32, 1), (8, 4), (11, 3), (3, 11), (12, 3), (61, 1),
              (1, 61), (8, 8), (64, 1), (5, 13), (13, 5), (65, 1)]
POOL_CASES = [(2, Tn, HW, 64, 5) for Tn, HW in POOL_SEAMS]
assert {c[1] * c[2] for c in POOL_CASES} == {1, 3, 4, 5, 28, 29, 32, 33, 36, 61, 64, 65}

CHANNEL_CASES = [(2, 2, 3, C, 5) for C in (8, 16, 56, 64, 72, 136, 2048)]
CLASS_CASES = [(2, 2, 3, C, N) for C in (72, 1024) for N in (1, 2, 15, 16, 17, 51, 63, 64, 65, 359, 400, 487, 1024)]
SMALL_CASES = POOL_CASES + CHANNEL_CASES + CLASS_CASES

# head_pool_bwd_kernel's cap is 8192 workgroups x 256 threads = 2 097 152 groups of 16 bytes: exactly at it, and 2048 groups past it (so
# that some threads take a second trip of the grid-stride loop and most do not)
CAP_GROUPS = 8192 * 256
GRID_CASES = {F32: [(4, 4, 256, 2048, 16), (5, 4, 205, 2048, 16)], BF16: [(4, 8, 256, 2048, 16), (5, 4, 410, 2048, 16)]}
for _dt, _cases in GRID_CASES.items():
    _g = [b * t * hw * (c // epl(_dt)) for b, t, hw, c, n in _cases]
    assert _g[0] == CAP_GROUPS and CAP_GROUPS < _g[1] < 2 * CAP_GROUPS, (_dt, _g)

BIAS_NONE_CASE = (2, 3, 11, 72, 65)
SLICE_CASE = (2, 3, 11, 72, 17)
MASK_CASE = (2, 2, 5, 64, 17)
REPEAT_CASE = (3, 3, 11, 136, 65)

# the engines' own heads: I3D (frame weights of the 2x7x7 pool) and VideoResNet (plain mean), at small time extents
I3D_HEADS = [(2, Tn, 49, 1024, 400) for Tn in (2, 3, 8)]
VRN_HEADS = [(2, 1, 49, 512, 400), (2, 2, 49, 512, 359), (2, 4, 196, 512, 487)]


def case_id(case):
    return "B{}-T{}-HW{}-C{}-N{}".format(*case)


def seed_of(case):
    B, Tn, HW, C, N = case
    return ((B * 131 + Tn) * 131 + HW) * 4099 + C * 1031 + N


def frame_weights(Tn):
    """distinct powers of two for 8 consecutive frames: a position charged to a neighbouring frame changes the sum"""
    return torch.tensor([2.0 ** -(t % 8) for t in range(Tn)], dtype=F32)


FEAT_GRAIN = 2.0 ** -7        # every term of feat and of logits is a multiple of this on the exact data; dfeat's terms are integers


def exact_data(case):
    """Small integers and powers of two: every product and, with the magnitudes checked in test_head_contract_cpu.py, every partial sum in
    any order is exact in fp32.  y in -2..2 (bf16-representable) with planted +0.0 and -0.0; W, dlogits in -2..2; bias in -4..4."""
    B, Tn, HW, C, N = case
    rng = np.random.default_rng(seed_of(case))
    y = rng.integers(-2, 3, size=(B, Tn, HW, C)).astype(np.float32)
    r = rng.random(size=y.shape)
    y[r < 0.08] = 0.0
    y[(r >= 0.08) & (r < 0.16)] = -0.0
    return {"y": torch.from_numpy(y), "wt": frame_weights(Tn),
            "W": torch.from_numpy(rng.integers(-2, 3, size=(C, N)).astype(np.float32)),
            "bias": torch.from_numpy(rng.integers(-4, 5, size=(N,)).astype(np.float32)),
            "dlogits": torch.from_numpy(rng.integers(-2, 3, size=(B, N)).astype(np.float32))}


def random_data(case, wt=None):
    """standard normal data (y has both signs, so the mask matters); wt: the frame weights (default: positive random ones)"""
    B, Tn, HW, C, N = case
    rng = np.random.default_rng(seed_of(case) + 1)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    if wt is None:
        wt = torch.from_numpy((rng.random(Tn) + 0.25).astype(np.float32) / (Tn * HW))
    return {"y": f(B, Tn, HW, C), "wt": wt.to(F32), "W": f(C, N), "bias": f(N), "dlogits": f(B, N)}
