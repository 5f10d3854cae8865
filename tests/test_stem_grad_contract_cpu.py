"""The fused stem delta-gradient (csrc/stem_grad.hip) on a machine without a GPU: the host-only chunking query
flk_stem_delta_grad_chunks, and the pointer contract of flk_stem_delta_grad / flk_stem_delta_grad_mask (include/flicker_hip.h) -- every
refusal is FLK_EINVAL with a message naming the alignment, and it comes BEFORE any GPU call.  Fake pointers, as in
tests/test_perturb_contract_cpu.py: each call is valid in everything but the one pointer (or size) under test, and no call here passes
a fully valid argument set -- nothing is ever launched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = 0x10000            # 16-byte aligned, never dereferenced
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def p(addr):
    return C.c_void_p(addr)


def refused(lib, rc, *words):
    msg = lib.flk_last_error().decode()
    assert rc == EINVAL, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


# ---- the chunking query ----------------------------------------------------------------------------------------------------------
# (B, T, H, per_clip) -> (nchunk, rows per chunk, rows of the last chunk)
CHUNKS = [
    # the cases of tests/test_stem_grad_edges_gpu.py
    ((8, 64, 48, 0), (1, 24, 24)),
    ((8, 90, 52, 0), (2, 13, 13)),
    ((3, 6, 38, 0), (10, 2, 1)),
    ((1, 2, 2, 0), (1, 1, 1)),
    ((1, 2, 4, 0), (2, 1, 1)),
    ((2, 8, 36, 0), (9, 2, 2)),
    ((2, 8, 224, 0), (16, 7, 7)),
    ((3, 8, 36, 1), (9, 2, 2)),
    # the product configurations at H = 224: bs 8 x T 64 (392 K steps in one chunk), the reference's T = 90, bs 1
    ((8, 64, 224, 0), (1, 112, 112)),
    ((8, 90, 224, 0), (2, 56, 56)),
    ((1, 64, 224, 0), (8, 14, 14)),
    # per-clip perturbations take the batch-1 chunking whatever B is
    ((8, 64, 224, 1), (8, 14, 14)),
    ((8, 90, 224, 1), (5, 23, 20)),    # 45 pairs: 5 chunks fill one round of 256 workgroups (225); the last chunk is short
]


@pytest.mark.parametrize("sizes,want", CHUNKS, ids=["x".join(map(str, s)) for s, _ in CHUNKS])
def test_chunking_query(lib, sizes, want):
    from flickering_adversarial_video_amd import ops
    n, rows = ops.stem_delta_grad_chunks(*sizes)
    Ho = sizes[2] // 2
    assert (n, rows, Ho - (n - 1) * rows) == want
    assert 1 <= n <= 16 and (n - 1) * rows < Ho <= n * rows             # no empty chunk, every output row in one
    B, T, H, per_clip = sizes
    if per_clip:                                                         # the invariant the per-clip bitwise tests rest on
        assert (n, rows) == ops.stem_delta_grad_chunks(1, T, H, False) == ops.stem_delta_grad_chunks(1, T, H, True)


def test_chunking_query_refusals(lib):
    n, r = C.c_int(-7), C.c_int(-7)
    refused(lib, lib.flk_stem_delta_grad_chunks(2, 8, 36, 0, None, C.byref(r)), "null output")
    refused(lib, lib.flk_stem_delta_grad_chunks(2, 8, 36, 0, C.byref(n), None), "null output")
    for B, T, H in ((0, 8, 36), (-1, 8, 36), (2, 7, 36), (2, 0, 36), (2, 8, 35), (2, 8, 0), (2, 8, -2)):
        refused(lib, lib.flk_stem_delta_grad_chunks(B, T, H, 0, C.byref(n), C.byref(r)), "T, H must be even")
    assert (n.value, r.value) == (-7, -7)                                # a refusal writes nothing


# ---- the pointer contract --------------------------------------------------------------------------------------------------------
def apply_args(x, u8, per_clip=False):
    from flickering_adversarial_video_amd import _lib
    a = _lib.ApplyArgs()
    a.x, a.x_is_u8, a.x_scale, a.x_bias = x, int(u8), 1.0 / 128.0, -1.0
    a.delta, a.delta_dense, a.dclip, a.delta_per_clip = GOOD, 0, 0.4, int(per_clip)
    a.inv_std = (C.c_float * 3)(1.0, 1.0, 1.0)
    a.lo, a.hi, a.adv_flag = -1.0, 1.0, 1.0
    a.B, a.T, a.H, a.W, a.fold_t = 2, 8, 36, 224, 2
    return a


def grad(lib, a, G=GOOD, g_ld=64, wf=GOOD, gdelta=GOOD, scratch=GOOD, mask_done=0):
    return lib.flk_stem_delta_grad(C.byref(a), p(G), g_ld, p(wf), p(gdelta), p(scratch), mask_done, None)


@pytest.mark.parametrize("per_clip", [False, True], ids=["shared", "per_clip"])
def test_stem_entry_points_refuse_a_misaligned_clip(lib, per_clip):
    for off in (1, 2, 3, 6):           # uint8: read as dwords (the perturbation entry points take 2-byte alignment; these do not)
        a = apply_args(GOOD + off, True, per_clip)
        refused(lib, lib.flk_stem_delta_grad_mask(C.byref(a), p(GOOD), None), "uint8 clip", "4-byte aligned")
        for md in (0, 1):
            refused(lib, grad(lib, a, mask_done=md), "uint8 clip", "4-byte aligned")
    for off in (4, 8, 12, 2):          # fp32: read as float4
        a = apply_args(GOOD + off, False, per_clip)
        refused(lib, lib.flk_stem_delta_grad_mask(C.byref(a), p(GOOD), None), "fp32 clip", "16-byte aligned")
        for md in (0, 1):
            refused(lib, grad(lib, a, mask_done=md), "fp32 clip", "16-byte aligned")


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32in"])
def test_stem_gradient_operands_are_16_byte_aligned(lib, u8):
    a = apply_args(GOOD, u8)
    for off in (2, 4, 8):
        refused(lib, lib.flk_stem_delta_grad_mask(C.byref(a), p(GOOD + off), None), "scratch", "16-byte aligned")
        for md in (0, 1):              # mask_done = 0: refused before the mask pre-pass, not behind it
            for g_ld in (64, 128):
                refused(lib, grad(lib, a, G=GOOD + off, g_ld=g_ld, mask_done=md), "G must be", "16-byte aligned")
            refused(lib, grad(lib, a, wf=GOOD + off, mask_done=md), "wf_dev", "16-byte aligned")
            refused(lib, grad(lib, a, scratch=GOOD + off, mask_done=md), "scratch", "16-byte aligned")
    for off in (1, 2, 3):
        for md in (0, 1):
            refused(lib, grad(lib, a, gdelta=GOOD + off, mask_done=md), "gdelta", "4-byte aligned")


def test_stem_gradient_refuses_everything_before_the_mask_pre_pass(lib):
    """what only the GEMM launch used to refuse -- behind a mask pre-pass already launched -- is refused up front"""
    a = apply_args(GOOD, True)
    for g_ld in (0, 32, 63, 68, 100):
        refused(lib, grad(lib, a, g_ld=g_ld), "bad channel stride")
    for k in range(4):                 # G, wf_dev, gdelta, scratch: one of them null
        ptrs = [None if j == k else GOOD for j in range(4)]
        refused(lib, grad(lib, a, G=ptrs[0], wf=ptrs[1], gdelta=ptrs[2], scratch=ptrs[3]), "null")
    a.B, a.T = 256, 128                # 256 x 64 x 18 x 112 positions of 128 channels: 4.2e9 elements, past the 31-bit offsets
    refused(lib, grad(lib, a, g_ld=128), "tensor too large")


def test_header_states_the_contract():
    hdr = re.sub(r"\s+\*?\s*", " ", open(os.path.join(ROOT, "include", "flicker_hip.h")).read())
    assert "a uint8 clip x is 4-byte aligned and an fp32 clip 16-byte aligned" in hdr
    assert "G, wf_dev and scratch are 16-byte aligned" in hdr
    assert "gdelta is 4-byte aligned" in hdr
    assert "flk_stem_delta_grad_chunks (host only" in hdr
