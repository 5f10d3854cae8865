"""The four classifier-head kernels of csrc/head.hip (head_pool_kernel, head_fc_kernel, head_fc_bwd_kernel, head_pool_bwd_kernel) run
directly through flk_head_forward / flk_head_backward, against the float64 restatement oracle/head_ref.py, at the seams where their
loops and guards change behaviour (the shapes and which seam each reaches: tests/head_cases.py).

What is asserted, and where the bounds come from (nothing here is measured):
  * exact data (small integers, frame weights 2^-(t mod 8)): ZERO tolerance.  tests/test_head_contract_cpu.py proves for every case used
    here that every sum is exact in fp32 in any order, so feat, logits, dfeat and fp32 gy must EQUAL the float64 values, and bf16 gy
    the float64 value rounded to bf16 once (the fp32 product wt * dfeat is exact, so that one rounding is the whole error).
  * standard normal data: the recursive-summation bound, which holds for ANY order of the additions and so does not encode the kernel's,
        feat    |err| <= (npos + 1) * 2^-24 * sum|wt * y|
        logits  |err| <= (C + 2) * 2^-24 * (|bias| + sum|feat * W|)           on the feat the GPU produced
        dfeat   |err| <= (N + 1) * 2^-24 * sum|dlogits * W|
        gy      one fp32 product of the dfeat the GPU produced: relative 2^-24; bf16 adds one round-to-nearest-even, relative 2^-8.
  * channels outside the slice the head was given keep a sentinel bit pattern; NaN outside the input slice reaches nothing.
  * two runs give the same bits, and a row of a batch the bits of that row run alone."""
import functools

import pytest
import torch

import head_cases as hc
from head_cases import BF16, F32
from oracle import head_ref

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
U32, U16 = 2.0 ** -24, 2.0 ** -8            # unit roundoff of fp32 and of bf16 (8 significant bits), round to nearest


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flickering_adversarial_video_amd import ops as o
    return o


def bits(x):
    """bit pattern of a float tensor (tells -0.0 from +0.0 and one NaN from another, unlike ==)"""
    x = x.detach().cpu().contiguous()
    return x.view(torch.int16 if x.dtype == BF16 else torch.int32)


def cuda(d, *names):
    return [None if d[n] is None else d[n].cuda() for n in names]


def equal(got, want64):
    """every element of the GPU tensor IS the float64 value (numbers compared: the sign of a zero is not a number; no NaN expected)"""
    got = got.detach().cpu().double()
    return got.shape == want64.shape and bool((got == want64).all())


def to_bf16_once(x64):
    """float64 values that are exact in fp32, rounded to bf16 once (round to nearest even)"""
    x32 = x64.to(F32)
    assert torch.equal(x32.double(), x64)
    return x32.to(BF16).double()


@functools.lru_cache(maxsize=None)
def exact_small(case):
    """data and float64 reference of a small exact case, computed once and shared by both dtypes (the integers are the same in fp32 and
    bf16 storage) and by the tests that use the case; never modified"""
    d = hc.exact_data(case)
    feat, logits, _, _ = head_ref.head_forward_ref(d["y"], d["wt"], d["W"], d["bias"])
    dfeat, gy, _ = head_ref.head_backward_ref(d["y"], d["wt"], d["W"], d["dlogits"], True)
    return d, {"feat": feat, "logits": logits, "dfeat": dfeat, "gy": gy}


def check_exact(ops, d, ref, dtype):
    y, wt, W, bias, dl = cuda({**d, "y": d["y"].to(dtype)}, "y", "wt", "W", "bias", "dlogits")
    feat, logits = ops.head_forward(y, wt, W, bias)
    assert equal(feat, ref["feat"]), "feat"
    assert equal(logits, ref["logits"]), "logits"
    gy, dfeat = ops.head_backward(y, wt, W, dl)
    assert equal(dfeat, ref["dfeat"]), "dfeat"
    assert gy.dtype == dtype and equal(gy, ref["gy"] if dtype == F32 else to_bf16_once(ref["gy"])), "gy"


def within(got, want64, bound64, what):
    err = (got.detach().cpu().double() - want64).abs()
    assert torch.isfinite(err).all(), what
    over = err > bound64
    assert not over.any(), f"{what}: {int(over.sum())} elements beyond the bound, worst |err| / bound = {float((err / bound64)[over].max()):.3f}"


def check_random(ops, case, dtype, wt=None):
    B, Tn, HW, Cn, N = case
    d = hc.random_data(case, wt)
    ys = d["y"].to(dtype)                                  # what the kernel reads
    y, wt_d, W, bias, dl = cuda({**d, "y": ys}, "y", "wt", "W", "bias", "dlogits")
    feat, logits = ops.head_forward(y, wt_d, W, bias)
    feat_ref, feat_mag = head_ref.pool_ref(ys, d["wt"])
    within(feat, feat_ref, (Tn * HW + 1) * U32 * feat_mag, "feat")
    logits_ref, logits_mag = head_ref.fc_ref(feat.cpu(), d["W"], d["bias"])
    within(logits, logits_ref, (Cn + 2) * U32 * logits_mag, "logits")
    gy, dfeat = ops.head_backward(y, wt_d, W, dl)
    dfeat_ref, dfeat_mag = head_ref.fc_bwd_ref(d["dlogits"], d["W"])
    within(dfeat, dfeat_ref, (N + 1) * U32 * dfeat_mag, "dfeat")
    gy_ref = head_ref.pool_bwd_ref(ys, d["wt"], dfeat.cpu(), True)
    rel = U32 if dtype == F32 else U32 + U16 * (1 + U32)
    within(gy, gy_ref, rel * gy_ref.abs(), "gy")
    assert bool((gy.cpu()[~(ys > 0)] == 0).all())
    return d, ys, logits.cpu().double()


# ---- the loop and guard seams ------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("case", hc.SMALL_CASES, ids=hc.case_id)
def test_exact_data_at_every_seam(ops, case, dtype):
    """pool loop seams (npos around 4, 32 and 64 with frame boundaries inside the unrolled group and the tail), channel guards (partial
    workgroups of all three channel-tiled kernels, the fc loop's 128 + 8, the sf[2048] limit) and class counts (n < N, fewer classes than
    lanes, sd[1024] in four trips): zero tolerance"""
    check_exact(ops, *exact_small(case), dtype)


@DTYPES
@pytest.mark.parametrize("case", hc.SMALL_CASES, ids=hc.case_id)
def test_random_data_at_every_seam(ops, case, dtype):
    check_random(ops, case, dtype)


@DTYPES
def test_no_bias(ops, dtype):
    d, _ = exact_small(hc.BIAS_NONE_CASE)
    y, wt, W = cuda({**d, "y": d["y"].to(dtype)}, "y", "wt", "W")
    feat, logits = ops.head_forward(y, wt, W, None)
    feat_ref, logits_ref, _, _ = head_ref.head_forward_ref(d["y"], d["wt"], d["W"], None)
    assert equal(feat, feat_ref) and equal(logits, logits_ref)
    assert not torch.equal(logits_ref, exact_small(hc.BIAS_NONE_CASE)[1]["logits"])


# ---- channel slices of wider buffers ----------------------------------------------------------------------------------------------------------
def sentinel_filled(shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    bits_view = t.view(torch.int16 if dtype == BF16 else torch.int32)
    bits_view.fill_(-0x4111 if dtype == BF16 else -0x21524111)           # 0xBEEF / 0xDEADBEEF
    return t


@DTYPES
def test_channel_slices_of_wider_buffers(ops, dtype):
    """y is channels [coff, coff + C) of a wider buffer whose other channels are NaN (forward: an odd coff, it has no alignment rule;
    backward: the smallest legal offsets), gy a slice of a wider buffer prefilled with a sentinel: the results are those of the dense
    call and every element outside [gcoff, gcoff + C) keeps its bits"""
    B, Tn, HW, Cn, N = hc.SLICE_CASE
    d, ref = exact_small(hc.SLICE_CASE)
    ys = d["y"].to(dtype)
    wt, W, bias, dl = cuda(d, "wt", "W", "bias", "dlogits")
    wide = torch.full((B, Tn, HW, Cn + 8), float("nan"), dtype=dtype)
    wide[..., 3:3 + Cn] = ys
    feat, logits = ops.head_forward(wide.cuda(), wt, W, bias, C=Cn, coff=3)
    assert equal(feat, ref["feat"]) and equal(logits, ref["logits"])
    e = hc.epl(dtype)
    want = ref["gy"] if dtype == F32 else to_bf16_once(ref["gy"])
    for coff, gcoff, ld, gld in ((e, e, Cn + 2 * e, Cn + 2 * e), (0, e, Cn + e, Cn + e), (e, 0, Cn + e, Cn + e)):
        wide = torch.full((B, Tn, HW, ld), float("nan"), dtype=dtype)
        wide[..., coff:coff + Cn] = ys
        gbuf = sentinel_filled((B, Tn, HW, gld), dtype)
        before = bits(gbuf).clone()
        gy, dfeat = ops.head_backward(wide.cuda(), wt, W, dl, gy=gbuf.cuda(), C=Cn, coff=coff, gcoff=gcoff)
        assert equal(dfeat, ref["dfeat"])
        assert equal(gy[..., gcoff:gcoff + Cn], want)
        after = bits(gy)
        outside = torch.ones(gld, dtype=torch.bool)
        outside[gcoff:gcoff + Cn] = False
        assert outside.sum() == gld - Cn and torch.equal(after[..., outside], before[..., outside])


# ---- the ReLU mask ------------------------------------------------------------------------------------------------------------------------
SPECIALS = ("+0", "-0", "denormal", "negative", "+inf", "nan")
PASSES = {"denormal", "+inf"}


def special_bits(name, dtype):
    b16 = {"+0": 0x0000, "-0": 0x8000, "denormal": 0x0001, "negative": 0xC040, "+inf": 0x7F80, "nan": 0x7FC0}[name]      # 0xC040 = -3.0
    v = b16 if dtype == BF16 or name == "denormal" else b16 << 16        # the smallest positive denormal of EACH format
    width = 16 if dtype == BF16 else 32
    return v - (1 << width) if v >> (width - 1) else v


def plant_specials(ys):
    """every special value in every lane of a 16-byte group, in both batch rows -> [(name, b, pos, c)]"""
    B, Tn, HW, Cn = ys.shape
    e, npos = hc.epl(ys.dtype), Tn * HW
    flat = ys.view(torch.int16 if ys.dtype == BF16 else torch.int32).view(B, npos, Cn)
    where = []
    for b in range(B):
        for i, name in enumerate(SPECIALS):
            for lane in range(e):
                pos, c = (i + lane + b) % npos, ((3 * i + lane) % (Cn // e)) * e + lane
                flat[b, pos, c] = special_bits(name, ys.dtype)
                where.append((name, b, pos, c))
    assert len({w[1:] for w in where}) == len(where)
    return where


@DTYPES
def test_mask_is_y_greater_than_zero(ops, dtype):
    """+0.0, -0.0, a negative and NaN give a zero gradient; the smallest positive denormal of the storage format and +inf pass wt * dfeat
    (the denormal is NOT flushed: the mask is a comparison of the stored number)"""
    B, Tn, HW, Cn, N = hc.MASK_CASE
    d, ref = exact_small(hc.MASK_CASE)
    ys = d["y"].to(dtype).clone()
    where = plant_specials(ys)
    wt, W, dl = cuda(d, "wt", "W", "dlogits")
    gy, dfeat = ops.head_backward(ys.cuda(), wt, W, dl)
    assert equal(dfeat, ref["dfeat"])
    full = head_ref.pool_bwd_ref(ys, d["wt"], ref["dfeat"], False)               # wt[t] * dfeat[b,c] everywhere
    full = full if dtype == F32 else to_bf16_once(full)
    got = gy.cpu().double().view(B, Tn * HW, Cn)
    seen = set()
    for name, b, pos, c in where:
        want = float(full.view(B, Tn * HW, Cn)[b, pos, c]) if name in PASSES else 0.0
        assert float(got[b, pos, c]) == want, (name, b, pos, c, float(got[b, pos, c]), want)
        if want != 0.0:
            seen.add(name)
    assert seen == PASSES                                                        # some passing gradient was not zero anyway
    assert equal(gy, torch.where(ys > 0, full, torch.zeros((), dtype=torch.float64)))


@DTYPES
def test_without_the_mask_y_is_not_read(ops, dtype):
    B, Tn, HW, Cn, N = hc.MASK_CASE
    d, ref = exact_small(hc.MASK_CASE)
    wt, W, dl = cuda(d, "wt", "W", "dlogits")
    full = head_ref.pool_bwd_ref(d["y"], d["wt"], ref["dfeat"], False)
    full = full if dtype == F32 else to_bf16_once(full)
    g_nan, dfeat = ops.head_backward(torch.full(d["y"].shape, float("nan"), dtype=dtype).cuda(), wt, W, dl, use_mask=False)
    g_y, _ = ops.head_backward(d["y"].to(dtype).cuda(), wt, W, dl, use_mask=False)
    assert equal(dfeat, ref["dfeat"]) and equal(g_nan, full) and torch.equal(bits(g_nan), bits(g_y))


# ---- the grid-stride loop of head_pool_bwd_kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,which", [(F32, 0), (F32, 1), (BF16, 0), (BF16, 1)], ids=["f32-at-cap", "f32-past-cap", "bf16-at-cap", "bf16-past-cap"])
def test_pool_backward_grid_stride(ops, dtype, which):
    """exactly 8192 x 256 groups of 16 bytes (every thread one trip) and 2048 groups more (some threads a second trip): every element"""
    case = hc.GRID_CASES[dtype][which]
    d = hc.exact_data(case)
    y, wt, W, bias, dl = cuda({**d, "y": d["y"].to(dtype)}, "y", "wt", "W", "bias", "dlogits")
    feat, logits = ops.head_forward(y, wt, W, bias)
    feat_ref, logits_ref, _, _ = head_ref.head_forward_ref(d["y"], d["wt"], d["W"], d["bias"])
    assert equal(feat, feat_ref) and equal(logits, logits_ref)
    gy, dfeat = ops.head_backward(y, wt, W, dl)
    dfeat_ref, gy_ref, _ = head_ref.head_backward_ref(d["y"], d["wt"], d["W"], d["dlogits"], True)
    assert equal(dfeat, dfeat_ref)
    want = gy_ref.to(F32)                                  # exact (tests/test_head_contract_cpu.py); compared in fp32 to keep the test quick
    want = want if dtype == F32 else want.to(BF16).float()
    got = gy.cpu().float()
    assert got.shape == want.shape and bool((got == want).all())
    assert bool((want != 0).any(dim=-1).view(-1)[-1])      # the last position, reached in the second trip, holds a gradient


# ---- order and batch independence -----------------------------------------------------------------------------------------------------------
@DTYPES
def test_repeatable_and_independent_of_the_batch(ops, dtype):
    """the header comment of csrc/head.hip: a fixed summation order.  Two runs on the same inputs give the same bits in all four outputs,
    and row b of a B = 3 call the bits of a B = 1 call on that row alone"""
    B, Tn, HW, Cn, N = hc.REPEAT_CASE
    d = hc.random_data(hc.REPEAT_CASE)
    y, wt, W, bias, dl = cuda({**d, "y": d["y"].to(dtype)}, "y", "wt", "W", "bias", "dlogits")

    def run(y, dl):
        feat, logits = ops.head_forward(y, wt, W, bias)
        gy, dfeat = ops.head_backward(y, wt, W, dl)
        return [bits(t) for t in (feat, logits, dfeat, gy)]

    first = run(y, dl)
    for a, b in zip(first, run(y, dl)):
        assert torch.equal(a, b)
    for r in range(B):
        for whole, alone in zip(first, run(y[r:r + 1].contiguous(), dl[r:r + 1].contiguous())):
            assert torch.equal(whole[r:r + 1], alone)


# ---- the engines' own heads, small ---------------------------------------------------------------------------------------------------------
def check_engine_head(ops, case, dtype, wt64):
    d, ys, logits = check_random(ops, case, dtype, wt64.to(F32))
    if dtype == F32:
        # tests/test_i3d_gpu.py and tests/test_videoresnet_gpu.py accept 1e-4 of the buffer maximum on the Logits link: the head alone is at
        # least ten times inside it (this records that the link's bar is not what holds the head up; the bounds above are)
        want = head_ref.head_forward_ref(ys, d["wt"], d["W"], d["bias"])[1]
        assert float((logits - want).abs().max()) <= 1e-5 * float(want.abs().max())


@DTYPES
@pytest.mark.parametrize("case", hc.I3D_HEADS, ids=hc.case_id)
def test_i3d_head(ops, case, dtype):
    check_engine_head(ops, case, dtype, head_ref.i3d_time_weights(case[1]))


@DTYPES
@pytest.mark.parametrize("case", hc.VRN_HEADS, ids=hc.case_id)
def test_videoresnet_head(ops, case, dtype):
    check_engine_head(ops, case, dtype, head_ref.videoresnet_time_weights(case[1], case[2]))
