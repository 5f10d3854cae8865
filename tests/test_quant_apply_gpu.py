"""The quantised apply on the GPU (flk_apply_args.q_lut, the QUANT instantiations of the four apply kernels): what it writes is BITWISE the
clean apply of the bytes flk_adv_export_u8 writes for the same arguments, on every kernel route; it quantises (a sub-level perturbation
moves nothing, whole levels move whole bytes); the gradient is the straight-through mask the gradient kernels already compute; an engine
built with quantise_train steps on the logits of the stored video; the single-video script's --quantise-train."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def clip_u8(B, T, H, W, seed):
    """random bytes with rows of 0 and of 255 planted and every byte value present: the clamp bounds are hit"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    u8 = vs.synthetic_clip_u8(B, T, H, W, seed=seed)
    u8[:, :, :2] = 0
    u8[:, :, 2:4] = 255
    free = u8[:, :, 4:].reshape(-1)                  # (a copy: the rows below the planted ones)
    free[:256] = np.arange(256, dtype=np.uint8)
    u8[:, :, 4:] = free.reshape(u8[:, :, 4:].shape)
    assert len(np.unique(u8)) == 256
    return u8


def torch_kw():
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    lo = float(np.max((0.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    hi = float(np.min((1.0 - np.array(vs.DEFAULT_MEAN)) / vs.DEFAULT_STD))
    return dict(dialect="torch", dclip=0.2, inv_std=tuple(1.0 / s for s in vs.DEFAULT_STD), lo=lo, hi=hi)


TF_KW = dict(dialect="tf", dclip=0.4, inv_std=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0)


def unfold(f, fold_t):
    """the apply kernel's fp32 space-to-depth output back to [B,T,H,W,3] (data movement only)"""
    if fold_t == 1:
        B, T, H2, W2 = f.shape[:4]
        return f[..., :12].reshape(B, T, H2, W2, 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, T, 2 * H2, 2 * W2, 3).contiguous()
    B, T2, H2, W2 = f.shape[:4]
    if fold_t == 3:             # channel (qt*2+qh)*8 + qw*3 + c
        f = f.reshape(B, T2, H2, W2, 2, 2, 8)[..., :6]
    else:                       # channel (qt*4+qh*2+qw)*3 + c
        f = f[..., :24]
    return f.reshape(B, T2, H2, W2, 2, 2, 2, 3).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, 2 * T2, 2 * H2, 2 * W2, 3).contiguous()


def offset_u8(u8, nbytes=4):
    """the clip on the device at a pointer `nbytes` past an allocation's start (allocations are at least 256-byte aligned)"""
    buf = torch.empty(u8.size + nbytes, dtype=torch.uint8, device="cuda")
    x = buf[nbytes:].view(u8.shape)
    x.copy_(torch.from_numpy(u8))
    assert x.is_contiguous() and x.data_ptr() % 8 == nbytes % 8
    return x


def source(kind, u8, offset=0):
    """(device clip, host clip, keywords, host decode table): 'fp32' and 'u8_lut' in the torch dialect, 'u8_tf' in the TF dialect"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import decode_table
    xu = offset_u8(u8, offset) if offset else torch.from_numpy(u8).cuda()
    if kind == "fp32":
        xf = vs.normalize_u8(u8)
        return torch.from_numpy(xf).cuda(), xf, torch_kw(), None
    if kind == "u8_lut":
        return xu, u8, dict(torch_kw(), x_lut=decode_table("cuda")), vs.u8_decode_table()
    return xu, u8, dict(TF_KW), None


def delta(kind, B, T, H, W, seed, amp=0.2):
    """(host delta, device keywords, host keywords): amplitudes up to +-amp -- tens of levels, beyond both clamp bounds on the planted rows"""
    rng = np.random.default_rng(seed)
    if kind == "shared":
        return rng.uniform(-amp, amp, (T, 3)).astype(np.float32), {}, {}
    if kind == "rolled":
        return rng.uniform(-amp, amp, (T, 3)).astype(np.float32), dict(shift_x=1, shift_p=3), dict(shift_x=1, shift_p=3)
    if kind == "per_clip":
        bounds = np.linspace(0.12, 0.2, B).astype(np.float32)
        return rng.uniform(-amp, amp, (B, T, 3)).astype(np.float32), dict(dclip_dev=torch.from_numpy(bounds).cuda()), dict(dclip_clip=bounds)
    assert kind == "dense"
    return rng.uniform(-amp, amp, (T, H, W, 3)).astype(np.float32), {}, {}


def clean_apply_of_bytes(frames, kw, fold_t, dtype):
    """the EXISTING clean apply (adv_flag = 0, q_lut = NULL) of stored frames, decoded as the dialect decodes uint8 clips and with the
    clamp bounds of a clean forward: none in the torch dialect (Perturbation.apply_args(adversarial=False)), [-1, 1] in the TF dialect
    (which no byte leaves).  (The rolls are in the frames already.)"""
    from flickering_adversarial_video_amd import ops
    kw = {k: v for k, v in kw.items() if k != "x_lut"}
    if kw["dialect"] == "torch":
        kw.update(lo=-float("inf"), hi=float("inf"))
    lut = dict(x_lut=ops.quant_table("torch", "cuda")) if kw["dialect"] == "torch" else {}
    zeros = torch.zeros((frames.shape[1], 3), dtype=F32, device="cuda")             # adv_flag = 0: no perturbation is read
    return ops.perturb_apply_s2d(ops.make_apply_args(frames.contiguous(), zeros, fold_t=fold_t, adv_flag=0.0, **kw, **lut), dtype)


# (id, shape, source, pointer offset, delta, fold_t, output dtypes): one case per kernel route, at the smallest shapes that reach it
ROUTES = [
    ("generic_fp32_src", (2, 4, 6, 10), "fp32", 0, "shared", 1, (F32, BF16)),
    ("generic_u8_lut", (2, 4, 6, 10), "u8_lut", 0, "shared", 1, (F32, BF16)),
    ("generic_tf_fold2", (1, 4, 8, 10), "u8_tf", 0, "shared", 2, (F32, BF16)),
    ("generic_tf_fold3", (1, 4, 8, 10), "u8_tf", 0, "shared", 3, (F32, BF16)),
    ("hilo_fp32_src", (2, 4, 6, 10), "fp32", 0, "shared", 4, (BF16,)),
    ("hilo_u8_narrow", (2, 4, 6, 10), "u8_lut", 0, "shared", 4, (BF16,)),               # W % 8 != 0: no fast path
    ("hilo_u8_offset4", (2, 4, 6, 16), "u8_lut", 4, "shared", 4, (BF16,)),              # W % 8 == 0, but the pointer refuses the fast path
    ("hilo_u8_fast", (2, 4, 6, 16), "u8_lut", 0, "shared", 4, (BF16,)),
    ("hilo_u8_fast_two_workgroups", (2, 4, 64, 112), "u8_lut", 0, "shared", 4, (BF16,)),  # 32 x 14 = 448 threads per frame
    ("hilo_u8_fast_dense", (1, 4, 6, 16), "u8_lut", 0, "dense", 4, (BF16,)),
    ("u8_flicker_fold2", (1, 4, 8, 16), "u8_tf", 0, "shared", 2, (F32, BF16)),
    ("u8_flicker_fold3", (1, 4, 8, 16), "u8_tf", 0, "shared", 3, (F32, BF16)),
    ("hilo_u8_fast_per_clip", (2, 4, 6, 16), "u8_lut", 0, "per_clip", 4, (BF16,)),
    ("hilo_u8_fast_rolled", (2, 4, 6, 16), "u8_lut", 0, "rolled", 4, (BF16,)),
    ("generic_u8_lut_per_clip", (2, 4, 6, 16), "u8_lut", 0, "per_clip", 1, (F32,)),      # the same variants where the host route can follow
    ("generic_u8_lut_rolled", (2, 4, 6, 16), "u8_lut", 0, "rolled", 1, (F32,)),
]


@pytest.mark.parametrize("shape,src,offset,dkind,fold_t,dtypes", [r[1:] for r in ROUTES], ids=[r[0] for r in ROUTES])
def test_quantised_apply_is_the_clean_apply_of_the_exported_bytes(shape, src, offset, dkind, fold_t, dtypes):
    from flickering_adversarial_video_amd import ops
    B, T, H, W = shape
    u8 = clip_u8(B, T, H, W, seed=41)
    xd, xh, kw, lut = source(src, u8, offset)
    d, dev_kw, host_kw = delta(dkind, B, T, H, W, seed=43)
    dd = torch.from_numpy(d).cuda()
    dialect = kw["dialect"]
    plain = ops.make_apply_args(xd, dd, fold_t=fold_t, adv_flag=1.0, **kw, **dev_kw)
    quant = ops.make_apply_args(xd, dd, fold_t=fold_t, adv_flag=1.0, quantise=dialect, **kw, **dev_kw)
    frames = ops.export_adversarial_u8(plain, dialect)
    assert int(frames.min()) == 0 and int(frames.max()) == 255                 # both clamp bounds / saturation ends are reached
    for dtype in dtypes:
        got = ops.perturb_apply_s2d(quant, dtype)
        want = clean_apply_of_bytes(frames, kw, fold_t, dtype)
        assert got.dtype == dtype and same_bits(got, want), (shape, src, dkind, fold_t, dtype)
        assert not same_bits(got, ops.perturb_apply_s2d(plain, dtype))         # the option does something
        if dtype == F32:
            host_extra = {k: v for k, v in kw.items() if k != "x_lut"}
            host = ops.perturb_apply_quantised_host(xh, d, adv_flag=1.0, x_lut=lut, **host_extra, **host_kw)
            assert same_bits(unfold(got, fold_t), host), (shape, src, dkind, fold_t)


@pytest.mark.parametrize("fold_t,dtype", [(1, F32), (4, BF16)], ids=["generic_fp32", "hilo_u8"])
def test_a_sub_level_perturbation_moves_nothing_torch(fold_t, dtype):
    """|delta| = 1e-4 (0.0255 levels) on a uint8 clip: the quantised output is bitwise the clean apply, the unquantised one is not.  Torch
    dialect: on values inside [lo, hi] -- bytes 10..233 in every channel; outside, the attack's clamp moves the value to a bound with any
    delta, and it is stored as the level nearest the bound (a bound is a byte value of one channel only), which the route test above pins
    on every byte."""
    from flickering_adversarial_video_amd import ops
    from flickering_adversarial_video_amd.torch_attack import decode_table
    B, T, H, W = 2, 4, 6, 16
    u8 = np.random.default_rng(47).integers(10, 234, (B, T, H, W, 3)).astype(np.uint8)
    xu = torch.from_numpy(u8).cuda()
    dd = torch.from_numpy((1e-4 * np.where(np.random.default_rng(53).random((T, 3)) < 0.5, -1.0, 1.0)).astype(np.float32)).cuda()
    kw = dict(torch_kw(), x_lut=decode_table("cuda"))
    clean = ops.perturb_apply_s2d(ops.make_apply_args(xu, dd, fold_t=fold_t, adv_flag=0.0, **kw), dtype)
    got = ops.perturb_apply_s2d(ops.make_apply_args(xu, dd, fold_t=fold_t, adv_flag=1.0, quantise="torch", **kw), dtype)
    plain = ops.perturb_apply_s2d(ops.make_apply_args(xu, dd, fold_t=fold_t, adv_flag=1.0, **kw), dtype)
    assert same_bits(got, clean) and not same_bits(plain, clean)


@pytest.mark.parametrize("W,fold_t", [(16, 2), (10, 3)], ids=["u8_flicker_fold2", "generic_fold3"])
def test_a_sub_level_perturbation_moves_nothing_tf(W, fold_t):
    """the TF dialect's clamp bounds are byte values (-1 is byte 0, byte 255 lies below +1): every byte 0..255 comes back"""
    from flickering_adversarial_video_amd import ops
    B, T, H = 1, 4, 8
    xu = torch.from_numpy(clip_u8(B, T, H, W, seed=59)).cuda()
    dd = torch.from_numpy((1e-4 * np.where(np.random.default_rng(61).random((T, 3)) < 0.5, -1.0, 1.0)).astype(np.float32)).cuda()
    clean = ops.perturb_apply_s2d(ops.make_apply_args(xu, dd, fold_t=fold_t, adv_flag=0.0, **TF_KW), F32)
    got = ops.perturb_apply_s2d(ops.make_apply_args(xu, dd, fold_t=fold_t, adv_flag=1.0, quantise="tf", **TF_KW), F32)
    plain = ops.perturb_apply_s2d(ops.make_apply_args(xu, dd, fold_t=fold_t, adv_flag=1.0, **TF_KW), F32)
    assert same_bits(got, clean) and not same_bits(plain, clean)


@pytest.mark.parametrize("fold_t,dtype", [(1, F32), (4, BF16)], ids=["generic_fp32", "hilo_u8"])
def test_whole_levels_move_whole_bytes(fold_t, dtype):
    """delta = k / 255 on bytes 30..200, every k in -20..20 (one per (clip, frame, channel)): exactly the clean apply of byte + k"""
    from flickering_adversarial_video_amd import ops
    from flickering_adversarial_video_amd.torch_attack import decode_table
    B, T, H, W = 2, 8, 6, 16
    rng = np.random.default_rng(67)
    u8 = rng.integers(30, 201, (B, T, H, W, 3)).astype(np.uint8)
    k = rng.permutation(np.concatenate([np.arange(-20, 21), rng.integers(-20, 21, B * T * 3 - 41)])).reshape(B, T, 3)
    moved = (u8.astype(np.int64) + k[:, :, None, None, :]).astype(np.uint8)
    dd = torch.from_numpy((k / 255.0).astype(np.float32)).cuda()
    kw = dict(torch_kw(), x_lut=decode_table("cuda"))
    got = ops.perturb_apply_s2d(ops.make_apply_args(torch.from_numpy(u8).cuda(), dd, fold_t=fold_t, adv_flag=1.0, quantise="torch", **kw), dtype)
    want = ops.perturb_apply_s2d(ops.make_apply_args(torch.from_numpy(moved).cuda(), dd, fold_t=fold_t, adv_flag=0.0, **kw), dtype)
    assert same_bits(got, want)


@pytest.mark.parametrize("dkind", ["shared", "per_clip", "dense"])
def test_gradient_is_the_straight_through_mask(dkind):
    """perturb_grad_reduce does not read the quantiser's fields: with them it returns the bits it returns without"""
    from flickering_adversarial_video_amd import ops
    B, T, H, W = 2, 4, 6, 16
    xd, _, kw, _ = source("u8_lut", clip_u8(B, T, H, W, seed=71))
    d, dev_kw, _ = delta(dkind, B, T, H, W, seed=73)
    dd = torch.from_numpy(d).cuda()
    gx = torch.from_numpy(np.random.default_rng(79).standard_normal((B, T, H // 2, W // 2, 16)).astype(np.float32)).cuda()
    plain = ops.perturb_grad_reduce(ops.make_apply_args(xd, dd, fold_t=1, adv_flag=1.0, **kw, **dev_kw), gx)
    quant = ops.perturb_grad_reduce(ops.make_apply_args(xd, dd, fold_t=1, adv_flag=1.0, quantise="torch", **kw, **dev_kw), gx)
    assert tuple(quant.shape) == tuple(d.shape) and same_bits(quant, plain) and float(plain.abs().max()) > 0


# ---- engines ---------------------------------------------------------------------------------------------------------------------
def engine(**kw):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    kw = dict(dict(batch_size=2, sample_length=8, image_size=64, dtype="bf16", l_inf_pert_norm=0.2, quantise_train=True), **kw)
    return FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), **kw)


@pytest.fixture(scope="module")
def vrn_bf16():
    return engine()


@pytest.fixture(scope="module")
def vrn_f32():
    return engine(batch_size=1, dtype="f32")


def set_delta(eng, seed, amp=0.05):
    p = eng.pert_model.perturbation
    p.copy_(torch.from_numpy(np.random.default_rng(seed).uniform(-amp, amp, tuple(p.shape)).astype(np.float32)))


def criterion(attack_type="flickering"):
    from flickering_adversarial_video_amd.torch_attack import Losses
    return Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True, attack_type=attack_type)


def clips(eng, seed):
    """the engine's batch as uint8 frames and as the fp32 clip they normalise to"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    u8 = clip_u8(eng.B, eng.T, eng.H, eng.W, seed=seed)
    return torch.from_numpy(u8).cuda(), torch.from_numpy(vs.normalize_u8(u8)).cuda()


@pytest.mark.parametrize("which", ["bf16_batch2", "f32_batch1"])
def test_engine_steps_on_the_logits_of_the_stored_video(which, vrn_bf16, vrn_f32):
    eng = vrn_bf16 if which == "bf16_batch2" else vrn_f32
    crit = criterion()
    for x in clips(eng, seed=83):
        lab = eng.logits(x, False).argmax(1).clone()
        set_delta(eng, 89)
        eng.step(x, lab, crit, update=False)
        stepped = eng._logits.clone()
        assert same_bits(stepped, eng.quantised_logits(x))
        # the test can fail: without the option the same delta gives other logits than the stored video's
        eng.quantise_train = False
        try:
            eng.step(x, lab, crit, update=False)
            assert not same_bits(eng._logits.clone(), eng.quantised_logits(x))
        finally:
            eng.quantise_train = True
        for _ in range(5):
            res = eng.step(x, lab, crit, lr=1e-2, update=True)
            during = eng._logits.clone()
        # the verdict of the last step is the stored video's for the delta that step ran with; the updated delta follows the same rule
        assert torch.equal(res["argmax"].reshape(-1), during.argmax(1))
        after = eng.logits(x, True).clone()
        assert same_bits(after, eng.quantised_logits(x)) and not same_bits(after, during)


@pytest.mark.parametrize("kw,attack_type", [(dict(per_clip=True), "flickering"), (dict(attack_type="L12"), "L12")], ids=["per_clip", "L12"])
def test_per_clip_and_dense_engines_step_on_the_stored_video(kw, attack_type):
    eng = engine(**kw)
    xu, _ = clips(eng, seed=97)
    lab = eng.logits(xu, False).argmax(1).clone()
    set_delta(eng, 101)
    eng.step(xu, lab, criterion(attack_type), lr=1e-2, update=True)
    stepped = eng._logits.clone()
    set_delta(eng, 101)                                  # the delta the step ran with
    assert same_bits(stepped, eng.quantised_logits(xu))
    eng.quantise_train = False
    assert not same_bits(eng.logits(xu, True).clone(), eng.quantised_logits(xu))


# ---- script ----------------------------------------------------------------------------------------------------------------------
def test_single_video_script_trains_on_the_stored_video(tmp_path, vrn_f32):
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    T, HW = 8, 64
    u8 = vs.synthetic_clip_u8(2, T, HW, HW, seed=67)
    lab = [int(vrn_f32.logits(torch.from_numpy(u8[i:i + 1]).cuda(), False).argmax()) for i in range(2)]
    np.savez(tmp_path / "v.npz", clips=u8, labels=np.array(lab), names=np.array(["a", "b"]))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_statistics_single_video_attack.py"), "--videos-npz", str(tmp_path / "v.npz"),
           "--base-model", "r3d_18", "--dtype", "f32", "--n-iter", "3", "--restart-after", "40", "--results-root", str(tmp_path / "q"),
           "--quantise-train", "--save-adversarial-u8"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(glob.glob(str(tmp_path / "q" / "**" / "*.npy"), recursive=True))
    assert len(files) == 2
    for f in files:
        res = np.load(f, allow_pickle=True).tolist()
        frames = torch.from_numpy(res["adv_video_u8"]).cuda()
        assert frames.dtype == torch.uint8 and tuple(frames.shape) == (1, T, HW, HW, 3)
        assert np.array_equal(res["quantised_pred"], vrn_f32.logits(frames, False).argmax(1).cpu().numpy())
