"""The training transform on the GPU (flk_clip_prepare_train, csrc/prepare.hip: clip_prepare_train_kernel): the kernel against the
reference's own classes and against an exact (float64) restatement, with bounds taken from the reference's own float32 error; the
identity box, the flip, boxes at the borders and degenerate boxes, ragged batches, strided sources; the engine and script wiring.

Bounds (the method of tests/test_clip_prepare_gpu.py; per case and rule, every element compared): with ref32 the float32 reference --
the fixture the reference's own classes wrote (rule "scale_factor"), or the same torch calls with F.interpolate(size=(Hr, Wr)) as the
first resize (rule "sizes") -- and ref64 the float64 restatement (tests/golden/make_prepare_train_golden.py: restate_train_fp64, whose
intermediate image is not rounded), e_ref = max|ref32 - ref64| is the reference's own float32 error and no code under test enters it.
The kernel works in the same precision in another operation order, so it may err as much again: max|gpu - ref64| <= 2 e_ref; by the
triangle inequality max|gpu - ref32| <= 3 e_ref."""
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_prepare_train_golden as gold  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def torch_route(frames, box, flip, rule, Hr, Wr, im_scale=128, S=(112, 112)):
    """the reference's chain in float32 with torch on the CPU, written out here (no package code): /255, the first resize by ``rule``
    (size=(Hr, Wr) or scale_factor), the box, F.interpolate(size=S), flip, (v - mean) / std"""
    import torch.nn.functional as F
    v = torch.from_numpy(np.ascontiguousarray(frames)).float().permute(3, 0, 1, 2) / 255.0
    if rule == "sizes":
        v = F.interpolate(v, size=(Hr, Wr), mode="bilinear", align_corners=False)
    else:
        v = F.interpolate(v, scale_factor=im_scale / min(frames.shape[1:3]), mode="bilinear", align_corners=False)
    assert tuple(v.shape[-2:]) == (Hr, Wr)
    i, j, h, w = box
    v = F.interpolate(v[..., i:i + h, j:j + w], size=S, mode="bilinear", align_corners=False)
    if flip:
        v = v.flip(-1)
    v = v.clone()
    v.sub_(torch.tensor(gold.MEAN)[:, None, None, None]).div_(torch.tensor(gold.STD)[:, None, None, None])
    return v.permute(1, 2, 3, 0).contiguous().numpy()


def noise(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def gpu_train(frames, box, flip, **kw):
    from flickering_adversarial_video_amd import ops
    x = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
    return ops.prepare_clips([x.cuda()], boxes=[box], flips=[flip], **kw)[0]


def check_bounds(rows):
    """rows of (name, rule, frames, box, flip, Hr, Wr[, im_scale, S]): the table of ratios, then the assertion"""
    failures = []
    print()
    print(f"{'case':26s} {'rule':12s} {'box':>20s} {'e_ref':>10s} {'|gpu-ref64|':>12s} {'/e_ref':>7s} {'|gpu-ref32|':>12s} {'/e_ref':>7s}")
    for name, rule, frames, box, flip, Hr, Wr, *rest in rows:
        im_scale, S = rest if rest else (128, (112, 112))
        ref32 = torch_route(frames, box, flip, rule, Hr, Wr, im_scale, S)
        ref64 = gold.restate_train_fp64(frames, box, flip, rule, im_scale, S)
        e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
        gpu = gpu_train(frames, box, flip, rule=rule, im_scale=im_scale, input_size=S).cpu().numpy()
        assert gpu.shape == ref32.shape and gpu.dtype == np.float32 and np.isfinite(gpu).all(), name
        d64 = float(np.abs(gpu.astype(np.float64) - ref64).max())
        d32 = float(np.abs(gpu.astype(np.float64) - ref32.astype(np.float64)).max())
        print(f"{name:26s} {rule:12s} {str(tuple(box)) + ('F' if flip else ' '):>20s} {e_ref:10.3e} {d64:12.3e} {d64 / e_ref:7.2f} {d32:12.3e} {d32 / e_ref:7.2f}")
        if not (e_ref > 0 and d64 <= 2 * e_ref and d32 <= 3 * e_ref):
            failures.append((name, rule, e_ref, d64, d32))
    assert not failures, failures


def test_kernel_against_the_reference_and_the_exact_value():
    need_gpu()
    rows = []
    for c in gold.load_cases():
        # the written-out torch route is the reference: it reproduces the fixture's bytes
        assert np.array_equal(torch_route(c["frames"], c["box"], c["flip"], "scale_factor", c["Hr"], c["Wr"]), c["out"]), c["name"]
        for rule in ("scale_factor", "sizes"):
            rows.append((c["name"], rule, c["frames"], c["box"], c["flip"], c["Hr"], c["Wr"]))
    check_bounds(rows)


def test_identity_box_is_the_evaluation_kernel_bitwise():
    """the evaluation transform's own window with no flip: stage 2 has step 1 and lambda 0, the bits are flk_clip_prepare's"""
    need_gpu()
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    for k, (H, W) in enumerate(((240, 320), (239, 317))):
        x = noise((2, H, W, 3), 40 + k).cuda()
        for rule in vs.RESIZE_RULES:
            _, _, _, _, ci, cj = vs.prepare_geometry(H, W, rule=rule)
            got = ops.prepare_clips([x], rule=rule, boxes=[(ci, cj, 112, 112)], flips=[False])
            assert torch.equal(got, ops.prepare_clips([x], rule=rule)), (H, W, rule)


def test_flip_reverses_w_bitwise():
    need_gpu()
    x = noise((2, 240, 320, 3), 50)
    for box, kw in (((5, 8, 121, 160), {}), ((3, 40, 94, 114), {}), ((10, 20, 100, 90), dict(input_size=(96, 128))), ((0, 0, 128, 170), dict(input_size=(96, 128))),
                    ((8, 29, 112, 112), {}), ((3, 11, 112, 112), {}), ((30, 40, 96, 128), dict(input_size=(96, 128))), ((1, 2, 90, 95), dict(input_size=(90, 95)))):
        a, b = gpu_train(x, box, False, **kw), gpu_train(x, box, True, **kw)
        assert torch.equal(b, a.flip(2)) and not torch.equal(a, b), box


def test_edges_and_degenerate_boxes():
    """boxes touching each border of the resized image, the whole image, h = 1, w = 1 and 1 x 1: finite and within the bounds of the
    exact value"""
    need_gpu()
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    rows = []
    for k, (H, W) in enumerate(((240, 320), (117, 133))):
        x = noise((1, H, W, 3), 60 + k).numpy()
        for rule in vs.RESIZE_RULES:
            Hr, Wr = vs.prepare_geometry(H, W, rule=rule)[:2]
            boxes = {"i=0": (0, 9, 100, 120), "j=0": (7, 0, 100, 120), "i+h=Hr": (Hr - 100, 9, 100, 120), "j+w=Wr": (7, Wr - 120, 100, 120),
                     "whole": (0, 0, Hr, Wr), "h=1 top": (0, 3, 1, 125), "h=1 bottom": (Hr - 1, 3, 1, 125), "w=1 left": (5, 0, 118, 1),
                     "w=1 right": (5, Wr - 1, 118, 1), "1x1": (Hr // 2, Wr // 2, 1, 1), "1x1 corner": (Hr - 1, Wr - 1, 1, 1)}
            for n, (name, box) in enumerate(boxes.items()):
                rows.append((f"{H}x{W} {name}", rule, x, box, bool(n % 2), Hr, Wr))
    # a tall box (step above 2 along H: the per-row pairs of intermediate rows) and a non-square output
    x = noise((1, 480, 270, 3), 63).numpy()
    rows.append(("480x270 h=227->96", "sizes", x, (0, 2, 227, 120), True, 227, 128, 128, (96, 128)))
    rows.append(("480x270 whole->40x40", "sizes", x, (0, 0, 227, 128), False, 227, 128, 128, (40, 40)))
    check_bounds(rows)


def test_ragged_batch_into_a_batch_buffer():
    """one call over clips of three source sizes with different boxes and flips, written at an offset into a larger buffer: the bits of
    per-clip calls, the other rows untouched; a list longer than one launch holds gives the bits of one-by-one calls"""
    need_gpu()
    from flickering_adversarial_video_amd import _lib, ops, videoresnet_spec as vs
    T = 2
    clips = [noise((T, H, W, 3), 10 + k).cuda() for k, (H, W) in enumerate(((240, 320), (480, 270), (117, 133)))]
    boxes, flips = [(5, 8, 121, 160), (49, 6, 156, 119), (0, 0, 128, 145)], [True, False, True]
    single = [ops.prepare_clips([x], boxes=[b], flips=[f])[0].clone() for x, b, f in zip(clips, boxes, flips)]
    buf = torch.full((6, T, 112, 112, 3), -77.0, device="cuda")
    rows = ops.prepare_clips(clips, out=buf, out_offset=2, boxes=boxes, flips=flips)
    assert rows.data_ptr() == buf[2].data_ptr() and rows.shape[0] == 3
    for k in range(3):
        assert torch.equal(buf[2 + k], single[k]), k
    assert bool((buf[:2] == -77.0).all()) and bool((buf[5:] == -77.0).all())
    assert not torch.equal(single[0], ops.prepare_clips([clips[0]])[0])                 # and it is not the evaluation clip
    # longer than the per-launch cap: 2 launches + a ragged tail, every clip its own box and flip
    n = 2 * _lib.FLK_PREP_MAX_CLIPS + 5
    small = [noise((1, 112 + (k % 3) * 16, 128 + (k % 5) * 8, 3), 100 + k).cuda() for k in range(n)]
    rng = random.Random(3)
    params = [vs.train_crop_params(*vs.prepare_geometry(x.shape[1], x.shape[2])[:2], rng=rng) for x in small]
    boxes, flips = [p[:4] for p in params], [p[4] for p in params]
    assert len(set(boxes)) > n // 2 and set(flips) == {False, True}
    one = [ops.prepare_clips([x], boxes=[b], flips=[f])[0].clone() for x, b, f in zip(small, boxes, flips)]
    many = ops.prepare_clips(small, boxes=boxes, flips=flips)
    assert many.shape == (n, 1, 112, 112, 3)
    for k in range(n):
        assert torch.equal(many[k], one[k]), k
    with pytest.raises(ValueError):
        ops.prepare_clips(clips, boxes=boxes[:2], flips=flips[:3])
    with pytest.raises(ValueError):
        ops.prepare_clips(clips[:1], boxes=[(0, 0, 129, 100)], flips=[False])          # outside 128 x 170


def test_strided_source_views():
    """the views of test_clip_prepare_gpu.py::test_strided_source_views -- frames sliced out of a longer video, windows of wider / taller
    frames (row pitch > 3 * Ws, a start that is not 4-byte aligned) -- give the bits of their contiguous copies"""
    need_gpu()
    from flickering_adversarial_video_amd import ops
    video = noise((11, 250, 333, 3), 5).cuda()
    views = [video[1:11:3], video[:4, 3:243, 7:327], video[2:6, :, 1:], video[::5, 5:, :-2]]
    for k, v in enumerate(views):
        assert not v.is_contiguous()
        kw = dict(boxes=[(3 + k, 1 + 2 * k, 110 + k, 120 + 3 * k)], flips=[bool(k % 2)])
        assert torch.equal(ops.prepare_clips([v], **kw), ops.prepare_clips([v.contiguous()], **kw))
    v = video[:2, :, ::2]                        # pixels not adjacent: copied by the wrapper
    kw = dict(boxes=[(0, 0, 128, 80)], flips=[True])
    assert torch.equal(ops.prepare_clips([v], **kw), ops.prepare_clips([v.contiguous()], **kw))
    kw = dict(im_scale=150, input_size=(96, 128), boxes=[(2, 5, 140, 180)], flips=[True])
    a = ops.prepare_clips([views[1]], **kw)
    assert a.shape == (1, 4, 96, 128, 3) and torch.equal(a, ops.prepare_clips([views[1].contiguous()], **kw))


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def test_engine_augment_wiring():
    need_gpu()
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import Adversarial_metrics, FlickerVideoResNet, Losses
    T, B, seed = 8, 2, 5
    raw = noise((B, T, 120, 160, 3), 21).cuda()
    Wt = vs.synthetic_weights("r3d_18", 42)
    eng = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32", augment={"seed": seed})
    x_eval = ops.prepare_clips(raw)
    x_tr = eng.prepare(raw, train=True).clone()
    la = eng.last_augment
    rng = random.Random(seed)
    want = [vs.train_crop_params(128, 170, rng=rng) for _ in range(B)]
    assert la["boxes"] == [w[:4] for w in want] and la["flips"] == [w[4] for w in want]
    assert torch.equal(x_tr, ops.prepare_clips(raw, boxes=la["boxes"], flips=la["flips"])) and not torch.equal(x_tr, x_eval)
    assert torch.equal(eng.prepare(raw), x_eval)                              # the default is still the evaluation clip
    assert torch.equal(eng._prepared(raw), x_eval)
    x_tr2 = eng.prepare(raw, train=True)                                       # the generator moves on
    assert eng.last_augment["boxes"] != la["boxes"] and not torch.equal(x_tr2, x_tr)
    plain = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32")
    with pytest.raises(ValueError):
        plain.prepare(raw, train=True)
    # logits on the device-prepared augmented clip and on the host route's: the fp32 logit tolerance of tests/test_clip_prepare_gpu.py
    xh = torch.stack([vs.prepare_host_train(raw[b].cpu(), la["boxes"][b], la["flips"][b]) for b in range(B)]).cuda()
    e = rel_err(plain.logits(xh).clone(), plain.logits(x_tr).clone())
    print(f"logits, host-prepared vs device-prepared augmented clip: max rel err {e:.3e}")
    assert e < 1e-3
    # train_an_epoch: the train phase augments, the valid phase never does.  lr = 0: the perturbation stays, so the valid metrics of
    # the two engines are equal, while their train losses are taken on different clips
    labels = plain.logits(x_eval).argmax(1).clone()
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=True)
    loaders = {"train": [(raw, labels, None)], "valid": [(raw, labels, None)]}
    res = {}
    for name, aug in (("aug", {"seed": seed}), ("plain", None)):
        e_ = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32", augment=aug)
        res[name] = e_.train_an_epoch(loaders, crit, Adversarial_metrics(targeted=False), lr=0.0)
        if aug:
            assert e_.last_augment["boxes"] == la["boxes"]                  # one batch drawn, by the train phase only
        else:
            assert e_.last_augment is None
        del e_
    assert res["aug"]["valid/loss"] == res["plain"]["valid/loss"] and res["aug"]["valid/fooling_ratio"] == res["plain"]["valid/fooling_ratio"]
    assert res["aug"]["train/loss"] != res["plain"]["train/loss"] and np.isfinite(res["aug"]["train/loss"])
    # augment with train clips at the engine's size: nothing to prepare
    e_ = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32", augment={"seed": 1})
    with pytest.raises(ValueError):
        e_.train_an_epoch({"train": [(x_eval, labels, None)], "valid": []}, crit, Adversarial_metrics(targeted=False), lr=0.0)


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_universal_script_train_transforms(tmp_path):
    need_gpu()
    T, N = 8, 4
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    raw = np.random.default_rng(8).integers(0, 256, (N, T, 120, 160, 3), dtype=np.uint8)
    val = np.ascontiguousarray(raw[:2, :, :, ::-1])
    # labels the victim gives the clean clips: the adversarial loss then depends on the clips (a misclassified clip contributes nothing)
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=2, sample_length=T, dtype="f32")
    labels, vlabels = (np.concatenate([eng.logits(ops.prepare_clips(torch.from_numpy(x[i:i + 2]).cuda()), False).argmax(1).cpu().numpy()
                                       for i in range(0, len(x), 2)]) for x in (raw, val))
    del eng
    np.savez(tmp_path / "train.npz", clips=raw, labels=labels)
    np.savez(tmp_path / "val.npz", clips=val, labels=vlabels)

    def run(tag, prepare, seed):
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_universal_attack.py"), "--train-npz", str(tmp_path / "train.npz"),
               "--val-npz", str(tmp_path / "val.npz"), "--results-root", str(tmp_path / tag), "--base-model", "r3d_18", "--batch-size", "2",
               "--dtype", "f32", "--prepare", prepare, "--train-transforms", "train", "--aug-seed", str(seed), "--epochs", "1"]
        r = _run(cmd)
        assert r.returncode == 0, r.stdout + r.stderr
        files = glob.glob(str(tmp_path / tag / "r3d_18" / "generalization" / "universal" / "val_test" / "all_cls_shuffle_flickering" / "t_4_v_2_*" / "*.npy"))
        assert [os.path.basename(f) for f in files] == ["r3d_18_001.npy"]
        res = np.load(files[0], allow_pickle=True)[-1]
        assert np.isfinite(res["train/loss"]) and res["valid/perturbation"].shape == (3, T, 1, 1)
        return res

    a, b, c = run("dev3", "device", 3), run("dev3again", "device", 3), run("dev4", "device", 4)
    assert a["train/loss"] == b["train/loss"] and a["train/loss"] != c["train/loss"]
    run("host3", "host", 3)
