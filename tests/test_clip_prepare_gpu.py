"""Clip preparation on the GPU (flk_clip_prepare, csrc/prepare.hip): the kernel against the reference's transform and against an exact
(float64) restatement, with bounds taken from the reference's own float32 error; ragged batches, batch-buffer offsets, strided
sources; the engine and script wiring.

Bounds (per case and rule, every element compared): with ref32 the float32 reference -- the fixture the reference's own transform
wrote (rule "scale_factor"), or torch's F.interpolate(size=...) between the /255 and the normalisation (rule "sizes") -- and ref64 the
float64 restatement (tests/golden/make_prepare_golden.py: restate_fp64), e_ref = max|ref32 - ref64| is the reference's own float32
error and no code under test enters it.  The kernel works in the same precision in another operation order, so it may err as much
again: max|gpu - ref64| <= 2 e_ref; by the triangle inequality max|gpu - ref32| <= 3 e_ref."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_prepare_golden as gold  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def sizes_route(frames, Hr, Wr, S=112):
    """rule "sizes" in float32 with torch on the CPU: /255, F.interpolate(size=(Hr, Wr)), centre crop, (v - mean) / std"""
    import torch.nn.functional as F
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    v = F.interpolate(torch.from_numpy(frames).float().permute(3, 0, 1, 2) / 255.0, size=(Hr, Wr), mode="bilinear", align_corners=False)
    i, j = int(round((Hr - S) / 2.0)), int(round((Wr - S) / 2.0))
    v = v[..., i:i + S, j:j + S].clone()
    v.sub_(torch.tensor(vs.DEFAULT_MEAN)[:, None, None, None]).div_(torch.tensor(vs.DEFAULT_STD)[:, None, None, None])
    return v.permute(1, 2, 3, 0).contiguous().numpy()


def noise(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def test_kernel_against_the_reference_and_the_exact_value():
    need_gpu()
    from flickering_adversarial_video_amd import ops
    failures = []
    print()
    print(f"{'case':16s} {'rule':12s} {'e_ref':>10s} {'|gpu-ref64|':>12s} {'/e_ref':>7s} {'|gpu-ref32|':>12s} {'/e_ref':>7s}")
    for c in gold.load_cases():
        for rule in ("scale_factor", "sizes"):
            ref32 = c["out"] if rule == "scale_factor" else sizes_route(c["frames"], c["Hr"], c["Wr"])
            ref64 = gold.restate_fp64(c["frames"], rule)
            e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
            gpu = ops.prepare_clips(torch.from_numpy(c["frames"]).cuda()[None], rule=rule)[0].cpu().numpy()
            assert gpu.shape == ref32.shape and gpu.dtype == np.float32 and np.isfinite(gpu).all()
            d64 = float(np.abs(gpu.astype(np.float64) - ref64).max())
            d32 = float(np.abs(gpu.astype(np.float64) - ref32.astype(np.float64)).max())
            print(f"{c['name']:16s} {rule:12s} {e_ref:10.3e} {d64:12.3e} {d64 / e_ref:7.2f} {d32:12.3e} {d32 / e_ref:7.2f}")
            if not (e_ref > 0 and d64 <= 2 * e_ref and d32 <= 3 * e_ref):
                failures.append((c["name"], rule, e_ref, d64, d32))
    assert not failures, failures


def test_ragged_batch_into_a_batch_buffer():
    """one call over clips of three source sizes, written at an offset into a larger buffer: the bits of per-clip calls, the other rows
    untouched; a list longer than one launch holds gives the same bits"""
    need_gpu()
    from flickering_adversarial_video_amd import _lib, ops
    T = 2
    clips = [noise((T, H, W, 3), 10 + k).cuda() for k, (H, W) in enumerate(((240, 320), (480, 270), (117, 133)))]
    single = [ops.prepare_clips([x])[0].clone() for x in clips]
    buf = torch.full((6, T, 112, 112, 3), -77.0, device="cuda")
    rows = ops.prepare_clips(clips, out=buf, out_offset=2)
    assert rows.data_ptr() == buf[2].data_ptr() and rows.shape[0] == 3
    for k in range(3):
        assert torch.equal(buf[2 + k], single[k]), k
    assert bool((buf[:2] == -77.0).all()) and bool((buf[5:] == -77.0).all())
    # the same through the 5-d tensor form, and a different rule changes the 240 x 320 clip but not its neighbours' rows
    assert torch.equal(ops.prepare_clips(clips[0][None])[0], single[0])
    assert not torch.equal(ops.prepare_clips([clips[0]], rule="scale_factor")[0], single[0])
    # longer than the per-launch cap: 2 launches + a ragged tail
    n = 2 * _lib.FLK_PREP_MAX_CLIPS + 5
    small = [noise((1, 112 + (k % 3) * 16, 128 + (k % 5) * 8, 3), 100 + k).cuda() for k in range(n)]
    one = [ops.prepare_clips([x])[0].clone() for x in small]
    many = ops.prepare_clips(small)
    assert many.shape == (n, 1, 112, 112, 3)
    for k in range(n):
        assert torch.equal(many[k], one[k]), k
    with pytest.raises(ValueError):
        ops.prepare_clips([clips[0], clips[1][:1]])                        # frame counts differ
    with pytest.raises(ValueError):
        ops.prepare_clips(clips, out=buf, out_offset=4)                    # rows 4..6 of a 6-row buffer
    with pytest.raises(ValueError):
        ops.prepare_clips([noise((1, 64, 64, 3), 1).cuda()], im_scale=100)  # resized image smaller than the crop


def test_strided_source_views():
    """frames sliced out of a longer video, and windows of wider / taller frames (row pitch > 3 * Ws, a start that is not 4-byte
    aligned), give the bits of their contiguous copies"""
    need_gpu()
    from flickering_adversarial_video_amd import ops
    video = noise((11, 250, 333, 3), 5).cuda()
    views = [video[1:11:3], video[:4, 3:243, 7:327], video[2:6, :, 1:], video[::5, 5:, :-2]]
    for v in views:
        assert not v.is_contiguous()
        assert torch.equal(ops.prepare_clips([v]), ops.prepare_clips([v.contiguous()]))
    # a view whose pixels are not adjacent (every other column) is copied by the wrapper: same result as its copy
    v = video[:2, :, ::2]
    assert torch.equal(ops.prepare_clips([v]), ops.prepare_clips([v.contiguous()]))
    # non-square output and another crop / scale
    a = ops.prepare_clips([views[1]], im_scale=150, input_size=(96, 128))
    b = ops.prepare_clips([views[1].contiguous()], im_scale=150, input_size=(96, 128))
    assert a.shape == (1, 4, 96, 128, 3) and torch.equal(a, b)


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def test_engine_prepare_wiring():
    need_gpu()
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    T, B = 8, 2
    raw = noise((B, T, 240, 320, 3), 21).cuda()
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=B, sample_length=T, dtype="f32")
    x_eng = eng.prepare(raw).clone()
    x_ops = ops.prepare_clips(raw)
    assert torch.equal(x_eng, x_ops) and x_eng.shape == (B, T, 112, 112, 3)
    la = eng.logits(eng.prepare(raw)).clone()
    lb = eng.logits(x_ops).clone()
    assert torch.equal(la, lb)
    labels = la.argmax(1)
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=True)
    ra = eng.step(eng.prepare(raw), labels, crit, update=False).host()
    rb = eng.step(x_ops, labels, crit, update=False).host()
    assert float(ra["adv_loss"]) == float(rb["adv_loss"]) and np.array_equal(np.asarray(ra["softmax"]), np.asarray(rb["softmax"]))
    # the drivers' path: raw frames are prepared into the engine's reused buffer
    assert torch.equal(eng.logits(eng._prepared(raw)), lb) and eng._prepared(x_ops) is x_ops
    u8_112 = noise((B, T, 112, 112, 3), 3).cuda()
    assert eng._prepared(u8_112) is u8_112                                   # clips at the engine's size: today's path, untouched
    # fed the host route's clip: within the fp32 logit tolerance of tests/test_videoresnet_gpu.py (1e-3 of the largest logit)
    xh = torch.stack([vs.prepare_host(raw[b].cpu()) for b in range(B)]).cuda()
    e = rel_err(eng.logits(xh), lb)
    print(f"logits, host-prepared vs device-prepared clip: max rel err {e:.3e}")
    assert e < 1e-3
    # the other rule is honoured by the engine
    eng2_rule = FlickerVideoResNet.__new__(FlickerVideoResNet)
    eng2_rule.__dict__.update(eng.__dict__)
    eng2_rule.resize_rule = "scale_factor"
    assert torch.equal(eng2_rule.prepare(raw), ops.prepare_clips(raw, rule="scale_factor"))
    with pytest.raises(ValueError):
        eng.prepare(raw[:, :4])                                              # frame count
    with pytest.raises(ValueError):
        FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=1, sample_length=T, dtype="f32", resize_rule="nearest")
    # fit_many_videos on raw frames: one by one and (per-clip engine) two at a time
    vids = [(raw[i:i + 1], labels[i:i + 1], f"v{i}") for i in range(B)]
    eng1 = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=1, sample_length=T, dtype="f32")
    out1 = eng1.fit_many_videos(vids, crit, n_iter=2, restart_after=40, reset_optimizer_per_video=True)
    del eng1
    engb = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=B, sample_length=T, dtype="f32", per_clip=True)
    outb = engb.fit_many_videos(vids, crit, n_iter=2, restart_after=40, reset_optimizer_per_video=True)
    assert set(out1) == set(outb) == {"v0", "v1"}
    for k in out1:
        assert out1[k] is not None and outb[k] is not None and len(out1[k]["loss/total"]) >= 2
        assert out1[k]["loss/total"] == outb[k]["loss/total"]


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_universal_script_on_raw_frames(tmp_path):
    need_gpu()
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    T, N = 8, 4
    raw = np.random.default_rng(8).integers(0, 256, (N, T, 120, 160, 3), dtype=np.uint8)
    val = np.ascontiguousarray(raw[:2, :, :, ::-1])
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=2, sample_length=T, dtype="f32")
    labels, vlabels = (np.concatenate([eng.logits(ops.prepare_clips(torch.from_numpy(x[i:i + 2]).cuda()), False).argmax(1).cpu().numpy()
                                       for i in range(0, len(x), 2)]) for x in (raw, val))
    del eng
    np.savez(tmp_path / "train.npz", clips=raw, labels=labels)
    np.savez(tmp_path / "val.npz", clips=val, labels=vlabels)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_universal_attack.py"), "--train-npz", str(tmp_path / "train.npz"),
           "--val-npz", str(tmp_path / "val.npz"), "--results-root", str(tmp_path / "results"), "--base-model", "r3d_18", "--batch-size", "2",
           "--dtype", "f32", "--prepare", "device", "--epochs", "1"]
    r = _run(cmd)
    assert r.returncode == 0, r.stdout + r.stderr
    dest = glob.glob(str(tmp_path / "results" / "r3d_18" / "generalization" / "universal" / "val_test" / "all_cls_shuffle_flickering" / "t_4_v_2_*"))
    assert len(dest) == 1 and [os.path.basename(f) for f in glob.glob(dest[0] + "/*.npy")] == ["r3d_18_001.npy"]
    res = np.load(os.path.join(dest[0], "r3d_18_001.npy"), allow_pickle=True)
    assert res[-1]["valid/perturbation"].shape == (3, T, 1, 1) and np.isfinite(res[-1]["train/loss"]) and 0.0 <= res[-1]["valid/fooling_ratio"] <= 1.0
    # the host A/B route and the other rule run the same way (fresh results folder: no resume)
    r = _run(cmd[:cmd.index("--results-root") + 1] + [str(tmp_path / "host")] + cmd[cmd.index("--results-root") + 2:-3]
             + ["host", "--resize-rule", "scale_factor", "--epochs", "1"])
    assert r.returncode == 0, r.stdout + r.stderr
    resh = np.load(glob.glob(str(tmp_path / "host" / "r3d_18" / "*" / "*" / "*" / "*" / "*" / "r3d_18_001.npy"))[0], allow_pickle=True)
    assert np.isfinite(resh[-1]["train/loss"])
    # validation clips of another length: the engine's ValueError, as for clips at the engine's size
    np.savez(tmp_path / "val4.npz", clips=raw[:2, :4], labels=labels[:2])
    bad = [str(tmp_path / "val4.npz") if c == str(tmp_path / "val.npz") else c for c in cmd]
    bad[bad.index("--results-root") + 1] = str(tmp_path / "bad")
    r = _run(bad)
    assert r.returncode != 0 and "ValueError" in r.stderr and "frames" in r.stderr


def test_single_video_statistics_script_on_raw_frames(tmp_path):
    need_gpu()
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    T = 8
    raw = np.random.default_rng(9).integers(0, 256, (2, T, 120, 160, 3), dtype=np.uint8)
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=1, sample_length=T, dtype="f32")
    lab = [int(eng.logits(ops.prepare_clips(torch.from_numpy(raw[i:i + 1]).cuda()), False).argmax()) for i in range(2)]
    del eng
    lab[1] = (lab[1] + 1) % 400                                               # second clip "misclassified": no attack, None result
    np.savez(tmp_path / "v.npz", clips=raw, labels=np.array(lab), names=np.array(["clipA", "clipB"]))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_statistics_single_video_attack.py"), "--videos-npz", str(tmp_path / "v.npz"),
           "--results-root", str(tmp_path / "res"), "--base-model", "r3d_18", "--dtype", "f32", "--n-iter", "3", "--restart-after", "40",
           "--prepare", "device"]
    r = _run(cmd)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clipA:" in r.stdout and "clipB: clean clip misclassified" in r.stdout
    files = sorted(glob.glob(str(tmp_path / "res" / "r3d_18" / "single_video_attack" / "flickering" / "*" / "*.npy")))
    assert [os.path.basename(f) for f in files] == [f"clipA_@{lab[0]}.npy", f"clipB_@{lab[1]}.npy"]
    ra = np.load(files[0], allow_pickle=True).tolist()
    assert len(ra["loss/total"]) >= 3 and ra["perturbation"][0].shape == (3, T, 1, 1) and ra["prob_clean_input"].shape == (1, 400)
    assert np.load(files[1], allow_pickle=True).tolist() is None
    # a frame count the model does not take: the script's usual error (R(2+1)D-34 takes 8 or 32 frames, model.py:373)
    np.savez(tmp_path / "v4.npz", clips=raw[:, :4], labels=np.array(lab))
    r = _run(cmd[:3] + [str(tmp_path / "v4.npz")] + cmd[4:] + ["--base-model", "kinetics"])
    assert r.returncode != 0 and "ValueError" in r.stderr and "sample_length" in r.stderr
