"""Clips cut from whole resident videos on the GPU (flk_clip_prepare_sampled; csrc/prepare.hip, the sampled form of both preparation
kernels): output frame t of clip k is prepared from source frame frame_idx[k][t].

No tolerance anywhere: the sampled form changes addressing only, so every comparison is BITWISE and every one is made against the
existing, unsampled path -- ``ops.prepare_clips`` on the frames gathered beforehand with torch -- never against the sampled path itself.
Tables come from the recorded reference tables (tests/golden/clip_sample_golden.npz) and from hand-made ones (reversed, one frame,
last-frame padding).  Then the engine (``prepare_videos``, ``evaluate_videos``) and the universal script on whole-video files."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_sample_golden as gold  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def noise(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def gathered(video, idx):
    """the frames a table names, gathered with torch: what the unsampled path is given"""
    return video[torch.as_tensor(np.asarray(idx, np.int64), device=video.device)].contiguous()


@pytest.fixture(scope="module")
def videos():
    """three resident videos: lengths 5 / 40 / 17, resolutions 117 x 133 / 250 x 333 / 120 x 160"""
    need_gpu()
    return [noise((5, 117, 133, 3), 1).cuda(), noise((40, 250, 333, 3), 2).cuda(), noise((17, 120, 160, 3), 3).cuda()]


def transforms(H, W):
    """(name, keywords) of the three forms: the evaluation transform, a resampled box with flip, a box of the output size (flipped)"""
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    Hr, Wr, _, _, ci, cj = vs.prepare_geometry(H, W)
    return [("eval", {}), ("box+flip", dict(boxes=[(3, 5, Hr - 9, Wr - 11)], flips=[True])),
            ("direct", dict(boxes=[(min(ci + 2, Hr - 112), max(cj - 1, 0), 112, 112)], flips=[False])),
            ("direct+flip", dict(boxes=[(ci, cj, 112, 112)], flips=[True]))]


def test_identity_table_is_the_existing_launch_bitwise(videos):
    from flickering_adversarial_video_amd import ops
    for v in videos:
        for T_out in (2, len(v)):
            clip = v[:T_out]
            for name, kw in transforms(v.shape[1], v.shape[2]):
                want = ops.prepare_clips([clip], **kw)
                got = ops.prepare_clips([clip], frame_idx=[np.arange(T_out)], **kw)
                assert got.shape == want.shape == (1, T_out, 112, 112, 3)
                assert torch.equal(got, want), (tuple(v.shape), T_out, name)
                got = ops.prepare_clips([v], frame_idx=[np.arange(T_out)], **kw)      # the same frames out of the whole video
                assert torch.equal(got, want), (tuple(v.shape), T_out, name)


def recorded_tables(num_frames, T, jitter=True):
    out = [c["table"] for c in gold.load_cases() if c["num_frames"] == num_frames and c["sample_length"] == T and c["temporal_jitter"] == jitter]
    assert out
    return out


def test_arbitrary_tables_equal_the_gathered_frames_bitwise(videos):
    from flickering_adversarial_video_amd import ops
    tables = {}
    # recorded, jittered (repeated frames, steps of 0 .. 2, tail padding): 8-frame clips of videos of 5 and 17 frames (train split, T + 1 = 17
    # frames: 2 * 8 + 1); 32-frame clips (T_out = 32) of the 40-frame video are hand-made below
    tables[0] = [t[:1][0] for t in recorded_tables(5, 8)][:3]
    tables[2] = [row for t in recorded_tables(17, 8) for row in t][:6]
    assert any((np.diff(r) == 0).any() for r in tables[2]) and any((np.diff(r) == 2).any() for r in tables[2])
    rng = np.random.RandomState(5)
    tables[1] = [np.arange(40)[::-1][:32].copy(),                         # reversed
                 np.full(8, 23),                                          # all one frame
                 np.minimum(np.arange(30, 62), 39),                       # last-frame padding, T_out = 32
                 rng.randint(40, size=32), np.array([39, 0])]             # any order; T_out = 2
    n = 0
    for k, v in enumerate(videos):
        for idx in tables[k]:
            assert idx.min() >= 0 and idx.max() < len(v)
            for name, kw in transforms(v.shape[1], v.shape[2]):
                want = ops.prepare_clips([gathered(v, idx)], **kw)
                got = ops.prepare_clips([v], frame_idx=[idx], **kw)
                assert got.shape == (1, len(idx), 112, 112, 3)
                assert torch.equal(got, want), (k, idx.tolist(), name)
                n += 1
    assert n >= 40
    # a repeated frame is the same frame again, and the table matters
    got = ops.prepare_clips([videos[1]], frame_idx=[[7, 7, 9]])
    assert torch.equal(got[0, 0], got[0, 1]) and not torch.equal(got[0, 1], got[0, 2])


def test_ragged_call_out_offset_and_long_lists(videos):
    from flickering_adversarial_video_amd import _lib, ops, videoresnet_spec as vs
    import random
    order = [1, 0, 1, 2, 2, 1, 0]                        # videos repeated in the list, one entry per clip
    rng = np.random.RandomState(11)
    idx = [np.sort(rng.randint(len(videos[k]), size=8)) for k in order]
    prng = random.Random(4)
    params = [vs.train_crop_params(*vs.prepare_geometry(videos[k].shape[1], videos[k].shape[2])[:2], rng=prng) for k in order]
    boxes, flips = [p[:4] for p in params], [p[4] for p in params]
    for kw in ({}, dict(boxes=boxes, flips=flips)):
        buf = torch.full((len(order) + 5, 8, 112, 112, 3), -77.0, device="cuda")
        rows = ops.prepare_clips([videos[k] for k in order], frame_idx=idx, out=buf, out_offset=3, **kw)
        assert rows.data_ptr() == buf[3].data_ptr() and rows.shape[0] == len(order)
        for j, k in enumerate(order):
            kw1 = dict(boxes=[boxes[j]], flips=[flips[j]]) if kw else {}
            assert torch.equal(buf[3 + j], ops.prepare_clips([gathered(videos[k], idx[j])], **kw1)[0]), (j, bool(kw))
        assert bool((buf[:3] == -77.0).all()) and bool((buf[3 + len(order):] == -77.0).all())
    # longer than the per-launch cap: 2 launches + a ragged tail; T_out = 2, three resolutions and lengths
    n = 2 * _lib.FLK_PREP_MAX_CLIPS + 5
    small = [noise((3 + k % 4, 112 + (k % 3) * 16, 128 + (k % 5) * 8, 3), 100 + k).cuda() for k in range(7)]
    pick = [k % 7 for k in range(n)]
    idx = [rng.randint(len(small[k]), size=2) for k in pick]
    many = ops.prepare_clips([small[k] for k in pick], frame_idx=np.stack(idx))
    assert many.shape == (n, 2, 112, 112, 3)
    for j, k in enumerate(pick):
        assert torch.equal(many[j], ops.prepare_clips([gathered(small[k], idx[j])])[0]), j


def test_strided_source_views():
    """a video sliced in time, windows of wider / taller frames (row pitch > 3 * Ws), a start that is not 4-byte aligned: the table
    indexes the VIEW's frames"""
    need_gpu()
    from flickering_adversarial_video_amd import ops
    video = noise((23, 250, 333, 3), 5).cuda()
    views = [video[1:23:3], video[:9, 3:243, 7:327], video[2:12, :, 1:], video[::5, 5:, :-2]]
    rng = np.random.RandomState(2)
    for k, v in enumerate(views):
        assert not v.is_contiguous()
        idx = rng.randint(len(v), size=8)
        for kw in ({}, dict(boxes=[(3 + k, 1 + 2 * k, 110 + k, 120 + 3 * k)], flips=[bool(k % 2)])):
            assert torch.equal(ops.prepare_clips([v], frame_idx=[idx], **kw), ops.prepare_clips([gathered(v, idx)], **kw)), (k, bool(kw))
    assert views[2].data_ptr() % 4 != 0 or views[2][1].data_ptr() % 4 != 0
    v = video[:6, :, ::2]                        # pixels not adjacent: copied by the wrapper
    assert torch.equal(ops.prepare_clips([v], frame_idx=[[5, 0, 3]]), ops.prepare_clips([gathered(v, [5, 0, 3])]))


def test_refusals(videos):
    from flickering_adversarial_video_amd import _lib, ops
    v = videos[0]                                 # 5 frames
    calls = []
    lib = _lib.load()
    real = lib.flk_clip_prepare_sampled

    class Spy:                                    # nothing reaches the library when the table is refused
        def __getattr__(self, name):
            if name == "flk_clip_prepare_sampled":
                calls.append(name)
            return getattr(lib, name)

    old = ops.load
    ops.load = lambda: Spy()
    try:
        for bad in ([[0, 1, 5]], [[-1, 0, 1]], [[0, 1], [0, 1]], [[0.0, 1.0]], [[]], [[[0, 1]]]):
            with pytest.raises(ValueError):
                ops.prepare_clips([v], frame_idx=bad)
        with pytest.raises(ValueError):
            ops.prepare_clips([v, videos[1]], frame_idx=[[0, 1, 2], [0, 1]])          # ragged
        with pytest.raises(ValueError):
            ops.prepare_clips([v, videos[1]], frame_idx=[[0, 1, 2], [0, 1, 40]])      # 40 is outside the second video
        with pytest.raises(ValueError):
            ops.prepare_clips(v[None], frame_idx=[[0, 1]])                            # not a list of videos
        with pytest.raises(ValueError):
            ops.prepare_clips([v], frame_idx=torch.tensor([[0, 1]]).cuda())           # a device table cannot be checked
        with pytest.raises(ValueError):
            ops.prepare_clips([v], frame_idx=[[0, 1]], out=torch.empty((1, 3, 112, 112, 3), device="cuda"))
        assert not calls
        ops.prepare_clips([v], frame_idx=[[0, 1]])
        assert calls == ["flk_clip_prepare_sampled"]
    finally:
        ops.load = old
    # the C entry: a null table and T_out outside 1..65535 are FLK_EINVAL before any GPU call
    plan, out, _ = ops.prepare_clips_plan([v], frame_idx=[[0, 1]])
    a = plan[0]
    table = a._frame_idx
    assert table.dtype == torch.int32 and table.is_cuda
    assert real(C.byref(a), None, None, 2, _lib.ptr(out), None) == -1 and b"frame_idx" in lib.flk_last_error()
    for bad_T in (0, -3, 65536):
        assert real(C.byref(a), None, _lib.ptr(table), bad_T, _lib.ptr(out), None) == -1 and b"T_out" in lib.flk_last_error()
    a.out_clip_stride = 2 * 112 * 112 * 3 - 1
    assert real(C.byref(a), None, _lib.ptr(table), 2, _lib.ptr(out), None) == -1 and b"out_clip_stride" in lib.flk_last_error()
    a.out_clip_stride = 2 * 112 * 112 * 3
    a.nclip = 0
    assert real(C.byref(a), None, _lib.ptr(table), 2, _lib.ptr(out), None) == -1
    a.nclip = 1
    box = _lib.PrepBox(0, 0, 500, 500, 0)
    assert real(C.byref(a), C.byref(box), _lib.ptr(table), 2, _lib.ptr(out), None) == -1 and b"box" in lib.flk_last_error()


@pytest.fixture(scope="module")
def engine_setup():
    need_gpu()
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    vids = [noise((20, 120, 160, 3), 31).cuda(), noise((9, 117, 133, 3), 32).cuda(), noise((31, 128, 171, 3), 33).cuda()]
    return vids, vs.synthetic_weights("r3d_18", 42)


def test_engine_prepare_videos(engine_setup):
    import random
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    vids, Wt = engine_setup
    T, B, seed = 8, 2, 9
    sampling = {"temporal_jitter": True, "random_shift": True, "seed": seed}
    eng = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32", sampling=sampling, augment={"seed": 4})
    assert eng.last_sampling is None
    # train: the training split's settings, two clips per video, tables from a fresh RandomState(seed) in video order
    x = eng.prepare_videos(vids, train=True, num_samples=2).clone()
    rng = np.random.RandomState(seed)
    want = [vs.sample_frame_indices(len(v), T, 2, 2, True, True, presample_length=T, rng=rng) for v in vids]
    assert len(eng.last_sampling) == 3 and all(np.array_equal(a, b) for a, b in zip(eng.last_sampling, want))
    prng = random.Random(4)
    par = [vs.train_crop_params(*vs.prepare_geometry(v.shape[1], v.shape[2])[:2], rng=prng) for v in vids for _ in range(2)]
    assert eng.last_augment == {"boxes": [p[:4] for p in par], "flips": [p[4] for p in par]}
    assert x.shape == (6, T, 112, 112, 3)
    for k in range(6):                            # video-major, sample-minor; against the unsampled path on the gathered frames
        ref = ops.prepare_clips([gathered(vids[k // 2], want[k // 2][k % 2])], boxes=[par[k][:4]], flips=[par[k][4]])[0]
        assert torch.equal(x[k], ref), k
    # test split: uniform offsets, no draws -- the generator does not move
    state = eng._samp_rng.get_state()[1].copy()
    y = eng.prepare_videos(vids[:2], num_samples=3)
    assert np.array_equal(eng._samp_rng.get_state()[1], state)
    for v, t in zip(vids[:2], eng.last_sampling):
        assert np.array_equal(t, vs.sample_frame_indices(len(v), T, num_samples=3))
    assert torch.equal(y[4], ops.prepare_clips([gathered(vids[1], eng.last_sampling[1][1])])[0])
    # the next training call draws on; an engine without augment samples in time only
    eng.prepare_videos(vids, train=True)
    assert np.array_equal(eng.last_sampling[0], vs.sample_frame_indices(len(vids[0]), T, 2, 1, True, True, presample_length=T, rng=rng))
    for bad in ({"sample_step": 0}, {"jitter": True}, [1], {"seed": -1}, {"random_shift": 1}):
        with pytest.raises(ValueError):
            FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32", sampling=bad)
    with pytest.raises(ValueError):
        eng.prepare_videos(vids[0])


def test_engine_evaluate_videos_and_training_driver(engine_setup):
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import Adversarial_metrics, FlickerVideoResNet, Losses
    vids, Wt = engine_setup
    T, B, S, V = 8, 2, 3, 3
    eng = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32")
    eng.pert_model.init_perturbation((np.random.default_rng(1).random(eng.pert_model.size, dtype=np.float32) * 2 - 1) * 0.1)
    # the clips by the EXISTING path, packed as documented: video-major, sample-minor, batches of B, the last one padded with its last clip
    tables = [vs.sample_frame_indices(len(v), T, num_samples=S) for v in vids]
    clips = [ops.prepare_clips([gathered(vids[k], tables[k][j])])[0].clone() for k in range(V) for j in range(S)]
    assert len(clips) % B == 1                   # 9 clips in batches of 2: the padded batch is part of the test
    want = {False: [], True: []}
    for first in range(0, V * S, B):
        xb = torch.stack([clips[min(first + b, V * S - 1)] for b in range(B)])
        for adv in (False, True):
            want[adv].append(eng.logits(xb, adv)[:min(B, V * S - first)].cpu().numpy().copy())
    want = {k: np.concatenate(v) for k, v in want.items()}
    labels = want[False].reshape(V, S, -1).sum(1).argmax(1)
    labels[1] = (labels[1] + 1) % want[False].shape[1]                  # one video misclassified when clean
    for adv in (False, True):
        r = eng.evaluate_videos(vids, labels, num_samples=S, adversarial=adv)
        assert all(np.array_equal(a, b) for a, b in zip(eng.last_sampling, tables))
        assert r["clip_logits"].dtype == np.float32 and np.array_equal(r["clip_logits"], want[adv])
        vl = np.zeros((V, want[adv].shape[1]), np.float32)
        for j in range(S):
            vl += want[adv][j::S]
        assert r["video_logits"].dtype == np.float32 and np.array_equal(r["video_logits"], vl)
        assert np.array_equal(r["video_preds"], vl.argmax(1)) and np.array_equal(r["clip_preds"], want[adv].argmax(1))
        assert np.array_equal(r["video_trues"], labels) and np.array_equal(r["clip_trues"], np.repeat(labels, S))
        assert r["video_accuracy"] == float((vl.argmax(1) == labels).mean())
        assert r["clip_accuracy"] == float((want[adv].argmax(1) == np.repeat(labels, S)).mean())
        if adv:
            cv = want[False].reshape(V, S, -1)
            cvl = cv[:, 0] + cv[:, 1] + cv[:, 2]
            assert np.array_equal(r["clean_clip_logits"], want[False]) and np.array_equal(r["clean_video_logits"], cvl)
            ok = cvl.argmax(1) == labels
            assert ok.sum() == 2
            assert r["video_fooling_ratio"] == float(((vl.argmax(1) != labels) & ok).sum() / ok.sum())
            assert r["clean_video_accuracy"] == float(ok.mean())
        else:
            assert "video_fooling_ratio" not in r
    assert not np.array_equal(want[False], want[True])
    with pytest.raises(ValueError):
        eng.evaluate_videos(vids, labels[:2])
    # train_an_epoch on lists of whole videos: the train phase samples with the training settings, the valid phase one clip, no shift, no jitter
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=True)
    lab = torch.from_numpy(labels[:2]).cuda()
    loaders = {"train": [(vids[:2], lab, None)], "valid": [([vids[2], vids[0]], lab, None)]}
    e2 = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32", sampling={"temporal_jitter": True, "random_shift": True, "seed": 2})
    res = e2.train_an_epoch(loaders, crit, Adversarial_metrics(targeted=False), lr=0.0)
    assert [t.tolist() for t in e2.last_sampling] == [vs.sample_frame_indices(len(v), T).tolist() for v in (vids[2], vids[0])]
    # the same epoch on clips cut beforehand by the existing path (lr = 0: the perturbation stays)
    rng = np.random.RandomState(2)
    tr = [vs.sample_frame_indices(len(v), T, 2, 1, True, True, presample_length=T, rng=rng)[0] for v in vids[:2]]
    xt = torch.stack([ops.prepare_clips([gathered(v, t)])[0] for v, t in zip(vids[:2], tr)])
    xv = torch.stack([ops.prepare_clips([gathered(v, vs.sample_frame_indices(len(v), T)[0])])[0] for v in (vids[2], vids[0])])
    e3 = FlickerVideoResNet("r3d_18", Wt, batch_size=B, sample_length=T, dtype="f32")
    ref = e3.train_an_epoch({"train": [(xt, lab, None)], "valid": [(xv, lab, None)]}, crit, Adversarial_metrics(targeted=False), lr=0.0)
    assert res["train/loss"] == ref["train/loss"] and res["valid/loss"] == ref["valid/loss"] and np.isfinite(res["train/loss"])


def _script_files(tmp_path):
    """(raw clips [4,T,120,160,3], val clips, labels, val labels, weights): a clips pair of files and the same frames as whole videos of
    exactly T frames; labels the victim gives the clean clips, so that the adversarial loss depends on the clips"""
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    T, N = 8, 4
    raw = np.random.default_rng(8).integers(0, 256, (N, T, 120, 160, 3), dtype=np.uint8)
    val = np.ascontiguousarray(raw[:2, :, :, ::-1])
    Wt = vs.synthetic_weights("r3d_18", 42)
    eng = FlickerVideoResNet("r3d_18", Wt, batch_size=2, sample_length=T, dtype="f32")
    labels, vlabels = (np.concatenate([eng.logits(ops.prepare_clips(torch.from_numpy(x[i:i + 2]).cuda()), False).argmax(1).cpu().numpy()
                                       for i in range(0, len(x), 2)]) for x in (raw, val))
    del eng
    return raw, val, labels, vlabels, Wt


def _run_universal(tmp_path, tag, train, valid, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_universal_attack.py"), "--train-npz", str(tmp_path / train),
           "--val-npz", str(tmp_path / valid), "--results-root", str(tmp_path / tag), "--base-model", "r3d_18", "--batch-size", "2",
           "--dtype", "f32", "--epochs", "1", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    dest = glob.glob(str(tmp_path / tag / "r3d_18" / "generalization" / "universal" / "val_test" / "all_cls_shuffle_flickering" / "t_4_v_2_*"))
    assert len(dest) == 1
    files = glob.glob(os.path.join(dest[0], "*.npy"))
    assert [os.path.basename(f) for f in files] == ["r3d_18_001.npy"]
    return np.load(files[0], allow_pickle=True)[-1], dest[0], r.stdout


def test_universal_script_clips_file_unchanged_and_whole_videos_of_clip_length(tmp_path):
    need_gpu()
    from flickering_adversarial_video_amd.torch_attack import Adversarial_metrics, FlickerVideoResNet, Losses
    raw, val, labels, vlabels, Wt = _script_files(tmp_path)
    T, N = raw.shape[1], len(raw)
    np.savez(tmp_path / "train.npz", clips=raw, labels=labels)
    np.savez(tmp_path / "val.npz", clips=val, labels=vlabels)
    np.savez(tmp_path / "vtrain.npz", labels=labels, **{f"video_{k:05d}": raw[k] for k in range(N)})
    np.savez(tmp_path / "vval.npz", labels=vlabels, **{f"video_{k:05d}": val[k] for k in range(2)})
    # a clips file produces what it produces through the engine's existing path (what the script did before whole videos existed)
    a, dest_a, _ = _run_universal(tmp_path, "clips", "train.npz", "val.npz", "--prepare", "device")
    assert not os.path.exists(os.path.join(dest_a, "video_eval.npz"))
    eng = FlickerVideoResNet("r3d_18", Wt, batch_size=2, sample_length=T, image_size=112, dtype="f32", l_inf_pert_norm=0.1)
    xd, yd, xv, yv = (torch.from_numpy(t).cuda() for t in (raw, labels, val, vlabels))
    loaders = {"train": [(xd[i:i + 2], yd[i:i + 2], None) for i in (0, 2)], "valid": [(xv, yv, None)]}
    ref = eng.fit(loaders, Losses(beta_1=0.5, lambda_=1.0, targeted=False, improve_loss=True, logits=False), Adversarial_metrics(targeted=False),
                  lr=0.001, epochs=1)[-1]
    for key in ("train/loss", "valid/loss", "train/fooling_ratio", "valid/fooling_ratio"):
        assert a[key] == ref[key] or (np.isnan(a[key]) and np.isnan(ref[key])), key
    assert np.array_equal(a["valid/perturbation"], ref["valid/perturbation"])
    # whole videos of exactly T frames, default flags (the reference scripts' settings): every table is the identity -- the clips run, bit for bit
    b, _, _ = _run_universal(tmp_path, "whole", "vtrain.npz", "vval.npz", "--sample-length", str(T))
    assert b["train/loss"] == a["train/loss"] and b["valid/loss"] == a["valid/loss"]
    assert np.array_equal(b["valid/perturbation"], a["valid/perturbation"])


def test_universal_script_random_windows_and_video_evaluation(tmp_path):
    need_gpu()
    T = 8
    rng = np.random.default_rng(9)
    longer = [rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) for n, h, w in ((21, 120, 160), (13, 117, 133), (30, 128, 171), (9, 120, 160))]
    labels, vlabels = np.array([3, 1, 4, 1], np.int64), np.array([5, 9], np.int64)
    np.savez(tmp_path / "ltrain.npz", labels=labels, **{f"video_{k:05d}": longer[k] for k in range(4)})
    np.savez(tmp_path / "lval.npz", labels=vlabels, **{f"video_{k:05d}": longer[k + 1] for k in range(2)})
    c, dest_c, out = _run_universal(tmp_path, "long", "ltrain.npz", "lval.npz", "--random-shift", "--temporal-jitter", "--eval-num-samples", "2",
                                    "--sample-length", str(T), "--sample-seed", "3")
    assert np.isfinite(c["train/loss"]) and c["valid/perturbation"].shape == (3, T, 1, 1)
    ev = np.load(os.path.join(dest_c, "video_eval.npz"))
    assert int(ev["num_samples"]) == 2 and ev["clip_logits"].shape == (4, 400) and ev["video_logits"].shape == (2, 400)
    assert np.array_equal(ev["video_trues"], vlabels) and 0.0 <= float(ev["video_accuracy"]) <= 1.0
    assert np.array_equal(ev["video_preds"], ev["video_logits"].argmax(1))
    assert np.array_equal(ev["video_logits"], ev["clip_logits"][0::2] + ev["clip_logits"][1::2])
    ok = ev["clean_video_preds"] == vlabels
    fr = float(ev["video_fooling_ratio"])
    assert (np.isnan(fr) and not ok.any()) or fr == float(((ev["video_preds"] != vlabels) & ok).sum() / ok.sum())
    assert "video fooling ratio" in out


def test_single_video_statistics_script_on_whole_videos(tmp_path):
    """one clip per video at the uniform offset (the default flags), cut and prepared on the device, then the usual per-video loop"""
    need_gpu()
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet
    T = 8
    rng = np.random.default_rng(10)
    vids = [rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) for n, h, w in ((19, 120, 160), (11, 117, 133))]
    eng = FlickerVideoResNet("r3d_18", vs.synthetic_weights("r3d_18", 42), batch_size=1, sample_length=T, dtype="f32")
    lab = []
    for v in vids:                               # the clip the script will cut, by the existing path
        idx = vs.sample_frame_indices(len(v), T)[0]
        lab.append(int(eng.logits(ops.prepare_clips([torch.from_numpy(v[idx]).cuda()]), False).argmax()))
    del eng
    lab[1] = (lab[1] + 1) % 400                  # second video "misclassified": no attack, None result
    np.savez(tmp_path / "v.npz", labels=np.array(lab), names=np.array(["vidA", "vidB"]), video_00000=vids[0], video_00001=vids[1])
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "r2plus1d_main_statistics_single_video_attack.py"), "--videos-npz", str(tmp_path / "v.npz"),
           "--results-root", str(tmp_path / "res"), "--base-model", "r3d_18", "--dtype", "f32", "--n-iter", "3", "--restart-after", "40",
           "--sample-length", str(T)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "vidA:" in r.stdout and "vidB: clean clip misclassified" in r.stdout
    files = sorted(glob.glob(str(tmp_path / "res" / "r3d_18" / "single_video_attack" / "flickering" / "*" / "*.npy")))
    assert [os.path.basename(f) for f in files] == [f"vidA_@{lab[0]}.npy", f"vidB_@{lab[1]}.npy"]
    ra = np.load(files[0], allow_pickle=True).tolist()
    assert len(ra["loss/total"]) >= 3 and ra["perturbation"][0].shape == (3, T, 1, 1) and ra["prob_clean_input"].shape == (1, 400)
    assert np.load(files[1], allow_pickle=True).tolist() is None
