#!/usr/bin/env python3
"""Timing of the device clip preparation (flk_clip_prepare and flk_clip_prepare_train, csrc/prepare.hip) against the host route.

1. one flk_clip_prepare call (one launch) for 16 clips of 16 x 240 x 320 and for 8 clips of 32 x 256 x 340: the arguments are built
   once (ops.prepare_clips_plan), a HIP-event pair brackets 10 back-to-back calls (one call is shorter than the host takes to issue
   it; the figure is the tenth), median / min / max over N such groups after a warm-up; the source bytes under the crop window plus
   the bytes written, and the GB/s they give at the median.  `wrapper` is ops.prepare_clips itself, one call per event pair: what a
   caller that builds the descriptors every time sees.  (The window's bytes are counted once: the two source rows of neighbouring
   output rows overlap and are re-read from cache.)
   `train`: one flk_clip_prepare_train call for the same clips, boxes and flips from the default sampler
   (videoresnet_spec.train_crop_params under random.Random(0)), timed the same way in the same run, groups alternating with the
   evaluation launch's; the source bytes under the boxes plus the bytes written; its ratio to the evaluation launch.  `train_crop_only`:
   the same with boxes of the output size (RandomCropVideo), which skip the second resampling.
2. the host route (videoresnet_spec.prepare_host, torch on the CPU) for the same clips in the same run, wall clock.
3. the mc3_18 batch-16 attack step (bf16, 16 frames) with every batch prepared from a resident raw shard -- by the evaluation transform
   (`raw`) and by the training transform with fresh draws every step (`raw_train`) -- against the same step on already-prepared fp32
   clips, the legs alternating step by step.  The last leg uses nothing this tool's subject added.  `videos`: every batch cut from 16
   resident whole videos of 300 x 240 x 320 with fresh tables (jitter and shift, the training split) and prepared in the same launch
   (engine.prepare_videos).
4. `sampled`: 16 clips of 16 frames cut from 16 resident videos of 300 x 240 x 320 through a frame-index table (flk_clip_prepare_sampled;
   tables of the training split with jitter and shift under RandomState(0)): ONE sampled launch against torch.index_select of every
   clip's frames into a [16,16,240,320,3] buffer followed by the existing launch on it, and against that existing launch alone, for
   both transforms, groups of 10 alternating inside one run; the sampled launch as bytes/s of its compulsory traffic (the bytes under
   the window or box of every DISTINCT frame a clip names, plus the bytes written).
5. `--parent-lib PATH` (a libflicker_hip.so built from the parent commit): flk_clip_prepare and flk_clip_prepare_train, unsampled, from this
   library and from that one on the same arguments, alternating; the parent is timed in two interleaved series, whose difference is the
   run-to-run spread of the parent against itself.

    python tools/prepare_time.py [--launches 30] [--steps 20] [--host-reps 3] [--skip-step] [--parent-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms, unit):
    k = 1e3 if unit == "us" else 1.0
    return {f"median_{unit}": round(statistics.median(ms) * k, 3), f"min_{unit}": round(min(ms) * k, 3), f"max_{unit}": round(max(ms) * k, 3), "n": len(ms)}


def window_bytes(T, Hs, Ws, S=112):
    """source bytes under the crop window of one clip: (rows h0(first) .. h1(last)) x (columns i0(first) .. i1(last)) x 3"""
    _, _, sh, sw, ci, cj = vs.prepare_geometry(Hs, Ws, 128, S)

    def span(step, c, n):
        lo = int(max(np.float32(step) * np.float32(c + 0.5) - np.float32(0.5), 0))
        hi = min(int(max(np.float32(step) * np.float32(c + S - 1 + 0.5) - np.float32(0.5), 0)) + 1, n - 1)
        return hi - lo + 1
    return T * span(sh, ci, Hs) * span(sw, cj, Ws) * 3


def box_bytes(T, Hs, Ws, box):
    """source bytes under one clip's box: the rows and columns the first resampling reads for resized rows i .. i + h - 1, columns j .. j + w - 1"""
    _, _, sh, sw, _, _ = vs.prepare_geometry(Hs, Ws, 128, 112)

    def span(step, c, m, n):
        lo = int(max(np.float32(step) * np.float32(c + 0.5) - np.float32(0.5), 0))
        hi = min(int(max(np.float32(step) * np.float32(c + m - 1 + 0.5) - np.float32(0.5), 0)) + 1, n - 1)
        return hi - lo + 1
    i, j, h, w = box
    return T * span(sh, i, h, Hs) * span(sw, j, w, Ws) * 3


def sampled_case(a, out, videos):
    """section 4 of the module docstring"""
    from flickering_adversarial_video_amd import _lib
    N, T, (H, W) = len(videos), 16, videos[0].shape[1:3]
    srng = np.random.RandomState(0)
    kw = vs.split_sampling({"temporal_jitter": True, "random_shift": True}, T, train=True)
    table = np.concatenate([vs.sample_frame_indices(len(v), rng=srng, **kw) for v in videos])
    idx_dev = [torch.from_numpy(r).cuda() for r in table]
    gbuf = torch.empty((N, T, H, W, 3), dtype=torch.uint8, device="cuda")
    buf = torch.empty((N, T, 112, 112, 3), dtype=torch.float32, device="cuda")
    Hr, Wr = vs.prepare_geometry(H, W, 128, 112)[:2]
    prng = random.Random(0)
    params = [vs.train_crop_params(Hr, Wr, rng=prng) for _ in range(N)]
    lib, outp, st = ops.load(), ops.ptr(buf), ops.stream_ptr()
    res = {"table_first_rows": table[:2].tolist(), "distinct_frames": int(sum(len(set(r.tolist())) for r in table))}
    for leg, bk in (("eval", {}), ("train", dict(boxes=[q[:4] for q in params], flips=[q[4] for q in params]))):
        splan, _, _ = ops.prepare_clips_plan(videos, out=buf, frame_idx=table, **bk)
        gplan, _, _ = ops.prepare_clips_plan(gbuf, out=buf, **bk)
        assert len(splan) == 1 and len(gplan) == 1
        sp, gp = splan[0], gplan[0]

        def existing():
            if gp._boxes is None:
                ops.check(lib.flk_clip_prepare(C.byref(gp), outp, st))
            else:
                ops.check(lib.flk_clip_prepare_train(C.byref(gp), gp._boxes, outp, st))

        def gather():
            for k in range(N):
                torch.index_select(videos[k], 0, idx_dev[k], out=gbuf[k])

        def ten_sampled():
            for _ in range(10):
                ops.check(lib.flk_clip_prepare_sampled(C.byref(sp), sp._boxes, _lib.ptr(sp._frame_idx), T, outp, st))

        def ten_gather_existing():
            for _ in range(10):
                gather()
                existing()

        def ten_existing():
            for _ in range(10):
                existing()

        fns = {"sampled": ten_sampled, "gather_plus_existing": ten_gather_existing, "existing_on_gathered": ten_existing}
        ten_gather_existing()
        want = buf.clone()
        ten_sampled()
        assert torch.equal(buf, want), "the sampled launch differs from gather + existing launch"
        for _ in range(4):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.launches):
            for k, f in fns.items():
                ms[k].append(timed(f) / 10)
        per_frame = [window_bytes(1, H, W) if not bk else box_bytes(1, H, W, q[:4]) for q in params]
        nbytes = sum(len(set(r.tolist())) * b for r, b in zip(table, per_frame)) + buf.numel() * 4
        r = {k: summary(v, "us") for k, v in ms.items()}
        r["compulsory_bytes"] = nbytes
        r["sampled_gb_per_s"] = round(nbytes / (r["sampled"]["median_us"] * 1e-6) / 1e9, 1)
        r["gather_plus_existing_over_sampled"] = round(r["gather_plus_existing"]["median_us"] / r["sampled"]["median_us"], 3)
        r["sampled_over_existing"] = round(r["sampled"]["median_us"] / r["existing_on_gathered"]["median_us"], 3)
        res[leg] = r
    out["sampled_16x16_from_300x240x320"] = res


def parent_case(a, out):
    """section 5 of the module docstring"""
    from flickering_adversarial_video_amd import _lib
    parent = C.CDLL(a.parent_lib)
    for name in ("flk_clip_prepare", "flk_clip_prepare_train"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib._SIGS[name]
    rng = np.random.default_rng(1)
    N, T, H, W = 16, 16, 240, 320
    raw = torch.from_numpy(rng.integers(0, 256, (N, T, H, W, 3), dtype=np.uint8)).cuda()
    buf = torch.empty((N, T, 112, 112, 3), dtype=torch.float32, device="cuda")
    Hr, Wr = vs.prepare_geometry(H, W, 128, 112)[:2]
    prng = random.Random(0)
    params = [vs.train_crop_params(Hr, Wr, rng=prng) for _ in range(N)]
    plans = {"flk_clip_prepare": ops.prepare_clips_plan(raw, out=buf)[0][0],
             "flk_clip_prepare_train": ops.prepare_clips_plan(raw, out=buf, boxes=[q[:4] for q in params], flips=[q[4] for q in params])[0][0]}
    outp, st = ops.ptr(buf), ops.stream_ptr()
    res = {}
    for name, p in plans.items():
        def ten(lib):
            for _ in range(10):
                if p._boxes is None:
                    ops.check(lib.flk_clip_prepare(C.byref(p), outp, st))
                else:
                    ops.check(lib.flk_clip_prepare_train(C.byref(p), p._boxes, outp, st))
        ten(parent)
        want = buf.clone()
        buf.zero_()
        ten(ops.load())
        assert torch.equal(buf, want), f"{name}: this library's output differs from the parent's"
        legs = {"this": ops.load(), "parent_a": parent, "parent_b": parent}
        for _ in range(4):
            for lib in legs.values():
                ten(lib)
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(a.launches):
            for k, lib in legs.items():
                ms[k].append(timed(lambda: ten(lib)) / 10)
        r = {k: summary(v, "us") for k, v in ms.items()}
        r["this_over_parent_a"] = round(r["this"]["median_us"] / r["parent_a"]["median_us"], 4)
        r["parent_b_over_parent_a"] = round(r["parent_b"]["median_us"] / r["parent_a"]["median_us"], 4)
        res[name] = r
    out["against_parent_library"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-clips", action="store_true", help="skip sections 1 and 2")
    ap.add_argument("--parent-lib", default="", help="a libflicker_hip.so built from the parent commit (section 5)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_time.py needs a GPU: a CPU run gives no time")
    out = {"torch_threads": torch.get_num_threads()}
    rng = np.random.default_rng(0)
    videos = [torch.randint(0, 256, (300, 240, 320, 3), dtype=torch.uint8, device="cuda") for _ in range(16)]      # resident whole videos
    sampled_case(a, out, videos)
    if a.parent_lib:
        parent_case(a, out)
    for tag, (N, T, H, W) in (() if a.skip_clips else (("16x16x240x320", (16, 16, 240, 320)), ("8x32x256x340", (8, 32, 256, 340)))):
        raw_h = torch.from_numpy(rng.integers(0, 256, (N, T, H, W, 3), dtype=np.uint8))
        raw = raw_h.cuda()
        buf = torch.empty((N, T, 112, 112, 3), dtype=torch.float32, device="cuda")
        plan, _, _ = ops.prepare_clips_plan(raw, out=buf)
        assert len(plan) == 1
        lib, arg, outp, st = ops.load(), C.byref(plan[0]), ops.ptr(buf), ops.stream_ptr()

        def ten():
            for _ in range(10):
                ops.check(lib.flk_clip_prepare(arg, outp, st))

        for _ in range(5):
            ops.prepare_clips(raw, out=buf)
            ten()
        # the training transform's launch on the same clips: default sampler, and boxes of the output size (no second resampling)
        Hr, Wr = vs.prepare_geometry(H, W, 128, 112)[:2]
        srng = random.Random(0)
        legs = {"train": [vs.train_crop_params(Hr, Wr, rng=srng) for _ in range(N)],
                "train_crop_only": [vs.train_crop_params(Hr, Wr, scales=None, rng=srng) for _ in range(N)]}
        tens = {}
        for leg, params in legs.items():
            tplan, _, _ = ops.prepare_clips_plan(raw, out=buf, boxes=[q[:4] for q in params], flips=[q[4] for q in params])
            assert len(tplan) == 1

            def ten_train(tp=tplan[0]):
                for _ in range(10):
                    ops.check(lib.flk_clip_prepare_train(C.byref(tp), tp._boxes, outp, st))
            tens[leg] = ten_train
            for _ in range(5):
                ten_train()
        torch.cuda.synchronize()
        ms, mt = [], {leg: [] for leg in legs}
        for _ in range(a.launches):
            ms.append(timed(ten) / 10)
            for leg in legs:
                mt[leg].append(timed(tens[leg]) / 10)
        mw = [timed(lambda: ops.prepare_clips(raw, out=buf)) for _ in range(a.launches)]
        nbytes = N * window_bytes(T, H, W) + buf.numel() * 4
        th = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            for k in range(N):
                vs.prepare_host(raw_h[k])
            th.append((time.perf_counter() - t0) * 1e3)
        dev = summary(ms, "us")
        out[tag] = dict(device=dev, wrapper=summary(mw, "us"), window_plus_written_bytes=nbytes, gb_per_s=round(nbytes / (dev["median_us"] * 1e-6) / 1e9, 1),
                        host=summary(th, "ms"), host_over_device=round(statistics.median(th) * 1e3 / dev["median_us"], 1))
        for leg, params in legs.items():
            tb = sum(box_bytes(T, H, W, q[:4]) for q in params) + buf.numel() * 4
            tdev = summary(mt[leg], "us")
            out[tag][leg] = dict(device=tdev, box_plus_written_bytes=tb, gb_per_s=round(tb / (tdev["median_us"] * 1e-6) / 1e9, 1),
                                 over_eval_launch=round(tdev["median_us"] / dev["median_us"], 3), boxes=[list(q[:4]) + [int(q[4])] for q in params[:4]])
    if not a.skip_step:
        B, T, nb = 16, 16, 4
        Wt = vs.synthetic_weights("mc3_18", 42)
        shard = torch.from_numpy(rng.integers(0, 256, (nb * B, T, 240, 320, 3), dtype=np.uint8)).cuda()      # resident raw shard: nb batches
        crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=False)
        engs = {leg: FlickerVideoResNet("mc3_18", Wt, batch_size=B, sample_length=T, dtype="bf16", l_inf_pert_norm=0.1,
                                        augment={"seed": 0} if leg == "raw_train" else None,
                                        sampling={"temporal_jitter": True, "random_shift": True} if leg == "videos" else None)
                for leg in ("raw", "raw_train", "videos", "prepared")}
        ready = [engs["prepared"].prepare(shard[k * B:(k + 1) * B]).clone() for k in range(nb)]
        labels = engs["prepared"].logits(ready[0], False).argmax(1).clone()
        it = [0]

        def step_raw():
            k = it[0] % nb
            engs["raw"].step(engs["raw"]._prepared(shard[k * B:(k + 1) * B]), labels, crit)

        def step_raw_train():
            k = it[0] % nb
            engs["raw_train"].step(engs["raw_train"]._prepared(shard[k * B:(k + 1) * B], train=True), labels, crit)

        def step_videos():
            e = engs["videos"]
            e.step(e.prepare_videos(videos, train=True, out=e._clip_buf("_prep_buf")), labels, crit)

        def step_prepared():
            engs["prepared"].step(ready[it[0] % nb], labels, crit)

        for _ in range(3):
            step_raw(); step_raw_train(); step_videos(); step_prepared(); it[0] += 1
        torch.cuda.synchronize()
        ts = {"raw": [], "raw_train": [], "videos": [], "prepared": []}
        for _ in range(a.steps):
            ts["raw"].append(timed(step_raw)); ts["raw_train"].append(timed(step_raw_train)); ts["videos"].append(timed(step_videos)); ts["prepared"].append(timed(step_prepared)); it[0] += 1
        s = {leg: summary(t, "ms") for leg, t in ts.items()}
        s["prepare_share_percent"] = round(100.0 * (s["raw"]["median_ms"] / s["prepared"]["median_ms"] - 1.0), 2)
        s["train_prepare_share_percent"] = round(100.0 * (s["raw_train"]["median_ms"] / s["prepared"]["median_ms"] - 1.0), 2)
        s["videos_sample_prepare_share_percent"] = round(100.0 * (s["videos"]["median_ms"] / s["prepared"]["median_ms"] - 1.0), 2)
        out["mc3_18_bs16_bf16_step"] = s
    print(json.dumps(out))


if __name__ == "__main__":
    main()
