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
   clips, the legs alternating step by step.  The last leg uses nothing this tool's subject added.

    python tools/prepare_time.py [--launches 30] [--steps 20] [--host-reps 3] [--skip-step]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_time.py needs a GPU: a CPU run gives no time")
    out = {"torch_threads": torch.get_num_threads()}
    rng = np.random.default_rng(0)
    for tag, (N, T, H, W) in (("16x16x240x320", (16, 16, 240, 320)), ("8x32x256x340", (8, 32, 256, 340))):
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
                                        augment={"seed": 0} if leg == "raw_train" else None) for leg in ("raw", "raw_train", "prepared")}
        ready = [engs["prepared"].prepare(shard[k * B:(k + 1) * B]).clone() for k in range(nb)]
        labels = engs["prepared"].logits(ready[0], False).argmax(1).clone()
        it = [0]

        def step_raw():
            k = it[0] % nb
            engs["raw"].step(engs["raw"]._prepared(shard[k * B:(k + 1) * B]), labels, crit)

        def step_raw_train():
            k = it[0] % nb
            engs["raw_train"].step(engs["raw_train"]._prepared(shard[k * B:(k + 1) * B], train=True), labels, crit)

        def step_prepared():
            engs["prepared"].step(ready[it[0] % nb], labels, crit)

        for _ in range(3):
            step_raw(); step_raw_train(); step_prepared(); it[0] += 1
        torch.cuda.synchronize()
        ts = {"raw": [], "raw_train": [], "prepared": []}
        for _ in range(a.steps):
            ts["raw"].append(timed(step_raw)); ts["raw_train"].append(timed(step_raw_train)); ts["prepared"].append(timed(step_prepared)); it[0] += 1
        s = {leg: summary(t, "ms") for leg, t in ts.items()}
        s["prepare_share_percent"] = round(100.0 * (s["raw"]["median_ms"] / s["prepared"]["median_ms"] - 1.0), 2)
        s["train_prepare_share_percent"] = round(100.0 * (s["raw_train"]["median_ms"] / s["prepared"]["median_ms"] - 1.0), 2)
        out["mc3_18_bs16_bf16_step"] = s
    print(json.dumps(out))


if __name__ == "__main__":
    main()
