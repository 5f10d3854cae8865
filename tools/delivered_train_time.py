#!/usr/bin/env python3
"""What training on the delivered video costs: the mc3_18 batch-16 attack step (bf16, 16 frames of 112 x 112, Adam, flicker on video time
with period 16) fed from 16 resident raw uint8 videos of 300 x 240 x 320, every batch cut with fresh tables of the training split and
prepared with the training transform (fresh boxes and flips).

1. Step legs on THIS build, in one process, stepping alternately, a HIP-event pair around every step:
   `raw`              -- today's raw route: prepare_videos(train=True) + step, additive (the flicker added to the resampled fp32 clip);
   `delivered`        -- step_videos, additive: gather, tone tables (the export launch on the ramp), toned prepare, the clean forward,
                         backward, slopes, flk_clip_prepare_grad, row fold, update;
   `delivered_illum`  -- step_videos, flicker_model="illumination".
2. Single launches on the step's shapes, `--reps` launches between one HIP-event pair, the median of the groups: the toned against the
   untoned sampled preparation (evaluation and training transform), flk_clip_prepare_grad (both transforms), the tone-table launch and
   the slope launch of both pixel models.  Arguments are built once (ops.prepare_clips_plan); the launches go through the C ABI.
3. `raw` against the PARENT commit (`--parent-root PATH`: a checkout of the parent with its library built): the same launches, so the
   trees only have to agree inside the run's spread.  Each tree is timed in processes of its own, alternating `--rounds` times; the
   spread is the range of one tree's per-process medians.

Prints one JSON line per leg and a summary line.  Needs the GPU; there is no fallback.

    python tools/delivered_train_time.py [--steps 40] [--warmup 8] [--rounds 2] [--reps 30] [--frames 300] [--parent-root PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, HW, P = 16, 16, 112, 16


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def worker(a):
    """one process: the engines of the tree `--root`, timed step by step; the JSON result on the last line of stdout"""
    sys.path.insert(0, a.root)
    import torch
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    assert torch.cuda.is_available(), "delivered_train_time needs the GPU"
    W = vs.synthetic_weights("mc3_18", 42)
    gen = torch.Generator(device="cuda").manual_seed(7)
    videos = [torch.randint(0, 256, (a.frames, 240, 320, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(B)]
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=False)
    common = dict(batch_size=B, sample_length=T, image_size=HW, dtype="bf16", l_inf_pert_norm=0.1, flicker_time="video", flicker_period=P,
                  augment={"seed": 0}, sampling={"temporal_jitter": True, "random_shift": True, "seed": 0})
    legs = {}
    for leg in a.legs.split(","):
        kw = {} if leg == "raw" else dict(train_delivered=True)
        if leg == "delivered_illum":
            kw["flicker_model"] = "illumination"
        legs[leg] = FlickerVideoResNet("mc3_18", W, **common, **kw)
    first = next(iter(legs.values()))
    buf = torch.empty((B, T, HW, HW, 3), dtype=torch.float32, device="cuda")
    lab = first.logits(first.prepare_videos(videos, train=False, out=buf), False).argmax(1).clone()
    ms = {leg: [] for leg in legs}
    for it in range(a.warmup + a.steps):
        for leg, eng in legs.items():                       # the legs alternate step by step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if leg == "raw":
                eng.step(eng.prepare_videos(videos, train=True, out=buf), lab, crit, lr=1e-3)
            else:
                eng.step_videos(videos, lab, crit, lr=1e-3, train=True)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[leg].append(e0.elapsed_time(e1))
    out = {leg: stats(v) for leg, v in ms.items()}
    if a.launches:
        out.update(launches(a, videos, legs["delivered"], legs["delivered_illum"], torch))
    print(json.dumps({"root": a.root, "legs": out}), flush=True)


def launches(a, videos, eng, eng_il, torch):
    """single launches on the step's shapes: `reps` launches between one event pair, per-launch milliseconds"""
    import ctypes as C
    import random

    import numpy as np
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd._lib import ptr, stream_ptr
    lib = ops.load()
    rows = np.concatenate([vs.sample_frame_indices(a.frames, T, temporal_jitter=True, random_shift=True, rng=np.random.RandomState(0)) for _ in range(B)])
    Hr, Wr = vs.prepare_geometry(240, 320)[:2]
    rng = random.Random(0)
    params = [vs.train_crop_params(Hr, Wr, rng=rng) for _ in range(B)]
    tf = {"eval": {}, "train": dict(boxes=[p[:4] for p in params], flips=[p[4] for p in params])}
    out_buf = torch.empty((B, T, HW, HW, 3), dtype=torch.float32, device="cuda")
    plans = {k: ops.prepare_clips_plan(videos, out_buf, frame_idx=rows, **kw)[0][0] for k, kw in tf.items()}
    calls = {}
    gx = torch.randn_like(eng._gx)
    gd = torch.empty((B, T, 3), dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.flk_clip_prepare_grad_scratch_bytes(B, T, HW) // 4, dtype=torch.float32, device="cuda")
    for name, e in (("additive", eng), ("illumination", eng_il)):
        pm = e.pert_model
        pm.perturbation.uniform_(-0.1, 0.1)
        pm.set_frame_numbers(rows)
        ramp = ops.tone_ramp(B, T)
        ta = pm.export_args(ramp, True, shift_p=0)
        il = pm.illum if name == "illumination" else None
        tone = ops.flicker_tone_tables(ta, il)
        slope, scale = ops.flicker_tone_slopes(ta, il)
        calls[f"tone_tables_{name}"] = lambda ta=ta, il=il, tone=tone: ops.flicker_tone_tables(ta, il, out=tone)
        calls[f"tone_slopes_{name}"] = lambda ta=ta, il=il, slope=slope, scale=scale: ops.flicker_tone_slopes(ta, il, slope, scale)
        if name == "additive":
            for k, pl in plans.items():
                calls[f"prepare_sampled_{k}"] = lambda pl=pl: lib.flk_clip_prepare_sampled(C.byref(pl), pl._boxes, ptr(pl._frame_idx), T, ptr(out_buf), stream_ptr())
                calls[f"prepare_toned_{k}"] = lambda pl=pl, tone=tone: lib.flk_clip_prepare_toned(C.byref(pl), pl._boxes, ptr(pl._frame_idx), T, ptr(tone),
                                                                                                  ptr(out_buf), stream_ptr())
                calls[f"prepare_grad_{k}"] = lambda pl=pl, slope=slope, scale=scale: lib.flk_clip_prepare_grad(
                    C.byref(pl), pl._boxes, ptr(pl._frame_idx), T, ptr(slope), ptr(scale), ptr(gx), ops.dtype_code(gx.dtype), ptr(gd), ptr(scratch), stream_ptr())
    out = {}
    for name, call in calls.items():
        for _ in range(5):
            call()
        v = []
        for _ in range(max(3, a.rounds * 3)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            e1.synchronize()
            v.append(e0.elapsed_time(e1) / a.reps)
        out[name] = stats(v)
    return out


def run_worker(root, legs, a, with_launches=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--legs", legs, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--reps", str(a.reps), "--rounds", str(a.rounds), "--frames", str(a.frames)] + (["--launches"] if with_launches else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({root}, {legs}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["legs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=300, help="frames of each of the 16 resident videos")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launches", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="raw,delivered,delivered_illum", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    same = run_worker(HERE, "raw,delivered,delivered_illum", a, with_launches=True)
    for leg, v in same.items():
        print(json.dumps({"what": "same build, one process", "leg": leg, **v}), flush=True)
    summary = {"delivered_minus_raw_ms": round(same["delivered"]["median_ms"] - same["raw"]["median_ms"], 4),
               "delivered_over_raw": round(same["delivered"]["median_ms"] / same["raw"]["median_ms"], 4),
               "delivered_illum_over_raw": round(same["delivered_illum"]["median_ms"] / same["raw"]["median_ms"], 4)}
    for k in ("eval", "train"):
        summary[f"toned_over_sampled_{k}"] = round(same[f"prepare_toned_{k}"]["median_ms"] / same[f"prepare_sampled_{k}"]["median_ms"], 3)
    if a.parent_root:
        med = {"this": [], "parent": []}
        for k in range(a.rounds):                           # the two trees alternate, a process each; who goes first alternates too
            for tree in (("parent", "this"), ("this", "parent"))[k % 2]:
                med[tree].append(run_worker(os.path.abspath(a.parent_root) if tree == "parent" else HERE, "raw", a)["raw"]["median_ms"])
        print(json.dumps({"what": "raw step, a process per tree and round", **{f"{t}_median_ms": v for t, v in med.items()}}), flush=True)
        for tree, v in med.items():
            summary[f"raw_{tree}_ms"] = round(statistics.median(v), 4)
            summary[f"raw_{tree}_spread_ms"] = round(max(v) - min(v), 4)
    else:
        summary.update(parent="not measured")
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
