#!/usr/bin/env python3
"""What training through a rolling-shutter capture channel costs: the mc3_18 batch-16 attack step on video time (bf16, 16 frames of
112 x 112, resident uint8 clips, Adam, period 16, the rows of 16 clips cut from 300-frame videos at the evaluation's offsets).

1. Three legs on THIS build, in one process, stepping alternately, a HIP-event pair around every step:
   `plain`   -- no channel: flk_flicker_rows_gather, the per-clip apply / gradient, flk_flicker_rows_grad;
   `channel` -- capture=CaptureChannel(subframe=(0, 1), exposure=(0.5, 2), gain=(0.7, 1), gain_mode="per_channel"), no readout:
                flk_flicker_rows_mix / flk_flicker_rows_mix_grad in the place of the gather / row gradient;
   `readout` -- the same channel with readout=(0, 1) and a fresh draw per step: the per-line tables (16 x 112 x K floats) are made on the host
                and go to the device every step, flk_flicker_lines_mix writes the per-line perturbation [16,16,112,3], the apply and the
                delta-gradient take their per-line forms (flk_apply_args.delta_per_line) and flk_flicker_lines_mix_grad (two launches) folds
                the per-line gradient back.
2. `plain` and `channel` against the PARENT commit (`--parent-root PATH`: a checkout of the parent with its library built): the same
   launches, so the trees only have to agree inside the run's spread.  Each is timed in processes of its own, the two trees alternating
   `--rounds` times; the spread is the range of one tree's per-process medians.

Prints one JSON line per leg and a summary line.  Needs the GPU; there is no fallback.

    python tools/rolling_shutter_time.py [--steps 40] [--warmup 8] [--rounds 2] [--parent-root PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, HW = 16, 16, 112


def worker(a):
    """one process: the engines of the tree `--root`, timed step by step; the JSON result on the last line of stdout"""
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    assert torch.cuda.is_available(), "rolling_shutter_time needs the GPU"
    W = vs.synthetic_weights("mc3_18", 42)
    x = torch.from_numpy(vs.synthetic_clip_u8(B, T, HW, HW, seed=7)).cuda()
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=False)
    channel = dict(subframe=(0.0, 1.0), exposure=(0.5, 2.0), gain=(0.7, 1.0), gain_mode="per_channel", seed=0)
    legs = {}
    for leg in a.legs.split(","):
        kw = {}
        if leg == "channel":
            kw["capture"] = vs.CaptureChannel(**channel)
        elif leg == "readout":
            kw["capture"] = vs.CaptureChannel(readout=(0.0, 1.0), **channel)
        eng = FlickerVideoResNet("mc3_18", W, batch_size=B, sample_length=T, image_size=HW, dtype="bf16", l_inf_pert_norm=0.1,
                                 flicker_time="video", flicker_period=T, **kw)
        eng.set_frame_numbers(np.concatenate([vs.sample_frame_indices(300, T, num_samples=1) + 3 * k for k in range(B)]))
        legs[leg] = eng
    lab = next(iter(legs.values())).logits(x, False).argmax(1).clone()
    ms = {leg: [] for leg in legs}
    for it in range(a.warmup + a.steps):
        for leg, eng in legs.items():                       # the legs alternate step by step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.step(x, lab, crit, lr=1e-3)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[leg].append(e0.elapsed_time(e1))
    out = {leg: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)} for leg, v in ms.items()}
    print(json.dumps({"root": a.root, "legs": out}), flush=True)


def run_worker(root, legs, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--legs", legs, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({root}, {legs}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["legs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="plain,channel,readout", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    same = run_worker(HERE, "plain,channel,readout", a)
    for leg, v in same.items():
        print(json.dumps({"what": "same build, one process, alternating steps", "leg": leg, **v}), flush=True)
    summary = {"channel_minus_plain_ms": round(same["channel"]["median_ms"] - same["plain"]["median_ms"], 4),
               "readout_minus_channel_ms": round(same["readout"]["median_ms"] - same["channel"]["median_ms"], 4),
               "readout_over_plain": round(same["readout"]["median_ms"] / same["plain"]["median_ms"], 4)}
    if a.parent_root:
        med = {("this", "plain"): [], ("this", "channel"): [], ("parent", "plain"): [], ("parent", "channel"): []}
        for k in range(a.rounds):                           # the two trees alternate, a process each; who goes first alternates too
            for tree in (("parent", "this"), ("this", "parent"))[k % 2]:
                res = run_worker(os.path.abspath(a.parent_root) if tree == "parent" else HERE, "plain,channel", a)
                for leg in ("plain", "channel"):
                    med[(tree, leg)].append(res[leg]["median_ms"])
        print(json.dumps({"what": "no readout, a process per tree and round", **{f"{t}_{l}_median_ms": v for (t, l), v in med.items()}}), flush=True)
        for (tree, leg), v in med.items():
            summary[f"{leg}_{tree}_ms"] = round(statistics.median(v), 4)
            summary[f"{leg}_{tree}_spread_ms"] = round(max(v) - min(v), 4)
    else:
        summary.update(parent="not measured")
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
