#!/usr/bin/env python3
"""Timing of the video-level loss head against the clip-level one.

1. flk_softmax_adv_loss_video vs flk_softmax_adv_loss on [16, 400] logits (torch dialect, improve-loss on probabilities): the clip head
   (16 workgroups), the video head at G = 1 (16 workgroups) and at G = 4 (4 workgroups), alternating; every sample is one HIP-event pair
   around `--batch` back-to-back launches, reported per launch (a single launch of a few microseconds is below what an event pair
   resolves); median, min and max over `--samples` samples after a warm-up.
2. one mc3_18 attack step (batch 16, T = 16, bf16) with clips_per_video = 1 (the clip-level step) and = 4 on the same clips, the two
   engines alternating step by step; `--rounds` rounds of `--steps` steps each, one median per round and engine: the range of the round
   medians is the run-to-run spread a difference between the two has to exceed.

    python tools/video_loss_time.py [--samples 30] [--batch 200] [--steps 20] [--rounds 3] [--skip-step]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses


def timed(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def summary(ms, unit):
    k = 1e3 if unit == "us" else 1.0
    return {f"median_{unit}": round(statistics.median(ms) * k, 3), f"min_{unit}": round(min(ms) * k, 3), f"max_{unit}": round(max(ms) * k, 3), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--batch", type=int, default=200, help="launches per timed sample of the heads")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_loss_time.py needs a GPU: a CPU run gives no time")
    B, Cn = 16, 400
    torch.manual_seed(0)
    lg = torch.randn(B, Cn, device="cuda") * 2
    kw = dict(dialect="torch", improve_loss=True, use_logits=False, margin=0.05)
    heads = {}
    lab = torch.randint(0, Cn, (B,), device="cuda")
    out_c = ops.softmax_adv_loss(lg, lab, **kw)
    heads["clip_head"] = lambda: ops.softmax_adv_loss(lg, lab, out=out_c, **kw)
    for G in (1, 4):
        labv = lab[:B // G].clone()
        out_v = ops.softmax_adv_loss_video(lg, labv, G, reduce="mean", **kw)
        heads[f"video_head_G{G}"] = (lambda G=G, labv=labv, out_v=out_v: ops.softmax_adv_loss_video(lg, labv, G, reduce="mean", out=out_v, **kw))
    for fn in heads.values():
        timed(fn, a.batch)
    ts = {k: [] for k in heads}
    for _ in range(a.samples):
        for k, fn in heads.items():
            ts[k].append(timed(fn, a.batch))
    out = dict(logits=[B, Cn], launches_per_sample=a.batch, heads={k: summary(t, "us") for k, t in ts.items()})
    if not a.skip_step:
        T = 16
        Wt = vs.synthetic_weights("mc3_18", 42)
        x = torch.from_numpy(vs.synthetic_clip(B, T, seed=1)).cuda()
        crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=False)
        engs = {G: FlickerVideoResNet("mc3_18", Wt, batch_size=B, sample_length=T, dtype="bf16", clips_per_video=G, video_reduce="mean") for G in (1, 4)}
        labels = {G: e.video_logits(e.logits(x, False)).argmax(1).clone() for G, e in engs.items()}
        for _ in range(3):
            for G, e in engs.items():
                e.step(x, labels[G], crit)
        torch.cuda.synchronize()
        rounds = {G: [] for G in engs}
        every = {G: [] for G in engs}
        for _ in range(a.rounds):
            t = {G: [] for G in engs}
            for _ in range(a.steps):
                for G, e in engs.items():
                    t[G].append(timed(lambda: e.step(x, labels[G], crit)))
            for G in engs:
                rounds[G].append(round(statistics.median(t[G]), 4))
                every[G] += t[G]
        out["mc3_18_bs16_T16_bf16_step"] = {f"G{G}": dict(summary(every[G], "ms"), round_medians_ms=rounds[G],
                                                           round_spread_ms=round(max(rounds[G]) - min(rounds[G]), 4)) for G in engs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
