#!/usr/bin/env python3
"""Timing of the projected sign-gradient (PGD) update against Adam.

1. flk_perturb_dense_l12_pgd vs flk_perturb_dense_l12_adam at [T,224,224,3] (default T = 64): whole entry points (the two reduction
   passes + the streaming update), one HIP-event pair per launch, the two optimisers alternating; median, min and max over N launches
   after a warm-up.  Bytes of the streaming pass alone: Adam 7 fp32 array passes (delta, m, v in and out, g in), PGD 3 (g, delta in,
   delta out); both entry points read delta twice more in the reduction pass (each frame and its predecessor).
2. one I3D attack step (batch 8, bf16, T frames) under each optimiser, the two engines alternating step by step.

    python tools/pgd_time.py [--frames 64] [--launches 30] [--steps 10] [--skip-step]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from flickering_adversarial_video_amd import i3d_spec, ops
from flickering_adversarial_video_amd.i3d_engine import FlickerI3D


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pgd_time.py needs a GPU: a CPU run gives no time")
    T, H, W = a.frames, 224, 224
    torch.manual_seed(0)
    d0 = (torch.rand(T, H, W, 3, device="cuda") - 0.5) * 0.1
    g = torch.randn(T, H, W, 3, device="cuda") * 1e-5
    da, dp = d0.clone(), d0.clone()
    m, v = torch.zeros_like(d0), torch.zeros_like(d0)
    scratch = torch.empty(ops.load().flk_dense_adam_scratch_bytes(T, H, W) // 4, dtype=torch.float32, device="cuda")
    sc = torch.empty(4, dtype=torch.float32, device="cuda")
    step = [0]

    def adam():
        step[0] += 1
        ops.perturb_dense_l12_adam(g, da, m, v, step[0], beta=1.0, lr=1e-6, scalars=sc, scratch=scratch)

    def pgd():
        ops.perturb_dense_l12_pgd(g, dp, beta=1.0, lr=1e-6, eps=0.04, scalars=sc, scratch=scratch)

    for _ in range(5):
        adam(); pgd()
    torch.cuda.synchronize()
    t_adam, t_pgd = [], []
    for _ in range(a.launches):
        t_adam.append(timed(adam)); t_pgd.append(timed(pgd))
    n = T * H * W * 3 * 4
    out = dict(shape=[T, H, W, 3], dense_adam=summary(t_adam, "us"), dense_pgd=summary(t_pgd, "us"),
               update_pass_bytes=dict(adam=7 * n, pgd=3 * n), reduction_pass_bytes=2 * n)
    out["dense_pgd_over_adam"] = round(out["dense_pgd"]["median_us"] / out["dense_adam"]["median_us"], 3)
    if not a.skip_step:
        Wt = i3d_spec.synthetic_i3d_weights(42)
        xu = torch.from_numpy(i3d_spec.synthetic_clip_u8(8, T, seed=1)).cuda()
        engs = {opt: FlickerI3D(Wt, batch_size=8, frames=T, dtype="bf16", optimizer=opt) for opt in ("adam", "pgd")}
        labels = engs["adam"].logits(xu, adv_flag=0.0).argmax(-1).clone()
        for _ in range(3):
            for e in engs.values():
                e.step(xu, labels)
        torch.cuda.synchronize()
        ts = {opt: [] for opt in engs}
        for _ in range(a.steps):
            for opt, e in engs.items():
                ts[opt].append(timed(lambda: e.step(xu, labels)))
        out["i3d_bs8_bf16_step"] = {opt: summary(t, "ms") for opt, t in ts.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
