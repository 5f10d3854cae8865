#!/usr/bin/env python3
"""What the 8-bit straight-through apply (flk_apply_args.q_lut, the QUANT instantiations of the apply kernels in csrc/attack.hip) costs in
an mc3_18 step at batch 16 (bf16, uint8 clips, Adam) with and without quantise_train: ONE engine, the attribute flipped between
alternating steps, a HIP-event pair around each step (--steps per leg).  (The single launches, every apply route with and without q_lut,
are the `vrn_apply_*` legs of tools/perturb_time.py.)

--tree PATH times the package of another checkout with this same tool -- the parent commit, to hold its plain steps against this
commit's: a package without the option gets the plain leg only.

    python tools/quant_apply_time.py [--steps 20] [--tree PATH]"""
import argparse
import json
import os
import statistics
import sys


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 3), "min_us": round(min(ms) * 1e3, 3), "max_us": round(max(ms) * 1e3, 3), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg of the mc3_18 step")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package is timed")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from flickering_adversarial_video_amd import _lib, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    if not torch.cuda.is_available():
        raise SystemExit("quant_apply_time.py needs a GPU: a CPU run gives no time")
    has_q = hasattr(_lib.ApplyArgs, "q_lut")
    res = {"tree": os.path.abspath(a.tree), "has_quantised_apply": has_q}
    B, T, HW = 16, 16, 112
    u8 = vs.synthetic_clip_u8(B, T, HW, HW, seed=1)
    if a.steps > 0:
        eng = FlickerVideoResNet("mc3_18", vs.synthetic_weights("mc3_18", 42), batch_size=B, sample_length=T, image_size=HW, dtype="bf16",
                                 l_inf_pert_norm=0.2)
        crit = Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)
        x = torch.from_numpy(u8).cuda()
        lab = eng.logits(x, False).argmax(1).clone()
        legs = {"plain": False, "quantise_train": True} if has_q else {"plain": False}

        def step(q):
            if has_q:
                eng.quantise_train = q
            eng.step(x, lab, crit, lr=1e-3, update=True)
        for _ in range(3):
            for q in legs.values():
                step(q)
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(a.steps):
            for k, q in legs.items():
                ms[k].append(timed(torch, lambda: step(q)))
        r = {k: summary(v) for k, v in ms.items()}
        if has_q:
            r["quantise_train_over_plain"] = round(r["quantise_train"]["median_us"] / r["plain"]["median_us"], 4)
        res["step_mc3_18_bs16_bf16_u8"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
