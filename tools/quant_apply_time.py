#!/usr/bin/env python3
"""What the 8-bit straight-through apply (flk_apply_args.q_lut, the QUANT instantiations of the apply kernels in csrc/attack.hip) costs.

1. every apply route at 16 x 16 x 112 x 112 in the torch dialect -- fp32 and uint8 source, fold 1 (fp32 out: the generic kernel) and
   fold 4 (bf16 hi/lo out: apply_s2d_hilo_kernel from fp32, apply_s2d_hilo_u8_kernel from uint8) -- with and without q_lut.  The
   arguments and the output are built once; a HIP-event pair brackets 10 back-to-back launches through the C ABI (the figure is the
   tenth); the plain and the quantised leg alternate group by group; median / min / max over N groups (--launches) after a warm-up.
   GB/s of the compulsory bytes (source + output).
2. an mc3_18 step at batch 16 (bf16, uint8 clips, Adam) with and without quantise_train: ONE engine, the attribute flipped between
   alternating steps, a HIP-event pair around each step (--steps per leg).

--tree PATH times the package of another checkout with this same tool -- the parent commit, to hold its plain launches against this
commit's: a package without the option gets the plain legs only.

    python tools/quant_apply_time.py [--launches 30] [--steps 20] [--tree PATH]"""
import argparse
import ctypes as C
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
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg of the mc3_18 step (0: skip it)")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package is timed")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch
    from flickering_adversarial_video_amd import _lib, ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses, Perturbation
    if not torch.cuda.is_available():
        raise SystemExit("quant_apply_time.py needs a GPU: a CPU run gives no time")
    has_q = hasattr(_lib.ApplyArgs, "q_lut")
    res = {"tree": os.path.abspath(a.tree), "has_quantised_apply": has_q}
    rng = np.random.default_rng(0)
    B, T, HW = 16, 16, 112
    u8 = vs.synthetic_clip_u8(B, T, HW, HW, seed=1)
    pm = Perturbation((3, T, 1, 1), max_norm=0.2)
    pm.init_perturbation(rng.uniform(-0.2, 0.2, (3, T, 1, 1)).astype(np.float32))
    lib, sp = ops.load(), ops.stream_ptr()
    srcs = {"u8": torch.from_numpy(u8).cuda(), "fp32": torch.from_numpy(vs.normalize_u8(u8)).cuda()}
    for sname, x in srcs.items():
        for fold_t, dt in ((1, torch.float32), (4, torch.bfloat16)):
            out = torch.empty((B, T, HW // 2, HW // 2, 32 if fold_t == 4 else 16), dtype=dt, device="cuda")
            args = {"plain": pm.apply_args(x, True, fold_t=fold_t)}
            if has_q:
                args["quantised"] = pm.apply_args(x, True, fold_t=fold_t, quantise=True)

            def ten(k):
                for _ in range(10):
                    ops.check(lib.flk_perturb_apply_s2d(C.byref(args[k]), ops.ptr(out), ops.dtype_code(dt), sp))
            for _ in range(3):
                for k in args:
                    ten(k)
            torch.cuda.synchronize()
            ms = {k: [] for k in args}
            for _ in range(a.launches):
                for k in args:
                    ms[k].append(timed(torch, lambda: ten(k)) / 10)
            r = {k: summary(v) for k, v in ms.items()}
            nbytes = x.numel() * x.element_size() + out.numel() * out.element_size()
            r["compulsory_bytes"] = nbytes
            for k in args:
                r[k]["gb_per_s"] = round(nbytes / (r[k]["median_us"] * 1e-6) / 1e9, 1)
            if has_q:
                r["quantised_over_plain"] = round(r["quantised"]["median_us"] / r["plain"]["median_us"], 3)
            res[f"apply_{sname}_fold{fold_t}_16x16x112x112"] = r
    del srcs, out, args
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
