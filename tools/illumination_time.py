#!/usr/bin/env python3
"""What the illumination pixel model costs: the mc3_18 batch-16 attack step (bf16, 16 frames of 112 x 112, resident uint8 clips, Adam,
clip time) and the three launches that differ between the models.

1. Step legs on THIS build, in one process, stepping alternately, a HIP-event pair around every step:
   `additive`          -- the default engine: flk_net_forward_apply (the plan applies in front of its stem), flk_perturb_grad_reduce;
   `illumination`      -- flicker_model="illumination": flk_illum_apply_s2d in front of flk_net_forward, flk_illum_grad_reduce;
   `additive_q` / `illumination_q` -- the same two with quantise_train (the 8-bit round trip inside the apply).
2. One launch of each model's apply (fold_t 4, bf16, plain and quantised), export and gradient on the step's shapes, `--reps` launches
   between one HIP-event pair, the median of `--rounds` such groups.
3. `additive` against the PARENT commit (`--parent-root PATH`: a checkout of the parent with its library built): the same launches, so
   the trees only have to agree inside the run's spread.  Each tree is timed in processes of its own, alternating `--rounds` times; the
   spread is the range of one tree's per-process medians.

Prints one JSON line per leg and a summary line.  Needs the GPU; there is no fallback.

    python tools/illumination_time.py [--steps 40] [--warmup 8] [--rounds 2] [--reps 50] [--parent-root PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, HW = 16, 16, 112


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def worker(a):
    """one process: the engines of the tree `--root`, timed step by step; the JSON result on the last line of stdout"""
    sys.path.insert(0, a.root)
    import torch
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    assert torch.cuda.is_available(), "illumination_time needs the GPU"
    W = vs.synthetic_weights("mc3_18", 42)
    x = torch.from_numpy(vs.synthetic_clip_u8(B, T, HW, HW, seed=7)).cuda()
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=False)
    legs = {}
    for leg in a.legs.split(","):
        kw = dict(quantise_train=leg.endswith("_q"))
        if leg.startswith("illumination"):
            kw["flicker_model"] = "illumination"
        legs[leg] = FlickerVideoResNet("mc3_18", W, batch_size=B, sample_length=T, image_size=HW, dtype="bf16", l_inf_pert_norm=0.1, **kw)
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
    out = {leg: stats(v) for leg, v in ms.items()}
    if a.launches:
        out.update(launches(a, x, legs["illumination"], torch))
    print(json.dumps({"root": a.root, "legs": out}), flush=True)


def launches(a, x, eng, torch):
    """single launches of both models on the step's shapes: `reps` launches between one event pair, per-launch milliseconds"""
    from flickering_adversarial_video_amd import ops
    pm = eng.pert_model
    pm.perturbation.uniform_(-0.1, 0.1)
    il = pm.illum
    xs, gx = eng._xs, torch.randn_like(eng._gx)
    frames = torch.empty_like(x)
    gd = torch.empty((T, 3), dtype=torch.float32, device=x.device)
    plain, quant = pm.apply_args(x, True, fold_t=4), pm.apply_args(x, True, fold_t=4, quantise=True)
    exp = pm.export_args(x, True)
    calls = {"apply_additive": lambda: ops.perturb_apply_s2d(plain, torch.bfloat16, out=xs),
             "apply_illumination": lambda: ops.illum_apply_s2d(plain, il, torch.bfloat16, out=xs),
             "apply_q_additive": lambda: ops.perturb_apply_s2d(quant, torch.bfloat16, out=xs),
             "apply_q_illumination": lambda: ops.illum_apply_s2d(quant, il, torch.bfloat16, out=xs),
             "export_additive": lambda: ops.export_adversarial_u8(exp, "torch", out=frames),
             "export_illumination": lambda: ops.illum_export_u8(exp, il, out=frames),
             "grad_additive": lambda: ops.perturb_grad_reduce(plain, gx, gd, eng._scratch),
             "grad_illumination": lambda: ops.illum_grad_reduce(plain, il, gx, gd, eng._scratch)}
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
           "--reps", str(a.reps), "--rounds", str(a.rounds)] + (["--launches"] if with_launches else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({root}, {legs}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["legs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launches", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="additive,illumination,additive_q,illumination_q", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    same = run_worker(HERE, "additive,illumination,additive_q,illumination_q", a, with_launches=True)
    for leg, v in same.items():
        print(json.dumps({"what": "same build, one process", "leg": leg, **v}), flush=True)
    summary = {"illumination_minus_additive_ms": round(same["illumination"]["median_ms"] - same["additive"]["median_ms"], 4),
               "illumination_over_additive": round(same["illumination"]["median_ms"] / same["additive"]["median_ms"], 4),
               "illumination_q_over_additive_q": round(same["illumination_q"]["median_ms"] / same["additive_q"]["median_ms"], 4)}
    for k in ("apply", "apply_q", "export", "grad"):
        summary[f"{k}_illumination_over_additive"] = round(same[f"{k}_illumination"]["median_ms"] / same[f"{k}_additive"]["median_ms"], 3)
    if a.parent_root:
        med = {"this": [], "parent": []}
        for k in range(a.rounds):                           # the two trees alternate, a process each; who goes first alternates too
            for tree in (("parent", "this"), ("this", "parent"))[k % 2]:
                med[tree].append(run_worker(os.path.abspath(a.parent_root) if tree == "parent" else HERE, "additive", a)["additive"]["median_ms"])
        print(json.dumps({"what": "additive step, a process per tree and round", **{f"{t}_median_ms": v for t, v in med.items()}}), flush=True)
        for tree, v in med.items():
            summary[f"additive_{tree}_ms"] = round(statistics.median(v), 4)
            summary[f"additive_{tree}_spread_ms"] = round(max(v) - min(v), 4)
    else:
        summary.update(parent="not measured")
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
