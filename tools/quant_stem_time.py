#!/usr/bin/env python3
"""What training the I3D attack on the stored video costs (flk_apply_args.q_lut on the I3D plan: the QUANT instantiation of the uint8
stem, csrc/stem_fwd.hip; FlickerI3D(quantise_train=True)), at the benchmark geometry: 8 clips x 64 x 224 x 224, bf16, uint8 clips.

(a) one plain uint8 stem launch on a half batch (4 clips: what the plan launches per stream), centred clip + position-class table;
(b) the QUANT launch on the same half batch (stored byte staged itself, no table).
    Arguments and output built once; a HIP-event pair brackets 10 back-to-back launches through the C ABI; the two legs alternate group
    by group; median / min / max per launch over --launches groups after a warm-up.
(c) the attack step, plain;  (d) the step with quantise_train.
    ONE engine, the attribute flipped between alternating steps, a HIP-event pair around each step; --steps per leg after a warm-up.
(e) the quantise_train step on the fallback route -- FLK_STEM_U8=0: the quantised apply writes the space-to-depth tensor and the folded
    stem reads it -- in a FRESH child process (the switch is the child's environment), with the plain step of that route (centred apply
    + folded stem) beside it as that process's own yardstick.  (d) against (e) is what staging the byte inside the stem saves.

--tree PATH times the package of another checkout with this same tool (the parent commit: plain legs only); --plain-only runs the plain
step back to back in either tree, the like-for-like pair (in (c) the plain steps alternate with quantised ones).  One JSON line.

    python tools/quant_stem_time.py [--launches 30] [--steps 30] [--tree PATH] [--no-fallback] [--plain-only]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2), "n": len(ms)}


def step_legs(torch, np, i3d_spec, FlickerI3D, has_q, steps, B, T, plain_only=False):
    """plain and quantise_train steps of one engine, alternating (plain_only: plain steps back to back, as a package without the option runs
    them -- the like-for-like figure against --tree PARENT)"""
    eng = FlickerI3D(i3d_spec.synthetic_i3d_weights(42), batch_size=B, frames=T, dtype="bf16")
    x = torch.from_numpy(i3d_spec.synthetic_clip_u8(B, T, seed=1234)).cuda()
    lab = eng.logits(x, 0.0, 0).argmax(-1).clone()
    eng.reset_perturbation(np.random.default_rng(3).uniform(-0.05, 0.05, (T, 3)).astype(np.float32))
    legs = {"plain": False, "quantise_train": True} if has_q and not plain_only else {"plain": False}

    def step(q):
        if has_q:
            eng.quantise_train = q
        eng.step(x, lab, lr=1e-3)
    for _ in range(5):
        for q in legs.values():
            step(q)
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(steps):
        for k, q in legs.items():
            ms[k].append(timed(torch, lambda: step(q)))
    r = {k: summary(v) for k, v in ms.items()}
    if "quantise_train" in r:
        r["quantise_train_over_plain"] = round(r["quantise_train"]["median_us"] / r["plain"]["median_us"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=30, help="timed steps per leg")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package is timed")
    ap.add_argument("--no-fallback", action="store_true", help="skip (e), the child process with FLK_STEM_U8=0")
    ap.add_argument("--steps-only", action="store_true", help="the step legs only (what the child process of (e) runs)")
    ap.add_argument("--plain-only", action="store_true", help="the plain step only, back to back, and no stem launches: the figure to hold "
                    "against the same flag on --tree PARENT")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import inspect
    import numpy as np
    import torch
    from flickering_adversarial_video_amd import i3d_spec, ops
    from flickering_adversarial_video_amd.i3d_engine import FlickerI3D
    if not torch.cuda.is_available():
        raise SystemExit("quant_stem_time.py needs a GPU: a CPU run gives no time")
    has_q = "quantise_train" in inspect.signature(FlickerI3D.__init__).parameters
    B, T = a.batch, a.frames
    res = {"tree": os.path.abspath(a.tree), "has_quantise_train": has_q, "geometry": [B, T, 224, 224], "FLK_STEM_U8": os.environ.get("FLK_STEM_U8")}
    if not a.steps_only and not a.plain_only:
        Bh = max(B // 2, 1)
        W = i3d_spec.synthetic_i3d_weights(42)
        w7 = W[i3d_spec.PREFIX + "Conv3d_1a_7x7/conv_3d/w"]
        rng = np.random.default_rng(0)
        scale = torch.from_numpy(rng.uniform(0.5, 1.5, 64).astype(np.float32)).cuda()
        bias = torch.from_numpy(rng.uniform(-0.3, 0.3, 64).astype(np.float32)).cuda()
        x = torch.from_numpy(i3d_spec.synthetic_clip_u8(Bh, T, seed=1)).cuda()
        delta = torch.from_numpy(rng.uniform(-0.05, 0.05, (T, 3)).astype(np.float32)).cuda()
        wts = ops.StemFwdU8Weights(w7)
        out = torch.empty((Bh, T // 2, 112, 112, 64), dtype=torch.bfloat16, device="cuda")
        plain = ops.make_apply_args(x, delta, fold_t=ops.I3D_FOLD, center=True)
        tab = ops.stem_delta_bias_table(plain, w7, scale.cpu().numpy())
        calls = {"plain": (plain, tab)}
        if has_q:
            calls["quant"] = (ops.make_apply_args(x, delta, fold_t=ops.I3D_FOLD, quantise="tf", center=False), None)
        lib, sp = ops.load(), ops.stream_ptr()

        def ten(k):
            args, pb = calls[k]
            for _ in range(10):
                ops.check(lib.flk_stem_fwd_u8(C.byref(args), wts.handle, ops.ptr(scale), ops.ptr(bias), ops.ptr(pb), 0, ops.ptr(out), 64, sp))
        for _ in range(3):
            for k in calls:
                ten(k)
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(a.launches):
            for k in calls:
                ms[k].append(timed(torch, lambda: ten(k)) / 10)
        r = {k: summary(v) for k, v in ms.items()}
        if has_q:
            r["quant_over_plain"] = round(r["quant"]["median_us"] / r["plain"]["median_us"], 4)
        res[f"stem_launch_half_batch_{Bh}x{T}"] = r
        del x, out, calls
    res["step"] = step_legs(torch, np, i3d_spec, FlickerI3D, has_q, a.steps, B, T, a.plain_only)
    if has_q and not a.no_fallback and not a.steps_only and not a.plain_only:
        # (e): a fresh process, the switch in ITS environment (the plan reads it per call; nothing of this process is reused)
        env = dict(os.environ, FLK_STEM_U8="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--steps-only", "--steps", str(a.steps), "--tree", a.tree, "--batch", str(B), "--frames", str(T)]
        child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            raise SystemExit("the FLK_STEM_U8=0 child failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        res["step_fallback_FLK_STEM_U8_0"] = json.loads(child.stdout.strip().splitlines()[-1])["step"]
        d, e = res["step"]["quantise_train"]["median_us"], res["step_fallback_FLK_STEM_U8_0"]["quantise_train"]["median_us"]
        res["in_stem_over_fallback"] = round(d / e, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
