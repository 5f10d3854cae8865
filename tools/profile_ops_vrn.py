#!/usr/bin/env python3
"""Per-layer timing of one VideoResNet attack iteration (HIP events around every launch of the plan): batched single-video attacks.
--u8: the clip is the resident uint8 frames (decoded by the apply kernel) instead of the normalised fp32 clip.  The apply runs inside
the stem's row of the plan; it is also timed alone (same launch, same arguments) and printed as the "apply" line."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from flickering_adversarial_video_amd import videoresnet_spec as vs
from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="r2plus1d_18", choices=vs.ARCHS); ap.add_argument("--batch", type=int, default=8); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--frames", type=int, default=None, help="clip length (default 16; r2plus1d_34: 32, the IG65M / Kinetics 32-frame models)")
ap.add_argument("--u8", action="store_true", help="attack the uint8 frames (device decode) instead of the host-normalised fp32 clip")
a = ap.parse_args()
T = a.frames or (32 if a.arch == "r2plus1d_34" else 16)
W = vs.synthetic_weights(a.arch, 42)
eng = FlickerVideoResNet(a.arch, W, batch_size=a.batch, sample_length=T, image_size=112, dtype="bf16", per_clip=a.batch > 1)
x = torch.from_numpy(vs.synthetic_clip_u8(a.batch, T, seed=1234) if a.u8 else vs.synthetic_clip(a.batch, T, seed=1234)).cuda()
lab = eng.logits(x).argmax(-1).clone()
crit = Losses(beta_1=0.5, lambda_=1.0, margin=0.05, improve_loss=True, logits=True)
for _ in range(2): eng.step(x, lab, crit)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
for _ in range(a.reps): eng.step(x, lab, crit)
ev[1].record(); torch.cuda.synchronize()
step_ms = ev[0].elapsed_time(ev[1]) / a.reps
eng.net.profile(True)
acc = {}
for _ in range(a.reps):
    eng.step(x, lab, crit)
    for i, r in enumerate(eng.net.profile_read()):
        k = (i, r["name"], r["pass"], r.get("kernel", ""))
        e = acc.setdefault(k, dict(ms=0.0, flops=r["flops"], bytes=r["bytes"]))
        e["ms"] += r["ms"] / a.reps
tot = sum(v["ms"] for v in acc.values())
print(f"{'op':44s} {'pass':4s} {'ms':>8s} {'%':>6s} {'TFLOP/s':>9s} {'GB/s':>8s}  kernel")
for k, v in sorted(acc.items(), key=lambda kv: -kv[1]["ms"]):
    print(f"{k[1][:44]:44s} {k[2]:4s} {v['ms']:8.3f} {100*v['ms']/tot:6.1f} {v['flops']/v['ms']/1e9 if v['flops'] else 0:9.1f} {v['bytes']/v['ms']/1e6 if v['bytes'] else 0:8.0f}  {k[3].replace('_kernel','')}")
print("total ms", tot)
eng.net.profile(False)
from flickering_adversarial_video_amd import ops
args = eng.pert_model.apply_args(x, True, fold_t=eng.net.input_fold)
for _ in range(3): ops.perturb_apply_s2d(args, eng._xs.dtype, out=eng._xs)
n_apply = 20 * a.reps
ev[0].record()
for _ in range(n_apply): ops.perturb_apply_s2d(args, eng._xs.dtype, out=eng._xs)
ev[1].record(); torch.cuda.synchronize()
apply_ms = ev[0].elapsed_time(ev[1]) / n_apply
nbytes = x.numel() * x.element_size() + eng._xs.numel() * eng._xs.element_size()
print(f"apply ms {apply_ms:.4f} ({'uint8' if a.u8 else 'fp32'} clip, fold_t {eng.net.input_fold}, {nbytes / apply_ms / 1e6:.0f} GB/s, alone, back to back)")
print(f"step ms {step_ms:.3f} (arch {a.arch}, bs {a.batch}, T {T}, {'uint8' if a.u8 else 'fp32'} clip, profiling off)")
