#!/usr/bin/env python3
"""Timing of the 8-bit export of the adversarial clip (flk_adv_export_u8, csrc/attack.hip) against the route available without it.

1. one export launch at 16 x 16 x 112 x 112 (torch dialect) from a uint8 clip through the decode table and from an fp32 clip, and one at
   8 x 64 x 224 x 224 (TF dialect, uint8 clip): the arguments are built once, a HIP-event pair brackets 10 back-to-back launches (the
   figure is the tenth), median / min / max over N such groups (--launches, printed as n) after a warm-up.  `kernel` is the bare
   launch through the C ABI with arguments built once and a buffer allocated once; `kernel_with_stats` the same with the statistics
   table; `wrapper` is ops.export_adversarial_u8(args, out=buffer) itself, which builds flk_export_args on every call: what a caller
   sees, and the leg to hold against the torch route, which also builds its arguments (and allocates its tensors) on every call.
   GB/s of the compulsory bytes: source + output + delta.
2. the route without the kernel, in the same run, groups alternating with the kernel's: Perturbation.forward (torch dialect: the apply
   kernel's folded fp32 tensor, unfolded by a permute) or the statements of FlickerI3D.adversarial_inputs_rgb (TF dialect; the network itself is not built), followed by de-normalise,
   times levels, round, clamp and to(uint8) with torch on the device.  Its bytes equal the kernel's wherever the encode's float32
   roundings agree (torch fuses nothing here either); the tool reports how many bytes differ instead of asserting it.

    python tools/export_time.py [--launches 30]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from flickering_adversarial_video_amd import i3d_spec, ops, videoresnet_spec as vs
from flickering_adversarial_video_amd.torch_attack import Perturbation


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_us": round(statistics.median(ms) * 1e3, 3), "min_us": round(min(ms) * 1e3, 3), "max_us": round(max(ms) * 1e3, 3), "n": len(ms)}


def case(a, tag, x, delta, dialect, kernel_args, torch_route):
    """time the export launch of `kernel_args` (with and without statistics) and `torch_route` (a callable returning uint8 frames)"""
    B, T, H, W = x.shape[:4]
    out = torch.empty((B, T, H, W, 3), dtype=torch.uint8, device="cuda")
    st = torch.empty((B, T, 3, 4), dtype=torch.int32, device="cuda")
    e = ops.make_export_args(dialect, T * H * W * 3)
    lib, sp = ops.load(), ops.stream_ptr()

    def ten_kernel():
        for _ in range(10):
            ops.check(lib.flk_adv_export_u8(C.byref(kernel_args), C.byref(e), ops.ptr(out), None, sp))

    def ten_stats():
        for _ in range(10):
            ops.check(lib.flk_adv_export_u8(C.byref(kernel_args), C.byref(e), ops.ptr(out), ops.ptr(st), sp))

    def ten_torch():
        for _ in range(10):
            torch_route()

    def ten_wrapper():
        for _ in range(10):
            ops.export_adversarial_u8(kernel_args, dialect, out=out)

    legs = {"kernel": ten_kernel, "kernel_with_stats": ten_stats, "wrapper": ten_wrapper, "torch_route": ten_torch}
    ten_kernel()
    differ = int((torch_route() != out).sum())
    for _ in range(3):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.launches):
        for k, f in legs.items():
            ms[k].append(timed(f) / 10)
    nbytes = x.numel() * x.element_size() + out.numel() + delta.numel() * 4
    r = {k: summary(v) for k, v in ms.items()}
    r["compulsory_bytes"] = nbytes
    r["kernel_gb_per_s"] = round(nbytes / (r["kernel"]["median_us"] * 1e-6) / 1e9, 1)
    r["torch_route_gb_per_s_of_the_same_bytes"] = round(nbytes / (r["torch_route"]["median_us"] * 1e-6) / 1e9, 1)
    r["torch_route_over_kernel"] = round(r["torch_route"]["median_us"] / r["kernel"]["median_us"], 2)
    r["torch_route_over_wrapper"] = round(r["torch_route"]["median_us"] / r["wrapper"]["median_us"], 2)
    r["bytes_where_the_torch_route_differs"] = differ
    return tag, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("export_time.py needs a GPU: a CPU run gives no time")
    rng = np.random.default_rng(0)
    res = {}
    # torch dialect, 16 x 16 x 112 x 112
    B, T, HW = 16, 16, 112
    u8 = vs.synthetic_clip_u8(B, T, HW, HW, seed=1)
    pm = Perturbation((3, T, 1, 1), max_norm=0.2)
    pm.init_perturbation(rng.uniform(-0.2, 0.2, (3, T, 1, 1)).astype(np.float32))
    std = torch.tensor(vs.DEFAULT_STD, dtype=torch.float32, device="cuda")
    mean = torch.tensor(vs.DEFAULT_MEAN, dtype=torch.float32, device="cuda")
    for tag, x in (("u8_table_16x16x112x112", torch.from_numpy(u8).cuda()), ("fp32_16x16x112x112", torch.from_numpy(vs.normalize_u8(u8)).cuda())):
        def route(x=x):
            y = pm.forward([x, True])
            return ((y * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8)
        k, r = case(a, tag, x, pm.perturbation, "torch", pm.export_args(x, True), route)
        res[k] = r
    del x, route
    # TF dialect, 8 x 64 x 224 x 224: the route of the parent commit is the engine's adversarial_inputs_rgb (apply in fp32 + unfold)
    B, T = 8, 64
    xu = torch.from_numpy(i3d_spec.synthetic_clip_u8(B, T, seed=2)).cuda()
    eps = torch.from_numpy(rng.uniform(-0.3, 0.3, (T, 3)).astype(np.float32)).cuda()

    def tf_route():
        f = ops.perturb_apply_s2d(ops.make_apply_args(xu, eps, dialect="tf", dclip=0.4, adv_flag=1.0, fold_t=2), "f32")
        B_, T2, H2, W2 = f.shape[:4]
        y = f[..., :24].reshape(B_, T2, H2, W2, 2, 2, 2, 3).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B_, 2 * T2, 2 * H2, 2 * W2, 3).contiguous()
        return ((y + 1.0) * 128.0).round().clamp(0, 255).to(torch.uint8)
    k, r = case(a, "tf_u8_8x64x224x224", xu, eps, "tf", ops.make_export_apply_args(xu, eps, dialect="tf", dclip=0.4), tf_route)
    res[k] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
