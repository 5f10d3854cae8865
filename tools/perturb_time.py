#!/usr/bin/env python3
"""Isolated timing of the perturbation kernels (csrc/attack.hip, csrc/illum.hip and the perturbation side of csrc/stem_grad.hip /
csrc/stem_fwd.hip) at the sizes users run, and the SHA-256 of everything each of them writes on seeded inputs.

Legs (`--reps` launches between one HIP-event pair, `--groups` pairs, per-launch microseconds; `_q`: with the 8-bit round trip q_lut):
  VideoResNet, torch dialect, 16 x 16 x 112 x 112
    vrn_apply_f1_f32[_q]          apply_s2d_kernel<float, S2D<1>>: fold 1, fp32 from an fp32 clip
    vrn_apply_f1_u8[_q]           the same kernel from the uint8 clip through its decode table
    vrn_apply_f4_f32[_q]          apply_s2d_kernel<bf16, HiLo>: fold 4 from an fp32 clip
    vrn_apply_f4_u8[_q]           apply_s2d_u8x4_kernel<bf16, HiLo, table>: fold 4 from the uint8 clip, flicker [T,3]
    vrn_apply_f4_u8_dense[_q]     the same, dense [T,H,W,3]
    vrn_apply_f4_u8_lines[_q]     the same, per line [B,T,H,3]
    vrn_grad_f1 / vrn_grad_f1_per_clip    grad_reduce_stage1 + stage2, fold 1, bf16 gradient; shared [T,3] and per clip [B,T,3]
    vrn_grad_dense / vrn_grad_lines       grad_dense_kernel / grad_lines_kernel, bf16 gradient
    vrn_export_u8[_stats] / vrn_export_f32[_stats]   adv_export_u8_kernel from the uint8 and from the fp32 clip
    illum_export_stats / illum_grad / illum_grad_lines   illum_export_kernel<true>, illum_grad_stage1 + stage2, illum_grad_lines_kernel
  I3D, TF dialect, 8 x 64 x 224 x 224
    i3d_apply_f2_u8 / i3d_apply_f3_u8     apply_s2d_u8x4_kernel<bf16, S2D<2|3>>: the uint8 clip to bf16
    i3d_apply_f2_f32                      apply_s2d_kernel<bf16, S2D<2>> from an fp32 clip
    i3d_grad_f2 / i3d_grad_f3             grad_reduce_stage1 + stage2, bf16 gradient
    i3d_stem_mask                         flk_stem_delta_grad_mask (stem_mask_kernel)
    i3d_stem_fwd / i3d_stem_fwd_q         flk_stem_fwd_u8, centred with its position bias / quantised

With `--parent-root PATH` (a checkout of the parent commit with its library built) the legs run in a process per tree and round, the trees
alternating and who goes first alternating too; per leg the hashes of the two trees must be equal (every kernel here has one fixed
summation order), and this tree's median of per-process medians is held to the parent's maximum plus the parent's spread (max - min over
its rounds).  Exit status 1 when a leg misses either.  Every worker process runs under `--timeout` seconds; nothing is started after a
worker that fails or times out.  Needs the GPU; there is no fallback.

    python tools/perturb_time.py [--legs a,b] [--reps 10] [--groups 5] [--parent-root PATH --rounds 4] [--timeout 300]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VRN, I3D = (16, 16, 112, 112), (8, 64, 224, 224)
ALL = ",".join([f"vrn_apply_{k}{q}" for k in ("f1_f32", "f1_u8", "f4_f32", "f4_u8", "f4_u8_dense", "f4_u8_lines") for q in ("", "_q")]
               + ["vrn_grad_f1", "vrn_grad_f1_per_clip", "vrn_grad_dense", "vrn_grad_lines", "vrn_export_u8", "vrn_export_u8_stats", "vrn_export_f32",
                  "vrn_export_f32_stats", "illum_export_stats", "illum_grad", "illum_grad_lines", "i3d_apply_f2_u8", "i3d_apply_f3_u8", "i3d_apply_f2_f32",
                  "i3d_grad_f2", "i3d_grad_f3", "i3d_stem_mask", "i3d_stem_fwd", "i3d_stem_fwd_q"])


def make_leg(name, torch, np, ops):
    """call: inputs seeded per geometry, call() launches once and returns the tensors it wrote"""
    from flickering_adversarial_video_amd import i3d_spec, videoresnet_spec as vs
    from oracle import attack_math as am
    bf, f32 = torch.bfloat16, torch.float32
    i3d = name.startswith("i3d_")
    B, T, H, W = I3D if i3d else VRN
    gen = torch.Generator(device="cuda").manual_seed(224 if i3d else 112)

    def uniform(shape, r):
        return (torch.rand(shape, device="cuda", generator=gen) * 2 - 1) * r

    xu = torch.randint(0, 256, (B, T, H, W, 3), device="cuda", generator=gen, dtype=torch.uint8)
    d = uniform((T, 3), 0.15).contiguous()                   # (the clamp bound is 0.1: a third of the rows sit at it)
    quant = name.endswith("_q")
    if i3d:
        kw = dict(dclip=0.1)
        if name.startswith("i3d_apply"):
            fold_t = 3 if "_f3_" in name else 2
            x = (xu.float() / 128 - 1).contiguous() if name.endswith("_f32") else xu
            args = ops.make_apply_args(x, d, fold_t=fold_t, **kw)
            out = torch.empty((B, T // 2, H // 2, W // 2, 32), dtype=bf, device="cuda")
            return lambda: (ops.perturb_apply_s2d(args, bf, out=out),)
        if name.startswith("i3d_grad"):
            args = ops.make_apply_args(xu, d, fold_t=3 if name.endswith("f3") else 2, **kw)
            gx = torch.randn((B, T // 2, H // 2, W // 2, 32), device="cuda", generator=gen).to(bf)
            return lambda: (ops.perturb_grad_reduce(args, gx),)
        if name == "i3d_stem_mask":
            args = ops.make_apply_args(xu, d, fold_t=ops.I3D_FOLD, center=True, **kw)
            lib = ops.load()
            scratch = torch.zeros(max(1, lib.flk_stem_delta_grad_scratch_bytes(B, T, H) // 4), dtype=f32, device="cuda")

            def mask():
                ops.check(lib.flk_stem_delta_grad_mask(C.byref(args), ops.ptr(scratch), ops.stream_ptr()))
                return (scratch,)
            return mask
        w7 = i3d_spec.synthetic_i3d_weights(42)[i3d_spec.PREFIX + "Conv3d_1a_7x7/conv_3d/w"]
        rng = np.random.default_rng(0)
        scale = torch.from_numpy(rng.uniform(0.5, 1.5, 64).astype(np.float32)).cuda()
        bias = torch.from_numpy(rng.uniform(-0.3, 0.3, 64).astype(np.float32)).cuda()
        wts = ops.StemFwdU8Weights(w7)
        out = torch.empty((B, T // 2, 112, 112, 64), dtype=bf, device="cuda")
        if quant:
            args, tab = ops.make_apply_args(xu, d, fold_t=ops.I3D_FOLD, quantise="tf", center=False, **kw), None
        else:
            args = ops.make_apply_args(xu, d, fold_t=ops.I3D_FOLD, center=True, **kw)
            tab = ops.stem_delta_bias_table(args, w7, scale.cpu().numpy())
        return lambda: (ops.stem_fwd_u8(args, wts, scale, bias, pos_bias=tab, out=out),)

    lut = torch.from_numpy(vs.u8_decode_table()).cuda()
    kw = dict(dclip=0.1, dialect="torch", inv_std=tuple(1.0 / s for s in am.DEFAULT_STD), lo=am.TORCH_MIN_VALUE, hi=am.TORCH_MAX_VALUE)
    xf = lut[xu.long(), torch.arange(3, device="cuda")].contiguous()
    dd, dl = uniform((T, H, W, 3), 0.15).contiguous(), uniform((B, T, H, 3), 0.15).contiguous()
    dpc = uniform((B, T, 3), 0.15).contiguous()
    form = {"dense": (dd, {}), "lines": (dl, dict(per_line=True)), "per_clip": (dpc, {})}
    delta, extra = next((v for k, v in form.items() if k in name), (d, {}))
    if name.startswith("vrn_apply"):
        fold_t, dt = (1, f32) if "_f1_" in name else (4, bf)
        src = dict(x_lut=lut) if "_u8" in name else {}
        args = ops.make_apply_args(xu if src else xf, delta, fold_t=fold_t, quantise="torch" if quant else None, **src, **extra, **kw)
        out = torch.empty((B, T, H // 2, W // 2, 32 if fold_t == 4 else 16), dtype=dt, device="cuda")
        return lambda: (ops.perturb_apply_s2d(args, dt, out=out),)
    if name.startswith("vrn_grad"):
        args = ops.make_apply_args(xu, delta, fold_t=4 if "lines" in name else 1, x_lut=lut, **extra, **kw)
        gx = torch.randn((B, T, H // 2, W // 2, 16), device="cuda", generator=gen).to(bf)
        return lambda: (ops.perturb_grad_reduce(args, gx),)
    if name.startswith("vrn_export"):
        src = dict(x_lut=lut) if "_u8" in name else {}
        args = ops.make_export_apply_args(xu if src else xf, d, **src, **kw)
        frames, stats = torch.empty_like(xu), name.endswith("_stats")

        def export():
            r = ops.export_adversarial_u8(args, "torch", out=frames, stats=stats)
            return r if stats else (r,)
        return export
    il = ops.make_illum_args(vs.illum_tables())
    ikw = dict(kw, x_lut=lut)
    if name == "illum_export_stats":
        args, frames = ops.make_export_apply_args(xu, d, **ikw), torch.empty_like(xu)
        return lambda: ops.illum_export_u8(args, il, out=frames, stats=True)
    if name in ("illum_grad", "illum_grad_lines"):
        lines = name.endswith("lines")
        args = ops.make_apply_args(xu, dl if lines else d, fold_t=4, per_line=lines, **ikw)
        gx = torch.randn((B, T, H // 2, W // 2, 16), device="cuda", generator=gen).to(bf)
        return lambda: (ops.illum_grad_reduce(args, il, gx),)
    raise SystemExit(f"unknown leg {name!r}; legs: {ALL}")


def worker(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from flickering_adversarial_video_amd import ops
    assert torch.cuda.is_available(), "perturb_time needs the GPU"
    out = {}
    for name in a.legs.split(","):
        call = make_leg(name, torch, np, ops)
        for _ in range(3):
            res = call()
        torch.cuda.synchronize()
        sha = hashlib.sha256()
        for t in res:
            sha.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        us = []
        for _ in range(a.groups):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()                                      # (outputs are reused or come from torch's cache: no device call)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / a.reps * 1e3)
        out[name] = {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "sha256": sha.hexdigest()}
        del call, res
        torch.cuda.empty_cache()
    print(json.dumps({"root": a.root, "legs": out}), flush=True)


def run_worker(root, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--legs", a.legs, "--reps", str(a.reps), "--groups", str(a.groups)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)       # (a worker that hangs ends the run: nothing is started after it)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({root}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["legs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=ALL)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a worker process may take")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root:
        for name, v in run_worker(HERE, a).items():
            print(json.dumps({"leg": name, **v}), flush=True)
        return 0
    runs = {"this": [], "parent": []}
    for k in range(a.rounds):                               # the two trees alternate, a process each; who goes first alternates too
        for tree in (("parent", "this"), ("this", "parent"))[k % 2]:
            runs[tree].append(run_worker(os.path.abspath(a.parent_root) if tree == "parent" else HERE, a))
    bad = 0
    for name in a.legs.split(","):
        med = {t: [r[name]["median_us"] for r in v] for t, v in runs.items()}
        hashes = {t: sorted({r[name]["sha256"] for r in v}) for t, v in runs.items()}
        bound = max(med["parent"]) + (max(med["parent"]) - min(med["parent"]))
        this = statistics.median(med["this"])
        same, within = hashes["this"] == hashes["parent"] and len(hashes["this"]) == 1, this <= bound
        bad += not (same and within)
        print(json.dumps({"leg": name, "this_us": med["this"], "parent_us": med["parent"], "this_median_us": round(this, 2),
                          "parent_median_us": round(statistics.median(med["parent"]), 2), "bound_us": round(bound, 2), "within": within,
                          "same_bits": same, "sha256": hashes["this"][0][:16]}), flush=True)
    print(json.dumps({"summary": {"legs": len(a.legs.split(",")), "missed": bad}}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
