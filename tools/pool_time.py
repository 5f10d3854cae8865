#!/usr/bin/env python3
"""Isolated timing of the max-pool kernels (csrc/pool.hip) at the geometries of the benchmark's I3D blocks (B = 8, 64 frames of 224 x 224),
and the SHA-256 of what each of them writes on seeded inputs.

Legs (bf16 unless named f32; `--reps` launches between one HIP-event pair, `--groups` pairs, per-launch microseconds):
  wrun_w7 / wrun_w8    the W-run forward (3x3x3 / 1) at W % 7 == 0 (Mixed_3c: 8 x 32 x 28 x 28 x 256) and at W % 7 != 0 (W = 30)
  fwd_k_133 / owner_133  maxpool_fwd_kernel_k and the owner backward, MaxPool3d_3a (1x3x3 / 1,2,2 over 8 x 32 x 56 x 56 x 192)
  fwd_k_333 / owner_333  the same for MaxPool3d_4a (3x3x3 / 2 over 8 x 32 x 28 x 28 x 480)
  scatter_333          maxpool_scatter_bwd, 3x3x3 / 1 (Mixed_3c)
  gemm_reg_k64 / gemm_reg_k128 / gemm_loop_k64
                       the fused Branch_3 backward (flk_maxpool3d_bwd_gemm): register form at Mixed_3c (K = 64) and Mixed_4f
                       (8 x 16 x 14 x 14 x 528, K = 128), loop form (FLK_POOL_GEMM_REG=0) at Mixed_3c
  conv_fwd / conv_bwd  the fused MaxPool3d_2a + Conv3d_2b kernels (8 x 32 x 112 x 112 x 64)
  f32_tiled_fwd / f32_tiled_bwd / f32_gather_bwd
                       the parity mode: LDS-tiled 3x3x3 / 1 forward and backward, gather backward (3x3x3 / 1,2,2), 2 x 8 x 28 x 28 x 64
Environment: GEO (B,T,H,W), C and K move the wrun_w7 and gemm_* legs off Mixed_3c; FLK_PF_DBG / FLK_PG_DBG reach a timing build of the
library (FLK_HIPCC_EXTRA=-DFLK_ABLATE python -m flickering_adversarial_video_amd.build --force: wrong results, the product build has no
such switch); FLK_POOL_GEMM_REG=0 turns the gemm_reg_* legs into the loop form as well.

With `--parent-root PATH` (a checkout of the parent commit with its library built) the legs run in a process per tree and round, the trees
alternating and who goes first alternating too; per leg the hashes of the two trees must be equal (the fixed-point forms are
order-independent, the fp32 forms have a fixed order), and this tree's median of per-process medians is held to the parent's maximum
plus the parent's spread (max - min over its rounds).  Exit status 1 when a leg misses either.  Every worker process runs under
`--timeout` seconds.  Needs the GPU; there is no fallback.

    python tools/pool_time.py [--legs a,b] [--reps 20] [--groups 5] [--parent-root PATH --rounds 4] [--timeout 240]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = [int(v) for v in os.environ.get("GEO", "8,32,28,28").split(",")]
C_, K_ = int(os.environ.get("C", 256)), int(os.environ.get("K", 64))
ALL = ("wrun_w7,wrun_w8,fwd_k_133,owner_133,fwd_k_333,owner_333,scatter_333,gemm_reg_k64,gemm_reg_k128,gemm_loop_k64,conv_fwd,conv_bwd,"
       "f32_tiled_fwd,f32_tiled_bwd,f32_gather_bwd")


def make_leg(name, torch, np, ops):
    """(call, outputs, a line of the two earlier tools or None): inputs seeded per leg, call() launches once and returns what it wrote"""
    bf, f32 = torch.bfloat16, torch.float32
    gen = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))

    def randn(shape, dtype, scale=1.0):
        return (torch.randn(shape, device="cuda", generator=gen) * scale).to(dtype)

    def pooled(shape, k, s, dtype=bf):
        x = torch.relu(randn(shape, dtype))
        out, idx, ctx = ops.maxpool3d(x, k, s)
        return x, out, idx, ctx

    if name in ("wrun_w7", "wrun_w8", "fwd_k_133", "fwd_k_333", "f32_tiled_fwd"):
        shape, k, s, dtype = {"wrun_w7": ((*GEO, C_), (3, 3, 3), (1, 1, 1), bf), "wrun_w8": ((8, 32, 28, 30, 256), (3, 3, 3), (1, 1, 1), bf),
                              "fwd_k_133": ((8, 32, 56, 56, 192), (1, 3, 3), (1, 2, 2), bf), "fwd_k_333": ((8, 32, 28, 28, 480), (3, 3, 3), (2, 2, 2), bf),
                              "f32_tiled_fwd": ((2, 8, 28, 28, 64), (3, 3, 3), (1, 1, 1), f32)}[name]
        x = torch.relu(randn(shape, dtype))
        line = None
        if name == "wrun_w7":
            B, T, H, W = GEO
            line = lambda ms: (f"{B}x{T}x{H}x{W} C={C_} FLK_PF_DBG={os.environ.get('FLK_PF_DBG', '0')}: {ms * 1e3:.1f} us  "
                               f"({B * T * H * W * C_ * 5 / ms / 1e6:.0f} GB/s: in + out + index bytes)")
        return (lambda: ops.maxpool3d(x, k, s)[:2]), line
    if name in ("owner_133", "owner_333", "scatter_333", "f32_tiled_bwd", "f32_gather_bwd"):
        shape, k, s, dtype = {"owner_133": ((8, 32, 56, 56, 192), (1, 3, 3), (1, 2, 2), bf), "owner_333": ((8, 32, 28, 28, 480), (3, 3, 3), (2, 2, 2), bf),
                              "scatter_333": ((8, 32, 28, 28, 256), (3, 3, 3), (1, 1, 1), bf), "f32_tiled_bwd": ((2, 8, 28, 28, 64), (3, 3, 3), (1, 1, 1), f32),
                              "f32_gather_bwd": ((2, 8, 28, 28, 64), (3, 3, 3), (1, 2, 2), f32)}[name]
        x, out, idx, ctx = pooled(shape, k, s, dtype)
        g = randn(tuple(out.shape), dtype, 0.01)
        return (lambda: (ops.maxpool3d_bwd(ctx, g, mask=x),)), None
    if name.startswith("gemm_"):
        B, T, H, W, C, K = (8, 16, 14, 14, 528, 128) if name == "gemm_reg_k128" else (*GEO, C_, K_)
        x, out, idx, ctx = pooled((B, T, H, W, C), (3, 3, 3), (1, 1, 1))
        g = randn((B, T, H, W, K), bf, 0.01)
        wp = ops.PoolGemmWeights((np.random.default_rng(0).standard_normal((K, C)) * 0.1).astype(np.float32))
        reg = "0" if name == "gemm_loop_k64" else os.environ.get("FLK_POOL_GEMM_REG", "1")

        def call():
            os.environ["FLK_POOL_GEMM_REG"] = reg           # (the library reads it per call)
            return (ops.maxpool3d_bwd_gemm(ctx, g, wp),)
        line = lambda ms: (f"{B}x{T}x{H}x{W} C={C} K={K} FLK_PG_DBG={os.environ.get('FLK_PG_DBG', '0')} FLK_POOL_GEMM_REG={reg}: "
                           f"{ms * 1e3:.1f} us  ({B * T * H * W * (2 * K + C + 2 * C) / ms / 1e6:.0f} GB/s of compulsory bytes: g + idx + gin)")
        return call, (line if name == "gemm_reg_k64" else None)
    if name in ("conv_fwd", "conv_bwd"):
        rng = np.random.default_rng(7)
        w = (rng.standard_normal((1, 1, 1, 64, 64)) * 0.2).astype(np.float32)
        scale = rng.uniform(0.5, 1.5, 64).astype(np.float32)
        x = torch.relu(randn((8, 32, 112, 112, 64), bf))
        sc, bi = torch.from_numpy(scale).cuda(), torch.from_numpy(rng.standard_normal(64).astype(np.float32)).cuda()
        wf = ops.ConvWeights(w, bf, 4)
        if name == "conv_fwd":
            return (lambda: ops.maxpool3d_conv1x1(x, wf, scale=sc, bias=bi, relu=True)[:2]), None
        wb = ops.ConvWeights(w, bf, 4, row_scale=scale, transpose=True)
        out, idx, ctx = ops.maxpool3d_conv1x1(x, wf, scale=sc, bias=bi, relu=True)
        g = randn(tuple(out.shape), bf, 0.01)
        return (lambda: (ops.maxpool3d_bwd_conv1x1(ctx, g, wb),)), None
    raise SystemExit(f"unknown leg {name!r}; legs: {ALL}")


def worker(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from flickering_adversarial_video_amd import ops
    assert torch.cuda.is_available(), "pool_time needs the GPU"
    out = {}
    for name in a.legs.split(","):
        call, line = make_leg(name, torch, np, ops)
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
                call()                                      # (outputs come from torch's cache: no device call)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / a.reps * 1e3)
        out[name] = {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "sha256": sha.hexdigest()}
        if line:
            out[name]["line"] = line(statistics.median(us) / 1e3)
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a worker process may take")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root:
        for name, v in run_worker(HERE, a).items():
            if "line" in v:
                print(v.pop("line"), flush=True)
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
