#!/usr/bin/env python3
"""What the codec-aware backward costs (flk_clip_prepare_grad_image, flk_codec_grad).

1. The two new launches at 16 clips x 16 frames x 240 x 320, quality 75, both subsamplings, through the C ABI with arguments built
   once: `--reps` launches between one HIP-event pair, the median of the groups.  `grad_image` is the transpose of the evaluation
   resampling (bf16 input gradient, packed fp32 images); `codec_grad_<sub>_<mode>` the launch pair of flk_codec_grad with a tone and a
   frame table cutting the frames from `--frames`-frame videos; beside them `prepare_grad`, the launch pair of the identity route, and
   `codec_fwd_<sub>`, the forward codec launch of the same frames.
2. The mc3_18 batch-16 `step_videos` (bf16, 16 frames of 112 x 112, Adam, period 16, training transform, Codec(75, "420")) under
   codec_grad "identity", "ste" and "cubic", in one process, stepping alternately, a HIP-event pair around every step.
3. Against the PARENT commit (`--parent-root PATH`: a checkout of the parent with its library built): the identity step, and
   `bench.py --gpus 1`, a process per tree and round, alternating -- no launch of theirs changes, so the trees only have to agree inside
   the spread of the parent's own runs.

Prints one JSON line per leg and a summary line.  Needs the GPU; there is no fallback.

    python tools/codec_grad_time.py [--steps 30] [--warmup 6] [--rounds 2] [--reps 20] [--frames 300] [--bench-steps 20] [--parent-root PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, HW, P = 16, 16, 112, 16


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def worker(a):
    sys.path.insert(0, a.root)
    import torch
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses
    assert torch.cuda.is_available(), "codec_grad_time needs the GPU"
    W = vs.synthetic_weights("mc3_18", 42)
    gen = torch.Generator(device="cuda").manual_seed(7)
    videos = [torch.randint(0, 256, (a.frames, 240, 320, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(B)]
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=False)
    common = dict(batch_size=B, sample_length=T, image_size=HW, dtype="bf16", l_inf_pert_norm=0.1, flicker_time="video", flicker_period=P,
                  augment={"seed": 0}, sampling={"temporal_jitter": True, "random_shift": True, "seed": 0}, train_delivered=True,
                  codec=vs.Codec(75, "420"))
    legs = {leg: FlickerVideoResNet("mc3_18", W, **common, **({} if leg == "identity" else dict(codec_grad=leg))) for leg in a.legs.split(",")}
    first = next(iter(legs.values()))
    lab = first.logits(first.prepare_videos(videos, train=False), False).argmax(1).clone()
    ms = {leg: [] for leg in legs}
    for it in range(a.warmup + a.steps):
        for leg, eng in legs.items():                       # the legs alternate step by step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.step_videos(videos, lab, crit, lr=1e-3, train=True)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[leg].append(e0.elapsed_time(e1))
    out = {leg: stats(v) for leg, v in ms.items()}
    if a.launches:
        out.update(launches(a, videos, first, torch))
    print(json.dumps({"root": a.root, "legs": out}), flush=True)


def launches(a, videos, eng, torch):
    """single launches on 16 x 16 x 240 x 320: `reps` launches between one event pair, per-launch milliseconds"""
    import ctypes as C
    import numpy as np
    from flickering_adversarial_video_amd import _lib, ops, videoresnet_spec as vs
    from flickering_adversarial_video_amd._lib import ptr, stream_ptr
    lib = ops.load()
    rows = np.concatenate([vs.sample_frame_indices(a.frames, T, temporal_jitter=True, random_shift=True, rng=np.random.RandomState(0)) for _ in range(B)])
    pm = eng.pert_model
    pm.perturbation.uniform_(-0.1, 0.1)
    pm.set_frame_numbers(rows)
    ta = pm.export_args(ops.tone_ramp(B, T), True, shift_p=0)
    tone = ops.flicker_tone_tables(ta, None)
    slope, scale = ops.flicker_tone_slopes(ta, None)
    table = torch.from_numpy(rows.astype(np.int32)).cuda()
    gx = torch.randn((B, T, HW // 2, HW // 2, 16), device="cuda").to(torch.bfloat16)
    n_img = T * 240 * 320 * 3
    flat, g_clip = torch.empty(B * n_img, dtype=torch.float32, device="cuda"), torch.empty((B, T, 3), dtype=torch.float32, device="cuda")
    images = [flat[k * n_img:(k + 1) * n_img].view(T, 240, 320, 3) for k in range(B)]
    outs = [torch.empty((T, 240, 320, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    identity_rows = np.broadcast_to(np.arange(T), (B, T))
    calls = {"prepare_grad": lambda: ops.prepare_clips_grad(videos, gx, slope, scale, input_size=(HW, HW), frame_idx=rows, gdelta=g_clip)}
    # the image transpose with its tables built and uploaded once
    words, offsets, K = vs.prepare_adjoint_tables([(240, 320)] * B, input_size=(HW, HW))
    tab = torch.from_numpy(words).cuda()
    ic = (_lib.GradImageClip * B)()
    for d, o, (th, tw) in zip(ic, images, offsets):
        d.dst, d.pitch_t, d.pitch_h, d.Hs, d.Ws, d.tab_h, d.tab_w = o.data_ptr(), o.stride(0), o.stride(1), 240, 320, th, tw
    calls["grad_image"] = lambda: lib.flk_clip_prepare_grad_image(B, ic, T, HW, HW, K, ptr(tab), tab.numel(), ptr(gx), _lib.FLK_BF16, stream_ptr())
    calls["grad_image_wrapper"] = lambda: ops.prepare_clips_grad_image(videos, gx, input_size=(HW, HW), frame_idx=identity_rows, out=images)
    arr = (_lib.CodecClip * B)()
    for d, v, o in zip(arr, videos, outs):
        d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = v.data_ptr(), v.shape[0], 240, 320, v.stride(0), v.stride(1)
        d.dst, d.dst_pitch_t, d.dst_pitch_h = o.data_ptr(), o.stride(0), o.stride(1)
    keep = []
    for sub in vs.CODEC_SUBSAMPLINGS:
        ca = _lib.CodecArgs()
        ca.nclip, ca.quality, ca.subsampling, ca.clips = B, 75, int(sub), arr
        ws = torch.empty(lib.flk_codec_grad_scratch_bytes(C.byref(ca), T) // 4, dtype=torch.float32, device="cuda")
        keep.append((ca, ws))
        calls[f"codec_fwd_{sub}"] = lambda ca=ca: lib.flk_codec_roundtrip_u8(C.byref(ca), ptr(table), T, ptr(tone), None, stream_ptr())
        for mode, code in (("ste", _lib.FLK_CODEC_GRAD_STE), ("cubic", _lib.FLK_CODEC_GRAD_CUBIC)):
            calls[f"codec_grad_{sub}_{mode}"] = lambda ca=ca, ws=ws, code=code: lib.flk_codec_grad(
                C.byref(ca), ptr(table), T, ptr(tone), code, ptr(flat), ptr(slope), ptr(scale), ptr(g_clip), None, ptr(ws), stream_ptr())
    calls["codec_grad_wrapper_420_cubic"] = lambda: ops.codec_grad(videos, vs.Codec(75, "420"), flat, slope, scale, "cubic", frame_idx=rows, tone=tone,
                                                                   gdelta=g_clip)
    out = {}
    for name, call in calls.items():
        for _ in range(3):
            rc = call()
            assert not isinstance(rc, int) or rc == 0, (name, lib.flk_last_error())
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
           "--reps", str(a.reps), "--rounds", str(a.rounds), "--frames", str(a.frames)]
    cmd += ["--launches"] if with_launches else []
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({root}, {legs}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["legs"]


def run_bench(root, a):
    """bench.py of a tree: its one JSON result line"""
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "5"], capture_output=True,
                       text=True, cwd=root)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed ({root}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=300, help="frames of each of the 16 resident videos")
    ap.add_argument("--bench-steps", type=int, default=20, help="--steps of the bench.py runs against the parent")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launches", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="identity,ste,cubic", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    same = run_worker(HERE, "identity,ste,cubic", a, with_launches=True)
    for leg, v in same.items():
        print(json.dumps({"what": "same build, one process", "leg": leg, **v}), flush=True)
    summary = {f"{leg}_minus_identity_ms": round(same[leg]["median_ms"] - same["identity"]["median_ms"], 4) for leg in ("ste", "cubic")}
    for sub in ("444", "420"):
        summary[f"codec_grad_{sub}_cubic_over_codec_fwd"] = round(same[f"codec_grad_{sub}_cubic"]["median_ms"] / same[f"codec_fwd_{sub}"]["median_ms"], 2)
    summary["new_launches_420_cubic_minus_prepare_grad_ms"] = round(same["grad_image"]["median_ms"] + same["codec_grad_420_cubic"]["median_ms"]
                                                                    - same["prepare_grad"]["median_ms"], 4)
    if a.parent_root:
        parent = os.path.abspath(a.parent_root)
        step, bench = {"this": [], "parent": []}, {"this": [], "parent": []}
        for k in range(a.rounds):                           # the two trees alternate, a process each; who goes first alternates too
            for tree in (("parent", "this"), ("this", "parent"))[k % 2]:
                root = parent if tree == "parent" else HERE
                step[tree].append(run_worker(root, "identity", a)["identity"]["median_ms"])
                res = run_bench(root, a)
                bench[tree].append(res)
        key = next((k for k in ("step_ms", "ms_per_step", "median_step_ms", "value") if k in bench["this"][0]), None)
        print(json.dumps({"what": "identity step, a process per tree and round", **{f"{t}_median_ms": v for t, v in step.items()}}), flush=True)
        print(json.dumps({"what": "bench.py, a process per tree and round", "key": key, **{t: [r.get(key) for r in v] for t, v in bench.items()},
                          "result_keys": sorted(bench["this"][0])[:40]}), flush=True)
        for tree, v in step.items():
            summary[f"identity_{tree}_ms"] = round(statistics.median(v), 4)
            summary[f"identity_{tree}_spread_ms"] = round(max(v) - min(v), 4)
    else:
        summary.update(parent="not measured")
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
