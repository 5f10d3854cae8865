#!/usr/bin/env python3
"""What the codec round trip costs (csrc/codec.hip, flk_codec_roundtrip_u8).

1. Single launches at 16 clips x 16 frames x 240 x 320, `--reps` launches between one HIP-event pair, the median of the groups:
   the codec at 4:4:4 and 4:2:0 (quality 75) through the C ABI with arguments built once (`launch_*`: plain, with stats, with a
   tone table and a frame table cutting the frames from 300-frame videos) and once through ops.codec_roundtrip (`wrapper_*`: its host
   checks and the table upload included); beside a device copy of the same bytes (3 read + 3 written per pixel, as the codec
   moves) and the uint8 export of the same frames as one video (export_video).
2. The mc3_18 batch-16 `step_videos` (bf16, 16 frames of 112 x 112, Adam, period 16, training transform) with and without a codec,
   in one process, stepping alternately, a HIP-event pair around every step.
3. The no-codec step against the PARENT commit (`--parent-root PATH`: a checkout of the parent with its library built): the same
   launches, so the trees only have to agree inside the run's spread.  A process per tree and round, alternating.

Prints one JSON line per leg and a summary line.  Needs the GPU; there is no fallback.

    python tools/codec_time.py [--steps 30] [--warmup 6] [--rounds 2] [--reps 20] [--frames 300] [--parent-root PATH]"""
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
    assert torch.cuda.is_available(), "codec_time needs the GPU"
    W = vs.synthetic_weights("mc3_18", 42)
    gen = torch.Generator(device="cuda").manual_seed(7)
    videos = [torch.randint(0, 256, (a.frames, 240, 320, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(B)]
    crit = Losses(beta_1=0.5, lambda_=1.0, improve_loss=True, logits=False)
    common = dict(batch_size=B, sample_length=T, image_size=HW, dtype="bf16", l_inf_pert_norm=0.1, flicker_time="video", flicker_period=P,
                  augment={"seed": 0}, sampling={"temporal_jitter": True, "random_shift": True, "seed": 0}, train_delivered=True)
    legs = {}
    for leg in a.legs.split(","):
        kw = {} if leg == "delivered" else dict(codec=vs.Codec(75, leg.split("_")[1]))
        legs[leg] = FlickerVideoResNet("mc3_18", W, **common, **kw)
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
    import numpy as np
    from flickering_adversarial_video_amd import ops, videoresnet_spec as vs
    rows = np.concatenate([vs.sample_frame_indices(a.frames, T, temporal_jitter=True, random_shift=True, rng=np.random.RandomState(0)) for _ in range(B)])
    clips = [v[:T] for v in videos]
    outs = [torch.empty((T, 240, 320, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    pm = eng.pert_model
    pm.perturbation.uniform_(-0.1, 0.1)
    pm.set_frame_numbers(rows)
    tone = ops.flicker_tone_tables(pm.export_args(ops.tone_ramp(B, T), True, shift_p=0), None)
    batch = torch.cat(clips)                                # the same B * T frames as ONE video: what export_video takes
    eout = torch.empty_like(batch)
    calls = {"device_copy": lambda: eout.copy_(batch), "export_u8": lambda: eng.export_video(batch)}
    # the codec through the C ABI with arguments built once: the launch alone, none of the wrapper's host checks
    import ctypes as C
    from flickering_adversarial_video_amd import _lib
    from flickering_adversarial_video_amd._lib import ptr, stream_ptr
    lib = ops.load()
    table = torch.from_numpy(rows.astype(np.int32)).cuda()
    st = torch.empty((B, T, 2), dtype=torch.int32, device="cuda")

    def descriptors(srcs):
        arr = (_lib.CodecClip * B)()
        for d, v, o in zip(arr, srcs, outs):
            d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = v.data_ptr(), v.shape[0], 240, 320, v.stride(0), v.stride(1)
            d.dst, d.dst_pitch_t, d.dst_pitch_h = o.data_ptr(), o.stride(0), o.stride(1)
        return arr

    keep = {"clips": descriptors(clips), "videos": descriptors(videos)}
    for sub in vs.CODEC_SUBSAMPLINGS:
        args = {}
        for k, arr in keep.items():
            args[k] = _lib.CodecArgs()
            args[k].nclip, args[k].quality, args[k].subsampling, args[k].clips = B, 75, int(sub), arr
        calls[f"launch_{sub}"] = lambda a=args["clips"]: lib.flk_codec_roundtrip_u8(C.byref(a), None, T, None, None, stream_ptr())
        calls[f"launch_{sub}_stats"] = lambda a=args["clips"]: lib.flk_codec_roundtrip_u8(C.byref(a), None, T, None, ptr(st), stream_ptr())
        calls[f"launch_{sub}_tone_idx"] = lambda a=args["videos"]: lib.flk_codec_roundtrip_u8(C.byref(a), ptr(table), T, ptr(tone), None, stream_ptr())
        # and through ops.codec_roundtrip: its checks, descriptors and the table upload included
        calls[f"wrapper_{sub}_tone_idx"] = lambda codec=vs.Codec(75, sub): ops.codec_roundtrip(videos, codec, frame_idx=rows, tone=tone, out=outs)
    out = {}
    for name, call in calls.items():
        for _ in range(3):
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
           "--reps", str(a.reps), "--rounds", str(a.rounds), "--frames", str(a.frames)] + (["--launches"] if with_launches else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({root}, {legs}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["legs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=300, help="frames of each of the 16 resident videos")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launches", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="delivered,codec_420,codec_444", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    same = run_worker(HERE, "delivered,codec_420,codec_444", a, with_launches=True)
    for leg, v in same.items():
        print(json.dumps({"what": "same build, one process", "leg": leg, **v}), flush=True)
    summary = {f"{leg}_minus_delivered_ms": round(same[leg]["median_ms"] - same["delivered"]["median_ms"], 4) for leg in ("codec_420", "codec_444")}
    for sub in ("444", "420"):
        summary[f"launch_{sub}_over_copy"] = round(same[f"launch_{sub}"]["median_ms"] / same["device_copy"]["median_ms"], 2)
        summary[f"launch_{sub}_over_export"] = round(same[f"launch_{sub}"]["median_ms"] / same["export_u8"]["median_ms"], 2)
    if a.parent_root:
        med = {"this": [], "parent": []}
        for k in range(a.rounds):                           # the two trees alternate, a process each; who goes first alternates too
            for tree in (("parent", "this"), ("this", "parent"))[k % 2]:
                med[tree].append(run_worker(os.path.abspath(a.parent_root) if tree == "parent" else HERE, "delivered", a)["delivered"]["median_ms"])
        print(json.dumps({"what": "no-codec step_videos, a process per tree and round", **{f"{t}_median_ms": v for t, v in med.items()}}), flush=True)
        for tree, v in med.items():
            summary[f"delivered_{tree}_ms"] = round(statistics.median(v), 4)
            summary[f"delivered_{tree}_spread_ms"] = round(max(v) - min(v), 4)
    else:
        summary.update(parent="not measured")
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
