#!/usr/bin/env python3
"""What the codec round trip costs (csrc/codec.hip, flk_codec_roundtrip_u8).

1. Single launches at 16 clips x 16 frames x 240 x 320, `--reps` launches between one HIP-event pair, the median of the groups:
   the codec at 4:4:4 and 4:2:0 (quality 75) through the C ABI with arguments built once (`launch_*`: plain, with stats, with a
   tone table and a frame table cutting the frames from 300-frame videos) and once through ops.codec_roundtrip (`wrapper_*`: its host
   checks and the table upload included); beside a device copy of the same bytes (3 read + 3 written per pixel, as the codec
   moves) and the uint8 export of the same frames as one video (export_video).
2. The mc3_18 batch-16 `step_videos` (bf16, 16 frames of 112 x 112, Adam, period 16, training transform) with and without a codec,
   in one process, stepping alternately, a HIP-event pair around every step.
   GOP legs (flk_codec_roundtrip_gop_u8, quality 75, `--gop` 12): `gop_launch_*` on 16 clips x (16 + 11 lead-in frames) x 240 x 320
   beside `intra_same_*`, the intra launch of the same frames; `gop_video_*` / `intra_video_*` on one whole `--frames` video; and the
   step with `Codec(75, "420", gop)` (`gop_420`) beside the intra one.
   Motion legs (flk_codec_roundtrip_mc_u8, `--search` 7; 0 leaves them out): `mc_launch_*` / `mc_video_*`, the launch sequence of the
   same frames as the GOP legs (one launch per frame position, the workspace allocated once), and the step with
   `Codec(75, "420", gop, search)` (`mc_420`).
3. The no-codec step and the intra, GOP and (with `--search` above 0) motion launches against the PARENT commit (`--parent-root PATH`: a checkout of the parent with its library
   built): the same launches, so the trees only have to agree inside the run's spread.  A process per tree and round, alternating.

Prints one JSON line per leg and a summary line.  Needs the GPU; there is no fallback.

    python tools/codec_time.py [--steps 30] [--warmup 6] [--rounds 2] [--reps 20] [--frames 300] [--gop 12] [--search 7] [--parent-root PATH]"""
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
        extra = dict(gop=a.gop) if leg.startswith("gop_") else dict(gop=a.gop, search=a.search) if leg.startswith("mc_") else {}
        kw = {} if leg == "delivered" else dict(codec=vs.Codec(75, leg.split("_")[1], **extra))
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
    if hasattr(lib, "flk_codec_roundtrip_gop_u8"):           # (absent from a parent tree from before the GOP entry)
        # GOPs: 16 spans of T + gop - 1 frames (a clip with the longest lead-in) from frame `gop` of every video, beside the intra launch of
        # the same frames; and one whole video.  Spans and counts are host arrays of the call
        L = T + a.gop - 1
        assert a.gop + L <= a.frames, "--frames too short for the GOP legs"
        span_outs = [torch.empty((L, 240, 320, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
        whole_out = torch.empty_like(videos[0])

        def gop_args(srcs, dsts, sub):
            arr = (_lib.CodecClip * len(srcs))()
            for d, v, o in zip(arr, srcs, dsts):
                d.src, d.T, d.Hs, d.Ws, d.pitch_t, d.pitch_h = v.data_ptr(), v.shape[0], 240, 320, v.stride(0), v.stride(1)
                d.dst, d.dst_pitch_t, d.dst_pitch_h = o.data_ptr(), o.stride(0), o.stride(1)
            g = _lib.CodecArgs()
            g.nclip, g.quality, g.subsampling, g.clips = len(srcs), 75, int(sub), arr
            g._keep = arr
            return g

        def ints(v, n):
            return (C.c_int32 * n)(*([v] * n))

        for sub in vs.CODEC_SUBSAMPLINGS:
            spans, same = gop_args(videos, span_outs, sub), gop_args([v[a.gop:a.gop + L] for v in videos], span_outs, sub)
            whole = gop_args(videos[:1], [whole_out], sub)
            calls[f"gop_launch_{sub}"] = lambda g=spans, f=ints(a.gop, B), c=ints(L, B): lib.flk_codec_roundtrip_gop_u8(
                C.byref(g), a.gop, f, c, L, None, None, stream_ptr())
            calls[f"intra_same_{sub}"] = lambda g=same: lib.flk_codec_roundtrip_u8(C.byref(g), None, L, None, None, stream_ptr())
            calls[f"gop_video_{sub}"] = lambda g=whole, f=ints(0, 1), c=ints(a.frames, 1): lib.flk_codec_roundtrip_gop_u8(
                C.byref(g), a.gop, f, c, a.frames, None, None, stream_ptr())
            calls[f"intra_video_{sub}"] = lambda g=whole: lib.flk_codec_roundtrip_u8(C.byref(g), None, a.frames, None, None, stream_ptr())
            if a.search > 0 and hasattr(lib, "flk_codec_roundtrip_mc_u8"):
                for name, g, f, c, n in ((f"mc_launch_{sub}", spans, ints(a.gop, B), ints(L, B), L), (f"mc_video_{sub}", whole, ints(0, 1), ints(a.frames, 1), a.frames)):
                    ws = torch.empty(lib.flk_codec_mc_scratch_bytes(C.byref(g), a.gop, c), dtype=torch.uint8, device="cuda")
                    calls[name] = lambda g=g, f=f, c=c, n=n, ws=ws: lib.flk_codec_roundtrip_mc_u8(
                        C.byref(g), a.gop, a.search, f, c, n, None, None, None, 0, ptr(ws), ws.numel(), stream_ptr())
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
           "--reps", str(a.reps), "--rounds", str(a.rounds), "--frames", str(a.frames), "--gop", str(a.gop), "--search", str(a.search)]
    cmd += ["--launches"] if with_launches else []
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
    ap.add_argument("--gop", type=int, default=12, help="the GOP length of the GOP legs")
    ap.add_argument("--search", type=int, default=7, help="the motion search range of the motion legs (0: none)")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with libflicker_hip.so built in it")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launches", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="delivered,codec_420,codec_444", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.gop < 2:
        ap.error("--gop must be >= 2 (1 is the intra codec, which the other legs time)")
    if a.worker:
        return worker(a)
    if not 0 <= a.search <= 15:
        ap.error("--search must be in 0..15")
    same = run_worker(HERE, "delivered,codec_420,codec_444,gop_420" + (",mc_420" if a.search else ""), a, with_launches=True)
    for leg, v in same.items():
        print(json.dumps({"what": "same build, one process", "leg": leg, **v}), flush=True)
    summary = {f"{leg}_minus_delivered_ms": round(same[leg]["median_ms"] - same["delivered"]["median_ms"], 4) for leg in ("codec_420", "codec_444")}
    summary["gop_420_minus_codec_420_ms"] = round(same["gop_420"]["median_ms"] - same["codec_420"]["median_ms"], 4)
    if a.search:
        summary["mc_420_minus_gop_420_ms"] = round(same["mc_420"]["median_ms"] - same["gop_420"]["median_ms"], 4)
    for sub in ("444", "420"):
        summary[f"gop_launch_{sub}_over_intra_same"] = round(same[f"gop_launch_{sub}"]["median_ms"] / same[f"intra_same_{sub}"]["median_ms"], 2)
        summary[f"gop_video_{sub}_over_intra_video"] = round(same[f"gop_video_{sub}"]["median_ms"] / same[f"intra_video_{sub}"]["median_ms"], 2)
        if a.search:
            summary[f"mc_launch_{sub}_over_gop_launch"] = round(same[f"mc_launch_{sub}"]["median_ms"] / same[f"gop_launch_{sub}"]["median_ms"], 2)
            summary[f"mc_video_{sub}_over_gop_video"] = round(same[f"mc_video_{sub}"]["median_ms"] / same[f"gop_video_{sub}"]["median_ms"], 2)
        summary[f"launch_{sub}_over_copy"] = round(same[f"launch_{sub}"]["median_ms"] / same["device_copy"]["median_ms"], 2)
        summary[f"launch_{sub}_over_export"] = round(same[f"launch_{sub}"]["median_ms"] / same["export_u8"]["median_ms"], 2)
    if a.parent_root:
        # the no-codec step and the launches of every codec kernel instantiation, which the parent has as well
        what = ("delivered", "launch_420", "launch_444", "gop_launch_420", "gop_launch_444") + (("mc_launch_420", "mc_launch_444") if a.search else ())
        med = {w: {"this": [], "parent": []} for w in what}
        for k in range(a.rounds):                           # the two trees alternate, a process each; who goes first alternates too
            for tree in (("parent", "this"), ("this", "parent"))[k % 2]:
                legs = run_worker(os.path.abspath(a.parent_root) if tree == "parent" else HERE, "delivered", a, with_launches=True)
                for w in what:
                    med[w][tree].append(legs[w]["median_ms"])
        for w in what:
            print(json.dumps({"what": f"{w}, a process per tree and round", **{f"{t}_median_ms": v for t, v in med[w].items()}}), flush=True)
            for tree, v in med[w].items():
                summary[f"{w}_{tree}_ms"] = round(statistics.median(v), 4)
                summary[f"{w}_{tree}_spread_ms"] = round(max(v) - min(v), 4)
    else:
        summary.update(parent="not measured")
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
