"""Generate the clip-preparation fixture from the REFERENCE's own evaluation transform.

Run in the build container only (needs /root/reference):   python tests/golden/make_prepare_golden.py
Writes tests/golden/clip_prepare_golden.npz.  The fixture holds data only: per case the source size, the seed / kind of the input
frames, a CRC of those frames, the resized size the reference produced and the reference's output; no reference source travels.

The reference's attack scripts build their datasets with ``get_transforms(train=False)`` (r2plus1d_main_universal_attack.py:169-170;
dataset.py:84-123), i.e. ``ToTensorVideo -> ResizeVideo(128, keep_ratio=True) -> CenterCropVideo(112) -> [flip, p = 0] ->
NormalizeVideo(DEFAULT_MEAN, DEFAULT_STD)``.  The four classes are imported from the reference
(utils_cv/action_recognition/references/transforms_video.py) with the stub-import recipe of make_golden.py and called in that order.
(``dataset.py`` itself imports decord / einops at module scope; its two constants DEFAULT_MEAN / DEFAULT_STD, dataset.py:28-29, are
the values of videoresnet_spec.)  Under the installed torch ``ResizeVideo`` hands ``scale_factor`` through to F.interpolate, so this
fixture pins ``rule="scale_factor"``.

Size: 14 outputs of 112 x 112 x 3 float32 are 2.1 MB and do not compress (1.25 MB deflated), more than a committed file may
hold, and the inputs would be megabytes more.  So
* the input frames are NOT stored: ``case_frames`` regenerates them from the case's seed, and the fixture records their CRC-32 so
  that a test on another machine notices a different random stream at once;
* each output is stored LOSSLESSLY as its distance in float32 steps from ``restate_fp64`` rounded to float32 -- an int32 array of
  mostly 0 / +-1 (thousands only where the value itself is next to zero), which deflates to a tenth -- plus the CRC-32 of the reference's bytes.  ``load_cases`` adds the distances back and checks the CRC, so
  what a test compares against is bit for bit what the reference computed, or the load fails.

``restate_fp64`` is the transform restated in float64 with numpy (elementwise IEEE operations only: the same bits on any machine).
The tests use it as the exact value the float32 implementations are measured against (ref64); it shares no code with the package."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "clip_prepare_golden.npz")
IM_SCALE, INPUT_SIZE, T = 128, 112, 1
# 240x320 / 360x480: the usual 4:3 sources; 480x270: portrait; 256x340, 128x171: in * scale is an integer (both rules agree), 171 - 112
# = 59 -> crop offset 29.5 -> 30 under round-half-to-even; 112x112: upsampling; 239x317: odd
SIZES = ((240, 320), (360, 480), (480, 270), (256, 340), (128, 171), (112, 112), (239, 317))
KINDS = ("noise", "ramp")


def case_name(H, W, kind):
    return f"{H}x{W}_{kind}"


def case_frames(H, W, kind, seed, frames=T):
    """uint8 [frames,H,W,3]: uniform noise from ``seed`` or a smooth ramp (x, y and diagonal gradients, inverted on odd frames)"""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (frames, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (H + W - 2)], -1).astype(np.uint8)
    return np.stack([f if t % 2 == 0 else 255 - f for t in range(frames)])


def restate_fp64(frames, rule, im_scale=IM_SCALE, input_size=INPUT_SIZE, mean=None, std=None):
    """the evaluation transform in float64: uint8 [T,H,W,3] -> float64 [T,S,S,3].  ``rule``: "sizes" (step = in / out) or
    "scale_factor" (step = 1 / scale).  mean / std: the float32 constants of dataset.py:28-29 taken to float64 (they are inputs)."""
    x = np.asarray(frames)
    _, Hs, Ws, _ = x.shape
    S = int(input_size)
    mean = (0.43216, 0.394666, 0.37645) if mean is None else mean
    std = (0.22803, 0.22145, 0.216989) if std is None else std
    scale = im_scale / min(Hs, Ws)
    Hr, Wr = int(np.floor(Hs * scale)), int(np.floor(Ws * scale))
    ci, cj = int(round((Hr - S) / 2.0)), int(round((Wr - S) / 2.0))
    sh, sw = (Hs / Hr, Ws / Wr) if rule == "sizes" else (1.0 / scale, 1.0 / scale)

    def axis(step, d, n):
        src = np.maximum(step * (d + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), src - i0

    h0, h1, lh = axis(sh, np.arange(ci, ci + S, dtype=np.float64), Hs)
    w0, w1, lw = axis(sw, np.arange(cj, cj + S, dtype=np.float64), Ws)
    v = x.astype(np.float64) / 255.0
    lw, lh = lw[None, None, :, None], lh[None, :, None, None]
    top = (1 - lw) * v[:, h0][:, :, w0] + lw * v[:, h0][:, :, w1]
    bot = (1 - lw) * v[:, h1][:, :, w0] + lw * v[:, h1][:, :, w1]
    m = np.asarray(mean, np.float32).astype(np.float64)
    s = np.asarray(std, np.float32).astype(np.float64)
    return ((1 - lh) * top + lh * bot - m) / s


def _steps(a32):
    """float32 -> int64 position on the monotone integer line of float32 values"""
    i = a32.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _from_steps(k):
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32).view(np.float32)


def load_cases(path=OUT):
    """[{name, H, W, kind, seed, Hr, Wr, frames uint8 [T,H,W,3], out float32 [T,112,112,3]}]: inputs regenerated, outputs decoded, both
    CRC-checked against what the generator saw"""
    z = np.load(path)
    cases = []
    for name in z["names"]:
        name = str(name)
        H, W, seed, crc_in, Hr, Wr, crc_out = (int(v) for v in z[name + "_meta"])
        kind = name.split("_")[1]
        x = case_frames(H, W, kind, seed)
        assert zlib.crc32(x.tobytes()) == crc_in, f"{name}: regenerated input frames differ from the generator's"
        base = restate_fp64(x, "scale_factor", int(z["im_scale"]), int(z["input_size"])).astype(np.float32)
        out = _from_steps(_steps(base) + z[name + "_delta"].astype(np.int64)).reshape(base.shape)
        assert zlib.crc32(out.tobytes()) == crc_out, f"{name}: decoded output differs from the reference's bytes"
        cases.append(dict(name=name, H=H, W=W, kind=kind, seed=seed, Hr=Hr, Wr=Wr, frames=x, out=out))
    return cases


def main():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from make_golden import import_reference_model
    import_reference_model()            # registers the stubs and puts the reference on sys.path
    from utils_cv.action_recognition.references import transforms_video as tv
    tfms = [tv.ToTensorVideo(), tv.ResizeVideo(IM_SCALE, True), tv.CenterCropVideo(INPUT_SIZE), tv.NormalizeVideo(vs.DEFAULT_MEAN, vs.DEFAULT_STD)]
    G = {"im_scale": np.int64(IM_SCALE), "input_size": np.int64(INPUT_SIZE), "names": np.array([case_name(H, W, k) for H, W in SIZES for k in KINDS])}
    seed = 20250101
    for H, W in SIZES:
        for kind in KINDS:
            seed += 1
            x = case_frames(H, W, kind, seed)
            clip = tfms[0](torch.from_numpy(x))
            resized = tfms[1](clip)
            out = tfms[3](tfms[2](resized))                          # [3,T,112,112]
            n = case_name(H, W, kind)
            ref = out.permute(1, 2, 3, 0).contiguous().numpy()                   # channels-last [T,112,112,3], the engine's layout
            delta = _steps(ref) - _steps(restate_fp64(x, "scale_factor").astype(np.float32))
            G[n + "_meta"] = np.array([H, W, seed, zlib.crc32(x.tobytes()), resized.shape[-2], resized.shape[-1], zlib.crc32(ref.tobytes())], np.int64)
            G[n + "_delta"] = delta.astype(np.int32)
    np.savez_compressed(OUT, **G)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(G), "arrays")
    for c in load_cases():                                                       # round trip
        print(c["name"], "resized", c["Hr"], "x", c["Wr"], "decoded ok")


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    main()
