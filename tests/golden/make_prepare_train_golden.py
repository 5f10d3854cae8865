"""Generate the training-transform fixture from the REFERENCE's own transform classes.

Run in the build container only (needs /root/reference):   python tests/golden/make_prepare_train_golden.py
Writes tests/golden/clip_prepare_train_golden.npz.  Data only, as clip_prepare_golden.npz: no reference source travels.

The reference's default for a training set is ``get_transforms(train=True)`` (dataset.py:84-123, 212-243): ``ToTensorVideo ->
ResizeVideo(128, keep_ratio=True) -> RandomResizedCropVideo(112, (0.6, 1.0)) -> RandomHorizontalFlipVideo(0.5) ->
NormalizeVideo(DEFAULT_MEAN, DEFAULT_STD)``.  The five classes are imported from the reference
(utils_cv/action_recognition/references/transforms_video.py) with the stub-import recipe of make_golden.py and called one by one in
that order under ``random.seed(s)``; the box the crop drew and the flip are read by replaying the generator's state around the
class's own call.  Under the installed torch ``ResizeVideo`` hands ``scale_factor`` to F.interpolate, so the images pin
``rule="scale_factor"``.

Image cases: SIZES x SEEDS, noise frames (make_prepare_golden.case_frames, T = 1), regenerated from their seed and CRC-checked; per case
the resized size, the box, the flip, the next ``random.random()`` after the chain (the state the reference left its generator in) and
the output, stored losslessly as float32-step distances from the float64 restatement (with float32 source coordinates and its intermediate
image rounded to float32: ``_storage_base`` says why) rounded to float32, plus the CRC-32 of the reference's bytes (the scheme of make_prepare_golden.py).

Sampler-only records (boxes and flips, no images), each followed by the next ``random.random()``:
* 20 consecutive draws of (RandomResizedCropVideo.get_params, RandomHorizontalFlipVideo) per resized size under one seed;
* ``scales=(1.0, 1.0)`` on 227 x 128: all 10 attempts fail (w or h exceeds the image), the central fallback with in_ratio 0.564 < 3/4
  gives w = 128, h = 171;
* ``scales=None`` (RandomCropVideo.get_params) on 128 x 170, and on 112 x 112, where no draw is made.

``restate_train_fp64`` is the transform restated in float64 with numpy -- the exact value: the intermediate (resized) image is not
rounded to float32 -- and shares no code with the package."""
import os
import random
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_prepare_golden import _from_steps, _steps, case_frames  # noqa: E402

OUT = os.path.join(HERE, "clip_prepare_train_golden.npz")
IM_SCALE, INPUT_SIZE, T = 128, 112, 1
SCALES, RATIO, FLIP_RATIO = (0.6, 1.0), (3.0 / 4.0, 4.0 / 3.0), 0.5
SIZES = ((240, 320), (480, 270), (112, 112), (239, 317), (128, 171))
SEEDS = (1, 2, 3)
SEQ_SEED, SEQ_N = 11, 20
MEAN, STD = (0.43216, 0.394666, 0.37645), (0.22803, 0.22145, 0.216989)       # dataset.py:28-29


def case_name(H, W, seed):
    return f"{H}x{W}_s{seed}"


def resized_size(Hs, Ws, im_scale=IM_SCALE):
    scale = im_scale / min(Hs, Ws)
    return int(np.floor(Hs * scale)), int(np.floor(Ws * scale))


def restate_train_fp64(frames, box, flip, rule, im_scale=IM_SCALE, input_size=INPUT_SIZE, mean=None, std=None, storage=False):
    """the training transform for a given box and flip in float64: uint8 [T,H,W,3] -> float64 [T,Ho,Wo,3].  ``rule``: "sizes" (step =
    in / out) or "scale_factor" (step = 1 / scale) for the first resize; the box is resampled at step h / Ho, w / Wo.  Nothing in
    between is rounded to float32: this is the exact value.  mean / std: the float32 constants of dataset.py:28-29 taken to float64
    (they are inputs).  ``storage`` (the fixture's storage only, see ``_storage_base``): source coordinates as float32 numbers, and the
    resized image, the resampled box and the difference from the mean each rounded to float32 -- the value the stored distances are
    counted from, not an exact value."""
    x = np.asarray(frames)
    _, Hs, Ws, _ = x.shape
    Ho, Wo = (int(input_size), int(input_size)) if np.isscalar(input_size) else (int(input_size[0]), int(input_size[1]))
    mean = MEAN if mean is None else mean
    std = STD if std is None else std
    scale = im_scale / min(Hs, Ws)
    Hr, Wr = resized_size(Hs, Ws, im_scale)
    sh, sw = (Hs / Hr, Ws / Wr) if rule == "sizes" else (1.0 / scale, 1.0 / scale)
    i, j, h, w = (int(v) for v in box)
    f32 = (lambda v: np.float64(np.float32(v))) if storage else (lambda v: v)

    def axis(step, d, n):
        src = np.maximum(f32(f32(step) * (d + 0.5) - 0.5), 0.0)      # storage: a float32 step, the multiply-subtract rounded once
        i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), src - i0

    def bilinear(v, a0, a1, la, b0, b1, lb):          # v [T,H,W,3]; rows (a0, a1, la), columns (b0, b1, lb)
        lb, la = lb[None, None, :, None], la[None, :, None, None]
        top = (1 - lb) * v[:, a0][:, :, b0] + lb * v[:, a0][:, :, b1]
        bot = (1 - lb) * v[:, a1][:, :, b0] + lb * v[:, a1][:, :, b1]
        return (1 - la) * top + la * bot

    v = x.astype(np.float64) / 255.0
    R = bilinear(v, *axis(sh, np.arange(i, i + h, dtype=np.float64), Hs), *axis(sw, np.arange(j, j + w, dtype=np.float64), Ws))      # the box
    if storage:
        R = f32(R)
    out = bilinear(R, *axis(h / Ho, np.arange(Ho, dtype=np.float64), h), *axis(w / Wo, np.arange(Wo, dtype=np.float64), w))
    if flip:
        out = out[:, :, ::-1]
    m = np.asarray(mean, np.float32).astype(np.float64)
    s = np.asarray(std, np.float32).astype(np.float64)
    return f32(f32(out) - m) / s


def _storage_base(x, box, flip, im_scale=IM_SCALE, input_size=INPUT_SIZE):
    """float32 [T,Ho,Wo,3] the outputs are stored as distances from: the float64 restatement with float32 source coordinates and float32
    roundings after each stage and after the mean's subtraction (where it cancels, later roundings count many times).  Counted from the exact value the distances of a float32 result on noise frames are +-100
    float32 steps and more (a float32 source coordinate is off by 1e-5 of a pixel, and neighbouring noise pixels differ by whole
    units), 15 outputs deflate to 0.97 MB, three times clip_prepare_golden.npz; counted from here only the last roundings are left.
    Either way the decoded bytes are the reference's, CRC-checked."""
    return restate_train_fp64(x, box, flip, "scale_factor", im_scale, input_size, storage=True).astype(np.float32)


def load_cases(path=OUT):
    """[{name, H, W, seed, rseed, Hr, Wr, box (i, j, h, w), flip, next, frames uint8 [T,H,W,3], out float32 [T,112,112,3]}]: inputs
    regenerated, outputs decoded, both CRC-checked against what the generator saw"""
    z = np.load(path)
    cases = []
    for name in z["names"]:
        name = str(name)
        H, W, seed, crc_in, Hr, Wr, i, j, h, w, flip, rseed, crc_out = (int(v) for v in z[name + "_meta"])
        x = case_frames(H, W, "noise", seed)
        assert zlib.crc32(x.tobytes()) == crc_in, f"{name}: regenerated input frames differ from the generator's"
        base = _storage_base(x, (i, j, h, w), flip, int(z["im_scale"]), int(z["input_size"]))
        out = _from_steps(_steps(base) + z[name + "_delta"].astype(np.int64)).reshape(base.shape)
        assert zlib.crc32(out.tobytes()) == crc_out, f"{name}: decoded output differs from the reference's bytes"
        cases.append(dict(name=name, H=H, W=W, seed=seed, rseed=rseed, Hr=Hr, Wr=Wr, box=(i, j, h, w), flip=bool(flip),
                          next=float(z[name + "_next"]), frames=x, out=out))
    return cases


def load_sampler_records(path=OUT):
    """[{name, Hr, Wr, seed, scales (tuple or None), draws int [n,5] = (i, j, h, w, flip), next}]"""
    z = np.load(path)
    recs = []
    for name in z["sampler_names"]:
        name = str(name)
        Hr, Wr, seed = (int(v) for v in z[name + "_cfg"])
        sc = z[name + "_scales"]
        recs.append(dict(name=name, Hr=Hr, Wr=Wr, seed=seed, scales=None if sc.size == 0 else (float(sc[0]), float(sc[1])),
                         draws=z[name + "_draws"].astype(np.int64), next=float(z[name + "_next"])))
    return recs


def main():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flickering_adversarial_video_amd import videoresnet_spec as vs
    from make_golden import import_reference_model
    import_reference_model()            # registers the stubs and puts the reference on sys.path
    from utils_cv.action_recognition.references import transforms_video as tv
    assert tuple(np.float32(vs.DEFAULT_MEAN)) == tuple(np.float32(MEAN)) and tuple(np.float32(vs.DEFAULT_STD)) == tuple(np.float32(STD))
    to_tensor, resize = tv.ToTensorVideo(), tv.ResizeVideo(IM_SCALE, True)
    crop, flipper = tv.RandomResizedCropVideo(INPUT_SIZE, SCALES), tv.RandomHorizontalFlipVideo(FLIP_RATIO)
    normalize = tv.NormalizeVideo(vs.DEFAULT_MEAN, vs.DEFAULT_STD)

    def drawn_box(tfm, clip, get_params):
        """tfm(clip) and the box its own get_params call drew: the generator's state is replayed around the call"""
        state = random.getstate()
        box = get_params()
        random.setstate(state)
        return tfm(clip), tuple(int(v) for v in box)

    def drawn_flip(clip):
        state = random.getstate()
        flip = random.random() < flipper.p
        random.setstate(state)
        return flipper(clip), flip

    G = {"im_scale": np.int64(IM_SCALE), "input_size": np.int64(INPUT_SIZE), "names": np.array([case_name(H, W, s) for H, W in SIZES for s in SEEDS])}
    seed = 20250201
    for H, W in SIZES:
        for rseed in SEEDS:
            seed += 1
            x = case_frames(H, W, "noise", seed)
            random.seed(rseed)
            resized = resize(to_tensor(torch.from_numpy(x)))
            cropped, box = drawn_box(crop, resized, lambda: tv.RandomResizedCropVideo.get_params(resized, crop.scale, crop.ratio))
            flipped, flip = drawn_flip(cropped)
            out = normalize(flipped)                                              # [3,T,112,112]
            nxt = random.random()
            n = case_name(H, W, rseed)
            ref = out.permute(1, 2, 3, 0).contiguous().numpy()                   # channels-last [T,112,112,3], the engine's layout
            assert (resized.shape[-2], resized.shape[-1]) == resized_size(H, W)
            delta = _steps(ref) - _steps(_storage_base(x, box, flip))
            assert np.abs(delta).max() < 2 ** 31
            G[n + "_meta"] = np.array([H, W, seed, zlib.crc32(x.tobytes()), resized.shape[-2], resized.shape[-1], *box, int(flip), rseed,
                                       zlib.crc32(ref.tobytes())], np.int64)
            G[n + "_delta"] = delta.astype(np.int16 if np.abs(delta).max() < 2 ** 15 else np.int32)
            G[n + "_next"] = np.float64(nxt)
    # sampler-only records
    marker = torch.arange(2.0).reshape(1, 1, 1, 2)
    records = [(f"seq_{Hr}x{Wr}", Hr, Wr, SCALES) for Hr, Wr in sorted({resized_size(H, W) for H, W in SIZES})]
    records += [("fallback_227x128", 227, 128, (1.0, 1.0)), ("randomcrop_128x170", 128, 170, None), ("randomcrop_112x112", 112, 112, None)]
    G["sampler_names"] = np.array([r[0] for r in records])
    for name, Hr, Wr, scales in records:
        clip = torch.empty(3, 1, Hr, Wr)
        random.seed(SEQ_SEED)
        draws = []
        for _ in range(SEQ_N):
            if scales is None:
                box = tv.RandomCropVideo.get_params(clip, (INPUT_SIZE, INPUT_SIZE))
            else:
                box = tv.RandomResizedCropVideo.get_params(clip, scales, RATIO)
            flip = bool(flipper(marker)[0, 0, 0, 0] == 1.0)
            draws.append([int(v) for v in box] + [int(flip)])
        G[name + "_cfg"] = np.array([Hr, Wr, SEQ_SEED], np.int64)
        G[name + "_scales"] = np.array([] if scales is None else scales, np.float64)
        G[name + "_draws"] = np.array(draws, np.int16)
        G[name + "_next"] = np.float64(random.random())
    np.savez_compressed(OUT, **G)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(G), "arrays")
    for c in load_cases():                                                       # round trip
        e = np.abs(c["out"].astype(np.float64) - restate_train_fp64(c["frames"], c["box"], c["flip"], "scale_factor")).max()
        print(c["name"], "resized", c["Hr"], "x", c["Wr"], "box", c["box"], "flip", c["flip"], f"e_ref {e:.2e}", "decoded ok")
    for r in load_sampler_records():
        print(r["name"], r["scales"], r["draws"][:3].tolist(), r["next"])


if __name__ == "__main__":
    main()
