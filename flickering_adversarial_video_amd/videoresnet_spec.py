"""torchvision-0.5.0 VideoResNet (r2plus1d_18 / r3d_18 / mc3_18) and R(2+1)D-34 layer tables and seeded synthetic weights.

R(2+1)D-34 is the victim the reference attacks by default (utils_cv/action_recognition/model.py:341, 418-441): the IG65M / Kinetics
models of moabitcoin/ig65m-pytorch (models.py there): torchvision ``VideoResNet(BasicBlock, [Conv2Plus1D] * 4, [3, 4, 6, 3], R2Plus1dStem)``
with ``layer{2,3,4}[0].conv2[0] = Conv2Plus1D(c, c, 288 / 576 / 1152)`` (the midplanes of the Caffe2 checkpoints) and every
``BatchNorm3d`` built with eps 1e-3 (the plan, net.cpp, applies that eps; a state_dict does not record it).

The reference loads pretrained weights through torchvision (utils_cv/action_recognition/model.py:421); neither
torchvision nor the checkpoints are available here, so benchmarks and tests use seeded synthetic weights under the
torchvision ``state_dict`` names -- a real ``state_dict`` converted to ``{name: ndarray}`` drops in.
"""
import numpy as np

DEFAULT_MEAN = (0.43216, 0.394666, 0.37645)      # dataset.py:28
DEFAULT_STD = (0.22803, 0.22145, 0.216989)       # dataset.py:29
ARCHS = ("r2plus1d_18", "r3d_18", "mc3_18", "r2plus1d_34")
PLANES = (64, 128, 256, 512)
# model name -> class count of its pretrained head (model.py:46-56)
MODELS = {"r2plus1d_34_32_ig65m": 359, "r2plus1d_34_32_kinetics": 400, "r2plus1d_34_8_ig65m": 487, "r2plus1d_34_8_kinetics": 400,
          "mc3_18": 400, "r2plus1d_18": 400, "r3d_18": 400}


def blocks_per_stage(arch):
    return (3, 4, 6, 3) if arch == "r2plus1d_34" else (2, 2, 2, 2)


def resolve_model(base_model, sample_length, num_classes=None):
    """``VideoLearnerAdversarial.init_model``'s choice (model.py:373, 418-441): ``(base_model, sample_length, num_classes)`` ->
    ``(arch, model name, class count)``.  ``ig65m`` / ``kinetics`` name ``r2plus1d_34_{8|32}_{base_model}`` (8 or 32 frames only); a
    model name of MODELS stands for itself; ``num_classes`` (a replaced ``fc`` head, model.py:436-437) overrides the table's count."""
    if base_model in ("ig65m", "kinetics"):
        if sample_length not in (8, 32):
            raise ValueError(f"base_model {base_model!r} needs sample_length 8 or 32 (model.py:373), got {sample_length!r}")
        name = f"r2plus1d_34_{sample_length}_{base_model}"
    elif base_model in MODELS:
        name = base_model
    else:
        raise ValueError(f"base_model must be 'ig65m', 'kinetics' or one of {sorted(MODELS)}, got {base_model!r}")
    arch = "r2plus1d_34" if name.startswith("r2plus1d_34_") else name
    return arch, name, int(num_classes) if num_classes is not None else MODELS[name]


def midplanes(inplanes, planes):
    return (inplanes * planes * 27) // (inplanes * 9 + 3 * planes)


def _kind(arch, layer):
    if arch in ("r2plus1d_18", "r2plus1d_34"):
        return "2plus1d"
    return "3d" if (arch == "r3d_18" or layer == 1) else "notemporal"


def conv_table(arch):
    """[(weight prefix, cout, cin, (kt,kh,kw), bn prefix)] in forward order"""
    assert arch in ARCHS, arch
    t = [("stem.0", 45, 3, (1, 7, 7), "stem.1"), ("stem.3", 64, 45, (3, 1, 1), "stem.4")] if _kind(arch, 2) == "2plus1d" else \
        [("stem.0", 64, 3, (3, 7, 7), "stem.1")]
    inpl = 64
    for li, planes in enumerate(PLANES, start=1):
        kind = _kind(arch, li)
        for bi in range(blocks_per_stage(arch)[li - 1]):
            stride = 2 if (li > 1 and bi == 0) else 1
            pre = f"layer{li}.{bi}"
            mid = midplanes(inpl, planes)
            for cname, ci, co in ((".conv1", inpl, planes), (".conv2", planes, planes)):
                if arch == "r2plus1d_34" and cname == ".conv2" and li > 1 and bi == 0:
                    mid = planes * 9 // 4            # 288 / 576 / 1152 (ig65m-pytorch's Caffe2 midplanes) instead of 230 / 460 / 921
                if kind == "2plus1d":
                    t += [(pre + cname + ".0.0", mid, ci, (1, 3, 3), pre + cname + ".0.1"),
                          (pre + cname + ".0.3", co, mid, (3, 1, 1), pre + cname + ".1")]
                else:
                    t += [(pre + cname + ".0", co, ci, (3, 3, 3) if kind == "3d" else (1, 3, 3), pre + cname + ".1")]
            if stride != 1 or inpl != planes:
                t += [(pre + ".downsample.0", planes, inpl, (1, 1, 1), pre + ".downsample.1")]
            inpl = planes
    return t


def synthetic_weights(arch, seed=42, num_classes=400):
    rng = np.random.default_rng(seed)
    W = {}
    for pre, co, ci, k, bnp in conv_table(arch):
        fan_in = ci * k[0] * k[1] * k[2]
        W[pre + ".weight"] = (rng.standard_normal((co, ci, *k), dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in)))
        W[bnp + ".weight"] = rng.uniform(0.8, 1.2, co).astype(np.float32)
        W[bnp + ".bias"] = (rng.standard_normal(co, dtype=np.float32) * 0.1).astype(np.float32)
        W[bnp + ".running_mean"] = (rng.standard_normal(co, dtype=np.float32) * 0.1).astype(np.float32)
        W[bnp + ".running_var"] = rng.uniform(0.5, 1.5, co).astype(np.float32)
    W["fc.weight"] = (rng.standard_normal((num_classes, 512), dtype=np.float32) * np.float32(0.01))   # keeps the synthetic logits O(5)
    W["fc.bias"] = (rng.standard_normal(num_classes, dtype=np.float32) * 0.1).astype(np.float32)
    return W


def normalize_u8(u8):
    """uint8 frames [...,3] -> the normalised fp32 clip ``(u8 / 255 - mean) / std`` (dataset.py:28-29 transforms), evaluated in float32:
    the expression of the scripts' host route, of ``synthetic_clip`` and of ``u8_decode_table``.  (A float64 or fused multiply-add
    evaluation rounds to a different float32 in over half of the 768 (byte, channel) entries.)"""
    x = np.asarray(u8).astype(np.float32)
    return ((x / 255.0 - np.array(DEFAULT_MEAN, np.float32)) / np.array(DEFAULT_STD, np.float32)).astype(np.float32)


def u8_decode_table():
    """fp32 [256,3]: entry [v, c] is the normalised value of byte v in channel c -- ``normalize_u8`` of every byte, so a uint8 clip
    decoded through it (flk_apply_args.x_lut) is bitwise the host-normalised fp32 clip"""
    return np.ascontiguousarray(normalize_u8(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)))


def encode_u8(x):
    """normalised fp32 values [...,3] -> the bytes of a frame, the inverse of ``normalize_u8``: ``y = x * std + mean; z = y * 255;
    q = min(rint(z), 255) where z >= 0, else 0`` in float32, one rounded operation per step (rint: half to even; NaN -> 0) -- the
    arithmetic of flk_adv_export_u8 in the torch dialect, restated on the host.  ``encode_u8(u8_decode_table())`` is every byte."""
    y = np.asarray(x, dtype=np.float32) * np.array(DEFAULT_STD, np.float32)
    y = y + np.array(DEFAULT_MEAN, np.float32)
    z = y * np.float32(255.0)
    with np.errstate(invalid="ignore"):
        q = np.where(z >= 0, np.minimum(np.rint(z), np.float32(255.0)), np.float32(0.0))
    return q.astype(np.uint8)


def synthetic_clip_u8(B, T=16, H=112, W=112, seed=1234):
    """uint8 frames [B,T,H,W,3] channels-last: the bytes ``synthetic_clip`` normalises for the same seed"""
    return np.random.default_rng(seed).integers(0, 256, (B, T, H, W, 3)).astype(np.uint8)


def synthetic_clip(B, T=16, H=112, W=112, seed=1234):
    """normalised fp32 clip [B,T,H,W,3] channels-last ((u8/255 - mean)/std, dataset.py transforms)"""
    return normalize_u8(synthetic_clip_u8(B, T, H, W, seed))


RESIZE_RULES = ("sizes", "scale_factor")


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def prepare_geometry(Hs, Ws, im_scale=128, input_size=112, rule="sizes"):
    """Geometry of the reference's evaluation transform (dataset.py:84-123: ``ResizeVideo(im_scale, keep_ratio=True)`` then
    ``CenterCropVideo(input_size)``) for ``Hs x Ws`` source frames: ``(Hr, Wr, step_h, step_w, crop_i, crop_j)``.  The one place
    on the host where these rules are written down; flk_clip_prepare and ``prepare_host`` both take their numbers from here.

    ``scale = im_scale / min(Hs, Ws)`` (a Python double); resized size ``Hr = floor(Hs * scale)``, ``Wr = floor(Ws * scale)`` -- what
    ``F.interpolate(scale_factor=scale)`` computes.  The source step per resized pixel, a float32, follows ``rule``:

    * ``"sizes"`` (default): ``float32(in) / float32(out)`` per axis -- ``F.interpolate(size=(Hr, Wr))``, and what torch 1.4.0, the
      version the reference pins (requirements.txt), did with ``scale_factor``: it only derived the output size from it.  This is the
      arithmetic of the paper's software, hence the default.
    * ``"scale_factor"``: ``float32(1.0 / scale)`` on both axes -- what a current torch does when ``ResizeVideo`` hands it
      ``scale_factor``.

    The two agree whenever ``in * scale`` is an integer (256x340, 128x171) and differ visibly otherwise (240x320).
    Crop offsets: ``round((Hr - Ho) / 2.0)``, Python's round-half-to-even (functional_video.py:60-61).  A resized image smaller than
    the crop raises ValueError (the reference asserts)."""
    if rule not in RESIZE_RULES:
        raise ValueError(f"rule must be one of {RESIZE_RULES}, got {rule!r}")
    Hs, Ws = int(Hs), int(Ws)
    Ho, Wo = _pair(input_size)
    if Hs <= 0 or Ws <= 0 or Ho <= 0 or Wo <= 0 or im_scale <= 0:
        raise ValueError(f"sizes must be positive: source {Hs} x {Ws}, im_scale {im_scale}, input_size {Ho} x {Wo}")
    scale = im_scale / min(Hs, Ws)
    Hr, Wr = int(np.floor(Hs * scale)), int(np.floor(Ws * scale))
    if Hr < Ho or Wr < Wo:
        raise ValueError(f"resized image {Hr} x {Wr} (from {Hs} x {Ws} at im_scale {im_scale}) is smaller than the crop {Ho} x {Wo}")
    if rule == "sizes":
        step_h, step_w = np.float32(Hs) / np.float32(Hr), np.float32(Ws) / np.float32(Wr)
    else:
        step_h = step_w = np.float32(1.0 / scale)
    return Hr, Wr, float(step_h), float(step_w), int(round((Hr - Ho) / 2.0)), int(round((Wr - Wo) / 2.0))


def prepare_host(frames, im_scale=128, input_size=112, mean=DEFAULT_MEAN, std=DEFAULT_STD, rule="sizes"):
    """The evaluation transform with torch on the CPU, the A/B route of ``ops.prepare_clips``: uint8 frames ``[T,H,W,3]`` (tensor
    or array) -> the normalised float32 clip ``[T,Ho,Wo,3]``.  Four steps in float32: ``/255``, bilinear ``F.interpolate``
    (``align_corners=False``; ``size=`` or ``scale_factor=`` by ``rule``), centre crop, ``(v - mean) / std``.  Geometry from
    ``prepare_geometry``."""
    import torch
    import torch.nn.functional as F
    x = torch.as_tensor(np.ascontiguousarray(frames) if isinstance(frames, np.ndarray) else frames).cpu()
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 [T,H,W,3], got {tuple(x.shape)} {x.dtype}")
    Hs, Ws = int(x.shape[1]), int(x.shape[2])
    Ho, Wo = _pair(input_size)
    Hr, Wr, _, _, ci, cj = prepare_geometry(Hs, Ws, im_scale, input_size, rule)
    clip = x.float().permute(3, 0, 1, 2) / 255.0                                     # [C,T,H,W]
    if rule == "sizes":
        clip = F.interpolate(clip, size=(Hr, Wr), mode="bilinear", align_corners=False)
    else:
        clip = F.interpolate(clip, scale_factor=im_scale / min(Hs, Ws), mode="bilinear", align_corners=False)
    assert tuple(clip.shape[-2:]) == (Hr, Wr), (tuple(clip.shape), Hr, Wr)
    clip = clip[..., ci:ci + Ho, cj:cj + Wo].clone()
    m = torch.as_tensor(mean, dtype=clip.dtype)
    s = torch.as_tensor(std, dtype=clip.dtype)
    clip.sub_(m[:, None, None, None]).div_(s[:, None, None, None])
    return clip.permute(1, 2, 3, 0).contiguous()


def train_crop_params(Hr, Wr, input_size=112, scales=(0.6, 1.0), ratio=(3 / 4, 4 / 3), flip_ratio=0.5, rng=None):
    """The random draws of the reference's training transform (dataset.py:105-118) for one clip whose resized image is ``Hr x Wr``:
    ``(i, j, h, w, flip)``, the crop box in the resized image and whether the clip is mirrored along W.  ``rng``: a ``random.Random``
    (None: a fresh unseeded one); the draws are made in the reference's order, so ``random.Random(s)`` gives the boxes the reference
    gives under ``random.seed(s)``.

    ``scales`` given: ``RandomResizedCropVideo.get_params`` (transforms_video.py:137-179) -- up to 10 attempts of ``uniform(*scales)``
    times the area, ``exp(uniform(log r0, log r1))`` as aspect ratio, ``w = round(sqrt(area * aspect))``, ``h = round(sqrt(area /
    aspect))``; the first box that fits draws ``randint(0, Hr - h)``, ``randint(0, Wr - w)``.  After 10 misses the central fallback:
    the whole width at ratio ``min(ratio)`` when the image is narrower than that, the whole height at ``max(ratio)`` when wider, else
    the whole image.  ``scales=None``: ``RandomCropVideo.get_params`` (:77-95) -- a box of ``input_size``, no draw when the image has
    that size already, else two ``randint``s.  Then ``rng.random() < flip_ratio`` (:272), a draw the reference makes whatever p is."""
    import math
    import random
    rng = random.Random() if rng is None else rng
    Hr, Wr = int(Hr), int(Wr)
    if scales is None:
        th, tw = _pair(input_size)
        if Hr < th or Wr < tw:
            raise ValueError(f"resized image {Hr} x {Wr} is smaller than the crop {th} x {tw}")
        if (Hr, Wr) == (th, tw):
            box = (0, 0, Hr, Wr)
        else:
            i = rng.randint(0, Hr - th)
            box = (i, rng.randint(0, Wr - tw), th, tw)
    else:
        area, box = Wr * Hr, None
        for _ in range(10):
            target_area = rng.uniform(*scales) * area
            aspect_ratio = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if w <= Wr and h <= Hr:
                i = rng.randint(0, Hr - h)
                box = (i, rng.randint(0, Wr - w), h, w)
                break
        if box is None:                          # central fallback
            in_ratio = Wr / Hr
            if in_ratio < min(ratio):
                w = Wr
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = Hr
                w = int(round(h * max(ratio)))
            else:
                w, h = Wr, Hr
            box = ((Hr - h) // 2, (Wr - w) // 2, h, w)
    flip = rng.random() < flip_ratio
    return box + (bool(flip),)


def prepare_host_train(frames, box, flip, im_scale=128, input_size=112, mean=DEFAULT_MEAN, std=DEFAULT_STD, rule="sizes"):
    """The training transform with torch on the CPU for a given ``box = (i, j, h, w)`` and ``flip`` (``train_crop_params`` draws them),
    the A/B route of ``ops.prepare_clips(..., boxes=, flips=)``: uint8 frames ``[T,H,W,3]`` -> the normalised float32 clip
    ``[T,Ho,Wo,3]``.  ``prepare_host``'s ``/255`` and resize (by ``rule``), then the box sliced out of the resized image and resampled
    with ``F.interpolate(size=(Ho, Wo), mode="bilinear", align_corners=False)`` (functional_video.py:33-49, resized_crop; on a box of the
    output size, the RandomCropVideo route, that resampling is the identity), ``flip(-1)`` when flagged, ``(v - mean) / std``."""
    import torch
    import torch.nn.functional as F
    x = torch.as_tensor(np.ascontiguousarray(frames) if isinstance(frames, np.ndarray) else frames).cpu()
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 [T,H,W,3], got {tuple(x.shape)} {x.dtype}")
    Hs, Ws = int(x.shape[1]), int(x.shape[2])
    Ho, Wo = _pair(input_size)
    if rule not in RESIZE_RULES:
        raise ValueError(f"rule must be one of {RESIZE_RULES}, got {rule!r}")
    scale = im_scale / min(Hs, Ws)
    Hr, Wr = int(np.floor(Hs * scale)), int(np.floor(Ws * scale))
    i, j, h, w = (int(v) for v in box)
    if h < 1 or w < 1 or i < 0 or j < 0 or i + h > Hr or j + w > Wr:
        raise ValueError(f"box ({i},{j})+{h}x{w} outside the resized image {Hr} x {Wr}")
    clip = x.float().permute(3, 0, 1, 2) / 255.0                                     # [C,T,H,W]
    if rule == "sizes":
        clip = F.interpolate(clip, size=(Hr, Wr), mode="bilinear", align_corners=False)
    else:
        clip = F.interpolate(clip, scale_factor=scale, mode="bilinear", align_corners=False)
    assert tuple(clip.shape[-2:]) == (Hr, Wr), (tuple(clip.shape), Hr, Wr)
    clip = clip[..., i:i + h, j:j + w]
    clip = F.interpolate(clip, size=(Ho, Wo), mode="bilinear", align_corners=False)
    if flip:
        clip = clip.flip(-1)
    m = torch.as_tensor(mean, dtype=clip.dtype)
    s = torch.as_tensor(std, dtype=clip.dtype)
    clip = clip.clone().sub_(m[:, None, None, None]).div_(s[:, None, None, None])
    return clip.permute(1, 2, 3, 0).contiguous()


SAMPLING_DEFAULTS = {"sample_step": 1, "temporal_jitter": False, "temporal_jitter_step": 2, "random_shift": False, "seed": 0}


def check_sampling(sampling):
    """``sampling`` (None or a dict with keys of ``SAMPLING_DEFAULTS``) completed with the defaults -- the reference *scripts'* settings
    (r2plus1d_main_universal_attack.py:155-163: step 1, no jitter, no shift).  Anything malformed is a ValueError."""
    if sampling is None:
        sampling = {}
    if not isinstance(sampling, dict):
        raise ValueError(f"sampling must be a dict with keys {sorted(SAMPLING_DEFAULTS)}, got {type(sampling).__name__}")
    unknown = sorted(set(sampling) - set(SAMPLING_DEFAULTS))
    if unknown:
        raise ValueError(f"sampling: unknown keys {unknown}; known: {sorted(SAMPLING_DEFAULTS)}")
    s = dict(SAMPLING_DEFAULTS, **sampling)
    for key in ("sample_step", "temporal_jitter_step"):
        v = s[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"sampling[{key!r}] must be an integer >= 1, got {v!r}")
        s[key] = int(v)
    for key in ("temporal_jitter", "random_shift"):
        if not isinstance(s[key], (bool, np.bool_)):
            raise ValueError(f"sampling[{key!r}] must be a bool, got {s[key]!r}")
        s[key] = bool(s[key])
    if isinstance(s["seed"], bool) or not isinstance(s["seed"], (int, np.integer)) or not 0 <= s["seed"] < 2 ** 32 - 4096:
        raise ValueError(f"sampling['seed'] must be an integer in [0, 2**32 - 4096) (a RandomState seed; the rank is added to it), got {s['seed']!r}")
    s["seed"] = int(s["seed"])
    return s


def split_sampling(sampling, sample_length, train):
    """The keyword arguments of ``sample_frame_indices`` for one side of the reference's train / test split (``split_train_test``,
    dataset.py:459-475) of the dataset settings ``sampling``.  The training split steps by ``temporal_jitter_step`` when jittering but
    keeps ``presample_length`` at the unjittered ``sample_length * sample_step``; the test split has no shift and no jitter."""
    s = check_sampling(sampling)
    presample = int(sample_length) * s["sample_step"]
    if train:
        return dict(sample_length=int(sample_length), sample_step=s["temporal_jitter_step"] if s["temporal_jitter"] else s["sample_step"],
                    temporal_jitter=s["temporal_jitter"], random_shift=s["random_shift"], presample_length=presample)
    return dict(sample_length=int(sample_length), sample_step=s["sample_step"], temporal_jitter=False, random_shift=False,
                presample_length=presample)


def sample_frame_indices(num_frames, sample_length, sample_step=1, num_samples=1, temporal_jitter=False, random_shift=False,
                         presample_length=None, rng=None):
    """Frame numbers of the ``num_samples`` clips the reference's ``VideoDataset`` cuts from a video of ``num_frames`` frames:
    ``_sample_indices`` then ``_get_frames`` (dataset.py:500-586) restated, int64 ``[num_samples, sample_length]``.  ``rng``: a
    ``numpy.random.RandomState`` (None: a fresh unseeded one); the draws are made in the reference's order, so ``RandomState(s)`` gives
    the tables the reference gives under ``np.random.seed(s)`` (it draws with ``numpy.random.randint``).

    Offsets: a video longer than ``presample_length`` (default ``sample_length * sample_step``; ``split_sampling`` says why it is an
    argument of its own) draws ONE ``randint(num_frames - presample_length + 1, size=num_samples)``, sorted, when ``random_shift``;
    otherwise offset x is ``int(d / 2 + d * x)`` with ``d = (num_frames - presample_length + 1) / num_samples``.  A video not longer
    than that starts every clip at frame 0.
    Frames, per clip in clip order: the offset, then ``sample_length - 1`` times a step -- ``randint(sample_step + 1)`` when
    ``temporal_jitter`` (0 repeats the previous frame), else ``sample_step``.  The first step that would pass the last frame ends the
    clip: no further draw is made and the rest of the clip repeats its last frame.

    The model of decord this rests on (decord is not available where this was written, so it is an assumption): after
    ``seek_accurate(o)`` a ``next()`` yields frame ``o``; ``skip_frames(k)`` advances by ``k`` without raising; a ``next()`` past the
    last frame raises ``StopIteration``."""
    N, T, step, S = int(num_frames), int(sample_length), int(sample_step), int(num_samples)
    P = T * step if presample_length is None else int(presample_length)
    if N < 1 or T < 1 or step < 1 or S < 1 or P < 1:
        raise ValueError(f"sample_frame_indices: num_frames {N}, sample_length {T}, sample_step {step}, num_samples {S} and "
                         f"presample_length {P} must all be >= 1")
    rng = np.random.RandomState() if rng is None else rng
    if N > P:
        if random_shift:
            offsets = np.sort(rng.randint(N - P + 1, size=S))
        else:
            d = (N - P + 1) / S
            offsets = np.array([int(d / 2.0 + d * x) for x in range(S)])
    else:
        offsets = np.zeros((S,), dtype=int)
    table = np.empty((S, T), np.int64)
    ramp = step * np.arange(T)
    for k, o in enumerate(offsets):
        cur, n = int(o), 1
        if not temporal_jitter:                    # o, o + step, ... while inside the video, then its last frame inside
            table[k] = np.minimum(cur + ramp, cur + (N - 1 - cur) // step * step)
            continue
        if cur + step * (T - 1) <= N - 1:          # no step can pass the last frame: all T - 1 draws are made -- as one call, which
            table[k, 0] = cur                      # leaves a RandomState where T - 1 single draws leave it
            table[k, 1:] = cur + np.cumsum(rng.randint(step + 1, size=T - 1))
            continue
        table[k, 0] = cur
        while n < T:
            st = int(rng.randint(step + 1))
            if st and cur + st > N - 1:
                break
            cur += st
            table[k, n] = cur
            n += 1
        table[k, n:] = cur
    return table


def flicker_rows(frame_numbers, period, phase=0):
    """The row of a period-``period`` flicker perturbation each frame carries on VIDEO time: ``rows = (frame_numbers - phase) mod period``,
    int32 of ``frame_numbers``' shape, never negative whatever the sign of ``phase``.  ``frame_numbers``: integers of any shape -- a table
    ``[clips, T]`` of ``sample_frame_indices`` or the numbers of a whole video; ``phase``: a scalar, or one value per clip (per leading row).
    By definition this is the rule of ``flk_adv_export_u8`` with ``delta_T = period`` and ``shift_p = phase`` (include/flicker_hip.h:
    "frame t takes row (t - shift_p) mod delta_T"), so a clip perturbed by these rows carries what the exported video shows at its frames."""
    n = np.asarray(frame_numbers)
    if n.dtype.kind not in "iu":
        raise ValueError(f"flicker_rows: frame numbers must be integers, got {n.dtype}")
    if isinstance(period, bool) or not isinstance(period, (int, np.integer)) or period < 1:
        raise ValueError(f"flicker_rows: period must be an integer >= 1, got {period!r}")
    ph = np.asarray(phase)
    if ph.dtype.kind not in "iu":
        raise ValueError(f"flicker_rows: phase must be an integer or one integer per clip, got {ph.dtype}")
    if ph.ndim:
        if ph.ndim != 1 or n.ndim < 1 or ph.shape[0] != n.shape[0]:
            raise ValueError(f"flicker_rows: {ph.shape} phases for frame numbers {n.shape}: one per clip (leading row) or a scalar")
        ph = ph.reshape((-1,) + (1,) * (n.ndim - 1))
    return np.mod(n.astype(np.int64) - ph.astype(np.int64), np.int64(period)).astype(np.int32, order="C")      # numpy's mod takes the divisor's sign


# ---- capture channel: the flicker as a camera records it ----------------------------------------------------------------------------
CAPTURE_MAX_EXPOSURE = 3.0      # emitter rows: with a sub-frame phase below 1 a frame then mixes at most 4 rows (flk_flicker_rows_mix's K)
CAPTURE_GAIN_MODES = ("common", "per_channel")


def capture_taps(subframe, exposure):
    """The weights a camera frame gives the rows of the flicker: frame n integrates the emitter over ``[n + subframe, n + subframe +
    exposure)`` (both in emitter rows), so it records ``sum_k w_k * delta[row(n) + k]`` with ``w_k = |[phi, phi + e) n [k, k + 1)| / e`` --
    fp32 ``[K]``, ``K = max(1, ceil(phi + e))``, computed in float64 and rounded once.  ``exposure`` 0: an instantaneous sample, ``[1]``.
    ``subframe`` must lie in [0,1) and ``exposure`` in [0,3]; anything else, or a non-finite value, is a ValueError."""
    try:
        phi, e = float(subframe), float(exposure)
    except (TypeError, ValueError):
        raise ValueError(f"capture_taps: subframe and exposure must be numbers, got {subframe!r} and {exposure!r}") from None
    if not (np.isfinite(phi) and 0.0 <= phi < 1.0):
        raise ValueError(f"capture_taps: the sub-frame phase must lie in [0,1), got {subframe!r}")
    if not (np.isfinite(e) and 0.0 <= e <= CAPTURE_MAX_EXPOSURE):
        raise ValueError(f"capture_taps: the exposure must lie in [0,{CAPTURE_MAX_EXPOSURE:g}] emitter rows, got {exposure!r}")
    if e == 0.0:
        return np.ones(1, np.float32)
    K = max(1, int(np.ceil(phi + e)))
    k = np.arange(K, dtype=np.float64)
    w = np.maximum(0.0, np.minimum(phi + e, k + 1.0) - np.maximum(phi, k)) / e
    return w.astype(np.float32)


def capture_line_taps(subframe, exposure, readout, H):
    """``capture_taps`` per LINE of a rolling-shutter frame of ``H`` lines: line h starts its exposure ``(readout * h) / H`` emitter rows
    after line 0 (``readout`` rho in [0,1]: the time from the start of line 0 to the start of a line one frame height further down), so it
    integrates the emitter over ``[n + psi_h, n + psi_h + e)`` with ``psi_h = subframe + (readout * h) / H`` -- float64, in exactly that
    order, in [0,2) -- and its taps follow ``capture_taps``' rule with psi_h in phi's place: ``w_k(h) = |[psi_h, psi_h + e) n [k, k + 1)| / e``.
    fp32 ``[H,K]``, ``K = max(1, ceil(max_h psi_h + e))`` <= 5, computed in float64 for all lines at once and rounded once; a line with
    psi_h < 1 holds the bits of ``capture_taps(psi_h, e)``, zero-padded.  ``exposure`` 0: an instantaneous sample, tap ``floor(psi_h)`` is 1
    (``K = floor(max_h psi_h) + 1``: the same number except where max psi_h is exactly 1).  Arguments as ``capture_taps``; ``readout``
    outside [0,1] or non-finite, or ``H < 1``, is a ValueError."""
    try:
        phi, e, rho = float(subframe), float(exposure), float(readout)
    except (TypeError, ValueError):
        raise ValueError(f"capture_line_taps: subframe, exposure and readout must be numbers, got {subframe!r}, {exposure!r} and {readout!r}") from None
    if not (np.isfinite(phi) and 0.0 <= phi < 1.0):
        raise ValueError(f"capture_line_taps: the sub-frame phase must lie in [0,1), got {subframe!r}")
    if not (np.isfinite(e) and 0.0 <= e <= CAPTURE_MAX_EXPOSURE):
        raise ValueError(f"capture_line_taps: the exposure must lie in [0,{CAPTURE_MAX_EXPOSURE:g}] emitter rows, got {exposure!r}")
    if not (np.isfinite(rho) and 0.0 <= rho <= 1.0):
        raise ValueError(f"capture_line_taps: the readout must lie in [0,1] emitter rows per frame height, got {readout!r}")
    if isinstance(H, bool) or not isinstance(H, (int, np.integer)) or H < 1:
        raise ValueError(f"capture_line_taps: the number of lines H must be an integer >= 1, got {H!r}")
    psi = phi + (rho * np.arange(int(H), dtype=np.float64)) / np.float64(int(H))
    if e == 0.0:
        at = np.floor(psi).astype(np.int64)
        w = np.zeros((int(H), int(at.max()) + 1), np.float32)
        w[np.arange(int(H)), at] = 1.0
        return w
    K = max(1, int(np.ceil(psi.max() + e)))
    k = np.arange(K, dtype=np.float64)[None, :]
    w = np.maximum(0.0, np.minimum((psi + e)[:, None], k + 1.0) - np.maximum(psi[:, None], k)) / e
    return w.astype(np.float32)


def _mix_tables(what, rows, clip_T, taps, gain):
    rows = np.asarray(rows)
    if rows.dtype.kind not in "iu" or rows.size < 1:
        raise ValueError(f"{what}: rows must be a non-empty integer table, got {rows.shape} {rows.dtype}")
    if isinstance(clip_T, bool) or not isinstance(clip_T, (int, np.integer)) or clip_T < 1 or rows.size % clip_T:
        raise ValueError(f"{what}: clip_T must be an integer >= 1 that divides the {rows.size} frames, got {clip_T!r}")
    nb = rows.size // int(clip_T)
    taps = np.asarray(taps)
    if taps.dtype != np.float32 or taps.ndim != 2 or taps.shape[0] != nb or not 1 <= taps.shape[1] <= 4:
        raise ValueError(f"{what}: taps must be float32 [{nb},K] with K in 1..4 (one row per clip), got {taps.shape} {taps.dtype}")
    if gain is not None:
        gain = np.asarray(gain)
        if gain.dtype != np.float32 or gain.shape != (nb, 3):
            raise ValueError(f"{what}: gain must be float32 [{nb},3] (one row per clip) or None, got {gain.shape} {gain.dtype}")
    return rows, nb, taps, gain


def flicker_rows_mix(delta, rows, clip_T, taps, gain=None):
    """``flk_flicker_rows_mix`` restated in numpy float32, operation for operation: ``delta`` fp32 ``[P,3]``, ``rows`` integers of any shape
    (frame i of the flattened table belongs to clip ``i // clip_T``), ``taps`` fp32 ``[clips,K]``, ``gain`` fp32 ``[clips,3]`` or None ->
    fp32 ``rows.shape + (3,)``.  ``r0 = clamp(rows[i], 0, P-1); acc = taps[b,0] * delta[r0]`` (the first product itself: a -0 stays -0), then
    ``acc = acc + taps[b,k] * delta[(r0 + k) mod P]`` for k = 1 .. K-1, then ``gain[b] * acc`` -- every product and sum rounded on its own."""
    what = "flicker_rows_mix"
    delta = np.asarray(delta)
    if delta.dtype != np.float32 or delta.ndim != 2 or delta.shape[1] != 3 or delta.shape[0] < 1:
        raise ValueError(f"{what}: delta must be float32 [P,3], got {delta.shape} {delta.dtype}")
    rows, nb, taps, gain = _mix_tables(what, rows, clip_T, taps, gain)
    P = delta.shape[0]
    r0 = np.clip(rows.reshape(-1).astype(np.int64), 0, P - 1)
    b = np.arange(r0.shape[0]) // int(clip_T)
    acc = taps[b, 0][:, None] * delta[r0]
    for k in range(1, taps.shape[1]):
        acc = acc + taps[b, k][:, None] * delta[(r0 + k) % P]
    if gain is not None:
        acc = gain[b] * acc
    assert acc.dtype == np.float32
    return np.ascontiguousarray(acc.reshape(rows.shape + (3,)))


def flicker_rows_mix_grad(g_clip, rows, clip_T, taps, gain, period):
    """``flk_flicker_rows_mix_grad`` restated in numpy float32, the transpose of ``flicker_rows_mix``: ``g_clip`` fp32 ``rows.shape + (3,)`` ->
    fp32 ``[period,3]``.  From +0, over the frames i ascending and within a frame the taps k ascending:
    ``g_rows[(rows[i] + k) mod P] += (gain[b] * taps[b,k]) * g_clip[i]`` (without a gain: ``taps[b,k] * g_clip[i]``), every product and sum
    rounded on its own; frames whose row lies outside [0,P) are skipped; a row nothing reaches stays +0.  ``period < K`` is legal."""
    what = "flicker_rows_mix_grad"
    rows, nb, taps, gain = _mix_tables(what, rows, clip_T, taps, gain)
    if isinstance(period, bool) or not isinstance(period, (int, np.integer)) or period < 1:
        raise ValueError(f"{what}: period must be an integer >= 1, got {period!r}")
    g = np.asarray(g_clip)
    if g.dtype != np.float32 or g.shape != rows.shape + (3,):
        raise ValueError(f"{what}: g_clip must be float32 {rows.shape + (3,)}, got {g.shape} {g.dtype}")
    P, K = int(period), taps.shape[1]
    g, r = g.reshape(-1, 3), rows.reshape(-1).astype(np.int64)
    b = np.arange(r.shape[0]) // int(clip_T)
    coef = taps[b][:, :, None] if gain is None else gain[b][:, None, :] * taps[b][:, :, None]          # [n,K,1 or 3]
    prod = coef * g[:, None, :]                                                                        # [n,K,3], one rounding each
    assert prod.dtype == np.float32
    target = (r[:, None] + np.arange(K)) % P
    out = np.zeros((P, 3), np.float32)
    for i in np.flatnonzero((r >= 0) & (r < P)):
        for k in range(K):
            out[target[i, k]] = out[target[i, k]] + prod[i, k]
    return out


def _lines_tables(what, rows, clip_T, taps, gain):
    rows = np.asarray(rows)
    if rows.dtype.kind not in "iu" or rows.size < 1:
        raise ValueError(f"{what}: rows must be a non-empty integer table, got {rows.shape} {rows.dtype}")
    if isinstance(clip_T, bool) or not isinstance(clip_T, (int, np.integer)) or clip_T < 1 or rows.size % clip_T:
        raise ValueError(f"{what}: clip_T must be an integer >= 1 that divides the {rows.size} frames, got {clip_T!r}")
    nb = rows.size // int(clip_T)
    taps = np.asarray(taps)
    if taps.dtype != np.float32 or taps.ndim != 3 or taps.shape[0] != nb or taps.shape[1] < 1 or not 1 <= taps.shape[2] <= 5:
        raise ValueError(f"{what}: taps must be float32 [{nb},H,K] with K in 1..5 (one table per clip), got {taps.shape} {taps.dtype}")
    if gain is not None:
        gain = np.asarray(gain)
        if gain.dtype != np.float32 or gain.shape != (nb, 3):
            raise ValueError(f"{what}: gain must be float32 [{nb},3] (one row per clip) or None, got {gain.shape} {gain.dtype}")
    return rows, nb, taps, gain


def flicker_lines_mix(delta, rows, clip_T, taps, gain=None):
    """``flk_flicker_lines_mix`` restated in numpy float32, operation for operation: ``delta`` fp32 ``[P,3]``, ``rows`` integers of any shape
    (frame i of the flattened table belongs to clip ``i // clip_T``), ``taps`` fp32 ``[clips,H,K]``, ``gain`` fp32 ``[clips,3]`` or None ->
    fp32 ``rows.shape + (H,3)``.  Per line h the arithmetic of ``flicker_rows_mix`` with the line's taps: ``acc = taps[b,h,0] * delta[r0]``
    (the first product itself), then ``acc = acc + taps[b,h,k] * delta[(r0 + k) mod P]``, then ``gain[b] * acc`` -- each rounded on its own."""
    what = "flicker_lines_mix"
    delta = np.asarray(delta)
    if delta.dtype != np.float32 or delta.ndim != 2 or delta.shape[1] != 3 or delta.shape[0] < 1:
        raise ValueError(f"{what}: delta must be float32 [P,3], got {delta.shape} {delta.dtype}")
    rows, nb, taps, gain = _lines_tables(what, rows, clip_T, taps, gain)
    P, H = delta.shape[0], taps.shape[1]
    r0 = np.clip(rows.reshape(-1).astype(np.int64), 0, P - 1)
    b = np.arange(r0.shape[0]) // int(clip_T)
    acc = taps[b, :, 0][:, :, None] * delta[r0][:, None, :]                                            # [n,H,3]
    for k in range(1, taps.shape[2]):
        acc = acc + taps[b, :, k][:, :, None] * delta[(r0 + k) % P][:, None, :]
    if gain is not None:
        acc = gain[b][:, None, :] * acc
    assert acc.dtype == np.float32
    return np.ascontiguousarray(acc.reshape(rows.shape + (H, 3)))


def flicker_lines_mix_grad(g_lines, rows, clip_T, taps, gain, period):
    """``flk_flicker_lines_mix_grad`` restated in numpy float32, the transpose of ``flicker_lines_mix`` in the kernels' two stages:
    ``g_lines`` fp32 ``rows.shape + (H,3)`` -> fp32 ``[period,3]``.  Stage 1: ``s[i,k] = sum over the lines h ascending, from +0, of
    (gain[b] * taps[b,h,k]) * g_lines[i,h]`` (without a gain: ``taps[b,h,k] * g_lines[i,h]``).  Stage 2: from +0, over the frames i
    ascending and within a frame the taps k ascending, ``g_rows[(rows[i] + k) mod P] += s[i,k]``; frames whose row lies outside [0,P)
    are skipped, a row nothing reaches stays +0, ``period < K`` is legal.  Every product and sum rounded on its own."""
    what = "flicker_lines_mix_grad"
    rows, nb, taps, gain = _lines_tables(what, rows, clip_T, taps, gain)
    if isinstance(period, bool) or not isinstance(period, (int, np.integer)) or period < 1:
        raise ValueError(f"{what}: period must be an integer >= 1, got {period!r}")
    H, K = taps.shape[1], taps.shape[2]
    g = np.asarray(g_lines)
    if g.dtype != np.float32 or g.shape != rows.shape + (H, 3):
        raise ValueError(f"{what}: g_lines must be float32 {rows.shape + (H, 3)}, got {g.shape} {g.dtype}")
    P = int(period)
    g, r = g.reshape(-1, H, 3), rows.reshape(-1).astype(np.int64)
    b = np.arange(r.shape[0]) // int(clip_T)
    s = np.zeros((r.shape[0], K, 3), np.float32)
    for h in range(H):
        coef = taps[b, h][:, :, None] if gain is None else gain[b][:, None, :] * taps[b, h][:, :, None]      # [n,K,1 or 3]
        s = s + coef * g[:, h][:, None, :]
    assert s.dtype == np.float32
    target = (r[:, None] + np.arange(K)) % P
    out = np.zeros((P, 3), np.float32)
    for i in np.flatnonzero((r >= 0) & (r < P)):
        for k in range(K):
            out[target[i, k]] = out[target[i, k]] + s[i, k]
    return out


# ---- the flicker as scene illumination (include/flicker_hip.h: flk_illum_*) ---------------------------------------------------------
FLICKER_MODELS = ("additive", "illumination")
ILLUM_RESPONSES = ("srgb", "linear")
ILLUM_N = 4096                  # segments of the built-in encode tables
ILLUM_MAX_N = 16384             # what the kernels stage in LDS


def illum_out_affine():
    """(out_mul, out_add) of the torch dialect, float32 [3] each: a display value e in [0,1] becomes ``e * (1 / std) + (-mean / std)``"""
    mean, std = np.array(DEFAULT_MEAN, np.float32), np.array(DEFAULT_STD, np.float32)
    return (np.float32(1.0) / std).astype(np.float32), (-mean / std).astype(np.float32)


def illum_tables(response="srgb"):
    """The camera curves of the illumination model as tables: ``dec`` float32 [256,3], the linear light in [0,1] of byte v of channel c,
    and ``enc`` float32 [N+1], the display value in [0,1] of linear light i / N, non-decreasing, interpolated linearly in between.
    ``response``: "srgb" (IEC 61966-2-1, N = 4096), "linear" (dec = v / 255, enc = i / N, N = 4096), or a pair of arrays (dec, enc) --
    a measured curve, N = len(enc) - 1 in 2..16384.  Every pair must give every byte back under no modulation (the round trip of
    ``illum_export_host`` with delta = 0 over all 256 levels x 3 channels); a pair that does not raises ValueError."""
    if isinstance(response, str):
        if response not in ILLUM_RESPONSES:
            raise ValueError(f"illum_tables: response must be one of {ILLUM_RESPONSES} or a (dec, enc) pair of arrays, got {response!r}")
        v, g = np.arange(256, dtype=np.float64) / 255.0, np.arange(ILLUM_N + 1, dtype=np.float64) / ILLUM_N
        if response == "srgb":
            lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
            enc = np.where(g <= 0.0031308, 12.92 * g, 1.055 * g ** (1.0 / 2.4) - 0.055)
        else:
            lin, enc = v, g
        dec = np.repeat(lin[:, None], 3, axis=1)
    else:
        try:
            dec, enc = response
            dec, enc = np.asarray(dec, dtype=np.float64), np.asarray(enc, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("illum_tables: response must be \"srgb\", \"linear\" or a (dec, enc) pair of arrays") from None
        if dec.shape != (256, 3) or enc.ndim != 1 or not 3 <= enc.shape[0] <= ILLUM_MAX_N + 1:
            raise ValueError(f"illum_tables: dec must be [256,3] and enc [N+1] with N in 2..{ILLUM_MAX_N}, got {dec.shape} and {enc.shape}")
    dec, enc = np.ascontiguousarray(dec, dtype=np.float32), np.ascontiguousarray(np.clip(enc, 0.0, 1.0) if isinstance(response, str) else enc, dtype=np.float32)
    if not (np.isfinite(dec).all() and np.isfinite(enc).all() and dec.min() >= 0 and dec.max() <= 1 and enc.min() >= 0 and enc.max() <= 1):
        raise ValueError("illum_tables: the values of dec and enc must lie in [0,1]")
    if (np.diff(enc) < 0).any():
        raise ValueError("illum_tables: enc must be non-decreasing")
    levels = np.ascontiguousarray(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1).reshape(1, 1, 16, 16, 3))
    back = illum_export_host(levels, np.zeros((1, 3), np.float32), (dec, enc))
    if not np.array_equal(back, levels):
        miss = int((back != levels).sum())
        raise ValueError(f"illum_tables: the pair does not give every byte back under no modulation ({miss} of 768 (level, channel) entries miss)")
    return dec, enc


def _illum_tables_checked(tables):
    dec, enc = tables
    dec, enc = np.asarray(dec), np.asarray(enc)
    if dec.dtype != np.float32 or dec.shape != (256, 3) or enc.dtype != np.float32 or enc.ndim != 1 or not 3 <= enc.shape[0] <= ILLUM_MAX_N + 1:
        raise ValueError(f"illumination tables: dec float32 [256,3] and enc float32 [N+1], N in 2..{ILLUM_MAX_N}, got {dec.shape} {dec.dtype} and {enc.shape} {enc.dtype}")
    return dec, enc


def _illum_factor(x, delta, dclip, dclip_clip, adv_flag, shift_p, delta_T, per_line):
    """s = 1 + adv_flag * clamp(delta), float32, broadcastable against [B,T,H,W,3]"""
    f32 = np.float32
    B, T, H = x.shape[:3]
    d = np.asarray(delta)
    if d.dtype != np.float32:
        raise ValueError(f"illumination: delta must be float32, got {d.dtype}")
    period = int(delta_T) or T
    rows = (np.arange(T) - int(shift_p)) % period                   # frame t carries row (t - shift_p) mod period
    if per_line:
        if d.shape == (period, H, 3):
            m = d[rows][None, :, :, None, :]
        elif d.shape == (B, T, H, 3) and not delta_T:
            m = d[:, rows][:, :, :, None, :]
        else:
            raise ValueError(f"illumination: a per-line delta is [{period},{H},3] or [{B},{T},{H},3], got {d.shape}")
    elif d.shape == (period, 3):
        m = d[rows][None, :, None, None, :]
    elif d.shape == (B, T, 3) and not delta_T:
        m = d[:, rows][:, :, None, None, :]
    else:
        raise ValueError(f"illumination: delta is [{period},3] or [{B},{T},3] (per_line: [{period},{H},3] or [{B},{T},{H},3]), got {d.shape}")
    dc = np.asarray(dclip_clip, f32).reshape(B, 1, 1, 1, 1) if dclip_clip is not None else f32(dclip)
    inside = np.ones(m.shape, bool)
    if dclip_clip is not None or dclip > 0:
        with np.errstate(invalid="ignore"):
            inside = np.broadcast_to((m >= -dc) & (m <= dc), np.broadcast_shapes(m.shape, np.shape(dc)))
        m = np.fmin(np.fmax(m, -dc), dc)
    s = (f32(1.0) + (f32(adv_flag) * m).astype(f32)).astype(f32)
    return s, inside, rows


def _illum_display(by, s, dec, enc):
    """per value: (e, p, L, d) of the header's formulas, float32, one rounded operation per step"""
    f32 = np.float32
    N = enc.shape[0] - 1
    L = dec[by, np.arange(3)]
    p = (L * s).astype(f32)
    u = np.fmin(np.fmax(p, f32(0.0)), f32(1.0))                     # (fmax / fmin: a NaN becomes 0, as on the device)
    z = (u * f32(N)).astype(f32)
    i = np.minimum(z.astype(np.int64), N - 1)
    f = (z - i.astype(f32)).astype(f32)
    e0 = enc[i]
    d = (enc[i + 1] - e0).astype(f32)
    e = (e0 + (f * d).astype(f32)).astype(f32)
    return e, p, L, d


def _illum_byte(e):
    z = (e * np.float32(255.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(z >= 0, np.minimum(np.rint(z), np.float32(255.0)), np.float32(0.0)).astype(np.uint8)


def _illum_clip(x):
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim != 5 or x.shape[4] != 3:
        raise ValueError(f"illumination: the clip must be uint8 [B,T,H,W,3], got {x.shape} {x.dtype}")
    return x


def illum_export_host(x, delta, tables, *, dclip=0.0, adv_flag=1.0, shift_x=0, shift_p=0, dclip_clip=None, delta_T=0, per_line=False, stats=False):
    """``flk_illum_export_u8`` restated in numpy float32 (one rounded operation per step): the bytes a camera stores of the uint8 clip
    ``x`` [B,T,H,W,3] lit by the flicker ``delta`` ([T,3], [B,T,3], with ``delta_T`` [delta_T,3]; ``per_line``: [T,H,3], [B,T,H,3] or
    [delta_T,H,3]).  With ``stats`` also the int64 [B,T,3,4] sums of q - v, |q - v|, [q != v] and [p outside [0,1]]."""
    x = _illum_clip(x)
    dec, enc = _illum_tables_checked(tables)
    s, _, _ = _illum_factor(x, delta, dclip, dclip_clip, adv_flag, shift_p, delta_T, per_line)
    src = np.roll(x, int(shift_x), axis=1)                           # x'[t] = x[(t - shift_x) mod T]
    e, p, _, _ = _illum_display(src, s, dec, enc)
    q = _illum_byte(e)
    if not stats:
        return q
    dq = q.astype(np.int64) - src.astype(np.int64)
    with np.errstate(invalid="ignore"):
        outside = (p < 0) | (p > 1)
    return q, np.stack([dq.sum((2, 3)), np.abs(dq).sum((2, 3)), (dq != 0).sum((2, 3)), outside.sum((2, 3))], axis=-1).astype(np.int64)


def illum_apply_host(x, delta, tables, *, dclip=0.0, adv_flag=1.0, shift_x=0, shift_p=0, dclip_clip=None, per_line=False, out_mul=None, out_add=None,
                     q_lut=None):
    """``flk_illum_apply_s2d`` restated in numpy float32, unfolded: the fp32 clip [B,T,H,W,3] the network sees.  Plain: ``e * out_mul +
    out_add`` (default ``illum_out_affine``); with ``q_lut`` (float32 [256,3]) the decode of the stored byte.  ``adv_flag`` = 0 is the
    clean clip of the additive entry point and is not restated here."""
    if adv_flag == 0:
        raise ValueError("illum_apply_host: adv_flag = 0 is the clean clip (flk_perturb_apply_s2d), not restated here")
    x = _illum_clip(x)
    dec, enc = _illum_tables_checked(tables)
    s, _, _ = _illum_factor(x, delta, dclip, dclip_clip, adv_flag, shift_p, 0, per_line)
    e, _, _, _ = _illum_display(np.roll(x, int(shift_x), axis=1), s, dec, enc)
    if q_lut is not None:
        return np.ascontiguousarray(np.asarray(q_lut, np.float32)[_illum_byte(e), np.arange(3)])
    mul, add = illum_out_affine()
    mul, add = (mul if out_mul is None else np.asarray(out_mul, np.float32)), (add if out_add is None else np.asarray(out_add, np.float32))
    return np.ascontiguousarray(((e * mul).astype(np.float32) + add).astype(np.float32))


def illum_grad_host(x, delta, tables, gx, *, dclip=0.0, adv_flag=1.0, shift_x=0, shift_p=0, dclip_clip=None, per_line=False, out_mul=None,
                    bound=False):
    """``flk_illum_grad_reduce`` restated: d(loss)/d(delta) from ``gx`` = d(loss)/d(x_adv), [B,T,H,W,3] unfolded.  The per-value weight
    ``(d * N) * L`` is the kernel's (float32, two rounded products); the products with ``gx``, the sums and the finishing factor
    ``adv_flag * out_mul[c]`` are float64.  Returns float64 in the shape of ``delta`` ([T,3], [B,T,3]; ``per_line``: [B,T,H,3] from a
    per-clip delta); with ``bound`` also the sum of the magnitudes of each output's terms and their number."""
    x = _illum_clip(x)
    dec, enc = _illum_tables_checked(tables)
    B, T, H, W = x.shape[:4]
    gx = np.asarray(gx, dtype=np.float64)
    if gx.shape != x.shape:
        raise ValueError(f"illum_grad_host: gx must have the clip's shape {x.shape}, got {gx.shape}")
    s, inside, rows = _illum_factor(x, delta, dclip, dclip_clip, adv_flag, shift_p, 0, per_line)
    d_shape = np.asarray(delta).shape
    per_clip = len(d_shape) == (4 if per_line else 3)
    if per_line and not per_clip:
        raise ValueError("illum_grad_host: the per-line gradient needs a per-clip delta [B,T,H,3]")
    _, p, L, d = _illum_display(np.roll(x, int(shift_x), axis=1), s, dec, enc)
    w = ((d * np.float32(enc.shape[0] - 1)).astype(np.float32) * L).astype(np.float32)
    with np.errstate(invalid="ignore"):
        live = (p >= 0) & (p <= 1)
    mul = illum_out_affine()[0] if out_mul is None else np.asarray(out_mul, np.float32)
    terms = np.where(live, gx * w.astype(np.float64), 0.0) * (float(np.float32(adv_flag)) * mul.astype(np.float64))
    axes = (3,) if per_line else (2, 3) if per_clip else (0, 2, 3)
    n = W if per_line else H * W if per_clip else B * H * W
    keep = np.broadcast_to(inside, (B if per_clip else 1, T, H if per_line else 1, 1, 3)).reshape(d_shape)     # by frame t: rolled back below
    g_t, mag_t = terms.sum(axes), np.abs(terms).sum(axes)                # indexed by frame t; delta row rows[t] receives it
    g, mag = np.zeros(d_shape), np.zeros(d_shape)
    t_axis = 1 if per_clip else 0
    idx = [slice(None)] * len(d_shape)
    idx[t_axis] = rows
    g[tuple(idx)], mag[tuple(idx)] = np.where(keep, g_t, 0.0), np.where(keep, mag_t, 0.0)
    return (g, mag, n) if bound else g


# ---- training on the delivered video at its native resolution: tone tables, their slopes, the gradient through the resampling ------
def tone_ramp_host(n, T):
    """uint8 [n,T,16,16,3]: pixel p of every frame holds level p in its three channels (ops.tone_ramp on the host)"""
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16, 1)
    return np.ascontiguousarray(np.broadcast_to(ramp, (int(n), int(T), 16, 16, 3)))


def additive_bounds():
    """(lo, hi) of the torch dialect's additive clamp: the largest normalised value of byte 0 and the smallest of byte 255 over the
    channels (model.py:72-75) -- what ``Perturbation`` clamps the perturbed clip to"""
    mean, std = np.array(DEFAULT_MEAN), np.array(DEFAULT_STD)
    return float(np.max((0.0 - mean) / std)), float(np.min((1 - mean) / std))


def _tone_delta(delta_clip):
    d = np.asarray(delta_clip)
    if d.dtype != np.float32 or d.ndim != 3 or d.shape[2] != 3:
        raise ValueError(f"tone tables: the per-clip delta must be float32 [n,T,3], got {d.shape} {d.dtype}")
    return d


def tone_tables_host(delta_clip, tables=None, *, dclip=0.0, adv_flag=1.0, lo=None, hi=None, dclip_clip=None):
    """``ops.flicker_tone_tables`` restated: uint8 [n,T,256,3], the byte source byte v of channel c is stored as under the delta row of
    frame t of clip k -- the host export of the pixel model (``ops.export_adversarial_u8_host`` in the torch dialect; with ``tables`` =
    ``illum_tables(...)``, ``illum_export_host``) on the ramp clip.  ``delta_clip``: float32 [n,T,3] (flicker_rows / flicker_rows_mix);
    ``lo`` / ``hi``: the additive clamp (default ``additive_bounds``)."""
    d = _tone_delta(delta_clip)
    n, T = d.shape[:2]
    ramp = tone_ramp_host(n, T)
    if tables is not None:
        q = illum_export_host(ramp, d, tables, dclip=dclip, adv_flag=adv_flag, dclip_clip=dclip_clip)
    else:
        from .ops import export_adversarial_u8_host
        lo0, hi0 = additive_bounds()
        q = export_adversarial_u8_host(ramp, d, dialect="torch", dclip=dclip, adv_flag=adv_flag, inv_std=tuple(1.0 / s for s in DEFAULT_STD),
                                       lo=lo0 if lo is None else lo, hi=hi0 if hi is None else hi, dclip_clip=dclip_clip, x_lut=u8_decode_table())
    return np.ascontiguousarray(q.reshape(n, T, 256, 3))


def tone_slopes_host(delta_clip, tables=None, *, dclip=0.0, adv_flag=1.0, lo=None, hi=None, dclip_clip=None, out_mul=None):
    """flk_flicker_tone_slopes restated in numpy float32: ``(slope [n,T,256,3], scale [n,T,3])``.  Additive (``tables`` None): slope = 1
    where ``lo <= x_lut[v,c] + adv_flag * clamp(delta) / std <= hi``, scale = ``adv_flag / std``; illumination: slope = the weight
    ``(d * N) * L`` of ``illum_grad_host``, 0 where the lit value leaves [0,1], scale = ``adv_flag * out_mul``.  scale is 0 where the
    delta value lies outside its clamp."""
    f32 = np.float32
    d = _tone_delta(delta_clip)
    n, T = d.shape[:2]
    dc = np.asarray(dclip_clip, f32).reshape(n, 1, 1) if dclip_clip is not None else f32(dclip)
    clamped = dclip_clip is not None or dclip > 0
    with np.errstate(invalid="ignore"):
        inside = ((d >= -dc) & (d <= dc)) if clamped else np.ones(d.shape, bool)
    if tables is not None:
        dec, enc = _illum_tables_checked(tables)
        ramp = tone_ramp_host(n, T)
        s, _, _ = _illum_factor(ramp, d, dclip, dclip_clip, adv_flag, 0, 0, False)
        _, p, L, dd = _illum_display(ramp, s, dec, enc)
        w = ((dd * f32(enc.shape[0] - 1)).astype(f32) * L).astype(f32)
        with np.errstate(invalid="ignore"):
            slope = np.where((p >= 0) & (p <= 1), w, f32(0.0)).astype(f32).reshape(n, T, 256, 3)
        mul = illum_out_affine()[0] if out_mul is None else np.asarray(out_mul, f32)
        factor = (f32(adv_flag) * mul).astype(f32)
    else:
        inv_std = np.array([1.0 / s for s in DEFAULT_STD]).astype(f32)
        lo0, hi0 = additive_bounds()
        lo, hi = f32(lo0 if lo is None else lo), f32(hi0 if hi is None else hi)
        m = np.fmin(np.fmax(d, -dc), dc) if clamped else d
        p = (m * inv_std).astype(f32)
        u = (u8_decode_table()[None, None] + (f32(adv_flag) * p).astype(f32)[:, :, None, :]).astype(f32)
        slope = ((u >= lo) & (u <= hi)).astype(f32)
        factor = (f32(adv_flag) * inv_std).astype(f32)
    scale = np.where(inside, np.broadcast_to(factor, d.shape), f32(0.0)).astype(f32)
    return np.ascontiguousarray(slope), np.ascontiguousarray(scale)


def _prep_axis(step, d, n_in):
    """source indices and the weight of the second one along an axis, as csrc/prepare.hip evaluates them in float32: src =
    max(fma(step, d + 0.5, -0.5), 0), i0 = min(int(src), n_in - 1), i1 = min(i0 + 1, n_in - 1), lambda = clamp(src - i0, 0, 1).  (The
    fused multiply-subtract is formed in float64, where it is exact, and rounded once.)"""
    d = np.asarray(d, dtype=np.int64)
    s = (np.float64(np.float32(step)) * (d.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    s = np.maximum(s, np.float32(0.0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = np.clip((s - i0.astype(np.float32)).astype(np.float32), np.float32(0.0), np.float32(1.0))
    return i0, i1, lam


def _blend_axis(v, i0, i1, lam, axis):
    """(1 - lambda) * v[i0] + lambda * v[i1] along ``axis``: the weights are the kernels' float32 values (1 - lambda rounded to float32
    as there), the products and the sum float64"""
    w1 = lam.astype(np.float64)
    w0 = (np.float32(1.0) - lam).astype(np.float32).astype(np.float64)
    shape = [1] * v.ndim
    shape[axis] = -1
    return w0.reshape(shape) * np.take(v, i0, axis=axis) + w1.reshape(shape) * np.take(v, i1, axis=axis)


def prepare_resample_host(values, box=None, flip=False, im_scale=128, input_size=112, rule="sizes"):
    """The resampling of csrc/prepare.hip on per-pixel VALUES, in float64: ``values`` [Hs,Ws,3] (any real numbers: decoded pixels, or
    slopes) -> [Ho,Wo,3].  The source indices and the interpolation weights are the kernels' own float32 numbers; the blends --
    along W within the two source rows, then along H; then, for a ``box = (i, j, h, w)`` of the resized image that is not of the
    output size, the second bilinear stage -- are float64.  ``box`` None: the evaluation transform's crop window.  ``flip``: mirrored
    along W.  No mean, no std: the map is linear in ``values``."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 3 or v.shape[2] != 3:
        raise ValueError(f"prepare_resample_host: values must be [Hs,Ws,3], got {v.shape}")
    Hs, Ws = v.shape[:2]
    Ho, Wo = _pair(input_size)
    Hr, Wr, step_h, step_w, ci, cj = prepare_geometry(Hs, Ws, im_scale, input_size, rule)
    i, j, h, w = (ci, cj, Ho, Wo) if box is None else (int(b) for b in box)
    if h < 1 or w < 1 or i < 0 or j < 0 or i + h > Hr or j + w > Wr:
        raise ValueError(f"prepare_resample_host: box ({i},{j})+{h}x{w} outside the resized image {Hr} x {Wr}")
    c0, c1, lw = _prep_axis(step_w, j + np.arange(w), Ws)
    r0, r1, lh = _prep_axis(step_h, i + np.arange(h), Hs)
    R = _blend_axis(_blend_axis(v, c0, c1, lw, 1), r0, r1, lh, 0)               # [h,w,3]: the resized image under the box
    if (h, w) != (Ho, Wo):
        step2_h, step2_w = np.float32(h) / np.float32(Ho), np.float32(w) / np.float32(Wo)
        x0, x1, lw2 = _prep_axis(step2_w, np.arange(Wo), w)
        y0, y1, lh2 = _prep_axis(step2_h, np.arange(Ho), h)
        R = _blend_axis(_blend_axis(R, x0, x1, lw2, 1), y0, y1, lh2, 0)
    return np.ascontiguousarray(R[:, ::-1] if flip else R)


def prepare_grad_host(video, frame_idx, gx, slope, scale, box=None, flip=False, im_scale=128, input_size=112, rule="sizes", bound=False):
    """flk_clip_prepare_grad restated in float64 for ONE clip: ``video`` uint8 [N,Hs,Ws,3], ``frame_idx`` the clip's T_out frame numbers,
    ``gx`` = d(loss)/d(prepared clip) [T_out,Ho,Wo,3] (unfolded), ``slope`` [T_out,256,3] and ``scale`` [T_out,3] of the clip
    (``tone_slopes_host``).  Returns float64 [T_out,3]: ``scale[t,c] * sum over (oh, ow) of gx * J``, J = ``prepare_resample_host`` of
    the frame's per-byte slopes.  ``bound``: also the sum of the magnitudes of each output's terms (times |scale|) and their number."""
    video, gx = np.asarray(video), np.asarray(gx, dtype=np.float64)
    if video.dtype != np.uint8 or video.ndim != 4 or video.shape[3] != 3:
        raise ValueError(f"prepare_grad_host: video must be uint8 [N,Hs,Ws,3], got {video.shape} {video.dtype}")
    idx = np.asarray(frame_idx, dtype=np.int64).reshape(-1)
    Ho, Wo = _pair(input_size)
    slope, scale = np.asarray(slope, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    if gx.shape != (idx.size, Ho, Wo, 3) or slope.shape != (idx.size, 256, 3) or scale.shape != (idx.size, 3):
        raise ValueError(f"prepare_grad_host: gx [{idx.size},{Ho},{Wo},3], slope [{idx.size},256,3], scale [{idx.size},3]; got {gx.shape}, "
                         f"{slope.shape}, {scale.shape}")
    g, mag = np.zeros((idx.size, 3)), np.zeros((idx.size, 3))
    for t, f in enumerate(idx):
        J = prepare_resample_host(slope[t][video[f], np.arange(3)], box, flip, im_scale, input_size, rule)
        terms = gx[t] * J
        g[t], mag[t] = terms.sum((0, 1)) * scale[t], np.abs(terms).sum((0, 1)) * np.abs(scale[t])
    return (g, mag, Ho * Wo) if bound else g


def _axis_matrix(i0, i1, lam, n_in):
    """one bilinear stage along an axis as a float64 matrix [len(i0), n_in]: row d holds float32(1 - lambda) at i0 and lambda at i1
    (added where the two coincide), the weights ``_blend_axis`` uses"""
    A = np.zeros((len(i0), n_in))
    rows = np.arange(len(i0))
    np.add.at(A, (rows, i0), (np.float32(1.0) - lam).astype(np.float32).astype(np.float64))
    np.add.at(A, (rows, i1), lam.astype(np.float64))
    return A


def prepare_adjoint_matrices(Hs, Ws, box=None, flip=False, im_scale=128, input_size=112, rule="sizes"):
    """The resampling of csrc/prepare.hip as two matrices: ``prepare_resample_host(V) = A_h V A_w^T`` per channel.  ``(A_h [Ho,Hs],
    A_w [Wo,Ws])`` float32: per axis the composite ``S2 S1`` of the two bilinear stages (``_prep_axis`` indices and lambdas of the
    forward; stage 2 skipped for a box of the output size, as there; the flip is the reversed row order of A_w), formed in float64
    and rounded ONCE to float32."""
    Hs, Ws = int(Hs), int(Ws)
    Ho, Wo = _pair(input_size)
    Hr, Wr, step_h, step_w, ci, cj = prepare_geometry(Hs, Ws, im_scale, input_size, rule)
    i, j, h, w = (ci, cj, Ho, Wo) if box is None else (int(b) for b in box)
    if h < 1 or w < 1 or i < 0 or j < 0 or i + h > Hr or j + w > Wr:
        raise ValueError(f"prepare_adjoint_matrices: box ({i},{j})+{h}x{w} outside the resized image {Hr} x {Wr}")
    A_h = _axis_matrix(*_prep_axis(step_h, i + np.arange(h), Hs), Hs)
    A_w = _axis_matrix(*_prep_axis(step_w, j + np.arange(w), Ws), Ws)
    if (h, w) != (Ho, Wo):
        A_h = _axis_matrix(*_prep_axis(np.float32(h) / np.float32(Ho), np.arange(Ho), h), h) @ A_h
        A_w = _axis_matrix(*_prep_axis(np.float32(w) / np.float32(Wo), np.arange(Wo), w), w) @ A_w
    if flip:
        A_w = A_w[::-1]
    return np.ascontiguousarray(A_h.astype(np.float32)), np.ascontiguousarray(A_w.astype(np.float32))


def _adjoint_ranges(A):
    """a matrix [n_out, n_in] by SOURCE index: (first_out [n_in], count [n_in]) of the outputs with a non-zero weight -- a contiguous
    range, both stages being monotone (zeros inside it are kept); a source index no output reads has count 0"""
    nz = A != 0
    any_ = nz.any(0)
    first = np.where(any_, nz.argmax(0), 0)
    last = np.where(any_, A.shape[0] - 1 - nz[::-1].argmax(0), -1)
    return first.astype(np.int64), (last - first + 1).astype(np.int64)


def prepare_adjoint_tables(sizes, boxes=None, flips=None, im_scale=128, input_size=112, rule="sizes"):
    """The tables flk_clip_prepare_grad_image reads, for the clips of one call: ``sizes`` a list of ``(Hs, Ws)``, ``boxes`` / ``flips`` as
    ``ops.prepare_clips`` takes them (None: the evaluation transform).  Returns ``(words, offsets, K)``: ``words`` int32, per clip its
    row table then its column table, entry s of a table being ``2 + K`` words ``(first_out, count, w[K] as float32 bits)`` -- column s
    of ``prepare_adjoint_matrices``' A_h or A_w over its range, zero-filled to K; ``offsets[k] = (tab_h, tab_w)`` in words; ``K`` the
    largest count of the call."""
    if (boxes is None) != (flips is None):
        raise ValueError("prepare_adjoint_tables: boxes and flips go together")
    mats = [prepare_adjoint_matrices(Hs, Ws, None if boxes is None else boxes[k], False if flips is None else bool(flips[k]), im_scale,
                                     input_size, rule) for k, (Hs, Ws) in enumerate(sizes)]
    ranges = [[_adjoint_ranges(A) for A in pair] for pair in mats]
    K = max(1, max(int(cnt.max()) for pair in ranges for _, cnt in pair))
    parts, offsets, at = [], [], 0
    for pair, rng in zip(mats, ranges):
        off = []
        for A, (first, cnt) in zip(pair, rng):
            e = np.zeros((A.shape[1], 2 + K), np.int32)
            e[:, 0], e[:, 1] = first, cnt
            take = np.minimum(first[:, None] + np.arange(K)[None], A.shape[0] - 1)
            w = np.where(np.arange(K)[None] < cnt[:, None], A[take, np.arange(A.shape[1])[:, None]], np.float32(0.0)).astype(np.float32)
            e[:, 2:] = w.view(np.int32)
            parts.append(e.reshape(-1))
            off.append(at)
            at += e.size
        offsets.append(tuple(off))
    return np.concatenate(parts), offsets, K


def prepare_grad_image_host(g, Hs, Ws, box=None, flip=False, im_scale=128, input_size=112, rule="sizes", bound=False):
    """flk_clip_prepare_grad_image restated in float64 for ONE frame: ``g`` = d(loss)/d(prepared frame) ``[Ho,Wo,3]`` -> the gradient
    with respect to the source frame ``[Hs,Ws,3]``, ``A_h^T g A_w`` with the float32 matrices of ``prepare_adjoint_matrices`` (the
    kernel's tables).  ``bound``: also the same product on magnitudes and the number of float32 roundings of an output in the
    kernel's order (count_h * count_w fused row terms and count_h fused column terms, at their largest)."""
    g = np.asarray(g, dtype=np.float64)
    Ho, Wo = _pair(input_size)
    if g.shape != (Ho, Wo, 3):
        raise ValueError(f"prepare_grad_image_host: g must be [{Ho},{Wo},3], got {g.shape}")
    A_h, A_w = (A.astype(np.float64) for A in prepare_adjoint_matrices(Hs, Ws, box, flip, im_scale, input_size, rule))
    back = lambda Ah, v, Aw: np.tensordot(np.tensordot(Ah, v, axes=(0, 0)), Aw, axes=(1, 0)).transpose(0, 2, 1)      # [Hs,Ws,3]
    out = back(A_h, g, A_w)
    if not bound:
        return out
    kh, kw = (int(_adjoint_ranges(A)[1].max()) for A in (A_h, A_w))
    return out, back(np.abs(A_h), np.abs(g), np.abs(A_w)), kh * kw + kh


def _capture_range(name, v, lo_bound, hi_bound):
    pair = (v, v) if np.ndim(v) == 0 else tuple(v)
    if len(pair) != 2:
        raise ValueError(f"CaptureChannel: {name} must be a number or a (lo, hi) pair, got {v!r}")
    lo, hi = float(pair[0]), float(pair[1])
    if not (np.isfinite(lo) and np.isfinite(hi) and lo_bound <= lo <= hi <= hi_bound):
        raise ValueError(f"CaptureChannel: {name} must satisfy {lo_bound:g} <= lo <= hi <= {hi_bound:g}, got {v!r}")
    return lo, hi


class CaptureChannel:
    """The distribution a capture channel is drawn from (host only): a camera that is not synchronised with the emitter records frame n
    as the emitter integrated over ``[n + subframe, n + subframe + exposure)`` (``capture_taps``), each channel scaled by a gain (the
    emitter's colour response, white balance, ambient dilution).  ``subframe`` in [0,1] (a drawn value stays below 1), ``exposure`` in
    [0,3] emitter rows and ``gain`` >= 0 are ``(lo, hi)`` ranges drawn uniformly, or scalars; equal bounds fix the value.  ``gain_mode``
    "common": one gain for the three channels; "per_channel": one each -- and then ``gain`` may also be three numbers, the fixed gains of
    R, G and B (a known colour cast).  The channel acts on the flicker only -- not on the scene.

    ``draw(V)``: V channels from the instance's ONE generator ``numpy.random.default_rng(seed)``, in this order: the V subframes, then
    the V exposures, then the gains (V values, or V x 3 in row-major order; none for three fixed gains) -- each a ``Generator.uniform``
    call, made whether or not the bounds are equal, so that fixing a range does not shift the other draws.

    ``readout`` (None, a number or a ``(lo, hi)`` range within [0,1]): a ROLLING shutter -- the time, in emitter rows, from the start of
    line 0 to the start of a line one frame height further down (``capture_line_taps``).  With a readout ``draw(V)`` draws the V readouts
    AFTER the gains (every earlier value of a seed is unchanged) and returns them under ``"readout"``; ``line_tables`` makes the per-line
    tables.  None: a global shutter -- the same calls and the same three keys as ever."""

    def __init__(self, subframe=(0.0, 1.0), exposure=(1.0, 1.0), gain=(1.0, 1.0), gain_mode="common", seed=0, readout=None):
        self.subframe = _capture_range("subframe", subframe, 0.0, 1.0)
        # rolling shutter: None -- a global shutter, nothing below changes -- or the range of the readout time (capture_line_taps)
        self.readout = None if readout is None else _capture_range("readout", readout, 0.0, 1.0)
        self.exposure = _capture_range("exposure", exposure, 0.0, CAPTURE_MAX_EXPOSURE)
        fmax = float(np.finfo(np.float32).max)
        self.gain_rgb = None                                           # three fixed gains (per_channel only): nothing is drawn for them
        if np.ndim(gain) == 1 and len(gain) == 3:
            if gain_mode != "per_channel":
                raise ValueError(f"CaptureChannel: three gains (one per colour channel) need gain_mode='per_channel', got {gain_mode!r}")
            self.gain_rgb = np.asarray([_capture_range("gain", g, 0.0, fmax)[0] for g in gain], np.float32)
            self.gain = (float(self.gain_rgb.min()), float(self.gain_rgb.max()))
        else:
            self.gain = _capture_range("gain", gain, 0.0, fmax)
        if self.subframe[0] >= 1.0:
            raise ValueError(f"CaptureChannel: the sub-frame phase lies in [0,1): its lower bound must be below 1, got {subframe!r}")
        if gain_mode not in CAPTURE_GAIN_MODES:
            raise ValueError(f"CaptureChannel: gain_mode must be one of {CAPTURE_GAIN_MODES}, got {gain_mode!r}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise ValueError(f"CaptureChannel: seed must be an integer, got {seed!r}")
        self.gain_mode, self.seed = gain_mode, int(seed)
        self._rng = np.random.default_rng(self.seed)

    def draw(self, V):
        """``V`` channels: ``{"subframe": float64 [V], "exposure": float64 [V], "gain": float32 [V,3]}`` (order of the draws: class docstring)"""
        if isinstance(V, bool) or not isinstance(V, (int, np.integer)) or V < 1:
            raise ValueError(f"CaptureChannel.draw: the number of channels must be an integer >= 1, got {V!r}")
        V = int(V)
        sub = np.minimum(self._rng.uniform(*self.subframe, size=V), np.nextafter(1.0, 0.0))
        exp = np.clip(self._rng.uniform(*self.exposure, size=V), *self.exposure)
        if self.gain_rgb is not None:
            gain = np.repeat(self.gain_rgb[None], V, axis=0)
        elif self.gain_mode == "common":
            gain = np.repeat(self._rng.uniform(*self.gain, size=V)[:, None], 3, axis=1)
        else:
            gain = self._rng.uniform(*self.gain, size=(V, 3))
        out = {"subframe": sub, "exposure": exp, "gain": np.ascontiguousarray(gain, dtype=np.float32)}
        if self.readout is not None:
            out["readout"] = np.clip(self._rng.uniform(*self.readout, size=V), *self.readout)
        return out

    @staticmethod
    def line_tables(draw, G, H):
        """the tables ``flicker_lines_mix`` takes for a ``draw`` with a ``"readout"`` (one channel may give scalars and ``gain [3]``), for frames
        of ``H`` lines: fp32 ``taps [V * G, H, Kmax]`` -- every video's ``capture_line_taps`` padded with zeros to the longest -- and fp32
        ``gain [V * G, 3]``.  The ``G`` clips of a video share their video's channel."""
        if not isinstance(draw, dict) or set(draw) != {"subframe", "exposure", "gain", "readout"}:
            raise ValueError(f"CaptureChannel.line_tables: a dict with the keys subframe, exposure, gain and readout, got {draw!r}")
        if isinstance(G, bool) or not isinstance(G, (int, np.integer)) or G < 1:
            raise ValueError(f"CaptureChannel.line_tables: clips per video must be an integer >= 1, got {G!r}")
        sub, exp = np.atleast_1d(np.asarray(draw["subframe"], np.float64)), np.atleast_1d(np.asarray(draw["exposure"], np.float64))
        ro = np.atleast_1d(np.asarray(draw["readout"], np.float64))
        gain = np.asarray(draw["gain"], np.float32)
        gain = gain[None] if gain.ndim == 1 else gain
        V = sub.shape[0]
        if sub.ndim != 1 or exp.shape != (V,) or ro.shape != (V,) or gain.shape != (V, 3) or not np.isfinite(gain).all():
            raise ValueError(f"CaptureChannel.line_tables: subframe [V], exposure [V], readout [V] and finite gain [V,3], got {sub.shape}, {exp.shape}, "
                             f"{ro.shape}, {gain.shape}")
        per_video = [capture_line_taps(s, e, r, H) for s, e, r in zip(sub, exp, ro)]
        taps = np.zeros((V, int(H), max(w.shape[1] for w in per_video)), np.float32)
        for v, w in enumerate(per_video):
            taps[v, :, :w.shape[1]] = w
        return np.repeat(taps, int(G), axis=0), np.ascontiguousarray(np.repeat(gain, int(G), axis=0))

    @staticmethod
    def tables(draw, G=1):
        """the tables ``flicker_rows_mix`` takes for ``draw`` (a dict as ``draw`` returns; one channel may give scalars and ``gain [3]``):
        fp32 ``taps [V * G, Kmax]`` -- every video's ``capture_taps`` padded with zeros to the longest -- and fp32 ``gain [V * G, 3]``.  The
        ``G`` clips of a video share their video's channel, as they share its phase."""
        if not isinstance(draw, dict) or set(draw) != {"subframe", "exposure", "gain"}:
            raise ValueError(f"CaptureChannel.tables: a dict with the keys subframe, exposure and gain, got {draw!r}")
        if isinstance(G, bool) or not isinstance(G, (int, np.integer)) or G < 1:
            raise ValueError(f"CaptureChannel.tables: clips per video must be an integer >= 1, got {G!r}")
        sub, exp = np.atleast_1d(np.asarray(draw["subframe"], np.float64)), np.atleast_1d(np.asarray(draw["exposure"], np.float64))
        gain = np.asarray(draw["gain"], np.float32)
        gain = gain[None] if gain.ndim == 1 else gain
        V = sub.shape[0]
        if sub.ndim != 1 or exp.shape != (V,) or gain.shape != (V, 3) or not np.isfinite(gain).all():
            raise ValueError(f"CaptureChannel.tables: subframe [V], exposure [V] and finite gain [V,3], got {sub.shape}, {exp.shape}, {gain.shape}")
        per_video = [capture_taps(s, e) for s, e in zip(sub, exp)]
        taps = np.zeros((V, max(len(w) for w in per_video)), np.float32)
        for v, w in enumerate(per_video):
            taps[v, :len(w)] = w
        return np.repeat(taps, int(G), axis=0), np.ascontiguousarray(np.repeat(gain, int(G), axis=0))


def is_video_file(path):
    """whether an ``.npz`` holds whole videos (``video_00000``, ...) and not a ``clips`` array"""
    with np.load(path, allow_pickle=True) as z:
        return "clips" not in z.files and "video_00000" in z.files


def load_video_file(path):
    """A whole-video ``.npz``: ``labels`` int64 ``[V]`` and ``video_00000``, ``video_00001``, ... each uint8 ``[N_k,H_k,W_k,3]`` (lengths and
    resolutions may differ), optionally ``names`` ``[V]`` -> ``(list of contiguous uint8 arrays, labels int64, names)``."""
    z = np.load(path, allow_pickle=True)
    labels = z["labels"].astype(np.int64).reshape(-1)
    videos = []
    for k in range(len(labels)):
        key = f"video_{k:05d}"
        if key not in z.files:
            raise ValueError(f"{path}: {len(labels)} labels but no {key}")
        v = z[key]
        if v.dtype != np.uint8 or v.ndim != 4 or v.shape[-1] != 3 or v.shape[0] < 1:
            raise ValueError(f"{path}: {key} must be uint8 [N,H,W,3], got {v.shape} {v.dtype}")
        videos.append(np.ascontiguousarray(v))
    names = [str(n) for n in z["names"]] if "names" in z.files else [f"video_{k:05d}" for k in range(len(labels))]
    return videos, labels, names


def load_weights(path, arch=None):
    """Victim weights for FlickerVideoResNet as ``{state_dict name: float32 ndarray}``.

    ``.pth`` / ``.pt``: a torchvision ``state_dict`` as ``torch.save`` writes it -- what the reference obtains through
    ``torchvision.models.video.<arch>(pretrained=True)`` (utils_cv/action_recognition/model.py:421; torchvision 0.5.0 files such as
    ``r2plus1d_18-91a641e6.pth``) -- or a checkpoint dict holding one under ``state_dict`` / ``model``; a ``module.`` prefix
    (``nn.DataParallel``, model.py:576-578) is stripped and ``num_batches_tracked`` counters are dropped.  ``.npz``: the same names.
    With ``arch`` the names and shapes are checked against that architecture's layer table."""
    if str(path).endswith(".npz"):
        W = {k: np.asarray(v, dtype=np.float32) for k, v in np.load(path).items()}
    else:
        import torch
        sd = torch.load(path, map_location="cpu", weights_only=True)
        for key in ("state_dict", "model"):
            if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
                sd = sd[key]
        W = {}
        for k, v in sd.items():
            if k.endswith("num_batches_tracked") or not hasattr(v, "numpy"):
                continue
            W[k[len("module."):] if k.startswith("module.") else k] = v.detach().to(torch.float32).numpy()
    if arch is not None:
        want = {}
        for pre, co, ci, k, bnp in conv_table(arch):
            want[pre + ".weight"] = (co, ci, *k)
            for s in (".weight", ".bias", ".running_mean", ".running_var"):
                want[bnp + s] = (co,)
        ncls = int(np.asarray(W["fc.bias"]).shape[0]) if "fc.bias" in W and np.asarray(W["fc.bias"]).ndim == 1 else None
        want["fc.bias"] = (ncls,)                  # the class count is the checkpoint's own (400 / 359 / 487 or a fine-tuned head)
        want["fc.weight"] = (ncls, 512)
        missing = sorted(set(want) - set(W))
        if missing:
            raise KeyError(f"{path}: not a {arch} state_dict, missing {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        bad = [k for k, shp in want.items() if tuple(W[k].shape) != tuple(shp)]
        if bad:
            raise ValueError(f"{path}: shape mismatch for {arch}: {bad[0]} is {W[bad[0]].shape}, expected {want[bad[0]]}")
    return W


def add_capture_arguments(ap):
    """the command-line surface of the capture channel, shared by the two r2plus1d scripts; everything off by default"""
    ap.add_argument("--capture-subframe", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="--flicker-time video: train through a "
                    "camera's capture channel, its sub-frame phase (where in the emitter's row a camera frame starts) drawn uniformly "
                    "from [LO, HI) within [0, 1] per video and step.  Any --capture-* option switches the channel on; the others keep "
                    "the identity (phase 0, exposure 1 row, gain 1)")
    ap.add_argument("--capture-exposure", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="the camera's exposure in emitter rows, "
                    "within [0, 3] (0: an instantaneous sample): a frame records the mix of the 1..4 rows its exposure window covers")
    ap.add_argument("--capture-gain", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="the gain the captured flicker is scaled by "
                    "(emitter colour response, white balance, ambient dilution), >= 0")
    ap.add_argument("--capture-readout", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="a rolling-shutter camera: the time from the "
                    "start of line 0 to the start of a line one frame height further down, in emitter rows, drawn uniformly from [LO, HI] within "
                    "[0, 1] per video and step -- every line of a frame then records its own mix of rows (default: absent, a global shutter)")
    ap.add_argument("--capture-gain-mode", default=None, choices=list(CAPTURE_GAIN_MODES), help="one gain for the three colour channels (common, "
                    "the default) or one each (per_channel)")
    ap.add_argument("--capture-seed", type=int, default=None, help="the channels are drawn from numpy.random.default_rng(seed) (default 0)")
    ap.add_argument("--eval-capture-draws", type=int, default=0, metavar="N", help="after training, score the attack over N random captures per "
                    "video drawn from the channel (evaluate_videos(capture=, capture_draws=N)): the fooling ratio of every draw, their mean "
                    "and minimum")


def add_flicker_model_arguments(ap):
    """the scripts' options of the flicker's pixel model (FlickerVideoResNet(flicker_model=, response=))"""
    ap.add_argument("--flicker-model", default="additive", choices=list(FLICKER_MODELS), help="additive: one offset per frame added to every "
                    "normalised pixel (the reference's model).  illumination: the flicker lights the scene -- linear light times (1 + m), then "
                    "the camera's response and 8 bits; the norm bound is the largest relative modulation; uint8 clips only")
    ap.add_argument("--response", default="srgb", choices=list(ILLUM_RESPONSES), help="--flicker-model illumination: the camera's response curve")


def capture_from_arguments(ap, a):
    """the CaptureChannel the ``--capture-*`` options of ``add_capture_arguments`` describe, or None when none of them is given.  Any of them
    without ``--flicker-time video`` is an argparse error, and so are values a channel cannot take"""
    given = [o for o, v in (("--capture-subframe", a.capture_subframe), ("--capture-exposure", a.capture_exposure), ("--capture-gain", a.capture_gain),
                            ("--capture-readout", a.capture_readout),
                            ("--capture-gain-mode", a.capture_gain_mode), ("--capture-seed", a.capture_seed),
                            ("--eval-capture-draws", a.eval_capture_draws or None)) if v is not None]
    if not given:
        return None
    if a.flicker_time != "video":
        ap.error(f"{', '.join(given)}: the capture channel needs --flicker-time video (it mixes the rows a video's frames carry)")
    if a.eval_capture_draws < 0:
        ap.error(f"--eval-capture-draws must be >= 0, got {a.eval_capture_draws}")
    try:
        return CaptureChannel(subframe=tuple(a.capture_subframe or (0.0, 0.0)), exposure=tuple(a.capture_exposure or (1.0, 1.0)),
                              gain=tuple(a.capture_gain or (1.0, 1.0)), gain_mode=a.capture_gain_mode or "common", seed=a.capture_seed or 0,
                              readout=None if a.capture_readout is None else tuple(a.capture_readout))
    except ValueError as e:
        ap.error(str(e))


# ----------------------------------------------------------------------------------------------------------------------------------
# Lossy intra-frame compression of the delivered video: a JPEG-style round trip defined in integers only.  The kernel
# (csrc/codec.hip, flk_codec_roundtrip_u8) performs the operations written here, one for one: codec_roundtrip_host is its definition.
CODEC_SUBSAMPLINGS = ("444", "420")
# ITU T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), row-major (natural) order
CODEC_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CODEC_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# the "slow integer" transform pair: round(x * 2^13) of the rotation constants; two passes, 2 extra bits kept between them
_C_BITS, _P1_BITS = 13, 2
_F_0_298, _F_0_390, _F_0_541, _F_0_765, _F_0_899, _F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
_F_1_501, _F_1_847, _F_1_961, _F_2_053, _F_2_562, _F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def check_codec(quality, subsampling, what="codec"):
    """the (quality, subsampling) of a codec, checked: an integer 1..100 and "444" or "420" (444 / 420 as integers are taken too)"""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"{what}: quality must be an integer in 1..100, got {quality!r}")
    if str(subsampling) not in CODEC_SUBSAMPLINGS or isinstance(subsampling, bool):
        raise ValueError(f"{what}: subsampling must be one of {CODEC_SUBSAMPLINGS}, got {subsampling!r}")
    return int(quality), str(subsampling)


def check_codec_gop(gop, what="codec"):
    """the GOP length of a codec, checked: an integer 1..65535 (1: every frame is an intra frame)"""
    if isinstance(gop, bool) or not isinstance(gop, (int, np.integer)) or not 1 <= int(gop) <= 65535:
        raise ValueError(f"{what}: gop must be an integer in 1..65535, got {gop!r}")
    return int(gop)


def check_codec_search(search, gop=None, what="codec"):
    """the motion search range of a codec, checked: an integer 0..15 (0: zero motion); ``gop`` given: a range above 0 needs P-frames"""
    if isinstance(search, bool) or not isinstance(search, (int, np.integer)) or not 0 <= int(search) <= 15:
        raise ValueError(f"{what}: search must be an integer in 0..15, got {search!r}")
    if gop is not None and int(search) > 0 and int(gop) == 1:
        raise ValueError(f"{what}: search {int(search)} needs gop > 1 (an intra-frame codec has no P-frames to search for)")
    return int(search)


class Codec:
    """A lossy codec the delivered video goes through: ``quality`` 1..100 (the IJG scale), chroma ``subsampling`` "444" or "420",
    ``gop``, the distance between intra frames (1: intra-frame only; N > 1: closed GOPs of one intra frame and N - 1 P-frames,
    DESIGN.md 10.9) and ``search``, the P-frames' motion search range in pixels (0: zero motion; R in 1..15: every 16 x 16 macroblock
    is predicted from the best of the (2R + 1)^2 full-pel displacements of the previous reconstruction; needs
    ``gop`` > 1).  A checked value object; ``ops.codec_roundtrip`` and the engines take it."""
    __slots__ = ("quality", "subsampling", "gop", "search")

    def __init__(self, quality=75, subsampling="420", gop=1, search=0):
        q, s = check_codec(quality, subsampling, "Codec")
        object.__setattr__(self, "quality", q)
        object.__setattr__(self, "subsampling", s)
        object.__setattr__(self, "gop", check_codec_gop(gop, "Codec"))
        object.__setattr__(self, "search", check_codec_search(search, self.gop, "Codec"))

    def __setattr__(self, name, value):
        raise AttributeError("Codec is immutable")

    def __repr__(self):
        return (f"Codec(quality={self.quality}, subsampling={self.subsampling!r}" + (f", gop={self.gop}" if self.gop > 1 else "")
                + (f", search={self.search}" if self.search else "") + ")")

    def _key(self):
        return (self.quality, self.subsampling, self.gop, self.search)

    def __eq__(self, other):
        return isinstance(other, Codec) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())


def codec_tables(quality):
    """the two quantisation tables at ``quality``: int32 ``[64]`` luma and chroma, row-major -- the Annex K base tables under the IJG
    rule  s = 5000 // q (q < 50) else 200 - 2 q;  Q = clamp((base * s + 50) // 100, 1, 255)"""
    q, _ = check_codec(quality, "444", "codec_tables")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(b, np.int64) * s + 50) // 100, 1, 255).astype(np.int32) for b in (CODEC_BASE_LUMA, CODEC_BASE_CHROMA))


def codec_inter_step(quality):
    """the quantiser step of the P-frames at ``quality``: Qp = clamp((16 * s + 50) // 100, 1, 255), s the IJG scale -- MPEG-2's flat
    default non-intra matrix (16 everywhere) under the rule of ``codec_tables``; one step for all 64 positions and all three planes"""
    q, _ = check_codec(quality, "444", "codec_inter_step")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return min(max((16 * s + 50) // 100, 1), 255)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n          # arithmetic shift: floor((x + 2^(n-1)) / 2^n)


def _fdct_1d(d, shift_even, shift_odd):
    """one 8-point forward pass over axis -1 (values d[..., 0..7]); shift_even < 0: a left shift of the two sums"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if shift_even < 0:
        o[0], o[4] = (t10 + t11) << -shift_even, (t10 - t11) << -shift_even
    else:
        o[0], o[4] = _descale(t10 + t11, shift_even), _descale(t10 - t11, shift_even)
    z1 = (t12 + t13) * _F_0_541
    o[2] = _descale(z1 + t13 * _F_0_765, shift_odd)
    o[6] = _descale(z1 - t12 * _F_1_847, shift_odd)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _F_1_175
    t4, t5, t6, t7 = t4 * _F_0_298, t5 * _F_2_053, t6 * _F_3_072, t7 * _F_1_501
    z1, z2, z3, z4 = -z1 * _F_0_899, -z2 * _F_2_562, -z3 * _F_1_961 + z5, -z4 * _F_0_390 + z5
    o[7], o[5] = _descale(t4 + z1 + z3, shift_odd), _descale(t5 + z2 + z4, shift_odd)
    o[3], o[1] = _descale(t6 + z2 + z3, shift_odd), _descale(t7 + z1 + z4, shift_odd)
    return np.stack(o, -1)


def _idct_1d(c, shift):
    """one 8-point inverse pass over axis -1"""
    z2, z3 = c[..., 2], c[..., 6]
    z1 = (z2 + z3) * _F_0_541
    t2, t3 = z1 - z3 * _F_1_847, z1 + z2 * _F_0_765
    t0, t1 = (c[..., 0] + c[..., 4]) << _C_BITS, (c[..., 0] - c[..., 4]) << _C_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _F_1_175
    t0, t1, t2, t3 = t0 * _F_0_298, t1 * _F_2_053, t2 * _F_3_072, t3 * _F_1_501
    z1, z2, z3, z4 = -z1 * _F_0_899, -z2 * _F_2_562, -z3 * _F_1_961 + z5, -z4 * _F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, shift) for v in o], -1)


def _codec_plane(p, qt, dt):
    """a padded plane [N, Hp, Wp] (values 0..255, Hp and Wp multiples of 8) through DCT, quantisation and back; also the levels"""
    return _codec_plane_parts(p, qt, dt)[:2]


def _codec_plane_parts(p, qt, dt):
    """``_codec_plane`` with what the codec's backward takes from the integer forward: ``(plane, levels, f, raw)`` -- f the forward
    coefficients [N, by, bx, 8, 8] and raw the reconstruction before its clamp, as a plane"""
    N, Hp, Wp = p.shape
    b = p.reshape(N, Hp // 8, 8, Wp // 8, 8).transpose(0, 1, 3, 2, 4).astype(dt) - 128          # [N, by, bx, row, col]
    f = _fdct_1d(b, -_P1_BITS, _C_BITS - _P1_BITS)                                              # pass 1: along the rows
    f = _fdct_1d(f.swapaxes(-1, -2), _P1_BITS, _C_BITS + _P1_BITS).swapaxes(-1, -2)             # pass 2: down the columns; 8 x the DCT
    d = (qt.reshape(8, 8).astype(dt) << 3)
    mag = (np.abs(f) + (d >> 1)) // d                                                           # half away from zero
    lev = np.where(f < 0, -mag, mag).astype(dt)
    c = lev * qt.reshape(8, 8).astype(dt)
    w = _idct_1d(c.swapaxes(-1, -2), _C_BITS - _P1_BITS).swapaxes(-1, -2)                       # pass 1: down the columns
    raw = _idct_1d(w, _C_BITS + _P1_BITS + 3) + 128                                             # pass 2: along the rows
    plane = lambda a: a.transpose(0, 1, 3, 2, 4).reshape(N, Hp, Wp)
    return plane(np.clip(raw, 0, 255)), lev, f, plane(raw)


def _codec_plane_inter(p, ref, qp, dt):
    """a P-frame's padded plane [N, Hp, Wp] predicted from ``ref`` (the previous reconstruction, same shape, zero motion): the residual
    through DCT, the flat quantiser ``qp`` (rounding offset 1/4 of a step) and back onto ``ref``; also the levels"""
    N, Hp, Wp = p.shape
    blocks = lambda a: a.reshape(N, Hp // 8, 8, Wp // 8, 8).transpose(0, 1, 3, 2, 4).astype(dt)   # [N, by, bx, row, col]
    rb = blocks(ref)
    f = _fdct_1d(blocks(p) - rb, -_P1_BITS, _C_BITS - _P1_BITS)                                  # the residual, -255..255: no -128
    f = _fdct_1d(f.swapaxes(-1, -2), _P1_BITS, _C_BITS + _P1_BITS).swapaxes(-1, -2)
    d = dt(qp << 3)
    mag = (np.abs(f) + (d >> 2)) // d                                                           # a dead zone: 1/4 of a step, not 1/2
    lev = np.where(f < 0, -mag, mag).astype(dt)
    w = _idct_1d((lev * dt(qp)).swapaxes(-1, -2), _C_BITS - _P1_BITS).swapaxes(-1, -2)
    o = np.clip(rb + _idct_1d(w, _C_BITS + _P1_BITS + 3), 0, 255)
    return o.transpose(0, 1, 3, 2, 4).reshape(N, Hp, Wp), lev


def codec_motion_search(cur_Y, ref_Y, search):
    """The P-frames' block search alone: per 16 x 16 macroblock of the padded luma plane ``cur_Y`` (cut from the
    top-left corner; the last column or row of macroblocks may be narrower, and is searched over its own pixels) the full-pel vector
    (dy, dx) into ``ref_Y``, the previous reconstruction of the same shape -- int8 ``[MBy, MBx, 2]``.
      SAD(dy, dx) = sum |cur_Y[y, x] - ref_Y[clamp(y + dy, 0, Hp - 1), clamp(x + dx, 0, Wp - 1)]| over the macroblock's pixels
    Candidates are visited in one order: (0, 0) first, then dy = -R..R (outer), dx = -R..R (inner); a candidate replaces the best only
    if its SAD is strictly smaller -- the minimum of the integer key SAD * 1024 + rank, rank 0 the zero vector and
    1 + (dy + R)(2R + 1) + (dx + R) the others (SAD <= 65280, rank <= 961: the key fits 27 bits)."""
    R = check_codec_search(search, what="codec_motion_search")
    cur, ref = np.asarray(cur_Y), np.asarray(ref_Y)
    if cur.ndim != 2 or cur.shape != ref.shape or min(cur.shape) < 1 or cur.dtype.kind not in "iu" or ref.dtype.kind not in "iu":
        raise ValueError(f"codec_motion_search: cur_Y and ref_Y must be integer planes of one shape [Hp, Wp], got {cur.shape} {cur.dtype} and "
                         f"{ref.shape} {ref.dtype}")
    if min(cur.min(), ref.min()) < 0 or max(cur.max(), ref.max()) > 255:
        raise ValueError("codec_motion_search: the planes hold bytes, 0..255")
    Hp, Wp = cur.shape
    cur, pad = cur.astype(np.int32), np.pad(ref.astype(np.int32), R, mode="edge")            # the edge sample beyond the plane
    ys, xs, n = np.arange(0, Hp, 16), np.arange(0, Wp, 16), 2 * R + 1

    def key(dy, dx, rank):
        sad = np.abs(cur - pad[R + dy:R + dy + Hp, R + dx:R + dx + Wp])
        return np.add.reduceat(np.add.reduceat(sad, ys, 0), xs, 1) * 1024 + rank

    best = key(0, 0, 0)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            best = np.minimum(best, key(dy, dx, 1 + (dy + R) * n + (dx + R)))
    rank = best & 1023
    k = np.maximum(rank - 1, 0)
    return np.stack([np.where(rank == 0, 0, k // n - R), np.where(rank == 0, 0, k % n - R)], -1).astype(np.int8)


def _codec_mc_predict(ref, mv, s420):
    """the motion-compensated prediction planes (Y, Cb, Cr) of a P-frame from the reference planes ``ref`` and the macroblock vectors
    ``mv`` [MBy, MBx, 2]: full-pel on luma (and on 4:4:4 chroma), half the vector at half-pel precision on 4:2:0 chroma; every sample
    read is clamped into its plane"""
    Y, Cb, Cr = ref
    Hp, Wp = Y.shape
    dy, dx = (mv[..., j].astype(np.int64).repeat(16, 0).repeat(16, 1)[:Hp, :Wp] for j in (0, 1))
    yy, xx = np.mgrid[0:Hp, 0:Wp]
    fy, fx = np.clip(yy + dy, 0, Hp - 1), np.clip(xx + dx, 0, Wp - 1)
    if not s420:
        return Y[fy, fx], Cb[fy, fx], Cr[fy, fx]
    Hc, Wc = Hp // 2, Wp // 2
    vy, vx = (mv[..., j].astype(np.int64).repeat(8, 0).repeat(8, 1) for j in (0, 1))         # a macroblock's 8 x 8 chroma block
    iy, hy, ix, hx = vy >> 1, (vy & 1) == 1, vx >> 1, (vx & 1) == 1                            # arithmetic shift: -3 -> -2 + 1/2
    yy, xx = np.mgrid[0:Hc, 0:Wc]
    y0, y1, x0, x1 = (np.clip(v, 0, m - 1) for v, m in ((yy + iy, Hc), (yy + iy + 1, Hc), (xx + ix, Wc), (xx + ix + 1, Wc)))

    def half(p):
        a, b, c, d = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
        return np.where(hy & hx, (a + b + c + d + 2) >> 2, np.where(hx, (a + b + 1) >> 1, np.where(hy, (a + c + 1) >> 1, a)))

    return Y[fy, fx], half(Cb), half(Cr)


def codec_roundtrip_host(frames, quality, subsampling="420", tone=None, stats=False, gop=1, first_frame=0, search=0, motion=False,
                         _dtype=np.int32):
    """The codec round trip on the host, in integers only: uint8 ``[N,H,W,3]`` (or one frame ``[H,W,3]``) -> uint8 of the same shape;
    with ``stats`` also int32 ``[N,2]``: per frame the number of non-zero quantised coefficients and the sum of their magnitudes.
    ``tone``: uint8 ``[N,256,3]`` (or ``[256,3]``), the byte -> byte table each frame goes through first.
    Stages (every shift is arithmetic; all values in ``_dtype``, int32 -- int64 gives the same, which is the overflow check):
      colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
               Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16;   Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
      pad      to multiples of 8 ("444") or 16 ("420") by repeating the last column and row
      420      Cb, Cr: (a + b + c + d + 1 + (x & 1)) >> 2 over each 2 x 2 cell, x the OUTPUT column
      DCT      value - 128; rows then columns (_fdct_1d); level = sign * ((|f| + 4 Q) // (8 Q)); back: level * Q, columns then rows
               (_idct_1d), + 128, clamp to 0..255
      420      chroma repeated 2 x 2
      colour   R = Y + ((91881 Cr' + 32768) >> 16);  G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16);  B = Y + ((116130 Cb' + 32768) >> 16)
               with Cb' = Cb - 128, Cr' = Cr - 128; clamp to 0..255; crop
    ``gop`` > 1: frame t is video frame n = ``first_frame`` + t (``first_frame`` a multiple of ``gop``); n % gop == 0
    is an intra frame, coded as above, every other one a P-frame predicted from the previous frame's reconstructed padded planes
    ``ref`` at zero motion -- per plane and 8 x 8 block, in place of the DCT stage:
      P        r = cur - ref (no - 128); the same two forward passes; level = sign * ((|f| + 2 Qp) // (8 Qp)), Qp = codec_inter_step(quality)
               for every position and plane; rec = clamp(ref + idct(level * Qp), 0, 255) (the same two inverse passes, no + 128); ref <- rec
    The stats of a P-frame count its levels.
    ``search`` = R > 0 (needs ``gop`` > 1): a P-frame is predicted with motion.  Its padded luma plane is cut into
    16 x 16 macroblocks, each takes the vector ``codec_motion_search`` finds in ref's luma, and in the step above ``ref`` is replaced by
      pred     luma (and chroma at "444"): ref[clamp(y + dy), clamp(x + dx)]; chroma at "420": the macroblock's 8 x 8 block moved by
               half the vector, iy = dy >> 1, hy = dy & 1 (ix, hx likewise): a, (a + b + 1) >> 1 with one half flag (b the next sample
               along that axis) or (a + b + c + d + 2) >> 2 with both; every sample read is clamped into its plane
    so r = cur - pred, rec = clamp(pred + idct(level * Qp), 0, 255), ref <- rec.  ``motion``: also return the vectors, int8
    ``[N, MBy, MBx, 2]`` as (dy, dx), zeros on intra frames (and everywhere at ``search`` 0), after the stats if both are asked for."""
    quality, subsampling = check_codec(quality, subsampling, "codec_roundtrip_host")
    gop = check_codec_gop(gop, "codec_roundtrip_host")
    search = check_codec_search(search, gop, "codec_roundtrip_host")
    if isinstance(first_frame, bool) or not isinstance(first_frame, (int, np.integer)) or first_frame < 0 or first_frame % gop:
        raise ValueError(f"codec_roundtrip_host: first_frame must be a non-negative multiple of gop {gop} (a span starts on an intra frame), "
                         f"got {first_frame!r}")
    x = np.asarray(frames)
    single = x.ndim == 3
    if single:
        x = x[None]
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[-1] != 3 or min(x.shape) < 1:
        raise ValueError(f"codec_roundtrip_host: frames must be uint8 [N,H,W,3], got {x.shape} {x.dtype}")
    N, H, W, _ = x.shape
    if tone is not None:
        tone = np.asarray(tone)
        if tone.ndim == 2:
            tone = np.broadcast_to(tone, (N, 256, 3))
        if tone.dtype != np.uint8 or tone.shape != (N, 256, 3):
            raise ValueError(f"codec_roundtrip_host: tone must be uint8 [{N},256,3], got {tone.shape} {tone.dtype}")
        x = np.stack([np.stack([tone[n, :, c][x[n, :, :, c]] for c in range(3)], -1) for n in range(N)])
    dt = _dtype
    m = 8 if subsampling == "444" else 16
    Hp, Wp = (H + m - 1) // m * m, (W + m - 1) // m * m
    x = np.pad(x, ((0, 0), (0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(dt)
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16
    if subsampling == "420":
        bias = (1 + (np.arange(Wp // 2) & 1)).astype(dt)
        Cb, Cr = ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + bias) >> 2 for p in (Cb, Cr))
    ql, qc = codec_tables(quality)
    mv = np.zeros((N, (Hp + 15) // 16, (Wp + 15) // 16, 2), np.int8)
    if gop == 1:
        (Y, ly), (Cb, lb), (Cr, lr) = _codec_plane(Y, ql, dt), _codec_plane(Cb, qc, dt), _codec_plane(Cr, qc, dt)
    elif search > 0:
        qp = codec_inter_step(quality)
        rec, coded = None, []
        for t in range(N):
            cur = (Y[t:t + 1], Cb[t:t + 1], Cr[t:t + 1])
            if (first_frame + t) % gop == 0:
                one = [_codec_plane(p, qt, dt) for p, qt in zip(cur, (ql, qc, qc))]
            else:
                mv[t] = codec_motion_search(cur[0][0], rec[0], search)
                pred = _codec_mc_predict(rec, mv[t], subsampling == "420")
                one = [_codec_plane_inter(p, q[None], qp, dt) for p, q in zip(cur, pred)]
            rec = [r[0] for r, _ in one]
            coded.append(one)
        (Y, ly), (Cb, lb), (Cr, lr) = ((np.concatenate([c[j][0] for c in coded]), np.concatenate([c[j][1] for c in coded])) for j in range(3))
    else:
        qp = codec_inter_step(quality)
        coded = []
        for p, qt in ((Y, ql), (Cb, qc), (Cr, qc)):
            rec, lev = [], []
            for t in range(N):
                r, l = _codec_plane(p[t:t + 1], qt, dt) if (first_frame + t) % gop == 0 else _codec_plane_inter(p[t:t + 1], rec[-1], qp, dt)
                rec.append(r)
                lev.append(l)
            coded.append((np.concatenate(rec), np.concatenate(lev)))
        (Y, ly), (Cb, lb), (Cr, lr) = coded
    if subsampling == "420":
        Cb, Cr = (p.repeat(2, 1).repeat(2, 2) for p in (Cb, Cr))
    cb, cr = Cb - 128, Cr - 128
    out = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], -1)
    out = np.clip(out, 0, 255).astype(np.uint8)[:, :H, :W]
    if single:
        out = out[0]
    res = (out,)
    if stats:
        st = np.stack([sum((l != 0).reshape(N, -1).sum(1) for l in (ly, lb, lr)), sum(np.abs(l).reshape(N, -1).sum(1) for l in (ly, lb, lr))], -1)
        res += (st.astype(np.int32),)
    if motion:
        res += (mv[0] if single else mv,)
    return res if len(res) > 1 else out


# ----------------------------------------------------------------------------------------------------------------------------------
# The codec's backward (csrc/codec.hip, flk_codec_grad).  The forward stays the integer codec above.  The backward
# differentiates a SURROGATE of the intra codec (gop = 1), per frame, with constants taken from the integer forward:
#   colour   the derivative of the fixed-point definitions: the integer constants over 2^16 (dyadic, exact in float32); rounding: 1
#   clamps   the plane clamp after the inverse DCT and the RGB clamp pass the gradient where the UNCLAMPED integer lies in 0..255
#   pad      padding repeats the last row and column: the transpose adds the padded pixels' gradients onto that row and column
#   420      the box mean gives 1/4 to each of its four pixels; the replication on decode sums its four pixels
#   DCT      the orthonormal 8 x 8 DCT-II matrix C in float32: G = C g C^T is the transpose of the inverse, C^T G C of the forward
#            (the forward's x 8 and the quantiser's 8 Q cancel)
#   quant    per coefficient f of level lev: r = (f - lev * 8 Q) / (8 Q) in [-1/2, 1/2] from the integers; the factor d is 1 ("ste") or
#            3 r^2 ("cubic": Shin & Song's differentiable-JPEG rounding round(u) + (u - round(u))^3 -- 0 at a bin centre, 3/4 at an edge)
# g_out [H,W,3] -> RGB mask, M_dec^T, chroma 2 x 2 sum, plane mask, C . C^T, x d, C^T . C, chroma 1/4 spread, padding fold, M_enc^T ->
# g_in [H,W,3];  gdelta[t][c] = scale[t][c] * sum over pixels of g_in(p, c) * slope[t][v(p, c)][c], v the SOURCE byte before the tone.
CODEC_GRAD_MODES = ("ste", "cubic")
CODEC_TILE_W, CODEC_TILE_H, CODEC_THREADS = 128, {"444": 32, "420": 64}, 192      # the tiling of csrc/codec.hip (kTW, CodecGeo::TH)
# [R, G, B] = _CODEC_DEC @ [Y, Cb - 128, Cr - 128] and [Y, Cb, Cr] = _CODEC_ENC @ [R, G, B] (+ offsets), the integer constants over 2^16
_CODEC_DEC = np.array([[65536, 0, 91881], [65536, -22554, -46802], [65536, 116130, 0]], np.float64) / 65536.0
_CODEC_ENC = np.array([[19595, 38470, 7471], [-11059, -21709, 32768], [32768, -27439, -5329]], np.float64) / 65536.0


def check_codec_grad(mode, what="codec_grad"):
    if mode not in CODEC_GRAD_MODES:
        raise ValueError(f"{what}: the codec gradient must be one of {CODEC_GRAD_MODES}, got {mode!r}")
    return mode


def codec_dct_matrix():
    """the orthonormal 8 x 8 DCT-II matrix, C[u][x] = a(u) cos((2 x + 1) u pi / 16), a(0) = sqrt(1/8), else 1/2, rounded to float32"""
    u, x = np.mgrid[0:8, 0:8]
    return np.where(u == 0, np.sqrt(1 / 8), 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.float32)


def _codec_grad_frames(what, frames, tone):
    x = np.asarray(frames)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[-1] != 3 or min(x.shape) < 1:
        raise ValueError(f"{what}: frames must be uint8 [N,H,W,3], got {x.shape} {x.dtype}")
    if tone is not None:
        tone = np.asarray(tone)
        if tone.ndim == 2:
            tone = np.broadcast_to(tone, (x.shape[0], 256, 3))
        if tone.dtype != np.uint8 or tone.shape != (x.shape[0], 256, 3):
            raise ValueError(f"{what}: tone must be uint8 [{x.shape[0]},256,3], got {tone.shape} {tone.dtype}")
    return x, tone


def codec_quant_slopes_host(frames, quality, subsampling="420", tone=None, mode="cubic"):
    """What the codec's backward takes from the INTEGER forward of ``codec_roundtrip_host(frames, quality, subsampling, tone)``:
    ``(d, plane_mask, rgb_mask)``.  ``d``: three float64 planes (Y, Cb, Cr; padded, chroma at its own size), the quantiser's factor of
    coefficient (u, v) of block (by, bx) at [n, 8 by + u, 8 bx + v] -- 1 under "ste", 3 r^2 under "cubic", r = (f - lev * 8 Q) / (8 Q)
    formed from the integers.  ``plane_mask``: three bool planes, True where the reconstruction before its clamp lies in 0..255.
    ``rgb_mask``: bool [N,H,W,3], True where the decoded channel before its clamp lies in 0..255."""
    quality, subsampling = check_codec(quality, subsampling, "codec_quant_slopes_host")
    check_codec_grad(mode, "codec_quant_slopes_host")
    x, tone = _codec_grad_frames("codec_quant_slopes_host", frames, tone)
    N, H, W, _ = x.shape
    if tone is not None:
        x = np.stack([np.stack([tone[n, :, c][x[n, :, :, c]] for c in range(3)], -1) for n in range(N)])
    dt = np.int64
    m = 8 if subsampling == "444" else 16
    Hp, Wp = (H + m - 1) // m * m, (W + m - 1) // m * m
    x = np.pad(x, ((0, 0), (0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(dt)
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    planes = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16, (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16,
              (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16]
    if subsampling == "420":
        bias = (1 + (np.arange(Wp // 2) & 1)).astype(dt)
        planes[1:] = [(p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + bias) >> 2 for p in planes[1:]]
    ql, qc = codec_tables(quality)
    d, keep, rec = [], [], []
    for p, qt in zip(planes, (ql, qc, qc)):
        o, lev, f, raw = _codec_plane_parts(p, qt, dt)
        q8 = qt.reshape(8, 8).astype(dt) << 3
        r = (f - lev * q8).astype(np.float64) / q8
        dd = 3.0 * r * r if mode == "cubic" else np.ones(r.shape)
        d.append(dd.transpose(0, 1, 3, 2, 4).reshape(p.shape))
        keep.append((raw >= 0) & (raw <= 255))
        rec.append(o)
    Y, Cb, Cr = rec
    if subsampling == "420":
        Cb, Cr = (p.repeat(2, 1).repeat(2, 2) for p in (Cb, Cr))
    cb, cr = Cb - 128, Cr - 128
    out = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], -1)
    return tuple(d), tuple(keep), ((out >= 0) & (out <= 255))[:, :H, :W]


def _codec_grad_chain(g, d, keep, rgb_mask, s420, magnitudes):
    """the linear chain of the codec's backward on g [N,H,W,3] in float64; ``magnitudes``: every matrix by its absolute values"""
    mat = np.abs if magnitudes else (lambda a: a)
    C = mat(codec_dct_matrix().astype(np.float64))
    N, H, W, _ = g.shape
    Hp, Wp = d[0].shape[1:]
    g = np.pad(g * rgb_mask, ((0, 0), (0, Hp - H), (0, Wp - W), (0, 0))) @ mat(_CODEC_DEC)           # M_dec^T: [.., Y, Cb, Cr]
    planes = [g[..., 0], g[..., 1], g[..., 2]]
    if s420:
        planes[1:] = [p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] for p in planes[1:]]
    for j, p in enumerate(planes):
        n, hp, wp = p.shape
        blocks = lambda a: a.reshape(n, hp // 8, 8, wp // 8, 8).transpose(0, 1, 3, 2, 4)
        b = C @ blocks(p * keep[j]) @ C.T
        b = C.T @ (b * blocks(d[j])) @ C
        planes[j] = b.transpose(0, 1, 3, 2, 4).reshape(n, hp, wp)
    if s420:
        planes[1:] = [0.25 * p.repeat(2, 1).repeat(2, 2) for p in planes[1:]]
    p = np.stack(planes, -1)
    out = p[:, :H, :W].copy()                                                                        # the padding folds onto the last row and column
    out[:, H - 1, :] += p[:, H:, :W].sum(1)
    out[:, :, W - 1] += p[:, :H, W:].sum(2)
    out[:, H - 1, W - 1] += p[:, H:, W:].sum((1, 2))
    return out @ mat(_CODEC_ENC)                                                                     # M_enc^T: [.., R, G, B]


def codec_grad_host(frames, quality, subsampling, tone, mode, g_out, slope=None, scale=None, bound=False, consts=None):
    """flk_codec_grad restated in float64: ``frames`` uint8 [N,H,W,3] (the SOURCE frames, frame n under ``tone[n]``), ``g_out`` =
    d(loss)/d(decoded RGB) [N,H,W,3].  Returns a dict: ``g_in`` [N,H,W,3], the gradient with respect to the codec's input frame, and,
    with ``slope`` [N,256,3] and ``scale`` [N,3] (``tone_slopes_host``), ``gdelta`` [N,3] = scale * sum over pixels of g_in * slope[source
    byte].  ``consts``: ``codec_quant_slopes_host``'s result, if the caller has it.  ``bound``: also ``g_in_mag`` / ``gdelta_mag``, the
    chain run on magnitudes (|matrices|, |g|, |slope|, |scale|), and ``g_in_roundings`` / ``gdelta_roundings``, the float32 roundings on
    the longest path to an output in the kernel's statement order: 3 (M_dec^T), 3 (2 x 2 sum), 32 (four 8-point passes), 5 (d), 5
    (M_enc^T), 8 spare for the float32 reciprocal of 8 Q and the first-order form of the bound, plus the (Hp - H + 1)(Wp - W + 1) terms of
    the fold; for gdelta also the product with the slope, a thread's pixels of a tile, the shuffle tree and the waves, the tiles of
    the frame and the scale.  |device - host| <= roundings * 2^-24 * magnitude, per element."""
    quality, subsampling = check_codec(quality, subsampling, "codec_grad_host")
    check_codec_grad(mode, "codec_grad_host")
    x, tone = _codec_grad_frames("codec_grad_host", frames, tone)
    g = np.asarray(g_out, dtype=np.float64)
    if g.shape != x.shape:
        raise ValueError(f"codec_grad_host: g_out must be {x.shape}, got {g.shape}")
    d, keep, rgb_mask = codec_quant_slopes_host(x, quality, subsampling, tone, mode) if consts is None else consts
    s420 = subsampling == "420"
    N, H, W, _ = x.shape
    res = {"g_in": _codec_grad_chain(g, d, keep, rgb_mask, s420, False)}
    if bound:
        Hp, Wp = d[0].shape[1:]
        res["g_in_mag"] = _codec_grad_chain(np.abs(g), d, keep, rgb_mask, s420, True)
        res["g_in_roundings"] = 56 + (Hp - H + 1) * (Wp - W + 1)
    if slope is not None:
        slope, scale = np.asarray(slope, dtype=np.float64), np.asarray(scale, dtype=np.float64)
        if slope.shape != (N, 256, 3) or scale.shape != (N, 3):
            raise ValueError(f"codec_grad_host: slope [{N},256,3] and scale [{N},3]; got {slope.shape}, {scale.shape}")
        s = np.stack([slope[n][x[n], np.arange(3)] for n in range(N)])                               # [N,H,W,3]: the slope of the source byte
        res["gdelta"] = (res["g_in"] * s).sum((1, 2)) * scale
        if bound:
            th = CODEC_TILE_H[subsampling]
            tiles = -(-Hp // th) * -(-Wp // CODEC_TILE_W)
            res["gdelta_mag"] = (res["g_in_mag"] * np.abs(s)).sum((1, 2)) * np.abs(scale)
            res["gdelta_roundings"] = res["g_in_roundings"] + 1 + -(-th * CODEC_TILE_W // CODEC_THREADS) + 6 + 3 + tiles + 1
    return res


def add_codec_arguments(ap):
    """the scripts' options of the codec the delivered video goes through; absent by default"""
    ap.add_argument("--codec-quality", type=int, default=None, metavar="Q", help="compress the delivered video lossily, intra-frame (JPEG-style: "
                    "colour transform, 8x8 DCT, quantisation at IJG quality Q in 1..100, and back) wherever a whole delivered video is scored, "
                    "saved or trained on: --eval-quantised video, --save-adversarial-u8 of whole videos, --train-delivered")
    ap.add_argument("--codec-subsampling", default=None, choices=list(CODEC_SUBSAMPLINGS), help="the codec's chroma subsampling (default 420); "
                    "needs --codec-quality")
    ap.add_argument("--codec-gop", type=int, default=None, metavar="N", help="the codec's distance between intra frames (default 1: every frame "
                    "is an intra frame); N > 1 codes closed GOPs of one intra frame and N - 1 zero-motion P-frames, whose quantised temporal "
                    "residual decides whether a flicker arrives; needs --codec-quality")
    ap.add_argument("--codec-search", type=int, default=None, metavar="R", help="the P-frames' motion search range in pixels, 0..15 (default 0: "
                    "zero motion; 7 is a usual choice): every 16x16 macroblock is predicted from the best full-pel displacement of the previous "
                    "reconstruction, so camera and object motion is not paid for as residual; needs --codec-gop above 1")
    ap.add_argument("--codec-grad", default=None, choices=["identity"] + list(CODEC_GRAD_MODES), help="the codec's Jacobian in the backward of "
                    "--train-delivered (default identity: straight through); ste and cubic differentiate the intra codec itself -- chroma "
                    "subsampling, clamps and the transform pair, the quantiser straight through (ste) or by the cubic rounding surrogate, which "
                    "passes nothing at a bin centre (cubic); needs --codec-quality, an intra-frame codec and --train-delivered")


def codec_from_arguments(ap, a, used):
    """the Codec the ``--codec-*`` options describe, or None.  ``used``: whether this run has a whole delivered video to compress (the
    caller's modes); the options anywhere else are an argparse error"""
    if a.codec_quality is None:
        if a.codec_subsampling is not None:
            ap.error("--codec-subsampling needs --codec-quality")
        if a.codec_gop is not None:
            ap.error("--codec-gop needs --codec-quality")
        if a.codec_search is not None:
            ap.error("--codec-search needs --codec-quality")
        if getattr(a, "codec_grad", None) not in (None, "identity"):
            ap.error("--codec-grad needs --codec-quality")
        return None
    if not used:
        ap.error("--codec-quality / --codec-subsampling act on whole delivered videos: give --eval-quantised video, --train-delivered or "
                 "--save-adversarial-u8 with whole videos")
    try:
        codec = Codec(a.codec_quality, a.codec_subsampling or "420", 1 if a.codec_gop is None else a.codec_gop,
                      0 if a.codec_search is None else a.codec_search)
    except ValueError as e:
        ap.error(str(e))
    if getattr(a, "codec_grad", None) not in (None, "identity"):
        if codec.gop > 1:
            ap.error("--codec-grad ste / cubic differentiate the intra codec: not with --codec-gop above 1")
        if not getattr(a, "train_delivered", False):
            ap.error("--codec-grad acts on the backward of --train-delivered")
    return codec


def flicker_keywords_from_arguments(a, delivered=False):
    """the flicker keywords of ``FlickerVideoResNet`` from the scripts' parsed arguments, ``a.capture`` and ``a.codec`` being what
    ``capture_from_arguments`` / ``codec_from_arguments`` returned.  ``delivered``: the construction of a script mode that has whole
    videos -- it also takes ``train_delivered`` and, only with it, the codec (elsewhere the codec acts on evaluation and export)"""
    kw = dict(flicker_time=a.flicker_time, flicker_period=a.flicker_period, capture=a.capture, flicker_model=a.flicker_model, response=a.response)
    if delivered:
        kw.update(train_delivered=a.train_delivered, codec=a.codec if a.train_delivered else None)
        if getattr(a, "codec_grad", None) not in (None, "identity"):
            kw.update(codec_grad=a.codec_grad)
    return kw
