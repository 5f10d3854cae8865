#!/usr/bin/env python3
"""Universal flickering attack on torchvision VideoResNets -- the MI355X counterpart of the reference's
r2plus1d_main_universal_attack.py (constants, destination folder, resume rules and the `learner.fit` call follow it:
r2plus1d_main_universal_attack.py:33-58,176-236).

What differs: clips come PRE-DECODED (the reference decodes mp4 with decord, which this image lacks): `--train-npz` /
`--val-npz` hold `clips` ([N,T,112,112,3]; uint8 frames or float32 already normalised with dataset.py:28-29 mean / std)
and `labels` ([N] int).  Weights: `--weights-npz` with torchvision state_dict names, else seeded synthetic weights.
One process per GPU (torch.distributed.run); every rank takes its shard of the training clips, the perturbation is
replicated (parallel.py).

uint8 clips stay uint8 (`--decode device`, the default): each rank uploads its shard once and every batch is a slice of that
resident tensor; the attack's apply kernel normalises the frames (bitwise the host route's float32 values).  `--decode host`
normalises on the host and copies every batch, as float32, per step -- the route of float32 files.

uint8 clips may also be RAW decoded frames of any H x W (what the reference's loader hands its transform, dataset.py:84-123): they are
resized (bilinear, shorter side to `--im-scale`), centre-cropped to `--image-size` and normalised per batch by one kernel from the
resident raw shard (`--prepare device`, the default for such files), or once on the host with torch (`--prepare host`, the A/B
route).  `--resize-rule` picks the coordinate rule of the resize (videoresnet_spec.prepare_geometry).  Clips are raw when they are
not square, or not `--image-size` when that is given, or whenever `--prepare` is given (the engine then is 112 x 112 unless
`--image-size` says otherwise); files of clips at the engine's size behave as before.

`--train-transforms train` prepares the TRAINING batches of raw frames with the reference's training transform (dataset.py:105-118:
RandomResizedCropVideo with `--aug-scales`, or RandomCropVideo with `--aug-no-resize`, then RandomHorizontalFlipVideo with `--flip-ratio`),
a fresh box and flip per clip and epoch from `random.Random(--aug-seed + rank)`: on the device by the second preparation kernel, or
with `--prepare host` per batch with torch (videoresnet_spec.prepare_host_train, same sampler).  The validation split and the default
(`eval`, what the reference's own attack scripts pass for both splits) keep the evaluation transform.

WHOLE-VIDEO files: an `.npz` with `labels` (int64 [V]) and `video_00000`, `video_00001`, ... (each uint8 [N_k,H_k,W_k,3], lengths and
resolutions free) instead of `clips`.  The videos of a rank's batches stay resident as uint8; every training batch cuts a new clip of
`--sample-length` frames from each of its videos as the reference's VideoDataset does (dataset.py:500-586; `--sample-step`,
`--temporal-jitter`, `--temporal-jitter-step`, `--random-shift`, generator `numpy.random.RandomState(--sample-seed + rank)`) and prepares it in
the same kernel launch; the validation split takes one clip per video with no shift and no jitter.  The default flags are the
reference script's settings (step 1, no jitter, no shift: r2plus1d_main_universal_attack.py:155-163).  `--eval-num-samples N` scores
whole validation videos after training as the reference's `evaluate(num_samples=N)` does (the argmax of the summed logits of N clips),
clean and under the trained perturbation, prints the video-level accuracy and fooling ratio and stores them in `video_eval.npz`
beside the checkpoints.  Both files of a run are of the same kind; files with a `clips` array behave exactly as before.

`--clips-per-video G` (whole-video files only) attacks that video-level decision: a batch of `--batch-size` clips holds `--batch-size / G`
videos, G clips are cut from each (training split: the sampling flags above; validation: the uniform offsets of the evaluation) and the
adversarial loss is taken on each video's aggregated logits -- `--video-reduce sum` (the evaluation's own sum) or `mean` (the sum / G:
same argmax, margin on the scale of one clip's logits).  Loss averages and fooling ratios then count videos.

`--flicker-time video` (with `--flicker-period P`) trains the flicker on video time: a perturbation of P rows, every frame of every clip
carrying the row of its frame number in its video -- what `--eval-quantised video` and `--save-adversarial-u8` lay over whole videos.
The epoch results hold `flicker_period`.
`--capture-subframe / --capture-exposure / --capture-gain / --capture-readout LO HI` (with `--capture-gain-mode`, `--capture-seed`; video
time only; `--capture-readout`: a rolling shutter, every line of a frame records its own mix of rows) train the
flicker through a camera's capture channel, one drawn per video and step; `--eval-capture-draws N` (whole-video files) scores the trained
flicker over N random captures of the validation videos (`video_eval_capture.npz`).
`--flicker-model illumination` (with `--response srgb|linear`) trains and scores the flicker as scene illumination -- multiplicative in
linear light, through the camera's response tables -- instead of an additive pixel offset; uint8 clips at the engine's size only."""
import argparse
import glob
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flickering_adversarial_video_amd import parallel, videoresnet_spec as vs  # noqa: E402
from flickering_adversarial_video_amd.torch_attack import Adversarial_metrics, FlickerVideoResNet, Losses  # noqa: E402

# ---- the reference's knobs (r2plus1d_main_universal_attack.py:33-58) ----
EPOCHS = 22
LR = 0.001
LAMBDA = 1.0
BETA_1 = 0.5
L_INF_PERT_NORM = 0.1
BASE_MODEL = "mc3_18"            # "mc3_18", "r2plus1d_18", "r3d_18", "ig65m", "kinetics"
USE_LOGITS = False
IMPROVE_LOSS = True
CYCLIC_PERT = False
ATTACK_TYPE = "flickering"
TARGETED_ATTACK = False
INIT_PERT_FROM_LAST_CKPT = True
CONTINUE_TRAIN = True
MODEL_INPUT_SIZE = 16            # frames per clip for the three VideoResNets
BATCH_SIZE = 8                   # BATCH_SIZE_ARRAY[1] (one device per process here)


def engine_size(clips, image_size=None, prepare=None):
    """(engine H = W, whether the clips are raw frames still to be resized / cropped): the clips' own size, as ever, unless they are
    uint8 and not square, or --image-size / --prepare say otherwise (then 112, dataset.py's input_size, or --image-size)"""
    H, W = clips.shape[2], clips.shape[3]
    if clips.dtype != np.uint8:
        return H, False
    S = image_size or (112 if (prepare or H != W) else H)
    return S, (H, W) != (S, S)


def prepare_host_clips(clips, S, im_scale, rule):
    """--prepare host: the four steps of the evaluation transform with torch on the CPU, clip by clip (videoresnet_spec.prepare_host)"""
    return np.stack([vs.prepare_host(c, im_scale=im_scale, input_size=S, rule=rule).numpy() for c in clips])


def host_train_loader(clips, labels, batch_size, S, im_scale, rule, augment, rng, rank=0, world=1):
    """--prepare host with --train-transforms train: every batch of raw frames through videoresnet_spec.prepare_host_train, one (box, flip)
    per clip in clip order from `rng` -- the draws the engine makes on the device route"""
    for i in batch_ids(len(clips), batch_size, rank, world):
        out = []
        for c in clips[i * batch_size:(i + 1) * batch_size]:
            Hr, Wr = vs.prepare_geometry(c.shape[1], c.shape[2], im_scale, S, rule)[:2]
            *box, flip = vs.train_crop_params(Hr, Wr, S, augment["scales"], augment["ratio"], augment["flip_ratio"], rng)
            out.append(vs.prepare_host_train(c, box, flip, im_scale=im_scale, input_size=S, rule=rule))
        yield torch.stack(out).cuda(), torch.from_numpy(labels[i * batch_size:(i + 1) * batch_size]).cuda(), None


def load_clips(path, decode="device", image_size=None, prepare=None, im_scale=128, rule="sizes", keep_raw=False):
    """clips as the file holds them when they are uint8 and decode == "device" (or raw with prepare != "host", or keep_raw: the host
    route's training transform prepares per batch), else normalised float32 on the host"""
    z = np.load(path)
    clips, labels = z["clips"], z["labels"].astype(np.int64)
    S, raw = engine_size(clips, image_size, prepare)
    if raw:
        if prepare == "host" and not keep_raw:
            return prepare_host_clips(clips, S, im_scale, rule), labels
        return np.ascontiguousarray(clips), labels
    if clips.dtype == np.uint8 and decode == "device":
        return np.ascontiguousarray(clips), labels
    if clips.dtype == np.uint8:      # get_normalize_transforms (dataset.py:212-243): /255, mean / std
        clips = vs.normalize_u8(clips)
    return np.ascontiguousarray(clips, dtype=np.float32), labels


def batch_ids(n, batch_size, rank=0, world=1):
    """the batches rank takes, dropping the ragged tail; ranks take alternating batches"""
    nb = n // batch_size
    return range(rank, nb - nb % world if world > 1 else nb, world)


def loader(clips, labels, batch_size, rank=0, world=1):
    """batches of (clip [B,T,H,W,3] on the GPU, label, None), copied from the host per step"""
    for i in batch_ids(len(clips), batch_size, rank, world):
        sl = slice(i * batch_size, (i + 1) * batch_size)
        yield torch.from_numpy(clips[sl]).cuda(), torch.from_numpy(labels[sl]).cuda(), None


class ResidentVideos:
    """whole uint8 videos of the batches one rank takes, uploaded once; a batch is the LIST of its videos (the engine cuts the clips)"""

    def __init__(self, videos, labels, batch_size, rank=0, world=1):
        self.batches = []
        for i in batch_ids(len(videos), batch_size, rank, world):
            sl = slice(i * batch_size, (i + 1) * batch_size)
            self.batches.append(([torch.from_numpy(v).cuda() for v in videos[sl]], torch.from_numpy(labels[sl]).cuda(), None))

    def __iter__(self):
        return iter(self.batches)


def run_whole_videos(a, world, rank, local_rank, augment):
    """main() for whole-video files"""
    if a.prepare == "host":
        raise ValueError("--prepare host applies to files of clips; whole videos are sampled and prepared on the device")
    vtr, ytr, _ = vs.load_video_file(a.train_npz)
    vva, yva, _ = vs.load_video_file(a.val_npz)
    T, HW = a.sample_length, a.image_size or 112
    sampling = {"sample_step": a.sample_step, "temporal_jitter": a.temporal_jitter, "temporal_jitter_step": a.temporal_jitter_step,
                "random_shift": a.random_shift, "seed": a.sample_seed}
    arch, _, ncls = vs.resolve_model(a.base_model, T)
    W = vs.load_weights(a.weights_npz, arch) if a.weights_npz else vs.synthetic_weights(arch, 42, num_classes=ncls)
    learner = FlickerVideoResNet(a.base_model, W, batch_size=a.batch_size, sample_length=T, image_size=HW, dtype=a.dtype,
                                 device=local_rank, l_inf_pert_norm=L_INF_PERT_NORM, cyclic_pert=CYCLIC_PERT, attack_type=a.attack_type,
                                 optimizer=a.optimizer, im_scale=a.im_scale, resize_rule=a.resize_rule, augment=augment, sampling=sampling,
                                 clips_per_video=a.clips_per_video, video_reduce=a.video_reduce, quantise_train=a.quantise_train,
                                 **vs.flicker_keywords_from_arguments(a, delivered=True))
    codec_keys = {} if a.codec is None else {"codec_quality": np.int64(a.codec.quality), "codec_subsampling": a.codec.subsampling,
                                                "codec_gop": np.int64(a.codec.gop), "codec_search": np.int64(a.codec.search)}
    if a.codec_grad not in (None, "identity"):          # (only when set: the default's result files keep their keys)
        codec_keys["codec_grad"] = a.codec_grad
    nvid = a.batch_size // a.clips_per_video          # videos per batch
    dest = os.path.join(a.results_root, learner.model_name, "generalization", "universal", "val_test", f"all_cls_shuffle_{a.attack_type}",
                        f"t_{len(vtr)}_v_{len(vva)}_linf_{L_INF_PERT_NORM}_lambda_{LAMBDA}_beta1_{BETA_1}_")
    start_epoch = 1
    ckpts = sorted(glob.glob(os.path.join(dest, "*.npy")), key=os.path.getmtime)
    if INIT_PERT_FROM_LAST_CKPT and ckpts:
        learner.pert_model.init_perturbation(np.load(ckpts[-1], allow_pickle=True)[-1]["valid/perturbation"])
        print("Success! init from last ckpt")
    if CONTINUE_TRAIN and ckpts:
        start_epoch = int(ckpts[-1].split("_")[-1].split(".")[0]) + 1
        print(f"Success! to continue from last epoch. init with {start_epoch}")
    crit = Losses(beta_1=BETA_1, lambda_=LAMBDA, targeted=TARGETED_ATTACK, improve_loss=IMPROVE_LOSS, logits=USE_LOGITS, attack_type=a.attack_type)
    resident = {"train": ResidentVideos(vtr, ytr, nvid, rank, world), "valid": ResidentVideos(vva, yva, nvid)}
    results = learner.fit(resident, crit, Adversarial_metrics(targeted=TARGETED_ATTACK), lr=a.lr, epochs=a.epochs, model_dir=dest if rank == 0 else None,
                          model_name=learner.model_name, save_model=rank == 0, start_epoch=start_epoch)
    if rank == 0:
        for e, r in enumerate(results, start_epoch):
            print(f"epoch {e}: train loss {r['train/loss']:.5f} fooling {r['train/fooling_ratio']:.4f} | valid loss {r['valid/loss']:.5f} "
                  f"fooling {r['valid/fooling_ratio']:.4f} | thickness {r['valid/pert_thickness']:.5f} roughness {r['valid/pert_roughness']:.5f}", flush=True)
        if a.eval_num_samples > 0:
            ev = learner.evaluate_videos([torch.from_numpy(v).cuda() for v in vva], yva, num_samples=a.eval_num_samples, adversarial=True)
            print(f"video evaluation, {a.eval_num_samples} clips per video, {len(vva)} videos: clean video accuracy {ev['clean_video_accuracy']:.4f} | "
                  f"adversarial video accuracy {ev['video_accuracy']:.4f} clip accuracy {ev['clip_accuracy']:.4f} | "
                  f"video fooling ratio {ev['video_fooling_ratio']:.4f}", flush=True)
            os.makedirs(dest, exist_ok=True)
            np.savez(os.path.join(dest, "video_eval.npz"), num_samples=np.int64(a.eval_num_samples), **ev)
        if a.eval_quantised:                    # the attack as 8-bit frames deliver it: video_eval_quantised.npz beside video_eval.npz
            S = max(a.eval_num_samples, 1)
            codec = a.codec if a.eval_quantised == "video" else None
            ev = learner.evaluate_videos([torch.from_numpy(v).cuda() for v in vva], yva, num_samples=S, quantise=a.eval_quantised,
                                         **({} if codec is None else {"codec": codec}))
            print(f"quantised ({a.eval_quantised}) video evaluation, {S} clips per video: adversarial video accuracy {ev['video_accuracy']:.4f} | "
                  f"video fooling ratio {ev['video_fooling_ratio']:.4f}" + ("" if codec is None else f" | through {codec}"), flush=True)
            if a.eval_quantised == "video":     # one [N_k,3] table per video: stored end to end, with the videos' lengths
                ev["realised_flicker_frames"] = np.array([len(f) for f in ev["realised_flicker"]], np.int64)
                ev["realised_flicker"] = np.concatenate(ev["realised_flicker"])
            if codec is not None:               # one [N_k,2] table per video, end to end like realised_flicker
                ev["codec_stats"] = np.concatenate(ev["codec_stats"])
            os.makedirs(dest, exist_ok=True)
            np.savez(os.path.join(dest, "video_eval_quantised.npz"), num_samples=np.int64(S), quantise=a.eval_quantised, **ev,
                     **({} if codec is None else codec_keys))
        if a.eval_capture_draws:                # the attack as N random cameras record it: video_eval_capture.npz
            S = max(a.eval_num_samples, 1)
            ev = learner.evaluate_videos([torch.from_numpy(v).cuda() for v in vva], yva, num_samples=S, adversarial=True, quantise=a.eval_quantised,
                                         capture=a.capture, capture_draws=a.eval_capture_draws,
                                         **({"codec": a.codec} if a.codec is not None and a.eval_quantised == "video" else {}))
            ev.pop("codec_stats", None)
            print(f"capture evaluation, {a.eval_capture_draws} draws, {S} clips per video: video fooling ratio mean "
                  f"{ev['capture_video_fooling_ratio_mean']:.4f} min {ev['capture_video_fooling_ratio_min']:.4f} (no channel: "
                  f"{ev['video_fooling_ratio']:.4f})", flush=True)
            draws = ev.pop("capture_draws")
            ev.pop("realised_flicker", None)
            os.makedirs(dest, exist_ok=True)
            np.savez(os.path.join(dest, "video_eval_capture.npz"), num_samples=np.int64(S), capture_subframe=np.stack([d["subframe"] for d in draws]),
                     capture_exposure=np.stack([d["exposure"] for d in draws]), capture_gain=np.stack([d["gain"] for d in draws]),
                     **({"capture_readout": np.stack([d["readout"] for d in draws])} if "readout" in draws[0] else {}), **ev)
        if a.save_adversarial_u8:               # the validation videos under the universal flicker, whole and at their own resolution
            os.makedirs(dest, exist_ok=True)
            np.savez(os.path.join(dest, "adversarial_u8.npz"), labels=yva, **codec_keys,
                     **{f"video_{i:05d}": learner.export_video(torch.from_numpy(v).cuda(), **({} if a.codec is None else {"codec": a.codec})).cpu().numpy()
                        for i, v in enumerate(vva)})


def quantised_clip_report(learner, clips, labels, batch_size, keep_frames):
    """the validation clips under the learner's perturbation as 8-bit frames, batch by batch (the ragged tail is dropped, as in training):
    what the network makes of the clean clips, of the float adversarial clips and of the frames"""
    out = {k: [] for k in ("clean_preds", "adv_preds", "quantised_preds", "realised_flicker", "adv_clips_u8")}
    for i in batch_ids(len(clips), batch_size):
        x = learner._prepared(torch.from_numpy(clips[i * batch_size:(i + 1) * batch_size]).cuda())
        out["clean_preds"].append(learner.logits(x, False).argmax(1).cpu().numpy())
        out["adv_preds"].append(learner.logits(x, True).argmax(1).cpu().numpy())
        frames, st = learner.adversarial_frames(x, stats=True)
        out["quantised_preds"].append(learner.logits(frames, False).argmax(1).cpu().numpy())
        out["realised_flicker"].append(st[..., 0].cpu().numpy() / float(learner.H * learner.W))
        if keep_frames:
            out["adv_clips_u8"].append(frames.cpu().numpy())
    out = {k: np.concatenate(v) for k, v in out.items() if v}
    y = labels[:len(out["clean_preds"])]
    ok = out["clean_preds"] == y
    out["labels"] = y
    out["fooling_ratio"] = float(((out["adv_preds"] != y) & ok).sum() / ok.sum()) if ok.any() else float("nan")
    out["quantised_fooling_ratio"] = float(((out["quantised_preds"] != y) & ok).sum() / ok.sum()) if ok.any() else float("nan")
    return out


class ResidentShard:
    """uint8 clips of the batches one rank takes, uploaded once; every epoch's batches are slices of the device tensor"""

    def __init__(self, clips, labels, batch_size, rank=0, world=1):
        ids = list(batch_ids(len(clips), batch_size, rank, world))
        rows = np.concatenate([np.arange(i * batch_size, (i + 1) * batch_size) for i in ids]) if ids else np.zeros(0, np.int64)
        self.bs, self.n = batch_size, len(ids)
        self.x = torch.from_numpy(np.ascontiguousarray(clips[rows])).cuda()
        self.y = torch.from_numpy(labels[rows]).cuda()

    def __iter__(self):
        for k in range(self.n):
            yield self.x[k * self.bs:(k + 1) * self.bs], self.y[k * self.bs:(k + 1) * self.bs], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-npz", required=True)
    ap.add_argument("--val-npz", required=True)
    ap.add_argument("--weights-npz", "--weights", dest="weights_npz", default="",
                    help="victim weights: a torchvision state_dict (.pth / .pt, what model.py:421 downloads) or an .npz of the same names; "
                         "'' = seeded synthetic weights")
    ap.add_argument("--attack-type", default=ATTACK_TYPE, choices=["flickering", "L12"], help="L12: dense [3,T,H,W] perturbation (model.py:380-384)")
    ap.add_argument("--results-root", default=os.path.join(os.getcwd(), "results"))
    ap.add_argument("--base-model", default=BASE_MODEL, help="r2plus1d_18 / r3d_18 / mc3_18, ig65m / kinetics (R(2+1)D-34 at 8 or 32 "
                    "frames, model.py:341,418-441) or an r2plus1d_34_{8|32}_{ig65m|kinetics} name")
    ap.add_argument("--epochs", type=int, default=EPOCHS)
    ap.add_argument("--batch-size", type=int, default=BATCH_SIZE)
    ap.add_argument("--lr", type=float, default=LR)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--optimizer", default="adam", choices=["adam", "pgd"], help="pgd: projected sign-gradient steps, delta <- clamp(delta - "
                    "lr * sgn(grad), +-l_inf norm), instead of Adam (model.py:868); --lr is the step size and StepLR scales it")
    ap.add_argument("--decode", default="device", choices=["device", "host"], help="uint8 clips: normalise on the device from a resident "
                    "uint8 copy (default), or on the host with a float32 copy per step (float32 files always take the host route)")
    ap.add_argument("--prepare", default=None, choices=["device", "host"], help="raw uint8 frames (not at the engine's H x W): resize, centre "
                    "crop and normalise every batch on the device from the resident raw shard (default for such files), or once on the host "
                    "with torch; ignored for clips already at the engine's size")
    ap.add_argument("--resize-rule", default="sizes", choices=list(vs.RESIZE_RULES), help="coordinate rule of the bilinear resize: sizes = step in / "
                    "out per axis (F.interpolate(size=...); torch 1.4.0, the reference's pin), scale_factor = step 1 / scale (current torch)")
    ap.add_argument("--image-size", type=int, default=None, help="engine H = W (default: the clips' own size; 112 for raw frames)")
    ap.add_argument("--im-scale", type=int, default=128, help="raw frames: the shorter side after the resize (dataset.py's im_scale)")
    ap.add_argument("--train-transforms", default="eval", choices=["eval", "train"], help="raw frames of the training split: eval = resize, centre "
                    "crop (what the reference's attack scripts use for both splits), train = the reference's training transform: random resized "
                    "crop and horizontal flip, new draws every epoch (dataset.py:105-118)")
    ap.add_argument("--aug-scales", type=float, nargs=2, default=[0.6, 1.0], metavar=("LO", "HI"), help="train: area range of the random "
                    "resized crop (dataset.py's random_crop_scales)")
    ap.add_argument("--aug-no-resize", action="store_true", help="train: RandomCropVideo(image size) instead of the resized crop (random_crop_scales=None)")
    ap.add_argument("--flip-ratio", type=float, default=0.5, help="train: probability of the horizontal flip")
    ap.add_argument("--aug-seed", type=int, default=0, help="train: the sampler is random.Random(seed + rank)")
    ap.add_argument("--sample-length", type=int, default=MODEL_INPUT_SIZE, help="whole-video files: frames per clip (files of clips bring their own)")
    ap.add_argument("--sample-step", type=int, default=1, help="whole-video files: frames between the frames of a clip (dataset.py's sample_step)")
    ap.add_argument("--temporal-jitter", action="store_true", help="whole-video files, training split: a random step of 0 .. "
                    "--temporal-jitter-step frames between the frames of a clip (step 0 repeats the frame)")
    ap.add_argument("--temporal-jitter-step", type=int, default=2)
    ap.add_argument("--random-shift", action="store_true", help="whole-video files, training split: clips start at random offsets, not uniform ones")
    ap.add_argument("--sample-seed", type=int, default=0, help="whole-video files: the frame sampler is numpy.random.RandomState(seed + rank)")
    ap.add_argument("--eval-num-samples", type=int, default=0, help="whole-video files: after training, score every validation video by N clips "
                    "(the reference's evaluate(num_samples=N)) clean and perturbed; 0 = skip")
    ap.add_argument("--clips-per-video", type=int, default=1, help="whole-video files: G clips per video in every batch and the adversarial loss "
                    "on each video's aggregated logits (what --eval-num-samples G decides on); --batch-size must be a multiple of G; 1 = per-clip loss")
    ap.add_argument("--video-reduce", default="mean", choices=["mean", "sum"], help="--clips-per-video > 1: the loss takes the mean (default) or "
                    "the sum of a video's clip logits")
    ap.add_argument("--gpus", type=int, default=None, help="data-parallel ranks, one process per GPU (the reference's DEVICES_IDS, "
                    "r2plus1d_main_universal_attack.py:30-33); without a launcher in the environment the script starts them itself")
    ap.add_argument("--save-adversarial-u8", action="store_true", help="after training, write the validation set under the universal perturbation "
                    "as 8-bit frames: quantised_eval.npz gains adv_clips_u8 uint8 [N,T,H,W,3] (files of clips); adversarial_u8.npz holds every "
                    "whole validation video flickered at its own resolution (whole-video files)")
    ap.add_argument("--quantise-train", action="store_true", help="optimise the attack on the STORED video: every adversarial forward of the "
                    "training loop sees the clip its 8-bit frames decode to (the round trip runs inside the apply kernel, straight-through "
                    "gradient), so the loop's verdicts are the stored video's.  Combines with --save-adversarial-u8 / --eval-quantised")
    ap.add_argument("--train-delivered", action="store_true", help="whole-video files, --flicker-time video: optimise the attack on the "
                    "DELIVERED video at its native resolution -- every training step flickers the raw frames in 8 bits as the whole-video "
                    "export does, resizes and crops the stored bytes and scores them clean (the chain --eval-quantised video scores), and "
                    "takes the gradient back through the resampling.  Files of clips at the engine's size: use --quantise-train")
    ap.add_argument("--flicker-time", default="clip", choices=["clip", "video"], help="which row of the perturbation a frame carries.  clip: row t "
                    "for frame t of every clip.  video: row (frame number - phase) mod period, the frame numbers being those the clip was cut "
                    "at in its video -- the flicker the whole-video export lays over the video, so the loop trains on what is delivered "
                    "(flickering attack, one shared perturbation; files of clips count their frames from 0)")
    ap.add_argument("--flicker-period", type=int, default=None, help="--flicker-time video: rows of the perturbation = the flicker's period in "
                    "frames (default: the clip length; 1..682)")
    ap.add_argument("--eval-quantised", default=None, choices=["clip", "video"], help="after training, score the attack as 8-bit frames deliver "
                    "it.  clip: every validation clip exported at the engine's size (quantised_eval.npz; whole-video files: "
                    "video_eval_quantised.npz); video (whole-video files): every validation video flickered whole at its own resolution, "
                    "then the clean evaluation (video_eval_quantised.npz)")
    vs.add_capture_arguments(ap)
    vs.add_flicker_model_arguments(ap)
    vs.add_codec_arguments(ap)
    a = ap.parse_args()
    a.capture = vs.capture_from_arguments(ap, a)
    a.codec = vs.codec_from_arguments(ap, a, a.eval_quantised == "video" or a.train_delivered
                                      or (a.save_adversarial_u8 and vs.is_video_file(a.val_npz)))
    if a.eval_capture_draws and not vs.is_video_file(a.val_npz):
        ap.error("--eval-capture-draws needs whole-video .npz files: the captures are scored on the validation videos' evaluation clips")
    if a.eval_quantised == "video" and not (vs.is_video_file(a.train_npz) and vs.is_video_file(a.val_npz)):      # before anything touches the GPU
        raise ValueError("--eval-quantised video needs whole-video .npz files: a file of clips holds no whole video to flicker")
    if (a.eval_quantised == "video" or (a.save_adversarial_u8 and vs.is_video_file(a.val_npz))) and a.attack_type != "flickering":
        raise ValueError("whole videos take the flickering perturbation only (a dense perturbation belongs to the clip's size)")
    if a.train_delivered and not (vs.is_video_file(a.train_npz) and vs.is_video_file(a.val_npz)):      # before anything touches the GPU
        raise ValueError("--train-delivered needs whole-video .npz files: clips have no native resolution to flicker at -- for files of "
                         "clips at the engine's size use --quantise-train, which trains on the same stored bytes")
    if a.train_delivered and a.flicker_time != "video":
        raise ValueError("--train-delivered needs --flicker-time video: the delivered video carries the flicker on its own frame numbers")
    if a.clips_per_video < 1:
        raise ValueError(f"--clips-per-video must be >= 1, got {a.clips_per_video}")
    if a.clips_per_video > 1 and not (vs.is_video_file(a.train_npz) and vs.is_video_file(a.val_npz)):      # before anything touches the GPU
        raise ValueError("--clips-per-video > 1 needs whole-video .npz files (labels and video_00000, video_00001, ...): the clips of "
                         "a video are cut from it; files with a `clips` array do not say which clips share a video")
    if a.gpus and a.gpus > 1 and "WORLD_SIZE" not in os.environ:      # before anything touches the GPU
        sys.exit(parallel.launch_ranks(a.gpus, __file__, sys.argv[1:]))
    world, rank, local_rank = parallel.ranks_from_env(a.gpus)
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    augment = None
    if a.train_transforms == "train":
        augment = {"scales": None if a.aug_no_resize else tuple(a.aug_scales), "ratio": (3 / 4, 4 / 3), "flip_ratio": a.flip_ratio, "seed": a.aug_seed}
    whole = vs.is_video_file(a.train_npz)
    if whole != vs.is_video_file(a.val_npz):
        raise ValueError("--train-npz and --val-npz must both hold clips or both hold whole videos")
    if whole:
        run_whole_videos(a, world, rank, local_rank, augment)
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    xtr, ytr = load_clips(a.train_npz, a.decode, a.image_size, a.prepare, a.im_scale, a.resize_rule, keep_raw=augment is not None)
    xva, yva = load_clips(a.val_npz, a.decode, a.image_size, a.prepare, a.im_scale, a.resize_rule)
    T, (HW, raw_train) = xtr.shape[1], engine_size(xtr, a.image_size, a.prepare)
    if augment is not None and not raw_train:
        raise ValueError("--train-transforms train applies to raw uint8 frames; the training clips are at the engine's size already")
    host_aug = augment is not None and a.prepare == "host"      # the host draws and prepares per batch; the engine then gets finished clips
    # --base-model: an architecture, "ig65m" / "kinetics" (R(2+1)D-34, 8 or 32 frames) or an r2plus1d_34_* name; the class count is the
    # weights' fc head (the synthetic stand-in takes the pretrained model's, model.py:46-56)
    arch, _, ncls = vs.resolve_model(a.base_model, T)
    W = vs.load_weights(a.weights_npz, arch) if a.weights_npz else vs.synthetic_weights(arch, 42, num_classes=ncls)
    learner = FlickerVideoResNet(a.base_model, W, batch_size=a.batch_size, sample_length=T, image_size=HW, dtype=a.dtype,
                                 device=local_rank, l_inf_pert_norm=L_INF_PERT_NORM, cyclic_pert=CYCLIC_PERT, attack_type=a.attack_type,
                                 optimizer=a.optimizer, im_scale=a.im_scale, resize_rule=a.resize_rule,
                                 augment=None if host_aug else augment, quantise_train=a.quantise_train,
                                 **vs.flicker_keywords_from_arguments(a))
    host_rng = random.Random(augment["seed"] + rank) if host_aug else None
    dest = os.path.join(a.results_root, learner.model_name, "generalization", "universal", "val_test", f"all_cls_shuffle_{a.attack_type}",
                        f"t_{len(xtr)}_v_{len(xva)}_linf_{L_INF_PERT_NORM}_lambda_{LAMBDA}_beta1_{BETA_1}_")
    start_epoch = 1
    ckpts = sorted(glob.glob(os.path.join(dest, "*.npy")), key=os.path.getmtime)
    if INIT_PERT_FROM_LAST_CKPT and ckpts:        # r2plus1d_main_universal_attack.py:199-208
        learner.pert_model.init_perturbation(np.load(ckpts[-1], allow_pickle=True)[-1]["valid/perturbation"])
        print("Success! init from last ckpt")
    if CONTINUE_TRAIN and ckpts:                  # :210-219
        start_epoch = int(ckpts[-1].split("_")[-1].split(".")[0]) + 1
        print(f"Success! to continue from last epoch. init with {start_epoch}")
    crit = Losses(beta_1=BETA_1, lambda_=LAMBDA, targeted=TARGETED_ATTACK, improve_loss=IMPROVE_LOSS, logits=USE_LOGITS, attack_type=a.attack_type)

    resident = {}

    class Loaders(dict):                          # fresh iterators every epoch
        def __getitem__(self, phase):
            x, y = (xtr, ytr) if phase == "train" else (xva, yva)
            r, w = (rank, world) if phase == "train" else (0, 1)
            if phase == "train" and host_aug:
                return host_train_loader(x, y, a.batch_size, HW, a.im_scale, a.resize_rule, FlickerVideoResNet._check_augment(augment), host_rng, r, w)
            if x.dtype == np.uint8:               # --decode device / --prepare device: the shard is uploaded on first use, then sliced
                if phase not in resident:
                    resident[phase] = ResidentShard(x, y, a.batch_size, r, w)
                return iter(resident[phase])
            return loader(x, y, a.batch_size, r, w)
    results = learner.fit(Loaders(), crit, Adversarial_metrics(targeted=TARGETED_ATTACK), lr=a.lr, epochs=a.epochs, model_dir=dest if rank == 0 else None,
                          model_name=learner.model_name, save_model=rank == 0, start_epoch=start_epoch)
    if rank == 0:
        for e, r in enumerate(results, start_epoch):
            print(f"epoch {e}: train loss {r['train/loss']:.5f} fooling {r['train/fooling_ratio']:.4f} | valid loss {r['valid/loss']:.5f} "
                  f"fooling {r['valid/fooling_ratio']:.4f} | thickness {r['valid/pert_thickness']:.5f} roughness {r['valid/pert_roughness']:.5f}", flush=True)
        if a.save_adversarial_u8 or a.eval_quantised:           # quantised_eval.npz: the validation clips as 8-bit frames and their verdict
            rep = quantised_clip_report(learner, xva, yva, a.batch_size, a.save_adversarial_u8)
            print(f"quantised evaluation, {len(rep['labels'])} validation clips: fooling ratio {rep['fooling_ratio']:.4f} as float clips, "
                  f"{rep['quantised_fooling_ratio']:.4f} as 8-bit frames", flush=True)
            os.makedirs(dest, exist_ok=True)
            np.savez(os.path.join(dest, "quantised_eval.npz"), **rep)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
