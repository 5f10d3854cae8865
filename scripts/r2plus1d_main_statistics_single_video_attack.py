#!/usr/bin/env python3
"""Single-video flickering attacks on a list of clips with per-video result files -- the MI355X counterpart of the reference's
r2plus1d_main_statistics_single_video_attack.py (knobs :28-48, `learner.fit_many_videos` :190-200, result files
model.py:917-921).  Clips come pre-decoded (no mp4 decoder here): `--videos-npz` holds `clips` [N,T,112,112,3] (uint8 or
normalised float32), `labels` [N] and optionally `names` [N]; class names from `--label-map` (one per line).  uint8 clips are
uploaded once and stay uint8 (`--decode device`, the default: the attack's apply kernel normalises them, bitwise the host route);
`--decode host` normalises them on the host into float32 and copies each video on its turn, like float32 files.
uint8 clips may also be RAW decoded frames of any H x W (what the reference's loader hands its transform, dataset.py:84-123): each
video is resized (shorter side to `--im-scale`), centre-cropped to `--image-size` and normalised by one kernel from the resident raw
upload (`--prepare device`, the default for such files) or on the host with torch (`--prepare host`); `--resize-rule` picks the
coordinate rule (videoresnet_spec.prepare_geometry).  Clips are raw when they are not square, or not `--image-size` when that is
given, or whenever `--prepare` is given (the engine then is 112 x 112 unless `--image-size` says otherwise).
WHOLE-VIDEO files: `labels` (int64 [V]) and `video_00000`, `video_00001`, ... (each uint8 [N_k,H_k,W_k,3]) instead of `clips`.  The
videos stay resident as uint8 and the clip of `--sample-length` frames attacked in each is cut as the reference's VideoDataset cuts
it (dataset.py:500-586: `--sample-step`, `--temporal-jitter`, `--temporal-jitter-step`, `--random-shift`, generator
`numpy.random.RandomState(--sample-seed)`) and prepared in the same kernel launch; the defaults are the reference script's settings
(one clip at the uniform offset, step 1, no jitter, no shift).
`--clips-per-video G` (whole-video files, `--batch 1`) attacks the video-level decision of the reference's evaluate(num_samples=G): the G
clips at the evaluation's uniform offsets are cut from each video once and the adversarial loss is taken on their aggregated logits
(`--video-reduce sum`, or `mean` = sum / G: same argmax); a video counts as adversarial when the argmax of those logits leaves its label.
`--flicker-time video` (with `--flicker-period P`) trains the flicker on video time: a perturbation of P rows, every frame carrying the row of
its frame number in the video, which is what `--eval-quantised video` lays over the whole video; the result files hold `flicker_period`.
`--capture-subframe / --capture-exposure / --capture-gain / --capture-readout LO HI` (with `--capture-gain-mode`, `--capture-seed`; video
time only; `--capture-readout`: a rolling shutter, every line of a frame records its own mix of rows) train the
flicker through a camera's capture channel, one drawn per video and step; `--eval-capture-draws N` scores the final flicker over N random
captures (`capture_video_preds`, `capture_video_is_adversarial` [N], `capture_draws`).
`--flicker-model illumination` (with `--response srgb|linear`) trains and scores the flicker as scene illumination -- multiplicative in
linear light, through the camera's response tables -- instead of an additive pixel offset; uint8 clips at the engine's size only."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flickering_adversarial_video_amd import videoresnet_spec as vs  # noqa: E402
from flickering_adversarial_video_amd.torch_attack import FlickerVideoResNet, Losses  # noqa: E402

BASE_MODEL = "r2plus1d_18"       # "mc3_18", "r2plus1d_18", "r3d_18", "ig65m", "kinetics"
USE_LOGITS = True
IMPROVE_LOSS = True
CYCLIC_PERT = False
ATTACK_TYPE = "flickering"
L_INF_PERT_NORM = 0.2
TARGETED_ATTACK = False
LR = 0.001
LAMBDA = 1.0
BETA_1 = 0.5
N_ITER = 3000                    # fit_single_video_attack(n_iter=3000), model.py:962
MODEL_INPUT_SIZE = 16            # frames per clip for the three VideoResNets


def run_whole_videos(a):
    """main() for whole-video files: one clip per video, cut and prepared on the device, then the loop of clips at the engine's size"""
    if a.prepare == "host":
        raise ValueError("--prepare host applies to files of clips; whole videos are sampled and prepared on the device")
    videos, labels, names = vs.load_video_file(a.videos_npz)
    T, S = a.sample_length, a.image_size or 112
    sampling = {"sample_step": a.sample_step, "temporal_jitter": a.temporal_jitter, "temporal_jitter_step": a.temporal_jitter_step,
                "random_shift": a.random_shift, "seed": a.sample_seed}
    classes = [l.strip() for l in open(a.label_map)] if a.label_map else None
    arch, _, ncls = vs.resolve_model(a.base_model, T)
    W = vs.load_weights(a.weights_npz, arch) if a.weights_npz else vs.synthetic_weights(arch, 42, num_classes=ncls)
    G = a.clips_per_video
    if G > 1 and a.batch > 1:
        raise ValueError("--clips-per-video > 1 attacks one video (its G clips) at a time: it does not combine with --batch > 1")
    learner = FlickerVideoResNet(a.base_model, W, batch_size=G if G > 1 else a.batch, sample_length=T, image_size=S, dtype=a.dtype,
                                 l_inf_pert_norm=L_INF_PERT_NORM, cyclic_pert=CYCLIC_PERT, attack_type=a.attack_type, per_clip=a.batch > 1,
                                 optimizer=a.optimizer, im_scale=a.im_scale, resize_rule=a.resize_rule, sampling=sampling,
                                 clips_per_video=G, video_reduce=a.video_reduce, quantise_train=a.quantise_train,
                                 **vs.flicker_keywords_from_arguments(a, delivered=True))
    dest =os.path.join(a.results_root, learner.model_name, "single_video_attack", a.attack_type,
                        f"linf_{L_INF_PERT_NORM}_lambda_{LAMBDA}_beta1_{BETA_1}_")
    crit = Losses(beta_1=BETA_1, lambda_=LAMBDA, targeted=TARGETED_ATTACK, improve_loss=IMPROVE_LOSS, logits=USE_LOGITS, attack_type=a.attack_type)
    xd, yd = [torch.from_numpy(v).cuda() for v in videos], torch.from_numpy(labels).cuda()
    # train=True: fit_many_videos iterates the dataset's TRAINING loader (model.py:832); with the default flags the two splits sample alike
    if G > 1 or a.train_delivered:        # whole videos go through: fit_single_video_attack cuts each one's G evaluation clips
        clips = ((xd[i], yd[i:i + 1], names[i]) for i in range(len(videos)))
    else:
        clips = ((learner.prepare_videos([xd[i]], train=True).clone(), yd[i:i + 1], names[i]) for i in range(len(videos)))
    out = learner.fit_many_videos(clips, crit, lr=LR, model_dir=dest, label_id_to_text=classes, n_iter=a.n_iter, restart_after=a.restart_after,
                                  reset_optimizer_per_video=a.reset_optimizer_per_video, **export_kw(a))
    if a.eval_capture_draws:
        # the attack as N random cameras record it: each video's final flicker through N channels drawn from --capture-*
        for i, name in enumerate(names):
            r = out.get(str(name))
            if r is None:
                continue
            learner.pert_model.init_perturbation(r["perturbation"][-1])
            learner.pert_model.dynamic_max_norm = max(learner.pert_model.max_norm, r["perturbation/inf_norm"])
            ev = learner.evaluate_videos([xd[i]], labels[i:i + 1], num_samples=G, adversarial=True, quantise=a.eval_quantised, capture=a.capture,
                                         capture_draws=a.eval_capture_draws)
            r["capture_draws"] = ev["capture_draws"]
            r["capture_video_preds"] = ev["capture_video_logits"].argmax(-1)[:, 0]
            r["capture_video_is_adversarial"] = r["capture_video_preds"] != labels[i]
            if a.eval_quantised != "video":          # (that branch below saves the file itself)
                cls = (classes[int(labels[i])] if classes is not None else str(int(labels[i]))).replace(" ", "_")
                np.save(os.path.join(dest, f"{os.path.basename(str(name))}_@{cls}.npy"), dict(r, prob_clean_input=r["prob_clean_input"].cpu().numpy()),
                        allow_pickle=True)
    if a.eval_quantised == "video":
        # the attack as a whole video delivers it: each video's final flicker laid over ALL its frames at their own resolution
        # (export_video), the stored video then scored by the ordinary clean evaluation over its G clips
        for i, name in enumerate(names):
            r = out.get(str(name))
            if r is None:
                continue
            learner.pert_model.init_perturbation(r["perturbation"][-1])              # the clamped final perturbation of this video ...
            learner.pert_model.dynamic_max_norm = max(learner.pert_model.max_norm, r["perturbation/inf_norm"])      # ... under its own bound
            exported, st = learner.export_video(xd[i], stats=True, **({} if a.codec is None else {"codec": a.codec}))
            if a.codec is not None:             # the stored video went through the codec before it is scored
                r["codec_quality"], r["codec_subsampling"], r["codec_gop"] = a.codec.quality, a.codec.subsampling, a.codec.gop
                r["codec_search"] = a.codec.search
                if a.codec_grad not in (None, "identity"):
                    r["codec_grad"] = a.codec_grad
            ev = learner.evaluate_videos([exported], labels[i:i + 1], num_samples=G, adversarial=False)
            r["quantised_video_pred"] = ev["video_preds"]
            r["quantised_video_is_adversarial"] = bool(ev["video_preds"][0] != labels[i])
            r["realised_flicker"] = st[:, :, 0].cpu().numpy() / float(xd[i].shape[1] * xd[i].shape[2])
            cls = (classes[int(labels[i])] if classes is not None else str(int(labels[i]))).replace(" ", "_")
            np.save(os.path.join(dest, f"{os.path.basename(str(name))}_@{cls}.npy"), dict(r, prob_clean_input=r["prob_clean_input"].cpu().numpy()),
                    allow_pickle=True)
    return out


def export_kw(a):
    """fit_many_videos keywords of --save-adversarial-u8 / --eval-quantised clip (none when both are off: the result files keep today's keys)"""
    if a.save_adversarial_u8:
        return {"export_u8": True}
    return {"export_u8": "verdict"} if a.eval_quantised == "clip" else {}


def report(out):
    for name, r in out.items():
        if r is None:
            print(f"{name}: clean clip misclassified, skipped")
        else:
            q = "".join(f", {k.replace('_', ' ')} {bool(r[k])}" for k in ("quantised_is_adversarial", "quantised_video_is_adversarial") if k in r)
            if "capture_video_is_adversarial" in r:
                q += f", adversarial in {int(r['capture_video_is_adversarial'].sum())} of {len(r['capture_video_is_adversarial'])} captures"
            print(f"{name}: {len(r['loss/total'])} iterations, adversarial {bool(r['is_adversarial'][-1])}, thickness "
                  f"{r['perturbation/thickness'][-1]:.4f}, roughness {r['perturbation/roughness'][-1]:.4f}, restarts {r['restarts']}{q}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos-npz", required=True)
    ap.add_argument("--label-map", default="")
    ap.add_argument("--weights-npz", "--weights", dest="weights_npz", default="",
                    help="victim weights: a torchvision state_dict (.pth / .pt, what model.py:421 downloads) or an .npz of the same names; "
                         "'' = seeded synthetic weights")
    ap.add_argument("--attack-type", default=ATTACK_TYPE, choices=["flickering", "L12"], help="L12: dense [3,T,H,W] perturbation (model.py:380-384)")
    ap.add_argument("--results-root", default=os.path.join(os.getcwd(), "results"))
    ap.add_argument("--base-model", default=BASE_MODEL, help="r2plus1d_18 / r3d_18 / mc3_18, ig65m / kinetics (R(2+1)D-34 at 8 or 32 "
                    "frames, model.py:341,418-441) or an r2plus1d_34_{8|32}_{ig65m|kinetics} name")
    ap.add_argument("--n-iter", type=int, default=N_ITER)
    ap.add_argument("--restart-after", type=int, default=3000)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--optimizer", default="adam", choices=["adam", "pgd"], help="pgd: projected sign-gradient steps, delta <- clamp(delta - "
                    "lr * sgn(grad), +-clamp bound), instead of Adam (model.py:868); the restart schedule grows the radius with the clamp bound")
    ap.add_argument("--batch", type=int, default=1, help="videos attacked at once, each with its own perturbation / clamp bound / Adam state "
                    "(flickering attack; 1 = the reference's one-by-one loop)")
    ap.add_argument("--decode", default="device", choices=["device", "host"], help="uint8 clips: normalise on the device from a resident "
                    "uint8 copy (default), or on the host into float32 (float32 files always take the host route)")
    ap.add_argument("--prepare", default=None, choices=["device", "host"], help="raw uint8 frames (not at the engine's H x W): resize, centre "
                    "crop and normalise each video on the device from the resident raw upload (default for such files), or on the host with "
                    "torch; ignored for clips already at the engine's size")
    ap.add_argument("--resize-rule", default="sizes", choices=list(vs.RESIZE_RULES), help="coordinate rule of the bilinear resize: sizes = step in / "
                    "out per axis (F.interpolate(size=...); torch 1.4.0, the reference's pin), scale_factor = step 1 / scale (current torch)")
    ap.add_argument("--image-size", type=int, default=None, help="engine H = W (default: the clips' own size; 112 for raw frames)")
    ap.add_argument("--im-scale", type=int, default=128, help="raw frames: the shorter side after the resize (dataset.py's im_scale)")
    ap.add_argument("--reset-optimizer-per-video", action="store_true", help="fresh Adam state for every video (the reference carries one "
                    "state from video to video, model.py:946; with --batch > 1 the carried state is per batch slot; --optimizer pgd keeps no "
                    "state, so there is nothing to reset)")
    ap.add_argument("--sample-length", type=int, default=MODEL_INPUT_SIZE, help="whole-video files: frames per clip (files of clips bring their own)")
    ap.add_argument("--sample-step", type=int, default=1, help="whole-video files: frames between the frames of a clip (dataset.py's sample_step)")
    ap.add_argument("--temporal-jitter", action="store_true", help="whole-video files, training split: a random step of 0 .. "
                    "--temporal-jitter-step frames between the frames of a clip (step 0 repeats the frame)")
    ap.add_argument("--temporal-jitter-step", type=int, default=2)
    ap.add_argument("--random-shift", action="store_true", help="whole-video files, training split: clips start at random offsets, not uniform ones")
    ap.add_argument("--sample-seed", type=int, default=0, help="whole-video files: the frame sampler is numpy.random.RandomState(seed + rank)")
    ap.add_argument("--clips-per-video", type=int, default=1, help="whole-video files: attack the decision on the aggregated logits of the G "
                    "evaluation clips of each video (the reference's evaluate(num_samples=G)); 1 = one clip, per-clip loss")
    ap.add_argument("--video-reduce", default="mean", choices=["mean", "sum"], help="--clips-per-video > 1: the loss takes the mean (default) or "
                    "the sum of a video's clip logits")
    ap.add_argument("--save-adversarial-u8", action="store_true", help="the result files also hold adv_video_u8 -- the attacked clip under its "
                    "final perturbation as 8-bit frames, uint8 [B,T,H,W,3], written by one kernel -- with quantised_pred and quantised_is_adversarial")
    ap.add_argument("--quantise-train", action="store_true", help="optimise the attack on the STORED video: every adversarial forward of the "
                    "training loop sees the clip its 8-bit frames decode to (the round trip runs inside the apply kernel, straight-through "
                    "gradient), so the loop's verdicts are the stored video's.  Combines with --save-adversarial-u8 / --eval-quantised")
    ap.add_argument("--train-delivered", action="store_true", help="whole-video files, --flicker-time video, --batch 1: optimise each attack on "
                    "the DELIVERED video at its native resolution -- every step flickers the raw frames in 8 bits as the whole-video export "
                    "does, resizes and crops the stored bytes and scores them clean, and takes the gradient back through the resampling.  "
                    "Files of clips at the engine's size: use --quantise-train")
    ap.add_argument("--flicker-time", default="clip", choices=["clip", "video"], help="which row of the perturbation a frame carries.  clip: row t "
                    "for frame t of every clip.  video: row (frame number - phase) mod period, the frame numbers being those the clip was cut "
                    "at in its video -- the flicker the whole-video export lays over the video, so the loop trains on what is delivered "
                    "(flickering attack, one shared perturbation; files of clips count their frames from 0)")
    ap.add_argument("--flicker-period", type=int, default=None, help="--flicker-time video: rows of the perturbation = the flicker's period in "
                    "frames (default: the clip length; 1..682)")
    ap.add_argument("--eval-quantised", default=None, choices=["clip", "video"], help="is the STORED video still adversarial?  clip: the result "
                    "files hold quantised_pred / quantised_is_adversarial of the clip's 8-bit frames; video (whole-video files, --batch 1): the "
                    "final flicker over the whole video at its own resolution, scored by the clean evaluation -- quantised_video_pred, "
                    "quantised_video_is_adversarial, realised_flicker (levels per frame and channel)")
    vs.add_capture_arguments(ap)
    vs.add_flicker_model_arguments(ap)
    vs.add_codec_arguments(ap)
    a = ap.parse_args()
    a.capture = vs.capture_from_arguments(ap, a)
    a.codec = vs.codec_from_arguments(ap, a, a.eval_quantised == "video" or a.train_delivered)
    if a.eval_capture_draws and not vs.is_video_file(a.videos_npz):
        ap.error("--eval-capture-draws needs a whole-video .npz file: the captures are scored on the video's evaluation clips")
    if a.eval_quantised == "video" and (not vs.is_video_file(a.videos_npz) or a.batch > 1 or a.attack_type != "flickering"):
        raise ValueError("--eval-quantised video needs a whole-video .npz file, --batch 1 and the flickering attack (one flicker per video, laid "
                         "over all its frames)")
    if a.train_delivered and (not vs.is_video_file(a.videos_npz) or a.batch > 1 or a.flicker_time != "video"):
        raise ValueError("--train-delivered needs a whole-video .npz file, --batch 1 and --flicker-time video: clips have no native resolution "
                         "to flicker at -- for files of clips at the engine's size use --quantise-train, which trains on the same stored bytes")
    if a.clips_per_video < 1:
        raise ValueError(f"--clips-per-video must be >= 1, got {a.clips_per_video}")
    if a.clips_per_video > 1 and not vs.is_video_file(a.videos_npz):
        raise ValueError("--clips-per-video > 1 needs a whole-video .npz file (labels and video_00000, video_00001, ...): the clips of a "
                         "video are cut from it")
    if vs.is_video_file(a.videos_npz):
        return report(run_whole_videos(a))
    z = np.load(a.videos_npz, allow_pickle=True)
    clips, labels = z["clips"], z["labels"].astype(np.int64)
    names = [str(n) for n in z["names"]] if "names" in z else [f"video_{i:05d}" for i in range(len(clips))]
    # engine H = W: the clips' own size, as ever, unless they are uint8 and not square, or --image-size / --prepare say otherwise
    S, raw = clips.shape[2], False
    if clips.dtype == np.uint8:
        S = a.image_size or (112 if (a.prepare or clips.shape[2] != clips.shape[3]) else clips.shape[2])
        raw = tuple(clips.shape[2:4]) != (S, S)
    if raw and a.prepare == "host":      # the four steps of the evaluation transform with torch on the CPU (videoresnet_spec.prepare_host)
        clips = np.stack([vs.prepare_host(c, im_scale=a.im_scale, input_size=S, rule=a.resize_rule).numpy() for c in clips])
    elif raw or (clips.dtype == np.uint8 and a.decode == "device"):
        clips = np.ascontiguousarray(clips)
    else:
        if clips.dtype == np.uint8:
            clips = vs.normalize_u8(clips)
        clips = np.ascontiguousarray(clips, dtype=np.float32)
    classes = [l.strip() for l in open(a.label_map)] if a.label_map else None
    # --base-model: an architecture, "ig65m" / "kinetics" (R(2+1)D-34, 8 or 32 frames) or an r2plus1d_34_* name; the class count is the
    # weights' fc head (the synthetic stand-in takes the pretrained model's, model.py:46-56)
    arch, _, ncls = vs.resolve_model(a.base_model, clips.shape[1])
    W = vs.load_weights(a.weights_npz, arch) if a.weights_npz else vs.synthetic_weights(arch, 42, num_classes=ncls)
    learner = FlickerVideoResNet(a.base_model, W, batch_size=a.batch, sample_length=clips.shape[1], image_size=S, dtype=a.dtype,
                                 l_inf_pert_norm=L_INF_PERT_NORM, cyclic_pert=CYCLIC_PERT, attack_type=a.attack_type, per_clip=a.batch > 1,
                                 optimizer=a.optimizer, im_scale=a.im_scale, resize_rule=a.resize_rule, quantise_train=a.quantise_train,
                                 **vs.flicker_keywords_from_arguments(a))
    dest = os.path.join(a.results_root, learner.model_name, "single_video_attack", a.attack_type,
                        f"linf_{L_INF_PERT_NORM}_lambda_{LAMBDA}_beta1_{BETA_1}_")
    crit = Losses(beta_1=BETA_1, lambda_=LAMBDA, targeted=TARGETED_ATTACK, improve_loss=IMPROVE_LOSS, logits=USE_LOGITS, attack_type=a.attack_type)
    if clips.dtype == np.uint8:          # resident: one upload, every video is a slice of it
        xd, yd = torch.from_numpy(clips).cuda(), torch.from_numpy(labels).cuda()
        videos = ((xd[i:i + 1], yd[i:i + 1], names[i]) for i in range(len(clips)))
    else:
        videos = ((torch.from_numpy(clips[i:i + 1]).cuda(), torch.from_numpy(labels[i:i + 1]).cuda(), names[i]) for i in range(len(clips)))
    out = learner.fit_many_videos(videos, crit, lr=LR, model_dir=dest, label_id_to_text=classes, n_iter=a.n_iter, restart_after=a.restart_after,
                                  reset_optimizer_per_video=a.reset_optimizer_per_video, **export_kw(a))
    report(out)


if __name__ == "__main__":
    main()
