"""Host-side mirror of the reference's torch attack surface (utils_cv/action_recognition/model.py:58-330) on top of
libflicker_hip.so: ``Perturbation``, ``Losses``, ``Adversarial_metrics`` and a VideoResNet attack engine
(``FlickerVideoResNet``, the hot loop of ``VideoLearnerAdversarial.fit_single_video_attack``, model.py:984-1205).

Same names, argument meaning and error behaviour as the reference classes; the arithmetic runs in the HIP kernels
(torch dialect flags), pinned by the reference's own golden vectors (tests/golden/torch_attack_golden.npz).
Clips are channels-last ``[B,T,H,W,3]`` on the device (the reference's NCDHW ``[B,3,T,H,W]`` permuted once at load)."""
import os
import random

import numpy as np
import torch

from . import ops, parallel
from ._lib import FLK_NET_MC3_18, FLK_NET_R2PLUS1D_18, FLK_NET_R2PLUS1D_34, FLK_NET_R3D_18
from .videoresnet_spec import (DEFAULT_MEAN, DEFAULT_STD, FLICKER_MODELS, RESIZE_RULES, CaptureChannel, Codec, check_codec_grad, check_sampling, flicker_rows, illum_tables,
                               resolve_model, sample_frame_indices, split_sampling, train_crop_params, u8_decode_table)

FLICKER_TIMES = ("clip", "video")


def check_flicker_time(flicker_time, flicker_period, sample_length, attack_type="flickering", per_clip=False, capture=None):
    """the period of the perturbation (its row count) for a ``flicker_time`` / ``flicker_period`` pair: ``sample_length`` on clip time; on
    video time ``flicker_period`` (None: ``sample_length``), 1..ops.FLICKER_MAX_PERIOD.  ``capture`` (a videoresnet_spec.CaptureChannel): on
    video time with one shared flickering perturbation only.  Host-only; anything else is a ValueError"""
    if flicker_time not in FLICKER_TIMES:
        raise ValueError(f"flicker_time must be one of {FLICKER_TIMES}, got {flicker_time!r}")
    if capture is not None:
        if not isinstance(capture, CaptureChannel):
            raise ValueError(f"capture must be a videoresnet_spec.CaptureChannel or None, got {type(capture).__name__}")
        if flicker_time != "video" or attack_type != "flickering" or per_clip:
            raise ValueError("capture needs flicker_time='video' and the flickering attack with one shared perturbation: the channel mixes the "
                             "rows a video's frames carry (clip time, dense and per-clip perturbations have none)")
    if flicker_time == "clip":
        if flicker_period is not None:
            raise ValueError("flicker_period needs flicker_time='video': on clip time the perturbation has one row per frame of the clip")
        return int(sample_length)
    if attack_type != "flickering" or per_clip:
        raise ValueError("flicker_time='video': the flickering attack with one shared perturbation only (a dense or per-clip perturbation "
                         "belongs to its clip, not to the video's frame numbers)")
    P = sample_length if flicker_period is None else flicker_period
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or not 1 <= P <= ops.FLICKER_MAX_PERIOD:
        raise ValueError(f"flicker_period must be an integer in 1..{ops.FLICKER_MAX_PERIOD} (3 * period values are what the update kernel holds), got {P!r}")
    return int(P)


ARCH_CODES = {"r2plus1d_18": FLK_NET_R2PLUS1D_18, "r3d_18": FLK_NET_R3D_18, "mc3_18": FLK_NET_MC3_18, "r2plus1d_34": FLK_NET_R2PLUS1D_34}
CLIP_DTYPES = (torch.float32, torch.uint8)
_DECODE_TABLES = {}
_INV_STD = tuple(1.0 / s for s in DEFAULT_STD)


def check_flicker_model(flicker_model, response="srgb", attack_type="flickering", dense=False):
    """the pixel model of the flicker: "additive" (the reference's: one offset per frame, in normalised display space) or "illumination"
    (the flicker lights the scene: multiplicative in linear light, through the camera curves ``videoresnet_spec.illum_tables(response)``).
    Returns the tables (None for "additive").  Host-only; anything else is a ValueError"""
    if flicker_model not in FLICKER_MODELS:
        raise ValueError(f"flicker_model must be one of {FLICKER_MODELS}, got {flicker_model!r}")
    if flicker_model == "additive":
        return None
    if attack_type != "flickering" or dense:
        raise ValueError("flicker_model='illumination': the flickering attack only (a lamp has one value per frame, or per line under a rolling shutter)")
    return illum_tables(response)


def decode_table(device):
    """the uint8 decode table (videoresnet_spec.u8_decode_table, fp32 [256,3]) on ``device``: one copy per device"""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _DECODE_TABLES:
        _DECODE_TABLES[key] = torch.from_numpy(u8_decode_table()).to(torch.device(dev.type, key[1]))
    return _DECODE_TABLES[key]


class Perturbation:
    """model.py:58-129.  size = [3,T,1,1] (flickering) or [3,T,H,W] (the dense "L12" attack, model.py:380-384); the parameter
    is stored time-major / channels-last on the device: [T,3] or [T,H,W,3].

    ``clip_length`` (flickering, one shared perturbation): the flicker runs on VIDEO time.  ``size`` is then [3,P,1,1], P the flicker's period
    (``self.T``, the row count of everything the optimiser sees), ``clip_length`` the frames of a clip (``self.clip_T``), and frame t of
    clip b carries row ``(frame_numbers[b,t] - phase) mod P`` (videoresnet_spec.flicker_rows; ``set_frame_numbers``, default ``arange``):
    every adversarial apply gathers its per-clip perturbation [B,clip_T,3] through that table (ops.flicker_rows_gather) and goes through
    the per-clip path of the kernels.  ``cyclic_pert`` then draws one phase per VIDEO (``clips_per_video`` consecutive clips) per
    adversarial forward -- a flicker not synchronised with the video's start; the phases last used are kept on ``last_phases``.

    ``capture`` (video time only; a videoresnet_spec.CaptureChannel): the distribution ``delta_clip(capture="draw")`` draws one capture
    channel per video from -- the per-clip perturbation is then the mix of rows a camera records (ops.flicker_rows_mix) instead of the
    gathered rows; the channels last used, with their tables, are kept on ``last_capture``.  A channel with a ``readout`` (a rolling
    shutter; a drawn or given dict then holds a ``"readout"``) gives every LINE of a frame its own mix: ``delta_clip`` returns
    ``[B,clip_T,H,3]`` (ops.flicker_lines_mix, tables from ``CaptureChannel.line_tables`` at the clips' height) and the apply / export
    arguments name it per line (flk_apply_args.delta_per_line)."""

    def __init__(self, size, requires_grad=True, device="cuda", max_value=None, min_value=None, max_norm=1.0, cyclic_pert=False, batch=None,
                 clip_length=None, clips_per_video=1, capture=None, flicker_model="additive", response="srgb"):
        if len(size) != 4 or size[0] != 3:
            raise ValueError(f"perturbation size must be [3,T,1,1] or [3,T,H,W], got {tuple(size)}")
        # flicker_model "illumination": the perturbation is a relative modulation of the scene's light (``max_norm`` its largest value),
        # applied, exported and differentiated by the flk_illum_* kernels through the camera tables of ``response``; uint8 clips only
        self.illum_tables = check_flicker_model(flicker_model, response, dense=not (size[2] == 1 and size[3] == 1))
        self.flicker_model, self.illumination, self._illum = flicker_model, flicker_model == "illumination", None
        self.size, self.device, self.requires_grad = tuple(size), device, requires_grad
        self.T = size[1]
        self.dense = not (size[2] == 1 and size[3] == 1)
        self.video_time = clip_length is not None
        self.clip_T = int(clip_length) if self.video_time else self.T          # frames of a clip (T rows on clip time, by definition)
        if self.video_time and (self.dense or batch is not None):
            raise ValueError("clip_length (flicker on video time): flickering perturbations shared by the batch only")
        if capture is not None and not (self.video_time and isinstance(capture, CaptureChannel)):
            raise ValueError("capture: a videoresnet_spec.CaptureChannel, with clip_length (flicker on video time) only")
        self.capture = capture
        self.last_capture = None         # the channels of the last adversarial apply that went through one: the draw + its "taps", "gain_rows"
        self.taps_dev = self.gain_dev = None                          # their tables on the device: fp32 [B,K] and [B,3]
        self.clips_per_video = int(clips_per_video)
        self.frame_numbers = None        # video time: int64 [B,clip_T] of the current batch, None = arange(clip_T) for every clip
        self.last_phases = None          # video time: the phases (one per video) of the last adversarial apply
        self.rows_host = self.rows_dev = self._delta_clip = None      # the rows table last uploaded, its device copy, the gathered perturbation
        self._delta_lines = None         # rolling shutter: the per-line perturbation [B,clip_T,H,3] (reused like _delta_clip)
        # batch = B (flickering only): B INDEPENDENT perturbations [B,T,3], one per clip of the batch, each with its own clamp bound
        # (``dyn_max_norm_dev`` [B]) -- single-video attacks advancing together (fit_many_videos, model.py:791-982)
        self.batch = batch
        if batch is not None and (self.dense or cyclic_pert):
            raise ValueError("batch: flickering perturbations without cyclic roll only")
        # model.py:72-75: attributes are only set when the argument is None -- reproduced
        if max_value is None:
            self.max_value = float(np.min((1 - np.array(DEFAULT_MEAN)) / DEFAULT_STD))
        if min_value is None:
            self.min_value = float(np.max((0.0 - np.array(DEFAULT_MEAN)) / DEFAULT_STD))
        self.max_norm = self.dynamic_max_norm = max_norm
        self.cyclic_pert = cyclic_pert
        self._rng = np.random.default_rng(0)
        self.perturbation = None
        if batch is not None:
            self.perturbation = torch.zeros((batch, self.T, 3), dtype=torch.float32, device="cuda")
            self.dyn_max_norm_dev = torch.full((batch,), float(max_norm), dtype=torch.float32, device="cuda")
            for b in range(batch):
                self.init_clip(b)
        else:
            self.init_perturbation()

    @property
    def _dev_shape(self):
        if self.batch is not None:
            return (self.batch, self.T, 3)
        return (self.T, self.size[2], self.size[3], 3) if self.dense else (self.T, 3)

    def init_clip(self, b, perturbation=(), max_norm=None):
        """batch mode: (re)start slot b -- ``init_perturbation`` for that clip alone, clamp bound back to ``max_norm`` (model.py:938-947)"""
        p = (self._rng.random(self.size, dtype=np.float32) * 2 - 1) * 1e-6 if len(perturbation) == 0 else perturbation
        p = np.asarray(p, dtype=np.float32).reshape(self.size)
        self.perturbation[b].copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(p, (1, 2, 3, 0)).reshape(self.T, 3))))
        self.dyn_max_norm_dev[b] = float(self.max_norm if max_norm is None else max_norm)

    def _to_dev(self, p_cthw):
        """[3,T,H,W] (reference layout) -> device layout"""
        p = np.asarray(p_cthw, dtype=np.float32).reshape(self.size)
        return np.ascontiguousarray(np.transpose(p, (1, 2, 3, 0)).reshape(self._dev_shape))

    def _to_ref(self, t):
        """device layout -> [3,T,H,W] like the reference tensors"""
        return t.reshape(self.T, self.size[2], self.size[3], 3).permute(3, 0, 1, 2)

    def init_perturbation(self, perturbation=(), requires_grad=True, device="cuda"):
        """model.py:121-126: U(-1,1)*1e-6 or the given numpy array [3,T,1,1] / [3,T,H,W] (batch mode: every slot gets it)"""
        if self.batch is not None:
            for b in range(self.batch):
                self.init_clip(b, perturbation, max_norm=float(self.dyn_max_norm_dev[b]))
            return
        if len(perturbation) == 0:
            p = (self._rng.random(self.size, dtype=np.float32) * 2 - 1) * 1e-6
        else:
            p = perturbation
        self.perturbation = torch.from_numpy(self._to_dev(p)).cuda()

    def set_frame_numbers(self, table):
        """video time: the frame numbers of the clips the next applies see -- integers ``[B,clip_T]`` (a table of
        videoresnet_spec.sample_frame_indices, stacked video-major and sample-minor), or None: ``arange(clip_T)`` for every clip"""
        if table is not None:
            table = np.asarray(table)
            if table.ndim != 2 or table.shape[1] != self.clip_T or table.dtype.kind not in "iu":
                raise ValueError(f"frame numbers must be an integer table [B,{self.clip_T}], got {table.shape} {table.dtype}")
            table = np.ascontiguousarray(table, dtype=np.int64)
        self.frame_numbers = table

    @staticmethod
    def _is_channel_dict(capture):
        return isinstance(capture, dict) and set(capture) - {"readout"} == {"subframe", "exposure", "gain"}

    def _capture_tables(self, B, capture, H=None):
        """the channel tables of a batch of B clips on the device (``taps_dev`` [B,K], ``gain_dev`` [B,3]), uploaded only when they differ
        from those already there.  ``capture``: "draw" -- one channel per video from ``self.capture`` -- or a dict ``subframe``,
        ``exposure``, ``gain`` holding one channel per video ([V], [V], [V,3]), one per clip ([B], ...) or one for all (scalars, ``gain`` [3]).
        A dict that also holds ``readout`` (a rolling shutter) gives per-line tables for frames of ``H`` lines, ``taps_dev`` [B,H,K]; returns
        whether it did."""
        G = self.clips_per_video
        V = -(-B // G)
        if isinstance(capture, str):
            if capture != "draw" or self.capture is None:
                raise ValueError(f"capture must be a channel dict, None or -- on a perturbation built with capture=CaptureChannel(...) -- 'draw', got {capture!r}")
            capture = self.capture.draw(V)
        if not self._is_channel_dict(capture):
            raise ValueError(f"capture must be a dict with the keys subframe, exposure and gain (and, for a rolling shutter, readout), got {capture!r}")
        lines = "readout" in capture
        if lines and (isinstance(H, bool) or not isinstance(H, (int, np.integer)) or H < 1):
            raise ValueError(f"capture with a readout: the height of the clips must be known, got {H!r}")
        if np.ndim(capture["subframe"]) == 0:                          # one channel for every video of the batch
            one = capture
            capture = {"subframe": np.full(V, float(one["subframe"])), "exposure": np.full(V, float(one["exposure"])),
                       "gain": np.broadcast_to(np.asarray(one["gain"], np.float32).reshape(-1, 3)[:1], (V, 3)).copy()}
            if lines:
                capture["readout"] = np.full(V, float(one["readout"]))
        if G > 1 and np.shape(capture["subframe"]) == (B,):              # one channel per CLIP (evaluate_videos packs clips, not videos)
            G, V = 1, B
        taps, gain = CaptureChannel.line_tables(capture, G, int(H)) if lines else CaptureChannel.tables(capture, G)
        if taps.shape[0] != V * G:
            raise ValueError(f"{taps.shape[0] // G} capture channels for {B} clips of {G} per video: one per video, or one for all")
        taps, gain = np.ascontiguousarray(taps[:B]), np.ascontiguousarray(gain[:B])
        last = self.last_capture
        if last is None or self.taps_dev is None or last["taps"].shape != taps.shape:
            self.taps_dev, self.gain_dev = (torch.from_numpy(t).to(self.perturbation.device) for t in (taps, gain))
        else:
            if not np.array_equal(taps, last["taps"]):
                self.taps_dev.copy_(torch.from_numpy(taps))
            if not np.array_equal(gain, last["gain_rows"]):
                self.gain_dev.copy_(torch.from_numpy(gain))
        self.last_capture = {**capture, "taps": taps, "gain_rows": gain}
        return lines

    def delta_clip(self, B, phases="draw", capture=None, H=None):
        """video time: the per-clip perturbation [B,clip_T,3] of the current frame numbers (a buffer reused from call to call, valid
        until the next one).  ``phases``: "draw" = one per video from the generator when ``cyclic_pert`` (else 0), or an integer / one
        integer per video; None: the buffer as it is, nothing gathered (a clean apply reads no perturbation).  The table goes to the
        device only when it differs from the one already there.  ``capture``: None -- the rows themselves (ops.flicker_rows_gather) --
        or the capture channels the frames are recorded through (``_capture_tables``: "draw" or a dict): ops.flicker_rows_mix -- or, for
        channels with a readout (a rolling shutter) and clips of ``H`` lines, ops.flicker_lines_mix: the result is then ``[B,clip_T,H,3]``."""
        if self.frame_numbers is not None and self.frame_numbers.shape[0] != B:
            raise ValueError(f"{B} clips, but the frame numbers set are for {self.frame_numbers.shape[0]} (set_frame_numbers)")
        if self._delta_clip is None or self._delta_clip.shape[0] != B:
            self._delta_clip = torch.zeros((B, self.clip_T, 3), dtype=torch.float32, device=self.perturbation.device)
        if phases is None:
            return self._delta_clip
        G = self.clips_per_video
        if isinstance(phases, str):
            if phases != "draw":
                raise ValueError(f"phases must be 'draw', an integer or one integer per video, got {phases!r}")
            phases = self._rng.integers(0, self.T, size=-(-B // G)) if self.cyclic_pert else 0
        ph = np.asarray(phases, dtype=np.int64)
        if ph.ndim:
            if ph.shape != (-(-B // G),):
                raise ValueError(f"{ph.shape} phases for {B} clips of {G} per video: one per video, or a scalar")
            ph = np.repeat(ph, G)[:B]
        self.last_phases = np.broadcast_to(np.asarray(phases, dtype=np.int64), (-(-B // G),)).copy()
        fn = self.frame_numbers if self.frame_numbers is not None else np.broadcast_to(np.arange(self.clip_T, dtype=np.int64), (B, self.clip_T))
        rows = flicker_rows(fn, self.T, ph)
        if self.rows_host is None or rows.shape != self.rows_host.shape:
            self.rows_dev = torch.from_numpy(rows).to(self.perturbation.device)
            self.rows_host = rows
        elif not np.array_equal(rows, self.rows_host):
            self.rows_dev.copy_(torch.from_numpy(rows))
            self.rows_host = rows
        if capture is None:
            return ops.flicker_rows_gather(self.perturbation, self.rows_dev, out=self._delta_clip)
        if not self._capture_tables(B, capture, H):
            return ops.flicker_rows_mix(self.perturbation, self.rows_dev, self.taps_dev, self.gain_dev, out=self._delta_clip)
        if self._delta_lines is None or tuple(self._delta_lines.shape) != (B, self.clip_T, int(H), 3):
            self._delta_lines = torch.zeros((B, self.clip_T, int(H), 3), dtype=torch.float32, device=self.perturbation.device)
        return ops.flicker_lines_mix(self.perturbation, self.rows_dev, self.taps_dev, self.gain_dev, out=self._delta_lines)

    def _no_capture_on_clip_time(self, capture):
        if capture is not None and not self.video_time:
            raise ValueError("capture: a perturbation on video time only (clip_length / flicker_time='video')")

    @property
    def illum(self):
        """the flk_illum_args of an illumination model (tables uploaded on first use)"""
        if self._illum is None:
            self._illum = ops.make_illum_args(self.illum_tables, self.perturbation.device)
        return self._illum

    def _check_illum_clip(self, x, adversarial):
        if self.illumination and adversarial and x.dtype != torch.uint8:
            raise ValueError(f"flicker_model='illumination' takes uint8 clips (the camera curves are tables over the stored bytes), got {x.dtype}")

    def apply_args(self, x, adversarial=True, fold_t=1, quantise=False, phases="draw", capture=None):
        """fold_t: 1 = the (h,w)-folded 16-channel tensor; 4 = the same as two bf16 numbers per value (the input of bf16 plans).
        x: the normalised fp32 clip, or its uint8 frames -- decoded on the device through ``decode_table`` (bitwise the fp32 clip
        ``videoresnet_spec.normalize_u8`` makes on the host).  quantise: every value goes through the 8-bit round trip of ``export_u8``
        inside the apply kernel (flk_apply_args.q_lut) -- the clip applied is the one the exported frames decode to, bit for bit"""
        delta, kw = self.perturbation, self._shared_args(x, adversarial, capture)
        if self.video_time:
            # the roll is in the rows; a clean apply reads no perturbation (adv_flag 0), so it gathers nothing and keeps the table
            delta, shift = self.delta_clip(int(x.shape[0]), phases if adversarial else None, capture, int(x.shape[2])), 0
        else:
            shift = int(self._rng.integers(0, self.T)) if (self.cyclic_pert and adversarial) else 0   # model.py:91-92
        return ops.make_apply_args(x, delta, shift_p=shift, fold_t=fold_t, quantise="torch" if quantise else None,
                                   q_lut=decode_table(x.device) if quantise else None,
                                   per_line=self.video_time and delta.dim() == 4, **kw)   # (video time has no dense delta: 4-D = per line)

    def _shared_args(self, x, adversarial, capture):
        """what ``apply_args`` and ``export_args`` have in common: the checks of the clip and the channel, and the keyword arguments that
        say how the perturbation meets the clip -- the dialect, the clamp bound(s) of the perturbation, the flag and the value range of
        an adversarial apply (a clean one has neither), 1 / std and the decode table of uint8 frames"""
        self._no_capture_on_clip_time(capture)
        self._check_illum_clip(x, adversarial)
        return dict(dialect="torch", dclip=self.dynamic_max_norm, adv_flag=1.0 if adversarial else 0.0, inv_std=_INV_STD,
                    lo=self.min_value if adversarial else -np.inf, hi=self.max_value if adversarial else np.inf,
                    dclip_dev=self.dyn_max_norm_dev if self.batch is not None else None,
                    x_lut=decode_table(x.device) if x.dtype == torch.uint8 else None)

    def export_args(self, x, adversarial=True, shift_p=0, delta_T=0, capture=None):
        """``apply_args`` for the 8-bit export (ops.make_export_apply_args): no fold, so T, H and W may be odd; no roll is drawn -- the
        frames of a cyclic perturbation are exported at the phase ``shift_p`` the caller names.  Video time: clips (``delta_T`` 0) take
        their rows at that phase (one per video, or a scalar) through the per-clip path; a whole video (``delta_T`` = the period) takes
        the shared perturbation itself -- the kernel's own rule IS the one the rows follow.  ``capture``: the channel(s) the flicker is
        recorded through -- clips: as ``delta_clip`` takes them; a whole video: ONE channel, the perturbation exported being its mix
        over ``rows = arange(P)`` (``captured_perturbation``; the mix commutes with the row shift)"""
        delta, kw = self.perturbation, self._shared_args(x, adversarial, capture)
        if self.video_time and not delta_T:
            delta, shift_p = self.delta_clip(int(x.shape[0]), shift_p if adversarial else None, capture, int(x.shape[2])), 0
        elif capture is not None and adversarial:
            delta = self.captured_perturbation(capture, int(x.shape[2]))
        return ops.make_export_apply_args(x, delta, shift_p=shift_p, delta_T=delta_T,
                                          per_line=self.video_time and delta.dim() - (0 if delta_T else 1) == 3, **kw)

    def export_args_like_last(self, x, frame_numbers, of, captured):
        """video time: the export arguments of FURTHER clips ``x`` [n,clip_T,h,w,3] at ``frame_numbers`` (integers [n,clip_T]) under the
        phase and -- ``captured`` -- the capture channel that the last adversarial apply gave clip ``of[i]`` of its batch: frame for
        frame the perturbation that apply would have given those frame numbers.  Nothing the last apply left behind (its rows, its
        tables, its per-clip perturbation, which its gradient still reads) is touched."""
        dev, of = self.perturbation.device, np.asarray(of, dtype=np.int64)
        ph = np.repeat(self.last_phases, self.clips_per_video)[of]
        rows = torch.from_numpy(flicker_rows(np.asarray(frame_numbers), self.T, ph)).to(dev)
        if captured:
            taps, gain = (torch.from_numpy(np.ascontiguousarray(self.last_capture[key][of])).to(dev) for key in ("taps", "gain_rows"))
            delta = ops.flicker_rows_mix(self.perturbation, rows, taps, gain)
        else:
            delta = ops.flicker_rows_gather(self.perturbation, rows)
        return ops.make_export_apply_args(x, delta, shift_p=0, delta_T=0, per_line=False, **self._shared_args(x, True, None))

    def captured_perturbation(self, capture, H=None):
        """video time: the shared perturbation as ONE capture channel records it, fp32 [P,3] -- one ops.flicker_rows_mix launch over
        ``rows = arange(P)`` as one clip of P frames: row r of the result is what a frame that carries row r records.  ``capture``: a dict
        ``subframe``, ``exposure`` (scalars) and ``gain`` [3].  Nothing of the batch's own tables is touched.  A channel that also holds a
        scalar ``readout`` (a rolling shutter) is recorded per line of a frame of ``H`` lines: fp32 [P,H,3], ops.flicker_lines_mix."""
        if not self._is_channel_dict(capture) or np.ndim(capture["subframe"]) != 0:
            raise ValueError(f"capture must be ONE channel: a dict of the scalars subframe and exposure and gain [3], got {capture!r}")
        dev = self.perturbation.device
        rows = torch.arange(self.T, dtype=torch.int32, device=dev)
        if "readout" in capture:
            taps, gain = CaptureChannel.line_tables(capture, 1, H)
            return ops.flicker_lines_mix(self.perturbation, rows, torch.from_numpy(taps).to(dev), torch.from_numpy(gain).to(dev))
        taps, gain = CaptureChannel.tables(capture, 1)
        return ops.flicker_rows_mix(self.perturbation, rows, torch.from_numpy(taps).to(dev), torch.from_numpy(gain).to(dev))

    def _channels_last(self, x):
        """a clip as ``forward`` and ``export_u8`` take it -- NCDHW or channels-last, fp32 or uint8, anywhere -- as the contiguous
        channels-last CUDA tensor the kernels read (uint8 stays uint8, anything else becomes fp32) -> ``(clip, whether x was NCDHW)``"""
        ncdhw = x.dim() == 5 and x.shape[1] == 3 and x.shape[-1] != 3
        xcl = (x.permute(0, 2, 3, 4, 1) if ncdhw else x).contiguous()
        xcl = xcl.cuda() if xcl.dtype == torch.uint8 else xcl.float().cuda()
        if xcl.shape[1] != self.clip_T:
            raise ValueError(f"clip has {xcl.shape[1]} frames, the perturbation {self.clip_T}")
        return xcl, ncdhw

    def export_u8(self, x, adversarial=True, stats=False, out=None, out_offset=0, shift_p=0, capture=None):
        """the clip ``forward([x, adversarial])`` makes, as the 8-bit frames a file or a display holds: uint8 ``[B,T,H,W,3]`` on the device,
        ``rint(255 * (x_adv * std + mean))`` saturated to 0..255 (ops.export_adversarial_u8, one kernel launch; the host route
        ``apply_perturbation`` goes through the folded fp32 tensor, a permute and numpy).  ``x`` as in ``forward`` (NCDHW or channels-last,
        fp32 or uint8; any T, H, W -- odd ones too).  ``adversarial=False``: the frames of the clean clip, i.e. a uint8 ``x`` itself.
        ``stats``: also int32 ``[B,T,3,4]``, per (clip, frame, channel) the sums of q - q_clean, |q - q_clean|, [q != q_clean] and
        [clamp active]; entry 0 / (H * W) is the flicker the frames really carry, in levels."""
        a = self.export_args(self._channels_last(x)[0], bool(adversarial), shift_p, capture=capture)
        if self.illumination and adversarial:           # the bytes a camera stores of the lit scene (clean frames: the existing call)
            return ops.illum_export_u8(a, self.illum, out=out, out_offset=out_offset, stats=stats)
        return ops.export_adversarial_u8(a, "torch", out=out, out_offset=out_offset, stats=stats)

    def forward(self, input, quantise=False):
        """model.py:80-101: ``input = [x, adversarial]`` -> the perturbed (or, with adversarial False, the untouched) clip; ``quantise``:
        the normalised clip its 8-bit frames (``export_u8``) decode to -- what a stored video delivers.  ``x`` is the
        reference's NCDHW tensor [B,3,T,H,W] or the channels-last [B,T,H,W,3] the engine works on; the result has x's layout.  The
        kernel writes the (h,w)-folded tensor the network consumes (flk_perturb_apply_s2d); it is unfolded here.  A uint8 ``x`` holds
        the frames themselves: they are normalised on the device (dataset.py:28-29), the result is the fp32 clip of the normalised input."""
        x, adversarial = input
        xcl, ncdhw = self._channels_last(x)
        B, T, H, W, _ = xcl.shape
        a = self.apply_args(xcl, bool(adversarial), quantise=bool(quantise))
        if self.illumination and adversarial:
            folded = ops.illum_apply_s2d(a, self.illum, torch.float32)
        else:
            folded = ops.perturb_apply_s2d(a, torch.float32)      # [B,T,H/2,W/2,16]
        out = folded[..., :12].reshape(B, T, H // 2, W // 2, 2, 2, 3).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, T, H, W, 3)
        return out.permute(0, 4, 1, 2, 3).contiguous() if ncdhw else out.contiguous()

    __call__ = forward

    @staticmethod
    def convert_adversarial_video_zero_one(adv_vid):
        """model.py:107-112: the normalised clip back to pixel range, as a NUMPY array ``[B,T,H,W,3]`` in [0,1]:
        ``(x^T + mean/std) * std`` (float64, like the reference's numpy arithmetic).  ``adv_vid`` is the reference's NCDHW
        tensor [B,3,T,H,W] or the engine's channels-last [B,T,H,W,3]."""
        x = adv_vid.detach().cpu().numpy()
        if x.ndim == 5 and x.shape[1] == 3 and x.shape[-1] != 3:
            x = x.transpose([0, 2, 3, 4, 1])
        return (x + np.array(DEFAULT_MEAN) / np.array(DEFAULT_STD)) * np.array(DEFAULT_STD)

    def apply_perturbation(self, x):
        """model.py:103-105: the perturbed clip de-normalised to [0,1], numpy [B,T,H,W,3] (what the scripts save / plot)"""
        return self.convert_adversarial_video_zero_one(self.forward([x, True]))

    def clamp_perturbation(self):
        if self.batch is not None:
            bound = self.dyn_max_norm_dev.view(-1, 1, 1)
            return torch.minimum(torch.maximum(self.perturbation, -bound), bound)
        return self.perturbation.clamp(-self.dynamic_max_norm, self.dynamic_max_norm)

    def clip_perturbation_ref(self, b):
        """batch mode: (clamped) perturbation of slot b in the reference layout [3,T,1,1]"""
        return self.clamp_perturbation()[b].t().reshape(3, self.T, 1, 1)

    def get_perturbation(self):
        """(clamped, raw) as [3,T,1,1] / [3,T,H,W] like the reference (model.py:128-129)"""
        return self._to_ref(self.clamp_perturbation()), self._to_ref(self.perturbation)

    def metric_calc(self):
        """model.py:113-118 on the raw parameter: roll over the time axis"""
        p = self.perturbation
        return p.abs().mean() * 100.0, (torch.roll(p, 1, 0) - p).abs().mean() * 100.0


class Losses:
    """model.py:131-250: __call__(labels, logits, prob, perturbation) -> [loss, adv, reg]; here the adversarial part and
    d(adv)/d(logits) come from flk_softmax_adv_loss (torch dialect), the regulariser from flk_perturb_reg_adam."""

    def __init__(self, beta_1=0.5, lambda_=1.0, targeted=False, target_class=None, margin=0.05, improve_loss=False, logits=False,
                 attack_type="flickering"):
        if attack_type not in ("flickering", "L12"):
            raise ValueError(f"attack_type must be 'flickering' or 'L12' (model.py:165-168), got {attack_type!r}")
        if targeted and improve_loss:
            # model.py:223-225 references undefined names: the reference crashes here; refuse instead of guessing
            raise NotImplementedError("the reference's targeted improve-loss is non-functional (model.py:223-225)")
        self.beta_1, self.lambda_, self.targeted, self.target_class = beta_1, lambda_, targeted, target_class
        self.margin, self.improve_loss, self.logits, self.attack_type = margin, improve_loss, logits, attack_type
        self.label_prob = None

    def __call__(self, labels, model_logits, prob, perturbation):
        """model.py:169-175: ``[loss, adv_loss, reg_loss]`` (values; the engine's step takes the gradients from the kernels).
        ``prob`` is accepted for signature parity -- the kernel recomputes the softmax; ``perturbation`` is the clamped delta in the
        reference layout [3,T,1,1] / [3,T,H,W] (model.py:1078).  Sets ``label_prob`` like the reference (:232)."""
        _, _, pc = self.adv(labels, model_logits.contiguous().float(), model_logits.shape[0])
        adv_loss = pc[:, 0].sum()
        reg_loss = self.regularization_loss(perturbation)
        return [adv_loss + self.lambda_ * reg_loss, adv_loss, reg_loss]

    def adv(self, labels, model_logits, global_batch, out=None):
        lab = labels if not self.targeted else torch.full_like(labels, self.target_class)
        sm, dl, pc = ops.softmax_adv_loss(model_logits, lab, dialect="torch", improve_loss=self.improve_loss, use_logits=self.logits,
                                          targeted=self.targeted, margin=self.margin, mean_scale=1.0 / global_batch, out=out)
        self.label_prob = pc[:, 1]
        return sm, dl, pc

    def adv_video(self, labels, model_logits, global_videos, clips_per_video, reduce="mean", out=None):
        """``adv`` on the videos' aggregated logits (the decision rule of evaluate(num_samples), model.py:1227-1317): ``model_logits``
        [V*G, classes] video-major and clip-minor, ``labels`` [V] -> (softmax [V,C], dlogits [V*G,C], per_video [V,4], video_logits [V,C])"""
        lab = labels if not self.targeted else torch.full_like(labels, self.target_class)
        sm, dl, pv, vl = ops.softmax_adv_loss_video(model_logits, lab, clips_per_video, reduce=reduce, dialect="torch",
                                                    improve_loss=self.improve_loss, use_logits=self.logits, targeted=self.targeted,
                                                    margin=self.margin, mean_scale=1.0 / global_videos, out=out)
        self.label_prob = pv[:, 1]
        return sm, dl, pv, vl

    def flickering_regularization_loss(self, perturbation):
        """model.py:198-209 on the CLAMPED perturbation [3,T,1,1] (model.py:1078): value only -- the gradient and the same
        value during an update come from flk_perturb_reg_adam.  Used for evaluation passes (no Adam step)."""
        p = perturbation
        right, left = torch.roll(p, 1, dims=1), torch.roll(p, -1, dims=1)
        norm_reg = torch.mean(p ** 2) + 1e-12
        diff_norm_reg = torch.mean((p - right) ** 2) + 1e-12
        laplacian_norm_reg = torch.mean((-2 * p + right + left) ** 2) + 1e-12
        return self.beta_1 * norm_reg + (1 - self.beta_1) * (diff_norm_reg + laplacian_norm_reg)

    def L12_regularization_loss(self, perturbation):
        """model.py:211-214 on the clamped perturbation [3,T,H,W]: value only (update passes take it from flk_perturb_dense_l12_adam)"""
        return torch.sum(torch.sqrt(torch.mean(perturbation ** 2, [0, 2, 3]))) + 1e-12

    def regularization_loss(self, perturbation):
        return self.L12_regularization_loss(perturbation) if self.attack_type == "L12" else self.flickering_regularization_loss(perturbation)


class Adversarial_metrics:
    """model.py:253-330"""

    def __init__(self, targeted=False, target_class=None):
        self.targeted, self.target_class = targeted, target_class

    def accuracy(self, output, ground_truth, topk=(1,), clean_pred=None):
        """model.py:262-291: fooling percentages as a list of 1-element tensors.  Targeted: ONE entry, 100 * #(top-maxk predictions
        equal to the target class) / batch.  Untargeted: per k, 100 * (1 - #(adv top-k hit AND clean top-k hit, at the SAME rank
        position) / #(clean top-k hits)) -- the rank-wise product is the reference's (model.py:287), reproduced as is."""
        with torch.no_grad():
            res = []
            batch_size = ground_truth.size(0)
            maxk = max(topk)
            pred = output.topk(maxk, 1, True, True)[1].t()
            if self.targeted:
                correct = pred.eq(self.target_class).reshape(-1).float().sum(0, keepdim=True)
                res.append(correct[0] * (100.0 / batch_size))
                return res
            correct = pred.eq(ground_truth.view(1, -1).expand_as(pred))
            pred_no_adv = clean_pred.topk(maxk, 1, True, True)[1].t()
            correct_no_adv = pred_no_adv.eq(ground_truth.view(1, -1).expand_as(pred_no_adv))
            for k in topk:
                correct_k = (correct[:k] * correct_no_adv[:k]).reshape(-1).float().sum(0, keepdim=True)
                res.append((1 - correct_k * (1.0 / correct_no_adv[:k].reshape(-1).float().sum())) * 100.0)
            return res

    def accuracy_for_eval(self, output, ground_truth, topk=(1,), clean_pred=None):
        adv, clean = output.argmax(1), clean_pred.argmax(1)
        correct_clean = clean == ground_truth
        if self.targeted:
            return (adv == self.target_class).float().sum() * (100.0 / ground_truth.numel())
        return ((adv != ground_truth) & correct_clean).float().sum(), correct_clean.float().sum()

    def adversarial_metric(self, perturbation):
        return perturbation.abs().mean() * 100.0, (torch.roll(perturbation, 1, dims=1) - perturbation).abs().mean() * 100.0


class FlickerVideoResNet:
    """Attack engine for torchvision-0.5.0 r2plus1d_18 / r3d_18 / mc3_18 and R(2+1)D-34 (model.py:337-399,418-441,984-1205).

    ``base_model``: an architecture of ARCH_CODES, ``"ig65m"`` / ``"kinetics"`` (R(2+1)D-34 at sample_length 8 or 32, model.py:341,373) or a
    model name of videoresnet_spec.MODELS (videoresnet_spec.resolve_model).  The class count is the weights' ``fc`` head; ``num_classes``,
    when given, must agree with it (a fine-tuned victim brings its own ``fc``, model.py:436-437)."""

    def __init__(self, base_model, weights, batch_size=1, sample_length=16, image_size=112, dtype="bf16", device=0, l_inf_pert_norm=0.2,
                 cyclic_pert=False, num_classes=None, process_group=None, attack_type="flickering", per_clip=False, optimizer="adam",
                 im_scale=128, resize_rule="sizes", augment=None, sampling=None, clips_per_video=1, video_reduce="mean", quantise_train=False,
                 flicker_time="clip", flicker_period=None, capture=None, flicker_model="additive", response="srgb", train_delivered=False, codec=None,
                 codec_grad="identity"):
        from .i3d_engine import check_optimizer
        # flicker_model "illumination": the flicker LIGHTS THE SCENE instead of being added to the displayed pixels -- a pixel of linear
        # light L becomes L * (1 + m), then goes through the camera's response and 8 bits (videoresnet_spec.illum_tables(response); the
        # flk_illum_* kernels).  ``l_inf_pert_norm`` is then the largest relative modulation.  Flickering attack, uint8 clips only; the
        # rows / capture / rolling-shutter seams, the optimisers, ``quantise_train`` and the video loss compose with it unchanged.
        # "additive" (default): the reference's model, every launch as before.  Checked before anything touches the device
        check_flicker_model(flicker_model, response, attack_type)
        self.flicker_model, self.illumination = flicker_model, flicker_model == "illumination"
        # flicker_time "video": the flicker runs on VIDEO time, as ``export_video`` delivers it -- a perturbation of period P =
        # ``flicker_period`` (default: sample_length) rows, frame t of clip b carrying row (frame number - phase) mod P, the frame numbers
        # being those the clips were cut at (``prepare_videos`` / whole-video loaders: ``last_sampling``; pre-cut clips:
        # ``set_frame_numbers``; nothing set: 0..T-1).  "clip" (default): row t for frame t of every clip, as ever.  Checked before
        # anything touches the device
        self.P = check_flicker_time(flicker_time, flicker_period, sample_length, attack_type, per_clip, capture)
        self.flicker_time, self.video_time = flicker_time, flicker_time == "video"
        # train_delivered: the attack is trained on the DELIVERED video at its native resolution (``step_videos``; whole-video loaders and
        # ``fit_single_video_attack`` on a whole video route through it).  The flicker is laid over the raw frames in 8 bits as
        # ``export_video`` lays it (per frame a byte -> byte tone table, ops.flicker_tone_tables), the stored bytes are resized and cropped
        # (ops.prepare_clips(tone=)) and scored clean -- the chain ``evaluate_videos(quantise="video")`` scores, bit for bit -- and the
        # gradient goes back through the resampling (ops.prepare_clips_grad).  ``quantise_train`` is implied.  A per-line flicker (a
        # capture channel with a readout) is not a per-frame byte map; dense and per-clip perturbations belong to their clips
        self.train_delivered = bool(train_delivered)
        if self.train_delivered:
            if not self.video_time or attack_type != "flickering" or per_clip:
                raise ValueError("train_delivered needs flicker_time='video' and the flickering attack with one shared perturbation (not per_clip, "
                                 "not L12): the delivered video carries the flicker on its own frame numbers")
            if capture is not None and capture.readout is not None:
                raise ValueError("train_delivered: a capture channel with a readout (rolling shutter) gives every line of a frame its own "
                                 "flicker, which is not a per-frame byte map")
        # codec (a videoresnet_spec.Codec; train_delivered only): the delivered video is COMPRESSED before the victim sees it.  The training
        # forward lays the flicker over the batch's frames and compresses them in one launch (ops.codec_roundtrip(frame_idx=, tone=)) into
        # reused uint8 buffers, prepares those and scores them clean -- the chain ``evaluate_videos(quantise="video", codec=)`` scores, bit
        # for bit.  The backward is the train_delivered one on the source videos: straight through the codec, whose Jacobian is taken as
        # the identity.  A codec with ``gop`` > 1 compresses per clip the span from the intra frame at
        # or before the clip's first frame (ops.codec_roundtrip(spans=, tone=)); the surrogate rec ~ cur holds for a P-frame as for an
        # intra frame, so the backward is the same.  A codec with ``search`` > 0 goes through the same calls: its GOPs
        # are still closed in time, so the spans stand, and the surrogate is unchanged (motion moves the prediction, not what the
        # reconstruction approximates).  None (default): every launch as before
        if self._check_codec(codec) is not None and not self.train_delivered:
            raise ValueError("codec: an engine built with train_delivered=True only (the codec compresses whole delivered frames; "
                             "evaluate_videos(quantise='video', codec=) and export_video(codec=) take one on any engine)")
        self.codec = codec
        # codec_grad: the codec's Jacobian in that backward.  "identity" (default): straight through, every launch as before.  "ste" /
        # "cubic" (an intra-frame codec only): the input gradient goes back through the resampling to the decoded
        # frames (ops.prepare_clips_grad_image) and through the codec's own transpose -- colour transforms, chroma subsampling, clamps,
        # the transform pair, the quantiser straight through or by the cubic rounding surrogate -- to the tone slopes (ops.codec_grad).
        # The forward is the same integer codec under all three
        if codec_grad != "identity":
            check_codec_grad(codec_grad, "codec_grad")
            if codec is None:
                raise ValueError(f"codec_grad={codec_grad!r} differentiates a codec: give codec=Codec(...) (and train_delivered=True)")
            if codec.gop > 1 or codec.search > 0:
                raise ValueError(f"codec_grad={codec_grad!r} differentiates the intra codec (gop 1, search 0); {codec!r} keeps "
                                 "codec_grad='identity'")
        self.codec_grad = codec_grad
        # capture (flicker_time "video"; a videoresnet_spec.CaptureChannel): the attack is trained OVER THE AIR.  Every adversarial training
        # forward (``step``) draws one capture channel per video -- sub-frame phase, exposure, colour gain -- and perturbs frame t by the mix
        # of rows a camera records (ops.flicker_rows_mix in the gather's place); the step folds its gradient through the same tables
        # (ops.flicker_rows_mix_grad).  Evaluation and export (``logits``, ``adversarial_frames``, ``quantised_logits``, ``export_video``,
        # ``evaluate_videos``) go through a channel only when they are given one: their default is none.  A channel with a ``readout`` is a
        # rolling shutter: every LINE of a frame gets its own mix (ops.flicker_lines_mix, the per-line apply and gradient,
        # ops.flicker_lines_mix_grad back to the same [P,3] payload); everything else is as for a channel without one
        self.capture = capture
        # quantise_train: the attack is optimised on the STORED video.  Every adversarial forward (``step`` in all its variants,
        # ``logits(x, True)``) applies decode(encode_u8(x_adv)) -- the 8-bit round trip inside the apply kernel, straight-through gradient --
        # so its logits are bit for bit ``quantised_logits(x)`` for the delta the step ran with, and the ``argmax`` / ``is_adversarial``
        # that ``step``, ``fit_single_video_attack``, ``fit_many_videos`` and ``train_an_epoch`` act on is the stored video's verdict: a
        # quantised stopping rule at no extra forward pass.  Clean forwards are not quantised (a uint8 clip is its own round trip).
        # (With cyclic_pert the step draws a roll; ``quantised_logits`` exports at phase 0 -- the identity is per roll.)
        self.quantise_train = bool(quantise_train)
        # clips_per_video = G > 1: the batch holds V = B / G videos of G clips each (video-major, sample-minor, as ``prepare_videos`` cuts
        # them) and the adversarial loss is taken on every video's aggregated logits -- video_reduce "sum" (what ``evaluate_videos``
        # decides on) or "mean" (the sum / G: same argmax, margin and CE on the scale of one clip's logits) -- with one label per video
        G = int(clips_per_video)
        self.video_scale = ops.video_scale(G, video_reduce)
        if int(batch_size) % G:
            raise ValueError(f"batch_size {batch_size} is not a multiple of clips_per_video {G}")
        if per_clip and G > 1:
            raise ValueError("per_clip (independent perturbations per clip) and clips_per_video > 1 (one loss per video) contradict each other")
        self.clips_per_video, self.video_reduce, self.V = G, video_reduce, int(batch_size) // G
        # raw-size uint8 frames are prepared on the device (``prepare``): ResizeVideo(im_scale) -> CenterCropVideo(image_size), dataset.py:84-123;
        # resize_rule: "sizes" = the arithmetic of torch 1.4.0 (the reference's pin), "scale_factor" = current torch (videoresnet_spec.prepare_geometry)
        if resize_rule not in RESIZE_RULES:
            raise ValueError(f"resize_rule must be one of {RESIZE_RULES}, got {resize_rule!r}")
        self.im_scale, self.resize_rule = im_scale, resize_rule
        # augment: the reference's training transform for raw frames (dataset.py:105-118; ``prepare(..., train=True)``, train_an_epoch's
        # "train" phase): {"scales": (0.6, 1.0) | None (RandomCropVideo), "ratio": (3/4, 4/3), "flip_ratio": 0.5, "seed": 0}; the engine owns
        # ONE generator, random.Random(seed + rank), drawn from in clip order
        self.augment = self._check_augment(augment)
        self.last_augment = None
        self._aug_rng = None if self.augment is None else random.Random(self.augment["seed"] + parallel.rank(process_group))
        # sampling: how clips are cut from whole videos (``prepare_videos``, ``evaluate_videos``, loaders that yield lists of videos) -- the
        # reference's VideoDataset settings (dataset.py:254-259, 500-586): {"sample_step": 1, "temporal_jitter": False, "temporal_jitter_step": 2,
        # "random_shift": False, "seed": 0}, the defaults being its scripts' (r2plus1d_main_universal_attack.py:155-163).  The temporal draws
        # come from a generator of their own, numpy.random.RandomState(seed + rank), as in the reference (numpy.random for the frames,
        # random for the crop boxes)
        self.sampling = check_sampling(sampling)
        self.last_sampling = None
        self._samp_rng = np.random.RandomState(self.sampling["seed"] + parallel.rank(process_group))
        # "pgd": delta <- clamp(delta - lr * sgn(g), +-dynamic_max_norm) instead of torch Adam (model.py:868) -- the radius is the clamp
        # bound the perturbation already has, so the restart schedule (model.py:1061-1066) widens it; no optimiser state
        self.optimizer = check_optimizer(optimizer)
        self.pgd = optimizer == "pgd"
        if base_model in ARCH_CODES:
            arch, name = base_model, base_model
        else:
            try:
                arch, name, _ = resolve_model(base_model, sample_length)
            except ValueError as e:
                raise ValueError(f"base_model must be one of {sorted(ARCH_CODES)}, 'ig65m' / 'kinetics' or an r2plus1d_34_* model name "
                                 f"(model.py:47-56): {e}") from None
        if not torch.cuda.is_available():
            raise RuntimeError("FlickerVideoResNet needs an MI355X (HIP) device; there is no CPU fallback")
        torch.cuda.set_device(device)
        self.arch = arch
        self.model_name, self.B, self.T, self.H, self.W, self.dtype = name, batch_size, sample_length, image_size, image_size, dtype
        self.pg, self.world = process_group, parallel.world_size(process_group)
        self.net = ops.Net(ARCH_CODES[arch], dtype, self.B, self.T, self.H, self.W, weights, device)
        if num_classes is not None and int(num_classes) != self.net.num_classes:
            raise ValueError(f"num_classes {num_classes} disagrees with the weights' fc head ({self.net.num_classes} classes)")
        self.num_classes = self.net.num_classes
        if attack_type not in ("flickering", "L12"):
            raise ValueError(f"attack_type must be 'flickering' or 'L12', got {attack_type!r}")
        self.attack_type = attack_type
        # model.py:380-384: [3,T,1,1] for the flickering attack, a dense [3,T,H,W] perturbation otherwise
        # per_clip: batch_size INDEPENDENT single-video attacks in one batch (fit_many_videos(batch=...)): a perturbation, Adam state,
        # step counter, clamp bound and "still attacking" flag per clip; replicas only (no collective)
        self.per_clip = bool(per_clip)
        if self.per_clip and (attack_type != "flickering" or cyclic_pert or self.world > 1):
            raise ValueError("per_clip: flickering attack, no cyclic roll, one rank")
        self.pert_model = Perturbation((3, self.P, 1, 1) if attack_type == "flickering" else (3, self.T, self.H, self.W),
                                       max_norm=l_inf_pert_norm, cyclic_pert=cyclic_pert, batch=self.B if self.per_clip else None,
                                       clip_length=self.T if self.video_time else None, clips_per_video=G, capture=capture,
                                       flicker_model=flicker_model, response=response)
        dev = torch.device("cuda", device)
        tdt = torch.bfloat16 if dtype in ("bf16", torch.bfloat16) else torch.float32
        # bf16 plans take the clip as TWO bf16 numbers per value (32 channels, fold_t = 4: the stem sees x + delta/std to ~16 bits -- one
        # bf16 per value swallowed |delta| = 1e-4 outright; the reference STARTS at U(+-1e-6), model.py:71); gradients: 16 channels
        self._xs = torch.empty((self.B, self.T, self.H // 2, self.W // 2, self.net.input_channels), dtype=tdt, device=dev)
        self._gx = torch.empty((self.B, self.T, self.H // 2, self.W // 2, 16), dtype=tdt, device=dev)
        self._logits = torch.empty((self.B, self.num_classes), dtype=torch.float32, device=dev)
        self._red = torch.zeros(parallel.payload_size(self.P), dtype=torch.float32, device=dev)
        # video time: the per-clip gradient [B,T,3] the rows fold back to [P,3] (reused every step, like the rows and the gathered delta)
        self._g_clip = torch.zeros((self.B, self.T, 3), dtype=torch.float32, device=dev) if self.video_time else None
        self._scratch = torch.empty(max(1, ops.load().flk_perturb_grad_scratch_bytes(self.B, self.T, self.H, self.W) // 4), dtype=torch.float32, device=dev)
        self._scalars = torch.empty(8, dtype=torch.float32, device=dev)
        self.adam_m = None if self.pgd else torch.zeros(self.pert_model._dev_shape, device=dev)
        self.adam_v = None if self.pgd else torch.zeros(self.pert_model._dev_shape, device=dev)
        self.adam_t = 0      # the reference keeps ONE Adam instance across videos: not reset by init_perturbation
        if self.per_clip:
            self.adam_steps = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.active = torch.ones(self.B, dtype=torch.int32, device=dev)

    def _forward(self, x, adversarial, phases="draw", capture=None):
        """Perturbation -> network: the apply arguments of this call (the backward pass masks with the same) ; logits in self._logits"""
        a = self.pert_model.apply_args(self._check_x(x), adversarial, fold_t=self.net.input_fold, quantise=self.quantise_train and bool(adversarial),
                                       phases=phases, capture=capture)
        if self.illumination and adversarial:                       # the illumination apply in front of the plan, then the plain forward
            ops.illum_apply_s2d(a, self.pert_model.illum, self._xs.dtype, out=self._xs)
            self.net.forward(self._xs, self._logits)
        else:
            self.net.forward_apply(a, self._xs, self._logits)       # the plan applies the perturbation in front of its stem
        return a

    def _grad_reduce(self, a, out):
        """d(loss)/d(delta) of the apply ``a`` from the input gradient of the last backward, under the engine's pixel model"""
        if self.illumination:
            return ops.illum_grad_reduce(a, self.pert_model.illum, self._gx, out, self._scratch)
        return ops.perturb_grad_reduce(a, self._gx, out, self._scratch)

    def _payload_grad(self, a, cap, delivered, out):
        """``step``'s route from the input gradient of the last backward to ``out``, the ``[P,3]`` gradient of the shared perturbation.
        ``a``: the apply arguments of the step's forward; ``cap``: whether it went through a capture channel; ``delivered``: the drawn
        clips of ``step_videos``, or None"""
        pm = self.pert_model
        if not self.video_time:                                 # clip time: frame t carries row t, the reduce writes the rows themselves
            return self._grad_reduce(a, out)
        if delivered is None and a.delta_per_line:
            # rolling shutter: the per-line gradient [B,T,H,3] (summed over w only; adv_flag, 1/std and the clamp mask applied per line),
            # then the transpose of the lines mix the forward ran, on the same tables, to the same [P,3] payload
            g_lines = self._buf("_g_lines", (self.B, self.T, self.H, 3))
            scratch = self._buf("_lines_scratch", (self.B * self.T * ops.FLICKER_LINES_MAX_TAPS * 3,))
            self._grad_reduce(a, g_lines)
            return ops.flicker_lines_mix_grad(g_lines, pm.rows_dev, self.P, pm.taps_dev, pm.gain_dev, out=out, scratch=scratch)
        if delivered is None:
            # per-clip gradient [B,T,3] (adv_flag, 1/std and the delta-clamp mask applied per frame)
            self._grad_reduce(a, self._g_clip)
        else:
            # the delivered video: the slopes of this step's tone tables, resampled as the clips were, give the per-clip gradient
            # [B,T,3] with its finishing factors
            clips, rows, boxes, flips = delivered
            slope, scale = self._buf("_slope", (self.B, self.T, 256, 3)), self._buf("_scale", (self.B, self.T, 3))
            ops.flicker_tone_slopes(a, pm.illum if self.illumination else None, slope, scale)
            if self.codec_grad != "identity":
                # through the codec: the gradient images of the decoded frames (the clips were prepared from the codec's output under
                # the identity frame table), packed one after the other in one reused buffer, then the codec's transpose on the source
                # frames under this step's tone tables
                shapes = [(self.T, int(v.shape[1]), int(v.shape[2]), 3) for v in clips]
                ends = np.cumsum([int(np.prod(s)) for s in shapes])
                flat = self._buf("_g_img", (int(ends[-1]),))
                images = [flat[e - int(np.prod(s)):e].view(*s) for s, e in zip(shapes, ends)]
                ops.prepare_clips_grad_image(list(clips), self._gx, im_scale=self.im_scale, input_size=(self.H, self.W), rule=self.resize_rule,
                                             boxes=boxes, flips=flips, frame_idx=np.broadcast_to(np.arange(self.T), (len(clips), self.T)), out=images)
                ops.codec_grad(list(clips), self.codec, flat, slope, scale, self.codec_grad, frame_idx=rows, tone=self._tone[:self.B],
                               gdelta=self._g_clip)
            else:
                ops.prepare_clips_grad(clips, self._gx, slope, scale, im_scale=self.im_scale, input_size=(self.H, self.W), rule=self.resize_rule,
                                       boxes=boxes, flips=flips, frame_idx=rows, gdelta=self._g_clip, scratch=self._pg_scratch)
        # the frames of the per-clip gradient fold onto their rows -- under a channel by the transpose of the mix the forward ran, on the same tables
        if cap is None:
            return ops.flicker_rows_grad(self._g_clip, pm.rows_dev, self.P, out=out)
        return ops.flicker_rows_mix_grad(self._g_clip, pm.rows_dev, self.P, pm.taps_dev, pm.gain_dev, out=out)

    def _check_x(self, x):
        """a clip is the normalised fp32 tensor or its uint8 frames (decoded on the device, bitwise the same clip)"""
        if tuple(x.shape) != (self.B, self.T, self.H, self.W, 3) or x.dtype not in CLIP_DTYPES or not x.is_cuda:
            raise ValueError(f"clip must be a CUDA float32 or uint8 channels-last tensor {(self.B, self.T, self.H, self.W, 3)}, "
                             f"got {tuple(x.shape)} {x.dtype}")
        return x.contiguous()

    def _buf(self, name, shape, dtype=torch.float32):
        """the engine's buffer ``self.<name>``, created on first use (an engine that never takes the path never holds it) and made anew
        only when more rows are asked for than it has: it grows on demand and never shrinks.  Uninitialised: its user writes it"""
        t = getattr(self, name, None)
        if t is None or t.shape[0] < shape[0]:
            t = torch.empty(shape, dtype=dtype, device=self._logits.device)
            setattr(self, name, t)
        return t

    def _clip_buf(self, name, n=0, dtype=torch.float32):
        """``_buf`` for clips at the engine's size: at least ``max(n, B)`` of them"""
        return self._buf(name, (max(int(n), self.B), self.T, self.H, self.W, 3), dtype)

    def _prepare_clips(self, clips, **kw):
        """ops.prepare_clips at the engine's geometry (``im_scale``, ``image_size``, ``resize_rule``)"""
        return ops.prepare_clips(clips, im_scale=self.im_scale, input_size=(self.H, self.W), rule=self.resize_rule, **kw)

    def set_frame_numbers(self, table):
        """flicker_time "video": the frame numbers of the batch the next forwards see -- integers ``[B,T]``, clip b's frame t being frame
        ``table[b,t]`` of its video (pre-cut clips; ``prepare_videos`` sets it itself), or None: 0..T-1 for every clip.  The table stays
        until the next one is set: clips from another source want their own"""
        if not self.video_time:
            raise ValueError("set_frame_numbers: an engine built with flicker_time='video' only (on clip time frame t takes row t)")
        if table is not None and np.asarray(table).shape != (self.B, self.T):
            raise ValueError(f"set_frame_numbers: an integer table {(self.B, self.T)}, got {np.asarray(table).shape}")
        self.pert_model.set_frame_numbers(table)

    @property
    def last_phases(self):
        """flicker_time "video": the phases, one per video of the batch, the last adversarial forward ran at"""
        return self.pert_model.last_phases

    @property
    def last_capture(self):
        """the capture channels, one per video of the batch, of the last adversarial forward that went through one: ``subframe`` [V],
        ``exposure`` [V], ``gain`` [V,3] and the tables made from them, one row per clip: ``taps`` fp32 [B,K], ``gain_rows`` fp32 [B,3]; a
        channel with a readout (rolling shutter) adds ``readout`` [V], and ``taps`` is then per line, fp32 [B,H,K]"""
        return self.pert_model.last_capture

    @staticmethod
    def _check_augment(augment):
        """the ``augment`` dict with its defaults filled in (None stays None); anything malformed is a ValueError"""
        if augment is None:
            return None
        known = {"scales": (0.6, 1.0), "ratio": (3 / 4, 4 / 3), "flip_ratio": 0.5, "seed": 0}
        if not isinstance(augment, dict) or set(augment) - set(known):
            raise ValueError(f"augment must be a dict with keys among {sorted(known)}, got {augment!r}")
        a = {**known, **augment}
        for key in ("scales", "ratio"):
            v = a[key]
            if v is None and key == "scales":
                continue
            if not (isinstance(v, (tuple, list)) and len(v) == 2 and 0 < float(v[0]) <= float(v[1])):
                raise ValueError(f"augment[{key!r}] must be an increasing pair of positive numbers{' or None' if key == 'scales' else ''}, got {v!r}")
            a[key] = (float(v[0]), float(v[1]))
        if not 0.0 <= float(a["flip_ratio"]) <= 1.0:
            raise ValueError(f"augment['flip_ratio'] must be a probability, got {a['flip_ratio']!r}")
        a["flip_ratio"], a["seed"] = float(a["flip_ratio"]), int(a["seed"])
        return a

    def prepare(self, frames, out=None, out_offset=0, train=False):
        """raw decoded uint8 frames -- a CUDA tensor ``[N,T,H,W,3]`` or a list of ``[T,H,W,3]`` tensors of any (differing) ``H x W`` -- to
        the normalised fp32 clips ``[N,T,self.H,self.W,3]`` this engine takes: the reference's evaluation transform (dataset.py:84-123) in
        one kernel (ops.prepare_clips), at the engine's ``im_scale`` / ``resize_rule``.  ``out``: rows ``out_offset ...`` of a batch buffer.
        ``train=True`` (an engine built with ``augment``): the training transform -- one ``(box, flip)`` per clip drawn in clip order
        from the engine's generator (videoresnet_spec.train_crop_params) and kept, as ``{"boxes": [...], "flips": [...]}``, on
        ``last_augment``."""
        if train and self.augment is None:
            raise ValueError("prepare(train=True) needs an engine built with augment={...}")
        clips = list(frames) if isinstance(frames, (list, tuple)) else frames
        for k in range(len(clips)):
            if torch.is_tensor(clips[k]) and clips[k].dim() == 4 and int(clips[k].shape[0]) != self.T:
                raise ValueError(f"clip {k} has {int(clips[k].shape[0])} frames, the engine takes {self.T}")
        boxes, flips = self._draw_boxes(clips) if train else (None, None)
        return self._prepare_clips(clips, out=out, out_offset=out_offset, boxes=boxes, flips=flips)

    def _draw_boxes(self, clips):
        """the training transform's draw: one ``(box, flip)`` per clip, in clip order, from the engine's generator
        (videoresnet_spec.train_crop_params on the clip's resized extent), kept on ``last_augment`` -> ``(boxes, flips)``"""
        boxes, flips = [], []
        for x in clips:                                              # (a 5-d tensor iterates over its clips)
            Hr, Wr = ops._prep_geometry(int(x.shape[-3]), int(x.shape[-2]), self.im_scale, (self.H, self.W), self.resize_rule)[:2]
            *box, flip = train_crop_params(Hr, Wr, (self.H, self.W), self.augment["scales"], self.augment["ratio"],
                                           self.augment["flip_ratio"], self._aug_rng)
            boxes.append(tuple(box))
            flips.append(flip)
        self.last_augment = {"boxes": boxes, "flips": flips}
        return boxes, flips

    def prepare_videos(self, videos, train=False, num_samples=1, out=None, out_offset=0):
        """whole decoded videos -- a list of CUDA uint8 tensors ``[N_k,H_k,W_k,3]`` of any (differing) length and resolution -- to
        ``len(videos) * num_samples`` normalised fp32 clips ``[T,self.H,self.W,3]``, video-major and sample-minor, in ONE launch per
        ``FLK_PREP_MAX_CLIPS`` clips: the frame-index tables are drawn on the host (videoresnet_spec.sample_frame_indices, in video order
        from the engine's temporal generator) and the kernel reads the resident videos through them (ops.prepare_clips(frame_idx=)).
        ``train=False``: the test split's settings (no shift, no jitter) and the evaluation transform.  ``train=True``: the training
        split's (videoresnet_spec.split_sampling) and, on an engine built with ``augment``, the training transform with one
        ``(box, flip)`` per clip as ``prepare(train=True)`` draws them.  The tables are kept, one int64 ``[num_samples, T]`` per video,
        on ``last_sampling``; boxes and flips on ``last_augment``."""
        clips, rows, boxes, flips = self._draw_video_clips(videos, train, num_samples, "prepare_videos")
        return self._prepare_clips(clips, out=out, out_offset=out_offset, boxes=boxes, flips=flips, frame_idx=rows)

    @staticmethod
    def _check_videos(videos, who):
        """whole videos as every method takes them -- a non-empty list of uint8 tensors ``[N,H,W,3]`` -- as a list"""
        videos = list(videos) if isinstance(videos, (list, tuple)) else None
        if not videos or any(not torch.is_tensor(v) or v.dim() != 4 or v.dtype != torch.uint8 or v.shape[0] < 1 for v in videos):
            raise ValueError(f"{who}: videos must be a non-empty list of uint8 tensors [N,H,W,3]")
        return videos

    def _draw_video_clips(self, videos, train, num_samples, who):
        """the host half of ``prepare_videos`` (and of ``step_videos``): the frame tables, boxes and flips of ``len(videos) * num_samples``
        clips drawn from the engine's generators, kept on ``last_sampling`` / ``last_augment`` and (video time) set as the batch's frame
        numbers -> ``(clips, rows, boxes, flips)``: the video of every clip, the tables stacked ``[n,T]``, the boxes / flips or None"""
        videos = self._check_videos(videos, who)
        if int(num_samples) < 1:
            raise ValueError(f"{who}: num_samples must be >= 1, got {num_samples!r}")
        kw = split_sampling(self.sampling, self.T, train)
        tables = [sample_frame_indices(int(v.shape[0]), num_samples=int(num_samples), rng=self._samp_rng, **kw) for v in videos]
        self.last_sampling = tables
        if self.video_time:                                          # the batch's frame numbers, video-major and sample-minor like its clips
            self.pert_model.set_frame_numbers(np.concatenate(tables))
        clips = [v for v in videos for _ in range(int(num_samples))]
        boxes, flips = self._draw_boxes(clips) if train and self.augment is not None else (None, None)
        return clips, np.concatenate(tables), boxes, flips

    def evaluate_videos(self, videos, labels, num_samples=10, adversarial=False, quantise=None, capture=None, capture_draws=1, codec=None):
        """``VideoLearnerAdversarial.evaluate(num_samples)`` (model.py:1227-1317) on whole videos resident on the device: every video is
        scored by the argmax of the summed logits of ``num_samples`` clips cut at uniform offsets (the test split: no shift, no jitter)
        and prepared with the evaluation transform.  ``videos``: a list of CUDA uint8 ``[N_k,H_k,W_k,3]``; ``labels``: one class per video.

        Packing: the ``V * num_samples`` clips are taken video-major and sample-minor and packed into consecutive batches of the
        engine's ``B``; the last batch is padded by repeating its last clip and the padded rows are dropped.  The per-video sums are
        taken in fp32, clip after clip.  ``adversarial=True`` runs every batch clean and through the engine's perturbation.
        Returns a dict of host arrays: ``clip_logits`` fp32 ``[V * num_samples, classes]`` and ``video_logits`` fp32 ``[V, classes]`` (the
        perturbed ones when ``adversarial``), ``video_preds``, ``video_trues``, ``clip_preds``, ``clip_trues`` (int64), ``video_accuracy``,
        ``clip_accuracy``; with ``adversarial`` also ``clean_clip_logits``, ``clean_video_logits``, ``clean_clip_preds``,
        ``clean_video_preds``, ``clean_video_accuracy``, ``clean_clip_accuracy`` and ``video_fooling_ratio`` -- among the videos
        classified correctly when clean, the share whose adversarial video prediction differs from the label (nan when there is none).
        ``quantise`` (implies ``adversarial``): score the attack as it is DELIVERED, in 8 bits per channel.  ``"clip"``: the adversarial
        logits are those of each prepared clip perturbed and exported to 8-bit frames at the engine's size (``logits(adversarial_frames(x),
        False)``).  ``"video"``: every whole video is flickered at its native resolution (``export_video``) and scored by the ordinary clean
        evaluation -- the exported videos are made batch by batch and no more of them are held than one batch needs.  Both add
        ``realised_flicker``: the mean of (frame byte - source byte) per frame and channel, in levels -- fp64 ``[V * num_samples, T, 3]``
        ("clip"; the source being the 8-bit encoding of the prepared clip) or a list of ``[N_k, 3]`` per video ("video").
        ``capture`` (a videoresnet_spec.CaptureChannel; flicker_time "video", with ``adversarial`` or ``quantise``) and ``capture_draws`` = N:
        the attack as N random cameras record it.  N times, one capture channel per video is drawn from ``capture`` (N ``draw(V)`` calls,
        made before anything is scored) and the adversarial scoring above is repeated with every video's flicker going through its
        channel (``logits(x, True, phases=0, capture=)``, ``adversarial_frames(capture=)`` or ``export_video(capture=)``).  Adds
        ``capture_draws`` (the list of the N draws), ``capture_clip_logits`` fp32 ``[N, V * num_samples, classes]``, ``capture_video_logits``
        fp32 ``[N, V, classes]``, ``capture_video_fooling_ratios`` fp64 ``[N]`` and their ``capture_video_fooling_ratio_mean`` /
        ``capture_video_fooling_ratio_min``.  Everything else in the result is what it is without ``capture`` (no channel).
        ``codec`` (a videoresnet_spec.Codec; with ``quantise="video"`` only): every exported video, those of the capture draws included,
        goes through the lossy codec (ops.codec_roundtrip) before it is scored -- the attack as a viewer of the compressed file
        receives it.  Adds ``codec_stats``: per video the int32 ``[N_k,2]`` table of the codec launch (non-zero quantised coefficients
        and the sum of their magnitudes per frame: a proxy for the bit rate).  None: exactly the result without it.
        Known difference from the reference: its loop starts at video 1 (``range(1, len(ds))``, model.py:1279-1281) and so never
        scores the first video; this one evaluates every video."""
        videos = self._check_videos(videos, "evaluate_videos")
        trues = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels, dtype=np.int64).reshape(-1)
        S, V = int(num_samples), len(videos)
        if S < 1 or trues.shape[0] != V:
            raise ValueError(f"evaluate_videos: {V} videos, {trues.shape[0]} labels, num_samples {num_samples!r}")
        kw = split_sampling(self.sampling, self.T, False)
        tables = [sample_frame_indices(int(v.shape[0]), num_samples=S, rng=self._samp_rng, **kw) for v in videos]
        self.last_sampling = tables
        rows = np.concatenate(tables)
        if quantise not in (None, "clip", "video"):
            raise ValueError(f"evaluate_videos: quantise must be None, 'clip' or 'video', got {quantise!r}")
        adversarial = adversarial or quantise is not None
        if self._check_codec(codec, "evaluate_videos") is not None and quantise != "video":
            raise ValueError(f"evaluate_videos: codec compresses whole delivered videos -- it needs quantise='video', got quantise={quantise!r}")
        if self.illumination and adversarial and quantise != "video":
            raise ValueError("evaluate_videos: flicker_model='illumination' lights the stored bytes of a video -- score it with quantise='video' "
                             "(the clips prepared here are resampled fp32 values, which the camera tables do not take)")
        draws = []
        if capture is not None:
            if not (isinstance(capture, CaptureChannel) and self.video_time and adversarial):
                raise ValueError("evaluate_videos: capture must be a videoresnet_spec.CaptureChannel, on an engine built with flicker_time='video', "
                                 "with adversarial=True or quantise")
            if isinstance(capture_draws, bool) or not isinstance(capture_draws, (int, np.integer)) or capture_draws < 1:
                raise ValueError(f"evaluate_videos: capture_draws must be an integer >= 1, got {capture_draws!r}")
            draws = [capture.draw(V) for _ in range(int(capture_draws))]
        kept = self.pert_model.frame_numbers                            # video time: every batch below brings its own frame numbers
        clean, adv, stats, delivered = [], [], ([], []), {}
        for ks, n, x in self._packed_batches(videos, rows, S):
            clean.append(self.logits(x, False)[:n].cpu())
            if adversarial:
                adv.append(self._adversarial_logits(x, videos, [k // S for k in ks], rows[ks], quantise, None, codec, delivered, stats)[:n].cpu())
        cap_adv = []
        for d in draws:                                                 # the adversarial scoring again, every video through its channel
            parts, delivered = [], {}
            for ks, n, x in self._packed_batches(videos, rows, S, prepare=quantise != "video"):
                parts.append(self._adversarial_logits(x, videos, [k // S for k in ks], rows[ks], quantise, d, codec, delivered)[:n].cpu())
            cap_adv.append(parts)
        self.pert_model.frame_numbers = kept

        def score(parts):
            clip = torch.cat(parts).numpy()
            video = np.zeros((V, clip.shape[1]), np.float32)
            for j in range(S):                                       # fp32, clip after clip
                video += clip[j::S]
            return clip, video, clip.argmax(1).astype(np.int64), video.argmax(1).astype(np.int64)

        clip_trues = np.repeat(trues, S)
        c_clip, c_video, c_cp, c_vp = score(clean)
        res = {"video_trues": trues, "clip_trues": clip_trues}
        if adversarial:
            clip, video, cp, vp = score(adv)
            ok = c_vp == trues
            res.update(clean_clip_logits=c_clip, clean_video_logits=c_video, clean_clip_preds=c_cp, clean_video_preds=c_vp,
                       clean_video_accuracy=float((c_vp == trues).mean()), clean_clip_accuracy=float((c_cp == clip_trues).mean()),
                       video_fooling_ratio=float(((vp != trues) & ok).sum() / ok.sum()) if ok.any() else float("nan"))
        else:
            clip, video, cp, vp = c_clip, c_video, c_cp, c_vp
        res.update(clip_logits=clip, video_logits=video, clip_preds=cp, video_preds=vp,
                   video_accuracy=float((vp == trues).mean()), clip_accuracy=float((cp == clip_trues).mean()))
        if quantise == "clip":                                       # (the padded rows of the last batch are its tail)
            res["realised_flicker"] = np.concatenate([st[:, :, :, 0].cpu().numpy() / float(self.H * self.W) for st in stats[0]])[:V * S]
        elif quantise == "video":
            res["realised_flicker"] = [st[:, :, 0].cpu().numpy() / float(v.shape[1] * v.shape[2]) for st, v in zip(stats[0], videos)]
        if codec is not None:
            res["codec_stats"] = [cs.cpu().numpy() for cs in stats[1]]
        if draws:
            scored = [score(parts) for parts in cap_adv]
            ratios = np.asarray([float(((s[3] != trues) & ok).sum() / ok.sum()) if ok.any() else float("nan") for s in scored], np.float64)
            res.update(capture_draws=draws, capture_clip_logits=np.stack([s[0] for s in scored]), capture_video_logits=np.stack([s[1] for s in scored]),
                       capture_video_fooling_ratios=ratios, capture_video_fooling_ratio_mean=float(ratios.mean()),
                       capture_video_fooling_ratio_min=float(ratios.min()))
        return res

    def _packed_batches(self, videos, rows, S, prepare=True):
        """``evaluate_videos``' packing: the ``len(videos) * S`` clips, video-major and sample-minor (clip k belongs to video ``k // S`` and
        is cut at ``rows[k]``), in consecutive batches of B, the last one repeating its last clip.  Per batch ``(ks, n, x)``: its clip
        numbers, how many of them are real, and -- unless ``prepare`` is off -- its clean clips in the engine's fp32 buffer"""
        x = self._clip_buf("_prep_buf")[:self.B]
        last = len(videos) * S - 1
        for first in range(0, last + 1, self.B):
            ks = [min(first + b, last) for b in range(self.B)]
            if prepare:
                self._prepare_clips([videos[k // S] for k in ks], out=x, frame_idx=rows[ks])
            yield ks, min(self.B, last + 1 - first), x

    def _adversarial_logits(self, x, videos, of, frame_idx, quantise=None, channels=None, codec=None, delivered=None, stats=None):
        """the logits of one batch under the engine's perturbation at phase 0, the way ``quantise`` delivers it.  ``x``: the batch's clean
        clips; ``of``: the number, in ``videos``, of every clip's video; ``frame_idx``: the frames the clips were cut at.  ``channels``: a
        draw of ``CaptureChannel.draw(len(videos))`` -- every video's flicker goes through its own channel -- or None.
        ``quantise`` None: ``logits(x, True)``; "clip": the clips exported to 8-bit frames, scored clean; "video": every video of the batch is
        flickered whole at its own resolution (``export_video``) and compressed by ``codec``, and its clips, cut from the stored bytes
        into the engine's fp32 buffer (``x`` is not read), are scored clean.  ``delivered``: {video number: its delivered form}, kept by
        the caller from batch to batch -- a video whose clips straddle two batches is exported once; videos the batch does not hold are
        dropped.  ``stats``: a pair of lists that take the export's stats table per batch ("clip") or per exported video ("video") and
        the codec's per video; None: none are made"""
        if self.video_time:                                          # the rows of these clips' own frames
            self.pert_model.set_frame_numbers(frame_idx)
        want = stats is not None

        def pair(res):                                               # (the launches return their stats only when asked)
            return res if want else (res, None)

        if quantise != "video":
            per_clip = None if channels is None else {k: channels[k][of] for k in channels}      # (with its readout, if the channel has one)
            if quantise is None:
                return self.logits(x, True, phases=0, capture=per_clip)    # (phases: video time only -- clip time draws its roll as ever)
            frames, st = pair(self.adversarial_frames(x, stats=want, capture=per_clip))
            if want:
                stats[0].append(st)
            return self.logits(frames, False)
        delivered = {} if delivered is None else delivered
        for v in [v for v in delivered if v not in of]:
            del delivered[v]
        for v in sorted(set(of) - set(delivered)):
            one = None if channels is None else {k: (channels[k][v] if k == "gain" else float(channels[k][v])) for k in channels}
            delivered[v], st = pair(self.export_video(videos[v], stats=want, capture=one))
            if want:
                stats[0].append(st)
            if codec is not None:
                (delivered[v],), cs = pair(ops.codec_roundtrip([delivered[v]], codec, stats=want))
                if want:
                    stats[1].append(cs[0])
        out = self._clip_buf("_prep_buf", len(of))
        return self.logits(self._prepare_clips([delivered[v] for v in of], out=out, frame_idx=frame_idx), False)

    def _is_raw(self, x):
        """uint8 frames that are not at the engine's H x W yet (clips that are take today's path: decoded by the apply kernel)"""
        return torch.is_tensor(x) and x.dtype == torch.uint8 and x.dim() == 5 and tuple(x.shape[2:4]) != (self.H, self.W)

    def _prepared(self, x, train=False):
        """``x`` itself, or -- raw-size uint8 frames -- their clips prepared into the engine's one reused fp32 buffer (valid until the next
        call).  ``train``: with the training transform (an engine built with ``augment`` only)."""
        if not self._is_raw(x):
            return x
        return self.prepare(x, out=self._clip_buf("_prep_buf", x.shape[0]), train=train)

    @staticmethod
    def _same_dtype(dtype, x, what):
        """the dtype every clip of one call shares (``dtype`` None: x's); a mixture is refused"""
        if x.dtype not in CLIP_DTYPES:
            raise ValueError(f"{what}: clips must be float32 or uint8, got {x.dtype}")
        if dtype is not None and x.dtype != dtype:
            raise ValueError(f"{what}: clips of one call must share a dtype, got {dtype} and {x.dtype}")
        return x.dtype

    def logits(self, x, adversarial=False, phases="draw", capture=None):
        """model([x, adversarial]) (model.py:1028,1073).  ``phases`` (flicker_time "video"): "draw" -- one per video when ``cyclic_pert``,
        else 0 -- or the phase(s) to apply at.  ``capture`` (flicker_time "video"): None -- no capture channel -- or the channel(s) the
        flicker is recorded through: "draw" (an engine built with ``capture``) or a dict (Perturbation.delta_clip)"""
        self._forward(x, adversarial, phases, capture)
        return self._logits

    def adversarial_frames(self, x, out=None, stats=False, adversarial=True, capture=None):
        """the perturbed clips as 8-bit frames: uint8 ``[N,T,H,W,3]`` of the engine's perturbation over ``x`` (fp32 or uint8 clips at the
        engine's size; per-clip engines: N == B), one kernel launch (Perturbation.export_u8).  ``out``: a uint8 buffer to fill.
        ``stats``: also the int32 ``[N,T,3,4]`` table of ops.export_adversarial_u8.  ``adversarial=False``: the frames of the clean clips."""
        if x.dim() != 5 or tuple(x.shape[1:]) != (self.T, self.H, self.W, 3) or x.dtype not in CLIP_DTYPES or not x.is_cuda:
            raise ValueError(f"clips must be CUDA float32 or uint8 channels-last tensors [N,{self.T},{self.H},{self.W},3], got {tuple(x.shape)} {x.dtype}")
        return self.pert_model.export_u8(x, adversarial, stats=stats, out=out, capture=capture)

    def quantised_logits(self, x, adversarial=True, capture=None):
        """the logits of the STORED adversarial video: ``x`` perturbed and written as 8-bit frames (``adversarial_frames``, into a buffer the
        engine reuses), then scored by the clean uint8 path -- ``logits(frames, False)``"""
        frames = self.adversarial_frames(self._check_x(x), out=self._clip_buf("_q_buf", dtype=torch.uint8), adversarial=adversarial, capture=capture)
        return self.logits(frames, False)

    @staticmethod
    def _check_codec(codec, what=None):
        """``codec`` itself, a videoresnet_spec.Codec or None (``what``: the method the message names; None: the constructor)"""
        if codec is not None and not isinstance(codec, Codec):
            raise ValueError(f"{what + ': ' if what else ''}codec must be a videoresnet_spec.Codec or None, got {type(codec).__name__}")
        return codec

    def export_video(self, video_u8, phase=0, stats=False, capture=None, codec=None):
        """the engine's flicker laid over a WHOLE video at its own resolution: ``video_u8`` uint8 ``[N,H,W,3]`` on the device -> uint8
        ``[N,H,W,3]``, frame n perturbed by row ``(n - phase) mod P`` of the perturbation (period P = the engine's T, or the ``flicker_period``
        of an engine on video time; the flicker is uniform over a frame, so it needs no resize).  One kernel launch.  Flicker attacks with
        one shared perturbation only.  ``stats``: also the int32 ``[N,3,4]`` table of ops.export_adversarial_u8.  ``capture`` (video time):
        ONE capture channel, a dict of the scalars ``subframe`` and ``exposure`` and ``gain`` [3] -- the video a camera with that channel
        records: the perturbation exported is the channel's mix of the rows (Perturbation.captured_perturbation, one launch), so frame n
        carries what a training step under that channel at that phase gives frame number n.  ``codec`` (a videoresnet_spec.Codec): the
        COMPRESSED delivered video -- the export followed by the codec launch, bit for bit ``ops.codec_roundtrip([export_video(video)],
        codec)[0]``; the stats stay the export's."""
        self._check_codec(codec, "export_video")
        if self.attack_type != "flickering" or self.per_clip:
            raise ValueError("export_video: the flickering attack with one shared perturbation only (a dense or per-clip perturbation belongs to its clip)")
        if not torch.is_tensor(video_u8) or video_u8.dim() != 4 or video_u8.dtype != torch.uint8 or video_u8.shape[-1] != 3 or not video_u8.is_cuda or video_u8.shape[0] < 1:
            raise ValueError("export_video: a CUDA uint8 tensor [N,H,W,3]")
        a = self.pert_model.export_args(video_u8.contiguous()[None], True, shift_p=int(phase), delta_T=self.P, capture=capture)
        if self.illumination:
            res = ops.illum_export_u8(a, self.pert_model.illum, stats=stats, delta_T=self.P)
        else:
            res = ops.export_adversarial_u8(a, "torch", stats=stats, delta_T=self.P)
        video = res[0][0] if stats else res[0]
        if codec is not None:
            video = ops.codec_roundtrip([video], codec)[0]
        return (video, res[1][0]) if stats else video

    def _check_video_labels(self, labels):
        """clips_per_video > 1: one label per VIDEO"""
        if not torch.is_tensor(labels) or labels.dim() != 1 or int(labels.shape[0]) != self.V:
            got = tuple(labels.shape) if torch.is_tensor(labels) else type(labels).__name__
            raise ValueError(f"clips_per_video = {self.clips_per_video}: labels must hold one class per video, shape ({self.V},), got {got}")

    def video_logits(self, clip_logits):
        """the videos' aggregated logits [V,classes] from clip logits [V*G,classes] (video-major, sample-minor) with torch: fp32 sums clip
        after clip, then the scale of ``video_reduce`` -- bitwise what the loss head forms and, for "sum", what ``evaluate_videos`` sums"""
        G = self.clips_per_video
        z = clip_logits.view(-1, G, clip_logits.shape[-1])
        acc = z[:, 0].clone()
        for g in range(1, G):
            acc = acc + z[:, g]
        return acc * self.video_scale

    def _whole_video(self, inputs):
        """fit_single_video_attack, clips_per_video > 1: ``inputs`` as ONE whole uint8 video [N,H,W,3] (or a one-element list of it), else None"""
        if isinstance(inputs, (list, tuple)) and len(inputs) == 1:
            inputs = inputs[0]
        if torch.is_tensor(inputs) and inputs.dim() == 4 and inputs.dtype == torch.uint8:
            return inputs
        return None

    def step_videos(self, videos, labels, criterion, lr=1e-3, update=True, train=True, _drawn=None):
        """one iteration on the DELIVERED videos (an engine built with ``train_delivered``): ``videos`` is a list of V = B /
        clips_per_video whole raw uint8 videos ``[N_k,H_k,W_k,3]`` on the device, of any length and resolution.  The frame tables, boxes
        and flips are drawn exactly as ``prepare_videos(videos, train, clips_per_video)`` draws them (same generators, same order, kept
        on ``last_sampling`` / ``last_augment``); the frame numbers are set; the per-clip perturbation of those frames is gathered (or
        mixed through a capture channel drawn per video) and turned into tone tables by the export kernel of the engine's pixel model
        on a ramp clip; the toned preparation writes the clips of the flickered, 8-bit videos into the engine's fp32 buffer; the CLEAN
        forward scores them -- the logits are bit for bit those of ``prepare_clips(export_video(v, phase), ...)`` -- and the backward's
        input gradient goes through the slopes of the tone tables and the resampling (ops.prepare_clips_grad) to the per-clip gradient
        the existing row fold and update kernels take.  ``train=False``: the test split's sampling and the evaluation transform (what
        ``evaluate_videos(quantise="video")`` scores).  ``StepResult`` as ``step``'s."""
        if not self.train_delivered:
            raise ValueError("step_videos: an engine built with train_delivered=True only")
        if criterion.attack_type != self.attack_type:
            raise ValueError(f"criterion.attack_type {criterion.attack_type!r} != engine attack_type {self.attack_type!r}")
        if _drawn is None:
            _drawn = self._draw_video_clips(videos, train, self.clips_per_video, "step_videos")
        if len(_drawn[0]) != self.B:
            raise ValueError(f"step_videos: {len(_drawn[0]) // self.clips_per_video} videos of {self.clips_per_video} clips, the engine takes {self.V}")
        return self.step(None, labels, criterion, lr=lr, update=update, _delivered=_drawn)

    def _forward_delivered(self, drawn, capture):
        """``step_videos``' forward: tone tables of the batch's frames, the toned preparation, the clean forward.  Returns the apply
        arguments of the ramp: the step takes the slopes from the same"""
        clips, rows, boxes, flips = drawn
        pm, dev = self.pert_model, self._logits.device
        if not hasattr(self, "_ramp"):                               # what only this chain reads: the ramp clip, the scratch of its backward
            self._ramp = ops.tone_ramp(self.B, self.T, dev)
            self._pg_scratch = torch.empty(max(1, ops.load().flk_clip_prepare_grad_scratch_bytes(min(self.B, ops.FLK_PREP_MAX_CLIPS), self.T, self.H) // 4),
                                           dtype=torch.float32, device=dev)
        ta = pm.export_args(self._ramp, True, shift_p="draw", capture=capture)      # the per-clip delta of this batch's frame numbers
        kw = dict(out=self._clip_buf("_prep_buf"), boxes=boxes, flips=flips)
        if self.codec is not None and self.codec.gop > 1:
            frames, picked = self._gop_frames(clips, rows, capture is not None)
            self._forward(self._prepare_clips(frames, frame_idx=picked, **kw), False)
            return ta
        tone = self._buf("_tone", (self.B, self.T, 256, 3), torch.uint8)
        ops.flicker_tone_tables(ta, pm.illum if self.illumination else None, out=tone)
        if self.codec is not None:
            # the compressed delivered video: ONE codec launch tones and compresses only the batch's B * T frames at their native
            # resolution into uint8 buffers the engine reuses; the untoned sampled preparation of those follows (identity frame table)
            frames = ops.codec_roundtrip(list(clips), self.codec, frame_idx=rows, tone=tone, out=self._codec_out(clips, [self.T] * len(clips)))
            x = self._prepare_clips(frames, frame_idx=np.broadcast_to(np.arange(self.T), (len(frames), self.T)), **kw)
        else:
            x = self._prepare_clips(clips, frame_idx=rows, tone=tone, **kw)
        self._forward(x, False)
        return ta

    def _gop_frames(self, clips, rows, captured):
        """``_forward_delivered`` under a codec with GOPs: a P-frame needs every frame since its intra frame, so per clip the SPAN from
        the intra frame at or before its first frame to its last frame is toned and compressed -- the lead-in frames in front of the
        clip at their own frame numbers, under the phase and the capture channel the step just drew for the clip -- in ONE GOP launch
        into reused uint8 buffers.  Returns them with the frame table that picks the clip's frames out of its span: what the untoned
        sampled preparation takes.  (The tone tables come from one export launch on the ramp, the span cut into pieces of T frames that
        stand in it as further clips: [B * pieces, T, 256, 3] IS [B, pieces * T, 256, 3].)"""
        pm, dev, T, N = self.pert_model, self._logits.device, self.T, self.codec.gop
        rows = np.asarray(rows, dtype=np.int64)
        first = rows.min(1) // N * N
        count = rows.max(1) - first + 1
        pieces = int(-(-count.max() // T))
        numbers = (first[:, None] + np.arange(pieces * T)).reshape(self.B * pieces, T)        # past a span's end: made, never read
        if getattr(self, "_span_ramp", None) is None or self._span_ramp.shape[0] != self.B * pieces:
            self._span_ramp = ops.tone_ramp(self.B * pieces, T, dev)
            self._span_tone = torch.empty((self.B * pieces, T, 256, 3), dtype=torch.uint8, device=dev)
        sa = pm.export_args_like_last(self._span_ramp, numbers, np.repeat(np.arange(self.B), pieces), captured)
        ops.flicker_tone_tables(sa, pm.illum if self.illumination else None, out=self._span_tone)
        frames = ops.codec_roundtrip(list(clips), self.codec, spans=np.stack([first, count], 1), tone=self._span_tone.view(self.B, pieces * T, 256, 3),
                                     out=self._codec_out(clips, count))
        return frames, rows - first[:, None]

    def _codec_out(self, clips, lengths):
        """the uint8 buffers the codec launch of ``_forward_delivered`` writes, one per clip of the batch at its video's resolution and
        of ``lengths[k]`` frames: kept from step to step while the slot's resolution stays, grown when a longer span comes"""
        if not hasattr(self, "_codec_bufs"):
            self._codec_bufs = {}
        bufs = self._codec_bufs
        want = [(k, int(v.shape[1]), int(v.shape[2])) for k, v in enumerate(clips)]
        for key in [key for key in bufs if key not in want]:
            del bufs[key]
        for key, n in zip(want, lengths):
            if key not in bufs or bufs[key].shape[0] < n:
                bufs[key] = torch.empty((int(n), key[1], key[2], 3), dtype=torch.uint8, device=self._logits.device)
        return [bufs[key][:int(n)] for key, n in zip(want, lengths)]

    def step(self, x, labels, criterion, lr=1e-3, update=True, _delivered=None):
        """one iteration of fit_single_video_attack (model.py:1073-1101): forward, Losses, backward, torch-Adam step.
        The kernels write into one of ``RESULT_SLOTS`` result slots (valid for the next RESULT_SLOTS - 1 iterations);
        ``loss`` / ``argmax`` are derived on first access (i3d_engine.StepResult).  (``_delivered``: ``step_videos``' clips.)"""
        from .i3d_engine import RESULT_SLOTS, StepResult
        if criterion.attack_type != self.attack_type:
            raise ValueError(f"criterion.attack_type {criterion.attack_type!r} != engine attack_type {self.attack_type!r}")
        if self.attack_type == "L12":
            return self._step_dense(x, labels, criterion, lr, update)
        if self.per_clip:
            return self._step_per_clip(x, labels, criterion, lr, update)
        G, V = self.clips_per_video, self.V                     # G = 1: V = B, every clip its own "video"
        if G > 1:
            self._check_video_labels(labels)
        if not hasattr(self, "_slots"):
            dev = self._logits.device
            self._slots = [dict(payload=torch.zeros(parallel.payload_size(self.P), dtype=torch.float32, device=dev),
                                sm=torch.empty((V, self.num_classes), dtype=torch.float32, device=dev),
                                pc=torch.empty((V, 4), dtype=torch.float32, device=dev),
                                scalars=torch.zeros(8, dtype=torch.float32, device=dev)) for _ in range(RESULT_SLOTS)]
            if G > 1:
                for s in self._slots:
                    s["vl"] = torch.empty((V, self.num_classes), dtype=torch.float32, device=dev)
            self._dl = torch.empty_like(self._logits)
            self._it = 0
        slot = self._slots[self._it % RESULT_SLOTS]
        self._it += 1
        red, sm, pc = slot["payload"], slot["sm"], slot["pc"]
        self._red = red
        cap = "draw" if self.capture is not None else None     # one capture channel per video, fresh every step
        a = self._forward(x, True, capture=cap) if _delivered is None else self._forward_delivered(_delivered, cap)
        gbatch = V * self.world
        if G > 1:
            criterion.adv_video(labels, self._logits, gbatch, G, self.video_reduce, out=(sm, self._dl, pc, slot["vl"]))
        else:
            criterion.adv(labels, self._logits, gbatch, out=(sm, self._dl, pc))
        self.net.backward(self._dl, self._gx)
        n = 3 * self.P                                          # (clip time: P == T)
        self._payload_grad(a, cap, _delivered, red[:n].view(self.P, 3))
        ops.pack_batch_sums(pc, 1.0 / gbatch, red[n:])
        parallel.allreduce_sum_(red, self.pg)
        res = StepResult(adv_loss=red[n], softmax=sm, label_prob=pc[:, 1], _argmax_f=pc[:, 3], _labels=labels, _targeted=bool(criterion.targeted))
        if G > 1:
            res["video_logits"] = slot["vl"]
        if update:
            self.adam_t += 1
            b1 = criterion.beta_1
            sc = slot["scalars"]
            if self.pgd:
                ops.perturb_reg_pgd(red[:n], self.pert_model.perturbation, dialect="torch", beta0=criterion.lambda_, beta1=b1, beta2=1 - b1,
                                    beta3=1 - b1, dyn_max_norm=self.pert_model.dynamic_max_norm, lr=lr, scalars=sc)
            else:
                ops.perturb_reg_adam(red[:n], self.pert_model.perturbation, self.adam_m, self.adam_v, self.adam_t, dialect="torch",
                                     beta0=criterion.lambda_, beta1=b1, beta2=1 - b1, beta3=1 - b1,
                                     dyn_max_norm=self.pert_model.dynamic_max_norm, lr=lr, scalars=sc)
            res.update(reg_loss=sc[0], _reg_weight=criterion.lambda_, _thickness=sc[4], _roughness=sc[5])
        else:
            res.update(reg_loss=criterion.regularization_loss(self.pert_model.get_perturbation()[0]), _reg_weight=criterion.lambda_)
        return res

    def _step_per_clip(self, x, labels, criterion, lr, update):
        """one iteration of B independent single-video attacks (torch dialect): per-clip loss / gradient / Adam, everything [B]-shaped.
        Per clip the arithmetic is that of ``step`` on a batch of one (bitwise in fp32)."""
        from .i3d_engine import RESULT_SLOTS, StepResult
        if not hasattr(self, "_slots"):
            dev = self._logits.device
            self._slots = [dict(sm=torch.empty_like(self._logits), pc=torch.empty((self.B, 4), dtype=torch.float32, device=dev),
                                scalars=torch.zeros((self.B, 8), dtype=torch.float32, device=dev),
                                g=torch.zeros((self.B, self.T, 3), dtype=torch.float32, device=dev)) for _ in range(RESULT_SLOTS)]
            self._dl = torch.empty_like(self._logits)
            self._it = 0
        slot = self._slots[self._it % RESULT_SLOTS]
        self._it += 1
        sm, pc, g = slot["sm"], slot["pc"], slot["g"]
        a = self._forward(x, True)
        criterion.adv(labels, self._logits, 1, out=(sm, self._dl, pc))            # every clip is its own batch of one
        self.net.backward(self._dl, self._gx)
        self._grad_reduce(a, g)
        self._gclip = g
        am = pc[:, 3].to(torch.int64)
        res = StepResult(adv_loss=pc[:, 0], softmax=sm, label_prob=pc[:, 1], argmax=am, _labels=labels, _targeted=bool(criterion.targeted),
                         _reg_weight=criterion.lambda_)
        if update:
            b1 = criterion.beta_1
            sc = slot["scalars"]
            if self.pgd:
                ops.perturb_reg_pgd_batched(g, self.pert_model.perturbation, self.adam_steps, self.active, dialect="torch",
                                            beta0=criterion.lambda_, beta1=b1, beta2=1 - b1, beta3=1 - b1, lr=lr, scalars=sc,
                                            dyn_max_norm_dev=self.pert_model.dyn_max_norm_dev)
            else:
                ops.perturb_reg_adam_batched(g, self.pert_model.perturbation, self.adam_m, self.adam_v, self.adam_steps, self.active, dialect="torch",
                                             beta0=criterion.lambda_, beta1=b1, beta2=1 - b1, beta3=1 - b1, lr=lr, scalars=sc,
                                             dyn_max_norm_dev=self.pert_model.dyn_max_norm_dev)
            res.update(reg_loss=sc[:, 0], _thickness=sc[:, 4], _roughness=sc[:, 5])
        else:
            pc_ = self.pert_model.clamp_perturbation()
            res.update(reg_loss=torch.stack([criterion.regularization_loss(pc_[b].t().reshape(3, self.T, 1, 1)) for b in range(self.B)]))
        return res

    def _step_dense(self, x, labels, criterion, lr, update):
        """the dense "L12" attack (model.py:211-214,380-384): loss = adv + lambda * L12(clamped delta); the data-parallel payload
        is the dense gradient [T,H,W,3] (2.4 MB at 16 x 112 x 112)"""
        from .i3d_engine import StepResult
        G, vl = self.clips_per_video, None
        if G > 1:
            self._check_video_labels(labels)
        a = self._forward(x, True)
        gbatch = self.V * self.world
        if G > 1:
            sm, dl, pc, vl = criterion.adv_video(labels, self._logits, gbatch, G, self.video_reduce)
        else:
            sm, dl, pc = criterion.adv(labels, self._logits, gbatch)
        self._dl = dl
        self.net.backward(dl, self._gx)
        if not hasattr(self, "_gdense"):
            self._gdense = torch.empty_like(self.pert_model.perturbation)
        ops.perturb_grad_reduce(a, self._gx, self._gdense)
        tail = pc[:, :3].sum(0)
        parallel.allreduce_sum_(self._gdense, self.pg)            # RCCL over xGMI: the dense gradient (2.4 MB at 16 x 112 x 112)
        parallel.allreduce_sum_(tail, self.pg)
        res = StepResult(adv_loss=tail[0].clone(), softmax=sm, label_prob=pc[:, 1], _argmax_f=pc[:, 3], _labels=labels,
                         _targeted=bool(criterion.targeted), _reg_weight=criterion.lambda_)
        if vl is not None:
            res["video_logits"] = vl
        if update:
            self.adam_t += 1
            if self.pgd:
                sc = ops.perturb_dense_l12_pgd(self._gdense, self.pert_model.perturbation, dialect="torch", beta=criterion.lambda_, lr=lr,
                                               dyn_max_norm=self.pert_model.dynamic_max_norm).clone()
            else:
                sc = ops.perturb_dense_l12_adam(self._gdense, self.pert_model.perturbation, self.adam_m, self.adam_v, self.adam_t, dialect="torch",
                                                beta=criterion.lambda_, lr=lr, dyn_max_norm=self.pert_model.dynamic_max_norm).clone()
            res.update(reg_loss=sc[0], _thickness=sc[1], _roughness=sc[2])
        else:
            res.update(reg_loss=criterion.L12_regularization_loss(self.pert_model.get_perturbation()[0]))
        return res

    # ---- drivers around step(): VideoLearnerAdversarial's loops without the plotting ------------------------------------
    def fit_single_video_attack(self, inputs, target, criterion, lr=1e-3, n_iter=3000, targeted_attack=False, target_class_id=None,
                                restart_after=3000, norm_growth=1.3, max_restarts=4, log_every=0, export_u8=False):
        """``VideoLearnerAdversarial.fit_single_video_attack`` (model.py:984-1205).
        ``export_u8``: the result also holds ``adv_video_u8`` (the attacked clips under the final perturbation as 8-bit frames, uint8
        ``[B,T,H,W,3]``), ``quantised_pred`` (the class those frames are given, per clip or -- clips_per_video > 1 -- per video) and
        ``quantised_is_adversarial`` (is the STORED video still adversarial?); ``export_u8="verdict"`` leaves the frames out.

        Returns None when the clean clip is misclassified (model.py:1030-1032).  Otherwise iterates
        ``while step < n_iter or not is_adversarial`` (model.py:1056); whenever ``step > restart_after`` the clamp norm
        grows by ``norm_growth`` and the step counter restarts, giving up after ``max_restarts`` (model.py:1061-1066:
        3000 / 1.3 / 4).  The result dict has the reference's keys (model.py:1193-1203); per-iteration values are host
        floats (the reference syncs every iteration as well: ``loss.item()``).  Raw-size uint8 frames are prepared on the device first.
        ``clips_per_video = G > 1``: ``inputs`` are B clips (V = B / G videos, video-major and sample-minor) or, on an engine with B == G, one
        whole uint8 video ``[N,H,W,3]`` (or a one-element list of it) whose G test-split clips are attacked; ``target`` holds one class per
        video and ``prob_clean_input``, ``is_adversarial``, ``max_prob`` and ``correct_cls_prob`` are the video's (aggregated logits)."""
        G = self.clips_per_video
        video = self._whole_video(inputs) if (G > 1 or self.train_delivered) else None
        delivered = self.train_delivered and video is not None      # one whole video on a train_delivered engine: every step is step_videos
        if self.train_delivered and video is None:
            raise ValueError("fit_single_video_attack: an engine built with train_delivered attacks one whole uint8 video [N,H,W,3] (clips at "
                             "the engine's size have no native resolution: build the engine with quantise_train instead)")
        if video is not None:
            # one whole video: its G test-split clips (uniform offsets, no shift, no jitter -- the clips evaluate_videos(num_samples=G)
            # scores) are cut once, into a buffer of their own, and kept for the whole attack
            if self.B != G:
                raise ValueError(f"a whole video needs an engine with batch_size == clips_per_video, got {self.B} and {G}")
            inputs = self.prepare_videos([video], train=False, num_samples=G)
        elif isinstance(inputs, (list, tuple)):
            raise ValueError("fit_single_video_attack: inputs must be clips [B,T,H,W,3] or (clips_per_video > 1) one whole uint8 video [N,H,W,3]")
        inputs = self._prepared(inputs)
        outputs_no_adv = self.logits(inputs, False).clone()
        if G > 1:                                            # the decision attacked is the video's: clean video logits [V,classes]
            self._check_video_labels(target)
            outputs_no_adv = self.video_logits(outputs_no_adv)
        if not bool((outputs_no_adv.argmax(1) == target).all()):
            return None
        hist = self._new_history()
        step, new_chance, is_adversarial = 0, 0, False
        while step < n_iter or not is_adversarial:
            if step > restart_after:
                new_chance += 1
                self.pert_model.dynamic_max_norm *= norm_growth
                step = 0
            if new_chance == max_restarts:
                break
            r = self.step_videos([video], target, criterion, lr=lr, train=False) if delivered else self.step(inputs, target, criterion, lr=lr)
            adv_class = r["argmax"]
            is_adversarial = bool((adv_class == target_class_id).all()) if targeted_attack else not bool(adv_class.equal(target))
            # (the perturbation after the update, like model.py:1110-1112)
            self._record(hist, is_adversarial, r["loss"], r["adv_loss"], r["reg_loss"], self.pert_model.get_perturbation()[0].cpu().numpy(),
                         r["softmax"].max(), r["label_prob"][0])
            if log_every and step % log_every == 0:
                print(f"batch {step} of {n_iter} | loss = {hist['loss/total'][-1]:.4f} | adv loss = {hist['loss/adv_loss'][-1]:.4f} | "
                      f"reg loss = {hist['loss/reg_loss'][-1]:.4f} | pert_thickness = {hist['perturbation/thickness'][-1]:.4f} | "
                      f"pert_roughness = {hist['perturbation/roughness'][-1]:.4f}", flush=True)
            step += 1
        res = self._attack_result(hist, self.pert_model.get_perturbation()[0].cpu().numpy(), outputs_no_adv, target, new_chance)
        if export_u8:
            if delivered:
                # the delivered video itself: flickered whole at its own resolution, its test-split clips cut from the stored bytes
                kept = {}
                ql = self._adversarial_logits(None, [video], [0] * G, np.concatenate(self.last_sampling), "video", delivered=kept)
                frames = kept[0]
            else:
                frames = self.adversarial_frames(inputs)
                ql = self.logits(frames, False)
            res.update(self._quantised_verdict(frames, self.video_logits(ql) if G > 1 else ql, target, targeted_attack, target_class_id, export_u8))
        return res

    @staticmethod
    def _new_history():
        """the per-iteration lists of one single-video attack, under the keys its result holds them by (model.py:1193-1203)"""
        return {k: [] for k in ("loss/total", "loss/adv_loss", "loss/reg_loss", "perturbation/thickness", "perturbation/roughness", "perturbation",
                                "is_adversarial", "max_prob", "correct_cls_prob")}

    @staticmethod
    def _record(hist, is_adversarial, loss, adv_loss, reg_loss, p, max_prob, label_prob):
        """one iteration into ``hist``.  ``p``: the clamped perturbation after the update as a numpy array in the reference's layout
        [3,T,1,1] -- the memory layout ``get_perturbation()`` hands over (numpy's float32 mean depends on it in the last bit)"""
        for key, v in (("loss/total", loss), ("loss/adv_loss", adv_loss), ("loss/reg_loss", reg_loss), ("perturbation/thickness", np.abs(p).mean()),
                       ("perturbation/roughness", np.abs(np.roll(p, 1, 1) - p).mean()), ("max_prob", max_prob), ("correct_cls_prob", label_prob)):
            hist[key].append(float(v))
        hist["is_adversarial"].append(is_adversarial)
        hist["perturbation"].append(p)

    def _attack_result(self, hist, p, clean, target, restarts):
        """the result dict of one single-video attack (model.py:1193-1203): its history, the final clamped perturbation ``p``'s norm, the
        clean logits, the label and the restarts taken"""
        res = dict(hist, **{"perturbation/inf_norm": float(np.abs(p).max()), "prob_clean_input": clean, "label": target.cpu().numpy(),
                            "restarts": restarts})
        if self.video_time:                                  # the perturbations have flicker_period rows, not sample_length
            res.update(flicker_time=self.flicker_time, flicker_period=self.P)
        return res

    @staticmethod
    def _quantised_verdict(frames, logits, target, targeted_attack, target_class_id, export_u8=True):
        """the result keys of ``export_u8``: the frames on the host (unless "verdict") and what the network makes of them"""
        pred = logits.argmax(1)
        is_adv = bool((pred == target_class_id).all()) if targeted_attack else not bool(pred.equal(target))
        res = {"quantised_pred": pred.cpu().numpy(), "quantised_is_adversarial": is_adv}
        if export_u8 != "verdict":
            res["adv_video_u8"] = frames.cpu().numpy()
        return res

    def train_an_epoch(self, data_loaders, criterion, metric, lr):
        """``train_an_epoch`` (model.py:627-789): 'train' then 'valid' over iterables of (inputs, target, _); the valid phase
        evaluates the same loss without an update.  Result keys as model.py:780-786.  A loader may yield ``inputs`` as a LIST of whole
        uint8 videos ``[N_k,H_k,W_k,3]`` (one per clip of the batch): the train phase then cuts a clip from each with the training split's
        sampling settings (and the training transform when the engine has ``augment``), the valid phase one clip with no shift and no
        jitter (``prepare_videos``).  With ``clips_per_video = G > 1`` a batch is V = B / G whole videos (G clips are cut from each: the train
        phase with the training split's settings, the valid phase at the test split's uniform offsets) or B clips already video-major and
        sample-minor, with V labels; the fooling metric compares the adversarial with the clean VIDEO logits and ``n`` counts videos."""
        import time
        G = self.clips_per_video
        result = {}
        for phase in ("train", "valid"):
            t0 = time.time()
            n, loss_sum, miss, valid = 0, 0.0, 0.0, 0.0
            xdt = None
            for inputs, target, *_ in data_loaders[phase]:
                whole = isinstance(inputs, (list, tuple))           # whole videos: sampled and prepared in one launch
                if self.train_delivered and not whole:
                    raise ValueError("train_an_epoch: an engine built with train_delivered takes loaders of whole uint8 videos (lists of "
                                     "[N,H,W,3]); for clips at the engine's size build it with quantise_train instead")
                drawn = None
                if whole and self.train_delivered:
                    # the delivered chain: ONE draw of tables / boxes / flips serves the clean reference (the untoned preparation) and the step
                    out = self._clip_buf("_clean_buf", len(inputs) * G)
                    drawn = self._draw_video_clips(inputs, phase == "train", G, "train_an_epoch")
                    inputs = self._prepare_clips(drawn[0], out=out, boxes=drawn[2], flips=drawn[3], frame_idx=drawn[1])
                elif whole:
                    inputs = self.prepare_videos(inputs, train=(phase == "train"), num_samples=G, out=self._clip_buf("_prep_buf", len(inputs) * G))
                xdt = self._same_dtype(xdt, inputs, f"train_an_epoch ({phase})")
                augmenting = phase == "train" and self.augment is not None and not whole
                if augmenting and not self._is_raw(inputs):
                    raise ValueError("augment is set but the train clips are at the engine's size already: there is nothing to prepare "
                                     "(the training transform applies to raw uint8 frames)")
                inputs = self._prepared(inputs, train=augmenting)   # raw-size uint8 frames: this batch's clips, in the reused fp32 buffer
                clean = self.logits(inputs, False).clone()
                if drawn is not None:
                    r = self.step_videos(None, target, criterion, lr=lr, update=(phase == "train"), train=(phase == "train"), _drawn=drawn)
                else:
                    r = self.step(inputs, target, criterion, lr=lr, update=(phase == "train"))
                adv_logits = self._logits
                if G > 1:
                    clean, adv_logits = self.video_logits(clean), r["video_logits"]
                m = metric.accuracy_for_eval(adv_logits, target, topk=(1,), clean_pred=clean)
                if isinstance(m, tuple):
                    miss += float(m[0]); valid += float(m[1])
                else:                                           # targeted: a percentage (model.py:300-302)
                    miss += float(m) / 100.0 * target.numel(); valid += target.numel()
                bs = inputs.shape[0] // G
                loss_sum += float(r["loss"]) * bs
                n += bs
            p = self.pert_model.get_perturbation()[0].cpu().numpy()
            result[f"{phase}/time"] = time.time() - t0
            result[f"{phase}/loss"] = loss_sum / max(n, 1)
            result[f"{phase}/fooling_ratio"] = miss / valid if valid else float("nan")
            result[f"{phase}/pert_thickness"] = float(np.abs(p).mean())
            result[f"{phase}/pert_roughness"] = float(np.abs(np.roll(p, 1, 1) - p).mean())
            result[f"{phase}/inf_norm"] = float(np.abs(p).max())
            result[f"{phase}/perturbation"] = p
            if self.video_time:
                result[f"{phase}/flicker_period"] = self.P
        return result

    def fit(self, data_loaders, criterion, metric, lr=1e-3, epochs=1, lr_gamma=0.1, lr_step_size=None, model_dir=None,
            model_name=None, save_model=False, start_epoch=1):
        """``VideoLearnerAdversarial.fit`` (model.py:460-625) with the step-decay schedule (StepLR, model.py:571-573:
        lr_e = lr * gamma ** floor((e - start_epoch) / lr_step_size), default step = ceil(2/3 * epochs), model.py:496-497).
        Returns the list of per-epoch result dicts; ``save_model`` writes ``{model_name}_{epoch:03d}.npy`` (model.py:613-619)."""
        if lr_step_size is None:
            lr_step_size = int(np.ceil(2 / 3 * epochs))
        results = []
        for e in range(start_epoch, epochs + 1):
            lr_e = lr * lr_gamma ** ((e - start_epoch) // max(int(lr_step_size), 1))   # a fresh StepLR on every (re)start, like the reference
            res = self.train_an_epoch(data_loaders, criterion, metric, lr_e)
            res["lr"] = lr_e
            results.append(res)
            if save_model and model_dir:
                os.makedirs(model_dir, exist_ok=True)
                np.save(os.path.join(model_dir, f"{model_name or self.model_name}_{str(e).zfill(3)}.npy"), np.array(results, dtype=object),
                        allow_pickle=True)
        return results

    def _fit_many_videos_batched(self, videos, criterion, lr, model_dir, label_id_to_text, save_model, n_iter, targeted_attack, target_class_id,
                                 restart_after=3000, norm_growth=1.3, max_restarts=4, reset_optimizer_per_video=False, log_every=0, export_u8=False):
        """``fit_many_videos`` with B = batch_size videos attacked AT ONCE (engine built with ``per_clip=True``): every slot runs the loop of
        ``fit_single_video_attack`` (model.py:1056-1101: while step < n_iter or not adversarial; restart with 1.3x clamp bound, give up
        after 4) on its own video with its own perturbation / clamp bound / step counters; a finished slot takes the next video.  Per
        video the iterations are those of the one-by-one loop (bitwise in fp32 when the optimiser state is reset per video; the
        reference's single Adam instance carried from video to video, SURVEY D.5, becomes one carried state PER SLOT here)."""
        import itertools
        assert self.per_clip
        B, T = self.B, self.T
        dev = self._logits.device
        it = iter(videos)
        first = next(it, None)
        # the slot buffer keeps the videos' dtype: uint8 frames stay uint8 (decoded on the device by the apply kernel)
        xdt = self._same_dtype(None, first[0], "fit_many_videos") if first is not None else torch.float32
        it = itertools.chain([first] if first is not None else [], it)
        # raw-size uint8 frames are prepared on the device straight into their slot of an fp32 buffer
        raw = first is not None and self._is_raw(first[0])
        x = torch.zeros((B, T, self.H, self.W, 3), dtype=torch.float32 if raw else xdt, device=dev)
        labels = torch.zeros(B, dtype=torch.int64, device=dev)
        rng = np.random.default_rng(0)
        slots, out = [None] * B, {}

        def refill(b):
            while True:
                nxt = next(it, None)
                if nxt is None:
                    slots[b] = None
                    self.active[b] = 0
                    return
                inputs, target, name = nxt
                self._same_dtype(xdt, inputs, "fit_many_videos")
                dest, todo = self._open_result_file(model_dir, name, target, label_id_to_text, save_model)
                if not todo:
                    continue
                self.pert_model.init_clip(b, (rng.random(self.pert_model.size, dtype=np.float32) * 2 - 1) * 0.005)     # model.py:938-947
                if reset_optimizer_per_video:                # (pgd keeps no moments: only the counter is reset)
                    if not self.pgd:
                        self.adam_m[b].zero_(); self.adam_v[b].zero_()
                    self.adam_steps[b] = 0
                self.active[b] = 1
                if self._is_raw(inputs) != raw:
                    raise ValueError("fit_many_videos: raw-size and engine-size clips cannot be mixed in one call")
                if raw:
                    self.prepare(inputs[:1], out=x, out_offset=b)
                else:
                    x[b].copy_(inputs[0])
                labels[b] = int(target[0])
                clean = self.logits(x, False)[b:b + 1].clone()
                if int(clean.argmax(1)) != int(target[0]):
                    out[str(name)] = None                                  # model.py:1030-1032
                    continue
                slots[b] = dict(name=str(name), dest=dest, target=target.clone(), clean=clean, step=0, new_chance=0, is_adv=False,
                                hist=self._new_history())
                return

        def finish(b):
            st = slots[b]
            res = self._attack_result(st["hist"], self.pert_model.clip_perturbation_ref(b).cpu().numpy(), st["clean"], st["target"], st["new_chance"])
            # slot b's frames under its own perturbation, scored by the clean uint8 path.  The plan's batch is fixed, so the clean forward
            # runs over all B slots and row b is kept: one extra forward per finished video, off the default path
            if export_u8:
                frames = self.adversarial_frames(x)
                res.update(self._quantised_verdict(frames[b:b + 1], self.logits(frames, False)[b:b + 1], st["target"], targeted_attack, target_class_id,
                                                   export_u8))
            out[st["name"]] = res
            self._save_result(st["dest"], res, save_model)
            refill(b)

        for b in range(B):
            refill(b)
        while any(st is not None for st in slots):
            # the loop head of fit_single_video_attack, per slot (a refilled slot is checked again: its fresh state passes trivially)
            for b in range(B):
                while slots[b] is not None:
                    st = slots[b]
                    if not (st["step"] < n_iter or not st["is_adv"]):
                        finish(b)
                        continue
                    if st["step"] > restart_after:
                        st["new_chance"] += 1
                        self.pert_model.dyn_max_norm_dev[b] *= norm_growth
                        st["step"] = 0
                    if st["new_chance"] == max_restarts:
                        finish(b)
                        continue
                    break
            if not any(st is not None for st in slots):
                break
            r = self.step(x, labels, criterion, lr=lr)
            h = r.host()
            pcl = self.pert_model.clamp_perturbation().cpu().numpy()               # [B,T,3] after the update (model.py:1110-1112)
            for b, st in enumerate(slots):
                if st is None:
                    continue
                adv_class = int(h["argmax"][b])
                st["is_adv"] = (adv_class == target_class_id) if targeted_attack else (adv_class != int(st["target"][0]))
                p = pcl[b].reshape(T, 1, 1, 3).transpose(3, 0, 1, 2)      # [3,T,1,1], the memory layout get_perturbation() hands the one-by-one loop
                                                                          # (numpy's float32 mean depends on it in the last bit)
                self._record(st["hist"], st["is_adv"], h["loss"][b], h["adv_loss"][b], h["reg_loss"][b], p, h["softmax"][b].max(), h["label_prob"][b])
                if log_every and st["step"] % log_every == 0:
                    hist = st["hist"]
                    print(f"[{st['name']}] batch {st['step']} of {n_iter} | loss = {hist['loss/total'][-1]:.4f} | "
                          f"adv loss = {hist['loss/adv_loss'][-1]:.4f} | reg loss = {hist['loss/reg_loss'][-1]:.4f}", flush=True)
                st["step"] += 1
        return out

    def fit_many_videos(self, videos, criterion, lr=1e-3, model_dir=None, label_id_to_text=None, save_model=True, n_iter=3000,
                        targeted_attack=False, target_class_id=None, reset_optimizer_per_video=False, **kw):
        """``VideoLearnerAdversarial.fit_many_videos`` (model.py:791-982): one single-video attack per (inputs, target, name);
        a video whose result file already shows a success is skipped, a placeholder (None) is written before the attack, the
        perturbation restarts from U(-1,1) * 0.005 and the clamp norm from ``max_norm`` (model.py:938-947).  Result files are
        ``<name>_@<class>.npy`` (model.py:917-921).  Returns {name: result dict or None}."""
        if self.per_clip:
            return self._fit_many_videos_batched(videos, criterion, lr, model_dir, label_id_to_text, save_model, n_iter, targeted_attack,
                                                 target_class_id, reset_optimizer_per_video=reset_optimizer_per_video, **kw)
        out = {}
        rng = np.random.default_rng(0)
        xdt = None
        for inputs, target, name in videos:
            # (clips_per_video > 1: a whole uint8 video, possibly as a one-element list, goes through to fit_single_video_attack)
            xdt = self._same_dtype(xdt, inputs[0] if isinstance(inputs, (list, tuple)) and len(inputs) else inputs, "fit_many_videos")
            dest, todo = self._open_result_file(model_dir, name, target, label_id_to_text, save_model)
            if not todo:
                continue
            self.pert_model.init_perturbation(((rng.random(self.pert_model.size, dtype=np.float32) * 2 - 1) * 0.005))
            self.pert_model.dynamic_max_norm = self.pert_model.max_norm
            if reset_optimizer_per_video:                       # (the reference carries ONE Adam state from video to video, SURVEY D.5: default)
                if not self.pgd:                                # (pgd keeps no state between videos: nothing to reset)
                    self.adam_m.zero_(); self.adam_v.zero_()
                self.adam_t = 0
            res = self.fit_single_video_attack(inputs, target, criterion, lr=lr, n_iter=n_iter, targeted_attack=targeted_attack,
                                               target_class_id=target_class_id, **kw)
            out[str(name)] = res
            self._save_result(dest, res, save_model)
        return out

    @staticmethod
    def _open_result_file(model_dir, name, target, label_id_to_text, save_model):
        """the result file of one video of ``fit_many_videos`` -> ``(dest, attack)``: ``<model_dir>/<name>_@<class>.npy`` (model.py:917-921;
        None without a ``model_dir``) and whether the video is still to be attacked -- not when the file is there and shows a success or
        holds None (the clean clip was misclassified, or the run was aborted).  A file about to be written (``save_model``) gets its
        placeholder, None, before the attack"""
        cls = (label_id_to_text[int(target[0])] if label_id_to_text is not None else str(int(target[0]))).replace(" ", "_")
        if not model_dir:
            return None, True
        dest = os.path.join(model_dir, f"{os.path.basename(str(name))}_@{cls}.npy")
        if os.path.exists(dest):
            prev = np.load(dest, allow_pickle=True).tolist()
            return dest, not (prev is None or np.array(prev["is_adversarial"]).any())
        if save_model:
            os.makedirs(model_dir, exist_ok=True)
            np.save(dest, None)
        return dest, True

    @staticmethod
    def _save_result(dest, res, save_model):
        """an attack's result into its file, in the placeholder's place (a misclassified clean clip keeps the placeholder)"""
        if res is not None and dest and save_model:
            np.save(dest, dict(res, prob_clean_input=res["prob_clean_input"].cpu().numpy()), allow_pickle=True)


class VideoLearnerAdversarial(FlickerVideoResNet):
    """The reference's class name and constructor keywords (model.py:337-347: ``dataset, num_classes, base_model, sample_length,
    cyclic_pert, l_inf_pert_norm, attack_type, labaels_id_to_text`` [sic]) over the HIP engine.  ``dataset`` only supplies
    ``sample_length`` / batch size when it has them (the decord mp4 loader stays out of scope); ``weights`` = torchvision
    ``state_dict`` arrays or a ``.pth`` / ``.npz`` path (videoresnet_spec.load_weights) replaces ``pretrained=True``.
    ``.pert_model``, ``.model_name``, ``.results``, ``.fit``, ``.fit_many_videos``, ``.fit_single_video_attack`` as in the reference."""

    def __init__(self, dataset=None, num_classes=None, base_model="r2plus1d_18", sample_length=None, cyclic_pert=False, l_inf_pert_norm=0.1,
                 attack_type="flickering", labaels_id_to_text=None, weights=None, batch_size=None, optimizer="adam", **engine_kw):
        # ``engine_kw``: the other keywords of the engine alone (``image_size``, ``dtype``, ``flicker_time``, ... : FlickerVideoResNet), passed
        # on as they are -- one the engine does not know is its TypeError
        from . import videoresnet_spec as vs
        if weights is None:
            raise ValueError("weights: a torchvision state_dict ({name: array}) or a .pth / .npz path -- there is no network to download "
                             "the pretrained checkpoint the reference uses (model.py:421)")
        if sample_length is None:
            sample_length = getattr(dataset, "sample_length", 16)
        if isinstance(weights, (str, bytes)):
            weights = vs.load_weights(weights, base_model if base_model in vs.ARCHS else vs.resolve_model(base_model, sample_length)[0])
        if batch_size is None:
            batch_size = getattr(dataset, "batch_size", 1)
        super().__init__(base_model, weights, batch_size=batch_size, sample_length=sample_length, l_inf_pert_norm=l_inf_pert_norm,
                         cyclic_pert=cyclic_pert, num_classes=num_classes, attack_type=attack_type, optimizer=optimizer, **engine_kw)
        self.dataset, self.labaels_id_to_text = dataset, labaels_id_to_text
        self.results = {}
