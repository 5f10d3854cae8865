"""Generate the temporal-sampling fixture from the REFERENCE's own ``VideoDataset._sample_indices`` / ``_get_frames``.

Run in the build container only (needs /root/reference):   python tests/golden/make_sample_golden.py
Writes tests/golden/clip_sample_golden.npz.  Data only (index tables and generator probes): no reference source travels.

The two methods (utils_cv/action_recognition/dataset.py:500-586) are imported with the stub-import recipe of make_golden.py -- ``decord``,
``einops``, ``matplotlib``, ``torchvision`` and ``sklearn`` are stubbed, with classes that accept arguments because dataset.py builds a
``Compose`` when it is imported -- and called unbound on a bare object that carries the attributes they read.  The video reader is a stub
whose frames carry their own number, with the model of decord the package documents (videoresnet_spec.sample_frame_indices):
``seek_accurate(o); next()`` yields frame ``o``, ``skip_frames(k)`` advances ``k``, ``next()`` past the end raises ``StopIteration``.

Per case, under ``np.random.seed(seed)``: the table int [num_samples, sample_length] of frame numbers, and the next
``np.random.random()`` after it, which pins the generator's state and hence the number of draws made."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "clip_sample_golden.npz")
REF = "/root/reference"

FIELDS = ("num_frames", "sample_length", "sample_step", "num_samples", "temporal_jitter", "random_shift", "presample_length", "seed")


def cases():
    """(num_frames, sample_length, sample_step, num_samples, temporal_jitter, random_shift, presample_length, seed) rows"""
    rows, seed = [], 100
    for T, step in ((8, 1), (8, 2), (4, 4), (16, 1), (32, 2)):
        P = T * step
        for N in (max(P - 3, 1), P, P + 1, P + 7, 10 * P + 3):          # shorter than, equal to, one longer than, longer, much longer
            for S in (1, 3, 10):
                for jitter in (False, True):
                    for shift in (False, True):
                        seed += 1
                        rows.append((N, T, step, S, int(jitter), int(shift), P, seed))
    # the train split of split_train_test: sample_step = temporal_jitter_step = 2, presample_length left at sample_length * 1
    for T in (8, 16):
        for N in (T - 2, T, T + 1, T + 5, 2 * T, 2 * T + 1, 300):
            for S in (1, 3, 10):
                for shift in (False, True):
                    seed += 1
                    rows.append((N, T, 2, S, 1, int(shift), T, seed))
    # a one-frame video
    for T, step, S, jitter, shift in ((8, 1, 1, 0, 0), (8, 2, 3, 1, 1), (2, 4, 10, 1, 0)):
        seed += 1
        rows.append((1, T, step, S, jitter, shift, T * step, seed))
    return np.array(rows, np.int64)


def load_cases(path=OUT):
    """[{num_frames, ..., seed (ints; the two switches bools), table int64 [num_samples, sample_length], next float}]"""
    z = np.load(path)
    out = []
    flat, at = z["tables"].astype(np.int64), 0
    for k, row in enumerate(z["cases"]):
        c = {f: int(v) for f, v in zip(FIELDS, row)}
        c["temporal_jitter"], c["random_shift"] = bool(c["temporal_jitter"]), bool(c["random_shift"])
        n = c["num_samples"] * c["sample_length"]
        c["table"] = flat[at:at + n].reshape(c["num_samples"], c["sample_length"])
        at += n
        c["next"] = float(z["next"][k])
        out.append(c)
    return out


def import_reference_dataset():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Any:
        def __init__(self, *a, **k):
            pass

        def __call__(self, x):
            return x

    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms", Compose=Any)
    tv.models = stub("torchvision.models")
    tv.models.video = stub("torchvision.models.video")
    tv.models.video.resnet = stub("torchvision.models.video.resnet", VideoResNet=object)
    stub("decord", VideoReader=object)
    e = stub("einops")
    e.layers = stub("einops.layers")
    e.layers.torch = stub("einops.layers.torch", Rearrange=Any)
    mpl = stub("matplotlib")
    mpl.pyplot = stub("matplotlib.pyplot")
    sk = stub("sklearn")
    sk.metrics = stub("sklearn.metrics", accuracy_score=None)
    ip = stub("IPython")
    ip.display = stub("IPython.display")
    import utils_cv.action_recognition.dataset as d
    return d


class Frame:
    def __init__(self, n):
        self.n = n

    def asnumpy(self):
        return np.array([self.n], np.int64)


class StubReader:
    """frames carry their own number; see the module docstring for the model"""

    def __init__(self, num_frames):
        self.n, self.pos = num_frames, 0

    def __len__(self):
        return self.n

    def seek_accurate(self, o):
        self.pos = int(o)

    def skip_frames(self, k=1):
        self.pos += int(k)

    def next(self):
        if self.pos >= self.n:
            raise StopIteration
        f = Frame(self.pos)
        self.pos += 1
        return f


def main():
    d = import_reference_dataset()
    rows = cases()
    G = {"cases": rows, "fields": np.array(FIELDS)}
    nxt, flat = [], []
    for k, (N, T, step, S, jitter, shift, P, seed) in enumerate(rows.tolist()):
        ds = types.SimpleNamespace(presample_length=P, random_shift=bool(shift), num_samples=S, warning=False, sample_length=T,
                                   sample_step=step, temporal_jitter=bool(jitter))
        rec = types.SimpleNamespace(num_frames=N, path="stub")
        np.random.seed(seed)
        offsets = d.VideoDataset._sample_indices(ds, rec)
        reader = StubReader(N)
        table = np.array([[int(f[0]) for f in d.VideoDataset._get_frames(ds, reader, o)] for o in offsets], np.int64)
        nxt.append(np.random.random())
        assert table.shape == (S, T) and table.min() >= 0 and table.max() < N
        flat.append(table.reshape(-1))
    G["tables"] = np.concatenate(flat).astype(np.int16)          # the cases' tables end to end, each [num_samples, sample_length]
    G["next"] = np.array(nxt, np.float64)
    np.savez_compressed(OUT, **G)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(rows), "cases")
    for c in load_cases()[:3] + load_cases()[-3:]:
        print({f: c[f] for f in FIELDS}, c["table"].tolist(), c["next"])


if __name__ == "__main__":
    main()
