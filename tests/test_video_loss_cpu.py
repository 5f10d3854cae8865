"""The video-level loss head (flk_softmax_adv_loss_video) without a GPU: the symbol, its binding, and the host-side argument checks
that return FLK_EINVAL before any device call."""
import ctypes as C
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from flickering_adversarial_video_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def loss_args(B=4, Cn=400, **kw):
    from flickering_adversarial_video_amd import _lib
    a = _lib.LossArgs()
    a.B, a.C, a.improve_loss, a.margin, a.mean_scale = B, Cn, 1, 0.05, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def call(lib, a, G, scale, logits=8, labels=8, dlogits=8, per_video=8):
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731  (never dereferenced: every case fails a host-side check first)
    return lib.flk_softmax_adv_loss_video(C.byref(a) if a is not None else None, G, scale, p(logits), p(labels), None, None, p(dlogits),
                                          p(per_video), None)


def test_symbol_exported_and_bound(lib):
    from flickering_adversarial_video_amd import _lib, ops
    assert "flk_softmax_adv_loss_video" in _lib.EXPORTS
    fn = lib.flk_softmax_adv_loss_video
    assert fn.restype is C.c_int and len(fn.argtypes) == 10 and fn.argtypes[1] is C.c_int and fn.argtypes[2] is C.c_float
    assert callable(ops.softmax_adv_loss_video)
    src = open(os.path.join(ROOT, "include", "flicker_hip.h")).read()
    assert "int flk_softmax_adv_loss_video(const flk_loss_args* a, int G, float scale" in src


def test_null_pointers_refused(lib):
    a = loss_args()
    assert call(lib, None, 2, 1.0) == -1 and b"null" in lib.flk_last_error()
    for missing in ("logits", "labels", "dlogits", "per_video"):
        assert call(lib, a, 2, 1.0, **{missing: 0}) == -1, missing
        assert b"flk_softmax_adv_loss_video" in lib.flk_last_error() and b"null" in lib.flk_last_error()


def test_group_and_scale_arguments_refused_by_name(lib):
    assert call(lib, loss_args(B=4), 0, 1.0) == -1
    assert b"G" in lib.flk_last_error() and b">= 1" in lib.flk_last_error()
    assert call(lib, loss_args(B=4), -3, 1.0) == -1 and b"G" in lib.flk_last_error()
    assert call(lib, loss_args(B=4), 3, 1.0) == -1
    msg = lib.flk_last_error()
    assert b"B = 4" in msg and b"G = 3" in msg and b"multiple" in msg
    for bad in (0.0, -0.5, float("nan")):
        assert call(lib, loss_args(B=4), 2, bad) == -1, bad
        assert b"scale" in lib.flk_last_error()


def test_everything_the_clip_head_refuses_is_refused(lib):
    assert call(lib, loss_args(Cn=1), 2, 1.0) == -1 and b"C" in lib.flk_last_error()
    assert call(lib, loss_args(Cn=1025), 2, 1.0) == -1 and b"1024" in lib.flk_last_error()
    assert call(lib, loss_args(torch_dialect=1, targeted=1), 2, 1.0) == -1 and b"non-functional" in lib.flk_last_error()
    assert call(lib, loss_args(margin=0.0), 2, 1.0) == -1 and b"margin" in lib.flk_last_error()


def test_python_wrapper_refuses_before_touching_a_device():
    from flickering_adversarial_video_amd import ops
    with pytest.raises(ValueError, match="reduce"):
        ops.video_scale(2, "max")
    with pytest.raises(ValueError, match="clips_per_video"):
        ops.video_scale(0, "sum")
    assert ops.video_scale(4, "sum") == 1.0 and ops.video_scale(4, "mean") == 0.25 and ops.video_scale(1, "mean") == 1.0


def test_gpu_tests_are_all_marked_gpu():
    """a run without a GPU (``-m "not gpu"``) reaches none of tests/test_video_loss_gpu.py: the module imports without a device and every
    test in it carries the gpu mark"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        mod = importlib.import_module("test_video_loss_gpu")
    finally:
        sys.path.pop(0)
    marks = mod.pytestmark if isinstance(mod.pytestmark, (list, tuple)) else [mod.pytestmark]
    assert any(m.name == "gpu" for m in marks)
    tests = [n for n in dir(mod) if n.startswith("test_") and callable(getattr(mod, n))]
    assert len(tests) >= 7
