"""flk_maxpool3d_conv1x1_eligible (csrc/pool.hip): which pool + 1x1x1 pairs the fused MaxPool3d_2a + Conv3d_2b kernels take, decided on the
host from the geometry alone -- no GPU.  The plan builder asks it once per plan; both fused entry points refuse whatever it refuses."""
import pytest


@pytest.fixture(scope="module")
def ops():
    from flickering_adversarial_video_amd import build, ops as o
    build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    return o


@pytest.mark.parametrize("frames", [32, 45])
@pytest.mark.parametrize("batch", [1, 4])
def test_takes_the_i3d_geometry(ops, frames, batch):
    """MaxPool3d_2a_3x3 over the stem's [B, T/2, 112, 112, 64] output, then Conv3d_2b_1x1 64 -> 64 (i3d.py:174-180): 64- and 90-frame clips"""
    assert ops.maxpool3d_conv1x1_eligible((batch, frames, 112, 112), 64, 64, 64, "bf16")


@pytest.mark.parametrize("why, kw", [
    ("fp32", dict(dtype="fp32")),
    ("C = 32", dict(C_=32, cin=32)),
    ("cout = 128", dict(cout=128)),
    ("odd H", dict(shape=(4, 32, 111, 112))),
    ("a (3,3,3) / 2 window", dict(k=(3, 3, 3), s=(2, 2, 2))),
    ("a mask operand", dict(has_mask=True)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_refuses(ops, why, kw):
    a = dict(shape=(4, 32, 112, 112), C_=64, cin=64, cout=64, dtype="bf16", k=(1, 3, 3), s=(1, 2, 2), has_mask=False)
    assert ops.maxpool3d_conv1x1_eligible(a["shape"], a["C_"], a["cin"], a["cout"], a["dtype"], k=a["k"], s=a["s"], has_mask=a["has_mask"])
    a.update(kw)
    assert not ops.maxpool3d_conv1x1_eligible(a["shape"], a["C_"], a["cin"], a["cout"], a["dtype"], k=a["k"], s=a["s"], has_mask=a["has_mask"]), why
