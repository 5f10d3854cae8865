"""The contents and the case list the motion-compensation tests share: tests/test_codec_mc_gpu.py runs the kernel on them against the
restatement, tests/test_codec_mc_cpu.py checks (without a GPU) that their restated vectors cover what the kernel can get wrong."""
import numpy as np

SUBS = ("444", "420")
# one macroblock (every displaced read is clamped); a partial macroblock at 4:4:4; less than one tile; 2 x 2 tiles at 4:2:0 and at 4:4:4
SIZES = ((16, 16), (40, 56), (90, 82), (66, 130), (34, 130))
# (content, quality, gop, search): every size x subsampling runs all of them on a video of 1 and one of 7 frames in one call
COMBOS = (("moving", 75, 3, 7), ("pan", 50, 7, 15), ("stripes", 75, 12, 7), ("moving", 1, 2, 1), ("pan", 100, 7, 4), ("flat", 50, 2, 15),
          ("pan", 75, 12, 7), ("moving", 50, 3, 15))
PANS = {1: (1, -1), 4: (4, -3), 7: (-7, 2), 15: (-6, 15)}          # the pan of a "pan" case, by its search range: (dy, dx) per frame


def moving(N, H, W, seed):
    """smooth luminance and chroma plus noise, drifting from frame to frame (the contents of the GOP tests)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for n in range(N):
        img = np.stack([128 + 70 * np.sin(xx / 9. + n / 3.) + 40 * np.cos(yy / 5.), 120 + 60 * np.cos(xx / 13. + yy / 7. - n / 4.),
                        100 + 80 * np.sin(yy / 11. + n / 5.) - 30 * np.cos(xx / 4.)], -1) + rng.normal(0, 6, (H, W, 3))
        out.append(np.clip(np.rint(img), 0, 255))
    return np.stack(out).astype(np.uint8)


def texture(H, W, seed):
    """a smooth coloured texture with Gaussian noise of sigma 6 (with weaker noise -- uniform +-6 was tried -- the quantisation error of a
    quality-50 reference outweighs the texture in some interior macroblocks, and the search no longer finds every pan)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 70 * np.sin(xx / 9.) + 40 * np.cos(yy / 5.), 120 + 60 * np.cos(xx / 13. + yy / 7.),
                    100 + 80 * np.sin(yy / 11.) - 30 * np.cos(xx / 4.)], -1) + rng.normal(0, 6, (H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def pan(N, H, W, vy, vx, seed=1):
    """a window on one texture that moves by (vy, vx) pixels per frame: frame n shows at (y, x) what frame n - 1 shows at
    (y + vy, x + vx), so the vector that finds a block in the previous frame is the pan"""
    m = (N - 1) * max(abs(vy), abs(vx), 1)
    tex = texture(H + 2 * m, W + 2 * m, seed)
    return np.stack([tex[m + n * vy:m + n * vy + H, m + n * vx:m + n * vx + W] for n in range(N)])


def stripes(N, H, W, step=3):
    """vertical stripes of period 8, moved by ``step`` columns per frame: many vectors tie, the visiting order decides"""
    x = np.arange(W)
    return np.stack([np.repeat(np.broadcast_to(64 + 128 * (((x + n * step) % 8) < 4), (H, W))[..., None], 3, -1) for n in range(N)]).astype(np.uint8)


def flat(N, H, W, grey=160):
    return np.full((N, H, W, 3), grey, np.uint8)


def case_videos(content, size, search):
    """the two videos (1 frame, 7 frames) of a case"""
    H, W = size
    if content == "moving":
        return [moving(1, H, W, seed=H + W), moving(7, H, W, seed=H * 1000 + W)]
    if content == "pan":
        return [pan(1, H, W, *PANS[search]), pan(7, H, W, *PANS[search], seed=H + W)]
    if content == "stripes":
        return [stripes(1, H, W), stripes(7, H, W)]
    return [flat(1, H, W), flat(7, H, W)]
