"""The contents and the case list the motion-compensation tests share: tests/test_codec_mc_gpu.py runs the kernel on them against the
restatement, tests/test_codec_mc_cpu.py checks (without a GPU) that their restated vectors cover what the kernel can get wrong.  Also
the view geometry across tile seams that the intra, GOP and motion-compensation view tests share (check_views_across_tile_seams)."""
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


# the geometries of the three test_source_and_destination_views: the one-tile view of each test, and the view across tile seams below
VIEW_GEOMETRIES = [(s, g) for g in ("tile", "seams") for s in SUBS]
VIEW_IDS = [s if g == "tile" else f"{s}-{g}" for s, g in VIEW_GEOMETRIES]


def check_views_across_tile_seams(ops, vs, sub, **codec_kw):
    """The second geometry of the three test_source_and_destination_views (intra, GOP, motion compensation; ``codec_kw`` is gop= and
    search=): a 70 x 133 view, which is two tiles along W with a 5-column second tile, three tile rows at 4:4:4 and two at 4:2:0 with
    a 6-row remainder.  The source lies in a 75 x 141 buffer one byte off a 4-byte boundary, so the row pitch is 423 bytes and rows take
    all four misalignments; the destination in a 0xA5-filled 74 x 139 buffer (row pitch 417) two bytes off.  5 frames through a tone table,
    with stats: output and stats bit for bit the restatement's, every guard byte still 0xA5, the bytes around the buffer unchanged."""
    import torch
    big = moving(6, 75, 141, seed=17)
    buf = torch.empty(big.size + 8, dtype=torch.uint8, device="cuda")
    whole = buf[1:1 + big.size].view(big.shape)
    whole.copy_(torch.from_numpy(big))
    src = whole[1:6, 2:72, 4:137]
    assert src.stride(1) == 423 and src.data_ptr() % 4 == (buf.data_ptr() + 1 + 75 * 423 + 2 * 423 + 12) % 4
    assert {(src.data_ptr() + r * 423) % 4 for r in range(4)} == {0, 1, 2, 3}
    tone = np.sort(np.random.RandomState(5).randint(0, 256, (1, 5, 256, 3)).astype(np.uint8), axis=2)
    exp, exp_st = vs.codec_roundtrip_host(big[1:6, 2:72, 4:137], 60, sub, tone=tone[0], stats=True, **codec_kw)
    n = 5 * 74 * 139 * 3
    dbuf = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    dwhole = dbuf[2:2 + n].view(5, 74, 139, 3)
    dst = dwhole[:, 3:73, 2:135]
    assert dst.stride(1) == 417 and dst.data_ptr() % 4 == (dbuf.data_ptr() + 2 + 3 * 417 + 6) % 4
    before = dbuf.clone()
    out, st = ops.codec_roundtrip([src], vs.Codec(60, sub, **codec_kw), tone=torch.from_numpy(tone).cuda(), stats=True, out=[dst])
    got, got_st = dst.cpu().numpy(), st[0].cpu().numpy()
    assert out[0].data_ptr() == dst.data_ptr()
    assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp)
    assert got_st.dtype == exp_st.dtype and got_st.shape == exp_st.shape and np.array_equal(got_st, exp_st), (got_st, exp_st)
    mask = torch.zeros_like(dwhole, dtype=torch.bool)
    mask[:, 3:73, 2:135] = True
    assert bool((dwhole[~mask] == 0xA5).all())
    assert torch.equal(dbuf[:2], before[:2]) and torch.equal(dbuf[2 + n:], before[2 + n:])


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
