"""Data-gradient of a strided convolution as stride-1 convolutions over parity classes -- TEST INFRASTRUCTURE, see
oracle/__init__.py.

Restated from the formula, independently of ``flk_net::pack_generic`` (csrc/net.cpp), so that the tests can drive
``flk_conv3d`` through the class operators themselves and compare the union with torch autograd.

Forward, per axis (kernel k, stride s, symmetric pad p):   y[o] = sum_kk x[o*s - p + kk] . w[kk]
Data-gradient:            gx[i] = sum_{kk : (i + p - kk) % s == 0} G[(i + p - kk) / s] . w[kk]^T
The input cells i = o*s + c of one class c in [0, s) all use the same taps, {kk : (c + p - kk) % s == 0}; taken in DESCENDING kk
their offsets into G, (c + p - kk) / s, ascend by one per tap: a stride-1 convolution over G with a box of those taps and
pad-before = -(first offset), written to the cells o*s + c of gx.  A class without taps in some axis gets no gradient from the
layer (nobody writes its cells); a class whose cells lie outside the input (ceil((n - c) / s) <= 0) does not exist.
"""
import itertools

import numpy as np


def axis_class(k, s, p, c):
    """one axis: (taps of class c in descending order, pad-before of the class operator); ([], 0) when the class has no tap"""
    taps = [kk for kk in range(k - 1, -1, -1) if (c + p - kk) % s == 0]
    if not taps:
        return taps, 0
    return taps, -((c + p - taps[0]) // s)


def classes(k, s, pad, in_dims, w=None):
    """Parity classes of the data-gradient of conv3d(kernel k, stride s, symmetric padding pad) over an input of extents in_dims
    (all (t, h, w) triples).  Per non-empty class a dict:
      offset  (ct, ch, cw)          the class; its cells of the gradient are o * s + offset
      grid    (nt, nh, nw)          logical output grid, ceil((n - c) / s) per axis
      pad     pad-before of the stride-1 class operator over the output gradient G
      taps    (kts, khs, kws)       the forward taps of each axis the operator's box holds, in box order
      w       [len(kts), len(khs), len(kws), cout, cin]   only with ``w`` ([kt,kh,kw,cin,cout], DHWIO): the box's weights with the two
              channel axes swapped -- DHWIO of the operator G (cout channels) -> gx (cin channels), i.e. already transposed
    """
    if w is not None:
        w = np.asarray(w)
        assert w.shape[:3] == tuple(k)
    out = []
    for off in itertools.product(*(range(ss) for ss in s)):
        per_axis = [axis_class(kk, ss, pp, c) for kk, ss, pp, c in zip(k, s, pad, off)]
        grid = tuple(-(-(n - c) // ss) for n, ss, c in zip(in_dims, s, off))
        if any(not taps for taps, _ in per_axis) or min(grid) <= 0:
            continue
        taps = tuple(t for t, _ in per_axis)
        cls = dict(offset=tuple(off), grid=grid, pad=tuple(pb for _, pb in per_axis), taps=taps)
        if w is not None:
            cls["w"] = np.ascontiguousarray(w[np.ix_(*taps)].swapaxes(3, 4))
        out.append(cls)
    return out


def out_dims(k, s, pad, in_dims):
    """extents of the forward output (torch: floor((n + 2p - k) / s) + 1)"""
    return tuple((n + 2 * p - kk) // ss + 1 for n, kk, ss, p in zip(in_dims, k, s, pad))
