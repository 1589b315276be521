"""Test-side references of the three kernels hrnet.hip adds to the conv kernels (the 3-channel stem, the exchange-unit sum,
the align_corners resize), in plain NumPy float64: no torch, nothing of the code under test.  tests/test_hrnet_ref_host.py
checks them against torch and against oracle/hrnet.py; tests/test_gpu_hrnet_kernels.py compares the device with them.

Layouts are the kernels': the image NCHW (B,3,H,W), everything else NHWC (B,H,W,C); weights OIHW (64,3,3,3)."""
import numpy as np

F64 = np.float64


def conv_out(n):
    """Output size of a 3x3 / stride 2 / pad 1 convolution."""
    return (n - 1) // 2 + 1


def _stem_acc(x, w):
    """float64 (B,OH,OW,64): sum over the 27 taps of w[co,c,ky,kx] * x[b,c,2oy-1+ky,2ox-1+kx], zero outside the image."""
    x, w = np.asarray(x, dtype=F64), np.asarray(w, dtype=F64)
    B, C, H, W = x.shape
    assert C == 3 and w.shape == (64, 3, 3, 3)
    OH, OW = conv_out(H), conv_out(W)
    xp = np.zeros((B, 3, 2 * OH + 1, 2 * OW + 1), dtype=F64)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    acc = np.zeros((B, OH, OW, 64), dtype=F64)
    for c in range(3):
        for ky in range(3):
            for kx in range(3):
                tap = xp[:, c, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]                 # (B,OH,OW)
                acc += tap[..., None] * w[:, c, ky, kx]
    return acc


def stem3x3(x, w, scale, shift):
    """ReLU(conv3x3 / stride 2 / pad 1 (x, w) * scale + shift) of the NCHW image, as (B,OH,OW,64) float64."""
    return np.maximum(_stem_acc(x, w) * np.asarray(scale, dtype=F64) + np.asarray(shift, dtype=F64), 0.0)


def stem3x3_abs(x, w):
    """sum |w| |x| over the taps of every output, (B,OH,OW,64): what a rounding-error bound of the stem scales with."""
    return _stem_acc(np.abs(np.asarray(x, dtype=F64)), np.abs(np.asarray(w, dtype=F64)))


def upsample_nearest(t, sh):
    """(B,h,w,C) -> (B, h << sh, w << sh, C): every pixel repeated 2^sh times along both axes (nn.Upsample(mode='nearest'))."""
    t = np.asarray(t)
    return t if sh == 0 else np.repeat(np.repeat(t, 1 << sh, axis=1), 1 << sh, axis=2)


def _fuse(terms, sh, relu, dtype):
    assert 1 <= len(terms) <= 4 and len(sh) == len(terms)
    y = upsample_nearest(np.asarray(terms[0], dtype=dtype), sh[0])
    for t, s in zip(terms[1:], sh[1:]):
        y = y + upsample_nearest(np.asarray(t, dtype=dtype), s)             # ((t0 + t1) + t2) + t3: one rounding per addition
        assert y.dtype == dtype
    return np.maximum(y, dtype(0)) if relu else y


def fuse_sum(terms, sh, relu):
    """[ReLU](((t0 + t1) + t2) + t3) in float64, term k (B, H >> sh[k], W >> sh[k], C) nearest-upsampled by 2^sh[k]."""
    return _fuse(terms, sh, relu, F64)


def fuse_sum_f32(terms, sh, relu):
    """The same sum with every addition rounded to float32, in the stated order: what the device must equal bit for bit."""
    return _fuse(terms, sh, relu, np.float32)


def _axis(n_in, n_out):
    """Source taps of one axis under align_corners=True: (i0, i1, weight of i1), coordinate o * (n_in - 1) / (n_out - 1), 0 if n_out == 1."""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    f = np.arange(n_out, dtype=F64) * scale
    i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, f - i0


def resize_ac(x, OH, OW):
    """F.interpolate(mode='bilinear', align_corners=True) of x (B,H,W,C) NHWC to (B,OH,OW,C), float64."""
    x = np.asarray(x, dtype=F64)
    _, H, W, _ = x.shape
    y0, y1, ly = _axis(H, OH)
    x0, x1, lx = _axis(W, OW)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = (1.0 - lx) * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
    bot = (1.0 - lx) * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
    return (1.0 - ly) * top + ly * bot


def is_exact_in_f32(a):
    """Does the float64 array survive the round trip through float32 unchanged?"""
    a = np.asarray(a, dtype=F64)
    return bool(np.all(a.astype(np.float32).astype(F64) == a))


# ---- the cases of tests/test_gpu_hrnet_kernels.py (stated here so that the host test can check every "exact" one is exact) ---------
# (B, H, W) of the stem: single pixels and rows, odd and even sizes, B*OH*OW == 64 (one full block) and == 65 (one pixel more)
STEM_SHAPES = [(1, 1, 1), (1, 2, 2), (1, 1, 5), (1, 5, 1), (1, 5, 7), (1, 6, 8), (3, 32, 32), (2, 33, 47), (1, 16, 16), (1, 10, 26)]
STEM_SCALES = (0.5, 1.0, 2.0)


def stem_integer_operands(B, H, W, seed):
    """Integer operands for which every fp32 partial sum of the stem is exact: image borders +-8 (loud), interior in [-1, 1]
    (quiet: a border tap that is read through a clamped coordinate but not zeroed changes the sum), weights in [-4, 4], scale
    from {0.5, 1, 2}, shift integers in [-3, 3].  |acc| <= 27 * 8 * 4 = 864."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, 2, (B, 3, H, W)).astype(F64)
    loud = lambda shape: rng.choice([-8.0, 8.0], shape)
    x[:, :, 0, :], x[:, :, -1, :] = loud((B, 3, W)), loud((B, 3, W))
    x[:, :, :, 0], x[:, :, :, -1] = loud((B, 3, H)), loud((B, 3, H))
    w = rng.integers(-4, 5, (64, 3, 3, 3)).astype(F64)
    scale = np.asarray(STEM_SCALES)[rng.integers(0, 3, 64)]
    shift = rng.integers(-3, 4, 64).astype(F64)
    return x, w, scale, shift


# per-axis (in -> out) sizes of the resize whose scale (in - 1) / (out - 1) is an integer or a half-integer (0 where out == 1): the
# 'interp' head's geometries of trunk inputs 32, 64 and 96.  Paired so that H and W differ within a case.
RESIZE_EXACT_AXES = [(1, 1), (2, 1), (4, 1), (8, 1), (8, 2), (16, 2), (4, 2), (24, 3), (12, 3), (6, 3), (3, 3)]
_AXIS_PAIRS = [(RESIZE_EXACT_AXES[i], RESIZE_EXACT_AXES[(i + 4) % 11]) for i in range(11)] + [((8, 1), (4, 1)), ((24, 3), (12, 3)), ((16, 2), (8, 2))]
RESIZE_EXACT_CASES = [((h, w), (oh, ow)) for (h, oh), (w, ow) in _AXIS_PAIRS]          # ((H, W), (OH, OW))
# ((H, W), (OH, OW)) whose scale is not dyadic
RESIZE_BOUNDED_CASES = [((56, 56), (7, 7)), ((28, 42), (7, 7)), ((32, 20), (4, 5)), ((14, 14), (7, 7))]


def resize_integer_input(B, H, W, C, seed, amp=64):
    """Integers in [-amp, amp] as float64 (B,H,W,C): a wrong neighbour is an O(1) error."""
    return np.random.default_rng(seed).integers(-amp, amp + 1, (B, H, W, C)).astype(F64)
