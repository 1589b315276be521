"""The ColorJitter contract (head of spec_amd/csrc/color_jitter.hip) restated in NumPy: what
torchvision's ``ColorJitter`` does to a PIL RGB image - four Pillow operations in a drawn order - byte for byte.
tests/test_color_jitter_host.py pins every function here against the installed Pillow; the GPU tests compare the kernels with
these functions and with tests/golden/color_jitter.npz.  Nothing here needs a device."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
REC = 8                                     # int32 words of a jitter record: four ids, three factors' bits, k


def luma(rgb):
    """Pillow's convert('L') of (..., 3) uint8 -> (...) uint8"""
    p = rgb.astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).astype(np.uint8)


def blend(d, v, a):
    """Pillow's Image.blend(degenerate, image, a) on uint8 arrays: t = float(d) + a * float(v - d), product and sum rounded
    to fp32 each; truncated for 0 <= a <= 1, else clamped to [0, 255] first."""
    a = np.float32(a)
    d32, v32 = np.asarray(d).astype(np.int32), np.asarray(v).astype(np.int32)
    prod = (a * (v32 - d32).astype(np.float32)).astype(np.float32)
    t = (d32.astype(np.float32) + prod).astype(np.float32)
    if 0.0 <= a <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32)))
    return out.astype(np.uint8)


def contrast_mean(rgb):
    """ImageEnhance.Contrast's grey level: int(mean of L + 0.5), the sum an exact integer, division and add in float64"""
    L = luma(rgb)
    return int(int(L.sum(dtype=np.int64)) / L.size + 0.5)


def rgb_to_hsv(rgb):
    """Pillow's convert('HSV') of (..., 3) uint8 -> (..., 3) uint8"""
    r, g, b = (rgb[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    s = cr / np.where(grey, 1, maxc).astype(np.float32)
    rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
    f64 = np.float64
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(np.float32),
                          (4.0 + gc.astype(f64) - rc.astype(f64)).astype(np.float32))).astype(np.float32)
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5))


def hsv_to_rgb(hsv):
    """Pillow's convert('RGB') of an HSV image, (..., 3) uint8 -> (..., 3) uint8.  As Pillow's C evaluates it: h * 6.0 / 255.0
    in double, f = that minus the fp32 sector, kept as fp32; fs = s / 255.0 kept as fp32; the three products in double,
    rounded half away from zero and clipped."""
    h, s, v = (hsv[..., c] for c in range(3))
    hh = h.astype(np.float64) * 6.0 / 255.0
    i = np.floor(hh)
    f = (hh - i).astype(np.float32).astype(np.float64)
    fs = (s.astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    vf = v.astype(np.float64)
    clip = lambda x: np.clip(_round_half_away(x), 0, 255).astype(np.uint8)
    p, q, t = clip(vf * (1.0 - fs)), clip(vf * (1.0 - fs * f)), clip(vf * (1.0 - fs * (1.0 - f)))
    sec = i.astype(np.int64) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.empty(hsv.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.choose(sec, [row[c] for row in table])
    grey = s == 0
    out[grey] = v[grey][:, None]
    return out


def hue_shift(rgb, k):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(k)) % 256
    return hsv_to_rgb(hsv)


def hue_k(hue):
    """torchvision's np.uint8(hue_factor * 255): truncation toward zero, then mod 256"""
    return int(np.trunc(float(hue) * 255.0)) % 256


def apply_op(rgb, op, factors, k):
    if op == BRIGHTNESS:
        return blend(np.zeros_like(rgb), rgb, factors[0])
    if op == CONTRAST:
        return blend(np.full_like(rgb, contrast_mean(rgb)), rgb, factors[1])
    if op == SATURATION:
        return blend(np.repeat(luma(rgb)[..., None], 3, axis=-1), rgb, factors[2])
    if op == HUE:
        return hue_shift(rgb, k)
    raise ValueError(f'operation {op}')


def jitter(rgb, order, factors, k):
    """One frame (H, W, 3) uint8 through the operations ``order`` (ids, -1 = none), ``factors`` = (brightness, contrast,
    saturation) and the hue shift ``k``"""
    out = np.ascontiguousarray(rgb)
    for op in order:
        if op >= 0:
            out = apply_op(out, int(op), factors, k)
    return out


def make_record(order, factors, k):
    """-> the eight int32 words of specmi_color_jitter's record"""
    ids = [int(o) for o in order] + [-1] * (4 - len(order))
    bits = np.asarray(factors, dtype=np.float32).view(np.int32)
    return np.asarray(ids + [int(b) for b in bits] + [int(k)], dtype=np.int32)


def jitter_record(rgb, rec):
    rec = np.asarray(rec, dtype=np.int32)
    return jitter(rgb, rec[:4], rec[4:7].view(np.float32), int(rec[7]))
