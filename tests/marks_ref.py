"""NumPy restatement of the marks contract (spec_amd/csrc/marks.hip, include/specmi.h ``specmi_draw_marks`` and
``specmi_denormalize_u8``): strips, mask blends and Pillow's wide line, applied to an (H, W, 3) uint8 frame in painter's order.
The wide line is Pillow's ``ImagingDrawWideLine`` for a convex quadrilateral reduced to a minimum and a maximum per row;
tests/test_marks_host.py pins it against the installed Pillow.  Imported by the host and the GPU tests; needs no device."""
import math

import numpy as np

STRIP, MASK, LINE = 0, 1, 2
REC = 8                     # int64 per mark: kind, r | g << 8 | b << 16, six parameters
LINE_MAX_COORD = 100000     # the end-point range pinned against Pillow
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def RU(f):
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(abs(f) + 0.5))


def RD(f):
    return int(math.ceil(f - 0.5)) if f >= 0 else -int(math.ceil(abs(f) - 0.5))


def _ru32(xx):
    """ROUND_UP on fp32 values: the + 0.5 is an fp32 addition."""
    h = np.float32(0.5)
    return np.where(xx >= 0, np.floor(xx + h), -np.floor(np.abs(xx) + h)).astype(np.int64)


def _rd32(xx):
    h = np.float32(0.5)
    return np.where(xx >= 0, np.ceil(xx - h), -np.ceil(np.abs(xx) - h)).astype(np.int64)


def line_edges(x0, y0, x1, y1, width):
    """The four edges of Pillow's wide line as (xmin, ymin, xmax, ymax, ex0, ey0, edx fp32, horizontal); the zero-length line
    is four horizontal edges on the one pixel."""
    dx, dy = x1 - x0, y1 - y0
    if dx == 0 and dy == 0:
        return [(x0, y0, x0, y0, x0, y0, np.float32(0), True)] * 4
    big, small = math.hypot(dx, dy), (width - 1) / 2.0
    rmax, rmin = RU(small) / big, RD(small) / big
    dxmin, dxmax, dymin, dymax = RD(rmin * dy), RD(rmax * dy), RU(rmin * dx), RU(rmax * dx)
    v = [(x0 - dxmin, y0 + dymax), (x1 - dxmin, y1 + dymax), (x1 + dxmax, y1 - dymin), (x0 + dxmax, y0 - dymin)]
    edges = []
    for i in range(4):
        (ax, ay), (bx, by) = v[i], v[(i + 1) % 4]
        horiz = ay == by
        edx = np.float32(0) if horiz else np.float32(bx - ax) / np.float32(by - ay)
        edges.append((min(ax, bx), min(ay, by), max(ax, bx), max(ay, by), ax, ay, edx, horiz))
    return edges


def line_spans(H, W, x0, y0, x1, y1, width):
    """-> (rows, xa, xb, hspans): the clipped span [xa, xb] of every row the non-horizontal edges reach (xa > xb: empty) and
    the clipped spans (y, xa, xb) of the horizontal edges."""
    edges = line_edges(x0, y0, x1, y1, width)
    hspans = [(e[1], max(e[0], 0), min(e[2], W - 1)) for e in edges if e[7] and 0 <= e[1] < H and e[0] <= W - 1 and e[2] >= 0]
    slanted = [e for e in edges if not e[7]]
    empty = np.zeros(0, np.int64)
    if not slanted:
        return empty, empty, empty, hspans
    ylo, yhi = max(min(e[1] for e in slanted), 0), min(max(e[3] for e in slanted), H - 1)
    if ylo > yhi:
        return empty, empty, empty, hspans
    ys = np.arange(ylo, yhi + 1, dtype=np.int64)
    lo = np.full(ys.shape, np.inf, np.float32)
    hi = np.full(ys.shape, -np.inf, np.float32)
    for (_, ymin, _, ymax, ex0, ey0, edx, _) in slanted:
        xx = (ys - ey0).astype(np.float32) * edx + np.float32(ex0)
        on = (ys >= ymin) & (ys <= ymax)
        lo = np.where(on, np.minimum(lo, xx), lo)
        hi = np.where(on, np.maximum(hi, xx), hi)
    ok = np.isfinite(lo)
    xa = np.where(ok, _ru32(np.where(ok, lo, 0)), 1)
    xb = np.where(ok, _rd32(np.where(ok, hi, 0)), 0)
    xa, xb = np.maximum(xa, 0), np.minimum(xb, W - 1)
    return ys, xa, xb, hspans


def draw_line(img, x0, y0, x1, y1, width, color):
    """Pillow's ``ImageDraw.line((x0, y0, x1, y1), fill=color, width=width)``, width >= 2, integer end points, in place."""
    H, W = img.shape[:2]
    ys, xa, xb, hspans = line_spans(H, W, x0, y0, x1, y1, width)
    for y, a, b in zip(ys.tolist(), xa.tolist(), xb.tolist()):
        if a <= b:
            img[y, a:b + 1] = color
    for y, a, b in hspans:
        if a <= b:
            img[y, a:b + 1] = color
    return img


def blend_mask(img, mask, x, y, ink):
    """Pillow's ``ImagingFill2`` with a mode L ``mask`` (mh, mw) whose top-left corner lies at (x, y), in place: per channel
    ``t = in * (255 - m) + ink * m + 128; out = ((t >> 8) + t) >> 8`` - ONE rounding of the sum, as the installed Pillow's
    ``BLEND`` does (the sum of two separately rounded MULDIV255 terms differs from it by one on general backgrounds).  A pixel
    under m == 0 keeps its value."""
    H, W = img.shape[:2]
    mh, mw = mask.shape
    xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + mw, W), min(y + mh, H)
    if xa >= xb or ya >= yb:
        return img
    m = mask[ya - y:yb - y, xa - x:xb - x].astype(np.int64)[..., None]
    dst = img[ya:yb, xa:xb]
    t = dst * (255 - m) + np.asarray(ink, np.int64).reshape(1, 1, -1) * m + 128
    out = ((t >> 8) + t) >> 8
    dst[...] = np.where(m != 0, out, dst).astype(np.uint8)
    return img


def unpack_rgb(c):
    return (int(c) & 255, (int(c) >> 8) & 255, (int(c) >> 16) & 255)


def pack_rgb(c):
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def apply_marks(img, marks, masks=None):
    """The ``marks`` (n, 8) int64 of one frame applied in order to ``img`` (H, W, 3) uint8, in place; ``masks`` the 1-D uint8
    mask buffer the mask marks index."""
    H = img.shape[0]
    for kind, rgb, p0, p1, p2, p3, p4, _ in np.asarray(marks, np.int64).reshape(-1, REC).tolist():
        c = unpack_rgb(rgb)
        if kind == STRIP:
            a, b = max(p0, 0), min(p1, H)
            if a < b:
                img[a:b] = c
        elif kind == MASK:
            blend_mask(img, np.asarray(masks[p4:p4 + p2 * p3]).reshape(p3, p2), p0, p1, c)
        elif kind == LINE:
            draw_line(img, p0, p1, p2, p3, p4, c)
        else:
            raise ValueError(f'mark kind {kind}')
    return img


def denormalize_u8(x, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """``x`` (3, h, w) fp32 -> (h, w, 3) uint8: v = (x * std + mean) * 255 in fp32, each operation rounded separately; NaN -> 0,
    v clamped to [0, 255], then truncated."""
    x = np.asarray(x, np.float32)
    s, m = np.asarray(std, np.float32).reshape(3, 1, 1), np.asarray(mean, np.float32).reshape(3, 1, 1)
    v = (x * s + m) * np.float32(255)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(255)))
    return np.ascontiguousarray(v.astype(np.uint8).transpose(1, 2, 0))
