"""The host records of the picture operations (include/specmi.h): everything ``specmi_render_views`` ... ``specmi_png_decode``
refuse that the host arrays decide, as ``ValueError`` before any device call.  The rules the operations share - rows, sides,
pitched rectangles in a slab, ranges, the two slabs, disjoint rectangles - are stated once, up front, as plain functions; the
``check_*`` of each operation follow.  Host only: numpy and the library's constants, no torch.  ``spec_amd.engine`` re-exports
the public names."""
from __future__ import annotations

import numpy as np

from . import _lib


def starts(sizes):
    """Where each of n blocks of ``sizes`` laid back to back begins: the exclusive prefix sum, int64."""
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.cumsum(sizes) - sizes


def rects_overlap(a, b) -> bool:
    """Do two byte rectangles (first byte, pitch, row bytes, rows) share a byte?  (rects_overlap of spec_amd/csrc/api.hip)"""
    if a[0] > b[0]:
        a, b = b, a
    (ao, ap, ar, ah), (bo, bp, br, bh) = a, b
    if bo >= ao + (ah - 1) * ap + ar:
        return False
    if ap == bp:
        q, c = divmod(bo - ao, ap)
        return (q < ah and c < ar) or (q + 1 < ah and c + br > ap)
    s0 = bo - ao + bp * np.arange(bh, dtype=np.int64)             # row r of b, counted from a's first byte
    e0 = s0 + br - 1
    k1, k2 = s0 // ap, np.minimum(e0 // ap, ah - 1)
    hit = lambda k: (k >= k1) & (k <= k2) & (np.maximum(s0, k * ap) <= np.minimum(e0, k * ap + ar - 1))
    return bool(((k2 - k1 >= 2) | hit(k1) | hit(k2)).any())


def byte_rects(off, pitch, W, H):
    """The (first byte, pitch, row bytes, rows) of n pitched rectangles of H rows of 3 W bytes; a single row has no next row, so
    its pitch counts as 3 W (stored_pitch of spec_amd/csrc/api.hip)."""
    return [(int(o), int(p) if h > 1 else 3 * int(w), 3 * int(w), int(h)) for o, p, w, h in zip(off, pitch, W, H)]


def first_overlap(rects):
    """The first two rectangles that share a byte, as (a, b) indices into ``rects``, or None: sorted by first byte, a rectangle
    is compared with those that start before it ends (first_overlap of spec_amd/csrc/api.hip)."""
    order = sorted(range(len(rects)), key=lambda v: rects[v][0])
    for i, a in enumerate(order):
        end = rects[a][0] + (rects[a][3] - 1) * rects[a][1] + rects[a][2]
        for b in order[i + 1:]:
            if rects[b][0] >= end:
                break
            if rects_overlap(rects[a], rects[b]):
                return a, b
    return None


def one_row_each(noun, **arrays):
    """``arrays``: name=(array, columns) of the call's record arrays -> n, the rows of the first: each is (n, columns)."""
    (first, cols), *rest = arrays.values()
    n = first.shape[0] if first.ndim == 2 else -1
    if first.ndim != 2 or first.shape[1] != cols or any(tuple(a.shape) != (n, c) for a, c in rest):
        parts = [f'{name} (n, {c})' for name, (_, c) in arrays.items()]
        raise ValueError(f'{noun}s: {", ".join(parts[:-1])} and {parts[-1]} with one row per {noun}')
    return n


MAX_RECORDS = 65535     # the records of a call are one dimension of its kernels' grids


def record_count(n, noun):
    """1 to ``MAX_RECORDS`` records per call."""
    if not 1 <= n <= MAX_RECORDS:
        raise ValueError(f'1 to {MAX_RECORDS} {noun}s per call, got {n}')


def sides(H, W, limit, noun, kind_known=True, kinds=''):
    """Every side within 1 .. ``limit`` pixels - and, for the decoders, every file of a kind (``kinds``) the library takes."""
    if ((H < 1) | (H > limit) | (W < 1) | (W > limit)).any() or not np.all(kind_known):
        raise ValueError(f'a {noun} of 1 .. {limit} pixels per side{kinds}')


def rectangles_in_slabs(H, W, *families):
    """Each family (off, pitch, slab_bytes, what, rows) of pitched rectangles of H rows of 3 W bytes: where ``rows`` is set, a
    pitch holds a row and the rectangle lies inside its slab of ``slab_bytes``.  Every pitch is looked at before any slab."""
    for _, pitch, _, _, rows in families:
        if (rows & (pitch < 3 * W)).any():
            raise ValueError('a pitch below 3 * W bytes')
    for off, pitch, slab_bytes, what, rows in families:
        if (rows & ((off < 0) | (off + (H - 1) * pitch + 3 * W > slab_bytes))).any():
            raise ValueError(f'{what} leaves the slab of {slab_bytes} bytes')


def ranges_within(first, count, total, noun, nouns):
    """Every [first, first + count) lies inside the call's ``total``."""
    if ((count < 0) | (first < 0) | (first + count > total)).any():
        raise ValueError(f'a {noun} range leaves the call\'s {total} {nouns}')


def two_slabs(in_bytes, out_bytes, in_ptr, out_ptr, name):
    """The ``name`` slab and the output slab are both there (a size of None or an address of 0: missing) and - where the
    addresses are known - share no byte."""
    if in_bytes is None or out_bytes is None or in_ptr == 0 or out_ptr == 0:
        raise ValueError(f'the {name} slab or the output slab is missing (a null pointer)')
    if in_ptr is not None and out_ptr is not None and out_ptr < in_ptr + in_bytes and in_ptr < out_ptr + out_bytes:
        raise ValueError(f'the {name} slab and the output slab overlap')


def no_shared_byte(rects, message):
    """No two of the byte rectangles share a byte; ``message`` may name the two ({0} and {1})."""
    pair = first_overlap(rects)
    if pair:
        raise ValueError(message.format(*pair))


def check_render_views(Mtot, V, F, geom, offsets, cams, in_bytes, out_bytes, rgb):
    """Every refusal of ``specmi_render_views`` (include/specmi.h) that the host arrays decide, as ``ValueError``: ``geom``
    (n, 5) [H, W, mesh0, count, flags], ``offsets`` (n, 4) [in_offset, in_pitch, out_offset, out_pitch], ``cams`` (n, 13)
    [R, fx, fy, cx, cy], the sizes of the two slabs (``in_bytes`` None: no frame slab) and ``rgb``.  -> the arrays as the
    library reads them (int32, int64, float32, float32).  Needs no device."""
    geom = np.ascontiguousarray(geom, dtype=np.int64)
    offsets, cams = np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(cams, dtype=np.float32)
    record_count(one_row_each('view', geom=(geom, 5), offsets=(offsets, 4), cams=(cams, 13)), 'view')
    if Mtot < 0 or V < 1 or F < 1:
        raise ValueError(f'{Mtot} meshes of {V} vertices and {F} faces')
    rgb = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1)
    if rgb.shape[0] != 3 or not np.isfinite(rgb).all():
        raise ValueError('rgb: three finite floats in [0, 1]')
    if out_bytes >= 1 << 32 or (in_bytes or 0) >= 1 << 32:
        raise ValueError('a slab of 4 GiB or more is beyond the kernels\' 32-bit offsets')
    H, W, mesh0, count, flags = geom.T
    in_off, in_pitch, out_off, out_pitch = offsets.T
    side, ground = (flags & _lib.RENDER_SIDE_VIEW) != 0, (flags & _lib.RENDER_GROUND_PLANE) != 0
    if (flags & ~15).any() or (ground & ~side).any():
        raise ValueError('flags: RENDER_SIDE_VIEW | RENDER_GROUND_PLANE (side view only) | RENDER_CULL | RENDER_THREAD_PER_TRIANGLE')
    if len(set((flags & _lib.RENDER_THREAD_PER_TRIANGLE).tolist())) != 1:
        raise ValueError('RENDER_THREAD_PER_TRIANGLE names the one raster launch of the call: on every view or on none')
    sides(H, W, 32768, 'view')
    ranges_within(mesh0, count, Mtot, 'mesh', 'meshes')
    if max(int(count.max()), int(count.sum())) * max(F, 3 * V) >= 1 << 31 or int((H * W).sum()) >= 1 << 31:
        raise ValueError('the views are beyond 31-bit indices (count * F, 3 * count * V, pixels)')
    if (ground & (count == 0)).any():
        raise ValueError('a ground plane needs a mesh to lie under (count == 0)')
    framed = in_off >= 0
    if (~framed & ~side).any():
        raise ValueError('an overlay needs the frame it is drawn over (in_offset < 0 is for side views)')
    if framed.any() and in_bytes is None:
        raise ValueError('a view names a frame, but there is no frame slab')
    rectangles_in_slabs(H, W, (out_off, out_pitch, out_bytes, 'an output rectangle', True), (in_off, in_pitch, in_bytes or 0, 'a frame', framed))
    if not (np.isfinite(cams).all() and (cams[:, 9:11] > 0).all()):
        raise ValueError('focal lengths must be positive and finite, the centre and R finite')
    no_shared_byte(byte_rects(out_off, out_pitch, W, H), 'the output rectangles of views {0} and {1} overlap')
    return geom.astype(np.int32), offsets, cams, rgb


def check_draw_skeletons(Mtot, J, D, bones, geom, offsets, slab_bytes, style=None):
    """Every refusal of ``specmi_draw_skeletons`` (include/specmi.h) that the host arrays decide, as ``ValueError``: ``bones``
    (NB, 2) joint indices (None or empty: no bones), ``geom`` (n, 4) [H, W, det0, count], ``offsets`` (n, 2) [byte offset, pitch],
    the size of the slab and the ``_lib.DrawStyle`` (None: the defaults).  -> the arrays as the library reads them (int32, int32,
    int64) and the style.  Needs no device."""
    geom, offsets = np.ascontiguousarray(geom, dtype=np.int64), np.ascontiguousarray(offsets, dtype=np.int64)
    bones = np.zeros((0, 2), np.int64) if bones is None else np.ascontiguousarray(bones, dtype=np.int64).reshape(-1, 2)
    record_count(one_row_each('frame', geom=(geom, 4), offsets=(offsets, 2)), 'frame')
    if J < 1 or D not in (2, 3) or Mtot < 0:
        raise ValueError(f'{Mtot} detections of {J} keypoints of {D} floats (J >= 1, D = 2 or 3)')
    NB = bones.shape[0]
    if NB and ((bones < 0) | (bones >= J)).any():
        raise ValueError(f'a bone names a joint outside [0, {J})')
    if Mtot * (J + NB) >= 1 << 31 or Mtot * J * D >= 1 << 31:
        raise ValueError('the keypoints are beyond 31-bit indices')
    style = _lib.DrawStyle() if style is None else style
    if not (0 <= style.radius <= _lib.DRAW_MAX_RADIUS and 1 <= style.thickness <= _lib.DRAW_MAX_THICKNESS):
        raise ValueError(f'radius 0 .. {_lib.DRAW_MAX_RADIUS}, thickness 1 .. {_lib.DRAW_MAX_THICKNESS}')
    if not np.isfinite(style.conf_thr):
        raise ValueError('the confidence threshold must be finite')
    H, W, det0, count = geom.T
    off, pitch = offsets.T
    sides(H, W, _lib.DRAW_MAX_SIDE, 'frame')
    ranges_within(det0, count, Mtot, 'detection', 'detections')
    rectangles_in_slabs(H, W, (off, pitch, slab_bytes, 'a frame rectangle', True))
    if int((-(-H // 32) * -(-W // 32))[count > 0].sum()) >= 1 << 31:
        raise ValueError('the frames hold 2^31 tiles of 32 x 32 pixels or more')
    no_shared_byte(byte_rects(off, pitch, W, H), 'frames {0} and {1} share a byte')
    return bones.astype(np.int32), geom.astype(np.int32), offsets, style


def check_draw_marks(geom, offsets, marks, slab_bytes, mask_bytes=0):
    """Every refusal of ``specmi_draw_marks`` (include/specmi.h) that the host arrays decide, as ``ValueError``: ``geom`` (n, 4)
    [H, W, mark0, count], ``offsets`` (n, 2) [byte offset, pitch], ``marks`` (nmarks, 8) [kind, r | g << 8 | b << 16, p0 .. p5]
    (strip: y0, y1; mask blend: x, y, mw, mh, byte offset in the mask buffer; wide line: x0, y0, x1, y1, width) and the sizes of
    the slab and of the mask buffer.  -> the arrays as the library reads them (int32, int64, int64).  Needs no device."""
    geom, offsets = np.ascontiguousarray(geom, dtype=np.int64), np.ascontiguousarray(offsets, dtype=np.int64)
    marks = np.ascontiguousarray(marks, dtype=np.int64)
    if marks.size == 0:
        marks = marks.reshape(0, _lib.MARK_REC)
    n = one_row_each('frame', geom=(geom, 4), offsets=(offsets, 2))
    if marks.ndim != 2 or marks.shape[1] != _lib.MARK_REC:
        raise ValueError(f'marks: (nmarks, {_lib.MARK_REC}) [kind, colour, p0 .. p5]')
    record_count(n, 'frame')
    nmarks = marks.shape[0]
    if nmarks >= 1 << 31:
        raise ValueError('2^31 marks or more')
    H, W, mark0, count = geom.T
    off, pitch = offsets.T
    sides(H, W, _lib.MARK_MAX_SIDE, 'frame')
    ranges_within(mark0, count, nmarks, 'mark', 'marks')
    rectangles_in_slabs(H, W, (off, pitch, slab_bytes, 'a frame rectangle', True))
    kind, rgb = marks[:, 0], marks[:, 1]
    if (~np.isin(kind, (_lib.MARK_STRIP, _lib.MARK_MASK, _lib.MARK_LINE))).any():
        raise ValueError('an unknown mark kind (MARK_STRIP, MARK_MASK, MARK_LINE)')
    if ((rgb < 0) | (rgb > 0xffffff)).any():
        raise ValueError('a colour is r | g << 8 | b << 16')
    ln, mk = marks[kind == _lib.MARK_LINE], marks[kind == _lib.MARK_MASK]
    if ((ln[:, 6] < _lib.MARK_MIN_WIDTH) | (ln[:, 6] > _lib.MARK_MAX_WIDTH)).any():
        raise ValueError(f'a line width outside {_lib.MARK_MIN_WIDTH} .. {_lib.MARK_MAX_WIDTH}')
    if (np.abs(ln[:, 2:6]) > _lib.MARK_MAX_COORD).any():
        raise ValueError(f'a line end point outside [-{_lib.MARK_MAX_COORD}, {_lib.MARK_MAX_COORD}]')
    if ((mk[:, 4:6] < 1) | (mk[:, 4:6] > _lib.MARK_MAX_MASK_SIDE)).any():
        raise ValueError(f'a mask of 1 .. {_lib.MARK_MAX_MASK_SIDE} bytes per side')
    if (np.abs(mk[:, 2:4]) > _lib.MARK_MAX_MASK_POS).any():
        raise ValueError(f'a mask position outside [-{_lib.MARK_MAX_MASK_POS}, {_lib.MARK_MAX_MASK_POS}]')
    if ((mk[:, 6] < 0) | (mk[:, 6] + mk[:, 4] * mk[:, 5] > mask_bytes)).any():
        raise ValueError(f'a mask leaves the mask buffer of {mask_bytes} bytes')
    no_shared_byte(byte_rects(off, pitch, W, H), 'frames {0} and {1} share a byte')
    return geom.astype(np.int32), offsets, marks


def check_color_jitter(geom, offsets, records, in_bytes, out_bytes, in_place):
    """Every refusal of ``specmi_color_jitter`` (include/specmi.h) that the host arrays decide, as ``ValueError``: ``geom`` (n, 2)
    [H, W], ``offsets`` (n, 4) [in_offset, in_pitch, out_offset, out_pitch], ``records`` (n, 8) int32 [four operation ids in
    application order (-1: none), the bits of the fp32 factors of brightness, contrast and saturation, the hue shift k], the sizes
    of the two slabs and whether they are the same slab.  -> the arrays as the library reads them (int32, int64, int32).  Needs no
    device."""
    geom, offsets = np.ascontiguousarray(geom, dtype=np.int64), np.ascontiguousarray(offsets, dtype=np.int64)
    records = np.ascontiguousarray(records)
    n = one_row_each('frame', geom=(geom, 2), offsets=(offsets, 4))
    if records.dtype != np.int32 or tuple(records.shape) != (n, _lib.JITTER_REC):
        raise ValueError(f'records: (n, {_lib.JITTER_REC}) int32 [four ids, three fp32 factors as bits, k]')
    record_count(n, 'frame')
    H, W = geom.T
    in_off, in_pitch, out_off, out_pitch = offsets.T
    sides(H, W, _lib.JITTER_MAX_SIDE, 'frame')
    rectangles_in_slabs(H, W, (in_off, in_pitch, in_bytes, 'a frame rectangle', True), (out_off, out_pitch, out_bytes, 'an output rectangle', True))
    if in_place and ((in_off != out_off) | ((in_pitch != out_pitch) & (H > 1))).any():
        raise ValueError('in place, but an output rectangle is not its input rectangle')
    ids = records[:, :4]
    if ((ids < -1) | (ids > 3)).any():
        raise ValueError('an operation id outside [-1, 3]')
    if any((ids == op).sum(axis=1).max() > 1 for op in range(4)):
        raise ValueError('an operation is named twice')
    factors = records[:, 4:7].view(np.float32)
    if not (np.isfinite(factors).all() and (factors >= 0).all()):
        raise ValueError('a factor is negative or not finite')
    if ((records[:, 7] < 0) | (records[:, 7] > 255)).any():
        raise ValueError('a hue shift outside [0, 255]')
    if int((-(-H // 16) * -(-W // 256)).sum()) >= 1 << 31:
        raise ValueError('the frames hold 2^31 tiles of 256 x 16 pixels or more')
    no_shared_byte(byte_rects(out_off, out_pitch, W, H), 'frames {0} and {1} share an output byte')
    return geom.astype(np.int32), offsets, records


def jpeg_capacity(H, W) -> int:
    """The room ``Engine.jpeg_encode`` gives an (H, W) picture at first: its raw size and 1 KiB for the header."""
    return 3 * int(H) * int(W) + 1024


def png_bound(H, W) -> int:
    """``specmi_png_bound``: the length no file of ``Engine.png_encode`` for an (H, W) picture exceeds.  Host only."""
    out = np.zeros(1, np.int64)
    if _lib.load().specmi_png_bound(int(H), int(W), out.ctypes.data_as(_lib.c_int64_p)) != _lib.OK:
        raise ValueError(f'a picture of {H} x {W}: 1 .. 32768 pixels per side')
    return int(out[0])


def encode_pictures(geom, offsets):
    """What ``check_jpeg_encode`` and ``check_png_encode`` refuse alike, each part where both refuse it: the arrays' shapes and
    the number of pictures -> geom, offsets (int64)."""
    geom, offsets = np.ascontiguousarray(geom, dtype=np.int64), np.ascontiguousarray(offsets, dtype=np.int64)
    record_count(one_row_each('picture', geom=(geom, 2), offsets=(offsets, 4)), 'picture')
    return geom, offsets


def encode_places(geom, offsets, in_bytes, out_bytes, in_ptr, out_ptr, min_cap, min_cap_what):
    """The same for the two slabs and every picture's geometry, rectangle in the picture slab and room in the output slab,
    ``min_cap`` bytes (``min_cap_what``) at least -> H, W, out_off, cap."""
    two_slabs(in_bytes, out_bytes, in_ptr, out_ptr, 'picture')
    H, W = geom.T
    in_off, in_pitch, out_off, cap = offsets.T
    sides(H, W, 32768, 'picture')
    rectangles_in_slabs(H, W, (in_off, in_pitch, in_bytes, 'a picture rectangle', True))
    if (cap < min_cap).any():
        raise ValueError(f'a capacity below {min_cap_what} {min_cap} bytes')
    if (out_off < 0).any() or (out_off + cap > out_bytes).any():
        raise ValueError(f'an output leaves the slab of {out_bytes} bytes')
    return H, W, out_off, cap


def encode_outputs_disjoint(out_off, cap):
    """The same after the pictures: no two outputs share a byte - each is one row of ``cap`` bytes."""
    no_shared_byte([(int(o), int(c), int(c), 1) for o, c in zip(out_off, cap)], 'two outputs share a byte')


def check_jpeg_encode(geom, offsets, in_bytes, out_bytes, quality, in_ptr=None, out_ptr=None):
    """Every refusal of ``specmi_jpeg_encode`` (include/specmi.h) that the host arrays decide, as ``ValueError``: ``geom`` (n, 2)
    [H, W], ``offsets`` (n, 4) [in_offset, in_pitch, out_offset, out_capacity], the sizes of the two slabs, the quality and -
    where known - the slabs' addresses (None for either: a missing slab).  -> the arrays as the library reads them (int32,
    int64).  Needs no device."""
    geom, offsets = encode_pictures(geom, offsets)
    if not (isinstance(quality, (int, np.integer)) and 1 <= quality <= 100):
        raise ValueError(f'quality {quality!r}: an integer in 1 .. 100')
    H, W, out_off, cap = encode_places(geom, offsets, in_bytes, out_bytes, in_ptr, out_ptr, _lib.JPEG_HEADER_BYTES, 'the header\'s')
    if int((-(-H // 16) * -(-W // 16)).sum()) > 1 << 24:
        raise ValueError('the pictures hold more than 2^24 blocks of 16 x 16 pixels')
    encode_outputs_disjoint(out_off, cap)
    return geom.astype(np.int32), offsets


def check_png_encode(geom, offsets, in_bytes, out_bytes, in_ptr=None, out_ptr=None):
    """Every refusal of ``specmi_png_encode`` (include/specmi.h) that the host arrays decide, as ``ValueError``: ``geom`` (n, 2)
    [H, W], ``offsets`` (n, 4) [in_offset, in_pitch, out_offset, out_capacity], the sizes of the two slabs and - where known - the
    slabs' addresses (None for either: a missing slab).  -> the arrays as the library reads them (int32, int64).  Needs no device."""
    geom, offsets = encode_pictures(geom, offsets)
    H, W, out_off, cap = encode_places(geom, offsets, in_bytes, out_bytes, in_ptr, out_ptr, _lib.PNG_OVERHEAD_BYTES, 'the fixed overhead of')
    stream = H * (1 + 3 * W)
    segments = -(-stream // 32768)
    if (6 + stream + 5 * segments >= 1 << 31).any():
        raise ValueError('a picture whose zlib stream may not fit one IDAT chunk (2^31 bytes)')
    if int(segments.sum()) > 1 << 23:
        raise ValueError('the pictures\' filtered streams hold more than 2^23 segments of 32768 bytes')
    encode_outputs_disjoint(out_off, cap)
    return geom.astype(np.int32), offsets


def decode_files(ranges, geom, outs, in_bytes, out_bytes, in_ptr, out_ptr, item):
    """What ``check_jpeg_decode`` and ``check_png_decode`` refuse alike before they look at the pictures: the arrays' shapes, the
    number of files, the two slabs and every file's range in the input slab, which holds one ``item`` ('file', 'stream') per
    file -> ranges, geom, outs (int64)."""
    ranges, geom, outs = (np.ascontiguousarray(x, dtype=np.int64) for x in (ranges, geom, outs))
    record_count(one_row_each('file', ranges=(ranges, 2), geom=(geom, 3), outs=(outs, 2)), 'file')
    two_slabs(in_bytes, out_bytes, in_ptr, out_ptr, item)
    off, length = ranges.T
    if (off < 0).any() or (length < 0).any() or (off + length > in_bytes).any():
        raise ValueError(f'a {item} leaves the slab of {in_bytes} bytes')
    return ranges, geom, outs


def decode_pictures(geom, outs, out_bytes, kinds, kinds_what):
    """The same for the pictures: sides, the third column of ``geom`` among ``kinds`` (``kinds_what``), pitches and rectangles
    in the output slab -> H, W, the third column."""
    H, W, kind = geom.T
    out_off, pitch = outs.T
    sides(H, W, 32768, 'picture', np.isin(kind, kinds), f', {kinds_what} (a file the probe refuses?)')
    rectangles_in_slabs(H, W, (out_off, pitch, out_bytes, 'a picture rectangle', True))
    return H, W, kind


def decode_rectangles_disjoint(geom, outs):
    """The same after the format's own bounds: no two pictures share a byte."""
    no_shared_byte(byte_rects(outs[:, 0], outs[:, 1], geom[:, 1], geom[:, 0]), 'two picture rectangles share a byte')


def check_jpeg_decode(ranges, geom, outs, in_bytes, out_bytes, in_ptr=None, out_ptr=None):
    """Every refusal of ``specmi_jpeg_decode`` (include/specmi.h) that the host arrays decide, as ``ValueError``: ``ranges`` (n, 2)
    [offset, length] of the files in the input slab, ``geom`` (n, 3) [H, W, sampling (420 or 444)] as the probe gave them,
    ``outs`` (n, 2) [offset, pitch] of the pictures in the output slab, the sizes of the two slabs and - where known - their
    addresses (None for either: a missing slab).  -> ranges and outs as the library reads them (int64).  Needs no device."""
    ranges, geom, outs = decode_files(ranges, geom, outs, in_bytes, out_bytes, in_ptr, out_ptr, 'file')
    H, W, sampling = decode_pictures(geom, outs, out_bytes, (420, 444), 'sampled 420 or 444')
    mcu = np.where(sampling == 420, 16, 8)
    if int((-(-H // mcu) * -(-W // mcu)).sum()) > 1 << 24:
        raise ValueError('the files hold more than 2^24 MCUs')
    decode_rectangles_disjoint(geom, outs)
    return ranges, outs


PNG_BPP = {0: 1, 2: 3, 4: 2, 6: 4}      # bytes per pixel of the colour types specmi_png_decode takes


def check_png_decode(ranges, geom, outs, in_bytes, out_bytes, in_ptr=None, out_ptr=None, raw_bytes=None):
    """Every refusal of ``specmi_png_decode`` (include/specmi.h) as ``ValueError``: ``ranges`` (n, 2) [offset, length] of the zlib
    streams in the input slab, ``geom`` (n, 3) [H, W, colour type] as the probe gave them, ``outs`` (n, 2) [offset, pitch] of the
    pictures in the output slab, the sizes of the two slabs and - where known - their addresses (None for either: a missing
    slab); ``raw_bytes``: the size of the optional raw output.  -> (ranges int64, geom int32, outs int64, the bytes ``raw``
    needs).  Needs no device."""
    ranges, geom, outs = decode_files(ranges, geom, outs, in_bytes, out_bytes, in_ptr, out_ptr, 'stream')
    if (ranges[:, 1] < 8).any():
        raise ValueError('a zlib stream shorter than 8 bytes')
    H, W, ctype = decode_pictures(geom, outs, out_bytes, tuple(PNG_BPP), 'colour type 0, 2, 4 or 6')
    bpp = np.array([PNG_BPP[int(c)] for c in ctype], np.int64)
    need = int(((H * (1 + W * bpp) + 255) // 256 * 256).sum())
    if need > 1 << 31:
        raise ValueError('the files\' inflated streams hold more than 2^31 bytes')
    if raw_bytes is not None and raw_bytes < need:
        raise ValueError(f'the raw output holds {raw_bytes} bytes, these files\' inflated streams take {need}')
    decode_rectangles_disjoint(geom, outs)
    return ranges, geom.astype(np.int32), outs, need
