"""The demo's pictures: the mesh overlay and the side view rasterised on the device (``specmi_render_meshes``,
spec_amd/csrc/render.hip) and the three-panel image the reference writes per detection
(``spec/utils/renderer_cam.py:147-218 render_image_group``, called from ``spec/tester.py:191-201`` and ``spec/trainer.py:366-``).

What is exact and what is this project's own: the geometry (the x flip of the translation, the 180 / 270 degree turns, the camera
pose and pyrender's intrinsics) is the reference's, and coverage and visibility follow a contract that is reproducible bit for
bit (tests/render_ref.py).  The look is NOT pyrender's: shading is ``rgb * min(1, 0.3 + 0.7 max(0, n.l))``, the side view's
ground plane is an analytic two-grey checker of 0.5 m tiles (the reference's ``get_checkerboard_plane`` lives in the un-vendored
``pare``), the colour table below is a stand-in for ``pare``'s ``get_colors`` and there is no alpha blending.  Triangles that
reach behind the near plane (z <= 0.05) are dropped, not clipped.  The horizon line and its caption are drawn exactly as
``camcalib/vis_utils.py:63-110`` does: on the host with Pillow (``show_horizon_line``), or - the ``panel0_device`` route - on the
device by ``specmi_draw_marks`` (spec_amd/csrc/marks.hip; ``horizon_marks``, ``show_horizon_lines``), byte for byte the same.

The 2D keypoint skeleton (``render_image_group(keypoints_2d=...)``, ``draw_skeleton``) is painted on the device by
``specmi_draw_skeletons`` (spec_amd/csrc/draw.hip).  ``pare.utils.vis_utils.draw_skeleton``, ``kp_utils.get_spin_skeleton`` and
``cv2`` are not vendored: which pixels a joint's disc and a bone cover, the bone table (``constants.SKELETON_SPIN``) and the
colours (green joints, bones alternately blue and red) are this project's own contract, exact and reproducible bit for bit
(tests/draw_ref.py) - cv2's look is not claimed.  The skeleton is drawn OVER the finished panel 0, where the reference draws it
before the horizon line and caption: the two differ only where a bone or joint crosses the line or the caption strip."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

# stand-ins for pare.utils.vis_utils.get_colors() (RGB, 0 .. 255)
COLORS = {'pinkish': (204, 128, 153), 'pink': (230, 153, 179), 'gray': (166, 166, 166), 'grey': (166, 166, 166), 'white': (255, 255, 255),
          'light_blue': (166, 191, 230), 'green': (128, 204, 128)}


def _rgb(color):
    c = COLORS[color] if isinstance(color, str) else color
    c = np.asarray(c, np.float32).reshape(3)
    return c / 255.0 if c.max() > 1.0 else c


_faces_cache = {}


def device_faces(faces, device) -> torch.Tensor:
    """``faces`` (None = the body model's table, ``assets.faces()``) as an (F, 3) int32 tensor on ``device``; the model's table is
    uploaded once per device."""
    if isinstance(faces, torch.Tensor):
        return faces.to(device=device, dtype=torch.int32).contiguous()
    if faces is not None:
        return torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).to(device)
    from . import assets
    table = assets.faces()
    key = (id(table), str(device))
    if key not in _faces_cache:
        _faces_cache.clear()
        _faces_cache[key] = (table, torch.from_numpy(table).to(device))
    return _faces_cache[key][1]


def render_overlay(frame_u8, vertices, cam_t, R, focal, center, faces=None, color='pinkish', side_view=False, ground_plane=False,
                   cull=True, engine=None, maps=False):
    """The meshes ``vertices`` (M, V, 3) - or one mesh (V, 3) - with translations ``cam_t`` (M, 3) drawn over ``frame_u8``
    (H, W, 3) uint8 as ``render_overlay_image`` places them (renderer_cam.py:74-117): camera rotation ``R`` (3, 3), ``focal`` =
    (fx, fy), ``center`` = (cx, cy).  ``side_view``: the 270 degree turn about y on a black background, ``ground_plane`` adds the
    checker plane to it.  Everything stays on the device: -> (H, W, 3) uint8 tensor (``maps``: the dict of
    ``Engine.render_meshes``).  There is no host path."""
    from . import cam_utils
    if not isinstance(frame_u8, torch.Tensor) or frame_u8.device.type != 'cuda':
        raise ValueError('frame_u8 must be a device tensor: the renderer has no host path')
    dev = frame_u8.device
    eng = engine or cam_utils._engine(dev)
    as_f32 = lambda x: torch.as_tensor(x).to(device=eng.device, dtype=torch.float32).contiguous()
    vertices, cam_t, R = as_f32(vertices), as_f32(cam_t), as_f32(R)
    if vertices.dim() == 2:
        vertices, cam_t = vertices[None], cam_t.reshape(1, 3)
    flags = ((_lib.RENDER_SIDE_VIEW if side_view else 0) | (_lib.RENDER_GROUND_PLANE if ground_plane else 0) | (_lib.RENDER_CULL if cull else 0))
    return eng.render_meshes(vertices, device_faces(faces, eng.device), cam_t, R, focal, center, frame=frame_u8.contiguous(),
                             rgb=_rgb(color), flags=flags, maps=maps)


def show_horizon_line(image, vfov, pitch, roll, focal_length=-1, color=(0, 255, 0), width=5, debug=False, GT=False, text_size=16):
    """``camcalib/vis_utils.py:63-110`` on the host with Pillow: the horizon of a camera with (vfov, pitch, roll) in radians as a
    line across ``image`` (H, W, 3), with ``debug`` a black caption strip of ``text_size`` rows (top, or bottom for ``GT``) and
    the angles in degrees in Pillow's default font.  -> (uint8 image, horizon height as a fraction of H)."""
    from PIL import Image, ImageDraw
    image = np.array(image)
    h, w = image.shape[:2]
    if image.dtype in (np.float32, np.float64):
        image = image.astype('uint8')
    if debug:
        strip = slice(h - text_size, h) if GT else slice(0, text_size)
        image[strip, :, :] = 0
    im = Image.fromarray(image)
    draw = ImageDraw.Draw(im)
    ctr = h * (0.5 - 0.5 * np.tan(pitch) / np.tan(vfov / 2))
    left, right = ctr - w * np.tan(roll) / 2, ctr + w * np.tan(roll) / 2
    if debug:
        caption = 'vfov:{0:.1f}, pitch:{1:.1f}, roll:{2:.1f}, f_pix:{3:.1f}'.format(np.degrees(vfov), np.degrees(pitch), np.degrees(roll), focal_length)
        draw.text((0, h - text_size) if GT else (0, 0), ('GT: ' if GT else '') + caption, (255, 255, 255))
    draw.line((0, left, w, right), fill=color, width=width)
    return np.array(im), ctr / h


_caption_cache = {}


def caption_mask(text):
    """The coverage mask Pillow's ``ImageDraw.text`` blends for ``text`` on an RGB image in its default font - whatever font and
    layout engine the installation has: ``getmask2(text, 'L', anchor='la')``.  -> ((mh, mw) uint8 array, (x, y) offset of its
    corner from the text position); cached by text."""
    hit = _caption_cache.get(text)
    if hit is None:
        from PIL import Image, ImageDraw
        font = ImageDraw.Draw(Image.new('RGB', (1, 1))).getfont()
        core, offset = font.getmask2(text, 'L', anchor='la')
        mw, mh = core.size
        mask = np.frombuffer(bytes(Image.Image()._new(core).tobytes()), np.uint8).reshape(mh, mw) if mw and mh else np.zeros((0, 0), np.uint8)
        if len(_caption_cache) >= 4096:
            _caption_cache.clear()
        hit = _caption_cache[text] = (mask, (int(offset[0]), int(offset[1])))
    return hit


def _pack_rgb(c) -> int:
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def horizon_marks(H, W, vfov, pitch, roll, focal_length=-1, color=(0, 255, 0), width=5, debug=False, GT=False, text_size=16, dtype=np.uint8):
    """One ``show_horizon_line`` call on an (H, W, 3) image as marks for ``Engine.draw_marks``: -> (marks (k, 8) int64 - the
    caption strip, the caption's mask blend (its mask at byte 0 of a mask buffer: the caller adds where it packs it), the wide
    line, in the reference's order -, the caption's (mask (mh, mw) uint8, offset) or None without ``debug``, ``ctr / h``).  The
    float64 arithmetic is the reference's (vis_utils.py:86-88: ``np.tan``, then C truncation of the end points), the caption its
    format, the mask the installed Pillow's (``caption_mask``).  -> None where the device route cannot reproduce the host: a
    non-finite end point or one beyond +-100000 (``_lib.MARK_MAX_COORD``), ``width`` < 2 (Pillow's Bresenham line) or > 64,
    ``text_size`` > H (the reference's negative slice wraps) or < 0, a colour that is not three integers in 0 .. 255, a frame
    beyond 8192 pixels per side, or an image ``dtype`` other than uint8 (the reference converts a float image first)."""
    h, w = int(H), int(W)
    if np.dtype(dtype) != np.uint8 or not (1 <= h <= _lib.MARK_MAX_SIDE and 1 <= w <= _lib.MARK_MAX_SIDE):
        return None
    try:
        rgb = tuple(int(c) for c in color)
        if isinstance(color, str) or len(rgb) != 3 or any(c != k or not 0 <= c <= 255 for c, k in zip(rgb, color)):
            return None
    except (TypeError, ValueError):
        return None
    if not (isinstance(width, (int, np.integer)) and _lib.MARK_MIN_WIDTH <= width <= _lib.MARK_MAX_WIDTH):
        return None
    if debug and not (isinstance(text_size, (int, np.integer)) and 0 <= text_size <= h):
        return None
    with np.errstate(all='ignore'):
        ctr = h * (0.5 - 0.5 * np.tan(pitch) / np.tan(vfov / 2))
        left, right = ctr - w * np.tan(roll) / 2, ctr + w * np.tan(roll) / 2
    if not (np.isfinite(left) and np.isfinite(right)) or max(abs(float(left)), abs(float(right))) >= _lib.MARK_MAX_COORD + 1:
        return None
    marks, caption = [], None
    if debug:
        top = h - text_size if GT else 0
        marks.append([_lib.MARK_STRIP, 0, top, top + text_size, 0, 0, 0, 0])
        text = ('GT: ' if GT else '') + 'vfov:{0:.1f}, pitch:{1:.1f}, roll:{2:.1f}, f_pix:{3:.1f}'.format(
            np.degrees(vfov), np.degrees(pitch), np.degrees(roll), focal_length)
        caption = caption_mask(text)
        mask, (ox, oy) = caption
        if mask.size:
            if max(mask.shape) > _lib.MARK_MAX_MASK_SIDE:
                return None
            marks.append([_lib.MARK_MASK, 0xffffff, ox, top + oy, mask.shape[1], mask.shape[0], 0, 0])
    marks.append([_lib.MARK_LINE, _pack_rgb(rgb), 0, int(left), w, int(right), int(width), 0])     # int(): C's truncation
    return np.asarray(marks, np.int64).reshape(-1, _lib.MARK_REC), caption, ctr / h


def plan_horizon_marks(sizes, params, dtypes=None):
    """The host side of ``show_horizon_lines``: ``sizes`` [(H, W)] and ``params``, per frame None or a list of horizons, each a
    dict of ``horizon_marks``' arguments (``vfov``, ``pitch``, ``roll`` and any of its keywords) or a (vfov, pitch, roll) tuple -
    drawn in order, e.g. ground truth, then prediction.  -> (geom columns [mark0, count] (n, 2) int64, marks (nmarks, 8) int64,
    the packed mask buffer (1-D uint8 host array: every distinct caption once), [[ctr / h per horizon] per frame]) - or None
    where ``horizon_marks`` gives None for some horizon."""
    ranges, rows, bufs, fracs, at, used = [], [], [], [], {}, 0
    for k, ((H, W), hs) in enumerate(zip(sizes, params)):
        first, fr = sum(r.shape[0] for r in rows), []
        for hz in hs or ():
            kw = dict(hz) if isinstance(hz, dict) else dict(zip(('vfov', 'pitch', 'roll'), hz))
            got = horizon_marks(H, W, dtype=np.uint8 if dtypes is None else dtypes[k], **kw)
            if got is None:
                return None
            marks, caption, frac = got
            marks = marks.copy()
            blend = marks[:, 0] == _lib.MARK_MASK
            if blend.any():
                key = id(caption[0])
                if key not in at:
                    at[key] = used
                    bufs.append(caption[0].reshape(-1))
                    used += caption[0].size
                marks[blend, 6] = at[key]
            rows.append(marks)
            fr.append(frac)
        ranges.append((first, sum(r.shape[0] for r in rows) - first))
        fracs.append(fr)
    marks = np.concatenate(rows) if rows else np.zeros((0, _lib.MARK_REC), np.int64)
    masks = np.concatenate(bufs) if bufs else np.zeros(0, np.uint8)
    return np.asarray(ranges, np.int64).reshape(-1, 2), marks, masks, fracs


def show_horizon_lines(slab, sizes, offsets, params, engine=None):
    """``show_horizon_line`` for the frames of a flush on the device: ``slab`` a 1-D uint8 device tensor holding the (H, W, 3)
    frames ``sizes`` at ``offsets`` - (n,) byte offsets of packed frames (``pack_frames``) or (n, 2) [byte offset, pitch] -,
    ``params`` as ``plan_horizon_marks`` takes them (a frame may carry several horizons, drawn in order).  All captions' masks
    go up in ONE buffer and ONE ``Engine.draw_marks`` call draws every frame in place: byte for byte what the host function
    makes.  -> [[ctr / h per horizon] per frame].  Raises ``ValueError`` for a horizon the device route cannot reproduce
    (``horizon_marks`` -> None): callers keep the host route for such a frame."""
    from . import cam_utils
    sizes = [(int(h), int(w)) for h, w in sizes]
    plan = plan_horizon_marks(sizes, params)
    if plan is None:
        raise ValueError('a horizon that the device route cannot reproduce (render.horizon_marks gives None): keep the host route for it')
    ranges, marks, masks, fracs = plan
    if not marks.shape[0]:
        return fracs
    eng = engine or cam_utils._engine(slab.device)
    offsets = np.asarray(offsets, np.int64)
    if offsets.ndim == 1:
        offsets = np.stack([offsets, 3 * np.asarray([w for _, w in sizes], np.int64)], axis=1)
    geom = np.concatenate([np.asarray(sizes, np.int64).reshape(-1, 2), ranges], axis=1)
    eng.draw_marks(slab, geom, offsets, marks, torch.from_numpy(masks).to(eng.device) if masks.size else None)
    return fracs


def write_obj(path: str, vertices, faces) -> str:
    """A Wavefront .obj with ``v`` and 1-based ``f`` records (17 significant digits are not needed: ``%.9g`` round-trips fp32)."""
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    with open(path, 'w') as fh:
        fh.writelines('v %.9g %.9g %.9g\n' % tuple(p) for p in v.tolist())
        fh.writelines('f %d %d %d\n' % tuple(t) for t in (f + 1).tolist())
    return path


def read_obj(path: str):
    """-> (vertices (V, 3) float32, faces (F, 3) int32, 0-based) of a file ``write_obj`` wrote (``f`` records may carry /vt/vn)."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == 'v':
                v.append([float(x) for x in p[1:4]])
            elif p and p[0] == 'f':
                f.append([int(x.split('/')[0]) - 1 for x in p[1:4]])
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)


def group_panel0(image, cam_params=None) -> np.ndarray:
    """Panel 0 of the three-panel picture on the host: ``image`` as uint8 (floats in [0, 1] are scaled, floats beyond 10 taken
    as 0 .. 255: renderer_cam.py:164-165) with, given ``cam_params`` = (vfov, pitch, roll, f_pix), the horizon line and caption
    of :170-173."""
    image = np.asarray(image)
    if image.dtype != np.uint8:
        image = np.clip(image * 255.0 if image.max() <= 10 else image, 0, 255).astype(np.uint8)
    if cam_params is not None:
        image, _ = show_horizon_line(image, cam_params[0], cam_params[1], cam_params[2], focal_length=cam_params[3], color=(0, 255, 0),
                                     width=5, debug=True, text_size=30)
    return np.ascontiguousarray(image)


def _panel0_horizon(cp):
    """The horizon of ``group_panel0`` for ``cam_params`` = (vfov, pitch, roll, f_pix) as ``plan_horizon_marks`` takes it."""
    return None if cp is None else [dict(vfov=cp[0], pitch=cp[1], roll=cp[2], focal_length=cp[3], color=(0, 255, 0), width=5, debug=True, text_size=30)]


def _panel0_raw(image, cam_params):
    """Can panel 0 of ``image`` be finished on the device?  -> the raw frame - a contiguous (H, W, 3) uint8 host array, or a
    uint8 device tensor as it is - when it is uint8 and ``horizon_marks`` can reproduce its horizon; None: ``group_panel0``."""
    if isinstance(image, torch.Tensor):
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            return None
        raw = image.detach() if image.device.type == 'cuda' else np.ascontiguousarray(image.detach().numpy())
    else:
        raw = np.asarray(image)
        if raw.dtype != np.uint8 or raw.ndim != 3 or raw.shape[2] != 3:
            return None
        raw = np.ascontiguousarray(raw)
    if plan_horizon_marks([raw.shape[:2]], [_panel0_horizon(cam_params)]) is None:
        return None
    return raw


def _pack_raw(frames, device):
    """``pack_frames`` for frames of which some lie on the device already: host frames go up, device frames are copied where
    they lie.  -> the 1-D uint8 slab on ``device``."""
    from .preprocess import pack_frames
    if all(isinstance(f, np.ndarray) for f in frames):
        return pack_frames(frames, device)[0]
    slab = torch.empty(sum(int(f.shape[0]) * int(f.shape[1]) * 3 for f in frames), device=device, dtype=torch.uint8)
    at = 0
    for f in frames:
        n = int(f.shape[0]) * int(f.shape[1]) * 3
        slab[at:at + n].copy_((torch.from_numpy(f) if isinstance(f, np.ndarray) else f).reshape(-1))
        at += n
    return slab


def _keypoints(kp, device, unnormalize=False, res=224) -> torch.Tensor:
    """``kp`` (J, D) or (M, J, D), D = 2 or 3, as a contiguous (M, J, D) fp32 tensor on ``device`` (a device tensor stays there);
    ``unnormalize``: x and y from [-1, 1] to pixels by ``(kp + 1) * res / 2``."""
    kp = torch.as_tensor(kp).detach().to(device=device, dtype=torch.float32)
    if kp.dim() == 2:
        kp = kp[None]
    if kp.dim() != 3 or kp.shape[2] not in (2, 3):
        raise ValueError('keypoints must be (J, D) or (M, J, D) with D = 2 (x, y) or 3 (x, y, confidence)')
    if unnormalize:
        kp = kp.clone()
        kp[..., :2] = (kp[..., :2] + 1.0) * float(res) / 2.0
    return kp.contiguous()


def draw_skeleton(image, kp_2d, dataset='spin', unnormalize=True, thickness=2, res=224, engine=None):
    """``pare.utils.vis_utils.draw_skeleton`` as ``render_image_group`` calls it (renderer_cam.py:168), on the device
    (``specmi_draw_skeletons``): the skeletons ``kp_2d`` (J, D) - or (M, J, D), drawn one after the other - over ``image``.
    ``image``: an (H, W, 3) uint8 device tensor is drawn into and returned; a host array (uint8, or floats as ``group_panel0``
    takes them) is uploaded and a uint8 host array returned.  ``dataset``: 'spin' only (``constants.SKELETON_SPIN``, J = 49).
    ``unnormalize``: the keypoints are in [-1, 1] of a ``res`` x ``res`` crop and become pixels by ``(kp + 1) * res / 2``.
    Joints are discs of radius 4, bones have ``thickness``; D = 3: a keypoint with confidence <= 0.3 is not drawn.  Coverage,
    bone table and colours are this project's own (module docstring)."""
    from . import cam_utils
    if dataset != 'spin':
        raise ValueError(f"dataset {dataset!r}: only the 'spin' skeleton (constants.SKELETON_SPIN) is defined")
    on_device = isinstance(image, torch.Tensor) and image.device.type == 'cuda'
    if on_device:
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or not image.is_contiguous():
            raise ValueError('a device image must be a contiguous (H, W, 3) uint8 tensor (it is drawn into)')
        eng = engine or cam_utils._engine(image.device)
        frame = image
    else:
        eng = engine or cam_utils._engine(torch.device('cuda'))
        frame = torch.from_numpy(group_panel0(image.detach().numpy() if isinstance(image, torch.Tensor) else image)).to(eng.device)
    kp = _keypoints(kp_2d, eng.device, unnormalize, res)
    H, W = int(frame.shape[0]), int(frame.shape[1])
    eng.draw_skeletons(kp, frame.view(-1), [[H, W, 0, kp.shape[0]]], [[0, 3 * W]], style=_lib.DrawStyle(thickness=thickness))
    return frame if on_device else frame.cpu().numpy()


def render_image_group(image, camera_translation, vertices, camera_rotation, focal_length, camera_center, mesh_color='pinkish',
                       alpha=1.0, faces=None, mesh_filename: Optional[str] = None, save_filename: Optional[str] = None, keypoints_2d=None,
                       cam_params: Optional[Sequence] = None, device=None, engine=None, jpeg_device=None, panel0_device=None, png_device=None):
    """The three panels of ``render_image_group`` (renderer_cam.py:147-218) side by side, (H, 3W, 3) uint8 on the device:

    0. ``image`` (H, W, 3; uint8, or floats in [0, 1] / [0, 255] as the reference accepts) with - given ``cam_params`` =
       (vfov, pitch, roll, f_pix) - the horizon line and caption of ``show_horizon_line(..., width=5, debug=True, text_size=30)``
       and - given ``keypoints_2d`` (J, D), or (M, J, D) for the M meshes, in pixels of ``image`` - the 2D skeletons
       (``draw_skeleton(..., unnormalize=False)``, on the device), so that they show in panels 0 and 1.  Stated deviation: the
       reference draws the skeleton BEFORE the line and caption (renderer_cam.py:167-173); here it is drawn over the finished
       panel, which differs only where a bone or joint crosses the line or the caption strip;
    1. the meshes drawn over panel 0;
    2. the side view at 270 degrees with the ground plane.

    ``vertices`` (M, V, 3) / ``camera_translation`` (M, 3) may hold all detections of a frame: they are drawn together, one
    launch sequence per panel (one mesh (V, 3) / (3,) is the reference's call).  ``mesh_filename``: the meshes after the 180
    degree turn as .obj (``NAME.obj``; ``NAME_<m>.obj`` from the second on) and the x-flipped translations as .npy
    (renderer_cam.py:74,87-90).  ``save_filename``: the image through Pillow (the reference's cv2.imwrite of the RGB-swapped
    array stores the same pixels); with ``jpeg_device`` (None = ``engine.JPEG_DEVICE_DEFAULT``) a ``.jpg`` / ``.jpeg`` name is
    encoded on the device (``save_picture``: the same bytes, and only they come down), with ``png_device`` (None =
    ``engine.PNG_DEVICE_DEFAULT``, off) a ``.png`` name (the same picture, other bytes).  ``alpha`` is accepted and ignored: the
    reference's material is ``alphaMode='OPAQUE'``.  ``panel0_device`` (None = ``engine.PANEL0_DEVICE_DEFAULT``): a uint8
    ``image`` goes up raw - a device tensor does not come down at all - and the line and caption are drawn where it lies
    (``show_horizon_lines``), before the skeleton and the meshes as on the host: the same bytes.  A float image, or a horizon
    that ``horizon_marks`` cannot reproduce, keeps the host route."""
    from . import cam_utils
    from .engine import flow_panel0_device
    if isinstance(image, torch.Tensor):
        device = device or (image.device if image.device.type == 'cuda' else None)
    dev = torch.device(device or 'cuda')
    eng = engine or cam_utils._engine(dev)
    raw = _panel0_raw(image, cam_params) if flow_panel0_device(panel0_device) else None
    if raw is not None:
        panel0 = (torch.from_numpy(raw) if isinstance(raw, np.ndarray) else raw).to(eng.device, copy=True).contiguous()
        if cam_params is not None:
            H, W = int(panel0.shape[0]), int(panel0.shape[1])
            show_horizon_lines(panel0.view(-1), [(H, W)], [0], [_panel0_horizon(cam_params)], engine=eng)
    else:
        image = group_panel0(image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else image, cam_params)
        panel0 = torch.from_numpy(np.ascontiguousarray(image)).to(eng.device)
    if keypoints_2d is not None:
        draw_skeleton(panel0, keypoints_2d, unnormalize=False, engine=eng)
    kw = dict(faces=faces, color=mesh_color, engine=eng, cull=_closed(faces))
    overlay = render_overlay(panel0, vertices, camera_translation, camera_rotation, focal_length, camera_center, **kw)
    side = render_overlay(panel0, vertices, camera_translation, camera_rotation, focal_length, camera_center, side_view=True, ground_plane=True, **kw)
    out = torch.cat([panel0, overlay, side], dim=1)
    if mesh_filename:
        v = torch.as_tensor(vertices).detach().float().cpu().numpy().reshape(-1, int(torch.as_tensor(vertices).shape[-2]), 3)
        t = torch.as_tensor(camera_translation).detach().float().cpu().numpy().reshape(-1, 3) * np.array([-1., 1., 1.], np.float32)
        table = device_faces(faces, eng.device).cpu().numpy()
        for m in range(v.shape[0]):
            name = mesh_filename if m == 0 else mesh_filename.replace('.obj', f'_{m}.obj')
            write_obj(name, v[m] * np.array([1., -1., -1.], np.float32), table)
            np.save(name.replace('.obj', '.npy'), t[m])
    if save_filename is not None:
        os.makedirs(os.path.dirname(os.path.abspath(save_filename)), exist_ok=True)
        save_picture(save_filename, out, engine=eng, jpeg_device=jpeg_device, png_device=png_device)
    return out


def save_picture(path: str, picture, engine=None, jpeg_device=None, png_device=None) -> str:
    """``picture`` - an (H, W, 3) uint8 device tensor, or the ``bytes`` of a file encoded already - written to ``path``.  A
    tensor goes through Pillow as before (``Image.fromarray(...).save(path)``) unless ``jpeg_device`` (None =
    ``engine.JPEG_DEVICE_DEFAULT``) is on, the name is ``.jpg`` / ``.jpeg`` and the tensor lies on the device: then ``Engine.jpeg_encode`` encodes it where it
    lies at Pillow's default quality 75 - byte for byte Pillow's file - and only those bytes come down.  Likewise with
    ``png_device`` (None = ``engine.PNG_DEVICE_DEFAULT``, off) and a ``.png`` name: ``Engine.png_encode`` writes a file that
    decodes to the same picture, with bytes of its own (include/specmi.h)."""
    from . import cam_utils
    from .engine import flow_jpeg_device, flow_png_device, is_jpeg_name, is_png_name
    if isinstance(picture, (bytes, bytearray)):
        data = picture
    elif flow_png_device(png_device) and is_png_name(path) and picture.device.type == 'cuda':
        eng = engine or cam_utils._engine(picture.device)
        H, W = int(picture.shape[0]), int(picture.shape[1])
        data = eng.png_encode(picture.contiguous().view(-1), [[H, W]], [[0, 3 * W]])[0]
    elif flow_jpeg_device(jpeg_device) and is_jpeg_name(path) and picture.device.type == 'cuda':
        eng = engine or cam_utils._engine(picture.device)
        H, W = int(picture.shape[0]), int(picture.shape[1])
        data = eng.jpeg_encode(picture.contiguous().view(-1), [[H, W]], [[0, 3 * W]], 75)[0]
    else:
        from PIL import Image
        Image.fromarray(picture.cpu().numpy()).save(path)
        return path
    with open(path, 'wb') as f:
        f.write(data)
    return path


def plan_views(sizes, counts, each=False, pixel_budget=None, gap=0, cull=True, frame_per_picture=False):
    """The view records and slab layouts of the three-panel pictures of many frames, for ``Engine.render_views``: pure host
    code.  ``sizes`` [(H, W)] and ``counts`` (detections per frame, >= 1) describe a flush whose meshes lie frame after frame in
    one (sum counts, V, 3) array.  One (H, 3W, 3) picture per frame holding all its detections - ``each``: one per detection,
    holding that detection alone, in frame then detection order.  A picture is three views of pitch 9 W, panel k at byte column
    3 W k: a ``count == 0`` view that copies panel 0, the overlay, and the side view with its ground plane, all reading the
    picture's frame.  The pictures are split into CHUNKS, one ``render_views`` call each, so that a chunk's view pixels
    (3 H W per picture) stay under ``pixel_budget`` (None = ``engine.RENDER_PIXEL_BUDGET``); a picture is never split and a
    chunk holds at least one.  A chunk's frame slab holds the frames its pictures name, each once, back to back in frame order
    (``pack_frames`` of those frames); its output slab holds its pictures back to back, ``gap`` bytes apart.
    ``frame_per_picture``: the frame slab holds one copy of the frame PER PICTURE instead, in picture order - what ``each``
    needs when something is drawn into the frames per detection (the 2D skeletons).
    -> a list of chunks, each a dict: ``frames`` (the frame indices of its frame slab), ``frame_dets`` (one [first detection,
    count] per slab frame: the detections of the pictures that read it), ``in_bytes``, ``pictures``
    [(frame, detection or None)], ``picture_offsets`` (byte offset of each picture in the output slab), ``out_bytes``,
    ``geom`` (n, 5) int32 [H, W, mesh0, count, flags], ``offsets`` (n, 4) int64 [in_offset, in_pitch, out_offset, out_pitch],
    ``view_frame`` (n,) the frame whose camera view v takes."""
    from .engine import RENDER_PIXEL_BUDGET
    sizes = [(int(h), int(w)) for h, w in sizes]
    counts = [int(c) for c in counts]
    if not sizes or len(sizes) != len(counts):
        raise ValueError('one (H, W) and one detection count per frame (at least one frame)')
    if min(counts) < 1 or min(min(s) for s in sizes) < 1:
        raise ValueError('every frame has at least one detection and at least one pixel per side')
    budget = RENDER_PIXEL_BUDGET if pixel_budget is None else int(pixel_budget)
    first = np.concatenate([[0], np.cumsum(counts)])
    pictures = [(f, i) for f, c in enumerate(counts) for i in range(c)] if each else [(f, None) for f in range(len(counts))]
    c = _lib.RENDER_CULL if cull else 0
    chunks, cur, px = [], [], 0
    for pic in pictures:
        need = 3 * sizes[pic[0]][0] * sizes[pic[0]][1]
        if cur and px + need > budget:
            chunks.append(cur)
            cur, px = [], 0
        cur.append(pic)
        px += need
    chunks.append(cur)
    out = []
    for pics in chunks:
        dets_of = lambda f, i: (int(first[f]), counts[f]) if i is None else (int(first[f]) + i, 1)
        if frame_per_picture:
            frames, frame_dets, slot = [f for f, _ in pics], [dets_of(f, i) for f, i in pics], list(range(len(pics)))
        else:
            frames = sorted({f for f, _ in pics})
            frame_dets, slot = [dets_of(f, None) for f in frames], [frames.index(f) for f, _ in pics]
        in_off, off = [], 0
        for f in frames:
            in_off.append(off)
            off += sizes[f][0] * sizes[f][1] * 3
        geom, offsets, view_frame, pic_off, o = [], [], [], [], 0
        for (f, i), sl in zip(pics, slot):
            H, W = sizes[f]
            mesh0, count = dets_of(f, i)
            pic_off.append(o)
            for k, (m0, cnt, flags) in enumerate(((0, 0, 0), (mesh0, count, c), (mesh0, count, c | _lib.RENDER_SIDE_VIEW | _lib.RENDER_GROUND_PLANE))):
                geom.append((H, W, m0, cnt, flags))
                offsets.append((in_off[sl], 3 * W, o + 3 * W * k, 9 * W))
                view_frame.append(f)
            o += 9 * H * W + gap
        out.append(dict(frames=frames, frame_dets=np.asarray(frame_dets, np.int64).reshape(-1, 2), frame_offsets=np.asarray(in_off, np.int64),
                        in_bytes=off, pictures=pics, picture_offsets=pic_off, out_bytes=o - gap,
                        geom=np.asarray(geom, np.int32), offsets=np.asarray(offsets, np.int64), view_frame=np.asarray(view_frame, np.int64)))
    return out


def view_cams(view_frame, rotations, focals, centers) -> np.ndarray:
    """The (n, 13) float32 camera rows [R row-major, fx, fy, cx, cy] of ``Engine.render_views`` for views that take the camera
    of frame ``view_frame[v]``: ``rotations`` (F, 3, 3), ``focals`` (F, 2) = (fx, fy), ``centers`` (F, 2) = (cx, cy)."""
    R = np.asarray(rotations, np.float32).reshape(-1, 9)
    cam = np.concatenate([R, np.asarray(focals, np.float64).reshape(-1, 2).astype(np.float32),
                          np.asarray(centers, np.float64).reshape(-1, 2).astype(np.float32)], axis=1)
    return np.ascontiguousarray(cam[np.asarray(view_frame, np.int64)])


def render_image_groups(frames, vertices, cam_t, counts, rotations, focals, centers, cam_params=None, each=False, mesh_color='pinkish',
                        faces=None, pixel_budget=None, device=None, engine=None, return_slabs=False, keypoints_2d=None, encode=None,
                        quality=75, panel0_device=None):
    """``render_image_group`` for the frames of a flush in one call per chunk (``specmi_render_views``): ``frames`` a list of
    (H, W, 3) host images of any sizes, ``vertices`` (sum counts, V, 3) / ``cam_t`` (sum counts, 3) the detections frame after
    frame (device tensors stay on the device), ``counts`` the detections per frame, ``rotations`` (F, 3, 3), ``focals`` (F, 2),
    ``centers`` (F, 2) and ``cam_params`` (a list of (vfov, pitch, roll, f_pix) or None per frame) the frames' cameras.
    Panel 0 is made per frame on the host (``group_panel0``: Pillow's horizon line) or, with ``panel0_device``, in the slab; per chunk of ``plan_views`` the panels go
    up in ONE slab, ONE ``render_views`` call draws every panel of every picture in place, and ONE slab comes down.
    -> the list of (H, 3W, 3) uint8 host arrays, one per frame - ``each``: one per detection, that detection alone -, equal byte
    for byte to ``render_image_group`` on the same frame and meshes.  ``return_slabs``: also [(device slab, picture offsets,
    [(H, 3W)])] per chunk.  ``keypoints_2d`` (sum counts, J, D), the detections' 2D keypoints in pixels of their frames (a device
    tensor stays on the device): drawn into each chunk's frame slab by ONE ``draw_skeletons`` call before the chunk's
    ``render_views`` call, as ``render_image_group(keypoints_2d=...)`` draws them per frame - the same bytes; with ``each`` the
    slab holds one copy of a frame per picture and each picture shows its own detection's skeleton alone.
    ``encode``: None, 'jpeg', 'png', or one of them per frame.  A picture of a 'png' frame comes back as the ``bytes`` of its PNG
    file (``Engine.png_encode``, ONE call per chunk: it decodes to the array, its bytes are not Pillow's).  A picture of a 'jpeg' frame comes back as the ``bytes`` of its JPEG
    file at ``quality`` instead of an array - encoded from the output slab where it lies by ONE ``Engine.jpeg_encode`` call per
    chunk, byte for byte what ``Image.fromarray(array).save(f, format='JPEG', quality=quality)`` writes; the raw slab does not
    come down (only the pictures of frames that are not encoded do, one by one).
    ``panel0_device`` (None = ``engine.PANEL0_DEVICE_DEFAULT``): uint8 frames go into the chunk's slab raw - a frame given as a
    device tensor does not come down at all - and ONE ``draw_marks`` call per chunk (``show_horizon_lines``) draws their lines
    and captions there, before the skeletons: the same bytes.  A float frame, or one whose horizon ``horizon_marks`` cannot
    reproduce, keeps ``group_panel0``."""
    from . import cam_utils
    from .engine import flow_panel0_device
    frames = list(frames)
    cam_params = [None] * len(frames) if cam_params is None else list(cam_params)
    if not (len(frames) == len(counts) == len(cam_params)):
        raise ValueError('one detection count (and one cam_params entry) per frame')
    encode = [encode] * len(frames) if encode is None or isinstance(encode, str) else list(encode)
    if len(encode) != len(frames) or any(e not in (None, 'jpeg', 'png') for e in encode):
        raise ValueError("encode: None, 'jpeg', 'png', or one of them per frame")
    raw = [_panel0_raw(im, cp) for im, cp in zip(frames, cam_params)] if flow_panel0_device(panel0_device) else [None] * len(frames)
    panel0 = [r if r is not None else group_panel0(im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else im, cp)
              for r, im, cp in zip(raw, frames, cam_params)]
    dev = torch.device(device or (vertices.device if isinstance(vertices, torch.Tensor) and vertices.device.type == 'cuda' else 'cuda'))
    eng = engine or cam_utils._engine(dev)
    as_f32 = lambda x: torch.as_tensor(x).to(device=eng.device, dtype=torch.float32).contiguous()
    vertices, cam_t = as_f32(vertices), as_f32(cam_t).reshape(-1, 3)
    if vertices.dim() != 3 or vertices.shape[0] != sum(int(c) for c in counts):
        raise ValueError('vertices must be (sum of counts, V, 3)')
    table, rgb = device_faces(faces, eng.device), _rgb(mesh_color)
    sizes = [(int(p.shape[0]), int(p.shape[1])) for p in panel0]
    if keypoints_2d is not None:
        keypoints_2d = _keypoints(keypoints_2d, eng.device)
        if keypoints_2d.shape[0] != vertices.shape[0]:
            raise ValueError('keypoints_2d must be (sum of counts, J, D)')
    pictures, slabs = [], []
    for ch in plan_views(sizes, counts, each=each, pixel_budget=pixel_budget, cull=_closed(faces), frame_per_picture=each and keypoints_2d is not None):
        in_slab = _pack_raw([panel0[f] for f in ch['frames']], eng.device)
        if any(raw[f] is not None and cam_params[f] is not None for f in ch['frames']):
            show_horizon_lines(in_slab, [sizes[f] for f in ch['frames']], ch['frame_offsets'],
                               [_panel0_horizon(cam_params[f]) if raw[f] is not None else None for f in ch['frames']], engine=eng)
        if keypoints_2d is not None:
            hw = np.asarray([sizes[f] for f in ch['frames']], np.int64).reshape(-1, 2)
            eng.draw_skeletons(keypoints_2d, in_slab, np.concatenate([hw, ch['frame_dets']], axis=1),
                               np.stack([ch['frame_offsets'], 3 * hw[:, 1]], axis=1))
        out_slab = torch.empty(ch['out_bytes'], device=eng.device, dtype=torch.uint8)
        eng.render_views(vertices, table, cam_t, ch['geom'], ch['offsets'], view_cams(ch['view_frame'], rotations, focals, centers),
                         in_slab, out_slab, rgb=rgb)
        shapes = [(sizes[f][0], 3 * sizes[f][1]) for f, _ in ch['pictures']]
        coded = [k for k, (f, _) in enumerate(ch['pictures']) if encode[f] == 'jpeg']
        as_png = [k for k, (f, _) in enumerate(ch['pictures']) if encode[f] == 'png']
        if not coded and not as_png:
            host = out_slab.cpu().numpy()
            pictures += [host[o:o + h * w3 * 3].reshape(h, w3, 3) for o, (h, w3) in zip(ch['picture_offsets'], shapes)]
        else:
            where = lambda ks: ([shapes[k] for k in ks], [(ch['picture_offsets'][k], 3 * shapes[k][1]) for k in ks])
            got = dict(zip(coded, eng.jpeg_encode(out_slab, *where(coded), quality))) if coded else {}
            if as_png:
                got.update(zip(as_png, eng.png_encode(out_slab, *where(as_png))))
            for k, (o, (h, w3)) in enumerate(zip(ch['picture_offsets'], shapes)):
                pictures.append(got[k] if k in got else out_slab[o:o + h * w3 * 3].cpu().numpy().reshape(h, w3, 3))
        slabs.append((out_slab, ch['picture_offsets'], shapes))
    return (pictures, slabs) if return_slabs else pictures


def _closed(faces) -> bool:
    """Cull back faces?  Yes for a caller's table and for the SMPL file's (closed, outward-wound); no for the synthetic body
    model's triangle soup, whose winding means nothing."""
    if faces is not None:
        return True
    from . import assets
    assets.faces()
    return assets._STATE['smpl_path'] is not None
