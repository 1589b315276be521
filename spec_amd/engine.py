"""Thin object wrapper over a libspecmi handle: parameter upload and forward calls with torch
device tensors (torch is plumbing here: HBM allocations + the current HIP stream)."""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Dict, List, Mapping, Optional

import numpy as np
import torch

from . import _lib
# the host records of the picture operations - what the wrappers below refuse before any device call - live in spec_amd.records
from .records import (PNG_BPP, check_color_jitter, check_draw_marks, check_draw_skeletons, check_jpeg_decode,  # noqa: F401
                      check_jpeg_encode, check_png_decode, check_png_encode, check_render_views, jpeg_capacity, png_bound, starts)

KIND = {'camcalib': _lib.MODEL_CAMCALIB, 'hmr': _lib.MODEL_HMR, 'smpl': _lib.MODEL_SMPL}

# The packed per-image record, stated once: (key, per-image shape) in packing order, None = (num_verts, 3).
# 85,164 B of SPEC outputs + 12 B of camera angles.  Every offset, every dense output shape and the all-gather payloads
# (spec_amd.pipeline, which re-exports this table) derive from it through ``record_layout``.
PACKED_KEYS = (
    ('smpl_vertices', None), ('smpl_joints3d', (49, 3)), ('smpl_joints2d', (49, 2)),
    ('pred_cam_t', (3,)), ('pred_pose', (24, 3, 3)), ('pred_cam', (3,)), ('pred_shape', (10,)),
    ('pred_pose_6d', (144,)), ('cam_vfov', ()), ('cam_pitch', ()), ('cam_roll', ()),
)
# the vertices come first and are the only size that depends on the body model: everything after them is the joints payload
assert PACKED_KEYS[0] == ('smpl_vertices', None) and all(shp is not None for _, shp in PACKED_KEYS[1:])
_HMR_KEYS = tuple(k for k, _ in _lib.HmrOutputs._fields_)     # what the head + SMPL calls write: the record without the angles
assert _HMR_KEYS == tuple(k for k, _ in PACKED_KEYS[:len(_HMR_KEYS)])
_ROTMATS = dict(PACKED_KEYS)['pred_pose']                     # one rotation matrix per joint: also what smpl / smpl_native take


@functools.lru_cache(maxsize=None)
def record_layout(num_verts: int):
    """((key, offset, per-image shape), ...) of the packed record in packing order, and its length in floats: 21,294 for
    V = 6890.  Pure and cached per ``num_verts``: do not modify the result."""
    lay, off = [], 0
    for k, shp in PACKED_KEYS:
        shp = (num_verts, 3) if shp is None else shp
        lay.append((k, off, shp))
        off += math.prod(shp)
    return tuple(lay), off


@functools.lru_cache(maxsize=None)
def _record_shapes(num_verts: int):
    return {k: shp for k, _, shp in record_layout(num_verts)[0]}


# specmi_hmr_loss (include/specmi.h), stated once: the tensors in the order of the C prototype with their per-image shapes
# (None = (num_verts, 3)), the constructor weights in the reference's order (spec/losses.py:27-36) and the keys of its loss_dict.
HMR_LOSS_INPUTS = {     # the prediction side is six entries of the packed record; the ground-truth side is stated beside the prototype
    'pred': tuple((k, dict(PACKED_KEYS)[k]) for k in ('pred_pose', 'pred_shape', 'pred_cam', 'smpl_joints3d', 'smpl_joints2d', 'smpl_vertices')),
    'gt': _lib.HMR_LOSS_GT,
}
HMR_LOSS_WEIGHTS = ('shape_loss_weight', 'keypoint_loss_weight', 'pose_loss_weight', 'smpl_part_loss_weight', 'beta_loss_weight',
                    'openpose_train_weight', 'gt_train_weight', 'loss_weight')
HMR_LOSS_KEYS = ('loss/loss_keypoints', 'loss/loss_keypoints_3d', 'loss/loss_regr_pose', 'loss/loss_regr_betas', 'loss/loss_shape',
                 'loss/loss_cam', 'loss/total_loss')


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_f32(t, device, shape=None):
    """-> contiguous fp32 tensor on `device` (accepts tensors / arrays / scalars), or None."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'expected shape {tuple(shape)}, got {tuple(t.shape)}')
    return t


def _u8_slab(name, x, device, optional=False):
    """``x`` is a contiguous 1-D uint8 tensor on ``device`` (``optional``: or None), or ``ValueError``."""
    if x is None and optional:
        return
    if not isinstance(x, torch.Tensor) or x.device != device or x.dtype != torch.uint8 or x.dim() != 1 or not x.is_contiguous():
        raise ValueError(f'{name} must be a contiguous 1-D uint8 tensor on the engine device')


def _dev_tensor(name, x, dtype, device, optional=False):
    """``x`` is a contiguous tensor of ``dtype`` and any shape on ``device`` (``optional``: or None), or ``ValueError``."""
    if x is None and optional:
        return
    if not isinstance(x, torch.Tensor) or x.device != device or x.dtype != dtype or not x.is_contiguous():
        raise ValueError(f'{name} must be a contiguous {dtype} tensor on the engine device')


def _dev_vector(name, x, n, dtype, device):
    """-> ``x``, a contiguous (n,) vector of ``dtype`` on ``device``, or a new one for None; anything else: ``ValueError``."""
    if x is None:
        return torch.empty(n, device=device, dtype=dtype)
    if not isinstance(x, torch.Tensor) or x.device != device or x.dtype != dtype or tuple(x.shape) != (n,) or not x.is_contiguous():
        raise ValueError(f'{name} must be a contiguous (n,) {dtype} tensor on the engine device')
    return x


def _mesh_inputs(vertices, faces, cam_t, device, min_meshes):
    """The meshes of ``render_meshes`` and ``render_views``: ``vertices`` (M, V, 3) / ``cam_t`` (M, 3) fp32 and ``faces`` (F, 3)
    int32 on ``device``, M >= ``min_meshes``, V >= 1, F >= 1 -> M, V, F."""
    for name, x, dt in (('vertices', vertices, torch.float32), ('cam_t', cam_t, torch.float32), ('faces', faces, torch.int32)):
        _dev_tensor(name, x, dt, device)
    if vertices.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[0] < min_meshes or vertices.shape[1] < 1:
        raise ValueError(f'vertices must be (M, V, 3) with M >= {min_meshes} and V >= 1')
    M, V = int(vertices.shape[0]), int(vertices.shape[1])
    if tuple(cam_t.shape) != (M, 3):
        raise ValueError('cam_t must be (M, 3)')
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError('faces must be (F, 3) with F >= 1')
    return M, V, int(faces.shape[0])


def _encode_rows(geom, offsets):
    """The host arrays of ``jpeg_encode`` and ``png_encode`` -> geom (n, 2) [H, W], offsets (n, 2) [in_offset, in_pitch], int64."""
    geom = np.ascontiguousarray(geom, dtype=np.int64).reshape(-1, 2)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if tuple(offsets.shape) != (geom.shape[0], 2):
        raise ValueError('offsets (n, 2): in_offset and in_pitch per picture')
    return geom, offsets


def nhwc8_input(images, precision: str) -> bool:
    """Is ``images`` the fp16 entrance of the fp16 trunk - a ``torch.float16`` tensor in the NHWC8 layout (B, H, W, 8) of
    include/specmi.h?  Validation only, no device call: an fp16 tensor of another shape, or one handed to a model whose
    precision is not 'fp16', raises ``ValueError`` (nothing is converted silently, in either direction)."""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.float16:
        return False
    if images.dim() != 4 or images.shape[3] != 8:
        raise ValueError(f'fp16 images must be NHWC8, shape (B,H,W,8) (spec_amd.preprocess, dtype=torch.float16), got {tuple(images.shape)}')
    if precision != 'fp16':
        raise ValueError("fp16 NHWC8 images feed the fp16 trunk only: call set_precision('fp16') on the model first "
                         f"(its precision is {precision!r}), or produce fp32 crops")
    return True


# Which route the flows that own their crop buffers (FrameStream, DemoPipeline, SPECTester, the two evaluation flows) take for a
# model at precision 'fp16': False = fp32 images converted inside the trunk (route (a), DESIGN.md 7b "Input"), True = NHWC8 fp16
# images read by the stem (route (b)).  Same bits either way; the default follows the measurement quoted there.
F16_CROPS_DEFAULT = False


def flow_image_dtype(module, fp32_crops=None):
    """The dtype such a flow asks the producers for: ``fp32_crops`` (the flow's private switch) decides, None = the default."""
    if fp32_crops is None:
        fp32_crops = not F16_CROPS_DEFAULT
    return torch.float32 if fp32_crops else getattr(module, 'image_dtype', torch.float32)


# Which route the flows whose frames differ in size (EvalDataset.batch, SPECTester.run_on_image_folder) take for their crops:
# False = one upload and one crop launch per frame (route (a)), True = one slab, one upload, one ragged launch per batch (route
# (b)).  Same bits either way; the default follows F16_CROPS_DEFAULT's rule: (b) where it is not slower than
# (a) beyond (a)'s own spread between rounds - and from host frames it is 3.5 x slower (profiles/ragged_crops_aux.json: the host-side
# packing pass and a pageable upload outweigh the launches saved).
RAGGED_CROPS_DEFAULT = False


def flow_ragged_crops(ragged_crops=None) -> bool:
    """``ragged_crops`` (the flow's private switch) decides, None = the default."""
    return RAGGED_CROPS_DEFAULT if ragged_crops is None else bool(ragged_crops)


# Which route the demo flow (SPECTester.run_on_image_folder) takes for its pictures: False = one render_image_group per frame -
# an upload, two specmi_render_meshes calls, a concatenation and a download each (route (a)), True = one render_image_groups per
# flush: one slab up, one specmi_render_views call and one slab down per chunk (route (b)).  Same bytes either
# way; the default follows F16_CROPS_DEFAULT's rule: (b) where it is not slower than (a) beyond (a)'s own spread between rounds -
# and from host frames to host pictures it is 2.2 - 2.6 x slower (profiles/render_batch_aux.json: on the device it is 1.2 - 1.3 x
# faster, but the packing pass and the large pageable copies outweigh that).
RENDER_BATCH_DEFAULT = False
# The view pixels one specmi_render_views call of render_image_groups may hold (the flush is split into chunks under it): 64 Mpx
# bound the depth keys at 512 MB.  A default, not a measurement.
RENDER_PIXEL_BUDGET = 64 << 20


def flow_render_batch(render_batch=None) -> bool:
    """``render_batch`` (the flow's private switch) decides, None = the default."""
    return RENDER_BATCH_DEFAULT if render_batch is None else bool(render_batch)


# Which route panel 0 of the pictures takes (render_image_group, render_image_groups, SPECTester, evaluation.save_batch_picture):
# False = render.group_panel0 draws the horizon line and caption per frame on the host with Pillow - a download of a device
# frame, a Pillow raster and an upload each (route (a)), True = uint8 frames go up raw and ONE specmi_draw_marks call per flush
# draws them in the slab (route (b)).  Same bytes either way; the default is (b) only where it is faster than (a)
# beyond the spread between repeats of the same run - and for eight 1080 x 1920 frames, host frames to the finished slab, it is
# 4.7 x faster (7.8 against 36.8 ms per flush, spread 0.4; the launch itself takes 10 us: profiles/horizon_panel_aux.json).
PANEL0_DEVICE_DEFAULT = True


def flow_panel0_device(panel0_device=None) -> bool:
    """``panel0_device`` (the flow's private switch) decides, None = the default."""
    return PANEL0_DEVICE_DEFAULT if panel0_device is None else bool(panel0_device)


# Which route the pictures the flows write as .jpg / .jpeg take (SPECTester._write_pictures, render_image_group(save_filename=),
# panorama.write_tree, evaluation.save_batch_picture): False = the raw picture comes down and Pillow encodes it on the host (route
# (a)), True = specmi_jpeg_encode encodes it where it lies and only the file's bytes come down (route (b)).
# Same bytes either way (on a libjpeg-turbo Pillow); the default follows F16_CROPS_DEFAULT's rule: (b) where it is not slower than
# (a) beyond (a)'s own spread between rounds - and it is 53 x faster on eight 1080 x 5760 pictures at quality 75 (0.25 against
# 13.0 ms per picture, spread 0.5) and 20 x on twelve 600 x 800 views at quality 95 (profiles/jpeg_encode_aux.json).
JPEG_DEVICE_DEFAULT = True


def flow_jpeg_device(jpeg_device=None) -> bool:
    """``jpeg_device`` (the flow's private switch) decides, None = the default."""
    return JPEG_DEVICE_DEFAULT if jpeg_device is None else bool(jpeg_device)


def is_jpeg_name(path) -> bool:
    """Does Pillow write ``path`` as a JPEG (by its extension)?"""
    return str(path).lower().endswith(('.jpg', '.jpeg'))


# Which route the pictures the flows write as .png take (the same flows as JPEG_DEVICE_DEFAULT's): False = the raw picture comes
# down and Pillow (zlib, one host thread) encodes it, True = specmi_png_encode encodes it where it lies and only the file's bytes
# come down.  Unlike the JPEG route the BYTES differ from the host route's - the file decodes to the same
# picture, but it is this library's deflate, not zlib's (include/specmi.h states the contract) - so the route is opt-in: off by
# default whatever scripts/bench_aux.py --only png_encode measures (6.3 against 336 ms per 1080 x 5760 picture, files of 0.43 of raw
# against Pillow's 0.23: profiles/png_encode_aux.json).
PNG_DEVICE_DEFAULT = False


def flow_png_device(png_device=None) -> bool:
    """``png_device`` (the flow's private switch) decides, None = the default."""
    return PNG_DEVICE_DEFAULT if png_device is None else bool(png_device)


def is_png_name(path) -> bool:
    """Does Pillow write ``path`` as a PNG (by its extension)?"""
    return str(path).lower().endswith('.png')


# Which route the .jpg / .jpeg frames the flows READ take (preprocess.decode_frames): False = Pillow decodes every file on the host
# and the raw frames go up (today's path, bit for bit), True = the files' bytes go up and specmi_jpeg_decode decodes the supported
# ones where they land.  Same pixels either way on a libjpeg-turbo Pillow.  The rule: True only when
# scripts/bench_aux.py --only jpeg_decode shows the device route ahead of 16 host threads at both qualities by more than the host
# route's own spread between rounds - and it is, on 64 frames of 1080p: 7.1 - 9.5 against 155.2 - 213.2 ms at quality 75 (spread
# 58.0), 31.9 - 37.3 against 162.1 - 185.7 ms at quality 95 (spread 23.6), identical slabs (profiles/jpeg_decode_aux.json).
JPEG_DECODE_DEVICE_DEFAULT = True


def flow_jpeg_decode_device(jpeg_decode_device=None) -> bool:
    """``jpeg_decode_device`` (the flow's private switch) decides, None = the default."""
    return JPEG_DECODE_DEVICE_DEFAULT if jpeg_decode_device is None else bool(jpeg_decode_device)


def jpeg_probe(data):
    """``specmi_jpeg_probe`` on a file's ``bytes`` -> (reason, H, W, sampling): reason is a name of ``_lib.JPEG_REASONS``
    ('supported' or why ``specmi_jpeg_decode`` refuses the file), sampling 420 or 444.  Host only: needs no device."""
    data = bytes(data)
    out = (C.c_int32 * 4)()
    p = [C.cast(C.byref(out, 4 * i), _lib.c_int32_p) for i in range(4)]
    rc = _lib.load().specmi_jpeg_probe(data, len(data), *p)
    if rc != _lib.OK:
        raise ValueError('specmi_jpeg_probe refused its arguments')
    return _lib.JPEG_REASONS[out[0]], int(out[1]), int(out[2]), int(out[3])


# Which route the .png frames the flows READ take (preprocess.decode_frames): False = Pillow decodes every file on the host and the
# raw frames go up (today's path, bit for bit), True = the files' zlib streams go up and specmi_png_decode inflates and unfilters
# the supported ones where they land.  Same pixels either way.  The rule is the JPEG rule: True only when
# scripts/bench_aux.py --only png_decode shows the device route ahead of 16 host threads in both content classes by more than the
# host route's own spread between rounds.  It is not in both (profiles/png_decode_aux.json, MI355X): 64 frames of 1080p 215.0 - 222.5 against
# 232.6 - 250.4 ms (spread 17.8), eight 1080 x 5760 three-panel pictures 476.6 - 480.1 against 134.0 - 142.1 ms (spread
# 8.1), identical slabs.  The inflate stage loses it: 73 of the 112 ms the kernels take on the frames, 370 of 464 on the
# pictures, where one wavefront resolves chains of dependent matches one at a time.  So the route is opt-in.
PNG_DECODE_DEVICE_DEFAULT = False


def flow_png_decode_device(png_decode_device=None) -> bool:
    """``png_decode_device`` (the flow's private switch) decides, None = the default."""
    return PNG_DECODE_DEVICE_DEFAULT if png_decode_device is None else bool(png_decode_device)


def png_probe(data):
    """``specmi_png_probe`` on a file's ``bytes`` -> (reason, H, W, colour_type, ranges): reason is a name of ``_lib.PNG_REASONS``
    ('supported' or why ``specmi_png_decode`` refuses the file); ranges (k, 2) int64 [offset, length] of the IDAT payloads, which
    joined are the file's zlib stream.  Host only: needs no device."""
    data = bytes(data)
    out = (C.c_int32 * 5)()
    p = [C.cast(C.byref(out, 4 * i), _lib.c_int32_p) for i in range(5)]
    ranges = np.zeros((64, 2), np.int64)
    for _ in range(2):
        rc = _lib.load().specmi_png_probe(data, len(data), p[0], p[1], p[2], p[3], ranges.ctypes.data_as(_lib.c_int64_p), ranges.shape[0], p[4])
        if rc != _lib.OK:
            raise ValueError('specmi_png_probe refused its arguments')
        if out[4] <= ranges.shape[0]:
            break
        ranges = np.zeros((int(out[4]), 2), np.int64)
    return _lib.PNG_REASONS[out[0]], int(out[1]), int(out[2]), int(out[3]), ranges[:int(out[4])].copy()


def png_stream(data, ranges) -> bytes:
    """The zlib stream of a file: its IDAT payloads (``png_probe``'s ranges) joined."""
    return b''.join(bytes(data[int(o):int(o + n)]) for o, n in ranges)


def png_takes_device(probe) -> bool:
    """Does a file with this ``png_probe`` answer go to the device?  Supported, and not beyond ``Image.MAX_IMAGE_PIXELS``: such a
    file takes the host route, so that Pillow's bomb warning or error stays what it is."""
    from PIL import Image
    limit = Image.MAX_IMAGE_PIXELS
    return probe[0] == 'supported' and (limit is None or probe[1] * probe[2] <= limit)


EVAL_STEP_OUTPUTS = ('err_sel', 'pa_err_sel', 'err_k', 'pa_err_k', 'v2v')
EVAL_STEP_MAX_JOINTS = 32      # kMaxJ of spec_amd/csrc/eval.hip: the joints are held on chip


def check_eval_step(B, V, J, nsel, joint_sel=None, Jk=0, pred_joints=False, gt_joints=False, joint_outputs=False):
    """Every refusal of ``specmi_eval_step`` (include/specmi.h) as ``ValueError``, and one more that only the host can make: an
    entry of ``joint_sel`` outside [0, J) (the library reads the selection from device memory and does not check it).
    ``joint_sel``: the selection on the host, or None for the first ``nsel`` joints; ``pred_joints`` / ``gt_joints``: is that
    joint set given; ``joint_outputs``: are ``err_k`` / ``pa_err_k`` asked for.  -> the selection as an int32 array, or None.
    Needs no device."""
    M = EVAL_STEP_MAX_JOINTS
    if B < 1 or V < 1:
        raise ValueError(f'{B} images of {V} vertices: at least one of each')
    if not (1 <= J <= M and 1 <= nsel <= M):
        raise ValueError(f'J = {J} and nsel = {nsel} must be in [1,{M}]')
    if joint_sel is None:
        if nsel > J:
            raise ValueError(f'joint_sel is None (the first nsel joints) but nsel = {nsel} exceeds J = {J}')
    else:
        joint_sel = np.ascontiguousarray(joint_sel, dtype=np.int64).reshape(-1)
        if joint_sel.shape[0] != nsel:
            raise ValueError(f'joint_sel holds {joint_sel.shape[0]} joints, nsel = {nsel}')
        if ((joint_sel < 0) | (joint_sel >= J)).any():
            raise ValueError(f'joint_sel names a joint outside [0,{J})')
        joint_sel = joint_sel.astype(np.int32)
    if bool(pred_joints) != bool(gt_joints):
        raise ValueError('pred_joints and gt_joints are given together or not at all')
    if joint_outputs and not pred_joints:
        raise ValueError('err_k / pa_err_k asked for without pred_joints and gt_joints')
    if pred_joints and not 1 <= Jk <= M:
        raise ValueError(f'Jk = {Jk} must be in [1,{M}]')
    return joint_sel


def check_hmr_loss_backward(B, V, terms_shape, counts_shape, want):
    """Every refusal of ``specmi_hmr_loss_backward`` (include/specmi.h) that is not already one of ``specmi_hmr_loss``, as
    ``ValueError``: ``terms`` / ``counts`` must be what the forward of the same batch produced, one output at least is wanted."""
    if B < 1 or V < 1:
        raise ValueError(f'{B} images of {V} vertices: at least one of each')
    if tuple(terms_shape) != (6, B) or tuple(counts_shape) != (2,):
        raise ValueError(f'terms must be (6, {B}) and counts (2,) as hmr_loss returned them, got {tuple(terms_shape)} and {tuple(counts_shape)}')
    if len(want) != 6 or not any(want):
        raise ValueError('want names the six prediction tensors (pred_pose, pred_shape, pred_cam, smpl_joints3d, smpl_joints2d, '
                         'smpl_vertices) and asks for one at least')


def check_smpl_backward(B, upstream, outputs, use_cam=False, camera=()):
    """Every refusal of ``specmi_smpl_backward`` (include/specmi.h) as ``ValueError``.  ``upstream``: which of g_vertices,
    g_joints3d, g_joints2d, g_cam_t are given (four truth values); ``outputs``: which of g_rotmat, g_betas, g_cam are wanted
    (three); ``camera``: which of the six camera arguments are given (read with ``use_cam`` only).  Needs no device."""
    if B < 1:
        raise ValueError(f'B = {B}: at least one image')
    if len(upstream) != 4 or len(outputs) != 3:
        raise ValueError('upstream names four gradients (vertices, joints3d, joints2d, cam_t), outputs three (rotmat, betas, cam)')
    if not any(upstream):
        raise ValueError('every upstream gradient is None (at least one of g_vertices, g_joints3d, g_joints2d, g_cam_t)')
    if not any(outputs):
        raise ValueError('no output is wanted (at least one of rotmat, betas, cam)')
    if use_cam and not (len(camera) == 6 and all(camera)):
        raise ValueError('use_cam needs cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h')


def check_rot6d_backward(x_shape, g_shape):
    """The shapes ``specmi_rot6d_backward`` takes: x6d (N, 6) or rows of 24 such rotations, g_rotmat with 9 numbers per rotation; -> N."""
    n = math.prod(x_shape)
    if n == 0 or n % 6 or x_shape[-1] % 6:
        raise ValueError(f'x6d must hold whole 6D rotations along its last axis, got shape {tuple(x_shape)}')
    if math.prod(g_shape) != n // 6 * 9:
        raise ValueError(f'g_rotmat of shape {tuple(g_shape)} does not hold {n // 6} 3x3 matrices')
    return n // 6


# pare's HMRHead: the width of fc1 / fc2, the rows of its three decoders = the widths of the record's pred_pose_6d | pred_shape | pred_cam,
# and the state vector they update
HMR_HEAD_HIDDEN = 1024
HMR_HEAD_DECODERS = {n: dict(PACKED_KEYS)[k][0] for n, k in (('decpose', 'pred_pose_6d'), ('decshape', 'pred_shape'), ('deccam', 'pred_cam'))}
HMR_HEAD_STATE = sum(HMR_HEAD_DECODERS.values())


def hmr_head_param_shapes(F, C):
    """name -> shape of the ten parameters of pare's HMRHead (``_lib.HMR_HEAD_PARAMS``) for F pooled features and C in (0, 7)."""
    H, rows = HMR_HEAD_HIDDEN, dict(HMR_HEAD_DECODERS, fc1=HMR_HEAD_HIDDEN, fc2=HMR_HEAD_HIDDEN)
    return {n: ((rows[n.split('.')[0]], F + HMR_HEAD_STATE + C if n == 'fc1.weight' else H) if n.endswith('weight') else
                (rows[n.split('.')[0]],)) for n in _lib.HMR_HEAD_PARAMS}


def hmr_head_tape_floats(B, n_iter):
    """What ``specmi_hmr_head_tape_floats`` answers, on the host."""
    return n_iter * B * (HMR_HEAD_STATE + 2 * HMR_HEAD_HIDDEN)


def check_hmr_head_train(B, F, C, n_iter, p=0.5, masks=False, param_shapes=None, cam_feats=None, ld_xf=None, outputs=None,
                         addresses=()):
    """Every refusal of ``specmi_hmr_head_train_forward`` / ``specmi_hmr_head_backward`` (include/specmi.h) as ``ValueError``,
    and the parameters' shapes, which the library cannot see.  ``masks``: are masks given; ``param_shapes``: name -> shape of the
    ten parameters (a missing or None entry is a NULL pointer), None = not checked; ``cam_feats``: is it given (None = as C
    says); ``ld_xf``: the row stride of xf (None = F); ``outputs``: which of g_xf and the ten parameter gradients are wanted
    (None = the forward, whose one output is required); ``addresses``: of the float tensors.  -> Kin.  Needs no device."""
    if not 1 <= B <= 1 << 20:
        raise ValueError(f'B = {B} must be in [1, 2^20]')
    if not 1 <= F <= 1 << 20:
        raise ValueError(f'F = {F} must be in [1, 2^20]')
    if C not in (0, 7):
        raise ValueError(f'C = {C} must be 0 or 7 (use_cam_feats)')
    if not 1 <= n_iter <= 3:
        raise ValueError(f'n_iter = {n_iter} must be in 1 .. 3')
    if masks and not 0.0 <= p < 1.0:
        raise ValueError(f'p = {p} must be in [0, 1) when masks are given')
    if param_shapes is not None:
        for name, shape in hmr_head_param_shapes(F, C).items():
            if param_shapes.get(name) is None:
                raise ValueError(f'{name} is missing')
            if tuple(param_shapes[name]) != shape:
                raise ValueError(f'{name} must be {shape} for F = {F}, C = {C}, got {tuple(param_shapes[name])}')
    if C == 7 and cam_feats is not None and not cam_feats:
        raise ValueError('cam_feats is required with C = 7')
    if any(a % 4 for a in addresses):
        raise ValueError('a float tensor is not 4-byte aligned')
    if ld_xf is not None and ld_xf < F:
        raise ValueError(f'the row stride of xf, {ld_xf}, is below the row length F = {F}')
    if outputs is not None and not any(outputs):
        raise ValueError('no output is wanted (g_xf or one parameter gradient at least)')
    return F + HMR_HEAD_STATE + C


def camcalib_head_param_names(L):
    """The state_dict names of CamCalib's three FC heads with L layers each (camcalib/model.py:59-70), ordered head, layer, weight
    / bias: ``fc_vfov.weight`` for one Linear, ``fc_vfov.0.weight`` .. for an ``nn.Sequential`` chain."""
    return tuple(f'{h}.{kind}' if L == 1 else f'{h}.{l}.{kind}' for h in _lib.CAMCALIB_HEADS for l in range(L) for kind in ('weight', 'bias'))


def camcalib_head_param_shapes(F, L, Hc, nbins):
    """name -> shape of the 6 L parameters of ``camcalib_head_param_names(L)``: widths F -> Hc -> .. -> nbins."""
    out = {}
    for h in _lib.CAMCALIB_HEADS:
        for l in range(L):
            nin, nout = (F if l == 0 else Hc), (nbins if l == L - 1 else Hc)
            stem = h if L == 1 else f'{h}.{l}'
            out[f'{stem}.weight'], out[f'{stem}.bias'] = (nout, nin), (nout,)
    return out


def camcalib_head_tape_floats(B, L, Hc):
    """What ``specmi_camcalib_head_tape_floats`` answers, on the host."""
    return 3 * (L - 1) * B * Hc


def check_camcalib_head_train(B, F, L, Hc, nbins, param_shapes=None, ld_xf=None, outputs=None, addresses=()):
    """Every refusal of ``specmi_camcalib_head_train_forward`` / ``specmi_camcalib_head_backward`` (include/specmi.h) as
    ``ValueError``, and the parameters' shapes, which the library cannot see.  ``param_shapes``: name -> shape of the 6 L
    parameters (a missing or None entry is a NULL pointer), None = not checked; ``ld_xf``: the row stride of xf (None = F);
    ``outputs``: which of g_xf and the 6 L parameter gradients are wanted (None = the forward, whose one output is required);
    ``addresses``: of the float tensors.  Needs no device."""
    if not 1 <= L <= _lib.CAMCALIB_HEAD_MAX_LAYERS:
        raise ValueError(f'L = {L} must be in 1 .. {_lib.CAMCALIB_HEAD_MAX_LAYERS}')
    for name, v in (('B', B), ('F', F), ('Hc', Hc), ('nbins', nbins)):
        if not 1 <= v <= 1 << 20:
            raise ValueError(f'{name} = {v} must be in [1, 2^20]')
    if param_shapes is not None:
        for name, shape in camcalib_head_param_shapes(F, L, Hc, nbins).items():
            if param_shapes.get(name) is None:
                raise ValueError(f'{name} is missing')
            if tuple(param_shapes[name]) != shape:
                raise ValueError(f'{name} must be {shape} for F = {F}, L = {L}, Hc = {Hc}, nbins = {nbins}, got {tuple(param_shapes[name])}')
    if any(a % 4 for a in addresses):
        raise ValueError('a float tensor is not 4-byte aligned')
    if ld_xf is not None and ld_xf < F:
        raise ValueError(f'the row stride of xf, {ld_xf}, is below the row length F = {F}')
    if outputs is not None and not any(outputs):
        raise ValueError('no output is wanted (g_xf or one parameter gradient at least)')


def check_camcalib_loss(B, nbins, loss_type, shapes=None, g_means_shape=None):
    """Every refusal of ``specmi_camcalib_loss`` / ``specmi_camcalib_loss_backward`` (include/specmi.h) as ``ValueError``, with the
    reference's text for an unknown ``loss_type`` (camcalib/loss.py:85).  ``shapes``: of the three logit and three target tensors
    (None = not checked); ``g_means_shape``: of the backward's upstream gradient.  -> SPECMI_LOSS_*.  Needs no device."""
    if loss_type not in _lib.LOSS_TYPES:
        raise ValueError(f'{loss_type} is not defined..')
    if not 1 <= B <= 1 << 20:
        raise ValueError(f'B = {B} must be in [1, 2^20]')
    if not 2 <= nbins <= 1 << 16:
        raise ValueError(f'nbins = {nbins} must be in [2, 2^16]')
    if shapes is not None:
        if len(shapes) != 6 or any(tuple(s) != (B, nbins) for s in shapes[:3]) or any(tuple(s) != (B,) for s in shapes[3:]):
            raise ValueError(f'three ({B}, {nbins}) logit tensors and three ({B},) targets, got {[tuple(s) for s in shapes]}')
    if g_means_shape is not None and tuple(g_means_shape) != (4,):
        raise ValueError(f'g_means must be (4,) = the gradients of loss, vfov_loss, pitch_loss, roll_loss, got {tuple(g_means_shape)}')
    return _lib.LOSS_TYPES[loss_type]


def out_dtype(dtype):
    """The ``dtype=`` keyword of the producers: torch.float32 -> the (n,3,H,W) fp32 image, torch.float16 -> NHWC8 fp16."""
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f'dtype must be torch.float32 ((n,3,H,W) images) or torch.float16 (NHWC8 (n,H,W,8) images), got {dtype}')
    return dtype == torch.float16


def image_tensor(n, H, W, device, f16: bool):
    return (torch.empty(n, H, W, 8, device=device, dtype=torch.float16) if f16 else
            torch.empty(n, 3, H, W, device=device, dtype=torch.float32))


def _image_out(out, n, H, W, f16: bool, device):
    """The image a producer writes: a fresh ``image_tensor``, or the caller's ``out=`` checked for shape, dtype, contiguity and
    device (a tensor on another device would hand the kernel a foreign pointer)."""
    if out is None:
        return image_tensor(n, H, W, device, f16)
    shape, dtype = ((n, H, W, 8), torch.float16) if f16 else ((n, 3, H, W), torch.float32)
    if tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != device:
        raise ValueError(f'out must be a contiguous {shape} {dtype} device tensor')
    return out


class Engine:
    def __init__(self, kind: str, device: torch.device):
        if device.type != 'cuda':
            raise RuntimeError('spec_amd runs on an AMD GPU (torch device "cuda"); there is no CPU path')
        self.lib = _lib.load()
        self.kind = kind
        self.device = torch.device('cuda', device.index if device.index is not None else torch.cuda.current_device())
        h = C.c_void_p()
        rc = self.lib.specmi_create(C.byref(h), self.device.index, KIND[kind])
        if rc != _lib.OK:
            raise _lib.SpecmiError(rc, (self.lib.specmi_last_error(None) or b'?').decode())
        self.h = h
        self.nbins = 256
        self.feat_channels = 2048
        self.num_verts = 0
        self._ld_opts = {}        # current value of the stride options ("output_ld", "angle_ld") on the handle

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.specmi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters ----------------------------------------------------------------------
    def set_option(self, name: str, value):
        if isinstance(value, float):
            _lib.check(self.h, self.lib.specmi_set_option_f32(self.h, name.encode(), value))
        else:
            _lib.check(self.h, self.lib.specmi_set_option_i32(self.h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        """The effective value of an integer option on this handle (what was set, else the library's default)."""
        v = C.c_int(0)
        _lib.check(self.h, self.lib.specmi_get_option_i32(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    # Precision of the ResNet trunk (include/specmi.h, "precision"): model state read by the next commit, not an option.
    PRECISIONS = {'fp32': _lib.PRECISION_FP32, 'fp16': _lib.PRECISION_FP16}

    def set_precision(self, precision: str):
        """'fp32' (default) or 'fp16' (the reference's TRAINING.USE_AMP trunk); takes effect at the next commit (load)."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {tuple(self.PRECISIONS)}")
        _lib.check(self.h, self.lib.specmi_set_precision(self.h, self.PRECISIONS[precision]))
        return self

    @property
    def precision(self) -> str:
        v = C.c_int(0)
        _lib.check(self.h, self.lib.specmi_get_precision(self.h, C.byref(v)))
        return {code: name for name, code in self.PRECISIONS.items()}[int(v.value)]

    def experimental(self, on: bool = True):
        """Let this handle accept the experimental option names (include/specmi.h): tuning thresholds, debug pins, opt-ins."""
        self.set_option('experimental', int(bool(on)))
        return self

    PLAN_NAMES = ('throughput', 'latency', 'single')

    def trunk_plan(self, B: int, H: int = 224, W: int = 224, pair: bool = False) -> str:
        """The execution plan a trunk forward of (B, 3, H, W) takes under the current options ('throughput' | 'latency' | 'single')."""
        mode = C.c_int32(0)
        _lib.check(self.h, self.lib.specmi_trunk_plan(self.h, int(B), int(H), int(W), int(bool(pair)), C.byref(mode)))
        return self.PLAN_NAMES[int(mode.value)]

    def sync_status(self) -> int:
        """Synchronises; 0 = every split-K arrival counter of this handle is back at zero, -2 = one is not (include/specmi.h)."""
        err = C.c_int32(0)
        _lib.check(self.h, self.lib.specmi_sync_status(self.h, C.byref(err)))
        return int(err.value)

    def sync_reset(self):
        _lib.check(self.h, self.lib.specmi_sync_reset(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def debug_poison_sync(self, value: int = 0xDEADBEEF):
        _lib.check(self.h, self.lib.specmi_debug_poison_sync(self.h, C.c_uint32(value)))

    def set_tensor(self, name: str, value):
        if isinstance(value, torch.Tensor):
            value = value.detach().cpu().numpy()
        a = np.asarray(value)
        if a.dtype.kind in 'iu' or a.dtype == np.bool_:
            a = np.ascontiguousarray(a, dtype=np.int32)
            fn = self.lib.specmi_set_tensor_i32
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            fn = self.lib.specmi_set_tensor_f32
        shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        _lib.check(self.h, fn(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    def load(self, tensors: Mapping[str, object], smpl: Optional[Mapping[str, object]] = None, **options):
        """Stage a state_dict-like mapping (+ the SMPL body model under 'smpl.*'), then commit."""
        for k, v in options.items():
            self.set_option(k, v)
        for k, v in tensors.items():
            if k.endswith('num_batches_tracked'):
                continue
            self.set_tensor(k, v)
        if smpl is not None:
            for k, v in smpl.items():
                self.set_tensor('smpl.' + k, v)
            self.num_verts = int(np.asarray(smpl['v_template']).shape[0]) if not isinstance(
                smpl['v_template'], torch.Tensor) else int(smpl['v_template'].shape[0])
        if 'fc_vfov.weight' in tensors:
            self.nbins = int(tensors['fc_vfov.weight'].shape[0])
        else:   # Sequential heads (num_fc_layers > 1): the last Linear of the chain has the bins
            last = [k for k in tensors if k.startswith('fc_vfov.') and k.endswith('.weight')]
            if last:
                self.nbins = int(tensors[sorted(last)[-1]].shape[0])
        self.feat_channels = {18: 512, 34: 512, 32: 480, 48: 720}.get(int(options.get('backbone', 50)), 2048)
        _lib.check(self.h, self.lib.specmi_commit(self.h))

    def _set_ld(self, name: str, value: int):
        if self._ld_opts.get(name, 0) != value:
            self.set_option(name, int(value))
            self._ld_opts[name] = value

    # ---- packed per-image record ------------------------------------------------
    def record_layout(self):
        """[(key, offset, per-image shape)] of the packed record the kernels can write directly:
        85,164 B of SPEC outputs + 12 B of camera angles = 21,294 floats for V = 6890."""
        lay, total = record_layout(self.num_verts)
        return list(lay), total

    def record_views(self, record: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Views of a (B, record_floats) record as the output dict (no copy)."""
        lay, total = record_layout(self.num_verts)
        if record.dim() != 2 or record.shape[1] != total or record.dtype != torch.float32 or record.stride(1) != 1:
            raise ValueError(f'record must be a (B, {total}) fp32 tensor with unit column stride')
        B = record.shape[0]
        return {k: record[:, off:off + math.prod(shp)].view(B, *shp) if shp else record[:, off] for k, off, shp in lay}

    # ---- forward ---------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, device=self.device, dtype=dtype)

    def _outputs(self, B, keys, views=None) -> Dict[str, torch.Tensor]:
        """The output dict of a call that writes ``keys`` of the record: those views of the caller's record, else fresh dense
        tensors of the table's shapes."""
        if views is not None:
            return {k: views[k] for k in keys}
        shapes = _record_shapes(self.num_verts)
        return {k: self._empty(B, *shapes[k]) for k in keys}

    def _hmr_outputs(self, B) -> Dict[str, torch.Tensor]:
        return self._outputs(B, _HMR_KEYS)

    def _images(self, images):
        if not isinstance(images, torch.Tensor) or images.device.type != 'cuda':
            raise RuntimeError('images must be a device tensor (no CPU path in spec_amd)')
        if images.dtype == torch.float16:
            raise ValueError('this call takes fp32 (B,3,H,W) images; fp16 NHWC8 images go to trunk / camcalib_forward / hmr_forward')
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f'images must be (B,3,H,W), got {tuple(images.shape)}')
        return images.to(device=self.device, dtype=torch.float32).contiguous()

    def _images_in(self, images):
        """-> (contiguous device tensor, B, H, W, f16): fp32 (B,3,H,W), or the fp16 trunk's NHWC8 (B,H,W,8) entrance (f16 = True:
        the call goes to the ``_f16in`` entry point)."""
        if isinstance(images, torch.Tensor) and images.dtype == torch.float16 and nhwc8_input(images, self.precision):
            if images.device.type != 'cuda':
                raise RuntimeError('images must be a device tensor (no CPU path in spec_amd)')
            x = images.to(device=self.device).contiguous()
            return x, x.shape[0], x.shape[1], x.shape[2], True
        x = self._images(images)
        return x, x.shape[0], x.shape[2], x.shape[3], False

    def trunk(self, images, stages=None):
        """The trunk's feature map (B, fh, fw, C) NHWC.  ``stages`` = 1 .. 4: the committed fp32 ResNet trunk cut after
        ``layer{stages}`` (``specmi_trunk_forward_stages`` - the frozen part of a fine-tuning step; 4 has this call's bits);
        ``None``: the whole trunk."""
        if stages is not None:
            return self._trunk_stages(images, stages)
        x, B, H, W, f16 = self._images_in(images)
        feat = self._empty(B, *self._feat_shape(H, W), self.feat_channels)
        if B == 0:
            return feat
        fn = self.lib.specmi_trunk_forward_f16in if f16 else self.lib.specmi_trunk_forward
        _lib.check(self.h, fn(self.h, _ptr(x), B, H, W, _ptr(feat), self._stream()))
        return feat

    def _trunk_stages(self, images, stages):
        if isinstance(stages, bool) or not isinstance(stages, int) or not 1 <= stages <= 4:
            raise ValueError(f'stages must be None or an int in 1 .. 4, got {stages!r}')
        x = self._images(images)
        B, _, H, W = x.shape
        out = self._empty(B, *self._feat_shape(H, W, stages), self.feat_channels >> (4 - stages))
        if B == 0:
            return out
        _lib.check(self.h, self.lib.specmi_trunk_forward_stages(self.h, _ptr(x), B, H, W, stages, _ptr(out), self._stream()))
        return out

    @staticmethod
    def _feat_shape(H, W, stages=4):
        """(fh, fw) of the trunk's feature map: the 7x7 stride-2 stem, then the max-pool and three stride-2 stages (3x3, pad 1);
        ``stages`` < 4: of the map after that stage."""
        def o(n, k, s, p):
            return (n + 2 * p - k) // s + 1
        fh, fw = o(H, 7, 2, 3), o(W, 7, 2, 3)
        for _ in range(stages):
            fh, fw = o(fh, 3, 2, 1), o(fw, 3, 2, 1)
        return fh, fw

    def trunk_pair(self, other: 'Engine', images, other_images):
        """The ResNet trunks of this engine and of ``other`` (same depth, same input shape) in lockstep, every layer of both
        as one grouped launch (``specmi_trunk_forward_pair``) -> (features of self, features of other), NHWC."""
        xa, xb = self._images(images), other._images(other_images)
        if xa.shape != xb.shape:
            raise ValueError(f'grouped trunk launches need equal input shapes, got {tuple(xa.shape)} and {tuple(xb.shape)}')
        B, _, H, W = xa.shape
        fh, fw = self._feat_shape(H, W)
        fa, fb = self._empty(B, fh, fw, self.feat_channels), self._empty(B, fh, fw, other.feat_channels)
        if B == 0:
            return fa, fb
        _lib.check(self.h, self.lib.specmi_trunk_forward_pair(self.h, other.h, _ptr(xa), _ptr(xb), B, H, W, _ptr(fa), _ptr(fb),
                                                              self._stream()))
        return fa, fb

    def camcalib_head(self, feat_nhwc):
        """avg-pool + the three Linear chains of CameraRegressorNetwork.forward from a trunk feature map."""
        f = _dev_f32(feat_nhwc, self.device)
        B, fh, fw, _ = f.shape
        out = self._empty(3, B, self.nbins)
        if B == 0:
            return [out[0], out[1], out[2]]
        _lib.check(self.h, self.lib.specmi_camcalib_head_forward(self.h, _ptr(f), B, fh, fw, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                                                 self._stream()))
        return [out[0], out[1], out[2]]

    def camcalib_forward(self, images):
        x, B, H, W, f16 = self._images_in(images)
        out = self._empty(3, B, self.nbins)
        if B == 0:                      # an empty batch gives empty outputs, as the reference's torch modules do
            return [out[0], out[1], out[2]]
        fn = self.lib.specmi_camcalib_forward_f16in if f16 else self.lib.specmi_camcalib_forward
        _lib.check(self.h, fn(
            self.h, _ptr(x), B, H, W, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), self._stream()))
        return [out[0], out[1], out[2]]

    def camcalib_head_decode(self, feat_nhwc, img_h=None, img_w=None, angles_out=None):
        """``camcalib_head`` + ``camcalib_decode`` as one call (one launch at small batches: ``specmi_camcalib_head_decode``) ->
        ([logits_vfov, logits_pitch, logits_roll], dict(vfov, pitch, roll, f_pix, cam_rotmat, cam_intrinsics))."""
        f = _dev_f32(feat_nhwc, self.device)
        B, fh, fw, _ = f.shape
        out = self._empty(3, B, self.nbins)
        img_h = _dev_f32(img_h, self.device, (B,))
        img_w = _dev_f32(img_w, self.device, (B,))
        cam = self._camera_outputs(B, img_h, img_w, angles_out)
        if B > 0:
            _lib.check(self.h, self.lib.specmi_camcalib_head_decode(
                self.h, _ptr(f), B, fh, fw, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(img_h), _ptr(img_w),
                *(_ptr(t) for t in cam.values()), self._stream()))
        return [out[0], out[1], out[2]], cam

    def _camera_outputs(self, B, img_h, img_w, angles_out) -> Dict[str, Optional[torch.Tensor]]:
        """What a decode call writes, in the order of its pointer arguments; sets the handle's angle stride ("angle_ld") for
        ``angles_out`` (see ``camcalib_decode``)."""
        if angles_out is not None:
            vf, pt, rl = angles_out
            ld = vf.stride(0) if B > 1 else 1
            if any(t.shape != (B,) or t.dtype != torch.float32 or (B > 1 and t.stride(0) != ld) for t in (vf, pt, rl)):
                raise ValueError('angles_out: three (B,) fp32 tensors with one common stride')
            self._set_ld('angle_ld', ld if ld != 1 else 0)
        else:
            vf, pt, rl = self._empty(B), self._empty(B), self._empty(B)
            self._set_ld('angle_ld', 0)
        return {'vfov': vf, 'pitch': pt, 'roll': rl, 'f_pix': self._empty(B) if img_h is not None else None,
                'cam_rotmat': self._empty(B, 3, 3),
                'cam_intrinsics': self._empty(B, 3, 3) if (img_h is not None and img_w is not None) else None}

    def camcalib_decode(self, lv, lp, lr, img_h=None, img_w=None, angles_out=None):
        """``angles_out``: optional (vfov, pitch, roll) tensors of shape (B,) with a common element stride
        (e.g. three columns of the packed record) that the kernel writes directly."""
        lv, lp, lr = (_dev_f32(t, self.device) for t in (lv, lp, lr))
        B, nb = lv.shape
        img_h = _dev_f32(img_h, self.device, (B,))
        img_w = _dev_f32(img_w, self.device, (B,))
        cam = self._camera_outputs(B, img_h, img_w, angles_out)
        _lib.check(self.h, self.lib.specmi_camcalib_decode(
            self.h, _ptr(lv), _ptr(lp), _ptr(lr), B, nb, _ptr(img_h), _ptr(img_w), *(_ptr(t) for t in cam.values()), self._stream()))
        return cam

    def camcalib_bins(self, logits, argmax=True, soft=False):
        """Per-row argmax (int32) and / or normalised soft-argmax of (..., nbins) device logits."""
        x = _dev_f32(logits, self.device)
        nb = x.shape[-1]
        rows = x.numel() // nb
        idx = torch.empty(x.shape[:-1], device=self.device, dtype=torch.int32) if argmax else None
        sf = torch.empty(x.shape[:-1], device=self.device, dtype=torch.float32) if soft else None
        _lib.check(self.h, self.lib.specmi_camcalib_bins(self.h, _ptr(x), rows, nb, _ptr(idx), _ptr(sf), self._stream()))
        return idx, sf

    def camcalib_eval(self, lv, lp, lr, targets, gts, loss_type, weights=(1.0, 1.0, 1.0)):
        """``specmi_camcalib_eval``: the loss terms, decode and angle errors of CamCalib's test step on three (B, nbins) logit
        tensors.  ``targets``: three (B,) arrays - integer bin indices for 'ce' / 'kl', fp32 soft indices for the soft-argmax losses;
        ``gts``: three (B,) angles in radians.  -> dict(loss_term, argmax, soft, angle, err: (3, B) device tensors in the order
        vfov, pitch, roll; means: (7,) = loss, vfov_loss, pitch_loss, roll_loss, vfov_acc, pitch_acc, roll_acc [degrees])."""
        if loss_type not in _lib.LOSS_TYPES:
            raise ValueError(f'{loss_type} is not defined..')
        lv, lp, lr = (_dev_f32(t, self.device) for t in (lv, lp, lr))
        B, nb = lv.shape
        if lp.shape != (B, nb) or lr.shape != (B, nb):
            raise ValueError('the three logit tensors must have one shape')
        tdt = torch.int32 if loss_type in ('ce', 'kl') else torch.float32
        tg = [torch.as_tensor(np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t)).to(device=self.device, dtype=tdt).contiguous()
              for t in targets]
        gt = [_dev_f32(g, self.device, (B,)) for g in gts]
        if any(t.shape != (B,) for t in tg):
            raise ValueError('targets: three (B,) arrays')
        res = {'loss_term': self._empty(3, B), 'argmax': self._empty(3, B, dtype=torch.int32), 'soft': self._empty(3, B),
               'angle': self._empty(3, B), 'err': self._empty(3, B), 'means': self._empty(7)}
        if B > 0:
            _lib.check(self.h, self.lib.specmi_camcalib_eval(
                self.h, _ptr(lv), _ptr(lp), _ptr(lr), B, nb, _lib.LOSS_TYPES[loss_type], _ptr(tg[0]), _ptr(tg[1]), _ptr(tg[2]),
                _ptr(gt[0]), _ptr(gt[1]), _ptr(gt[2]), float(weights[0]), float(weights[1]), float(weights[2]), _ptr(res['loss_term']),
                _ptr(res['argmax']), _ptr(res['soft']), _ptr(res['angle']), _ptr(res['err']), _ptr(res['means']), self._stream()))
        return res

    def _hmr_loss_args(self, mode, pred, gt, weights):
        """The 16 tensors of ``specmi_hmr_loss`` / ``specmi_hmr_loss_backward`` in the prototype's order, checked -> (args, B, V)."""
        if mode not in (_lib.HMR_LOSS, _lib.HMR_CAM_LOSS):
            raise ValueError(f'mode must be 0 (HMRLoss) or 1 (HMRCamLoss), got {mode!r}')
        if len(weights) != len(HMR_LOSS_WEIGHTS):
            raise ValueError(f'weights: {len(HMR_LOSS_WEIGHTS)} values in the order {HMR_LOSS_WEIGHTS}')
        verts = _dev_f32(pred['smpl_vertices'], self.device)
        if verts.dim() != 3 or verts.shape[2] != 3 or min(verts.shape[:2]) < 1:
            raise ValueError(f'smpl_vertices must be (B, V, 3) with B, V >= 1, got {tuple(verts.shape)}')
        B, V = int(verts.shape[0]), int(verts.shape[1])
        args = [verts if k == 'smpl_vertices' else _dev_f32(pred[k], self.device, (B,) + shp) for k, shp in HMR_LOSS_INPUTS['pred']]
        for k, shp in HMR_LOSS_INPUTS['gt']:
            shp = (B,) + ((V, 3) if shp is None else shp)
            if k in ('has_smpl', 'has_pose_3d'):      # .bool() of the reference: non-zero = annotated
                m = gt[k] if isinstance(gt[k], torch.Tensor) else torch.as_tensor(np.asarray(gt[k]))
                m = (m.to(self.device) != 0).to(torch.int32).contiguous()
                if tuple(m.shape) != shp:
                    raise ValueError(f'{k}: expected shape {shp}, got {tuple(m.shape)}')
                args.append(m)
            elif k == 'vertices':
                v = gt.get('vertices')
                if v is None and float(weights[0]) != 0.0:
                    raise ValueError("gt['vertices'] is needed when shape_loss_weight != 0 (spec_amd.losses.gt_vertices makes them)")
                args.append(_dev_f32(v, self.device, shp))
            elif k in ('orig_shape', 'scale'):
                args.append(_dev_f32(gt[k], self.device, shp) if mode == _lib.HMR_CAM_LOSS else None)
            else:
                args.append(_dev_f32(gt['keypoints_orig' if (k == 'keypoints' and mode == _lib.HMR_CAM_LOSS) else k], self.device, shp))
        return args, B, V

    def hmr_loss(self, mode, pred, gt, weights, out=None):
        """``specmi_hmr_loss``: the forward value of the reference's HMRLoss (``mode`` 0) / HMRCamLoss (``mode`` 1).  ``pred``
        and ``gt`` map the names of ``HMR_LOSS_INPUTS`` to tensors or arrays ((B, ...) each; gt['vertices'] may be None when the
        shape weight is 0; 'orig_shape' as (H, W) and 'scale' are read in mode 1 only), ``weights`` the eight constructor
        arguments in ``HMR_LOSS_WEIGHTS`` order.  -> dict(terms (6, B), counts (2,) int32 = Nv, Np, means (7,) in
        ``HMR_LOSS_KEYS`` order), device tensors; ``out`` supplies them (a captured graph replays into the same three)."""
        args, B, V = self._hmr_loss_args(mode, pred, gt, weights)
        res = out if out is not None else {'terms': self._empty(6, B), 'counts': self._empty(2, dtype=torch.int32), 'means': self._empty(len(HMR_LOSS_KEYS))}
        for k, shp, dt in (('terms', (6, B), torch.float32), ('counts', (2,), torch.int32), ('means', (len(HMR_LOSS_KEYS),), torch.float32)):
            if tuple(res[k].shape) != shp or res[k].dtype != dt or not res[k].is_contiguous() or res[k].device != self.device:
                raise ValueError(f'out[{k!r}] must be a contiguous {shp} {dt} tensor on the engine device')
        _lib.check(self.h, self.lib.specmi_hmr_loss(self.h, int(mode), *(_ptr(t) for t in args), B, V, *(float(w) for w in weights),
                                                    _ptr(res['terms']), _ptr(res['counts']), _ptr(res['means']), self._stream()))
        return res

    def hmr_loss_backward(self, mode, pred, gt, weights, res, g_means, want=(True,) * 6):
        """``specmi_hmr_loss_backward``: the gradient of the seven means of ``hmr_loss`` with respect to the six prediction tensors.
        ``pred``, ``gt``, ``weights`` as given to ``hmr_loss``, ``res`` what it returned (``terms`` and ``counts`` are read),
        ``g_means`` (7) the upstream gradient; -> {key of ``pred``: gradient, or None where ``want`` (in the order of
        ``HMR_LOSS_INPUTS['pred']``) says not wanted}."""
        args, B, V = self._hmr_loss_args(mode, pred, gt, weights)
        check_hmr_loss_backward(B, V, tuple(res['terms'].shape), tuple(res['counts'].shape), want)
        for k, dt in (('terms', torch.float32), ('counts', torch.int32)):
            if res[k].dtype != dt or not res[k].is_contiguous() or res[k].device != self.device:
                raise ValueError(f'res[{k!r}] must be the contiguous {dt} tensor hmr_loss returned, on the engine device')
        gm = _dev_f32(g_means, self.device, (len(HMR_LOSS_KEYS),))
        out = [torch.empty_like(a) if w else None for a, w in zip(args[:6], want)]
        _lib.check(self.h, self.lib.specmi_hmr_loss_backward(
            self.h, int(mode), *(_ptr(t) for t in args), B, V, *(float(w) for w in weights), _ptr(res['terms']), _ptr(res['counts']),
            _ptr(gm), *(_ptr(o) for o in out), self._stream()))
        return {k: o for (k, _), o in zip(HMR_LOSS_INPUTS['pred'], out)}

    def eval_step(self, pred_vertices, gt_vertices, J_regressor, joint_sel=None, nsel=None, pred_joints=None, gt_joints=None,
                  outputs=None):
        """``specmi_eval_step``: what the reference's validation step scores for a batch, per joint and in METRES, in one launch.
        ``pred_vertices`` / ``gt_vertices`` (B, V, 3), ``J_regressor`` (J, V), ``joint_sel`` a host sequence of joint indices (None:
        the first ``nsel`` joints, ``nsel`` None: all J), ``pred_joints`` / ``gt_joints`` (B, Jk, 3) or both None.  ``outputs``: the
        names of ``EVAL_STEP_OUTPUTS`` to compute (None: all the inputs allow).  -> {name: device tensor}: err_sel, pa_err_sel
        (B, nsel), err_k, pa_err_k (B, Jk), v2v (B,)."""
        pv = _dev_f32(pred_vertices, self.device)
        if pv.dim() != 3 or pv.shape[2] != 3:
            raise ValueError(f'pred_vertices must be (B, V, 3), got {tuple(pv.shape)}')
        B, V = int(pv.shape[0]), int(pv.shape[1])
        gv = _dev_f32(gt_vertices, self.device, (B, V, 3))
        Jr = _dev_f32(J_regressor, self.device)
        if Jr.dim() != 2 or Jr.shape[1] != V:
            raise ValueError(f'J_regressor must be (J, {V}), got {tuple(Jr.shape)}')
        J = int(Jr.shape[0])
        if joint_sel is not None:
            joint_sel = [int(j) for j in joint_sel]
            nsel = len(joint_sel) if nsel is None else nsel
        nsel = J if nsel is None else int(nsel)
        pj = _dev_f32(pred_joints, self.device)
        if pj is not None and (pj.dim() != 3 or pj.shape[0] != B or pj.shape[2] != 3):
            raise ValueError(f'pred_joints must be ({B}, Jk, 3), got {tuple(pj.shape)}')
        Jk = int(pj.shape[1]) if pj is not None else 0
        names = tuple(k for k in EVAL_STEP_OUTPUTS if pred_joints is not None or k not in ('err_k', 'pa_err_k')) if outputs is None else tuple(outputs)
        if set(names) - set(EVAL_STEP_OUTPUTS):
            raise ValueError(f'outputs: names of {EVAL_STEP_OUTPUTS}, got {names}')
        sel = check_eval_step(B, V, J, nsel, joint_sel, Jk, pred_joints is not None, gt_joints is not None,
                              'err_k' in names or 'pa_err_k' in names)
        gj = _dev_f32(gt_joints, self.device, (B, Jk, 3))
        sel_t = None if sel is None else torch.from_numpy(sel).to(self.device)
        shapes = {'err_sel': (B, nsel), 'pa_err_sel': (B, nsel), 'err_k': (B, Jk), 'pa_err_k': (B, Jk), 'v2v': (B,)}
        res = {k: self._empty(*shapes[k]) for k in names}
        _lib.check(self.h, self.lib.specmi_eval_step(self.h, _ptr(pv), _ptr(gv), B, V, _ptr(Jr), J, _ptr(sel_t), nsel, _ptr(pj), _ptr(gj), Jk,
                                                     *(_ptr(res.get(k)) for k in EVAL_STEP_OUTPUTS), self._stream()))
        return res

    def resize_normalize_ragged(self, slab, offsets, geom, out=None, dtype=torch.float32):
        """``specmi_resize_normalize_ragged``: ``slab`` = 1-D uint8 device tensor holding n RGB HWC frames, ``offsets`` (n,) byte
        offsets, ``geom`` (n, 4) [H, W, OH, OW] (both on the host) -> (n, 3, max OH, max OW) fp32, frame f in the top-left
        corner of its image, exact zeros elsewhere.  ``dtype=torch.float16``: (n, max OH, max OW, 8) NHWC8 fp16
        (``specmi_resize_normalize_ragged_f16``), the same values rounded once."""
        f16 = out_dtype(dtype)
        if not isinstance(slab, torch.Tensor) or slab.device.type != 'cuda' or slab.dtype != torch.uint8 or slab.dim() != 1:
            raise ValueError('slab must be a 1-D uint8 device tensor')
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        geom = np.ascontiguousarray(geom, dtype=np.int32).reshape(-1, 4)
        n = geom.shape[0]
        if n < 1 or offsets.shape[0] != n:
            raise ValueError('one offset and one [H, W, OH, OW] row per frame (at least one frame)')
        Hmax, Wmax = int(geom[:, 2].max()), int(geom[:, 3].max())
        out = _image_out(out, n, Hmax, Wmax, f16, self.device)
        fn = self.lib.specmi_resize_normalize_ragged_f16 if f16 else self.lib.specmi_resize_normalize_ragged
        _lib.check(self.h, fn(
            self.h, _ptr(slab.contiguous()), slab.numel(), offsets.ctypes.data_as(_lib.c_int64_p), geom.ctypes.data_as(_lib.c_int32_p),
            n, Hmax, Wmax, _ptr(out), self._stream()))
        return out

    def pano_extract_views(self, pano, views, out_hw, offsets=None, out=None):
        """``specmi_pano_extract_views``: ``pano`` = (PH, PW, 3) uint8 device tensor, ``views`` (n, 5) float64 [elevation, azimuth,
        roll (rad), vfov (deg), ratio], ``out_hw`` (n, 2) - both on the host -> (1-D uint8 device slab, (n,) byte offsets): view f
        is the (H_f, W_f, 3) block at ``offsets[f]``.  Default offsets pack the views back to back; ``out`` supplies the slab."""
        if (not isinstance(pano, torch.Tensor) or pano.device != self.device or pano.dtype != torch.uint8 or pano.dim() != 3
                or pano.shape[2] != 3 or not pano.is_contiguous()):
            raise ValueError('pano must be a contiguous (PH, PW, 3) uint8 tensor on the engine device')
        views = np.ascontiguousarray(views, dtype=np.float64).reshape(-1, 5)
        out_hw = np.ascontiguousarray(out_hw, dtype=np.int32).reshape(-1, 2)
        n = views.shape[0]
        if out_hw.shape[0] != n:
            raise ValueError('one [H, W] row per view')
        nbytes = out_hw.astype(np.int64).prod(axis=1) * 3
        if offsets is None:
            offsets = starts(nbytes)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.shape[0] != n:
            raise ValueError('one offset per view')
        if out is None:
            out = torch.empty(int((offsets + nbytes).max()) if n else 0, device=self.device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != self.device:
            raise ValueError('out must be a contiguous 1-D uint8 device tensor')
        _lib.check(self.h, self.lib.specmi_pano_extract_views(
            self.h, _ptr(pano), int(pano.shape[0]), int(pano.shape[1]), views.ctypes.data_as(_lib.c_double_p),
            out_hw.ctypes.data_as(_lib.c_int32_p), offsets.ctypes.data_as(_lib.c_int64_p), out.numel(), _ptr(out), n, self._stream()))
        return out, offsets

    def render_meshes(self, vertices, faces, cam_t, R, focal, center, frame=None, size=None, rgb=(1., 1., 1.), flags=0, maps=False):
        """``specmi_render_meshes``: ``vertices`` (M, V, 3) / ``cam_t`` (M, 3) / ``R`` (3, 3) fp32 and ``faces`` (F, 3) int32 on the
        engine device, ``focal`` = (fx, fy), ``center`` = (cx, cy), ``frame`` (H, W, 3) uint8 (may be None in side view, then
        ``size`` = (H, W)), ``flags`` of ``_lib.RENDER_*``.  -> the (H, W, 3) uint8 image; with ``maps`` a dict that also holds
        ``id_map`` (H, W) int32, ``depth`` (H, W) fp32, ``screen_xy`` (M, V, 2) int32 and ``screen_z`` (M, V) fp32.
        Everything is checked here, before the library is called."""
        d = self.device
        M, V, F = _mesh_inputs(vertices, faces, cam_t, d, 1)
        _dev_tensor('R', R, torch.float32, d)
        if tuple(R.shape) != (3, 3):
            raise ValueError('R must be (3, 3)')
        side = bool(flags & _lib.RENDER_SIDE_VIEW)
        if flags & ~15 or (flags & _lib.RENDER_GROUND_PLANE and not side):
            raise ValueError('flags: RENDER_SIDE_VIEW | RENDER_GROUND_PLANE (side view only) | RENDER_CULL | RENDER_THREAD_PER_TRIANGLE')
        if frame is not None:
            if (not isinstance(frame, torch.Tensor) or frame.device != d or frame.dtype != torch.uint8 or frame.dim() != 3
                    or frame.shape[2] != 3 or not frame.is_contiguous()):
                raise ValueError('frame must be a contiguous (H, W, 3) uint8 tensor on the engine device')
            size = tuple(frame.shape[:2])
        elif not side or size is None:
            raise ValueError('an overlay needs its frame; a side view its frame or size=(H, W)')
        H, W = int(size[0]), int(size[1])
        if not (1 <= H <= 32768 and 1 <= W <= 32768):
            raise ValueError('a frame of 1 .. 32768 pixels per side')
        cam = [float(focal[0]), float(focal[1]), float(center[0]), float(center[1])]
        if not (all(np.isfinite(cam)) and cam[0] > 0 and cam[1] > 0):
            raise ValueError('focal lengths must be positive and finite, the centre finite')
        rgb = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1)
        if rgb.shape[0] != 3 or not np.isfinite(rgb).all():
            raise ValueError('rgb: three finite floats in [0, 1]')
        out = torch.empty(H, W, 3, device=d, dtype=torch.uint8)
        id_map = torch.empty(H, W, device=d, dtype=torch.int32) if maps else None
        depth = torch.empty(H, W, device=d, dtype=torch.float32) if maps else None
        screen = torch.empty(M, V, 3, device=d, dtype=torch.int32) if maps else None
        _lib.check(self.h, self.lib.specmi_render_meshes(
            self.h, _ptr(vertices), M, V, _ptr(faces), F, _ptr(cam_t), _ptr(R), *cam, _ptr(frame), H, W,
            rgb.ctypes.data_as(_lib.c_float_p), int(flags), _ptr(out), _ptr(id_map), _ptr(depth), _ptr(screen), self._stream()))
        if not maps:
            return out
        return {'image': out, 'id_map': id_map, 'depth': depth, 'screen_xy': screen[..., :2], 'screen_z': screen[..., 2].contiguous().view(torch.float32)}

    def render_views(self, vertices, faces, cam_t, geom, offsets, cams, in_slab, out_slab, rgb=(1., 1., 1.), maps=False):
        """``specmi_render_views``: many views - each what one ``render_meshes`` call draws - in one call.  ``vertices``
        (Mtot, V, 3) / ``cam_t`` (Mtot, 3) fp32 and ``faces`` (F, 3) int32 on the engine device; the view record as three host
        arrays, one row per view: ``geom`` (n, 5) [H, W, mesh0, count, flags], ``offsets`` (n, 4) [in_offset (-1: none), in_pitch,
        out_offset, out_pitch] in bytes, ``cams`` (n, 13) [R row-major, fx, fy, cx, cy] (``render.plan_views`` lays them out);
        ``in_slab`` (1-D uint8, what ``pack_frames`` builds; None when no view names a frame) and ``out_slab`` (1-D uint8), both
        on the engine device and not overlapping.  Writes the views into ``out_slab`` and returns it; with ``maps`` a dict that
        also holds ``id_map`` int32 and ``depth`` fp32 (the views' H * W back to back), ``screen_xy`` (P, V, 2) int32 and
        ``screen_z`` (P, V) fp32 (P = the (view, mesh) pairs in view order).  Everything is checked here, before the library is
        called (``check_render_views``)."""
        d = self.device
        Mtot, V, F = _mesh_inputs(vertices, faces, cam_t, d, 0)
        _u8_slab('in_slab', in_slab, d, optional=True)
        _u8_slab('out_slab', out_slab, d)
        if in_slab is not None and in_slab.data_ptr() < out_slab.data_ptr() + out_slab.numel() and out_slab.data_ptr() < in_slab.data_ptr() + in_slab.numel():
            raise ValueError('in_slab and out_slab overlap')
        geom, offsets, cams, rgb = check_render_views(Mtot, V, F, geom, offsets, cams, None if in_slab is None else in_slab.numel(), out_slab.numel(), rgb)
        n, px, pairs = geom.shape[0], int((geom[:, 0].astype(np.int64) * geom[:, 1]).sum()), int(geom[:, 3].sum())
        id_map = torch.empty(px, device=d, dtype=torch.int32) if maps else None
        depth = torch.empty(px, device=d, dtype=torch.float32) if maps else None
        screen = torch.empty(pairs, V, 3, device=d, dtype=torch.int32) if maps else None
        _lib.check(self.h, self.lib.specmi_render_views(
            self.h, _ptr(vertices), Mtot, V, _ptr(faces), F, _ptr(cam_t), rgb.ctypes.data_as(_lib.c_float_p),
            _ptr(in_slab), 0 if in_slab is None else in_slab.numel(), _ptr(out_slab), out_slab.numel(),
            geom.ctypes.data_as(_lib.c_int32_p), offsets.ctypes.data_as(_lib.c_int64_p), cams.ctypes.data_as(_lib.c_float_p), n,
            _ptr(id_map), _ptr(depth), _ptr(screen), self._stream()))
        if not maps:
            return out_slab
        return {'slab': out_slab, 'id_map': id_map, 'depth': depth, 'screen_xy': screen[..., :2], 'screen_z': screen[..., 2].contiguous().view(torch.float32)}

    def draw_skeletons(self, kp, slab, geom, offsets, bones=None, style=None):
        """``specmi_draw_skeletons``: the 2D skeletons of ``kp`` (Mtot, J, D) fp32 on the engine device - D = 2 (x, y) or 3
        (x, y, confidence), in pixels of the detection's frame - painted in place into the frames of ``slab`` (1-D uint8 on the
        engine device; what ``pack_frames`` builds, or the panel-0 columns of pictures).  The frame record as two host arrays, one
        row per frame: ``geom`` (n, 4) [H, W, det0, count] and ``offsets`` (n, 2) [byte offset, pitch]; ``bones`` (NB, 2) joint
        indices (None = ``constants.SKELETON_SPIN``, which needs J = 49; an empty table draws joints only), ``style`` a
        ``_lib.DrawStyle`` (None = radius 4, thickness 2, threshold 0.3, green joints, blue / red bones).  Returns ``slab``.
        Everything is checked here, before the library is called (``check_draw_skeletons``)."""
        d = self.device
        _dev_tensor('kp', kp, torch.float32, d)
        if kp.dim() != 3:
            raise ValueError('kp must be (Mtot, J, D)')
        _u8_slab('slab', slab, d)
        if bones is None:
            from .constants import SKELETON_SPIN
            bones = SKELETON_SPIN
        Mtot, J, D = (int(x) for x in kp.shape)
        bones, geom, offsets, style = check_draw_skeletons(Mtot, J, D, bones, geom, offsets, slab.numel(), style)
        _lib.check(self.h, self.lib.specmi_draw_skeletons(
            self.h, _ptr(kp), Mtot, J, D, bones.ctypes.data_as(_lib.c_int32_p) if bones.shape[0] else None, int(bones.shape[0]), C.byref(style),
            _ptr(slab), slab.numel(), geom.ctypes.data_as(_lib.c_int32_p), offsets.ctypes.data_as(_lib.c_int64_p), int(geom.shape[0]),
            self._stream()))
        return slab

    def draw_marks(self, slab, geom, offsets, marks, masks=None):
        """``specmi_draw_marks``: strips, mask blends and Pillow's wide lines drawn in place into the frames of ``slab`` (1-D
        uint8 on the engine device; what ``pack_frames`` builds, or the panel-0 columns of pictures), every frame of the call in
        one launch.  Host arrays: ``geom`` (n, 4) [H, W, mark0, count], ``offsets`` (n, 2) [byte offset, pitch] and ``marks``
        (nmarks, 8) int64 [kind, r | g << 8 | b << 16, p0 .. p5] (``check_draw_marks``; ``render.horizon_marks`` builds the marks
        of a horizon line).  ``masks``: the 1-D uint8 device buffer the mask blends index (None: no mask blend).  Returns
        ``slab``.  Everything the host arrays decide is checked here, before the library is called."""
        _u8_slab('slab', slab, self.device)
        _u8_slab('masks', masks, self.device, optional=True)
        geom, offsets, marks = check_draw_marks(geom, offsets, marks, slab.numel(), 0 if masks is None else masks.numel())
        _lib.check(self.h, self.lib.specmi_draw_marks(
            self.h, _ptr(slab), slab.numel(), geom.ctypes.data_as(_lib.c_int32_p), offsets.ctypes.data_as(_lib.c_int64_p), int(geom.shape[0]),
            marks.ctypes.data_as(_lib.c_int64_p) if marks.shape[0] else None, int(marks.shape[0]), _ptr(masks),
            0 if masks is None else masks.numel(), self._stream()))
        return slab

    def color_jitter(self, slab, offsets, sizes, records, out=None, out_offsets=None):
        """``specmi_color_jitter``: torchvision's ColorJitter, in Pillow's bytes, on the frames of ``slab`` (1-D uint8 on the engine
        device: what ``pack_frames``, the decoders and ``pano_extract_views`` build).  Host arrays: ``offsets`` (n,) byte offsets
        of dense frames or (n, 2) [byte offset, pitch], ``sizes`` (n, 2) [H, W], ``records`` (n, 8) int32 (``augment.ColorJitter
        .records``).  ``out``: the slab the jittered frames go to - None: a new slab of the same size, ``slab`` itself: in place -
        at ``out_offsets`` (None: the same rectangles).  Returns ``out``.  Everything the host arrays decide is checked here,
        before the library is called (``check_color_jitter``)."""
        _u8_slab('slab', slab, self.device)
        if out is None:
            out = torch.empty_like(slab)
        _u8_slab('out', out, self.device)
        sizes = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1, 2)

        def pitched(o):
            o = np.ascontiguousarray(o, dtype=np.int64)
            if o.ndim == 1 and o.shape[0] == sizes.shape[0]:
                o = np.stack([o, 3 * sizes[:, 1]], axis=1)
            if o.ndim != 2 or o.shape != (sizes.shape[0], 2):
                raise ValueError('offsets: (n,) byte offsets of dense frames or (n, 2) [byte offset, pitch]')
            return o
        in_o = pitched(offsets)
        both = np.concatenate([in_o, in_o if out_offsets is None else pitched(out_offsets)], axis=1)
        in_place = out.data_ptr() == slab.data_ptr()
        if not in_place and slab.data_ptr() < out.data_ptr() + out.numel() and out.data_ptr() < slab.data_ptr() + slab.numel():
            raise ValueError('slab and out overlap without being the same slab')
        geom, both, records = check_color_jitter(sizes, both, records, slab.numel(), out.numel(), in_place)
        _lib.check(self.h, self.lib.specmi_color_jitter(
            self.h, _ptr(slab), slab.numel(), _ptr(out), out.numel(), geom.ctypes.data_as(_lib.c_int32_p), both.ctypes.data_as(_lib.c_int64_p),
            records.ctypes.data_as(_lib.c_int32_p), int(geom.shape[0]), self._stream()))
        return out

    def denormalize_u8(self, x, index, H, W, slab=None, offset=0, pitch=None, mean=None, std=None):
        """``specmi_denormalize_u8``: image ``index`` of ``x`` (B, 3, Hp, Wp) fp32 on the engine device, cut to its top-left
        ``H`` x ``W``, as an HWC uint8 frame at byte ``offset`` / ``pitch`` (None = 3 W) of ``slab`` (1-D uint8; None: a new
        slab of that one frame).  v = (x * std + mean) * 255 in fp32, NaN -> 0, clamped to [0, 255], truncated; ``mean`` /
        ``std`` None = ImageNet's.  Returns ``slab``."""
        d = self.device
        if not isinstance(x, torch.Tensor) or x.device != d or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError('x must be a contiguous (B, 3, Hp, Wp) float32 tensor on the engine device')
        H, W, index, offset = int(H), int(W), int(index), int(offset)
        pitch = 3 * W if pitch is None else int(pitch)
        B, _, Hp, Wp = (int(v) for v in x.shape)
        if not (0 <= index < B and 1 <= H <= Hp and 1 <= W <= Wp and pitch >= 3 * W and offset >= 0):
            raise ValueError(f'image {index} of {B}, {H} x {W} of {Hp} x {Wp}, pitch {pitch}, offset {offset}')
        if slab is None:
            slab = torch.empty(offset + (H - 1) * pitch + 3 * W, device=d, dtype=torch.uint8)
        _u8_slab('slab', slab, d)
        if offset + (H - 1) * pitch + 3 * W > slab.numel():
            raise ValueError(f'the frame leaves the slab of {slab.numel()} bytes')
        f3 = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float32).reshape(3)
        mean, std = f3(mean), f3(std)
        as_p = lambda v: None if v is None else v.ctypes.data_as(_lib.c_float_p)
        _lib.check(self.h, self.lib.specmi_denormalize_u8(self.h, _ptr(x), B, Hp, Wp, index, H, W, as_p(mean), as_p(std), _ptr(slab),
                                                           slab.numel(), offset, pitch, self._stream()))
        return slab

    def jpeg_encode_into(self, slab, out_slab, geom, offsets, quality=75, sizes=None):
        """``specmi_jpeg_encode``: the pictures ``geom`` (n, 2) [H, W] at ``offsets`` (n, 4) [in_offset, in_pitch, out_offset,
        out_capacity] of ``slab`` (1-D uint8 on the engine device: the output slab of ``render_views``, what ``pack_frames``
        builds) encoded as baseline JPEG files into ``out_slab`` (1-D uint8, same device, not overlapping) at one ``quality``.
        -> ``sizes`` (n,) int64 on the device (given or new): every file's true length, also of a picture that did not fit its
        capacity (nothing is written beyond it).  Nothing is synchronised or downloaded here; a repeat of the previous records
        can be captured in a graph.  Everything is checked before the library is called (``check_jpeg_encode``)."""
        _u8_slab('slab', slab, self.device)
        _u8_slab('out_slab', out_slab, self.device)
        geom, offsets = check_jpeg_encode(geom, offsets, slab.numel(), out_slab.numel(), quality, slab.data_ptr(), out_slab.data_ptr())
        n = int(geom.shape[0])
        sizes = _dev_vector('sizes', sizes, n, torch.int64, self.device)
        _lib.check(self.h, self.lib.specmi_jpeg_encode(
            self.h, _ptr(slab), slab.numel(), _ptr(out_slab), out_slab.numel(), geom.ctypes.data_as(_lib.c_int32_p),
            offsets.ctypes.data_as(_lib.c_int64_p), n, int(quality), _ptr(sizes), self._stream()))
        return sizes

    def jpeg_encode(self, slab, geom, offsets, quality=75) -> List[bytes]:
        """The pictures ``geom`` (n, 2) [H, W] at ``offsets`` (n, 2) [in_offset, in_pitch] of ``slab`` as JPEG files, byte for
        byte what ``PIL.Image.fromarray(a).save(f, format='JPEG', quality=quality)`` writes (include/specmi.h states the
        contract): one ``jpeg_encode_into`` call into a private slab with ``jpeg_capacity(H, W)`` bytes per picture, a download
        of the sizes, then of the used bytes only; a picture that did not fit (noise at a high quality) is encoded again with
        the room its size asks for.  -> the files as a list of ``bytes``."""
        geom, offsets = _encode_rows(geom, offsets)
        files = [None] * geom.shape[0]
        todo, cap = np.arange(geom.shape[0]), np.array([jpeg_capacity(h, w) for h, w in geom], np.int64)
        while todo.size:
            sizes, got = self._encode_round(lambda *a: self.jpeg_encode_into(slab, *a, quality), geom[todo], offsets[todo], cap[todo])
            for i, f in zip(todo, got):
                files[i] = f
            fits = sizes <= cap[todo]
            cap[todo] = sizes
            todo = todo[~fits]
        return files

    def _encode_round(self, into, geom, offsets, cap):
        """What ``jpeg_encode`` and ``png_encode`` share: one ``into(out_slab, geom, offsets (n, 4))`` call into a private slab
        with ``cap`` bytes per picture, a download of the sizes, then - in one copy - of the used bytes of the files that fit
        -> (sizes on the host, the files as ``bytes``: None where one did not fit)."""
        out_off = starts(cap)
        out_slab = torch.empty(int(cap.sum()), device=self.device, dtype=torch.uint8)
        sizes = into(out_slab, geom, np.concatenate([offsets, out_off[:, None], cap[:, None]], axis=1)).cpu().numpy()
        fits = sizes <= cap
        files = [None] * len(cap)
        if fits.any():
            host = torch.cat([out_slab[int(o):int(o + s)] for o, s in zip(out_off[fits], sizes[fits])]).cpu().numpy().tobytes()
            for i, a, s in zip(np.flatnonzero(fits), starts(sizes[fits]), sizes[fits]):
                files[i] = host[int(a):int(a + s)]
        return sizes, files

    def png_encode_into(self, slab, out_slab, geom, offsets, sizes=None):
        """``specmi_png_encode``: the pictures ``geom`` (n, 2) [H, W] at ``offsets`` (n, 4) [in_offset, in_pitch, out_offset,
        out_capacity] of ``slab`` (1-D uint8 on the engine device, as ``jpeg_encode_into`` takes it) encoded as PNG files into
        ``out_slab`` (1-D uint8, same device, not overlapping).  -> ``sizes`` (n,) int64 on the device (given or new): every
        file's true length, also of a picture that did not fit its capacity (nothing is written beyond it; with
        ``png_bound(H, W)`` of room every picture fits).  Nothing is synchronised or downloaded here; a repeat of the previous
        records can be captured in a graph.  Everything is checked before the library is called (``check_png_encode``)."""
        _u8_slab('slab', slab, self.device)
        _u8_slab('out_slab', out_slab, self.device)
        geom, offsets = check_png_encode(geom, offsets, slab.numel(), out_slab.numel(), slab.data_ptr(), out_slab.data_ptr())
        n = int(geom.shape[0])
        sizes = _dev_vector('sizes', sizes, n, torch.int64, self.device)
        _lib.check(self.h, self.lib.specmi_png_encode(
            self.h, _ptr(slab), slab.numel(), _ptr(out_slab), out_slab.numel(), geom.ctypes.data_as(_lib.c_int32_p),
            offsets.ctypes.data_as(_lib.c_int64_p), n, _ptr(sizes), self._stream()))
        return sizes

    def png_encode(self, slab, geom, offsets) -> List[bytes]:
        """The pictures ``geom`` (n, 2) [H, W] at ``offsets`` (n, 2) [in_offset, in_pitch] of ``slab`` as PNG files that decode
        to exactly the pictures (include/specmi.h states the contract; the bytes are not Pillow's): one ``png_encode_into`` call
        into a private slab with ``png_bound(H, W)`` bytes per picture - every file fits, so there is no second call - a
        download of the sizes, then of the used bytes only.  -> the files as a list of ``bytes``."""
        geom, offsets = _encode_rows(geom, offsets)
        cap = np.array([png_bound(h, w) for h, w in geom], np.int64)
        sizes, files = self._encode_round(lambda *a: self.png_encode_into(slab, *a), geom, offsets, cap)
        if (sizes > cap).any():
            raise RuntimeError('specmi_png_encode reports a file beyond specmi_png_bound')
        return files

    def jpeg_decode_into(self, host, slab, ranges, geom, out_slab, outs, status=None, coef=None):
        """``specmi_jpeg_decode``: the files at ``ranges`` (n, 2) [offset, length] of ``slab`` (1-D uint8 on the engine device)
        and of ``host`` (the same bytes on the host: a 1-D uint8 array; only the sizes are compared, that the bytes agree is the caller's
        contract), of ``geom`` (n, 3) [H, W, sampling] as ``jpeg_probe``
        gave them, decoded into the rectangles ``outs`` (n, 2) [offset, pitch] of ``out_slab`` (1-D uint8, same device, not
        overlapping).  -> (``status`` (n,) int32 on the device, given or new: 0 where the file's pixels are Pillow's; passes of
        the sync stage).  ``coef``: an int16 device tensor that receives the coefficients.  Synchronises the stream between
        passes; everything the arrays decide is checked before the library is called (``check_jpeg_decode``)."""
        _u8_slab('slab', slab, self.device)
        _u8_slab('out_slab', out_slab, self.device)
        host = np.ascontiguousarray(host, dtype=np.uint8).reshape(-1)
        if host.size != slab.numel():
            raise ValueError('host and slab hold the same bytes: their sizes differ')
        ranges, outs = check_jpeg_decode(ranges, geom, outs, slab.numel(), out_slab.numel(), slab.data_ptr(), out_slab.data_ptr())
        n = int(ranges.shape[0])
        status = _dev_vector('status', status, n, torch.int32, self.device)
        _dev_tensor('coef', coef, torch.int16, self.device, optional=True)
        passes = C.c_int32(0)
        _lib.check(self.h, self.lib.specmi_jpeg_decode(
            self.h, host.ctypes.data_as(C.c_void_p), _ptr(slab), slab.numel(), ranges.ctypes.data_as(_lib.c_int64_p), _ptr(out_slab),
            out_slab.numel(), outs.ctypes.data_as(_lib.c_int64_p), n, _ptr(status), _ptr(coef), 0 if coef is None else 2 * coef.numel(),
            C.byref(passes), self._stream()))
        self.jpeg_decode_passes = int(passes.value)           # of the last call: what scripts/bench_aux.py records
        return status, self.jpeg_decode_passes

    def jpeg_decode(self, files):
        """``files``: a list of ``bytes``, every one a file ``jpeg_probe`` calls supported -> (slab, offsets, sizes, status): the
        pictures back to back in one 1-D uint8 device slab with their (n,) int64 byte offsets and [(H, W)] - the triple
        ``preprocess.pack_frames`` builds from Pillow's decodes of the same files, bit for bit where ``status`` (n,) int32 on the
        device is 0 (include/specmi.h states the contract).  One upload of the files' bytes, one ``specmi_jpeg_decode``."""
        return self._decode(files, jpeg_probe, lambda f, p: f, 'baseline JPEG', lambda host, *a: self.jpeg_decode_into(host, *a)[0])

    def _decode(self, files, probe, payload, what, into):
        """What ``jpeg_decode`` and ``png_decode`` share: every file probed (``probe``) and refused unless supported (a ``what``
        file), its ``payload(file, probe answer)`` - what the device reads of it - back to back in one uploaded slab, dense
        output rectangles, one ``into(host bytes, slab, ranges, geom, out_slab, outs)`` call -> (slab, offsets, sizes, status)."""
        files = [bytes(f) for f in files]
        if not files:
            raise ValueError('at least one file')
        probes = [probe(f) for f in files]
        for i, p in enumerate(probes):
            if p[0] != 'supported':
                raise ValueError(f'file {i} is not a supported {what} file ({p[0]})')
        payloads = [payload(f, p) for f, p in zip(files, probes)]
        length = np.array([len(s) for s in payloads], np.int64)
        ranges = np.stack([starts(length), length], axis=1)
        host = np.frombuffer(b''.join(payloads), np.uint8)
        geom = np.array([p[1:4] for p in probes], np.int64)
        size = 3 * geom[:, 0] * geom[:, 1]
        offsets = starts(size)
        slab = torch.from_numpy(host.copy()).to(self.device)
        out_slab = torch.empty(int(size.sum()), device=self.device, dtype=torch.uint8)
        status = into(host, slab, ranges, geom, out_slab, np.stack([offsets, 3 * geom[:, 1]], axis=1))
        return out_slab, offsets, [(int(h), int(w)) for h, w, _ in geom], status

    def png_decode_into(self, slab, ranges, geom, out_slab, outs, status=None, raw=None):
        """``specmi_png_decode``: the zlib streams at ``ranges`` (n, 2) [offset, length] of ``slab`` (1-D uint8 on the engine
        device; every file's IDAT payloads joined, ``png_stream``), of ``geom`` (n, 3) [H, W, colour type] as ``png_probe`` gave
        them, inflated and unfiltered into the rectangles ``outs`` (n, 2) [offset, pitch] of ``out_slab`` (1-D uint8, same device,
        not overlapping).  -> ``status`` (n,) int32 on the device, given or new: 0 where the file's pixels are Pillow's.  ``raw``:
        a uint8 device tensor that receives the inflated streams, each from a multiple of 256.  Everything the arrays decide is
        checked before the library is called (``check_png_decode``)."""
        _u8_slab('slab', slab, self.device)
        _u8_slab('out_slab', out_slab, self.device)
        _dev_tensor('raw', raw, torch.uint8, self.device, optional=True)      # any shape: the streams land in its bytes
        ranges, geom, outs, _ = check_png_decode(ranges, geom, outs, slab.numel(), out_slab.numel(), slab.data_ptr(), out_slab.data_ptr(),
                                                 None if raw is None else raw.numel())
        n = int(ranges.shape[0])
        status = _dev_vector('status', status, n, torch.int32, self.device)
        _lib.check(self.h, self.lib.specmi_png_decode(
            self.h, _ptr(slab), slab.numel(), ranges.ctypes.data_as(_lib.c_int64_p), geom.ctypes.data_as(_lib.c_int32_p), _ptr(out_slab),
            out_slab.numel(), outs.ctypes.data_as(_lib.c_int64_p), n, _ptr(status), _ptr(raw), 0 if raw is None else raw.numel(),
            self._stream()))
        return status

    def png_decode(self, files):
        """``files``: a list of ``bytes``, every one a file ``png_probe`` calls supported -> (slab, offsets, sizes, status): the
        pictures back to back in one 1-D uint8 device slab with their (n,) int64 byte offsets and [(H, W)] - the triple
        ``preprocess.pack_frames`` builds from Pillow's decodes of the same files, bit for bit where ``status`` (n,) int32 on the
        device is 0 (include/specmi.h states the contract).  One upload of the files' zlib streams, one ``specmi_png_decode``."""
        return self._decode(files, png_probe, lambda f, p: png_stream(f, p[4]), 'PNG', lambda host, *a: self.png_decode_into(*a))

    def _cam_args(self, B, cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h):
        d = self.device
        return (_dev_f32(cam_rotmat, d, (B, 3, 3)), _dev_f32(cam_intrinsics, d, (B, 3, 3)),
                _dev_f32(bbox_scale, d, (B,)), _dev_f32(bbox_center, d, (B, 2)),
                _dev_f32(img_w, d, (B,)), _dev_f32(img_h, d, (B,)))

    def _out_for(self, B, record):
        """Output dict + the handle's output stride: dense tensors, or views of a (B, record_floats) record the
        kernels write in place."""
        if record is None:
            self._set_ld('output_ld', 0)
            return None
        if record.shape[0] != B or record.device != self.device:
            raise ValueError('record must be a (B, record_floats) tensor on the model device')
        views = self.record_views(record)
        self._set_ld('output_ld', record.stride(0))
        return views

    def hmr_forward(self, images, cam_rotmat=None, cam_intrinsics=None, bbox_scale=None,
                    bbox_center=None, img_w=None, img_h=None, out: Optional[Dict[str, torch.Tensor]] = None,
                    record: Optional[torch.Tensor] = None):
        x, B, H, W, f16 = self._images_in(images)
        R, K, sc, ce, iw, ih = self._cam_args(B, cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h)
        views = self._out_for(B, record)
        out = views if views is not None else (out if out is not None else self._hmr_outputs(B))
        if B == 0:
            return out
        o = _lib.HmrOutputs(**{k: out[k].data_ptr() for k in _HMR_KEYS})
        fn = self.lib.specmi_hmr_forward_f16in if f16 else self.lib.specmi_hmr_forward
        _lib.check(self.h, fn(
            self.h, _ptr(x), B, H, W, _ptr(R), _ptr(K), _ptr(sc), _ptr(ce), _ptr(iw), _ptr(ih),
            C.byref(o), self._stream()))
        return out

    def hmr_regress(self, feat_nhwc, cam_rotmat=None, cam_intrinsics=None, bbox_scale=None, bbox_center=None,
                    img_w=None, img_h=None, record: Optional[torch.Tensor] = None):
        """Regressor head + SMPL head from a trunk feature map (hmr.py:94-122), one library call."""
        f = _dev_f32(feat_nhwc, self.device)
        B, fh, fw, _ = f.shape
        R, K, sc, ce, iw, ih = self._cam_args(B, cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h)
        views = self._out_for(B, record)
        out = views if views is not None else self._hmr_outputs(B)
        if B == 0:                      # empty batch: empty outputs, like hmr_forward / trunk
            return out
        o = _lib.HmrOutputs(**{k: out[k].data_ptr() for k in _HMR_KEYS})
        _lib.check(self.h, self.lib.specmi_hmr_regress(
            self.h, _ptr(f), B, fh, fw, _ptr(R), _ptr(K), _ptr(sc), _ptr(ce), _ptr(iw), _ptr(ih),
            C.byref(o), self._stream()))
        return out

    def hmr_uncertainty(self, B: int):
        """(pred_pose_var (B, 288), pred_shape_var (B, 20)) of a model committed with ``estimate_var``: call right after the head
        forward of the same batch on the same stream (``specmi_hmr_uncertainty``)."""
        pv, sv = self._empty(B, 288), self._empty(B, 20)
        if B > 0:
            _lib.check(self.h, self.lib.specmi_hmr_uncertainty(self.h, int(B), _ptr(pv), _ptr(sv), self._stream()))
        return pv, sv

    def hmr_head(self, feat_nhwc, cam_rotmat=None, cam_intrinsics=None, img_h=None, record=None):
        f = _dev_f32(feat_nhwc, self.device)
        B, fh, fw, _ = f.shape
        R = _dev_f32(cam_rotmat, self.device, (B, 3, 3))
        K = _dev_f32(cam_intrinsics, self.device, (B, 3, 3))
        ih = _dev_f32(img_h, self.device, (B,))
        out = self._outputs(B, ('pred_pose', 'pred_shape', 'pred_cam', 'pred_pose_6d'), self._out_for(B, record))
        if B == 0:
            return out
        _lib.check(self.h, self.lib.specmi_hmr_head_forward(
            self.h, _ptr(f), B, fh, fw, _ptr(R), _ptr(K), _ptr(ih), _ptr(out['pred_pose']),
            _ptr(out['pred_shape']), _ptr(out['pred_cam']), _ptr(out['pred_pose_6d']), self._stream()))
        return out

    def smpl(self, rotmat, betas, cam, cam_rotmat=None, cam_intrinsics=None, bbox_scale=None,
             bbox_center=None, img_w=None, img_h=None, record=None):
        rot = _dev_f32(rotmat, self.device)
        B = rot.shape[0]
        rot = rot.reshape(B, *_ROTMATS).contiguous()
        be = _dev_f32(betas, self.device, (B, 10))
        cm = _dev_f32(cam, self.device, (B, 3))
        R, K, sc, ce, iw, ih = self._cam_args(B, cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h)
        out = self._outputs(B, ('smpl_vertices', 'smpl_joints3d', 'smpl_joints2d', 'pred_cam_t'), self._out_for(B, record))
        if B == 0:
            return out
        _lib.check(self.h, self.lib.specmi_smpl_forward(
            self.h, _ptr(rot), _ptr(be), _ptr(cm), B, _ptr(R), _ptr(K), _ptr(sc), _ptr(ce), _ptr(iw),
            _ptr(ih), _ptr(out['smpl_vertices']), _ptr(out['smpl_joints3d']), _ptr(out['smpl_joints2d']),
            _ptr(out['pred_cam_t']), self._stream()))
        return out

    def smpl_backward(self, rotmat, betas, cam, cam_rotmat=None, cam_intrinsics=None, bbox_scale=None, bbox_center=None,
                      img_w=None, img_h=None, g_vertices=None, g_joints3d=None, g_joints2d=None, g_cam_t=None,
                      want=(True, True, True)):
        """``specmi_smpl_backward``: the vector-Jacobian product of ``smpl`` at its own inputs.  Upstream gradients that are None
        count as zero; -> (g_rotmat (B,24,3,3), g_betas (B,10), g_cam (B,3)), None where ``want`` says not wanted."""
        rot = _dev_f32(rotmat, self.device)
        B = rot.shape[0]
        rot = rot.reshape(B, *_ROTMATS).contiguous()
        be = _dev_f32(betas, self.device, (B, 10))
        cm = _dev_f32(cam, self.device, (B, 3))
        camera = self._cam_args(B, cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h)
        shapes = _record_shapes(self.num_verts)
        up = tuple(_dev_f32(g, self.device, (B, *shapes[k])) for g, k in
                   ((g_vertices, 'smpl_vertices'), (g_joints3d, 'smpl_joints3d'), (g_joints2d, 'smpl_joints2d'), (g_cam_t, 'pred_cam_t')))
        check_smpl_backward(B, [g is not None for g in up], want, self.get_option('use_cam'), [c is not None for c in camera])
        out = [self._empty(B, *shp) if w else None for w, shp in zip(want, (_ROTMATS, (10,), (3,)))]
        _lib.check(self.h, self.lib.specmi_smpl_backward(
            self.h, _ptr(rot), _ptr(be), _ptr(cm), B, *(_ptr(c) for c in camera), *(_ptr(g) for g in up),
            *(_ptr(o) for o in out), self._stream()))
        return tuple(out)

    def rot6d_to_rotmat(self, x6d):
        """``specmi_rot6d_forward``: (N,6), or the head's pose rows of 24 rotations -> (N,3,3) rotation matrices (its Gram-Schmidt)."""
        x = _dev_f32(x6d, self.device)
        n = check_rot6d_backward(tuple(x.shape), (math.prod(x.shape) // 6 * 9,))
        out = self._empty(n, 3, 3)
        _lib.check(self.h, self.lib.specmi_rot6d_forward(self.h, _ptr(x), n, _ptr(out), self._stream()))
        return out

    def rot6d_backward(self, x6d, g_rotmat):
        """``specmi_rot6d_backward``: x6d as ``rot6d_to_rotmat`` takes it, g_rotmat (N,3,3) or (B,24,3,3) -> the gradient of x6d, in its shape."""
        x = _dev_f32(x6d, self.device)
        g = _dev_f32(g_rotmat, self.device)
        n = check_rot6d_backward(tuple(x.shape), tuple(g.shape))
        out = torch.empty_like(x)
        _lib.check(self.h, self.lib.specmi_rot6d_backward(self.h, _ptr(x), _ptr(g), n, _ptr(out), self._stream()))
        return out

    def _hmr_head_args(self, params, xf, cam_feats, masks, p, n_iter, outputs, others):
        """The arguments the two HMRHead training calls share, checked: -> (params struct, xf, ld_xf, cam_feats, masks, B, F, C).
        ``params``: the ten tensors under their state_dict names, read where they lie - fp32, contiguous, on this device."""
        ps = {n: params[n].detach() if params.get(n) is not None else None for n in _lib.HMR_HEAD_PARAMS}
        for n, t in ps.items():
            if t is not None and (t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f'{n} must be a contiguous fp32 tensor on {self.device} (the library reads it in place)')
        x = xf.detach() if isinstance(xf, torch.Tensor) else xf
        if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.device == self.device and x.dtype == torch.float32 and
                (x.stride(1) == 1 or x.shape[1] == 1)):
            x = _dev_f32(x, self.device)
        if x.dim() != 2:
            raise ValueError(f'xf must be (B, F), got {tuple(x.shape)}')
        B, F = x.shape
        ld = x.stride(0) if B > 1 else F
        cf = _dev_f32(cam_feats, self.device, (B, 7))
        C_ = 7 if cf is not None else 0
        if masks is not None:
            if masks.dtype == torch.bool:
                masks = masks.view(torch.uint8)
            if masks.dtype != torch.uint8 or tuple(masks.shape) != (2 * n_iter, B, HMR_HEAD_HIDDEN) or masks.device != self.device:
                raise ValueError(f'masks must be uint8 or bool ({2 * n_iter}, {B}, {HMR_HEAD_HIDDEN}) on {self.device}')
            masks = masks.contiguous()
        fc1 = ps['fc1.weight']
        if fc1 is not None and fc1.dim() == 2 and fc1.shape[1] == F + HMR_HEAD_STATE + 7 and cf is None:
            raise ValueError('cam_feats is required with C = 7')
        check_hmr_head_train(B, F, C_, n_iter, p, masks is not None, {n: None if t is None else t.shape for n, t in ps.items()},
                             ld_xf=ld, outputs=outputs,
                             addresses=[t.data_ptr() for t in (*ps.values(), x, cf, *others) if t is not None])
        st = _lib.HmrHeadParams(*(t.data_ptr() for t in ps.values()))
        return st, x, ld, cf, masks, B, F, C_

    def hmr_head_train_forward(self, params, xf, init_state, cam_feats=None, masks=None, p=0.5, n_iter=3, tape=None):
        """``specmi_hmr_head_train_forward``: pare's HMRHead loop on ``params`` (the ten tensors under their state_dict names, read
        in place), xf (B, F) pooled features, init_state (B, 157), cam_feats (B, 7) when the head was built with use_cam_feats,
        masks uint8 / bool (2 n_iter, B, 1024) or None = eval mode.  -> (state_n (B, 157), the tape ``hmr_head_backward`` needs;
        ``tape=`` takes a caller's flat fp32 buffer of at least ``hmr_head_tape_floats(B, n_iter)`` floats)."""
        init = _dev_f32(init_state, self.device)
        st, x, ld, cf, masks, B, F, C_ = self._hmr_head_args(params, xf, cam_feats, masks, p, n_iter, None, (init,))
        if tuple(init.shape) != (B, HMR_HEAD_STATE):
            raise ValueError(f'init_state must be ({B}, {HMR_HEAD_STATE}), got {tuple(init.shape)}')
        need = hmr_head_tape_floats(B, n_iter)
        if tape is None:
            tape = self._empty(need)
        elif tape.device != self.device or tape.dtype != torch.float32 or not tape.is_contiguous() or tape.numel() < need:
            raise ValueError(f'tape must be a contiguous fp32 tensor of at least {need} floats on {self.device}')
        state = self._empty(B, HMR_HEAD_STATE)
        _lib.check(self.h, self.lib.specmi_hmr_head_train_forward(
            self.h, C.byref(st), _ptr(x), ld, _ptr(cf), _ptr(init), _ptr(masks), float(p), B, F, C_, int(n_iter), _ptr(state),
            _ptr(tape), self._stream()))
        return state, tape

    def hmr_head_backward(self, params, xf, tape, g_state, cam_feats=None, masks=None, p=0.5, n_iter=3, want_xf=True,
                          want_params=True):
        """``specmi_hmr_head_backward``: the forward's arguments and its tape, g_state (B, 157) -> (g_xf (B, F) or None, {name:
        gradient} of the wanted parameters).  ``want_params``: True (all ten), False, or the names wanted."""
        g = _dev_f32(g_state, self.device)
        names = _lib.HMR_HEAD_PARAMS if want_params is True else tuple(want_params or ())
        if set(names) - set(_lib.HMR_HEAD_PARAMS):
            raise ValueError(f'want_params names {sorted(set(names) - set(_lib.HMR_HEAD_PARAMS))}: not parameters of the head')
        outputs = [bool(want_xf)] + [n in names for n in _lib.HMR_HEAD_PARAMS]
        st, x, ld, cf, masks, B, F, C_ = self._hmr_head_args(params, xf, cam_feats, masks, p, n_iter, outputs, (g, tape))
        if tuple(g.shape) != (B, HMR_HEAD_STATE):
            raise ValueError(f'g_state must be ({B}, {HMR_HEAD_STATE}), got {tuple(g.shape)}')
        need = hmr_head_tape_floats(B, n_iter)
        if tape.device != self.device or tape.dtype != torch.float32 or not tape.is_contiguous() or tape.numel() < need:
            raise ValueError(f'tape must be the contiguous fp32 tensor of at least {need} floats the forward wrote')
        g_xf = self._empty(B, F) if want_xf else None
        shapes = hmr_head_param_shapes(F, C_)
        grads = {n: self._empty(*shapes[n]) for n in _lib.HMR_HEAD_PARAMS if n in names}
        gs = _lib.HmrHeadParams(*(grads[n].data_ptr() if n in grads else None for n in _lib.HMR_HEAD_PARAMS))
        _lib.check(self.h, self.lib.specmi_hmr_head_backward(
            self.h, C.byref(st), _ptr(x), ld, _ptr(cf), _ptr(masks), float(p), B, F, C_, int(n_iter), _ptr(tape), _ptr(g), _ptr(g_xf),
            C.byref(gs) if grads else None, self._stream()))
        return g_xf, grads

    def _camcalib_loss_args(self, preds, targets, loss_type, weights):
        """The arguments ``specmi_camcalib_loss`` and its backward share, checked -> (logits, targets, B, nbins, SPECMI_LOSS_*)."""
        if loss_type not in _lib.LOSS_TYPES:
            raise ValueError(f'{loss_type} is not defined..')
        if len(preds) != 3 or len(targets) != 3 or len(weights) != 3:
            raise ValueError('three logit tensors, three targets and three weights, in the order vfov, pitch, roll')
        lg = [_dev_f32(t, self.device) for t in preds]
        if lg[0].dim() != 2:
            raise ValueError(f'the logit tensors must be (B, nbins), got {tuple(lg[0].shape)}')
        B, nb = (int(v) for v in lg[0].shape)
        tdt = torch.int32 if loss_type in ('ce', 'kl') else torch.float32
        tg = [(t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))).to(device=self.device, dtype=tdt).contiguous() for t in targets]
        lt = check_camcalib_loss(B, nb, loss_type, [t.shape for t in lg + tg])
        return lg, tg, B, nb, lt

    def camcalib_loss(self, preds, targets, loss_type, weights=(1.0, 1.0, 1.0)):
        """``specmi_camcalib_loss``: CameraRegressorLoss on three (B, nbins) logit tensors (vfov, pitch, roll).  ``targets``: three
        (B,) arrays - integer bin indices for 'ce' / 'kl', fp32 soft indices for the soft-argmax losses.  -> dict(loss_term (3, B),
        means (4,) = loss, vfov_loss, pitch_loss, roll_loss), the bits of ``camcalib_eval`` on the same inputs."""
        lg, tg, B, nb, lt = self._camcalib_loss_args(preds, targets, loss_type, weights)
        res = {'loss_term': self._empty(3, B), 'means': self._empty(4)}
        _lib.check(self.h, self.lib.specmi_camcalib_loss(
            self.h, *(_ptr(t) for t in lg), B, nb, lt, *(_ptr(t) for t in tg), *(float(w) for w in weights), _ptr(res['loss_term']),
            _ptr(res['means']), self._stream()))
        return res

    def camcalib_loss_backward(self, preds, targets, loss_type, weights, g_means):
        """``specmi_camcalib_loss_backward``: the arguments of ``camcalib_loss`` and ``g_means`` (4,), the upstream gradients of
        loss, vfov_loss, pitch_loss, roll_loss -> the three (B, nbins) gradients of the logits."""
        lg, tg, B, nb, lt = self._camcalib_loss_args(preds, targets, loss_type, weights)
        gm = _dev_f32(g_means, self.device)
        check_camcalib_loss(B, nb, loss_type, g_means_shape=gm.shape)
        out = [torch.empty_like(t) for t in lg]
        _lib.check(self.h, self.lib.specmi_camcalib_loss_backward(
            self.h, *(_ptr(t) for t in lg), B, nb, lt, *(_ptr(t) for t in tg), *(float(w) for w in weights), _ptr(gm),
            *(_ptr(t) for t in out), self._stream()))
        return out

    def _camcalib_head_args(self, params, xf, L, outputs, others):
        """The arguments the two CamCalib head training calls share, checked -> (params struct, xf, ld_xf, B, F, Hc, nbins).
        ``params``: the 6 L tensors under their state_dict names, read where they lie - fp32, contiguous, on this device."""
        if not 1 <= int(L) <= _lib.CAMCALIB_HEAD_MAX_LAYERS:
            raise ValueError(f'L = {L} must be in 1 .. {_lib.CAMCALIB_HEAD_MAX_LAYERS}')
        names = camcalib_head_param_names(L)
        ps = {n: params[n].detach() if params.get(n) is not None else None for n in names}
        for n, t in ps.items():
            if t is not None and (t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f'{n} must be a contiguous fp32 tensor on {self.device} (the library reads it in place)')
        x = xf.detach() if isinstance(xf, torch.Tensor) else xf
        if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.device == self.device and x.dtype == torch.float32 and
                (x.stride(1) == 1 or x.shape[1] == 1)):
            x = _dev_f32(x, self.device)
        if x.dim() != 2:
            raise ValueError(f'xf must be (B, F), got {tuple(x.shape)}')
        B, F = (int(v) for v in x.shape)
        ld = x.stride(0) if B > 1 else F
        first, last = ps[names[0]], ps[names[-2]]
        if first is None or last is None or first.dim() != 2 or last.dim() != 2:
            raise ValueError(f'{names[0]} and {names[-2]} must be 2-D weights')
        Hc, nbins = (int(first.shape[0]) if L > 1 else 1), int(last.shape[0])
        check_camcalib_head_train(B, F, L, Hc, nbins, {n: None if t is None else t.shape for n, t in ps.items()}, ld_xf=ld, outputs=outputs,
                                  addresses=[t.data_ptr() for t in (*ps.values(), x, *others) if t is not None])
        st = _lib.CamcalibHeadParams()
        for i, n in enumerate(names):
            k, l, kind = i // (2 * L), i // 2 % L, i % 2
            (st.bias if kind else st.weight)[k][l] = ps[n].data_ptr()
        return st, x, ld, B, F, Hc, nbins

    def camcalib_head_train_forward(self, params, xf, L, tape=None):
        """``specmi_camcalib_head_train_forward``: CamCalib's three FC heads on ``params`` (the 6 L tensors of
        ``camcalib_head_param_names(L)``, read in place) and xf (B, F) pooled features -> (logits (3, B, nbins), the tape
        ``camcalib_head_backward`` needs; ``tape=`` takes a caller's flat fp32 buffer of at least
        ``camcalib_head_tape_floats(B, L, Hc)`` floats)."""
        st, x, ld, B, F, Hc, nbins = self._camcalib_head_args(params, xf, L, None, ())
        need = camcalib_head_tape_floats(B, L, Hc)
        if tape is None:
            tape = self._empty(need)
        elif tape.device != self.device or tape.dtype != torch.float32 or not tape.is_contiguous() or tape.numel() < need:
            raise ValueError(f'tape must be a contiguous fp32 tensor of at least {need} floats on {self.device}')
        logits = self._empty(3, B, nbins)
        _lib.check(self.h, self.lib.specmi_camcalib_head_train_forward(
            self.h, C.byref(st), _ptr(x), ld, B, F, int(L), Hc, nbins, _ptr(tape) if need else None, _ptr(logits), self._stream()))
        return logits, tape

    def camcalib_head_backward(self, params, xf, L, tape, g_logits, want_xf=True, want_params=True):
        """``specmi_camcalib_head_backward``: the forward's arguments and its tape, g_logits (3, B, nbins) -> (g_xf (B, F) or None,
        {name: gradient} of the wanted parameters).  ``want_params``: True (all 6 L), False, or the names wanted."""
        g = _dev_f32(g_logits, self.device)
        all_names = camcalib_head_param_names(L)
        names = all_names if want_params is True else tuple(want_params or ())
        if set(names) - set(all_names):
            raise ValueError(f'want_params names {sorted(set(names) - set(all_names))}: not parameters of the heads')
        outputs = [bool(want_xf)] + [n in names for n in all_names]
        st, x, ld, B, F, Hc, nbins = self._camcalib_head_args(params, xf, L, outputs, (g, tape))
        if tuple(g.shape) != (3, B, nbins):
            raise ValueError(f'g_logits must be (3, {B}, {nbins}), got {tuple(g.shape)}')
        need = camcalib_head_tape_floats(B, L, Hc)
        if tape is None or tape.device != self.device or tape.dtype != torch.float32 or not tape.is_contiguous() or tape.numel() < need:
            raise ValueError(f'tape must be the contiguous fp32 tensor of at least {need} floats the forward wrote')
        g_xf = self._empty(B, F) if want_xf else None
        shapes = camcalib_head_param_shapes(F, L, Hc, nbins)
        grads = {n: self._empty(*shapes[n]) for n in all_names if n in names}
        gs = _lib.CamcalibHeadParams()
        for i, n in enumerate(all_names):
            if n in grads:
                k, l, kind = i // (2 * L), i // 2 % L, i % 2
                (gs.bias if kind else gs.weight)[k][l] = grads[n].data_ptr()
        _lib.check(self.h, self.lib.specmi_camcalib_head_backward(
            self.h, C.byref(st), _ptr(x), ld, B, F, int(L), Hc, nbins, _ptr(tape) if need else None, _ptr(g), _ptr(g_xf),
            C.byref(gs) if grads else None, self._stream()))
        return g_xf, grads

    def smpl_native(self, pose, betas, vertices=True, joints24=True):
        """smplx-style body model call: ``pose`` (B,24,3,3) rotation matrices or (B,72) axis-angle; returns
        (vertices (B,V,3) | None, joints24 (B,24,3) | None)."""
        p = _dev_f32(pose, self.device)
        B = p.shape[0]
        aa = p.dim() == 2
        if aa and p.shape[1] != 72 or not aa and tuple(p.shape[1:]) != _ROTMATS:
            raise ValueError(f'pose must be (B,72) axis-angle or (B,24,3,3) rotation matrices, got {tuple(p.shape)}')
        be = _dev_f32(betas, self.device, (B, 10))
        v = self._empty(B, self.num_verts, 3) if vertices else None
        j = self._empty(B, 24, 3) if joints24 else None
        self._set_ld('output_ld', 0)
        _lib.check(self.h, self.lib.specmi_smpl_native(self.h, _ptr(p), int(aa), _ptr(be), B, _ptr(v), _ptr(j),
                                                       self._stream()))
        return v, j

    @staticmethod
    def _pixel_rows(t):
        """A (B,H,W,C) NHWC tensor or channel-sliced view of one -> its pixel stride ld (unit stride along C, one stride
        ld >= C from pixel to pixel, pixels dense in B, H, W), or None if it is laid out otherwise."""
        _, H, W, Cc = t.shape
        ld = t.stride(2) if W > 1 else t.stride(1) // W if H > 1 else t.stride(0) // (H * W) if t.shape[0] > 1 else Cc
        want = (H * W * ld, W * ld, ld, 1)
        return ld if ld >= Cc and all(n == 1 or st == wt for n, st, wt in zip(t.shape, t.stride(), want)) else None

    def _conv_train_args(self, x, w, scale, stride, pad):
        """The layer of the two training calls, checked -> (x, w, scale, B, H, W, Cin, Cout, k, OH, OW); the tensors are read in
        place when they are dense fp32 on this device."""
        x, w, scale = _dev_f32(x, self.device), _dev_f32(w, self.device), _dev_f32(scale, self.device)
        if x.dim() != 4 or w.dim() != 4 or x.shape[3] != w.shape[1] or w.shape[2] != w.shape[3]:
            raise ValueError(f'x must be (B, H, W, Cin) NHWC and w (Cout, Cin, k, k), got {tuple(x.shape)} and {tuple(w.shape)}')
        B, H, W, Cin = x.shape
        Cout, _, k, _ = w.shape
        if not (((k, pad) in ((1, 0), (3, 1)) and stride in (1, 2)) or (k, pad, stride) == (7, 3, 2)):
            raise ValueError(f'the layers built are 1x1 pad 0 and 3x3 pad 1 at stride 1 or 2 and 7x7 pad 3 at stride 2, got k = {k}, pad = {pad}, '
                             f'stride = {stride}')
        if tuple(scale.shape) != (Cout,):
            raise ValueError(f'scale must be ({Cout},), got {tuple(scale.shape)}')
        return x, w, scale, B, H, W, Cin, Cout, k, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1

    def conv2d_wgrad_splits(self, B, H, W, Cin, Cout, k, stride, pad):
        """``specmi_conv2d_wgrad_splits``: the number of splits S of the weight gradient's contraction at this layer shape (1 = one
        launch); a function of the shape alone."""
        s = C.c_int(0)
        if self.lib.specmi_conv2d_wgrad_splits(B, H, W, Cin, Cout, k, k, stride, pad, C.byref(s)) != 0:
            raise ValueError(f'not a layer the trainable conv builds: B = {B}, H = {H}, W = {W}, Cin = {Cin}, Cout = {Cout}, k = {k}, '
                             f'stride = {stride}, pad = {pad}')
        return s.value

    def conv2d_train_forward(self, x, w, scale, shift, stride, pad, residual=None, relu=True):
        """``specmi_conv2d_train_forward``: y = act(conv(x, w) * scale + shift [+ residual]) with x (B, H, W, Cin) NHWC, w torch's
        (Cout, Cin, k, k) tensor and scale / shift (Cout), all read on the device where they lie -> y (B, OH, OW, Cout) NHWC."""
        x, w, scale, B, H, W, Cin, Cout, k, OH, OW = self._conv_train_args(x, w, scale, stride, pad)
        shift = _dev_f32(shift, self.device, (Cout,))
        res = _dev_f32(residual, self.device, (B, OH, OW, Cout))
        y = self._empty(B, OH, OW, Cout)
        if y.numel():
            _lib.check(self.h, self.lib.specmi_conv2d_train_forward(self.h, _ptr(x), B, H, W, Cin, _ptr(w), _ptr(scale), _ptr(shift), Cout, k, k,
                                                                    stride, pad, _ptr(res), int(bool(relu)), _ptr(y), self._stream()))
        return y

    def conv2d_backward(self, x, w, scale, stride, pad, y, g_y, relu=True, g_x_add=None, want=(True, True, False), g_x_out=None):
        """``specmi_conv2d_backward``: the forward's x, w, scale, its output y (may be None without relu) and g_y -> (g_x, g_w, g_res),
        None where ``want`` = (g_x, g_w, g_res) says so.  ``g_x_add`` (B, H, W, Cin) is added to g_x; ``g_x_out``: the tensor g_x is
        written to (it may be ``g_x_add`` itself: the sum in place)."""
        x, w, scale, B, H, W, Cin, Cout, k, OH, OW = self._conv_train_args(x, w, scale, stride, pad)
        g = _dev_f32(g_y, self.device, (B, OH, OW, Cout))
        yy = _dev_f32(y, self.device, (B, OH, OW, Cout))
        if relu and yy is None:
            raise ValueError('relu needs y (the mask is y > 0)')
        if not any(want):
            raise ValueError('no output is wanted')
        add = _dev_f32(g_x_add, self.device, (B, H, W, Cin)) if want[0] else None
        g_x = None
        if want[0]:
            g_x = g_x_out if g_x_out is not None else self._empty(B, H, W, Cin)
            if tuple(g_x.shape) != (B, H, W, Cin) or g_x.dtype != torch.float32 or g_x.device != self.device or not g_x.is_contiguous():
                raise ValueError(f'g_x_out must be a dense fp32 tensor of shape {(B, H, W, Cin)} on {self.device}')
        g_w = torch.empty_like(w) if want[1] else None
        g_res = self._empty(B, OH, OW, Cout) if want[2] else None
        _lib.check(self.h, self.lib.specmi_conv2d_backward(self.h, _ptr(x), B, H, W, Cin, _ptr(w), _ptr(scale), Cout, k, k, stride, pad, _ptr(yy),
                                                           int(bool(relu)), _ptr(g), _ptr(add), _ptr(g_x), _ptr(g_w), _ptr(g_res), self._stream()))
        return g_x, g_w, g_res

    def _bn_args(self, z, gamma):
        """The tensor of the two BatchNorm calls, checked -> (z, gamma, M, C): z (..., C) with C contiguous, read in place when it is
        dense fp32 on this device."""
        z, gamma = _dev_f32(z, self.device), _dev_f32(gamma, self.device)
        if z.dim() < 2 or z.shape[-1] < 1 or tuple(gamma.shape) != (z.shape[-1],):
            raise ValueError(f'z must be (..., C) with C >= 1 and gamma (C,), got {tuple(z.shape)} and {tuple(gamma.shape)}')
        C_ = z.shape[-1]
        M = z.numel() // C_
        if M < 2:
            raise ValueError(f'batch statistics need more than one value per channel, got {M}')
        return z, gamma, M, C_

    def batchnorm_train_forward(self, z, gamma, beta, eps=1e-5, residual=None, relu=False, running_mean=None, running_var=None, momentum=0.1):
        """``specmi_batchnorm_train_forward``: BatchNorm on the statistics of the batch, y = (z - mean) invstd gamma + beta [+ residual]
        [max(., 0)], z (..., C) NHWC -> (y, mean (C), invstd (C)).  ``running_mean`` / ``running_var`` (both or neither; dense fp32
        vectors on this device) are updated IN PLACE with the factor ``momentum``."""
        z, gamma, M, C_ = self._bn_args(z, gamma)
        beta = _dev_f32(beta, self.device, (C_,))
        res = _dev_f32(residual, self.device, tuple(z.shape))
        if (running_mean is None) != (running_var is None):
            raise ValueError('running_mean and running_var are given together or not at all')
        for name, t in (('running_mean', running_mean), ('running_var', running_var)):
            _dev_tensor(name, t, torch.float32, self.device, optional=True)
            if t is not None and tuple(t.shape) != (C_,):
                raise ValueError(f'{name} must be ({C_},), got {tuple(t.shape)}')
        y, mean, invstd = torch.empty_like(z), self._empty(C_), self._empty(C_)
        _lib.check(self.h, self.lib.specmi_batchnorm_train_forward(self.h, _ptr(z), M, C_, _ptr(gamma), _ptr(beta), _ptr(res), int(bool(relu)),
                                                                   float(eps), float(momentum), _ptr(running_mean), _ptr(running_var), _ptr(y),
                                                                   _ptr(mean), _ptr(invstd), self._stream()))
        return y, mean, invstd

    def batchnorm_backward(self, z, gamma, mean, invstd, y, g_y, relu=False, want=(True, True, True, False), g_res_out=None):
        """``specmi_batchnorm_backward``: the forward's z, gamma, mean, invstd, its output y (may be None without relu) and g_y ->
        (g_z, g_gamma, g_beta, g_res), None where ``want`` says so.  ``g_res_out``: the tensor g_res is written to (it may be ``g_y``
        itself)."""
        z, gamma, M, C_ = self._bn_args(z, gamma)
        mean, invstd = _dev_f32(mean, self.device, (C_,)), _dev_f32(invstd, self.device, (C_,))
        g = _dev_f32(g_y, self.device, tuple(z.shape))
        yy = _dev_f32(y, self.device, tuple(z.shape))
        if relu and yy is None:
            raise ValueError('relu needs y (the mask is y > 0)')
        if not any(want):
            raise ValueError('no output is wanted')
        g_z = torch.empty_like(z) if want[0] else None
        g_gamma = self._empty(C_) if want[1] else None
        g_beta = self._empty(C_) if want[2] else None
        g_res = None
        if want[3]:
            g_res = g_res_out if g_res_out is not None else torch.empty_like(z)
            if g_res.shape != z.shape or g_res.dtype != torch.float32 or g_res.device != self.device or not g_res.is_contiguous():
                raise ValueError(f'g_res_out must be a dense fp32 tensor of shape {tuple(z.shape)} on {self.device}')
        _lib.check(self.h, self.lib.specmi_batchnorm_backward(self.h, _ptr(z), M, C_, _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(yy), int(bool(relu)),
                                                              _ptr(g), _ptr(g_z), _ptr(g_gamma), _ptr(g_beta), _ptr(g_res), self._stream()))
        return g_z, g_gamma, g_beta, g_res

    def conv2d(self, x, w_oihw, scale, shift, stride, pad, residual=None, relu=True, nchw_input=False, out=None,
               x2=None, w2_oihw=None, stride2=1):
        """Single fused layer (tests).  x NHWC device tensor (NCHW for the 7x7 stem).  x, x2 and out may be channel-sliced views
        of wider NHWC maps (unit channel stride, pixel stride ld >= C: specmi_conv2d_strided's ldx / ldx2 / ldo); a residual is
        read with out's pixel stride.  out: where the result goes (only its (pixel, channel < Cout) floats are written); by
        default a dense new tensor.  x2 / w2_oihw / stride2: the second A source of a 1x1 layer (B,H2,W2,Cin2) and its 1x1
        weights (Cout,Cin2,1,1), concatenated after w along K."""
        def rows(t):      # (tensor, pixel stride): a view that fits is passed as it is, anything else as a dense copy
            if isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 4:
                t = t.to(self.device)         # (a tensor already there is returned as it is, strides included)
                ld = self._pixel_rows(t)
                if ld is not None:
                    return t, ld
            t = _dev_f32(t, self.device)
            return t, t.shape[-1]
        w = np.asarray(w_oihw, dtype=np.float32)
        sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float32))
        sh = np.ascontiguousarray(np.asarray(shift, dtype=np.float32))
        cout, cin, kh, kw = w.shape
        if nchw_input:
            x = _dev_f32(x, self.device)
            B, _, H, W = x.shape
            ldx = cin
        else:
            x, ldx = rows(x)
            B, H, W, _ = x.shape
        cin2 = H2 = W2 = ldx2 = 0
        if x2 is not None:
            x2, ldx2 = rows(x2)
            _, H2, W2, cin2 = x2.shape
            w = np.concatenate([w, np.asarray(w2_oihw, dtype=np.float32)], axis=1)
        w = np.ascontiguousarray(w)
        oh, ow = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
        if out is None:
            out = torch.empty(B, oh, ow, cout, device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (B, oh, ow, cout) or out.dtype != torch.float32 or not out.is_cuda:
            raise ValueError(f'out must be a float32 cuda tensor of shape {(B, oh, ow, cout)}')
        ldo = self._pixel_rows(out)
        if ldo is None:
            raise ValueError(f'out: unit channel stride and one pixel stride >= Cout expected, got strides {tuple(out.stride())}')
        res, ldr = (None, ldo) if residual is None else rows(residual)
        if res is not None and tuple(res.shape) != (B, oh, ow, cout):
            raise ValueError(f'expected shape {(B, oh, ow, cout)}, got {tuple(res.shape)}')
        if ldr != ldo:
            raise ValueError(f'the residual is read with the pixel stride of out ({ldo}), got {ldr}')
        _lib.check(self.h, self.lib.specmi_conv2d_strided(
            self.h, _ptr(x), B, H, W, cin, ldx, w.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
            sh.ctypes.data_as(C.c_void_p), cout, kh, kw, stride, pad, _ptr(res), int(relu), _ptr(out), ldo,
            _ptr(x2), H2, W2, cin2, ldx2, int(stride2), self._stream()))
        return out

    def conv2d_f16(self, x, w_oihw, scale, shift, stride, pad, residual=None, relu=True, out_f32=False,
                   x2=None, w2_oihw=None, stride2=1):
        """Single fused layer of the fp16 trunk (tests).  x (B,H,W,Cp) fp16 NHWC device tensor, Cp = Cin rounded up to 8
        (zero padded); w (Cout,Cin,KH,KW) the unfolded weights, scale / shift the BN fold.  x2 / w2_oihw: the folded
        downsample's second A source (B,H2,W2,Cin2) and its 1x1 weights (Cout,Cin2,1,1), concatenated after w along K."""
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float16 and x.is_cuda):
            raise TypeError('x must be a float16 cuda tensor')
        x = x.contiguous()
        w = np.asarray(w_oihw, dtype=np.float32)
        cout, cin, kh, kw = w.shape
        B, H, W, _ = x.shape
        cin2, H2, W2 = 0, 0, 0
        if x2 is not None:
            x2 = x2.contiguous()
            _, H2, W2, cin2 = x2.shape
            w = np.concatenate([w, np.asarray(w2_oihw, dtype=np.float32)], axis=1)
        w = np.ascontiguousarray(w)
        sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float32))
        sh = np.ascontiguousarray(np.asarray(shift, dtype=np.float32))
        oh, ow = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
        out = torch.empty(B, oh, ow, cout, device=self.device, dtype=torch.float32 if out_f32 else torch.float16)
        res = None if residual is None else residual.contiguous()
        _lib.check(self.h, self.lib.specmi_conv2d_f16(
            self.h, _ptr(x), B, H, W, cin, w.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
            sh.ctypes.data_as(C.c_void_p), cout, kh, kw, stride, pad, _ptr(res), int(relu), _ptr(out), int(bool(out_f32)),
            _ptr(x2), H2, W2, cin2, int(stride2), self._stream()))
        return out

    def maxpool(self, x):
        x = _dev_f32(x, self.device)
        B, H, W, Cc = x.shape
        out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, device=self.device, dtype=torch.float32)
        _lib.check(self.h, self.lib.specmi_maxpool3x3s2(self.h, _ptr(x), B, H, W, Cc, _ptr(out), self._stream()))
        return out

    def maxpool_train_forward(self, x):
        """``specmi_maxpool3x3s2_train_forward``: MaxPool2d(3, 2, 1) of x (B, H, W, C) NHWC fp32 -> (y (B, OH, OW, C), idx uint8 of y's
        shape: the winning tap ky * 3 + kx, torch's tie and NaN rule)."""
        x = _dev_f32(x, self.device)
        if x.dim() != 4 or not x.numel():
            raise ValueError(f'x must be (B, H, W, C) NHWC with every dimension >= 1, got {tuple(x.shape)}')
        B, H, W, Cc = x.shape
        y = self._empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc)
        idx = torch.empty(y.shape, device=self.device, dtype=torch.uint8)
        _lib.check(self.h, self.lib.specmi_maxpool3x3s2_train_forward(self.h, _ptr(x), B, H, W, Cc, _ptr(y), _ptr(idx), self._stream()))
        return y, idx

    def maxpool_backward(self, g_y, idx, H, W):
        """``specmi_maxpool3x3s2_backward``: g_y (B, OH, OW, C) and the forward's idx -> g_x (B, H, W, C), H and W the forward's input
        extents ((H - 1) // 2 + 1 == OH); every element is written, pixels that never won are exactly zero."""
        g = _dev_f32(g_y, self.device)
        _dev_tensor('idx', idx, torch.uint8, self.device)
        if g.dim() != 4 or not g.numel() or idx.shape != g.shape or not idx.is_contiguous():
            raise ValueError(f'g_y must be (B, OH, OW, C) with every dimension >= 1 and idx a dense uint8 tensor of its shape, got '
                             f'{tuple(g.shape)} and {tuple(idx.shape)}')
        B, OH, OW, Cc = g.shape
        if H < 1 or W < 1 or ((H - 1) // 2 + 1, (W - 1) // 2 + 1) != (OH, OW):
            raise ValueError(f'an input of {H} x {W} pools to {(H - 1) // 2 + 1} x {(W - 1) // 2 + 1}, not to {OH} x {OW}')
        g_x = self._empty(B, H, W, Cc)
        _lib.check(self.h, self.lib.specmi_maxpool3x3s2_backward(self.h, _ptr(g), _ptr(idx), B, H, W, Cc, _ptr(g_x), self._stream()))
        return g_x

    def maxpool_f16(self, x):
        """MaxPool2d(3, 2, 1) of the fp16 trunk (tests).  x (B,H,W,C) fp16 NHWC device tensor, C % 8 == 0."""
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float16 and x.is_cuda):
            raise TypeError('x must be a float16 cuda tensor')
        x = x.contiguous()
        B, H, W, Cc = x.shape
        out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, device=self.device, dtype=torch.float16)
        _lib.check(self.h, self.lib.specmi_maxpool3x3s2_f16(self.h, _ptr(x), B, H, W, Cc, _ptr(out), self._stream()))
        return out

    def to_nhwc_f16(self, x):
        """The fp16 trunk's image conversion (tests).  x (B,C,H,W) fp32 NCHW, C <= 8 -> (B,H,W,8) fp16 NHWC, pad channels zero."""
        x = _dev_f32(x, self.device)
        B, Cc, H, W = x.shape
        out = torch.empty(B, H, W, 8, device=self.device, dtype=torch.float16)
        _lib.check(self.h, self.lib.specmi_to_nhwc_f16(self.h, _ptr(x), B, Cc, H, W, _ptr(out), self._stream()))
        return out

    def avgpool(self, x):
        x = _dev_f32(x, self.device)
        B, H, W, Cc = x.shape
        out = torch.empty(B, Cc, device=self.device, dtype=torch.float32)
        _lib.check(self.h, self.lib.specmi_avgpool(self.h, _ptr(x), B, H * W, Cc, _ptr(out), self._stream()))
        return out

    def fc_forward(self, w, bias, x, out, B, residual=None, path=0, ldx=None, ldo=None):
        """One Linear layer of the heads on its own (specmi_fc_forward, tests).  One head: w (N,K), bias (N), x, out; up to three
        heads of one shape: lists of those.  x: fp32 device tensors holding B rows of ldx floats (default: the tensor's row stride),
        out (and residual, which may be out itself): device tensors of 4-byte words holding B rows of ldo words - only
        out[b*ldo + n], n < N, is written.  path 0 = the small-batch GEMV kernel, 1 = the matrix-core GEMM (one head)."""
        many = isinstance(w, (list, tuple))
        ws, bs, xs, outs = (list(v) if many else [v] for v in (w, bias, x, out))
        rs = None if residual is None else (list(residual) if many else [residual])
        n = len(ws)
        if not 1 <= n <= 3 or len(bs) != n or len(xs) != n or len(outs) != n or (rs is not None and len(rs) != n):
            raise ValueError('one to three heads, each with its weights, bias, x and out')
        ws = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in ws]
        bs = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in bs]
        N, K = ws[0].shape
        if any(a.shape != (N, K) for a in ws) or any(a.shape != (N,) for a in bs):
            raise ValueError(f'every head needs (N, K) = {(N, K)} weights and an (N,) bias')
        for a in xs + outs + (rs or []):
            if not (isinstance(a, torch.Tensor) and a.device == self.device and a.element_size() == 4):
                raise ValueError(f'x, out and residual must be tensors of 4-byte words on {self.device}')
        ldx = int(xs[0].stride(0) if ldx is None else ldx)
        ldo = int(outs[0].stride(0) if ldo is None else ldo)
        arr = lambda ptrs: (C.c_void_p * 3)(*ptrs, *([None] * (3 - n)))
        _lib.check(self.h, self.lib.specmi_fc_forward(
            self.h, n, arr([a.ctypes.data for a in ws]), arr([a.ctypes.data for a in bs]), N, K, arr([a.data_ptr() for a in xs]), ldx,
            None if rs is None else arr([a.data_ptr() for a in rs]), arr([a.data_ptr() for a in outs]), ldo, int(B), int(path),
            self._stream()))
        return out

    # ---- HRNet's own kernels on their own (tests): the launchers the trunk calls ---------------
    def _nhwc_rows(self, t):
        """-> (fp32 device tensor, pixel stride): a (B,H,W,C) view with unit channel stride and one pixel stride ld >= C is
        passed as it is (a channel slice of a wider map), anything else as a dense copy."""
        if isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 4 and t.device == self.device:
            ld = self._pixel_rows(t)
            if ld is not None:
                return t, ld
        t = _dev_f32(t, self.device)
        if t.dim() != 4:
            raise ValueError(f'expected a (B,H,W,C) tensor, got shape {tuple(t.shape)}')
        return t, t.shape[-1]

    def _nhwc_out(self, out, shape):
        """The output of a kernel-level call: ``out`` (a float32 device view of ``shape`` in pixel rows) or a dense new tensor."""
        if out is None:
            return self._empty(*shape), shape[-1]
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == self.device and tuple(out.shape) == tuple(shape)):
            raise ValueError(f'out must be a float32 tensor of shape {tuple(shape)} on {self.device}')
        ldo = self._pixel_rows(out)
        if ldo is None:
            raise ValueError(f'out: unit channel stride and one pixel stride >= C expected, got strides {tuple(out.stride())}')
        return out, ldo

    def hr_stem3x3(self, images, w_oihw, scale, shift, out=None):
        """HRNet's first layer on its own (specmi_hr_stem3x3): images (B,3,H,W) fp32 NCHW, w (64,3,3,3) OIHW, scale / shift (64)
        -> ReLU(conv3x3 / stride 2 / pad 1 * scale + shift) as (B,OH,OW,64) NHWC.  out: a dense tensor of that shape to write into."""
        x = _dev_f32(images, self.device)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f'images must be (B,3,H,W), got {tuple(x.shape)}')
        w = np.asarray(w_oihw, dtype=np.float32)
        if w.shape != (64, 3, 3, 3):
            raise ValueError(f'w must be (64,3,3,3), got {w.shape}')
        wk = _dev_f32(np.ascontiguousarray(w.reshape(64, 27).T), self.device)       # [(c*3+ky)*3+kx][cout]
        sc, sh = _dev_f32(scale, self.device, (64,)), _dev_f32(shift, self.device, (64,))
        B, _, H, W = x.shape
        out, ldo = self._nhwc_out(out, (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64))
        if ldo != 64:
            raise ValueError('the stem writes a dense (B,OH,OW,64) map')
        _lib.check(self.h, self.lib.specmi_hr_stem3x3(self.h, _ptr(x), B, H, W, _ptr(wk), _ptr(sc), _ptr(sh), _ptr(out), self._stream()))
        return out

    def hr_fuse_sum(self, terms, sh, relu=True, out=None):
        """HRNet's exchange-unit sum on its own (specmi_hr_fuse_sum): out = [ReLU](((t0 + t1) + t2) + t3) in that order, term k
        (B, H >> sh[k], W >> sh[k], C) NHWC read nearest-upsampled by 2^sh[k].  Terms and out may be channel-sliced views of
        wider maps (each with its own pixel stride); one term, relu=False: the strided copy into the concat head's slice."""
        n = len(terms)
        if not 1 <= n <= 4 or len(sh) != n:
            raise ValueError('one to four terms, one shift each')
        rows = [self._nhwc_rows(t) for t in terms]
        B, h0, w0, Cc = rows[0][0].shape
        H, W = h0 << sh[0], w0 << sh[0]
        for (t, _), s in zip(rows, sh):
            if s < 0 or tuple(t.shape) != (B, H >> s, W >> s, Cc) or (H >> s) << s != H or (W >> s) << s != W:
                raise ValueError(f'term of shape {tuple(t.shape)} with shift {s} does not make a {(B, H, W, Cc)} map')
        out, ldo = self._nhwc_out(out, (B, H, W, Cc))
        ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t, _ in rows], *([None] * (4 - n)))
        lds = (C.c_int * 4)(*[ld for _, ld in rows], *([0] * (4 - n)))
        shs = (C.c_int * 4)(*[int(s) for s in sh], *([0] * (4 - n)))
        _lib.check(self.h, self.lib.specmi_hr_fuse_sum(self.h, ptrs, lds, shs, n, B, H, W, Cc, int(bool(relu)), _ptr(out), ldo, self._stream()))
        return out

    def hr_resize_ac(self, x, size, out=None):
        """HRNet's 'interp' head resize on its own (specmi_hr_resize_ac): F.interpolate(bilinear, align_corners=True) of x
        (B,H,W,C) NHWC to size = (OH, OW).  x and out may be channel-sliced views of wider maps."""
        x, ld = self._nhwc_rows(x)
        B, H, W, Cc = x.shape
        OH, OW = int(size[0]), int(size[1])
        out, ldo = self._nhwc_out(out, (B, OH, OW, Cc))
        _lib.check(self.h, self.lib.specmi_hr_resize_ac(self.h, _ptr(x), B, H, W, Cc, ld, _ptr(out), OH, OW, ldo, self._stream()))
        return out

    # ---- profiling -------------------------------------------------------------------------
    def profile(self, on: bool):
        _lib.check(self.h, self.lib.specmi_profile_enable(self.h, int(on)))

    def profile_read(self, max_entries: int = 512):
        arr = (_lib.ProfEntry * max_entries)()
        n = C.c_int(0)
        _lib.check(self.h, self.lib.specmi_profile_read(self.h, arr, max_entries, C.byref(n)))
        return [{'kernel': arr[i].kernel.decode(), 'label': arr[i].label.decode(), 'ms': arr[i].ms,
                 'flops': arr[i].flops, 'bytes': arr[i].bytes, 'launches': arr[i].launches}
                for i in range(min(n.value, max_entries))]
