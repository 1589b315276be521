"""The tail of the reference's training step with gradients, on the device: ``rot6d_to_rotmat`` and the two SMPL heads of
``spec/models/hmr.py:101-120`` as ``torch.autograd.Function``s over the library's own forward (``specmi_smpl_forward``, the
head's Gram-Schmidt) and its hand-written backward (``specmi_smpl_backward``, ``specmi_rot6d_backward``;
spec_amd/csrc/smpl_bwd.hip).  No trained parameters and no BatchNorm live here: the chain is head state (144 rot6d + 10 betas
+ 3 cam) -> rotation matrices -> SMPL LBS + 49 joints -> camera translation + perspective projection.  It is what
camera-aware test-time refinement needs - optimise pose / shape / camera of a detection against 2D keypoints under the
CamCalib camera - and where a trunk backward would start, from the gradient of the head's state vector.

First derivatives only (``once_differentiable``).  The camera arguments (``cam_rotmat``, ``cam_intrinsics``, the box, the image
size) get no gradient.  With no input requiring grad the heads return exactly what ``Engine.smpl`` returns.
"""
from __future__ import annotations

import threading

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .cam_utils import _engine
from .engine import Engine

_tls = threading.local()
_KEYS = ('smpl_vertices', 'smpl_joints3d', 'smpl_joints2d', 'pred_cam_t')


def _smpl_engine(device, model, use_cam, img_res, focal_length) -> Engine:
    """One SMPL-only engine per thread, device and head configuration (a handle is not thread-safe), rebuilt when the body model
    it was built from is no longer the one asked for - the rule of ``losses.gt_vertices``."""
    if model is None:
        from . import assets
        model = assets.smpl_model()
    dev = torch.device('cuda', device.index if device.index is not None else torch.cuda.current_device())
    cache = getattr(_tls, 'engines', None)
    if cache is None:
        cache = _tls.engines = {}
    key = (dev, bool(use_cam), int(img_res), float(focal_length))
    if key not in cache or cache[key][0] is not model:      # the entry holds the dict it was built from: `is` cannot alias
        eng = Engine('smpl', dev)
        eng.load({}, smpl=model, use_cam=int(bool(use_cam)), img_res=int(img_res), focal_length=float(focal_length))
        cache[key] = (model, eng)
    return cache[key][1]


def _device_of(t):
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise RuntimeError('spec_amd.differentiable needs device tensors (no CPU path)')
    return t.device


class _Rot6d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xc = x.detach().float().contiguous()
        ctx.save_for_backward(xc)
        return _engine(xc.device).rot6d_to_rotmat(xc)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        return _engine(xc.device).rot6d_backward(xc, g)


def rot6d_to_rotmat(x):
    """``pare.utils.geometry.rot6d_to_rotmat`` (spec/losses.py:23, the last line of HMRHead): (B, 144) or (N, 6) ->
    (N, 3, 3), Gram-Schmidt with columns b1, b2, b3 on the device, differentiable in ``x``."""
    _device_of(x)
    return _Rot6d.apply(x)


class _Smpl(torch.autograd.Function):
    """(rotmat, betas, cam) -> the four outputs of ``Engine.smpl``; ``camera`` = the six camera tensors (or Nones)."""

    @staticmethod
    def forward(ctx, eng, camera, rotmat, betas, cam):
        out = eng.smpl(rotmat.detach(), betas.detach(), cam.detach(), *camera)
        ctx.eng, ctx.camera = eng, camera
        ctx.set_materialize_grads(False)      # an unused output arrives as None = the library's NULL, not as a (B,V,3) tensor of zeros
        ctx.save_for_backward(rotmat.detach(), betas.detach(), cam.detach())
        ctx.rot_shape = rotmat.shape
        return tuple(out[k] for k in _KEYS)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_vertices, g_joints3d, g_joints2d, g_cam_t):
        rotmat, betas, cam = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[2:5])
        g = ctx.eng.smpl_backward(rotmat, betas, cam, *ctx.camera, g_vertices=g_vertices, g_joints3d=g_joints3d,
                                  g_joints2d=g_joints2d, g_cam_t=g_cam_t, want=want)
        g_rot = g[0].reshape(ctx.rot_shape) if g[0] is not None else None
        return None, None, g_rot, g[1], g[2]


def _run(eng, camera, rotmat, betas, cam):
    _device_of(rotmat)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (rotmat, betas, cam)):
        return dict(zip(_KEYS, _Smpl.apply(eng, camera, rotmat, betas, cam)))
    return eng.smpl(rotmat, betas, cam, *camera)


class SMPLCamHead(nn.Module):
    """``SMPLCamHead(img_res)`` of spec/models/hmr.py:69, call signature of :101-112: SMPL + full-image camera translation +
    perspective projection, differentiable in ``rotmat``, ``shape`` and ``cam``.  ``model``: the body model's tensor dict
    (default ``spec_amd.assets.smpl_model()``)."""

    def __init__(self, img_res=224, model=None):
        super().__init__()
        self.img_res = img_res
        self.model = model

    def forward(self, rotmat, shape, cam, cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h,
                normalize_joints2d=False):
        if normalize_joints2d:
            raise NotImplementedError('SMPLCamHead is built as the reference calls it (spec/models/hmr.py:111: normalize_joints2d=False)')
        eng = _smpl_engine(_device_of(rotmat), self.model, True, self.img_res, 5000.)
        return _run(eng, (cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h), rotmat, shape, cam)


class SMPLHead(nn.Module):
    """``SMPLHead(focal_length, img_res)`` of spec/models/hmr.py:71-74, call signature of :115-120: weak perspective, R = I,
    2D joints divided by ``img_res / 2``."""

    def __init__(self, focal_length=5000., img_res=224, model=None):
        super().__init__()
        self.focal_length = focal_length
        self.img_res = img_res
        self.model = model

    def forward(self, rotmat, shape, cam, normalize_joints2d=True):
        if not normalize_joints2d:
            raise NotImplementedError('SMPLHead is built as the reference calls it (spec/models/hmr.py:119: normalize_joints2d=True)')
        eng = _smpl_engine(_device_of(rotmat), self.model, False, self.img_res, self.focal_length)
        return _run(eng, (None,) * 6, rotmat, shape, cam)
