"""The tail of the reference's training step with gradients, on the device: ``rot6d_to_rotmat`` and the two SMPL heads of
``spec/models/hmr.py:101-120`` as ``torch.autograd.Function``s over the library's own forward (``specmi_smpl_forward``, the
head's Gram-Schmidt) and its hand-written backward (``specmi_smpl_backward``, ``specmi_rot6d_backward``;
spec_amd/csrc/smpl_bwd.hip).  No trained parameters and no BatchNorm live here: the chain is head state (144 rot6d + 10 betas
+ 3 cam) -> rotation matrices -> SMPL LBS + 49 joints -> camera translation + perspective projection.  It is what
camera-aware test-time refinement needs - optimise pose / shape / camera of a detection against 2D keypoints under the
CamCalib camera - and where a trunk backward would start, from the gradient of the head's state vector.

Upstream of that state vector sits :class:`HMRHead`, pare's iterative regressor with its five trained Linears, as it runs in
training: dropout on in ``.train()``, the loop and its backward on the library's exact-fp32 matrix-core kernels
(``specmi_hmr_head_train_forward`` / ``specmi_hmr_head_backward``; spec_amd/csrc/head_bwd.hip), which read the Parameters where
torch keeps them - an optimiser steps them as they are.  Its gradient with respect to the pooled feature is where a trunk
backward would start.

Beside it :class:`CameraRegressorHead`: CamCalib's three FC heads (``fc_vfov`` / ``fc_pitch`` / ``fc_roll``, one Linear or a chain of
two or three with no activation between them) on the pooled feature, forward and backward on the same kernels
(``specmi_camcalib_head_train_forward`` / ``specmi_camcalib_head_backward``) - with ``spec_amd.losses.CameraRegressorLoss`` the
differentiable tail of the reference's CamCalib ``training_step`` on a frozen trunk.

Below the pooled feature :class:`ResNetStage`: one stage of a Bottleneck ResNet trunk, every block one
``torch.autograd.Function`` over the trainable conv layer (``specmi_conv2d_train_forward`` / ``specmi_conv2d_backward``;
spec_amd/csrc/conv_bwd.hip) - with ``Engine.trunk(images, stages=3)`` as the frozen part, layer4 of either network fine-tunes.
Its BatchNorm is frozen (``bn='frozen'``, the default) or, as in the reference's ``training_step``, runs on the statistics of the
batch with its running statistics moving and gamma / beta trained (``bn='batch'``; ``specmi_batchnorm_train_forward`` /
``specmi_batchnorm_backward``, spec_amd/csrc/bn_train.hip).

First derivatives only (``once_differentiable``).  The camera arguments (``cam_rotmat``, ``cam_intrinsics``, the box, the image
size) get no gradient.  With no input requiring grad the heads return exactly what ``Engine.smpl`` returns.
"""
from __future__ import annotations

import threading

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .cam_utils import _engine
from .engine import Engine, camcalib_head_param_names
from .modules import HMRHeadParams

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


class _Regressor(torch.autograd.Function):
    """(xf, the ten parameters in the order of ``_lib.HMR_HEAD_PARAMS``) -> state_n (B, 157); ``fixed`` = (init_state, cam_feats,
    masks, p, n_iter), which get no gradient."""

    @staticmethod
    def forward(ctx, eng, fixed, xf, *params):
        init_state, cam_feats, masks, p, n_iter = fixed
        ps = [t.detach() for t in params]
        state, tape = eng.hmr_head_train_forward(dict(zip(_lib.HMR_HEAD_PARAMS, ps)), xf.detach(), init_state, cam_feats, masks, p, n_iter)
        ctx.eng, ctx.fixed = eng, fixed
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf.detach(), tape, *ps)     # (an optimiser step between forward and backward is caught by autograd's version check)
        return state

    @staticmethod
    @once_differentiable
    def backward(ctx, g_state):
        if g_state is None:
            return (None,) * (3 + len(_lib.HMR_HEAD_PARAMS))
        xf, tape, *ps = ctx.saved_tensors
        _, cam_feats, masks, p, n_iter = ctx.fixed
        names = [n for n, need in zip(_lib.HMR_HEAD_PARAMS, ctx.needs_input_grad[3:]) if need]
        g_xf, grads = ctx.eng.hmr_head_backward(dict(zip(_lib.HMR_HEAD_PARAMS, ps)), xf, tape, g_state, cam_feats, masks, p, n_iter,
                                                want_xf=ctx.needs_input_grad[2], want_params=names)
        return (None, None, g_xf) + tuple(grads.get(n) for n in _lib.HMR_HEAD_PARAMS)


class HMRHead(HMRHeadParams):
    """pare's ``HMRHead`` as spec/models/hmr.py:57-64 builds it and :94-98 calls it, trainable: the Parameters and buffers of
    ``modules.HMRHeadParams`` (pare's state_dict names and shapes), ``forward`` with pare's signature and output dict.  In
    ``.train()`` the two ``nn.Dropout(p)`` are on: their keep-masks are ``torch.rand((2 n_iter, B, 1024), generator=self.generator)
    >= p``, ordered (iteration, layer), unless ``dropout_masks`` passes them; in ``.eval()`` they are the identity (masks passed
    are not read).  ``features``: (B, F, h, w), or (B, h, w, F) with ``channels_last=True`` (what ``Engine.trunk`` returns), or
    (B, F) already pooled; it and the ten Parameters get gradients, ``init_*`` and the camera inputs do not.  When grad is
    disabled or nothing requires grad no tape is kept."""

    def __init__(self, num_input_features=2048, use_cam_feats=False, mean_params=None, p=0.5, estimate_var=False):
        if estimate_var:
            raise NotImplementedError('estimate_var: the variance outputs and their losses are not built for training (DESIGN.md section 6)')
        if not 0.0 <= p < 1.0:
            raise ValueError(f'p = {p} must be in [0, 1)')
        super().__init__(num_input_features, use_cam_feats, mean_params)
        self.num_input_features = int(num_input_features)
        self.use_cam_feats = bool(use_cam_feats)
        self.p = float(p)
        self.generator = None       # a torch.Generator on the features' device; None = torch's default generator

    @classmethod
    def from_hmr(cls, hmr, p=0.5):
        """A head that SHARES the Parameter objects and buffers of ``hmr.head`` (a ``spec_amd.modules.HMR``): an optimiser step on
        this head's parameters is a step on the model's, and the model's next eval-mode call sees the bumped tensor versions and
        commits them again by itself."""
        if hmr.estimate_var:
            raise NotImplementedError('estimate_var: the variance outputs and their losses are not built for training (DESIGN.md section 6)')
        src = hmr.head
        C = 7 if hmr.use_cam_feats else 0
        mp = {'pose': src.init_pose.detach().cpu().numpy(), 'shape': src.init_shape.detach().cpu().numpy(), 'cam': src.init_cam.detach().cpu().numpy()}
        head = cls(src.fc1.in_features - 157 - C, bool(hmr.use_cam_feats), mp, p)
        for name in ('fc1', 'fc2', 'decpose', 'decshape', 'deccam'):
            setattr(head, name, getattr(src, name))
        for name in ('init_pose', 'init_shape', 'init_cam'):
            head._buffers[name] = src._buffers[name]
        return head

    def forward(self, features, init_pose=None, init_shape=None, init_cam=None, cam_rotmat=None, cam_vfov=None, n_iter=3, *,
                channels_last=False, dropout_masks=None):
        dev = _device_of(features)
        if features.dim() == 4:
            xf = features.mean(dim=(1, 2) if channels_last else (2, 3))       # the average pool, inside autograd
        elif features.dim() == 2:
            xf = features
        else:
            raise ValueError(f'features must be (B, F, h, w), (B, h, w, F) with channels_last, or (B, F), got {tuple(features.shape)}')
        B = xf.shape[0]
        with torch.no_grad():
            init = [t if t is not None else getattr(self, k).expand(B, -1) for t, k in
                    ((init_pose, 'init_pose'), (init_shape, 'init_shape'), (init_cam, 'init_cam'))]
            init_state = torch.cat([t.to(dev, torch.float32) for t in init], 1)
            cam_feats = None
            if self.use_cam_feats:
                if cam_rotmat is None or cam_vfov is None:
                    raise ValueError('a head built with use_cam_feats needs cam_rotmat and cam_vfov')
                cam_feats = torch.cat([cam_rotmat.reshape(-1, 3, 3)[:, :, :2].reshape(B, 6), cam_vfov.reshape(B, 1)], 1).to(dev, torch.float32)
            masks = None
            if self.training:
                masks = dropout_masks if dropout_masks is not None else \
                    torch.rand(2 * n_iter, B, 1024, device=dev, generator=self.generator) >= self.p
        params = tuple(getattr(getattr(self, n.split('.')[0]), n.split('.')[1]) for n in _lib.HMR_HEAD_PARAMS)
        eng = _engine(dev)
        if torch.is_grad_enabled() and (xf.requires_grad or any(t.requires_grad for t in params)):
            state = _Regressor.apply(eng, (init_state, cam_feats, masks, self.p, n_iter), xf, *params)
        else:
            state, _ = eng.hmr_head_train_forward(dict(zip(_lib.HMR_HEAD_PARAMS, params)), xf, init_state, cam_feats, masks, self.p, n_iter)
        pose6d, shape, cam = state[:, :144], state[:, 144:154], state[:, 154:]
        return {'pred_pose': rot6d_to_rotmat(pose6d).view(B, 24, 3, 3), 'pred_cam': cam, 'pred_shape': shape, 'pred_pose_6d': pose6d}


class _CamHeads(torch.autograd.Function):
    """(xf, the 6 L parameters in the order of ``camcalib_head_param_names(L)``) -> logits (3, B, nbins)."""

    @staticmethod
    def forward(ctx, eng, L, xf, *params):
        names = camcalib_head_param_names(L)
        ps = [t.detach() for t in params]
        logits, tape = eng.camcalib_head_train_forward(dict(zip(names, ps)), xf.detach(), L)
        ctx.eng, ctx.L = eng, L
        ctx.save_for_backward(xf.detach(), tape, *ps)     # (an optimiser step between forward and backward is caught by autograd's version check)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logits):
        xf, tape, *ps = ctx.saved_tensors
        names = camcalib_head_param_names(ctx.L)
        want = [n for n, need in zip(names, ctx.needs_input_grad[3:]) if need]
        g_xf, grads = ctx.eng.camcalib_head_backward(dict(zip(names, ps)), xf, ctx.L, tape, g_logits, want_xf=ctx.needs_input_grad[2],
                                                     want_params=want)
        return (None, None, g_xf) + tuple(grads.get(n) for n in names)


class CameraRegressorHead(nn.Module):
    """The three FC heads of ``CameraRegressorNetwork`` (camcalib/model.py:42-70), trainable: the reference's state_dict names
    (``fc_vfov.weight``, or ``fc_vfov.0.weight`` .. for chains) and its initialisation (N(0, 0.01) weights and zero bias for one
    Linear, ``nn.Linear``'s default for chains).  ``forward(features)`` -> [vfov, pitch, roll] logits, each (B, num_out_channels).
    ``features``: (B, F, h, w), or (B, h, w, F) with ``channels_last=True`` (what ``Engine.trunk`` returns), or (B, F) already
    pooled; it and the parameters get gradients.  When grad is disabled or nothing requires grad no tape is kept."""

    def __init__(self, num_input_features=2048, num_fc_layers=1, num_fc_channels=1024, num_out_channels=256):
        super().__init__()
        if not 1 <= num_fc_layers <= _lib.CAMCALIB_HEAD_MAX_LAYERS:
            raise NotImplementedError(f'num_fc_layers in 1 .. {_lib.CAMCALIB_HEAD_MAX_LAYERS} are built')
        self.num_input_features, self.num_fc_layers = int(num_input_features), int(num_fc_layers)
        self.num_fc_channels, self.num_out_channels = int(num_fc_channels), int(num_out_channels)
        for name in _lib.CAMCALIB_HEADS:
            if num_fc_layers == 1:
                fc = nn.Linear(num_input_features, num_out_channels)
                nn.init.normal_(fc.weight, mean=0, std=0.01)
                nn.init.constant_(fc.bias, 0)
            else:
                widths = [num_input_features] + [num_fc_channels] * (num_fc_layers - 1) + [num_out_channels]
                fc = nn.Sequential(*(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:])))
            setattr(self, name, fc)

    @classmethod
    def from_model(cls, net):
        """A head that SHARES the ``fc_*`` modules of ``net`` (a ``spec_amd.modules.CameraRegressorNetwork``), and so its Parameter
        objects: an optimiser step on this head's parameters is a step on the network's, and the network's next call sees the
        bumped tensor versions and commits them again by itself."""
        first = net.fc_vfov if net.num_fc_layers == 1 else net.fc_vfov[0]
        head = cls(first.in_features, net.num_fc_layers, net.num_fc_channels, net.num_out_channels)
        for name in _lib.CAMCALIB_HEADS:
            setattr(head, name, getattr(net, name))
        return head

    def _params(self):
        sd = dict(self.named_parameters())
        return tuple(sd[n] for n in camcalib_head_param_names(self.num_fc_layers))

    def forward(self, features, channels_last=False):
        dev = _device_of(features)
        if features.dim() == 4:
            xf = features.mean(dim=(1, 2) if channels_last else (2, 3))       # the average pool, inside autograd
        elif features.dim() == 2:
            xf = features
        else:
            raise ValueError(f'features must be (B, F, h, w), (B, h, w, F) with channels_last, or (B, F), got {tuple(features.shape)}')
        params, L = self._params(), self.num_fc_layers
        eng = _engine(dev)
        if torch.is_grad_enabled() and (xf.requires_grad or any(t.requires_grad for t in params)):
            logits = _CamHeads.apply(eng, L, xf, *params)
        else:
            logits, _ = eng.camcalib_head_train_forward(dict(zip(camcalib_head_param_names(L), params)), xf, L)
        return list(logits.unbind(0))


def _fold_bn(bn):
    """Frozen BatchNorm as the affine map of ``commit.hip``'s ``fold_bn``, in its fp32 expression, from the running statistics on the
    device: scale = gamma / sqrt(var + eps), shift = beta - mean * scale.  No gradient reaches gamma or beta."""
    with torch.no_grad():
        invstd = 1.0 / torch.sqrt(bn.running_var.float() + float(bn.eps))
        scale = invstd * bn.weight.float()
        return scale.contiguous(), (bn.bias.float() - bn.running_mean.float() * scale).contiguous()


def _bottleneck_forward(eng, stride, folds, x, ws):
    """conv1 -> conv2 -> [downsample, relu = 0] -> conv3 with the residual -> (y1, y2, out)."""
    y1 = eng.conv2d_train_forward(x, ws[0], *folds[0], 1, 0)
    y2 = eng.conv2d_train_forward(y1, ws[1], *folds[1], stride, 1)
    idn = eng.conv2d_train_forward(x, ws[3], *folds[3], stride, 0, relu=False) if len(ws) == 4 else x
    return y1, y2, eng.conv2d_train_forward(y2, ws[2], *folds[2], 1, 0, residual=idn)


class _Bottleneck(torch.autograd.Function):
    """(x NHWC, conv1 / conv2 / conv3 [/ downsample] weights) -> the block's output NHWC; ``folds`` = the (scale, shift) pairs of the
    frozen BatchNorms in the same order, which get no gradient."""

    @staticmethod
    def forward(ctx, eng, stride, folds, x, *ws):
        xd, wd = x.detach().float().contiguous(), [w.detach() for w in ws]
        y1, y2, out = _bottleneck_forward(eng, stride, folds, xd, wd)
        ctx.eng, ctx.stride, ctx.scales = eng, stride, [f[0] for f in folds]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xd, y1, y2, out, *wd)       # (an optimiser step between forward and backward is caught by autograd's version check)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        x, y1, y2, out, *ws = ctx.saved_tensors
        n = len(ws)
        if g_out is None:
            return (None,) * (4 + n)
        eng, s, sc = ctx.eng, ctx.stride, ctx.scales
        need_x, need_w = ctx.needs_input_grad[3], list(ctx.needs_input_grad[4:])
        below1 = need_x or need_w[0]                      # is g_y1 needed, is g_y2
        below2 = below1 or need_w[1]
        has_ds = n == 4
        g_w = [None] * n
        want3 = (below2, need_w[2], need_x or (has_ds and need_w[3]))
        if not any(want3):
            return (None,) * (4 + n)
        g_y2, g_w[2], g_res = eng.conv2d_backward(y2, ws[2], sc[2], 1, 0, out, g_out, True, want=want3)
        skip = g_res
        if has_ds and (need_x or need_w[3]):
            skip, g_w[3], _ = eng.conv2d_backward(x, ws[3], sc[3], s, 0, None, g_res, False, want=(need_x, need_w[3], False))
        g_x = None
        if below2:
            g_y1, g_w[1], _ = eng.conv2d_backward(y1, ws[1], sc[1], s, 1, y2, g_y2, True, want=(below1, need_w[1], False))
            if below1:
                # the skip (or downsample) gradient is summed in conv1's epilogue, in place where the buffer is this call's own
                own = need_x and has_ds
                g_x, g_w[0], _ = eng.conv2d_backward(x, ws[0], sc[0], 1, 0, y1, g_y1, True, g_x_add=skip if need_x else None,
                                                     want=(need_x, need_w[0], False), g_x_out=skip if own else None)
        return (None, None, None, g_x) + tuple(g_w)


def _identity_affine(eng, n):
    """The identity affine map of a layer with n output channels, (ones, zeros) on the engine's device, cached on the engine: with it
    ``specmi_conv2d_train_forward`` is the plain product and ``specmi_conv2d_backward`` the product's own gradients."""
    cache = eng.__dict__.setdefault('_identity_affine', {})
    if n not in cache:
        cache[n] = (torch.ones(n, device=eng.device), torch.zeros(n, device=eng.device))
    return cache[n]


def _block_bns(blk):
    return [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if hasattr(blk, 'downsample') else [])


def _bn_step(bn):
    """What ``nn.BatchNorm2d.forward`` does before it normalises in training mode: ``num_batches_tracked`` + 1 and the factor of the
    running-statistics update -> (eps, factor, running_mean, running_var), the last two None for a module that tracks none."""
    if bn.running_mean is None:
        return float(bn.eps), 0.0, None, None
    with torch.no_grad():
        bn.num_batches_tracked.add_(1)
    f = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
    return float(bn.eps), f, bn.running_mean, bn.running_var


def _conv_bn(eng, x, w, stride, pad, gamma, beta, step, residual=None, relu=True):
    """One conv + training-mode BatchNorm [+ residual] [+ ReLU] -> (z, y, mean, invstd): the conv as a plain product, then
    ``specmi_batchnorm_train_forward``, which also moves the running statistics of ``step`` (``_bn_step``) in place."""
    eps, f, rm, rv = step
    z = eng.conv2d_train_forward(x, w, *_identity_affine(eng, w.shape[0]), stride, pad, relu=False)
    y, mean, invstd = eng.batchnorm_train_forward(z, gamma, beta, eps, residual, relu, rm, rv, f)
    for t in (rm, rv):
        if t is not None:
            torch.autograd.graph.increment_version(t)         # written through its pointer: whoever watches the version sees it
    return z, y, mean, invstd


def _bottleneck_batch_forward(eng, stride, steps, x, ws, gammas, betas):
    """The bottleneck on batch statistics -> (out, tape): tape = [(z, y, mean, invstd)] in the order conv1, conv2, conv3[, downsample]."""
    t1 = _conv_bn(eng, x, ws[0], 1, 0, gammas[0], betas[0], steps[0])
    t2 = _conv_bn(eng, t1[1], ws[1], stride, 1, gammas[1], betas[1], steps[1])
    td = _conv_bn(eng, x, ws[3], stride, 0, gammas[3], betas[3], steps[3], relu=False) if len(ws) == 4 else None
    t3 = _conv_bn(eng, t2[1], ws[2], 1, 0, gammas[2], betas[2], steps[2], residual=td[1] if td is not None else x)
    return t3[1], [t1, t2, t3] + ([td] if td is not None else [])


class _BottleneckBatch(torch.autograd.Function):
    """``_Bottleneck`` on BATCH statistics: (x NHWC, the n conv weights, the n gammas, the n betas) -> the block's output NHWC, n = 3
    or 4 in the order conv1, conv2, conv3[, downsample]; ``steps`` = ``_bn_step`` of the BatchNorms in the same order.  Saves z, mean
    and invstd of every BatchNorm; the backward runs ``specmi_batchnorm_backward`` and then ``specmi_conv2d_backward`` on g_z with the
    identity scale and no ReLU."""

    @staticmethod
    def forward(ctx, eng, stride, steps, x, *params):
        n = len(params) // 3
        xd, pd = x.detach().float().contiguous(), [p.detach() for p in params]
        out, tape = _bottleneck_batch_forward(eng, stride, steps, xd, pd[:n], pd[n:2 * n], pd[2 * n:])
        ctx.eng, ctx.stride, ctx.n = eng, stride, n
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xd, *pd[:2 * n], *(t for rec in tape for t in rec))       # (an optimiser step in between is caught by autograd's version check)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        n = ctx.n
        none = (None,) * (4 + 3 * n)
        if g_out is None:
            return none
        x, *rest = ctx.saved_tensors
        ws, gammas, tape = rest[:n], rest[n:2 * n], [rest[2 * n + 4 * i:2 * n + 4 * i + 4] for i in range(n)]
        eng, s = ctx.eng, ctx.stride
        need_x, need = ctx.needs_input_grad[3], list(ctx.needs_input_grad[4:])
        need_w, need_g, need_b = need[:n], need[n:2 * n], need[2 * n:]
        has_ds = n == 4
        # what each launch has to hand down, from the block's input upwards
        conv_any = [need_x or need_w[0]]                                   # conv i's backward is launched: BatchNorm i's g_z is wanted
        bn_any = [conv_any[0] or need_g[0] or need_b[0]]                   # BatchNorm i's backward is launched: its g_y is wanted
        for i in (1, 2):
            conv_any.append(bn_any[i - 1] or need_w[i])
            bn_any.append(conv_any[i] or need_g[i] or need_b[i])
        if has_ds:
            conv_any.append(need_x or need_w[3])
            bn_any.append(conv_any[3] or need_g[3] or need_b[3])
        want_res = bn_any[3] if has_ds else need_x
        if not (bn_any[2] or want_res):
            return none
        g_w, g_g, g_b = [None] * n, [None] * n, [None] * n
        ones = lambda i: _identity_affine(eng, ws[i].shape[0])[0]

        def bn_bwd(i, g_y, relu, res=False):
            z, y, mean, invstd = tape[i]
            g_z, g_g[i], g_b[i], g_res = eng.batchnorm_backward(z, gammas[i], mean, invstd, y if relu else None, g_y, relu,
                                                                want=(conv_any[i], need_g[i], need_b[i], res))
            return g_z, g_res
        g_z3, g_res = bn_bwd(2, g_out, True, want_res)
        skip = g_res
        if has_ds and bn_any[3]:
            g_zd, _ = bn_bwd(3, g_res, False)
            skip = None
            if conv_any[3]:
                skip, g_w[3], _ = eng.conv2d_backward(x, ws[3], ones(3), s, 0, None, g_zd, False, want=(need_x, need_w[3], False))
        g_x = None
        if conv_any[2]:
            g_y2, g_w[2], _ = eng.conv2d_backward(tape[1][1], ws[2], ones(2), 1, 0, None, g_z3, False, want=(bn_any[1], need_w[2], False))
            if bn_any[1]:
                g_z2, _ = bn_bwd(1, g_y2, True)
                if conv_any[1]:
                    g_y1, g_w[1], _ = eng.conv2d_backward(tape[0][1], ws[1], ones(1), s, 1, None, g_z2, False, want=(bn_any[0], need_w[1], False))
                    if bn_any[0]:
                        g_z1, _ = bn_bwd(0, g_y1, True)
                        if conv_any[0]:
                            # the skip (or downsample) gradient is summed in conv1's epilogue, in place where the buffer is this call's own
                            own = need_x and has_ds
                            g_x, g_w[0], _ = eng.conv2d_backward(x, ws[0], ones(0), 1, 0, None, g_z1, False, g_x_add=skip if need_x else None,
                                                                 want=(need_x, need_w[0], False), g_x_out=skip if own else None)
        return (None, None, None, g_x) + tuple(g_w) + tuple(g_g) + tuple(g_b)


class ResNetStage(nn.Module):
    """One stage (``layer1`` .. ``layer4``) of a torchvision-layout Bottleneck trunk (ResNet-50 / 101 / 152), trainable:
    ``forward(x)`` takes (B, h, w, Cin) NHWC - what ``Engine.trunk(images, stages=n - 1)`` returns - and gives
    (B, oh, ow, 4 planes) NHWC.  Every bottleneck is one ``torch.autograd.Function`` over the library's trainable layer
    (``specmi_conv2d_train_forward`` / ``specmi_conv2d_backward``; spec_amd/csrc/conv_bwd.hip), which reads the conv weights where
    torch keeps them - an optimiser steps them as they are.

    ``bn='frozen'`` (the default): BatchNorm is frozen whatever ``train()`` says: at every forward each BN is the affine map
    scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, computed on the device; batch statistics are never
    built, the running statistics are not updated, and gamma / beta get no gradient.  The trainable parameters are the conv weights
    (``conv_parameters()``).

    ``bn='batch'``: the reference's semantics (its trainers are Lightning modules: the whole network is in ``train()`` during
    ``training_step``).  A block in ``train()`` mode normalises every conv's output with the statistics of the batch
    (``specmi_batchnorm_train_forward`` / ``specmi_batchnorm_backward``; spec_amd/csrc/bn_train.hip), moves ``running_mean`` /
    ``running_var`` in place by torch's rule, increments ``num_batches_tracked``, and gamma / beta (``bn_parameters()``) get gradients
    beside the conv weights; an image's output then depends on the rest of its batch.  A block in ``eval()`` mode runs exactly the
    frozen path, on the running statistics as they are by then.
    First derivatives only."""

    def __init__(self, blocks, bn='frozen'):
        super().__init__()
        if bn not in ('frozen', 'batch'):
            raise ValueError(f"bn = {bn!r}: 'frozen' and 'batch' are built")
        self.blocks = blocks
        self.bn = bn

    @classmethod
    def from_model(cls, net, name='layer4', bn='frozen'):
        """The stage ``name`` of ``net.backbone`` (a ``spec_amd.modules.CameraRegressorNetwork`` or ``HMR``), SHARING its block modules
        and so their Parameter objects: an optimiser step on ``conv_parameters()`` is a step on the network's weights, and the
        network's next call sees the bumped tensor versions and commits them again by itself."""
        from .modules import ResNet50Params
        if name not in ('layer1', 'layer2', 'layer3', 'layer4'):
            raise ValueError(f'{name!r} is not a stage: layer1 .. layer4')
        backbone = getattr(net, 'backbone', None)
        if not isinstance(backbone, ResNet50Params):
            raise NotImplementedError(f'ResNetStage is built for the Bottleneck trunks (ResNet-50 / 101 / 152), not for {type(backbone).__name__}')
        return cls(getattr(backbone, name), bn)

    def conv_parameters(self):
        """The conv weights, block by block in the order conv1, conv2, conv3[, downsample]: what an optimiser is given."""
        out = []
        for blk in self.blocks:
            out += [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight] + ([blk.downsample[0].weight] if hasattr(blk, 'downsample') else [])
        return out

    def bn_parameters(self):
        """gamma and beta of every BatchNorm, block by block in the order bn1, bn2, bn3[, downsample]: what an optimiser is given
        beside ``conv_parameters()`` with ``bn='batch'``."""
        return [p for blk in self.blocks for bn in _block_bns(blk) for p in (bn.weight, bn.bias)]

    def forward(self, x):
        dev = _device_of(x)
        if x.dim() != 4:
            raise ValueError(f'x must be (B, h, w, Cin) NHWC, got {tuple(x.shape)}')
        eng = _engine(dev)
        for blk in self.blocks:
            ds = hasattr(blk, 'downsample')
            ws = [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight] + ([blk.downsample[0].weight] if ds else [])
            stride = blk.conv2.stride[0]
            if x.shape[3] != blk.conv1.in_channels:
                raise ValueError(f'the stage takes {blk.conv1.in_channels} channels, x has {x.shape[3]}')
            if self.bn == 'batch' and blk.training:
                bns = _block_bns(blk)
                params = ws + [bn.weight for bn in bns] + [bn.bias for bn in bns]
                steps = [_bn_step(bn) for bn in bns]
                if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
                    x = _BottleneckBatch.apply(eng, stride, steps, x, *params)
                else:
                    n = len(ws)
                    pd = [p.detach() for p in params]
                    x = _bottleneck_batch_forward(eng, stride, steps, x.detach().float().contiguous(), pd[:n], pd[n:2 * n], pd[2 * n:])[0]
                continue
            folds = [_fold_bn(bn) for bn in _block_bns(blk)]
            if torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in ws)):
                x = _Bottleneck.apply(eng, stride, folds, x, *ws)
            else:
                x = _bottleneck_forward(eng, stride, folds, x.detach().float().contiguous(), [w.detach() for w in ws])[2]
        return x


def _stem_frozen_forward(eng, fold, x, w):
    """conv7x7/2 on the folded BatchNorm with ReLU, then the max-pool with its record -> (y, idx, out)."""
    y = eng.conv2d_train_forward(x, w, *fold, 2, 3)
    out, idx = eng.maxpool_train_forward(y)
    return y, idx, out


class _Stem(torch.autograd.Function):
    """(x NHWC images, conv1's weight) -> the pooled stem output NHWC on a FROZEN BatchNorm (``fold`` = its scale / shift, which get no
    gradient).  Saves x, y and idx; the backward runs the pool backward and then ``specmi_conv2d_backward`` wanting g_w alone: the
    images get no gradient."""

    @staticmethod
    def forward(ctx, eng, fold, x, w):
        wd = w.detach()
        y, idx, out = _stem_frozen_forward(eng, fold, x, wd)
        ctx.eng, ctx.scale = eng, fold[0]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, y, idx, wd)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        if g_out is None or not ctx.needs_input_grad[3]:
            return None, None, None, None
        x, y, idx, w = ctx.saved_tensors
        g_y = ctx.eng.maxpool_backward(g_out, idx, y.shape[1], y.shape[2])
        return None, None, None, ctx.eng.conv2d_backward(x, w, ctx.scale, 2, 3, y, g_y, True, want=(False, True, False))[1]


class _StemBatch(torch.autograd.Function):
    """``_Stem`` on BATCH statistics: (x, conv1's weight, gamma, beta) -> the pooled output; ``step`` = ``_bn_step`` of bn1.  Saves x,
    z, y, mean, invstd and idx; the backward runs the pool backward, ``specmi_batchnorm_backward`` with the ReLU mask, then
    ``specmi_conv2d_backward`` on g_z with the identity scale."""

    @staticmethod
    def forward(ctx, eng, step, x, w, gamma, beta):
        wd, gd = w.detach(), gamma.detach()
        z, y, mean, invstd = _conv_bn(eng, x, wd, 2, 3, gd, beta.detach(), step)
        out, idx = eng.maxpool_train_forward(y)
        ctx.eng = eng
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, wd, gd, z, y, mean, invstd, idx)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        need_w, need_g, need_b = ctx.needs_input_grad[3:]
        if g_out is None or not (need_w or need_g or need_b):
            return (None,) * 6
        x, w, gamma, z, y, mean, invstd, idx = ctx.saved_tensors
        eng = ctx.eng
        g_y = eng.maxpool_backward(g_out, idx, y.shape[1], y.shape[2])
        g_z, g_gamma, g_beta, _ = eng.batchnorm_backward(z, gamma, mean, invstd, y, g_y, True, want=(need_w, need_g, need_b, False))
        g_w = None
        if need_w:
            g_w = eng.conv2d_backward(x, w, _identity_affine(eng, w.shape[0])[0], 2, 3, None, g_z, False, want=(False, True, False))[1]
        return None, None, None, g_w, g_gamma, g_beta


class ResNetStem(nn.Module):
    """The stem of a torchvision-layout ResNet, trainable: ``forward(images)`` takes (B, 3, H, W) NCHW fp32 images - as
    ``camcalib_eval.pad_batch`` makes them; the permute to NHWC is torch's - and runs conv7x7/2 -> BatchNorm -> ReLU ->
    MaxPool2d(3, 2, 1) as ONE ``torch.autograd.Function`` -> (B, oh, ow, 64) NHWC, what ``ResNetStage`` ('layer1') takes.  SHARES
    ``conv1`` and ``bn1`` with the backbone they come from.  ``bn`` as in ``ResNetStage``: 'frozen' folds bn1 into scale / shift
    whatever ``train()`` says; 'batch' with bn1 in ``train()`` normalises with the statistics of the batch, moves the running
    statistics and ``num_batches_tracked`` and trains gamma / beta.  The images get no gradient.  First derivatives only."""

    def __init__(self, conv1, bn1, bn='frozen'):
        super().__init__()
        if bn not in ('frozen', 'batch'):
            raise ValueError(f"bn = {bn!r}: 'frozen' and 'batch' are built")
        if tuple(conv1.kernel_size) != (7, 7) or tuple(conv1.stride) != (2, 2) or tuple(conv1.padding) != (3, 3) or conv1.bias is not None:
            raise NotImplementedError('the stem built is conv 7x7, stride 2, padding 3 without bias')
        self.conv1, self.bn1, self.bn = conv1, bn1, bn

    def conv_parameters(self):
        return [self.conv1.weight]

    def bn_parameters(self):
        return [self.bn1.weight, self.bn1.bias]

    def forward(self, images):
        dev = _device_of(images)
        if images.dim() != 4 or images.shape[1] != self.conv1.in_channels:
            raise ValueError(f'images must be (B, {self.conv1.in_channels}, H, W) NCHW, got {tuple(images.shape)}')
        eng = _engine(dev)
        x = images.detach().float().permute(0, 2, 3, 1).contiguous()
        w, bn1 = self.conv1.weight, self.bn1
        if self.bn == 'batch' and bn1.training:
            step = _bn_step(bn1)
            if torch.is_grad_enabled() and any(p.requires_grad for p in (w, bn1.weight, bn1.bias)):
                return _StemBatch.apply(eng, step, x, w, bn1.weight, bn1.bias)
            y = _conv_bn(eng, x, w.detach(), 2, 3, bn1.weight.detach(), bn1.bias.detach(), step)[1]
            return eng.maxpool_train_forward(y)[0]
        fold = _fold_bn(bn1)
        if torch.is_grad_enabled() and w.requires_grad:
            return _Stem.apply(eng, fold, x, w)
        return _stem_frozen_forward(eng, fold, x, w.detach())[2]


TRUNK_PARTS = ('stem', 'layer1', 'layer2', 'layer3', 'layer4')


class ResNetTrunk(nn.Module):
    """A Bottleneck trunk trainable from ``first`` upwards: ``forward(images)`` takes (B, 3, H, W) NCHW images and returns the NHWC
    feature map of layer4.  What lies below ``first`` runs frozen and under ``no_grad`` (``below``: images -> NHWC map, None with a
    trainable stem), then the trainable stem (``stem``, or None) and the ``ResNetStage``s in ``stages``."""

    def __init__(self, stem, stages, below=None):
        super().__init__()
        if (stem is None) == (below is None):
            raise ValueError('a trunk has a trainable stem or a frozen part below its first stage, not both and not neither')
        self.stem = stem
        self.stages = nn.ModuleList(stages)
        self._below = below

    @classmethod
    def from_model(cls, net, first='layer4', bn='frozen', cut_trunk=None):
        """The trunk of ``net`` (a ``spec_amd.modules.CameraRegressorNetwork`` or ``HMR`` on a Bottleneck ResNet) trainable from
        ``first`` ('stem', 'layer1' .. 'layer4') upwards, SHARING the backbone's modules and Parameters as ``ResNetStage.from_model``
        does.  Below ``first``: ``Engine.trunk(images, stages=k)`` of the committed network for 'layer2' and above; for 'layer1' the
        stem's own frozen path (``ResNetStem`` on the folded bn1) without gradients.  ``cut_trunk``: a callable (images, k) -> the NHWC
        map behind layer k that replaces ``Engine.trunk(images, stages=k)`` for 'layer2' and above, e.g. one that runs it in
        sub-batches (``camcalib_train.trunk_features``); the frozen stem below 'layer1' always takes the batch whole."""
        from .modules import ResNet50Params
        if first not in TRUNK_PARTS:
            raise ValueError(f'{first!r} is not a part of the trunk: {TRUNK_PARTS}')
        backbone = getattr(net, 'backbone', None)
        if not isinstance(backbone, ResNet50Params):
            raise NotImplementedError(f'ResNetTrunk is built for the Bottleneck trunks (ResNet-50 / 101 / 152), not for {type(backbone).__name__}')
        k = TRUNK_PARTS.index(first)
        stem = below = None
        if k == 0:
            stem = ResNetStem(backbone.conv1, backbone.bn1, bn)
        elif k == 1:
            frozen = ResNetStem(backbone.conv1, backbone.bn1, 'frozen')
            below = lambda images: frozen(images)
        else:
            cut = cut_trunk if cut_trunk is not None else (lambda images, n: net.engine(images.device).trunk(images, stages=n))
            below = lambda images: cut(images, k - 1)
        return cls(stem, [ResNetStage(getattr(backbone, n), bn) for n in TRUNK_PARTS[max(k, 1):]], below)

    def conv_parameters(self):
        """The conv weights of the trainable part, the stem's first: what an optimiser is given."""
        return (self.stem.conv_parameters() if self.stem is not None else []) + [p for st in self.stages for p in st.conv_parameters()]

    def bn_parameters(self):
        """gamma and beta of the trainable part's BatchNorms (given to the optimiser with ``bn='batch'``)."""
        return (self.stem.bn_parameters() if self.stem is not None else []) + [p for st in self.stages for p in st.bn_parameters()]

    def trained_modules(self):
        """The backbone modules of the trainable part: what ``bn='batch'`` puts in ``train()``."""
        return ([self.stem.bn1] if self.stem is not None else []) + [st.blocks for st in self.stages]

    def forward(self, images):
        if self.stem is not None:
            x = self.stem(images)
        else:
            with torch.no_grad():
                x = self._below(images)
        for st in self.stages:
            x = st(x)
        return x
