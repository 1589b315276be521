"""The forward value of the reference's two loss modules on the device (``spec/losses.py``: ``HMRLoss`` :26-141,
``HMRCamLoss`` :144-271) - the objective a checkpoint was trained under, as an evaluation quantity and, since the tail of the
training step has a backward, as something to descend: when grad is enabled and a tensor of ``pred`` requires grad, every entry
of ``loss_dict`` carries a ``grad_fn`` whose backward is ``specmi_hmr_loss_backward`` (first derivatives only; the ground truth
is a constant).  ``loss.backward()`` then reaches whatever produced ``pred`` - the heads of ``spec_amd.differentiable``, say.
With no tensor requiring grad nothing changes: the same launch, the same bits, no ``grad_fn``.  The trunk, the head's Linears,
optimisers, datasets and augmentation stay out of scope.

Everything numeric runs in ``specmi_hmr_loss`` (spec_amd/csrc/loss.hip; the quirks of the reference it restates are listed at
its declaration in include/specmi.h): one launch reduces every image, one folds the batch.

Stated deviations from the reference:

* ``pred['smpl_joints2d']`` is NOT overwritten in place (``HMRCamLoss`` normalises it in place at :191; here ``pred`` is only read).
* ``estimate_var=True`` raises ``NotImplementedError``: the reference's branch cannot run - ``smpl_losses_uncertainty`` (:390-397)
  is called with ``gt_pose_conf`` in the position of its ``criterion`` parameter (:79-87) - and the uncertainty criterion it names is an
  un-vendored pare class.
* a ``pred_segm_rgb`` key in ``pred`` raises ``NotImplementedError``: ``self.criterion_part`` (:131, :259) is never defined in
  the reference.
"""
from __future__ import annotations

import threading

import torch
import torch.nn as nn

from torch.autograd.function import once_differentiable

from . import _lib
from .cam_utils import _engine
from .engine import HMR_LOSS_INPUTS, HMR_LOSS_KEYS, HMR_LOSS_WEIGHTS

_PRED_KEYS = tuple(k for k, _ in HMR_LOSS_INPUTS['pred'])

_tls = threading.local()


@torch.no_grad()
def gt_vertices(pose, betas, body_model=None):
    """What ``SPECTrainer.training_step`` puts in ``gt['vertices']`` (spec/trainer.py:149-155,166): the vertices of
    ``self.smpl(betas=gt_betas, body_pose=gt_pose[:, 3:], global_orient=gt_pose[:, :3])`` for (B, 72) axis-angle poses, through
    ``specmi_smpl_native(pose_is_axis_angle=1)``.  ``body_model``: a ``spec_amd.metrics.BodyModel`` (default: one per thread
    and device on the assets of ``spec_amd.assets``)."""
    if body_model is None:
        from . import assets
        from .metrics import BodyModel
        dev = pose.device if isinstance(pose, torch.Tensor) and pose.device.type == 'cuda' else torch.device('cuda', torch.cuda.current_device())
        cache = getattr(_tls, 'bodies', None)
        if cache is None:
            cache = _tls.bodies = {}
        model = assets.smpl_model()
        if dev not in cache or cache[dev][0] is not model:      # the entry holds the asset dict it was built from: `is` cannot alias
            cache[dev] = (model, BodyModel(model, device=dev))
        body_model = cache[dev][1]
    return body_model.native(pose, betas, vertices=True, joints24=False)[0]


class _HmrLossFn(torch.autograd.Function):
    """means (7) = Engine.hmr_loss of the six prediction tensors; backward = Engine.hmr_loss_backward."""

    @staticmethod
    def forward(ctx, eng, mode, gt, weights, *pred_tensors):
        pred = {k: v.detach() if isinstance(v, torch.Tensor) else v for k, v in zip(_PRED_KEYS, pred_tensors)}
        res = eng.hmr_loss(mode, pred, gt, weights)
        ctx.eng, ctx.mode, ctx.gt, ctx.weights, ctx.pred, ctx.res = eng, mode, gt, weights, pred, res
        return res['means']

    @staticmethod
    @once_differentiable
    def backward(ctx, g_means):
        want = tuple(ctx.needs_input_grad[4:])
        g = ctx.eng.hmr_loss_backward(ctx.mode, ctx.pred, ctx.gt, ctx.weights, ctx.res, g_means, want)
        return (None, None, None, None) + tuple(None if g[k] is None else g[k].reshape(ctx.pred[k].shape) for k in _PRED_KEYS)


class _LossBase(nn.Module):
    _mode = None

    def _set_weights(self, kw):
        for name in HMR_LOSS_WEIGHTS:
            setattr(self, name, kw[name])

    def forward(self, pred, gt):
        """-> (loss, loss_dict): the seven keys of the reference in its order, 0-dim device tensors; ``loss`` is
        ``loss_dict['loss/total_loss']``.  ``gt['vertices']`` is used when present (``gt_vertices`` makes it) and may be
        missing while ``shape_loss_weight`` is 0.  Differentiable in the six tensors of ``pred`` (module docstring)."""
        if 'pred_segm_rgb' in pred:
            raise NotImplementedError("'pred_segm_rgb': the part-segmentation term calls self.criterion_part, which the reference never "
                                      'defines (spec/losses.py:131,259)')
        v = pred['smpl_vertices']
        if not isinstance(v, torch.Tensor) or v.device.type != 'cuda':
            raise RuntimeError('spec_amd.losses needs device tensors (no CPU path)')
        weights = [getattr(self, n) for n in HMR_LOSS_WEIGHTS]
        if torch.is_grad_enabled() and any(isinstance(pred[k], torch.Tensor) and pred[k].requires_grad for k in _PRED_KEYS):
            means = _HmrLossFn.apply(_engine(v.device), self._mode, gt, weights, *(pred[k] for k in _PRED_KEYS))
        else:
            with torch.no_grad():
                means = _engine(v.device).hmr_loss(self._mode, pred, gt, weights)['means']
        loss_dict = dict(zip(HMR_LOSS_KEYS, means.unbind(0)))
        return loss_dict['loss/total_loss'], loss_dict


class HMRLoss(_LossBase):
    """spec/losses.py:26-141; ``gt['keypoints']`` is the crop-normalised annotation."""
    _mode = _lib.HMR_LOSS

    def __init__(
            self,
            shape_loss_weight=0,
            keypoint_loss_weight=5.,
            pose_loss_weight=1.,
            smpl_part_loss_weight=1.,
            beta_loss_weight=0.001,
            openpose_train_weight=0.,
            gt_train_weight=1.,
            loss_weight=60.,
            estimate_var=False,
            uncertainty_loss='MultivariateGaussianNegativeLogLikelihood',
    ):
        super().__init__()
        if estimate_var:
            raise NotImplementedError(
                'estimate_var=True: the branch cannot run in the reference - smpl_losses_uncertainty receives gt_pose_conf in its '
                f'criterion slot (spec/losses.py:79-87,390-397) - and its criterion {uncertainty_loss!r} is an un-vendored pare class')
        self.estimate_var = estimate_var
        self._set_weights(locals())


class HMRCamLoss(_LossBase):
    """spec/losses.py:144-271; reads ``gt['keypoints_orig']`` (pixels), ``gt['orig_shape']`` (H, W) and ``gt['scale']``."""
    _mode = _lib.HMR_CAM_LOSS

    def __init__(
            self,
            shape_loss_weight=0,
            keypoint_loss_weight=5.,
            pose_loss_weight=1.,
            smpl_part_loss_weight=1.,
            beta_loss_weight=0.001,
            openpose_train_weight=0.,
            gt_train_weight=1.,
            loss_weight=60.,
    ):
        super().__init__()
        self._set_weights(locals())


# ---- CamCalib: CameraRegressorLoss (camcalib/loss.py:24-125) --------------------------------------------------------------------
CAMCALIB_LOSS_KEYS = ('loss', 'vfov_loss', 'pitch_loss', 'roll_loss')


class _CamLossFn(torch.autograd.Function):
    """means (4) = Engine.camcalib_loss of the three logit tensors; backward = Engine.camcalib_loss_backward."""

    @staticmethod
    def forward(ctx, eng, loss_type, targets, weights, pv, pp, pr):
        preds = [t.detach() for t in (pv, pp, pr)]
        ctx.eng, ctx.loss_type, ctx.targets, ctx.weights, ctx.preds = eng, loss_type, targets, weights, preds
        return eng.camcalib_loss(preds, targets, loss_type, weights)['means']

    @staticmethod
    @once_differentiable
    def backward(ctx, g_means):
        g = ctx.eng.camcalib_loss_backward(ctx.preds, ctx.targets, ctx.loss_type, ctx.weights, g_means)
        return (None, None, None, None) + tuple(gi.reshape(p.shape) if need else None for gi, p, need in zip(g, ctx.preds, ctx.needs_input_grad[4:]))


def _camcalib_means(preds, targets, loss_type, weights):
    """The four means of CameraRegressorLoss on device logits; a graph only when grad is enabled and a pred requires grad."""
    if loss_type not in _lib.LOSS_TYPES:
        raise ValueError(f'{loss_type} is not defined..')
    preds = [p.squeeze(-1) if isinstance(p, torch.Tensor) else p for p in preds]
    v = preds[0]
    if not isinstance(v, torch.Tensor) or v.device.type != 'cuda':
        raise RuntimeError('spec_amd.losses needs device tensors (no CPU path)')
    if torch.is_grad_enabled() and any(p.requires_grad for p in preds):
        return _CamLossFn.apply(_engine(v.device), loss_type, tuple(targets), tuple(weights), *preds)
    with torch.no_grad():
        return _engine(v.device).camcalib_loss(preds, targets, loss_type, weights)['means']


class CameraRegressorLoss(nn.Module):
    """camcalib/loss.py:62-125: ``forward(pred_vfov, pred_pitch, pred_roll, gt_vfov, gt_pitch, gt_roll)`` -> (loss, loss_dict) with
    the keys ``loss``, ``vfov_loss``, ``pitch_loss``, ``roll_loss`` (0-dim device tensors).  The targets are integer bin indices
    (any integer dtype) for 'ce' / 'kl', fp32 soft indices in [-1, 1] for the soft-argmax losses.  When grad is enabled and a pred
    requires grad every entry carries a ``grad_fn`` whose backward is ``specmi_camcalib_loss_backward`` (first derivatives only);
    otherwise the values are ``Engine.camcalib_eval(...)['means'][:4]`` bit for bit, without a graph."""

    def __init__(self, vfov_loss_weight=1.0, pitch_loss_weight=1.0, roll_loss_weight=1.0, loss_type='kl'):
        super().__init__()
        if loss_type not in _lib.LOSS_TYPES:
            raise ValueError(f'{loss_type} is not defined..')
        self.loss_type = loss_type
        self.vfov_loss_weight = vfov_loss_weight
        self.pitch_loss_weight = pitch_loss_weight
        self.roll_loss_weight = roll_loss_weight

    def forward(self, pred_vfov, pred_pitch, pred_roll, gt_vfov, gt_pitch, gt_roll):
        means = _camcalib_means((pred_vfov, pred_pitch, pred_roll), (gt_vfov, gt_pitch, gt_roll), self.loss_type,
                                (self.vfov_loss_weight, self.pitch_loss_weight, self.roll_loss_weight))
        loss_dict = dict(zip(CAMCALIB_LOSS_KEYS, means.unbind(0)))
        return loss_dict['loss'], loss_dict


class _OneHead(nn.Module):
    """A leaf criterion of camcalib/loss.py on ONE head: the row arithmetic of the vfov head (the only one 'biased_l2' differs
    on), weight 1, the other two heads fed the same logits."""
    _loss_type = None

    def forward(self, pred, target):
        return _camcalib_means((pred, pred.detach(), pred.detach()), (target, target, target), self._loss_type, (1.0, 1.0, 1.0))[1]


class KLDivergence(_OneHead):
    """camcalib/loss.py:24-30: ``F.kl_div(log_softmax(pred), one_hot(target), 'batchmean')`` of (N, nbins) logits."""
    _loss_type = 'kl'


class SoftargmaxClsLoss(_OneHead):
    """camcalib/loss.py:33-59: pred (N, nbins), target (N,) in [-1, 1]; ``criterion`` 'l2' or 'biased_l2'."""

    def __init__(self, criterion='l2'):
        super().__init__()
        if criterion not in ('l2', 'biased_l2'):
            raise ValueError(f'{criterion} is not defined!')
        self.criterion = criterion
        self._loss_type = 'softargmax_l2' if criterion == 'l2' else 'softargmax_biased_l2'
