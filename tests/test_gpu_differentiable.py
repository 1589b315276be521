"""The whole differentiable tail on the device at (V, B) = (257, 3): head state -> ``spec_amd.differentiable`` (rot6d_to_rotmat,
SMPLCamHead) -> ``spec_amd.losses.HMRCamLoss`` -> ``loss.backward()``, against the float64 composition of the two restatements
(tests/tail_grad_ref.py)."""
import numpy as np
import pytest
import torch

from tests import smpl_grad_ref as S
from tests import tail_grad_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items() if v is not None}


def _loss(head, crit, state, camera, gt):
    from spec_amd import differentiable as D
    rot = D.rot6d_to_rotmat(state['x6d']).view(-1, 24, 3, 3)
    out = head(rot, state['betas'], state['cam'], *[camera[k] for k in S.CAM_KEYS])
    return crit(dict(out, pred_pose=rot, pred_shape=state['betas'], pred_cam=state['cam']), gt)[0]


def test_gradient_of_the_state_vs_float64():
    from spec_amd import differentiable as D
    from spec_amd.losses import HMRCamLoss
    state, camera, gt = T.problem()
    _, g64 = T.grad64({k: v.astype(np.float64) for k, v in state.items()}, camera, gt, T.WEIGHTS)
    head, crit = D.SMPLCamHead(S.IMG_RES, model=S.model(T.NV)), HMRCamLoss(**T.WEIGHTS)
    with torch.enable_grad():
        leaves = {k: v.requires_grad_(True) for k, v in _dev(state).items()}
        loss = _loss(head, crit, leaves, _dev(camera), _dev(gt))
        loss.backward()
    for k in T.STATE:
        e = S.err(leaves[k].grad.cpu().numpy(), g64[k])
        print(f'd total / d {k}: {e:.3g}')
        assert e < 1e-5, (k, e)
    # with no leaf the heads return exactly what Engine.smpl returns: no graph, the same bits
    with torch.enable_grad():
        d = _dev(state)
        rot = D.rot6d_to_rotmat(d['x6d']).view(-1, 24, 3, 3)
        out = head(rot, d['betas'], d['cam'], *[_dev(camera)[k] for k in S.CAM_KEYS])
    eng = D._smpl_engine(DEV, S.model(T.NV), True, S.IMG_RES, S.FOCAL)
    plain = eng.smpl(rot, d['betas'], d['cam'], *[_dev(camera)[k] for k in S.CAM_KEYS])
    assert all(out[k].grad_fn is None and torch.equal(out[k], plain[k]) for k in plain)


def test_weak_perspective_head_backward():
    from spec_amd import differentiable as D
    inp, ups, g64 = S.case(257, 3, 1)
    head = D.SMPLHead(S.FOCAL, S.IMG_RES, model=S.model(257))
    with torch.enable_grad():
        leaves = [torch.from_numpy(inp[k]).to(DEV).requires_grad_(True) for k in S.IN_KEYS]
        out = head(*leaves, normalize_joints2d=True)
        sum((out[k] * torch.from_numpy(g).to(DEV)).sum() for k, g in ups.items()).backward()
    for k, leaf in zip(S.IN_KEYS, leaves):
        assert S.err(leaf.grad.cpu().numpy(), g64[k]) < 1e-5, k


def test_six_steps_of_gradient_descent_lower_the_loss():
    from spec_amd import differentiable as D
    from spec_amd.losses import HMRCamLoss
    start, camera, gt = T.descent_problem()
    head, crit = D.SMPLCamHead(S.IMG_RES, model=S.model(T.NV)), HMRCamLoss(**T.DESCENT_WEIGHTS)
    cam_d, gt_d = _dev(camera), _dev(gt)
    state = _dev(start)
    losses = []
    for _ in range(T.DESCENT_STEPS):
        with torch.enable_grad():
            leaves = {k: v.detach().requires_grad_(True) for k, v in state.items()}
            loss = _loss(head, crit, leaves, cam_d, gt_d)
            loss.backward()
        losses.append(float(loss.detach()))
        state = {k: (leaves[k].detach() - T.DESCENT_LR * leaves[k].grad) for k in T.STATE}
    with torch.no_grad():
        losses.append(float(_loss(head, crit, state, cam_d, gt_d)))
    print(['%.6g' % v for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
