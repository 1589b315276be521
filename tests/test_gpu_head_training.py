"""``spec_amd.differentiable.HMRHead`` in a training step on the device at B = 3, F = 40, use_cam_feats, V = 257: features ->
HMRHead -> SMPLCamHead -> HMRCamLoss -> ``loss.backward()`` against the float64 chain of tests/head_grad_ref.py (bound 1e-5, as
tests/test_gpu_differentiable.py), the modes, the mask draw, six steps of descent, and ``HMRHead.from_hmr`` with an optimiser."""
import numpy as np
import pytest
import torch

from tests import head_grad_ref as R
from tests import smpl_grad_ref as S
from tests import tail_grad_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items() if v is not None}


def _head(params):
    from spec_amd import differentiable as D
    ms = R.mean_state(1)[0]
    head = D.HMRHead(R.TRAIN_F, True, mean_params={'pose': ms[:144], 'shape': ms[144:154], 'cam': ms[154:]})
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    assert not unexpected and set(missing) == {'init_pose', 'init_shape', 'init_cam'}
    return head.to(DEV)


def _loss(head, smpl_head, crit, features, camera, gt, **kw):
    """camera, gt: device dicts; -> (loss, the head's output dict)."""
    vfov = 2.0 * torch.atan(camera['img_h'] / (2.0 * camera['cam_intrinsics'][:, 0, 0]))
    pred = head(features, cam_rotmat=camera['cam_rotmat'], cam_vfov=vfov, **kw)
    out = smpl_head(pred['pred_pose'], pred['pred_shape'], pred['pred_cam'], *[camera[k] for k in S.CAM_KEYS])
    return crit(dict(out, **pred), gt)[0], pred


def _setup(descent=False, weights=T.WEIGHTS):
    from spec_amd import differentiable as D
    from spec_amd.losses import HMRCamLoss
    params, features, masks, camera, gt = R.train_problem(descent)
    return (params, features, masks, camera, gt, _head(params), D.SMPLCamHead(S.IMG_RES, model=S.model(T.NV)), HMRCamLoss(**weights),
            _dev(camera), _dev(gt))


def test_gradients_of_the_chain_vs_float64():
    params, features, masks, camera, gt, head, smpl_head, crit, cam_d, gt_d = _setup()
    loss64, g_feat64, g64 = R.chain64(params, features, masks, camera, gt, T.WEIGHTS)
    head.train()
    with torch.enable_grad():
        x = torch.from_numpy(features).to(DEV).requires_grad_(True)
        loss, pred = _loss(head, smpl_head, crit, x, cam_d, gt_d, dropout_masks=torch.from_numpy(masks).to(DEV))
        assert pred['pred_pose'].shape == (T.B, 24, 3, 3) and pred['pred_pose_6d'].shape == (T.B, 144)
        assert pred['pred_shape'].shape == (T.B, 10) and pred['pred_cam'].shape == (T.B, 3)
        loss.backward()
    print(f'loss {float(loss.detach()):.8g} (float64 {loss64:.8g})')
    assert abs(float(loss.detach()) - loss64) < 1e-5 * abs(loss64)
    got = dict(head.named_parameters())
    e = {'features': S.err(x.grad.cpu().numpy(), g_feat64), **{n: S.err(got[n].grad.cpu().numpy(), g64[n]) for n in R.NAMES}}
    print({k: f'{v:.3g}' for k, v in e.items()})
    assert max(e.values()) < 1e-5, e


def test_eval_without_grad_keeps_no_graph_and_equals_the_c_call():
    from spec_amd.cam_utils import _engine
    params, features, _, camera, _, head, _, _, cam_d, _ = _setup()
    head.eval()
    x = torch.from_numpy(features).to(DEV)
    vfov = 2.0 * torch.atan(cam_d['img_h'] / (2.0 * cam_d['cam_intrinsics'][:, 0, 0]))
    with torch.no_grad():
        pred = head(x, cam_rotmat=cam_d['cam_rotmat'], cam_vfov=vfov)
    assert all(v.grad_fn is None and not v.requires_grad for v in pred.values())
    cam_feats = torch.cat([cam_d['cam_rotmat'][:, :, :2].reshape(T.B, 6), vfov[:, None]], 1)
    state, _ = _engine(DEV).hmr_head_train_forward(dict(head.named_parameters()), x.mean(dim=(2, 3)), torch.from_numpy(R.mean_state(T.B)).to(DEV),
                                                   cam_feats, None)
    assert torch.equal(pred['pred_pose_6d'], state[:, :144]) and torch.equal(pred['pred_shape'], state[:, 144:154])
    assert torch.equal(pred['pred_cam'], state[:, 154:])
    # a frozen head on features that need no gradient: no graph either, with grad enabled
    for q in head.parameters():
        q.requires_grad_(False)
    with torch.enable_grad():
        assert head(x, cam_rotmat=cam_d['cam_rotmat'], cam_vfov=vfov)['pred_cam'].grad_fn is None


def test_masks_are_drawn_from_the_module_generator():
    _, features, _, _, _, head, smpl_head, crit, cam_d, gt_d = _setup()
    head.train()
    head.generator = torch.Generator(device=DEV)
    x = torch.from_numpy(features).to(DEV)
    losses = []
    for seed in (5, 5, 6):
        head.generator.manual_seed(seed)
        with torch.no_grad():
            losses.append(_loss(head, smpl_head, crit, x, cam_d, gt_d)[0])
    assert torch.equal(losses[0], losses[1]) and not torch.equal(losses[0], losses[2]), losses
    head.eval()
    with torch.no_grad():
        assert not torch.equal(_loss(head, smpl_head, crit, x, cam_d, gt_d)[0], losses[0])


def test_six_steps_of_gradient_descent_on_the_parameters_lower_the_loss():
    _, features, _, _, _, head, smpl_head, crit, cam_d, gt_d = _setup(True, T.DESCENT_WEIGHTS)
    head.eval()                                                     # eval-mode dropout: the float64 chain the rate was chosen on
    x = torch.from_numpy(features).to(DEV)
    opt = torch.optim.SGD(head.parameters(), lr=R.DESCENT_LR)
    losses = []
    for _ in range(R.DESCENT_STEPS):
        opt.zero_grad()
        with torch.enable_grad():
            loss, _ = _loss(head, smpl_head, crit, x, cam_d, gt_d)
            loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    with torch.no_grad():
        losses.append(float(_loss(head, smpl_head, crit, x, cam_d, gt_d)[0]))
    print(['%.6g' % v for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


def test_from_hmr_shares_the_parameters_and_the_model_commits_them_again():
    from oracle.models import cam_params
    from spec_amd import assets, synth
    from spec_amd import differentiable as D
    from spec_amd.modules import HMR
    assets.use_synthetic_assets(1003)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    sd = synth.hmr_state(1702, True, backbone='resnet18')
    hmr = HMR(backbone='resnet18', use_cam=True, use_cam_feats=True)
    hmr.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
    hmr = hmr.to(DEV).eval()
    B = 2
    x = t(synth.images(83, B, 64, 64)).to(DEV)
    sc, ce, iw, ih = [t(a) for a in synth.bbox_inputs(83, B, 640., 480.)]
    g = torch.Generator().manual_seed(7)
    Rc, K = cam_params(0.3 * torch.randn(B, generator=g), 0.2 * torch.randn(B, generator=g), (400 + 200 * torch.rand(B, generator=g)).numpy(), iw, ih)
    cam = dict(cam_rotmat=Rc.to(DEV), cam_intrinsics=K.to(DEV), bbox_scale=sc.to(DEV), bbox_center=ce.to(DEV), img_w=iw.to(DEV), img_h=ih.to(DEV))
    before = hmr(x, **cam)['pred_pose_6d'].clone()
    feat = hmr.engine(DEV).trunk(x)                                  # (B, 2, 2, 512), frozen
    head = D.HMRHead.from_hmr(hmr)
    assert head.use_cam_feats and head.num_input_features == 512
    assert all(a is b for a, b in zip(head.parameters(), hmr.head.parameters())) and head.init_pose is hmr.head.init_pose
    vfov = 2.0 * torch.atan(cam['img_h'] / (2.0 * cam['cam_intrinsics'][:, 0, 0]))
    opt = torch.optim.Adam(head.parameters(), lr=1e-4)
    head.train()
    head.generator = torch.Generator(device=DEV).manual_seed(11)
    for _ in range(2):
        opt.zero_grad()
        with torch.enable_grad():
            pred = head(feat, cam_rotmat=cam['cam_rotmat'], cam_vfov=vfov, channels_last=True)
            (pred['pred_pose_6d'].square().sum() + pred['pred_shape'].square().sum() + pred['pred_cam'].square().sum()).backward()
        opt.step()
    head.eval()
    with torch.no_grad():
        ref = head(feat, cam_rotmat=cam['cam_rotmat'], cam_vfov=vfov, channels_last=True)['pred_pose_6d']
    after = hmr(x, **cam)['pred_pose_6d']                            # the bumped versions are seen: the model commits by itself
    top = float(ref.abs().max())
    agree, moved = float((after - ref).abs().max()) / top, float((after - before).abs().max()) / top
    print(f'after the steps: model vs differentiable head {agree:.3g}, model after vs before {moved:.3g}')
    assert agree < 1e-5 and moved > 100 * agree and moved > 1e-3, (agree, moved)
