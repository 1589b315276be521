"""The trainable ResNet stage as a user meets it: the trunk cut after a stage (``Engine.trunk(images, stages=n)``),
``spec_amd.differentiable.ResNetStage`` against the float64 stage of tests/conv_grad_ref.py, ``from_model`` on committed networks
with an optimiser of torch's, and ``camcalib_train.finetune_heads(..., unfreeze=('layer4',))`` on the stand-in tree."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import conv_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Tests that ran earlier in the process may have switched autograd off for good (the scripts do)."""
    with torch.enable_grad():
        yield


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _camcalib_net():
    from spec_amd import synth
    from spec_amd.modules import CameraRegressorNetwork
    sd = synth.camcalib_state(2201)
    net = CameraRegressorNetwork()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    return net.to(DEV).eval(), _t(synth.images(86, 2, 64, 64))


def _stage_module(case, dtype=torch.float32):
    """The blocks of a stage case as the trunk's own parameter containers: BatchNorm with gamma = scale, beta = shift, running mean 0
    and running variance 1 - eps, so that the frozen fold gives back scale and shift (to an ulp)."""
    from spec_amd.modules import _BottleneckParams
    blocks = []
    for b in case['blocks']:
        planes, inplanes = b['c1']['w'].shape[:2]
        m = _BottleneckParams(inplanes, planes, b['stride'], 'ds' in b)
        pairs = [(m.conv1, m.bn1, 'c1'), (m.conv2, m.bn2, 'c2'), (m.conv3, m.bn3, 'c3')] + ([(m.downsample[0], m.downsample[1], 'ds')] if 'ds' in b else [])
        with torch.no_grad():
            for conv, bn, c in pairs:
                conv.weight.copy_(b[c]['w'])
                bn.weight.copy_(b[c]['scale']); bn.bias.copy_(b[c]['shift'])
                bn.running_mean.zero_(); bn.running_var.fill_(1.0 - bn.eps)
        blocks.append(m)
    return nn.Sequential(*blocks).to(dtype)


def test_the_cut_trunk_has_the_whole_trunks_bits_and_the_stage_continues_it():
    from spec_amd.differentiable import ResNetStage
    net, x = _camcalib_net()
    eng = net.engine(DEV)
    whole = eng.trunk(x)
    assert torch.equal(eng.trunk(x, stages=4), whole)
    shapes = [tuple(eng.trunk(x, stages=n).shape) for n in (1, 2, 3)]
    assert shapes == [(2, 16, 16, 256), (2, 8, 8, 512), (2, 4, 4, 1024)], shapes
    with torch.no_grad():
        mine = ResNetStage.from_model(net, 'layer4')(eng.trunk(x, stages=3))
    assert mine.shape == whole.shape and mine.grad_fn is None
    e = R.err(mine.mean(dim=(1, 2)), whole.mean(dim=(1, 2)))
    print(f'pooled feature, stages=3 -> ResNetStage vs Engine.trunk: {e:.3g}')
    assert e < BOUND
    # layer3 on top of stages=2 gives the stages=3 map
    with torch.no_grad():
        l3 = ResNetStage.from_model(net, 'layer3')(eng.trunk(x, stages=2))
    assert R.err(l3, eng.trunk(x, stages=3)) < BOUND
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError):
            eng.trunk(x, stages=bad)


def test_stage_vs_float64():
    """Bound per tensor: 4 times the error torch's own fp32 CPU autograd makes on the same case against the float64 reference - the
    margin two correct fp32 chains with different summation orders get over each other - with a floor of 1e-5.  Measured on an
    MI355X: the figures are in DESIGN.md section 7, f-22."""
    from spec_amd.differentiable import ResNetStage
    case = R.stage_case()
    ref = R.bottleneck_stage(case['x'], case['blocks'], case['g_out'])
    names = ['out', 'g_x'] + [f'g_w[{i}]' for i in range(10)]
    want = [ref['out'], ref['g_x']] + ref['g_w']

    def run(stage, x, g_out, ws):
        out = stage(x)
        out.backward(g_out)
        return [out.detach(), x.grad] + [w.grad for w in ws]
    # torch's fp32 chain on the CPU: the same containers through F.conv2d and F.batch_norm in eval mode
    cpu = _stage_module(case)

    def torch_stage(x):
        v = x.permute(0, 3, 1, 2)
        for m in cpu:
            bn = lambda t, b: F.batch_norm(t, b.running_mean, b.running_var, b.weight.detach(), b.bias.detach(), False, 0.0, b.eps)
            y = torch.relu(bn(m.conv1(v), m.bn1))
            y = torch.relu(bn(m.conv2(y), m.bn2))
            idn = bn(m.downsample[0](v), m.downsample[1]) if hasattr(m, 'downsample') else v
            v = torch.relu(bn(m.conv3(y), m.bn3) + idn)
        return v.permute(0, 2, 3, 1)
    cpu_ws = ResNetStage(cpu).conv_parameters()
    theirs = run(torch_stage, case['x'].float().requires_grad_(True), case['g_out'].float(), cpu_ws)
    dev = _stage_module(case).to(DEV)
    stage = ResNetStage(dev)
    ws = stage.conv_parameters()
    assert len(ws) == 10
    mine = run(stage, case['x'].float().to(DEV).requires_grad_(True), case['g_out'].float().to(DEV), ws)
    worst = 0.0
    for n, a, b, w in zip(names, mine, theirs, want):
        e_dev, e_torch = R.err(a, w), R.err(b, w)
        print(f'{n}: device {e_dev:.3g}, torch fp32 CPU {e_torch:.3g}')
        assert a.shape == w.shape
        assert e_dev < max(4 * e_torch, BOUND), (n, e_dev, e_torch)
        worst = max(worst, e_dev)
    print(f'worst device error {worst:.3g}')
    for m in dev:                                                        # BatchNorm is frozen: no gradient, nothing updated
        for bn in [m.bn1, m.bn2, m.bn3] + ([m.downsample[1]] if hasattr(m, 'downsample') else []):
            assert bn.weight.grad is None and bn.bias.grad is None and not bn.running_mean.any() and int(bn.num_batches_tracked) == 0


def test_from_model_shares_the_parameters_and_the_network_commits_them_again():
    from spec_amd.differentiable import CameraRegressorHead, ResNetStage
    from spec_amd.losses import CameraRegressorLoss
    net, x = _camcalib_net()
    eng = net.engine(DEV)
    before = torch.stack(net(x)).clone()
    bn_before = {k: v.clone() for k, v in net.state_dict().items() if '.bn' in k or 'downsample.1' in k}
    feat3 = eng.trunk(x, stages=3)
    stage, head = ResNetStage.from_model(net, 'layer4'), CameraRegressorHead.from_model(net)
    mine, theirs = dict(stage.blocks.named_parameters()), dict(net.backbone.layer4.named_parameters())
    assert stage.blocks is net.backbone.layer4 and all(mine[k] is theirs[k] for k in theirs)
    ws = stage.conv_parameters()
    assert len(ws) == 10 and all(any(w is p for p in net.parameters()) for w in ws)
    crit = CameraRegressorLoss(loss_type='softargmax_l2')
    targets = [torch.tensor([0.3, -0.4], device=DEV), torch.tensor([-0.2, 0.1], device=DEV), torch.tensor([0.0, 0.6], device=DEV)]
    opt = torch.optim.SGD(ws, lr=1e-2)
    opt.zero_grad()
    crit(*head(stage(feat3), channels_last=True), *targets)[0].backward()
    assert all(w.grad is not None and torch.isfinite(w.grad).all() and w.grad.any() for w in ws)
    opt.step()
    with torch.no_grad():
        ref = torch.stack(head(stage(feat3), channels_last=True))
    after = torch.stack(net(x))                                      # the bumped versions are seen: the network commits by itself
    assert torch.equal(eng.trunk(x, stages=3), feat3)                # layers 1-3 are where they were
    top = float(ref.abs().max())
    agree, moved = float((after - ref).abs().max()) / top, float((after - before).abs().max()) / top
    print(f'after the step: network vs stage + head {agree:.3g}, network after vs before {moved:.3g}')
    assert agree < 1e-5 and moved > 100 * agree, (agree, moved)
    sd = net.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in bn_before.items())
    for m in net.backbone.layer4:
        for bn in (m.bn1, m.bn2, m.bn3):
            assert bn.weight.grad is None and bn.bias.grad is None


def test_six_sgd_steps_on_stage_and_head_lower_the_loss_every_time():
    from spec_amd.differentiable import CameraRegressorHead, ResNetStage
    from spec_amd.losses import CameraRegressorLoss
    p = R.sgd_problem()
    stage = ResNetStage(_stage_module(p['stage']).to(DEV))
    head = CameraRegressorHead(128, 1, 1024, R.SGD_NBINS)
    head.load_state_dict({k: v.float() for k, v in p['head'].items()})
    head = head.to(DEV)
    crit = CameraRegressorLoss(1.0, 1.0, 1.0, 'ce')
    x, tg = p['stage']['x'].float().to(DEV), [t.to(DEV) for t in p['targets']]
    opt = torch.optim.SGD(stage.conv_parameters() + list(head.parameters()), lr=R.SGD_RATE)
    losses = []
    for _ in range(R.SGD_STEPS):
        opt.zero_grad()
        loss, _ = crit(*head(stage(x), channels_last=True), *tg)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(crit(*head(stage(x), channels_last=True), *tg)[0]))
    want = R.sgd_losses64()
    print(' '.join(f'{v:.6f}' for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert max(abs(a - b) for a, b in zip(losses, want)) < 1e-4 * want[0]       # the float64 chain's path, step by step


def test_finetune_with_layer4_unfrozen_on_the_standin_tree(tmp_path):
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    ce.write_standin_tree(str(tmp_path), n_images=4, backbone='resnet50')
    hp = ct.load_config(str(tmp_path / ce.STANDIN_CFG))
    start = torch.load(str(tmp_path / ce.STANDIN_CKPT), map_location='cpu')['state_dict']
    start = {k: v.reshape(()) if k.endswith('num_batches_tracked') else v for k, v in start.items()}      # (1,) in the synthetic file, () in a module
    lines = []
    res = ct.finetune_heads(hp, data_root=str(tmp_path), epochs=1, seed=3, log=lines.append, unfreeze=('layer4',))
    assert set(res['epochs'][0]) == set(ct.TRAIN_KEYS) and np.isfinite(res['epochs'][0]['train/loss'])
    assert set(res['before']) == set(res['after']) == {'val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc'} and res['before'] != res['after']
    end = torch.load(res['ckpt'], map_location='cpu')['state_dict']
    assert set(end) == set(start)
    conv4 = [k for k in start if 'backbone.layer4' in k and (k.endswith('.weight') and start[k].dim() == 4)]
    assert len(conv4) == 10 and all(not torch.equal(start[k], end[k]) for k in conv4)
    heads = [k for k in start if '.fc_' in k]
    assert len(heads) == 6 and all(not torch.equal(start[k], end[k]) for k in heads)
    assert all(torch.equal(start[k], end[k]) for k in start if k not in conv4 and k not in heads)      # layers 1-3, every BatchNorm tensor
    again = ce.build_model(hp, res['ckpt'], str(tmp_path), DEV)         # the after-evaluation ran on the recommitted model
    _, x = _camcalib_net()
    assert all(torch.equal(a, b) for a, b in zip(res['model'](x), again(x)))
    with pytest.raises(NotImplementedError):
        ct.finetune_heads(hp, data_root=str(tmp_path), epochs=1, unfreeze=('layer3',), evaluate=False)


def test_unfreeze_nothing_is_the_head_only_flow_bit_for_bit(tmp_path):
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    ce.write_standin_tree(str(tmp_path), n_images=4)
    hp = ct.load_config(str(tmp_path / ce.STANDIN_CFG))
    kw = dict(data_root=str(tmp_path), epochs=1, seed=3, log=lambda s: None, evaluate=False)
    a = ct.finetune_heads(hp, out=str(tmp_path / 'a.ckpt'), **kw)
    b = ct.finetune_heads(hp, out=str(tmp_path / 'b.ckpt'), unfreeze=(), **kw)
    sa, sb = (torch.load(r['ckpt'], map_location='cpu')['state_dict'] for r in (a, b))
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa) and a['epochs'] == b['epochs']
    with pytest.raises(NotImplementedError):                            # the stand-in tree's default trunk is a BasicBlock ResNet-34
        ct.finetune_heads(hp, unfreeze=('layer4',), **kw)


def test_hmr_layer4_gets_gradients_through_the_head_and_the_loss():
    from spec_amd import assets, synth
    from spec_amd import differentiable as D
    from spec_amd.losses import HMRLoss
    from spec_amd.modules import HMR
    from tests import smpl_grad_ref as S
    from tests import tail_grad_ref as T
    assets.use_synthetic_assets(1003)
    sd = synth.hmr_state(2202, False)
    hmr = HMR()
    hmr.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    hmr = hmr.to(DEV).eval()
    x = _t(synth.images(87, T.B, 64, 64))
    _, _, gt = T.problem()
    gt = {k: _t(v) for k, v in gt.items()}
    stage, head = D.ResNetStage.from_model(hmr, 'layer4'), D.HMRHead.from_hmr(hmr)
    smpl_head = D.SMPLHead(S.FOCAL, S.IMG_RES, model=S.model(T.NV))
    head.eval()
    pred = head(stage(hmr.engine(DEV).trunk(x, stages=3)), channels_last=True)
    out = smpl_head(pred['pred_pose'], pred['pred_shape'], pred['pred_cam'])
    HMRLoss()(dict(out, **pred), gt)[0].backward()
    ws = stage.conv_parameters()
    assert len(ws) == 10
    for w in ws:
        assert w.grad is not None and w.grad.shape == w.shape and torch.isfinite(w.grad).all() and w.grad.any()


def test_trunks_without_bottlenecks_are_refused():
    from spec_amd.differentiable import ResNetStage
    from spec_amd.modules import HMR, CameraRegressorNetwork
    with pytest.raises(NotImplementedError):
        ResNetStage.from_model(CameraRegressorNetwork(backbone='resnet34'), 'layer4')
    with pytest.raises(NotImplementedError):
        ResNetStage.from_model(HMR(backbone='hrnet_w32-conv'), 'layer4')
    with pytest.raises(ValueError):
        ResNetStage.from_model(CameraRegressorNetwork(), 'layer5')
