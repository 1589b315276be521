"""The trainable trunk as a user meets it: ``spec_amd.differentiable.ResNetStem`` / ``ResNetTrunk`` against the float64 chains of
tests/trunk_grad_ref.py, against the inference trunk of a committed network, and ``camcalib_train.finetune_heads`` with the longer
suffixes of the trunk unfrozen on the stand-in tree."""
import numpy as np
import pytest
import torch

from tests import conv_grad_ref as R
from tests import trunk_grad_ref as T
from tests.test_gpu_trunk_finetune import BOUND, DEV, _camcalib_net, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Tests that ran earlier in the process may have switched autograd off for good (the scripts do)."""
    with torch.enable_grad():
        yield


def _trunk(case, bn, device, dtype=torch.float32):
    from spec_amd.differentiable import ResNetStage, ResNetStem, ResNetTrunk
    conv1, bn1, stages = T.trunk_modules(case, dtype)
    mods = torch.nn.ModuleList([conv1, bn1] + stages).to(device)
    if bn == 'frozen':
        mods.eval()
    return ResNetTrunk(ResNetStem(conv1, bn1, bn), [ResNetStage(st, bn) for st in stages]), conv1, bn1, stages


def _bns(bn1, stages):
    return [bn1] + [bn for st in stages for b in st for bn in (b.bn1, b.bn2, b.bn3, b.downsample[1])]


@pytest.mark.parametrize('bn', ['frozen', 'batch'])
def test_small_trunk_vs_float64(bn):
    """Bound per tensor: 4 times the error torch's own fp32 CPU autograd makes on the same case against the float64 chain, with a
    floor of 1e-5 (the rule of ``test_stage_vs_float64``).  The figures measured on an MI355X are in DESIGN.md section 7, f-24."""
    case = T.trunk_case()
    ref = (T.trunk_batch if bn == 'batch' else T.trunk_frozen)(case, case['g_out'])
    want = [ref['out']] + ref['g_w']
    names = ['out'] + [f'g_w[{i}]' for i in range(17)]
    if bn == 'batch':
        want += ref['g_gamma'] + ref['g_beta'] + [r[0] for r in ref['running']] + [r[1] for r in ref['running']]
        names += [f'{k}[{i}]' for k in ('g_gamma', 'g_beta', 'running_mean', 'running_var') for i in range(17)]

    def run(fn, conv1, bn1, stages, images, g_out):
        out = fn(images)
        out.backward(g_out)
        bns = _bns(bn1, stages)
        got = [out.detach()] + [p.grad for p in trunk_ws(conv1, stages)]
        if bn == 'batch':
            got += [b.weight.grad for b in bns] + [b.bias.grad for b in bns] + [b.running_mean for b in bns] + [b.running_var for b in bns]
        return got

    def trunk_ws(conv1, stages):
        return [conv1.weight] + [p for st in stages for b in st for p in (b.conv1.weight, b.conv2.weight, b.conv3.weight, b.downsample[0].weight)]
    # torch's fp32 chain on the CPU on the same containers
    conv1, bn1, stages = T.trunk_modules(case)
    if bn == 'frozen':
        for m in [conv1, bn1] + stages:
            m.eval()
    theirs = run(lambda v: T.torch_trunk(conv1, bn1, stages, v.permute(0, 2, 3, 1)), conv1, bn1, stages,
                 case['x'].float().permute(0, 3, 1, 2).contiguous(), case['g_out'].float())
    trunk, dconv1, dbn1, dstages = _trunk(case, bn, DEV)
    assert len(trunk.conv_parameters()) == 17 and len(trunk.bn_parameters()) == 34
    assert all(a is b for a, b in zip(trunk.conv_parameters(), trunk_ws(dconv1, dstages)))
    mine = run(trunk, dconv1, dbn1, dstages, case['x'].float().permute(0, 3, 1, 2).contiguous().to(DEV), case['g_out'].float().to(DEV))
    worst = 0.0
    for n, a, b, w in zip(names, mine, theirs, want):
        e_dev, e_torch = R.err(a, w), R.err(b, w)
        print(f'{bn} {n}: device {e_dev:.3g}, torch fp32 CPU {e_torch:.3g}')
        assert a.shape == w.shape
        assert e_dev < max(4 * e_torch, BOUND), (n, e_dev, e_torch)
        worst = max(worst, e_dev)
    print(f'{bn}: worst device error {worst:.3g}')
    tracked = [int(b.num_batches_tracked) for b in _bns(dbn1, dstages)]
    assert tracked == [1 if bn == 'batch' else 0] * 17
    if bn == 'frozen':
        assert all(b.weight.grad is None and b.bias.grad is None for b in _bns(dbn1, dstages))


def test_composition_and_the_inference_trunk():
    from spec_amd.differentiable import ResNetStage, ResNetTrunk
    net, x = _camcalib_net()
    eng = net.engine(DEV)
    with torch.no_grad():
        # first = 'layer2': Engine.trunk(stages = 1) followed by the three stages, bit for bit
        v = eng.trunk(x, stages=1)
        for name in ('layer2', 'layer3', 'layer4'):
            v = ResNetStage.from_model(net, name)(v)
        assert torch.equal(ResNetTrunk.from_model(net, 'layer2')(x), v)
        # the frozen whole trunk, and the one whose stem runs frozen below layer1, against the inference trunk's pooled feature
        whole = eng.trunk(x).mean(dim=(1, 2))
        a, b = ResNetTrunk.from_model(net, 'stem')(x), ResNetTrunk.from_model(net, 'layer1')(x)
        e = R.err(a.mean(dim=(1, 2)), whole)
        print(f'pooled feature, ResNetTrunk(stem) vs Engine.trunk: {e:.3g}')
        assert e < BOUND and torch.equal(a, b)
        # the stem alone against the trunk cut after layer1's input: Engine.trunk(stages = 1) is layer1's output, so compare there
        l1 = ResNetStage.from_model(net, 'layer1')(ResNetTrunk.from_model(net, 'stem').stem(x))
        assert R.err(l1, eng.trunk(x, stages=1)) < BOUND
    t = ResNetTrunk.from_model(net, 'stem')
    assert len(t.conv_parameters()) == 53 and len(t.bn_parameters()) == 106 and t.conv_parameters()[0] is net.backbone.conv1.weight
    assert len(ResNetTrunk.from_model(net, 'layer3').conv_parameters()) == 19 + 10
    with pytest.raises(ValueError):
        ResNetTrunk.from_model(net, 'layer5')


def test_trunks_without_bottlenecks_are_refused():
    from spec_amd import assets
    from spec_amd.differentiable import ResNetTrunk
    from spec_amd.modules import HMR, CameraRegressorNetwork
    assets.use_synthetic_assets(1003)                  # HMR's head reads the mean parameters when it is built
    with pytest.raises(NotImplementedError):
        ResNetTrunk.from_model(CameraRegressorNetwork(backbone='resnet34'), 'stem')
    with pytest.raises(NotImplementedError):
        ResNetTrunk.from_model(HMR(backbone='hrnet_w32-conv'), 'layer1')


def test_hmr_conv1_gets_a_gradient_through_the_head_and_the_loss():
    from spec_amd import assets, synth
    from spec_amd import differentiable as D
    from spec_amd.losses import HMRLoss
    from spec_amd.modules import HMR
    from tests import smpl_grad_ref as S
    from tests import tail_grad_ref as TG
    assets.use_synthetic_assets(1003)
    sd = synth.hmr_state(2202, False)
    hmr = HMR()
    hmr.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    hmr = hmr.to(DEV).eval()
    x = _t(synth.images(87, TG.B, 64, 64))
    _, _, gt = TG.problem()
    gt = {k: _t(v) for k, v in gt.items()}
    trunk, head = D.ResNetTrunk.from_model(hmr, 'stem'), D.HMRHead.from_hmr(hmr)
    smpl_head = D.SMPLHead(S.FOCAL, S.IMG_RES, model=S.model(TG.NV))
    head.eval()
    pred = head(trunk(x), channels_last=True)
    out = smpl_head(pred['pred_pose'], pred['pred_shape'], pred['pred_cam'])
    HMRLoss()(dict(out, **pred), gt)[0].backward()
    ws = trunk.conv_parameters()
    assert len(ws) == 53 and ws[0] is hmr.backbone.conv1.weight
    for w in ws:
        assert w.grad is not None and w.grad.shape == w.shape and torch.isfinite(w.grad).all() and w.grad.any()


def test_finetune_the_whole_trunk_on_the_standin_tree(tmp_path):
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    ce.write_standin_tree(str(tmp_path), n_images=4, backbone='resnet50')
    hp = ct.load_config(str(tmp_path / ce.STANDIN_CFG))
    start = torch.load(str(tmp_path / ce.STANDIN_CKPT), map_location='cpu')['state_dict']
    start = {k: v.reshape(()) if k.endswith('num_batches_tracked') else v for k, v in start.items()}
    kw = dict(data_root=str(tmp_path), epochs=1, seed=3, log=lambda s: None, evaluate=False)
    res = ct.finetune_heads(hp, out=str(tmp_path / 'all.ckpt'), unfreeze='all', bn='batch', **kw)
    end = torch.load(res['ckpt'], map_location='cpu')['state_dict']
    assert set(end) == set(start) and np.isfinite(res['epochs'][0]['train/loss'])
    convs = [k for k in start if '.backbone.' in k and start[k].dim() == 4]
    bns = [k for k in start if '.backbone.' in k and start[k].dim() < 4]
    heads = [k for k in start if '.fc_' in k]
    assert len(convs) == 53 and len(bns) == 53 * 5 and len(heads) == 6
    assert all(not torch.equal(start[k], end[k]) for k in convs + bns + heads)
    again = ce.build_model(hp, res['ckpt'], str(tmp_path), DEV)         # the checkpoint reloaded: the fine-tuned model's eval() bits
    _, x = _camcalib_net()
    assert all(torch.equal(a, b) for a, b in zip(res['model'](x), again(x)))
    # ('layer3', 'layer4') in any order: the stem, layer1 and layer2 stay bit-identical
    res = ct.finetune_heads(hp, out=str(tmp_path / 'l34.ckpt'), unfreeze=('layer4', 'layer3'), **kw)
    end = torch.load(res['ckpt'], map_location='cpu')['state_dict']
    moved = [k for k in start if not torch.equal(start[k], end[k])]
    assert moved and all('.fc_' in k or 'backbone.layer3' in k or 'backbone.layer4' in k for k in moved)
    assert sum(1 for k in moved if start[k].dim() == 4) == 19 + 10
    for bad in (('stem',), ('layer1', 'layer3', 'layer4'), ('layer4', 'layer4'), 'layer2'):
        with pytest.raises(NotImplementedError):
            ct.finetune_heads(hp, unfreeze=bad, **kw)
    assert ct.normalise_unfreeze('all') == ct.normalise_unfreeze(('layer2', 'stem', 'layer4', 'layer1', 'layer3')) == ('stem', 'layer1', 'layer2', 'layer3', 'layer4')


@pytest.mark.parametrize('bn', ['frozen', 'batch'])
def test_six_sgd_steps_through_the_trunk_follow_the_float64_chain(bn):
    """Plain gradient descent on the small trunk's 17 conv weights (with ``bn='batch'`` also its gammas and betas, the running
    statistics moving) and three Linear heads: every step lowers the loss, and the losses follow the float64 chain of
    tests/trunk_grad_ref.py to 1e-4 of the first.  On batch statistics that bound is below what fp32 can keep on this trunk - layer4's
    BatchNorms see 4 values per channel, and torch's own fp32 CPU autograd leaves the float64 path by 1.6e-3 within the six steps
    (``trunk_grad_ref.sgd_losses_torch32``) - so there the bound is the rule of ``test_small_trunk_vs_float64``: 4 times the deviation of
    torch's fp32 CPU chain, with 1e-4 of the first loss as the floor.  Measured on an MI355X: frozen 1.0e-6, batch 1.65e-3 (torch 1.61e-3)."""
    from spec_amd.differentiable import CameraRegressorHead
    from spec_amd.losses import CameraRegressorLoss
    p = T.sgd_problem()
    trunk, _, _, _ = _trunk(p['trunk'], bn, DEV)
    head = CameraRegressorHead(p['head']['fc_vfov.weight'].shape[1], 1, 1024, T.SGD_NBINS)
    head.load_state_dict({k: v.float() for k, v in p['head'].items()})
    head = head.to(DEV)
    crit = CameraRegressorLoss(1.0, 1.0, 1.0, 'ce')
    images = p['trunk']['x'].float().permute(0, 3, 1, 2).contiguous().to(DEV)
    tg = [t.to(DEV) for t in p['targets']]
    opt = torch.optim.SGD(trunk.conv_parameters() + (trunk.bn_parameters() if bn == 'batch' else []) + list(head.parameters()), lr=T.SGD_RATE)
    losses = []
    for _ in range(T.SGD_STEPS):
        opt.zero_grad()
        loss, _ = crit(*head(trunk(images), channels_last=True), *tg)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(crit(*head(trunk(images), channels_last=True), *tg)[0]))
    want = T.sgd_losses64(bn)
    print(bn, ' '.join(f'{v:.6f}' for v in losses), '| float64', ' '.join(f'{v:.6f}' for v in want))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    dev = max(abs(a - b) for a, b in zip(losses, want))
    bound = 1e-4 * want[0]
    if bn == 'batch':
        theirs = max(abs(a - b) for a, b in zip(T.sgd_losses_torch32(bn), want))
        print(f'batch: device {dev:.3g}, torch fp32 CPU {theirs:.3g}')
        bound = max(bound, 4 * theirs)
    assert dev < bound, (dev, bound)
