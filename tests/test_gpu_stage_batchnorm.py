"""``spec_amd.differentiable.ResNetStage(bn='batch')`` - a stage of bottlenecks with BatchNorm on the statistics of the batch, as the
reference's ``training_step`` runs it - against the float64 stage of tests/bn_ref.py, beside the frozen route it must leave alone,
and ``camcalib_train.finetune_heads(..., unfreeze=('layer4',), bn='batch')`` on the stand-in tree."""
import numpy as np
import pytest
import torch

from tests import bn_ref as N

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Tests that ran earlier in the process may have switched autograd off for good (the scripts do)."""
    with torch.enable_grad():
        yield


def _convs(mods):
    return [c for m in mods for c in [m.conv1, m.conv2, m.conv3] + ([m.downsample[0]] if hasattr(m, 'downsample') else [])]


def _run(stage, mods, x, g_out):
    """One forward and backward -> the tensors test_stage_vs_float64 compares, in the order of its names."""
    out = stage(x)
    out.backward(g_out)
    bns = N.module_bns(mods)
    return ([out.detach(), x.grad] + [c.weight.grad for c in _convs(mods)] + [b.weight.grad for b in bns] + [b.bias.grad for b in bns] +
            [b.running_mean for b in bns] + [b.running_var for b in bns])


def test_stage_vs_float64():
    """Bound per tensor: 4 times the error torch's own fp32 CPU autograd makes on the same blocks in ``train()`` against the float64
    reference, with a floor of 1e-5 (the rule of tests/test_gpu_trunk_finetune.py).  Measured on an MI355X: DESIGN.md section 7, f-23."""
    from spec_amd.differentiable import ResNetStage
    case = N.stage_case()
    ref = N.bottleneck_stage_batch(case['x'], case['blocks'], case['stats'], case['g_out'])
    names = (['out', 'g_x'] + [f'g_w[{i}]' for i in range(7)] + [f'g_gamma[{i}]' for i in range(7)] + [f'g_beta[{i}]' for i in range(7)] +
             [f'running_mean[{i}]' for i in range(7)] + [f'running_var[{i}]' for i in range(7)])
    want = [ref['out'], ref['g_x']] + ref['g_w'] + ref['g_gamma'] + ref['g_beta'] + [r[0] for r in ref['running']] + [r[1] for r in ref['running']]
    cpu = N.stage_module(case)
    theirs = _run(lambda v: N.torch_stage(cpu, v), cpu, case['x'].float().requires_grad_(True), case['g_out'].float())
    dev = N.stage_module(case).to(DEV)
    stage = ResNetStage(dev, bn='batch')
    assert len(stage.conv_parameters()) == 7 and len(stage.bn_parameters()) == 14
    assert all(any(p is q for q in dev.parameters()) for p in stage.bn_parameters())
    mine = _run(stage, dev, case['x'].float().to(DEV).requires_grad_(True), case['g_out'].float().to(DEV))
    worst = 0.0
    for n, a, b, w in zip(names, mine, theirs, want):
        e_dev, e_torch = N.err(a, w), N.err(b, w)
        print(f'{n}: device {e_dev:.3g}, torch fp32 CPU {e_torch:.3g}')
        assert a.shape == w.shape
        assert e_dev < max(4 * e_torch, BOUND), (n, e_dev, e_torch)
        worst = max(worst, e_dev)
    print(f'worst device error {worst:.3g}')
    assert all(int(b.num_batches_tracked) == 1 for b in N.module_bns(dev))
    # a forward under no_grad still is a training-mode forward: the statistics move and the count goes on, no tape is kept
    with torch.no_grad():
        again = stage(case['x'].float().to(DEV))
    assert again.grad_fn is None and all(int(b.num_batches_tracked) == 2 for b in N.module_bns(dev))
    assert torch.equal(again, mine[0])                     # the batch's own statistics: the same output bits


def test_needs_input_grad_chooses_what_is_computed():
    """Only gamma and beta of the downsample BatchNorm and conv3's weight require grad: exactly those get gradients, with the bits of
    the full backward."""
    from spec_amd.differentiable import ResNetStage
    case = N.stage_case()
    x, g_out = case['x'].float().to(DEV), case['g_out'].float().to(DEV)
    full_mods = N.stage_module(case).to(DEV)
    ResNetStage(full_mods, bn='batch')(x).backward(g_out)
    mods = N.stage_module(case).to(DEV)
    for p in mods.parameters():
        p.requires_grad_(False)
    picked = [mods[0].downsample[1].weight, mods[0].downsample[1].bias, mods[0].conv3.weight]
    for p in picked:
        p.requires_grad_(True)
    ResNetStage(mods, bn='batch')(x).backward(g_out)
    full = dict(full_mods.named_parameters())
    for name, p in mods.named_parameters():
        if any(p is q for q in picked):
            assert torch.equal(p.grad, full[name].grad), name
        else:
            assert p.grad is None, name


def test_the_default_route_and_eval_mode_are_the_frozen_path_bit_for_bit():
    from spec_amd.differentiable import ResNetStage
    case = N.stage_case()
    x, g_out = case['x'].float().to(DEV), case['g_out'].float().to(DEV)

    def run(make, mode):
        mods = N.stage_module(case).to(DEV).train(mode)
        stage = make(mods)
        leaf = x.clone().requires_grad_(True)
        out = stage(leaf)
        out.backward(g_out)
        sd = {k: v.clone() for k, v in mods.state_dict().items()}
        return [out.detach(), leaf.grad] + [c.weight.grad for c in _convs(mods)], mods, sd
    start = N.stage_module(case).state_dict()
    # the parent's route: _Bottleneck on the folds, called as the parent's forward calls it
    from spec_amd import differentiable as D

    def parent(mods):
        def fwd(v):
            eng = D._engine(DEV)
            for blk in mods:
                ds = hasattr(blk, 'downsample')
                ws = [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight] + ([blk.downsample[0].weight] if ds else [])
                folds = [D._fold_bn(bn) for bn in [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if ds else [])]
                v = D._Bottleneck.apply(eng, blk.conv2.stride[0], folds, v, *ws)
            return v
        return fwd
    want, _, _ = run(parent, False)
    routes = {'default, eval': (lambda m: ResNetStage(m), False), 'default, train': (lambda m: ResNetStage(m), True),
              'frozen, train': (lambda m: ResNetStage(m, bn='frozen'), True), 'batch, eval': (lambda m: ResNetStage(m, bn='batch'), False)}
    for name, (make, mode) in routes.items():
        got, mods, sd = run(make, mode)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), name
        # no statistic moved, nothing counted, gamma and beta got no gradient
        assert all(torch.equal(sd[k].cpu(), start[k]) for k in start), name
        assert all(b.weight.grad is None and b.bias.grad is None and int(b.num_batches_tracked) == 0 for b in N.module_bns(mods)), name
    batch, _, _ = run(lambda m: ResNetStage(m, bn='batch'), True)
    assert not torch.equal(batch[0], want[0])
    with pytest.raises(ValueError):
        ResNetStage(N.stage_module(case), bn='sync')


def test_six_sgd_steps_on_stage_batchnorm_and_head_lower_the_loss_every_time():
    from spec_amd.differentiable import CameraRegressorHead, ResNetStage
    from spec_amd.losses import CameraRegressorLoss
    p = N.sgd_problem()
    stage = ResNetStage(N.stage_module(p['stage']).to(DEV), bn='batch')
    head = CameraRegressorHead(32, 1, 1024, N.SGD_NBINS)
    head.load_state_dict({k: v.float() for k, v in p['head'].items()})
    head = head.to(DEV)
    crit = CameraRegressorLoss(1.0, 1.0, 1.0, 'ce')
    x, tg = p['stage']['x'].float().to(DEV), [t.to(DEV) for t in p['targets']]
    opt = torch.optim.SGD(stage.conv_parameters() + stage.bn_parameters() + list(head.parameters()), lr=N.SGD_RATE)
    losses = []
    for _ in range(N.SGD_STEPS):
        opt.zero_grad()
        loss, _ = crit(*head(stage(x), channels_last=True), *tg)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(crit(*head(stage(x), channels_last=True), *tg)[0]))
    want = N.sgd_losses64()
    print(' '.join(f'{v:.6f}' for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert max(abs(a - b) for a, b in zip(losses, want)) < 1e-4 * want[0]       # the float64 chain's path, step by step


def test_finetune_on_batch_statistics_on_the_standin_tree(tmp_path):
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    from spec_amd import synth
    ce.write_standin_tree(str(tmp_path), n_images=4, backbone='resnet50')
    hp = ct.load_config(str(tmp_path / ce.STANDIN_CFG))
    start = torch.load(str(tmp_path / ce.STANDIN_CKPT), map_location='cpu')['state_dict']
    start = {k: v.reshape(()) if k.endswith('num_batches_tracked') else v for k, v in start.items()}      # (1,) in the synthetic file, () in a module
    kw = dict(data_root=str(tmp_path), epochs=1, seed=3, log=lambda s: None, evaluate=False, unfreeze=('layer4',))
    res = ct.finetune_heads(hp, out=str(tmp_path / 'batch.ckpt'), bn='batch', **kw)
    assert np.isfinite(res['epochs'][0]['train/loss'])
    assert not any(m.training for m in res['model'].backbone.layer4.modules())                             # back in eval()
    end = torch.load(res['ckpt'], map_location='cpu')['state_dict']
    assert set(end) == set(start)
    l4 = [k for k in start if 'backbone.layer4' in k]
    stats = [k for k in l4 if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    affine = [k for k in l4 if start[k].dim() == 1 and k.endswith(('.weight', '.bias'))]
    convs = [k for k in l4 if start[k].dim() == 4]
    heads = [k for k in start if '.fc_' in k]
    assert len(stats) == 3 * 10 and len(affine) == 2 * 10 and len(convs) == 10 and len(heads) == 6
    assert all(not torch.equal(start[k], end[k]) for k in stats + affine + convs + heads)
    counts = [int(end[k] - start[k]) for k in stats if k.endswith('num_batches_tracked')]
    assert counts[0] >= 1 and len(set(counts)) == 1                                                        # one count per training batch
    touched = set(stats + affine + convs + heads)
    assert all(torch.equal(start[k], end[k]) for k in start if k not in touched)                           # the stem and layers 1-3
    # reloaded into a fresh network, its eval() forward is the fine-tuned network's: the recommitted trunk carries the new statistics
    again = ce.build_model(hp, res['ckpt'], str(tmp_path), DEV)
    x = torch.from_numpy(np.ascontiguousarray(synth.images(86, 2, 64, 64))).to(DEV)
    a, b = torch.stack(res['model'](x)), torch.stack(again(x))
    e = float((a - b).abs().max()) / float(b.abs().max())
    print(f'fine-tuned network vs its checkpoint reloaded: {e:.3g}')
    assert e < BOUND
    # bn='frozen' is the default flow, bit for bit
    fa = ct.finetune_heads(hp, out=str(tmp_path / 'a.ckpt'), **kw)
    fb = ct.finetune_heads(hp, out=str(tmp_path / 'b.ckpt'), bn='frozen', **kw)
    sa, sb = (torch.load(r['ckpt'], map_location='cpu')['state_dict'] for r in (fa, fb))
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa) and fa['epochs'] == fb['epochs']
    assert all(torch.equal(start[k], sa[k]) for k in stats + affine)                                       # frozen: no BatchNorm tensor moves
    with pytest.raises(ValueError):
        ct.finetune_heads(hp, bn='batch', **dict(kw, unfreeze=()))
    with pytest.raises(ValueError):
        ct.finetune_heads(hp, bn='sync', **kw)
