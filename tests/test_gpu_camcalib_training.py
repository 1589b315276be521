"""CamCalib's differentiable tail as a user meets it: ``spec_amd.differentiable.CameraRegressorHead`` ->
``spec_amd.losses.CameraRegressorLoss`` -> ``backward()`` -> an optimiser of torch's, against the float64 chain of
tests/camcalib_grad_ref.py; ``from_model`` on a committed network; ``camcalib_train.finetune_heads`` on the stand-in tree.

Bound 1e-5 on max |a - b| / max |b| per tensor, the project's bound for every gradient of the differentiable tail."""
import numpy as np
import pytest
import torch

from tests import camcalib_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5
B, F, L, HC, NBINS = R.TRAIN_SHAPE


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Tests that ran earlier in the process may have switched autograd off for good (the scripts do)."""
    with torch.enable_grad():
        yield


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _head(params):
    from spec_amd.differentiable import CameraRegressorHead
    head = CameraRegressorHead(F, L, HC, NBINS)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return head.to(DEV)


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
def test_features_head_loss_backward_vs_float64(lt):
    from spec_amd.losses import CameraRegressorLoss
    params, xf, _ = R.head_case(*R.TRAIN_SHAPE)
    _, targets = R.loss_case(B, NBINS, lt)
    want_means, want_xf, want = R.tail_grads(params, xf, L, targets, lt)
    head = _head(params)
    crit = CameraRegressorLoss(*R.WEIGHTS, loss_type=lt)
    # a (B, F, h, w) feature map whose spatial mean is xf: the pool runs inside autograd
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((B, F, 2, 3)).astype(np.float32)
    feat = _t(xf[:, :, None, None] + noise - noise.mean((2, 3), keepdims=True)).requires_grad_(True)
    preds = head(feat)
    assert len(preds) == 3 and all(p.shape == (B, NBINS) and p.requires_grad for p in preds)
    loss, d = crit(*preds, *(_t(t) for t in targets))
    assert list(d) == list(R.LOSS_KEYS) and loss is d['loss'] and all(v.dim() == 0 and v.grad_fn is not None for v in d.values())
    loss.backward()
    e = {'means': R.err(torch.stack(list(d.values())).detach().cpu().numpy(), want_means),
         'features': R.err(feat.grad.cpu().numpy(), np.broadcast_to(want_xf[:, :, None, None] / 6.0, (B, F, 2, 3))),
         **{n: R.err(p.grad.cpu().numpy(), want[n]) for n, p in head.named_parameters()}}
    worst = max(e, key=e.get)
    print(f'{lt}: worst {worst} {e[worst]:.3g}')
    assert e[worst] < BOUND, e
    # any entry of loss_dict may be backpropagated; trailing singleton dimensions are squeezed
    head.zero_grad()
    crit(*(p.unsqueeze(-1) for p in head(_t(xf))), *(_t(t) for t in targets))[1]['pitch_loss'].backward()
    assert head.fc_vfov[0].weight.grad is None or not head.fc_vfov[0].weight.grad.any()
    want_pitch = R.chain_backward(params, xf, L, R.camcalib_loss(R.chain_forward(params, xf, L)[0], targets, lt, g_means=(0, 0, 1, 0))[2])[1]
    assert R.err(head.fc_pitch[1].weight.grad.cpu().numpy(), want_pitch['fc_pitch.1.weight']) < BOUND


@pytest.mark.parametrize('lt', ('kl', 'softargmax_biased_l2'))
def test_eval_keeps_no_graph_and_equals_the_c_call(lt):
    from spec_amd.cam_utils import _engine
    from spec_amd.losses import CameraRegressorLoss
    params, xf, _ = R.head_case(*R.TRAIN_SHAPE)
    _, targets = R.loss_case(B, NBINS, lt)
    head = _head(params)
    crit = CameraRegressorLoss(*R.WEIGHTS, loss_type=lt)
    eng = _engine(DEV)
    with torch.no_grad():
        preds = head(_t(xf))
        loss, d = crit(*preds, *targets)
    assert all(p.grad_fn is None and not p.requires_grad for p in preds) and all(v.grad_fn is None for v in d.values())
    logits, _ = eng.camcalib_head_train_forward({k: v.detach() for k, v in head.named_parameters()}, _t(xf), L)
    assert all(torch.equal(a, b) for a, b in zip(preds, logits))
    ev = eng.camcalib_eval(*logits, targets, np.zeros((3, B), np.float32), lt, R.WEIGHTS)
    assert torch.equal(torch.stack(list(d.values())), ev['means'][:4])
    # with grad enabled but nothing requiring grad: the same, without a graph
    detached = [p.detach() for p in preds]
    loss2, d2 = crit(*detached, *targets)
    assert loss2.grad_fn is None and torch.equal(torch.stack(list(d2.values())), ev['means'][:4])
    # with a graph: the same bits
    leaf = [p.clone().requires_grad_(True) for p in detached]
    loss3, _ = crit(*leaf, *targets)
    assert loss3.grad_fn is not None and torch.equal(loss3.detach(), ev['means'][0])
    with pytest.raises(ValueError, match='l2 is not defined'):
        CameraRegressorLoss(loss_type='l2')


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
def test_six_sgd_steps_lower_the_loss_every_time(lt):
    from spec_amd.losses import CameraRegressorLoss
    params, xf, _ = R.head_case(*R.TRAIN_SHAPE)
    _, targets = R.loss_case(B, NBINS, lt)
    head = _head(params)
    crit = CameraRegressorLoss(*R.WEIGHTS, loss_type=lt)
    opt = torch.optim.SGD(head.parameters(), lr=R.SGD_RATE)
    x, tg = _t(xf), [_t(t) for t in targets]
    losses = []
    for _ in range(R.SGD_STEPS):
        opt.zero_grad()
        loss, _ = crit(*head(x), *tg)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(crit(*head(x), *tg)[0]))
    want = R.sgd_losses(lt)
    print(lt, ' '.join(f'{v:.6f}' for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert max(abs(a - b) for a, b in zip(losses, want)) < 1e-4 * want[0]       # the float64 chain's path, step by step


@pytest.mark.parametrize('backbone,layers', (('resnet18', 1), ('resnet34', 2)))
def test_from_model_shares_the_parameters_and_the_network_commits_them_again(backbone, layers):
    from spec_amd import synth
    from spec_amd.differentiable import CameraRegressorHead
    from spec_amd.losses import CameraRegressorLoss
    from spec_amd.modules import CameraRegressorNetwork
    sd = synth.camcalib_state(1801, backbone=backbone, num_fc_layers=layers, num_fc_channels=64)
    net = CameraRegressorNetwork(backbone=backbone, num_fc_layers=layers, num_fc_channels=64)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    net = net.to(DEV).eval()
    n = 2
    x = _t(synth.images(84, n, 64, 64))
    before = torch.stack(net(x)).clone()
    feat = net.engine(DEV).trunk(x)                                  # (n, 2, 2, 512), frozen
    head = CameraRegressorHead.from_model(net)
    assert head.num_input_features == 512 and head.num_fc_layers == layers and head.num_out_channels == 256
    mine, theirs = dict(head.named_parameters()), dict(net.named_parameters())
    assert len(mine) == 6 * layers and all(mine[k] is theirs[k] for k in mine)
    crit = CameraRegressorLoss(loss_type='softargmax_l2')
    targets = [torch.tensor([0.3, -0.4], device=DEV), torch.tensor([-0.2, 0.1], device=DEV), torch.tensor([0.0, 0.6], device=DEV)]
    opt = torch.optim.Adam(head.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad()
        with torch.enable_grad():
            crit(*head(feat, channels_last=True), *targets)[0].backward()
        opt.step()
    with torch.no_grad():
        ref = torch.stack(head(feat, channels_last=True))
    after = torch.stack(net(x))                                      # the bumped versions are seen: the network commits by itself
    top = float(ref.abs().max())
    agree, moved = float((after - ref).abs().max()) / top, float((after - before).abs().max()) / top
    print(f'{backbone}, {layers} layers, after the steps: network vs differentiable head {agree:.3g}, network after vs before {moved:.3g}')
    assert agree < 1e-5 and moved > 100 * agree, (agree, moved)


def test_finetune_heads_on_the_standin_tree(tmp_path):
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    from spec_amd import synth
    ce.write_standin_tree(str(tmp_path))
    hp = ct.load_config(str(tmp_path / ce.STANDIN_CFG))
    lines = []
    res = ct.finetune_heads(hp, data_root=str(tmp_path), epochs=2, seed=3, log=lines.append)
    e1, e2 = res['epochs']
    print(e1, e2, res['before'], res['after'])
    assert set(e1) == set(ct.TRAIN_KEYS) and e2['train/loss'] < e1['train/loss']
    assert set(res['before']) == set(res['after']) == {'val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc'}
    assert any(line.startswith('[EPOCH 1] train/loss') for line in lines)
    again = ce.build_model(hp, res['ckpt'], str(tmp_path), DEV)
    x = _t(synth.images(85, 2, 96, 128))
    a, b = res['model'](x), again(x)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    first = ce.build_model(hp, None, str(tmp_path), DEV)                # the checkpoint it started from answers otherwise
    assert not torch.equal(first(x)[0], a[0])
