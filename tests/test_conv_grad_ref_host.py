"""tests/conv_grad_ref.py checked on the host: its three gradients against ``torch.autograd`` on ``F.conv2d`` in float64, the mask
condition of every committed case, and the exactness of the exact cases.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_grad_ref as R


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Tests that ran earlier in the process may have switched autograd off for good (the scripts do)."""
    with torch.enable_grad():
        yield


def _autograd(t, relu, residual, add):
    x = t['x'].clone().requires_grad_(True)
    w = t['w'].clone().requires_grad_(True)
    res = t['res'].clone().requires_grad_(True) if residual else None
    z = F.conv2d(x.permute(0, 3, 1, 2), w, stride=t['stride'], padding=t['pad']).permute(0, 2, 3, 1) * t['scale'] + t['shift']
    if residual:
        z = z + res
    y = torch.relu(z) if relu else z
    y.backward(t['g_y'])
    g_x = x.grad + (t['g_x_add'] if add else 0)
    return y.detach(), g_x, w.grad, (res.grad if residual else None)


@pytest.mark.parametrize('shape', R.LAYER_CASES, ids=str)
@pytest.mark.parametrize('relu,residual,add', [(True, True, True), (True, False, False), (False, True, False), (False, False, True)])
def test_reference_equals_autograd(shape, relu, residual, add):
    t = R.layer_case(shape)
    res = t['res'] if residual else None
    y, z = R.layer_forward(t['x'], t['w'], t['scale'], t['shift'], t['stride'], t['pad'], res, relu)
    g_x, g_w, g_res = R.layer_backward(t['x'], t['w'], t['scale'], t['stride'], t['pad'], z, t['g_y'], relu, t['g_x_add'] if add else None)
    ay, agx, agw, agres = _autograd(t, relu, residual, add)
    for mine, theirs in ((y, ay), (g_x, agx), (g_w, agw)) + (((g_res, agres),) if residual else ()):
        assert torch.allclose(mine, theirs, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('shape', R.LAYER_CASES, ids=str)
def test_band_condition_of_the_layer_cases(shape):
    t = R.layer_case(shape)
    assert t['seed_steps'] < R.MAX_SEED_STEPS
    for res in (None, t['res']):
        z = R.layer_forward(t['x'], t['w'], t['scale'], t['shift'], t['stride'], t['pad'], res, True)[1]
        assert z.abs().min().item() > R.BAND * z.abs().max().item()


def test_band_condition_of_the_stage_case():
    t = R.stage_case()
    assert t['seed_steps'] < R.MAX_SEED_STEPS
    r = R.bottleneck_stage(t['x'], t['blocks'], t['g_out'])
    assert R.band_empty(r['zs']) and len(r['g_w']) == 10
    assert [tuple(g.shape) for g in r['g_w']] == [tuple(b[c]['w'].shape) for b in t['blocks'] for c in ('c1', 'c2', 'c3', 'ds') if c in b]


def test_stage_reference_equals_autograd():
    t = R.stage_case()
    r = R.bottleneck_stage(t['x'], t['blocks'], t['g_out'])
    x = t['x'].clone().requires_grad_(True)
    ws = []

    def layer(v, c, s, p, relu, res=None):
        c['leaf'] = c['w'].clone().requires_grad_(True)
        z = F.conv2d(v.permute(0, 3, 1, 2), c['leaf'], stride=s, padding=p).permute(0, 2, 3, 1) * c['scale'] + c['shift']
        if res is not None:
            z = z + res
        return torch.relu(z) if relu else z
    v = x
    for blk in t['blocks']:
        y1 = layer(v, blk['c1'], 1, 0, True)
        y2 = layer(y1, blk['c2'], blk['stride'], 1, True)
        idn = layer(v, blk['ds'], blk['stride'], 0, False) if 'ds' in blk else v
        v = layer(y2, blk['c3'], 1, 0, True, idn)
        ws += [blk[c]['leaf'] for c in ('c1', 'c2', 'c3', 'ds') if c in blk]
    v.backward(t['g_out'])
    assert torch.allclose(r['out'], v.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(r['g_x'], x.grad, rtol=1e-12, atol=1e-12)
    assert len(ws) == 10
    for mine, w in zip(r['g_w'], ws):
        assert torch.allclose(mine, w.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('shape', R.LAYER_CASES, ids=str)
def test_exact_cases_are_exact(shape):
    t = R.layer_case(shape, exact=True)
    f = {k: v.float() if isinstance(v, torch.Tensor) else v for k, v in t.items()}
    outs = []
    for d in (t, f):
        y, z = R.layer_forward(d['x'], d['w'], d['scale'], d['shift'], d['stride'], d['pad'], d['res'], True)
        outs.append((y, z) + R.layer_backward(d['x'], d['w'], d['scale'], d['stride'], d['pad'], z, d['g_y'], True, d['g_x_add']))
    for a64, a32 in zip(*outs):
        assert a32.dtype == torch.float32 and torch.equal(a64, a32.double())
    assert (outs[0][1] == 0).any(), 'an exact case is there for its z == 0 elements'


def test_the_descent_rate_has_a_factor_two_margin():
    for rate in (R.SGD_RATE, 2 * R.SGD_RATE):
        losses = R.sgd_losses64(rate)
        assert len(losses) == R.SGD_STEPS + 1 and all(b < a for a, b in zip(losses, losses[1:])), (rate, losses)
