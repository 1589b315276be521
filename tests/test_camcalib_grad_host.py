"""The float64 yardstick of CamCalib's differentiable tail (tests/camcalib_grad_ref.py) against the gradients the reference's own
camcalib/loss.py gives under torch.autograd (tests/golden/camcalib_loss_grad.npz), against float64 autograd of plain restatements,
and against central differences - on the CPU.  The shim's import is checked here too.

Bound of the fp32 comparison: the one of tests/test_hmr_loss_grad_host.py - both sides evaluate the same formulae, the fixture in
fp32: a handful of roundings per element and a softmax over at most 256 bins, below 1e-6 of the tensor's largest magnitude."""
import numpy as np
import pytest
import torch

from tests import camcalib_grad_ref as R
from tests.util import golden

FP32_BOUND = 1e-6
CASES = [(name, lt) for name in R.FIXTURE_CASES for lt in R.LOSS_TYPES]


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Tests that ran earlier in the process may have switched autograd off for good (the scripts do)."""
    with torch.enable_grad():
        yield


@pytest.fixture(scope='module')
def fx():
    return golden('camcalib_loss_grad.npz')


def restated_loss(logits, targets, loss_type, weights):
    """CameraRegressorLoss in plain torch on float64 tensors -> the four values of loss_dict."""
    n = logits[0].shape[-1]
    heads = []
    for k in range(3):
        if loss_type in ('ce', 'kl'):
            term = torch.nn.functional.cross_entropy(logits[k], targets[k], reduction='none')
        else:
            p = torch.softmax(logits[k], -1)
            s = 2 * (p * torch.arange(n, dtype=p.dtype)).sum(-1) / (n - 1) - 1
            l2 = (targets[k].to(p.dtype) - s) ** 2
            term = torch.where(s > targets[k], l2, l2 / (l2 + 1)) if (loss_type == 'softargmax_biased_l2' and k == 0) else l2
        heads.append(weights[k] * term.mean())
    return [heads[0] + heads[1] + heads[2], *heads]


@pytest.mark.parametrize('name,lt', CASES)
def test_yardstick_matches_the_reference_gradients(fx, name, lt):
    B, nbins, scale = R.FIXTURE_CASES[name]
    logits, targets = R.loss_case(B, nbins, lt, scale)
    _, means, grads = R.camcalib_loss(logits, targets, lt)
    e = R.err(fx[f'{name}.{lt}.grads'], grads)
    print(f'{name} {lt}: {e:.3g}')
    assert e < FP32_BOUND
    assert np.all(np.abs(fx[f'{name}.{lt}.values'] - means) <= FP32_BOUND * np.abs(means).max())


@pytest.mark.parametrize('name,lt', CASES)
def test_yardstick_matches_float64_autograd(name, lt):
    B, nbins, scale = R.FIXTURE_CASES[name]
    logits, targets = R.loss_case(B, nbins, lt, scale)
    for j in range(4):                                 # every entry of loss_dict may be backpropagated
        x = torch.from_numpy(logits).double().requires_grad_(True)
        vals = restated_loss(x, torch.from_numpy(targets), lt, R.WEIGHTS)
        vals[j].backward()
        _, means, grads = R.camcalib_loss(logits, targets, lt, g_means=np.eye(4)[j])
        assert R.err(grads, x.grad.numpy()) < 1e-12
        assert abs(means[j] - vals[j].item()) <= 1e-12 * max(abs(vals[j].item()), 1.0)


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
def test_yardstick_matches_central_differences(lt):
    B, nbins = 2, 9
    logits, targets = R.loss_case(B, nbins, lt, 1.0)
    _, _, grads = R.camcalib_loss(logits, targets, lt)
    x = logits.astype(np.float64)
    h = 1e-6
    num = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        hi, lo = x.copy(), x.copy()
        hi[i] += h
        lo[i] -= h
        num[i] = (R.camcalib_loss(hi, targets, lt)[1][0] - R.camcalib_loss(lo, targets, lt)[1][0]) / (2 * h)
    assert R.err(grads, num) < 1e-8                    # h^2 x the third derivative, O(1): 1e-12, and 1e-16 / h of rounding


def test_centred_sum_keeps_the_saturated_rows_digits():
    """On the row that spans +-1e4 the neighbour of the hot bin holds exp(-78) = 1e-34: the gradient there is that small, not 0."""
    for lt in ('softargmax_l2', 'softargmax_biased_l2'):
        logits, targets = R.saturated_case(257, lt)
        _, _, grads = R.camcalib_loss(logits, targets, lt)
        row = grads[1, 4]
        assert row[256] != 0 and row[255] != 0 and abs(row[256] + row[255]) <= 1e-12 * abs(row[256])      # sum_i p_i (i - E) = 0


@pytest.mark.parametrize('shape', R.HEAD_SHAPES[:3] + ((2, 7, 1, 1, 5),))
def test_chain_backward_matches_float64_autograd(shape):
    B, F, L, Hc, nbins = shape
    params, xf, g_logits = R.head_case(*shape)
    heads = []
    for h in R.HEADS:
        widths = [F] + [Hc] * (L - 1) + [nbins]
        seq = torch.nn.Sequential(*(torch.nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))).double()
        heads.append(seq[0] if L == 1 else seq)
    net = torch.nn.ModuleDict(dict(zip(R.HEADS, heads)))
    net.load_state_dict({k: torch.from_numpy(v).double() for k, v in params.items()})
    x = torch.from_numpy(xf).double().requires_grad_(True)
    logits = torch.stack([net[h](x) for h in R.HEADS])
    logits.backward(torch.from_numpy(g_logits).double())
    want_logits, _ = R.chain_forward(params, xf, L)
    g_xf, grads = R.chain_backward(params, xf, L, g_logits)
    assert R.err(want_logits, logits.detach().numpy()) < 1e-12
    assert R.err(g_xf, x.grad.numpy()) < 1e-12
    assert set(grads) == set(R.param_names(L)) == set(dict(net.named_parameters()))
    for k, p in net.named_parameters():
        assert grads[k].shape == tuple(p.shape) and R.err(grads[k], p.grad.numpy()) < 1e-12, k


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
def test_sgd_rate_descends_on_the_float64_chain(lt):
    for rate in (R.SGD_RATE, 10 * R.SGD_RATE):
        losses = R.sgd_losses(lt, rate=rate)
        assert len(losses) == R.SGD_STEPS + 1 and all(b < a for a, b in zip(losses, losses[1:])), (rate, losses)


def test_shim_imports_and_has_no_cpu_path():
    from camcalib.loss import CameraRegressorLoss, KLDivergence, SoftargmaxClsLoss
    x, t = torch.zeros(2, 4), torch.zeros(2, dtype=torch.long)
    with pytest.raises(RuntimeError, match='no CPU path'):
        CameraRegressorLoss()(x, x, x, t, t, t)
    with pytest.raises(RuntimeError, match='no CPU path'):
        KLDivergence()(x, t)
    with pytest.raises(RuntimeError, match='no CPU path'):
        SoftargmaxClsLoss('biased_l2')(x, t.float())
    with pytest.raises(ValueError, match='bogus is not defined'):
        CameraRegressorLoss(loss_type='bogus')
    from spec_amd.differentiable import CameraRegressorHead
    head = CameraRegressorHead(8, 2, 5, 3)
    assert list(head.state_dict()) == list(R.param_names(2))
    with pytest.raises(RuntimeError, match='no CPU path'):
        head(torch.zeros(2, 8))
    one = CameraRegressorHead(8, 1, 5, 3)
    assert list(one.state_dict()) == list(R.param_names(1)) and not one.fc_roll.bias.any()
