"""tests/bn_ref.py against torch's own float64 autograd of ``F.batch_norm`` on the host - the reference of the BatchNorm kernels is
itself checked before a device is asked anything - and the properties its cases rely on."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as N

OFFSET_CASES = [(513, 4), (4097, 3)]


@pytest.mark.parametrize('relu,residual', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('M,C', [(2, 1), (2, 5), (18, 65), (7, 4), (63, 3), (129, 130)])
def test_formulas_vs_float64_autograd_of_batch_norm(M, C, relu, residual):
    t = N.case(M, C)
    f = 0.3
    mine = N.forward(t['z'], t['gamma'], t['beta'], N.EPS, t['res'] if residual else None, relu, t['running_mean'], t['running_var'], f)
    g_z, g_gamma, g_beta, g_res = N.backward(t['z'], t['gamma'], mine['mean'], mine['invstd'], mine['pre'], t['g_y'], relu)
    with torch.enable_grad():
        z, gamma, beta, res = (t[k].clone().requires_grad_(True) for k in ('z', 'gamma', 'beta', 'res'))
        rm, rv = t['running_mean'].clone(), t['running_var'].clone()
        y = F.batch_norm(z, rm, rv, gamma, beta, True, f, N.EPS)
        if residual:
            y = y + res
        if relu:
            y = torch.relu(y)
        y.backward(t['g_y'])
    bound = 1e-12
    assert N.err(mine['y'], y) < bound and N.err(mine['running_mean'], rm) < bound and N.err(mine['running_var'], rv) < bound
    assert N.err(g_z, z.grad) < 1e-9        # at M = 2 the gradient is a difference of nearly equal terms
    assert N.err(g_gamma, gamma.grad) < bound and N.err(g_beta, beta.grad) < bound
    if residual:
        assert N.err(g_res, res.grad) < bound
    # the saved statistics are torch's
    assert N.err(mine['mean'], t['z'].mean(0)) < bound and N.err(mine['var'], t['z'].var(0, unbiased=False)) < bound
    assert N.err(mine['invstd'], 1 / torch.sqrt(t['z'].var(0, unbiased=False) + N.EPS)) < bound


def test_an_exact_zero_passes_no_gradient():
    z = torch.tensor([[3.0, 1.0], [3.0, -1.0], [3.0, 2.0]], dtype=torch.float64)
    gamma, beta = torch.tensor([2.0, 1.0], dtype=torch.float64), torch.tensor([0.0, 0.5], dtype=torch.float64)
    f = N.forward(z, gamma, beta, relu=True)
    assert (f['mean'][0] == 3) and (f['var'][0] == 0) and (f['y'][:, 0] == 0).all()
    g_z, g_gamma, g_beta, g_res = N.backward(z, gamma, f['mean'], f['invstd'], f['pre'], torch.ones_like(z), True)
    assert not g_res[:, 0].any() and not g_z[:, 0].any() and g_gamma[0] == 0 and g_beta[0] == 0


@pytest.mark.parametrize('M,C', OFFSET_CASES)
def test_the_offset_case_discriminates(M, C):
    """An uncentred fp32 variance is off by more than 1e-4 on y there, torch's own fp32 stays below 1e-5."""
    t = N.case(M, C, offset=True)
    want = N.forward(t['z'], t['gamma'], t['beta'])['y']
    e_unc = N.err(N.uncentred_y_fp32(t['z'], t['gamma'], t['beta']), want)
    e_torch = N.err(F.batch_norm(t['z'].float(), None, None, t['gamma'].float(), t['beta'].float(), True, 0.0, N.EPS), want)
    print(f'{(M, C)}: uncentred fp32 {e_unc:.3g}, torch fp32 {e_torch:.3g}')
    assert e_unc > 1e-4 and e_torch < 1e-5


def test_cases_find_an_empty_band_well_inside_the_seed_walk():
    shapes = [(2, 1), (2, 5), (18, 65), (7, 4), (63, 3), (65, 64), (129, 130), (8, 2048)]
    assert all(N.case(M, C)['seed_steps'] < 64 for M, C in shapes)
    assert all(N.case(M, C, offset=True)['seed_steps'] < 64 for M, C in OFFSET_CASES)
    assert N.stage_case()['seed_steps'] < 16


def test_stage_on_batch_statistics_vs_float64_autograd():
    case = N.stage_case()
    ref = N.bottleneck_stage_batch(case['x'], case['blocks'], case['stats'], case['g_out'])
    mods = N.stage_module(case, torch.float64)
    bns = N.module_bns(mods)
    with torch.enable_grad():
        x = case['x'].clone().requires_grad_(True)
        out = N.torch_stage(mods, x)
        out.backward(case['g_out'])
    convs = [m for blk in mods for m in [blk.conv1, blk.conv2, blk.conv3] + ([blk.downsample[0]] if hasattr(blk, 'downsample') else [])]
    bound = 1e-10
    assert N.err(ref['out'], out) < bound and N.err(ref['g_x'], x.grad) < bound
    assert len(convs) == len(bns) == len(ref['g_w']) == 7
    for conv, bn, g_w, g_gamma, g_beta, (rm, rv) in zip(convs, bns, ref['g_w'], ref['g_gamma'], ref['g_beta'], ref['running']):
        assert N.err(g_w, conv.weight.grad) < bound and N.err(g_gamma, bn.weight.grad) < bound and N.err(g_beta, bn.bias.grad) < bound
        assert N.err(rm, bn.running_mean) < bound and N.err(rv, bn.running_var) < bound and int(bn.num_batches_tracked) == 1


def test_the_sgd_chain_falls_at_its_rate_and_at_twice_it():
    for rate in (N.SGD_RATE, 2 * N.SGD_RATE):
        losses = N.sgd_losses64(rate)
        print(rate, ' '.join(f'{v:.6f}' for v in losses))
        assert len(losses) == N.SGD_STEPS + 1 and all(b < a for a, b in zip(losses, losses[1:])), (rate, losses)
