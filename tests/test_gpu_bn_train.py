"""``specmi_batchnorm_train_forward`` / ``specmi_batchnorm_backward`` (spec_amd/csrc/bn_train.hip) through the C ABI, against the
float64 reference of tests/bn_ref.py.

Bound 1e-5 on max |a - b| / max |b| per tensor, the project's bound for every gradient of the differentiable tail; for g_z the
error is divided by max |gamma invstd g| instead - the size of the terms that cancel in it (at M = 2 the true g_z is nearly zero,
and torch's own fp32 is off by 1.8e-5 of max |g_z| there: dividing by the gradient's own maximum would test conditioning only).
The offset cases, z ~ N(100, 1), get max(4 e_torch, 1e-5) per tensor, e_torch = the error of torch's fp32 CPU ``F.batch_norm`` on
the same inputs - the rule of ``test_stage_vs_float64``; an uncentred variance is off by about 1e-3 there
(tests/test_bn_ref_host.py).  Measured on an MI355X: DESIGN.md section 7, f-23."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spec_amd import _lib
from tests import bn_ref as N

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5
ROWS = _lib.BN_ROWS_PER_CHUNK
# (M, C): one row pair; a channel tail; rows and channels past one tile's lanes; the vector path at its smallest; M around the
# chunk and its multiples with scalar, vector and mixed channel tiles; layer4's own channel count
SHAPES = [(2, 1), (2, 5), (18, 65), (7, 4), (ROWS - 1, 3), (ROWS + 1, 64), (2 * ROWS + 1, 130), (8, 2048)]
OFFSET_SHAPES = [(513, 4), (4097, 3)]
VARIANTS = [(False, False, False), (True, True, True), (True, False, True), (False, True, False)]       # (relu, residual, running statistics)
F_UPDATE = 0.3


@functools.lru_cache(maxsize=None)
def _engine():
    from spec_amd.engine import Engine
    return Engine('smpl', DEV)          # any handle kind, nothing committed: the calls read nothing of a model


def _d(t):
    return None if t is None else t.float().to(DEV).contiguous()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _case(M, Cn, offset=False):
    """The seeded case, computed once and shared: its float64 tensors and their fp32 device copies."""
    t = N.case(M, Cn, offset=offset)
    return t, {k: _d(v) for k, v in t.items() if isinstance(v, torch.Tensor)}


@functools.lru_cache(maxsize=None)
def _ref(M, Cn, relu, residual, offset=False, f=F_UPDATE):
    t, _ = _case(M, Cn, offset)
    fw = N.forward(t['z'], t['gamma'], t['beta'], N.EPS, t['res'] if residual else None, relu, t['running_mean'], t['running_var'], f)
    g_z, g_gamma, g_beta, g_res = N.backward(t['z'], t['gamma'], fw['mean'], fw['invstd'], fw['pre'], t['g_y'], relu)
    return dict(fw, g_z=g_z, g_gamma=g_gamma, g_beta=g_beta, g_res=g_res, den=float((t['gamma'] * fw['invstd'] * g_res).abs().max()) or 1.0)


def _forward(d, relu, residual, running, f=F_UPDATE, eps=N.EPS):
    """The forward through the C ABI -> dict(y, mean, invstd, running_mean, running_var) (clones of the case's statistics, updated)."""
    eng = _engine()
    M, Cn = d['z'].shape
    o = dict(y=torch.empty_like(d['z']), mean=torch.empty(Cn, device=DEV), invstd=torch.empty(Cn, device=DEV),
             running_mean=d['running_mean'].clone() if running else None, running_var=d['running_var'].clone() if running else None)
    rc = eng.lib.specmi_batchnorm_train_forward(eng.h, _p(d['z']), M, Cn, _p(d['gamma']), _p(d['beta']), _p(d['res'] if residual else None),
                                                int(relu), eps, f, _p(o['running_mean']), _p(o['running_var']), _p(o['y']), _p(o['mean']),
                                                _p(o['invstd']), eng._stream())
    assert rc == 0, eng.lib.specmi_last_error(eng.h)
    return o


def _backward(d, fw, relu, want=(True, True, True, True), g_y=None, alias=False):
    """The backward through the C ABI -> [g_z, g_gamma, g_beta, g_res], None where not wanted; ``alias``: g_res is written over g_y."""
    eng = _engine()
    M, Cn = d['z'].shape
    g_y = (d['g_y'] if g_y is None else g_y).clone()
    outs = [torch.empty_like(d['z']) if want[0] else None, torch.empty(Cn, device=DEV) if want[1] else None,
            torch.empty(Cn, device=DEV) if want[2] else None, (g_y if alias else torch.empty_like(d['z'])) if want[3] else None]
    rc = eng.lib.specmi_batchnorm_backward(eng.h, _p(d['z']), M, Cn, _p(d['gamma']), _p(fw['mean']), _p(fw['invstd']), _p(fw['y'] if relu else None),
                                           int(relu), _p(g_y), *(_p(o) for o in outs), eng._stream())
    assert rc == 0, eng.lib.specmi_last_error(eng.h)
    return outs


def _errors(fw, bw, r, running):
    e = {k: N.err(fw[k], r[k]) for k in ('y', 'mean', 'invstd') + (('running_mean', 'running_var') if running else ())}
    e.update(g_gamma=N.err(bw[1], r['g_gamma']), g_beta=N.err(bw[2], r['g_beta']), g_res=N.err(bw[3], r['g_res']))
    e['g_z'] = float((bw[0].cpu().double() - r['g_z']).abs().max()) / r['den']
    return e


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_outputs_vs_float64(shape):
    _, d = _case(*shape)
    worst = {}
    for relu, residual, running in VARIANTS:
        fw = _forward(d, relu, residual, running)
        bw = _backward(d, fw, relu)
        e = _errors(fw, bw, _ref(*shape, relu, residual), running)
        print(f'{shape} relu={relu} residual={residual} running={running}: ' + ', '.join(f'{k} {v:.3g}' for k, v in e.items()))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
    assert all(v < BOUND for v in worst.values()), worst


@pytest.mark.parametrize('shape', OFFSET_SHAPES, ids=str)
def test_offset_cases_vs_float64_within_four_times_torchs_fp32_error(shape):
    t, d = _case(*shape, True)
    for relu, residual, running in ((False, False, True), (True, True, True)):
        r = _ref(*shape, relu, residual, True)
        with torch.enable_grad():
            z, gamma, beta = (t[k].float().requires_grad_(True) for k in ('z', 'gamma', 'beta'))
            rm, rv = t['running_mean'].float(), t['running_var'].float()
            y = F.batch_norm(z, rm, rv, gamma, beta, True, F_UPDATE, N.EPS)
            y = y + t['res'].float() if residual else y
            y = torch.relu(y) if relu else y
            y.backward(t['g_y'].float())
        e_torch = dict(y=N.err(y, r['y']), running_mean=N.err(rm, r['running_mean']), running_var=N.err(rv, r['running_var']), g_gamma=N.err(gamma.grad, r['g_gamma']),
                       g_beta=N.err(beta.grad, r['g_beta']), g_z=float((z.grad.double() - r['g_z']).abs().max()) / r['den'])
        fw = _forward(d, relu, residual, running)
        e = _errors(fw, _backward(d, fw, relu), r, running)
        for k, v in e.items():
            bound = max(4 * e_torch.get(k, 0.0), BOUND)            # mean, invstd and g_res have no torch counterpart here: the floor alone
            print(f'{shape} relu={relu} {k}: device {v:.3g}, torch fp32 CPU {e_torch.get(k, float("nan")):.3g}, bound {bound:.3g}')
            assert v < bound, (shape, relu, k, v, bound)


def _exact_case(M, Cn, beta0=0.0):
    """Random channels beside channel 0, which is constant: z = 3 there, gamma = 1.5, beta = beta0."""
    t, _ = _case(M, Cn)
    d = {k: _d(v) for k, v in t.items() if isinstance(v, torch.Tensor)}
    d['z'][:, 0] = 3.0
    d['gamma'][0], d['beta'][0] = 1.5, beta0
    return d


@pytest.mark.parametrize('shape', [(7, 4), (ROWS + 1, 64), (2 * ROWS + 1, 130), (513, 3)], ids=str)
def test_a_constant_channel_is_exact(shape):
    d = _exact_case(*shape, beta0=0.25)
    M = shape[0]
    eps32 = float(np.float32(N.EPS))
    for relu, residual in ((False, False), (True, True)):
        fw = _forward(d, relu, residual, True)
        assert float(fw['mean'][0]) == 3.0
        assert fw['invstd'][0].cpu().numpy() == np.float32(1.0 / np.sqrt(eps32))
        want = d['beta'][0] + d['res'][:, 0] if residual else d['beta'][0].expand(M)
        assert torch.equal(fw['y'][:, 0], want.clamp_min(0) if relu else want)
        # the running variance moves towards 0 by the rule, the running mean towards 3: double from fp32 values, rounded once
        f = float(np.float32(F_UPDATE))
        rm0, rv0 = float(d['running_mean'][0]), float(d['running_var'][0])
        assert fw['running_mean'][0].cpu().numpy() == np.float32((1.0 - f) * rm0 + f * 3.0)
        assert fw['running_var'][0].cpu().numpy() == np.float32((1.0 - f) * rv0)
        g_z, g_gamma, g_beta, g_res = _backward(d, fw, relu)
        assert float(g_gamma[0]) == 0.0


@pytest.mark.parametrize('shape', [(7, 4), (2 * ROWS + 1, 130)], ids=str)
def test_an_output_that_is_exactly_zero_passes_no_gradient(shape):
    d = _exact_case(*shape, beta0=0.0)                 # y = beta = 0 on the whole constant channel
    fw = _forward(d, True, False, False)
    assert not fw['y'][:, 0].any()
    g_z, g_gamma, g_beta, g_res = _backward(d, fw, True, g_y=d['g_y'].abs() + 1.0)
    assert not g_res[:, 0].any() and not g_z[:, 0].any() and float(g_gamma[0]) == 0.0 and float(g_beta[0]) == 0.0
    assert g_res[:, 1:].any() and torch.equal(g_res != 0, fw['y'] > 0)


def test_momentum_zero_keeps_the_running_statistics_bits_and_one_replaces_them():
    _, d = _case(ROWS + 1, 64)
    keep = _forward(d, False, False, True, f=0.0)
    assert torch.equal(keep['running_mean'], d['running_mean']) and torch.equal(keep['running_var'], d['running_var'])
    new = _forward(d, False, False, True, f=1.0)
    assert torch.equal(new['running_mean'], new['mean'])
    r = _ref(ROWS + 1, 64, False, False, f=1.0)
    assert N.err(new['running_var'], r['running_var']) < BOUND and not torch.equal(new['running_var'], d['running_var'])
    assert torch.equal(new['y'], keep['y']) and torch.equal(new['invstd'], keep['invstd'])           # the factor touches nothing else


def test_at_two_rows_the_running_variance_carries_the_factor_two():
    z = torch.tensor([[1.0, -2.0, 0.5], [3.0, 2.0, 0.5]], device=DEV)               # var = 1, 4, 0: unbiased 2, 8, 0
    d = dict(z=z, gamma=torch.ones(3, device=DEV), beta=torch.zeros(3, device=DEV), running_mean=torch.zeros(3, device=DEV),
             running_var=torch.full((3,), 4.0, device=DEV))
    fw = _forward(d, False, False, True, f=1.0)
    assert fw['mean'].tolist() == [2.0, 0.0, 0.5] and fw['running_var'].tolist() == [2.0, 8.0, 0.0]
    fw = _forward(d, False, False, True, f=0.5)
    assert fw['running_mean'].tolist() == [1.0, 0.0, 0.25] and fw['running_var'].tolist() == [3.0, 6.0, 2.0]


@pytest.mark.parametrize('shape', [(2 * ROWS + 1, 130), (18, 65), (8, 2048)], ids=str)
def test_two_runs_give_the_same_bits_and_a_wanted_output_does_not_depend_on_the_others(shape):
    _, d = _case(*shape)
    a, b = _forward(d, True, True, True), _forward(d, True, True, True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    bare = _forward(d, True, True, False)                      # without running statistics: the same y, mean, invstd
    assert all(torch.equal(a[k], bare[k]) for k in ('y', 'mean', 'invstd'))
    full = _backward(d, a, True)
    assert all(torch.equal(p, q) for p, q in zip(full, _backward(d, a, True)))
    wants = [tuple(i == j for i in range(4)) for j in range(4)] + [(True, False, False, True), (False, True, True, False)]
    for want in wants:
        got = _backward(d, a, True, want)
        for w, mine, ref in zip(want, got, full):
            assert (mine is None) if not w else torch.equal(mine, ref), want
    assert torch.equal(_backward(d, a, True, alias=True)[3], full[3])                  # g_res written over g_y
    assert torch.equal(_backward(d, a, True, (False, False, False, True), alias=True)[3], full[3])


def test_with_only_g_res_wanted_no_reduction_is_launched():
    eng = _engine()
    _, d = _case(18, 65)
    fw = _forward(d, True, False, False)
    kernels = {}
    for want in ((False, False, False, True), (True, False, False, False), (False, True, False, False)):
        eng.profile(True)
        try:
            _backward(d, fw, True, want)
            kernels[want] = {r['kernel'] for r in eng.profile_read()}
        finally:
            eng.profile(False)
    assert kernels[(False, False, False, True)] == {'bn_bwd_apply'}
    assert kernels[(True, False, False, False)] == {'bn_bwd_reduce', 'bn_bwd_finish', 'bn_bwd_apply'}
    assert kernels[(False, True, False, False)] == {'bn_bwd_reduce', 'bn_bwd_finish'}


def test_unaligned_rows_take_the_scalar_path_with_the_same_bits():
    """C % 4 == 0 but a base pointer that is only 4-byte aligned: the scalar loads, channel for channel the vector path's bits."""
    _, d = _case(ROWS + 1, 64)
    M, Cn = d['z'].shape
    shifted = {}
    for k in ('z', 'res', 'g_y'):
        buf = torch.empty(M * Cn + 1, device=DEV)
        buf[1:].copy_(d[k].reshape(-1))
        shifted[k] = buf[1:].view(M, Cn)
        assert shifted[k].data_ptr() % 16 == 4
    e = dict(d, **shifted)
    a, b = _forward(d, True, True, False), _forward(e, True, True, False)
    assert all(torch.equal(a[k], b[k]) for k in ('y', 'mean', 'invstd'))
    assert all(torch.equal(p, q) for p, q in zip(_backward(d, a, True), _backward(e, a, True)))


def test_refusals_write_nothing_and_leave_the_handle_usable():
    eng = _engine()
    shape = (18, 65)
    _, d = _case(*shape)
    M, Cn = shape
    mk = lambda like: torch.full_like(like, 7.0)
    y, mean, invstd, rm, rv = mk(d['z']), mk(d['gamma']), mk(d['gamma']), mk(d['gamma']), mk(d['gamma'])
    g_z, g_gamma, g_beta, g_res = mk(d['z']), mk(d['gamma']), mk(d['gamma']), mk(d['z'])
    odd = torch.zeros(M * Cn * 4 + 8, dtype=torch.uint8, device=DEV)[1:]        # a float pointer that is not 4-byte aligned
    saved = _forward(d, True, False, False)

    def fwd(**kw):
        v = dict(z=d['z'], M=M, C=Cn, gamma=d['gamma'], beta=d['beta'], res=None, relu=1, eps=N.EPS, f=0.1, rm=rm, rv=rv, y=y, mean=mean, invstd=invstd)
        v.update(kw)
        return eng.lib.specmi_batchnorm_train_forward(eng.h, _p(v['z']), v['M'], v['C'], _p(v['gamma']), _p(v['beta']), _p(v['res']), v['relu'], v['eps'],
                                                      v['f'], _p(v['rm']), _p(v['rv']), _p(v['y']), _p(v['mean']), _p(v['invstd']), eng._stream())

    def bwd(**kw):
        v = dict(z=d['z'], M=M, C=Cn, gamma=d['gamma'], mean=saved['mean'], invstd=saved['invstd'], y=saved['y'], relu=1, g_y=d['g_y'], g_z=g_z,
                 g_gamma=g_gamma, g_beta=g_beta, g_res=g_res)
        v.update(kw)
        return eng.lib.specmi_batchnorm_backward(eng.h, _p(v['z']), v['M'], v['C'], _p(v['gamma']), _p(v['mean']), _p(v['invstd']), _p(v['y']), v['relu'],
                                                 _p(v['g_y']), _p(v['g_z']), _p(v['g_gamma']), _p(v['g_beta']), _p(v['g_res']), eng._stream())
    shapes = [dict(M=1), dict(M=0), dict(M=-3), dict(C=0), dict(C=-1), dict(M=1 << 16, C=1 << 15), dict(M=(1 << 31) - 1, C=1 << 4)]
    refused = [(fwd, kw) for kw in shapes + [dict(z=None), dict(gamma=None), dict(beta=None), dict(y=None), dict(mean=None), dict(invstd=None),
                                             dict(eps=-1e-5), dict(eps=float('nan')), dict(f=-0.1), dict(f=1.5), dict(f=float('nan')),
                                             dict(rm=None), dict(rv=None), dict(z=odd), dict(res=odd), dict(y=odd), dict(gamma=odd), dict(rm=odd),
                                             dict(mean=odd)]]
    refused += [(bwd, kw) for kw in shapes + [dict(z=None), dict(gamma=None), dict(mean=None), dict(invstd=None), dict(g_y=None), dict(y=None),
                                              dict(g_z=None, g_gamma=None, g_beta=None, g_res=None), dict(z=odd), dict(y=odd), dict(g_y=odd),
                                              dict(g_z=odd), dict(g_gamma=odd), dict(g_beta=odd), dict(g_res=odd)]]
    for fn, kw in refused:
        rc = fn(**kw)
        msg = eng.lib.specmi_last_error(eng.h)
        assert rc == 1 and msg, (fn.__name__, kw, rc)              # SPECMI_ERR_ARG with a message
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in (y, mean, invstd, rm, rv, g_z, g_gamma, g_beta, g_res))
    assert fwd(rm=None, rv=None) == 0 and (rm == 7.0).all()         # neither running statistic is fine
    assert bwd(y=None, relu=0) == 0                                # y is not read without relu
    fw = _forward(d, True, True, True)                             # and the handle is still usable
    e = _errors(fw, _backward(d, fw, True), _ref(*shape, True, True), True)
    assert all(v < BOUND for v in e.values()), e


def test_capturable_after_one_eager_call():
    """The workspace grows on the first call of a shape and nothing is allocated afterwards: the second call of the shape is
    captured into a graph (an allocation would invalidate the capture) and replays with the eager call's bits."""
    eng = _engine()
    g = torch.Generator().manual_seed(5)
    M, Cn = 3 * ROWS + 5, 2052                        # more chunk partials than any other shape of this file: the workspace grows here
    d = {k: torch.randn(*s, generator=g).to(DEV) for k, s in (('z', (M, Cn)), ('res', (M, Cn)), ('g_y', (M, Cn)), ('gamma', (Cn,)), ('beta', (Cn,)))}

    def step():
        y, mean, invstd = eng.batchnorm_train_forward(d['z'], d['gamma'], d['beta'], N.EPS, d['res'], True)
        return [y, mean, invstd, *eng.batchnorm_backward(d['z'], d['gamma'], mean, invstd, y, d['g_y'], True, want=(True, True, True, True))]
    eager = step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(out) == 7 and all(torch.equal(a, b) for a, b in zip(eager, out))
    assert N.err(out[1], d['z'].mean(0)) < BOUND and N.err(out[5], out[6].sum(0)) < BOUND          # (and they are the statistics)
