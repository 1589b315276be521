"""``specmi_hmr_head_train_forward`` / ``specmi_hmr_head_backward`` (spec_amd/csrc/head_bwd.hip) through ``Engine``, against the
float64 restatement of tests/head_grad_ref.py.

Bound 1e-5 on max |a - b| / max |b| per tensor, the project's bound for every gradient of the differentiable tail.  The
reference's own fp32 arithmetic (CPU torch autograd of oracle.heads.HMRHead) is worth 2.9e-7 .. 5.2e-7 on these cases
(tests/test_head_grad_host.py prints it); the device measured 9e-8 .. 9.7e-7."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import head_grad_ref as R
from tests import smpl_grad_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5


@functools.lru_cache(maxsize=None)
def _engine():
    from spec_amd.engine import Engine
    return Engine('smpl', DEV)          # any handle kind, nothing committed: the calls read nothing of a model


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _args(c, rows=None):
    """The device arguments of case ``c`` (rows: a slice of the batch)."""
    sl = slice(None) if rows is None else rows
    return {'params': {k: _t(v) for k, v in c['params'].items()}, 'xf': _t(c['xf'][sl]), 'init_state': _t(c['init_state'][sl]),
            'cam_feats': _t(None if c['cam_feats'] is None else c['cam_feats'][sl]),
            'masks': _t(None if c['masks'] is None else c['masks'][:, sl]), 'p': 0.5 if c['p'] is None else c['p'], 'n_iter': c['n_iter'],
            'g_state': _t(c['g_state'][sl])}


def _run(a, want_xf=True, want_params=True, tape=None):
    eng = _engine()
    state, tape = eng.hmr_head_train_forward(a['params'], a['xf'], a['init_state'], a['cam_feats'], a['masks'], a['p'], a['n_iter'], tape=tape)
    g_xf, grads = eng.hmr_head_backward(a['params'], a['xf'], tape, a['g_state'], a['cam_feats'], a['masks'], a['p'], a['n_iter'],
                                        want_xf=want_xf, want_params=want_params)
    return state, g_xf, grads


@pytest.mark.parametrize('F,B,cam,n_iter,p', R.variants())
def test_state_and_gradients_vs_float64(F, B, cam, n_iter, p):
    c = R.case(F, B, cam, n_iter, p)
    state, g_xf, grads = _run(_args(c))
    e = {'state': S.err(state.cpu().numpy(), c['state']), 'g_xf': S.err(g_xf.cpu().numpy(), c['g_xf']),
         **{n: S.err(grads[n].cpu().numpy(), c['grads'][n]) for n in R.NAMES}}
    worst = max(e, key=e.get)
    print(f'F = {F}, B = {B}, cam = {cam}, n_iter = {n_iter}, p = {p}: worst {worst} {e[worst]:.3g}, state {e["state"]:.3g}, g_xf {e["g_xf"]:.3g}')
    assert e[worst] < BOUND, e


def test_a_wanted_output_has_the_same_bits_whatever_else_is_wanted():
    eng = _engine()
    a = _args(R.case(40, 70, True, 3, 0.5))
    _run(a)                                                       # the workspace has grown: the profiled calls below allocate nothing
    eng.profile(True)
    try:
        _, only_xf, none = _run(a, True, False)
        first = eng.profile_read()
    finally:
        eng.profile(False)
    _, no_xf, only_params = _run(a, False, True)
    _, g_xf, grads = _run(a, True, True)
    _, _, two = _run(a, False, ('fc2.bias', 'deccam.weight'))
    assert none == {} and no_xf is None
    assert torch.equal(only_xf, g_xf)
    assert set(only_params) == set(grads) == set(R.NAMES) and all(torch.equal(only_params[n], grads[n]) for n in R.NAMES)
    assert set(two) == {'fc2.bias', 'deccam.weight'} and all(torch.equal(two[n], grads[n]) for n in two)
    kernels = {r['kernel'] for r in first}
    assert 'head_train_fwd_gemm' in kernels and 'head_bwd_dgrad_gemm' in kernels, kernels
    assert not any('wgrad' in k or 'bias_grad' in k for k in kernels), kernels


def test_two_runs_give_the_same_bits_and_a_row_does_not_depend_on_its_batch():
    c = R.case(40, 70, True, 3, 0.5)
    a = _args(c)
    s1, x1, g1 = _run(a)
    s2, x2, g2 = _run(a)
    assert torch.equal(s1, s2) and torch.equal(x1, x2) and all(torch.equal(g1[n], g2[n]) for n in R.NAMES)
    s3, x3, _ = _run(_args(c, slice(0, 3)))
    assert torch.equal(s1[:3], s3) and torch.equal(x1[:3], x3)


def test_the_tape_is_the_only_state_and_is_not_overrun():
    from spec_amd.engine import hmr_head_tape_floats
    eng = _engine()
    ca, cb = R.case(40, 70, True, 3, 0.5), R.case(40, 3, False, 3, 0.5)
    a, b = _args(ca), _args(cb)
    _, x_direct, g_direct = _run(a)
    n = hmr_head_tape_floats(70, 3)
    lib_n = C.c_int64(0)
    assert eng.lib.specmi_hmr_head_tape_floats(70, 40, 7, 3, C.byref(lib_n)) == 0 and lib_n.value == n
    buf = torch.full((n + 1,), 12345.0, device=DEV)
    _, tape_a = eng.hmr_head_train_forward(a['params'], a['xf'], a['init_state'], a['cam_feats'], a['masks'], a['p'], 3, tape=buf)
    assert tape_a.data_ptr() == buf.data_ptr() and float(buf[n]) == 12345.0
    _run(b)                                                        # another forward and backward in between, into another tape
    g_xf, grads = eng.hmr_head_backward(a['params'], a['xf'], tape_a, a['g_state'], a['cam_feats'], a['masks'], a['p'], 3)
    assert torch.equal(g_xf, x_direct) and all(torch.equal(grads[k], g_direct[k]) for k in R.NAMES)
    assert float(buf[n]) == 12345.0


def test_refusals_launch_nothing():
    """Every refusal of include/specmi.h returns SPECMI_ERR_ARG and leaves pre-filled outputs as they were.  Argument checks only:
    every pointer handed over is a good device pointer, NULL, or a good one plus 2 bytes (never dereferenced)."""
    from spec_amd import _lib
    eng = _engine()
    c = R.case(40, 3, True, 3, 0.5)
    a = _args(c)
    B, F = 3, 40
    tape = torch.zeros(3 * B * (157 + 2048), device=DEV)
    state = torch.full((B, 157), 7.0, device=DEV)
    g_xf = torch.full((B, F), 7.0, device=DEV)
    gw = torch.full((1024, 1024), 7.0, device=DEV)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    odd = lambda t: C.c_void_p(t.data_ptr() + 2)

    def params(**kw):
        return _lib.HmrHeadParams(*(kw[n] if n in kw else a['params'][n].data_ptr() for n in _lib.HMR_HEAD_PARAMS))

    def fwd(**kw):
        v = dict(params=C.byref(params()), xf=ptr(a['xf']), ld=F, cf=ptr(a['cam_feats']), init=ptr(a['init_state']), masks=ptr(a['masks']),
                 p=0.5, B=B, F=F, C=7, n=3, state=ptr(state), tape=ptr(tape))
        v.update(kw)
        return eng.lib.specmi_hmr_head_train_forward(eng.h, v['params'], v['xf'], v['ld'], v['cf'], v['init'], v['masks'], v['p'], v['B'],
                                                     v['F'], v['C'], v['n'], v['state'], v['tape'], eng._stream())

    def bwd(**kw):
        grads = _lib.HmrHeadParams(**{'fc2_weight': gw.data_ptr()})
        v = dict(params=C.byref(params()), xf=ptr(a['xf']), ld=F, cf=ptr(a['cam_feats']), masks=ptr(a['masks']), p=0.5, B=B, F=F, C=7, n=3,
                 tape=ptr(tape), g=ptr(a['g_state']), g_xf=ptr(g_xf), grads=C.byref(grads))
        v.update(kw)
        return eng.lib.specmi_hmr_head_backward(eng.h, v['params'], v['xf'], v['ld'], v['cf'], v['masks'], v['p'], v['B'], v['F'], v['C'],
                                                v['n'], v['tape'], v['g'], v['g_xf'], v['grads'], eng._stream())

    shared = [dict(B=0), dict(F=0), dict(C=3), dict(n=0), dict(n=4), dict(p=1.0), dict(p=-0.25), dict(params=None),
              dict(params=C.byref(params(**{'decshape.bias': None}))), dict(xf=None), dict(tape=None), dict(cf=None),
              dict(xf=odd(a['xf'])), dict(params=C.byref(params(**{'fc1.weight': a['params']['fc1.weight'].data_ptr() + 2}))),
              dict(tape=odd(tape)), dict(ld=F - 1)]
    for kw in shared + [dict(init=None), dict(state=None), dict(state=odd(state)), dict(init=odd(a['init_state']))]:
        assert fwd(**kw) == _lib.ERR_ARG, kw
        assert eng.lib.specmi_last_error(eng.h)
    for kw in shared + [dict(g=None), dict(g=odd(a['g_state'])), dict(g_xf=None, grads=None), dict(g_xf=odd(g_xf)),
                        dict(g_xf=None, grads=C.byref(_lib.HmrHeadParams()))]:
        assert bwd(**kw) == _lib.ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((g_xf == 7.0).all()) and bool((gw == 7.0).all()) and bool((tape == 0).all())
    # and the same argument blocks, unmodified, are accepted
    assert fwd() == _lib.OK and bwd() == _lib.OK
    torch.cuda.synchronize()
    assert S.err(state.cpu().numpy(), c['state']) < BOUND and S.err(gw.cpu().numpy(), c['grads']['fc2.weight']) < BOUND
