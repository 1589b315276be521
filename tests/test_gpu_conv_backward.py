"""``specmi_conv2d_train_forward`` / ``specmi_conv2d_backward`` (spec_amd/csrc/conv_bwd.hip) through ``Engine``, against the float64
layer of tests/conv_grad_ref.py.

Bound 1e-5 on max |a - b| / max |b| per tensor, the project's bound for every gradient of the differentiable tail.  The products
are exact-fp32 fma chains of at most 1170 terms cut into four partial sums (DESIGN.md section 7, f-22 holds the measured worst)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import conv_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5
VARIANTS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]     # (relu, residual, g_x_add)


@functools.lru_cache(maxsize=None)
def _engine():
    from spec_amd.engine import Engine
    return Engine('smpl', DEV)          # any handle kind, nothing committed: the calls read nothing of a model


def _d(t):
    return None if t is None else t.float().to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _case(shape, exact=False):
    """The seeded case, computed once and shared: its float64 tensors and their fp32 device copies."""
    t = R.layer_case(shape, exact=exact)
    return t, {k: _d(v) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def _ref(shape, relu, residual, add, exact=False):
    t, _ = _case(shape, exact)
    y, z = R.layer_forward(t['x'], t['w'], t['scale'], t['shift'], t['stride'], t['pad'], t['res'] if residual else None, relu)
    return (y, z) + R.layer_backward(t['x'], t['w'], t['scale'], t['stride'], t['pad'], z, t['g_y'], relu, t['g_x_add'] if add else None)


def _run(d, relu, residual, add, want=(True, True, True), g_y=None, alias=False):
    eng = _engine()
    y = eng.conv2d_train_forward(d['x'], d['w'], d['scale'], d['shift'], d['stride'], d['pad'], d['res'] if residual else None, relu)
    g_x_add = d['g_x_add'].clone() if add else None
    g = eng.conv2d_backward(d['x'], d['w'], d['scale'], d['stride'], d['pad'], y, d['g_y'] if g_y is None else g_y, relu, g_x_add, want,
                            g_x_out=g_x_add if alias else None)
    return (y,) + g


@pytest.mark.parametrize('shape', R.LAYER_CASES, ids=str)
def test_outputs_vs_float64(shape):
    _, d = _case(shape)
    worst = {}
    for relu, residual, add in VARIANTS:
        y, g_x, g_w, g_res = _run(d, relu, residual, add)
        ry, _, rgx, rgw, rgres = _ref(shape, relu, residual, add)
        e = {'y': R.err(y, ry), 'g_x': R.err(g_x, rgx), 'g_w': R.err(g_w, rgw), 'g_res': R.err(g_res, rgres)}
        print(f'{shape} relu={relu} residual={residual} g_x_add={add}: ' + ', '.join(f'{k} {v:.3g}' for k, v in e.items()))
        assert g_x.shape == d['x'].shape and g_w.shape == d['w'].shape and g_res.shape == y.shape
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
    assert all(v < BOUND for v in worst.values()), worst


@pytest.mark.parametrize('shape', R.LAYER_CASES, ids=str)
def test_exact_cases_bit_for_bit(shape):
    t, d = _case(shape, True)
    for relu, residual, add in VARIANTS:
        outs = _run(d, relu, residual, add)
        ry, z, rgx, rgw, rgres = _ref(shape, relu, residual, add, True)
        for name, mine, ref in zip(('y', 'g_x', 'g_w', 'g_res'), outs, (ry, rgx, rgw, rgres)):
            assert torch.equal(mine.cpu().double(), ref), (name, relu, residual, add)
    # y == 0 exactly passes no gradient: with g_y nonzero only there, every output is exactly zero
    _, z = _ref(shape, True, True, False, True)[:2]
    assert (z == 0).any()
    g_y = torch.where(z == 0, t['g_y'] + 5.0, torch.zeros_like(z))
    y, g_x, g_w, g_res = _run(d, True, True, False, g_y=_d(g_y))
    assert (y.cpu()[z == 0] == 0).all()
    assert not g_x.any() and not g_w.any() and not g_res.any()


def test_unreached_input_pixels_get_exactly_zero():
    shape = (2, 5, 7, 33, 35, 1, 2)
    _, d = _case(shape)
    _, g_x, _, _ = _run(d, True, False, False)
    assert not g_x[:, 1::2].any() and not g_x[:, :, 1::2].any() and g_x[:, ::2, ::2].abs().min() > 0


@pytest.mark.parametrize('shape', [(2, 6, 5, 33, 32, 3, 2), (33, 1, 1, 8, 8, 1, 1)], ids=str)
def test_two_runs_give_the_same_bits_and_an_image_does_not_depend_on_its_batch(shape):
    _, d = _case(shape)
    a = _run(d, True, True, True)
    b = _run(d, True, True, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    less = {k: (v[:-1].contiguous() if isinstance(v, torch.Tensor) and v.dim() == 4 and k != 'w' else v) for k, v in d.items()}
    y, g_x, g_w, g_res = _run(less, True, True, True)
    assert torch.equal(a[0][:-1], y) and torch.equal(a[1][:-1], g_x) and torch.equal(a[3][:-1], g_res)
    assert not torch.equal(a[2], g_w)


def test_a_wanted_output_has_the_same_bits_whatever_else_is_wanted():
    eng = _engine()
    shape = (2, 6, 5, 33, 32, 3, 2)
    _, d = _case(shape)
    y, g_x, g_w, g_res = _run(d, True, True, True)              # the workspace has grown: the profiled calls below allocate nothing
    kernels = {}
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        eng.profile(True)
        try:
            got = _run(d, True, True, True, want)
            kernels[want] = {r['kernel'] for r in eng.profile_read()}
        finally:
            eng.profile(False)
        for w, mine, full in zip(want, got[1:], (g_x, g_w, g_res)):
            assert (mine is None) if not w else torch.equal(mine, full), want
    assert kernels[(True, False, False)] == {'conv_train_fwd_wt', 'conv_train_fwd_gemm', 'conv_bwd_prep', 'conv_bwd_dgrad_gemm'}
    assert kernels[(False, True, False)] == {'conv_train_fwd_wt', 'conv_train_fwd_gemm', 'conv_bwd_prep', 'conv_bwd_wgrad_gemm'}
    assert kernels[(False, False, True)] == {'conv_train_fwd_wt', 'conv_train_fwd_gemm', 'conv_bwd_prep'}


@pytest.mark.parametrize('shape', [(2, 5, 7, 33, 35, 1, 2), (2, 3, 3, 9, 34, 3, 1)], ids=str)
def test_g_x_add_may_be_g_x_itself(shape):
    _, d = _case(shape)
    a = _run(d, True, False, True)
    b = _run(d, True, False, True, alias=True)
    assert torch.equal(a[1], b[1])


@pytest.mark.parametrize('k,stride', [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_train_forward_vs_the_inference_layer(k, stride):
    """``Engine.conv2d`` (the packed inference kernels) on the same layer at Cin % 32 == 0: other kernels and folds, so within the
    bound and not bit for bit."""
    eng = _engine()
    g = torch.Generator().manual_seed(7 + 10 * k + stride)
    B, H, W, Cin, Cout = 2, 9, 10, 64, 96
    x = torch.randn(B, H, W, Cin, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    scale, shift = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
    oh, ow = R.out_size(H, k, stride, k // 2), R.out_size(W, k, stride, k // 2)
    res = torch.randn(B, oh, ow, Cout, generator=g).to(DEV)
    for relu, r in ((True, res), (False, None)):
        want = eng.conv2d(x, w.numpy(), scale.numpy(), shift.numpy(), stride, k // 2, residual=r, relu=relu)
        got = eng.conv2d_train_forward(x, w.to(DEV), scale.to(DEV), shift.to(DEV), stride, k // 2, r, relu)
        e = R.err(got, want)
        print(f'k={k} stride={stride} relu={relu}: {e:.3g}')
        assert e < BOUND


def test_refusals_write_nothing_and_leave_the_handle_usable():
    eng = _engine()
    shape = (2, 3, 3, 9, 34, 3, 1)
    _, d = _case(shape)
    B, H, W, Cin, Cout, k, stride = shape
    y = torch.full((B, H, W, Cout), 7.0, device=DEV)
    g_x, g_w, g_res = torch.full_like(d['x'], 7.0), torch.full_like(d['w'], 7.0), torch.full_like(y, 7.0)
    odd = torch.zeros(y.numel() * 4 + 8, dtype=torch.uint8, device=DEV)[1:]        # a float pointer that is not 4-byte aligned
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def fwd(**kw):
        v = dict(x=d['x'], B=B, H=H, W=W, Cin=Cin, w=d['w'], scale=d['scale'], shift=d['shift'], Cout=Cout, KH=k, KW=k, stride=stride, pad=1,
                 res=None, y=y)
        v.update(kw)
        return eng.lib.specmi_conv2d_train_forward(eng.h, p(v['x']), v['B'], v['H'], v['W'], v['Cin'], p(v['w']), p(v['scale']), p(v['shift']),
                                                   v['Cout'], v['KH'], v['KW'], v['stride'], v['pad'], p(v['res']), 1, p(v['y']), eng._stream())

    def bwd(**kw):
        v = dict(x=d['x'], B=B, H=H, W=W, Cin=Cin, w=d['w'], scale=d['scale'], Cout=Cout, KH=k, KW=k, stride=stride, pad=1, y=d['res'], relu=1,
                 g_y=d['g_y'], add=None, g_x=g_x, g_w=g_w, g_res=g_res)
        v.update(kw)
        return eng.lib.specmi_conv2d_backward(eng.h, p(v['x']), v['B'], v['H'], v['W'], v['Cin'], p(v['w']), p(v['scale']), v['Cout'], v['KH'],
                                              v['KW'], v['stride'], v['pad'], p(v['y']), v['relu'], p(v['g_y']), p(v['add']), p(v['g_x']),
                                              p(v['g_w']), p(v['g_res']), eng._stream())
    shapes = [dict(KH=3, KW=3, pad=0), dict(KH=1, KW=1, pad=1), dict(KH=5, KW=5, pad=2), dict(KH=3, KW=1), dict(stride=3), dict(stride=0),
              dict(B=0), dict(H=0), dict(W=-1), dict(Cin=0), dict(Cout=0), dict(B=1 << 15, H=1 << 8, W=1 << 8), dict(Cout=1 << 28)]
    refused = [(fwd, kw) for kw in shapes + [dict(x=None), dict(w=None), dict(scale=None), dict(shift=None), dict(y=None), dict(x=odd),
                                             dict(res=odd), dict(y=odd), dict(w=odd)]]
    refused += [(bwd, kw) for kw in shapes + [dict(x=None), dict(w=None), dict(scale=None), dict(g_y=None), dict(y=None),
                                              dict(g_x=None, g_w=None, g_res=None), dict(g_y=odd), dict(g_x=odd), dict(g_w=odd),
                                              dict(g_res=odd), dict(add=odd), dict(y=odd)]]
    for fn, kw in refused:
        rc = fn(**kw)
        msg = eng.lib.specmi_last_error(eng.h)
        assert rc == 1 and msg, (fn.__name__, kw, rc)              # SPECMI_ERR_ARG with a message
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in (y, g_x, g_w, g_res))
    assert bwd(y=None, relu=0) == 0                                # y is not read without relu
    ry, _, rgx, rgw, rgres = _ref(shape, True, False, False)       # and the handle is still usable
    outs = _run(d, True, False, False)
    assert all(R.err(a, b) < BOUND for a, b in zip(outs, (ry, rgx, rgw, rgres)))
