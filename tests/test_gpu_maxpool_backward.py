"""``specmi_maxpool3x3s2_train_forward`` / ``specmi_maxpool3x3s2_backward`` (spec_amd/csrc/pool_bwd.hip) through ``Engine`` and the
C ABI, against the reference of tests/trunk_grad_ref.py evaluated on the SAME fp32 values.

Everything is compared bit for bit: the forward selects one of its inputs, and the backward adds at most four fp32 values in
double and rounds once, exactly what the float64 reference does in the same order (no case here has addends more than 29 binary
orders apart, the one way a double sum of four floats could round).  ``y`` is compared with ``Engine.maxpool``'s bits where
C % 4 == 0 only - the inference kernel takes whole 4-channel vectors and refuses (1, 1, 1, 1) and (2, 5, 7, 5) - and with the
reference, which is the same selection of an input value, on every shape."""
import ctypes as C
import functools

import pytest
import torch

from tests import trunk_grad_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _engine():
    from spec_amd.engine import Engine
    return Engine('smpl', DEV)          # any handle kind, nothing committed: the calls read nothing of a model


@functools.lru_cache(maxsize=None)
def _case(shape):
    """fp32 inputs (CPU), computed once and shared: x random / post-ReLU with at least half zeros / constant, integer and float g_y,
    and the reference's y, idx for each x."""
    B, H, W, Cn = shape
    g = torch.Generator().manual_seed(11 + sum(shape))
    x = torch.randn(*shape, generator=g)
    xs = {'random': x, 'relu': torch.relu(x - 0.3), 'constant': torch.full(shape, 1.5)}
    fw = {k: T.maxpool_forward(v.double()) for k, v in xs.items()}
    oshape = fw['random'][0].shape
    return dict(x=xs, fw=fw, g_int=torch.randint(-3, 4, oshape, generator=g).float(), g_float=torch.randn(oshape, generator=g))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _shifted(t):
    """A dense copy of t whose pointer is one element past a 256-byte boundary: 4-byte aligned floats, odd uint8 addresses."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize('shape', T.POOL_CASES, ids=str)
def test_forward_values_and_winning_taps(shape):
    eng, c = _engine(), _case(shape)
    B, H, W, Cn = shape
    for name, x in c['x'].items():
        y, idx = eng.maxpool_train_forward(x.to(DEV))
        ry, ridx = c['fw'][name]
        assert idx.dtype == torch.uint8 and idx.shape == y.shape == ry.shape
        assert torch.equal(y.cpu().double(), ry), name
        assert torch.equal(idx.cpu(), ridx), name
        if Cn % 4 == 0:                                             # the inference kernel takes whole vectors only
            assert torch.equal(y, eng.maxpool(x.to(DEV))), name
        # border windows: a padding tap is never named
        k = idx.cpu().long()
        ky, kx = k // 3, k % 3
        oy = torch.arange(y.shape[1]).view(1, -1, 1, 1)
        ox = torch.arange(y.shape[2]).view(1, 1, -1, 1)
        iy, ix = oy * 2 - 1 + ky, ox * 2 - 1 + kx
        assert int(k.max()) <= 8 and bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()), name
    if B * H * W * Cn > 100:
        assert (c['x']['relu'] == 0).float().mean() >= 0.5


@pytest.mark.parametrize('shape', T.POOL_CASES, ids=str)
def test_backward_bit_for_bit(shape):
    eng, c = _engine(), _case(shape)
    B, H, W, Cn = shape
    for name, x in c['x'].items():
        ridx = c['fw'][name][1]
        _, idx = eng.maxpool_train_forward(x.to(DEV))
        for kind in ('g_int', 'g_float'):
            g_y = c[kind]
            g_x = eng.maxpool_backward(g_y.to(DEV), idx, H, W)
            ref = T.maxpool_backward(g_y.double(), ridx, H, W)
            assert g_x.shape == x.shape
            assert torch.equal(g_x.cpu(), ref.float()), (name, kind)          # the float64 sum rounded once
            if kind == 'g_int':
                assert torch.equal(g_x.cpu().double(), ref)
                assert torch.equal(g_x.sum((0, 1, 2)).cpu(), g_y.sum((0, 1, 2))), name      # nothing lost, nothing counted twice
    # the constant tensor: the first in-range tap wins every window, so only pixels with even (iy, ix) (and row / column 0) win
    _, idx = eng.maxpool_train_forward(c['x']['constant'].to(DEV))
    g_x = eng.maxpool_backward(torch.ones_like(c['g_int']).to(DEV), idx, H, W).cpu()
    assert torch.equal(g_x != 0, T.maxpool_backward(torch.ones_like(c['g_int']).double(), c['fw']['constant'][1], H, W) != 0)


@pytest.mark.parametrize('shape', [(2, 6, 4, 64), (1, 7, 9, 68), (1, 2, 2, 4)], ids=str)
def test_the_vector_and_the_scalar_form_give_the_same_bits(shape):
    eng, c = _engine(), _case(shape)
    B, H, W, Cn = shape
    for name in ('random', 'relu'):
        x = c['x'][name].to(DEV)
        y, idx = eng.maxpool_train_forward(x)
        g_y = c['g_float'].to(DEV)
        g_x = eng.maxpool_backward(g_y, idx, H, W)
        assert x.data_ptr() % 16 == 0 and g_y.data_ptr() % 16 == 0 and idx.data_ptr() % 4 == 0
        y2, idx2 = eng.maxpool_train_forward(_shifted(x))
        assert torch.equal(y, y2) and torch.equal(idx, idx2)
        # the backward's scalar form, reached through the floats and through idx alone
        assert torch.equal(g_x, eng.maxpool_backward(_shifted(g_y), idx, H, W))
        assert torch.equal(g_x, eng.maxpool_backward(g_y, _shifted(idx), H, W))
        # and the forward's through its outputs: y and idx one element past alignment
        yb, ib = _shifted(torch.zeros_like(y)), _shifted(torch.zeros_like(idx))
        assert eng.lib.specmi_maxpool3x3s2_train_forward(eng.h, _p(x), B, H, W, Cn, _p(yb), _p(ib), eng._stream()) == 0
        assert torch.equal(y, yb) and torch.equal(idx, ib)


def test_every_element_of_g_x_is_written_once():
    eng, shape = _engine(), (2, 5, 7, 5)
    c = _case(shape)
    B, H, W, Cn = shape
    _, idx = eng.maxpool_train_forward(c['x']['relu'].to(DEV))
    g_y = c['g_float'].to(DEV)
    g_x = torch.full(shape, 7.0, device=DEV)
    assert eng.lib.specmi_maxpool3x3s2_backward(eng.h, _p(g_y), _p(idx), B, H, W, Cn, _p(g_x), eng._stream()) == 0
    want = eng.maxpool_backward(g_y, idx, H, W)
    assert torch.equal(g_x, want) and (want == 0).any() and not (want == 7.0).any()
    # an idx that names no tap of its window passes no gradient and breaks nothing
    assert not eng.maxpool_backward(g_y, torch.full_like(idx, 200), H, W).any()


@pytest.mark.parametrize('shape', [(2, 5, 7, 5), (2, 6, 4, 64)], ids=str)
def test_two_runs_give_the_same_bits_and_an_image_does_not_depend_on_its_batch(shape):
    eng, c = _engine(), _case(shape)
    B, H, W, Cn = shape
    x, g_y = c['x']['relu'].to(DEV), c['g_float'].to(DEV)

    def run(x, g_y):
        y, idx = eng.maxpool_train_forward(x)
        return y, idx, eng.maxpool_backward(g_y, idx, H, W)
    a, b = run(x, g_y), run(x, g_y)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    less = run(x[:-1].contiguous(), g_y[:-1].contiguous())
    assert all(torch.equal(p[:-1], q) for p, q in zip(a, less))


def test_a_nan_follows_torch():
    eng, shape = _engine(), (1, 7, 9, 68)
    x = _case(shape)['x']['random'].clone()
    x[0, 3, 4, 1] = float('nan')
    x[0, 0, 0, 66] = float('nan')            # in the scalar tail of nothing: C % 4 == 0, lane 2 of the last vector
    x[0, 6, 8, 67] = float('nan')
    ry, ridx = T.maxpool_forward(x.double())
    ty, _ = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    for xin in (x.to(DEV), _shifted(x.to(DEV))):
        y, idx = eng.maxpool_train_forward(xin)
        assert torch.equal(torch.isnan(y.cpu()), torch.isnan(ty.permute(0, 2, 3, 1))) and int(torch.isnan(y).sum()) == 4
        assert torch.equal(torch.nan_to_num(y.cpu(), nan=-5.0).double(), torch.nan_to_num(ry, nan=-5.0))
        assert torch.equal(idx.cpu(), ridx)


def test_capturable():
    """No workspace, nothing allocated by the library: the two calls replay from a graph with the same bits."""
    eng, shape = _engine(), (2, 6, 4, 64)
    c = _case(shape)
    B, H, W, Cn = shape
    x, g_y = c['x']['relu'].to(DEV), c['g_float'].to(DEV)

    def step():
        y, idx = eng.maxpool_train_forward(x)
        return [y, idx, eng.maxpool_backward(g_y, idx, H, W)]
    eager = step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, out))


def test_refusals_write_nothing_and_leave_the_handle_usable():
    eng, shape = _engine(), (2, 5, 7, 5)
    c = _case(shape)
    B, H, W, Cn = shape
    x, g_y = c['x']['random'].to(DEV), c['g_float'].to(DEV)
    y = torch.full(g_y.shape, 7.0, device=DEV)
    idx = torch.full(g_y.shape, 77, dtype=torch.uint8, device=DEV)
    g_x = torch.full(shape, 7.0, device=DEV)
    odd = torch.zeros(x.numel() * 4 + 8, dtype=torch.uint8, device=DEV)[1:]         # a float pointer that is not 4-byte aligned

    def fwd(**kw):
        v = dict(x=x, B=B, H=H, W=W, C=Cn, y=y, idx=idx)
        v.update(kw)
        return eng.lib.specmi_maxpool3x3s2_train_forward(eng.h, _p(v['x']), v['B'], v['H'], v['W'], v['C'], _p(v['y']), _p(v['idx']), eng._stream())

    def bwd(**kw):
        v = dict(g_y=g_y, idx=idx, B=B, H=H, W=W, C=Cn, g_x=g_x)
        v.update(kw)
        return eng.lib.specmi_maxpool3x3s2_backward(eng.h, _p(v['g_y']), _p(v['idx']), v['B'], v['H'], v['W'], v['C'], _p(v['g_x']), eng._stream())
    dims = [dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(B=1 << 15, H=1 << 8, W=1 << 8)]
    refused = [(fwd, kw) for kw in dims + [dict(x=None), dict(y=None), dict(idx=None), dict(x=odd), dict(y=odd)]]
    refused += [(bwd, kw) for kw in dims + [dict(g_y=None), dict(idx=None), dict(g_x=None), dict(g_y=odd), dict(g_x=odd)]]
    for fn, kw in refused:
        rc = fn(**kw)
        assert rc == 1 and eng.lib.specmi_last_error(eng.h), (fn.__name__, kw, rc)          # SPECMI_ERR_ARG with a message
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (idx == 77).all() and (g_x == 7.0).all()
    assert fwd() == 0 and bwd() == 0                                                        # and the handle is still usable
    assert torch.equal(y.cpu().double(), c['fw']['random'][0]) and torch.equal(idx.cpu(), c['fw']['random'][1])
