"""The stem's layer shape - 7x7, pad 3, stride 2 - in ``specmi_conv2d_train_forward`` / ``specmi_conv2d_backward``
(spec_amd/csrc/conv_bwd.hip), against the float64 layer of tests/conv_grad_ref.py, which is generic in k.  The cases, the bound
and the same-bits rules are those of tests/test_gpu_conv_backward.py, whose helpers run them; the forward of this shape cuts its
contraction into kernel rows (Kc = 7 Cin), the two gradients run the template's own tap logic."""
import ctypes as C

import pytest
import torch

from tests import conv_grad_ref as R
from tests import trunk_grad_ref as T
from tests.test_gpu_conv_backward import BOUND, DEV, VARIANTS, _case, _engine, _ref, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('shape', T.STEM_CASES, ids=str)
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


@pytest.mark.parametrize('shape', T.STEM_CASES, ids=str)
def test_exact_cases_bit_for_bit(shape):
    _, d = _case(shape, True)
    for relu, residual, add in VARIANTS:
        outs = _run(d, relu, residual, add)
        ry, z, rgx, rgw, rgres = _ref(shape, relu, residual, add, True)
        for name, mine, ref in zip(('y', 'g_x', 'g_w', 'g_res'), outs, (ry, rgx, rgw, rgres)):
            assert torch.equal(mine.cpu().double(), ref), (name, relu, residual, add)


def test_two_runs_give_the_same_bits_and_an_image_does_not_depend_on_its_batch():
    shape = (2, 16, 13, 3, 64, 7, 2)
    _, d = _case(shape)
    a = _run(d, True, True, True)
    b = _run(d, True, True, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    less = {k: (v[:-1].contiguous() if isinstance(v, torch.Tensor) and v.dim() == 4 and k != 'w' else v) for k, v in d.items()}
    y, g_x, g_w, g_res = _run(less, True, True, True)
    assert torch.equal(a[0][:-1], y) and torch.equal(a[1][:-1], g_x) and torch.equal(a[3][:-1], g_res)
    assert not torch.equal(a[2], g_w)


def test_a_wanted_output_has_the_same_bits_whatever_else_is_wanted():
    shape = (2, 9, 11, 3, 5, 7, 2)
    _, d = _case(shape)
    y, g_x, g_w, g_res = _run(d, True, True, True)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        got = _run(d, True, True, True, want)
        for w, mine, full in zip(want, got[1:], (g_x, g_w, g_res)):
            assert (mine is None) if not w else torch.equal(mine, full), want


def test_other_7x7_layers_stay_refused():
    eng = _engine()
    shape = (2, 9, 11, 3, 5, 7, 2)
    _, d = _case(shape)
    B, H, W, Cin, Cout, k, _ = shape
    y = torch.full((B, 5, 6, Cout), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    for stride, pad in ((2, 2), (1, 3), (3, 3), (2, 0)):
        rc = eng.lib.specmi_conv2d_train_forward(eng.h, p(d['x']), B, H, W, Cin, p(d['w']), p(d['scale']), p(d['shift']), Cout, 7, 7, stride, pad,
                                                 None, 1, p(y), eng._stream())
        assert rc == 1 and eng.lib.specmi_last_error(eng.h), (stride, pad)
        rc = eng.lib.specmi_conv2d_backward(eng.h, p(d['x']), B, H, W, Cin, p(d['w']), p(d['scale']), Cout, 7, 7, stride, pad, None, 0, p(d['g_y']),
                                            None, None, p(y), None, eng._stream())
        assert rc == 1 and eng.lib.specmi_last_error(eng.h), (stride, pad)
        with pytest.raises(ValueError):
            eng.conv2d_train_forward(d['x'], d['w'], d['scale'], d['shift'], stride, pad)
    torch.cuda.synchronize()
    assert (y == 7.0).all()
