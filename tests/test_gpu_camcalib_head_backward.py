"""``specmi_camcalib_head_train_forward`` / ``specmi_camcalib_head_backward`` (spec_amd/csrc/head_bwd.hip) through ``Engine``,
against the float64 chains of tests/camcalib_grad_ref.py.

Bound 1e-5 on max |a - b| / max |b| per tensor, the project's bound for every gradient of the differentiable tail.  The products
are exact-fp32 fma chains of at most 2048 terms cut into four partial sums; the device measured 8e-9 .. 7.5e-7 (DESIGN.md
section 7, f-20)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import camcalib_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5
SMALL = (33, 65, 3, 31, 257)          # three layers, tails in every dimension, two tiles of rows


@functools.lru_cache(maxsize=None)
def _engine():
    from spec_amd.engine import Engine
    return Engine('smpl', DEV)          # any handle kind, nothing committed: the calls read nothing of a model


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The seeded case with its float64 yardstick, computed once and shared."""
    params, xf, g_logits = R.head_case(*shape)
    L = shape[2]
    logits, _ = R.chain_forward(params, xf, L)
    g_xf, grads = R.chain_backward(params, xf, L, g_logits)
    return params, xf, g_logits, logits, g_xf, grads


def _run(params, xf, g_logits, L, want_xf=True, want_params=True, tape=None):
    eng = _engine()
    p = {k: (v if isinstance(v, torch.Tensor) else _t(v)) for k, v in params.items()}
    x, g = _t(xf), _t(g_logits)
    logits, tape = eng.camcalib_head_train_forward(p, x, L, tape=tape)
    g_xf, grads = eng.camcalib_head_backward(p, x, L, tape, g, want_xf=want_xf, want_params=want_params)
    return logits, g_xf, grads


@pytest.mark.parametrize('shape', R.HEAD_SHAPES)
def test_logits_and_gradients_vs_float64(shape):
    params, xf, g_logits, want_logits, want_xf, want = _case(shape)
    logits, g_xf, grads = _run(params, xf, g_logits, shape[2])
    e = {'logits': R.err(logits.cpu().numpy(), want_logits), 'g_xf': R.err(g_xf.cpu().numpy(), want_xf),
         **{n: R.err(grads[n].cpu().numpy(), want[n]) for n in R.param_names(shape[2])}}
    worst = max(e, key=e.get)
    print(f'(B, F, L, Hc, nbins) = {shape}: worst {worst} {e[worst]:.3g}, logits {e["logits"]:.3g}, g_xf {e["g_xf"]:.3g}')
    assert set(grads) == set(want) and all(grads[n].shape == want[n].shape for n in want)
    assert e[worst] < BOUND, e


def test_two_runs_give_the_same_bits_and_a_row_does_not_depend_on_its_batch():
    params, xf, g_logits = _case(SMALL)[:3]
    L = SMALL[2]
    l1, x1, g1 = _run(params, xf, g_logits, L)
    l2, x2, g2 = _run(params, xf, g_logits, L)
    assert torch.equal(l1, l2) and torch.equal(x1, x2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    l3, x3, _ = _run(params, xf[:-1], g_logits[:, :-1], L)            # B and B + 1: 32 rows fill one tile, 33 open a second
    assert torch.equal(l1[:, :-1], l3) and torch.equal(x1[:-1], x3)


def test_a_head_does_not_depend_on_the_other_heads_parameters():
    params, xf, g_logits = _case(SMALL)[:3]
    L = SMALL[2]
    l1, _, g1 = _run(params, xf, g_logits, L)
    for keep in R.HEADS:
        other = {k: (v if k.startswith(keep + '.') else (v * -1.75 + 0.125).astype(np.float32)) for k, v in params.items()}
        l2, _, g2 = _run(other, xf, g_logits, L)
        k = R.HEADS.index(keep)
        assert torch.equal(l1[k], l2[k]) and not torch.equal(l1[(k + 1) % 3], l2[(k + 1) % 3])
        assert all(torch.equal(g1[n], g2[n]) for n in g1 if n.startswith(keep + '.'))
        assert not any(torch.equal(g1[n], g2[n]) for n in g1 if n.endswith('.weight') and not n.startswith(keep + '.'))


def test_a_wanted_output_has_the_same_bits_whatever_else_is_wanted():
    eng = _engine()
    params, xf, g_logits = _case(SMALL)[:3]
    L = SMALL[2]
    names = R.param_names(L)
    _, g_xf, grads = _run(params, xf, g_logits, L)                    # the workspace has grown: the profiled calls below allocate nothing
    eng.profile(True)
    try:
        _, only_xf, none = _run(params, xf, g_logits, L, True, False)
        first = eng.profile_read()
    finally:
        eng.profile(False)
    _, no_xf, only_params = _run(params, xf, g_logits, L, False, True)
    assert none == {} and no_xf is None and torch.equal(only_xf, g_xf)
    assert set(only_params) == set(names) and all(torch.equal(only_params[n], grads[n]) for n in names)
    # one head's last layer only (no data gradient is needed at all), one bias of the first layer, two heads of one layer
    for subset in (('fc_pitch.2.weight',), ('fc_roll.0.bias',), ('fc_vfov.1.weight', 'fc_roll.1.weight'), ('fc_vfov.0.weight', 'fc_pitch.2.bias')):
        _, x, some = _run(params, xf, g_logits, L, False, subset)
        assert x is None and set(some) == set(subset) and all(torch.equal(some[n], grads[n]) for n in subset), subset
    kernels = {r['kernel'] for r in first}
    assert 'cam_head_fwd_gemm' in kernels and 'cam_head_bwd_dgrad_gemm' in kernels, kernels
    assert not any('wgrad' in k or 'bias_grad' in k for k in kernels), kernels


def test_grouped_and_single_launches_give_the_same_bits():
    eng = _engine()
    params, xf, g_logits = _case(SMALL)[:3]
    L = SMALL[2]
    l1, x1, g1 = _run(params, xf, g_logits, L)
    eng.set_option('camcalib_head_group', 0)
    try:
        l2, x2, g2 = _run(params, xf, g_logits, L)
    finally:
        eng.set_option('camcalib_head_group', 1)
    assert torch.equal(l1, l2) and torch.equal(x1, x2) and all(torch.equal(g1[n], g2[n]) for n in g1)


def test_the_tape_is_the_only_state_and_is_not_overrun():
    from spec_amd.engine import camcalib_head_tape_floats
    eng = _engine()
    B, F, L, Hc, nbins = SMALL
    params, xf, g_logits = _case(SMALL)[:3]
    _, x_direct, g_direct = _run(params, xf, g_logits, L)
    n = camcalib_head_tape_floats(B, L, Hc)
    lib_n = C.c_int64(-1)
    assert eng.lib.specmi_camcalib_head_tape_floats(B, F, L, Hc, nbins, C.byref(lib_n)) == 0 and lib_n.value == n == 3 * 2 * B * Hc
    assert eng.lib.specmi_camcalib_head_tape_floats(B, F, 1, 1, nbins, C.byref(lib_n)) == 0 and lib_n.value == 0
    assert eng.lib.specmi_camcalib_head_tape_floats(B, F, 4, Hc, nbins, C.byref(lib_n)) != 0
    p = {k: _t(v) for k, v in params.items()}
    buf = torch.full((n + 1,), 12345.0, device=DEV)
    _, tape = eng.camcalib_head_train_forward(p, _t(xf), L, tape=buf)
    assert tape.data_ptr() == buf.data_ptr() and float(buf[n]) == 12345.0
    other = _case((3, 40, 2, 33, 65))
    _run(*other[:3], 2)                                               # another forward and backward in between, into another tape
    g_xf, grads = eng.camcalib_head_backward(p, _t(xf), L, tape, _t(g_logits))
    assert torch.equal(g_xf, x_direct) and all(torch.equal(grads[k], g_direct[k]) for k in grads)
    assert float(buf[n]) == 12345.0


def test_capturable_after_one_eager_call():
    """Nothing is allocated per call: after one eager call of the shape forward and backward replay from a graph, same bits."""
    eng = _engine()
    params, xf, g_logits = _case(SMALL)[:3]
    L = SMALL[2]
    p, x, g = {k: _t(v) for k, v in params.items()}, _t(xf), _t(g_logits)

    def step():
        logits, tape = eng.camcalib_head_train_forward(p, x, L)
        g_xf, grads = eng.camcalib_head_backward(p, x, L, tape, g)
        return [logits, g_xf, *grads.values()]
    eager = step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(out) == 2 + 6 * L and all(torch.equal(a, b) for a, b in zip(eager, out))


def test_a_strided_feature_tensor_is_read_in_place():
    params, xf, g_logits = _case((3, 40, 2, 33, 65))[:3]
    eng = _engine()
    p = {k: _t(v) for k, v in params.items()}
    wide = torch.full((3, 47), float('nan'), device=DEV)
    wide[:, :40] = _t(xf)
    l1, tape1 = eng.camcalib_head_train_forward(p, wide[:, :40], 2)
    l2, tape2 = eng.camcalib_head_train_forward(p, _t(xf), 2)
    assert torch.equal(l1, l2)
    a = eng.camcalib_head_backward(p, wide[:, :40], 2, tape1, _t(g_logits))
    b = eng.camcalib_head_backward(p, _t(xf), 2, tape2, _t(g_logits))
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


def test_refusals_launch_nothing():
    """Every refusal of include/specmi.h returns SPECMI_ERR_ARG and leaves pre-filled outputs as they were.  Argument checks only:
    every pointer handed over is a good device pointer, NULL, or a good one plus 2 bytes (never dereferenced)."""
    from spec_amd import _lib
    from spec_amd.engine import check_camcalib_head_train
    eng = _engine()
    B, F, L, Hc, nbins = 3, 40, 2, 33, 65
    params, xf, g_logits = _case((B, F, L, Hc, nbins))[:3]
    p = {k: _t(v) for k, v in params.items()}
    names = R.param_names(L)
    x, g = _t(xf), _t(g_logits)
    tape = torch.zeros(3 * B * Hc, device=DEV)
    logits = torch.full((3, B, nbins), 7.0, device=DEV)
    g_xf = torch.full((B, F), 7.0, device=DEV)
    gw = torch.full((Hc, F), 7.0, device=DEV)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    odd = lambda t: C.c_void_p(t.data_ptr() + 2)

    def struct(values):
        st = _lib.CamcalibHeadParams()
        for i, n in enumerate(names):
            if values.get(n) is not None:
                (st.bias if i % 2 else st.weight)[i // (2 * L)][i // 2 % L] = values[n]
        return st

    def pstruct(**kw):
        return struct({n: kw.get(n, p[n].data_ptr()) for n in names})

    def fwd(**kw):
        v = dict(params=C.byref(pstruct()), xf=ptr(x), ld=F, B=B, F=F, L=L, Hc=Hc, n=nbins, tape=ptr(tape), logits=ptr(logits))
        v.update(kw)
        return eng.lib.specmi_camcalib_head_train_forward(eng.h, v['params'], v['xf'], v['ld'], v['B'], v['F'], v['L'], v['Hc'], v['n'],
                                                          v['tape'], v['logits'], eng._stream())

    def bwd(**kw):
        grads = struct({'fc_vfov.0.weight': gw.data_ptr()})
        v = dict(params=C.byref(pstruct()), xf=ptr(x), ld=F, B=B, F=F, L=L, Hc=Hc, n=nbins, tape=ptr(tape), g=ptr(g), g_xf=ptr(g_xf),
                 grads=C.byref(grads))
        v.update(kw)
        return eng.lib.specmi_camcalib_head_backward(eng.h, v['params'], v['xf'], v['ld'], v['B'], v['F'], v['L'], v['Hc'], v['n'], v['tape'],
                                                     v['g'], v['g_xf'], v['grads'], eng._stream())

    big = (1 << 20) + 1
    shared = [dict(L=0), dict(L=4), dict(B=0), dict(B=big), dict(F=0), dict(F=big), dict(Hc=0), dict(Hc=big), dict(n=0), dict(n=big),
              dict(params=None), dict(params=C.byref(pstruct(**{'fc_pitch.1.weight': None}))), dict(params=C.byref(pstruct(**{'fc_roll.0.bias': None}))),
              dict(params=C.byref(pstruct(**{'fc_vfov.0.weight': p['fc_vfov.0.weight'].data_ptr() + 2}))),
              dict(xf=None), dict(xf=odd(x)), dict(tape=None), dict(tape=odd(tape)), dict(ld=F - 1)]
    for kw in shared + [dict(logits=None), dict(logits=odd(logits))]:
        assert fwd(**kw) == _lib.ERR_ARG, kw
        assert eng.lib.specmi_last_error(eng.h)
    none = struct({})
    for kw in shared + [dict(g=None), dict(g=odd(g)), dict(g_xf=None, grads=None), dict(g_xf=None, grads=C.byref(none)), dict(g_xf=odd(g_xf)),
                        dict(grads=C.byref(struct({'fc_vfov.0.weight': gw.data_ptr() + 2})))]:
        assert bwd(**kw) == _lib.ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((logits == 7).all()) and bool((g_xf == 7).all()) and bool((gw == 7).all())
    assert fwd() == _lib.OK and bwd() == _lib.OK                       # the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert not bool((logits == 7).any()) and not bool((g_xf == 7).any()) and not bool((gw == 7).any())
    # the wrapper's checks are the library's, stated once
    for kw in (dict(L=0), dict(L=4), dict(B=0), dict(F=big), dict(Hc=0), dict(nbins=big)):
        a = dict(B=B, F=F, L=L, Hc=Hc, nbins=nbins)
        a.update(kw)
        with pytest.raises(ValueError, match='must be in'):
            check_camcalib_head_train(**a)
    with pytest.raises(ValueError, match='no output is wanted'):
        check_camcalib_head_train(B, F, L, Hc, nbins, outputs=[False] * 13)
    with pytest.raises(ValueError, match='fc_roll.1.bias is missing'):
        check_camcalib_head_train(B, F, L, Hc, nbins, param_shapes={n: v.shape for n, v in params.items() if n != 'fc_roll.1.bias'})
    with pytest.raises(ValueError, match='below the row length'):
        check_camcalib_head_train(B, F, L, Hc, nbins, ld_xf=F - 1)
    with pytest.raises(ValueError, match='no output is wanted'):
        eng.camcalib_head_backward(p, x, L, tape, g, want_xf=False, want_params=False)
