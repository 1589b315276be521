"""``specmi_camcalib_loss`` / ``specmi_camcalib_loss_backward`` (spec_amd/csrc/camcalib_bwd.hip) through ``Engine``, against
``specmi_camcalib_eval`` (the forward's bits) and the float64 yardstick of tests/camcalib_grad_ref.py (the gradients).

Bound on Gaussian logits: 1e-5 on max |a - b| / max |b| per tensor, the project's bound for every gradient of the differentiable
tail; the reference's own fp32 autograd is worth 6e-8 .. 3.6e-7 on such inputs (tests/test_camcalib_grad_host.py prints it); the
device measured 4e-8 .. 5.5e-7, and 4.8e-6 on one row whose target lies 0.03 from its soft-argmax (t - s is a difference).
Saturated rows (one-hot first / middle / last, all equal, a span of +-1e4): per row and head, 4 x the error of the reference's
fp32 CPU autograd against float64 on that row (tests/golden/camcalib_loss_grad.npz holds its gradients), or 1e-5 of the row's
largest gradient, whichever is larger.  Measured, fp32 autograd / device: one-hot rows 4.0e-8 /
4.0e-8, all-equal rows 7.0e-7 / 7.7e-7; the span row at 256 / 257 bins (every gradient about 1e-34) 1.0 / 6.6e-8 - the fp32
autograd returns 0 for the whole row, the centred sum keeps it; the span row at 63 .. 65 bins (every gradient about 1e-136, below
fp32's range) 1.0 / 1.0: no fp32 output can hold it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import camcalib_grad_ref as R
from tests import head_ref
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5
BATCHES = (1, 2, 65)


@functools.lru_cache(maxsize=None)
def _engine():
    from spec_amd.engine import Engine
    return Engine('smpl', DEV)          # any handle kind, nothing committed: the calls read nothing of a model


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(B, nbins, lt):
    """The seeded case with its float64 yardstick, computed once and shared."""
    logits, targets = R.loss_case(B, nbins, lt)
    terms, means, grads = R.camcalib_loss(logits, targets, lt)
    return logits, targets, terms, means, grads


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
@pytest.mark.parametrize('nbins', head_ref.NBINS)
@pytest.mark.parametrize('B', BATCHES)
def test_forward_bits_and_gradients_vs_float64(B, nbins, lt):
    eng = _engine()
    logits, targets, terms, means, grads = _case(B, nbins, lt)
    x = _t(logits)
    res = eng.camcalib_loss(x, targets, lt, R.WEIGHTS)
    ev = eng.camcalib_eval(*x, targets, np.zeros((3, B), np.float32), lt, R.WEIGHTS)
    assert torch.equal(res['loss_term'], ev['loss_term']) and torch.equal(res['means'], ev['means'][:4])
    assert R.err(res['means'].cpu().numpy(), means) < BOUND
    g = eng.camcalib_loss_backward(x, targets, lt, R.WEIGHTS, [1.0, 0.0, 0.0, 0.0])
    e = [R.err(g[k].cpu().numpy(), grads[k]) for k in range(3)]
    print(f'B = {B}, nbins = {nbins}, {lt}: vfov {e[0]:.3g}, pitch {e[1]:.3g}, roll {e[2]:.3g}')
    assert max(e) < BOUND, e


@pytest.mark.parametrize('lt', R.LOSS_TYPES)
@pytest.mark.parametrize('nbins', head_ref.NBINS)
def test_saturated_rows(nbins, lt):
    eng = _engine()
    logits, targets = R.saturated_case(nbins, lt)
    _, _, want = R.camcalib_loss(logits, targets, lt)
    fp32 = golden('camcalib_loss_grad.npz')[f'sat{nbins}.{lt}.grads']
    got = np.stack([t.cpu().numpy() for t in eng.camcalib_loss_backward(_t(logits), targets, lt, R.WEIGHTS, [1.0, 0.0, 0.0, 0.0])])
    assert np.isfinite(got).all()
    names = [head_ref.ROW_NAMES[r] for r in R.SATURATED_ROWS]
    worst_ref, worst_dev = [0.0] * len(names), [0.0] * len(names)
    for k in range(3):
        for b in range(logits.shape[1]):
            w = want[k, b]
            top = np.abs(w).max()
            if top == 0:                               # an exactly one-hot row on its target: every gradient is exactly 0
                assert not got[k, b].any(), (k, b)
                continue
            ref_err = float(np.abs(fp32[k, b] - w).max() / top)
            dev_err = float(np.abs(got[k, b] - w).max() / top)
            worst_ref[b], worst_dev[b] = max(worst_ref[b], ref_err), max(worst_dev[b], dev_err)
            assert dev_err <= max(4 * ref_err, BOUND), (k, b, dev_err, ref_err)
    print(f'nbins = {nbins}, {lt}, fp32 CPU autograd / device, of the row\'s largest gradient: ' +
          ', '.join(f'{n} {r:.2g} / {d:.2g}' for n, r, d in zip(names, worst_ref, worst_dev)))


@pytest.mark.parametrize('lt', ('kl', 'softargmax_biased_l2'))
def test_each_entry_of_g_means_selects_its_term(lt):
    eng = _engine()
    B, nbins = 2, 65
    logits, targets, _, _, _ = _case(B, nbins, lt)
    x = _t(logits)
    for j in range(4):
        gm = np.eye(4, dtype=np.float32)[j] * 0.75
        g = eng.camcalib_loss_backward(x, targets, lt, R.WEIGHTS, gm)
        want = R.camcalib_loss(logits, targets, lt, g_means=gm)[2]
        for k in range(3):
            if j == 0 or j == 1 + k:
                assert R.err(g[k].cpu().numpy(), want[k]) < BOUND, (j, k)
            else:
                assert not g[k].any(), (j, k)


@pytest.mark.parametrize('lt', ('ce', 'softargmax_l2'))
def test_a_row_does_not_depend_on_the_other_rows_and_two_runs_agree(lt):
    eng = _engine()
    B, nbins = 65, 257
    logits, targets, _, _, _ = _case(B, nbins, lt)
    gm = [1.0, 0.0, 0.0, 0.0]
    g1 = eng.camcalib_loss_backward(_t(logits), targets, lt, R.WEIGHTS, gm)
    g2 = eng.camcalib_loss_backward(_t(logits), targets, lt, R.WEIGHTS, gm)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    other = logits.copy()
    other[:, 1:] = other[:, 1:][:, ::-1] * 0.5        # every row but the first holds other numbers
    g3 = eng.camcalib_loss_backward(_t(other), targets, lt, R.WEIGHTS, gm)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(g1, g3)) and not torch.equal(g1[0][1], g3[0][1])
    moved = np.roll(logits, 3, axis=1)                # the same rows at other places of the batch (the batch mean keeps B)
    g4 = eng.camcalib_loss_backward(_t(moved), np.roll(targets, 3, axis=1), lt, R.WEIGHTS, gm)
    assert all(torch.equal(torch.roll(a, 3, 0), b) for a, b in zip(g1, g4))


def test_integer_targets_of_any_dtype_and_the_largest_row():
    eng = _engine()
    logits, targets, _, _, grads = _case(2, 256, 'ce')
    x = _t(logits)
    base = eng.camcalib_loss_backward(x, targets, 'ce', R.WEIGHTS, [1.0, 0.0, 0.0, 0.0])
    for dt in (torch.int16, torch.int32, torch.int64, torch.uint8):
        g = eng.camcalib_loss_backward(x, torch.from_numpy(targets).to(dt), 'ce', R.WEIGHTS, [1.0, 0.0, 0.0, 0.0])
        assert all(torch.equal(a, b) for a, b in zip(base, g)), dt
    n = 1 << 16                                        # the largest row the call takes: 1024 trips of the wave
    rng = np.random.default_rng(16)
    big = rng.standard_normal((3, 1, n)).astype(np.float32)
    t = np.array([[0], [n - 1], [n // 2]], np.int64)
    want = R.camcalib_loss(big, t, 'kl')[2]
    g = eng.camcalib_loss_backward(_t(big), t, 'kl', R.WEIGHTS, [1.0, 0.0, 0.0, 0.0])
    assert max(R.err(g[k].cpu().numpy(), want[k]) for k in range(3)) < BOUND


def test_capturable():
    """Neither call allocates in the library: loss and gradient replay from a graph, same bits."""
    eng = _engine()
    logits, targets, _, _, _ = _case(65, 257, 'softargmax_biased_l2')
    x, tg, gm = _t(logits), _t(targets), torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV)

    def step():
        res = eng.camcalib_loss(x, tg, 'softargmax_biased_l2', R.WEIGHTS)
        return [res['loss_term'], res['means'], *eng.camcalib_loss_backward(x, tg, 'softargmax_biased_l2', R.WEIGHTS, gm)]
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


def test_refusals_launch_nothing():
    """Every refusal of include/specmi.h returns SPECMI_ERR_ARG and leaves pre-filled outputs as they were.  Argument checks only:
    every pointer handed over is a good device pointer or NULL."""
    from spec_amd import _lib
    from spec_amd.engine import check_camcalib_loss
    eng = _engine()
    B, n = 2, 8
    x = torch.zeros(3, B, n, device=DEV)
    t = torch.zeros(3, B, dtype=torch.int32, device=DEV)
    gm = torch.ones(4, device=DEV)
    term, means = torch.full((3, B), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV)
    g = torch.full((3, B, n), 7.0, device=DEV)
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())

    def fwd(**kw):
        v = dict(lv=x[0], lp=x[1], lr=x[2], B=B, n=n, lt=0, tv=t[0], tp=t[1], tr=t[2], term=term, means=means)
        v.update(kw)
        return eng.lib.specmi_camcalib_loss(eng.h, ptr(v['lv']), ptr(v['lp']), ptr(v['lr']), v['B'], v['n'], v['lt'], ptr(v['tv']), ptr(v['tp']),
                                            ptr(v['tr']), 1.0, 1.0, 1.0, ptr(v['term']), ptr(v['means']), eng._stream())

    def bwd(**kw):
        v = dict(lv=x[0], lp=x[1], lr=x[2], B=B, n=n, lt=0, tv=t[0], tp=t[1], tr=t[2], gm=gm, gv=g[0], gp=g[1], gr=g[2])
        v.update(kw)
        return eng.lib.specmi_camcalib_loss_backward(eng.h, ptr(v['lv']), ptr(v['lp']), ptr(v['lr']), v['B'], v['n'], v['lt'], ptr(v['tv']),
                                                     ptr(v['tp']), ptr(v['tr']), 1.0, 1.0, 1.0, ptr(v['gm']), ptr(v['gv']), ptr(v['gp']),
                                                     ptr(v['gr']), eng._stream())

    shared = [dict(lv=None), dict(lp=None), dict(lr=None), dict(tv=None), dict(tp=None), dict(tr=None), dict(B=0), dict(B=(1 << 20) + 1),
              dict(n=1), dict(n=(1 << 16) + 1), dict(lt=-1), dict(lt=4)]
    for kw in shared + [dict(term=None), dict(means=None)]:
        assert fwd(**kw) == _lib.ERR_ARG, kw
        assert eng.lib.specmi_last_error(eng.h)
    for kw in shared + [dict(gm=None), dict(gv=None), dict(gp=None), dict(gr=None)]:
        assert bwd(**kw) == _lib.ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((term == 7).all()) and bool((means == 7).all()) and bool((g == 7).all())
    assert fwd() == _lib.OK and bwd() == _lib.OK
    torch.cuda.synchronize()
    assert not bool((g == 7).any()) and not bool((means == 7).any())
    # the wrapper's checks are the library's, stated once
    for args in ((0, 8, 'ce'), ((1 << 20) + 1, 8, 'ce'), (2, 1, 'ce'), (2, (1 << 16) + 1, 'ce')):
        with pytest.raises(ValueError, match='must be in'):
            check_camcalib_loss(*args)
    with pytest.raises(ValueError, match='l2 is not defined'):
        check_camcalib_loss(2, 8, 'l2')
    with pytest.raises(ValueError, match='g_means'):
        check_camcalib_loss(2, 8, 'ce', g_means_shape=(7,))
