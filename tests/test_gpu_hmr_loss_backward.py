"""``specmi_hmr_loss_backward`` (spec_amd/csrc/loss.hip) and the autograd path of ``spec_amd.losses``: against the gradients of the
reference's own spec/losses.py (tests/golden/hmr_loss_grad.npz, CPU fp32) and against float64 autograd of the restatement
(tests/hmr_loss_grad_ref.py), on the four fixture cases in both modes.  Per tensor max|g - ref| / max|ref| < 1e-5, the bound of the
SMPL backward's tests; a tensor whose reference is all zero must be exactly zero."""
import functools

import numpy as np
import pytest
import torch

from spec_amd import cam_utils
from tests import hmr_loss_grad_ref as G
from tests import hmr_loss_ref as R
from tests.util import golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOUND = 1e-5
SMALL = ('pred_pose', 'pred_shape', 'pred_cam', 'smpl_joints3d', 'smpl_joints2d')
CASES = [(n, m) for n in R.CASES for m in (0, 1)]


@functools.lru_cache(maxsize=None)
def case(name, mode):
    """(pred, gt, weights, float64 gradients of the total) - computed once, left unchanged."""
    pred, gt, weights = R.case_inputs(name, mode)
    return pred, gt, weights, G.grads(mode, pred, gt, weights)[0]


def dev(d):
    return {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in d.items()}


def weight_list(weights):
    w = dict(R.DEFAULT_WEIGHTS, **weights)
    return [w[k] for k in R.WEIGHT_NAMES]


def device_grads(mode, pred, gt, weights, g_means, want=(True,) * 6):
    eng = cam_utils._engine(DEV)
    p, g = dev(pred), dev(gt)
    res = eng.hmr_loss(mode, p, g, weight_list(weights))
    out = eng.hmr_loss_backward(mode, p, g, weight_list(weights), res, g_means, want)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def close(tag, got, want):
    if not np.asarray(want).any():
        assert not got.any(), tag
        return
    e = G.err(got, want)
    print(f'{tag}: {e:.3g}')
    assert e < BOUND, (tag, e)


E6 = [0, 0, 0, 0, 0, 0, 1.0]


@pytest.mark.parametrize('name,mode', CASES)
def test_total_vs_reference_fixture_and_float64(name, mode):
    fx = golden('hmr_loss_grad.npz')
    pred, gt, weights, g64 = case(name, mode)
    got = device_grads(mode, pred, gt, weights, E6)
    for k in SMALL:
        close(f'{name} mode {mode} {k} vs reference', got[k], fx[f'{name}.{mode}.{k}'])
        close(f'{name} mode {mode} {k} vs float64', got[k], g64[k])
    close(f'{name} mode {mode} smpl_vertices vs float64', got['smpl_vertices'], g64['smpl_vertices'])
    B, V = R.CASES[name][:2]
    s, want = G.vertex_summary(got['smpl_vertices'], G.probe(B, V)), fx[f'{name}.{mode}.vertex_summary']
    assert np.array_equal(s[:, 0], want[:, 0])                                       # the same count of non-zeros per image
    assert np.all(np.abs(s[:, 1:3] - want[:, 1:3]) <= BOUND * want[:, 1:3])
    scale = np.abs(g64['smpl_vertices'] * G.probe(B, V)).reshape(B, -1).sum(1)
    assert np.all(np.abs(s[:, 3] - want[:, 3]) <= BOUND * scale)
    assert all(np.isfinite(v).all() for v in got.values())                           # 'masks0': zeros, never NaN
    # a masked-out image gets +0, not -0
    hs = np.asarray(gt['has_smpl']).astype(bool)
    for k in ('pred_pose', 'pred_shape', 'smpl_vertices'):
        assert not np.signbit(got[k][~hs]).any() and not got[k][~hs].any(), k
    assert not got['smpl_joints3d'][:, :25].any() and not got['pred_cam'][:, 1:].any()


@pytest.mark.parametrize('mode', (0, 1))
def test_every_entry_of_g_means_and_linearity(mode):
    name = 'weights'
    pred, gt, weights, _ = case(name, mode)
    basis = []
    for k in range(7):
        e = np.eye(7)[k]
        got, want = device_grads(mode, pred, gt, weights, e), G.grads(mode, pred, gt, weights, g_means=e)[0]
        for key in G.PRED_KEYS:
            close(f'mode {mode} g_means = e{k} {key}', got[key], want[key])
        basis.append(got)
    gm = np.random.default_rng(3).standard_normal(7)
    got, want = device_grads(mode, pred, gt, weights, gm), G.grads(mode, pred, gt, weights, g_means=gm)[0]
    for key in G.PRED_KEYS:
        close(f'mode {mode} random g_means {key}', got[key], want[key])
        lin = sum(c * b[key].astype(np.float64) for c, b in zip(gm, basis))
        close(f'mode {mode} linearity {key}', got[key], lin)


def test_outputs_may_be_null_and_vertices_equal_to_the_ground_truth():
    name, mode = 'mixed', 1
    pred, gt, weights, _ = case(name, mode)
    pred = dict(pred, smpl_vertices=pred['smpl_vertices'].copy())
    pred['smpl_vertices'][0, 5:9] = gt['vertices'][0, 5:9]                           # |x| at exactly 0: slope 0
    full = device_grads(mode, pred, gt, weights, E6)
    gv = full['smpl_vertices']
    assert not gv[0, 5:9].any() and not np.signbit(gv[0, 5:9]).any() and gv[0, 4].all() and gv[0, 9].all()
    for i, k in enumerate(G.PRED_KEYS):
        one = device_grads(mode, pred, gt, weights, E6, want=tuple(j == i for j in range(6)))
        assert [v is not None for v in one.values()] == [j == i for j in range(6)] and np.array_equal(one[k], full[k])
    eng = cam_utils._engine(DEV)
    res = eng.hmr_loss(mode, dev(pred), dev(gt), weight_list(weights))
    with pytest.raises(ValueError):
        eng.hmr_loss_backward(mode, dev(pred), dev(gt), weight_list(weights), res, E6, want=(False,) * 6)


@pytest.mark.parametrize('mode', (0, 1))
def test_modules_backward_fills_the_six_leaves(mode):
    from spec_amd.losses import HMRCamLoss, HMRLoss
    cls = (HMRLoss, HMRCamLoss)[mode]
    name = 'mixed'
    pred, gt, weights, g64 = case(name, mode)
    mod = cls(**weights)
    with torch.no_grad():
        plain, plain_d = mod(dev(pred), dev(gt))
    assert plain.grad_fn is None and not plain.requires_grad
    with torch.enable_grad():
        frozen, _ = mod(dev(pred), dev(gt))                                          # grad enabled, no leaf: nothing changes
        assert frozen.grad_fn is None and torch.equal(frozen, plain)
        leaves = {k: v.requires_grad_(True) for k, v in dev(pred).items()}
        before = leaves['smpl_joints2d'].detach().clone()
        loss, d = mod(leaves, dev(gt))
        assert loss.grad_fn is not None and all(torch.equal(d[k], plain_d[k]) for k in R.KEYS)      # the values: bit for bit today's
        loss.backward()
    assert torch.equal(leaves['smpl_joints2d'].detach(), before)                     # pred is still only read
    for k in G.PRED_KEYS:
        close(f'{cls.__name__}.backward {k}', leaves[k].grad.cpu().numpy(), g64[k])
    with torch.enable_grad():                                                        # one entry of the dict, one leaf
        leaf = dev(pred)['pred_shape'].requires_grad_(True)
        _, d = mod(dict(dev(pred), pred_shape=leaf), dev(gt))
        d['loss/loss_regr_betas'].backward()
    close('loss_regr_betas alone', leaf.grad.cpu().numpy(), G.grads(mode, pred, gt, weights, g_means=np.eye(7)[3])[0]['pred_shape'])


def test_abi_refusals():
    from spec_amd import _lib
    import ctypes as C
    mode, name = 1, 'single'
    pred, gt, weights, _ = case(name, mode)
    eng = cam_utils._engine(DEV)
    p, g = dev(pred), dev(gt)
    wl = weight_list(weights)
    res = eng.hmr_loss(mode, p, g, wl)
    args, B, V = eng._hmr_loss_args(mode, p, g, wl)
    gm = torch.tensor(E6, device=DEV, dtype=torch.float32)
    outs = [torch.full_like(a, 7.0) for a in args[:6]]
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def call(B_=B, terms=res['terms'], counts=res['counts'], gm_=gm, outs_=outs, mode_=mode):
        return eng.lib.specmi_hmr_loss_backward(eng.h, mode_, *(ptr(a) for a in args), B_, V, *(float(w) for w in wl), ptr(terms),
                                                ptr(counts), ptr(gm_), *(ptr(o) for o in outs_), eng._stream())

    assert call(B_=0) == _lib.ERR_ARG and call(terms=None) == _lib.ERR_ARG and call(counts=None) == _lib.ERR_ARG
    assert call(gm_=None) == _lib.ERR_ARG and call(outs_=[None] * 6) == _lib.ERR_ARG and call(mode_=2) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)                                 # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert not bool((outs[4] == 7.0).any())
