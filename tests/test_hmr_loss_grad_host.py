"""The differentiable restatement of the two loss modules (tests/hmr_loss_grad_ref.py) against the gradients the reference's own
spec/losses.py gives under torch.autograd (tests/golden/hmr_loss_grad.npz), on the CPU.

Bound of the fp32 comparison: both sides evaluate the same formulae in fp32, an element of a gradient is a chain of at most
eight roundings (difference, confidence, the factor 2, the normalisations, the weights) times batch scalars that are means of at
most 5 x 6890 x 3 addends accumulated pairwise - about 12 ulp = 7e-7 of the element, hence of the tensor's largest magnitude."""
import json

import numpy as np
import pytest
import torch

from tests import hmr_loss_grad_ref as G
from tests import hmr_loss_ref as R
from tests.util import golden

FP32_BOUND = 1e-6
SMALL = ('pred_pose', 'pred_shape', 'pred_cam', 'smpl_joints3d', 'smpl_joints2d')
CASES = [(n, m) for n in R.CASES for m in (0, 1)]


@pytest.fixture(scope='module')
def fx():
    return golden('hmr_loss_grad.npz')


@pytest.mark.parametrize('name,mode', CASES)
def test_fp32_restatement_matches_the_reference_gradients(fx, name, mode):
    pred, gt, weights = R.case_inputs(name, mode)
    g, vals = G.grads(mode, pred, gt, weights, dtype=torch.float32)
    assert abs(vals[6] - float(fx[f'{name}.{mode}.total'])) <= 8 * R.ulp32(vals[6])
    for k in SMALL:
        want = fx[f'{name}.{mode}.{k}']
        e = G.err(g[k], want)
        print(f'{name} mode {mode} {k}: {e:.3g}')
        assert e < FP32_BOUND, (k, e)
        assert np.array_equal(g[k] == 0, want == 0), k                     # the same elements are exactly zero
    B, V = R.CASES[name][:2]
    got, want = G.vertex_summary(g['smpl_vertices'], G.probe(B, V)), fx[f'{name}.{mode}.vertex_summary']
    assert np.array_equal(got[:, 0], want[:, 0])
    assert np.all(np.abs(got[:, 1:3] - want[:, 1:3]) <= FP32_BOUND * want[:, 1:3])
    scale = np.abs(np.asarray(g['smpl_vertices'], np.float64) * G.probe(B, V)).reshape(B, -1).sum(1)
    assert np.all(np.abs(got[:, 3] - want[:, 3]) <= FP32_BOUND * scale)


@pytest.mark.parametrize('name,mode', CASES)
def test_masked_terms_are_exactly_zero(fx, name, mode):
    pred, gt, weights = R.case_inputs(name, mode)
    g, _ = G.grads(mode, pred, gt, weights)
    hs, hp = np.asarray(gt['has_smpl']).astype(bool), np.asarray(gt['has_pose_3d']).astype(bool)
    for k in ('pred_pose', 'pred_shape', 'smpl_vertices'):
        assert not g[k][~hs].any(), k
        if k != 'smpl_vertices':
            assert not fx[f'{name}.{mode}.{k}'][~hs].any(), k
    assert np.array_equal(fx[f'{name}.{mode}.vertex_summary'][:, 0] > 0, hs & (dict(R.DEFAULT_WEIGHTS, **weights)['shape_loss_weight'] != 0))
    assert not g['smpl_joints3d'][~hp].any() and not g['smpl_joints3d'][:, :25].any()
    assert not fx[f'{name}.{mode}.smpl_joints3d'][~hp].any() and not fx[f'{name}.{mode}.smpl_joints3d'][:, :25].any()
    assert not g['pred_cam'][:, 1:].any()
    assert all(np.isfinite(v).all() for v in g.values())


@pytest.mark.parametrize('name,mode', CASES)
def test_forward_value_is_hmr_loss_ref(name, mode):
    pred, gt, weights = R.case_inputs(name, mode)
    _, vals = G.grads(mode, pred, gt, weights)
    want = R.hmr_loss(mode, pred, gt, weights)
    for v, k in zip(vals, R.KEYS):
        assert abs(v - want[k]) <= 1e-12 * max(abs(want[k]), 1e-30), (k, v, want[k])


def test_any_entry_of_the_loss_dict_may_be_differentiated():
    """d total = loss_weight * the sum of the six: linear in g_means."""
    pred, gt, weights = R.case_inputs('weights', 1)
    tot, _ = G.grads(1, pred, gt, weights)
    parts = [G.grads(1, pred, gt, weights, g_means=np.eye(7)[k])[0] for k in range(6)]
    lw = weights['loss_weight']
    for key in G.PRED_KEYS:
        assert G.err(lw * sum(p[key] for p in parts), tot[key]) < 1e-12


def test_fixture_says_where_it_comes_from(fx):
    meta = json.loads(str(fx['meta']))
    assert 'spec/losses.py' in meta['reference_produced'] and meta['probe_seed'] == G.PROBE_SEED


def test_wrapper_argument_checks():
    from spec_amd.engine import check_hmr_loss_backward
    check_hmr_loss_backward(3, 10, (6, 3), (2,), [False] * 5 + [True])
    for a in ((0, 10, (6, 0), (2,), [True] * 6), (3, 10, (6, 2), (2,), [True] * 6), (3, 10, (6, 3), (3,), [True] * 6),
              (3, 10, (6, 3), (2,), [False] * 6), (3, 10, (6, 3), (2,), [True] * 5)):
        with pytest.raises(ValueError):
            check_hmr_loss_backward(*a)
