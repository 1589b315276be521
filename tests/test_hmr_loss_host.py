"""Host side of the loss forward (spec_amd/losses.py, spec/losses.py): the import path, the constructor signatures, the two
stated refusals, and the float64 restatement (tests/hmr_loss_ref.py) against the reference's own fp32 results
(tests/golden/hmr_loss.npz, written by tests/golden/make_hmr_loss_fixture.py from the reference's HMRLoss / HMRCamLoss).

Bound of the restatement (``hmr_loss_ref.format_bound``, from the number format alone): a reduced key of the reference is an fp32
mean of elements of at most five rounded operations each, folded by torch's cascaded sum, times a weight - a handful of half-ulp
roundings, bounded here by 8 ulp(value); loss_cam is ill-conditioned by its formula (the rounding of 10 * cam is amplified by
|10 * cam| ~ 6 .. 11 through exp and doubled by the square) and gets the bound derived there; the total carries the six.  A key
the reference returns as exactly 0 must be exactly 0.  Measured: reduced keys at most 2.73 ulp (keypoints, 'single', HMRCamLoss),
loss_cam at most 4.56 ulp ('single') against a bound of 20.5 ulp, the total at most 2.15 ulp.
"""
import inspect
import json
import os

import numpy as np
import pytest

from tests import hmr_loss_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hmr_loss.npz')


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(GOLDEN))


def fixture_case(fx, name, mode):
    """The case as the fixture stores it: small tensors from the file, the two vertex tensors regenerated from the seed and
    checked against the stored checksum."""
    pred, gt, weights = ref.case_inputs(name, mode)
    assert weights == json.loads(str(fx[f'{name}.weights']))
    assert fx[f'{name}.seed_B_V'].tolist() == [ref.CASE_SEED[name], ref.CASES[name][0], ref.CASES[name][1]]
    chk = np.array([pred['smpl_vertices'].astype(np.float64).sum(), gt['vertices'].astype(np.float64).sum()])
    assert np.array_equal(chk, fx[f'{name}.vertex_checksum']), 'the seeded generator no longer reproduces the fixture inputs'
    small_pred = {k: fx[f'{name}.{k}'] for k in ('pred_pose', 'pred_shape', 'pred_cam', 'smpl_joints3d')}
    small_gt = {k: fx[f'{name}.{k}'] for k in gt if k != 'vertices'}
    pred = dict(small_pred, smpl_joints2d=fx[f'{name}.joints2d{mode}'], smpl_vertices=pred['smpl_vertices'])
    return pred, dict(small_gt, vertices=gt['vertices']), weights


def test_import_path():
    from spec.losses import HMRCamLoss, HMRLoss
    import spec_amd.losses as L
    assert HMRLoss is L.HMRLoss and HMRCamLoss is L.HMRCamLoss
    assert HMRLoss().loss_weight == 60. and HMRCamLoss(beta_loss_weight=0.5).beta_loss_weight == 0.5


def test_constructor_signatures():
    """Names, order and defaults of spec/losses.py:27-39 and :145-155."""
    from spec.losses import HMRCamLoss, HMRLoss
    common = [('shape_loss_weight', 0), ('keypoint_loss_weight', 5.), ('pose_loss_weight', 1.), ('smpl_part_loss_weight', 1.),
              ('beta_loss_weight', 0.001), ('openpose_train_weight', 0.), ('gt_train_weight', 1.), ('loss_weight', 60.)]
    want = {HMRLoss: common + [('estimate_var', False), ('uncertainty_loss', 'MultivariateGaussianNegativeLogLikelihood')],
            HMRCamLoss: common}
    for cls, params in want.items():
        got = [(p.name, p.default) for p in inspect.signature(cls.__init__).parameters.values()][1:]
        assert got == params, cls
        assert all(type(d) is type(w) for (_, d), (_, w) in zip(got, params)), cls          # 0 stays an int, 5. a float
    assert [n for n, _ in common] == list(ref.WEIGHT_NAMES)
    from spec_amd.engine import HMR_LOSS_KEYS, HMR_LOSS_WEIGHTS
    assert HMR_LOSS_WEIGHTS == ref.WEIGHT_NAMES and HMR_LOSS_KEYS == ref.KEYS


def test_stated_refusals():
    from spec.losses import HMRCamLoss, HMRLoss
    with pytest.raises(NotImplementedError, match='criterion slot'):
        HMRLoss(estimate_var=True)
    for cls in (HMRLoss, HMRCamLoss):
        with pytest.raises(NotImplementedError, match='criterion_part'):
            cls()({'pred_segm_rgb': None}, {})


@pytest.mark.parametrize('name', list(ref.CASES))
def test_restatement_meets_the_reference(fx, name):
    for mode in (0, 1):
        pred, gt, weights = fixture_case(fx, name, mode)
        f64 = ref.hmr_loss(mode, pred, gt, weights)
        got = fx[f'{name}.ref{mode}'].astype(np.float64)
        want = np.array([f64[k] for k in ref.KEYS])
        d, bound = np.abs(got - want), ref.format_bound(pred, want, weights, ulps=8)
        nz = want != 0
        print(name, mode, 'distance in fp32 ulp per key:', np.round(d[nz] / ref.ulp32(want[nz]), 2), 'bound:', np.round(bound[nz] / ref.ulp32(want[nz]), 1))
        assert ((got == 0) == (want == 0)).all(), (name, mode, got, want)
        assert (d <= bound).all(), (name, mode, d, bound)


def test_cases_cover_what_they_claim(fx):
    """The zero branches, the mixed masks, the non-default weights: a fixture that stopped exercising them would pass silently."""
    z = fx['masks0.ref1']
    assert (z[1:5] == 0).all() and z[0] > 0 and z[5] > 0
    m = fx['mixed.has_smpl'], fx['mixed.has_pose_3d']
    assert 0 < m[0].sum() < 5 and 0 < m[1].sum() < 5 and (m[0] != m[1]).any()
    w = json.loads(str(fx['weights.weights']))
    assert w['openpose_train_weight'] != 0 and set(w) == set(ref.WEIGHT_NAMES)
    assert (fx['weights.keypoints_orig'][:, :, 2] == 0).any() and (fx['weights.orig_shape'][:, 0] != fx['weights.orig_shape'][:, 1]).all()
    assert (fx['single.ref0'][:4] != fx['single.ref1'][:4]).any()              # the two modules differ on the keypoint term only
    assert np.array_equal(fx['single.ref0'][1:6], fx['single.ref1'][1:6])


def test_rodrigues_is_a_rotation_and_not_smplx_at_the_guard():
    r = np.random.default_rng(3)
    th = r.standard_normal((50, 3))
    th[0] = 0
    R = ref.batch_rodrigues(th)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14 and np.abs(np.linalg.det(R) - 1).max() < 1e-14
    assert np.array_equal(R[0], np.eye(3))
    ang = np.linalg.norm(th[1:], axis=1)
    assert np.abs(np.trace(R[1:], axis1=1, axis2=2) - (1 + 2 * np.cos(ang))).max() < 1e-7
