"""The validation-step scores without a GPU: tests/eval_step_ref.py (the float64 yardstick of tests/test_gpu_eval_step.py)
reproduces the reference's functions when cast to their float32 data flow and passes its own rule on every input the GPU test
uses; ``engine.check_eval_step`` makes every refusal of ``specmi_eval_step``; ``EvalDataset.eval_gt`` chooses the pose key;
``EvalDump`` carries the four per-joint arrays; the five lines and the json have the reference's layout."""
import json
import os

import numpy as np
import pytest

from tests import eval_step_ref as R
from tests import metrics_ref as M


# ---- the yardstick -------------------------------------------------------------------------------------------------------------

def test_float32_flow_equals_the_restated_pare_functions():
    """In float32 the restatement equals ``oracle.metrics.reconstruction_error(..., reduction=None)[1]`` and
    ``compute_error_verts`` on random bodies (parity with the restated pare functions, not pinned against pare itself).

    Bound on a joint's aligned error, from fp32 roundoff alone.  Both sides run the same algorithm on the same float32 joints
    (the oracle keeps Z in float64, so R, the scale and the transformed points are float64 there and float32 here); the aligned
    point moves by at most the coordinate scale c = max |coordinate| times the relative error of s R, plus its own roundings:
    N 2^-24 for the N-term sums of the means, var1 and K (worst case, each term rounded once), about 10 x 2^-24 for LAPACK's 3x3
    SVD (backward stable, ||dK|| <= p(3) eps ||K||; the rotation's sensitivity to K is 1 / (sigma_i + sigma_j), which is O(1 / ||K||)
    for these bodies: 30 cm of spread in every direction against 3 cm of noise), 9 for the two 3x3 products and the trace, 3 per
    coordinate of the final product, the translation and the distance.  (N + 40) 2^-24 c covers the sum with room for the
    distance's own square root; with c about 1.5 m and N = 24 that is 6 micrometres; the aligned errors themselves are
    asserted to be 20 times that and more.
    V2V: identical operations on identical float32 inputs, pairwise summation on both sides - (log2(V) + 4) 2^-24 relative covers
    any difference in how NumPy blocks the two reductions."""
    from oracle import metrics as OM
    pred, gt, Jr, pj, gj = R.random_bodies(5, 700, 1)
    for p, g in (R.regressed_aligned(pred, gt, Jr, M.H36M_TO_J14, np.float32), (pj - pj[:, :1], gj - gj[:, :1])):
        assert p.dtype == np.float32 and g.dtype == np.float32
        _, pk, ph = R.aligned_per_joint(p, g, np.float32)
        _, ref = OM.reconstruction_error(p, g, reduction=None)
        c = max(np.abs(p).max(), np.abs(g).max())
        bound = (p.shape[1] + 40) * M.U24 * c
        assert ref.shape == pk.shape and ref.min() > 20 * bound
        assert np.abs(pk - ref).max() <= bound, (np.abs(pk - ref).max(), bound)
        assert np.abs(ph - ref).max() <= bound, (np.abs(ph - ref).max(), bound)
        _, pk64, ph64 = R.aligned_per_joint(p, g)
        assert np.abs(pk64 - ref).max() <= bound and np.abs(pk64 - ph64).max() < 1e-12
    v32, ref = R.raw_v2v(pred, gt, np.float32), OM.compute_error_verts(pred_verts=pred, target_verts=gt)
    assert np.all(np.abs(v32 - ref) <= (np.log2(pred.shape[1]) + 4) * M.U24 * ref)
    assert np.all(np.abs(R.raw_v2v(pred, gt) - ref) <= (np.log2(pred.shape[1]) + 4) * M.U24 * ref)


def _own_rule(err, pk, ph, what):
    why = R.check_per_joint(err.astype(np.float32), pk.astype(np.float32), err, pk, ph)
    assert why is None, (what, why)


def test_the_yardstick_passes_its_own_rule_on_the_gpu_inputs():
    """Rounded to float32 the yardstick passes ``check_per_joint`` on every input of the exact-regression sweep (the regression is
    exact there: checked in the flesh) and of the Procrustes families."""
    exact = set()
    for V, J, B, sel, Jk in R.sweep():
        pred, gt, Jr = R.mesh(V, J, B)
        if (V, J, B) not in exact:
            M.assert_exact_sums(pred, Jr), M.assert_exact_sums(gt, Jr)
            exact.add((V, J, B))
        if Jk == R.STEP_JK[0]:
            _own_rule(*R.mesh_per_joint(pred, gt, Jr, sel), (V, J, B, len(sel)))
        if len(sel) == 1:
            _own_rule(*R.given_per_joint(*R.dyadic_joints(B, Jk)), (B, Jk))
    for name, (p, g, expect) in M.procrustes_cases().items():
        err, pk, ph = R.given_per_joint(p, g)
        if expect == 'range':
            continue                                    # no unique per-joint value: the GPU test pins the range of the mean
        _own_rule(err, pk, ph, name)
        if expect == 'nan':
            assert np.all(np.isnan(pk)) and np.all(np.isfinite(err)), name
        elif expect == 'zero':
            assert pk.max() < R.EXACT_FIT_REF_M and ph.max() < R.EXACT_FIT_REF_M, (name, pk.max(), ph.max())


def test_per_joint_means_are_the_per_image_yardstick():
    """1000 x the mean over the joints of the per-joint yardstick is metrics_ref's per-image value in millimetres."""
    p, g = M.random_batch(7, 14, 3)
    err, pk, ph = R.given_per_joint(p, g)
    mp, mk, mh = M.joint_errors(p, g)
    for a, b in ((err, mp), (pk, mk), (ph, mh)):
        assert np.allclose(1000 * a.mean(-1), b, rtol=1e-13, atol=0)


# ---- the argument checker ------------------------------------------------------------------------------------------------------

def test_check_eval_step_refusals_and_edges():
    from spec_amd.engine import check_eval_step as chk
    ok = dict(B=2, V=64, J=17, nsel=14, joint_sel=list(M.H36M_TO_J14), Jk=24, pred_joints=True, gt_joints=True, joint_outputs=True)
    sel = chk(**ok)
    assert sel.dtype == np.int32 and sel.tolist() == list(M.H36M_TO_J14)
    bad = [dict(J=0), dict(J=33), dict(nsel=0, joint_sel=None), dict(nsel=33, joint_sel=list(range(17)) * 2), dict(Jk=0), dict(Jk=33),
           dict(joint_sel=None, nsel=18), dict(pred_joints=False), dict(gt_joints=False),
           dict(pred_joints=False, gt_joints=False), dict(B=0), dict(V=0), dict(joint_sel=[17] * 14), dict(joint_sel=[-1] * 14),
           dict(joint_sel=[0] * 13)]
    for change in bad:
        with pytest.raises(ValueError):
            chk(**dict(ok, **change))
    # the edges: the cap on all three, one vertex, no joints and no joint outputs (then Jk is not read)
    assert chk(1, 1, 32, 32, None, 32, True, True, True) is None
    assert chk(1, 1, 32, 32, list(range(32)), 32, True, True, False).tolist() == list(range(32))
    assert chk(3, 1, 1, 1, None, 99, False, False, False) is None
    assert chk(3, 6890, 17, 17, None) is None


# ---- the flow's host side ------------------------------------------------------------------------------------------------------

class _Body:
    """Records the pose it is given; joints = pose[:, :3] + joint index, so the pelvis subtraction shows."""

    def native(self, pose, betas, vertices=True, joints24=True):
        import torch
        self.pose = pose.cpu().numpy()
        j = pose[:, None, :3] + torch.arange(24, dtype=pose.dtype)[None, :, None]
        return torch.zeros(pose.shape[0], 5, 3), j


def test_eval_gt_pose_key_rule(tmp_path):
    from spec_amd.evaluation import EvalDataset
    rng = np.random.default_rng(0)
    ann = {'imgname': np.array(['a.png', 'b.png', 'c.png']), 'pose': rng.standard_normal((3, 72)), 'shape': rng.standard_normal((3, 10))}
    np.savez(tmp_path / 'plain.npz', **ann)
    np.savez(tmp_path / 'yaw.npz', pose_0yaw_inverseyz=ann['pose'] + 1.0, **ann)
    np.savez(tmp_path / 'none.npz', imgname=ann['imgname'])
    idx = np.array([2, 0])
    for name, want in (('plain', ann['pose']), ('yaw', ann['pose'] + 1.0)):
        body = _Body()
        gt = EvalDataset('spec-syn', dataset_file=str(tmp_path / f'{name}.npz'), img_dir='.').eval_gt(idx, 'cpu', body)
        assert np.array_equal(body.pose, want[idx].astype(np.float32)), name
        assert set(gt) == {'vertices', 'joints_24'} and gt['vertices'].shape == (2, 5, 3)
        j = gt['joints_24'].numpy()
        assert j.shape == (2, 24, 3) and np.all(j[:, 0] == 0) and np.array_equal(j[:, 5], np.full((2, 3), 5.0, np.float32))
    with pytest.raises(KeyError):
        EvalDataset('spec-syn', dataset_file=str(tmp_path / 'none.npz'), img_dir='.').eval_gt(idx, 'cpu', _Body())


def test_eval_dump_round_trips_the_per_joint_keys(tmp_path):
    import joblib
    import torch
    from spec_amd.io_formats import EvalDump
    rng = np.random.default_rng(1)
    dump, want = EvalDump(), {k: [] for k in ('mpjpe', 'pampjpe', 'mpjpe_24', 'pampjpe_24')}
    for n in (4, 2):                                     # two batches, the last one short
        pred = {'pred_pose': torch.zeros(n, 24, 3, 3), 'pred_shape': torch.zeros(n, 10), 'pred_cam': torch.zeros(n, 3),
                'smpl_vertices': torch.zeros(n, 7, 3)}
        e = {k: torch.from_numpy(rng.random((n, 24 if k.endswith('24') else 14)).astype(np.float32)) for k in want}
        e['pampjpe'][0, 3] = float('nan')
        dump.add(pred, imgnames=[f'{n}_{i}.png' for i in range(n)], dataset_name='spec-syn', **e)
        for k in want:
            want[k].append(e[k].numpy())
    out = joblib.load(dump.write(str(tmp_path), 'spec-syn'))
    for k, v in want.items():
        assert out[k].dtype == np.float32 and np.array_equal(out[k], np.concatenate(v), equal_nan=True), k
    assert out['mpjpe'].shape == (6, 14) and out['pampjpe_24'].shape == (6, 24) and len(out['imgname']) == 6
    plain = EvalDump()
    plain.add(pred)
    assert set(joblib.load(plain.write(str(tmp_path / 'plain'), 'spec-syn'))) == {'pose', 'shape', 'cam', 'vertices'}


def test_five_lines_and_json_layout(tmp_path):
    """``step_accuracy`` / ``step_lines`` / ``write_val_accuracy`` against spec/trainer.py:494-512,655-662 worked by hand: the
    mean over the images of each image's mean over its joints, x 1000, in float64; the multi-dataset wording; [[0, acc, 0]]."""
    from spec_amd import evaluation as E
    rng = np.random.default_rng(2)
    per = {k: rng.random((6, 24 if k.endswith('24') else 14)).astype(np.float32) for k in E.STEP_KEYS}
    v2v = rng.random(6).astype(np.float32)
    acc = E.step_accuracy(per, v2v)
    assert list(acc) == ['val_mpjpe', 'val_pampjpe', 'val_mpjpe_24', 'val_pampjpe_24', 'val_v2v']
    for k in E.STEP_KEYS:
        per_image = np.array([row.astype(np.float64).mean() for row in per[k]])
        assert acc['val_' + k] == 1000 * per_image.mean() and isinstance(acc['val_' + k], float)
    assert acc['val_v2v'] == 1000 * v2v.astype(np.float64).mean()
    assert E.step_lines('spec-mtp', acc) == ['spec-mtp MPJPE: ' + str(acc['val_mpjpe']), 'spec-mtp PA-MPJPE: ' + str(acc['val_pampjpe']),
                                             'spec-mtp MPJPE (24j): ' + str(acc['val_mpjpe_24']),
                                             'spec-mtp PA-MPJPE (24j): ' + str(acc['val_pampjpe_24']), 'spec-mtp V2V: ' + str(acc['val_v2v'])]
    path = E.write_val_accuracy(str(tmp_path / 'logs'), 'spec-mtp', acc)
    assert os.path.basename(path) == 'val_accuracy_results_spec-mtp.json'
    text = open(path).read()
    assert json.loads(text) == [[0, acc, 0]] and text == json.dumps([[0, acc, 0]], indent=4)
