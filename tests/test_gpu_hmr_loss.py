"""The loss forward on the device (specmi_hmr_loss, spec_amd/losses.py), against the float64 restatement of tests/hmr_loss_ref.py.

Tolerance of a value of the loss dict (``check_dict``).  With ``f64`` the restatement and ``e_ref = |reference fp32 - f64|`` the
reference's own distance, the GPU must satisfy ``|gpu - f64| <= margin * e_ref`` on every key where ``e_ref > 0``; where the reference
hits float64's rounding exactly (``e_ref == 0``) the floor is 4 ulp(value); a key that is exactly 0 in float64 (the zero branches)
must be exactly 0.
* Fixture cases: ``e_ref`` is the reference's own modules' (tests/golden/hmr_loss.npz), ``margin`` = 4 (two CPU summation orders were
  measured 3.0 x apart in this project).
* Shapes the fixture does not hold: the reference is not there to run, so ``e_ref`` comes from a STAND-IN, the restatement evaluated in
  fp32 with NumPy's summation order.  By the same measurement the reference's own distance may be 3 x the stand-in's, so the margin over
  the stand-in is 4 x 3 = 12.  Measured ratios against the stand-in on MI355X: largest 4.19 (keypoints, B = 3, V = 6890: stand-in 0.31
  ulp, GPU 1.31 ulp), next 3.25; everywhere else at most 2.65.

Two further checks go beyond the reference and test the implementation against ITS OWN stated summation order (include/specmi.h,
loss.hip): ``check_terms`` (per-image sums, which the reference never forms) and ``check_fold`` (the second launch against a float64
fold of the first launch's output).  Their bounds are worst cases of that order - a kernel that summed otherwise would have to restate
them along with its header.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from spec_amd import _lib, cam_utils
from tests import hmr_loss_ref as ref
from tests.test_hmr_loss_host import GOLDEN, fixture_case

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope='module')
def eng():
    return cam_utils._engine(torch.device(DEV))


def dev(d):
    return {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in d.items()}


def weight_list(weights):
    w = dict(ref.DEFAULT_WEIGHTS, **weights)
    return [w[k] for k in ref.WEIGHT_NAMES]


def rows_bound(mode, pred, gt, t64, weights):
    """Worst case of fp32 on the six per-image sums UNDER THE ORDER THE KERNEL DOCUMENTS (not a bound from the reference): a lane adds ceil(n / 1024) chunk sums one after the
    other, six shuffle steps and three LDS additions follow, an element costs at most five roundings - relative (ceil(n / 1024) + 16)
    2^-24 on a sum of non-negative elements.  Three rows square a DIFFERENCE of rounded quantities and are conditioned by it: with an
    absolute error eps_d on d_i and elements k_i d_i^2, the sum moves by at most 2 eps_d sqrt(sum k_i) sqrt(sum k_i d_i^2)
    (Cauchy-Schwarz).  Row 0 in mode 1: d = (2 p / size - 1) - (2 g / size - 1), each side within 3 x 2^-24 of a value below 2.  Row
    1: d = (p - pelvis_p) - (g - pelvis_g), five roundings of magnitudes up to M = max |coordinate|.  Row 2: an element of the
    Rodrigues matrix is a sum of four products of quaternion components (2-ulp sin / cos, normalisation: 9 half-ulps each, doubled
    by the product, three additions): 24 x 2^-24 absolute."""
    w = dict(ref.DEFAULT_WEIGHTS, **weights)
    V3 = pred['smpl_vertices'].shape[1] * 3
    n = np.array([98, 72, 216, 24, 10, V3])
    b = (np.ceil(n / 1024) + 16)[:, None] * EPS * np.abs(t64)
    kp = np.asarray(gt['keypoints_orig' if mode == 1 else 'keypoints'], np.float64)
    conf = kp[:, :, 2] * np.r_[np.full(25, w['openpose_train_weight']), np.full(24, w['gt_train_weight'])]
    if mode == 1:
        k = conf[:, :, None] * (np.asarray(gt['orig_shape'], np.float64)[:, None, ::-1] / (np.asarray(gt['scale'], np.float64) * 200)[:, None, None])
        b[0] += 2 * (12 * EPS) * np.sqrt(k.reshape(len(k), -1).sum(1) * t64[0])
    M = max(np.abs(pred['smpl_joints3d']).max(), np.abs(gt['pose_3d'][:, :, :3]).max())
    b[1] += 2 * (8 * EPS * M) * np.sqrt(3 * np.asarray(gt['pose_3d'], np.float64)[:, :, 3].sum(1) * t64[1])
    b[2] += 2 * (24 * EPS) * np.sqrt(216 * t64[2])
    return b


FIXTURE_MARGIN, STANDIN_MARGIN = 4, 12


def check_dict(tag, got, f64, e_ref, margin):
    want = np.array([f64[k] for k in ref.KEYS])
    tol = np.where(e_ref > 0, margin * e_ref, 4 * ref.ulp32(want))
    d = np.abs(np.asarray(got, np.float64) - want)
    nz = want != 0
    print(tag, 'gpu', got, '\n   |gpu - f64| / e_ref', np.round(d[nz] / np.maximum(e_ref[nz], 1e-300), 2), ' in ulp', np.round(d[nz] / ref.ulp32(want[nz]), 2),
          ' e_ref in ulp', np.round(e_ref[nz] / ref.ulp32(want[nz]), 2))
    assert (np.asarray(got)[~nz] == 0).all(), (tag, got, want)
    assert (d <= tol).all(), (tag, d / np.maximum(e_ref, 1e-300), margin)


def check_terms(tag, mode, terms, pred, gt, weights):
    t64 = ref.per_image_terms(mode, pred, gt, weights)
    t32 = ref.per_image_terms(mode, pred, gt, weights, np.float32).astype(np.float64)
    tol = np.maximum(STANDIN_MARGIN * np.abs(t32 - t64), rows_bound(mode, pred, gt, t64, weights))
    d = np.abs(terms.astype(np.float64) - t64)
    print(tag, 'terms: worst |gpu - f64| / tolerance per row', np.round((d / np.maximum(tol, 1e-300)).max(1), 3))
    assert (d <= tol).all(), (tag, d / np.maximum(tol, 1e-300))


def fold64(mode, terms, counts, pred, gt, weights):
    """The seven values from the kernel's OWN per-image sums, folded in float64 - what the second launch has to reproduce."""
    w = {k: np.float64(np.float32(v)) for k, v in dict(ref.DEFAULT_WEIGHTS, **weights).items()}
    t = terms.astype(np.float64)
    hs, hp = np.asarray(gt['has_smpl']) != 0, np.asarray(gt['has_pose_3d']) != 0
    Nv, Np, B = int(hs.sum()), int(hp.sum()), t.shape[1]
    assert counts.tolist() == [Nv, Np]
    V3 = pred['smpl_vertices'].shape[1] * 3
    out = [w['keypoint_loss_weight'] * t[0].sum() / (B * 98), w['keypoint_loss_weight'] * (t[1][hp].sum() / (Np * 72) if Np else 0.),
           w['pose_loss_weight'] * ((t[3][hs].sum() / (Nv * 24)) * (t[2][hs].sum() / (Nv * 216)) if Nv else 0.),
           w['beta_loss_weight'] * (t[4][hs].sum() / (Nv * 10) if Nv else 0.),
           w['shape_loss_weight'] * (t[5][hs].sum() / (Nv * V3) if Nv and gt.get('vertices') is not None else 0.),
           (np.exp(-np.asarray(pred['pred_cam'], np.float64)[:, 0] * 10) ** 2).mean()]
    return np.array(out + [w['loss_weight'] * sum(out)])


def check_fold(tag, mode, res, pred, gt, weights):
    """means against fold64: a lane adds ceil(B / 64) rows, six shuffle steps, a division, a weight (the pose term: two of each
    and a product) - (ceil(B / 64) + 12) ulp; loss_cam and the total as format_bound states them."""
    terms, counts, means = (res[k].cpu().numpy() for k in ('terms', 'counts', 'means'))
    want = fold64(mode, terms, counts, pred, gt, weights)
    tol = ref.format_bound(pred, want, weights, ulps=math.ceil(terms.shape[1] / 64) + 12)
    d = np.abs(means.astype(np.float64) - want)
    print(tag, 'means', means, 'fold of own terms in float64', want)
    assert (means[want == 0] == 0).all() and (d <= tol).all(), (tag, d, tol)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ref.CASES))
def test_fixture_cases_through_the_modules(fx, name):
    """Measured on MI355X (gfx950): on 38 of the 46 non-zero keys |gpu - f64| equals the reference's own distance (ratio 1.00); largest
    ratio 3.99 (keypoints, 'weights', HMRLoss: reference 0.40 ulp, GPU 1.60 ulp), largest distance 4.56 ulp (loss_cam, 'single', the
    reference's own 4.56)."""
    from spec.losses import HMRCamLoss, HMRLoss
    for mode, cls in ((0, HMRLoss), (1, HMRCamLoss)):
        pred, gt, weights = fixture_case(fx, name, mode)
        f64 = ref.hmr_loss(mode, pred, gt, weights)
        e_ref = np.abs(fx[f'{name}.ref{mode}'].astype(np.float64) - np.array([f64[k] for k in ref.KEYS]))
        p = dev(pred)
        before = p['smpl_joints2d'].clone()
        loss, d = cls(**weights)(p, dev(gt))
        assert tuple(d) == ref.KEYS and all(v.dim() == 0 and v.device.type == 'cuda' and v.dtype == torch.float32 for v in d.values())
        assert torch.equal(loss, d['loss/total_loss'])
        assert torch.equal(p['smpl_joints2d'], before)                 # pred is not mutated (the reference's HMRCamLoss does, :191)
        check_dict(f'{name} mode {mode}', np.array([float(v) for v in d.values()], np.float32), f64, e_ref, FIXTURE_MARGIN)


def test_modules_without_gt_vertices(fx):
    """shape_loss_weight = 0 is the modules' default, and gt['vertices'] may then be missing: the same bits as with it, loss_shape 0."""
    from spec.losses import HMRCamLoss, HMRLoss
    for mode, cls in ((0, HMRLoss), (1, HMRCamLoss)):
        pred, gt, weights = fixture_case(fx, 'single', mode)
        assert weights == {}
        _, with_v = cls()(dev(pred), dev(gt))
        _, without = cls()(dev(pred), dev({k: v for k, v in gt.items() if k != 'vertices'}))
        _, none_v = cls()(dev(pred), dev(dict(gt, vertices=None)))
        for k in ref.KEYS:
            assert torch.equal(with_v[k], without[k]) and torch.equal(with_v[k], none_v[k]), k
        assert float(without['loss/loss_shape']) == 0.0
        with pytest.raises(ValueError, match='vertices'):
            cls(shape_loss_weight=0.5)(dev(pred), dev(dict(gt, vertices=None)))
    e = cam_utils._engine(torch.device(DEV))
    bad = {'terms': torch.empty(6, 1, device=DEV), 'counts': torch.empty(2, dtype=torch.int32, device=DEV), 'means': torch.empty(6, device=DEV)}
    with pytest.raises(ValueError, match='means'):
        e.hmr_loss(1, dev(pred), dev(gt), weight_list({}), out=bad)


ABI_NAMES = ('pred_pose', 'pred_shape', 'pred_cam', 'joints3d', 'joints2d', 'vertices', 'pose', 'betas', 'pose_conf', 'pose_3d', 'keypoints',
             'gt_vertices', 'has_smpl', 'has_pose_3d', 'orig_shape', 'scale')


def abi_tensors(mode, pred, gt):
    """The sixteen device tensors of the C prototype, in its order."""
    p, g = dev(pred), dev(gt)
    return [p[k] for k in ref.PRED_KEYS] + [g[k] for k in ('pose', 'betas', 'pose_conf', 'pose_3d', 'keypoints_orig' if mode == 1 else 'keypoints',
                                                           'vertices')] + [g['has_smpl'], g['has_pose_3d'], g['orig_shape'].float(), g['scale']]


def abi_call(eng, mode, tens, B, V, wl, out, drop=None):
    ptr = lambda x: None if x is None else x.data_ptr()
    return eng.lib.specmi_hmr_loss(eng.h, mode, *[None if n == drop else ptr(x) for n, x in zip(ABI_NAMES, tens)], B, V, *[float(w) for w in wl],
                                   ptr(out[0]), ptr(out[1]), ptr(out[2]), None)


@pytest.mark.parametrize('B,V,mode', [(1, 6890, 1), (3, 6890, 0), (5, 7, 0), (5, 7, 1), (5, 65, 0), (5, 65, 1), (300, 65, 1)])
def test_shapes_through_the_abi(eng, B, V, mode):
    """B = 1; V * 3 = 20670 (not a multiple of 4 x 64, image bases 8 bytes off a 16-byte boundary); V = 7 (21 floats: five chunks and
    a one-float tail, fewer chunks than lanes) and V = 65 (195 floats: a three-float tail); B = 300 (a lane of the fold adds five rows).
    Every case calls the exported symbol directly (ctypes, raw device pointers), not the Engine wrapper."""
    rng = np.random.default_rng(B * 1000 + V)
    pred, gt, j2d = ref.inputs(9000 + B + V, B, V, has_smpl=(rng.random(B) > 0.3).astype(np.int32), has_pose_3d=(rng.random(B) > 0.5).astype(np.int32))
    pred['smpl_joints2d'] = j2d[mode]
    weights = {'shape_loss_weight': 0.7, 'openpose_train_weight': 0.5}
    tens, runs = abi_tensors(mode, pred, gt), []
    for _ in range(2):
        out = (torch.empty(6, B, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV), torch.empty(7, device=DEV))
        assert abi_call(eng, mode, tens, B, V, weight_list(weights), out) == _lib.OK
        runs.append(dict(zip(('terms', 'counts', 'means'), out)))
    res, res2 = runs
    for k in res:
        assert torch.equal(res[k].view(torch.int32), res2[k].view(torch.int32)), k                # two runs, equal bits
    tag = f'B={B} V={V} mode={mode}'
    check_terms(tag, mode, res['terms'].cpu().numpy(), pred, gt, weights)
    check_fold(tag, mode, res, pred, gt, weights)
    f64, f32 = ref.hmr_loss(mode, pred, gt, weights), ref.hmr_loss(mode, pred, gt, weights, np.float32)
    e_ref = np.abs(np.array([f32[k] for k in ref.KEYS], np.float64) - np.array([f64[k] for k in ref.KEYS]))
    check_dict(tag, res['means'].cpu().numpy(), f64, e_ref, STANDIN_MARGIN)


def test_an_image_does_not_depend_on_its_batch(eng):
    """Image b's terms in a batch of 5 == the image alone == the image at another position of a permuted batch, bit for bit; with
    V = 6890 the image's first float sits at a different offset from a 16-byte boundary in each of them."""
    pred, gt, j2d = ref.inputs(777, 5, 6890, has_smpl=[1, 0, 1, 1, 0], has_pose_3d=[0, 1, 1, 0, 1])
    pred['smpl_joints2d'] = j2d[1]
    wl = weight_list({'shape_loss_weight': 1.0})
    full = eng.hmr_loss(1, dev(pred), dev(gt), wl)['terms'].cpu()
    perm = [3, 0, 4, 2, 1]
    sub = lambda d, idx: {k: (None if v is None else v[idx]) for k, v in d.items()}
    permuted = eng.hmr_loss(1, dev(sub(pred, perm)), dev(sub(gt, perm)), wl)['terms'].cpu()
    for b in range(5):
        one = eng.hmr_loss(1, dev(sub(pred, [b])), dev(sub(gt, [b])), wl)['terms'].cpu()
        assert torch.equal(one[:, 0].view(torch.int32), full[:, b].view(torch.int32)), b
        assert torch.equal(permuted[:, perm.index(b)].view(torch.int32), full[:, b].view(torch.int32)), b
    assert (full[5] > 0).all() and eng.sync_status() == 0


def test_end_to_end_from_the_network():
    """Synthetic HMR(use_cam=True) at B = 2, 224 x 224, into HMRCamLoss with gt vertices from the helper."""
    from spec.losses import HMRCamLoss
    from spec_amd import assets, losses, synth
    from spec_amd.cam_utils import cam_params_from_angles
    from spec_amd.modules import HMR
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    assets.use_synthetic_assets(1003)
    hm = HMR(use_cam=True, use_cam_feats=True)
    hm.load_state_dict({k: t(v) for k, v in synth.hmr_state(1002, True).items()}, strict=False)
    hm.to(DEV).eval().commit(torch.device(DEV), freeze=True)
    B = 2
    scale, center, img_w, img_h = synth.bbox_inputs(5, B, 640., 480.)
    R, K = cam_params_from_angles(np.float32([0.1, -0.2]), np.float32([0.05, 0.1]), np.float32([500., 700.]), img_w, img_h)
    out = hm(t(synth.images(123, B)).to(DEV), R, K, t(scale).to(DEV), t(center).to(DEV), t(img_w).to(DEV), t(img_h).to(DEV))
    _, gt, _ = ref.inputs(31, B, 4, has_pose_3d=[1, 0])
    gt.update(scale=np.asarray(scale, np.float32), orig_shape=np.stack([img_h, img_w], 1).astype(np.int64))
    gtd = dev({k: v for k, v in gt.items() if k != 'vertices'})
    gtd['vertices'] = losses.gt_vertices(gtd['pose'], gtd['betas'])
    assert tuple(gtd['vertices'].shape) == tuple(out['smpl_vertices'].shape)
    weights = {'shape_loss_weight': 1.0}
    loss, d = HMRCamLoss(**weights)(out, gtd)
    got = np.array([float(v) for v in d.values()], np.float32)
    assert np.isfinite(got).all() and float(loss) == got[6]
    pred = {k: out[k].cpu().numpy() for k in ref.PRED_KEYS}
    gt['vertices'] = gtd['vertices'].cpu().numpy()
    f64, f32 = ref.hmr_loss(1, pred, gt, weights), ref.hmr_loss(1, pred, gt, weights, np.float32)
    e_ref = np.abs(np.array([f32[k] for k in ref.KEYS], np.float64) - np.array([f64[k] for k in ref.KEYS]))
    check_dict('end to end', got, f64, e_ref, STANDIN_MARGIN)


def test_abi_refusals(eng):
    pred, gt, j2d = ref.inputs(5, 2, 7)
    pred['smpl_joints2d'] = j2d[1]
    tens, names = abi_tensors(1, pred, gt), ABI_NAMES
    terms, counts, means = torch.full((6, 2), -7.0, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(7, device=DEV)

    def call(mode=1, B=2, V=7, w_shape=1.0, drop=None, out=(terms, counts, means)):
        return abi_call(eng, mode, tens, B, V, [w_shape, 5., 1., 1., 0.001, 0., 1., 60.], out, drop)

    def refused(word, **kw):
        assert call(**kw) == _lib.ERR_ARG, kw
        msg = eng.lib.specmi_last_error(eng.h).decode()
        assert word in msg, (kw, msg)
    refused('B', B=0)
    refused('B', B=-3)
    refused('V', V=0)
    refused('mode', mode=2)
    refused('mode', mode=-1)
    for n in names:
        if n not in ('gt_vertices', 'orig_shape', 'scale'):
            refused(n, drop=n)
    refused('terms', out=(None, counts, means))
    refused('orig_shape', drop='orig_shape')
    refused('scale', drop='scale')
    refused('gt_vertices', drop='gt_vertices')                                 # shape_loss_weight != 0
    torch.cuda.synchronize()
    assert (terms == -7.0).all()                                               # nothing was launched
    assert call(w_shape=0.0, drop='gt_vertices') == _lib.OK                    # NULL is accepted with weight 0
    assert call(mode=0, drop='orig_shape') == _lib.OK and call(mode=0, drop='scale') == _lib.OK
    assert call(out=(terms, None, None)) == _lib.OK
    torch.cuda.synchronize()
    assert (terms != -7.0).all() and eng.sync_status() == 0


def test_spec_eval_loss_flag(tmp_path):
    """``spec_eval.py --standin DIR --loss`` prints the seven keys after the error lines and nothing else moves; the result file is,
    byte for byte, the one the flagless command writes (the path the parent commit runs), which a third, in-process run of that
    path reproduces again."""
    from spec_amd import evaluation
    script = os.path.join(ROOT, 'scripts', 'spec_eval.py')
    pkl = tmp_path / 'logs' / 'eval_standin' / 'evaluation_results_spec-syn.pkl'
    runs = {}
    for tag, extra in (('plain', []), ('loss', ['--loss'])):
        p = subprocess.run([sys.executable, script, '--standin', str(tmp_path), '--limit', '4'] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        runs[tag] = (p.stdout.splitlines(), pkl.read_bytes())
    assert runs['loss'][1] == runs['plain'][1]
    assert not any('loss/' in l for l in runs['plain'][0])
    lines = runs['loss'][0]
    loss_lines = [l for l in lines if l.startswith('loss/')]
    assert [l.split(':')[0] for l in loss_lines] == list(ref.KEYS)
    printed = [float(l.split(':')[1]) for l in loss_lines]
    assert np.isfinite(printed).all() and printed[2] > 0 and printed[5] > 0 and printed[6] > 0
    assert [l for l in lines if not l.startswith('loss/')] == runs['plain'][0]                  # nothing else moved
    assert lines.index(loss_lines[0]) > max(i for i, l in enumerate(lines) if 'MPJPE' in l or 'V2V' in l)
    hp = evaluation.load_config(str(tmp_path / 'data/spec/checkpoints/spec_config.yaml'))
    res = evaluation.run_evaluation(hp, data_root=str(tmp_path), limit=4, log=lambda s: None)
    assert pkl.read_bytes() == runs['plain'][1] and 'loss' not in res['spec-syn']
    res = evaluation.run_evaluation(hp, data_root=str(tmp_path), limit=4, log=lambda s: None, loss=True)
    assert tuple(res['spec-syn']['loss']) == ref.KEYS and pkl.read_bytes() == runs['plain'][1]
    assert [float(f'{v:.6g}') for v in res['spec-syn']['loss'].values()] == printed
