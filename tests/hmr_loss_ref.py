"""NumPy restatement of the reference's two loss modules (spec/losses.py: HMRLoss :26-141, HMRCamLoss :144-271) and of pare's
``batch_rodrigues`` (SPIN's form), in the dtype of its inputs: float64 when the tests use it as the yardstick, float32 when
tests/golden/make_hmr_loss_fixture.py binds it in place of the un-vendored ``pare.utils.geometry.batch_rodrigues``.

``hmr_loss(mode, pred, gt, weights)`` returns the seven values of the reference's ``loss_dict`` in its order, ``per_image_terms``
the six unnormalised per-image sums of ``specmi_hmr_loss`` (include/specmi.h), ``inputs(seed, B, V, ...)`` the seeded inputs the
fixture and the GPU tests share (the large tensors are regenerated from the seed, never stored)."""
import numpy as np

KEYS = ('loss/loss_keypoints', 'loss/loss_keypoints_3d', 'loss/loss_regr_pose', 'loss/loss_regr_betas', 'loss/loss_shape',
        'loss/loss_cam', 'loss/total_loss')
WEIGHT_NAMES = ('shape_loss_weight', 'keypoint_loss_weight', 'pose_loss_weight', 'smpl_part_loss_weight', 'beta_loss_weight',
                'openpose_train_weight', 'gt_train_weight', 'loss_weight')
DEFAULT_WEIGHTS = dict(zip(WEIGHT_NAMES, (0, 5., 1., 1., 0.001, 0., 1., 60.)))
PRED_KEYS = ('pred_pose', 'pred_shape', 'pred_cam', 'smpl_joints3d', 'smpl_joints2d', 'smpl_vertices')


def batch_rodrigues(theta):
    """(N, 3) axis-angle -> (N, 3, 3): angle = |theta + 1e-8|, axis = theta / angle, the quaternion (cos(angle / 2),
    sin(angle / 2) axis) divided by its norm, then the quaternion's rotation matrix."""
    theta = np.asarray(theta)
    dt = theta.dtype.type
    angle = np.sqrt(((theta + dt(1e-8)) ** 2).sum(1, keepdims=True))
    axis = theta / angle
    half = angle * dt(0.5)
    q = np.concatenate([np.cos(half), np.sin(half) * axis], 1)
    q = q / np.sqrt((q ** 2).sum(1, keepdims=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    R = np.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                  2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                  2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], 1)
    return R.reshape(-1, 3, 3)


def _cast(d, dtype):
    return {k: np.asarray(v, dtype) for k, v in d.items() if v is not None and k not in ('has_smpl', 'has_pose_3d')}


def per_image_terms(mode, pred, gt, weights=None, dtype=np.float64):
    """(6, B): rows keypoints, keypoints_3d, pose squared error, pose confidence, betas, vertices - every image, no mask.
    ``dtype=np.float32`` evaluates the same formulae in fp32 with NumPy's summation order (a second fp32 opinion)."""
    w = dict(DEFAULT_WEIGHTS, **(weights or {}))
    p, g = _cast(pred, dtype), _cast(gt, dtype)
    B = p['pred_cam'].shape[0]
    kp = g['keypoints_orig' if mode == 1 else 'keypoints']
    conf = kp[:, :, 2:3].copy()
    conf[:, :25] *= dtype(np.float32(w['openpose_train_weight']))
    conf[:, 25:] *= dtype(np.float32(w['gt_train_weight']))
    j2d, gxy = p['smpl_joints2d'], kp[:, :, :2]
    if mode == 1:
        size = g['orig_shape'][:, None, ::-1]                       # (H, W) -> (W, H)
        e = conf * (((2 * (j2d / size) - 1) - (2 * (gxy / size) - 1)) ** 2)
        e = e * (size / (g['scale'] * dtype(200.))[:, None, None])
    else:
        e = conf * (j2d - gxy) ** 2
    t = np.zeros((6, B), dtype)
    t[0] = e.reshape(B, -1).sum(1)
    pj, gj, c3 = p['smpl_joints3d'][:, 25:], g['pose_3d'][:, :, :3], g['pose_3d'][:, :, 3:]
    pj = pj - ((pj[:, 2] + pj[:, 3]) / 2)[:, None]
    gj = gj - ((gj[:, 2] + gj[:, 3]) / 2)[:, None]
    t[1] = (c3 * (pj - gj) ** 2).reshape(B, -1).sum(1)
    R = batch_rodrigues(g['pose'].reshape(-1, 3)).reshape(B, 24, 3, 3)
    t[2] = ((p['pred_pose'] - R) ** 2).reshape(B, -1).sum(1)
    t[3] = g['pose_conf'].sum(1)
    t[4] = ((p['pred_shape'] - g['betas']) ** 2).sum(1)
    if gt.get('vertices') is not None:
        t[5] = np.abs(p['smpl_vertices'] - g['vertices']).reshape(B, -1).sum(1)
    return t


def hmr_loss(mode, pred, gt, weights=None, dtype=np.float64):
    """-> dict of the seven values (float64, or fp32 arithmetic with ``dtype=np.float32``) under the reference's keys, in its order."""
    w = {k: dtype(np.float32(v)) for k, v in dict(DEFAULT_WEIGHTS, **(weights or {})).items()}
    t = per_image_terms(mode, pred, gt, weights, dtype)
    B = t.shape[1]
    hs, hp = np.asarray(gt['has_smpl']).astype(bool), np.asarray(gt['has_pose_3d']).astype(bool)
    Nv, Np = int(hs.sum()), int(hp.sum())
    V3 = np.asarray(pred['smpl_vertices']).shape[1] * 3
    z, n = dtype(0), lambda k: dtype(k)
    out = [w['keypoint_loss_weight'] * (t[0].sum() / n(B * 98)),
           w['keypoint_loss_weight'] * (t[1][hp].sum() / n(Np * 72) if Np else z),
           w['pose_loss_weight'] * ((t[3][hs].sum() / n(Nv * 24)) * (t[2][hs].sum() / n(Nv * 216)) if Nv else z),
           w['beta_loss_weight'] * (t[4][hs].sum() / n(Nv * 10) if Nv else z),
           w['shape_loss_weight'] * (t[5][hs].sum() / n(Nv * V3) if Nv and gt.get('vertices') is not None else z),
           (np.exp(-np.asarray(pred['pred_cam'], dtype)[:, 0] * dtype(10)) ** 2).mean()]
    out.append(w['loss_weight'] * sum(out[1:], out[0]))
    return dict(zip(KEYS, (float(v) for v in out)))


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def format_bound(pred, want, weights=None, ulps=4):
    """What fp32 itself allows on the seven values ``want`` (float64, KEYS order), whoever computes them: ``ulps`` ulp(value) on the
    five reduced terms; loss_cam is ill-conditioned by its own formula - x = 10 * pred_cam[:, 0] is rounded once (relative 2^-24,
    i.e. |x| 2^-24 absolute), exp keeps that as a RELATIVE error and adds its own ulp, the square doubles both and rounds again
    - relative (2 max|x| + 5) 2^-24, plus ``ulps`` / 2 ulp for the mean; the total carries the six through loss_weight and
    adds its own ``ulps`` ulp."""
    w = dict(DEFAULT_WEIGHTS, **(weights or {}))
    want = np.asarray(want, np.float64)
    b = ulps * ulp32(want)
    xmax = np.abs(10.0 * np.asarray(pred['pred_cam'], np.float64)[:, 0]).max()
    b[5] = (2 * xmax + 5) * 2.0 ** -24 * abs(want[5]) + ulps / 2 * ulp32(want[5])
    b[6] = abs(w['loss_weight']) * b[:6].sum() + ulps * ulp32(want[6])
    return b


def inputs(seed, B, V, has_smpl=None, has_pose_3d=None, zero_conf=False, shapes_hw=None):
    """Seeded fp32 inputs of plausible magnitude: a prediction dict and a ground-truth batch (both modes' keys)."""
    r = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    pose = r.standard_normal((B, 72)) * 0.3
    pose[0, 3:6] = 0.0                                              # the 1e-8 guard of batch_rodrigues
    R = batch_rodrigues(pose.reshape(-1, 3)).reshape(B, 24, 3, 3)
    gtv = (r.random((B, V, 3)) - 0.5) * [0.6, 1.7, 0.3]
    hw = np.asarray(shapes_hw if shapes_hw is not None else [[360 + 40 * (b % 3), 480 + 64 * (b % 2)] for b in range(B)], np.float64)
    kp_px = np.concatenate([r.random((B, 49, 2)) * hw[:, None, ::-1], (r.random((B, 49, 1)) > 0.2) * r.random((B, 49, 1))], 2)
    kp_n = np.concatenate([r.random((B, 49, 2)) * 2 - 1, kp_px[:, :, 2:]], 2)
    p3 = np.concatenate([r.standard_normal((B, 24, 3)) * 0.4, r.random((B, 24, 1))], 2)
    pc = np.ones((B, 24))
    if zero_conf:
        kp_px[:, 30:34, 2] = kp_n[:, 30:34, 2] = 0.0
        p3[:, 5:9, 3] = 0.0
        pc[:, ::3] = r.random((B, 8))
        pc[:, 1] = 0.0
    pred = {'pred_pose': f(R + r.standard_normal(R.shape) * 0.05), 'pred_shape': f(r.standard_normal((B, 10)) * 0.8),
            'pred_cam': f(np.stack([0.6 + 0.5 * r.random(B), r.standard_normal(B) * 0.1, r.standard_normal(B) * 0.1], 1)),
            'smpl_joints3d': f(r.standard_normal((B, 49, 3)) * 0.4),
            'smpl_joints2d': None, 'smpl_vertices': f(gtv + r.standard_normal(gtv.shape) * 0.02)}
    j2d_px = f(kp_px[:, :, :2] + r.standard_normal((B, 49, 2)) * 12.0)
    j2d_n = f(kp_n[:, :, :2] + r.standard_normal((B, 49, 2)) * 0.05)
    gt = {'pose': f(pose), 'betas': f(r.standard_normal((B, 10)) * 0.8), 'pose_conf': f(pc), 'pose_3d': f(p3),
          'keypoints': f(kp_n), 'keypoints_orig': f(kp_px), 'vertices': f(gtv),
          'has_smpl': np.asarray(has_smpl if has_smpl is not None else np.ones(B), np.int32),
          'has_pose_3d': np.asarray(has_pose_3d if has_pose_3d is not None else np.ones(B), np.int32),
          'orig_shape': hw.astype(np.int64), 'scale': f(0.8 + r.random(B))}
    return pred, gt, {0: j2d_n, 1: j2d_px}


# the fixture's cases (the issue's table): name -> (B, V, keyword arguments of inputs(), constructor weights)
CASES = {
    'single': (1, 6890, {}, {}),
    'mixed': (5, 6890, {'has_smpl': [1, 0, 1, 1, 0], 'has_pose_3d': [0, 1, 1, 0, 1]}, {'shape_loss_weight': 0.5}),
    'masks0': (5, 6890, {'has_smpl': [0] * 5, 'has_pose_3d': [0] * 5}, {'shape_loss_weight': 0.5}),
    'weights': (3, 6890, {'has_smpl': [1, 1, 0], 'zero_conf': True, 'shapes_hw': [[1080, 1920], [640, 360], [500, 333]]},
                {'shape_loss_weight': 1.5, 'keypoint_loss_weight': 3., 'pose_loss_weight': 2., 'smpl_part_loss_weight': 4.,
                 'beta_loss_weight': 0.01, 'openpose_train_weight': 0.25, 'gt_train_weight': 0.75, 'loss_weight': 10.}),
}
CASE_SEED = {'single': 8101, 'mixed': 8102, 'masks0': 8103, 'weights': 8104}


def case_inputs(name, mode):
    B, V, kw, weights = CASES[name]
    pred, gt, j2d = inputs(CASE_SEED[name], B, V, **kw)
    pred = dict(pred, smpl_joints2d=j2d[mode])
    return pred, gt, weights
