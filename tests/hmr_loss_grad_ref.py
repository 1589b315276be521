"""A torch restatement of the reference's two loss modules (spec/losses.py: HMRLoss :59-141, HMRCamLoss :171-271) that autograd
can differentiate, in float64 (the arbiter of the device's ``specmi_hmr_loss_backward``) or in float32 (the same formulae at the
reference's own precision; tests/golden/hmr_loss_grad.npz holds what the reference's file itself gives).  The formulae are those
of tests/hmr_loss_ref.py, whose forward values this file must reproduce; ``batch_rodrigues`` of the ground truth is a constant
and comes from there.  ``pred`` is only read (the reference normalises ``smpl_joints2d`` in place)."""
import numpy as np
import torch

from tests import hmr_loss_ref as R

PRED_KEYS = R.PRED_KEYS
PROBE_SEED = 4711          # the probe the fixture dots d/d smpl_vertices with


def loss_values(mode, pred, gt, weights=None, dtype=torch.float64):
    """``pred``: {PRED_KEYS: torch tensor of ``dtype``} (leaves or not), ``gt``: numpy -> the seven values (0-dim tensors, R.KEYS order)."""
    w = {k: float(np.float32(v)) for k, v in dict(R.DEFAULT_WEIGHTS, **(weights or {})).items()}
    g = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in gt.items() if v is not None and k not in ('has_smpl', 'has_pose_3d')}
    hs, hp = (torch.from_numpy(np.asarray(gt[k]).astype(bool)) for k in ('has_smpl', 'has_pose_3d'))
    Nv, Np = int(hs.sum()), int(hp.sum())
    zero = torch.zeros((), dtype=dtype)
    kp = g['keypoints_orig' if mode == 1 else 'keypoints']
    conf = kp[:, :, 2:3].clone()
    conf[:, :25] *= w['openpose_train_weight']
    conf[:, 25:] *= w['gt_train_weight']
    j2d, gxy = pred['smpl_joints2d'], kp[:, :, :2]
    if mode == 1:
        size = g['orig_shape'].flip(-1)[:, None, :]                  # (H, W) -> (W, H)
        e = conf * ((2 * (j2d / size) - 1) - (2 * (gxy / size) - 1)) ** 2
        e = e * (size / (g['scale'] * 200.)[:, None, None])
    else:
        e = conf * (j2d - gxy) ** 2
    l_kp = w['keypoint_loss_weight'] * e.mean()
    if Np:
        pj, gj, c3 = pred['smpl_joints3d'][:, 25:][hp], g['pose_3d'][hp][:, :, :3], g['pose_3d'][hp][:, :, 3:]
        pj = pj - ((pj[:, 2] + pj[:, 3]) / 2)[:, None]
        gj = gj - ((gj[:, 2] + gj[:, 3]) / 2)[:, None]
        l_kp3 = w['keypoint_loss_weight'] * (c3 * (pj - gj) ** 2).mean()
    else:
        l_kp3 = zero
    if Nv:
        B = hs.shape[0]
        rot = torch.from_numpy(R.batch_rodrigues(np.asarray(gt['pose'], np.float64 if dtype == torch.float64 else np.float32).reshape(-1, 3))
                               ).to(dtype).reshape(B, 24, 3, 3)
        l_pose = w['pose_loss_weight'] * (g['pose_conf'][hs].mean() * ((pred['pred_pose'][hs] - rot[hs]) ** 2).mean())
        l_betas = w['beta_loss_weight'] * ((pred['pred_shape'][hs] - g['betas'][hs]) ** 2).mean()
        l_shape = w['shape_loss_weight'] * (pred['smpl_vertices'][hs] - g['vertices'][hs]).abs().mean() if 'vertices' in g else zero
    else:
        l_pose = l_betas = l_shape = zero
    l_cam = (torch.exp(-pred['pred_cam'][:, 0] * 10) ** 2).mean()
    six = [l_kp, l_kp3, l_pose, l_betas, l_shape, l_cam]
    total = w['loss_weight'] * (((((six[0] + six[1]) + six[2]) + six[3]) + six[4]) + six[5])
    return six + [total]


def grads(mode, pred, gt, weights=None, g_means=None, dtype=torch.float64):
    """d (g_means . means) / d pred by autograd -> ({PRED_KEYS: float ndarray}, the seven forward values as floats).  ``g_means``
    None = the total alone.  A term that does not reach a tensor (masked out entirely) counts as zero."""
    gm = np.zeros(7) if g_means is None else np.asarray(g_means, np.float64)
    if g_means is None:
        gm[6] = 1.0
    with torch.enable_grad():
        leaves = {k: torch.from_numpy(np.ascontiguousarray(pred[k])).to(dtype).requires_grad_(True) for k in PRED_KEYS}
        vals = loss_values(mode, leaves, gt, weights, dtype)
        obj = sum(float(c) * v for c, v in zip(gm, vals))
        gs = torch.autograd.grad(obj, [leaves[k] for k in PRED_KEYS], allow_unused=True)
    out = {k: (np.zeros(leaves[k].shape) if gi is None else gi.numpy()) for k, gi in zip(PRED_KEYS, gs)}
    return out, [float(v.detach()) for v in vals]


def probe(B, V):
    return np.random.default_rng(PROBE_SEED).standard_normal((B, V, 3))


def vertex_summary(gv, probe_):
    """What the fixture keeps of d/d smpl_vertices, per image: [non-zeros, min |g| over them, max |g|, g . probe in float64]."""
    gv = np.asarray(gv, np.float64)
    out = np.zeros((gv.shape[0], 4))
    for b, row in enumerate(gv):
        nz = np.abs(row[row != 0])
        out[b] = [nz.size, nz.min() if nz.size else 0.0, nz.max() if nz.size else 0.0, (row * probe_[b]).sum()]
    return out


def err(got, ref):
    """max |got - ref| / max |ref| (0 / 0 = 0: a tensor that must be zero is checked exactly by the caller)."""
    ref = np.asarray(ref, np.float64)
    d = np.abs(np.asarray(got, np.float64) - ref).max()
    m = np.abs(ref).max()
    return float(d / m) if m > 0 else float(d)
