"""Reference for the SMPL heads' backward: the chain rotation matrices -> ``SMPLOracle`` -> ``convert_pare_to_full_img_cam`` /
``convert_weak_perspective_to_perspective`` -> perspective projection, built from oracle/smpl.py and oracle/geometry.py with
the body model's buffers cast to the working dtype, differentiated by torch.autograd on the CPU - in float64 (the arbiter) or
in float32 (what the reference's own arithmetic is worth).  ``oracle.geometry.perspective_projection`` casts to float inside, so
its three lines are restated here in the working dtype.  Seeded inputs as ``tests/hmr_loss_ref.inputs`` draws them (scale
0.6 .. 1.1, box scale 0.8 .. 1.8, image sizes 360-440 x 480-544: z and s stay away from 0)."""
import functools

import numpy as np
import torch

from oracle.geometry import convert_pare_to_full_img_cam, convert_weak_perspective_to_perspective, rot6d_to_rotmat
from oracle.smpl import SMPLOracle, batch_rodrigues

SHAPES = ((257, 1), (257, 3), (257, 33), (1000, 9), (6890, 2))      # (V, B) of the device tests
MODES = (0, 1)                                                      # 0 = SMPLCamHead, 1 = SMPLHead (normalize_joints2d)
OUT_KEYS = ('smpl_vertices', 'smpl_joints3d', 'smpl_joints2d', 'pred_cam_t')
IN_KEYS = ('rotmat', 'betas', 'cam')
CAM_KEYS = ('cam_rotmat', 'cam_intrinsics', 'bbox_scale', 'bbox_center', 'img_w', 'img_h')
FOCAL, IMG_RES = 5000., 224


@functools.lru_cache(maxsize=None)
def model(nv, repeat_joint=False):
    from spec_amd import synth
    m = dict(synth.smpl_model(77, nv))
    if repeat_joint:                       # two of the 49 joints read the same of the 54: their gradients must add
        jm = m['joint_map'].copy()
        jm[5] = jm[30]
        m['joint_map'] = jm
    return m


def inputs(seed, B):
    """-> dict of fp32 arrays: rotmat (B,24,3,3) (a rotation plus 0.05 noise, as a regressor's is not orthonormal to the last
    bit), betas, cam and the six camera arguments."""
    r = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    pose = r.standard_normal((B, 72)) * 0.3
    R = batch_rodrigues(torch.from_numpy(pose.reshape(-1, 3))).numpy().reshape(B, 24, 3, 3)
    hw = np.asarray([[360 + 40 * (b % 3), 480 + 64 * (b % 2)] for b in range(B)], np.float64)
    K = np.zeros((B, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = (0.9 + 0.6 * r.random(B)) * hw.max(1)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = hw[:, 1] / 2, hw[:, 0] / 2, 1.0
    Rc = batch_rodrigues(torch.from_numpy(r.standard_normal((B, 3)) * 0.15)).numpy()
    return {'rotmat': f(R + r.standard_normal(R.shape) * 0.05), 'betas': f(r.standard_normal((B, 10)) * 0.8),
            'cam': f(np.stack([0.6 + 0.5 * r.random(B), r.standard_normal(B) * 0.1, r.standard_normal(B) * 0.1], 1)),
            'cam_rotmat': f(Rc), 'cam_intrinsics': f(K), 'bbox_scale': f(0.8 + r.random(B)),
            'bbox_center': f(hw[:, ::-1] / 2 + r.standard_normal((B, 2)) * 0.1 * hw[:, ::-1]), 'img_w': f(hw[:, 1]), 'img_h': f(hw[:, 0])}


def upstream(seed, B, V, mode):
    """Random upstream gradients, scaled so that the four contribute comparably to the outputs: a sum over V vertices grows like
    sqrt(V), one over 49 joints like 7, and a pixel of mode 0 is worth ~f / z ~ 100 times a metre."""
    r = np.random.default_rng(seed + 1)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {'smpl_vertices': f(r.standard_normal((B, V, 3)) / np.sqrt(V)), 'smpl_joints3d': f(r.standard_normal((B, 49, 3)) / 7.),
            'smpl_joints2d': f(r.standard_normal((B, 49, 2)) / (700. if mode == 0 else 7.)), 'pred_cam_t': f(r.standard_normal((B, 3)) * 0.1)}


@functools.lru_cache(maxsize=None)
def _oracle(nv, repeat_joint, dtype):
    return SMPLOracle(model(nv, repeat_joint)).to(dtype)


def forward(smpl, mode, rotmat, betas, cam, camera):
    """The four outputs in the dtype of the arguments; ``camera``: the six camera tensors in CAM_KEYS order (mode 0)."""
    vertices, joints3d = smpl(betas, rotmat)
    B = rotmat.shape[0]
    if mode == 0:
        R, K, scale, center, img_w, img_h = camera
        cam_t = convert_pare_to_full_img_cam(pare_cam=cam, bbox_height=scale * 200., bbox_center=center, img_w=img_w, img_h=img_h,
                                             focal_length=K[:, 0, 0], crop_res=IMG_RES)
    else:
        cam_t = convert_weak_perspective_to_perspective(cam, FOCAL, IMG_RES)
        K = torch.zeros(B, 3, 3, dtype=rotmat.dtype)
        K[:, 0, 0] = K[:, 1, 1] = FOCAL
        K[:, 2, 2] = 1.0
        R = torch.eye(3, dtype=rotmat.dtype).unsqueeze(0).expand(B, -1, -1)
    # oracle.geometry.perspective_projection without its cast to float
    points = torch.einsum('bij,bkj->bki', R, joints3d) + cam_t.unsqueeze(1)
    projected = points / points[:, :, -1].unsqueeze(-1)
    joints2d = torch.einsum('bij,bkj->bki', K, projected)[:, :, :-1]
    if mode == 1:
        joints2d = joints2d / (IMG_RES / 2.)
    return dict(zip(OUT_KEYS, (vertices, joints3d, joints2d, cam_t)))


def grads(nv, mode, inp, ups, dtype=torch.float64, repeat_joint=False):
    """The vector-Jacobian product by autograd: ``ups`` maps some of OUT_KEYS to upstream gradients (a missing key is zero) ->
    {rotmat, betas, cam: ndarray in ``dtype``}."""
    smpl = _oracle(nv, repeat_joint, dtype)
    with torch.enable_grad():
        leaves = [torch.from_numpy(inp[k]).to(dtype).requires_grad_(True) for k in IN_KEYS]
        out = forward(smpl, mode, *leaves, [torch.from_numpy(inp[k]).to(dtype) for k in CAM_KEYS])
        total = sum((out[k] * torch.from_numpy(g).to(dtype)).sum() for k, g in ups.items())
        g = torch.autograd.grad(total, leaves, allow_unused=True)
    return {k: (torch.zeros_like(l) if gi is None else gi).detach().numpy() for k, l, gi in zip(IN_KEYS, leaves, g)}


@functools.lru_cache(maxsize=None)
def case(nv, B, mode):
    """(inputs, upstream gradients, float64 gradients) of one shape and mode, computed once per process and left unchanged."""
    inp, ups = inputs(9000 + nv + B, B), upstream(9000 + nv + B, B, nv, mode)
    return inp, ups, grads(nv, mode, inp, ups)


def err(got, ref):
    """max |got - ref| / max |ref|: the metric of the forward's own head test (tests/test_gpu_c5.py:151-153)."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def rot6d_grad(x6d, g, dtype=torch.float64):
    """autograd through ``oracle.geometry.rot6d_to_rotmat``: x6d (N,6), g (N,3,3) -> (N,6)."""
    with torch.enable_grad():
        x = torch.from_numpy(x6d).to(dtype).requires_grad_(True)
        (gx,) = torch.autograd.grad((rot6d_to_rotmat(x) * torch.from_numpy(g).to(dtype)).sum(), x)
    return gx.numpy()
