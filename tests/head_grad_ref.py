"""Reference for the trainable HMRHead (spec_amd/csrc/head_bwd.hip, spec_amd.differentiable.HMRHead): pare's iterative regressor
restated in NumPy float64 with explicit dropout masks and the scalar ``s``, its backward written out by hand (forward64 /
grad64; tests/test_head_grad_host.py holds both against torch autograd of ``oracle.heads.HMRHead``), seeded cases, and the
chain head -> tests/tail_grad_ref.py that tests/test_gpu_head_training.py solves.

    xc_t = [xf | state_t | c],  a1_t = (xc_t W1^T + b1) * m1_t s,  a2_t = (a1_t W2^T + b2) * m2_t s,
    state_{t+1} = state_t + a2_t [Wpose; Wshape; Wcam]^T + [bpose | bshape | bcam]

masks: uint8 (2 n_iter, B, 1024) ordered (t, layer), or None = eval mode (no multiply)."""
import functools

import numpy as np
import torch

from tests import smpl_grad_ref as S
from tests import tail_grad_ref as T

H, NS = 1024, 157
NAMES = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'decpose.weight', 'decpose.bias', 'decshape.weight', 'decshape.bias',
         'deccam.weight', 'deccam.bias')
CASES = ((40, 3, False), (40, 70, True), (2048, 3, True))       # (F, B, use_cam_feats) of the device tests
# plain gradient descent on the ten parameters through the chain below (tests/test_gpu_head_training.py): chosen on the float64
# chain so that the loss falls at every one of six steps at this rate AND at twice it (tests/test_head_grad_host.py asserts both)
DESCENT_LR, DESCENT_STEPS = 2e-6, 6
TRAIN_F, TRAIN_HW = 40, 2                                        # features (B, 40, 2, 2) of the chain


def scale(p):
    """s = float32(1 / (1 - p)) of a float32 p, as include/specmi.h states it."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


def _dec(params, kind):
    return np.concatenate([params[f'{n}.{kind}'] for n in ('decpose', 'decshape', 'deccam')], 0)


def forward64(params, xf, init_state, cam_feats=None, masks=None, s=1.0, n_iter=3):
    """-> (state_n (B, 157), tape = (states [n], a1 [n], a2 [n])); everything float64."""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    xf, state = np.asarray(xf, np.float64), np.asarray(init_state, np.float64)
    c = np.zeros((xf.shape[0], 0)) if cam_feats is None else np.asarray(cam_feats, np.float64)
    Wd, bd = _dec(P, 'weight'), _dec(P, 'bias')
    states, a1s, a2s = [], [], []
    for t in range(n_iter):
        xc = np.concatenate([xf, state, c], 1)
        a1 = xc @ P['fc1.weight'].T + P['fc1.bias']
        if masks is not None:
            a1 = a1 * (masks[2 * t] != 0) * s
        a2 = a1 @ P['fc2.weight'].T + P['fc2.bias']
        if masks is not None:
            a2 = a2 * (masks[2 * t + 1] != 0) * s
        states.append(state), a1s.append(a1), a2s.append(a2)
        state = state + a2 @ Wd.T + bd
    return state, (states, a1s, a2s)


def grad64(params, xf, init_state, g_state, cam_feats=None, masks=None, s=1.0, n_iter=3):
    """The vector-Jacobian product at upstream g_state (B, 157) -> (g_xf (B, F), {name: gradient}); float64."""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    xf = np.asarray(xf, np.float64)
    F = xf.shape[1]
    c = np.zeros((xf.shape[0], 0)) if cam_feats is None else np.asarray(cam_feats, np.float64)
    _, (states, a1s, a2s) = forward64(params, xf, init_state, cam_feats, masks, s, n_iter)
    W1, W2, Wd = P['fc1.weight'], P['fc2.weight'], _dec(P, 'weight')
    gW1, gb1, gW2, gb2 = np.zeros_like(W1), np.zeros(H), np.zeros_like(W2), np.zeros(H)
    gWd, gbd = np.zeros_like(Wd), np.zeros(NS)
    g_xf = np.zeros_like(xf)
    g = np.asarray(g_state, np.float64)
    for t in range(n_iter - 1, -1, -1):
        gWd += g.T @ a2s[t]
        gbd += g.sum(0)
        g_h2 = g @ Wd
        if masks is not None:
            g_h2 = g_h2 * (masks[2 * t + 1] != 0) * s
        gW2 += g_h2.T @ a1s[t]
        gb2 += g_h2.sum(0)
        g_h1 = g_h2 @ W2
        if masks is not None:
            g_h1 = g_h1 * (masks[2 * t] != 0) * s
        gW1 += g_h1.T @ np.concatenate([xf, states[t], c], 1)
        gb1 += g_h1.sum(0)
        g_xc = g_h1 @ W1
        g_xf += g_xc[:, :F]
        g = g + g_xc[:, F:F + NS]
    grads = {'fc1.weight': gW1, 'fc1.bias': gb1, 'fc2.weight': gW2, 'fc2.bias': gb2}
    for n, (lo, hi) in (('decpose', (0, 144)), ('decshape', (144, 154)), ('deccam', (154, 157))):
        grads[f'{n}.weight'], grads[f'{n}.bias'] = gWd[lo:hi], gbd[lo:hi]
    return g_xf, grads


def draw_params(r, F, C):
    """fp32 parameters: fc1 / fc2 as nn.Linear draws them (uniform in +-1 / sqrt(fan_in)), the decoders xavier-uniform at gain 0.3 -
    O(1) steps of the state, so that the three iterations matter - with nn.Linear's biases."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    P = {}
    for n, rows, cols in (('fc1', H, F + NS + C), ('fc2', H, H), ('decpose', 144, H), ('decshape', 10, H), ('deccam', 3, H)):
        bound = 0.3 * np.sqrt(6.0 / (rows + cols)) if n.startswith('dec') else 1.0 / np.sqrt(cols)
        P[f'{n}.weight'] = f(r.uniform(-bound, bound, (rows, cols)))
        P[f'{n}.bias'] = f(r.uniform(-1.0 / np.sqrt(cols), 1.0 / np.sqrt(cols), rows))
    return P


def mean_state(B):
    return np.tile(np.concatenate([np.tile([1., 0, 0, 1, 0, 0], 24), np.zeros(10), [0.9, 0, 0]]).astype(np.float32), (B, 1))


def draw_masks(r, n_iter, B, p):
    return (r.random((2 * n_iter, B, H)) >= p).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(F, B, use_cam, n_iter=3, p=None):
    """One seeded problem and its float64 answers, computed once per process and left unchanged: -> dict with params, xf in [0, 1.5),
    init_state (the mean state plus noise), cam_feats or None, masks or None (p None = eval mode), s, g_state (random upstream),
    and state / g_xf / grads in float64."""
    r = np.random.default_rng(4000 + F + 7 * B + 100 * n_iter + (1 if use_cam else 0))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = {'params': draw_params(r, F, 7 if use_cam else 0), 'xf': f(r.random((B, F)) * 1.5),
         'init_state': f(mean_state(B) + r.standard_normal((B, NS)) * 0.05), 'n_iter': n_iter, 'p': p,
         'cam_feats': f(np.concatenate([S.inputs(5, B)['cam_rotmat'][:, :, :2].reshape(B, 6), 0.6 + 0.8 * r.random((B, 1))], 1)) if use_cam else None,
         'g_state': f(r.standard_normal((B, NS)))}
    c['masks'] = None if p is None else draw_masks(r, n_iter, B, p)
    c['s'] = 1.0 if p is None else scale(p)
    c['state'], _ = forward64(c['params'], c['xf'], c['init_state'], c['cam_feats'], c['masks'], c['s'], n_iter)
    c['g_xf'], c['grads'] = grad64(c['params'], c['xf'], c['init_state'], c['g_state'], c['cam_feats'], c['masks'], c['s'], n_iter)
    return c


def variants():
    """(F, B, use_cam, n_iter, p) of every device run: each case in eval mode and at p = 0.5 (s = 2, exact), the first also at
    p = 0.2 and with one iteration."""
    out = []
    for i, (F, B, cam) in enumerate(CASES):
        out += [(F, B, cam, 3, None), (F, B, cam, 3, 0.5)]
        if i == 0:
            out += [(F, B, cam, 3, 0.2), (F, B, cam, 1, None), (F, B, cam, 1, 0.5)]
    return out


# ---- the chain of tests/test_gpu_head_training.py: features (3, 40, 2, 2) -> HMRHead (use_cam_feats) -> SMPLCamHead -> HMRCamLoss ----
def cam_feats_of(camera):
    """[rotmat_to_rot6d(cam_rotmat) | vfov] with vfov = 2 atan(img_h / (2 f)) (spec/models/hmr.py:95) -> (B, 7) fp32, and vfov (B,)."""
    vfov = 2.0 * np.arctan(camera['img_h'].astype(np.float64) / (2.0 * camera['cam_intrinsics'][:, 0, 0]))
    B = vfov.shape[0]
    return np.concatenate([camera['cam_rotmat'][:, :, :2].reshape(B, 6), vfov[:, None]], 1).astype(np.float32), vfov.astype(np.float32)


@functools.lru_cache(maxsize=None)
def train_problem(descent=False):
    """-> (params, features (B, 40, 2, 2), masks (p = 0.5), camera, gt) at B = 3: the camera and ground truth of
    tail_grad_ref.problem() (descent: of its descent_problem())."""
    _, camera, gt = T.descent_problem() if descent else T.problem()
    r = np.random.default_rng(4100)
    return (draw_params(r, TRAIN_F, 7), np.ascontiguousarray(r.random((T.B, TRAIN_F, TRAIN_HW, TRAIN_HW)) * 1.5, dtype=np.float32),
            draw_masks(r, 3, T.B, 0.5), camera, gt)


def chain64(params, features, masks, camera, gt, weights):
    """-> (loss, g_features (B, F, h, w), {name: gradient}) of the chain in float64; masks None = eval mode."""
    B = features.shape[0]
    xf = np.asarray(features, np.float64).mean((2, 3))
    cf, _ = cam_feats_of(camera)
    s = 1.0 if masks is None else scale(0.5)
    state, _ = forward64(params, xf, mean_state(B), cf, masks, s)
    loss, g = T.grad64({'x6d': state[:, :144], 'betas': state[:, 144:154], 'cam': state[:, 154:]}, camera, gt, weights)
    g_xf, grads = grad64(params, xf, mean_state(B), np.concatenate([g[k] for k in T.STATE], 1), cf, masks, s)
    hw = features.shape[2] * features.shape[3]
    return loss, np.broadcast_to((g_xf / hw)[:, :, None, None], features.shape).copy(), grads


def descend64(lr, steps=DESCENT_STEPS):
    """The losses of ``steps`` steps of plain gradient descent on the ten parameters (eval-mode dropout) in float64: steps + 1 values."""
    params, features, _, camera, gt = train_problem(True)
    P = {k: v.astype(np.float64) for k, v in params.items()}
    losses = []
    for _ in range(steps):
        loss, _, g = chain64(P, features, None, camera, gt, T.DESCENT_WEIGHTS)
        losses.append(loss)
        P = {k: P[k] - lr * g[k] for k in NAMES}
    losses.append(chain64(P, features, None, camera, gt, T.DESCENT_WEIGHTS)[0])
    return losses
