"""Host side of the trainable HMRHead: the float64 restatement (tests/head_grad_ref.py) against torch autograd of
``oracle.heads.HMRHead`` and against central differences, what the reference's own fp32 arithmetic is worth on the device
tests' cases, the descent rate's head-room, the pure argument checks and the C ABI surface.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import head_grad_ref as R
from tests import smpl_grad_ref as S
from tests import tail_grad_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ((40, 3, False), (40, 5, True))


class _FixedDrop(torch.nn.Module):
    """nn.Dropout with its draws replaced by given keep-masks: call i multiplies by masks[i] * s."""

    def __init__(self, masks, s, dtype):
        super().__init__()
        self.masks, self.s, self.i = [torch.from_numpy(m != 0).to(dtype) for m in masks], s, 0

    def forward(self, x):
        self.i += 1
        return x * self.masks[self.i - 1] * self.s


def _autograd(c, dtype):
    """state_n, g_xf and the ten parameter gradients of case ``c`` by torch autograd of oracle.heads.HMRHead in ``dtype``."""
    from oracle.heads import HMRHead
    F = c['xf'].shape[1]
    B = c['xf'].shape[0]
    head = HMRHead(F, smpl_mean_params={'pose': np.zeros(144), 'shape': np.zeros(10), 'cam': np.zeros(3)},
                   use_cam_feats=c['cam_feats'] is not None)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c['params'].items()}, strict=False)
    head = head.to(dtype)
    if c['masks'] is not None:
        head.train()
        head.drop1 = _FixedDrop(c['masks'][0::2], c['s'], dtype)
        head.drop2 = _FixedDrop(c['masks'][1::2], c['s'], dtype)
    else:
        head.eval()
    t = lambda a: torch.from_numpy(a).to(dtype)
    kw = {}
    if c['cam_feats'] is not None:
        rot = torch.zeros(B, 3, 3, dtype=dtype)
        rot[:, :, :2] = t(c['cam_feats'][:, :6]).reshape(B, 3, 2)
        kw = {'cam_rotmat': rot, 'cam_vfov': t(c['cam_feats'][:, 6])}
    init = t(c['init_state'])
    with torch.enable_grad():
        feats = t(c['xf'])[:, :, None, None].clone().requires_grad_(True)
        out = head(feats, init[:, :144], init[:, 144:154], init[:, 154:], n_iter=c['n_iter'], **kw)
        state = torch.cat([out['pred_pose_6d'], out['pred_shape'], out['pred_cam']], 1)
        ps = dict(head.named_parameters())
        g = torch.autograd.grad((state * t(c['g_state'])).sum(), [feats] + [ps[n] for n in R.NAMES])
    return state.detach().numpy(), g[0].numpy()[:, :, 0, 0], {n: gi.numpy() for n, gi in zip(R.NAMES, g[1:])}


def _errors(c, got):
    state, g_xf, grads = got
    return {'state': S.err(state, c['state']), 'g_xf': S.err(g_xf, c['g_xf']), **{n: S.err(grads[n], c['grads'][n]) for n in R.NAMES}}


@pytest.mark.parametrize('F,B,cam', SMALL)
@pytest.mark.parametrize('p', (None, 0.5, 0.2))
def test_restatement_equals_float64_autograd_of_the_oracle_head(F, B, cam, p):
    c = R.case(F, B, cam, 3, p)
    e = _errors(c, _autograd(c, torch.float64))
    assert max(e.values()) < 1e-12, e


def test_central_differences_of_three_directions():
    c = R.case(40, 3, True, 3, 0.5)
    r = np.random.default_rng(7)
    g = c['g_state'].astype(np.float64)

    def value(params, xf):
        return float((R.forward64(params, xf, c['init_state'], c['cam_feats'], c['masks'], c['s'])[0] * g).sum())
    for _ in range(3):
        d_xf = r.standard_normal(c['xf'].shape)
        d_p = {n: r.standard_normal(v.shape) for n, v in c['params'].items()}
        eps = 1e-5
        plus = value({n: v + eps * d_p[n] for n, v in c['params'].items()}, c['xf'] + eps * d_xf)
        minus = value({n: v - eps * d_p[n] for n, v in c['params'].items()}, c['xf'] - eps * d_xf)
        want = (c['g_xf'] * d_xf).sum() + sum((c['grads'][n] * d_p[n]).sum() for n in R.NAMES)
        assert abs((plus - minus) / (2 * eps) - want) < 1e-6 * abs(want), ((plus - minus) / (2 * eps), want)


def test_fp32_autograd_of_the_reference_on_the_device_cases():
    """What the reference's own fp32 arithmetic (CPU torch) is worth against float64 on every case of
    tests/test_gpu_head_backward.py: the device bound 1e-5 must leave a margin over it, so a case above 3e-6 is changed."""
    for F, B, cam, n_iter, p in R.variants():
        c = R.case(F, B, cam, n_iter, p)
        e = _errors(c, _autograd(c, torch.float32))
        worst = max(e, key=e.get)
        print(f'fp32 CPU autograd, F = {F}, B = {B}, cam = {cam}, n_iter = {n_iter}, p = {p}: worst {worst} {e[worst]:.3g}, state {e["state"]:.3g}')
        assert e[worst] < 3e-6, (F, B, cam, n_iter, p, e)


def test_descent_rate_has_a_factor_two_of_head_room():
    for lr in (R.DESCENT_LR, 2 * R.DESCENT_LR):
        losses = R.descend64(lr)
        print(lr, ['%.6g' % v for v in losses])
        assert all(b < a for a, b in zip(losses, losses[1:])), (lr, losses)


def test_check_hmr_head_train():
    from spec_amd.engine import check_hmr_head_train, hmr_head_param_shapes, hmr_head_tape_floats
    shapes = hmr_head_param_shapes(40, 7)
    assert shapes['fc1.weight'] == (1024, 204) and shapes['decshape.weight'] == (10, 1024) and shapes['deccam.bias'] == (3,)
    assert check_hmr_head_train(3, 40, 7, 3, 0.5, True, shapes, cam_feats=True, ld_xf=40, outputs=[True] + [False] * 10, addresses=[64, 4]) == 204
    assert check_hmr_head_train(70, 2048, 0, 1) == 2205
    assert check_hmr_head_train(1, 1, 0, 2, p=7.0, masks=False) == 158            # p is not read without masks
    assert hmr_head_tape_floats(3, 2) == 2 * 3 * (157 + 2048)
    bad = [dict(B=0), dict(F=0), dict(C=3), dict(n_iter=0), dict(n_iter=4), dict(p=1.0, masks=True), dict(p=-0.1, masks=True),
           dict(param_shapes={k: v for k, v in shapes.items() if k != 'fc2.bias'}), dict(param_shapes=dict(shapes, **{'fc1.weight': (1024, 197)})),
           dict(cam_feats=False), dict(addresses=[64, 6]), dict(ld_xf=39), dict(outputs=[False] * 11)]
    for kw in bad:
        args = dict(B=3, F=40, C=7, n_iter=3)
        args.update(kw)
        with pytest.raises(ValueError):
            check_hmr_head_train(**args)


def test_exports_are_declared_documented_bound_and_built():
    from spec_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    for name, nargs in (('specmi_hmr_head_tape_floats', 5), ('specmi_hmr_head_train_forward', 15), ('specmi_hmr_head_backward', 16)):
        m = re.search(r'int ' + name + r'\(([^;]*)\);', hdr)
        assert m, name
        assert m.group(1).count(',') + 1 == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert re.search(r'STABLE.{0,4000}specmi_hmr_head_params', hdr, flags=re.S) and 'specmi_hmr_head_grads' in hdr
    assert 'head_bwd.hip' in build.SOURCES
    build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ('specmi_hmr_head_tape_floats', 'specmi_hmr_head_train_forward', 'specmi_hmr_head_backward'))
    n = C.c_int64(0)
    assert lib.specmi_hmr_head_tape_floats(70, 40, 7, 3, C.byref(n)) == _lib.OK and n.value == 3 * 70 * (157 + 2048)
    for B, F, Cc, it in ((0, 40, 7, 3), (3, 0, 7, 3), (3, 40, 1, 3), (3, 40, 7, 4)):
        assert lib.specmi_hmr_head_tape_floats(B, F, Cc, it, C.byref(n)) == _lib.ERR_ARG
    assert lib.specmi_hmr_head_tape_floats(3, 40, 7, 3, None) == _lib.ERR_ARG
    assert lib.specmi_hmr_head_train_forward(None, None, None, 0, None, None, None, 0.5, 1, 1, 0, 1, None, None, None) == _lib.ERR_ARG
