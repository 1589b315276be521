"""``specmi_smpl_backward`` / ``specmi_rot6d_backward`` (spec_amd/csrc/smpl_bwd.hip) against float64 autograd of the reference
chain (tests/smpl_grad_ref.py), on synthetic body models.  Shapes (V, B): (257, .) = four full 64-vertex chunks plus one vertex alone in a
fifth, a partial 32-vertex group; (., 33) = one image in a second 32-image MFMA tile; 6890 = 215 * 32 + 10 is the real model size.  The bound
1e-5 on max|g - g64| / max|g64| is the forward's own (tests/test_gpu_c5.py:151-153); float32 autograd on the CPU sits at 3e-8 ..
6e-7 on the same cases (tests/test_smpl_grad_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import smpl_grad_ref as G
from tests.util import t

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GRADS = ('g_vertices', 'g_joints3d', 'g_joints2d', 'g_cam_t')       # keyword of Engine.smpl_backward per G.OUT_KEYS entry


def _engine(nv, mode, repeat_joint=False):
    from spec_amd import differentiable
    return differentiable._smpl_engine(DEV, G.model(nv, repeat_joint), mode == 0, G.IMG_RES, G.FOCAL)


def _dev(inp):
    return {k: t(v).to(DEV) for k, v in inp.items()}


def _backward(eng, mode, d, ups, want=(True, True, True)):
    """d: device inputs; ups: {OUT_KEY: device tensor or None}."""
    camera = [d[k] for k in G.CAM_KEYS] if mode == 0 else [None] * 6
    kw = {GRADS[G.OUT_KEYS.index(k)]: g for k, g in ups.items()}
    return eng.smpl_backward(d['rotmat'], d['betas'], d['cam'], *camera, want=want, **kw)


def _check(got, ref, what):
    for k, g in zip(G.IN_KEYS, got):
        e = G.err(g.cpu().numpy(), ref[k])
        print(f'{what} {k}: {e:.3g}')
        assert e < 1e-5, (what, k, e)


@pytest.mark.parametrize('mode', G.MODES)
@pytest.mark.parametrize('nv,B', G.SHAPES)
def test_smpl_backward_vs_float64_autograd(nv, B, mode):
    inp, ups, g64 = G.case(nv, B, mode)
    eng = _engine(nv, mode)
    got = _backward(eng, mode, _dev(inp), _dev(ups))
    _check(got, g64, f'V={nv} B={B} mode={mode}')
    again = _backward(eng, mode, _dev(inp), _dev(ups))              # determinism: the same bits in every run
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize('mode', G.MODES)
def test_each_upstream_gradient_alone_and_null_is_zero(mode):
    nv, B = 257, 3
    inp, ups, _ = G.case(nv, B, mode)
    eng, d, u = _engine(nv, mode), _dev(inp), _dev(ups)
    for k in G.OUT_KEYS:
        alone = _backward(eng, mode, d, {k: u[k]})
        zeros = _backward(eng, mode, d, {kk: (u[kk] if kk == k else torch.zeros_like(u[kk])) for kk in G.OUT_KEYS})
        assert all(torch.equal(a, b) for a, b in zip(alone, zeros)), k          # NULL = an all-zero tensor, bit for bit
        ref = G.grads(nv, mode, inp, {k: ups[k]})
        for name, g in zip(G.IN_KEYS, alone):
            if np.abs(ref[name]).max() == 0.0:                                  # e.g. pred_cam_t does not depend on the pose
                assert not g.any(), (k, name)
            else:
                e = G.err(g.cpu().numpy(), ref[name])
                print(f'mode={mode} {k} alone, {name}: {e:.3g}')
                assert e < 1e-5, (k, name, e)


@pytest.mark.parametrize('mode', G.MODES)
def test_outputs_may_be_null(mode):
    nv, B = 257, 3
    inp, ups, _ = G.case(nv, B, mode)
    eng, d, u = _engine(nv, mode), _dev(inp), _dev(ups)
    full = _backward(eng, mode, d, u)
    for i in range(3):
        want = tuple(j == i for j in range(3))
        got = _backward(eng, mode, d, u, want=want)
        assert [g is not None for g in got] == list(want) and torch.equal(got[i], full[i])


@pytest.mark.parametrize('mode', G.MODES)
def test_an_image_does_not_depend_on_its_batch(mode):
    """The same image alone, at position 0 and at position 32 of a batch of 33 (the second 32-image tile): the same bits."""
    nv = 257
    inp, ups, _ = G.case(nv, 33, mode)
    inp, ups = {k: v.copy() for k, v in inp.items()}, {k: v.copy() for k, v in ups.items()}
    for a in list(inp.values()) + list(ups.values()):
        a[32] = a[0]
    eng = _engine(nv, mode)
    g33 = _backward(eng, mode, _dev(inp), _dev(ups))
    g1 = _backward(eng, mode, _dev({k: v[:1] for k, v in inp.items()}), _dev({k: v[:1] for k, v in ups.items()}))
    for a, b in zip(g33, g1):
        assert torch.equal(a[0], b[0]) and torch.equal(a[32], b[0])


def test_repeated_joint_map_entries_add():
    nv, B, mode = 257, 3, 0
    inp, ups, _ = G.case(nv, B, mode)
    got = _backward(_engine(nv, mode, True), mode, _dev(inp), _dev(ups))
    _check(got, G.grads(nv, mode, inp, ups, repeat_joint=True), 'joint_map[5] = joint_map[30]')


def test_on_an_hmr_handle():
    """The same call on a full HMR handle (V = 6890, use_cam), which owns the workspace of the regressor too."""
    from tests.util import gpu_models, smpl_model
    _, hm = gpu_models(use_cam=True)
    eng = hm.engine(DEV)
    B, nv = 2, 6890
    inp, ups = G.inputs(77, B), G.upstream(77, B, nv, 0)
    got = _backward(eng, 0, _dev(inp), _dev(ups))
    smpl = G.SMPLOracle(smpl_model()).double()
    with torch.enable_grad():
        leaves = [t(inp[k]).double().requires_grad_(True) for k in G.IN_KEYS]
        out = G.forward(smpl, 0, *leaves, [t(inp[k]).double() for k in G.CAM_KEYS])
        ref = torch.autograd.grad(sum((out[k] * t(g).double()).sum() for k, g in ups.items()), leaves)
    _check(got, dict(zip(G.IN_KEYS, (r.numpy() for r in ref))), 'HMR handle')


def test_argument_errors_launch_nothing():
    from spec_amd import _lib
    nv, B, mode = 257, 3, 0
    inp, ups, _ = G.case(nv, B, mode)
    eng, d, u = _engine(nv, mode), _dev(inp), _dev(ups)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    outs = [torch.full((B, 24, 3, 3), 7.0, device=DEV), torch.full((B, 10), 7.0, device=DEV), torch.full((B, 3), 7.0, device=DEV)]
    camera, grads = [d[k] for k in G.CAM_KEYS], [u[k] for k in G.OUT_KEYS]

    def call(B_=B, camera_=camera, grads_=grads, outs_=outs):
        return eng.lib.specmi_smpl_backward(eng.h, p(d['rotmat']), p(d['betas']), p(d['cam']), B_, *(p(c) for c in camera_),
                                            *(p(g) for g in grads_), *(p(o) for o in outs_), eng._stream())

    assert call(B_=0) == _lib.ERR_ARG and call(B_=-3) == _lib.ERR_ARG
    assert call(grads_=[None] * 4) == _lib.ERR_ARG
    assert call(outs_=[None] * 3) == _lib.ERR_ARG
    for i in range(6):                                                           # mode 0 reads every camera argument
        assert call(camera_=[None if j == i else c for j, c in enumerate(camera)]) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    assert call() == _lib.OK                                                     # and the handle is still good
    torch.cuda.synchronize()
    assert not any(bool((o == 7.0).all()) for o in outs)
    # mode 1 needs none of them
    e1 = _engine(nv, 1)
    g = e1.smpl_backward(d['rotmat'], d['betas'], d['cam'], g_cam_t=u['pred_cam_t'], want=(False, False, True))
    assert g[0] is None and g[1] is None and g[2].shape == (B, 3)
    with pytest.raises(ValueError):
        e1.smpl_backward(d['rotmat'], d['betas'], d['cam'])


def test_capturable_after_one_eager_call():
    """Nothing is allocated per call: after one eager call of the shape the backward replays from a graph, same bits."""
    nv, B, mode = 257, 3, 0
    inp, ups, _ = G.case(nv, B, mode)
    eng, d, u = _engine(nv, mode), _dev(inp), _dev(ups)
    eager = _backward(eng, mode, d, u)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _backward(eng, mode, d, u)
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, out))


@pytest.mark.parametrize('kind', ['random', 'orthonormal'])
@pytest.mark.parametrize('n', [1, 72])
def test_rot6d_backward_vs_float64_autograd(n, kind):
    from spec_amd import differentiable, synth
    make = synth._random_rot6d if kind == 'random' else synth._orthonormal_rot6d
    x = make(4242, f'rot6d_bwd.{kind}.{n}', n).reshape(n, 6)
    g = np.random.default_rng(n).standard_normal((n, 3, 3)).astype(np.float32)
    eng = _engine(257, 1)
    got = eng.rot6d_backward(t(x).to(DEV), t(g).to(DEV))
    e = G.err(got.cpu().numpy(), G.rot6d_grad(x, g))
    print(f'rot6d {kind} N={n}: {e:.3g}')
    assert got.shape == (n, 6) and e < 1e-5
    # the forward export is the head's Gram-Schmidt, and autograd reaches the backward through spec_amd.differentiable
    R = eng.rot6d_to_rotmat(t(x).to(DEV))
    from oracle.geometry import rot6d_to_rotmat
    assert G.err(R.cpu().numpy(), rot6d_to_rotmat(t(x).double()).numpy()) < 1e-6
    with torch.enable_grad():
        leaf = t(x).to(DEV).requires_grad_(True)
        differentiable.rot6d_to_rotmat(leaf).backward(t(g).to(DEV))
    assert torch.equal(leaf.grad, got)
