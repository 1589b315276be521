"""Error behaviour of the C ABI on a GPU box (include/specmi.h conventions): every misuse returns a code and leaves a
message on the handle - no exception crosses the boundary, nothing crashes, the handle stays usable."""
import ctypes as C

import numpy as np
import pytest
import torch

from spec_amd import _lib, synth
from tests.util import t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def _err(lib, h):
    return (lib.specmi_last_error(h) or b'').decode()


def test_create_and_call_order_errors():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.specmi_create(C.byref(h), 0, 7) == _lib.ERR_ARG and 'model kind' in _err(lib, None)
    assert lib.specmi_create(C.byref(h), 99, _lib.MODEL_HMR) == _lib.ERR_ARG and 'out of range' in _err(lib, None)
    assert lib.specmi_create(None, 0, _lib.MODEL_HMR) == _lib.ERR_ARG
    assert lib.specmi_create(C.byref(h), 0, _lib.MODEL_CAMCALIB) == _lib.OK and h.value
    x = torch.zeros(1, 3, 224, 224, device=DEV)
    out = torch.empty(3, 1, 256, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr())
    # forward before commit
    rc = lib.specmi_camcalib_forward(h, p(x), 1, 224, 224, p(out[0]), p(out[1]), p(out[2]), None)
    assert rc == _lib.ERR_STATE and 'commit' in _err(lib, h)
    # commit with nothing staged: names the first missing tensor
    assert lib.specmi_commit(h) == _lib.ERR_MISSING and 'backbone.conv1.weight' in _err(lib, h)
    # a tensor of the wrong size
    w = np.zeros((64, 3, 7, 6), np.float32)
    shape = (C.c_int64 * 4)(*w.shape)
    assert lib.specmi_set_tensor_f32(h, b'backbone.conv1.weight', w.ctypes.data_as(C.c_void_p), shape, 4) == _lib.OK
    assert lib.specmi_commit(h) == _lib.ERR_ARG and 'elements' in _err(lib, h)
    # bad arguments to setters
    assert lib.specmi_set_tensor_f32(h, None, w.ctypes.data_as(C.c_void_p), shape, 4) == _lib.ERR_ARG
    assert lib.specmi_set_option_i32(h, None, 1) == _lib.ERR_ARG
    assert lib.specmi_set_option_i32(h, b'backbone', 77) == _lib.OK
    assert lib.specmi_commit(h) == _lib.ERR_ARG and 'backbone 77' in _err(lib, h)
    assert lib.specmi_destroy(h) == _lib.OK
    assert lib.specmi_destroy(None) == _lib.OK


def test_forward_argument_errors_keep_the_handle_usable():
    from spec_amd.modules import CameraRegressorNetwork
    cc = CameraRegressorNetwork()
    cc.load_state_dict({k: t(v) for k, v in synth.camcalib_state(1001).items()})
    cc = cc.to(DEV).eval()
    x = t(synth.images(1, 1)).to(DEV)
    good = [l.clone() for l in cc(x)]
    eng, lib = cc._engine, _lib.load()
    h = eng.h
    out = torch.empty(3, 1, 256, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr())
    assert lib.specmi_camcalib_forward(h, None, 1, 224, 224, p(out[0]), p(out[1]), p(out[2]), None) == _lib.ERR_ARG
    assert lib.specmi_camcalib_forward(h, p(x), 0, 224, 224, p(out[0]), p(out[1]), p(out[2]), None) == _lib.ERR_ARG
    assert lib.specmi_camcalib_forward(h, p(x), 1, 16, 16, p(out[0]), p(out[1]), p(out[2]), None) == _lib.ERR_ARG
    assert 'too small' in _err(lib, h)
    # an HMR entry point on a CamCalib handle
    assert lib.specmi_hmr_forward(h, p(x), 1, 224, 224, None, None, None, None, None, None, None, None) == _lib.ERR_STATE
    assert lib.specmi_smpl_native(h, p(x), 0, p(x), 1, p(x), None, None) == _lib.ERR_STATE
    # decode / metrics argument checks (no parameters needed)
    assert lib.specmi_camcalib_decode(h, p(out[0]), p(out[1]), p(out[2]), 1, 1, None, None, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.specmi_camcalib_bins(h, p(out[0]), 1, 256, None, None, None) == _lib.ERR_ARG
    assert lib.specmi_eval_joints(h, p(x), p(x), 1, 40, None, None, None) == _lib.ERR_ARG and '[1,32]' in _err(lib, h)
    assert lib.specmi_crop_resize_normalize(h, None, 10, 10, None, 1, 224, None, None) == _lib.ERR_ARG
    # the handle still works and gives the same answer
    again = cc(x)
    for a, b in zip(good, again):
        assert torch.equal(a, b)


def test_python_front_end_raises_with_the_library_message():
    from spec_amd import assets
    from spec_amd._lib import SpecmiError
    from spec_amd.modules import HMR
    assets.use_synthetic_assets(1003)
    hm = HMR(use_cam=True, use_cam_feats=True)
    hm.load_state_dict({k: t(v) for k, v in synth.hmr_state(1002, True).items()}, strict=False)
    hm = hm.to(DEV).eval()
    x = t(synth.images(2, 2)).to(DEV)
    with pytest.raises(SpecmiError) as e:            # use_cam without the camera inputs
        hm(x)
    assert 'use_cam' in str(e.value) and e.value.code == _lib.ERR_ARG
    with pytest.raises(RuntimeError):                # CPU tensors never fall back
        hm(x.cpu())
    with pytest.raises(ValueError):                  # wrong image rank
        hm(x[0])
    sc, ce, iw, ih = [t(a).to(DEV) for a in synth.bbox_inputs(2, 2)]
    with pytest.raises(ValueError):                  # wrong side-input shape
        hm(x, torch.eye(3, device=DEV)[None].repeat(3, 1, 1), torch.eye(3, device=DEV)[None].repeat(2, 1, 1), sc, ce, iw, ih)


def test_fc_forward_refusals():
    """specmi_fc_forward refuses what launch_fc_gemv / run_fc cannot take - with SPECMI_ERR_ARG, a message, nothing written - and the
    handle then runs the same layer."""
    from spec_amd.engine import Engine
    eng = Engine('camcalib', torch.device(DEV))
    lib, h = eng.lib, eng.h
    N, K, B, ldx, ldo = 5, 40, 2, 64, 8                    # K rounded up to 32 is 64
    w, b = np.ones((N, K), np.float32), np.arange(N, dtype=np.float32)
    x = torch.ones(B * ldx + 8, device=DEV)
    out = torch.full((B * ldo + 8,), 0x5A5AA5A5, dtype=torch.int32, device=DEV)
    arr = lambda *v: (C.c_void_p * 3)(*v)

    def call(nheads=1, N=N, K=K, B=B, ldx=ldx, ldo=ldo, path=0, xoff=0, ooff=0, res=False, wp=None):
        wp = arr(*[w.ctypes.data] * 3) if wp is None else wp
        o = arr(*[out.data_ptr() + ooff] * 3)
        return lib.specmi_fc_forward(h, nheads, wp, arr(*[b.ctypes.data] * 3), N, K, arr(*[x.data_ptr() + xoff] * 3), ldx, o if res else None,
                                     o, ldo, B, path, None)

    for kwargs, word in ((dict(nheads=0), 'nheads'), (dict(nheads=4), 'nheads'), (dict(N=0), 'positive'), (dict(K=0), 'positive'),
                         (dict(B=0), 'positive'), (dict(path=2), 'path'), (dict(ldx=60), 'ldx (60) <'), (dict(ldx=66), 'multiple of 4'),
                         (dict(ldo=4), 'ldo (4) < N (5)'), (dict(xoff=4), '16-byte'), (dict(ooff=2), '4-byte'), (dict(ooff=2, res=True), '4-byte'),
                         (dict(path=1, nheads=2), 'one head'), (dict(path=1, ldx=60), 'ldx (60) <'), (dict(path=1, xoff=8), '16-byte'),
                         (dict(wp=arr(None, None, None)), 'NULL')):
        assert call(**kwargs) == _lib.ERR_ARG and word in _err(lib, h), (kwargs, _err(lib, h))
    assert lib.specmi_fc_forward(h, 1, None, None, N, K, None, ldx, None, None, ldo, B, 0, None) == _lib.ERR_ARG and 'NULL' in _err(lib, h)
    torch.cuda.synchronize()
    assert bool((out == 0x5A5AA5A5).all())
    for path in (0, 1):
        assert call(path=path) == _lib.OK, _err(lib, h)
        got = out.cpu().numpy()
        assert np.array_equal(got[:B * ldo].reshape(B, ldo)[:, :N].copy().view(np.float32), np.tile(K + b, (B, 1)))
        assert np.all(got[:B * ldo].reshape(B, ldo)[:, N:] == 0x5A5AA5A5) and np.all(got[B * ldo:] == 0x5A5AA5A5)
        out.fill_(0x5A5AA5A5)
    eng.close()
