"""The oracle of the SMPL heads' backward, on the CPU: what float32 autograd of the reference chain is worth against its
float64 self on every shape the device tests use - the room the 1e-5 bound of tests/test_gpu_smpl_backward.py leaves the
device - and the argument checks of the two wrappers, which need no device."""
import pytest
import torch

from tests import smpl_grad_ref as G


@pytest.mark.parametrize('mode', G.MODES)
@pytest.mark.parametrize('nv,B', G.SHAPES)
def test_fp32_autograd_within_1e5_of_float64(nv, B, mode):
    inp, ups, g64 = G.case(nv, B, mode)
    g32 = G.grads(nv, mode, inp, ups, dtype=torch.float32)
    for k in G.IN_KEYS:
        e = G.err(g32[k], g64[k])
        print(f'V={nv} B={B} mode={mode} {k}: fp32 autograd vs float64 {e:.3g}')
        assert e < 1e-5, (k, e)


def test_float64_chain_matches_the_fp32_oracle_heads():
    """The restated projection is the oracle's: the float32 forward of this chain equals oracle.heads on the same model."""
    from oracle import heads
    nv, B = 257, 3
    inp = G.inputs(5, B)
    heads.set_assets(smpl_model=G.model(nv))
    tt = lambda k: torch.from_numpy(inp[k])
    with torch.no_grad():
        ref = heads.SMPLCamHead(G.IMG_RES)(tt('rotmat'), tt('betas'), tt('cam'), *[tt(k) for k in G.CAM_KEYS])
        got = G.forward(G._oracle(nv, False, torch.float32), 0, tt('rotmat'), tt('betas'), tt('cam'), [tt(k) for k in G.CAM_KEYS])
        ref1 = heads.SMPLHead(G.FOCAL, G.IMG_RES)(tt('rotmat'), tt('betas'), tt('cam'), normalize_joints2d=True)
        got1 = G.forward(G._oracle(nv, False, torch.float32), 1, tt('rotmat'), tt('betas'), tt('cam'), None)
    for k in G.OUT_KEYS:
        assert torch.equal(ref[k], got[k]), k
        assert torch.equal(ref1[k], got1[k]), k


def test_repeated_joint_map_entry_adds_in_the_reference():
    inp = G.inputs(6, 2)
    ups = {'smpl_joints3d': G.upstream(6, 2, 257, 0)['smpl_joints3d']}
    a, b = G.grads(257, 0, inp, ups), G.grads(257, 0, inp, ups, repeat_joint=True)
    assert G.err(a['rotmat'], b['rotmat']) > 1e-3          # the case is not vacuous


def test_wrapper_argument_checks():
    from spec_amd.engine import check_rot6d_backward, check_smpl_backward
    check_smpl_backward(1, [True, False, False, False], [False, False, True])
    check_smpl_backward(2, [False, False, False, True], [True, True, True], use_cam=True, camera=[True] * 6)
    for kw in (dict(B=0, upstream=[True] * 4, outputs=[True] * 3), dict(B=1, upstream=[False] * 4, outputs=[True] * 3),
               dict(B=1, upstream=[True] * 4, outputs=[False] * 3),
               dict(B=1, upstream=[True] * 4, outputs=[True] * 3, use_cam=True, camera=[True] * 5 + [False])):
        with pytest.raises(ValueError):
            check_smpl_backward(**kw)
    assert check_rot6d_backward((3, 144), (3, 24, 3, 3)) == 72 and check_rot6d_backward((5, 6), (5, 3, 3)) == 5
    for x, g in (((5, 7), (5, 3, 3)), ((0, 6), (0, 3, 3)), ((5, 6), (4, 3, 3))):
        with pytest.raises(ValueError):
            check_rot6d_backward(x, g)


def test_the_library_exports_the_backward():
    import ctypes

    from spec_amd import _lib, build
    assert 'smpl_bwd.hip' in build.SOURCES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (('specmi_smpl_backward', 19), ('specmi_rot6d_backward', 6), ('specmi_rot6d_forward', 5)):
        assert hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == nargs
