"""HRNet-W32 / W48 trunks under the HMR regressor (spec/models/hmr.py:44-51: 'hrnet_w32-conv', 'hrnet_w32-interp', ...)
against the CPU oracle's restatement of PARE's PoseHighResolutionNet, through the drop-in nn.Module and the C ABI."""
import numpy as np
import pytest
import torch

from spec_amd import synth
from tests.util import rel_err, smpl_model, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def _models(backbone, use_cam=True, ucf=True, seed=1202):
    from oracle import heads
    from oracle.models import HMROracle, load_numpy_state
    from spec_amd import assets
    from spec_amd.modules import HMR
    hs = synth.hmr_state(seed, ucf, backbone=backbone)
    assets.use_synthetic_assets(1003)
    heads.set_assets(smpl_model=smpl_model())
    hm = HMR(backbone=backbone, use_cam=use_cam, use_cam_feats=ucf)
    missing, unexpected = hm.load_state_dict({k: t(v) for k, v in hs.items()}, strict=False)
    assert not unexpected and all(m.startswith('smpl.') for m in missing), (missing[:5], unexpected[:5])
    ohm = load_numpy_state(HMROracle(backbone=backbone, use_cam=use_cam, use_cam_feats=ucf).eval(), hs)
    return hm.to(DEV).eval(), ohm


def test_hrnet_state_dict_layout_matches_upstream_naming():
    """Key list of the parameter container == key list of the oracle's PoseHighResolutionNet (strict load both ways)."""
    from oracle.hrnet import hrnet_w32, hrnet_w48
    from spec_amd.modules import HRNetParams, get_backbone_info
    for width, ctor in ((32, hrnet_w32), (48, hrnet_w48)):
        for use_conv in (True, False):
            a = list(HRNetParams(width, use_conv).state_dict().keys())
            b = list(ctor(use_conv=use_conv).state_dict().keys())
            assert a == b
            assert 'transition2.2.0.0.weight' in a and 'stage4.2.fuse_layers.3.0.2.1.running_var' in a
            assert ('downsample_stage_1.6.weight' in a) == use_conv
    assert get_backbone_info('hrnet_w32')['n_output_channels'] == 480
    assert get_backbone_info('hrnet_w48')['n_output_channels'] == 720


@pytest.mark.parametrize('backbone,B,H,W', [('hrnet_w32-conv', 2, 224, 224), ('hrnet_w32-interp', 2, 224, 224),
                                            ('hrnet_w48-conv', 1, 224, 224), ('hrnet_w48-interp', 2, 96, 160)])
def test_hrnet_trunk_vs_oracle(backbone, B, H, W):
    hm, ohm = _models(backbone)
    x = t(synth.images(61, B))[:, :, :H, :W].contiguous()
    feat = hm.engine(torch.device(DEV)).trunk(x.to(DEV)).cpu()
    ref = ohm.backbone(x).permute(0, 2, 3, 1)
    assert feat.shape == ref.shape and feat.shape[-1] == (480 if 'w32' in backbone else 720)
    err = rel_err(feat.numpy(), ref.numpy())
    assert err < 5e-5, err


def test_hrnet_rejects_sizes_the_reference_cannot_fuse():
    hm, _ = _models('hrnet_w32-conv')
    from spec_amd._lib import ERR_ARG, SpecmiError
    eng = hm.engine(torch.device(DEV))
    with pytest.raises(SpecmiError):
        eng.trunk(torch.zeros(1, 3, 200, 224, device=DEV))
    # below the smallest input (a level of size 0), a level that does not halve, an empty side
    for H, W in ((16, 32), (32, 48), (0, 32)):
        with pytest.raises(SpecmiError) as e:
            eng.trunk(torch.zeros(1, 3, H, W, device=DEV))
        assert e.value.code == ERR_ARG, (H, W, str(e.value))
    # an empty batch: empty tensors out, no launch, no error - what the ResNet trunks do (test_empty_batch_returns_empty_outputs)
    feat = eng.trunk(torch.empty(0, 3, 32, 32, device=DEV))
    assert feat.shape == (0, 1, 1, 480)
    e = lambda *s: torch.empty(*s, device=DEV)
    out = hm(e(0, 3, 224, 224), cam_rotmat=e(0, 3, 3), cam_intrinsics=e(0, 3, 3), bbox_scale=e(0), bbox_center=e(0, 2), img_w=e(0), img_h=e(0))
    assert out['smpl_vertices'].shape == (0, 6890, 3) and out['pred_pose'].shape == (0, 24, 3, 3)
    x = t(synth.images(64, 1))[:, :, :32, :32].contiguous().to(DEV)      # and the engine still works afterwards
    assert torch.isfinite(eng.trunk(x)).all()


@pytest.mark.parametrize('backbone,use_cam,ucf', [('hrnet_w32-conv', True, True), ('hrnet_w32-interp', True, False),
                                                  ('hrnet_w48-conv', False, False), ('resnet34', True, True)])
def test_hmr_hrnet_end_to_end_vs_oracle(backbone, use_cam, ucf):
    hm, ohm = _models(backbone, use_cam, ucf)
    B = 3
    x = t(synth.images(62, B))
    sc, ce, iw, ih = [t(a) for a in synth.bbox_inputs(62, B, 640., 480.)]
    kw, okw = {}, {}
    if use_cam:
        from spec_amd.cam_utils import cam_params_from_angles
        R, K = cam_params_from_angles(np.array([0.1, -0.2, 0.3], np.float32), np.array([0.05, 0.1, -0.1], np.float32),
                                      np.array([500., 700., 900.], np.float32), iw, ih)
        kw = dict(cam_rotmat=R, cam_intrinsics=K, bbox_scale=sc.to(DEV), bbox_center=ce.to(DEV), img_w=iw.to(DEV), img_h=ih.to(DEV))
        okw = dict(cam_rotmat=R.cpu(), cam_intrinsics=K.cpu(), bbox_scale=sc, bbox_center=ce, img_w=iw, img_h=ih)
    out = hm(x.to(DEV), **kw)
    ref = ohm(x, **okw)
    assert set(out.keys()) == set(ref.keys())
    for k in ref:
        err = rel_err(out[k].cpu().numpy(), ref[k].numpy())
        tol = 1e-4
        if k == 'pred_cam_t':
            # tz = 2 f / (res * s): in the max-norm an error of pred_cam's scale s comes back multiplied by max|pred_cam| / min|s|.
            # The random-weight HRNets produce an s close to 0 for one of these images (condition number > 100), where two fp32
            # evaluations that agree to 1e-6 in pred_cam differ by 1e-4 in tz; pred_cam itself is held to 5e-6 for it
            pc = ref['pred_cam'].numpy()
            cond = float(np.abs(pc).max() / np.abs(pc[:, 0]).min())
            assert rel_err(out['pred_cam'].cpu().numpy(), pc) < 5e-6
            tol = max(tol, 5e-6 * cond)
        assert err < tol, (k, err)
    # collapsed regressor (default) vs the nine-GEMM loop on the 480 / 720-feature head
    eng = hm.engine(torch.device(DEV))
    eng.set_option('head_collapse', 0)
    out_i = hm(x.to(DEV), **kw)
    eng.set_option('head_collapse', 1)
    for k in ('pred_pose_6d', 'smpl_vertices'):
        assert rel_err(out[k].cpu().numpy(), out_i[k].cpu().numpy()) < 2e-5, k


def test_hrnet_batch_invariance():
    hm, _ = _models('hrnet_w32-conv')
    x = t(synth.images(63, 5)).to(DEV)
    eng = hm.engine(torch.device(DEV))
    full = eng.trunk(x).clone()
    one = eng.trunk(x[3:4])
    assert torch.equal(one[0], full[3])


# ---- the smallest and the non-square inputs, slice by slice against a float64 oracle ----------------------------------------------
BACKBONES = ['hrnet_w32-conv', 'hrnet_w32-interp', 'hrnet_w48-conv', 'hrnet_w48-interp']
# at 32x32 the four levels are 8, 4, 2 and 1 pixels wide (1x1 and 2x1 maps inside the walk, the OH == 1 branch of the resize); at
# 32x64 / 64x32 / 96x64 the height differs from the width at every level
SMALL_SHAPES = [(1, 32, 32), (3, 32, 64), (2, 64, 32), (2, 96, 64)]
SLICE_FLOOR = 1e-6       # of the slice's maximum: a slice the CPU happens to get right is not held against the GPU
_small = {}


def _slice_factor():
    """The allowance for a different but equally long summation tree: the one ``channel_report`` of tests/test_gpu_pretrained_like.py
    grants a channel (CHANNEL_HARD = 8 x the larger of the two CPU fp32 errors; its heavy-tail argument is stated there)."""
    from tests.test_gpu_pretrained_like import CHANNEL_HARD
    return CHANNEL_HARD


def _small_models(backbone):
    """(GPU module, fp32 oracle trunk, float64 oracle trunk) of a backbone, built once per process."""
    import copy
    if backbone not in _small:
        hm, ohm = _models(backbone)
        _small[backbone] = (hm, ohm.backbone, copy.deepcopy(ohm.backbone).double())
    return _small[backbone]


def concat_slices(backbone):
    C = 32 if 'w32' in backbone else 48
    return [(0, C), (C, 3 * C), (3 * C, 7 * C), (7 * C, 15 * C)]


def small_shape_report(backbone, B, H, W):
    """The trunk at (B, H, W) on the GPU and on the oracle in float64 and in float32 in both memory formats (NCHW on all threads,
    channels_last on one: two summation orders of the reference's own arithmetic).  -> one dict per concat slice: its maximum in the
    float64 map, e_gpu, e_cpu (the larger of the two fp32 runs), the two CPU errors, the bound."""
    from tests.util import cpu_threads
    hm, o32, o64 = _small_models(backbone)
    x = t(synth.images(61, B))[:, :, :H, :W].contiguous()
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().numpy()
    with cpu_threads():
        f64 = nhwc(o64(x.double()))
    f32 = nhwc(o32(x))
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        f32b = nhwc(o32(x.contiguous(memory_format=torch.channels_last)))
    finally:
        torch.set_num_threads(nt)
    feat = hm.engine(torch.device(DEV)).trunk(x.to(DEV)).cpu().numpy()
    assert feat.shape == f64.shape == (B, H // 32, W // 32, concat_slices(backbone)[-1][1]) and np.isfinite(feat).all()
    rows = []
    for lo, hi in concat_slices(backbone):
        r = f64[..., lo:hi]
        err = lambda a: float(np.abs(a[..., lo:hi].astype(np.float64) - r).max())
        cmax, e_a, e_b = float(np.abs(r).max()), err(f32), err(f32b)
        rows.append({'channels': [lo, hi], 'max': cmax, 'e_gpu': err(feat), 'e_cpu': max(e_a, e_b), 'e_cpu_nchw': e_a,
                     'e_cpu_channels_last': e_b, 'bound': max(_slice_factor() * max(e_a, e_b), SLICE_FLOOR * cmax)})
    return rows


@pytest.mark.parametrize('B,H,W', SMALL_SHAPES)
@pytest.mark.parametrize('backbone', BACKBONES)
def test_hrnet_small_and_non_square_inputs_per_concat_slice(backbone, B, H, W):
    """Each slice of the concat head against the float64 oracle, relative to its OWN maximum (a quiet branch cannot hide behind a loud
    one), and no less accurate than the oracle's own fp32 arithmetic: e_gpu <= factor x e_cpu, floor 1e-6 of the slice maximum.  The
    tolerance is measured, not chosen: profiles/hrnet_small_shapes.json holds the figures of every slice."""
    for row in small_shape_report(backbone, B, H, W):
        print(backbone, (B, H, W), row)
        assert row['max'] > 0, ('dead slice in the reference', row)
        assert row['e_gpu'] <= row['bound'], (backbone, (B, H, W), row)


# ---- the activation pool's lifetime -----------------------------------------------------------------------------------------------
POOL_SLOTS = 10          # HR_SLOTS of hrnet.hip
# (B, H, W) in call order, with what the pool must do and the batch width it must have afterwards
POOL_SEQUENCE = [((3, 64, 64), 'build', 3), ((1, 64, 64), 'reuse', 3), ((2, 32, 64), 'build', 3), ((3, 32, 64), 'reuse', 3),
                 ((5, 32, 64), 'build', 5), ((3, 64, 64), 'build', 5)]


def _pool_bytes(backbone, H, W, width):
    """Size of the pool of hrnet.hip for ``width`` images of H x W: POOL_SLOTS buffers per level (channels padded to 32) + the
    concat map."""
    C = 32 if 'w32' in backbone else 48
    per_image = (H // 32) * (W // 32) * 15 * C * 4
    for l in range(4):
        per_image += POOL_SLOTS * (H >> (2 + l)) * (W >> (2 + l)) * (-(-(C << l) // 32) * 32) * 4
    return per_image * width


@pytest.mark.parametrize('backbone', ['hrnet_w48-interp', 'hrnet_w32-conv'])
def test_hrnet_pool_lifetime(backbone):
    """One engine through batch sizes and image sizes that make the pool reuse its slots (smaller batch), rebuild them (another size;
    the batch width it remembers must not shrink) and grow: every output equals that of an engine whose pool was never used before
    (W48: slots that held another geometry's data must not leak into the zero pad channels), and the first and last call agree bit
    for bit.  What the pool did is read from the launch profile: a rebuild leaves one 'hrnet_pool_build' record whose bytes are the
    size of a pool of the remembered width."""
    from spec_amd.modules import HMR
    hm, _, _ = _small_models(backbone)
    hm.commit(torch.device(DEV))                              # whatever earlier tests left in its pool is gone: the width starts at 0
    eng = hm.engine(torch.device(DEV))
    # a second module with the same parameters: committing it again gives it an HRNet with an empty pool
    fresh = HMR(backbone=backbone, use_cam=True, use_cam_feats=True)
    fresh.load_state_dict(hm.state_dict(), strict=False)
    fresh = fresh.to(DEV).eval()
    outs, want = [], {}
    for (B, H, W), action, width in POOL_SEQUENCE:
        x = t(synth.images(65, B))[:, :, :H, :W].contiguous().to(DEV)
        if (B, H, W) not in want:
            fresh.commit(torch.device(DEV))
            want[(B, H, W)] = fresh.engine(torch.device(DEV)).trunk(x).clone()
        eng.profile(True)
        try:
            y = eng.trunk(x).clone()
            builds = [e for e in eng.profile_read() if e['kernel'] == 'hrnet_pool_build']
        finally:
            eng.profile(False)
        assert len(builds) == (1 if action == 'build' else 0), ((B, H, W), action, builds)
        if builds:
            assert builds[0]['launches'] == 1 and builds[0]['bytes'] == _pool_bytes(backbone, H, W, width), ((B, H, W), builds, width)
        assert torch.isfinite(y).all()
        assert torch.equal(y, want[(B, H, W)]), ((B, H, W), action, float((y - want[(B, H, W)]).abs().max()))
        outs.append(y)
    assert torch.equal(outs[0], outs[-1])
