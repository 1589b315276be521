"""The fp16 trunk's own entrance: NHWC8 fp16 images (include/specmi.h) written by the ``_f16`` producers from uint8 frames and
read by the ``_f16in`` forwards, with no fp32 image and no conversion launch in between.

Every comparison is bit-exact (``torch.equal`` on the integer view, no tolerance).  The reference is the existing route - the fp32
producer followed by ``specmi_to_nhwc_f16`` / the existing forward on the fp32 image - which tests/test_gpu_fp16_shapes.py pins."""
import ctypes as C

import numpy as np
import pytest
import torch

from spec_amd import _lib, cam_utils, synth
from spec_amd import camcalib_eval as ce
from spec_amd.engine import _ptr
from tests.util import gpu_models, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan(*shape):
    return torch.full(shape, float('nan'), device=DEV, dtype=torch.float16)


def _check_nhwc8(out16, ref32, eng):
    """out16 (n,H,W,8) against to_nhwc_f16 of the fp32 producer's (n,3,H,W) image; pad channels +0; nothing left of the NaN fill"""
    assert out16.dtype == torch.float16 and out16.shape == (ref32.shape[0], ref32.shape[2], ref32.shape[3], 8)
    assert not torch.isnan(out16).any(), 'a pixel was not written'
    assert _same(out16, eng.to_nhwc_f16(ref32))
    assert not (_bits(out16)[..., 3:] != 0).any(), 'channels 3-7 must be +0 (bits 0x0000)'


@pytest.fixture(scope='module')
def eng():
    return cam_utils._engine(torch.device(DEV))


@pytest.fixture(scope='module')
def frames():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (2, 37, 53, 3), dtype=torch.uint8, generator=g).to(DEV)


# ---- 1. producers ----------------------------------------------------------------------------------------------------------
# [cx, cy, w, h]: over the top-left corner, larger than the frame, one pixel wide, two ordinary ones
BOXES = [[2., 3., 30., 30.], [26., 18., 200., 200.], [20., 15., 1., 20.], [40., 30., 20., 25.], [10.5, 25.25, 16., 16.]]
FIDX = [0, 1, 0, 1, 1]


@pytest.mark.parametrize('S', [224, 32])
def test_crop_f16_equals_converted_fp32_crop(eng, frames, S):
    from spec_amd.preprocess import crop_detections, crop_detections_batch
    n = len(BOXES)
    ref = crop_detections_batch(frames, FIDX, BOXES, crop_size=S)
    out = {'inp_images': _nan(n, S, S, 8), 'bbox_scale': torch.empty(n, device=DEV), 'bbox_center': torch.empty(n, 2, device=DEV)}
    got = crop_detections_batch(frames, FIDX, BOXES, crop_size=S, out=out, dtype=torch.float16)
    assert got['inp_images'] is out['inp_images']
    _check_nhwc8(got['inp_images'], ref['inp_images'], eng)
    assert _same(got['bbox_scale'], ref['bbox_scale']) and _same(got['bbox_center'], ref['bbox_center'])
    # the single-frame crop is the batch call with one frame; raw_hwc stays where it was
    one = crop_detections(frames[1], BOXES, crop_size=S, return_raw=True, dtype=torch.float16)
    one32 = crop_detections(frames[1], BOXES, crop_size=S, return_raw=True)
    _check_nhwc8(one['inp_images'], one32['inp_images'], eng)
    assert torch.equal(one['raw'], one32['raw'])


@pytest.mark.parametrize('S', [224, 32])
def test_crop_resize_f16_equals_converted_fp32_crop(eng, frames, S):
    # integer boxes [ulx, uly, brx, bry] that clip at the border, the whole frame, and an empty box (the constant-fill path)
    boxes = torch.tensor([[-5, -7, 20, 18], [30, 20, 60, 45], [0, 0, 53, 37], [10, 10, 10, 20]], dtype=torch.int32, device=DEV)
    n, (H, W) = boxes.shape[0], frames.shape[1:3]
    for f in range(2):
        ref = torch.empty(n, 3, S, S, device=DEV)
        _lib.check(eng.h, eng.lib.specmi_crop_resize_normalize(eng.h, _ptr(frames[f]), H, W, _ptr(boxes), n, S, _ptr(ref), eng._stream()))
        out = _nan(n, S, S, 8)
        _lib.check(eng.h, eng.lib.specmi_crop_resize_normalize_f16(eng.h, _ptr(frames[f]), H, W, _ptr(boxes), n, S, _ptr(out), eng._stream()))
        _check_nhwc8(out, ref, eng)
    from spec_amd.preprocess import dataset_crops
    centers, scales = [[20., 15.], [50., 30.]], [0.2, 0.1]
    _check_nhwc8(dataset_crops(frames[0], centers, scales, S, dtype=torch.float16), dataset_crops(frames[0], centers, scales, S), eng)


@pytest.mark.parametrize('H,W,OH,OW', [(45, 70, 32, 50), (33, 33, 64, 64), (1080, 1, 600, 32)])
def test_resize_f16_equals_converted_fp32_frame(eng, H, W, OH, OW):
    g = torch.Generator().manual_seed(H * 7 + W)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(DEV)
    ref, raw32 = torch.empty(1, 3, OH, OW, device=DEV), torch.empty(OH, OW, 3, dtype=torch.uint8, device=DEV)
    _lib.check(eng.h, eng.lib.specmi_resize_normalize(eng.h, _ptr(frame), H, W, OH, OW, _ptr(ref), _ptr(raw32), eng._stream()))
    out, raw16 = _nan(1, OH, OW, 8), torch.empty(OH, OW, 3, dtype=torch.uint8, device=DEV)
    _lib.check(eng.h, eng.lib.specmi_resize_normalize_f16(eng.h, _ptr(frame), H, W, OH, OW, _ptr(out), _ptr(raw16), eng._stream()))
    _check_nhwc8(out, ref, eng)
    assert torch.equal(raw16, raw32)


def test_camcalib_transform_dtype(eng, frames):
    from spec_amd.preprocess import camcalib_transform, camcalib_transform_batch
    ref = camcalib_transform_batch(frames, 48)
    out = _nan(2, ref.shape[2], ref.shape[3], 8)
    assert camcalib_transform_batch(frames, 48, out=out, dtype=torch.float16) is out
    _check_nhwc8(out, ref, eng)
    _check_nhwc8(camcalib_transform(frames[0], 48, dtype=torch.float16), ref[:1], eng)


def _ragged_case():
    """Three frames resampled / copied to 40 x 64, 64 x 40 and 33 x 33 (the last one kept as it is) inside a 64 x 64 batch"""
    g = torch.Generator().manual_seed(9)
    geom = [(50, 80, 40, 64), (96, 60, 64, 40), (33, 33, 33, 33)]
    parts, offsets, off = [], [], 0
    for H, W, _, _ in geom:
        parts.append(torch.randint(0, 256, (H * W * 3,), dtype=torch.uint8, generator=g))
        offsets.append(off)
        off += H * W * 3
    return torch.cat(parts).to(DEV), offsets, geom


def test_ragged_f16_equals_converted_fp32_batch_and_pads_with_zero_bits(eng):
    slab, offsets, geom = _ragged_case()
    ref = eng.resize_normalize_ragged(slab, offsets, geom)
    assert ref.shape == (3, 3, 64, 64)
    out = _nan(3, 64, 64, 8)
    assert eng.resize_normalize_ragged(slab, offsets, geom, out=out, dtype=torch.float16) is out
    _check_nhwc8(out, ref, eng)
    b = _bits(out)
    for f, (_, _, oh, ow) in enumerate(geom):
        assert not (b[f, oh:] != 0).any() and not (b[f, :, ow:] != 0).any(), 'padding must be 0x0000, not -0'
        assert (b[f, :oh, :ow, :3] != 0).any()


# ---- 2. consumers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def models16():
    cc, hm = gpu_models(True, True, DEV)
    cc.set_precision('fp16')
    hm.set_precision('fp16')
    cc.set_plan('throughput'); hm.set_plan('throughput')
    return cc, hm


def _uint8_batch(eng, B, H, W, seed):
    """(fp32 (B,3,H,W), NHWC8 fp16 (B,H,W,8)) of the same B uint8 frames through the fp32 and the fp16 producer"""
    g = torch.Generator().manual_seed(seed)
    if H == W:                 # square: crops of one frame
        frame = torch.randint(0, 256, (1, 90, 120, 3), dtype=torch.uint8, generator=g).to(DEV)
        boxes = [[30. + 9 * i, 40. + 3 * i, 50. + 7 * i, 60. + 5 * i] for i in range(B)]
        from spec_amd.preprocess import crop_detections_batch
        return tuple(crop_detections_batch(frame, [0] * B, boxes, crop_size=H, dtype=dt)['inp_images'] for dt in (torch.float32, torch.float16))
    slab = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, generator=g).to(DEV)
    offsets, geom = [i * H * W * 3 for i in range(B)], [(H, W, H, W)] * B
    return tuple(eng.resize_normalize_ragged(slab, offsets, geom, dtype=dt) for dt in (torch.float32, torch.float16))


def _hmr_args(B):
    sc, ce_, iw, ih = [t(a).to(DEV) for a in synth.bbox_inputs(9, B, 640., 480.)]
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    K = torch.tensor([[500., 0., 320.], [0., 500., 240.], [0., 0., 0.]], device=DEV).repeat(B, 1, 1)
    return dict(cam_rotmat=R, cam_intrinsics=K, bbox_scale=sc, bbox_center=ce_, img_w=iw, img_h=ih)


@pytest.mark.parametrize('B', [1, 3, 5])
@pytest.mark.parametrize('H,W', [(64, 96), (224, 224)])
def test_f16in_forwards_equal_the_forwards_on_fp32_images(eng, models16, B, H, W):
    cc, hm = models16
    x32, x16 = _uint8_batch(eng, B, H, W, seed=B * 1000 + H)
    assert x16.dtype == torch.float16 and x16.shape == (B, H, W, 8)
    l32, l16 = cc(x32), cc(x16)
    assert len(l16) == 3
    for a, b in zip(l16, l32):
        assert _same(a, b)
    kw = _hmr_args(B)
    o32, o16 = hm(x32, **kw), hm(x16, **kw)
    assert set(o16) == set(o32) and len(o16) >= 8
    for k in o32:
        assert _same(o16[k], o32[k]), k
    for m in (cc, hm):
        e = m.engine(torch.device(DEV))
        assert _same(e.trunk(x16), e.trunk(x32))
        assert e.sync_status() == 0


# ---- 3. whole flows at fp16 ---------------------------------------------------------------------------------------------
def _kernels(module):
    return {p['kernel'] for p in module.engine(torch.device(DEV)).profile_read()}


def test_demo_step_from_uint8_frames_has_no_conversion_launch(models16):
    from spec_amd.pipeline import DemoPipeline
    cc, hm = models16
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (1, 96, 128, 3), dtype=torch.uint8, generator=g).to(DEV)
    boxes = torch.tensor([[40., 50., 60., 80.], [90., 40., 50., 70.]], device=DEV)
    fidx = torch.zeros(2, dtype=torch.int32, device=DEV)
    dp = DemoPipeline(cc, hm, min_size=64)
    outs, kernels = {}, {}
    for forced in (True, False):
        dp._fp32_crops = forced
        for m in (cc, hm):
            m.engine(torch.device(DEV)).profile(True)
        outs[forced] = {k: v.clone() for k, v in dp(frames, boxes, fidx).items()}
        torch.cuda.synchronize()
        kernels[forced] = _kernels(cc) | _kernels(hm)
        for m in (cc, hm):
            m.engine(torch.device(DEV)).profile(False)
    assert 'to_nhwc_f16' in kernels[True], kernels[True]            # the forced route is the old one
    assert 'to_nhwc_f16' not in kernels[False], kernels[False]
    assert any(k.startswith('conv_f16') for k in kernels[False])
    for k, v in outs[True].items():
        assert _same(outs[False][k], v), k


def test_frame_stream_cuts_fp16_crops_for_an_fp16_step(models16):
    from spec_amd.frames import FrameStream
    from spec_amd.pipeline import SpecPipeline
    cc, hm = models16
    pipe = SpecPipeline(cc, hm, overlap=False)
    assert pipe.image_dtype == torch.float16
    H, W, N = 96, 128, 2
    res = {}
    for forced in (True, False):
        fs = FrameStream(pipe, DEV, (H, W), 1, N, copy_stream=torch.cuda.Stream(device=DEV), _fp32_crops=forced)
        assert fs.x.dtype == (torch.float32 if forced else torch.float16)
        hf, hb, hi = fs.host_buffers()
        hf.copy_(torch.randint(0, 256, hf.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(4)))
        hb.copy_(torch.tensor([[40., 50., 60., 80.], [90., 40., 50., 70.]]))
        hi.zero_()
        o = fs.submit(hf, hb, hi)
        fs.drain()
        res[forced] = {k: o[k].clone() for k in ('smpl_vertices', 'smpl_joints2d', 'pred_cam_t', 'cam_vfov', 'cam_pitch', 'cam_roll')}
    for k, v in res[True].items():
        assert _same(res[False][k], v), k


def test_graphed_pipeline_replay_on_fp16_static_buffers(eng, models16):
    from spec_amd.pipeline import GraphedPipeline, SpecPipeline
    cc, hm = models16
    B = 2
    x32, x16 = _uint8_batch(eng, B, 224, 224, seed=77)
    kw = _hmr_args(B)
    args = (kw['bbox_scale'], kw['bbox_center'], kw['img_w'], kw['img_h'])
    pipe = SpecPipeline(cc, hm, overlap=True)
    keys = ('smpl_vertices', 'smpl_joints3d', 'smpl_joints2d', 'pred_cam_t', 'pred_pose', 'cam_vfov', 'cam_pitch', 'cam_roll')
    eager32 = {k: v.clone() for k, v in pipe(x32, *args).items() if k in keys}
    eager16 = {k: v.clone() for k, v in pipe(x16, *args).items() if k in keys}
    gp = GraphedPipeline(pipe, torch.zeros_like(x16), *args)
    assert gp.static_in[0].dtype == torch.float16 and gp.image_dtype == torch.float16
    replay = gp(x16, *args)
    torch.cuda.synchronize()
    for k in keys:
        assert _same(eager16[k], eager32[k]), k
        assert _same(replay[k], eager32[k]), k


@pytest.fixture(scope='module')
def standin(tmp_path_factory):
    d = tmp_path_factory.mktemp('f16_input_tree')
    ce.write_standin_tree(str(d), n_images=3, min_res=48, max_res=80, batch_size=3, backbone='resnet50', loss_type='softargmax_l2')
    hp = ce.load_config(str(d / ce.STANDIN_CFG))
    model = ce.build_model(hp, None, str(d), DEV)
    model.set_precision('fp16')
    return hp, str(d), model


def test_camcalib_validation_batch_of_ragged_frames(standin):
    hp, root, model = standin
    quiet = lambda s: None
    new = ce.run_evaluation(hp, root, model=model, log=quiet, _fp32_images=False)
    old = ce.run_evaluation(hp, root, model=model, log=quiet, _fp32_images=True)
    assert new['logits'].shape == (3, 3, 256) and new['batches'][0]['padded_hw'] == old['batches'][0]['padded_hw']
    assert len({tuple(s) for s in new['img_sizes']}) > 1, 'the stand-in frames must be ragged'
    assert np.array_equal(new['logits'].view(np.int32), old['logits'].view(np.int32))
    for k in ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc'):
        assert new[k] == old[k], k


# ---- 4. sub-batching ------------------------------------------------------------------------------------------------------
def test_sub_batches_slice_whole_images_of_the_fp16_batch(standin):
    hp, root, model = standin
    ds = ce.PanoValDataset(ce.val_dataset_name(hp), root)
    frames = [ds.frame(i) for i in range(3)]
    e = model.engine(torch.device(DEV))
    x16 = ce.pad_batch(frames, 48, 80, DEV, e, dtype=torch.float16)
    x32 = ce.pad_batch(frames, 48, 80, DEV, e)
    assert x16.shape == (3, x32.shape[2], x32.shape[3], 8)
    whole = ce.forward_padded(model, x16)
    ones = ce.forward_padded(model, x16, sub_batch=1)
    twos = ce.forward_padded(model, x16, sub_batch=2)
    ref = ce.forward_padded(model, x32)
    for k in range(3):
        assert whole[k].shape == (3, 256)
        assert _same(ones[k], whole[k]) and _same(twos[k], whole[k]) and _same(whole[k], ref[k])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def _trunk_f16in(e, x, B, H, W, feat):
    return e.lib.specmi_trunk_forward_f16in(e.h, C.c_void_p(x), B, H, W, _ptr(feat), e._stream())


def test_refusals_leave_the_handle_usable(eng, models16):
    cc16, hm16 = models16
    x32, x16 = _uint8_batch(eng, 1, 64, 96, seed=1)
    feat = torch.empty(1, 2, 3, 2048, device=DEV)
    # a handle committed at fp32
    cc32, _ = gpu_models(True, True, DEV)
    e32 = cc32.engine(torch.device(DEV))
    assert _trunk_f16in(e32, x16.data_ptr(), 1, 64, 96, feat) == _lib.ERR_STATE
    assert b'FP16' in e32.lib.specmi_last_error(e32.h)
    out = torch.empty(3, 1, 256, device=DEV)
    assert e32.lib.specmi_camcalib_forward_f16in(e32.h, _ptr(x16), 1, 64, 96, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), e32._stream()) == _lib.ERR_STATE
    assert torch.isfinite(e32.trunk(x32)).all() and e32.sync_status() == 0
    _, hm32 = gpu_models(True, True, DEV)
    eh = hm32.engine(torch.device(DEV))
    o = eh._hmr_outputs(1)
    outs = _lib.HmrOutputs(**{k: o[k].data_ptr() for k, _ in _lib.HmrOutputs._fields_})
    kw = _hmr_args(1)
    hmr_args = [_ptr(kw[k]) for k in ('cam_rotmat', 'cam_intrinsics', 'bbox_scale', 'bbox_center', 'img_w', 'img_h')]
    assert eh.lib.specmi_hmr_forward_f16in(eh.h, _ptr(x16), 1, 64, 96, *hmr_args, C.byref(outs), eh._stream()) == _lib.ERR_STATE
    assert torch.isfinite(hm32(x32, **kw)['smpl_vertices']).all() and eh.sync_status() == 0
    eh16 = hm16.engine(torch.device(DEV))
    assert eh16.lib.specmi_hmr_forward_f16in(eh16.h, C.c_void_p(x16.data_ptr() + 8), 1, 64, 96, *hmr_args, C.byref(outs), eh16._stream()) == _lib.ERR_ARG
    assert eh16.lib.specmi_hmr_forward_f16in(eh16.h, _ptr(x16), 1, 64, 96, *hmr_args, C.byref(outs), eh16._stream()) == _lib.OK
    assert torch.isfinite(o['smpl_vertices']).all()
    # an fp16 handle: misaligned pointer, H below 32 - and then a good call with the same buffers
    e16 = cc16.engine(torch.device(DEV))
    good = e16.trunk(x16)
    big = torch.zeros(x16.numel() + 8, dtype=torch.float16, device=DEV)
    assert _trunk_f16in(e16, big.data_ptr() + 8, 1, 64, 96, feat) == _lib.ERR_ARG
    assert b'aligned' in e16.lib.specmi_last_error(e16.h)
    assert _trunk_f16in(e16, x16.data_ptr(), 1, 31, 96, feat) == _lib.ERR_ARG
    assert _trunk_f16in(e16, x16.data_ptr(), 1, 64, 96, feat) == _lib.OK
    assert _same(feat, good) and e16.sync_status() == 0
    # the producers refuse a misaligned output
    frame = torch.zeros(40, 40, 3, dtype=torch.uint8, device=DEV)
    assert eng.lib.specmi_resize_normalize_f16(eng.h, _ptr(frame), 40, 40, 32, 32, C.c_void_p(big.data_ptr() + 8), None, eng._stream()) == _lib.ERR_ARG
    assert eng.lib.specmi_resize_normalize_f16(eng.h, _ptr(frame), 40, 40, 32, 32, _ptr(big), None, eng._stream()) == _lib.OK


def test_hrnet_handle_refuses_fp16_images(eng):
    from spec_amd import assets
    from spec_amd.modules import HMR
    assets.use_synthetic_assets(1003)
    hs = synth.hmr_state(1202, True, backbone='hrnet_w32-conv')
    hm = HMR(backbone='hrnet_w32-conv', use_cam=True, use_cam_feats=True)
    hm.load_state_dict({k: t(v) for k, v in hs.items()}, strict=False)
    e = hm.to(DEV).eval().engine(torch.device(DEV))
    x32, x16 = _uint8_batch(eng, 1, 224, 224, seed=2)
    feat = torch.empty(1, 7, 7, 480, device=DEV)
    assert _trunk_f16in(e, x16.data_ptr(), 1, 224, 224, feat) == _lib.ERR_STATE
    assert b'HRNet' in e.lib.specmi_last_error(e.h)
    assert torch.isfinite(e.trunk(x32)).all()
    with pytest.raises(ValueError, match='set_precision'):
        hm(x16)


def test_python_refuses_fp16_on_an_fp32_module_and_other_dtypes(eng, frames):
    from spec_amd.preprocess import camcalib_transform, crop_detections_batch
    cc32, hm32 = gpu_models(True, True, DEV)
    _, x16 = _uint8_batch(eng, 1, 64, 96, seed=1)
    for m in (cc32, hm32):
        with pytest.raises(ValueError, match='set_precision'):
            m(x16)
        with pytest.raises(ValueError, match='set_precision'):
            m.engine(torch.device(DEV)).trunk(x16)
    from spec_amd.pipeline import SpecPipeline
    x32 = torch.zeros(1, 3, 64, 96, device=DEV)
    kw = _hmr_args(1)
    with pytest.raises(ValueError, match='one layout'):       # a mixed pair is refused, not silently ungrouped
        SpecPipeline(cc32, hm32)(x32, kw['bbox_scale'], kw['bbox_center'], kw['img_w'], kw['img_h'], camcalib_images=x16)
    with pytest.raises(ValueError, match='dtype'):
        crop_detections_batch(frames, FIDX, BOXES, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='dtype'):
        camcalib_transform(frames[0], 48, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='dtype'):
        ce.pad_batch([np.zeros((40, 40, 3), np.uint8)], 48, 80, DEV, eng, dtype=torch.bfloat16)
