"""Host-side half of the fp16 entrance (NHWC8 fp16 images, include/specmi.h): every new export is declared, exported and bound,
and the dtype / shape validation of spec_amd.preprocess and spec_amd.modules raises before any device call (CPU tensors here)."""
import os
import re

import numpy as np
import pytest
import torch

from spec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('specmi_crop_normalize_batch_f16', 'specmi_crop_resize_normalize_f16', 'specmi_resize_normalize_f16',
       'specmi_resize_normalize_ragged_f16', 'specmi_trunk_forward_f16in', 'specmi_camcalib_forward_f16in', 'specmi_hmr_forward_f16in')


def _declared():
    with open(os.path.join(ROOT, 'include', 'specmi.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    return set(re.findall(r'\b(specmi_\w+)\s*\(', text))


def test_new_exports_are_declared_exported_and_bound():
    declared = _declared()
    lib = _lib.load()
    for name in NEW:
        assert name in declared, f'{name} is not declared in include/specmi.h'
        assert name in _lib.PROTOTYPES, f'{name} has no prototype in spec_amd/_lib.py'
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    # every name with the new suffixes in the header is one of the seven, and each takes the arguments of its fp32 twin
    assert {n for n in declared if n.endswith('_f16in') or (n.endswith('_f16') and 'normalize' in n)} == set(NEW)
    for name in NEW:
        twin = name[:-len('_f16in')] if name.endswith('_f16in') else name[:-len('_f16')]
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES[twin][1]), (name, twin)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float64, torch.uint8, None])
def test_producers_refuse_other_dtypes_before_any_device_call(dtype):
    from spec_amd import preprocess
    from spec_amd.camcalib_eval import pad_batch
    frame = torch.zeros(40, 40, 3, dtype=torch.uint8)            # CPU tensors: a device call would raise RuntimeError instead
    slab = torch.zeros(2, 40, 40, 3, dtype=torch.uint8)
    dets = [[20., 20., 10., 10.]]
    calls = (lambda: preprocess.crop_detections(frame, dets, dtype=dtype),
             lambda: preprocess.crop_detections_batch(slab, [0], dets, dtype=dtype),
             lambda: preprocess.dataset_crops(frame, [[20., 20.]], [0.1], dtype=dtype),
             lambda: preprocess.camcalib_transform(frame, 32, dtype=dtype),
             lambda: preprocess.camcalib_transform_batch(slab, 32, dtype=dtype),
             lambda: pad_batch([np.zeros((40, 40, 3), np.uint8)], 32, 64, 'cuda:0', engine=object(), dtype=dtype))
    for call in calls:
        with pytest.raises(ValueError, match='dtype'):
            call()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_producers_accept_both_dtypes_up_to_the_device_check(dtype):
    from spec_amd import preprocess
    with pytest.raises(RuntimeError, match='device tensor'):
        preprocess.crop_detections(torch.zeros(40, 40, 3, dtype=torch.uint8), [[20., 20., 10., 10.]], dtype=dtype)


def _modules():
    from spec_amd import assets
    from spec_amd.modules import HMR, CameraRegressorNetwork
    assets.use_synthetic_assets(1003)
    return CameraRegressorNetwork(), HMR(use_cam=True, use_cam_feats=True)


def test_modules_refuse_fp16_images_at_fp32_and_wrong_shapes_before_any_device_call():
    cc, hm = _modules()
    x16 = torch.zeros(2, 64, 96, 8, dtype=torch.float16)        # on the CPU: reaching the engine would raise RuntimeError
    for m in (cc, hm):
        assert m.precision == 'fp32' and m.image_dtype == torch.float32
        with pytest.raises(ValueError, match='set_precision'):
            m(x16)
        m.set_precision('fp16')                                  # no engine yet: recorded for the next commit
        assert m.image_dtype == torch.float16
        for bad in (torch.zeros(2, 3, 64, 96, dtype=torch.float16), torch.zeros(2, 64, 96, 4, dtype=torch.float16),
                    torch.zeros(64, 96, 8, dtype=torch.float16)):
            with pytest.raises(ValueError, match='NHWC8'):
                m(bad)
        with pytest.raises(RuntimeError):                        # a well-formed fp16 batch gets as far as the device check
            m(x16)


def test_nhwc8_input_rule():
    from spec_amd.engine import nhwc8_input, out_dtype
    assert nhwc8_input(torch.zeros(1, 32, 32, 8, dtype=torch.float16), 'fp16') is True
    assert nhwc8_input(torch.zeros(1, 3, 32, 32), 'fp16') is False and nhwc8_input(torch.zeros(1, 3, 32, 32), 'fp32') is False
    assert out_dtype(torch.float16) is True and out_dtype(torch.float32) is False
    meta = torch.empty(4, 224, 224, 8, dtype=torch.float16, device='meta')
    assert nhwc8_input(meta, 'fp16') is True
    with pytest.raises(ValueError, match='set_precision'):
        nhwc8_input(meta, 'fp32')


def test_pipeline_image_dtype_follows_both_models():
    from spec_amd.pipeline import SpecPipeline
    cc, hm = _modules()
    pipe = SpecPipeline(cc, hm)
    assert pipe.image_dtype == torch.float32
    hm.set_precision('fp16')
    assert pipe.image_dtype == torch.float32                     # CamCalib reads the same crops and still runs at fp32
    cc.set_precision('fp16')
    assert pipe.image_dtype == torch.float16
