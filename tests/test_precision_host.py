"""fp16 trunk (the reference's TRAINING.USE_AMP switch), host side: the C ABI surface, argument validation, the evaluation's
precision decision and the test-side fp16 reference.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('specmi_set_precision', 'specmi_get_precision', 'specmi_conv2d_f16', 'specmi_maxpool3x3s2_f16', 'specmi_to_nhwc_f16')


@pytest.fixture(scope='module')
def lib():
    from spec_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_precision_symbols_exported_prototyped_documented(lib):
    from spec_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
        assert re.search(r'\bint ' + name + r'\(', hdr), name
    assert re.search(r'SPECMI_PRECISION_FP32 = 0', hdr) and re.search(r'SPECMI_PRECISION_FP16 = 1', hdr)
    assert (_lib.PRECISION_FP32, _lib.PRECISION_FP16) == (0, 1)
    assert 'conv_f16.hip' in open(os.path.join(ROOT, 'spec_amd', 'build.py')).read()


def test_null_handle_is_refused(lib):
    import ctypes as C
    from spec_amd import _lib
    assert lib.specmi_set_precision(None, 1) == _lib.ERR_ARG
    v = C.c_int(7)
    assert lib.specmi_get_precision(None, C.byref(v)) == _lib.ERR_ARG


def test_set_precision_validates_its_argument():
    from spec_amd import assets
    from spec_amd.modules import HMR, CameraRegressorNetwork
    from tests.util import SEED_SMPL
    assets.use_synthetic_assets(SEED_SMPL)
    cc = CameraRegressorNetwork()
    for bad in ('bf16', 'FP16', 16, None):
        with pytest.raises(ValueError):
            cc.set_precision(bad)
    assert cc.precision == 'fp32'
    cc.set_precision('fp16')                 # no engine yet: recorded, packed at the first commit
    assert cc.precision == 'fp16'
    cc.set_precision('fp32')
    assert cc.precision == 'fp32'
    hm = HMR(backbone='hrnet_w32-conv')
    with pytest.raises(NotImplementedError):
        hm.set_precision('fp16')
    assert hm.precision == 'fp32'
    hm.set_precision('fp32')


def test_engine_precision_names():
    from spec_amd.engine import Engine
    assert Engine.PRECISIONS == {'fp32': 0, 'fp16': 1}


@pytest.mark.parametrize('opts,expected', [(['TRAINING.USE_AMP', 'True'], 'fp16'), (['TRAINING.USE_AMP', 'False'], 'fp32'),
                                           ([], 'fp32'), (['TRAINING.USE_AMP', 'true'], 'fp16')])
def test_eval_precision_from_config(opts, expected):
    from spec_amd import evaluation
    hp = evaluation.load_config(None, opts)
    assert evaluation.DEFAULTS['TRAINING']['USE_AMP'] is False
    assert evaluation.eval_precision(hp) == expected


def test_eval_precision_absent_key():
    from spec_amd import evaluation
    assert evaluation.eval_precision({'TRAINING': {}}) == 'fp32'
    assert evaluation.eval_precision({}) == 'fp32'


def test_fp16_reference_differs_from_fp64_by_an_fp16_class_amount():
    """The test-side reference rounds where the contract rounds: fp16-class error on a ResNet-50 trunk (2^-11 per rounding,
    ~50 roundings on the path), not zero and not more."""
    from spec_amd import synth
    from tests import fp16_ref
    sd, _ = synth.resnet_family_state(1001, 'resnet50', 'backbone.')
    x = synth.images(5, 1)[:, :, :64, :64].astype(np.float64)
    with torch.inference_mode():
        a = fp16_ref.trunk(sd, x)
        b = fp16_ref.trunk_fp64(sd, x)
    assert a.shape == b.shape == (1, 2048, 2, 2)
    err = float(np.abs(a - b).max() / np.abs(b).max())
    assert 1e-5 < err < 2e-2, err
    # fp16-rounding is what the reference does to its intermediate maps: the image is rounded exactly once
    assert np.array_equal(fp16_ref.f16(np.float64(1.0) + 2.0 ** -12), 1.0)        # a tie rounds to even
    assert fp16_ref.f16(2.0 ** -24) == 2.0 ** -24 and fp16_ref.f16(2.0 ** -26) == 0.0
    with np.errstate(over='ignore'):
        assert np.isinf(fp16_ref.f16(65520.0)) and fp16_ref.f16(65519.0) == 65504.0
