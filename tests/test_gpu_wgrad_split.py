"""The deterministic split of the weight gradient's contraction (``specmi_conv2d_wgrad_splits``, conv_gemm_kernel<2, true> and
conv_wgrad_reduce_kernel in spec_amd/csrc/conv_bwd.hip): where the rule keeps one launch, and on the smallest shapes above its
threshold (B OH >= 128 with fewer than 256 tiles) the split product against the float64 layer of tests/conv_grad_ref.py, within
the bound of tests/test_gpu_conv_backward.py, whose helpers run the cases."""
import pytest
import torch

from tests import bn_ref as N
from tests import conv_grad_ref as R
from tests.test_gpu_conv_backward import BOUND, _case, _engine, _ref, _run

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cout, k, stride): one segment list that divides by S, one that does not (129 = 4 * 32 + 1), and the stem's 7x7
SPLIT_CASES = [(2, 64, 3, 8, 8, 1, 1), (1, 129, 4, 5, 9, 3, 1), (4, 70, 6, 3, 16, 7, 2)]
# layer4 of ResNet-50 at B = 64 frames of 600 x 1000 (a 38 x 63 map in, 19 x 32 out)
LAYER4 = [(64, 38, 63, 1024, 512, 1, 1), (64, 38, 63, 512, 512, 3, 2), (64, 19, 32, 512, 2048, 1, 1), (64, 38, 63, 1024, 2048, 1, 2),
          (64, 19, 32, 2048, 512, 1, 1), (64, 19, 32, 512, 512, 3, 1)]


def _splits(shape):
    B, H, W, Cin, Cout, k, stride = shape
    return _engine().conv2d_wgrad_splits(B, H, W, Cin, Cout, k, stride, k // 2)


def _stage_layers(inplanes, planes, nblocks, stride, B, H, W):
    """The layer shapes of a stage of bottlenecks as the stage tests build it."""
    out, cin = [], inplanes
    for i in range(nblocks):
        s = stride if i == 0 else 1
        oh, ow = R.out_size(H, 3, s, 1), R.out_size(W, 3, s, 1)
        out += [(B, H, W, cin, planes, 1, 1), (B, H, W, planes, planes, 3, s), (B, oh, ow, planes, 4 * planes, 1, 1)]
        if i == 0 and (s != 1 or cin != 4 * planes):
            out.append((B, H, W, cin, 4 * planes, 1, s))
        cin, H, W = 4 * planes, oh, ow
    return out


def test_one_launch_where_the_rule_says_so():
    stage_cases = _stage_layers(64, 32, 3, 2, 2, 5, 6) + _stage_layers(**N.STAGE)          # tests/test_gpu_trunk_finetune.py, test_gpu_stage_batchnorm.py
    for shape in R.LAYER_CASES + stage_cases + LAYER4:
        assert _splits(shape) == 1, shape
    # B OH one below the threshold, and a product of exactly 256 tiles
    assert _splits((1, 127, 3, 8, 8, 1, 1)) == 1 and _splits((1, 128, 3, 8, 8, 1, 1)) > 1
    assert _splits((1, 512, 3, 512, 512, 1, 1)) == 1 and _splits((1, 512, 3, 512, 480, 1, 1)) > 1
    with pytest.raises(ValueError):
        _engine().conv2d_wgrad_splits(1, 128, 3, 8, 8, 5, 1, 2)


def test_the_split_cases_are_split():
    s = [_splits(shape) for shape in SPLIT_CASES]
    nseg = [shape[0] * R.out_size(shape[1], shape[5], shape[6], shape[5] // 2) for shape in SPLIT_CASES]
    print('S', s, 'B OH', nseg)
    assert all(v >= 2 for v in s) and max(s) >= 3 and any(n % v for n, v in zip(nseg, s))


@pytest.mark.parametrize('shape', SPLIT_CASES, ids=str)
def test_g_w_vs_float64_and_the_same_bits(shape):
    eng = _engine()
    _, d = _case(shape)
    full = _run(d, True, False, False)
    rgw = _ref(shape, True, False, False)[3]
    e = R.err(full[2], rgw)
    print(f'{shape} S={_splits(shape)}: g_w {e:.3g}')
    assert e < BOUND
    again = _run(d, True, False, False)
    assert torch.equal(full[2], again[2])                                    # two runs
    eng.profile(True)
    try:
        alone = _run(d, True, False, False, (False, True, False))            # without g_x: the same bits
        kernels = {r['kernel'] for r in eng.profile_read()}
    finally:
        eng.profile(False)
    assert torch.equal(full[2], alone[2])
    assert kernels == {'conv_train_fwd_wt', 'conv_train_fwd_gemm', 'conv_bwd_prep', 'conv_bwd_wgrad_gemm', 'conv_bwd_wgrad_reduce'}


@pytest.mark.parametrize('shape', SPLIT_CASES, ids=str)
def test_the_integer_case_bit_for_bit(shape):
    _, d = _case(shape, True)
    for relu, residual in ((True, True), (False, False)):
        g_w = _run(d, relu, residual, False)[2]
        assert torch.equal(g_w.cpu().double(), _ref(shape, relu, residual, False, True)[3])


def test_no_reduce_kernel_without_a_split():
    eng = _engine()
    shape = (2, 6, 5, 33, 32, 3, 2)
    _, d = _case(shape)
    _run(d, True, False, False)
    eng.profile(True)
    try:
        _run(d, True, False, False, (False, True, False))
        kernels = {r['kernel'] for r in eng.profile_read()}
    finally:
        eng.profile(False)
    assert _splits(shape) == 1 and 'conv_bwd_wgrad_reduce' not in kernels and 'conv_bwd_wgrad_gemm' in kernels
