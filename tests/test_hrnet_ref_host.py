"""tests/hrnet_ref.py (the NumPy float64 references of HRNet's own kernels) against torch in float64 and against the exchange unit
of oracle/hrnet.py, and the exactness of every case tests/test_gpu_hrnet_kernels.py compares bit for bit.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import hrnet_ref as R

torch.set_grad_enabled(False)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


@pytest.mark.parametrize('B,H,W', R.STEM_SHAPES)
def test_stem_reference_is_torch_conv2d(B, H, W):
    rng = np.random.default_rng(B * 1000 + H * 37 + W)
    x, w = rng.standard_normal((B, 3, H, W)), rng.standard_normal((64, 3, 3, 3))
    scale, shift = rng.uniform(-2, 2, 64), rng.standard_normal(64)
    want = torch.relu(F.conv2d(t64(x), t64(w), stride=2, padding=1) * t64(scale).view(1, -1, 1, 1) + t64(shift).view(1, -1, 1, 1))
    want = want.permute(0, 2, 3, 1).numpy()
    got = R.stem3x3(x, w, scale, shift)
    assert got.shape == want.shape == (B, R.conv_out(H), R.conv_out(W), 64)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    wabs = F.conv2d(t64(np.abs(x)), t64(np.abs(w)), stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    assert np.abs(R.stem3x3_abs(x, w) - wabs).max() <= 1e-13 * wabs.max()


@pytest.mark.parametrize('B,H,W', R.STEM_SHAPES)
def test_stem_integer_cases_are_exact_in_fp32(B, H, W):
    """Borders loud, interior quiet, and sum |w||x| far below 2^24: every partial sum in any order, the scaled sum and the shifted
    one are fp32 numbers, so the float64 reference is what an fp32 evaluation gives, fused or not."""
    x, w, scale, shift = R.stem_integer_operands(B, H, W, seed=H * 100 + W)
    assert np.abs(x[:, :, 0]).min() == 8 and np.abs(x[:, :, -1]).min() == 8 and np.abs(x[..., 0]).min() == 8 and np.abs(x[..., -1]).min() == 8
    if H > 2 and W > 2:
        assert np.abs(x[:, :, 1:-1, 1:-1]).max() <= 1
    assert np.all(x == np.round(x)) and np.all(w == np.round(w)) and np.abs(w).max() <= 4
    assert set(np.unique(scale)) <= set(R.STEM_SCALES) and np.all(shift == np.round(shift))
    S = R.stem3x3_abs(x, w)
    assert S.max() <= 864 < 2 ** 24
    acc = R._stem_acc(x, w)
    assert np.all(acc == np.round(acc)) and R.is_exact_in_f32(acc * scale) and R.is_exact_in_f32(acc * scale + shift)
    assert R.is_exact_in_f32(R.stem3x3(x, w, scale, shift))


@pytest.mark.parametrize('hw,ohw', R.RESIZE_EXACT_CASES + R.RESIZE_BOUNDED_CASES + [((5, 9), (11, 4)), ((2, 3), (7, 7))])
def test_resize_reference_is_torch_interpolate(hw, ohw):
    (H, W), (OH, OW) = hw, ohw
    x = np.random.default_rng(H * 31 + W * 7 + OH).standard_normal((2, H, W, 8))
    want = F.interpolate(t64(x).permute(0, 3, 1, 2), size=(OH, OW), mode='bilinear', align_corners=True).permute(0, 2, 3, 1).numpy()
    got = R.resize_ac(x, OH, OW)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-13 * np.abs(x).max()


def test_resize_exact_cases_cover_the_axes_and_differ_in_h_and_w():
    axes_h = {(h, oh) for (h, w), (oh, ow) in R.RESIZE_EXACT_CASES}
    axes_w = {(w, ow) for (h, w), (oh, ow) in R.RESIZE_EXACT_CASES}
    assert axes_h == axes_w == set(R.RESIZE_EXACT_AXES)           # every axis geometry runs along H and along W
    assert all((h, oh) != (w, ow) for (h, w), (oh, ow) in R.RESIZE_EXACT_CASES)
    # the geometries of the 'interp' head at trunk inputs 32, 64 and 96: levels 8 / 4 / 2 (x 1, 2, 3) -> 1, 2, 3
    assert {(l * k, k) for k in (1, 2, 3) for l in (8, 4, 2)} <= set(R.RESIZE_EXACT_AXES)


@pytest.mark.parametrize('hw,ohw', R.RESIZE_EXACT_CASES)
def test_resize_exact_cases_are_exact_in_fp32(hw, ohw):
    """Integer or half-integer scales: the weights are 0, 0.5 or 1, the data integers up to 64 - every product and sum is a multiple
    of 0.25 below 2^8, hence exact in fp32, and so is the scale itself ((in-1)/(out-1) as an fp32 quotient) and scale * o."""
    (H, W), (OH, OW) = hw, ohw
    for n_in, n_out in (hw[0], ohw[0]), (hw[1], ohw[1]):
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        assert scale * 2 == round(scale * 2)
        assert np.float32(n_in - 1) / np.float32(max(n_out - 1, 1)) == (scale if n_out > 1 else n_in - 1)
    x = R.resize_integer_input(3, H, W, 32, seed=H * 100 + W)
    ref = R.resize_ac(x, OH, OW)
    assert np.all(ref * 4 == np.round(ref * 4)) and R.is_exact_in_f32(ref)


SH_SETS = [(0, 1), (0, 0), (0, 1, 2), (0, 0, 1), (0, 0, 0), (0, 1, 2, 3), (0, 0, 1, 2), (0, 0, 0, 1), (0, 0, 0, 0)]


def test_fuse_reference_float32_variant_adds_in_the_stated_order():
    rng = np.random.default_rng(5)
    terms = [(rng.standard_normal((2, 8 >> s, 16 >> s, 8)) * 10.0 ** e).astype(np.float32) for s, e in zip((0, 1, 2, 3), (3, -3, 0, 1))]
    sh = (0, 1, 2, 3)
    up = [R.upsample_nearest(t, s) for t, s in zip(terms, sh)]
    want = ((up[0] + up[1]) + up[2]) + up[3]
    assert want.dtype == np.float32
    got = R.fuse_sum_f32(terms, sh, False)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    other = up[0] + (up[1] + (up[2] + up[3]))
    assert not np.array_equal(other, want)            # the order is visible in these operands
    assert np.array_equal(R.fuse_sum_f32(terms, sh, True), np.maximum(want, np.float32(0)))
    assert np.abs(R.fuse_sum(terms, sh, False) - want).max() <= 4 * 2.0 ** -24 * sum(np.abs(u).max() for u in up)
    # nearest upsampling: pixel (y, x) reads (y >> sh, x >> sh)
    y, x = np.meshgrid(np.arange(8), np.arange(16), indexing='ij')
    assert np.array_equal(up[2], terms[2][:, y >> 2, x >> 2])


@pytest.mark.parametrize('width', [32, 48])
@pytest.mark.parametrize('nb,H,W', [(2, 8, 16), (3, 16, 8), (4, 8, 24), (4, 8, 8)])
def test_fuse_reference_is_the_oracles_exchange_unit(nb, H, W, width):
    """HighResolutionModule.forward of oracle/hrnet.py with its branches replaced by the identity is the exchange unit alone: the
    reference's sum of the same terms (each fuse layer's conv + BN output, before its Upsample) must reproduce every output level."""
    from oracle.hrnet import HighResolutionModule
    torch.manual_seed(nb * 100 + H + W + width)
    C = [width << l for l in range(nb)]
    m = HighResolutionModule(nb, [4] * nb, C).eval().double()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_()
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.normal_()
            mod.bias.data.normal_()
    m.branches = torch.nn.ModuleList([torch.nn.Identity() for _ in range(nb)])
    x = [torch.randn(2, C[l], H >> l, W >> l, dtype=torch.float64) for l in range(nb)]
    want = m(list(x))
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().numpy()
    for i in range(nb):
        terms, sh = [], []
        for j in range(nb):
            if j == i:
                terms.append(nhwc(x[j])); sh.append(0)
            elif j > i:
                seq = m.fuse_layers[i][j]
                assert isinstance(seq[2], torch.nn.Upsample) and seq[2].scale_factor == 2 ** (j - i) and seq[2].mode == 'nearest'
                terms.append(nhwc(seq[1](seq[0](x[j])))); sh.append(j - i)
            else:
                terms.append(nhwc(m.fuse_layers[i][j](x[j]))); sh.append(0)
        assert tuple(sh) in SH_SETS
        got = R.fuse_sum(terms, sh, True)
        assert got.shape == nhwc(want[i]).shape
        assert np.abs(got - nhwc(want[i])).max() <= 1e-12 * np.abs(nhwc(want[i])).max()
