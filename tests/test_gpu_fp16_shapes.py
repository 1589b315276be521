"""The fp16 conv path (conv_f16.hip) away from the ResNet-50 shapes, on the MI355X.  Products are fp16 x fp16 accumulated in fp32:
with small-integer operands every partial sum is exact in any order, so the device must equal a float64 reference BIT FOR BIT -
ragged shapes, every tail, every kernel instance, the weight rounding and layout, the batch split beyond 2 GiB and the two small
kernels are all compared without a tolerance.  The only tolerances here are the two the project already owns: _check's derived
bound (realistic magnitudes, where fp32 accumulation rounds) and TRUNK_BAR (whole trunks of the other depths).

Measured on MI355X: the file (128 tests) takes 12.4 s; the batch-split test peaks at 6.1 GiB of device memory (the x2 case)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spec_amd import synth
from tests import fp16_ref
from tests.fp16_ref import DEV, _check, _run_shape, conv_out
from tests.test_gpu_fp16 import TRUNK_BAR
from tests.util import cpu_threads, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CASES = fp16_ref.shape_cases()


@pytest.fixture(scope='module')
def eng():
    from spec_amd.engine import Engine
    e = Engine('camcalib', torch.device(DEV))
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def _assert_bit_exact(y, ref, out32, what=''):
    """y as the device stored it (float32 or float16 ndarray) against the float64 reference: the values themselves for fp32, the
    bits of fp16_rne(ref) for fp16 (inf included).  A mismatch names its first indices."""
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    if out32:
        assert y.dtype == np.float32
        bad = y.astype(np.float64) != ref
    else:
        assert y.dtype == np.float16
        with np.errstate(over='ignore'):
            bad = _bits(y) != _bits(ref.astype(np.float16))
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError((what, int(bad.sum()), 'of', bad.size, 'first (b, oy, ox, n)', idx[:8].tolist(),
                              'got', y[bad][:8].tolist(), 'want', ref[bad][:8].tolist()))


def _ref(c, o):
    with cpu_threads():
        return fp16_ref.layer_reference(o, c['stride'], c['pad'], c['relu'], c['ds'][3] if c['ds'] else 1)


# ---- a. exact-integer fuzz ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=fp16_ref.case_id)
def test_conv_f16_integer_cases_bit_exact(eng, c):
    o = fp16_ref.integer_operands(c)
    _assert_bit_exact(fp16_ref.run_case(eng, c, o), _ref(c, o), c['out32'], fp16_ref.case_id(c))


def _ones_conv(eng, x, scale=1.0, out32=False, cout=64):
    """x (B,H,W,8) float64 through a 1x1 conv of ones: every output channel is scale * the channel sum of its pixel."""
    cin = x.shape[-1]
    return eng.conv2d_f16(torch.from_numpy(x).half().to(DEV), np.ones((cout, cin, 1, 1), np.float32), np.full(cout, scale, np.float32),
                          np.zeros(cout, np.float32), 1, 0, relu=False, out_f32=out32).cpu().numpy()


def test_conv_f16_store_ties_round_to_even(eng):
    x, sums, want = fp16_ref.tie_case()
    y = _ones_conv(eng, x)
    assert np.array_equal(_bits(y), _bits(np.broadcast_to(want[None, None, :, None], y.shape))), y[0, 0, :, 0]
    assert np.array_equal(_ones_conv(eng, x, out32=True)[0, 0, :, 0].astype(np.float64), sums)      # the fp32 store keeps the sum


def test_conv_f16_subnormal_sums_through_the_fp16_store(eng):
    """Sums of a few multiples of 2^-24: with scale 1 they are fp16 subnormals (or the first normals) and come back as they are;
    with scale 0.5 the odd ones are ties between two subnormals, 2^-25 is the tie to zero - all rounded to nearest even."""
    rng = np.random.default_rng(9)
    n = rng.integers(0, 130, (1, 5, 7, 8)).astype(np.float64)
    n[0, 0, 0] = (1, 0, 0, 0, 0, 0, 0, 0)              # 2^-24, and 2^-25 when halved: the tie to zero
    n[0, 0, 1] = (1, 2, 0, 0, 0, 0, 0, 0)              # 3 * 2^-25: the tie between 2^-24 and 2^-23, rounds to 2^-23
    n[0, 0, 2] = (1023, 1, 0, 0, 0, 0, 0, 0)           # 2^-14: the first normal
    n[0, 0, 3] = (1023, 1022, 2, 0, 0, 0, 0, 0)        # 2047 * 2^-24 (a normal with spacing 2^-24); halved: a tie again
    for scale in (1.0, 0.5):
        exact = n.sum(-1, keepdims=True) * 2.0 ** -24 * scale
        y = _ones_conv(eng, n * 2.0 ** -24, scale)
        _assert_bit_exact(y, np.broadcast_to(exact, y.shape), False, 'scale %g' % scale)
        assert np.array_equal(_ones_conv(eng, n * 2.0 ** -24, scale, out32=True).astype(np.float64), np.broadcast_to(exact, y.shape))
    assert np.array_equal(fp16_ref.f16(np.array([1.0, 3.0, 2047.0]) * 2.0 ** -25), np.array([0.0, 2.0, 1024.0]) * 2.0 ** -24)


def test_conv_f16_overflow_stores_inf(eng):
    """overflow follows IEEE (inf), no clamping.  65519 is the last sum that stays finite, 65520 the tie that goes up."""
    x = np.zeros((1, 1, 6, 8))
    x[0, 0, :, 0] = (65504, 65504, 16384, -65504, -65504, -16384)
    x[0, 0, :, 1] = (15, 16, 16384, -15, -16, -16384)
    x[0, 0, 2, 2:] = 16384
    x[0, 0, 5, 2:] = -16384
    y = _ones_conv(eng, x)[0, 0, :, 5].astype(np.float64)
    assert np.array_equal(y, np.array([65504.0, np.inf, np.inf, -65504.0, -np.inf, -np.inf])), y
    y = _ones_conv(eng, x, out32=True)[0, 0, :, 5].astype(np.float64)
    assert np.array_equal(y, x.sum(-1)[0, 0]), y
    # ReLU and the residual act before the store: a residual that brings the sum back below 65520 keeps it finite
    res = torch.full((1, 1, 6, 64), -16.0, dtype=torch.float16, device=DEV)
    y = eng.conv2d_f16(torch.from_numpy(x).half().to(DEV), np.ones((64, 8, 1, 1), np.float32), np.ones(64, np.float32), np.zeros(64, np.float32),
                       1, 0, residual=res, relu=True).cpu().numpy()[0, 0, :, 9].astype(np.float64)
    assert np.array_equal(y, np.array([65504.0, 65504.0, np.inf, 0.0, 0.0, 0.0])), y


@pytest.mark.parametrize('cin,k,stride,H,W', [(8, 3, 2, 6, 5), (3, 7, 3, 11, 9), (12, 3, 3, 7, 7)])
def test_conv_f16_padding_octets_read_nothing(eng, cin, k, stride, H, W):
    """K is padded to a multiple of 32: the octets past the last tap carry zero weights, and their A side must read zeros too -
    not whatever image row a tap index beyond the filter happens to address (0 x NaN is NaN).  The last image row is one that no
    real tap reaches (pad 0, (H - k) % stride != 0) and is filled with NaN; the outputs must not notice."""
    assert (H - k) % stride and (k * k * (-(-cin // 8) * 8)) % 32
    c = dict(B=2, H=H, W=W, cin=cin, cout=64, k=k, stride=stride, pad=0, res=False, relu=False, out32=True, ds=None, seed=77)
    o = fp16_ref.integer_operands(c)
    o['x'][:, (conv_out(H, k, stride, 0) - 1) * stride + k:] = 0.0
    ref = _ref(c, o)
    o['x'][:, (conv_out(H, k, stride, 0) - 1) * stride + k:] = np.nan
    y = fp16_ref.run_case(eng, c, o)
    assert not np.isnan(y).any(), np.argwhere(np.isnan(y))[:8].tolist()
    _assert_bit_exact(y, ref, True)


# ---- b. every template instance is run -----------------------------------------------------------------------------------------
def test_conv_f16_every_instance_is_used(eng):
    seen = {}
    eng.profile(True)
    try:
        eng.profile_read()
        for inst, name in fp16_ref.INSTANCE_NAMES.items():
            c = min((c for c in CASES if fp16_ref.instance(c) == inst), key=lambda c: c['B'] * c['H'] * c['W'] * c['cin'] * c['k'] ** 2)
            o = fp16_ref.integer_operands(c)
            y = fp16_ref.run_case(eng, c, o)
            names = [e['kernel'] for e in eng.profile_read()]
            assert names == [name], (fp16_ref.case_id(c), names)
            seen[name] = fp16_ref.case_id(c)
            _assert_bit_exact(y, _ref(c, o), c['out32'], name)
    finally:
        eng.profile(False)
    assert sorted(seen) == sorted(fp16_ref.INSTANCE_NAMES.values()), seen


# ---- c. weight rounding and layout -------------------------------------------------------------------------------------------
def _probe_values():
    """float32 values around every rounding decision of binary16: the midpoint of each pair of adjacent finite non-negative fp16
    values (exact in float32; the first one, 2^-25, is the tie to zero), its two float32 neighbours, every fp16 value itself,
    the neighbourhoods of 2^-14, 2^-24, 2^-25, 65504 and the largest float32 below 65520 (rounds to 65504); both signs."""
    h = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64) * 2, h[:-1].astype(np.float64) + h[1:].astype(np.float64))
    inf = np.float32(np.inf)
    around = lambda v: [np.nextafter(np.float32(v), -inf), np.float32(v), np.nextafter(np.float32(v), inf)]
    special = around(2.0 ** -14) + around(2.0 ** -24) + around(2.0 ** -25) + around(2.0 ** -26) + around(1.5 * 2.0 ** -24) + \
        around(65504.0)[:2] + [np.nextafter(np.float32(65504.0), inf), np.nextafter(np.float32(65520.0), -inf), np.float32(65519.0)]
    v = np.concatenate([mid, np.nextafter(mid, inf), np.nextafter(mid, -inf), h, np.asarray(special, np.float32)])
    assert np.abs(v).max() < 65520.0
    return np.concatenate([v, -v])


def test_f16_weight_packing_matches_numpy_rne(eng):
    """A 1x1 conv of the identity (pixel i has channel i = 1, shift 0, no ReLU, fp32 out) returns the packed weight matrix:
    y[0, 0, i, n] = fp16(w[n, i] * scale[n]).  The truth is numpy's single rounding of the float64 product, which is exact.
    (A weight that rounds to -0 comes back as +0: it is added to the accumulator's +0.  Zeros are compared as values.)"""
    cin, cout = 256, 2048
    v = _probe_values()
    assert v.size <= cin * cout
    w = np.zeros(cin * cout, np.float32)
    w[:v.size] = v
    w = w.reshape(cout, cin, 1, 1)
    x = torch.eye(cin, dtype=torch.float16, device=DEV).view(1, 1, cin, cin)
    rng = np.random.default_rng(4)
    for scale in (np.ones(cout, np.float32), (0.5 + 0.5 * rng.random(cout)).astype(np.float32)):
        y = eng.conv2d_f16(x, w, scale, np.zeros(cout, np.float32), 1, 0, relu=False, out_f32=True).cpu().numpy()[0, 0]      # (i, n)
        want = (w[:, :, 0, 0].astype(np.float64) * scale.astype(np.float64)[:, None]).astype(np.float16).T
        assert np.array_equal(y.astype(np.float16).astype(np.float32), y), 'an fp32 output that is not an fp16 value'
        got, wb = _bits(y.astype(np.float16)), _bits(want)
        got[y == 0], wb[want == 0] = 0, 0
        bad = got != wb
        assert not bad.any(), (int(bad.sum()), [(float(w[n, i, 0, 0]), float(scale[n]), float(y[i, n]), float(want[i, n])) for i, n in np.argwhere(bad)[:8]])


@pytest.mark.parametrize('cin,cout', [(3, 64), (12, 16)])
def test_f16_weight_layout_3x3_tap_by_tap(eng, cin, cout):
    """k = 3 with a unique small-integer code per (n, ci, ky, kx) and one-hot inputs: image ci has a 1 at pixel (2, 2), channel ci,
    so output (oy, ox, n) is the code of (n, ci, 3 - oy, 3 - ox) and nothing else - the (ky, kx, ci) order of K.  A second set of
    images puts the 1 into the channels past Cin: their weights are the zero padding of the layout, and every output is 0."""
    cp = -(-cin // 8) * 8
    code = 1.0 + np.arange(cout * cin * 9, dtype=np.float64).reshape(cout, cin, 3, 3)
    assert code.max() <= 2048
    x = np.zeros((cp, 5, 5, cp))
    x[np.arange(cp), 2, 2, np.arange(cp)] = 1.0
    y = eng.conv2d_f16(torch.from_numpy(x).half().to(DEV), code.astype(np.float32), np.ones(cout, np.float32), np.zeros(cout, np.float32),
                       1, 1, relu=False, out_f32=True).cpu().numpy().astype(np.float64)
    want = np.zeros((cp, 5, 5, cout))
    for ci in range(cin):
        for ky in range(3):
            for kx in range(3):
                want[ci, 3 - ky, 3 - kx] = code[:, ci, ky, kx]
    assert np.array_equal(y, want), np.argwhere(y != want)[:8].tolist()
    with cpu_threads():
        ref = fp16_ref.layer_reference(dict(x=x[:cin, :, :, :cin], w=code, scale=np.ones(cout), shift=np.zeros(cout)), 1, 1, False)
    assert np.array_equal(y[:cin], ref)


# ---- d. ragged shapes at realistic magnitudes ---------------------------------------------------------------------------------
@pytest.mark.parametrize('c', fp16_ref.shape_cases(24, seed=20240608), ids=fp16_ref.case_id)
def test_conv_f16_random_shapes(eng, c):
    with cpu_threads():
        y, ref, bound = _run_shape(eng, c['cin'], c['cout'], c['k'], c['stride'], c['pad'], c['H'], c['W'], c['B'], c['res'], c['relu'],
                                   c['out32'], c['ds'], seed=c['seed'])
    print('random shape', fp16_ref.case_id(c), 'max err / bound', _check(y, ref, bound, c['out32']))


# ---- e. the batch split beyond 2 GiB --------------------------------------------------------------------------------------------
def _run_split(eng, c, o, b0, b1):
    sl = lambda a: None if a is None else a[b0:b1]
    kw = dict(x2=sl(o['x2']), w2_oihw=o['w2'].astype(np.float32), stride2=c['ds'][3]) if c['ds'] else {}
    return eng.conv2d_f16(sl(o['x']), o['w'].astype(np.float32), o['scale'].astype(np.float32), o['shift'].astype(np.float32), c['stride'],
                          c['pad'], residual=sl(o['res']), relu=c['relu'], out_f32=c['out32'], **kw)


@pytest.mark.parametrize('c', fp16_ref.SPLIT_CASES, ids=lambda c: c['side'])
def test_conv_f16_batch_split_beyond_2gib(eng, c):
    """launch_conv_f16 cuts the batch into launches of whole images so that 32-bit buffer offsets suffice, and addresses the output
    with size_t.  Integer operands, built on the device: the images on both sides of every boundary (and the first and last) equal
    the float64 CPU reference bit for bit, and the whole result equals the same call made in chunks of 32 images."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    o = fp16_ref.split_operands(c, c['B'], DEV)
    y = _run_split(eng, c, o, 0, c['B'])
    probes = fp16_ref.split_probe_images(c)
    with cpu_threads():
        ref = fp16_ref.split_reference(c, o, probes)
    _assert_bit_exact(y[probes].cpu().numpy(), ref, c['out32'], 'images %s' % probes)
    for b0 in range(0, c['B'], 32):
        b1 = min(b0 + 32, c['B'])
        part = _run_split(eng, c, o, b0, b1)
        assert torch.equal(part, y[b0:b1]), (c['side'], 'images', b0, b1, torch.nonzero((part != y[b0:b1]).flatten(1).any(1)).flatten().tolist())
        del part
    print('batch split', c['side'], 'images per launch', fp16_ref.split_images_per_launch(c), 'probes', probes,
          'peak device memory %.2f GiB' % (torch.cuda.max_memory_allocated() / 2 ** 30))
    del o, y
    torch.cuda.empty_cache()


# ---- f. refusals ----------------------------------------------------------------------------------------------------------------
def test_conv_f16_unsupported_shapes_are_refused(eng):
    """conv_f16_shape_ok sits in front of the launch: each of these is an argument error, nothing is launched, and the handle
    serves a valid call right after with the right bits."""
    from spec_amd import _lib
    ok = next(c for c in CASES if c['ds'] and c['res'])
    good = fp16_ref.integer_operands(ok)
    good_ref = _ref(ok, good)
    h16 = lambda *s: torch.ones(*s, dtype=torch.float16, device=DEV)
    ones = lambda cout, cin: (np.ones((cout, cin, 1, 1), np.float32), np.ones(cout, np.float32), np.zeros(cout, np.float32))
    w2 = lambda cout, cin2: dict(w2_oihw=np.ones((cout, cin2, 1, 1), np.float32))
    misaligned = torch.ones(4 + 4 * 4 * 32, dtype=torch.float16, device=DEV)[4:].view(1, 4, 4, 32)
    assert misaligned.data_ptr() % 16 == 8 and misaligned.is_contiguous()
    refused = {
        'Cout % 4 != 0': lambda: eng.conv2d_f16(h16(1, 4, 4, 32), *ones(6, 32), 1, 0),
        'two sources with fp32 out': lambda: eng.conv2d_f16(h16(1, 4, 4, 32), *ones(64, 32), 1, 0, out_f32=True, x2=h16(1, 4, 4, 32), **w2(64, 32)),
        'two sources, Cin % 32 != 0': lambda: eng.conv2d_f16(h16(1, 4, 4, 16), *ones(64, 16), 1, 0, x2=h16(1, 4, 4, 32), **w2(64, 32)),
        'two sources, Cin2 % 32 != 0': lambda: eng.conv2d_f16(h16(1, 4, 4, 32), *ones(64, 32), 1, 0, x2=h16(1, 4, 4, 16), **w2(64, 16)),
        'x2 one row short of (OH - 1) * stride2': lambda: eng.conv2d_f16(h16(1, 4, 4, 32), *ones(64, 32), 1, 0, x2=h16(1, 6, 7, 32), stride2=2, **w2(64, 32)),
        'x2 one column short of (OW - 1) * stride2': lambda: eng.conv2d_f16(h16(1, 4, 4, 32), *ones(64, 32), 1, 0, x2=h16(1, 7, 6, 32), stride2=2, **w2(64, 32)),
        'x offset by 8 bytes': lambda: eng.conv2d_f16(misaligned, *ones(64, 32), 1, 0),
    }
    for what, call in refused.items():
        with pytest.raises(_lib.SpecmiError) as ei:
            call()
        assert ei.value.code == _lib.ERR_ARG, (what, ei.value)
        _assert_bit_exact(fp16_ref.run_case(eng, ok, good), good_ref, ok['out32'], 'after: ' + what)
    # the neighbours of the refused x2 sizes are served: exactly (OH - 1) * stride2 + 1 rows and columns
    y = eng.conv2d_f16(h16(1, 4, 4, 32), *ones(64, 32), 1, 0, relu=False, x2=h16(1, 7, 7, 32), stride2=2, **w2(64, 32)).cpu().numpy()
    assert np.array_equal(y.astype(np.float64), np.full((1, 4, 4, 64), 64.0))


# ---- g. the two small kernels ------------------------------------------------------------------------------------------------
def _pool_maps(shape, seed):
    """fp16 maps as float64: mixed signs, all negative (a zero-padded pool would answer 0), and all negative with -65504 and
    negative subnormals mixed in.  No zeros: the max of -0 and +0 has no agreed sign."""
    rng = np.random.default_rng(seed)
    mixed = fp16_ref.f16(rng.standard_normal(shape) * 3)
    mixed[mixed == 0] = 1.0
    neg = fp16_ref.f16(-np.abs(mixed) - 2.0 ** -10)
    edge = np.where(rng.random(shape) < 0.3, -65504.0, np.where(rng.random(shape) < 0.5, -rng.integers(1, 1024, shape) * 2.0 ** -24, neg))
    tiny = rng.integers(1, 1024, shape) * 2.0 ** -24 * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return {'mixed': mixed, 'negative': neg, 'negative, -65504 and subnormals': edge, 'subnormals of both signs': tiny}


@pytest.mark.parametrize('shape', [(2, 112, 112, 64), (1, 300, 533, 64), (3, 7, 5, 8), (1, 1, 9, 16), (2, 9, 1, 8), (1, 2, 2, 24), (1, 1, 1, 8)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_f16_bit_exact(eng, shape):
    for what, x in _pool_maps(shape, sum(shape)).items():
        assert np.array_equal(fp16_ref.f16(x), x)
        y = eng.maxpool_f16(torch.from_numpy(x).half().to(DEV)).cpu().numpy()
        ref = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
        assert y.shape == ref.shape == (shape[0], (shape[1] - 1) // 2 + 1, (shape[2] - 1) // 2 + 1, shape[3])
        bad = _bits(y) != _bits(ref.astype(np.float16))
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist(), y[bad][:8].tolist(), ref[bad][:8].tolist())


def test_maxpool_f16_refuses_a_channel_count_off_the_octet(eng):
    from spec_amd import _lib
    with pytest.raises(_lib.SpecmiError) as ei:
        eng.maxpool_f16(torch.zeros(1, 4, 4, 12, dtype=torch.float16, device=DEV))
    assert ei.value.code == _lib.ERR_ARG


@pytest.mark.parametrize('B,C,H,W', [(2, 3, 17, 23), (1, 1, 5, 3), (3, 8, 9, 11), (1, 3, 225, 301)])
def test_to_nhwc_f16_bit_exact(eng, B, C, H, W):
    """fp32 NCHW image -> fp16 NHWC, 8 channels: numpy's float32 -> float16 (round to nearest even, |v| >= 65520 to inf, subnormals
    kept, -0 kept) bit for bit, the channels past C exactly +0."""
    rng = np.random.default_rng(B + C + H + W)
    x = (rng.standard_normal((B, C, H, W)) * 4).astype(np.float32)
    v = _probe_values()
    big = np.array([65520.0, 7e4, 1e5, 3.4e38, -65520.0, -7e4, -3.4e38, np.nextafter(np.float32(65520.0), np.float32(0)), 0.0, -0.0], np.float32)
    inject = np.concatenate([rng.choice(v, min(x.size // 2, 4096)), big[:min(len(big), x.size // 4)]])
    flat = x.reshape(-1)
    flat[rng.choice(x.size, inject.size, replace=False)] = inject
    y = eng.to_nhwc_f16(torch.from_numpy(x)).cpu().numpy()
    assert y.shape == (B, H, W, 8) and y.dtype == np.float16
    with np.errstate(over='ignore'):
        want = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float16)
    bad = _bits(y[..., :C]) != _bits(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist(), x.transpose(0, 2, 3, 1)[bad][:8].tolist(), y[..., :C][bad][:8].tolist())
    assert not _bits(y[..., C:]).any()
    if x.size >= 64:
        assert np.isinf(want).any() and (np.abs(want[want != 0]) < 2.0 ** -14).any()


def test_to_nhwc_f16_refuses_more_than_eight_channels(eng):
    from spec_amd import _lib
    with pytest.raises(_lib.SpecmiError) as ei:
        eng.to_nhwc_f16(torch.zeros(1, 9, 4, 4))
    assert ei.value.code == _lib.ERR_ARG


# ---- h. fp16 trunks of the other depths -----------------------------------------------------------------------------------------
def _trunk_model(depth):
    from spec_amd import assets
    from spec_amd.modules import HMR, CameraRegressorNetwork
    from tests.util import SEED_SMPL
    assets.use_synthetic_assets(SEED_SMPL)
    if depth == 101:
        sd = synth.hmr_state(1801, True, backbone='resnet101')
        m = HMR(backbone='resnet101', use_cam=True, use_cam_feats=True)
        missing, unexpected = m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(k.startswith('smpl.') for k in missing)
    else:
        sd = synth.camcalib_state(1800 + depth, backbone='resnet%d' % depth)
        m = CameraRegressorNetwork(backbone='resnet%d' % depth)
        m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    m.set_precision('fp16')
    return m, sd


@pytest.mark.parametrize('depth,H,W', [(18, 224, 224), (34, 224, 224), (34, 224, 160), (101, 224, 224)])
def test_trunk_other_depths_vs_fp16_reference(depth, H, W):
    """BasicBlock trunks (the downsample is a conv of its own, stored as fp16 and used as the residual; the last conv is a 3x3 with
    a residual and an fp32 store) and the 101-layer Bottleneck trunk at fp16, against the float64 walk of the fp16 contract."""
    m, sd = _trunk_model(depth)
    x = synth.images(12, 3, H, W)
    f = m.engine(DEV).trunk(t(x).to(DEV)).cpu().double().numpy().transpose(0, 3, 1, 2)
    with cpu_threads():
        ref = fp16_ref.trunk(sd, x.astype(np.float64), depth=depth)
    assert f.shape == ref.shape
    err = float(np.abs(f - ref).max() / np.abs(ref).max())
    print('trunk resnet%d' % depth, 3, H, W, 'max |gpu - fp16_ref| / max |ref| =', err)
    assert err <= TRUNK_BAR, (depth, H, W, err)


def test_batch_invariance_resnet34():
    m, _ = _trunk_model(34)
    e = m.engine(DEV)
    x = t(synth.images(31, 9)).to(DEV)
    f9 = e.trunk(x).clone()
    f2 = e.trunk(x[:2].contiguous())
    assert torch.equal(f9[:2], f2)
