"""tests/color_jitter_ref.py - the ColorJitter contract in NumPy - against the installed Pillow, every assertion an exact
equality: blend on the whole 256 x 256 table, L, both colour conversions on all 2^24 inputs, the mean's tie, the full chain in
all 24 orders, skipped operations; and what ``spec_amd.augment.ColorJitter`` draws.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from spec_amd import _lib, augment
from tests import color_jitter_ref as R

FACTORS = (1.13, 0.87, 1.19)
K = augment.hue_shift(-0.07)


def _all_triples():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.fixture(scope='module')
def triples():
    return _all_triples()


def pil_hue(img, k):
    """torchvision's adjust_hue on a PIL image, with the shift already an integer"""
    h, s, v = img.convert('HSV').split()
    h = Image.fromarray(((np.asarray(h).astype(np.int32) + k) % 256).astype(np.uint8), 'L')
    return Image.merge('HSV', (h, s, v)).convert('RGB')


def pil_jitter(rgb, order, factors, k):
    img = Image.fromarray(rgb)
    for op in order:
        if op == R.BRIGHTNESS:
            img = ImageEnhance.Brightness(img).enhance(factors[0])
        elif op == R.CONTRAST:
            img = ImageEnhance.Contrast(img).enhance(factors[1])
        elif op == R.SATURATION:
            img = ImageEnhance.Color(img).enhance(factors[2])
        elif op == R.HUE:
            img = pil_hue(img, k)
    return np.asarray(img)


# 0, 1, both ends of [0.8, 1.2], two interior values, and 1.9: above 1 and saturating
@pytest.mark.parametrize('a', [0.0, 1.0, 0.8, 1.2, 0.8371, 1.13, 1.1999, 1.9])
def test_blend_table(a):
    d, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    want = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(v), a))
    assert np.array_equal(R.blend(d, v, a), want)
    if a == 1.9:
        assert (want == 255).any() and (want == 0).any()


def test_luma(triples):
    assert np.array_equal(R.luma(triples), np.asarray(Image.fromarray(triples).convert('L')))


def test_rgb_to_hsv_all_colours(triples):
    assert np.array_equal(R.rgb_to_hsv(triples), np.asarray(Image.fromarray(triples).convert('HSV')))


def test_hsv_to_rgb_all_triples(triples):
    want = np.asarray(Image.frombytes('HSV', (4096, 4096), triples.tobytes()).convert('RGB'))
    assert np.array_equal(R.hsv_to_rgb(triples), want)


def test_mean_tie():
    # L = 10 and 11: the mean 10.5 goes up to 11
    rgb = np.asarray([[[10, 10, 10], [11, 11, 11]]], np.uint8)
    assert R.luma(rgb).tolist() == [[10, 11]] and R.contrast_mean(rgb) == 11
    for f in (0.0, 0.8, 1.2):
        assert np.array_equal(R.apply_op(rgb, R.CONTRAST, (1.0, f, 1.0), 0), np.asarray(ImageEnhance.Contrast(Image.fromarray(rgb)).enhance(f)))
    assert np.asarray(ImageEnhance.Contrast(Image.fromarray(rgb)).enhance(0.0)).tolist() == [[[11] * 3] * 2]


def test_full_chain_all_24_orders():
    rgb = np.random.default_rng(7).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    seen = set()
    for order in itertools.permutations(range(4)):
        got = R.jitter(rgb, order, FACTORS, K)
        assert np.array_equal(got, pil_jitter(rgb, order, FACTORS, K)), order
        seen.add(got.tobytes())
    assert len(seen) == 24                  # the order is part of the contract


def test_skipped_operations():
    rgb = np.random.default_rng(8).integers(0, 256, (9, 13, 3), dtype=np.uint8)
    for order in ((), (3,), (1,), (2, 0), (3, 1, 0), (0, 2, 3)):
        rec = R.make_record(order, FACTORS, K)
        assert rec[:4].tolist() == list(order) + [-1] * (4 - len(order))
        assert np.array_equal(R.jitter_record(rgb, rec), pil_jitter(rgb, order, FACTORS, K))
    assert np.array_equal(R.jitter_record(rgb, R.make_record((), FACTORS, K)), rgb)


@pytest.mark.parametrize('hue, k', [(0.1, 25), (-0.1, 231), (0.5, 127), (-0.5, 129), (0.0, 0)])
def test_hue_shift(hue, k):
    assert augment.hue_shift(hue) == k == R.hue_k(hue)


def test_get_params_ranges_and_generator_order():
    cj = augment.ColorJitter(**augment.CAMCALIB_TRAIN_JITTER)
    assert cj.brightness == cj.contrast == cj.saturation == (0.8, 1.2) and cj.hue == (-0.1, 0.1)
    g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for _ in range(50):
        order, b, c, s, h = cj.get_params(g)
        # the stated consumption: randperm(4), then four uniform_ draws of one element each
        want_order = torch.randperm(4, generator=g2).tolist()
        want = [float(torch.empty(1).uniform_(lo, hi, generator=g2)) for lo, hi in ((0.8, 1.2),) * 3 + ((-0.1, 0.1),)]
        assert order == want_order and [b, c, s, h] == want
        assert sorted(order) == [0, 1, 2, 3]
        assert all(0.8 <= v <= 1.2 for v in (b, c, s)) and -0.1 <= h <= 0.1
    assert g.get_state().equal(g2.get_state())


def test_switched_off_operations_draw_nothing():
    cj = augment.ColorJitter(brightness=0.2, contrast=None, saturation=0, hue=0.1)
    g, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    order, b, c, s, h = cj.get_params(g)
    assert c is None and s is None
    assert order == torch.randperm(4, generator=g2).tolist()
    assert b == float(torch.empty(1).uniform_(0.8, 1.2, generator=g2)) and h == float(torch.empty(1).uniform_(-0.1, 0.1, generator=g2))
    rec = cj.record((order, b, c, s, h))
    assert rec[:4].tolist() == [op for op in order if op in (0, 3)] + [-1, -1]
    assert rec[4:7].view(np.float32).tolist() == [np.float32(b), 1.0, 1.0] and rec[7] == augment.hue_shift(h)
    with pytest.raises(ValueError):
        augment.ColorJitter(hue=0.6)
    with pytest.raises(ValueError):
        augment.ColorJitter(brightness=-0.1)


def test_records_are_the_draws_in_frame_order():
    cj = augment.ColorJitter(**augment.CAMCALIB_TRAIN_JITTER)
    recs = cj.records(6, torch.Generator().manual_seed(3))
    g = torch.Generator().manual_seed(3)
    assert recs.dtype == np.int32 and recs.shape == (6, 8)
    for r in recs:
        order, b, c, s, h = cj.get_params(g)
        assert np.array_equal(r, R.make_record(order, (b, c, s), augment.hue_shift(h)))


def test_prototype():
    res, args = _lib.PROTOTYPES['specmi_color_jitter']
    assert res is C.c_int and len(args) == 10
    assert args[1] is C.c_void_p and args[2] is C.c_size_t and args[3] is C.c_void_p and args[4] is C.c_size_t
    assert args[5] is _lib.c_int32_p and args[6] is _lib.c_int64_p and args[7] is _lib.c_int32_p and args[8] is C.c_int
    assert (_lib.JITTER_BRIGHTNESS, _lib.JITTER_CONTRAST, _lib.JITTER_SATURATION, _lib.JITTER_HUE, _lib.JITTER_REC) == (0, 1, 2, 3, 8)


def test_check_color_jitter_refusals():
    from spec_amd.engine import check_color_jitter
    rec = R.make_record((0, 1, 2, 3), FACTORS, K)[None]
    ok = lambda **kw: check_color_jitter(kw.get('geom', [(4, 5)]), kw.get('offsets', [(0, 15, 0, 15)]), kw.get('records', rec), kw.get('nin', 60),
                                         kw.get('nout', 60), kw.get('in_place', False))
    ok()

    def bad(word, value):
        r = rec.copy()
        r[0, word] = value
        return r
    nan = int(np.asarray([np.nan], np.float32).view(np.int32)[0])
    neg = int(np.asarray([-0.5], np.float32).view(np.int32)[0])
    for kw in (dict(geom=[(0, 5)]), dict(geom=[(4, 8193)]), dict(offsets=[(0, 14, 0, 15)]), dict(offsets=[(0, 15, 0, 14)]), dict(nin=59), dict(nout=59),
               dict(offsets=[(-1, 15, 0, 15)]), dict(offsets=[(0, 15, 3, 15)], nout=63, in_place=True), dict(records=bad(0, 4)), dict(records=bad(0, -2)),
               dict(records=bad(1, 0)), dict(records=bad(5, nan)), dict(records=bad(6, neg)), dict(records=bad(7, 256)), dict(records=bad(7, -1)),
               dict(records=rec.astype(np.int64)), dict(geom=[(4, 5), (4, 5)], offsets=[(0, 15, 0, 15), (0, 15, 14, 15)], records=np.repeat(rec, 2, 0), nout=90)):
        with pytest.raises(ValueError):
            ok(**kw)
