"""The JPEG decode contract without a GPU: tests/jpeg_dec_ref.py (the NumPy restatement every GPU test compares with, the parallel
subsequence scheme included) against Pillow's own pixels - the committed fixture, and the installed Pillow where it is a
libjpeg-turbo build; the marker probe the library runs on the host; the host-side check of the file records."""
import io

import os

import numpy as np
import pytest

from spec_amd import _lib
from spec_amd.engine import check_jpeg_decode, jpeg_probe
from tests import jpeg_dec_ref as ref
from tests import jpeg_ref
from tests.test_jpeg_host import _need_turbo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_decode.npz')


def test_reference_equals_the_fixture():
    g = np.load(GOLDEN)
    assert len(g['cases']) == 7 and str(g['pillow_version']) and str(g['libjpeg_turbo_version'])
    for i in range(len(g['cases'])):
        px, _, _, status = ref.decode(g[f'file{i}'].tobytes())
        assert status == 0 and np.array_equal(px, g[f'pixels{i}']), str(g['cases'][i])


@pytest.mark.parametrize('size', ref.SIZES, ids=lambda s: '%dx%d' % s)
def test_reference_equals_the_installed_pillow(size):
    _need_turbo()
    for c in jpeg_ref.CONTENTS:
        a = jpeg_ref.picture(c, *size)
        for q in ref.QUALITIES:
            data = jpeg_ref.encode(a, q)
            px, _, _, status = ref.decode(data)
            assert status == 0 and np.array_equal(px, ref.pillow_pixels(data)), (c, q)


def test_variants_equal_the_installed_pillow():
    _need_turbo()
    files = ref.variant_set()
    assert {ref.probe(d)['s420'] for _, d in files} == {True, False}
    assert any(not np.array_equal(ref.probe(d)['q'][0], jpeg_ref.quant_tables(q)[0]) for _, d in files for q in (50, 75, 90))
    for name, data in files:
        px, _, _, status = ref.decode(data)
        assert status == 0 and np.array_equal(px, ref.pillow_pixels(data)), name
        assert jpeg_probe(data)[0] == 'supported', name


def test_the_group_scheme_gives_the_same_coefficients():
    data = jpeg_ref.encode(jpeg_ref.picture('noise', 65, 130), 95)
    info = ref.probe(data)
    a, b = ref.entropy_decode(data, info, group=1), ref.entropy_decode(data, info, group=4)
    assert a[2] == b[2] == 0 and np.array_equal(a[0], b[0]) and b[1] <= -(-a[3] // 4) and a[1] <= a[3]
    coef = jpeg_ref.coefficients(jpeg_ref.picture('noise', 65, 130), 95)          # zigzag order, what the encoder coded
    nat = np.zeros_like(coef)
    nat[..., jpeg_ref.ZIGZAG] = coef
    assert np.array_equal(a[0], nat.reshape(-1, 64))


def test_the_periodic_scan_needs_every_pass():
    """The constant picture's scan is periodic (32 bits per MCU): a wrong phase never corrects itself, so the truth advances one
    subsequence per pass - the worst case is in the set."""
    data = jpeg_ref.encode(jpeg_ref.picture('zeros', 192, 256), 75)
    coef, passes, status, nsub, _ = ref.entropy_decode(data, ref.probe(data))
    assert status == 0 and passes == nsub == 7
    assert np.array_equal(ref.pixels(coef, ref.probe(data)), np.zeros((192, 256, 3), np.uint8))


def test_a_boundary_falls_between_a_ff_and_its_stuffed_zero():
    """Computed from the bytes: subsequence boundaries are multiples of 128 file bytes from the scan's start."""
    hits = []
    for name, data in ref.file_set():
        if not name.startswith('noise'):
            continue
        s0, s1 = ref.probe(data)['scan']
        scan = data[s0:s1]
        n = sum(1 for k in range(128, len(scan), 128) if scan[k - 1] == 0xFF and scan[k] == 0)
        assert n == ref.entropy_decode(data, ref.probe(data))[4]
        if n:
            hits.append(name)
    assert 'noise 65x130 q95' in hits, hits


def _kinds():
    from PIL import Image
    a = jpeg_ref.picture('noise', 33, 47)
    png = io.BytesIO()
    Image.fromarray(a).save(png, format='PNG')
    cmyk = io.BytesIO()
    Image.fromarray(a).convert('CMYK').save(cmyk, format='JPEG')
    base = ref.pillow_save(a)
    kinds = {'progressive': ('progressive', ref.pillow_save(a, progressive=True)),
             'L': ('components', ref.pillow_save(a[..., 0])),
             'CMYK': ('components', cmyk.getvalue()),
             'subsampling=1': ('sampling', ref.pillow_save(a, subsampling=1)),
             'PNG': ('not_jpeg', png.getvalue()),
             'truncated header': ('truncated', base[:300]),
             'no EOI': ('truncated', base[:-2]),
             'bytes behind the EOI': ('trailing', base + b'\x00\x00'),
             'empty': ('not_jpeg', b'')}
    try:
        kinds['restart interval'] = ('restart', ref.pillow_save(a, restart_marker_blocks=2))
        assert b'\xff\xdd' in kinds['restart interval'][1]
    except (TypeError, AssertionError):            # this Pillow cannot write one: the marker is put in by hand
        kinds['restart interval'] = ('restart', base[:2] + b'\xff\xdd\x00\x04\x00\x02' + base[2:])
    return base, kinds


def test_the_probe_refuses_each_unsupported_kind_by_name():
    base, kinds = _kinds()
    assert jpeg_probe(base) == ('supported', 33, 47, 420)
    assert jpeg_probe(ref.pillow_save(jpeg_ref.picture('noise', 33, 47), subsampling=0)) == ('supported', 33, 47, 444)
    for kind, (reason, data) in kinds.items():
        assert jpeg_probe(data) == (reason, 0, 0, 0), kind
        with pytest.raises(ref.Unsupported) as e:
            ref.probe(data)
        assert e.value.reason == reason, kind
    assert ref.REASONS == _lib.JPEG_REASONS
    adobe = base[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01' + base[2:]
    assert jpeg_probe(adobe)[0] == 'colourspace'
    for _, data in ref.file_set()[::37]:
        info = ref.probe(data)
        assert jpeg_probe(data) == ('supported', info['H'], info['W'], 420)


GOOD = dict(ranges=[[0, 700], [700, 900]], geom=[[16, 24, 420], [9, 5, 444]], outs=[[0, 72], [2000, 15]], in_bytes=1600, out_bytes=2135)
BAD = {
    'no file': dict(ranges=np.zeros((0, 2)), geom=np.zeros((0, 3)), outs=np.zeros((0, 2))),
    'too many files': dict(ranges=np.tile([[0, 1]], (65536, 1)), geom=np.tile([[1, 1, 420]], (65536, 1)), outs=np.tile([[0, 3]], (65536, 1))),
    'file leaves its slab': dict(in_bytes=1599),
    'negative file offset': dict(ranges=[[-1, 700], [700, 900]]),
    'negative length': dict(ranges=[[0, -1], [700, 900]]),
    'H 0': dict(geom=[[0, 24, 420], [9, 5, 444]]),
    'W 32769': dict(geom=[[16, 24, 420], [9, 32769, 444]]),
    'a file the probe refuses': dict(geom=[[16, 24, 0], [9, 5, 444]]),
    'pitch below 3 W': dict(outs=[[0, 71], [2000, 15]]),
    'rectangle leaves its slab': dict(out_bytes=2134),
    'negative offset': dict(outs=[[-1, 72], [2000, 15]]),
    'rectangles share a byte': dict(outs=[[0, 72], [71, 15]]),
    'overlapping slabs': dict(in_ptr=4096, out_ptr=4096 + 1599),
    'null slab': dict(in_ptr=0, out_ptr=8192),
    'missing slab': dict(out_bytes=None),
    'shapes': dict(geom=[[16, 24], [9, 5]]),
    # five pictures of 32768 x 32768 at 4:2:0 are 5 x 2^22 MCUs; four are exactly 2^24 and pass (below)
    'more than 2^24 MCUs': dict(ranges=[[0, 700]] * 5, geom=[[32768, 32768, 420]] * 5, outs=[[k * 3 * 2 ** 30, 3 * 32768] for k in range(5)],
                                out_bytes=15 * 2 ** 30),
    'more than 2^24 MCUs at 4:4:4': dict(ranges=[[0, 700]] * 2, geom=[[32768, 32768, 444], [8, 8, 444]], outs=[[0, 3 * 32768], [3 * 2 ** 30, 24]],
                                         out_bytes=4 * 2 ** 30),
}


def test_check_accepts_a_good_record_and_interleaved_rectangles():
    ranges, outs = check_jpeg_decode(**GOOD, in_ptr=4096, out_ptr=4096 + 1600)
    assert ranges.dtype == outs.dtype == np.int64 and ranges.shape == outs.shape == (2, 2)
    check_jpeg_decode(**{**GOOD, 'outs': [[0, 100], [72, 100]], 'out_bytes': 4000})        # side by side in one picture: no byte shared
    check_jpeg_decode(ranges=[[0, 700]], geom=[[32768, 32768, 444]], outs=[[0, 3 * 32768]], in_bytes=1600, out_bytes=3 * 2 ** 30)   # exactly 2^24 MCUs


@pytest.mark.parametrize('name', sorted(BAD))
def test_check_refuses(name):
    with pytest.raises(ValueError):
        check_jpeg_decode(**{**GOOD, **BAD[name]})


def large_coefficient_file():
    """A 16 x 16 file at quality 1 (every quantiser 255) whose coefficients are all +-128: |coefficient x quantiser| = 32640 passes
    rule 2, and the sums of the IDCT leave 32 bits - the reference and libjpeg's JLONG hold them in 64."""
    rng = np.random.default_rng(9)
    coef = (128 * rng.choice([-1, 1], (1, 1, 6, 64))).astype(np.int64)
    return jpeg_ref.header(1, 16, 16) + jpeg_ref.scan(coef) + b'\xff\xd9'


def test_the_idct_holds_sums_beyond_32_bits():
    data = large_coefficient_file()
    info = ref.probe(data)
    assert (info['q'] == 255).all()
    coef, _, status, _, _ = ref.entropy_decode(data, info)
    assert status == 0 and (np.abs(coef) == 128).all()
    d = coef[:1] * info['q'][0]
    odd = np.abs(d.reshape(8, 8)[1::2]).sum(axis=0).max()
    assert odd * 25172 > 2 ** 31                                   # one product of the odd part alone
    px = ref.pixels(coef, info)
    assert px.shape == (16, 16, 3) and len(np.unique(px)) > 2
