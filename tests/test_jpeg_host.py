"""The JPEG contract without a GPU: tests/jpeg_ref.py (the NumPy restatement every GPU test compares with) against Pillow's own
bytes - the committed fixture, and the installed Pillow where it is a libjpeg-turbo build; the header the library builds on the
host; the host-side check of the picture records.  Every comparison is == on bytes."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from spec_amd import _lib
from spec_amd.engine import check_jpeg_encode, jpeg_capacity
from tests import jpeg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_pillow.npz')


def test_reference_equals_the_fixture():
    g = np.load(GOLDEN)
    cases = [str(c).split() for c in g['cases']]
    assert len(cases) == 6 and {c[0] for c in cases} == set(jpeg_ref.CONTENTS)
    assert str(g['pillow_version']) and str(g['libjpeg_turbo_version'])
    for i, (content, H, W, q) in enumerate(cases):
        assert jpeg_ref.encode(jpeg_ref.picture(content, int(H), int(W)), int(q)) == g[f'case{i}'].tobytes(), (content, H, W, q)


def _pillow(a, **kw):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, format='JPEG', **kw)
    return f.getvalue()


def _need_turbo():
    from PIL import features
    if not features.check_feature('libjpeg_turbo'):
        pytest.skip('the contract is Pillow on libjpeg-turbo; this Pillow is built on another libjpeg, whose bytes may differ')


@pytest.mark.parametrize('size', jpeg_ref.SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('content', jpeg_ref.CONTENTS)
def test_reference_equals_the_installed_pillow(size, content):
    _need_turbo()
    a = jpeg_ref.picture(content, *size)
    for q in jpeg_ref.QUALITIES:
        assert jpeg_ref.encode(a, q) == _pillow(a, quality=q, optimize=False, progressive=False), q


def test_quality_75_is_a_plain_save_and_the_cases_bite():
    _need_turbo()
    a = jpeg_ref.picture('noise', 40, 56)
    assert jpeg_ref.encode(a, 75) == _pillow(a)
    assert jpeg_ref.encode(jpeg_ref.picture('noise', 65, 130), 100).count(b'\xff\x00') >= 100       # hundreds of stuffed FF bytes
    coef = jpeg_ref.coefficients(jpeg_ref.picture('checker', 24, 24), 100)
    assert np.abs(coef[..., 1:]).max() >= 512                                                        # the largest AC category
    coef = jpeg_ref.coefficients(jpeg_ref.picture('sparse', 65, 130), 95)[..., 1:]
    runs = [np.diff(np.concatenate([[-1], np.nonzero(b)[0]])).max() - 1 for b in coef.reshape(-1, 63) if b.any()]
    assert max(runs) > 15                                                                            # ZRL codes


def _header(q, H, W, capacity=623):
    buf = (C.c_uint8 * max(capacity, 1))()
    rc = _lib.load().specmi_jpeg_header(q, H, W, buf, capacity)
    return rc, bytes(buf)[:623]


@pytest.mark.parametrize('q', jpeg_ref.QUALITIES)
def test_library_header_equals_the_reference(q):
    for H, W in jpeg_ref.SIZES + ((32768, 32768),):
        assert _header(q, H, W) == (_lib.OK, jpeg_ref.header(q, H, W)), (H, W)
    assert len(jpeg_ref.header(q, 8, 8)) == _lib.JPEG_HEADER_BYTES == 623


def test_library_header_refusals():
    for q, H, W, cap in ((0, 8, 8, 623), (101, 8, 8, 623), (75, 0, 8, 623), (75, 8, 32769, 623), (75, 8, 8, 622)):
        assert _header(q, H, W, cap)[0] == _lib.ERR_ARG, (q, H, W, cap)
    assert _lib.load().specmi_jpeg_header(75, 8, 8, None, 623) == _lib.ERR_ARG


GOOD = dict(geom=[[16, 24], [9, 5]], offsets=[[0, 72, 0, 2000], [2000, 15, 2000, 700]], in_bytes=4000, out_bytes=2700, quality=75)
BAD = {
    'no picture': dict(geom=np.zeros((0, 2)), offsets=np.zeros((0, 4))),
    'too many pictures': dict(geom=np.tile([[1, 1]], (65536, 1)), offsets=np.tile([[0, 3, 0, 700]], (65536, 1))),
    'quality 0': dict(quality=0),
    'quality 101': dict(quality=101),
    'H 0': dict(geom=[[0, 24], [9, 5]]),
    'W 32769': dict(geom=[[16, 24], [9, 32769]]),
    'pitch below 3 W': dict(offsets=[[0, 71, 0, 2000], [2000, 15, 2000, 700]]),
    'rectangle leaves its slab': dict(in_bytes=2000 + 8 * 15 + 14),
    'negative offset': dict(offsets=[[-1, 72, 0, 2000], [2000, 15, 2000, 700]]),
    'capacity below the header': dict(offsets=[[0, 72, 0, 2000], [2000, 15, 2000, 622]]),
    'output leaves its slab': dict(out_bytes=2699),
    'outputs share a byte': dict(offsets=[[0, 72, 0, 2001], [2000, 15, 2000, 700]]),
    'overlapping slabs': dict(in_ptr=4096, out_ptr=4096 + 3999),
    'null slab': dict(in_ptr=0, out_ptr=8192),
    'missing slab': dict(out_bytes=None),
    'shapes': dict(offsets=[[0, 72], [2000, 15]]),
}


def test_check_accepts_a_good_record():
    geom, offsets = check_jpeg_encode(**GOOD, in_ptr=4096, out_ptr=4096 + 4000)
    assert geom.dtype == np.int32 and offsets.dtype == np.int64 and geom.shape == (2, 2) and offsets.shape == (2, 4)
    assert jpeg_capacity(1080, 5760) == 3 * 1080 * 5760 + 1024


@pytest.mark.parametrize('name', sorted(BAD))
def test_check_refuses(name):
    with pytest.raises(ValueError):
        check_jpeg_encode(**{**GOOD, **BAD[name]})
