"""The PNG contract without a GPU: tests/png_ref.py (the restatement every GPU test compares with) decodes back exactly through
Pillow and zlib; its header against Pillow's and the library's; the bound; the pictures of png_ref.EDGES provably reach every edge of
the rules (asserted on the reference's own report); the host-side check of the picture records."""
import ctypes as C
import functools
import io
import struct
import zlib

import numpy as np
import pytest

from spec_amd import _lib
from spec_amd.engine import check_png_encode, is_png_name, png_bound
from tests import jpeg_ref, png_ref

CONTENTS = jpeg_ref.CONTENTS + ('constant', 'all255')           # 'noise' is jpeg_ref's
SIZES = jpeg_ref.SIZES + ((300, 1), (3, 5000))


def _picture(content, H, W):
    if content == 'constant':
        return np.full((H, W, 3), (12, 200, 77), np.uint8)
    if content == 'all255':
        return np.full((H, W, 3), 255, np.uint8)
    return jpeg_ref.picture(content, H, W)


def _idat(f):
    """The chunks of a file -> IDAT's data; every CRC and the layout of rule 1 checked on the way."""
    assert f[:8] == png_ref.SIGNATURE
    at, kinds, data = 8, [], None
    while at < len(f):
        n, kind = struct.unpack('>I', f[at:at + 4])[0], f[at + 4:at + 8]
        assert struct.unpack('>I', f[at + 8 + n:at + 12 + n])[0] == zlib.crc32(f[at + 4:at + 8 + n])
        kinds.append(kind)
        if kind == b'IDAT':
            data = f[at + 8:at + 8 + n]
        at += 12 + n
    assert kinds == [b'IHDR', b'IDAT', b'IEND'] and at == len(f) and data[:2] == b'\x78\x01'
    return data


def _pillow(a):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, format='PNG')
    return f.getvalue()


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_reference_decodes_back_exactly(size):
    from PIL import Image
    for content in CONTENTS:
        a = _picture(content, *size)
        rep = {}
        f = png_ref.encode(a, rep)
        Image.open(io.BytesIO(f)).verify()
        assert np.array_equal(np.array(Image.open(io.BytesIO(f)).convert('RGB')), a), content
        stream = png_ref.filter_rows(a)[0].tobytes()
        assert zlib.decompress(_idat(f)) == stream, content
        assert f[:33] == _pillow(a)[:33] == png_ref.header(*size)
        assert len(f) <= png_ref.bound(*size) == png_bound(*size)
        if content == 'noise' and size[1] > 1:      # rows of one pixel: every fourth byte is a filter type, and that much codes
            assert len(f) == png_ref.bound(*size) and all(s['stored'] for s in rep['segments'])      # the bound is reached


def test_a_constant_picture_is_under_two_percent_of_raw():
    a = png_ref.EDGES['constant']()
    assert a.shape == (64, 1365, 3) and len(png_ref.encode(a)) < 0.02 * a.size


def _header(H, W, capacity=33):
    buf = (C.c_uint8 * max(capacity, 1))()
    rc = _lib.load().specmi_png_header(H, W, buf, capacity)
    return rc, bytes(buf)[:33]


def test_library_header_and_bound():
    lib = _lib.load()
    for H, W in SIZES + ((32768, 32768), (1080, 5760)):
        assert _header(H, W) == (_lib.OK, png_ref.header(H, W)), (H, W)
        assert png_bound(H, W) == png_ref.bound(H, W)
    assert _lib.PNG_HEADER_BYTES == 33 and _lib.PNG_OVERHEAD_BYTES == png_ref.OVERHEAD_BYTES == len(png_ref.encode(np.zeros((1, 1, 3), np.uint8))) - 9
    for H, W, cap in ((0, 8, 33), (8, 32769, 33), (8, 8, 32)):
        assert _header(H, W, cap)[0] == _lib.ERR_ARG, (H, W, cap)
    assert lib.specmi_png_header(8, 8, None, 33) == _lib.ERR_ARG
    out = np.zeros(1, np.int64)
    assert lib.specmi_png_bound(8, 8, None) == _lib.ERR_ARG and lib.specmi_png_bound(0, 8, out.ctypes.data_as(_lib.c_int64_p)) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        png_bound(8, 32769)
    assert is_png_name('a/b.PNG') and not is_png_name('a/b.jpg')


# ---- the edges ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge(name):
    a, rep = png_ref.EDGES[name](), {}
    f = png_ref.encode(a, rep)
    assert zlib.decompress(_idat(f)) == png_ref.filter_rows(a)[0].tobytes()
    return a, rep


def _tokens(rep):
    return [tk for s in rep['segments'] for tk in s['tokens']]


def test_every_filter_type_is_chosen_and_a_tie_goes_to_the_lowest():
    _, rep = _edge('filters')
    assert set(rep['filters'].tolist()) == {0, 1, 2, 3, 4}
    _, rep = _edge('tie')
    assert (rep['sums'] == 0).all() and (rep['filters'] == 0).all()
    a, rep = _edge('constant')          # rows below the first: Up and Paeth both cost 0, and the lower type wins
    assert (rep['sums'][1:, 2] == rep['sums'][1:, 4]).all() and (rep['filters'][1:] == 2).all()


def test_matches_of_every_length_at_both_distances_and_the_runs():
    a, rep = _edge('matches')
    assert rep['filters'].tolist() == [1]                        # the stream is what matches_row wrote
    toks = _tokens(rep)
    for d in (1, 3):
        assert {n for n, dist in toks if dist == d} >= set(range(3, 259)), d
    stream = png_ref.filter_rows(a)[0].reshape(-1)
    change = np.flatnonzero(np.diff(stream.astype(int)) != 0)
    repeats = set((np.diff(change) - 1).tolist())                # how often a byte repeats the one before it, per run
    assert repeats >= {0, 1, 2, 259, 260, 261}
    # what the greedy parse makes of the long runs: 258 and a literal; 258 and two literals; 258 and a match of 3
    seq = ''.join('M' if n == 258 and d == 1 else 'm' if n == 3 and d == 1 else 'l' if d == 0 else '.' for n, d in toks)
    assert 'lMll' in seq and 'lMlll' in seq and 'lMml' in seq
    assert len(rep['segments']) == 3 and not any(s['stored'] or s['halved'] for s in rep['segments'])


def test_runs_cut_by_segment_ends_and_the_distance_codes():
    a, rep = _edge('cut')
    stream = png_ref.filter_rows(a)[0].reshape(-1)
    S = png_ref.SEGMENT
    assert len(rep['segments']) == 2 and stream[S - 2] == stream[S - 1] == stream[S] == stream[S + 1]
    first, second = rep['segments'][0]['tokens'], rep['segments'][1]['tokens']
    assert first[-1][1] == 1 and second[0] == (1, 0) and second[1] == (258, 1)          # the run ends with the segment and starts again with a literal
    _, rep = _edge('constant')
    assert len(rep['segments']) == 8 and all(s['distances'][0] > 0 and s['distances'][1] == 0 for s in rep['segments'])      # a single distance code
    _, rep = _edge('noise')
    assert [s['distances'] for s in rep['segments']] == [(0, 0), (0, 0)]                # no match: no distance code
    assert [s['stored'] for s in rep['segments']] == [True, True] and [s['bytes'] for s in rep['segments']] == [S, 12 * 4096 - S]
    _, rep = _edge('matches')
    assert any(s['distances'][0] and s['distances'][1] for s in rep['segments'])        # both


def test_the_length_limit_path_is_taken():
    a, rep = _edge('deep')
    assert rep['filters'].tolist() == [1]
    seg, = rep['segments']
    assert seg['halved'] >= 1 and not seg['stored'] and seg['distances'] == (0, 0) and all(tk == (1, 0) for tk in seg['tokens'])
    stream = png_ref.filter_rows(a)[0].reshape(-1)
    counts = np.bincount(stream, minlength=286)
    counts[256] = 1
    assert max(png_ref.huffman_lengths(counts)[0]) <= 15
    # without the rule the tree is deeper than deflate allows
    raw = sorted(c for c in counts if c)
    assert all(raw[i] + raw[i + 1] <= raw[i + 2] + 1 for i in range(len(raw) - 2)) and len(raw) >= 18


def test_the_adler_modulo_is_crossed():
    for name in ('all255', 'noise'):
        a, _ = _edge(name)
        stream = png_ref.filter_rows(a)[0].reshape(-1).astype(np.int64)
        s1 = 1 + np.cumsum(stream)
        assert s1.sum() > 65521 * 1000, name                       # the second sum, many times over
    assert s1[-1] > 65521 * 10                                      # and on noise the first


# ---- the host-side check ----------------------------------------------------------------------------------------------------------
GOOD = dict(geom=[[16, 24], [9, 5]], offsets=[[0, 72, 0, 2000], [2000, 15, 2000, 700]], in_bytes=4000, out_bytes=2700)
BAD = {
    'no picture': dict(geom=np.zeros((0, 2)), offsets=np.zeros((0, 4))),
    'too many pictures': dict(geom=np.tile([[1, 1]], (65536, 1)), offsets=np.tile([[0, 3, 0, 700]], (65536, 1))),
    'H 0': dict(geom=[[0, 24], [9, 5]]),
    'W 32769': dict(geom=[[16, 24], [9, 32769]]),
    'pitch below 3 W': dict(offsets=[[0, 71, 0, 2000], [2000, 15, 2000, 700]]),
    'rectangle leaves its slab': dict(in_bytes=2000 + 8 * 15 + 14),
    'negative offset': dict(offsets=[[-1, 72, 0, 2000], [2000, 15, 2000, 700]]),
    'capacity below the overhead': dict(offsets=[[0, 72, 0, 2000], [2000, 15, 2000, 62]]),
    'output leaves its slab': dict(out_bytes=2699),
    'outputs share a byte': dict(offsets=[[0, 72, 0, 2001], [2000, 15, 2000, 700]]),
    'overlapping slabs': dict(in_ptr=4096, out_ptr=4096 + 3999),
    'null slab': dict(in_ptr=0, out_ptr=8192),
    'missing slab': dict(out_bytes=None),
    'shapes': dict(offsets=[[0, 72], [2000, 15]]),
    'IDAT beyond 2^31': dict(geom=[[32768, 32768]], offsets=[[0, 98304, 0, 4000]], in_bytes=32768 * 98304, out_bytes=4000),
}


def test_check_refuses_by_name_what_only_a_faked_slab_reaches():
    with pytest.raises(ValueError, match='one IDAT chunk'):
        check_png_encode(**{**GOOD, **BAD['IDAT beyond 2^31']})
    many = dict(in_bytes=3 * 26750 * 26750, out_bytes=129 * 63)
    with pytest.raises(ValueError, match='2\\^23 segments'):         # 129 x 65513 segments
        check_png_encode([[26750, 26750]] * 129, [[0, 80250, 63 * i, 63] for i in range(129)], **many)
    check_png_encode([[26750, 26750]] * 128, [[0, 80250, 63 * i, 63] for i in range(128)], **many)


def test_check_accepts_a_good_record():
    geom, offsets = check_png_encode(**GOOD, in_ptr=4096, out_ptr=4096 + 4000)
    assert geom.dtype == np.int32 and offsets.dtype == np.int64 and geom.shape == (2, 2) and offsets.shape == (2, 4)
    check_png_encode(**{**GOOD, 'offsets': [[0, 72, 0, 2000], [2000, 15, 2000, 63]]})          # the overhead itself is a capacity
    # a square whose stream still fits one IDAT; 26760 x 26760 does not
    check_png_encode([[26750, 26750]], [[0, 3 * 26750, 0, 63]], 3 * 26750 * 26750, 63)
    with pytest.raises(ValueError):
        check_png_encode([[26760, 26760]], [[0, 3 * 26760, 0, 63]], 3 * 26760 * 26760, 63)


@pytest.mark.parametrize('name', sorted(BAD))
def test_check_refuses(name):
    with pytest.raises(ValueError):
        check_png_encode(**{**GOOD, **BAD[name]})
