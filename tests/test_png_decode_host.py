"""The PNG decoder's contract on the host: tests/png_dec_ref.py - the restatement of spec_amd/csrc/png_dec.hip with its windows and
settle rounds - equals Pillow on Pillow-saved, hand-assembled, token-by-token and tests/png_ref.encode files, reaches every path the
device scheme has (from its own counters), gives a non-zero status with every index in range on damaged streams; the host probe
(specmi_png_probe) names every reason and agrees with the restatement; ``check_png_decode`` makes every refusal.  No device."""
import functools
import io
import struct
import zlib

import numpy as np
import pytest

from spec_amd import _lib, engine, preprocess
from tests import png_dec_ref as ref


@functools.lru_cache(maxsize=None)
def _decoded(which):
    """{name: (file, pixels, status, counters)} of a file set, decoded once by the reference."""
    files = {'pillow': ref.pillow_set, 'hand': ref.hand_set, 'crafted': ref.crafted_set, 'big': lambda: [ref.big_file()],
             'encoder': lambda: [(n, f) for n, f, _ in ref.encoder_set()]}[which]()
    out = {}
    for name, f in files:
        c = ref.new_counters()
        px, st, _ = ref.decode(f, c)
        out[name] = (f, px, st, c)
    return out


def _total(which, key):
    return sum(c.get(key, 0) for _, _, _, c in _decoded(which).values())


@pytest.mark.parametrize('which', ['pillow', 'hand', 'crafted', 'big', 'encoder'])
def test_reference_equals_pillow(which):
    for name, (f, px, st, _) in _decoded(which).items():
        assert st == 0, (name, st)
        assert np.array_equal(px, ref.pillow_pixels(f)), name


def test_the_host_probe_is_the_references():
    for which in ('pillow', 'hand', 'crafted', 'big', 'encoder'):
        for name, (f, _, _, _) in _decoded(which).items():
            want = ref.probe(f)
            got = engine.png_probe(f)
            assert got[0] == 'supported' == want['reason'], name
            assert got[1:4] == (want['H'], want['W'], want['ctype']), name
            assert got[4].tolist() == [list(r) for r in want['ranges']], name
    _, big = ref.big_file()
    lengths = engine.png_probe(big)[4][:, 1].tolist()
    assert lengths[:6] == [1, 0, 65536, 1, 0, 65536] and len(lengths) == 7


def test_the_encoder_and_the_decoder_meet():
    for name, f, a in ref.encoder_set():
        assert np.array_equal(_decoded('encoder')[name][1], a), name


def test_every_filter_on_every_row():
    d = _decoded('hand')
    for ft in range(5):
        for H, W in ref.SIZES:
            for ct in ref.MODES:
                f = d[f'filter{ft}-{H}x{W}-ct{ct}'][0]
                raw = zlib.decompress(ref.stream_of(f, ref.probe(f)['ranges']))
                assert set(raw[::1 + W * ref.BPP[ct]]) == {ft}


def test_what_reaches_which_path():
    """Pictures that do not reach a path are not a test of it."""
    for key in ('stored', 'fixed', 'dynamic'):
        assert _total('pillow', key) > 0 and _total('hand', key) > 0, key
    assert max(c['windows_max'] for _, _, _, c in _decoded('hand').values()) >= 2, 'a block spanning two windows (120 x 121 noise, Z_HUFFMAN_ONLY)'
    big = _decoded('big')['noisy-300x300'][3]
    assert big['windows_max'] >= 2 and big['dynamic'] >= 2
    assert big['lane_decodes_max'] >= 3, 'a lane that needed more than one settle round'
    assert big['header_mid_subsequence'] >= 1
    crafted = _decoded('crafted')
    assert crafted['eob-last-lane'][3]['eob_last_lane'] == 1
    assert crafted['distance-32768'][3]['dist32768'] == 1 and crafted['distance-32768'][3]['stored'] == 1
    assert crafted['runs-258'][3]['len258_dist1'] == 4 and crafted['runs-258'][3].get('crosses_row', 0) >= 4
    assert crafted['runs-258'][3]['stored'] == 1 and crafted['runs-258'][3]['fixed'] == 3
    assert _total('hand', 'len258_dist1') > 0 and _total('hand', 'crosses_row') > 0
    assert _total('pillow', 'strip_boundary') > 0 and _total('hand', 'strip_boundary') > 0, 'a strip boundary at row 64'
    assert _total('pillow', 'batches_of_one') > 0 and _total('pillow', 'batches_of_many') > 0
    flush = _decoded('hand')['flush-65x3'][3]
    assert flush['stored'] >= 1 and flush['dynamic'] + flush['fixed'] >= 2, 'Z_FULL_FLUSH: an empty stored block between two coded ones'
    assert engine.png_probe(_decoded('hand')['wbits9-65x3'][0])[0] == 'supported'
    f = _decoded('hand')['wbits9-65x3'][0]
    assert ref.stream_of(f, ref.probe(f)['ranges'])[0] >> 4 == 1, 'CINFO 1: a window of 512 bytes'


def _reason_files():
    a = ref.picture(9, 11, 2, 'smooth')
    good = ref.hand_file(a, 2)
    s = ref.hand_file(a, 2, stream_only=True)
    from PIL import Image
    b16, pal = io.BytesIO(), io.BytesIO()
    Image.fromarray(np.arange(99, dtype=np.uint16).reshape(9, 11) * 600).save(b16, 'PNG')
    Image.fromarray(a).convert('P').save(pal, 'PNG')
    body = lambda lace=0, W=11: ref.SIGNATURE + ref.chunk(b'IHDR', struct.pack('>IIBBBBB', W, 9, 8, 2, 0, 0, lace)) + ref.chunk(b'IDAT', s) + ref.chunk(b'IEND', b'')
    crc = bytearray(good)
    crc[45] ^= 1
    return {'not_png': b'\x89PNX' + good[4:], 'truncated': good[:-5], 'crc': bytes(crc), 'depth': b16.getvalue(), 'palette': pal.getvalue(),
            'interlaced': body(lace=1), 'animated': ref.assemble(9, 11, 2, s, before=[ref.chunk(b'acTL', struct.pack('>II', 1, 0))]),
            'chunk': ref.assemble(9, 11, 2, s, before=[ref.chunk(b'ABCD', b'xy')]), 'size': body(W=40000), 'trailing': good + b'\0',
            'supported': good}


@pytest.mark.parametrize('reason', _lib.PNG_REASONS)
def test_probe_reasons(reason):
    f = _reason_files()[reason]
    got = engine.png_probe(f)
    assert got[0] == reason == ref.probe(f)['reason']
    if reason != 'supported':
        assert got[1:4] == (0, 0, 0) and len(got[4]) == 0


def test_probe_chunk_order():
    a = ref.picture(9, 11, 2, 'smooth')
    s = ref.hand_file(a, 2, stream_only=True)
    split = ref.SIGNATURE + ref.ihdr(9, 11, 2) + ref.chunk(b'IDAT', s[:5]) + ref.chunk(b'tEXt', b'k\0v') + ref.chunk(b'IDAT', s[5:]) + ref.chunk(b'IEND', b'')
    none = ref.SIGNATURE + ref.ihdr(9, 11, 2) + ref.chunk(b'IEND', b'')
    late = ref.SIGNATURE + ref.chunk(b'gAMA', struct.pack('>I', 1)) + ref.ihdr(9, 11, 2) + ref.chunk(b'IDAT', s) + ref.chunk(b'IEND', b'')
    for f in (split, none, late):
        assert engine.png_probe(f)[0] == 'chunk' == ref.probe(f)['reason']
    assert engine.png_probe(b'')[0] == 'truncated' and engine.png_probe(b'abc')[0] == 'not_png'


def _good_args():
    return dict(ranges=[[0, 100], [100, 50]], geom=[[4, 5, 2], [3, 2, 6]], outs=[[0, 15], [60, 8]], in_bytes=150, out_bytes=82, in_ptr=1 << 20,
                out_ptr=1 << 21)


def test_check_png_decode_accepts():
    ranges, geom, outs, need = engine.check_png_decode(**_good_args())
    assert ranges.dtype == np.int64 and geom.dtype == np.int32 and outs.dtype == np.int64 and need == 512


@pytest.mark.parametrize('name,change', [
    ('null input', dict(in_ptr=0)), ('null output', dict(out_bytes=None)), ('no files', dict(ranges=np.zeros((0, 2)), geom=np.zeros((0, 3)), outs=np.zeros((0, 2)))),
    ('too many files', dict(ranges=np.zeros((65536, 2)), geom=np.zeros((65536, 3)), outs=np.zeros((65536, 2)))),
    ('range leaves', dict(ranges=[[0, 100], [100, 51]])), ('negative range', dict(ranges=[[-1, 100], [100, 50]])),
    ('short stream', dict(ranges=[[0, 100], [100, 7]])), ('size', dict(geom=[[4, 5, 2], [0, 2, 6]])), ('colour type', dict(geom=[[4, 5, 2], [3, 2, 3]])),
    ('pitch', dict(outs=[[0, 14], [60, 8]])), ('rectangle leaves', dict(out_bytes=81)), ('negative offset', dict(outs=[[-1, 15], [60, 8]])),
    ('overlapping slabs', dict(out_ptr=(1 << 20) + 149)), ('shared byte', dict(outs=[[0, 15], [59, 8]])), ('raw too small', dict(raw_bytes=511)),
    ('shapes', dict(geom=[[4, 5], [3, 2]])),
    ('too much', dict(ranges=[[0, 100]] * 3, geom=[[32768, 32768, 0]] * 3, outs=[[k * 3 * 32768 * 32768, 3 * 32768] for k in range(3)], out_bytes=9 * 32768 * 32768)),
])
def test_check_png_decode_refuses(name, change):
    with pytest.raises(ValueError):
        engine.check_png_decode(**{**_good_args(), **change})


@pytest.mark.parametrize('name', [n for n, _ in ref.damaged_set()])
def test_damaged_streams(name):
    """A non-zero status in the reference with every index in range (its assertions); the host route is what it was."""
    f = dict(ref.damaged_set())[name]
    assert engine.png_probe(f)[0] == 'supported'
    px, st, _ = ref.decode(f)
    assert st != 0 and px is None

    def outcome(fn):
        try:
            return fn()
        except Exception as e:                                # noqa: BLE001 - whatever Pillow raises is the contract
            return type(e)
    want = outcome(lambda: preprocess._host_rgb(f))
    got = outcome(lambda: preprocess.decode_frames([f], None, False, False)[0])
    assert (want is got) if isinstance(want, type) else np.array_equal(got, want.reshape(-1))


def test_a_flipped_adler_byte_is_pillows_broken_data_stream():
    with pytest.raises(OSError):
        preprocess._host_rgb(dict(ref.damaged_set())['damaged-adler'])


def test_status_names():
    assert ref.ST['zlib'] == 1 and ref.ST['filter'] == 8192 and len(ref.ST) == 14
    a = ref.picture(5, 4, 0, 'smooth')
    raw = bytearray(ref.filter_rows(a, [0] * 5))
    raw[5] = 5                                                  # the second row's filter byte
    px, st, _ = ref.decode(ref.assemble(5, 4, 0, zlib.compress(bytes(raw))))
    assert st == ref.ST['filter']
    bw = ref.BitWriter()
    bw.put(1 | 3 << 1, 3)
    bw.put(0, 13)
    _, st, _ = ref.decode_stream(ref.zlib_wrap(bw, b''), 1, 1, 0)
    assert st == ref.ST['btype']
    bw = ref.BitWriter()
    ref.fixed_block(bw, [0, (3, 2)], 1)
    _, st, _ = ref.decode_stream(ref.zlib_wrap(bw, b'\0\0\0\0'), 1, 3, 0)
    assert st == ref.ST['far']
    bw = ref.BitWriter()
    ref.fixed_block(bw, [0, 0, 0, 0, 0], 1)
    _, st, _ = ref.decode_stream(ref.zlib_wrap(bw, b'\0\0\0\0\0'), 1, 3, 0)
    assert st == ref.ST['length']
    bw = ref.BitWriter()
    bw.put(0, 3)
    bw.align()
    bw.put(4, 16)
    bw.put(4, 16)
    bw.out += b'\0\0\0\0'
    _, st, _ = ref.decode_stream(ref.zlib_wrap(bw, b'\0\0\0\0'), 1, 3, 0)
    assert st == ref.ST['stored']


def test_the_switch_is_off_until_measured():
    assert engine.flow_png_decode_device(None) is engine.PNG_DECODE_DEVICE_DEFAULT
    assert engine.flow_png_decode_device(True) is True and engine.flow_png_decode_device(False) is False
    assert (_lib.PNG_DECODE_LANES, _lib.PNG_DECODE_SUB_BITS) == (256, 512)


def test_a_file_beyond_pillows_pixel_limit_takes_the_host_route(monkeypatch):
    from PIL import Image
    probe = engine.png_probe(_reason_files()['supported'])
    assert engine.png_takes_device(probe)
    monkeypatch.setattr(Image, 'MAX_IMAGE_PIXELS', 9 * 11 - 1)
    assert not engine.png_takes_device(probe)
    monkeypatch.setattr(Image, 'MAX_IMAGE_PIXELS', None)
    assert engine.png_takes_device(probe)
    assert not engine.png_takes_device(engine.png_probe(_reason_files()['palette']))
