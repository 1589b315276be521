"""specmi_color_jitter on MI355X through ``Engine.color_jitter``: every assertion is a byte equality with
tests/golden/color_jitter.npz (Pillow's own outputs) or with tests/color_jitter_ref.py (the contract in NumPy, pinned against the
installed Pillow by tests/test_color_jitter_host.py on the whole domain of every map).

The all-colours frame (4096 x 4096: the whole domain of the hue arithmetic) costs one to two seconds of NumPy per hue shift on
the machine the GPU tests run on; its HSV image is computed once, and the full chain on that frame starts with the hue shift
25 so that it shares that case's result too."""
import ctypes as C

import numpy as np
import pytest
import torch

from spec_amd import _lib, augment
from tests import color_jitter_ref as R
from tests.util import golden, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0xA5
FACTORS = (1.13, 0.87, 1.19)
K = augment.hue_shift(-0.07)


@pytest.fixture(scope='module')
def eng():
    from spec_amd import cam_utils
    return cam_utils._engine(torch.device(DEV))


@pytest.fixture(scope='module')
def gold():
    d = golden('color_jitter.npz')
    frames, outputs, o = [], [], 0
    for H, W in d['sizes']:
        n = int(H) * int(W) * 3
        frames.append(d['frames'][o:o + n].reshape(H, W, 3))
        outputs.append(d['outputs'][o:o + n].reshape(H, W, 3))
        o += n
    return frames, d['records'], outputs


def _layout(frames, pitches=None, gaps=0):
    offsets, off = [], 0
    for k, fr in enumerate(frames):
        H, W = fr.shape[:2]
        p = 3 * W if pitches is None or pitches[k] is None else pitches[k]
        off += gaps
        offsets.append((off, p))
        off += (H - 1) * p + 3 * W
    return np.asarray(offsets, np.int64), off + gaps


def _fill(frames, offsets, nbytes, base=None):
    slab = np.full(nbytes, SENTINEL, np.uint8) if base is None else base.copy()
    for fr, (off, p) in zip(frames, offsets.tolist()):
        H, W = fr.shape[:2]
        for i in range(H):
            slab[off + i * p: off + i * p + 3 * W] = fr[i].reshape(-1)
    return slab


def _sizes(frames):
    return [fr.shape[:2] for fr in frames]


def _run(eng, frames, records, pitches=None, gaps=0, in_place=False):
    """One call -> the output slab on the host, and the layout"""
    offsets, nbytes = _layout(frames, pitches, gaps)
    src = t(_fill(frames, offsets, nbytes)).to(DEV)
    out = src if in_place else torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
    got = eng.color_jitter(src, offsets, _sizes(frames), np.asarray(records, np.int32).reshape(-1, 8), out=out)
    assert got is out
    return out.cpu().numpy(), offsets, nbytes


def _check(eng, frames, records, want, **kw):
    got, offsets, nbytes = _run(eng, frames, records, **kw)
    assert np.array_equal(got, _fill(want, offsets, nbytes))        # the frames, and the sentinel everywhere else


def _frame(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


# ---- the fixture: Pillow's own bytes -------------------------------------------------------------------------------------------
def test_five_ragged_frames_odd_offsets_and_pitches(eng, gold):
    frames, records, outputs = gold
    pick = [0, 1, 2, 3, 30]                                      # 1 x 1, 1 x 7, 5 x 3, 37 x 53, 9 x 13
    fr, rec, want = [frames[i] for i in pick], records[pick], [outputs[i] for i in pick]
    # gaps of 5 bytes put the frames at odd offsets; 5 x 3 at pitch 3 W + 2, 37 x 53 at 3 W + 7 (rows at every alignment), 9 x 13 at 3 W + 1
    for in_place in (False, True):
        _check(eng, fr, rec, want, pitches=[None, None, 11, 3 * 53 + 7, 40], gaps=5, in_place=in_place)
    _check(eng, fr, rec, want)                                  # dense and back to back
    for i in pick[:4]:                                          # and each size alone
        _check(eng, [frames[i]], records[i:i + 1], [outputs[i]])


def test_all_24_orders_in_one_call(eng, gold):
    frames, records, outputs = gold
    assert len({records[i, :4].tobytes() for i in range(4, 28)}) == 24 and len({outputs[i].tobytes() for i in range(4, 28)}) == 24
    _check(eng, frames[4:28], records[4:28], outputs[4:28], gaps=1)
    _check(eng, frames[4:28], records[4:28], outputs[4:28], pitches=[48] * 24)   # every row dword aligned: the wide route


def test_switched_off_operations(eng, gold):
    frames, records, outputs = gold
    sel = list(range(28, 34))
    without = [i for i in sel if R.CONTRAST not in records[i, :4]]
    assert len(without) == 4 and len(sel) - len(without) == 2
    _check(eng, [frames[i] for i in without], records[without], [outputs[i] for i in without], gaps=3)    # no contrast anywhere: one launch
    _check(eng, [frames[i] for i in sel], records[sel], [outputs[i] for i in sel], gaps=3)                # mixed
    assert np.array_equal(outputs[28], frames[28])              # no operation at all: a copy


def test_mean_tie(eng, gold):
    frames, records, outputs = gold
    assert outputs[34].tolist() == [[[11] * 3] * 2]
    _check(eng, [frames[34]], records[34:35], [outputs[34]])


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_factors_0_1_and_1p2(eng):
    rng = np.random.default_rng(51)
    frames = [_frame(rng, 21, 35) for _ in range(3)]
    records = [R.make_record((0, 1, 2, 3), (f, f, f), 25) for f in (0.0, 1.0, 1.2)]
    frames += [_frame(rng, 21, 35) for _ in range(3)]
    records += [R.make_record((2, 3, 1, 0), (f, f, f), 231) for f in (0.0, 1.0, 1.2)]
    want = [R.jitter_record(fr, rec) for fr, rec in zip(frames, records)]
    assert not want[0].any()                                    # brightness 0 first: black
    _check(eng, frames, records, want, gaps=2)


def test_in_place_equals_out_of_place_and_repeats(eng):
    rng = np.random.default_rng(52)
    frames = [_frame(rng, H, W) for H, W in ((33, 300), (7, 5), (40, 257))]
    records = augment.ColorJitter(**augment.CAMCALIB_TRAIN_JITTER).records(3, torch.Generator().manual_seed(52))
    kw = dict(pitches=[904, None, None], gaps=3)
    a, offsets, nbytes = _run(eng, frames, records, **kw)
    b, _, _ = _run(eng, frames, records, **kw)
    c, _, _ = _run(eng, frames, records, in_place=True, **kw)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(a, _fill([R.jitter_record(fr, rec) for fr, rec in zip(frames, records)], offsets, nbytes))


def test_sum_across_workgroups(eng):
    frame = _frame(np.random.default_rng(53), 300, 300)         # 2 x 19 tiles
    for order in ((1,), (3, 0, 1, 2), (2, 1, 3)):
        rec = R.make_record(order, FACTORS, K)
        _check(eng, [frame], [rec], [R.jitter_record(frame, rec)])


def test_sum_beyond_32_bits(eng):
    # L = 255 on 4200 x 4200 pixels: S = 4.498e9 > 2^32, m = 255, every byte stays 255; a 32-bit sum would give m = 12
    H = W = 4200
    assert 255 * H * W > 1 << 32
    src = torch.full((H * W * 3,), 255, dtype=torch.uint8, device=DEV)
    out = eng.color_jitter(src, [0], [(H, W)], R.make_record((1,), (1.0, 0.8, 1.0), 0)[None])
    assert bool((out == 255).all())


_all = {}


def _all_colours():
    """The 4096 x 4096 frame of all 2^24 colours, its HSV image and the hue-shifted frames, each computed once"""
    if 'rgb' not in _all:
        a = np.arange(1 << 24, dtype=np.uint32)
        _all['rgb'] = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
        _all['hsv'] = R.rgb_to_hsv(_all['rgb'])
        _all['dev'] = t(_all['rgb'].reshape(-1)).to(DEV)
    return _all


def _all_colours_shifted(k):
    d = _all_colours()
    if k in d:
        return d[k]
    hsv = d['hsv'].copy()
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + k) % 256
    rgb = R.hsv_to_rgb(hsv)
    if k == 25:                                                 # the full chain starts from this one
        d[k] = rgb
    return rgb


@pytest.mark.parametrize('k', [0, 1, 25, 231, 128])
def test_all_colours_through_hue(eng, k):
    want = _all_colours_shifted(k)
    out = eng.color_jitter(_all_colours()['dev'], [0], [(4096, 4096)], R.make_record((3,), (1.0, 1.0, 1.0), k)[None])
    assert torch.equal(out, t(want.reshape(-1)).to(DEV))


def test_all_colours_through_the_full_chain(eng):
    want = R.jitter(_all_colours_shifted(25), (0, 1, 2), FACTORS, 0)
    out = eng.color_jitter(_all_colours()['dev'], [0], [(4096, 4096)], R.make_record((3, 0, 1, 2), FACTORS, 25)[None])
    assert torch.equal(out, t(want.reshape(-1)).to(DEV))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_every_refusal(eng):
    rng = np.random.default_rng(54)
    frames = [_frame(rng, 8, 9), _frame(rng, 4, 4)]
    off2, nbytes = _layout(frames, [30, None], gaps=3)
    offsets = np.concatenate([off2, off2], axis=1)
    src = t(_fill(frames, off2, nbytes)).to(DEV)
    big = torch.full((2 * nbytes,), 7, dtype=torch.uint8, device=DEV)
    out = big[:nbytes]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    records = np.stack([R.make_record((0, 1, 2, 3), FACTORS, K), R.make_record((3, 2), FACTORS, K)])
    good = dict(src=p(src), nin=nbytes, out=p(out), nout=nbytes, geom=np.array([[8, 9], [4, 4]], np.int32), offsets=offsets, records=records, n=2)

    def call(a):
        arr = lambda x, ty: None if x is None else np.ascontiguousarray(x).ctypes.data_as(ty)
        return eng.lib.specmi_color_jitter(eng.h, a['src'], a['nin'], a['out'], a['nout'], arr(a['geom'], _lib.c_int32_p), arr(a['offsets'], _lib.c_int64_p),
                                           arr(a['records'], _lib.c_int32_p), a['n'], eng._stream())

    def with_(name, row, col, value):
        x = good[name].copy()
        x[row, col] = value
        return {name: x}
    bits = lambda v: int(np.asarray([v], np.float32).view(np.int32)[0])
    shifted = C.c_void_p(big.data_ptr() + 5)
    bad = [dict(src=None), dict(out=None), dict(geom=None), dict(offsets=None), dict(records=None),           # null pointers
           dict(n=0), dict(n=-1), dict(n=65536),                                                               # nframes outside [1, 65535]
           with_('geom', 0, 0, 0), with_('geom', 0, 1, 8193), with_('geom', 1, 0, -3), with_('geom', 1, 0, 8193),  # H or W outside [1, 8192]
           with_('offsets', 0, 1, 26), with_('offsets', 1, 3, 11),                                             # a pitch below 3 W
           dict(nin=nbytes - 4), dict(nout=nbytes - 4), with_('offsets', 0, 0, -1), with_('offsets', 1, 2, nbytes - 47),  # a rectangle leaves a slab
           with_('offsets', 1, 2, 236), with_('offsets', 1, 2, 3),                                             # two frames share an output byte
           dict(out=p(src), **with_('offsets', 0, 2, 4)), dict(out=p(src), **with_('offsets', 0, 3, 31)),      # the same slab, other rectangles
           dict(src=p(big), nin=2 * nbytes, out=shifted, nout=nbytes),                                         # overlapping, not the same
           with_('records', 0, 0, 4), with_('records', 1, 2, -2), with_('records', 0, 1, 0), with_('records', 1, 2, 3),  # an id outside [-1, 3] or repeated
           with_('records', 0, 4, bits(-0.5)), with_('records', 1, 5, bits(np.nan)), with_('records', 0, 6, bits(np.inf)),  # a factor negative or not finite
           with_('records', 0, 7, 256), with_('records', 1, 7, -1)]                                            # k outside [0, 255]
    for b in bad:
        assert call(dict(good, **b)) == _lib.ERR_ARG, {k: None for k in b}
        assert eng.lib.specmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert bool((big == 7).all())                               # nothing was launched
    assert call(good) == _lib.OK
    want = _fill([R.jitter_record(fr, rec) for fr, rec in zip(frames, records)], off2, nbytes, base=np.full(nbytes, 7, np.uint8))
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError):                             # and the Python binding refuses before the library is reached
        eng.color_jitter(src, off2, [(8, 9), (4, 4)], with_('records', 0, 7, 256)['records'], out=out)


def test_graph_capture_needs_the_records_of_the_previous_call(eng):
    frame = _frame(np.random.default_rng(55), 20, 70)
    rec = R.make_record((0, 1, 2, 3), FACTORS, K)[None]
    src = t(frame.reshape(-1).copy()).to(DEV)
    want = eng.color_jitter(src, [0], [(20, 70)], rec).clone()             # also the warm-up call of the capture below
    assert np.array_equal(want.cpu().numpy().reshape(20, 70, 3), R.jitter_record(frame, rec[0]))
    out = torch.zeros_like(src)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):
        try:                                                                # new records: refused, and the capture goes on
            eng.color_jitter(src, [0], [(20, 70)], R.make_record((3,), FACTORS, K)[None], out=out)
        except _lib.SpecmiError as e:
            err = e
        eng.color_jitter(src, [0], [(20, 70)], rec, out=out)                # the previous call's records: captured
    assert err is not None and err.code == _lib.ERR_STATE, err
    torch.cuda.synchronize()
    assert not out.any()                                                    # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    g.replay()                                                              # the sums are zeroed inside the graph
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ---- through the resize -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_through_the_resize(eng, dtype):
    from spec_amd.camcalib_eval import pad_batch
    from spec_amd.preprocess import pack_frames
    rng = np.random.default_rng(56)
    frames = [_frame(rng, H, W) for H, W in ((60, 80), (75, 50), (40, 40))]
    cj = augment.ColorJitter(**augment.CAMCALIB_TRAIN_JITTER)
    records = cj.records(3, torch.Generator().manual_seed(56))
    jittered = cj(pack_frames(frames, torch.device(DEV)), torch.Generator().manual_seed(56), engine=eng)
    got = pad_batch(jittered, 32, 48, DEV, eng, dtype=dtype)
    want = pad_batch([R.jitter_record(fr, rec) for fr, rec in zip(frames, records)], 32, 48, DEV, eng, dtype=dtype)
    assert got.dtype == dtype and torch.equal(got, want)
