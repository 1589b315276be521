"""The two crops from frames of DIFFERENT sizes in one launch (specmi_crop_normalize_ragged, specmi_crop_resize_normalize_ragged
and their NHWC8 fp16 twins; spec_amd.preprocess.crop_detections_ragged / dataset_crops_ragged) against the per-frame calls on
the same frame.  The ragged kernels run the per-frame kernels' device functions on the frame's own H and W, so every
comparison is ``torch.equal``: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from spec_amd import _lib, cam_utils
from spec_amd.engine import _ptr
from spec_amd.preprocess import (crop_detections, crop_detections_ragged, dataset_crops, dataset_crops_ragged, pack_frames,
                                 pare_crop_boxes)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
# 3 x 2 = 18 bytes is the smallest frame that takes the 8-byte tap load; packed back to back the offsets come out odd
SIZES = [(1, 1), (1, 7), (2, 1), (3, 2), (37, 53), (64, 48), (240, 320)]
UNUSED = 5            # the 64 x 48 frame serves no crop
SIZES_S = (224, 33, 8)


@pytest.fixture(scope='module')
def eng():
    return cam_utils._engine(torch.device(DEV))


def _demo_boxes(H, W):
    """[cx, cy, w, h]: inside, across the four edges, wholly outside, larger than the frame, w = 0, h = 0, covering the frame"""
    bw, bh = 0.6 * W + 1, 0.6 * H + 1
    return [[W / 2, H / 2, max(0.5 * W, 1), max(0.5 * H, 1)], [0, H / 2, bw, bh], [W, H / 2, bw, bh], [W / 2, 0, bw, bh], [W / 2, H, bw, bh],
            [3 * W + 50, 3 * H + 50, bw, bh], [W / 2, H / 2, 2.5 * W + 3, 2.5 * H + 3], [W / 2, H / 2, 0, H], [W / 2, H / 2, W, 0],
            [W / 2, H / 2, W, H]]


def _dataset_boxes(H, W):
    """(centre x, centre y, scale): the integer box is [c - 100 s, c + 100 s).  Same cases; degenerate = br <= ul (a tiny scale)"""
    s = (0.6 * min(H, W) + 2) / 200
    return [[W / 2, H / 2, max(min(H, W) / 400, 0.006)], [0, H / 2, s], [W, H / 2, s], [W / 2, 0, s], [W / 2, H, s],
            [3 * W + 50, 3 * H + 50, 0.1], [W / 2, H / 2, max(H, W) / 100 + 0.05], [W / 2 + 0.5, H / 2 + 0.5, 1e-4],
            [W / 2, H / 2, max(H, W) / 200 + 0.01]]


@pytest.fixture(scope='module')
def world():
    """The frames, two slabs that hold them (back to back in order / another order with gaps of 255s), and the crops: listed out
    of frame order, the big frame serving many, one frame serving none."""
    rng = np.random.default_rng(20)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SIZES]
    slab_a, off_a, sizes = pack_frames(frames, DEV)
    assert sizes == SIZES and int(off_a[-1]) + 240 * 320 * 3 == slab_a.numel()            # the last frame ends on the last byte
    assert any(int(o) % 2 for o in off_a)
    order, gaps = [6, 2, 0, 4, 3, 5, 1], [0, 1, 5, 13, 0, 1, 5]
    parts, off_b = [], [0] * len(SIZES)
    pos = 0
    for f, g in zip(order, gaps):
        parts.append(np.full(g, 255, np.uint8))
        off_b[f] = pos + g
        parts.append(frames[f].reshape(-1))
        pos += g + frames[f].size
    slab_b = torch.from_numpy(np.concatenate(parts)).to(DEV)
    demo, data, fidx = [], [], []
    for f, (H, W) in enumerate(SIZES):
        if f == UNUSED:
            continue
        demo += [(f, b) for b in _demo_boxes(H, W)]
        data += [(f, b) for b in _dataset_boxes(H, W)]
    demo += [(6, [rng.uniform(0, 320), rng.uniform(0, 240), rng.uniform(40, 300), rng.uniform(40, 260)]) for _ in range(8)]
    data += [(6, [rng.uniform(0, 320), rng.uniform(0, 240), rng.uniform(0.2, 1.6)]) for _ in range(8)]
    demo = [demo[i] for i in rng.permutation(len(demo))]
    data = [data[i] for i in rng.permutation(len(data))]
    boxes_i = pare_crop_boxes([b[:2] for _, b in data], [b[2] for _, b in data])
    assert (boxes_i[:, 2] <= boxes_i[:, 0]).any(), 'no degenerate dataset box'
    return {'frames': [torch.from_numpy(fr).to(DEV) for fr in frames], 'sizes': sizes,
            'slabs': {'packed': (slab_a, off_a), 'gaps': (slab_b, np.asarray(off_b, np.int64))},
            'demo_fidx': np.asarray([f for f, _ in demo], np.int32), 'demo_boxes': np.asarray([b for _, b in demo], np.float32),
            'data_fidx': np.asarray([f for f, _ in data], np.int32), 'data_c': np.asarray([b[:2] for _, b in data], np.float64),
            'data_s': np.asarray([b[2] for _, b in data], np.float64)}


@pytest.fixture(scope='module')
def refs(world, eng):
    """Per crop size: what the per-frame calls give for every crop, frame by frame - computed once, never modified."""
    out = {}
    for S in SIZES_S:
        n = len(world['demo_fidx'])
        d = {'img': torch.empty(n, 3, S, S, device=DEV), 'raw': torch.empty(n, S, S, 3, dtype=torch.uint8, device=DEV),
             'sc': torch.empty(n, device=DEV), 'ce': torch.empty(n, 2, device=DEV),
             'data': torch.empty(len(world['data_fidx']), 3, S, S, device=DEV)}
        for f, frame in enumerate(world['frames']):
            sel = np.nonzero(world['demo_fidx'] == f)[0]
            if len(sel):
                r = crop_detections(frame, world['demo_boxes'][sel], scale=1.0, crop_size=S, return_raw=True)
                d['img'][sel], d['raw'][sel], d['sc'][sel], d['ce'][sel] = r['inp_images'], r['raw'], r['bbox_scale'], r['bbox_center']
            sel = np.nonzero(world['data_fidx'] == f)[0]
            if len(sel):
                d['data'][sel] = dataset_crops(frame, world['data_c'][sel], world['data_s'][sel], S)
        d['img16'], d['data16'] = eng.to_nhwc_f16(d['img']), eng.to_nhwc_f16(d['data'])
        out[S] = d
    torch.cuda.synchronize()
    return out


def _host(a, ctype, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a, (None if a.size == 0 else a.ctypes.data_as(ctype))


def _raw_demo(eng, slab, slab_bytes, offsets, geom, nframes, fidx, boxes, n, S, out, f16=False, raw=None, sc=None, ce=None, scale=1.0):
    """specmi_crop_normalize_ragged / specmi_crop_normalize_f16_ragged as a C caller sees it; a None / empty argument is a null pointer"""
    _o, po = _host([] if offsets is None else offsets, _lib.c_int64_p, np.int64)
    _g, pg = _host([] if geom is None else geom, _lib.c_int32_p, np.int32)
    fn = eng.lib.specmi_crop_normalize_f16_ragged if f16 else eng.lib.specmi_crop_normalize_ragged
    return fn(eng.h, _ptr(slab), slab_bytes, po, pg, nframes, _ptr(fidx), _ptr(boxes), n, scale, S, out if isinstance(out, int) else _ptr(out),
              _ptr(raw), _ptr(sc), _ptr(ce), eng._stream())


def _raw_data(eng, slab, slab_bytes, offsets, geom, nframes, fidx, boxes, n, S, out, f16=False):
    _o, po = _host([] if offsets is None else offsets, _lib.c_int64_p, np.int64)
    _g, pg = _host([] if geom is None else geom, _lib.c_int32_p, np.int32)
    fn = eng.lib.specmi_crop_resize_normalize_f16_ragged if f16 else eng.lib.specmi_crop_resize_normalize_ragged
    return fn(eng.h, _ptr(slab), slab_bytes, po, pg, nframes, _ptr(fidx), _ptr(boxes), n, S, out if isinstance(out, int) else _ptr(out),
              eng._stream())


@pytest.mark.parametrize('which', ['packed', 'gaps'])
@pytest.mark.parametrize('S', SIZES_S)
def test_demo_crops_equal_the_per_frame_crops(world, refs, eng, S, which):
    slab, offsets = world['slabs'][which]
    ref, n = refs[S], len(world['demo_fidx'])
    fidx, boxes = torch.from_numpy(world['demo_fidx']).to(DEV), torch.from_numpy(world['demo_boxes']).to(DEV)
    for f16 in (False, True):
        img = torch.empty((n, S, S, 8), dtype=torch.float16, device=DEV) if f16 else torch.empty(n, 3, S, S, device=DEV)
        raw, sc, ce = torch.empty_like(ref['raw']), torch.empty_like(ref['sc']), torch.empty_like(ref['ce'])
        _lib.check(eng.h, _raw_demo(eng, slab, slab.numel(), offsets, world['sizes'], len(SIZES), fidx, boxes, n, S, img, f16, raw, sc, ce))
        assert torch.equal(img, ref['img16'] if f16 else ref['img']), f16
        assert torch.equal(raw, ref['raw']) and torch.equal(sc, ref['sc']) and torch.equal(ce, ref['ce']), f16
        got = crop_detections_ragged(slab, offsets, world['sizes'], world['demo_fidx'], world['demo_boxes'], crop_size=S,
                                     dtype=torch.float16 if f16 else torch.float32)
        assert torch.equal(got['inp_images'], img) and torch.equal(got['bbox_scale'], sc) and torch.equal(got['bbox_center'], ce)


@pytest.mark.parametrize('which', ['packed', 'gaps'])
@pytest.mark.parametrize('S', SIZES_S)
def test_dataset_crops_equal_the_per_frame_crops(world, refs, S, which):
    slab, offsets = world['slabs'][which]
    args = (slab, offsets, world['sizes'], world['data_fidx'], world['data_c'], world['data_s'], S)
    assert torch.equal(dataset_crops_ragged(*args), refs[S]['data'])
    assert torch.equal(dataset_crops_ragged(*args, dtype=torch.float16), refs[S]['data16'])


def test_a_crop_beyond_the_coordinate_tables(world, eng):
    """S = 2049 takes the TABLE = false kernels: one crop per kind from the 37 x 53 frame, fp32 and NHWC8 fp16."""
    S, f = 2049, 4
    slab, offsets = world['slabs']['packed']
    box = np.asarray([[30.0, 20.0, 45.0, 50.0]], np.float32)
    ref = crop_detections(world['frames'][f], box, crop_size=S)
    got = crop_detections_ragged(slab, offsets, world['sizes'], [f], box, crop_size=S)
    assert all(torch.equal(got[k], ref[k]) for k in ref)
    got = crop_detections_ragged(slab, offsets, world['sizes'], [f], box, crop_size=S, dtype=torch.float16)
    assert torch.equal(got['inp_images'], eng.to_nhwc_f16(ref['inp_images']))
    del got
    ref = dataset_crops(world['frames'][f], [[25.0, 18.0]], [0.21], S)
    assert torch.equal(dataset_crops_ragged(slab, offsets, world['sizes'], [f], [[25.0, 18.0]], [0.21], S), ref)
    assert torch.equal(dataset_crops_ragged(slab, offsets, world['sizes'], [f], [[25.0, 18.0]], [0.21], S, dtype=torch.float16),
                       eng.to_nhwc_f16(ref))


@pytest.mark.parametrize('f16', [False, True])
def test_out_slices_are_written_in_place_and_nothing_beyond(world, refs, f16):
    S, n = 33, len(world['demo_fidx'])
    slab, offsets = world['slabs']['packed']
    dtype, key = (torch.float16, 'img16') if f16 else (torch.float32, 'img')
    buf = {'inp_images': torch.full((n + 5, S, S, 8) if f16 else (n + 5, 3, S, S), 7.0, dtype=dtype, device=DEV),
           'bbox_scale': torch.full((n + 5,), 7.0, device=DEV), 'bbox_center': torch.full((n + 5, 2), 7.0, device=DEV)}
    got = crop_detections_ragged(slab, offsets, world['sizes'], world['demo_fidx'], world['demo_boxes'], crop_size=S, dtype=dtype,
                                 out={k: v[2:2 + n] for k, v in buf.items()})
    assert got['inp_images'].data_ptr() == buf['inp_images'][2:].data_ptr()
    for k, r in (('inp_images', refs[S][key]), ('bbox_scale', refs[S]['sc']), ('bbox_center', refs[S]['ce'])):
        assert torch.equal(buf[k][2:2 + n], r), k
        assert bool((buf[k][:2] == 7).all()) and bool((buf[k][2 + n:] == 7).all()), k
    nd = len(world['data_fidx'])
    big = torch.full((nd + 3, S, S, 8) if f16 else (nd + 3, 3, S, S), 7.0, dtype=dtype, device=DEV)
    dataset_crops_ragged(slab, offsets, world['sizes'], world['data_fidx'], world['data_c'], world['data_s'], S, dtype=dtype, out=big[1:1 + nd])
    assert torch.equal(big[1:1 + nd], refs[S]['data16' if f16 else 'data']) and bool((big[:1] == 7).all()) and bool((big[1 + nd:] == 7).all())
    with pytest.raises(ValueError):
        crop_detections_ragged(slab, offsets, world['sizes'], world['demo_fidx'], world['demo_boxes'], crop_size=S, dtype=dtype,
                               out={k: v[:n - 1] for k, v in buf.items()})
    with pytest.raises(ValueError):
        dataset_crops_ragged(slab, offsets, world['sizes'], world['data_fidx'], world['data_c'], world['data_s'], S, dtype=dtype, out=big)


def test_frame_index_out_of_range_is_rejected_on_the_host_and_clamped_on_the_device(world, eng):
    slab, offsets = world['slabs']['packed']
    F, S = len(SIZES), 33
    dets = np.asarray([[20., 16., 30., 30.], [100., 100., 120., 150.], [1., 1., 3., 3.]], np.float32)
    cs, sc = [[20., 16.], [100., 100.], [1., 1.]], [0.2, 0.7, 0.02]
    for bad in ([0, F, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match=rf'\[0, {F}\)'):
            crop_detections_ragged(slab, offsets, world['sizes'], bad, dets, crop_size=S)
        with pytest.raises(ValueError, match=rf'\[0, {F}\)'):
            dataset_crops_ragged(slab, offsets, world['sizes'], torch.tensor(bad, dtype=torch.int32), cs, sc, S)
    on_dev = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)        # the host cannot look at it: the kernel clamps
    bad = crop_detections_ragged(slab, offsets, world['sizes'], on_dev([4, F + 70, -5]), dets, crop_size=S)
    ref = crop_detections_ragged(slab, offsets, world['sizes'], on_dev([4, F - 1, 0]), dets, crop_size=S)
    assert torch.equal(bad['inp_images'], ref['inp_images'])
    assert torch.equal(ref['inp_images'][1:2], crop_detections(world['frames'][F - 1], dets[1:2], crop_size=S)['inp_images'])
    assert torch.equal(ref['inp_images'][2:3], crop_detections(world['frames'][0], dets[2:3], crop_size=S)['inp_images'])
    bad = dataset_crops_ragged(slab, offsets, world['sizes'], on_dev([4, 2 ** 31 - 1, -2 ** 31]), cs, sc, S)
    assert torch.equal(bad[1:2], dataset_crops(world['frames'][F - 1], cs[1:2], sc[1:2], S))
    assert torch.equal(bad[2:3], dataset_crops(world['frames'][0], cs[2:3], sc[2:3], S))


@pytest.mark.parametrize('kind', ['demo', 'dataset'])
def test_bad_arguments_are_refused_launch_nothing_and_leave_the_handle_usable(world, refs, eng, kind):
    S = 8
    slab, offsets = world['slabs']['packed']
    demo = kind == 'demo'
    n = len(world['demo_fidx'] if demo else world['data_fidx'])
    fidx = torch.from_numpy(world['demo_fidx'] if demo else world['data_fidx']).to(DEV)
    boxes = torch.from_numpy(world['demo_boxes'] if demo else pare_crop_boxes(world['data_c'], world['data_s'], S)).to(DEV)
    call = _raw_demo if demo else _raw_data
    ref32, ref16 = (refs[S]['img'], refs[S]['img16']) if demo else (refs[S]['data'], refs[S]['data16'])
    out32, out16 = torch.full_like(ref32, 7.0), torch.full((n * S * S * 8 + 8,), 7.0, dtype=torch.float16, device=DEV)
    good = dict(slab=slab, slab_bytes=slab.numel(), offsets=offsets, geom=world['sizes'], nframes=len(SIZES), fidx=fidx, boxes=boxes, n=n,
                S=S, out=out32)
    # the frame with the bad record is never named by a crop: every crop of these calls is cut from frame 0
    two = dict(nframes=2, fidx=torch.zeros(n, dtype=torch.int32, device=DEV))
    geom2 = lambda H, W: dict(two, geom=[(1, 1), (H, W)], offsets=[0, 3])
    bad = {
        'null slab': dict(slab=None), 'null offsets': dict(offsets=None), 'null sizes': dict(geom=None), 'null frame_index': dict(fidx=None),
        'null boxes': dict(boxes=None), 'null output': dict(out=None),
        'n = 0': dict(n=0), 'n < 0': dict(n=-1), 'n > 65535': dict(n=65536), 'nframes = 0': dict(nframes=0), 'nframes < 0': dict(nframes=-3),
        'H < 1': geom2(0, 1), 'W < 1': geom2(1, 0), 'H < 0': geom2(-4, 1),
        'H = 2^24': dict(geom2(1 << 24, 1), slab_bytes=3 + 3 * (1 << 24)), 'W = 2^24': dict(geom2(1, 1 << 24), slab_bytes=3 + 3 * (1 << 24)),
        'negative offset': dict(two, geom=[(1, 1), (1, 1)], offsets=[0, -1]),
        'a frame that leaves the slab': dict(slab_bytes=slab.numel() - 1),
        'an offset that leaves the slab': dict(two, geom=[(1, 1), (2, 2)], offsets=[0, slab.numel() - 11]),
        'a slab of 4 GiB': dict(slab_bytes=1 << 32), 'crop_size = 0': dict(S=0), 'crop_size < 0': dict(S=-224),
        'NHWC8 output off 16 bytes': dict(out=out16.data_ptr() + 2, f16=True),
    }
    names = ('crop_normalize_ragged', 'crop_normalize_ragged_f16') if demo else ('crop_resize_normalize_ragged', 'crop_resize_normalize_ragged_f16')
    launches = lambda: sum(e['launches'] for e in eng.profile_read(64) if e['kernel'] in names)
    eng.profile(True)
    try:
        for what, change in bad.items():
            rc = call(eng, **dict(good, **change))
            assert rc == _lib.ERR_ARG, (what, rc)
            assert eng.lib.specmi_last_error(eng.h), what
            torch.cuda.synchronize()
            assert launches() == 0, f'{what}: a refused call launched the kernel'
            assert bool((out32 == 7).all()) and bool((out16 == 7).all()), what
            # ... and the handle serves the next call, bit for bit
            eng.profile(False)
            assert call(eng, **good) == 0, what
            assert torch.equal(out32, ref32), what
            out32.fill_(7.0)
            eng.profile(True)
        assert call(eng, **dict(good, out=out16[:n * S * S * 8], f16=True)) == 0
        torch.cuda.synchronize()
        assert launches() == 1
    finally:
        eng.profile(False)
    assert torch.equal(out16[:n * S * S * 8].view(n, S, S, 8), ref16) and bool((out16[n * S * S * 8:] == 7).all())


def test_the_table_is_rewritten_only_when_the_records_change(world, refs):
    """Equal records twice, different records (the other slab's offsets, then a subset of the frames), the first again: every
    call reads the table that belongs to it."""
    S = 33
    (slab_a, off_a), (slab_b, off_b) = world['slabs']['packed'], world['slabs']['gaps']
    demo = lambda slab, off: crop_detections_ragged(slab, off, world['sizes'], world['demo_fidx'], world['demo_boxes'], crop_size=S)
    data = lambda slab, off: dataset_crops_ragged(slab, off, world['sizes'], world['data_fidx'], world['data_c'], world['data_s'], S)
    got = [demo(slab_a, off_a), demo(slab_a, off_a), demo(slab_b, off_b), demo(slab_a, off_a)]
    got_d = [data(slab_a, off_a), data(slab_a, off_a), data(slab_b, off_b), data(slab_a, off_a)]     # the same table serves both kinds
    # fewer frames than the table holds: the last two frames alone, as a slab of their own
    H, W = SIZES[6]
    sub = crop_detections_ragged(slab_a[int(off_a[5]):], off_a[5:] - off_a[5], SIZES[5:], [1, 1], [[160., 120., 200., 220.], [0., 0., 90., 90.]],
                                 crop_size=S)
    again = demo(slab_a, off_a)
    for g in got + [again]:
        assert torch.equal(g['inp_images'], refs[S]['img']) and torch.equal(g['bbox_center'], refs[S]['ce'])
    for g in got_d:
        assert torch.equal(g, refs[S]['data'])
    ref = crop_detections(world['frames'][6], [[160., 120., 200., 220.], [0., 0., 90., 90.]], crop_size=S)
    assert torch.equal(sub['inp_images'], ref['inp_images'])
