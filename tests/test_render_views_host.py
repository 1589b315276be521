"""The host side of specmi_render_views: ``render.plan_views`` lays out the three-panel pictures of a flush (offsets, pitches,
mesh ranges, chunks) and ``engine.check_render_views`` - everything ``Engine.render_views`` checks that needs no device - refuses
what include/specmi.h lists.  No GPU."""
import numpy as np
import pytest

from spec_amd import _lib, engine, records, render

SIZES, COUNTS = [(33, 47), (64, 96), (40, 40)], [3, 2, 1]
SIDE = _lib.RENDER_SIDE_VIEW | _lib.RENDER_GROUND_PLANE | _lib.RENDER_CULL


def _rows(ch):
    """the set of (first byte, bytes) of every row of every view of a chunk's output slab"""
    rows = []
    for (H, W, *_), (_, _, off, pitch) in zip(ch['geom'].tolist(), ch['offsets'].tolist()):
        rows += [(off + i * pitch, 3 * W) for i in range(H)]
    return rows


def _check_layout(ch, gap):
    pics = ch['pictures']
    assert ch['geom'].shape == (3 * len(pics), 5) and ch['offsets'].shape == (3 * len(pics), 4) and ch['geom'].dtype == np.int32
    at = 0
    for p, (f, _) in enumerate(pics):
        H, W = SIZES[f]
        assert ch['picture_offsets'][p] == at
        for k in range(3):
            in_off, in_pitch, out_off, out_pitch = ch['offsets'][3 * p + k]
            assert (out_off, out_pitch, in_pitch) == (at + 3 * W * k, 9 * W, 3 * W)
            assert in_off == sum(SIZES[g][0] * SIZES[g][1] * 3 for g in ch['frames'] if g < f)
            assert tuple(ch['geom'][3 * p + k][:2]) == (H, W) and ch['view_frame'][3 * p + k] == f
        at += 9 * H * W + gap
    assert ch['out_bytes'] == at - gap
    assert ch['in_bytes'] == sum(SIZES[g][0] * SIZES[g][1] * 3 for g in ch['frames'])
    # rectangles: inside the slab, disjoint, and together exactly the pictures (every byte of a picture belongs to one view)
    rows = sorted(_rows(ch))
    assert rows[0][0] >= 0 and rows[-1][0] + rows[-1][1] <= ch['out_bytes']
    assert all(a + n <= b for (a, n), (b, _) in zip(rows, rows[1:]))
    assert sum(n for _, n in rows) == sum(9 * SIZES[f][0] * SIZES[f][1] for f, _ in pics)


@pytest.mark.parametrize('gap', [0, 7])
def test_plan_views_together(gap):
    (ch,) = render.plan_views(SIZES, COUNTS, gap=gap)
    assert ch['pictures'] == [(0, None), (1, None), (2, None)] and ch['frames'] == [0, 1, 2]
    _check_layout(ch, gap)
    want = []
    for m0, c in ((0, 3), (3, 2), (5, 1)):
        want += [(0, 0, 0), (m0, c, _lib.RENDER_CULL), (m0, c, SIDE)]
    assert [tuple(r) for r in ch['geom'][:, 2:].tolist()] == want


def test_plan_views_each_detection_alone():
    (ch,) = render.plan_views(SIZES, COUNTS, each=True, cull=False)
    assert ch['pictures'] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)] and ch['frames'] == [0, 1, 2]
    _check_layout(ch, 0)
    want = []
    for m in range(6):
        want += [(0, 0, 0), (m, 1, 0), (m, 1, SIDE & ~_lib.RENDER_CULL)]
    assert [tuple(r) for r in ch['geom'][:, 2:].tolist()] == want


def test_plan_views_chunks():
    px = [3 * h * w for h, w in SIZES]
    # a budget that holds any one picture but no two: three chunks, each with its own frame slab from offset 0
    chunks = render.plan_views(SIZES, COUNTS, pixel_budget=max(px))
    assert [c['pictures'] for c in chunks] == [[(0, None)], [(1, None)], [(2, None)]] and [c['frames'] for c in chunks] == [[0], [1], [2]]
    for c in chunks:
        _check_layout(c, 0)
        assert (c['offsets'][:, 0] == 0).all()
    assert [tuple(c['geom'][1, 2:4]) for c in chunks] == [(0, 3), (3, 2), (5, 1)]          # mesh ranges stay those of the flush
    # smaller than a single picture: a view is never split, a chunk still holds one picture
    chunks = render.plan_views(SIZES, COUNTS, pixel_budget=100)
    assert [c['pictures'] for c in chunks] == [[(0, None)], [(1, None)], [(2, None)]]
    # two pictures fit, the third does not; with `each` a frame whose detections straddle two chunks is in both frame slabs
    chunks = render.plan_views(SIZES, COUNTS, pixel_budget=px[0] + px[1])
    assert [c['pictures'] for c in chunks] == [[(0, None), (1, None)], [(2, None)]]
    chunks = render.plan_views(SIZES, COUNTS, each=True, pixel_budget=2 * px[0])
    assert [c['pictures'] for c in chunks] == [[(0, 0), (0, 1)], [(0, 2)], [(1, 0)], [(1, 1)], [(2, 0)]]
    assert [c['frames'] for c in chunks] == [[0], [0], [1], [1], [2]]
    for c in chunks:
        _check_layout(c, 0)
        assert sum(h * w for h, w, *_ in c['geom'].tolist()) <= 2 * px[0] or len(c['pictures']) == 1
    assert render.plan_views(SIZES, COUNTS)[0]['out_bytes'] * 8 // 9 < engine.RENDER_PIXEL_BUDGET          # the default holds the flush
    for bad in (dict(sizes=[], counts=[]), dict(sizes=SIZES, counts=[1, 1]), dict(sizes=SIZES, counts=[1, 0, 1]), dict(sizes=[(0, 4)], counts=[1])):
        with pytest.raises(ValueError):
            render.plan_views(**bad)


def _good():
    (ch,) = render.plan_views(SIZES, COUNTS)
    cams = render.view_cams(ch['view_frame'], np.stack([np.eye(3)] * 3), [(40., 41.)] * 3, [(20., 16.)] * 3)
    return dict(Mtot=6, V=162, F=320, geom=ch['geom'].copy(), offsets=ch['offsets'].copy(), cams=cams, in_bytes=ch['in_bytes'],
                out_bytes=ch['out_bytes'], rgb=(0.8, 0.5, 0.6))


def _set(name, row, col, value):
    def change(a):
        a[name][row, col] = value
    return change


# one entry per refusal of include/specmi.h that the host arrays decide
REFUSALS = {
    'no views': lambda a: a.update(geom=a['geom'][:0], offsets=a['offsets'][:0], cams=a['cams'][:0]),
    'too many views': lambda a: a.update(geom=np.repeat(a['geom'], 8000, 0), offsets=np.repeat(a['offsets'], 8000, 0), cams=np.repeat(a['cams'], 8000, 0)),
    'rows disagree': lambda a: a.update(cams=a['cams'][:-1]),
    'V below 1': lambda a: a.update(V=0),
    'F below 1': lambda a: a.update(F=0),
    'mesh range past Mtot': lambda a: a.update(Mtot=5),
    'negative mesh0': _set('geom', 1, 2, -1),
    'negative count': _set('geom', 1, 3, -1),
    'count * F of 2^31': lambda a: (a.update(Mtot=1 << 23, F=1 << 9), _set('geom', 1, 3, 1 << 22)(a)),
    'pixels of 2^31': lambda a: (a['geom'].__setitem__((slice(None), slice(0, 2)), 32768), a['offsets'].__setitem__((slice(None), 3), 9 * 32768)),
    'H of 0': _set('geom', 4, 0, 0),
    'W past 32768': _set('geom', 4, 1, 32769),
    'out pitch below 3 W': _set('offsets', 2, 3, 3 * 47 - 1),
    'in pitch below 3 W': _set('offsets', 1, 1, 3 * 47 - 1),
    'output leaves the slab': lambda a: a.update(out_bytes=a['out_bytes'] - 1),
    'negative out offset': _set('offsets', 0, 2, -1),
    'frame leaves the slab': lambda a: a.update(in_bytes=a['in_bytes'] - 1),
    'slab of 4 GiB': lambda a: a.update(out_bytes=1 << 32),
    'frame slab of 4 GiB': lambda a: a.update(in_bytes=1 << 32),
    'views overlap (same pitch)': _set('offsets', 1, 2, 3 * 47 - 1),
    'views overlap (other pitch)': lambda a: (_set('offsets', 8, 2, 0)(a), _set('offsets', 8, 3, 3 * 40)(a)),
    'unknown flag': _set('geom', 1, 4, 16),
    'ground plane without side view': _set('geom', 1, 4, _lib.RENDER_GROUND_PLANE),
    'ground plane without meshes': _set('geom', 0, 4, SIDE),
    'overlay without frame': _set('offsets', 1, 0, -1),
    'frame without slab': lambda a: a.update(in_bytes=None),
    'thread per triangle on one view': _set('geom', 1, 4, _lib.RENDER_CULL | _lib.RENDER_THREAD_PER_TRIANGLE),
    'focal of 0': _set('cams', 3, 9, 0.0),
    'focal not finite': _set('cams', 3, 10, np.inf),
    'centre not finite': _set('cams', 3, 12, np.nan),
    'R not finite': _set('cams', 3, 4, np.nan),
    'colour not finite': lambda a: a.update(rgb=(1., np.nan, 1.)),
    'colour of two': lambda a: a.update(rgb=(1., 1.)),
}


def test_check_render_views_accepts_the_plan():
    geom, offsets, cams, rgb = engine.check_render_views(**_good())
    assert (geom.dtype, offsets.dtype, cams.dtype, rgb.dtype) == (np.int32, np.int64, np.float32, np.float32)
    assert all(a.flags['C_CONTIGUOUS'] for a in (geom, offsets, cams, rgb))
    a = _good()       # a side view needs no frame, and then no frame slab; a single row may have any pitch
    a['offsets'][:, 0] = -1
    a['geom'][:, 4] |= _lib.RENDER_SIDE_VIEW
    a['in_bytes'] = None
    engine.check_render_views(**a)
    a = dict(_good(), geom=np.array([[1, 5, 0, 1, 4]]), offsets=np.array([[0, 0, 3, 1]]), cams=_good()['cams'][:1])
    with pytest.raises(ValueError):
        engine.check_render_views(**a)       # 1 < 3 W even for a single row
    a['offsets'][0, 1:] = (1 << 40, 3, 1 << 40)
    engine.check_render_views(**a)


@pytest.mark.parametrize('name', list(REFUSALS))
def test_check_render_views_refuses(name):
    a = _good()
    REFUSALS[name](a)
    with pytest.raises(ValueError):
        engine.check_render_views(**a)


def test_first_overlap_against_every_byte():
    """``records.first_overlap`` reports a pair exactly when two rectangles share a byte, and then a pair that does: against the
    bytes of every rectangle written out, on seeded sets of small rectangles of mixed pitches, one-row ones among them."""
    rng = np.random.default_rng(5)
    met = 0
    for _ in range(400):
        rects = []
        for _ in range(int(rng.integers(2, 7))):
            H, row = int(rng.integers(1, 5)), int(rng.integers(1, 7))
            pitch = int(rng.integers(row, 13)) if H > 1 else row        # a single row's pitch counts as its row (records.byte_rects)
            rects.append((int(rng.integers(0, 120)), pitch, row, H))
        held = [{o + y * p + x for y in range(h) for x in range(r)} for o, p, r, h in rects]
        shared = any(held[a] & held[b] for a in range(len(rects)) for b in range(a))
        pair = records.first_overlap(rects)
        assert (pair is not None) == shared, rects
        if pair:
            assert pair[0] != pair[1] and held[pair[0]] & held[pair[1]], (rects, pair)
            met += 1
    assert 50 <= met <= 350         # both answers are exercised, each by 50 of the 400 sets at least
