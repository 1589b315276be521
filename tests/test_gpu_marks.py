"""specmi_draw_marks and specmi_denormalize_u8 on MI355X: every assertion is an equality with tests/marks_ref.py (the marks
contract in NumPy, itself pinned against the installed Pillow by tests/test_marks_host.py) - ragged slabs with padding, gaps and
a panel-0 column, lines of every kind, masks at every edge, painter's order, every refusal of the C ABI, the two routes of
``render_image_group(s)`` byte for byte, and CamCalib's validation pictures."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from spec_amd import _lib, render
from tests import marks_ref as MR
from tests.test_gpu_render import SCENES
from tests.util import t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0xA5
STRIP, MASK, LINE = MR.STRIP, MR.MASK, MR.LINE


@pytest.fixture(scope='module')
def eng():
    from spec_amd import cam_utils
    return cam_utils._engine(torch.device(DEV))


def strip(y0, y1, c=(0, 0, 0)):
    return [STRIP, MR.pack_rgb(c), y0, y1, 0, 0, 0, 0]


def blend(x, y, mw, mh, off, c=(255, 255, 255)):
    return [MASK, MR.pack_rgb(c), x, y, mw, mh, off, 0]


def line(x0, y0, x1, y1, width, c=(0, 255, 0)):
    return [LINE, MR.pack_rgb(c), x0, y0, x1, y1, width, 0]


def _layout(frames, pitches=None, gaps=0):
    offsets, off = [], 0
    for k, fr in enumerate(frames):
        H, W = fr.shape[:2]
        p = 3 * W if pitches is None or pitches[k] is None else pitches[k]
        off += gaps
        offsets.append((off, p))
        off += (H - 1) * p + 3 * W
    return np.asarray(offsets, np.int64), off + gaps


def _fill(frames, offsets, nbytes):
    slab = np.full(nbytes, SENTINEL, np.uint8)
    for fr, (off, p) in zip(frames, offsets.tolist()):
        H, W = fr.shape[:2]
        for i in range(H):
            slab[off + i * p: off + i * p + 3 * W] = fr[i].reshape(-1)
    return slab


def _run(eng, frames, per_frame, masks=None, offsets=None, nbytes=None, pitches=None, gaps=0):
    """One draw_marks call: ``per_frame`` the mark lists of the frames -> (device result, reference) as host slabs."""
    if offsets is None:
        offsets, nbytes = _layout(frames, pitches, gaps)
    first = np.concatenate([[0], np.cumsum([len(m) for m in per_frame])]).tolist()
    marks = np.asarray([m for ms in per_frame for m in ms], np.int64).reshape(-1, MR.REC)
    geom = [(fr.shape[0], fr.shape[1], first[k], len(per_frame[k])) for k, fr in enumerate(frames)]
    dev = t(_fill(frames, offsets, nbytes)).to(DEV)
    mdev = None if masks is None else t(masks).to(DEV)
    eng.draw_marks(dev, geom, offsets, marks, mdev)
    want = _fill([MR.apply_marks(fr.copy(), np.asarray(ms, np.int64).reshape(-1, MR.REC), masks) for fr, ms in zip(frames, per_frame)], offsets, nbytes)
    return dev, want, (geom, offsets, marks, mdev)


def _frame(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


# ---- 1. one launch over five ragged frames -------------------------------------------------------------------------------------
def test_one_launch_over_five_ragged_frames(eng):
    rng = np.random.default_rng(41)
    sizes = [(1, 1), (3, 5), (30, 200), (31, 65), (64, 96)]
    frames = [_frame(rng, H, W) for H, W in sizes]
    masks = rng.integers(0, 256, 11 * 40 + 5, dtype=np.uint8)
    # back to back with gaps of 5 bytes; 31 x 65 at pitch 3 W + 7; 64 x 96 as the panel-0 column of a 9 W picture
    offsets, nbytes = _layout(frames[:4], [None, None, None, 3 * 65 + 7], gaps=5)
    pic = nbytes + 3
    offsets = np.concatenate([offsets, [[pic, 9 * 96]]])
    nbytes = pic + 64 * 9 * 96 + 9
    per = [[line(0, 0, 1, 0, 2), strip(0, 1, (9, 8, 7))],
           [strip(0, 2), line(0, 2, 5, 0, 3, (255, 0, 0))],
           [strip(0, 16), blend(0, 1, 40, 11, 5), line(0, 12, 200, 25, 5)],
           [],                                                                      # zero marks: untouched
           [strip(48, 64), blend(0, 49, 40, 11, 5), line(0, 40, 96, 55, 3, (0, 0, 255)), strip(0, 16), blend(0, 1, 40, 11, 0), line(0, 10, 96, 30, 3, (255, 0, 0))]]
    dev, want, call = _run(eng, frames, per, masks, offsets, nbytes)
    got = dev.cpu().numpy()
    assert np.array_equal(got, want)
    inside = np.zeros(nbytes, bool)
    for (H, W), (off, p) in zip(sizes, offsets.tolist()):
        for i in range(H):
            inside[off + i * p: off + i * p + 3 * W] = True
    assert (~inside).sum() > 64 * 6 * 96 and (got[~inside] == SENTINEL).all()        # padding, gaps, panels 1 and 2
    o3, p3 = offsets[3].tolist()
    assert all(np.array_equal(got[o3 + i * p3: o3 + i * p3 + 195], frames[3][i].reshape(-1)) for i in range(31))
    assert (got[inside] != _fill(frames, offsets, nbytes)[inside]).sum() > 3000      # the marks did draw
    eng.draw_marks(dev, *call)                                                        # the same records again: the same bytes
    assert np.array_equal(dev.cpu().numpy(), MR_twice(frames, per, masks, offsets, nbytes))


def MR_twice(frames, per, masks, offsets, nbytes):
    out = []
    for fr, ms in zip(frames, per):
        m = np.asarray(ms, np.int64).reshape(-1, MR.REC)
        out.append(MR.apply_marks(MR.apply_marks(fr.copy(), m, masks), m, masks))
    return _fill(out, offsets, nbytes)


# ---- 2. lines ------------------------------------------------------------------------------------------------------------------
LINES = [(5, 10, 70, 40), (-20, 30, 60, 35), (30, -15, 50, 20), (40, 20, 130, 44), (20, 40, 45, 80),      # inside; leaving at each side
         (-300, -200, -100, -50), (200, 10, 400, 30), (10, 100, 90, 300),                                   # wholly outside
         (0, 25, 97, 25), (-1000, 33, 1000, 33), (0, 30, 97, 31), (-100000, 20, 100000, 21), (3, 44, 94, 43),  # horizontal; one-row slope
         (48, -5, 49, 70), (50, 0, 50, 57), (47, 100000, 49, -100000),                                      # near-vertical, vertical
         (33, 21, 33, 21), (0, 0, 0, 0), (96, 56, 96, 56), (-1, 5, -1, 5)]                                   # zero length (the last two: outside)


@pytest.mark.parametrize('width', [2, 3, 5, 64])
def test_lines(eng, width):
    rng = np.random.default_rng(42)
    frames = [_frame(rng, 57, 97) for _ in LINES] + [_frame(rng, 57, 97)]
    per = [[line(*xy, width, (k, 255 - k, 7))] for k, xy in enumerate(LINES)]
    per.append([line(*xy, width, (k, 9, 255 - k)) for k, xy in enumerate(LINES)])     # all of them on one frame, in order
    dev, want, _ = _run(eng, frames, per, gaps=3)
    assert np.array_equal(dev.cpu().numpy(), want)
    base = _fill(frames, *_layout(frames, None, 3))
    assert (want != base).sum() > 2000


def test_lines_on_a_large_frame_and_a_one_pixel_frame(eng):
    """More than one tile per side, tiles skipped in between, the steepest legal slopes."""
    rng = np.random.default_rng(43)
    frames = [_frame(rng, 150, 333), _frame(rng, 1, 1), _frame(rng, 1, 130), _frame(rng, 130, 1)]
    per = [[line(0, 140, 333, 3, 5), line(-100000, -100000, 100000, 100000, 7, (1, 2, 3)), line(0, 75, 333, 75, 2, (255, 0, 0)), strip(16, 17, (4, 4, 4))],
           [line(-5, -5, 5, 5, 3)],
           [line(0, -3, 130, 2, 4), line(64, 0, 64, 0, 2, (9, 9, 9))],
           [line(-3, 0, 2, 130, 4), line(0, 64, 0, 64, 64, (9, 9, 9))]]
    dev, want, _ = _run(eng, frames, per)
    assert np.array_equal(dev.cpu().numpy(), want)


# ---- 3. masks ------------------------------------------------------------------------------------------------------------------
def test_masks(eng):
    rng = np.random.default_rng(44)
    mask = rng.integers(0, 256, (21, 70), dtype=np.uint8)
    mask[0, :6] = [0, 1, 127, 128, 254, 255]
    mask[5:9, 10:30] = 0                                                            # a hole: not written
    every = np.arange(256, dtype=np.uint8).reshape(4, 64)
    masks = np.concatenate([np.full(3, 77, np.uint8), mask.reshape(-1), every.reshape(-1)])
    o1 = 3 + mask.size
    ink = (200, 13, 77)
    frames = [_frame(rng, 40, 90) for _ in range(6)]
    for f in frames:
        f[:, :8] = rng.choice([0, 255], (40, 8, 3))                                 # the extremes of the background too
    per = [[blend(3, 5, 70, 21, 3, ink)],                                           # inside
           [blend(60, 30, 70, 21, 3, ink)],                                         # clipped right and bottom
           [blend(-13, -9, 70, 21, 3, ink)],                                        # a negative position
           [blend(0, 0, 64, 4, o1, ink), blend(1, 1, 64, 4, o1, (0, 255, 1)), blend(26, 36, 64, 4, o1, (255, 255, 255))],   # blends over blends
           [blend(90, 0, 70, 21, 3, ink), blend(0, 40, 70, 21, 3, ink), blend(-70, 0, 70, 21, 3, ink), blend(0, -21, 70, 21, 3, ink)],  # wholly outside
           [blend(-16383, -16383, 70, 21, 3, ink), blend(16383, 16383, 70, 21, 3, ink), blend(89, 39, 70, 21, 3, (1, 2, 3))]]
    dev, want, _ = _run(eng, frames, per, masks, gaps=2)
    got = dev.cpu().numpy()
    assert np.array_equal(got, want)
    offsets, nbytes = _layout(frames, None, 2)
    base = _fill(frames, offsets, nbytes)
    o4 = int(offsets[4, 0])
    assert np.array_equal(got[o4:o4 + 40 * 270], base[o4:o4 + 40 * 270]) and (got != base).sum() > 4000


# ---- 4. order ------------------------------------------------------------------------------------------------------------------
def test_painters_order(eng):
    rng = np.random.default_rng(45)
    img = _frame(rng, 100, 140)
    f = lambda v: 100 / 2 / np.tan(v / 2)
    gt = dict(vfov=1.0, pitch=0.1, roll=-0.05, focal_length=f(1.0), color=(0, 0, 255), width=3, debug=True, GT=True, text_size=16)
    pr = dict(vfov=0.8, pitch=0.12, roll=0.3, focal_length=f(0.8), color=(255, 0, 0), width=3, debug=True, GT=False, text_size=16)
    wants = []
    for order in ((gt, pr), (pr, gt)):                                              # ground truth then prediction, and the reverse
        want = img
        for kw in order:
            kw = dict(kw)
            want, _ = render.show_horizon_line(want, kw.pop('vfov'), kw.pop('pitch'), kw.pop('roll'), **kw)
        wants.append(want)
    slab = t(np.concatenate([img.reshape(-1), img.reshape(-1)])).to(DEV)
    fr = render.show_horizon_lines(slab, [(100, 140)] * 2, [0, 42000], [[gt, pr], [pr, gt]], engine=eng)
    got = slab.cpu().numpy()
    assert np.array_equal(got[:42000].reshape(100, 140, 3), wants[0]) and np.array_equal(got[42000:].reshape(100, 140, 3), wants[1])
    assert not np.array_equal(wants[0], wants[1]) and len(fr) == 2 and len(fr[0]) == 2
    # a strip over an earlier line, a line over text, text over a line
    text, (ox, oy) = render.caption_mask('GT: vfov:57.3')
    masks = text.reshape(-1).copy()
    mh, mw = text.shape
    frames = [_frame(rng, 40, 90) for _ in range(3)]
    per = [[line(0, 5, 90, 30, 5), strip(10, 20, (7, 7, 7))],
           [strip(0, 16), blend(ox, oy, mw, mh, 0), line(0, 2, 90, 12, 3, (255, 0, 0))],
           [line(0, 2, 90, 12, 3, (255, 0, 0)), blend(ox, oy, mw, mh, 0, (0, 255, 255))]]
    dev, want, _ = _run(eng, frames, per, masks)
    assert np.array_equal(dev.cpu().numpy(), want)
    assert not np.array_equal(want, _run(eng, frames, [p[::-1] for p in per], masks)[1])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_library(eng):
    frames = [np.full((8, 9, 3), 7, np.uint8), np.full((4, 4, 3), 7, np.uint8)]
    offsets, nbytes = _layout(frames, [30, None], 0)
    slab = torch.full((nbytes,), 7, dtype=torch.uint8, device=DEV)
    mask = torch.full((14,), 200, dtype=torch.uint8, device=DEV)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    marks = np.asarray([strip(0, 4, (1, 2, 3)), blend(1, 1, 4, 3, 2), line(0, 3, 9, 5, 3), line(0, 0, 4, 4, 2)], np.int64)
    good = dict(slab=p(slab), slab_bytes=nbytes, geom=np.array([[8, 9, 0, 3], [4, 4, 3, 1]], np.int32), offsets=offsets, n=2, marks=marks, nmarks=4,
                masks=p(mask), mask_bytes=14)

    def call(a):
        arr = lambda x, ty: None if x is None else np.ascontiguousarray(x).ctypes.data_as(ty)
        return eng.lib.specmi_draw_marks(eng.h, a['slab'], a['slab_bytes'], arr(a['geom'], _lib.c_int32_p), arr(a['offsets'], _lib.c_int64_p), a['n'],
                                         arr(a['marks'], _lib.c_int64_p), a['nmarks'], a['masks'], a['mask_bytes'], eng._stream())

    def with_(name, row, col, value):
        x = good[name].copy()
        x[row, col] = value
        return {name: x}

    bad = [dict(slab=None), dict(geom=None), dict(offsets=None), dict(marks=None), dict(masks=None),          # a null required pointer
           dict(n=0), dict(n=-1), dict(n=65536),                                                               # nframes outside [1, 65535]
           with_('geom', 0, 0, 0), with_('geom', 0, 1, 8193), with_('geom', 1, 0, -3), with_('geom', 1, 0, 8193),  # H or W outside [1, 8192]
           with_('offsets', 0, 1, 26), with_('offsets', 1, 1, 11),                                             # a pitch below 3 W
           dict(slab_bytes=nbytes - 1), with_('offsets', 0, 0, -1), with_('offsets', 1, 0, nbytes - 47),       # a rectangle that leaves the slab
           with_('offsets', 1, 0, 236), with_('offsets', 1, 0, 0),                                             # two frames share a byte
           with_('geom', 0, 2, -1), with_('geom', 1, 3, 2), with_('geom', 0, 3, -1), dict(nmarks=3), dict(nmarks=-1),  # a mark range outside the record
           with_('marks', 0, 0, 3), with_('marks', 3, 0, -1),                                                  # an unknown kind
           with_('marks', 2, 6, 1), with_('marks', 2, 6, 65), with_('marks', 3, 6, 0),                         # a width outside [2, 64]
           with_('marks', 2, 2, -100001), with_('marks', 2, 3, 100001), with_('marks', 3, 4, 1 << 40), with_('marks', 3, 5, -(1 << 40)),
           dict(mask_bytes=13), with_('marks', 1, 6, 3), with_('marks', 1, 6, -1),                             # a mask that leaves the buffer
           with_('marks', 1, 4, 0), with_('marks', 1, 5, 0), with_('marks', 1, 4, 8193), with_('marks', 1, 5, 8193),  # mw or mh outside [1, 8192]
           with_('marks', 1, 2, 16384), with_('marks', 1, 2, -16384), with_('marks', 1, 3, 16384), with_('marks', 1, 3, -16384)]
    for b in bad:
        assert call(dict(good, **b)) == _lib.ERR_ARG, {k: None for k in b}
        assert eng.lib.specmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert (slab == 7).all()                                                        # nothing was launched
    assert call(good) == _lib.OK
    want = _fill([MR.apply_marks(frames[0].copy(), marks[:3], np.full(14, 200, np.uint8)), MR.apply_marks(frames[1].copy(), marks[3:])], offsets, nbytes)
    want[want == SENTINEL] = 7
    assert np.array_equal(slab.cpu().numpy(), want)
    nomask = dict(with_('marks', 1, 0, STRIP), masks=None, mask_bytes=0)                # no mask blend among the marks: no buffer
    assert call(dict(good, **nomask)) == _lib.OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):                                                 # and the Python binding refuses before the library is reached
        eng.draw_marks(slab, good['geom'], offsets, with_('marks', 2, 6, 1)['marks'], mask)


def test_graph_capture_needs_the_records_of_the_previous_call(eng):
    rng = np.random.default_rng(46)
    frame = _frame(rng, 20, 70)
    marks = np.asarray([strip(0, 5), line(0, 3, 70, 15, 3)], np.int64)
    geom, offs = [[20, 70, 0, 2]], [[0, 210]]
    fresh = lambda: t(frame.reshape(-1).copy()).to(DEV)
    want = eng.draw_marks(fresh(), geom, offs, marks).clone()                       # also the warm-up call of the capture below
    assert np.array_equal(want.cpu().numpy().reshape(20, 70, 3), MR.apply_marks(frame.copy(), marks))
    slab = fresh()
    before = slab.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):
        try:                                                                        # new records: refused, and the capture goes on
            eng.draw_marks(slab, [[20, 70, 0, 1]], offs, marks[:1])
        except _lib.SpecmiError as e:
            err = e
        eng.draw_marks(slab, geom, offs, marks)                                     # the previous call's records: captured
    assert err is not None and err.code == _lib.ERR_STATE, err
    torch.cuda.synchronize()
    assert torch.equal(slab, before)                                                # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(slab, want)


# ---- 6. the flows --------------------------------------------------------------------------------------------------------------
def _scenes():
    a = dict(SCENES['two_spheres'], size=(96, 128))
    a['cam'] = a['cam'][:2] + (64.0, 48.0)
    c = dict(SCENES['icosphere_off_centre'], size=(40, 40))
    c['cam'] = c['cam'][:2] + (20.25, 18.75)
    return [a, c, SCENES['three_partly_outside_and_near']]


FRAMES = _scenes()
SIZES = [d['size'] for d in FRAMES]                                                 # (96, 128), (40, 40), (33, 47)
COUNTS = [d['v'].shape[0] for d in FRAMES]
FIRST = np.concatenate([[0], np.cumsum(COUNTS)]).tolist()
CAM_PARAMS = [(1.0, 0.1, -0.05, 40.0), (0.9, -0.2, 0.1, 80.0), None]                # 40 wide: narrower than the caption; one without a horizon


@pytest.fixture(scope='module')
def world(eng):
    rng = np.random.default_rng(47)
    frames = [_frame(rng, H, W) for H, W in SIZES]
    kp = np.concatenate([np.concatenate([rng.uniform(-4, W + 4, (n, 49, 1)), rng.uniform(-4, H + 4, (n, 49, 1)), rng.uniform(0.0, 1.0, (n, 49, 1))], axis=2)
                         for (H, W), n in zip(SIZES, COUNTS)]).astype(np.float32)
    return dict(eng=eng, frames=frames, kp=kp, v=t(np.concatenate([d['v'] for d in FRAMES])).to(DEV), t=t(np.concatenate([d['t'] for d in FRAMES])).to(DEV),
                f=FRAMES[0]['f'], R=[d['R'] for d in FRAMES], focal=[d['cam'][:2] for d in FRAMES], center=[d['cam'][2:] for d in FRAMES])


@pytest.mark.parametrize('with_kp', [False, True])
def test_render_image_group_routes_are_byte_identical(world, with_kp, tmp_path):
    w = world
    for f in range(3):
        m0, m1 = FIRST[f], FIRST[f + 1]
        kw = dict(faces=w['f'], keypoints_2d=w['kp'][m0:m1] if with_kp else None, cam_params=CAM_PARAMS[f], engine=w['eng'])
        args = (w['t'][m0:m1], w['v'][m0:m1], w['R'][f], w['focal'][f], w['center'][f])
        host = render.render_image_group(w['frames'][f], *args, panel0_device=False, **kw).cpu().numpy()
        dev = render.render_image_group(w['frames'][f], *args, panel0_device=True, **kw).cpu().numpy()
        assert np.array_equal(dev, host), f
        given = t(w['frames'][f]).to(DEV)                                            # a frame that lies on the device already
        keep = given.clone()
        assert np.array_equal(render.render_image_group(given, *args, panel0_device=True, **kw).cpu().numpy(), host), f
        assert torch.equal(given, keep)                                             # and is not drawn into
        if CAM_PARAMS[f] is not None:
            W = SIZES[f][1]
            assert (host[:, :W] != w['frames'][f]).any()
    flt = w['frames'][0].astype(np.float32) / 255.0                                 # a float frame takes the host route
    kw = dict(faces=w['f'], cam_params=CAM_PARAMS[0], engine=w['eng'])
    args = (w['t'][:2], w['v'][:2], w['R'][0], w['focal'][0], w['center'][0])
    assert torch.equal(render.render_image_group(flt, *args, panel0_device=True, **kw), render.render_image_group(flt, *args, panel0_device=False, **kw))
    a, b = str(tmp_path / 'a.jpg'), str(tmp_path / 'b.jpg')
    render.render_image_group(w['frames'][0], *args, panel0_device=True, save_filename=a, **kw)
    render.render_image_group(w['frames'][0], *args, panel0_device=False, save_filename=b, **kw)
    assert open(a, 'rb').read() == open(b, 'rb').read()


@pytest.mark.parametrize('with_kp', [False, True])
def test_render_image_groups_routes_are_byte_identical(world, with_kp):
    w = world
    flt = w['frames'][1].astype(np.float32) / 255.0
    frames = [t(w['frames'][0]).to(DEV), flt, w['frames'][2]]                        # a device tensor, a float frame (host route), a host frame
    args = (w['v'], w['t'], COUNTS, w['R'], w['focal'], w['center'])
    kw = dict(faces=w['f'], cam_params=CAM_PARAMS, engine=w['eng'], keypoints_2d=w['kp'] if with_kp else None)
    for extra in (dict(), dict(each=True), dict(encode='jpeg'), dict(pixel_budget=3 * (96 * 128 + 40 * 40))):
        host = render.render_image_groups([w['frames'][0], flt, w['frames'][2]], *args, panel0_device=False, **kw, **extra)
        dev = render.render_image_groups(frames, *args, panel0_device=True, **kw, **extra)
        assert len(dev) == len(host) == (6 if extra.get('each') else 3)
        for a, b in zip(dev, host):
            assert (a == b) if isinstance(a, bytes) else np.array_equal(a, b), extra
    one = render.render_image_group(w['frames'][0], w['t'][:2], w['v'][:2], w['R'][0], w['focal'][0], w['center'][0], faces=w['f'],
                                    keypoints_2d=w['kp'][:2] if with_kp else None, cam_params=CAM_PARAMS[0], engine=w['eng'], panel0_device=False)
    assert np.array_equal(render.render_image_groups(frames, *args, panel0_device=True, **kw)[0], one.cpu().numpy())


# ---- 7. denormalisation and CamCalib's validation pictures ---------------------------------------------------------------------
def test_denormalize_u8(eng):
    rng = np.random.default_rng(48)
    x = rng.normal(0, 1.2, (3, 3, 37, 70)).astype(np.float32)
    x[1, :, 0, :6] = np.array([np.nan, -np.inf, np.inf, -5.0, 50.0, 0.0], np.float32)
    xd = t(x).to(DEV)
    got = eng.denormalize_u8(xd, 1, 37, 70).cpu().numpy().reshape(37, 70, 3)
    assert np.array_equal(got, MR.denormalize_u8(x[1]))
    slab = torch.full((5 + 30 * 200,), SENTINEL, dtype=torch.uint8, device=DEV)
    eng.denormalize_u8(xd, 2, 30, 65, slab=slab, offset=5, pitch=200, mean=(0.5, 0.4, 0.3), std=(0.2, 0.3, 0.4))
    host = slab.cpu().numpy()
    want = MR.denormalize_u8(x[2][:, :30, :65], (0.5, 0.4, 0.3), (0.2, 0.3, 0.4))
    rows = host[5:].reshape(30, 200)
    assert np.array_equal(rows[:, :195].reshape(30, 65, 3), want) and (rows[:-1, 195:] == SENTINEL).all() and (host[:5] == SENTINEL).all()
    p = lambda v: C.c_void_p(v.data_ptr())
    for B, idx, H, W, off, pitch in ((3, 3, 30, 65, 5, 200), (3, -1, 30, 65, 5, 200), (3, 0, 38, 65, 5, 200), (3, 0, 30, 71, 5, 213), (3, 0, 30, 65, 5, 194),
                                     (3, 0, 30, 65, 11, 200), (3, 0, 0, 65, 5, 200), (0, 0, 30, 65, 5, 200)):
        assert eng.lib.specmi_denormalize_u8(eng.h, p(xd), B, 37, 70, idx, H, W, None, None, p(slab), slab.numel(), off, pitch, eng._stream()) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(slab.cpu().numpy(), host)


def test_camcalib_eval_saves_the_validation_pictures(tmp_path):
    from PIL import Image
    from spec_amd import camcalib_eval as ce
    root = str(tmp_path)
    ce.write_standin_tree(root, n_images=10, min_res=96, max_res=160, batch_size=2)
    hp = ce.load_config(os.path.join(root, ce.STANDIN_CFG))
    model = ce.build_model(hp, None, root, DEV)
    eng = model.engine(torch.device(DEV))
    plain = ce.run_evaluation(hp, root, model=model, log=lambda s: None)
    assert plain['pictures'] == [] and not os.path.exists(os.path.join(root, hp['LOG_DIR']))        # off unless the config or the caller says so
    lines = []
    res = ce.run_evaluation(hp, root, model=model, log=lines.append, save_images=True)
    out = os.path.join(root, hp['LOG_DIR'], 'val_output_images')
    assert sorted(os.listdir(out)) == ['result_0000000_00000.jpg', 'result_0000000_00004.jpg']
    assert res['pictures'] == [os.path.join(out, n) for n in sorted(os.listdir(out))] and sum(l.startswith('wrote ') for l in lines) == 2
    assert np.array_equal(res['logits'], plain['logits'])
    hp2 = ce.load_config(os.path.join(root, ce.STANDIN_CFG), ['TRAINING.SAVE_IMAGES', 'True'])       # the config's own switch, another folder
    res2 = ce.run_evaluation(hp2, root, model=model, log=lambda s: None, image_dir=str(tmp_path / 'pics'))
    assert sorted(os.listdir(str(tmp_path / 'pics'))) == sorted(os.listdir(out)) and len(res2['pictures']) == 2
    # batch 4 = images 8, 9: its first picture rebuilt on the host from the downloaded network input
    ds = ce.PanoValDataset(hp['DATASET']['VAL_DS'], root)
    images = ce.pad_batch([ds.frame(8), ds.frame(9)], 96, 160, DEV, eng).cpu().numpy()
    h, w = res['img_sizes'][8]
    img = MR.denormalize_u8(images[0])[:h, :w]
    gt = tuple(np.float32(res['gt_' + k][8]) for k in ('vfov', 'pitch', 'roll'))
    pred = tuple(res['pred_' + k][8] for k in ('vfov', 'pitch', 'roll'))
    img, _ = render.show_horizon_line(img, *gt, focal_length=h / 2. / np.tan(gt[0] / 2.), debug=True, color=(0, 0, 255), width=3, GT=True)
    img, _ = render.show_horizon_line(img, *pred, focal_length=h / 2. / np.tan(pred[0] / 2.), debug=True, color=(255, 0, 0), width=3, GT=False)
    ref = render.save_picture(str(tmp_path / 'ref.jpg'), t(img).to(DEV), engine=eng, jpeg_device=False)
    got = np.array(Image.open(os.path.join(out, 'result_0000000_00004.jpg')))
    assert got.shape == (h, w, 3) and np.array_equal(got, np.array(Image.open(ref)))
    assert open(ref, 'rb').read() == open(os.path.join(out, 'result_0000000_00004.jpg'), 'rb').read()
    assert (img[-16:] == 0).all(axis=2).mean() > 0.5 and (img[:16] == 0).all(axis=2).mean() > 0.5    # both caption strips are there
