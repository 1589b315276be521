"""specmi_draw_skeletons on MI355X: every assertion is an equality with tests/draw_ref.py (the drawing contract in NumPy, itself
pinned against exact rationals by tests/test_draw_skeleton_host.py) - single frames with bones of every kind and every
visibility case, painter's order, ragged slabs with padding and gaps, the extremes of the ranges, the table rule, every refusal
of the C ABI, and the three users: ``render_image_group(s)``, the demo flow and the evaluation flow."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

from spec_amd import _lib, constants, render
from tests import draw_ref
from tests.test_gpu_render import SCENES
from tests.util import gpu_models, synth_states, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def eng():
    from spec_amd import cam_utils
    return cam_utils._engine(torch.device(DEV))


def _style_kw(style):
    return dict(radius=style.radius, thickness=style.thickness, thr=style.conf_thr, joint_rgb=tuple(style.joint_rgb),
                bone_rgb=tuple(tuple(c) for c in style.bone_rgb))


def _layout(frames, pitches=None, gaps=0):
    """Frames at their pitches (None = 3 W), ``gaps`` bytes before each and after the last -> (offsets (n, 2), slab bytes)."""
    offsets, off = [], 0
    for k, fr in enumerate(frames):
        H, W = fr.shape[:2]
        p = 3 * W if pitches is None or pitches[k] is None else pitches[k]
        off += gaps
        offsets.append((off, p))
        off += (H - 1) * p + 3 * W
    return np.asarray(offsets, np.int64), off + gaps


def _fill(frames, offsets, nbytes):
    """The host slab: SENTINEL everywhere, the frames' pixels in their rectangles."""
    slab = np.full(nbytes, SENTINEL, np.uint8)
    for fr, (off, p) in zip(frames, offsets.tolist()):
        H, W = fr.shape[:2]
        for i in range(H):
            slab[off + i * p: off + i * p + 3 * W] = fr[i].reshape(-1)
    return slab


def _draw(eng, frames, kp, counts, bones, style=None, pitches=None, gaps=0, slab=None):
    """One draw_skeletons call over ``frames`` (host arrays) holding ``counts`` detections each -> the host slab after it."""
    offsets, nbytes = _layout(frames, pitches, gaps)
    first = np.concatenate([[0], np.cumsum(counts)])
    geom = [(fr.shape[0], fr.shape[1], int(first[k]), int(counts[k])) for k, fr in enumerate(frames)]
    dev = t(_fill(frames, offsets, nbytes)).to(DEV) if slab is None else slab
    eng.draw_skeletons(t(np.asarray(kp, np.float32)).to(DEV), dev, geom, offsets, bones=bones, style=style)
    return dev.cpu().numpy()


def _want(frames, kp, counts, bones, style=None, pitches=None, gaps=0):
    """The same slab by the reference: each frame drawn on its own, everything else SENTINEL."""
    style = style or _lib.DrawStyle()
    offsets, nbytes = _layout(frames, pitches, gaps)
    first = np.concatenate([[0], np.cumsum(counts)])
    drawn = [draw_ref.draw(fr, np.asarray(kp, np.float32)[first[k]:first[k + 1]], bones=bones, **_style_kw(style)) for k, fr in enumerate(frames)]
    return _fill(drawn, offsets, nbytes), drawn


def _frame(rng, H, W):
    return rng.integers(0, 200, (H, W, 3), dtype=np.uint8)       # below 255: no frame byte equals a full colour channel


# ---- 1. one frame, every kind of bone, every visibility case ------------------------------------------------------------------
NEXT = float(np.nextafter(np.float32(0.3), np.float32(1)))
BONES6 = [(0, 1), (1, 2), (0, 4), (4, 5), (2, 2), (0, 3), (5, 3)]      # horizontal, vertical, slope 1, shallow with an end left of 0,
#                                                                        zero length, an end beyond W, both ends off the frame
KP6 = np.array([
    [[5, 10, 1], [40, 10, 1], [40, 30, 1], [60.7, 5.5, 1], [25, 30, 1], [-8.5, 24.2, 1]],
    # confidence exactly 0.3f (invisible), the next float (visible), NaN, an infinite x
    [[8, 15, np.float32(0.3)], [43, 15, NEXT], [43, 35, np.nan], [np.inf, 10, 1], [28, 35, 1], [-5.5, 29.2, 1]],
    [[-0.5, -0.9, 1], [52.9, 36.9, 1], [53, 0, 1], [0, 37, 1], [20.5, 3.5, 0.31], [30, 33, 0.29]],       # truncation toward zero; the corners
], np.float32)


@pytest.mark.parametrize('D', [2, 3])
def test_one_frame_every_bone_kind_and_visibility_case(eng, D):
    rng = np.random.default_rng(21)
    frame = _frame(rng, 37, 53)
    kp = KP6[..., :D]
    got = _draw(eng, [frame], kp, [3], BONES6)
    want, (drawn,) = _want([frame], kp, [3], BONES6)
    assert np.array_equal(got, want)
    hit = draw_ref.covered(37, 53, kp, bones=BONES6)
    assert {0, 1, 2} <= set(np.unique(hit).tolist()) and (hit < 0).sum() > 500          # the case is not empty, nor the frame full
    vis = [draw_ref.visible(k)[0].tolist() for k in kp]
    assert vis[1] == ([True, True, True, False, True, True] if D == 2 else [False, True, False, False, True, True])
    assert vis[2][5] == (D == 2) and hit[0, 0] >= 0 and hit[36, 52] >= 0 and hit[2, 50] == 0       # the corners; the disc of a joint beyond W


# ---- 2. painter's order; more primitives than one chunk -----------------------------------------------------------------------
def test_painters_order_in_both_detection_orders(eng):
    rng = np.random.default_rng(22)
    frame = _frame(rng, 40, 44)
    bones = [(0, 1), (1, 2)]
    kp = np.array([[[6, 6], [30, 8], [34, 30]], [[30, 5], [8, 9], [30, 33]]], np.float32)
    style = _lib.DrawStyle(radius=3, thickness=5)
    out = {}
    for name, k in (('ab', kp), ('ba', kp[::-1].copy())):
        out[name] = _draw(eng, [frame], k, [2], bones, style)
        assert np.array_equal(out[name], _want([frame], k, [2], bones, style)[0]), name
    hit_ab, hit_ba = (draw_ref.covered(40, 44, k, bones=bones, radius=3, thickness=5) for k in (kp, kp[::-1]))
    assert np.array_equal(hit_ab >= 0, hit_ba >= 0) and (hit_ab != hit_ba).sum() > 10 and not np.array_equal(out['ab'], out['ba'])


def test_more_primitives_than_one_chunk(eng):
    rng = np.random.default_rng(23)
    frame = _frame(rng, 70, 90)                                       # 3 x 3 tiles, none whole
    kp = np.concatenate([rng.uniform(-10, 100, (8, 49, 1)), rng.uniform(-10, 80, (8, 49, 1)), rng.uniform(0.1, 1.0, (8, 49, 1))], axis=2).astype(np.float32)
    assert 8 * (49 + len(constants.SKELETON_SPIN)) > 2 * 256
    got = _draw(eng, [frame], kp, [8], None)                          # None: constants.SKELETON_SPIN
    assert np.array_equal(got, _want([frame], kp, [8], constants.SKELETON_SPIN)[0])
    got = _draw(eng, [frame], kp, [8], [])                            # no bones at all
    assert np.array_equal(got, _want([frame], kp, [8], [])[0])


# ---- 3. ragged slabs ----------------------------------------------------------------------------------------------------------
def test_ragged_frames_padding_gaps_and_the_untouched_frame(eng):
    rng = np.random.default_rng(24)
    frames = [_frame(rng, 1, 1), _frame(rng, 37, 53), _frame(rng, 64, 96)]
    counts, pitches = [1, 0, 3], [None, 3 * 53 + 11, None]
    kp = np.concatenate([np.array([[[0.2, 0.7, 1]] * 49], np.float32),
                         np.concatenate([rng.uniform(-5, 100, (3, 49, 1)), rng.uniform(-5, 70, (3, 49, 1)), rng.uniform(0.2, 1.0, (3, 49, 1))], axis=2)]).astype(np.float32)
    got = _draw(eng, frames, kp, counts, None, pitches=pitches, gaps=13)
    want, drawn = _want(frames, kp, counts, constants.SKELETON_SPIN, pitches=pitches, gaps=13)
    assert np.array_equal(got, want)                                  # padding, gaps and the count-0 frame included
    assert np.array_equal(drawn[1], frames[1]) and drawn[0].reshape(-1).tolist() == [0, 0, 255] and not np.array_equal(drawn[2], frames[2])
    # the three single-frame calls
    kpd = t(kp).to(DEV)
    for k, fr in enumerate(frames):
        single = t(fr.reshape(-1).copy()).to(DEV)
        eng.draw_skeletons(kpd, single, [(fr.shape[0], fr.shape[1], sum(counts[:k]), counts[k])], [(0, 3 * fr.shape[1])])
        assert np.array_equal(single.cpu().numpy().reshape(fr.shape), drawn[k]), k
    # a repeated call: the same records, the same bytes
    offsets, nbytes = _layout(frames, pitches, 13)
    slab = t(_fill(frames, offsets, nbytes)).to(DEV)
    a = _draw(eng, frames, kp, counts, None, pitches=pitches, gaps=13, slab=slab).copy()
    b = _draw(eng, frames, kp, counts, None, pitches=pitches, gaps=13, slab=slab)
    assert np.array_equal(a, want) and np.array_equal(b, want)


# ---- 4. the extremes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius,thickness', [(0, 1), (64, 64), (4, 64), (64, 1)])
def test_extreme_radius_and_thickness(eng, radius, thickness):
    rng = np.random.default_rng(25)
    style = _lib.DrawStyle(radius=radius, thickness=thickness)
    bones = [(0, 1), (2, 3)]
    for H, W, kp in ((8, 8, [[[2, 3], [6, 5], [70, 4], [4, 75]]]), (50, 45, [[[10, 12], [38, 30], [100, 20], [20, 110]]])):
        frame = _frame(rng, H, W)
        got = _draw(eng, [frame], np.asarray(kp, np.float32), [1], bones, style)
        want, (drawn,) = _want([frame], np.asarray(kp, np.float32), [1], bones, style)
        assert np.array_equal(got, want), (H, W)
        if radius == 64 and H == 8:
            assert (drawn != frame).any(axis=2).all()                 # the whole 8 x 8 frame lies inside the discs
        if radius == 0 and H == 50:
            assert (draw_ref.covered(H, W, kp, bones=[], radius=0) >= 0).sum() == 2


def test_coordinate_range_ends(eng):
    rng = np.random.default_rng(26)
    frame = _frame(rng, 8, 8)
    lim = float(draw_ref.MAX_COORD)
    inside = np.array([[[lim + 0.9, 5], [-lim - 0.9, 5], [-lim, -lim], [lim, lim]]], np.float32)         # int-cast: +-16383
    outside = np.array([[[lim + 1, 5], [-lim - 1, 5], [-lim - 1, -lim], [lim, lim + 1]]], np.float32)     # +-16384: dropped
    bones = [(0, 1), (2, 3)]
    got = _draw(eng, [frame], inside, [1], bones)
    want, (drawn,) = _want([frame], inside, [1], bones)
    assert np.array_equal(got, want)
    assert (drawn[5, 0] == (0, 0, 255)).all() and (drawn[3, 3] == (255, 0, 0)).all()      # both bones reach the frame from +-16383
    got = _draw(eng, [frame], outside, [1], bones)
    assert np.array_equal(got.reshape(frame.shape), frame) and np.array_equal(_want([frame], outside, [1], bones)[1][0], frame)


@pytest.mark.parametrize('H,W', [(1, _lib.DRAW_MAX_SIDE), (_lib.DRAW_MAX_SIDE, 1)])
def test_strip_at_the_side_limit(eng, H, W):
    rng = np.random.default_rng(27)
    frame = _frame(rng, H, W)
    far, lim = _lib.DRAW_MAX_SIDE - 1, draw_ref.MAX_COORD
    kp = np.array([[[far, 0] if H == 1 else [0, far], [far - 40, 30] if H == 1 else [30, far - 40], [-lim, -lim], [lim, lim - 3], [4000, 0] if H == 1 else [0, 4000],
                    [-lim, lim], [lim, -lim]]], np.float32)
    bones = [(0, 1), (2, 3), (4, 4), (5, 6), (0, 4)]
    style = _lib.DrawStyle(radius=7, thickness=9)
    got = _draw(eng, [frame], kp, [1], bones, style)
    want, (drawn,) = _want([frame], kp, [1], bones, style)
    assert np.array_equal(got, want)
    assert (drawn[H - 1, W - 1] != frame[H - 1, W - 1]).any() and (drawn[0, 0] != frame[0, 0]).any()      # the last pixel and the diagonal through the origin


# ---- 5. refusals and the table rule -------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_library(eng):
    rng = np.random.default_rng(28)
    frames = [_frame(rng, 8, 9), _frame(rng, 4, 4)]
    offsets, nbytes = _layout(frames, [30, None], 0)
    assert nbytes == 7 * 30 + 27 + 48
    slab = torch.full((nbytes,), 7, dtype=torch.uint8, device=DEV)
    kp = t(rng.uniform(0, 8, (3, 6, 3)).astype(np.float32)).to(DEV)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    good = dict(kp=p(kp), Mtot=3, J=6, D=3, bones=np.array([(0, 1), (4, 5)], np.int32), NB=2, style=_lib.DrawStyle(), slab=p(slab), slab_bytes=nbytes,
                geom=np.array([[8, 9, 0, 2], [4, 4, 2, 1]], np.int32), offsets=offsets, n=2)

    def call(a):
        arr = lambda x, ty: None if x is None else np.ascontiguousarray(x).ctypes.data_as(ty)
        return eng.lib.specmi_draw_skeletons(eng.h, a['kp'], a['Mtot'], a['J'], a['D'], arr(a['bones'], _lib.c_int32_p), a['NB'],
                                             None if a['style'] is None else C.byref(a['style']), a['slab'], a['slab_bytes'],
                                             arr(a['geom'], _lib.c_int32_p), arr(a['offsets'], _lib.c_int64_p), a['n'], eng._stream())

    def with_(name, row, col, value):
        x = good[name].copy()
        x[row, col] = value
        return {name: x}

    bad = [dict(kp=None), dict(slab=None), dict(geom=None), dict(offsets=None),                                  # a null required pointer
           dict(n=0), dict(n=-1), dict(n=65536),                                                                # nframes outside [1, 65535]
           dict(J=0), dict(D=1), dict(D=4),                                                                     # J < 1, D not 2 or 3
           dict(NB=-1), dict(bones=None),                                                                       # NB < 0, NB > 0 with null bones
           with_('bones', 1, 1, 6), with_('bones', 0, 0, -1),                                                   # a bone index outside [0, J)
           dict(style=_lib.DrawStyle(radius=-1)), dict(style=_lib.DrawStyle(radius=65)), dict(style=_lib.DrawStyle(thickness=0)),
           dict(style=_lib.DrawStyle(thickness=65)),
           with_('geom', 0, 0, 0), with_('geom', 0, 1, _lib.DRAW_MAX_SIDE + 1), with_('geom', 1, 0, -3), with_('geom', 1, 0, _lib.DRAW_MAX_SIDE + 1),
           with_('geom', 0, 2, -1), with_('geom', 1, 3, 2), with_('geom', 0, 3, -1), dict(Mtot=2),             # a detection range outside [0, Mtot]
           with_('offsets', 0, 1, 26), with_('offsets', 1, 1, 11),                                              # a pitch below 3 W
           dict(slab_bytes=nbytes - 1), with_('offsets', 0, 0, -1), with_('offsets', 1, 0, nbytes - 47),        # a rectangle that leaves the slab
           with_('offsets', 1, 0, 236), with_('offsets', 1, 0, 0), dict(with_('offsets', 1, 0, 26), **with_('geom', 1, 1, 2)),   # two frames share a byte
           dict(style=_lib.DrawStyle(conf_thr=float('nan'))), dict(style=_lib.DrawStyle(conf_thr=float('inf')))]              # a non-finite thr
    for b in bad:
        assert call(dict(good, **b)) == _lib.ERR_ARG, {k: None for k in b}
        assert eng.lib.specmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert (slab == 7).all()                                                  # nothing was launched
    # what is legal: the defaults for a NULL style, no bones, a frame in the other's row padding, a 2160 x 3840 frame
    assert call(dict(good, style=None)) == _lib.OK
    kph = kp.cpu().numpy()
    host = [np.full((8, 9, 3), 7, np.uint8), np.full((4, 4, 3), 7, np.uint8)]
    want = _fill([draw_ref.draw(host[0], kph[:2], bones=good['bones'].tolist()), draw_ref.draw(host[1], kph[2:], bones=good['bones'].tolist())],
                 offsets, nbytes)
    want[want == SENTINEL] = 7
    assert np.array_equal(slab.cpu().numpy(), want)
    assert call(dict(good, NB=0, bones=None)) == _lib.OK
    assert call(dict(good, offsets=np.array([[0, 30], [27, 30]], np.int64), **with_('geom', 1, 1, 1))) == _lib.OK      # a column in the other's row padding
    big = torch.zeros(2160 * 3840 * 3, dtype=torch.uint8, device=DEV)
    assert call(dict(good, slab=p(big), slab_bytes=big.numel(), geom=np.array([[2160, 3840, 0, 3]], np.int32), offsets=np.array([[0, 3 * 3840]], np.int64), n=1)) == _lib.OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):       # and the Python binding refuses before the library is reached
        eng.draw_skeletons(kp, slab, good['geom'], with_('offsets', 1, 1, 11)['offsets'], bones=good['bones'])


def test_graph_capture_needs_the_records_of_the_previous_call(eng):
    rng = np.random.default_rng(29)
    frames = [_frame(rng, 20, 30), _frame(rng, 33, 17)]
    kp = np.concatenate([rng.uniform(0, 30, (3, 49, 2))], axis=2).astype(np.float32)
    offsets, nbytes = _layout(frames)
    geom = [(20, 30, 0, 2), (33, 17, 2, 1)]
    fresh = lambda: t(_fill(frames, offsets, nbytes)).to(DEV)
    kpd, slab = t(kp).to(DEV), fresh()
    want = eng.draw_skeletons(kpd, fresh(), geom, offsets).clone()            # also the warm-up call of the capture below
    assert np.array_equal(want.cpu().numpy(), _want(frames, kp, [2, 1], constants.SKELETON_SPIN)[0])
    before = slab.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):
        try:      # new records: refused, and the capture goes on
            eng.draw_skeletons(kpd, slab, geom[:1], offsets[:1])
        except _lib.SpecmiError as e:
            err = e
        eng.draw_skeletons(kpd, slab, geom, offsets)                          # the previous call's records: captured
    assert err is not None and err.code == _lib.ERR_STATE, err
    torch.cuda.synchronize()
    assert torch.equal(slab, before)                                          # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(slab, want)
    other = eng.draw_skeletons(kpd, fresh(), geom[:1], offsets[:1])           # eagerly the other records are fine
    assert torch.equal(other[:1800], want[:1800]) and torch.equal(other[1800:], before[1800:])


# ---- 6. render_image_group and render_image_groups ----------------------------------------------------------------------------
def _scenes():
    c = dict(SCENES['icosphere_off_centre'], size=(40, 40))
    c['cam'] = c['cam'][:2] + (20.25, 18.75)
    return [SCENES['two_spheres'], c, SCENES['three_partly_outside_and_near']]


FRAMES = _scenes()
SIZES = [d['size'] for d in FRAMES]                                   # (64, 96), (40, 40), (33, 47)
COUNTS = [d['v'].shape[0] for d in FRAMES]
FIRST = np.concatenate([[0], np.cumsum(COUNTS)]).tolist()
CAM_PARAMS = [(1.0, 0.1, -0.05, 40.0), (0.9, -0.2, 0.1, 80.0), (1.1, 0.0, 0.0, 70.0)]


@pytest.fixture(scope='module')
def world(eng):
    assert COUNTS == [2, 1, 3]
    rng = np.random.default_rng(31)
    frames = [_frame(rng, H, W) for H, W in SIZES]
    kp = np.concatenate([np.concatenate([rng.uniform(-4, W + 4, (n, 49, 1)), rng.uniform(-4, H + 4, (n, 49, 1)), rng.uniform(0.0, 1.0, (n, 49, 1))], axis=2)
                         for (H, W), n in zip(SIZES, COUNTS)]).astype(np.float32)
    w = dict(eng=eng, frames=frames, kp=kp, v=t(np.concatenate([d['v'] for d in FRAMES])).to(DEV), t=t(np.concatenate([d['t'] for d in FRAMES])).to(DEV),
             f=FRAMES[0]['f'], R=[d['R'] for d in FRAMES], focal=[d['cam'][:2] for d in FRAMES], center=[d['cam'][2:] for d in FRAMES])
    # the per-frame route, and per single detection: {(frame, detection or None): (H, 3W, 3) uint8 host array}
    groups = {}
    for f in range(3):
        for i in [None] + list(range(COUNTS[f])):
            m0, m1 = (FIRST[f], FIRST[f + 1]) if i is None else (FIRST[f] + i, FIRST[f] + i + 1)
            groups[f, i] = render.render_image_group(frames[f], w['t'][m0:m1], w['v'][m0:m1], w['R'][f], w['focal'][f], w['center'][f], faces=w['f'],
                                                     keypoints_2d=kp[m0:m1], cam_params=CAM_PARAMS[f], engine=eng).cpu().numpy()
    w['groups'] = groups
    return w


def test_render_image_group_draws_the_skeleton_onto_panel_0(world):
    eng = world['eng']
    for f in range(3):
        H, W = SIZES[f]
        m0, m1 = FIRST[f], FIRST[f + 1]
        panel0 = render.group_panel0(world['frames'][f], CAM_PARAMS[f])       # the host-made panel 0: the horizon line and its caption
        drawn = draw_ref.draw(panel0, world['kp'][m0:m1])
        assert np.array_equal(render.draw_skeleton(panel0, world['kp'][m0:m1], unnormalize=False, engine=eng), drawn)
        assert (drawn != panel0).any(axis=2).sum() > 50
        want = render.render_image_group(drawn, world['t'][m0:m1], world['v'][m0:m1], world['R'][f], world['focal'][f], world['center'][f],
                                         faces=world['f'], engine=eng).cpu().numpy()                      # today's call on the drawn panel
        assert np.array_equal(world['groups'][f, None], want), f
        assert np.array_equal(want[:, :W], drawn)
    # one skeleton (J, D), a device image drawn in place, [-1, 1] keypoints of a res x res crop, alpha accepted and ignored
    img = t(world['frames'][0]).to(DEV)
    one = world['kp'][0]
    norm = np.concatenate([one[:, :2] / 32.0 - 1.0, one[:, 2:]], axis=1)
    back = np.concatenate([(norm[:, :2] + np.float32(1.0)) * np.float32(64.0) / np.float32(2.0), one[:, 2:]], axis=1)
    out = render.draw_skeleton(img, norm, res=64, thickness=3, engine=eng)
    assert out is img and np.array_equal(img.cpu().numpy(), draw_ref.draw(world['frames'][0], back[None], thickness=3))
    with pytest.raises(ValueError):
        render.draw_skeleton(img, one, dataset='coco')
    a = render.render_image_group(world['frames'][1], world['t'][2:3], world['v'][2:3], world['R'][1], world['focal'][1], world['center'][1], 'pinkish', 0.5,
                                  world['f'], None, None, world['kp'][2], CAM_PARAMS[1], engine=eng).cpu().numpy()
    assert np.array_equal(a, world['groups'][1, None])


@pytest.mark.parametrize('budget', [None, 3 * (64 * 96 + 40 * 40)])
def test_render_image_groups_equals_the_per_frame_calls(world, budget):
    kw = dict(faces=world['f'], cam_params=CAM_PARAMS, engine=world['eng'], pixel_budget=budget)
    assert len(render.plan_views(SIZES, COUNTS, pixel_budget=budget)) == (1 if budget is None else 2)
    args = (world['frames'], world['v'], world['t'], COUNTS, world['R'], world['focal'], world['center'])
    kpd = t(world['kp']).to(DEV)
    got = render.render_image_groups(*args, keypoints_2d=kpd, **kw)
    assert len(got) == 3
    for f in range(3):
        assert np.array_equal(got[f], world['groups'][f, None]), f
    each = render.render_image_groups(*args, keypoints_2d=world['kp'], each=True, **kw)
    keys = [(f, i) for f in range(3) for i in range(COUNTS[f])]
    assert len(each) == 6
    for k, pic in zip(keys, each):
        assert np.array_equal(pic, world['groups'][k]), k
    assert not np.array_equal(world['groups'][0, 0][:, :96], world['groups'][0, 1][:, :96])          # each detection's own skeleton on panel 0
    plain = render.render_image_groups(*args, **kw)
    assert not np.array_equal(plain[0], got[0]) and np.array_equal(plain[0][:, 2 * 96:], got[0][:, 2 * 96:])      # the side view does not show it


# ---- 7. the demo flow ---------------------------------------------------------------------------------------------------------
def test_demo_flow_draws_the_predicted_joints(tmp_path):
    import joblib
    from types import SimpleNamespace
    from PIL import Image
    from spec_amd import evaluation
    from spec_amd.tester import SPECTester
    tree = str(tmp_path / 'tree')
    evaluation.write_standin_data_tree(tree, n_images=1)
    folder = str(tmp_path / 'frames')
    os.makedirs(folder)
    rng = np.random.default_rng(5)
    sizes, counts = [(96, 128), (120, 90), (110, 140)], [2, 1, 1]
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 200, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, f'frame{k}.png'))
    dets = [np.stack([rng.uniform(0.3 * w, 0.7 * w, n), rng.uniform(0.3 * h, 0.7 * h, n), rng.uniform(40, 80, n), rng.uniform(40, 80, n)], 1)
            .astype(np.float32) for (h, w), n in zip(sizes, counts)]
    hs = {k_: t(v) for k_, v in synth_states(True)[1].items()}
    args = SimpleNamespace(cfg=None, ckpt=hs, no_save=False, no_render=False, save_obj=False, synthetic_assets=True, frame_batch=4, plan='throughput',
                           decode_threads=2, camcalib_model=gpu_models(True, True, DEV)[0], detections=dets, render_each=False)
    cwd = os.getcwd()
    os.chdir(tree)
    try:
        te = SPECTester(args)
        runs = {}
        # (draw_keypoints: None = the attribute is absent, batched route, each)
        for flag, batch, each in ((None, False, False), (False, False, False), (True, False, False), (True, True, False), (True, True, True), (False, True, True)):
            out = str(tmp_path / f'out_{flag}_{int(batch)}{int(each)}')
            if runs:
                shutil.copytree(str(tmp_path / 'out_None_00' / 'camcalib'), os.path.join(out, 'camcalib'))
            else:
                te.run_camcalib(folder, out)
            if flag is None:
                assert not hasattr(args, 'draw_keypoints')
            else:
                args.draw_keypoints = flag
            te._render_batch, args.render_each = batch, each
            assert te.run_on_image_folder(folder, te.run_detector(folder), out, os.path.join(out, 'pictures')) == 3
            pics = {f: np.array(Image.open(os.path.join(out, 'pictures', f))) for f in sorted(os.listdir(os.path.join(out, 'pictures')))}
            raw = {f: open(os.path.join(out, 'pictures', f), 'rb').read() for f in sorted(os.listdir(os.path.join(out, 'pictures')))}
            res = {f: joblib.load(os.path.join(out, 'spec_results', f)) for f in sorted(os.listdir(os.path.join(out, 'spec_results')))}
            runs[flag, batch, each] = (pics, raw, res)
    finally:
        os.chdir(cwd)
    pics0, raw0, res0 = runs[None, False, False]
    assert sorted(pics0) == sorted(f'frame{k}_{i:06d}.png' for k, n in enumerate(counts) for i in range(n))
    assert runs[False, False, False][1] == raw0                               # the switch off: the files byte for byte
    for key, (pics, raw, res) in runs.items():
        assert sorted(pics) == sorted(pics0), key
        for f in res0:
            for k_, val in res0[f].items():
                assert res[f][k_].tobytes() == val.tobytes(), (key, f, k_)      # the result files do not change
    flagged = runs[True, False, False][0]
    assert runs[True, True, False][1] == runs[True, False, False][1]          # both routes: the same files
    each, each_plain = runs[True, True, True][0], runs[False, True, True][0]
    for k, n in enumerate(counts):
        (H, W), joints = sizes[k], res0[f'frame{k}.pkl']['smpl_joints2d']
        assert joints.shape == (n, 49, 2) and joints.dtype == np.float32
        hit = draw_ref.covered(H, W, joints)
        assert (hit >= 0).sum() > 20, k                                       # the predicted joints reach the frame
        for i in range(n):
            name = f'frame{k}_{i:06d}.png'
            a, b = pics0[name], flagged[name]
            assert np.array_equal(b[:, :W], draw_ref.draw(a[:, :W], joints))                     # panel 0: exactly the reference's pixels
            assert ((a[:, :W] != b[:, :W]).any(axis=2) <= (hit >= 0)).all()
            assert np.array_equal(b[:, W:2 * W][hit < 0], a[:, W:2 * W][hit < 0])                # the overlay: nothing else moved
            assert np.array_equal(b[:, 2 * W:], a[:, 2 * W:])                                    # the side view: unchanged
            own = draw_ref.covered(H, W, joints[i:i + 1])
            assert np.array_equal(each[name][:, :W], draw_ref.draw(each_plain[name][:, :W], joints[i:i + 1]))        # its own skeleton alone
            assert np.array_equal(each[name][:, W:2 * W][own < 0], each_plain[name][:, W:2 * W][own < 0])


# ---- 8. the evaluation flow ---------------------------------------------------------------------------------------------------
def test_run_evaluation_saves_pictures_with_the_ground_truth_keypoints(tmp_path):
    from PIL import Image
    from spec_amd import assets, evaluation
    d = str(tmp_path)
    truth = evaluation.write_standin_data_tree(d, n_images=6, keypoints=True)
    ann = truth['annotations']
    assert ann['openpose'].shape == (6, 25, 3) and ann['part'].shape == (6, 24, 3)
    cfg = os.path.join(d, 'data/spec/checkpoints/spec_config.yaml')
    base = ['DATASET.BATCH_SIZE', '2', 'TESTING.SAVE_FREQ', '2']
    out_dir = os.path.join(d, 'logs/eval_standin/output_images')
    try:
        plain = evaluation.run_evaluation(evaluation.load_config(cfg, base), data_root=d, log=lambda s: None)['spec-syn']
        assert not os.path.exists(out_dir)
        alone = evaluation.run_evaluation(evaluation.load_config(cfg, base + ['TESTING.SAVE_IMAGES', 'True']), data_root=d, log=lambda s: None)['spec-syn']
        assert not os.path.exists(out_dir) or os.listdir(out_dir) == []      # TESTING.SAVE_IMAGES alone writes no file
        lines = []
        both = evaluation.run_evaluation(evaluation.load_config(cfg, base + ['TESTING.SAVE_IMAGES', 'True', 'TRAINING.SAVE_IMAGES', 'True']), data_root=d,
                                         log=lines.append)['spec-syn']
    finally:
        assets.use_synthetic_assets(1003)
    assert sorted(os.listdir(out_dir)) == ['0000_00_00000_00_frame_0000.png', '0000_00_00002_00_frame_0004.png']
    for res in (alone, both):
        assert res['mean'] == plain['mean']                                   # the errors do not change
    H, W = truth['frame_hw']
    for name, i in (('0000_00_00000_00_frame_0000.png', 0), ('0000_00_00002_00_frame_0004.png', 4)):
        pic = np.array(Image.open(os.path.join(out_dir, name)))
        assert pic.shape == (H, 3 * W, 3)
        image = np.array(Image.open(os.path.join(d, 'data/dataset_folders/spec-syn', str(ann['imgname'][i]))).convert('RGB'))
        cam_params = np.array([float(ann[k][i]) for k in ('camcalib_vfov', 'camcalib_pitch', 'camcalib_roll', 'camcalib_f_pix')])
        kp = np.concatenate([ann['openpose'][i], ann['part'][i]])[None].astype(np.float32)
        panel0 = render.group_panel0(image, cam_params)
        want = draw_ref.draw(panel0, kp)
        assert np.array_equal(pic[:, :W], want), name
        assert (want != panel0).any(axis=2).sum() > 100 and not draw_ref.visible(kp[0])[0].all()
    assert sum('output_images' in l for l in lines) == 2
