"""The skeleton drawing without a GPU: tests/draw_ref.py (the integer formula every GPU test compares with) against an
independent brute-force definition of the same contract in exact rationals; the declared bone table; the drop-in signatures;
the C header."""
import importlib.util
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from spec_amd import constants
from tests import draw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the contract by brute force: squared distance from a pixel to the closed segment as a Fraction ---------------------------
def _dist2(p, a, b) -> Fraction:
    ax, ay, bx, by = (Fraction(int(v)) for v in (*a, *b))
    px, py = Fraction(p[0]), Fraction(p[1])
    dx, dy = bx - ax, by - ay
    L = dx * dx + dy * dy
    u = Fraction(0) if L == 0 else min(Fraction(1), max(Fraction(0), ((px - ax) * dx + (py - ay) * dy) / L))
    qx, qy = ax + u * dx, ay + u * dy
    return (px - qx) ** 2 + (py - qy) ** 2


def _brute_bone(H, W, a, b, t):
    return np.array([[_dist2((x, y), a, b) <= Fraction(t * t, 4) for x in range(W)] for y in range(H)])


def _brute_disc(H, W, c, r):
    return np.array([[(x - int(c[0])) ** 2 + (y - int(c[1])) ** 2 <= r * r for x in range(W)] for y in range(H)])


BONES = {'horizontal': ((3, 7), (19, 7)), 'vertical': ((11, 2), (11, 20)), 'slope_1': ((4, 4), (18, 18)), 'slope_minus_1': ((20, 3), (5, 18)),
         'shallow': ((2, 9), (22, 13)), 'steep': ((9, 1), (13, 22)), 'zero_length': ((12, 12), (12, 12)), 'reversed': ((19, 7), (3, 7)),
         'ends_off_frame': ((-9, 5), (31, 17)), 'wholly_off_frame': ((-30, -4), (-5, -20)), 'one_end_far': ((10, 10), (400, -250))}


@pytest.mark.parametrize('name', sorted(BONES))
@pytest.mark.parametrize('t', [1, 2, 3, 5])
def test_bone_formula_equals_the_exact_distance(name, t):
    a, b = BONES[name]
    for H, W in ((24, 24), (17, 23)):
        got = draw_ref.segment_mask(H, W, a, b, t * t)
        assert got.dtype == bool and np.array_equal(got, _brute_bone(H, W, a, b, t)), (name, t, H, W)
    if name in ('horizontal', 'slope_1', 'zero_length'):      # the cases are not empty
        assert draw_ref.segment_mask(24, 24, a, b, t * t).sum() >= 1


@pytest.mark.parametrize('r', [0, 1, 4])
def test_disc_formula(r):
    for c in ((12, 12), (0, 0), (23, 5), (-2, 10), (30, 30)):
        got = draw_ref.segment_mask(24, 24, c, c, 4 * r * r)
        assert np.array_equal(got, _brute_disc(24, 24, c, r)), (c, r)
    assert draw_ref.segment_mask(24, 24, (12, 12), (12, 12), 4 * r * r).sum() == {0: 1, 1: 5, 4: 49}[r]


def test_visibility_rule():
    nxt = np.nextafter(np.float32(0.3), np.float32(1))
    kp = np.array([[5.9, 7.2, 1.0], [-0.9, -0.9, 1.0], [5, 5, 0.3], [5, 5, nxt], [5, 5, np.nan], [np.inf, 5, 1], [5, np.nan, 1],
                   [16383.9, -16383.9, 1], [16384, 0, 1], [0, -16384, 1], [3e30, 0, 1]], np.float32)
    vis, xi, yi = draw_ref.visible(kp)
    assert vis.tolist() == [True, True, False, True, False, False, False, True, False, False, False]
    assert (xi[0], yi[0]) == (5, 7) and (xi[1], yi[1]) == (0, 0) and (xi[7], yi[7]) == (16383, -16383)      # truncation toward zero
    assert draw_ref.visible(kp[:, :2])[0].tolist() == [True, True, True, True, True, False, False, True, False, False, False]


def test_painters_order_and_colours():
    # two detections of three joints and the one bone (0, 1); joint 2 of the second lies on the first one's bone
    kp = np.array([[[4, 4], [12, 4], [1, 10]], [[3, 9], [9, 9], [8, 4]]], np.float32)
    kw = dict(bones=[(0, 1)], radius=1, thickness=3)
    hit = draw_ref.covered(12, 16, kp, **kw)
    assert hit[4, 4] == 1                      # a detection's bones lie over its own discs
    assert hit[4, 8] == 0 and hit[3, 8] == 0   # the later detection's disc lies over the earlier one's bone
    assert hit[4, 6] == 1 and hit[10, 1] == 0 and hit[0, 15] == -1
    back = draw_ref.covered(12, 16, kp[::-1], **kw)
    assert back[4, 8] == 1 and back[3, 8] == 1 and np.array_equal(back >= 0, hit >= 0) and not np.array_equal(back, hit)
    odd = draw_ref.covered(12, 16, kp[:1], bones=[(2, 2), (0, 1)], radius=0, thickness=1)
    assert odd[4, 8] == 2 and odd[10, 1] == 1                                  # bone 1 takes the odd colour, bone 0 the even one
    img = draw_ref.draw(np.full((12, 16, 3), 9, np.uint8), kp[:1], bones=[(2, 2), (0, 1)], radius=0, thickness=1)
    assert img[4, 8].tolist() == [255, 0, 0] and img[10, 1].tolist() == [0, 0, 255] and img[0, 0].tolist() == [9, 9, 9]


def test_skeleton_spin_is_a_valid_table():
    sk = constants.SKELETON_SPIN
    assert len(sk) == 25 and len(constants.JOINT_NAMES49) == 49
    assert all(len(b) == 2 and 0 <= b[0] < 49 and 0 <= b[1] < 49 and b[0] != b[1] for b in sk)
    assert len({tuple(sorted(b)) for b in sk}) == len(sk)                      # no bone twice, in either direction


def test_render_image_group_takes_the_reference_argument_list():
    from spec.utils import renderer_cam
    from spec_amd import render
    want = ['image', 'camera_translation', 'vertices', 'camera_rotation', 'focal_length', 'camera_center', 'mesh_color', 'alpha', 'faces',
            'mesh_filename', 'save_filename', 'keypoints_2d', 'cam_params']
    for fn in (render.render_image_group, renderer_cam.render_image_group):
        params = inspect.signature(fn).parameters
        assert list(params)[:len(want)] == want
        assert params['alpha'].default == 1.0 and params['keypoints_2d'].default is None
    assert 'keypoints_2d' in inspect.signature(render.render_image_groups).parameters
    sig = inspect.signature(render.draw_skeleton).parameters
    assert list(sig)[:6] == ['image', 'kp_2d', 'dataset', 'unnormalize', 'thickness', 'res']
    assert (sig['dataset'].default, sig['unnormalize'].default, sig['thickness'].default, sig['res'].default) == ('spin', True, 2, 224)


def test_demo_parser_accepts_draw_keypoints():
    spec = importlib.util.spec_from_file_location('spec_demo_script', os.path.join(ROOT, 'scripts', 'spec_demo.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    assert parser.parse_args(['--draw_keypoints']).draw_keypoints is True
    assert parser.parse_args([]).draw_keypoints is False


def test_plan_views_frame_per_picture():
    from spec_amd import render
    sizes, counts = [(4, 5), (3, 2)], [2, 1]
    (a,) = render.plan_views(sizes, counts, each=True)
    (b,) = render.plan_views(sizes, counts, each=True, frame_per_picture=True)
    assert a['frames'] == [0, 1] and a['frame_dets'].tolist() == [[0, 2], [2, 1]] and a['in_bytes'] == 60 + 18
    assert b['frames'] == [0, 0, 1] and b['frame_dets'].tolist() == [[0, 1], [1, 1], [2, 1]] and b['in_bytes'] == 2 * 60 + 18
    assert b['frame_offsets'].tolist() == [0, 60, 120] and b['offsets'][:, 0].tolist() == [0] * 3 + [60] * 3 + [120] * 3
    assert np.array_equal(a['geom'], b['geom']) and np.array_equal(a['offsets'][:, 1:], b['offsets'][:, 1:])


def test_check_draw_skeletons_refuses_what_the_library_refuses():
    from spec_amd import _lib
    from spec_amd.engine import check_draw_skeletons
    good = dict(Mtot=3, J=6, D=3, bones=[(0, 1), (4, 5)], geom=[[8, 9, 0, 2], [4, 4, 2, 1]], offsets=[[0, 30], [240, 12]], slab_bytes=288)
    bones, geom, offsets, style = check_draw_skeletons(**good)
    assert bones.dtype == np.int32 and geom.dtype == np.int32 and offsets.dtype == np.int64 and (style.radius, style.thickness) == (4, 2)
    assert abs(style.conf_thr - 0.3) < 1e-7 and bytes(style.joint_rgb) == bytes([0, 255, 0]) and bytes(style.bone_rgb[1]) == bytes([255, 0, 0])
    bad = [dict(J=0), dict(D=4), dict(D=1), dict(Mtot=-1), dict(bones=[(0, 6)]), dict(bones=[(-1, 0)]), dict(geom=[[8, 9, 0, 2]]),
           dict(geom=[[8, 9, 0, 2], [4, 4, 2, 2]]), dict(geom=[[8, 9, -1, 2], [4, 4, 2, 1]]), dict(geom=[[0, 9, 0, 2], [4, 4, 2, 1]]),
           dict(geom=[[8, 8193, 0, 2], [4, 4, 2, 1]]), dict(offsets=[[0, 26], [240, 12]]), dict(offsets=[[0, 30], [240, 11]]), dict(slab_bytes=287),
           dict(offsets=[[-1, 30], [240, 12]]), dict(offsets=[[0, 30], [236, 12]]), dict(offsets=[[0, 30], [27, 30]]),
           dict(style=_lib.DrawStyle(radius=65)), dict(style=_lib.DrawStyle(radius=-1)), dict(style=_lib.DrawStyle(thickness=0)),
           dict(style=_lib.DrawStyle(thickness=65)), dict(style=_lib.DrawStyle(conf_thr=float('nan'))), dict(style=_lib.DrawStyle(conf_thr=float('inf')))]
    for b in bad:
        with pytest.raises(ValueError):
            check_draw_skeletons(**dict(good, **b))
    check_draw_skeletons(**dict(good, offsets=[[0, 30], [27, 30]], geom=[[8, 9, 0, 2], [4, 1, 2, 1]]))        # a column in the other's row padding
    check_draw_skeletons(**dict(good, geom=[[2160, 3840, 0, 3]], offsets=[[0, 3 * 3840]], slab_bytes=2160 * 3840 * 3))


def test_header_declares_and_documents_the_call():
    with open(os.path.join(ROOT, 'include', 'specmi.h')) as f:
        text = f.read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int specmi_draw_skeletons\(specmi_handle\* h, const float\* kp, int Mtot, int J, int D, const int32_t\* bones, '
                  r'int NB,\s*const specmi_draw_style\* style, uint8_t\* slab, size_t slab_bytes, const int32_t\* frame_geom,\s*'
                  r'const int64_t\* frame_offsets, int nframes, void\* stream\);', text, re.S)
    assert m, 'specmi_draw_skeletons is not declared as the issue states it'
    doc = m.group(1)
    for word in ('replaces', 'Refused (SPECMI_ERR_ARG)', 'SPECMI_ERR_STATE', 'SYNCHRONISES THE WHOLE', 'painter', 'count == 0', 'pitch', "PROJECT'S OWN"):
        assert word in doc, word
    assert 'typedef struct specmi_draw_style' in text
    from spec_amd import _lib
    assert 'specmi_draw_skeletons' in _lib.PROTOTYPES and len(_lib.PROTOTYPES['specmi_draw_skeletons'][1]) == 14
