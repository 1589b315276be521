"""Host side of the demo's pictures (spec_amd/render.py, specmi_render_meshes): the C ABI surface, the refusals made before any
launch, the top-left rule of the CPU restatement (tests/render_ref.py), what its normal sums and its resolve stage state and the
conditions tests/test_gpu_render_edges.py relies on for its shading bounds, panel 0 against the reference's own
show_horizon_line and the .obj writer.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests.util import NoLibrary, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'specmi_render_meshes'


def test_export_is_declared_documented_bound_and_built():
    from spec_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int ' + NAME + r'\(([^;]*)\);', hdr, flags=re.S)
    assert m, 'no documented declaration in include/specmi.h'
    assert m.group(2).count(',') + 1 == 22 == len(_lib.PROTOTYPES[NAME][1])
    doc = m.group(1)
    assert 'replaces' in doc and 'renderer_cam.py' in doc and 'NO CLIPPING' in doc and 'SPECMI_ERR_ARG' in doc
    for flag, value in (('SIDE_VIEW', 1), ('GROUND_PLANE', 2), ('CULL', 4), ('THREAD_PER_TRIANGLE', 8)):
        assert re.search(rf'#define SPECMI_RENDER_{flag} {value}\b', hdr) and getattr(_lib, 'RENDER_' + flag) == value
    assert 'render.hip' in build.SOURCES
    build.build(verbose=False)
    assert hasattr(_lib.load(), NAME)


def test_null_handle_is_refused():
    from spec_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    rgb = (C.c_float * 3)(1, 1, 1)
    assert lib.specmi_render_meshes(None, None, 1, 1, None, 1, None, None, 1., 1., 0., 0., None, 1, 1, rgb, 0, None, None, None, None, None) == _lib.ERR_ARG


def test_wrapper_refuses_bad_arguments_before_any_library_call():
    from spec_amd import _lib, render
    from spec_amd.engine import Engine
    eng = NoLibrary()
    call = lambda **kw: Engine.render_meshes(eng, **{**good, **kw})
    v, f = RR.octahedron()
    good = dict(vertices=torch.from_numpy(v)[None], faces=torch.from_numpy(f), cam_t=torch.tensor([[0., 0., 5.]]), R=torch.eye(3),
                focal=(50., 50.), center=(16., 12.), frame=torch.zeros(24, 32, 3, dtype=torch.uint8), flags=_lib.RENDER_CULL)
    bad = [dict(vertices=good['vertices'].double()), dict(vertices=good['vertices'][0]), dict(vertices=good['vertices'][:, :0]),
           dict(faces=good['faces'].long()), dict(faces=good['faces'][:, :2]), dict(faces=good['faces'][:0]),
           dict(cam_t=torch.zeros(2, 3)), dict(R=torch.eye(4)), dict(R=torch.eye(3)[None]),
           dict(frame=None), dict(frame=torch.zeros(24, 32, 3)), dict(frame=torch.zeros(24, 32, 4, dtype=torch.uint8)),
           dict(frame=None, flags=_lib.RENDER_SIDE_VIEW), dict(frame=None, flags=_lib.RENDER_SIDE_VIEW, size=(0, 5)),
           dict(flags=_lib.RENDER_GROUND_PLANE), dict(flags=16), dict(focal=(0., 50.)), dict(focal=(50., float('nan'))),
           dict(center=(float('inf'), 0.)), dict(rgb=(1., 1.)), dict(rgb=(1., float('nan'), 0.))]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match='host path'):                                # a host frame
        render.render_overlay(good['frame'], v, [0., 0., 5.], np.eye(3), (50., 50.), (16., 12.), faces=f)


def _count(tris, H, W):
    n = np.zeros((H, W), np.int64)
    for x, y in tris:
        c = RR.triangle_cover(x, y, H, W, cull=False)
        if c is not None:
            np.add.at(n, (c[0], c[1]), 1)
    return n


@pytest.mark.parametrize('quad', ['square', 'diamond', 'skew'])
def test_top_left_rule_shared_edge_is_covered_once(quad):
    """Two triangles that share an edge, over a sweep of sub-pixel offsets and both windings: every pixel centre strictly inside
    the quad is covered exactly once (also those ON the shared diagonal), none twice, none outside."""
    H, W = 12, 14
    base = {'square': [(256, 256), (1792, 256), (1792, 1792), (256, 1792)],           # diagonal through pixel centres at offset 128
            'diamond': [(1152, 128), (2176, 1152), (1152, 2176), (128, 1152)],
            'skew': [(300, 200), (2500, 700), (2100, 2300), (100, 1500)]}[quad]
    on_diagonal = 0
    offsets = [(ox, oy) for ox in range(0, 256, 16) for oy in (0, 1, 127, 128, 129, 255)] + [(o, o) for o in range(0, 256, 8)]
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    X, Y = 256 * jj + 128, 256 * ii + 128
    for ox, oy in offsets:
        q = [(x + ox, y + oy) for x, y in base]
        for order in ((0, 1, 2, 3), (3, 2, 1, 0)):
            a, b, c, d = (q[k] for k in order)
            tris = [((a[0], b[0], c[0]), (a[1], b[1], c[1])), ((a[0], c[0], d[0]), (a[1], c[1], d[1]))]
            n = _count(tris, H, W)
            e = np.stack([RR._orient(q[k][0], q[k][1], q[(k + 1) % 4][0], q[(k + 1) % 4][1], X, Y) for k in range(4)])
            inside, outside = (e > 0).all(0) | (e < 0).all(0), ((e > 0).any(0) & (e < 0).any(0))
            assert n.max() <= 1 and (n[inside] == 1).all() and (n[outside] == 0).all(), (quad, ox, oy, order)
            on_diagonal += int((inside & (RR._orient(a[0], a[1], c[0], c[1], X, Y) == 0)).sum())
    assert quad == 'skew' or on_diagonal > 0          # the sweep does put pixel centres on the shared edge


def test_quad_split_either_way_covers_the_same_pixels():
    """The boundary of a quad is treated the same whichever diagonal splits it (the rule is a property of the edge)."""
    q = [(256 + 128, 256 + 128), (2048 + 128, 256 + 128), (2048 + 128, 1536 + 128), (256 + 128, 1536 + 128)]     # corners ON pixel centres
    tri = lambda *k: (tuple(q[i][0] for i in k), tuple(q[i][1] for i in k))
    n1, n2 = _count([tri(0, 1, 2), tri(0, 2, 3)], 10, 12), _count([tri(0, 1, 3), tri(1, 2, 3)], 10, 12)
    assert np.array_equal(n1, n2) and n1.max() == 1
    assert n1[1, 1] == 1 and n1[1, 8] == 0 and n1[6, 1] == 0          # the top-left corner pixel is in, right and bottom edges out
    assert n1.sum() == 7 * 5


def test_normal_sums_nan_wrap_and_foreign_indices():
    """What ``normal_sums`` states beyond the plain sum: a non-finite face normal, the int32 wrap, faces that name no vertex."""
    v = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    one = RR.normal_sums(v, f)
    assert np.array_equal(one[0, :3], [[0, 0, 2 ** 28]] * 3) and not one[0, 3].any()
    # faces naming -1, V or INT32_MIN contribute nothing, to no vertex
    assert np.array_equal(RR.normal_sums(v, np.array([[0, 1, 2], [0, 1, -1], [4, 1, 2], [0, -2 ** 31, 2]], np.int64)), one)
    # a NaN anywhere in a face makes each NaN component -2^30 at ALL three of its vertices; +-Inf clamps to +-2^30
    w = v.copy()
    w[0, 2] = np.nan
    assert np.array_equal(RR.normal_sums(w, f)[0, :3], [[-2 ** 30] * 3] * 3)
    w[0, 2] = [0, np.inf, 0]
    assert np.array_equal(RR.normal_sums(w, f)[0, 0], [-2 ** 30, 0, 2 ** 30])          # (0 0 - 0 inf, 0 0 - 1 0, 1 inf - 0 0) = (NaN, 0, inf)
    # the sums wrap as int32: three faces of 2 * 4 m^2 each clamp to 2^30 per face and add up to 3 * 2^30 = -2^30 (mod 2^32)
    big = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]]], np.float32)
    assert np.array_equal(RR.normal_sums(big, np.array([[0, 1, 2]] * 3, np.int32))[0, 0], [0, 0, -2 ** 30])


def _host_pictures(meshes, side):
    """The shading scene through the restatement alone: ids from ``rasterize``, then ``resolve`` in fp32 and in float64."""
    d = RR.shading_scene(meshes)
    xs, ys, z, keep = RR.vertex_stage(d['v'], d['t'], d['R'], *d['cam'], side=side)
    assert keep.all()
    sx, sy = RR.snap(xs, ys, keep)
    ids = RR.rasterize(sx, sy, z, d['f'], *d['size'])[0]
    run = lambda dtype, variant=None: RR.resolve(sx, sy, z, d['v'], d['f'], ids, d['rgb'], side, dtype, variant)
    return d, ids, run


@pytest.mark.parametrize('meshes', [1, 2])
@pytest.mark.parametrize('side', [False, True])
def test_shading_scene_margin_cap_and_discrimination(meshes, side):
    """The conditions tests/test_gpu_render_edges.py relies on, for the restatement alone.  (a) The scene: about 260 pixels,
    at least 7 faces, dozens of distinct bytes per channel (with M = 2 both meshes show).  (b) delta = 4 x max |fp32 - float64|
    of ``resolve``, computed here from the inputs: at most 1 % of the covered pixel-channels lie within delta of a half-integer,
    so the byte is decided by the float64 value at 99 % of them at least.  (c) Each deliberate mistake of ``resolve`` moves
    EVERY channel's byte by 2 or more at more than a quarter of the covered pixels - a +-1 byte test could not hide it."""
    d, ids, run = _host_pictures(meshes, side)
    cov = ids >= 0
    (v32, b32), (v64, b64) = run(np.float32), run(np.float64)
    assert 200 < cov.sum() < 1000 and len(np.unique(ids[cov])) >= 7 and min(len(np.unique(b64[cov][:, c])) for c in range(3)) >= 50
    assert meshes == 1 or all(((ids[cov] // 20) == m).sum() > 50 for m in range(2))
    gap, delta, near, covered = RR.half_integer_margin(v32, v64)
    assert np.array_equal(covered, np.repeat(cov[..., None], 3, 2))
    share = near.sum() / covered.sum()
    print(f'M={meshes} side={side}: {cov.sum()} px, {len(np.unique(ids[cov]))} faces, |fp32 - float64| {gap:.3e} byte, delta {delta:.3e}, '
          f'near a half-integer {near.sum()} of {covered.sum()} ({share:.4f}), fp32 bytes != float64 bytes {(b32 != b64).sum()}')
    assert 0 < gap < 1e-3                   # fp32 rounding of a chain of some 60 operations on values up to 255; 0 would mean one chain ran twice
    assert share <= 0.01
    assert np.array_equal(b32[~near], b64[~near]) and (np.abs(b32.astype(np.int64) - b64) <= 1).all()
    for variant in RR.RESOLVE_VARIANTS[1:]:
        moved = (np.abs(run(np.float32, variant)[1].astype(np.int64) - b32)[cov].min(axis=1) >= 2).mean()
        print(f'   {variant}: every channel off by 2 or more at {moved:.3f} of the covered pixels')
        assert moved > 0.25, variant


def test_panel0_equals_the_reference_show_horizon_line():
    import PIL
    from spec_amd import render
    g = golden('horizon_line.npz')
    assert str(g['pillow_version']) == PIL.__version__, 'the caption font is Pillow\'s: regenerate the fixture for this Pillow'
    assert g['frame'].shape == (48, 64, 3)
    for k, cp in enumerate(g['cam_params']):
        assert np.array_equal(render.group_panel0(g['frame'], cp), g[f'out_{k}']), k
        img, ctr = render.show_horizon_line(g['frame'].astype(np.float64), cp[0], cp[1], cp[2], focal_length=cp[3], color=(0, 255, 0),
                                            width=5, debug=True, text_size=30)
        assert np.array_equal(img, g[f'out_{k}']) and ctr == float(g[f'ctr_{k}'])
    assert not np.array_equal(g['out_0'], g['out_1']) and (g['out_0'][:30] != g['frame'][:30]).any()


def test_obj_writer_round_trips(tmp_path):
    from spec_amd import render
    v, f = RR.icosphere(1, 0.731)
    v = (v * np.float32(1 / 3) + np.float32(1e-7)).astype(np.float32)             # values that need all nine digits
    path = render.write_obj(str(tmp_path / 'mesh.obj'), v, f)
    v2, f2 = render.read_obj(path)
    assert v2.dtype == np.float32 and np.array_equal(v2, v) and f2.dtype == np.int32 and np.array_equal(f2, f)
    assert open(path).readline().startswith('v ') and ' 0 ' not in ''.join(l for l in open(path) if l.startswith('f'))     # 1-based


def test_synthetic_assets_carry_a_face_table():
    from spec_amd import assets
    model = assets.use_synthetic_assets(1003)
    f = assets.faces()
    assert f.shape == (13776, 3) and f.dtype == np.int32 and f.min() == 0 and f.max() == model['v_template'].shape[0] - 1
    assert len(np.unique(f)) == model['v_template'].shape[0] and (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all()
    assert np.array_equal(f, assets.faces())
