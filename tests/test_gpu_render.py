"""specmi_render_meshes on MI355X against the CPU restatement of its contract (tests/render_ref.py): the vertex stage against
float64, coverage / visibility bit for bit from the GPU's own snapped coordinates, orientation, composite, determinism and
batching, alignment with the path's own projection at SMPL size, the side view and its plane, and the demo flow.

The depth bound: Z_BOUND = 4 x the largest |fp32 NumPy vertex stage - float64 vertex stage| in z over the scenes of this file
(the factor covers the GPU's own rounding of the same operations), computed below from the inputs and recorded in DESIGN.md f-8."""
import os

import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests.util import gpu_models, synth_states, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


_rot = RR.rot          # shared with tests/test_render_host.py and tests/test_gpu_render_edges.py


def _scenes():
    """name -> dict(v (M,V,3), f, t (M,3), R, cam (fx, fy, cx, cy), size (H, W))"""
    ov, of = RR.octahedron(1.0)
    sv, sf = RR.icosphere(2, 1.0)
    spin = _rot(0.4, 0.7).astype(np.float64)
    ov = (ov.astype(np.float64) @ spin.T).astype(np.float32)              # no edge of the octahedron is axis-aligned
    s = {}
    s['octahedron'] = dict(v=ov[None], f=of, t=[[0.1, -0.05, 4.0]], R=_rot(0.1, -0.05), cam=(40., 40., 23.5, 16.5), size=(33, 47))
    s['icosphere_off_centre'] = dict(v=sv[None], f=sf, t=[[0.2, 0.1, 3.5]], R=_rot(-0.2, 0.15), cam=(70., 75., 30.25, 40.75), size=(64, 96))
    # two spheres of diameter 1.2 overlapping on screen, 2 m apart in depth (more than a diameter)
    s['two_spheres'] = dict(v=np.stack([sv * 0.6, sv * 0.6]), f=sf, t=[[-0.1, 0.0, 3.0], [0.25, 0.1, 5.0]], R=_rot(0.05, 0.0),
                            cam=(80., 80., 48., 32.), size=(64, 96))
    # three meshes: a sphere partly outside the frame, a sphere flattened to a disc below the camera that straddles the near plane
    # (z from -0.5 to 2.5: its triangles there are dropped whole, its far part shows), a small sphere
    disc = sv * np.array([1.5, 0.02, 1.5], np.float32)
    s['three_partly_outside_and_near'] = dict(v=np.stack([sv * 0.5, disc, sv * 0.5]), f=sf,
                                              t=[[1.3, -0.3, 3.0], [0.0, 0.4, 1.0], [-0.8, -0.2, 4.0]], R=_rot(0.0, 0.1),
                                              cam=(45., 45., 20., 12.), size=(33, 47))
    for d in s.values():
        d['v'], d['t'] = np.ascontiguousarray(d['v'], np.float32), np.asarray(d['t'], np.float32)
    return s


SCENES = _scenes()


def _stage(d, side, dtype):
    return RR.vertex_stage(d['v'], d['t'], d['R'], *d['cam'], side=side, dtype=dtype)


def _z_bound():
    worst = 0.0
    for d in SCENES.values():
        for side in (False, True):
            z32, z64 = _stage(d, side, np.float32)[2], _stage(d, side, np.float64)[2]
            worst = max(worst, float(np.abs(z32.astype(np.float64) - z64).max()))
    return 4.0 * worst


Z_BOUND = _z_bound()


def _render(d, flags, maps=True, frame=None, rgb=(0.8, 0.5, 0.6)):
    from spec_amd import cam_utils
    eng = cam_utils._engine(torch.device(DEV))
    H, W = d['size']
    if frame is None:
        frame = torch.from_numpy(np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)
    out = eng.render_meshes(t(d['v']).to(DEV), t(d['f']).to(DEV), t(d['t']).to(DEV), t(d['R']).to(DEV), d['cam'][:2], d['cam'][2:],
                            frame=frame, rgb=rgb, flags=flags, maps=maps)
    out = {k: v.cpu().numpy() for k, v in out.items()} if maps else out.cpu().numpy()
    return out, frame.cpu().numpy()


@pytest.fixture(scope='module')
def rendered():
    """Every scene once per mode, shared by the tests below: (GPU maps, frame)."""
    from spec_amd import _lib
    return {(name, side): _render(d, _lib.RENDER_CULL | (_lib.RENDER_SIDE_VIEW if side else 0)) for name, d in SCENES.items() for side in (False, True)}


@pytest.fixture(scope='module')
def reference(rendered):
    """render_ref fed the GPU's own snapped coordinates and depths: (id_map, depth) per scene and mode."""
    out = {}
    for (name, side), (g, _) in rendered.items():
        d = SCENES[name]
        out[name, side] = RR.rasterize(g['screen_xy'][..., 0], g['screen_xy'][..., 1], g['screen_z'], d['f'], *d['size'], cull=True)[:2]
    return out


@pytest.mark.parametrize('name', list(SCENES))
@pytest.mark.parametrize('side', [False, True])
def test_screen_output_vs_float64_vertex_stage(rendered, name, side):
    g, _ = rendered[name, side]
    xs, ys, z, keep = _stage(SCENES[name], side, np.float64)
    sx, sy = RR.snap(xs, ys, keep)
    # a vertex within the bound of the near plane may be kept by one stage and dropped by the other: none here by construction
    assert (np.abs(z - RR.ZNEAR) > 1e-3).all()
    gx, gy = g['screen_xy'][..., 0].astype(np.int64), g['screen_xy'][..., 1].astype(np.int64)
    assert np.array_equal(gx == RR.DROPPED, ~keep) and np.array_equal(gy == RR.DROPPED, ~keep)
    ex, ey, ez = np.abs(gx - sx)[keep].max(), np.abs(gy - sy)[keep].max(), np.abs(g['screen_z'].astype(np.float64) - z).max()
    print(f'{name} side={side}: |dx| {ex} |dy| {ey} (1/256 px), |dz| {ez:.3e} (bound {Z_BOUND:.3e})')
    assert ex <= 1 and ey <= 1
    assert ez <= Z_BOUND
    if name == 'three_partly_outside_and_near':
        assert (~keep[1]).any() and keep[1].any() and keep[0].all()          # mesh 1 does straddle the near plane


@pytest.mark.parametrize('name', list(SCENES))
@pytest.mark.parametrize('side', [False, True])
def test_coverage_ids_and_depth_vs_render_ref(rendered, reference, name, side):
    g, _ = rendered[name, side]
    ids, depth = reference[name, side]
    assert np.array_equal(g['id_map'] >= 0, ids >= 0)                        # coverage: bit-identical
    assert (ids >= 0).sum() > 20
    assert np.array_equal(g['id_map'], ids)
    assert np.array_equal((g['depth'] > 0), ids >= 0)
    err = np.abs(g['depth'].astype(np.float64) - depth.astype(np.float64)).max()
    print(f'{name} side={side}: covered {(ids >= 0).sum()} px, |depth - ref| {err:.3e} (bound {Z_BOUND:.3e})')
    assert err <= Z_BOUND


def test_two_spheres_are_separated_and_the_nearer_wins(rendered):
    """The reference's two nearest layers at every pixel both spheres cover differ by more than 1e-3 relative (no near ties),
    and the nearer sphere (mesh 0) owns those pixels."""
    d = SCENES['two_spheres']
    g, _ = rendered['two_spheres', False]
    sx, sy, sz = g['screen_xy'][..., 0], g['screen_xy'][..., 1], g['screen_z']
    layers = [RR.rasterize(sx[m:m + 1], sy[m:m + 1], sz[m:m + 1], d['f'], *d['size'], cull=True) for m in range(2)]
    both = (layers[0][0] >= 0) & (layers[1][0] >= 0)
    assert both.sum() > 50
    z0, z1 = layers[0][1][both].astype(np.float64), layers[1][1][both].astype(np.float64)
    assert (np.abs(z1 - z0) / np.minimum(z0, z1)).min() > 1e-3
    F = d['f'].shape[0]
    assert (g['id_map'][both] < F).all() and (g['id_map'][(layers[1][0] >= 0) & ~both] >= F).all()


def test_inward_wound_sphere_draws_nothing_with_cull_on(rendered):
    """Orientation.  Every face an outward-wound sphere shows, wound the other way, is culled: the inward-wound surface that
    faces the camera draws NOTHING.  (Of a whole closed sphere wound inward the far half then faces the camera from inside - as
    under any back-face culling - so "nothing" holds for the surface the camera sees from outside, and the closed sphere is
    checked for drawing only faces the outward-wound one hides, all behind the faces it shows.)"""
    from spec_amd import _lib
    d = dict(SCENES['icosphere_off_centre'])
    g_out, _ = rendered['icosphere_off_centre', False]
    F = d['f'].shape[0]
    # which faces face the camera, from the float64 vertex stage (not from the renderer under test)
    xs, ys, z, _ = _stage(d, False, np.float64)
    fx_, fy_ = xs[0][d['f']], ys[0][d['f']]                                   # (F, 3)
    facing = RR._orient(fx_[:, 0], fy_[:, 0], fx_[:, 1], fy_[:, 1], fx_[:, 2], fy_[:, 2]) < 0
    assert 50 < facing.sum() < F - 50 and set(np.unique(g_out['id_map'][g_out['id_map'] >= 0])) <= set(np.nonzero(facing)[0])
    near_inward = dict(d, f=np.ascontiguousarray(d['f'][facing][:, ::-1]))
    g, frame = _render(near_inward, _lib.RENDER_CULL)
    assert (g['id_map'] == -1).all() and (g['depth'] == 0).all() and np.array_equal(g['image'], frame)
    g_off, _ = _render(near_inward, 0)                                       # the same surface with culling off is drawn
    assert np.array_equal(g_off['id_map'] >= 0, g_out['id_map'] >= 0)
    whole_inward = dict(d, f=np.ascontiguousarray(d['f'][:, ::-1]))
    g2, _ = _render(whole_inward, _lib.RENDER_CULL)
    drawn = np.unique(g2['id_map'][g2['id_map'] >= 0])
    assert drawn.size > 50 and not facing[drawn].any()
    both = (g2['id_map'] >= 0) & (g_out['id_map'] >= 0)                       # the inside of the far half lies behind the near half
    assert both.sum() > 1000 and (g2['depth'][both] > g_out['depth'][both]).all()


def test_composite_uncovered_is_the_frame_and_a_facing_triangle_has_the_formula_byte(rendered):
    from spec_amd import _lib
    for (name, side), (g, frame) in rendered.items():
        if not side:
            assert np.array_equal(g['image'][g['id_map'] < 0], frame[g['id_map'] < 0]), name
    # one triangle facing the camera: model normal (0, 0, -1) -> n.l = 1 overlay; tilted by 60 degrees about y: n.l = 0.5
    rgb = (0.8, 0.5, 0.6)
    for tilt, ndl in ((0.0, 1.0), (np.pi / 3, 0.5)):
        c, s = np.cos(tilt), np.sin(tilt)
        v = np.array([[-1., -1., 0.], [1., -1., 0.], [0., 1., 0.]]) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
        d = dict(v=np.ascontiguousarray(v[None], np.float32), f=np.array([[0, 2, 1]], np.int32), t=np.array([[0., 0., 4.]], np.float32),
                 R=np.eye(3, dtype=np.float32), cam=(30., 30., 23.5, 16.5), size=(33, 47))
        g, frame = _render(d, _lib.RENDER_CULL, rgb=rgb)
        hit = g['id_map'] == 0
        assert hit.sum() > 30
        want = RR.shaded_byte(rgb, ndl).astype(np.int64)
        assert (np.abs(g['image'][hit].astype(np.int64) - want) <= 1).all(), (tilt, g['image'][hit][0], want)
        assert np.array_equal(g['image'][~hit], frame[~hit])


@pytest.mark.parametrize('name', ['two_spheres', 'three_partly_outside_and_near'])
def test_determinism_batching_and_launch_shape(rendered, name):
    from spec_amd import _lib
    d = SCENES[name]
    g, frame = rendered[name, False]
    again, _ = _render(d, _lib.RENDER_CULL)
    thread, _ = _render(d, _lib.RENDER_CULL | _lib.RENDER_THREAD_PER_TRIANGLE)
    for k in ('image', 'id_map', 'depth', 'screen_xy', 'screen_z'):
        assert again[k].tobytes() == g[k].tobytes(), k                       # two runs: bit-identical
        assert thread[k].tobytes() == g[k].tobytes(), k                      # one thread per triangle: the same bits
    # M meshes in one call == the nearer-wins merge of M single calls, by depth
    M, F = d['v'].shape[0], d['f'].shape[0]
    ids, depth, image = np.full(d['size'], -1, np.int32), np.zeros(d['size'], np.float32), frame.copy()
    for m in range(M):
        one, _ = _render(dict(d, v=d['v'][m:m + 1], t=d['t'][m:m + 1]), _lib.RENDER_CULL)
        win = (one['depth'] > 0) & ((depth == 0) | (one['depth'] < depth))
        ids[win], depth[win], image[win] = one['id_map'][win] + m * F, one['depth'][win], one['image'][win]
    assert np.array_equal(ids, g['id_map']) and depth.tobytes() == g['depth'].tobytes() and np.array_equal(image, g['image'])


def test_side_view_background_and_checker_plane():
    from spec_amd import _lib
    d = SCENES['icosphere_off_centre']
    g, _ = _render(d, _lib.RENDER_CULL | _lib.RENDER_SIDE_VIEW | _lib.RENDER_GROUND_PLANE)
    bare, _ = _render(d, _lib.RENDER_CULL | _lib.RENDER_SIDE_VIEW)
    assert (bare['image'][bare['id_map'] < 0] == 0).all() and (bare['id_map'] >= 0).sum() > 100
    H, W = d['size']
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    s, grey, ok = RR.checker(ii, jj, d['R'], d['t'][0], *d['cam'], RR.lowest_y(d['v'], d['t'], d['R']))
    mesh_z = np.where(bare['depth'] > 0, bare['depth'], np.inf)
    plane = ok & (s < mesh_z)
    assert 200 < plane.sum() < H * W and len(np.unique(grey[plane])) == 2
    assert np.array_equal(g['id_map'] == -2, plane)
    assert (np.abs(g['image'][plane].astype(np.int64) - grey[plane][:, None].astype(np.int64)) <= 1).all()
    assert np.allclose(g['depth'][plane], s[plane], rtol=1e-6)
    nothing = ~plane & (bare['id_map'] < 0)
    assert nothing.sum() > 50 and (g['image'][nothing] == 0).all() and (g['depth'][nothing] == 0).all() and (g['id_map'][nothing] == -1).all()
    mesh = ~plane & (bare['id_map'] >= 0)
    assert np.array_equal(g['image'][mesh], bare['image'][mesh]) and np.array_equal(g['id_map'][mesh], bare['id_map'][mesh])


def test_bad_arguments_are_refused_by_the_library():
    import ctypes as C
    from spec_amd import _lib, cam_utils
    eng = cam_utils._engine(torch.device(DEV))
    d = SCENES['octahedron']
    H, W = d['size']
    v, f, tt, R = t(d['v']).to(DEV), t(d['f']).to(DEV), t(d['t']).to(DEV), t(d['R']).to(DEV)
    frame, out = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV), torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)
    rgb = (C.c_float * 3)(1, 1, 1)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    good = dict(v=p(v), M=1, V=6, f=p(f), F=8, t=p(tt), R=p(R), fx=40., fy=40., cx=20., cy=16., frame=p(frame), H=H, W=W, rgb=rgb, flags=4, out=p(out))
    call = lambda a: eng.lib.specmi_render_meshes(eng.h, a['v'], a['M'], a['V'], a['f'], a['F'], a['t'], a['R'], a['fx'], a['fy'], a['cx'], a['cy'],
                                                  a['frame'], a['H'], a['W'], a['rgb'], a['flags'], a['out'], None, None, None, eng._stream())
    for bad in (dict(v=None), dict(f=None), dict(t=None), dict(R=None), dict(out=None), dict(frame=None), dict(rgb=None), dict(M=0), dict(V=0),
                dict(F=0), dict(H=0), dict(W=40000), dict(fx=0.), dict(fy=float('nan')), dict(cx=float('inf')), dict(flags=16), dict(flags=2),
                dict(M=1 << 20, F=1 << 12), dict(rgb=(C.c_float * 3)(1, float('nan'), 1))):
        assert call(dict(good, **bad)) == _lib.ERR_ARG, bad
        assert eng.lib.specmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert (out == 7).all()                                                   # nothing was launched
    assert call(good) == _lib.OK and call(dict(good, frame=None, flags=1)) == _lib.OK        # a side view needs no frame


@pytest.fixture(scope='module')
def hmr_step():
    from spec_amd import assets, cam_utils, synth
    _, hm = gpu_models(True, True, DEV)
    B, H, W = 2, 128, 160
    x = t(synth.images(9, B)).to(DEV)
    pitch, roll, f_pix = 0.12, 0.06, 150.0
    R, K = cam_utils.cam_params_from_angles([pitch] * B, [roll] * B, [f_pix] * B, [W] * B, [H] * B, device=DEV)
    boxes = dict(bbox_scale=torch.tensor([0.5, 0.4], device=DEV), bbox_center=torch.tensor([[70., 60.], [95., 70.]], device=DEV),
                 img_w=torch.full((B,), float(W), device=DEV), img_h=torch.full((B,), float(H), device=DEV))
    out = hm(x, cam_rotmat=R, cam_intrinsics=K, **boxes)
    return dict(out=out, R=R[0].cpu().numpy(), pitch=pitch, roll=roll, f=f_pix, size=(H, W), faces=assets.faces())


def test_alignment_with_the_path_at_smpl_size(hmr_step):
    """A synthetic-asset HMR(use_cam=True) forward at B = 2 on a 128 x 160 frame, drawn with the tester's rotation
    Rx(-pitch) Rz(roll): the bounding box of each mesh's mask equals, within 1 px, the bounding box of its vertices projected by
    K (R v + t) on the host (R = the model's cam_rotmat, centre (W // 2, H // 2)), clipped to the frame."""
    from spec_amd import render
    h = hmr_step
    H, W = h['size']
    v, tt = h['out']['smpl_vertices'], h['out']['pred_cam_t']
    assert tuple(v.shape) == (2, 6890, 3) and h['faces'].shape == (13776, 3)
    frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    F = h['faces'].shape[0]
    for m in range(2):
        g = render.render_overlay(frame, v[m:m + 1], tt[m:m + 1], _rot(-h['pitch'], h['roll']), (h['f'], h['f']), (W // 2, H // 2), cull=False, maps=True)
        mask = g['id_map'].cpu().numpy() >= 0
        P = v[m].cpu().numpy().astype(np.float64) @ h['R'].astype(np.float64).T + tt[m].cpu().numpy().astype(np.float64)
        assert (P[:, 2] > 0.05).all(), 'the synthetic mesh reaches behind the near plane'
        x, y = W // 2 + h['f'] * P[:, 0] / P[:, 2], H // 2 + h['f'] * P[:, 1] / P[:, 2]
        rows, cols = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
        assert rows.size and cols.size
        # the rows / columns whose pixel centres (index + 0.5) lie inside the projected box, clipped to the frame
        got = np.array([cols[0], cols[-1], rows[0], rows[-1]])
        want = np.array([np.clip(np.ceil(x.min() - 0.5), 0, W - 1), np.clip(np.floor(x.max() - 0.5), 0, W - 1),
                         np.clip(np.ceil(y.min() - 0.5), 0, H - 1), np.clip(np.floor(y.max() - 0.5), 0, H - 1)])
        print(f'mesh {m}: mask box {got}, projected box {want} ({x.min():.2f} .. {x.max():.2f}, {y.min():.2f} .. {y.max():.2f}), {mask.sum()} px')
        assert want[1] - want[0] > 8 and want[3] - want[2] > 8, 'the synthetic mesh misses the frame'
        assert (np.abs(got - want) <= 1).all()


def test_demo_flow_writes_pictures_and_leaves_the_pickles_alone(tmp_path):
    import joblib
    from types import SimpleNamespace
    from PIL import Image
    from spec_amd import evaluation, render
    from spec_amd.tester import SPECTester
    tree = str(tmp_path / 'tree')
    evaluation.write_standin_data_tree(tree, n_images=2)
    folder = os.path.join(tree, 'data/sample_images')
    names = sorted(os.listdir(folder))
    sizes = [Image.open(os.path.join(folder, n)).size for n in names]
    rng = np.random.default_rng(3)
    dets = [np.stack([rng.uniform(0.3 * w, 0.7 * w, n), rng.uniform(0.3 * h, 0.7 * h, n), rng.uniform(60, 120, n), rng.uniform(60, 120, n)], 1)
            .astype(np.float32) for (w, h), n in zip(sizes, (2, 1))]
    hs = {k_: t(v) for k_, v in synth_states(True)[1].items()}
    cwd = os.getcwd()
    os.chdir(tree)
    try:
        res = {}
        for no_render in (True, False):
            out = str(tmp_path / f'out_{int(no_render)}')
            args = SimpleNamespace(cfg=None, ckpt=hs, no_save=False, no_render=no_render, save_obj=not no_render, synthetic_assets=True,
                                   frame_batch=256, plan='throughput', decode_threads=2, camcalib_model=gpu_models(True, True, DEV)[0], detections=dets)
            te = SPECTester(args)
            te.run_camcalib(folder, out)
            assert te.run_on_image_folder(folder, te.run_detector(folder), out, os.path.join(out, 'pictures')) == 2
            res[no_render] = {f: joblib.load(os.path.join(out, 'spec_results', f)) for f in sorted(os.listdir(os.path.join(out, 'spec_results')))}
    finally:
        os.chdir(cwd)
    assert sorted(res[True]) == sorted(res[False]) and len(res[True]) == 2
    for f, rec in res[True].items():
        for key, val in rec.items():
            assert res[False][f][key].tobytes() == val.tobytes(), (f, key)
    assert not os.path.exists(str(tmp_path / 'out_1' / 'pictures'))
    pics = sorted(os.listdir(str(tmp_path / 'out_0' / 'pictures')))
    stems = [os.path.splitext(n) for n in names]
    assert pics == sorted([f'{stems[0][0]}_{i:06d}{stems[0][1]}' for i in range(2)] + [f'{stems[1][0]}_000000{stems[1][1]}'])
    for pic in pics:
        (w, h) = sizes[0] if pic.startswith(stems[0][0] + '_') else sizes[1]
        im = np.array(Image.open(str(tmp_path / 'out_0' / 'pictures' / pic)))
        assert im.shape == (h, 3 * w, 3) and im.dtype == np.uint8
        assert (im[:30, :w] == 0).mean() > 0.5 and (im[:, 2 * w:] != im[:, :w]).any()          # the caption strip; a side view that is no copy
    v, f = render.read_obj(str(tmp_path / 'out_0' / 'meshes' / stems[0][0] / '000001.obj'))
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    assert np.array_equal(v * np.array([1, -1, -1], np.float32), res[False][stems[0][0] + '.pkl']['smpl_vertices'][1])
