"""specmi_render_views on MI355X: every view of one call equals, bit for bit, the specmi_render_meshes call with that view's
arguments (image rectangle, id map, depth, screen coordinates); views land where ``render.plan_views`` puts them and nowhere
else; the table rule (same records: no rewrite, capturable; new records under capture: refused); every refusal of the C ABI;
``render_image_groups`` and the demo flow against the per-frame route.  Every assertion is an equality.

Frames: A 33 x 47 with the three meshes of ``three_partly_outside_and_near``, B 64 x 96 with the two of ``two_spheres``, C 40 x 40
with the one of ``icosphere_off_centre`` (its camera centre moved to (20.25, 18.75) so that it lands in the frame): six
``icosphere(2)`` meshes (V = 162, F = 320) in one array, one camera per frame, random uint8 frames."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

from spec_amd import _lib, render
from spec_amd.preprocess import pack_frames
from tests.test_gpu_render import SCENES
from tests.util import gpu_models, synth_states, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
RGB = (0.8, 0.5, 0.6)
CULL, SIDE, GROUND, THREAD = _lib.RENDER_CULL, _lib.RENDER_SIDE_VIEW, _lib.RENDER_GROUND_PLANE, _lib.RENDER_THREAD_PER_TRIANGLE
MAPS = ('id_map', 'depth', 'screen_xy', 'screen_z')


def _frames():
    c = dict(SCENES['icosphere_off_centre'], size=(40, 40))
    c['cam'] = c['cam'][:2] + (20.25, 18.75)
    return [SCENES['three_partly_outside_and_near'], SCENES['two_spheres'], c]


FRAMES = _frames()
SIZES = [d['size'] for d in FRAMES]
COUNTS = [d['v'].shape[0] for d in FRAMES]
FIRST = np.concatenate([[0], np.cumsum(COUNTS)]).tolist()
# the 13 views of case 1: (frame, first mesh of the frame, count, flags)
VIEWS = ([(f, 0, COUNTS[f], fl) for f in range(3) for fl in (CULL, CULL | SIDE | GROUND)] +
         [(f, m, 1, CULL) for f in (0, 1) for m in range(COUNTS[f])] + [(2, 0, 0, 0), (0, 0, COUNTS[0], 0)])


@pytest.fixture(scope='module')
def world():
    """The engine, the six meshes and three frames on the device, and the reference of every view: the render_meshes call
    with its arguments (the frame itself for the view without meshes)."""
    from spec_amd import cam_utils
    eng = cam_utils._engine(torch.device(DEV))
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SIZES]
    w = dict(eng=eng, frames=frames, v=t(np.concatenate([d['v'] for d in FRAMES])).to(DEV), t=t(np.concatenate([d['t'] for d in FRAMES])).to(DEV),
             f=t(FRAMES[0]['f']).to(DEV), R=[d['R'] for d in FRAMES], focal=[d['cam'][:2] for d in FRAMES], center=[d['cam'][2:] for d in FRAMES])
    assert tuple(w['v'].shape) == (6, 162, 3) and tuple(w['f'].shape) == (320, 3) and all((d['f'] == FRAMES[0]['f']).all() for d in FRAMES)
    w['slab'], w['in_off'], _ = pack_frames(frames, DEV)
    dev_frames = [t(fr).to(DEV) for fr in frames]
    ref = []
    for f, m, c, fl in VIEWS:
        if c == 0:
            ref.append({'image': dev_frames[f]})
            continue
        m0 = FIRST[f] + m
        ref.append(eng.render_meshes(w['v'][m0:m0 + c], w['f'], w['t'][m0:m0 + c], t(w['R'][f]).to(DEV), w['focal'][f], w['center'][f],
                                     frame=dev_frames[f], rgb=RGB, flags=fl, maps=True))
    w['ref'] = ref
    return w


def _records(w, views, extra=0):
    """Dense records for ``views``: view v's rectangle at pitch 3 W, the rectangles back to back in the order given."""
    geom, offsets, off = [], [], 0
    for f, m, c, fl in views:
        H, W = SIZES[f]
        geom.append((H, W, FIRST[f] + m if c else 0, c, fl | extra))
        offsets.append((int(w['in_off'][f]), 3 * W, off, 3 * W))
        off += H * W * 3
    return np.asarray(geom, np.int32), np.asarray(offsets, np.int64), render.view_cams([v[0] for v in views], w['R'], w['focal'], w['center']), off


def _call(w, geom, offsets, cams, out_bytes, maps=True, out=None):
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device=DEV) if out is None else out
    return w['eng'].render_views(w['v'], w['f'], w['t'], geom, offsets, cams, w['slab'], out, rgb=RGB, maps=maps)


def _split(got, geom, offsets):
    """The batched call's outputs cut into one dict per view, shaped like ``render_meshes(maps=True)``'s."""
    views, px, pair = [], 0, 0
    for (H, W, _, c, _), (_, _, off, pitch) in zip(geom.tolist(), offsets.tolist()):
        rows = torch.stack([got['slab'][off + i * pitch: off + i * pitch + 3 * W] for i in range(H)])
        views.append({'image': rows.reshape(H, W, 3), 'id_map': got['id_map'][px:px + H * W].reshape(H, W), 'depth': got['depth'][px:px + H * W].reshape(H, W),
                      'screen_xy': got['screen_xy'][pair:pair + c], 'screen_z': got['screen_z'][pair:pair + c]})
        px, pair = px + H * W, pair + c
    return views


def _assert_views_equal_references(w, views, order=None):
    for k, v in enumerate(order if order is not None else range(len(views))):
        ref = w['ref'][v]
        assert torch.equal(views[k]['image'], ref['image']), (v, 'image')
        if VIEWS[v][2] == 0:       # no meshes: nothing drawn anywhere
            assert (views[k]['id_map'] == -1).all() and (views[k]['depth'] == 0).all() and views[k]['screen_xy'].shape[0] == 0
            continue
        for key in MAPS:
            assert torch.equal(views[k][key], ref[key]), (v, key)


# ---- 1. per-view identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thread', [False, True])
def test_every_view_equals_its_render_meshes_call(world, thread):
    geom, offsets, cams, nbytes = _records(world, VIEWS, THREAD if thread else 0)
    assert len(VIEWS) == 13 and sum(1 for v in world['ref'] if 'id_map' in v) == 12
    got = _call(world, geom, offsets, cams, nbytes)
    _assert_views_equal_references(world, _split(got, geom, offsets))
    # the references are not trivially empty
    assert all((r['id_map'] >= 0).sum() > 20 for r in world['ref'] if 'id_map' in r)
    assert (world['ref'][5]['id_map'] == -2).sum() > 50                      # the ground plane is in the picture


# ---- 2. placement ------------------------------------------------------------------------------------------------------------
def test_plan_views_pictures_land_in_place_and_nothing_else_is_touched(world):
    faces = FRAMES[0]['f']
    (ch,) = render.plan_views(SIZES, COUNTS, gap=7)
    assert ch['in_bytes'] == world['slab'].numel() and ch['offsets'][:, 0].tolist() == np.repeat(world['in_off'], 3).tolist()
    before = world['slab'].clone()
    out = torch.full((ch['out_bytes'] + 7,), 0xA5, dtype=torch.uint8, device=DEV)          # a gap after the last picture as well
    _call(world, ch['geom'], ch['offsets'], render.view_cams(ch['view_frame'], world['R'], world['focal'], world['center']), 0, maps=False, out=out)
    used = torch.zeros_like(out, dtype=torch.bool)
    for f, off in enumerate(ch['picture_offsets']):
        H, W = SIZES[f]
        m0, m1 = FIRST[f], FIRST[f + 1]
        want = render.render_image_group(world['frames'][f], world['t'][m0:m1], world['v'][m0:m1], world['R'][f], world['focal'][f], world['center'][f],
                                         mesh_color=RGB, faces=faces, engine=world['eng'])
        assert tuple(want.shape) == (H, 3 * W, 3)
        assert torch.equal(out[off:off + 9 * H * W].reshape(H, 3 * W, 3), want), f
        used[off:off + 9 * H * W] = True
    assert (~used).sum() == 7 * 3 and (out[~used] == 0xA5).all()
    assert torch.equal(world['slab'], before)


# ---- 3. tables and order -----------------------------------------------------------------------------------------------------
def test_repeated_and_reordered_calls_give_the_same_bytes(world):
    geom, offsets, cams, nbytes = _records(world, VIEWS)
    a = _call(world, geom, offsets, cams, nbytes)
    b = _call(world, geom, offsets, cams, nbytes)
    for key in ('slab',) + MAPS:
        assert torch.equal(a[key], b[key]), key
    # the views reversed, each keeping its record (and with it its rectangle): the same slab, the same maps per view
    r = _call(world, geom[::-1].copy(), offsets[::-1].copy(), cams[::-1].copy(), nbytes)
    assert torch.equal(r['slab'], a['slab'])
    _assert_views_equal_references(world, _split(r, geom[::-1], offsets[::-1]), order=list(range(len(VIEWS)))[::-1])


def test_graph_capture_needs_the_records_of_the_previous_call(world):
    eng = world['eng']
    geom, offsets, cams, nbytes = _records(world, VIEWS)
    other = _records(world, VIEWS[:6])
    want = _call(world, geom, offsets, cams, nbytes, maps=False).clone()      # also the warm-up call of the capture below
    out = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):
        try:      # new records: refused, and the capture goes on
            _call(world, *other[:3], 0, maps=False, out=out)
        except _lib.SpecmiError as e:
            err = e
        _call(world, geom, offsets, cams, 0, maps=False, out=out)          # the previous call's records: captured
    assert err is not None and err.code == _lib.ERR_STATE, err
    torch.cuda.synchronize()
    assert (out == 0xA5).all()                                                # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(_call(world, *other[:3], other[3], maps=False), want[:other[3]])      # eagerly the other records are fine


# ---- 4. refusals through the C ABI -------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_library(world):
    eng = world['eng']
    geom, offsets, cams, nbytes = _records(world, VIEWS)
    out = torch.full((nbytes,), 7, dtype=torch.uint8, device=DEV)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    rgb = (C.c_float * 3)(*RGB)
    good = dict(v=p(world['v']), Mtot=6, V=162, f=p(world['f']), F=320, t=p(world['t']), rgb=rgb, slab=p(world['slab']), in_bytes=world['slab'].numel(),
                out=p(out), out_bytes=nbytes, geom=geom, offsets=offsets, cams=cams, n=len(VIEWS))

    def call(a):
        arr = lambda x, ty: None if x is None else np.ascontiguousarray(x).ctypes.data_as(ty)
        return eng.lib.specmi_render_views(eng.h, a['v'], a['Mtot'], a['V'], a['f'], a['F'], a['t'], a['rgb'], a['slab'], a['in_bytes'], a['out'], a['out_bytes'],
                                           arr(a['geom'], _lib.c_int32_p), arr(a['offsets'], _lib.c_int64_p), arr(a['cams'], _lib.c_float_p), a['n'],
                                           None, None, None, eng._stream())

    def with_(name, row, col, value):
        x = good[name].copy()
        x[row, col] = value
        return {name: x}

    huge = 32768 * 32768 * 3
    two_huge = dict(geom=np.array([[32768, 32768, 0, 0, SIDE]] * 2, np.int32), offsets=np.array([[-1, 0, 0, 3 * 32768]] * 2, np.int64), cams=cams[:2], n=2,
                    out_bytes=huge)
    bad = [dict(v=None), dict(f=None), dict(t=None), dict(rgb=None), dict(out=None), dict(geom=None), dict(offsets=None), dict(cams=None), dict(slab=None),
           dict(n=0), dict(n=-1), dict(n=65536), dict(V=0), dict(F=0), dict(Mtot=5), with_('geom', 0, 2, -1), with_('geom', 0, 3, -1),
           dict(with_('geom', 0, 3, 1 << 20), Mtot=1 << 21, F=1 << 12), dict(with_('geom', 0, 3, 1 << 20), Mtot=1 << 21, V=1 << 12), two_huge,
           with_('geom', 3, 0, 0), with_('geom', 3, 1, 32769), with_('geom', 3, 0, -4),
           with_('offsets', 2, 3, 3 * 64 - 1), with_('offsets', 2, 1, 3 * 96 - 1),
           dict(out_bytes=nbytes - 1), with_('offsets', 0, 2, -1), dict(in_bytes=world['slab'].numel() - 1), with_('offsets', 12, 0, 1 << 20),
           dict(out_bytes=1 << 32), dict(in_bytes=1 << 32),
           dict(out=p(world['slab']), out_bytes=world['slab'].numel()), dict(out=C.c_void_p(world['slab'].data_ptr() + world['slab'].numel() - 1)),
           with_('offsets', 1, 2, 3 * 47 - 1), with_('offsets', 1, 2, 0), with_('offsets', 0, 3, 3 * 47 + 1),
           with_('geom', 0, 4, 16), with_('geom', 0, 4, CULL | GROUND), with_('geom', 11, 4, SIDE | GROUND), with_('offsets', 0, 0, -1),
           with_('geom', 4, 4, CULL | THREAD),
           with_('cams', 2, 9, 0.0), with_('cams', 2, 10, np.nan), with_('cams', 2, 9, np.inf), with_('cams', 2, 11, np.inf), with_('cams', 2, 3, np.nan),
           dict(rgb=(C.c_float * 3)(1, float('nan'), 1))]
    for b in bad:
        assert call(dict(good, **b)) == _lib.ERR_ARG, {k: None for k in b}
        assert eng.lib.specmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert (out == 7).all()                                                   # nothing was launched
    assert call(good) == _lib.OK
    want = _call(world, geom, offsets, cams, nbytes, maps=False)
    assert torch.equal(out, want)
    # side views need neither frames nor a frame slab
    sides = [v for v in VIEWS if v[3] & SIDE]
    g2, o2, c2, n2 = _records(world, sides)
    o2[:, 0] = -1
    assert call(dict(good, geom=g2, offsets=o2, cams=c2, n=len(sides), slab=None, in_bytes=0, out_bytes=n2)) == _lib.OK
    torch.cuda.synchronize()
    for k, v in enumerate(v for v in range(len(VIEWS)) if VIEWS[v][3] & SIDE):
        H, W = SIZES[VIEWS[v][0]]
        assert torch.equal(out[o2[k, 2]:o2[k, 2] + 3 * H * W].reshape(H, W, 3), world['ref'][v]['image'])
    with pytest.raises(ValueError):       # and the Python binding refuses before the library is reached
        world['eng'].render_views(world['v'], world['f'], world['t'], geom, offsets, cams, world['slab'], world['slab'], rgb=RGB)


# ---- 5. render_image_groups --------------------------------------------------------------------------------------------------
CAM_PARAMS = [(1.0, 0.1, -0.05, 40.0), (0.9, -0.2, 0.1, 80.0), (1.1, 0.0, 0.0, 70.0)]


@pytest.fixture(scope='module')
def groups(world):
    """render_image_group per frame, and per single detection: {(frame, detection or None): (H, 3W, 3) uint8 host array}"""
    out = {}
    for f in range(3):
        for i in [None] + list(range(COUNTS[f])):
            m0, m1 = (FIRST[f], FIRST[f + 1]) if i is None else (FIRST[f] + i, FIRST[f] + i + 1)
            out[f, i] = render.render_image_group(world['frames'][f], world['t'][m0:m1], world['v'][m0:m1], world['R'][f], world['focal'][f],
                                                  world['center'][f], faces=FRAMES[0]['f'], cam_params=CAM_PARAMS[f], engine=world['eng']).cpu().numpy()
    return out


@pytest.mark.parametrize('budget', [None, 3 * (33 * 47 + 64 * 96)])
def test_render_image_groups_equals_the_per_frame_calls(world, groups, budget):
    kw = dict(faces=FRAMES[0]['f'], cam_params=CAM_PARAMS, engine=world['eng'], pixel_budget=budget)
    assert len(render.plan_views(SIZES, COUNTS, pixel_budget=budget)) == (1 if budget is None else 2)
    got, slabs = render.render_image_groups(world['frames'], world['v'], world['t'], COUNTS, world['R'], world['focal'], world['center'], return_slabs=True, **kw)
    assert len(got) == 3 and len(slabs) == (1 if budget is None else 2)
    for f in range(3):
        assert got[f].dtype == np.uint8 and np.array_equal(got[f], groups[f, None]), f
        assert (got[f][:30, :SIZES[f][1]] == 0).mean() > 0.5                  # the caption strip of the horizon line is on panel 0
    slab, offs, shapes = slabs[0]
    assert slab.device.type == 'cuda' and np.array_equal(slab[offs[1]:offs[1] + shapes[1][0] * shapes[1][1] * 3].cpu().numpy().reshape(got[1].shape), got[1])
    each = render.render_image_groups(world['frames'], world['v'], world['t'], COUNTS, world['R'], world['focal'], world['center'], each=True, **kw)
    keys = [(f, i) for f in range(3) for i in range(COUNTS[f])]
    assert len(each) == 6
    for k, pic in zip(keys, each):
        assert np.array_equal(pic, groups[k]), k
    assert not np.array_equal(groups[0, 0], groups[0, None])


# ---- 6. the demo flow --------------------------------------------------------------------------------------------------------
def test_demo_flow_batched_pictures_equal_the_per_frame_ones(tmp_path):
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
    sizes, counts = [(96, 128), (120, 90), (96, 128), (110, 140)], [2, 1, 1, 3]      # (H, W): three different sizes; 2 + 1 + 1 crops fill one flush of 4
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, f'frame{k}.png'))
    names = sorted(os.listdir(folder))
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
        for batch, ragged, each in ((False, False, False), (True, False, False), (False, True, False), (True, True, False), (False, False, True)):
            out = str(tmp_path / f'out_{int(batch)}{int(ragged)}{int(each)}')
            if runs:
                shutil.copytree(str(tmp_path / 'out_000' / 'camcalib'), os.path.join(out, 'camcalib'))
            else:
                te.run_camcalib(folder, out)
            te._render_batch, te._ragged_crops, args.render_each = batch, ragged, each
            assert te.run_on_image_folder(folder, te.run_detector(folder), out, os.path.join(out, 'pictures')) == 4
            read = lambda sub: {f: open(os.path.join(out, sub, f), 'rb').read() for f in sorted(os.listdir(os.path.join(out, sub)))}
            runs[batch, ragged, each] = (read('pictures'), {f: joblib.load(os.path.join(out, 'spec_results', f)) for f in sorted(os.listdir(os.path.join(out, 'spec_results')))})
        cams = [te._frame_camera(os.path.join(folder, n), s, str(tmp_path / 'out_000')) for n, s in zip(names, sizes)]
    finally:
        os.chdir(cwd)
    pics0, res0 = runs[False, False, False]
    assert sorted(pics0) == sorted(f'frame{k}_{i:06d}.png' for k, n in enumerate(counts) for i in range(n))
    for key, (pics, res) in runs.items():
        assert sorted(pics) == sorted(pics0) and sorted(res) == sorted(res0), key
        for f in res0:
            for k_, val in res0[f].items():
                assert res[f][k_].tobytes() == val.tobytes(), (key, f, k_)
        if not key[2]:
            assert pics == pics0, key                                         # the picture files, byte for byte
    each = runs[False, False, True][0]
    for k, n in enumerate(counts):
        rot, focal, center, cam_params = cams[k]
        rec = res0[f'frame{k}.pkl']
        frame = np.array(Image.open(os.path.join(folder, f'frame{k}.png')).convert('RGB'))
        for i in range(n):
            want = render.render_image_group(frame, t(rec['pred_cam_t'][i:i + 1]).to(DEV), t(rec['smpl_vertices'][i:i + 1]).to(DEV), rot, focal, center,
                                             cam_params=cam_params, device=DEV).cpu().numpy()
            assert np.array_equal(np.array(Image.open(str(tmp_path / 'out_001' / 'pictures' / f'frame{k}_{i:06d}.png'))), want), (k, i)
        if n > 1:
            assert each[f'frame{k}_000000.png'] != each[f'frame{k}_000001.png'] and pics0[f'frame{k}_000000.png'] == pics0[f'frame{k}_000001.png']
