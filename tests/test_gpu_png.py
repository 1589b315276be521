"""specmi_png_encode on MI355X: every device-encoded picture equals, byte for byte, tests/png_ref.py (the contract in NumPy and plain
Python, itself pinned against Pillow's and zlib's decoders by tests/test_png_host.py) and decodes through Pillow to the picture -
the smallest shapes that can go wrong and the pictures that reach the edges of the rules, ragged pictures at a foreign pitch
inside a larger slab, the capacity rule, every refusal of the C ABI, and the users against the host route."""
import functools
import io
import os
import shutil

import numpy as np
import pytest
import torch

from spec_amd import _lib, render
from spec_amd.engine import png_bound
from tests import jpeg_ref, png_ref
from tests.test_gpu_render_views import CAM_PARAMS, COUNTS, FRAMES, world  # noqa: F401  (world: a module fixture, used below)
from tests.util import gpu_models, synth_states, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0xA5

# 1x1; rows of 4 bytes; one row over two segments; a stream of exactly one segment; one segment and 4096 or 24 bytes; two contents
# at 64x1365 (eight whole segments); the pictures of png_ref.EDGES
SHAPES = {'1x1': ('noise', 1, 1), '300x1': ('smooth', 300, 1), '1x11000': ('sparse', 1, 11000), '8x1365': ('smooth', 8, 1365),
          '9x1365': ('sparse', 9, 1365), '8x1366': ('checker', 8, 1366)}
CASES = sorted(SHAPES) + sorted(png_ref.EDGES)


@pytest.fixture(scope='module')
def eng():
    from spec_amd import cam_utils
    return cam_utils._engine(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _case(name):
    """A test picture and its reference file: computed once, shared by every test that needs them, never changed."""
    a = png_ref.EDGES[name]() if name in png_ref.EDGES else jpeg_ref.picture(*SHAPES[name])
    a.setflags(write=False)
    return a, png_ref.encode(a)


def _dense(pics):
    """Pictures back to back at pitch 3 W -> (device slab, geom, offsets (n, 2))."""
    off = np.concatenate([[0], np.cumsum([p.size for p in pics])])
    slab = t(np.concatenate([p.reshape(-1) for p in pics])).to(DEV)
    return slab, [p.shape[:2] for p in pics], [(int(o), 3 * p.shape[1]) for o, p in zip(off, pics)]


def _decode(f):
    from PIL import Image
    Image.open(io.BytesIO(f)).verify()
    return np.array(Image.open(io.BytesIO(f)).convert('RGB'))


@pytest.mark.parametrize('name', CASES)
def test_device_bytes_equal_the_reference(eng, name):
    a, want = _case(name)
    got = eng.png_encode(*_dense([a]))[0]
    assert len(got) == len(want) <= png_bound(*a.shape[:2])
    assert got == want
    assert np.array_equal(_decode(got), a)


RAGGED = ('1x1', 'filters', '9x1365', 'tie', 'noise', '300x1', 'deep')


def _ragged(eng, names=RAGGED, short=None):
    """The pictures as the left third (pitch 9 W) of rows inside a larger slab with gaps, encoded by ONE call into an output slab
    with gaps, each with the bound's room (`short`: that picture one byte less than its file) -> (files cut at the reported
    sizes, the host output slab, out offsets, sizes, capacities)"""
    rng = np.random.default_rng(3)
    pics = [_case(k)[0] for k in names]
    in_off, off = [], 0
    for p in pics:
        off += 37
        in_off.append(off)
        off += (p.shape[0] - 1) * 9 * p.shape[1] + 3 * p.shape[1]
    slab = rng.integers(0, 256, off + 11, dtype=np.uint8)
    for p, o in zip(pics, in_off):
        for r in range(p.shape[0]):
            slab[o + r * 9 * p.shape[1]: o + r * 9 * p.shape[1] + 3 * p.shape[1]] = p[r].reshape(-1)
    cap = [png_bound(*p.shape[:2]) for p in pics]
    if short is not None:
        cap[short] = len(_case(names[short])[1]) - 1
    out_off = np.concatenate([[0], np.cumsum(cap)])[:-1] + 13 * (1 + np.arange(len(pics)))
    out = torch.full((int(out_off[-1] + cap[-1] + 13),), SENTINEL, dtype=torch.uint8, device=DEV)
    offsets = [(o, 9 * p.shape[1], int(oo), c) for o, p, oo, c in zip(in_off, pics, out_off, cap)]
    sizes = eng.png_encode_into(t(slab).to(DEV), out, [p.shape[:2] for p in pics], offsets).cpu().numpy()
    host = out.cpu().numpy()
    return [host[o:o + s].tobytes() for o, s in zip(out_off, sizes)], host, out_off, sizes, cap


def test_ragged_pictures_in_one_call_equal_the_single_calls(eng):
    files, host, out_off, sizes, _ = _ragged(eng)
    touched = np.zeros(host.size, bool)
    for k, f, o, s in zip(RAGGED, files, out_off, sizes):
        assert f == _case(k)[1], k                                                # == the same file alone (the test above)
        touched[o:o + s] = True
    assert (host[~touched] == SENTINEL).all() and (~touched).sum() > 13 * 8      # bytes outside the files are untouched
    again = _ragged(eng)
    assert again[0] == files and np.array_equal(again[1], host)                   # two calls, the same bytes
    assert _ragged(eng, RAGGED[::-1])[0] == files[::-1]                           # and in another order, with other neighbours


def test_a_capacity_one_byte_short_reports_the_size_and_the_bound_fits(eng):
    k = RAGGED.index('noise')
    files, host, out_off, sizes, cap = _ragged(eng, short=k)
    want = [_case(name)[1] for name in RAGGED]
    assert sizes.tolist() == [len(w) for w in want]                               # the true sizes, also of the one that did not fit
    touched = np.zeros(host.size, bool)
    for i, (o, s, c) in enumerate(zip(out_off, sizes, cap)):
        touched[o:o + min(s, c)] = True
        if i != k:
            assert files[i] == want[i], RAGGED[i]                                 # the neighbours are intact
    assert (host[~touched] == SENTINEL).all()                                     # nothing at or beyond the capacity
    assert _ragged(eng)[0] == want                                                # with the bound's room it fits


def test_refusals_of_the_c_abi(eng):
    lib = _lib.load()
    pic = jpeg_ref.picture('smooth', 16, 24)
    # one allocation, the output slab below the picture slab: a picture slab whose size is faked upwards (nothing is launched on a
    # refusal, so nothing reads it) then overlaps nothing, and the refusal is the one the case names
    buf = torch.full((16384 + 2000,), SENTINEL, dtype=torch.uint8, device=DEV)
    out, slab = buf[:16384], buf[16384:]
    slab.copy_(t(np.concatenate([pic.reshape(-1), np.zeros(848, np.uint8)])).to(DEV))     # 2000 bytes
    sizes = torch.zeros(2, dtype=torch.int64, device=DEV)
    good = dict(slab=slab.data_ptr(), in_bytes=2000, out=out.data_ptr(), out_bytes=4000, geom=[[16, 24], [9, 5]],
                offsets=[[0, 72, 0, 2000], [1152, 15, 2000, 700]], n=2, sizes=sizes.data_ptr())

    def call(a):
        geom = None if a['geom'] is None else np.asarray(a['geom'], np.int32)
        offsets = None if a['offsets'] is None else np.asarray(a['offsets'], np.int64)
        return lib.specmi_png_encode(eng.h, a['slab'], a['in_bytes'], a['out'], a['out_bytes'],
                                     None if geom is None else geom.ctypes.data_as(_lib.c_int32_p),
                                     None if offsets is None else offsets.ctypes.data_as(_lib.c_int64_p), a['n'], a['sizes'], None)

    bad = {'null slab': dict(slab=None), 'null out': dict(out=None), 'null geom': dict(geom=None), 'null offsets': dict(offsets=None),
           'null sizes': dict(sizes=None), 'n 0': dict(n=0), 'n 65536': dict(n=65536),
           'H 0': dict(geom=[[0, 24], [9, 5]]), 'W 32769': dict(geom=[[16, 24], [9, 32769]]),
           'pitch': dict(offsets=[[0, 71, 0, 2000], [1152, 15, 2000, 700]]),
           'leaves the slab': dict(offsets=[[0, 72, 0, 2000], [1866, 15, 2000, 700]]),
           'capacity below the overhead': dict(offsets=[[0, 72, 0, 2000], [1152, 15, 2000, 62]]),
           'output leaves the slab': dict(out_bytes=2699),
           'overlapping slabs': dict(out=slab.data_ptr() + 1000, out_bytes=1000, offsets=[[0, 72, 0, 700]], geom=[[4, 24]], n=1),
           'outputs share a byte': dict(offsets=[[0, 72, 0, 2001], [1152, 15, 2000, 700]]),
           'IDAT beyond 2^31': dict(geom=[[32768, 32768]], offsets=[[0, 98304, 0, 4000]], n=1, in_bytes=32768 * 98304),
           # 129 pictures of 65513 segments each: more than 2^23 workgroups of the per-segment launches
           'segments beyond 2^23': dict(geom=[[26750, 26750]] * 129, offsets=[[0, 80250, 63 * i, 63] for i in range(129)], n=129,
                                        in_bytes=3 * 26750 * 26750, out_bytes=16384)}
    says = {'IDAT beyond 2^31': b'one IDAT chunk', 'segments beyond 2^23': b'2^23 segments', 'overlapping slabs': b'overlap'}
    for name, change in bad.items():
        assert call({**good, **change}) == _lib.ERR_ARG, name
        assert says.get(name, b'') in lib.specmi_last_error(eng.h), name
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                                # nothing was launched
    assert call(good) == _lib.OK                                                  # and the handle serves the next call
    n0, n1 = sizes.tolist()
    host = out.cpu().numpy()
    assert host[:n0].tobytes() == png_ref.encode(pic) and host[2000:2000 + n1].tobytes() == png_ref.encode(np.zeros((9, 5, 3), np.uint8))
    assert (host[n0:2000] == SENTINEL).all() and (host[2000 + n1:] == SENTINEL).all()


def test_more_rows_than_the_filter_launch_has_workgroups(eng):
    # 34 pictures of 32768 x 1: 1114112 rows against a grid capped at 2^20, so the last two pictures' rows are second rows of their
    # workgroups.  Three contents, three reference files
    pics = [jpeg_ref.picture('sparse', 32768, 1, seed=k) for k in (0, 1, 2)]
    order = [0] * 32 + [1, 2]
    assert 32 * 32768 == 1 << 20
    want = [png_ref.encode(p) for p in pics]
    files = eng.png_encode(*_dense([pics[k] for k in order]))
    assert files == [want[k] for k in order] and len(set(want)) == 3


def test_a_repeated_call_replays_from_a_graph(eng):
    pics = [_case('filters')[0], _case('tie')[0]]
    slab, geom, off = _dense(pics)
    cap = [png_bound(*g) for g in geom]
    offsets = [off[0] + (0, cap[0]), off[1] + (cap[0], cap[1])]
    out = torch.zeros(sum(cap), dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(2, dtype=torch.int64, device=DEV)
    eng.png_encode_into(slab, out, geom, offsets, sizes=sizes)                    # also the warm-up call of the capture below
    want, want_sizes = out.clone(), sizes.clone()
    assert out[:int(sizes[0])].cpu().numpy().tobytes() == _case('filters')[1]
    out.zero_(), sizes.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):
        try:      # other records are another table: refused, and the capture goes on
            eng.png_encode_into(slab, out, geom[:1], offsets[:1], sizes=sizes[:1])
        except _lib.SpecmiError as e:
            err = e
        eng.png_encode_into(slab, out, geom, offsets, sizes=sizes)                # the previous call's records: captured
    assert err is not None and err.code == _lib.ERR_STATE, err
    torch.cuda.synchronize()
    assert not out.any() and not sizes.any()                                      # capturing ran nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(sizes, want_sizes)
        out.zero_()


# ---- the users ----------------------------------------------------------------------------------------------------------------
def _pillow(a):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, format='PNG')
    return f.getvalue()


def test_save_picture_writes_a_png_that_decodes_to_the_picture(eng, tmp_path):
    a = _case('filters')[0]
    on, off, other = (str(tmp_path / n) for n in ('on.png', 'off.png', 'on.jpg'))
    pic = t(a.copy()).to(DEV)
    render.save_picture(on, pic, engine=eng, png_device=True)
    render.save_picture(off, pic, engine=eng)                                     # the default: off, the parent's route
    render.save_picture(other, pic, engine=eng, png_device=True, jpeg_device=False)
    assert open(on, 'rb').read() == _case('filters')[1] and open(off, 'rb').read() == _pillow(a)
    assert open(other, 'rb').read()[:2] == b'\xff\xd8'                            # the switch touches .png names only


def test_render_image_groups_encodes_pngs_that_decode_to_the_arrays(world):  # noqa: F811
    kw = dict(faces=FRAMES[0]['f'], cam_params=CAM_PARAMS, engine=world['eng'])
    args = (world['frames'], world['v'], world['t'], COUNTS, world['R'], world['focal'], world['center'])
    arrays = render.render_image_groups(*args, **kw)
    files = render.render_image_groups(*args, encode='png', **kw)
    assert [type(f) for f in files] == [bytes] * 3
    for a, f in zip(arrays, files):
        assert np.array_equal(_decode(f), a) and f == png_ref.encode(a)
    mixed = render.render_image_groups(*args, encode=['png', None, 'jpeg'], each=True, **kw)
    each = render.render_image_groups(*args, each=True, **kw)
    frame_of = [f for f, n in enumerate(COUNTS) for _ in range(n)]
    for f, a, m in zip(frame_of, each, mixed):
        assert (np.array_equal(_decode(m), a) if f == 0 else np.array_equal(m, a) if f == 1 else m == jpeg_ref.encode(a, 75)), f


def test_demo_flow_writes_png_files_that_decode_to_the_host_runs(tmp_path):
    from types import SimpleNamespace
    from PIL import Image
    from spec_amd import evaluation
    from spec_amd.tester import SPECTester
    tree = str(tmp_path / 'tree')
    evaluation.write_standin_data_tree(tree, n_images=1)
    folder = str(tmp_path / 'frames')
    os.makedirs(folder)
    rng = np.random.default_rng(6)
    sizes, counts = [(96, 128), (120, 90), (97, 131)], [2, 1, 1]
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, f'frame{k}.png'))
    dets = [np.stack([rng.uniform(0.3 * w, 0.7 * w, n), rng.uniform(0.3 * h, 0.7 * h, n), rng.uniform(40, 80, n), rng.uniform(40, 80, n)], 1)
            .astype(np.float32) for (h, w), n in zip(sizes, counts)]
    hs = {k_: t(v) for k_, v in synth_states(True)[1].items()}
    args = SimpleNamespace(cfg=None, ckpt=hs, no_save=False, no_render=False, save_obj=False, synthetic_assets=True, frame_batch=4, plan='throughput',
                           decode_threads=2, camcalib_model=gpu_models(True, True, DEV)[0], detections=dets, render_each=False)
    cwd = os.getcwd()
    os.chdir(tree)
    try:
        te = SPECTester(args)
        runs, results = {}, {}
        for batch, on in ((False, None), (False, True), (True, True)):
            out = str(tmp_path / f'out_{int(batch)}{int(bool(on))}')
            if runs:
                shutil.copytree(str(tmp_path / 'out_00' / 'camcalib'), os.path.join(out, 'camcalib'))
            else:
                te.run_camcalib(folder, out)
            te._render_batch, te._png_device = batch, on
            assert te.run_on_image_folder(folder, te.run_detector(folder), out, os.path.join(out, 'pictures')) == 3
            runs[batch, on] = {f: open(os.path.join(out, 'pictures', f), 'rb').read() for f in sorted(os.listdir(os.path.join(out, 'pictures')))}
            results[batch, on] = {f: open(os.path.join(out, 'spec_results', f), 'rb').read() for f in sorted(os.listdir(os.path.join(out, 'spec_results')))}
    finally:
        os.chdir(cwd)
    host = runs[False, None]
    assert sorted(host) == sorted(f'frame{k}_{i:06d}.png' for k, n in enumerate(counts) for i in range(n))
    assert sorted(results[False, None]) == ['frame0.pkl', 'frame1.pkl', 'frame2.pkl']
    for name, f in host.items():
        a = _decode(f)
        assert f == _pillow(a), name                                              # the switch off: the parent route's bytes
        for run in ((False, True), (True, True)):
            assert runs[run][name] == png_ref.encode(a) != f and np.array_equal(_decode(runs[run][name]), a), (run, name)
    assert results[False, True] == results[False, None] and results[True, True] == results[False, None]


def test_write_tree_writes_png_views_that_decode_to_the_host_routes(tmp_path):
    from PIL import Image
    from spec_amd import panorama
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:64, 0:128]
    pano = np.stack([127 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 + c) for c in range(3)], -1)
    pano = np.clip(pano + rng.normal(0, 10, pano.shape), 0, 255).astype(np.uint8)
    os.makedirs(tmp_path / 'panos')
    Image.fromarray(pano).save(str(tmp_path / 'panos' / 'scene.png'))
    ds = panorama.PanoViewDataset([str(tmp_path / 'panos' / 'scene.png')], views_per_pano=3, seed=17, device=DEV)
    folders = [panorama.write_tree(ds, str(tmp_path / name), image_format='PNG', log=lambda s: None, png_device=on)
               for name, on in (('host', None), ('device', True))]
    names = sorted(n for n in os.listdir(os.path.join(folders[0], 'images')) if n.endswith('.jpg'))
    assert len(names) == 3 and sorted(os.listdir(os.path.join(folders[0], 'images'))) == sorted(os.listdir(os.path.join(folders[1], 'images')))
    for n in names:
        a, b = (open(os.path.join(f, 'images', n), 'rb').read() for f in folders)
        view = _decode(a)
        assert a == _pillow(view) and b == png_ref.encode(view), n               # off: Pillow's file as before; on: the contract's
