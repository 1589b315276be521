"""specmi_jpeg_encode on MI355X: every device-encoded picture equals, byte for byte, tests/jpeg_ref.py (the contract in NumPy,
itself pinned against Pillow's own bytes by tests/test_jpeg_host.py) - the size x content list, the quality list, ragged pictures
at a foreign pitch inside a larger slab, the capacity rule, every refusal of the C ABI, the table rule under graph capture, and
the users: ``render_image_groups(encode='jpeg')``, the demo flow and ``write_tree`` against the host route.  Every comparison is
== on bytes."""
import functools
import io
import os
import shutil

import numpy as np
import pytest
import torch

from spec_amd import _lib, panorama, render
from spec_amd.engine import jpeg_capacity
from tests import jpeg_ref
from tests.test_gpu_render_views import CAM_PARAMS, COUNTS, FRAMES, world  # noqa: F401  (world: a module fixture, used below)
from tests.util import gpu_models, synth_states, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def eng():
    from spec_amd import cam_utils
    return cam_utils._engine(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _ref(content, H, W, q):
    """The reference file of a test picture: computed once, shared by every test that needs it."""
    return jpeg_ref.encode(jpeg_ref.picture(content, H, W), q)


def _dense(pics):
    """Pictures back to back at pitch 3 W -> (device slab, geom, offsets (n, 2))."""
    off = np.concatenate([[0], np.cumsum([p.size for p in pics])])
    slab = t(np.concatenate([p.reshape(-1) for p in pics])).to(DEV)
    return slab, [p.shape[:2] for p in pics], [(int(o), 3 * p.shape[1]) for o, p in zip(off, pics)]


@pytest.mark.parametrize('q', [75, 95])
@pytest.mark.parametrize('size', jpeg_ref.SIZES, ids=lambda s: '%dx%d' % s)
def test_device_bytes_equal_the_reference(eng, size, q):
    pics = [jpeg_ref.picture(c, *size) for c in jpeg_ref.CONTENTS]
    files = eng.jpeg_encode(*_dense(pics), q)
    for c, f in zip(jpeg_ref.CONTENTS, files):
        assert f == _ref(c, *size, q), c


@pytest.mark.parametrize('q', jpeg_ref.QUALITIES)
def test_every_quality_at_40x56(eng, q):
    for c in jpeg_ref.CONTENTS:
        assert eng.jpeg_encode(*_dense([jpeg_ref.picture(c, 40, 56)]), q)[0] == _ref(c, 40, 56, q), c


def _ragged(eng):
    """Ten pictures of different sizes as the left third (pitch 9 W) of rows inside a larger slab with gaps, encoded by ONE call
    into an output slab with gaps -> (files cut at the reported sizes, the host output slab, out offsets, capacities, pictures)"""
    rng = np.random.default_rng(3)
    pics = [jpeg_ref.picture(jpeg_ref.CONTENTS[k % 6], H, W, seed=k) for k, (H, W) in enumerate(jpeg_ref.SIZES)]
    in_off, off = [], 0
    for p in pics:
        off += 37
        in_off.append(off)
        off += (p.shape[0] - 1) * 9 * p.shape[1] + 3 * p.shape[1]
    slab = rng.integers(0, 256, off + 11, dtype=np.uint8)
    for p, o in zip(pics, in_off):
        for r in range(p.shape[0]):
            slab[o + r * 9 * p.shape[1]: o + r * 9 * p.shape[1] + 3 * p.shape[1]] = p[r].reshape(-1)
    cap = [jpeg_capacity(*p.shape[:2]) for p in pics]
    out_off = np.concatenate([[0], np.cumsum(cap)])[:-1] + 13 * (1 + np.arange(len(pics)))
    out = torch.full((int(out_off[-1] + cap[-1] + 13),), SENTINEL, dtype=torch.uint8, device=DEV)
    offsets = [(o, 9 * p.shape[1], int(oo), c) for o, p, oo, c in zip(in_off, pics, out_off, cap)]
    sizes = eng.jpeg_encode_into(t(slab).to(DEV), out, [p.shape[:2] for p in pics], offsets, 75).cpu().numpy()
    host = out.cpu().numpy()
    return [host[o:o + s].tobytes() for o, s in zip(out_off, sizes)], host, out_off, sizes, pics


def test_ten_ragged_pictures_in_one_call_equal_the_single_calls(eng):
    files, host, out_off, sizes, pics = _ragged(eng)
    assert len({p.shape[:2] for p in pics}) == 10
    touched = np.zeros(host.size, bool)
    for k, (p, f, o, s) in enumerate(zip(pics, files, out_off, sizes)):
        assert f == eng.jpeg_encode(*_dense([p]), 75)[0] == jpeg_ref.encode(p, 75), k
        touched[o:o + s] = True
    assert (host[~touched] == SENTINEL).all() and (~touched).sum() > 130          # bytes outside the outputs are untouched


def test_pillow_opens_every_output(eng):
    from PIL import Image, JpegImagePlugin
    files, _, _, _, pics = _ragged(eng)
    for p, f in zip(pics, files):
        im = Image.open(io.BytesIO(f))
        assert im.format == 'JPEG' and im.mode == 'RGB' and im.size == (p.shape[1], p.shape[0])
        assert JpegImagePlugin.get_sampling(im) == 2                              # 4:2:0
        im.load()
        assert np.asarray(im).shape == p.shape


def test_a_capacity_one_byte_short_reports_the_size_and_the_retry_succeeds(eng, monkeypatch):
    pic = jpeg_ref.picture('noise', 33, 47)
    want = _ref('noise', 33, 47, 95)
    slab, geom, off = _dense([pic])
    out = torch.full((len(want) + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    sizes = eng.jpeg_encode_into(slab, out, geom, [off[0] + (16, len(want) - 1)], 95)
    assert sizes.tolist() == [len(want)]                                          # the true size
    host = out.cpu().numpy()
    assert (host[:16] == SENTINEL).all() and (host[16 + len(want) - 1:] == SENTINEL).all()        # nothing beyond the capacity
    sizes = eng.jpeg_encode_into(slab, out, geom, [off[0] + (16, len(want))], 95)
    assert sizes.tolist() == [len(want)] and out[16:16 + len(want)].cpu().numpy().tobytes() == want
    # the binding's own retry, with its first guess made too small for two of three pictures
    from spec_amd import engine
    monkeypatch.setattr(engine, 'jpeg_capacity', lambda H, W: 700)
    big, one = jpeg_ref.picture('noise', 65, 130), jpeg_ref.picture('zeros', 1, 1)
    assert len(_ref('zeros', 1, 1, 100)) <= 700 < len(_ref('noise', 33, 47, 100))
    assert eng.jpeg_encode(*_dense([big, one, pic]), 100) == [_ref('noise', 65, 130, 100), _ref('zeros', 1, 1, 100), _ref('noise', 33, 47, 100)]


def test_refusals_of_the_c_abi(eng):
    lib = _lib.load()
    pic = jpeg_ref.picture('smooth', 16, 24)
    slab = t(np.concatenate([pic.reshape(-1), np.zeros(848, np.uint8)])).to(DEV)          # 2000 bytes
    out = torch.full((4000,), SENTINEL, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(2, dtype=torch.int64, device=DEV)
    good = dict(slab=slab.data_ptr(), in_bytes=2000, out=out.data_ptr(), out_bytes=4000, geom=[[16, 24], [9, 5]],
                offsets=[[0, 72, 0, 2000], [1152, 15, 2000, 700]], n=2, q=75, sizes=sizes.data_ptr())

    def call(a):
        geom = None if a['geom'] is None else np.asarray(a['geom'], np.int32)
        offsets = None if a['offsets'] is None else np.asarray(a['offsets'], np.int64)
        return lib.specmi_jpeg_encode(eng.h, a['slab'], a['in_bytes'], a['out'], a['out_bytes'],
                                      None if geom is None else geom.ctypes.data_as(_lib.c_int32_p),
                                      None if offsets is None else offsets.ctypes.data_as(_lib.c_int64_p), a['n'], a['q'], a['sizes'], None)

    bad = {'null slab': dict(slab=None), 'null out': dict(out=None), 'null geom': dict(geom=None), 'null offsets': dict(offsets=None),
           'null sizes': dict(sizes=None), 'n 0': dict(n=0), 'n 65536': dict(n=65536), 'q 0': dict(q=0), 'q 101': dict(q=101),
           'H 0': dict(geom=[[0, 24], [9, 5]]), 'W 32769': dict(geom=[[16, 24], [9, 32769]]),
           'pitch': dict(offsets=[[0, 71, 0, 2000], [1152, 15, 2000, 700]]),
           'leaves the slab': dict(offsets=[[0, 72, 0, 2000], [1866, 15, 2000, 700]]),
           'capacity below the header': dict(offsets=[[0, 72, 0, 2000], [1152, 15, 2000, 622]]),
           'output leaves the slab': dict(out_bytes=2699),
           'overlapping slabs': dict(out=slab.data_ptr() + 1000, out_bytes=1000, offsets=[[0, 72, 0, 700]], geom=[[4, 24]], n=1),
           'outputs share a byte': dict(offsets=[[0, 72, 0, 2001], [1152, 15, 2000, 700]])}
    for name, change in bad.items():
        assert call({**good, **change}) == _lib.ERR_ARG, name
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                                # nothing was launched
    assert call(good) == _lib.OK                                                  # and the handle serves the next call
    n0, n1 = sizes.tolist()
    host = out.cpu().numpy()
    assert host[:n0].tobytes() == jpeg_ref.encode(pic, 75) and n1 > 623 and (host[2000 + n1:2700] == SENTINEL).all()


def test_a_repeated_call_replays_from_a_graph(eng):
    pics = [jpeg_ref.picture('noise', 33, 47), jpeg_ref.picture('sparse', 40, 56)]
    slab, geom, off = _dense(pics)
    cap = [jpeg_capacity(*g) for g in geom]
    offsets = [off[0] + (0, cap[0]), off[1] + (cap[0], cap[1])]
    out = torch.zeros(sum(cap), dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(2, dtype=torch.int64, device=DEV)
    eng.jpeg_encode_into(slab, out, geom, offsets, 95, sizes=sizes)               # also the warm-up call of the capture below
    want, want_sizes = out.clone(), sizes.clone()
    assert out[:int(sizes[0])].cpu().numpy().tobytes() == _ref('noise', 33, 47, 95)
    out.zero_(), sizes.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):
        try:      # another quality is another table: refused, and the capture goes on
            eng.jpeg_encode_into(slab, out, geom, offsets, 75, sizes=sizes)
        except _lib.SpecmiError as e:
            err = e
        eng.jpeg_encode_into(slab, out, geom, offsets, 95, sizes=sizes)           # the previous call's records: captured
    assert err is not None and err.code == _lib.ERR_STATE, err
    torch.cuda.synchronize()
    assert not out.any() and not sizes.any()                                      # capturing ran nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(sizes, want_sizes)
        out.zero_()


# ---- the users ----------------------------------------------------------------------------------------------------------------
def _pillow(a, **kw):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, format='JPEG', **kw)
    return f.getvalue()


def test_render_image_groups_encodes_what_pillow_saves(world):  # noqa: F811
    kw = dict(faces=FRAMES[0]['f'], cam_params=CAM_PARAMS, engine=world['eng'])
    args = (world['frames'], world['v'], world['t'], COUNTS, world['R'], world['focal'], world['center'])
    arrays = render.render_image_groups(*args, **kw)
    files = render.render_image_groups(*args, encode='jpeg', **kw)
    assert [type(f) for f in files] == [bytes] * 3
    for a, f in zip(arrays, files):
        assert f == _pillow(a) == jpeg_ref.encode(a, 75)
    mixed = render.render_image_groups(*args, encode=['jpeg', None, 'jpeg'], quality=95, each=True, **kw)
    each = render.render_image_groups(*args, each=True, **kw)
    frame_of = [f for f, n in enumerate(COUNTS) for _ in range(n)]
    for f, a, m in zip(frame_of, each, mixed):
        assert (np.array_equal(m, a) if f == 1 else m == _pillow(a, quality=95)), f


def test_write_tree_on_the_device_equals_the_host_route(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:64, 0:128]
    pano = np.stack([127 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 + c) for c in range(3)], -1)
    pano = np.clip(pano + rng.normal(0, 10, pano.shape), 0, 255).astype(np.uint8)
    os.makedirs(tmp_path / 'panos')
    Image.fromarray(pano).save(str(tmp_path / 'panos' / 'scene.png'))
    ds = panorama.PanoViewDataset([str(tmp_path / 'panos' / 'scene.png')], views_per_pano=3, seed=17, device=DEV)
    folders = [panorama.write_tree(ds, str(tmp_path / name), log=lambda s: None, jpeg_device=on) for name, on in (('host', False), ('device', True))]
    names = sorted(os.listdir(os.path.join(folders[0], 'images')))
    assert names == sorted(os.listdir(os.path.join(folders[1], 'images'))) and sum(n.endswith('.jpg') for n in names) == 3
    for n in (n for n in names if n.endswith('.jpg')):
        a, b = (open(os.path.join(f, 'images', n), 'rb').read() for f in folders)
        assert a == b and a[:2] == b'\xff\xd8', n


def test_demo_flow_writes_the_same_jpg_files_with_the_switch_on(tmp_path):
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
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, f'frame{k}.jpg'))
    dets = [np.stack([rng.uniform(0.3 * w, 0.7 * w, n), rng.uniform(0.3 * h, 0.7 * h, n), rng.uniform(40, 80, n), rng.uniform(40, 80, n)], 1)
            .astype(np.float32) for (h, w), n in zip(sizes, counts)]
    hs = {k_: t(v) for k_, v in synth_states(True)[1].items()}
    args = SimpleNamespace(cfg=None, ckpt=hs, no_save=True, no_render=False, save_obj=False, synthetic_assets=True, frame_batch=4, plan='throughput',
                           decode_threads=2, camcalib_model=gpu_models(True, True, DEV)[0], detections=dets, render_each=False)
    cwd = os.getcwd()
    os.chdir(tree)
    try:
        te = SPECTester(args)
        runs = {}
        for batch, on in ((False, False), (False, True), (True, True)):
            out = str(tmp_path / f'out_{int(batch)}{int(on)}')
            if runs:
                shutil.copytree(str(tmp_path / 'out_00' / 'camcalib'), os.path.join(out, 'camcalib'))
            else:
                te.run_camcalib(folder, out)
            te._render_batch, te._jpeg_device = batch, on
            assert te.run_on_image_folder(folder, te.run_detector(folder), out, os.path.join(out, 'pictures')) == 3
            runs[batch, on] = {f: open(os.path.join(out, 'pictures', f), 'rb').read() for f in sorted(os.listdir(os.path.join(out, 'pictures')))}
    finally:
        os.chdir(cwd)
    host = runs[False, False]
    assert sorted(host) == sorted(f'frame{k}_{i:06d}.jpg' for k, n in enumerate(counts) for i in range(n))
    assert runs[False, True] == host and runs[True, True] == host                 # the files, byte for byte
    assert host['frame0_000000.jpg'] == host['frame0_000001.jpg'] and host['frame0_000000.jpg'][:2] == b'\xff\xd8'
