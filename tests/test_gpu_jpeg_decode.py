"""specmi_jpeg_decode on MI355X: every device-decoded file equals, element for element, what Pillow decodes (and the coefficients
tests/jpeg_dec_ref.py decodes, itself pinned against Pillow by tests/test_jpeg_decode_host.py) - the whole size x content x
quality set in one call, 4:4:4 / optimised tables / custom quantisers, a periodic scan across workgroups, independence of the
batch and the slab layout, every refusal of the C ABI, damaged scans, and ``preprocess.decode_frames`` against the host route."""
import functools
import os

import numpy as np
import pytest
import torch

from spec_amd import _lib, preprocess
from spec_amd.engine import jpeg_probe
from tests import jpeg_dec_ref as ref
from tests import jpeg_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def eng():
    from spec_amd import cam_utils
    return cam_utils._engine(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _files():
    return ref.file_set()


def _blocks(data):
    info = ref.probe(data)
    my, mx, bpm, _ = ref.geometry(info['H'], info['W'], info['s420'])
    return my * mx * bpm


def _decode(eng, files, gap=0, extra_pitch=0, coef=False):
    """One call on ``files`` -> (pictures as host arrays, status, passes, host output slab, rectangles, coefficients or None).  The
    files lie ``gap`` bytes apart in their slab; the pictures ``gap`` bytes apart at pitch 3 W + ``extra_pitch`` in a slab filled
    with SENTINEL."""
    probes = [jpeg_probe(f) for f in files]
    assert all(p[0] == 'supported' for p in probes)
    ranges, blob = [], b''
    for f in files:
        blob += bytes([0x5A]) * gap
        ranges.append((len(blob), len(f)))
        blob += f
    blob += bytes([0x5A]) * gap
    host = np.frombuffer(blob, np.uint8)
    geom = np.array([p[1:] for p in probes], np.int64)
    outs, at = [], 0
    for H, W, _ in geom:
        at += gap
        outs.append((at, 3 * W + extra_pitch))
        at += (H - 1) * (3 * W + extra_pitch) + 3 * W
    out_slab = torch.full((int(at + gap),), SENTINEL, device=DEV, dtype=torch.uint8)
    cbuf = torch.empty(sum(_blocks(f) for f in files), 64, device=DEV, dtype=torch.int16) if coef else None
    status, passes = eng.jpeg_decode_into(host, torch.from_numpy(host.copy()).to(DEV), ranges, geom, out_slab, outs, coef=cbuf)
    o = out_slab.cpu().numpy()
    pics = [np.lib.stride_tricks.as_strided(o[off:], (H, W, 3), (pitch, 3, 1)).copy() for (off, pitch), (H, W, _) in zip(outs, geom)]
    return pics, status.cpu().numpy(), passes, o, [(off, pitch, int(H), int(W)) for (off, pitch), (H, W, _) in zip(outs, geom)], cbuf


def _untouched(o, rects):
    """Every byte of the host slab ``o`` outside the rectangles still holds SENTINEL."""
    mask = np.ones(o.size, bool)
    for off, pitch, H, W in rects:
        for y in range(H):
            mask[off + y * pitch:off + y * pitch + 3 * W] = False
    return bool((o[mask] == SENTINEL).all())


def test_the_whole_set_in_one_call(eng):
    """(a) 600 files, one call: Pillow's pixels, status 0, nothing left to the host route; the coefficients are the reference's."""
    names, files = zip(*_files())
    pics, status, passes, o, rects, coef = _decode(eng, list(files), gap=5, coef=True)
    assert not status.any() and passes == 1
    for name, f, px in zip(names, files, pics):
        assert np.array_equal(px, ref.pillow_pixels(f)), name
    assert _untouched(o, rects)
    coef, at = coef.cpu().numpy(), 0
    for name, f in zip(names, files):
        want = ref.entropy_decode(f, ref.probe(f))[0]
        assert np.array_equal(coef[at:at + len(want)], want), name
        at += len(want)
    slab, offsets, sizes, st = eng.jpeg_decode(list(files[:40]))
    assert not st.any().item() and sizes == [p.shape[:2] for p in pics[:40]]
    assert torch.equal(slab.cpu(), torch.from_numpy(np.concatenate([p.reshape(-1) for p in pics[:40]])))
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([p.size for p in pics[:40]])[:-1]]).tolist()


def test_variants(eng):
    """(b) 4:4:4, optimised Huffman tables, custom quantisers."""
    names, files = zip(*ref.variant_set())
    pics, status, _, o, rects, _ = _decode(eng, list(files), gap=3)
    assert not status.any() and _untouched(o, rects)
    for name, f, px in zip(names, files, pics):
        assert np.array_equal(px, ref.pillow_pixels(f)), name


def test_periodic_scan_across_groups(eng):
    """(c) A constant picture's scan never corrects a wrong phase: the truth advances one GROUP of 256 subsequences per pass.
    2560 x 2560 zeros is 800 subsequences, four groups; a natural-like picture of two groups beside it must not be disturbed by
    the passes the other one needs."""
    zeros = ref.pillow_save(np.zeros((2560, 2560, 3), np.uint8), quality=75)
    s0, s1 = ref.probe(zeros)['scan']
    groups = -(-(-(-(s1 - s0) // 128)) // ref.GROUP)
    assert groups >= 3
    yy, xx = np.mgrid[0:400, 0:500]
    rng = np.random.default_rng(11)
    nat = np.clip(128 + 90 * np.sin(yy / 37.0)[..., None] * np.cos(xx / 53.0)[..., None] + rng.normal(0, 6, (400, 500, 3)), 0, 255).astype(np.uint8)
    natf = ref.pillow_save(nat, quality=95)
    pics, status, passes, _, _, _ = _decode(eng, [zeros, natf])
    assert not status.any() and 2 <= passes <= groups
    assert np.array_equal(pics[0], ref.pillow_pixels(zeros))
    assert np.array_equal(pics[1], ref.pillow_pixels(natf))


def test_a_file_does_not_depend_on_its_batch(eng):
    """(d) Alone, in the batch, in reversed order, at another slab offset and pitch: the same bytes; sentinels untouched."""
    files = [f for _, f in _files()[3::61]] + [f for _, f in ref.variant_set()[::7]]
    base, status, _, o, rects, _ = _decode(eng, files)
    assert not status.any() and _untouched(o, rects)
    rev, status, _, o, rects, _ = _decode(eng, files[::-1], gap=11, extra_pitch=7)
    assert not status.any() and _untouched(o, rects)
    for a, b in zip(base, rev[::-1]):
        assert np.array_equal(a, b)
    for k in (0, len(files) // 2, len(files) - 1):
        alone, status, _, o, rects, _ = _decode(eng, [files[k]], gap=2, extra_pitch=1)
        assert not status.any() and _untouched(o, rects) and np.array_equal(alone[0], base[k])


def test_refusals(eng):
    """(e) SPECMI_ERR_ARG, nothing launched, the slab untouched, the handle usable afterwards."""
    good = _files()[100][1]
    other = _files()[200][1]
    H, W = jpeg_probe(good)[1:3]
    H2, W2 = jpeg_probe(other)[1:3]
    blob = np.frombuffer(good + other, np.uint8)
    dev_in = torch.from_numpy(blob.copy()).to(DEV)
    out = torch.full((3 * H * W + 3 * H2 * W2 + 64,), SENTINEL, device=DEV, dtype=torch.uint8)
    st = torch.full((2,), 77, device=DEV, dtype=torch.int32)
    progressive = np.frombuffer(ref.pillow_save(jpeg_ref.picture('noise', 16, 16), progressive=True), np.uint8)

    def call(host=blob, slab=dev_in, in_bytes=None, ranges=((0, len(good)), (len(good), len(other))), out_slab=out, out_bytes=None,
             outs=((0, 3 * W), (3 * H * W, 3 * W2)), n=2, status=st, coef=None, coef_bytes=0):
        r = None if ranges is None else np.ascontiguousarray(ranges, dtype=np.int64)
        o = None if outs is None else np.ascontiguousarray(outs, dtype=np.int64)
        ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)
        rows = lambda x: None if x is None else x.ctypes.data_as(_lib.c_int64_p)
        return eng.lib.specmi_jpeg_decode(eng.h, ptr(host), ptr(slab), dev_in.numel() if in_bytes is None else in_bytes, rows(r), ptr(out_slab),
                                          out.numel() if out_bytes is None else out_bytes, rows(o), n, ptr(status), ptr(coef), coef_bytes, None, None)

    small = torch.empty(8, device=DEV, dtype=torch.int16)
    prog_dev = torch.from_numpy(progressive.copy()).to(DEV)
    # five files whose frame header claims 32768 x 32768 (2^22 MCUs each): nothing is launched, so the output slab is only stated -
    # 15 GiB from the first address behind the input slab, which no byte of it is ever written to
    huge = bytearray(good)
    at = 163                                                              # H and W in the 623-byte header (tests/jpeg_ref.header)
    assert bytes(huge[at - 5:at - 3]) == b'\xff\xc0'
    huge[at:at + 4] = bytes([0x80, 0x00, 0x80, 0x00])
    huge = np.frombuffer(bytes(huge), np.uint8)
    assert jpeg_probe(huge.tobytes()) == ('supported', 32768, 32768, 420)
    huge_dev = torch.from_numpy(huge.copy()).to(DEV)
    one = 3 * 32768 * 32768
    too_many = dict(host=huge, slab=huge_dev, in_bytes=huge.size, ranges=[(0, huge.size)] * 5, out_slab=huge_dev.data_ptr() + huge.size,
                    out_bytes=5 * one, outs=[(k * one, 3 * 32768) for k in range(5)], n=5, status=torch.full((5,), 77, device=DEV, dtype=torch.int32))
    bad = {
        'null host bytes': dict(host=None), 'null status': dict(status=None), 'n 0': dict(n=0), 'n 65536': dict(n=65536),
        'null file slab': dict(slab=None), 'null output slab': dict(out_slab=None), 'null file ranges': dict(ranges=None),
        'null output offsets': dict(outs=None), 'more than 2^24 MCUs': too_many,
        'file leaves the slab': dict(in_bytes=len(good) + len(other) - 1),
        'negative range': dict(ranges=((-1, len(good)), (len(good), len(other)))),
        'pitch below 3 W': dict(outs=((0, 3 * W - 1), (3 * H * W, 3 * W2))),
        'rectangle leaves the slab': dict(out_bytes=3 * H * W + 3 * H2 * W2 - 1),
        'rectangles share a byte': dict(outs=((0, 3 * W), (3 * H * W - 1, 3 * W2))),
        'overlapping slabs': dict(out_slab=dev_in, outs=((0, 3), (0, 3))),
        'a file the probe refuses': dict(host=progressive, slab=prog_dev, ranges=((0, progressive.size),), outs=((0, 48),), n=1),
        'a range that is no file': dict(ranges=((1, len(good) - 1), (len(good), len(other)))),
        'coefficient output too small': dict(coef=small, coef_bytes=16),
    }
    for name, kw in bad.items():
        assert call(**kw) == _lib.ERR_ARG, name
        assert eng.lib.specmi_last_error(eng.h), name
        if name == 'more than 2^24 MCUs':
            assert b'2^24 MCUs' in eng.lib.specmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (st.cpu().numpy() == 77).all()
    probe = torch.zeros(4, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):                                   # under capture: asked first, the capture stays valid
        try:
            eng.jpeg_decode_into(blob, dev_in, [(0, len(good))], [(H, W, 420)], out, [(0, 3 * W)], status=st[:1])
        except _lib.SpecmiError as e:
            err = e
        probe.add_(1)
    assert err is not None and err.code == _lib.ERR_STATE, err
    g.replay()
    torch.cuda.synchronize()
    assert probe.tolist() == [1, 1, 1, 1]
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert call() == _lib.OK                                              # the handle is usable
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    o = out.cpu().numpy()
    assert np.array_equal(o[:3 * H * W].reshape(H, W, 3), ref.pillow_pixels(good))
    assert np.array_equal(o[3 * H * W:3 * H * W + 3 * H2 * W2].reshape(H2, W2, 3), ref.pillow_pixels(other))
    assert (o[3 * H * W + 3 * H2 * W2:] == SENTINEL).all()


def _damaged():
    d = jpeg_ref.encode(jpeg_ref.picture('noise', 65, 130), 95)
    s0, s1 = ref.probe(d)['scan']
    rng = np.random.default_rng(5)
    return d, {'cut inside the scan': d[:s0 + (s1 - s0) // 2] + b'\xff\xd9',
               'seeded noise': d[:s0] + rng.integers(0, 255, s1 - s0, dtype=np.uint8).tobytes() + b'\xff\xd9',
               'all 0xFF': d[:s0] + b'\xff' * (s1 - s0) + b'\xff\xd9',
               'all zero': d[:s0] + b'\x00' * (s1 - s0) + b'\xff\xd9',
               'no scan': d[:s0] + b'\xff\xd9',
               'a second scan behind the first': d[:s1] + d[s0:s1] + b'\xff\xd9'}


def test_damaged_scans(eng, tmp_path):
    """(f) The status is non-zero exactly where the reference's is (every one of these breaks rule 2), nothing is written outside
    the rectangles, the sound file beside them is Pillow's; ``decode_frames`` then does what the host route does."""
    good, bad = _damaged()
    files = [bad[k] for k in bad] + [good]
    want = [ref.entropy_decode(f, ref.probe(f))[2] for f in files]
    assert all(want[:-1]) and not want[-1]
    pics, status, _, o, rects, _ = _decode(eng, files, gap=9, extra_pitch=5)
    assert [bool(s) for s in status] == [bool(s) for s in want]
    assert _untouched(o, rects) and np.array_equal(pics[-1], ref.pillow_pixels(good))
    for k, (name, f) in enumerate(bad.items()):
        p = tmp_path / f'd{k}.jpg'
        p.write_bytes(f)
        try:
            host = preprocess.pack_frames([preprocess._host_rgb(str(p))], DEV)
        except Exception as e:
            with pytest.raises(type(e)):
                preprocess.decode_frames([str(p)], DEV, True)
            continue
        got = preprocess.decode_frames([str(p)], DEV, True)
        assert torch.equal(got[0], host[0]) and got[2] == host[2], name


def test_decode_frames_on_a_mixed_folder(eng, tmp_path):
    """(g) Supported, progressive, greyscale, PNG: the triple of ``pack_frames`` of the host decodes, bit for bit."""
    from PIL import Image
    a = [jpeg_ref.picture(c, h, w) for c, (h, w) in zip(('noise', 'smooth', 'sparse', 'checker', 'noise'), ((65, 130), (33, 47), (40, 56), (24, 24), (9, 200)))]
    paths = [str(tmp_path / n) for n in ('a.jpg', 'b.jpeg', 'c.jpg', 'd.png', 'e.JPG', 'f.jpg')]
    Image.fromarray(a[0]).save(paths[0], quality=95)
    Image.fromarray(a[1]).save(paths[1], quality=75, progressive=True)
    Image.fromarray(a[2][..., 0]).save(paths[2])
    Image.fromarray(a[3]).save(paths[3])
    Image.fromarray(a[4]).save(paths[4], quality=90, subsampling=0, format='JPEG')
    Image.fromarray(a[1]).save(paths[5], quality=50, optimize=True)
    want = preprocess.pack_frames([preprocess._host_rgb(p) for p in paths], DEV)
    assert [jpeg_probe(open(p, 'rb').read())[0] for p in paths] == ['supported', 'progressive', 'components', 'not_jpeg', 'supported', 'supported']
    for items in (paths, [open(p, 'rb').read() for p in paths[:3]] + paths[3:]):
        got = preprocess.decode_frames(items, DEV, True)
        assert torch.equal(got[0], want[0]) and got[1].tolist() == want[1].tolist() and got[2] == want[2]
        assert got[0].device == want[0].device and got[1].dtype == want[1].dtype
    off = preprocess.decode_frames(paths, DEV, False)
    assert torch.equal(off[0], want[0]) and off[2] == want[2]
    assert preprocess.decode_frames(paths, DEV)[2] == want[2]            # None: the default


def test_evaluation_batch_reads_the_same_crops(eng, tmp_path):
    """(h, the evaluation step's part) the ragged crops ``EvalDataset.batch`` cuts are the same with the switch on and off."""
    from PIL import Image
    paths = []
    for k, (h, w) in enumerate(((120, 160), (97, 131))):
        paths.append(str(tmp_path / f'{k}.jpg'))
        Image.fromarray(jpeg_ref.picture('smooth' if k else 'noise', h, w)).save(paths[-1], quality=90)
    crops = []
    for switch in (False, True):
        slab, offsets, shapes = preprocess.decode_frames(paths, DEV, switch)
        crops.append(preprocess.dataset_crops_ragged(slab, offsets, shapes, np.arange(2, dtype=np.int32), np.array([[80., 60.], [60., 50.]]),
                                                     np.array([0.5, 0.4]), 224))
    assert torch.equal(crops[0], crops[1])


# ---- (h) the flows: the same files with the switch on and off -----------------------------------------------------------------------
def test_camcalib_eval_reads_the_same_frames(tmp_path):
    """The stand-in 'pano_scalenet' tree holds .jpg frames: the epoch's logits and figures do not change, bit for bit."""
    from spec_amd import camcalib_eval as ce
    ce.write_standin_tree(str(tmp_path), n_images=10, min_res=96, max_res=160, batch_size=4, loss_type='softargmax_l2')
    hp = ce.load_config(str(tmp_path / ce.STANDIN_CFG))
    model = ce.build_model(hp, None, str(tmp_path), DEV)
    host = ce.run_evaluation(hp, str(tmp_path), model=model, log=lambda s: None, jpeg_decode_device=False, save_images=False)
    dev = ce.run_evaluation(hp, str(tmp_path), model=model, log=lambda s: None, jpeg_decode_device=True, save_images=False)
    assert np.array_equal(host['logits'].view(np.int32), dev['logits'].view(np.int32))
    for k in ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc'):
        assert host[k] == dev[k]


def test_camcalib_eval_script_with_the_switch(tmp_path):
    import json
    import subprocess
    import sys
    from spec_amd import camcalib_eval as ce
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rep = tmp_path / 'rep.json'
    p = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'camcalib_eval.py'), '--standin', str(tmp_path / 'tree'), '--device-decode',
                        '--report', str(rep)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    hp = ce.load_config(str(tmp_path / 'tree' / ce.STANDIN_CFG))
    res = ce.run_evaluation(hp, str(tmp_path / 'tree'), log=lambda s: None, jpeg_decode_device=False)
    with open(rep) as f:
        got = json.load(f)
    assert [got[k] for k in ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc')] == [res[k] for k in ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc')]


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """The stand-in data tree with three .jpg dataset images of different sizes beside its own."""
    from PIL import Image
    from spec_amd import evaluation
    d = str(tmp_path_factory.mktemp('jpeg_decode_flows'))
    evaluation.write_standin_data_tree(d, n_images=3)
    for k, (h, w) in enumerate(((360, 480), (200, 260), (97, 135))):
        Image.fromarray(jpeg_ref.picture('smooth' if k == 1 else 'noise', h, w, seed=k)).save(os.path.join(d, 'data/dataset_folders/spec-syn/images', f'j{k}.jpg'),
                                                                                             quality=(75, 95, 50)[k])
    return d


def test_eval_batch_is_the_same_with_the_switch(tree):
    from spec_amd import evaluation
    ds = evaluation.EvalDataset('spec-syn', tree)
    ds.imgname = np.array([f'images/j{k}.jpg' for k in range(3)])
    ds._ragged_crops, got = True, {}
    for switch in (False, True):
        ds._jpeg_decode_device = switch
        got[switch] = ds.batch(np.arange(3), DEV, 224)
    for k, v in got[False].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(got[True][k], v), k
        else:
            assert got[True][k] == v, k
    assert got[True]['img_h'].tolist() == [360.0, 200.0, 97.0]


def test_folder_demo_writes_the_same_files_with_the_switch(tree, tmp_path):
    import joblib
    from types import SimpleNamespace
    from PIL import Image
    from spec_amd import synth
    from spec_amd.tester import SPECTester
    from tests.util import gpu_models, t
    folder = str(tmp_path / 'photos')
    os.makedirs(folder)
    rng = np.random.default_rng(6)
    dets = []
    sizes = [(360, 480), (200, 260), (97, 135), (200, 260)]
    for i, (h, w) in enumerate(sizes):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i == 1:
            Image.fromarray(a).save(os.path.join(folder, 'p1.png'))
        else:
            Image.fromarray(a).save(os.path.join(folder, f'p{i}.jpg'), quality=90, progressive=i == 3)
        n = [2, 1, 3, 1][i]
        dets.append(np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(30, w, n), rng.uniform(40, h, n)], 1).astype(np.float32))
    hs = {k_: t(v) for k_, v in synth.hmr_state(1002, True).items()}
    cwd = os.getcwd()
    os.chdir(tree)
    try:
        args = SimpleNamespace(cfg=None, ckpt=hs, no_save=False, no_render=True, synthetic_assets=True, frame_batch=256, plan='throughput',
                               decode_threads=2, camcalib_model=gpu_models(True, True, DEV)[0], detections=dets)
        te = SPECTester(args)
        te._ragged_crops, results = True, {}
        for switch in (False, True):
            out = str(tmp_path / f'out_{int(switch)}')
            te._jpeg_decode_device = switch
            te.run_camcalib(folder, out)
            assert te.run_on_image_folder(folder, te.run_detector(folder), out, None) == 4
            res_dir = os.path.join(out, 'spec_results')
            results[switch] = {f: joblib.load(os.path.join(res_dir, f)) for f in sorted(os.listdir(res_dir))}
    finally:
        os.chdir(cwd)
    assert sorted(results[False]) == sorted(results[True]) == ['p0.pkl', 'p1.pkl', 'p2.pkl', 'p3.pkl']
    for f, rec in results[False].items():
        for key, v in rec.items():
            a = results[True][f][key]
            assert a.dtype == v.dtype and a.shape == v.shape and a.tobytes() == v.tobytes(), (f, key)


def test_the_idct_holds_sums_beyond_32_bits(eng):
    """Coefficients of +-128 at quantisers of 255 pass rule 2 with status 0, and the IDCT's sums leave 32 bits: the pixels are the
    reference's, which holds them in 64 (no encoder writes such a file; what Pillow's 16-bit SIMD path makes of it is not claimed)."""
    from tests.test_jpeg_decode_host import large_coefficient_file
    data = large_coefficient_file()
    want, coef, _, status = ref.decode(data)
    assert status == 0
    pics, st, _, o, rects, got = _decode(eng, [data, _files()[7][1]], gap=4, coef=True)
    assert not st.any() and _untouched(o, rects)
    assert np.array_equal(got.cpu().numpy()[:6], coef) and np.array_equal(pics[0], want)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def test_spec_eval_script_writes_the_same_files_with_the_switch(tmp_path):
    """(h) ``scripts/spec_eval.py`` as a child process on a stand-in tree whose frames are .jpg files (baseline at three qualities, one
    4:4:4, one progressive) and one .png: ``evaluation_results_<ds>.pkl`` and ``val_accuracy_results_<ds>.json`` with
    ``--ragged-crops --device-decode`` equal those with ``--ragged-crops --host-decode``."""
    import json
    import shutil
    import subprocess
    import sys
    import joblib
    from PIL import Image
    from spec_amd import evaluation
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = str(tmp_path / 'tree')
    ann = evaluation.write_standin_data_tree(d, n_images=6)['annotations']
    folder = os.path.join(d, 'data/dataset_folders/spec-syn')
    names = []
    for k, name in enumerate(ann['imgname']):
        a = np.array(Image.open(os.path.join(folder, str(name))).convert('RGB'))
        a = (a // 2 + jpeg_ref.picture('smooth', *a.shape[:2]) // 2).astype(np.uint8)
        if k == 5:
            names.append(str(name))                                  # stays a .png
            continue
        names.append(str(name).replace('.png', '.jpg'))
        Image.fromarray(a).save(os.path.join(folder, names[-1]), quality=(75, 95, 50, 90, 85)[k], subsampling=0 if k == 3 else 2, progressive=k == 4)
    np.savez(os.path.join(d, evaluation.DATASET_FILES['spec-syn']), **{**ann, 'imgname': np.array(names)})
    assert [jpeg_probe(open(os.path.join(folder, n), 'rb').read())[0] for n in names] == ['supported'] * 4 + ['progressive', 'not_jpeg']
    got = {}
    for tag, flags in (('device', ['--ragged-crops', '--device-decode']), ('host', ['--ragged-crops', '--host-decode'])):
        p = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'spec_eval.py'), '--data-root', d] + flags, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        log_dir = os.path.join(d, 'logs/eval_standin')
        with open(os.path.join(log_dir, 'val_accuracy_results_spec-syn.json')) as f:
            got[tag] = (joblib.load(os.path.join(log_dir, 'evaluation_results_spec-syn.pkl')), json.load(f),
                        [l for l in p.stdout.splitlines() if 'MPJPE' in l or 'V2V' in l])
        shutil.rmtree(log_dir)
    assert len(got['device'][2]) >= 3
    assert _same(got['device'][0], got['host'][0]) and got['device'][1] == got['host'][1] and got['device'][2] == got['host'][2]
