"""specmi_png_decode on MI355X: every device-decoded file equals, element for element, what Pillow decodes, and its inflated
stream is zlib's - the whole set of tests/png_dec_ref.py (itself pinned against Pillow by tests/test_png_decode_host.py) in one
call of mixed sizes and colour types; independence of the batch and the slab layout; damaged streams beside good ones; every
refusal of the C ABI; ``preprocess.decode_frames`` and CamCalib's evaluation against the host route."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

from spec_amd import _lib, engine, preprocess
from tests import png_dec_ref as ref

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
    return ref.pillow_set() + ref.hand_set() + ref.crafted_set() + [ref.big_file()] + [(n, f) for n, f, _ in ref.encoder_set()]


def _decode(eng, files, gap=0, extra_pitch=0, raw=False):
    """One call on ``files`` -> (pictures as host arrays, status, host output slab, rectangles, the inflated streams or None).  The
    streams lie ``gap`` bytes apart in their slab; the pictures ``gap`` bytes apart at pitch 3 W + ``extra_pitch`` in a slab filled
    with SENTINEL."""
    probes = [engine.png_probe(f) for f in files]
    assert all(p[0] == 'supported' for p in probes)
    ranges, blob = [], b''
    for f, p in zip(files, probes):
        s = engine.png_stream(f, p[4])
        blob += bytes([0x5A]) * gap
        ranges.append((len(blob), len(s)))
        blob += s
    blob += bytes([0x5A]) * gap
    geom = np.array([p[1:4] for p in probes], np.int64)
    outs, at = [], 0
    for H, W, _ in geom:
        at += gap
        outs.append((at, 3 * W + extra_pitch))
        at += (H - 1) * (3 * W + extra_pitch) + 3 * W
    out_slab = torch.full((int(at + gap),), SENTINEL, device=DEV, dtype=torch.uint8)
    lines = [int(H * (1 + W * ref.BPP[int(ct)])) for H, W, ct in geom]
    rbuf = torch.full((sum((n + 255) // 256 * 256 for n in lines),), SENTINEL, device=DEV, dtype=torch.uint8) if raw else None
    status = eng.png_decode_into(torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(DEV), ranges, geom, out_slab, outs, raw=rbuf)
    o = out_slab.cpu().numpy()
    pics = [np.lib.stride_tricks.as_strided(o[off:], (H, W, 3), (pitch, 3, 1)).copy() for (off, pitch), (H, W, _) in zip(outs, geom)]
    raws = None
    if raw:
        r, at, raws = rbuf.cpu().numpy(), 0, []
        for n in lines:
            raws.append(r[at:at + n].tobytes())
            at += (n + 255) // 256 * 256
    return pics, status.cpu().numpy(), o, [(off, pitch, int(H), int(W)) for (off, pitch), (H, W, _) in zip(outs, geom)], raws


def _untouched(o, rects):
    """Every byte of the host slab ``o`` outside the rectangles still holds SENTINEL."""
    mask = np.ones(o.size, bool)
    for off, pitch, H, W in rects:
        for y in range(H):
            mask[off + y * pitch:off + y * pitch + 3 * W] = False
    return bool((o[mask] == SENTINEL).all())


def test_the_whole_set_in_one_call(eng):
    """One call of mixed sizes and colour types: Pillow's pixels, status 0, zlib's inflated streams, nothing else written."""
    names, files = zip(*_files())
    pics, status, o, rects, raws = _decode(eng, list(files), gap=5, raw=True)
    assert not status.any(), [(n, int(s)) for n, s in zip(names, status) if s]
    for name, f, px, raw in zip(names, files, pics, raws):
        assert raw == zlib.decompress(ref.stream_of(f, ref.probe(f)['ranges'])), name
        assert np.array_equal(px, ref.pillow_pixels(f)), name
    assert _untouched(o, rects)
    slab, offsets, sizes, st = eng.png_decode(list(files[:40]))
    assert not st.any().item() and sizes == [p.shape[:2] for p in pics[:40]]
    assert torch.equal(slab.cpu(), torch.from_numpy(np.concatenate([p.reshape(-1) for p in pics[:40]])))
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([p.size for p in pics[:40]])[:-1]]).tolist()


def _some():
    d = dict(_files())
    return [d[k] for k in ('noisy-300x300', 'pillow-120x121-ct6-smooth-l6', 'pillow-65x3-ct4-noise-l9', 'eob-last-lane', 'runs-258',
                           'pillow-1x1-ct0-flat-l1', 'distance-32768', 'filter4-120x121-ct2', 'flat-rle-120x121', 'encoder-matches-row')]


def test_neighbours_and_position_do_not_matter(eng):
    files = _some()
    whole, st, _, _, raws = _decode(eng, files, raw=True)
    assert not st.any()
    for i, f in enumerate(files):
        alone, st1, _, _, raw1 = _decode(eng, [f], raw=True)
        assert not st1.any() and np.array_equal(alone[0], whole[i]) and raw1[0] == raws[i]
    back, st2, _, _, _ = _decode(eng, files[::-1], gap=7)
    assert not st2.any()
    for a, b in zip(whole, back[::-1]):
        assert np.array_equal(a, b)


def test_a_larger_pitch_leaves_the_gaps(eng):
    files = _some()
    pics, st, o, rects, _ = _decode(eng, files, gap=3, extra_pitch=11)
    assert not st.any() and _untouched(o, rects)
    for f, px in zip(files, pics):
        assert np.array_equal(px, ref.pillow_pixels(f))


def test_damaged_files_beside_good_ones(eng):
    """The damaged files have passed tests/png_dec_ref.py with every index in range (tests/test_png_decode_host.py); here they
    come back with a non-zero status - the reference's -, and their neighbours exact."""
    damaged = ref.damaged_set()
    good = _some()[:4]
    files = []
    for k, (_, f) in enumerate(damaged):
        files += [good[k % len(good)], f]
    files.append(good[0])
    pics, status, o, rects, _ = _decode(eng, files, gap=2)
    assert _untouched(o, rects)
    for i, f in enumerate(files):
        if i % 2 == 1:
            name = damaged[i // 2][0]
            assert status[i] != 0, name
            assert int(status[i]) == ref.decode(f)[1], name
        else:
            assert status[i] == 0 and np.array_equal(pics[i], ref.pillow_pixels(f))


def test_decode_frames_equals_the_host_route(eng, tmp_path):
    from PIL import Image
    d = dict(_files())
    rng = np.random.default_rng(3)
    names = []
    for k, key in enumerate(('pillow-120x121-ct2-smooth-l6', 'pillow-65x3-ct6-noise-l6', 'filter3-120x121-ct0', 'noisy-300x300')):
        names.append(str(tmp_path / f'f{k}.png'))
        with open(names[-1], 'wb') as f:
            f.write(d[key])
    names.append(str(tmp_path / 'j.jpg'))
    Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(names[-1], quality=90)
    names.append(str(tmp_path / 'deep.png'))
    Image.fromarray((np.arange(99, dtype=np.uint16).reshape(9, 11) * 600)).save(names[-1])
    assert engine.png_probe(open(names[-1], 'rb').read())[0] == 'depth'
    items = names + [d['pillow-7x1-ct4-flat-opt'], rng.integers(0, 256, (5, 6, 3), dtype=np.uint8)]
    want = preprocess.decode_frames(items, DEV, False, False)
    for jd in (False, True):
        got = preprocess.decode_frames(items, DEV, jd, True)
        assert torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    # a damaged file raises on the host route what it raises without the switch
    bad = str(tmp_path / 'bad.png')
    with open(bad, 'wb') as f:
        f.write(dict(ref.damaged_set())['damaged-adler'])
    with pytest.raises(OSError) as host:
        preprocess.decode_frames(names + [bad], DEV, False, False)
    with pytest.raises(OSError) as dev:
        preprocess.decode_frames(names + [bad], DEV, True, True)
    assert type(host.value) is type(dev.value)


def test_camcalib_evaluation_is_the_same_with_the_switch(tmp_path):
    """CamCalib's test step over the stand-in 'pano' tree, whose frames are .png: the epoch's logits and figures do not change."""
    from spec_amd import camcalib_eval as ce
    ce.write_standin_tree(str(tmp_path), n_images=6, dataset='pano', min_res=96, max_res=128, batch_size=4, loss_type='softargmax_l2')
    hp = ce.load_config(str(tmp_path / ce.STANDIN_CFG))
    model = ce.build_model(hp, None, str(tmp_path), DEV)
    host = ce.run_evaluation(hp, str(tmp_path), model=model, log=lambda s: None, jpeg_decode_device=False, png_decode_device=False, save_images=False)
    dev = ce.run_evaluation(hp, str(tmp_path), model=model, log=lambda s: None, jpeg_decode_device=False, png_decode_device=True, save_images=False)
    assert np.array_equal(host['logits'].view(np.int32), dev['logits'].view(np.int32))
    for k in ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc'):
        assert host[k] == dev[k]


def test_a_repeated_call_replays_from_a_graph(eng):
    """The table's rule under capture (as tests/test_gpu_png.py pins it for the encoder): other records are refused with
    ERR_STATE and leave the capture valid, the previous call's records are captured, and the replay writes the eager call's bytes."""
    import io
    from PIL import Image
    rng = np.random.default_rng(11)
    files = []
    for H, W in ((8, 8), (5, 3)):
        f = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(f, format='PNG')
        files.append(f.getvalue())
    probes = [engine.png_probe(f) for f in files]
    assert [p[:4] for p in probes] == [('supported', 8, 8, 2), ('supported', 5, 3, 2)]
    streams = [engine.png_stream(f, p[4]) for f, p in zip(files, probes)]
    slab = torch.from_numpy(np.frombuffer(b''.join(streams), np.uint8).copy()).to(DEV)
    ranges = [(0, len(streams[0])), (len(streams[0]), len(streams[1]))]
    geom, outs = [p[1:4] for p in probes], [(0, 24), (192, 9)]
    out = torch.full((192 + 45,), SENTINEL, device=DEV, dtype=torch.uint8)
    status = torch.ones(2, device=DEV, dtype=torch.int32)
    eng.png_decode_into(slab, ranges, geom, out, outs, status=status)             # also the warm-up call of the capture below
    want = out.clone()
    assert not status.any().item()
    assert want.cpu().numpy().tobytes() == b''.join(ref.pillow_pixels(f).tobytes() for f in files)
    out.fill_(SENTINEL), status.fill_(1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, stream=s):
        try:      # other records are another table: refused, and the capture goes on
            eng.png_decode_into(slab, ranges[:1], geom[:1], out, outs[:1], status=status[:1])
        except _lib.SpecmiError as e:
            err = e
        eng.png_decode_into(slab, ranges, geom, out, outs, status=status)         # the previous call's records: captured
    assert err is not None and err.code == _lib.ERR_STATE, err
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and status.all().item()                 # capturing ran nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and not status.any().item()
        out.fill_(SENTINEL)
    other, st, _, _, _ = _decode(eng, files[::-1])                                # the handle is usable afterwards, with other records
    assert not st.any() and all(np.array_equal(px, ref.pillow_pixels(f)) for px, f in zip(other, files[::-1]))


def _call(eng, **change):
    """specmi_png_decode on two good files with one argument changed -> the return code; the output slab must stay untouched."""
    files = [dict(_files())[k] for k in ('pillow-7x1-ct2-smooth-l6', 'pillow-1x7-ct6-noise-l6')]
    probes = [engine.png_probe(f) for f in files]
    streams = [engine.png_stream(f, p[4]) for f, p in zip(files, probes)]
    slab = torch.from_numpy(np.frombuffer(b''.join(streams), np.uint8).copy()).to(DEV)
    out = torch.full((64,), SENTINEL, device=DEV, dtype=torch.uint8)
    a = dict(in_slab=slab.data_ptr(), in_bytes=slab.numel(), ranges=np.array([[0, len(streams[0])], [len(streams[0]), len(streams[1])]], np.int64),
             geom=np.array([p[1:4] for p in probes], np.int32), out_slab=out.data_ptr(), out_bytes=out.numel(),
             outs=np.array([[0, 3], [21, 21]], np.int64), n=2, status=torch.zeros(2, device=DEV, dtype=torch.int32).data_ptr(), raw=None, raw_bytes=0)
    if change.pop('overlap', False):                          # the output slab begins inside the stream slab
        a.update(out_slab=slab.data_ptr() + 1, out_bytes=slab.numel())
    a.update(change)
    ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
    rc = eng.lib.specmi_png_decode(eng.h, a['in_slab'], a['in_bytes'], ptr(a['ranges'], _lib.c_int64_p), ptr(a['geom'], _lib.c_int32_p), a['out_slab'],
                                   a['out_bytes'], ptr(a['outs'], _lib.c_int64_p), a['n'], a['status'], a['raw'], a['raw_bytes'], None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), slab


def test_every_refusal_of_the_c_abi(eng):
    rc, out, _ = _call(eng)
    assert rc == _lib.OK and (out[:42] != SENTINEL).any() and (out[42:] == SENTINEL).all()
    i64 = lambda x: np.array(x, np.int64)
    rawbuf = torch.empty(511, device=DEV, dtype=torch.uint8)
    cases = {
        'null in_slab': dict(in_slab=None), 'null ranges': dict(ranges=None), 'null geom': dict(geom=None), 'null out_slab': dict(out_slab=None),
        'null outs': dict(outs=None), 'null status': dict(status=None), 'n = 0': dict(n=0), 'n = 65536': dict(n=65536),
        'range leaves': dict(in_bytes=10), 'negative range': dict(ranges=i64([[-1, 20], [20, 20]])), 'short stream': dict(ranges=i64([[0, 7], [20, 20]])),
        'pitch': dict(outs=i64([[0, 2], [21, 21]])), 'rectangle leaves': dict(out_bytes=41), 'negative offset': dict(outs=i64([[-1, 3], [21, 21]])),
        'shared byte': dict(outs=i64([[0, 3], [20, 21]])), 'size': dict(geom=np.array([[0, 1, 2], [1, 7, 6]], np.int32)),
        'colour type': dict(geom=np.array([[7, 1, 3], [1, 7, 6]], np.int32)), 'raw too small': dict(raw=rawbuf.data_ptr(), raw_bytes=511),
        'overlapping slabs': dict(overlap=True, outs=i64([[0, 3], [21, 21]])),
    }
    for name, change in cases.items():
        rc, out, _ = _call(eng, **change)
        assert rc == _lib.ERR_ARG, name
        assert (out == SENTINEL).all(), name
    rc = C.c_int32()
    assert eng.lib.specmi_png_probe(None, 0, C.byref(rc), C.byref(rc), C.byref(rc), C.byref(rc), None, 0, C.byref(rc)) == _lib.ERR_ARG
