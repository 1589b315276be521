"""The host side of the ragged crops (spec_amd.preprocess.pack_frames, crop_detections_ragged, dataset_crops_ragged and the four
specmi_crop_*_ragged exports): the slab packer, its use by camcalib_eval.pad_batch, the C ABI surface and the checks the
wrappers make before any library call.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {'specmi_crop_normalize_ragged': 16, 'specmi_crop_normalize_f16_ragged': 16,
           'specmi_crop_resize_normalize_ragged': 12, 'specmi_crop_resize_normalize_f16_ragged': 12}


def _frames(seed=1, sizes=((1, 1), (3, 2), (5, 7), (2, 9))):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def test_packer_offsets_sizes_and_bytes():
    from spec_amd.preprocess import pack_frames
    frames = _frames()
    frames[2] = np.asfortranarray(frames[2])                 # not C-contiguous: packed in HWC order all the same
    slab, offsets, sizes = pack_frames(frames)
    assert isinstance(slab, np.ndarray) and slab.dtype == np.uint8 and slab.ndim == 1
    assert sizes == [(1, 1), (3, 2), (5, 7), (2, 9)] and offsets.dtype == np.int64 and offsets.tolist() == [0, 3, 21, 126]
    assert slab.size == 126 + 54
    for fr, off in zip(frames, offsets):
        assert np.array_equal(slab[off:off + fr.size].reshape(fr.shape), fr)
    on_host, offsets2, sizes2 = pack_frames(frames, 'cpu')   # device given: a tensor there, the same bytes
    assert isinstance(on_host, torch.Tensor) and on_host.dtype == torch.uint8 and np.array_equal(on_host.numpy(), slab)
    assert offsets2.tolist() == offsets.tolist() and sizes2 == sizes


@pytest.mark.parametrize('bad', [[], [np.zeros((2, 2, 3), np.float32)], [np.zeros((2, 2, 3), np.int8)], [np.zeros((2, 2), np.uint8)],
                                 [np.zeros((2, 2, 4), np.uint8)], [np.zeros((1, 2, 2, 3), np.uint8)],
                                 [np.zeros((2, 2, 3), np.uint8), torch.zeros(2, 2, 3, dtype=torch.uint8)]])
def test_packer_refuses(bad):
    from spec_amd.preprocess import pack_frames
    with pytest.raises(ValueError):
        pack_frames(bad)


def test_pad_batch_builds_its_slab_with_the_shared_packer(monkeypatch):
    from spec_amd import camcalib_eval, preprocess
    frames = _frames(2, ((30, 40), (17, 23), (40, 30)))
    seen = {}

    class Engine:
        device = torch.device('cpu')

        def resize_normalize_ragged(self, slab, offsets, geom, dtype=torch.float32):
            seen.update(slab=slab, offsets=list(offsets), geom=list(geom))
            return 'batch'
    calls = []
    real = preprocess.pack_frames
    monkeypatch.setattr(preprocess, 'pack_frames', lambda *a, **k: calls.append(1) or real(*a, **k))
    assert camcalib_eval.pad_batch(frames, 20, 30, 'cpu', engine=Engine()) == 'batch'
    assert calls == [1]
    assert np.array_equal(seen['slab'].numpy(), np.concatenate([fr.reshape(-1) for fr in frames]))
    assert seen['offsets'] == [0, 30 * 40 * 3, 30 * 40 * 3 + 17 * 23 * 3]
    assert seen['geom'] == [(H, W) + camcalib_eval.resize_size(W, H, 20, 30) for H, W in ((30, 40), (17, 23), (40, 30))]
    with pytest.raises(ValueError):
        camcalib_eval.pad_batch([np.zeros((4, 4, 3), np.float32)], 20, 30, 'cpu', engine=Engine())


def test_exports_are_declared_documented_and_bound():
    from spec_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    for name, nargs in EXPORTS.items():
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int ' + name + r'\(([^;]*)\);', hdr, flags=re.S)
        assert m, f'{name}: no documented declaration in include/specmi.h'
        assert m.group(2).count(',') + 1 == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert 'replaces' in m.group(1), f'{name}: the declaration does not say what it replaces'
    doc = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int specmi_crop_normalize_ragged\(', hdr, flags=re.S).group(1)
    assert 'SYNCHRONISES THE WHOLE DEVICE' in doc and 'SPECMI_ERR_STATE' in doc and 'CLAMPED' in doc


def test_exports_resolve_in_the_built_library():
    from spec_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    for name in EXPORTS:
        assert hasattr(lib, name), name


def test_wrappers_check_on_the_host_before_any_library_call(monkeypatch):
    from spec_amd import preprocess

    def no_engine(*a, **k):
        raise AssertionError('the engine was asked for before the arguments were checked')
    monkeypatch.setattr(preprocess, '_engine', no_engine)
    slab, offsets, sizes = preprocess.pack_frames(_frames(), 'cpu')
    dets, cs, sc = np.asarray([[1, 1, 2, 2], [3, 2, 4, 4]], np.float32), [[1., 1.], [3., 2.]], [0.01, 0.02]
    for fidx in ([0, 4], [-1, 0], torch.tensor([0, 9], dtype=torch.int32), np.asarray([7, 0], np.int64)):
        with pytest.raises(ValueError, match=r'\[0, 4\)'):
            preprocess.crop_detections_ragged(slab, offsets, sizes, fidx, dets)
        with pytest.raises(ValueError, match=r'\[0, 4\)'):
            preprocess.dataset_crops_ragged(slab, offsets, sizes, fidx, cs, sc)
    with pytest.raises(ValueError):                                                # one index per crop
        preprocess.crop_detections_ragged(slab, offsets, sizes, [0, 1, 2], dets)
    with pytest.raises(ValueError):                                                # one offset per frame
        preprocess.dataset_crops_ragged(slab, offsets[:3], sizes, [0, 1], cs, sc)
    with pytest.raises(RuntimeError, match='device tensor'):                       # a host slab
        preprocess.crop_detections_ragged(slab, offsets, sizes, [0, 1], dets)
    with pytest.raises(RuntimeError, match='device tensor'):
        preprocess.dataset_crops_ragged(slab.numpy(), offsets, sizes, [0, 1], cs, sc)
    for dtype in (torch.bfloat16, torch.float64, None):
        with pytest.raises(ValueError):
            preprocess.crop_detections_ragged(slab, offsets, sizes, [0, 1], dets, dtype=dtype)
        with pytest.raises(ValueError):
            preprocess.dataset_crops_ragged(slab, offsets, sizes, [0, 1], cs, sc, dtype=dtype)
