"""Perspective views out of panoramas on the device (spec_amd/csrc/panorama.hip, specmi_pano_extract_views,
spec_amd/panorama.py) against tests/golden/pano_views.npz, which the reference's own ``extractImage`` produced.

Parity bound.  The kernel restates the reference's fp64 arithmetic operation by operation; what can differ is the last ulp
of the device's asin / atan2 / sin / cos / atan, which moves the unrounded pixel value by about 1e-11 (a coordinate of at
most 96 pixels times 2^-52 relative, times a texel difference of at most 255).  The fixture marks the pixels whose unrounded
reference value lies within 1e-6 of a rounding tie (``tie_K``, at most 1 in 1000 by construction): outside that mask every
uint8 must EQUAL the reference's, inside it may differ by one.
"""
import os

import numpy as np
import pytest
import torch

from spec_amd import _lib, cam_utils, panorama
from spec_amd import camcalib_eval as ce

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pano_views.npz')


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope='module')
def eng():
    return cam_utils._engine(torch.device(DEV))


@pytest.fixture(scope='module')
def extracted(fx, eng):
    """Every fixture view, the views of one panorama in ONE launch -> {view index: (H, W, 3) uint8 host array}."""
    out = {}
    for p, name in enumerate(('pano_even', 'pano_odd')):
        idx = np.flatnonzero(fx['pano_of'] == p)
        pano = torch.from_numpy(fx[name]).to(DEV)
        views = panorama.extract_views(pano, fx['views'][idx], fx['heights'][idx], eng)
        torch.cuda.synchronize()
        for k, v in zip(idx, views):
            out[int(k)] = v.cpu().numpy()
    return out


def test_parity_with_the_reference_fixture(fx, extracted):
    n = len(fx['views'])
    assert sorted(extracted) == list(range(n))
    ties = off_by_one = 0
    for k in range(n):
        got, ref, tie = extracted[k], fx[f'u8_{k}'], fx[f'tie_{k}']
        assert got.shape == ref.shape == tuple(fx['out_hw'][k]) + (3,) and got.dtype == np.uint8
        d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
        print(f'view {k}: {ref.shape[0]}x{ref.shape[1]}  differing outside the mask {int((d[~tie] != 0).sum())}  inside {int((d[tie] != 0).sum())} of {int(tie.sum())}')
        assert not d[~tie].any(), (k, np.argwhere((d != 0) & ~tie)[:4])
        assert d[tie].max(initial=0) <= 1, k
        ties += int(tie.sum()); off_by_one += int((d[tie] != 0).sum())
    print(f'near-tie pixels {ties}, of which moved by one: {off_by_one}')


def test_one_launch_equals_one_view_per_launch(fx, eng, extracted):
    for k in range(len(fx['views'])):
        pano = torch.from_numpy(fx[('pano_even', 'pano_odd')[fx['pano_of'][k]]]).to(DEV)
        one = panorama.extract_views(pano, fx['views'][k:k + 1], fx['heights'][k:k + 1], eng)
        assert len(one) == 1 and np.array_equal(one[0].cpu().numpy(), extracted[k]), k


def test_one_by_one_view_is_the_corner_sample(fx, eng, extracted):
    """The reference cannot produce a 1 x 1 view (its np.mat product raises), so there is no reference output to compare with.
    What the extractor computes is fixed by arithmetic the fixture does pin: numpy.linspace of ONE sample is its start, -fov,
    and sample 0 of a longer linspace is 0 * step + start = the same number - so a 1 x 1 view at ratio 1 must equal, bit for
    bit, pixel [0, 0] of a square view with the same angles and vfov."""
    checked = 0
    for k in range(len(fx['views'])):
        if fx['views'][k][4] != 1.0:
            continue
        pano = torch.from_numpy(fx[('pano_even', 'pano_odd')[fx['pano_of'][k]]]).to(DEV)
        one = panorama.extract_views(pano, fx['views'][k:k + 1], [1], eng)
        assert tuple(one[0].shape) == (1, 1, 3)
        assert np.array_equal(one[0].cpu().numpy()[0, 0], extracted[k][0, 0]) and np.array_equal(extracted[k][0, 0], fx[f'u8_{k}'][0, 0]), k
        checked += 1
    assert checked >= 3


def test_gaps_between_views_stay_untouched(fx, eng, extracted):
    idx = np.flatnonzero(fx['pano_of'] == 0)
    pano = torch.from_numpy(fx['pano_even']).to(DEV)
    hw = fx['out_hw'][idx]
    nbytes = hw.astype(np.int64).prod(1) * 3
    gaps = np.array([7, 1, 64, 3, 129, 5, 2, 11, 33, 17])[:len(idx)]           # odd gaps: views start at unaligned bytes
    offsets = np.cumsum(gaps + np.concatenate([[0], nbytes[:-1]]))
    total = int(offsets[-1] + nbytes[-1] + 19)
    slab = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    eng.pano_extract_views(pano, fx['views'][idx], hw, offsets=offsets, out=slab)
    host = slab.cpu().numpy()
    covered = np.zeros(total, bool)
    for k, o, nb in zip(idx, offsets, nbytes):
        assert np.array_equal(host[o:o + nb].reshape(extracted[int(k)].shape), extracted[int(k)]), k
        covered[o:o + nb] = True
    assert (~covered).sum() == gaps.sum() + 19 and (host[~covered] == 0xA5).all()


def test_slab_feeds_the_ragged_resize_as_an_upload_does(fx, eng):
    idx = np.flatnonzero(fx['pano_of'] == 1)
    pano = torch.from_numpy(fx['pano_odd']).to(DEV)
    views = panorama.extract_views(pano, fx['views'][idx], fx['heights'][idx], eng)
    geom = [(h, w) + ce.resize_size(w, h, 24, 40) for h, w in views.sizes]
    direct = eng.resize_normalize_ragged(views.slab, views.offsets, geom).clone()
    host = [v.cpu().numpy() for v in views]
    uploaded = ce.pad_batch(host, 24, 40, DEV, eng)
    assert direct.shape == uploaded.shape and torch.equal(direct, uploaded)
    assert torch.equal(ce.pad_batch((views.slab, list(views.offsets), views.sizes), 24, 40, DEV, eng), uploaded)


def test_end_to_end_generated_views_equal_the_written_tree(tmp_path):
    from PIL import Image
    truth = ce.write_standin_tree(str(tmp_path / 'standin'), n_images=1, min_res=96, max_res=160, batch_size=2)
    hp = ce.load_config(str(tmp_path / 'standin' / ce.STANDIN_CFG))
    assert hp['DATASET']['BATCH_SIZE'] == 2 and hp['DATASET']['MIN_RES'] == 96 and truth['config']['DATASET']['VAL_DS'] == 'pano_scalenet'
    model = ce.build_model(hp, None, str(tmp_path / 'standin'), DEV)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:64, 0:128]
    pano = np.stack([127 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 + c) for c in range(3)], -1)
    pano = np.clip(pano + rng.normal(0, 10, pano.shape), 0, 255).astype(np.uint8)
    os.makedirs(tmp_path / 'panos')
    Image.fromarray(pano).save(str(tmp_path / 'panos' / 'scene.png'))
    ds = panorama.PanoViewDataset([str(tmp_path / 'panos' / 'scene.png')], views_per_pano=3, seed=17, device=DEV)
    cams = panorama.sample_cameras(3, np.random.default_rng(17))
    res = ce.run_evaluation(hp, model=model, dataset=ds, log=lambda s: None)
    assert [o['n'] for o in res['batches']] == [2, 1] and res['logits'].shape == (3, 3, 256)
    for k in ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc'):
        assert np.isfinite(res[k]), k
    assert np.isfinite(res['logits']).all() and all(np.isfinite(res['err_' + a]).all() for a in ('vfov', 'pitch', 'roll'))
    for a in ('vfov', 'pitch', 'roll'):
        assert res['gt_' + a].tolist() == [c[a] for c in cams]
    # the same views through a stored tree; PNG bytes under the .jpg names keep the comparison free of JPEG's loss
    panorama.write_tree(ds, str(tmp_path / 'tree'), image_format='PNG', log=lambda s: None)
    tree = ce.run_evaluation(hp, str(tmp_path / 'tree'), model=model, log=lambda s: None)
    assert [os.path.basename(n) for n in tree['imgname']] == res['imgname']
    for a in ('vfov', 'pitch', 'roll'):
        assert tree['gt_' + a].tolist() == res['gt_' + a].tolist()
    assert np.array_equal(tree['logits'].view(np.int32), res['logits'].view(np.int32))
    assert tree['val_loss'] == res['val_loss'] and tree['img_sizes'] == res['img_sizes']
    # a batch that is exactly one panorama's views is handed over as the extraction's own slab, not a concatenation
    slab, offsets, sizes = ds.device_batch(range(3))
    assert slab is ds.views_of(0).slab and offsets == [int(o) for o in ds.views_of(0).offsets] and sizes == ds.views_of(0).sizes
    hp3 = ce.load_config(str(tmp_path / 'standin' / ce.STANDIN_CFG), ['DATASET.BATCH_SIZE', '3'])
    res3 = ce.run_evaluation(hp3, model=model, dataset=ds, log=lambda s: None)
    tree3 = ce.run_evaluation(hp3, str(tmp_path / 'tree'), model=model, log=lambda s: None)
    assert [o['n'] for o in res3['batches']] == [3]
    assert np.array_equal(tree3['logits'].view(np.int32), res3['logits'].view(np.int32)) and tree3['val_loss'] == res3['val_loss']


def _call(eng, pano, PH, PW, views, hw, offsets, slab_bytes, out, n):
    from spec_amd.engine import _ptr
    views, hw, offsets = np.ascontiguousarray(views, np.float64), np.ascontiguousarray(hw, np.int32), np.ascontiguousarray(offsets, np.int64)
    return eng.lib.specmi_pano_extract_views(
        eng.h, None if pano is None else _ptr(pano), PH, PW, None if views.size == 0 else views.ctypes.data_as(_lib.c_double_p),
        None if hw.size == 0 else hw.ctypes.data_as(_lib.c_int32_p), None if offsets.size == 0 else offsets.ctypes.data_as(_lib.c_int64_p),
        slab_bytes, None if out is None else _ptr(out), n, eng._stream())


def test_bad_arguments_are_refused_and_launch_nothing(eng):
    pano = torch.zeros(8, 16, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((4 * 5 * 3,), 0x5A, dtype=torch.uint8, device=DEV)
    good = dict(pano=pano, PH=8, PW=16, views=[[0.1, 0.2, 0.0, 60.0, 1.25]], hw=[[4, 5]], offsets=[0], slab_bytes=60, out=out, n=1)
    nan, inf = float('nan'), float('inf')
    bad = {
        'null panorama': dict(pano=None), 'null views': dict(views=[]), 'null sizes': dict(hw=[]), 'null offsets': dict(offsets=[]),
        'null slab': dict(out=None), 'n = 0': dict(n=0), 'n < 0': dict(n=-1), 'PH < 1': dict(PH=0), 'PW < 1': dict(PW=0),
        'height < 1': dict(hw=[[0, 5]]), 'width < 1': dict(hw=[[4, 0]]),
        'NaN elevation': dict(views=[[nan, 0.2, 0.0, 60.0, 1.25]]), 'infinite azimuth': dict(views=[[0.1, inf, 0.0, 60.0, 1.25]]),
        'NaN roll': dict(views=[[0.1, 0.2, nan, 60.0, 1.25]]), 'infinite vfov': dict(views=[[0.1, 0.2, 0.0, inf, 1.25]]),
        'NaN ratio': dict(views=[[0.1, 0.2, 0.0, 60.0, nan]]),
        'vfov = 0': dict(views=[[0.1, 0.2, 0.0, 0.0, 1.25]]), 'vfov < 0': dict(views=[[0.1, 0.2, 0.0, -60.0, 1.25]]),
        'vfov = 180': dict(views=[[0.1, 0.2, 0.0, 180.0, 1.25]]), 'ratio = 0': dict(views=[[0.1, 0.2, 0.0, 60.0, 0.0]]),
        'ratio < 0': dict(views=[[0.1, 0.2, 0.0, 60.0, -1.25]], hw=[[4, 5]]),
        'overrun': dict(slab_bytes=59), 'offset overrun': dict(offsets=[1]), 'negative offset': dict(offsets=[-1]),
        'width is not round(h * ratio)': dict(hw=[[4, 6]]),
    }
    eng.profile(True)
    try:
        for what, change in bad.items():
            rc = _call(eng, **dict(good, **change))
            assert rc == _lib.ERR_ARG, (what, rc)
            assert eng.lib.specmi_last_error(eng.h), what
        torch.cuda.synchronize()
        assert not [e for e in eng.profile_read(64) if e['kernel'] == 'pano_extract'], 'a refused call launched the kernel'
        assert (out == 0x5A).all()
        assert _call(eng, **good) == 0
        torch.cuda.synchronize()
        assert [e['launches'] for e in eng.profile_read(64) if e['kernel'] == 'pano_extract'] == [1]
    finally:
        eng.profile(False)
    assert not (out == 0x5A).all()
