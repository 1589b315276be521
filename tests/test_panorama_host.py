"""The host side of the panorama view generator (spec_amd/panorama.py, tests/golden/make_panorama_fixture.py): the C ABI
surface, the fixture's pin to the reference's source, the camera sampler's distribution and the stored tree.  No GPU."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
REFERENCE = os.environ.get('SPEC_REFERENCE', '/root/reference')


def test_entry_point_is_exported_prototyped_and_documented():
    from spec_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, 'specmi_pano_extract_views') and 'specmi_pano_extract_views' in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES['specmi_pano_extract_views']
    assert len(args) == 11
    hdr = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int specmi_pano_extract_views\(([^;]*)\);', hdr, flags=re.S)
    assert m, 'no documented declaration in include/specmi.h'
    doc, params = m.group(1), m.group(2)
    assert 'image_extraction.py:129-159' in doc and 'generateCalibrationDataset.py' in doc and 'map_coordinates' in doc
    assert params.count(',') + 1 == len(args)
    assert 'panorama.hip' in build.SOURCES


def test_fixture_meets_its_own_condition():
    fx = np.load(os.path.join(GOLDEN, 'pano_views.npz'))
    meta = json.loads(str(fx['meta']))
    n = len(fx['views'])
    ties = sum(int(fx[f'tie_{k}'].sum()) for k in range(n))
    total = sum(fx[f'tie_{k}'].size for k in range(n))
    assert (ties, total) == (meta['near_tie'], meta['values']) and ties <= total / 1000
    assert fx['pano_even'].shape == (48, 96, 3) and fx['pano_odd'].shape == (47, 95, 3)
    assert 15 <= n <= 20 and fx['out_hw'][:, 0].max() <= 40 and fx['out_hw'][:, 1].max() <= 60 and fx['out_hw'][:, 0].min() == 1
    for k in range(n):
        f64, u8 = fx[f'f64_{k}'], fx[f'u8_{k}']
        assert np.array_equal(np.abs(f64 - np.floor(f64) - 0.5) <= meta['tie_eps'], fx[f'tie_{k}'])
        assert np.array_equal(np.where(f64 > 0, np.floor(f64 + 0.5), 0).clip(0, 255).astype(np.uint8), u8)    # scipy's uint8 store
    v = fx['views']
    assert {15.0, 67.5, 120.0} <= set(v[:, 3]) and {4 / 3, 3 / 4, 1.0} <= set(v[:, 4]) and {1.5, -1.5, 0.0} <= set(v[:, 0])
    assert {0.0, np.pi / 6, -np.pi / 6, np.pi} <= set(v[:, 2]) and (np.abs(v[:, 1]) > 3.0).any()
    assert (fx['out_hw'][:, 1] % 2 == 0).any() and (fx['out_hw'][:, 1] % 2 == 1).any() and set(fx['pano_of']) == {0, 1}


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, 'camcalib', 'datagen', 'image_extraction.py')),
                    reason='reference checkout not present')
def test_selfcheck_reproduces_the_committed_fixture_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_panorama_fixture.py'), '--selfcheck', '--reference', REFERENCE],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ' 0 differ' in r.stdout


def test_generator_copies_no_reference_text():
    src = open(os.path.join(GOLDEN, 'make_panorama_fixture.py')).read()
    assert 'spec_from_file_location' in src and 'map_coordinates(' not in src and 'arctan2' not in src


@pytest.fixture(scope='module')
def cams():
    from spec_amd import panorama
    return panorama.sample_cameras(20000, np.random.default_rng(20260117))


def test_sample_cameras_stays_inside_the_reference_bounds(cams):
    from spec_amd import panorama as P
    col = lambda k: np.array([c[k] for c in cams])
    js = lambda k: np.array([c['json'][k] for c in cams])
    assert ((-np.pi <= col('yaw')) & (col('yaw') < np.pi)).all()
    assert ((P.ROLL_LOWER < col('roll')) & (col('roll') < P.ROLL_UPPER)).all()
    assert ((P.HORIZON_LOWER < js('horizon')) & (js('horizon') < P.HORIZON_UPPER)).all()
    f = js('focal_length_35mm_eq')
    assert ((P.FOCAL_LOWER < f) & (f < P.FOCAL_UPPER)).all()
    port = col('is_portrait').astype(bool)
    table = np.array(P.ASPECT_RATIOS)
    ratio = col('ratio')
    assert np.isin(ratio[~port], table).all() and np.isin(ratio[port], 1 / table).all()
    assert set(ratio[~port]) == set(table)                                   # 20 000 draws reach every row, the 1 % one too
    sensor = js('sensor_size')
    assert np.array_equal(sensor, np.where(port, 36, 24))
    assert np.array_equal(col('vfov'), 2 * np.arctan2(sensor, 2 * f)) and np.array_equal(js('vfov'), col('vfov'))
    assert np.array_equal(js('f_px'), f / 24)
    assert np.array_equal(col('pitch'), -np.arctan((js('horizon') - 0.5) / js('f_px'))) and np.array_equal(js('pitch'), col('pitch'))
    # resolution: resY = 600 and resX = int(resY / ratio) unless that is below 256 (no table ratio reaches it at 600)
    assert (col('resX') >= 256).all() and (col('resY') == 600).all()
    assert np.array_equal(col('resX'), np.array([int(600 / r) for r in ratio]))
    assert np.array_equal(js('height'), col('resX')) and np.array_equal(js('width'), col('resY'))   # swapped, as the reference writes it
    share, n = port.mean(), len(cams)
    assert abs(share - 0.2) <= 4 * np.sqrt(0.2 * 0.8 / n), share
    # the two roll scales: about a third of the rolls come from the 0.001 Cauchy (|roll| < 0.01 for 94 % of those, for 6 % of the others)
    small = (np.abs(col('roll')) < 0.01).mean()
    assert 0.30 < small < 0.45, small
    assert set(cams[0]['json']) == {'yaw', 'pitch', 'roll', 'vfov', 'focal_length_35mm_eq', 'f_px', 'height', 'width', 'sensor_size', 'horizon'}


def test_sample_cameras_is_reproducible_and_the_low_resolution_rule_holds(monkeypatch):
    from spec_amd import panorama as P
    a, b = P.sample_cameras(50, np.random.default_rng(3)), P.sample_cameras(50, np.random.default_rng(3))
    assert a == b and a != P.sample_cameras(50, np.random.default_rng(4))
    monkeypatch.setattr(P, 'RES_Y', 300)                                     # int(300 / (16/9)) = 168 < 256: the rule fires
    c = P.sample_cameras(400, np.random.default_rng(5))
    assert all(x['resX'] >= 256 for x in c)
    low = [x for x in c if int(300 / x['ratio']) < 256]
    assert low and all(x['resX'] == 256 and x['resY'] == int(256 * x['ratio']) for x in low)
    assert all(x['resY'] == 300 for x in c if int(300 / x['ratio']) >= 256)


def test_view_size_is_pythons_round():
    from spec_amd import panorama as P
    assert P.view_size(600, 4 / 3) == (600, 800) and P.view_size(600, 3 / 4) == (600, 450) and P.view_size(600, 9 / 16) == (600, 338)
    assert P.view_size(2, 3 / 4) == (2, 2) and P.view_size(1, 4 / 3) == (1, 1) and P.view_size(1, 16 / 9) == (1, 2)
    fx = np.load(os.path.join(GOLDEN, 'pano_views.npz'))
    for v, h, hw in zip(fx['views'], fx['heights'], fx['out_hw']):
        assert P.view_size(int(h), float(v[4])) == tuple(hw)


def test_grey_and_rgba_panoramas_become_rgb():
    from spec_amd import panorama as P
    g = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(P.as_rgb(g), np.stack([g, g, g], -1))
    rgba = np.arange(3 * 4 * 4, dtype=np.uint8).reshape(3, 4, 4)
    assert np.array_equal(P.as_rgb(rgba), rgba[:, :, :3])
    with pytest.raises(ValueError):
        P.as_rgb(g.astype(np.float32))


def test_extract_views_has_no_host_path():
    from spec_amd import panorama as P
    with pytest.raises(ValueError):
        P.extract_views(torch.zeros(8, 16, 3, dtype=torch.uint8), [[0, 0, 0, 60, 1.0]], [4])


def test_write_tree_is_what_the_validation_loader_reads(tmp_path, monkeypatch):
    """The tree of --write-tree, labels and layout; the views themselves need the GPU (tests/test_gpu_panorama.py), so the
    extractor is replaced by one that returns grey views of the right sizes."""
    from PIL import Image
    from spec_amd import panorama as P
    from spec_amd import camcalib_eval as ce
    os.makedirs(tmp_path / 'panos')
    for name in ('b_scene.png', 'a_scene.jpg'):
        Image.fromarray(np.full((8, 16, 3), 90, np.uint8)).save(str(tmp_path / 'panos' / name))
    (tmp_path / 'panos' / 'notes.txt').write_text('not an image')
    files = P.list_panoramas(str(tmp_path / 'panos'))
    assert [os.path.basename(f) for f in files] == ['a_scene.jpg', 'b_scene.png']

    def grey_views(pano, views, heights, engine=None):
        assert tuple(pano.shape) == (8, 16, 3) and pano.dtype == torch.uint8
        out = P.ViewList(torch.full(P.view_size(h, v[4]) + (3,), 128, dtype=torch.uint8) for v, h in zip(np.asarray(views), heights))
        return out
    monkeypatch.setattr(P, 'extract_views', grey_views)
    ds = P.PanoViewDataset(files, views_per_pano=2, seed=9, device='cpu')
    assert len(ds) == 4 and ds.imgname(1) == 'a_scene.jpg.01.jpg' and ds.imgname(2) == 'b_scene.png.00.jpg'
    extractions = []
    real = P.extract_views
    monkeypatch.setattr(P, 'extract_views', lambda *a, **k: (extractions.append(1), real(*a, **k))[1])
    folder = P.write_tree(ds, str(tmp_path / 'out'), log=lambda s: None)
    assert len(extractions) == 2                                             # every panorama once
    # written while the dataset is walked (what --write-tree does around the evaluation): the same files, still one extraction each
    ds2 = P.PanoViewDataset(files, views_per_pano=2, seed=9, device='cpu')
    folder2 = P.write_tree(ds2, str(tmp_path / 'out2'), log=lambda s: None, while_evaluating=True)
    assert os.path.isfile(os.path.join(folder2, 'val_images.pkl')) and not os.listdir(os.path.join(folder2, 'images'))
    for i in range(len(ds2)):
        ds2.device_batch([i])
    assert len(extractions) == 4
    for name in sorted(os.listdir(os.path.join(folder, 'images'))):
        a, b = (open(os.path.join(f, 'images', name), 'rb').read() for f in (folder, folder2))
        assert a == b or name.endswith('.json'), name
    assert sorted(os.listdir(os.path.join(folder, 'images'))) == sorted(os.listdir(os.path.join(folder2, 'images')))
    assert folder == str(tmp_path / 'out' / ce.DATASET_FOLDERS['pano_scalenet'])
    val = ce.PanoValDataset('pano_scalenet', str(tmp_path / 'out'))
    assert len(val) == 4 and [os.path.basename(val.imgname(i)) for i in range(4)] == ds.image_filenames
    cams = P.sample_cameras(4, np.random.default_rng(9))
    for i in range(4):
        assert val.labels(i) == ds.labels(i) == (cams[i]['vfov'], cams[i]['pitch'], cams[i]['roll'])
        fr = val.frame(i)
        assert fr.shape == P.view_size(cams[i]['resY'], cams[i]['ratio']) + (3,) and fr.dtype == np.uint8
        with Image.open(val.imgname(i)) as im:
            assert im.format == 'JPEG'
        with open(val.imgname(i).replace('.jpg', '.json')) as f:
            data = json.load(f)
        assert data == dict(cams[i]['json'], imgname=val.imgname(i))
        assert data['height'] == cams[i]['resX'] and data['width'] == cams[i]['resY']
