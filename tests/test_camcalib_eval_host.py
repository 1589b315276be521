"""Host side of CamCalib's test step (spec_amd/camcalib_eval.py): geometry, ground-truth encoding, config, the stand-in
tree and the epoch aggregation.  No GPU.  The expected sizes come from the reference's own ``Resize.get_size``
(tests/golden/camcalib_eval.npz, written by tests/golden/make_camcalib_eval_fixture.py)."""
import json
import os

import numpy as np
import pytest

from spec_amd import cam_utils
from spec_amd import camcalib_eval as ce

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'camcalib_eval.npz')


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(GOLDEN))


def test_fixture_says_what_is_reference_produced(fx):
    meta = json.loads(str(fx['meta']))
    assert 'ref_loss_*' in meta['reference_produced'] and 'ref_term_*' in meta['reference_produced']
    assert 'size_out' in meta['reference_produced'] + meta['restated']
    assert 'ref_acc_*' in meta['restated']


def test_resize_size_matches_reference_table(fx):
    sin, sout = fx['size_in'], fx['size_out']
    assert len(sin) >= 20
    for (w, h, mn, mx), (oh, ow) in zip(sin.tolist(), sout.tolist()):
        assert ce.resize_size(w, h, mn, None if mx < 0 else mx) == (oh, ow), (w, h, mn, mx)


def test_resize_size_named_cases():
    # cap hit: 1920 x 1080 would be 1066 wide -> the shorter side drops to round(1000 * 1080 / 1920) = 562 (the longer side lands
    # on int(562 * 1920 / 1080) = 999, not 1000: the reference truncates)
    assert ce.resize_size(1920, 1080, 600, 1000) == (562, 999)
    assert ce.resize_size(1080, 1920, 600, 1000) == (999, 562)                 # portrait
    assert ce.resize_size(800, 600, 600, 1000) == (600, 800)                   # already at size: unchanged
    assert ce.resize_size(1000, 1000, 600, 1000) == (600, 600)                 # square
    assert ce.resize_size(640, 480, 600, 1000) == (600, 800)                   # cap not hit
    assert ce.resize_size(1067, 600, 600, 1000) == (562, 999)                  # 600 x 1067: over the cap by a fraction
    assert ce.resize_size(1920, 1080, 600, None) == (600, 1066)                # no cap = the demo's Resize(600)
    # differs from the demo's geometry exactly where the cap bites
    from spec_amd.preprocess import resize_output_size
    assert resize_output_size(1920, 1080, 600) == (1066, 600)


def test_target_encoding_at_and_next_to_bin_edges(fx):
    for bins, pick in ((cam_utils.vfov_bins, 0), (cam_utils.pitch_bins, 1), (cam_utils.roll_bins, 2)):
        edges = bins[[0, 1, 100, 127, 253, 254]]
        vals = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [bins[0] - 1.0, bins[-1] + 1.0]])
        args = [np.zeros_like(vals)] * 3
        args[pick] = vals
        got = ce.encode_targets(*args, 'ce')[pick]
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, np.digitize(vals, bins))
        assert got.min() == 0 and got.max() == 255                              # bin 0 = below the first edge, 255 = at / above the last
        np.testing.assert_array_equal(ce.encode_targets(*args, 'kl')[pick], got)
    # the fixture's targets were encoded with the reference's tables and helpers
    gt = fx['gt']
    for lt, key in (('ce', 'target_bins'), ('softargmax_l2', 'target_soft'), ('softargmax_biased_l2', 'target_soft')):
        got = np.stack(ce.encode_targets(gt[0], gt[1], gt[2], lt))
        assert got.dtype == fx[key].dtype
        np.testing.assert_array_equal(got, fx[key])
    with pytest.raises(ValueError):
        ce.encode_targets(gt[0], gt[1], gt[2], 'l2')


def test_config_defaults_and_opts(tmp_path):
    hp = ce.load_config(None)
    assert hp['DATASET'] == {'TRAIN_DS': 'pano', 'VAL_DS': 'pano', 'MIN_RES': 600, 'MAX_RES': 1000, 'BATCH_SIZE': 64}
    assert hp['MODEL'] == {'BACKBONE': 'resnet34', 'NUM_FC_LAYERS': 1, 'NUM_FC_CHANNELS': 1024, 'LOSS_VFOV_WEIGHT': 1.0,
                           'LOSS_PITCH_WEIGHT': 1.0, 'LOSS_ROLL_WEIGHT': 1.0, 'LOSS_TYPE': 'ce'}
    assert hp['TRAINING']['PRETRAINED'] is None
    cfg = tmp_path / 'c.yaml'
    cfg.write_text('DATASET:\n  VAL_DS: pano_scalenet\n  BATCH_SIZE: 8\nMODEL:\n  LOSS_TYPE: softargmax_biased_l2\n')
    hp = ce.load_config(str(cfg), ['MODEL.LOSS_ROLL_WEIGHT', '3.0', 'DATASET.MIN_RES', '96', 'MODEL.BACKBONE', 'resnet50'])
    assert hp['DATASET']['VAL_DS'] == 'pano_scalenet' and hp['DATASET']['BATCH_SIZE'] == 8 and hp['DATASET']['MAX_RES'] == 1000
    assert hp['DATASET']['MIN_RES'] == 96 and hp['MODEL']['LOSS_ROLL_WEIGHT'] == 3.0 and hp['MODEL']['BACKBONE'] == 'resnet50'
    assert hp['MODEL']['LOSS_TYPE'] == 'softargmax_biased_l2'
    assert ce.load_config(None)['DATASET']['BATCH_SIZE'] == 64                  # the defaults are not edited in place
    # the SPEC evaluation's own defaults are untouched by the shared merge
    from spec_amd import evaluation
    assert evaluation.load_config(None)['METHOD'] == 'hmr_cam'
    with pytest.raises(ValueError):
        ce.load_config(None, ['MODEL.BACKBONE'])


def test_pano_agora_refused_by_name(tmp_path):
    for key in ('TRAIN_DS', 'VAL_DS'):
        hp = ce.load_config(None, [f'DATASET.{key}', 'pano_agora'])
        with pytest.raises(NotImplementedError, match='pano_agora'):
            ce.val_dataset_name(hp)
    with pytest.raises(NotImplementedError, match='pano_agora'):
        ce.PanoValDataset('pano_agora', str(tmp_path))
    # the quirk: TRAIN_DS only decides pano_agora or not; the set that is read is VAL_DS
    hp = ce.load_config(None, ['DATASET.TRAIN_DS', 'pano', 'DATASET.VAL_DS', 'pano_scalenet'])
    assert ce.val_dataset_name(hp) == 'pano_scalenet'
    with pytest.raises(ValueError):
        ce.val_dataset_name(ce.load_config(None, ['DATASET.VAL_DS', 'sun360']))


@pytest.mark.parametrize('dataset', ['pano_scalenet', 'pano'])
def test_standin_tree_round_trip(tmp_path, dataset):
    from PIL import Image
    truth = ce.write_standin_tree(str(tmp_path), n_images=10, dataset=dataset, loss_type='softargmax_l2', weights=(0.5, 2.0, 3.0))
    hp = ce.load_config(str(tmp_path / ce.STANDIN_CFG))
    assert hp['DATASET']['VAL_DS'] == dataset and hp['MODEL']['LOSS_PITCH_WEIGHT'] == 2.0 and hp['MODEL']['LOSS_TYPE'] == 'softargmax_l2'
    ds = ce.PanoValDataset(ce.val_dataset_name(hp), str(tmp_path))
    assert len(ds) == 10 and ds.image_filenames == truth['names']
    kinds = set()
    for i in range(len(ds)):
        fr = ds.frame(i)
        w, h = truth['sizes_wh'][i]
        assert fr.shape == (h, w, 3) and fr.dtype == np.uint8
        with Image.open(ds.imgname(i)) as im:
            assert im.format == ('JPEG' if dataset == 'pano_scalenet' else 'PNG')
        np.testing.assert_allclose(ds.labels(i), truth['labels'][i], rtol=0, atol=1e-15)
        oh, ow = ce.resize_size(w, h, hp['DATASET']['MIN_RES'], hp['DATASET']['MAX_RES'])
        kinds.add('landscape' if w > h else 'portrait' if h > w else 'square')
        if (oh, ow) == (h, w):
            kinds.add('at_size')
        if min(oh, ow) < hp['DATASET']['MIN_RES']:
            kinds.add('capped')
            assert max(oh, ow) <= hp['DATASET']['MAX_RES']
    assert kinds == {'landscape', 'portrait', 'square', 'at_size', 'capped'}
    if dataset == 'pano':                                                       # vfov is stored in degrees there
        with open(ds.imgname(0).replace('images', 'annotations').replace('.png', '.json')) as f:
            assert abs(np.radians(json.load(f)['vfov']) - truth['labels'][0][0]) < 1e-12
    # the checkpoint has the Lightning layout and loads strictly into the configured backbone
    from spec_amd.checkpoint import read_checkpoint
    sd = read_checkpoint(str(tmp_path / ce.STANDIN_CKPT))['state_dict']
    assert all(k.startswith('model.') for k in sd) and 'model.fc_vfov.weight' in sd


def test_epoch_end_is_mean_of_batch_means():
    # ten per-image values split 4, 4, 2: the short last batch weighs as much as a full one
    v = np.array([1., 1., 1., 1., 2., 2., 2., 2., 10., 10.])
    outs = [{'loss': v[a:b].mean(), 'vfov_acc': v[a:b].mean(), 'pitch_acc': 0.0, 'roll_acc': 1.0} for a, b in ((0, 4), (4, 8), (8, 10))]
    res = ce.epoch_end(outs)
    assert res['val_loss'] == pytest.approx((1 + 2 + 10) / 3) and res['vfov_acc'] == pytest.approx(13 / 3)
    assert abs(res['val_loss'] - v.mean()) > 0.5                                # 4.33 vs the global mean 3.4
    assert res['pitch_acc'] == 0.0 and res['roll_acc'] == 1.0


def test_forward_limit_keeps_the_stem_below_2gib():
    n = ce.forward_limit(600, 1000)
    assert 1 <= n < 64 and n * 300 * 500 * 64 * 4 < 2 ** 31 <= (n + 1) * 300 * 500 * 64 * 4
    assert ce.forward_limit(96, 160) > 64
