"""The two flows whose frames differ in size - EvalDataset.batch (config 5) and SPECTester.run_on_image_folder (the folder demo) -
on the ragged crop route (one slab, one upload, one launch per batch) against the per-frame route: the same bits, whichever
way the private ``_ragged_crops`` switch points."""
import os

import numpy as np
import pytest
import torch

from tests.util import gpu_models, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SIZES = [(360, 480), (200, 260), (97, 135), (200, 260), (360, 480), (97, 135)]      # three sizes, interleaved


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """The stand-in data tree with its six equal-sized dataset images replaced by images of three sizes."""
    from PIL import Image
    from spec_amd import evaluation
    d = str(tmp_path_factory.mktemp('ragged_flows'))
    gt = evaluation.write_standin_data_tree(d, n_images=len(SIZES))
    rng = np.random.default_rng(41)
    for name, (h, w) in zip(gt['annotations']['imgname'], SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, 'data/dataset_folders/spec-syn', str(name)))
    return d


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_eval_batch_is_the_same_on_both_routes(tree, dtype):
    from spec_amd import evaluation
    from spec_amd.preprocess import dataset_crops
    ds = evaluation.EvalDataset('spec-syn', tree)
    idx = np.arange(len(SIZES))
    got = {}
    for ragged in (False, True):
        ds._ragged_crops = ragged
        got[ragged] = ds.batch(idx, DEV, 224, dtype=dtype)
    assert sorted(got[True]) == sorted(got[False])
    for k, v in got[False].items():
        if isinstance(v, torch.Tensor):
            assert got[True][k].dtype == v.dtype and torch.equal(got[True][k], v), k
        else:
            assert got[True][k] == v, k
    # the per-sample route written out: one upload, one single-crop launch per sample, then the concatenation
    crops = []
    for i in idx:
        frame = torch.from_numpy(evaluation.read_image_rgb(os.path.join(ds.img_dir, str(ds.imgname[i])))).to(DEV)
        assert tuple(frame.shape[:2]) == SIZES[i]
        crops.append(dataset_crops(frame, ds.data['center'][i:i + 1], ds.data['scale'][i:i + 1], 224, dtype=dtype))
    assert torch.equal(got[True]['img'], torch.cat(crops))
    assert got[True]['img_h'].tolist() == [float(h) for h, _ in SIZES] and got[True]['img_w'].tolist() == [float(w) for _, w in SIZES]


def test_folder_demo_writes_the_same_files_on_both_routes(tree, tmp_path):
    import joblib
    from types import SimpleNamespace
    from PIL import Image
    from spec_amd import synth
    from spec_amd.tester import SPECTester
    folder = str(tmp_path / 'photos')
    os.makedirs(folder)
    rng = np.random.default_rng(6)
    dets = []
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, f'p{i}.png'))
        n = [2, 1, 3, 0, 4, 1][i]
        dets.append(np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(30, w, n), rng.uniform(40, h, n)], 1).astype(np.float32))
    hs = {k_: t(v) for k_, v in synth.hmr_state(1002, True).items()}
    cwd = os.getcwd()
    os.chdir(tree)
    try:
        args = SimpleNamespace(cfg=None, ckpt=hs, no_save=False, no_render=True, synthetic_assets=True, frame_batch=1, plan='throughput',
                               decode_threads=2, camcalib_model=gpu_models(True, True, DEV)[0], detections=dets)
        te = SPECTester(args)
        results = {}
        for fb in (1, 256):
            for ragged in (False, True):
                out = str(tmp_path / f'out_{fb}_{int(ragged)}')
                args.frame_batch, te._ragged_crops = fb, ragged
                te.run_camcalib(folder, out)
                assert te.run_on_image_folder(folder, te.run_detector(folder), out, None) == 5
                res_dir = os.path.join(out, 'spec_results')
                results[fb, ragged] = {f: joblib.load(os.path.join(res_dir, f)) for f in sorted(os.listdir(res_dir))}
    finally:
        os.chdir(cwd)
    ref = results[1, False]
    assert sorted(ref) == ['p0.pkl', 'p1.pkl', 'p2.pkl', 'p4.pkl', 'p5.pkl']
    for tag, res in results.items():
        assert sorted(res) == sorted(ref), tag
        for f, rec in ref.items():
            assert sorted(res[f]) == sorted(rec), (tag, f)
            for key, v in rec.items():
                a = res[f][key]
                assert a.dtype == v.dtype and a.shape == v.shape and a.tobytes() == v.tobytes(), (tag, f, key)
