"""``camcalib_train.finetune_heads(augment=...)`` on the synthetic stand-in tree with its synthetic checkpoint: the training
ColorJitter runs on the device between the batch's slab and the resize, is reproducible from its seed, changes what the heads
see, and leaves the flow without it exactly as it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Tests that ran earlier in the process may have switched autograd off for good (the scripts do)."""
    with torch.enable_grad():
        yield


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    import joblib
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    root = tmp_path_factory.mktemp('standin')
    info = ce.write_standin_tree(str(root), n_images=6)
    folder = root / ce.DATASET_FOLDERS['pano_scalenet']
    joblib.dump(info['names'][:4], str(folder / 'train_images.pkl'))
    return str(root), ct.load_config(str(root / ce.STANDIN_CFG)), info


def _run(tree, tmp_path, name, **kw):
    from spec_amd import camcalib_train as ct
    root, hp, _ = tree
    res = ct.finetune_heads(hp, data_root=root, epochs=2, seed=3, log=lambda _: None, out=str(tmp_path / name), evaluate=False, **kw)
    return [[e[k] for k in ct.TRAIN_KEYS] for e in res['epochs']]


def test_augment_is_reproducible_and_off_by_default(tree, tmp_path):
    plain = _run(tree, tmp_path, 'a.ckpt')
    assert _run(tree, tmp_path, 'b.ckpt', augment=False) == plain           # the argument's default changes nothing
    first = _run(tree, tmp_path, 'c.ckpt', augment=True, augment_seed=7)
    again = _run(tree, tmp_path, 'd.ckpt', augment=True, augment_seed=7)
    assert np.isfinite(first).all() and np.asarray(first).shape == (2, 4)
    assert first == again                                                   # the same four epoch figures twice
    assert first != plain                                                   # the heads saw other pixels


def test_train_split_and_device_batches(tree, tmp_path):
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    root, hp, info = tree
    ds = ce.PanoValDataset('pano_scalenet', root, split='train')
    assert ds.image_filenames == info['names'][:4] and len(ce.PanoValDataset('pano_scalenet', root)) == 6
    with pytest.raises(ValueError):
        ce.PanoValDataset('pano_scalenet', root, split='test')
    lines = []
    res = ct.finetune_heads(hp, data_root=root, epochs=1, seed=3, log=lines.append, out=str(tmp_path / 't.ckpt'), evaluate=False, augment=True,
                            split='train')
    assert 'Train dataset len: 4' in lines and np.isfinite(list(res['epochs'][0].values())).all()

    class OnDevice:
        """the same frames handed over as a device slab, as ``PanoViewDataset.device_batch`` does"""
        def __init__(self, ds):
            self.ds = ds
        def __len__(self):
            return len(self.ds)
        def labels(self, i):
            return self.ds.labels(i)
        def device_batch(self, idx):
            from spec_amd.preprocess import pack_frames
            return pack_frames([self.ds.frame(i) for i in idx], DEV)
    res2 = ct.finetune_heads(hp, data_root=root, epochs=1, seed=3, log=lambda _: None, out=str(tmp_path / 'u.ckpt'), evaluate=False, augment=True,
                             dataset=OnDevice(ds))
    assert res2['epochs'] == res['epochs']
