#!/usr/bin/env python
"""Head-only fine-tuning of CamCalib in one command - the part of the reference's ``python scripts/camcalib_train.py --cfg FILE``
(camcalib/trainer.py:60-82,201-205) that adapts a released checkpoint to other cameras:

    python scripts/camcalib_finetune.py --cfg camcalib_config.yaml [--ckpt FILE] [--epochs 5] [--out FILE] [--augment [--train-split]]
                                        [--unfreeze layer4 [--bn batch]] [--opts OPTIMIZER.LR 0.0003 ...]

The trunk stays FROZEN and committed; only the three FC heads (fc_vfov / fc_pitch / fc_roll) are trained, on the trunk's pooled
features, under ``CameraRegressorLoss(MODEL.LOSS_*)`` with ``torch.optim.Adam(lr=OPTIMIZER.LR)``.  ``--unfreeze layer4`` also trains
the last ResNet stage, on frozen BatchNorm or with ``--bn batch`` on batch statistics with gamma / beta trained, as the reference's
``training_step`` runs it; the stem and layers 1-3 stay frozen.  ``--augment`` applies the reference's training ColorJitter (brightness, contrast, saturation 0.2, hue 0.1:
camcalib/pano_dataset.py:65) to every frame on the device, in Pillow's bytes, seeded by ``--augment-seed``; ``--train-split``
takes the frames ``train_images.pkl`` lists, as the reference's ``is_train=True`` half does.  The labelled frames are those of ``DATASET.VAL_DS`` under ``--data-root``
(``data/dataset_folders/pano`` / ``pano_scalenet``: the frames ``val_images.pkl`` lists), batched ``DATASET.BATCH_SIZE`` at a time in
a shuffle seeded by ``--seed``.  The test step runs before and after, the four ``train/...`` means are logged per epoch, and the
result is a Lightning-layout checkpoint that ``scripts/camcalib_eval.py --ckpt`` (and the reference) loads.

``--standin DIR`` first writes a small synthetic tree in the REAL formats under DIR and fine-tunes on that: a dry run of the whole
flow, the numbers are meaningless.  ``--panoramas DIR`` trains on views generated on the device from the equirectangular
panoramas under DIR (``--views-per-pano`` cameras each, drawn with ``--seed``), as ``scripts/camcalib_eval.py --panoramas``
evaluates on them.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description='Head-only fine-tuning of CamCalib on a frozen, committed trunk: the three FC heads are '
                                 'trained, nothing else.')
    ap.add_argument('--cfg', type=str, default=None, help='cfg file path (the reference\'s YAML keys)')
    ap.add_argument('--opts', default=[], nargs='*', help='additional options to update config, e.g. OPTIMIZER.LR 0.0003')
    ap.add_argument('--ckpt', type=str, default=None, help='checkpoint to start from (default: TRAINING.PRETRAINED of the config)')
    ap.add_argument('--epochs', type=int, default=1, help='passes over the labelled frames')
    ap.add_argument('--out', type=str, default=None, help='the checkpoint to write (default: LOG_DIR/camcalib_finetuned.ckpt)')
    ap.add_argument('--data-root', type=str, default='.', help='directory that holds data/')
    ap.add_argument('--standin', type=str, default=None, help='write a synthetic tree in the real formats here and fine-tune on it')
    ap.add_argument('--panoramas', type=str, default=None, metavar='DIR', help='train on views generated from the panoramas in DIR')
    ap.add_argument('--views-per-pano', type=int, default=12)
    ap.add_argument('--seed', type=int, default=0, help='seed of the shuffle (and of the camera sampler with --panoramas)')
    ap.add_argument('--augment', action='store_true', help="the reference's training ColorJitter on every frame, on the device")
    ap.add_argument('--augment-seed', type=int, default=0, help='seed of the jitter parameters')
    ap.add_argument('--train-split', action='store_true', help='train on the frames train_images.pkl lists (default: val_images.pkl)')
    ap.add_argument('--unfreeze', nargs='*', default=[], choices=['stem', 'layer1', 'layer2', 'layer3', 'layer4', 'all'], metavar='PART',
                    help="also train the conv weights of these parts of the ResNet trunk: a suffix of stem layer1 layer2 layer3 layer4 "
                         "in any order ('layer4', 'layer3 layer4', ...), or 'all'")
    ap.add_argument('--bn', choices=['frozen', 'batch'], default='frozen',
                    help="BatchNorm of the unfrozen stage: 'frozen' = its running statistics, gamma / beta untouched; 'batch' = the "
                         "reference's training mode: batch statistics, running statistics moved, gamma / beta trained (needs --unfreeze layer4)")
    ap.add_argument('--report', type=str, default=None, metavar='train.json')
    args = ap.parse_args()
    if args.bn == 'batch' and not args.unfreeze:
        ap.error("--bn batch trains the BatchNorms of an unfrozen stage: add --unfreeze layer4")
    from spec_amd import camcalib_eval as ce
    from spec_amd import camcalib_train as ct
    root, cfg = args.data_root, args.cfg
    if args.standin:
        ce.write_standin_tree(args.standin)
        root = args.standin
        cfg = cfg or os.path.join(root, ce.STANDIN_CFG)
    hp = ct.load_config(cfg, args.opts)
    dataset = None
    if args.panoramas:
        from spec_amd import panorama
        dataset = panorama.PanoViewDataset(panorama.list_panoramas(args.panoramas), args.views_per_pano, args.seed)
    res = ct.finetune_heads(hp, data_root=root, ckpt=args.ckpt, epochs=args.epochs, seed=args.seed, out=args.out, dataset=dataset,
                            augment=args.augment, augment_seed=args.augment_seed, split='train' if args.train_split else 'val',
                            unfreeze='all' if 'all' in args.unfreeze else tuple(args.unfreeze), bn=args.bn)
    if args.report:
        with open(args.report, 'w') as f:
            json.dump({k: res[k] for k in ('ckpt', 'epochs', 'before', 'after')}, f, indent=1)
        print(f'report written to {args.report}')


if __name__ == '__main__':
    main()
