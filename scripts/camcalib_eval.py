#!/usr/bin/env python
"""CamCalib's test step in one command - the MI355X counterpart of the reference's
``python scripts/camcalib_train.py --cfg FILE`` with ``RUN_TEST: True`` (scripts/camcalib_train.py:91-93):

    python scripts/camcalib_eval.py --cfg camcalib_config.yaml [--ckpt FILE] [--opts DATASET.VAL_DS pano_scalenet ...]

reads the validation set under ``--data-root`` (``data/dataset_folders/pano`` / ``pano_scalenet``), batches
``DATASET.BATCH_SIZE`` frames the way the reference's collator does (each resized with Resize(MIN_RES, MAX_RES), padded with
zeros to the batch's largest size), runs CamCalib, the configured loss and the decode on the GPU and prints the four lines
the reference logs at epoch end: val loss, vfov / pitch / roll mean absolute error in degrees.

``--standin DIR`` first writes a small synthetic tree in the REAL formats under DIR (frames of mixed sizes, JSON labels,
``val_images.pkl``, a Lightning-layout checkpoint, the YAML config) and evaluates that: a dry run of the whole flow, the
numbers are meaningless.  ``--report FILE`` writes the result (without the logits) as JSON.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', type=str, default=None, help='cfg file path (the reference\'s YAML keys)')
    ap.add_argument('--opts', default=[], nargs='*', help='additional options to update config')
    ap.add_argument('--ckpt', type=str, default=None, help='checkpoint (default: TRAINING.PRETRAINED of the config)')
    ap.add_argument('--data-root', type=str, default='.', help='directory that holds data/')
    ap.add_argument('--standin', type=str, default=None, help='write a synthetic tree in the real formats here and evaluate it')
    ap.add_argument('--report', type=str, default=None, metavar='eval.json')
    args = ap.parse_args()
    import torch
    torch.set_grad_enabled(False)
    from spec_amd import camcalib_eval as ce
    root, cfg = args.data_root, args.cfg
    if args.standin:
        ce.write_standin_tree(args.standin)
        root = args.standin
        cfg = cfg or os.path.join(root, ce.STANDIN_CFG)
    hp = ce.load_config(cfg, args.opts)
    res = ce.run_evaluation(hp, data_root=root, ckpt=args.ckpt)
    if args.report:
        rep = {k: (v.tolist() if hasattr(v, 'tolist') else v) for k, v in res.items() if k != 'logits'}
        with open(args.report, 'w') as f:
            json.dump(rep, f, indent=1)
        print(f'report written to {args.report}')


if __name__ == '__main__':
    main()
