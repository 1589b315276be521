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

``--save-images`` / ``--no-save-images`` (default: ``TRAINING.SAVE_IMAGES`` of the config): the reference's validation pictures
(camcalib/trainer.py:118-169) - the network input of the first image of every fourth batch with the ground-truth horizon (blue,
caption at the bottom) and the predicted one (red, caption at the top), ``result_0000000_{batch:05d}.jpg`` under ``--image-dir``
(default ``LOG_DIR/val_output_images``), denormalised, drawn and encoded on the device.

``--panoramas DIR`` evaluates on views generated from the equirectangular panoramas under DIR instead of a stored validation
set - the reference's dataset generator (camcalib/datagen/generateCalibrationDataset.py) on the GPU: ``--views-per-pano``
cameras per panorama drawn from its distribution with ``--seed``, cut out on the device and fed to the network without
leaving it.  ``--write-tree OUT`` also stores these views as a 'pano_scalenet' tree under OUT (JPEG quality 95 + JSON labels +
``val_images.pkl``), which ``--data-root OUT --opts DATASET.VAL_DS pano_scalenet`` (and the reference's loader) reads.
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
    ap.add_argument('--panoramas', type=str, default=None, metavar='DIR', help='evaluate on views generated from the panoramas in DIR')
    ap.add_argument('--views-per-pano', type=int, default=12)
    ap.add_argument('--seed', type=int, default=0, help='seed of the camera sampler (--panoramas)')
    ap.add_argument('--write-tree', type=str, default=None, metavar='OUT', help='with --panoramas: also write the views as a pano_scalenet tree')
    ap.add_argument('--device-jpeg', action='store_true', help="with --write-tree: encode a panorama's views on the device in one call and "
                    "download only the files' bytes (the same bytes as Pillow's; default: engine.JPEG_DEVICE_DEFAULT)")
    ap.add_argument('--tree-format', choices=['JPEG', 'PNG'], default='JPEG', help="with --write-tree: what is encoded into the tree's image files "
                    "(write_tree's image_format; PNG takes the JPEG round trip out of a comparison between the tree and the evaluation)")
    ap.add_argument('--device-png', action='store_true', help="with --write-tree --tree-format PNG: encode a panorama's views on the device in one "
                    "call and download only the files' bytes (they decode to the same views; the bytes are not Pillow's; default: "
                    "engine.PNG_DEVICE_DEFAULT, off)")
    ap.add_argument('--device-decode', dest='device_decode', action='store_true', default=None,
                    help="send the frames' .jpg and .png files up as bytes and decode them on the device instead of with Pillow on the host (the same "
                    "pixels; defaults: engine.JPEG_DECODE_DEVICE_DEFAULT, engine.PNG_DECODE_DEVICE_DEFAULT)")
    ap.add_argument('--host-decode', dest='device_decode', action='store_false', help='decode every frame with Pillow on the host')
    ap.add_argument('--save-images', dest='save_images', action='store_true', default=None,
                    help='write the validation pictures (default: TRAINING.SAVE_IMAGES of the config)')
    ap.add_argument('--no-save-images', dest='save_images', action='store_false')
    ap.add_argument('--image-dir', type=str, default=None, help='where the validation pictures go (default: LOG_DIR/val_output_images)')
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
    dataset = None
    if args.write_tree and not args.panoramas:
        ap.error('--write-tree needs --panoramas')
    if args.panoramas:
        from spec_amd import panorama
        dataset = panorama.PanoViewDataset(panorama.list_panoramas(args.panoramas), args.views_per_pano, args.seed)
        if args.write_tree:
            panorama.write_tree(dataset, args.write_tree, while_evaluating=True,      # every view is generated once
                                image_format=args.tree_format, jpeg_device=True if args.device_jpeg else None,
                                png_device=True if args.device_png else None)
    res = ce.run_evaluation(hp, data_root=root, ckpt=args.ckpt, dataset=dataset, save_images=args.save_images, image_dir=args.image_dir,
                            jpeg_device=True if args.device_jpeg else None, jpeg_decode_device=args.device_decode,
                            png_decode_device=args.device_decode)
    if args.report:
        rep = {k: (v.tolist() if hasattr(v, 'tolist') else v) for k, v in res.items() if k != 'logits'}
        with open(args.report, 'w') as f:
            json.dump(rep, f, indent=1)
        print(f'report written to {args.report}')


if __name__ == '__main__':
    main()
