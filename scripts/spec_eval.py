#!/usr/bin/env python
"""Config 5 in one command - the MI355X counterpart of the reference's ``scripts/spec_eval.py``:

    python scripts/spec_eval.py --cfg data/spec/checkpoints/spec_config.yaml --opts DATASET.VAL_DS spec-syn

With the reference's ``data/`` tree present (README.md:127-147: licensed SMPL model, checkpoints, datasets) this loads
the Lightning checkpoint + SMPL pickle + annotations, runs every image through the hot path on the GPU in batches of
``DATASET.BATCH_SIZE`` with the dataset's precomputed CamCalib camera (or the GT camera with TESTING.USE_GT_CAM
True), writes ``evaluation_results_<ds>.pkl`` in the reference's format, scores it on the device like
``spec/utils/compute_error.py`` and prints W-MPJPE / PA-MPJPE / W-PVE beside the README table (README.md:155-159).
Every batch is also scored on the device as the reference's ``validation_step`` scores it, against the dataset's own ground
truth: the per-joint arrays ``mpjpe``, ``pampjpe``, ``mpjpe_24``, ``pampjpe_24`` of the pkl, the five ``<ds> MPJPE: ...`` lines and
``val_accuracy_results_<ds>.json`` (``--no-step-metrics`` leaves them out).

``--standin DIR`` first writes a small synthetic ``data/`` tree in the REAL container formats under DIR and evaluates
that (a dry run of the whole flow; the numbers are meaningless).  ``--synthetic N`` is the quick in-memory variant.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(args):
    """In-memory stand-in: ground truth = the model's own prediction + noise, scored with the device metrics."""
    from spec_amd import assets, synth, metrics, io_formats
    from spec_amd.cam_utils import cam_params_from_angles
    from spec_amd.modules import HMR
    dev = torch.device('cuda')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    N = args.synthetic
    smpl = assets.use_synthetic_assets(1003)
    hm = HMR(use_cam=True, use_cam_feats=True)
    hm.load_state_dict({k: t(v) for k, v in synth.hmr_state(1002, True).items()}, strict=False)
    hm.to(dev).eval().commit(dev, freeze=True)
    scale, center, img_w, img_h = synth.bbox_inputs(5, N, 640., 480.)
    rng = np.random.default_rng(0)
    ang = rng.uniform(-0.4, 0.4, (N, 2)).astype(np.float32)
    R, K = cam_params_from_angles(ang[:, 0], ang[:, 1], rng.uniform(300, 900, N).astype(np.float32), img_w, img_h)
    img = synth.images(123, N)
    J24 = t(smpl['J_regressor']).to(dev)
    Jh = t(synth.h36m_regressor(1003)).to(dev)
    dump = io_formats.EvalDump()
    acc = {'w_mpjpe_24': [], 'pa_mpjpe_24': [], 'w_v2v': []}
    for b0 in range(0, N, args.batch_size):
        sl = slice(b0, min(N, b0 + args.batch_size))
        pred = hm(t(img[sl]).to(dev), R[sl], K[sl], t(scale[sl]).to(dev), t(center[sl]).to(dev), t(img_w[sl]).to(dev),
                  t(img_h[sl]).to(dev))                         # positional call order of spec/trainer.py:139
        dump.add(pred)
        g = torch.Generator(device=dev).manual_seed(b0)        # synthetic ground truth: prediction + 1 cm noise + offset
        gt = pred['smpl_vertices'] + 0.01 * torch.randn(pred['smpl_vertices'].shape, device=dev, generator=g) + 0.05
        gt_j24 = metrics.regress_joints(gt, J24)               # stands for the GT kinematic-chain joints
        mp, pa = metrics.w_mpjpe_24(pred['smpl_vertices'], gt_j24, J24)
        _, _, v2v = metrics.eval_single(pred['smpl_vertices'], gt, Jh)
        acc['w_mpjpe_24'].append(mp); acc['pa_mpjpe_24'].append(pa); acc['w_v2v'].append(v2v)
    path = dump.write(args.log_dir, args.dataset_name)
    res = {k: float(torch.cat(v).mean()) for k, v in acc.items()}
    print(f'***** RESULTS ON {args.dataset_name.upper()} ({N} samples) *****')
    print(f"W-MPJPE-24: {res['w_mpjpe_24']:.3f}\nPA-MPJPE-24: {res['pa_mpjpe_24']:.3f}\nW-V2V: {res['w_v2v']:.3f}")
    print('dump:', path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', type=str, default=None, help='cfg file path (reference: data/spec/checkpoints/spec_config.yaml)')
    ap.add_argument('--opts', default=[], nargs='*', help='additional options to update config')
    ap.add_argument('--data-root', type=str, default='.', help='directory that holds data/ (the reference runs from its repo root)')
    ap.add_argument('--ckpt', type=str, default=None, help='checkpoint (default: TRAINING.PRETRAINED_LIT of the config, '
                                                            'else data/spec/checkpoints/spec_checkpoint.ckpt)')
    ap.add_argument('--limit', type=int, default=None, help='evaluate only the first N samples of each dataset')
    ap.add_argument('--standin', type=str, default=None, help='write a synthetic data/ tree in the real formats here and evaluate it')
    ap.add_argument('--synthetic', type=int, default=0)
    ap.add_argument('--batch_size', type=int, default=64)
    ap.add_argument('--log_dir', type=str, default='logs/eval')
    ap.add_argument('--dataset_name', type=str, default='spec-syn')
    ap.add_argument('--loss', action='store_true', help="also report the mean of HMRCamLoss's loss dict (the training objective of "
                                                        'spec/losses.py, forward value only) over each dataset; off by default')
    ap.add_argument('--no-step-metrics', action='store_true', help="do not score the batches as the reference's validation step does "
                    '(the per-joint arrays of the pkl, the five "<ds> MPJPE: ..." lines, val_accuracy_results_<ds>.json)')
    ap.add_argument('--save-images', action='store_true', help='one three-panel picture (full image with the 2D keypoints and horizon line | mesh '
                    'overlay | side view) of the first image of every TESTING.SAVE_FREQ-th batch under LOG_DIR/output_images: sets '
                    'TESTING.SAVE_IMAGES and TRAINING.SAVE_IMAGES (the reference writes the files only with both)')
    ap.add_argument('--device-jpeg', action='store_true', help='with --save-images: encode .jpg / .jpeg pictures on the device and download '
                    "only the files' bytes (the same bytes as Pillow's; default: engine.JPEG_DEVICE_DEFAULT)")
    ap.add_argument('--device-png', action='store_true', help='with --save-images: encode .png pictures on the device and download only the '
                    "files' bytes (they decode to the same pictures; the bytes are not Pillow's; default: engine.PNG_DEVICE_DEFAULT, off)")
    ap.add_argument('--ragged-crops', action='store_true', help="a batch's images in one slab, one upload and one crop launch instead of one of "
                    'each per sample (the same crops; default: engine.RAGGED_CROPS_DEFAULT).  The device decode below is part of this route only')
    ap.add_argument('--device-decode', dest='device_decode', action='store_true', default=None,
                    help="with --ragged-crops: send a batch's .jpg and .png files up as bytes and decode them on the device instead of with Pillow on "
                    "the host (the same pixels; defaults: engine.JPEG_DECODE_DEVICE_DEFAULT, engine.PNG_DECODE_DEVICE_DEFAULT)")
    ap.add_argument('--host-decode', dest='device_decode', action='store_false', help='with --ragged-crops: decode every frame with Pillow on the host')
    ap.add_argument('--device-panel0', action='store_true', help='with --save-images: draw the horizon line and caption of panel 0 on the '
                    "device instead of with Pillow on the host (the same bytes; default: engine.PANEL0_DEVICE_DEFAULT)")
    ap.add_argument('--report', type=str, default=None, metavar='eval.json',
                    help='write the scores and the delta against the reference README table (README.md:155-159) as JSON; the exit '
                         'code is 3 when |delta W-MPJPE| > 0.1 mm on a dataset the table lists (use on the real assets)')
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if args.device_jpeg:
        from spec_amd import engine
        engine.JPEG_DEVICE_DEFAULT = True
    if args.device_png:
        from spec_amd import engine
        engine.PNG_DEVICE_DEFAULT = True
    if args.device_panel0:
        from spec_amd import engine
        engine.PANEL0_DEVICE_DEFAULT = True
    if args.ragged_crops:
        from spec_amd import engine
        engine.RAGGED_CROPS_DEFAULT = True
    if args.device_decode is not None:
        from spec_amd import engine
        engine.JPEG_DECODE_DEVICE_DEFAULT = engine.PNG_DECODE_DEVICE_DEFAULT = args.device_decode
    if args.synthetic:
        return synthetic(args)
    from spec_amd import evaluation
    root = args.data_root
    cfg = args.cfg
    if args.standin:
        evaluation.write_standin_data_tree(args.standin, dataset=args.dataset_name)
        root = args.standin
        cfg = cfg or os.path.join(root, 'data/spec/checkpoints/spec_config.yaml')
    if cfg is None and os.path.exists(os.path.join(root, 'data/spec/checkpoints/spec_config.yaml')):
        cfg = os.path.join(root, 'data/spec/checkpoints/spec_config.yaml')
    hp = evaluation.load_config(cfg, args.opts)
    if args.save_images:
        hp['TESTING']['SAVE_IMAGES'] = hp['TRAINING']['SAVE_IMAGES'] = True
    ckpt = args.ckpt
    if ckpt is None and hp['TRAINING']['PRETRAINED_LIT'] is None:
        ckpt = 'data/spec/checkpoints/spec_checkpoint.ckpt'          # scripts/spec_demo.py:31
    if not os.path.isdir(os.path.join(root, 'data')):
        sys.exit(f'{os.path.join(root, "data")} not found: download the reference data (README.md:127-147) or use --standin DIR')
    results = evaluation.run_evaluation(hp, data_root=root, ckpt=ckpt, limit=args.limit, loss=args.loss, step_metrics=not args.no_step_metrics)
    if args.report:
        import json
        rep = {'config': cfg, 'checkpoint': ckpt or hp['TRAINING']['PRETRAINED_LIT'], 'data_root': os.path.abspath(root),
               'standin_tree': bool(args.standin), 'limit': args.limit, 'target_abs_delta_wmpjpe_mm': 0.1,
               'precision': evaluation.eval_precision(hp), 'datasets': {}}
        ok = True
        for name, res in results.items():
            m, ref = res['mean'], evaluation.README_TABLE.get(name)
            entry = {'mean': {k: float(v) for k, v in m.items()}, 'readme': None, 'delta_mm': res.get('readme_delta_mm'), 'within_target': None}
            if 'loss' in res:
                entry['loss'] = res['loss']
            if 'step' in res:
                entry['step'] = res['step']['acc']
            if ref:
                entry['readme'] = {'wmpjpe': ref[0], 'pampjpe': ref[1], 'wpve': ref[2]}
                entry['within_target'] = abs(res['readme_delta_mm']['wmpjpe']) <= 0.1
                ok = ok and entry['within_target']
            rep['datasets'][name] = entry
        rep['pass'] = ok
        with open(args.report, 'w') as f:
            json.dump(rep, f, indent=1)
        print(f'report written to {args.report}: pass = {ok}' + (' (stand-in tree: synthetic weights, the README delta is not meaningful)' if args.standin else ''))
        if not ok and not args.standin:
            sys.exit(3)


if __name__ == '__main__':
    main()
