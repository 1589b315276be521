#!/usr/bin/env python
"""Drop-in for the reference's ``scripts/camcalib_demo.py`` (same flags: --img_folder --out_folder --loss --ckpt --show
--no_save) on MI355X: CamCalib on every image of a folder, one ``<image name>.pkl`` with ``{'vfov','f_pix','pitch','roll'}``
per image in ``--out_folder`` (what ``spec/utils/cam_params.py:28-35`` reads back) and, without ``--no_save``, the image with
the predicted horizon line and caption next to it under the image's own name (scripts/camcalib_demo.py:154-155,217-218 of the
reference: ``show_horizon_line(..., debug=True, color=(255, 0, 0), width=3)``, drawn on the host with Pillow - with
``--device-horizon`` on the device by ``render.show_horizon_lines``, one image at a time: the same pixels).  The logit plots of
``--show`` (matplotlib) are not produced."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CKPT = 'data/camcalib/checkpoints/camcalib_sa_biased_l2.ckpt'


def main(args):
    import torch
    from spec_amd.tester import run_camcalib_folder
    torch.set_grad_enabled(False)
    if args.img_folder in (None, '-'):
        sys.exit('only --img_folder input is built (the dataset modes need the Pano360 / SPEC datasets)')
    if args.show:
        print('[camcalib_demo] the logit plots of --show are not produced by this build', file=sys.stderr)
    res = run_camcalib_folder(args.img_folder, args.out_folder, ckpt=args.ckpt or CKPT, loss_type=args.loss)
    if not args.no_save:
        from PIL import Image
        from spec_amd.render import show_horizon_line
        from spec_amd.tester import _read_rgb
        from spec_amd.render import plan_horizon_marks, show_horizon_lines
        for img_fname, rec in res.items():
            rgb = _read_rgb(img_fname)
            kw = dict(vfov=float(rec['vfov']), pitch=float(rec['pitch']), roll=float(rec['roll']), focal_length=float(rec['f_pix']), debug=True,
                      color=(255, 0, 0), width=3, GT=False)
            if args.device_horizon and plan_horizon_marks([rgb.shape[:2]], [[kw]]) is not None:
                slab = torch.from_numpy(rgb.reshape(-1)).cuda()
                show_horizon_lines(slab, [rgb.shape[:2]], [0], [[kw]])
                img = slab.cpu().numpy().reshape(rgb.shape)
            else:
                img, _ = show_horizon_line(rgb, kw.pop('vfov'), kw.pop('pitch'), kw.pop('roll'), **kw)
            Image.fromarray(img).save(os.path.join(args.out_folder, os.path.basename(img_fname)))
    print(f'CamCalib: {len(res)} images -> {args.out_folder}')


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('--img_folder', help='input image folder', type=str)
    parser.add_argument('--out_folder', help='output folder', type=str)
    parser.add_argument('--dataset', type=str, default=None)
    parser.add_argument('--loss', default='softargmax_l2')
    parser.add_argument('--ckpt', default=CKPT)
    parser.add_argument('--show', help='visualize raw network predictions', action='store_true')
    parser.add_argument('--no_save', help='do not save output images', action='store_true')
    parser.add_argument('--device-horizon', help='draw the horizon line and caption of the saved images on the device (same pixels)',
                        action='store_true')
    main(parser.parse_args())
