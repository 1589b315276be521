#!/usr/bin/env python
"""Generate tests/golden/horizon_line.npz -- run ONLY where the reference checkout is present.

Panel 0 of the reference's three-panel picture: its OWN ``show_horizon_line`` (``camcalib/vis_utils.py``), imported from the
reference checkout by file path and called as ``render_image_group`` calls it (``spec/utils/renderer_cam.py:170-173``: colour
(0, 255, 0), width 5, debug=True, text_size 30) on one seeded 48 x 64 frame for three (vfov, pitch, roll) triples.  None of its
text is copied; only data is stored: ``frame`` (48, 64, 3) uint8, ``cam_params`` (3, 4) float64 [vfov, pitch, roll, f_pix],
``out_K`` the reference's uint8 image, ``ctr_K`` its second return value.  The caption is drawn in Pillow's default font, so the
file pins the Pillow of the image it was made in (``pillow_version``).

    python tests/golden/make_horizon_fixture.py [--reference DIR] [--out tests/golden/horizon_line.npz]
"""
import argparse
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261
# vfov, pitch, roll (radians): level, pitched down with a roll, pitched up so far that the horizon leaves the frame
TRIPLES = [(1.0, 0.0, 0.0), (0.9, -0.25, 0.12), (0.6, 0.5, -0.3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(HERE, 'horizon_line.npz'))
    args = ap.parse_args()
    path = os.path.join(args.reference, 'camcalib', 'vis_utils.py')
    if not os.path.isfile(path):
        raise SystemExit(f'{path} not found: the fixture is produced by the reference checkout only')
    spec = importlib.util.spec_from_file_location('reference_vis_utils', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import PIL
    frame = np.random.default_rng(SEED).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    data = {'frame': frame, 'pillow_version': np.array(PIL.__version__)}
    params = []
    for k, (vfov, pitch, roll) in enumerate(TRIPLES):
        f_pix = frame.shape[0] / 2.0 / np.tan(vfov / 2.0)
        params.append([vfov, pitch, roll, f_pix])
        img, ctr = mod.show_horizon_line(frame.astype(np.float64), vfov, pitch, roll, focal_length=f_pix, color=(0, 255, 0), width=5,
                                         debug=True, text_size=30)
        data[f'out_{k}'], data[f'ctr_{k}'] = img, np.float64(ctr)
    data['cam_params'] = np.asarray(params, np.float64)
    np.savez_compressed(args.out, **data)
    print('wrote', args.out, {k: getattr(v, 'shape', None) for k, v in data.items()})


if __name__ == '__main__':
    main()
