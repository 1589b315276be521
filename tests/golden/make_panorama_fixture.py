#!/usr/bin/env python
"""Generate tests/golden/pano_views.npz -- run ONLY where the reference checkout is present.

Perspective views cut out of two small seeded panoramas by the reference's OWN ``extractImage``
(``camcalib/datagen/image_extraction.py``, ``mode="image"``), imported from the reference checkout over import-time
stubs: ``skimage.io`` (a top-level import the function never reaches for an array input) and the numpy aliases
``np.product`` / ``np.mat`` that numpy 2 removed.  None of its text is copied; only data is stored:

* ``pano_even`` (48, 96, 3) and ``pano_odd`` (47, 95, 3) uint8 - the historical ``mode="wrap"`` of
  ``scipy.ndimage.map_coordinates`` has period N - 1, so both parities matter;
* ``views`` (n, 5) float64 [elevation, azimuth, roll (rad), vfov (deg), ratio], ``heights`` (n,), ``out_hw`` (n, 2),
  ``pano_of`` (n,) 0 = even / 1 = odd;
* per view ``u8_K`` = the reference's uint8 output, ``f64_K`` = the same call with ``out_dtype="float64"`` (the value
  before scipy's rounding) and ``tie_K`` = |frac(f64) - 0.5| <= 1e-6: the pixels where one ulp in a coordinate may move
  the rounded value by one.  The generator asserts that at most 1 pixel in 1000 is such a near tie.

    python tests/golden/make_panorama_fixture.py [--reference DIR] [--out tests/golden/pano_views.npz]
    python tests/golden/make_panorama_fixture.py --selfcheck      # regenerate and compare with the committed file, bit for bit
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_OUT = os.path.join(HERE, 'pano_views.npz')
SEED = 20260
TIE_EPS = 1e-6
PANOS = (('pano_even', (48, 96, 3)), ('pano_odd', (47, 95, 3)))
PI = float(np.pi)
# (pano, elevation, azimuth, roll, vfov_deg, ratio, output_height)
VIEWS = [
    (0, 0.0, 0.0, 0.0, 67.5, 4 / 3, 24),              # even width 32: the centre column falls between two texels
    (0, 0.0, 0.0, 0.0, 67.5, 1.0, 25),                # odd width 25: the centre column is the panorama's centre
    (1, 0.0, 0.0, 0.0, 67.5, 3 / 4, 40),              # portrait on the odd panorama
    (0, 0.3, PI - 0.05, PI / 6, 120.0, 4 / 3, 30),    # across the +pi seam, wide
    (1, -0.3, -PI + 0.05, -PI / 6, 120.0, 4 / 3, 30),  # across the -pi seam
    (0, 0.0, PI, 0.0, 67.5, 4 / 3, 15),               # centred ON the seam
    (1, 0.0, -PI, PI, 15.0, 1.0, 17),                 # upside down, narrow
    (0, 1.5, 0.4, 0.0, 67.5, 4 / 3, 27),              # at the upper pole (elevation pixel reaches PH)
    (1, 1.5, -2.0, PI / 6, 120.0, 3 / 4, 36),
    (0, -1.5, 2.5, -PI / 6, 120.0, 1.0, 33),          # at the lower pole
    (1, -1.5, 0.0, PI, 67.5, 4 / 3, 21),
    (0, 0.7, 1.0, PI, 15.0, 3 / 4, 40),
    (1, -0.7, -1.0, PI / 6, 15.0, 4 / 3, 12),
    # output height 1: linspace(-fovY, fovY, 1) is the single sample -fovY.  (A 1 x 1 view - height 1 at ratio 4/3, 3/4 or 1 -
    # makes the reference's own np.mat product raise, so these two use wider ratios: widths 2 and 5.)
    (0, 0.2, 3.0, -PI / 6, 67.5, 16 / 9, 1),
    (1, 0.0, 0.0, 0.0, 120.0, 5.0, 1),
    (0, 0.1, -3.1, PI / 6, 67.5, 3 / 4, 2),           # width round(1.5) = 2: Python's round-half-to-even
    (1, np.pi / 2, 0.0, 0.0, 67.5, 1.0, 9),           # looking straight up: the centre pixel has elevation pi/2 exactly
]


def import_extract_image(reference_root):
    """The reference's image_extraction module, loaded from its own file over the import-time stubs."""
    path = os.path.join(reference_root, 'camcalib', 'datagen', 'image_extraction.py')
    if not os.path.isfile(path):
        raise SystemExit(f'{path} not found: the fixture is produced by the reference checkout only')
    if 'skimage.io' not in sys.modules:
        sk, io = types.ModuleType('skimage'), types.ModuleType('skimage.io')
        io.imread = io.imsave = None
        sk.io = io
        sys.modules['skimage'], sys.modules['skimage.io'] = sk, io
    if not hasattr(np, 'product'):
        np.product = np.prod
    if not hasattr(np, 'mat'):
        np.mat = np.asmatrix
    import warnings
    spec = importlib.util.spec_from_file_location('reference_image_extraction', path)
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                # scipy.ndimage.interpolation is a deprecated name
        spec.loader.exec_module(mod)
    assert os.path.abspath(mod.__file__).startswith(os.path.abspath(reference_root))
    return mod


def generate(reference_root, seed=SEED):
    ie = import_extract_image(reference_root)
    rng = np.random.default_rng(seed)
    out = {name: rng.integers(0, 256, shape, dtype=np.uint8) for name, shape in PANOS}
    panos = [out[name] for name, _ in PANOS]
    views, heights, hw, ties, total = [], [], [], 0, 0
    import warnings
    for k, (p, el, az, roll, vfov, ratio, h) in enumerate(VIEWS):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            u8 = ie.extractImage(panos[p], [el, az, roll], h, vfov=vfov, ratio=ratio)
            f64 = ie.extractImage(panos[p], [el, az, roll], h, vfov=vfov, ratio=ratio, out_dtype='float64')
        assert u8.dtype == np.uint8 and f64.dtype == np.float64 and u8.shape == f64.shape == (h, round(h * ratio), 3), u8.shape
        assert u8.shape[0] <= 40 and u8.shape[1] <= 60
        tie = np.abs(f64 - np.floor(f64) - 0.5) <= TIE_EPS
        out[f'u8_{k}'], out[f'f64_{k}'], out[f'tie_{k}'] = u8, f64, tie
        views.append((el, az, roll, vfov, ratio)); heights.append(h); hw.append(u8.shape[:2])
        ties += int(tie.sum()); total += tie.size
    out['views'] = np.asarray(views, np.float64)
    out['heights'] = np.asarray(heights, np.int32)
    out['out_hw'] = np.asarray(hw, np.int32)
    out['pano_of'] = np.asarray([v[0] for v in VIEWS], np.int32)
    share = ties / total
    assert share <= 1e-3, f'{ties} near-tie pixels of {total} ({share:.2e}): pick another seed'
    out['meta'] = np.array(json.dumps({'seed': seed, 'tie_eps': TIE_EPS, 'near_tie': ties, 'values': total,
                                       'reference_produced': ['u8_*', 'f64_*'], 'derived': ['tie_*']}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('SPEC_REFERENCE', '/root/reference'))
    ap.add_argument('--out', default=DEFAULT_OUT)
    ap.add_argument('--selfcheck', action='store_true', help='regenerate and compare with --out bit for bit (writes nothing)')
    args = ap.parse_args()
    out = generate(args.reference)
    meta = json.loads(str(out['meta']))
    if args.selfcheck:
        have = np.load(args.out)
        bad = [k for k in out if k not in have.files or have[k].dtype != out[k].dtype or have[k].shape != out[k].shape
               or have[k].tobytes() != out[k].tobytes()]
        bad += [k for k in have.files if k not in out]
        print(f'selfcheck: {len(out)} arrays, {len(bad)} differ {bad[:8]}; near ties {meta["near_tie"]} of {meta["values"]}')
        return 1 if bad else 0
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes;', meta)
    return 0


if __name__ == '__main__':
    sys.exit(main())
