#!/usr/bin/env python
"""Golden vectors for the baseline JPEG contract of ``specmi_jpeg_encode`` (spec_amd/csrc/jpeg.hip): the bytes the installed
Pillow - a libjpeg-turbo build - writes for six small seeded pictures of tests/jpeg_ref.py, with the version strings of Pillow
and of its libjpeg-turbo.  Output: tests/golden/jpeg_pillow.npz (a few KB).

    python tests/golden/make_jpeg_fixture.py
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import jpeg_ref  # noqa: E402

# (content, H, W, quality): every content once, odd sizes, both qualities the flows write and the two extremes
CASES = (('noise', 33, 47, 75), ('zeros', 7, 5, 95), ('ones', 17, 16, 75), ('checker', 24, 24, 100), ('sparse', 40, 56, 95), ('smooth', 9, 200, 1))


def main():
    if not features.check_feature('libjpeg_turbo'):
        raise SystemExit('the fixture is Pillow-on-libjpeg-turbo\'s output: this Pillow is built on another libjpeg')
    out = {'pillow_version': PIL.__version__, 'libjpeg_turbo_version': features.version('jpg'),
           'cases': np.array(['%s %d %d %d' % c for c in CASES])}
    for i, (content, H, W, q) in enumerate(CASES):
        f = io.BytesIO()
        Image.fromarray(jpeg_ref.picture(content, H, W)).save(f, format='JPEG', quality=q, optimize=False, progressive=False)
        out[f'case{i}'] = np.frombuffer(f.getvalue(), np.uint8)
    path = os.path.join(ROOT, 'tests', 'golden', 'jpeg_pillow.npz')
    np.savez_compressed(path, **out)
    print('written', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
