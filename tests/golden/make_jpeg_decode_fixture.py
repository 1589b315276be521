"""Writes tests/golden/jpeg_decode.npz: a handful of baseline JPEG files with the pixels Pillow (on libjpeg-turbo) decodes them to,
and the versions that did.  It pins tests/jpeg_dec_ref.py where the installed Pillow is built on another libjpeg.
Run from the repository root:  python -m tests.golden.make_jpeg_decode_fixture"""
import io
import os

import numpy as np

from tests import jpeg_ref

CASES = (('noise', 33, 47, dict(quality=95)), ('smooth', 65, 130, dict(quality=75)), ('checker', 24, 24, dict(quality=100)),
         ('sparse', 40, 56, dict(quality=50, optimize=True)), ('noise', 17, 16, dict(quality=90, subsampling=0)),
         ('noise', 2, 3, dict(quality=75)), ('zeros', 7, 5, dict(quality=1)))


def main():
    import PIL
    from PIL import Image, features
    assert features.check_feature('libjpeg_turbo'), 'the contract is Pillow on libjpeg-turbo'
    out = {'cases': np.array([f'{c} {h} {w} {sorted(kw.items())}' for c, h, w, kw in CASES]), 'pillow_version': np.array(PIL.__version__),
           'libjpeg_turbo_version': np.array(features.version('libjpeg_turbo'))}
    for i, (content, H, W, kw) in enumerate(CASES):
        f = io.BytesIO()
        Image.fromarray(jpeg_ref.picture(content, H, W)).save(f, format='JPEG', **kw)
        out[f'file{i}'] = np.frombuffer(f.getvalue(), np.uint8)
        out[f'pixels{i}'] = np.array(Image.open(io.BytesIO(f.getvalue())).convert('RGB'))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg_decode.npz'), **out)


if __name__ == '__main__':
    main()
