#!/usr/bin/env python
"""Generate tests/golden/color_jitter.npz -- needs only the installed Pillow.

A few small seeded frames, their jitter records and what PILLOW makes of them (``ImageEnhance.Brightness`` / ``Contrast`` /
``Color`` and the HSV shift of torchvision's ``adjust_hue``, applied in the record's order by ``pil_jitter`` of
tests/test_color_jitter_host.py), so that the GPU tests do not depend on the Pillow of the machine they run on.  Stored:
``sizes`` (n, 2) [H, W], ``records`` (n, 8) int32, ``frames`` and ``outputs`` as the frames' bytes back to back, and
``pillow_version``.  Frames 0 .. 3 are 1 x 1, 1 x 7, 5 x 3 and 37 x 53 with drawn parameters; 4 .. 27 one 16 x 16 frame in all 24
orders; 28 .. 33 records with operations switched off; 34 the two-pixel frame whose mean L is the tie 10.5.

    python tests/golden/make_color_jitter_fixture.py [--out tests/golden/color_jitter.npz]
"""
import argparse
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SEED = 20271


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'color_jitter.npz'))
    args = ap.parse_args()
    import PIL
    import torch
    from spec_amd import augment
    from tests import color_jitter_ref as R
    from tests.test_color_jitter_host import pil_jitter
    rng = np.random.default_rng(SEED)
    frame = lambda H, W: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    cj = augment.ColorJitter(**augment.CAMCALIB_TRAIN_JITTER)
    g = torch.Generator().manual_seed(SEED)
    frames = [frame(H, W) for H, W in ((1, 1), (1, 7), (5, 3), (37, 53))]
    records = [cj.record(cj.get_params(g)) for _ in frames]
    f16 = frame(16, 16)
    for order in itertools.permutations(range(4)):
        frames.append(f16)
        records.append(R.make_record(order, (1.13, 0.87, 1.19), augment.hue_shift(-0.07)))
    for order in ((), (3,), (1,), (2, 0), (3, 1, 0), (0, 2, 3)):
        frames.append(frame(9, 13))
        records.append(R.make_record(order, (0.8, 1.2, 0.0), 231))
    frames.append(np.asarray([[[10, 10, 10], [11, 11, 11]]], np.uint8))
    records.append(R.make_record((1,), (1.0, 0.0, 1.0), 0))
    records = np.stack(records).astype(np.int32)
    outputs = [pil_jitter(fr, [op for op in rec[:4] if op >= 0], rec[4:7].view(np.float32).tolist(), int(rec[7])) for fr, rec in zip(frames, records)]
    data = {'sizes': np.asarray([fr.shape[:2] for fr in frames], np.int32), 'records': records,
            'frames': np.concatenate([fr.reshape(-1) for fr in frames]), 'outputs': np.concatenate([o.reshape(-1) for o in outputs]),
            'pillow_version': np.array(PIL.__version__)}
    np.savez_compressed(args.out, **data)
    print('wrote', args.out, {k: getattr(v, 'shape', None) for k, v in data.items()})


if __name__ == '__main__':
    main()
