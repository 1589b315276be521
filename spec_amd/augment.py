"""Training augmentation on the device.  ``ColorJitter`` is the one step by which the reference's
``CameraRegressorDataset(is_train=True)`` differs from its validation half (camcalib/pano_dataset.py:62-78):
``transforms.ColorJitter(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1)`` on the PIL frame before ``Resize``.  Here the
frames stay in the uint8 slab the decoders and ``pano_extract_views`` left them in, and ``specmi_color_jitter`` applies the four
Pillow operations byte for byte.  There is no host fallback; the NumPy restatement of the
contract lives in tests/color_jitter_ref.py.

The parameters are drawn as torchvision's ``ColorJitter.get_params`` / ``forward`` draw them, from a torch CPU generator:
``torch.randperm(4)`` - read with ``tolist()`` -, then one ``torch.empty(1).uniform_(lo, hi)`` for each of brightness, contrast,
saturation and hue that is set.  torchvision is not a dependency: the rule is restated, parity with its random stream is not
pinned."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

# camcalib/pano_dataset.py:65
CAMCALIB_TRAIN_JITTER = dict(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1)


def hue_shift(hue: float) -> int:
    """torchvision's ``np.uint8(hue_factor * 255)`` as the HSV shift k: truncation toward zero, mod 256 (-0.1 -> 231, 0.1 -> 25)"""
    return int(math.trunc(float(hue) * 255.0)) % 256


class ColorJitter:
    """torchvision's ``ColorJitter(brightness, contrast, saturation, hue)`` for frames in a device slab.  A number x sets the range
    [max(0, 1 - x), 1 + x] (hue: [-x, x], 0 <= x <= 0.5), a pair sets it directly, None or 0 switches the operation off."""

    def __init__(self, brightness=None, contrast=None, saturation=None, hue=None):
        self.brightness = self._range(brightness, 'brightness')
        self.contrast = self._range(contrast, 'contrast')
        self.saturation = self._range(saturation, 'saturation')
        self.hue = self._range(hue, 'hue', center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def _range(value, name, center=1.0, bound=(0.0, float('inf')), clip_first_on_zero=True) -> Optional[Tuple[float, float]]:
        if value is None:
            return None
        if isinstance(value, (int, float)):
            if value < 0:
                raise ValueError(f'If {name} is a single number, it must be non negative.')
            lo, hi = center - float(value), center + float(value)
            if clip_first_on_zero:
                lo = max(lo, 0.0)
        else:
            lo, hi = (float(v) for v in value)
        if not bound[0] <= lo <= hi <= bound[1]:
            raise ValueError(f'{name} values should be between {bound}, got ({lo}, {hi}).')
        return None if lo == hi == center else (lo, hi)

    def get_params(self, generator: Optional[torch.Generator] = None):
        """-> (order, brightness, contrast, saturation, hue): the permutation of the ids 0 brightness, 1 contrast, 2 saturation,
        3 hue as a list, and a Python float per operation, None where it is switched off (no draw is made for it)"""
        order = torch.randperm(4, generator=generator).tolist()
        draw = lambda r: None if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=generator))
        return (order,) + tuple(draw(r) for r in (self.brightness, self.contrast, self.saturation, self.hue))

    def record(self, params) -> np.ndarray:
        """The parameters of one ``get_params`` as the eight int32 words of ``specmi_color_jitter``'s record"""
        order, values = params[0], params[1:]
        ids = [int(op) for op in order if values[int(op)] is not None]
        factors = np.asarray([1.0 if v is None else v for v in values[:3]], dtype=np.float32)
        k = 0 if values[3] is None else hue_shift(values[3])
        return np.asarray(ids + [-1] * (4 - len(ids)) + factors.view(np.int32).tolist() + [k], dtype=np.int32)

    def records(self, n: int, generator: Optional[torch.Generator] = None) -> np.ndarray:
        """``n`` draws in frame order -> the (n, 8) int32 host array of the call"""
        return np.stack([self.record(self.get_params(generator)) for _ in range(int(n))]).reshape(int(n), _lib.JITTER_REC)

    def __call__(self, frames, generator: Optional[torch.Generator] = None, engine=None, out=None):
        """``frames`` = (slab, offsets, sizes) as ``pack_frames`` and ``PanoViewDataset.device_batch`` build it -> the same tuple
        with the jittered frames in a new slab (``out`` = the slab itself: in place), which ``camcalib_eval.pad_batch`` accepts."""
        slab, offsets, sizes = frames
        if engine is None:
            from . import cam_utils
            engine = cam_utils._engine(slab.device)
        recs = self.records(len(sizes), generator)
        return engine.color_jitter(slab, offsets, sizes, recs, out=out), offsets, sizes
