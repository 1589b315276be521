#!/usr/bin/env python
"""Generate tests/golden/camcalib_loss_grad.npz -- run ONLY where the reference checkout is present.

The gradient of ``loss`` of the reference's OWN ``camcalib/loss.py`` (CameraRegressorLoss, imported from its file over
``oracle/refshim.py``: ``loguru`` and ``softargmax1d`` are bound to the shim) with respect to the three logit tensors, by
torch.autograd on CPU fp32 with one thread, for the four loss types on the seeded cases of
``tests/camcalib_grad_ref.py: FIXTURE_CASES`` with its unequal weights, and on its saturated rows (``saturated_case``: one-hot,
all equal, a span of +-1e4) at every bin count of ``tests/head_ref.py: NBINS`` - there the fp32 autograd's own error against
float64 is what sizes the device's bound.  Stored per case and loss type: the three gradients as one (3, B, nbins) array and the
four values of ``loss_dict``.  The inputs are regenerated from the seed.  Only data is stored.

    python tests/golden/make_camcalib_loss_grad_fixture.py --reference DIR [--out tests/golden/camcalib_loss_grad.npz]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refshim  # noqa: E402

from tests import camcalib_grad_ref as R  # noqa: E402
from tests import head_ref  # noqa: E402


def import_reference_loss(reference_root):
    refshim.install(reference_root)
    for name in [n for n in sys.modules if n == 'camcalib' or n.startswith('camcalib.')]:
        del sys.modules[name]
    sys.path = [reference_root] + [p for p in sys.path if p != reference_root]
    loss = importlib.import_module('camcalib.loss')
    assert loss.__file__.startswith(reference_root), loss.__file__
    return loss


def reference_grads(module, logits, targets, loss_type, weights=R.WEIGHTS):
    """-> (grads (3, B, nbins) float32, the four loss values float32) of the reference's module under CPU fp32 autograd."""
    crit = module.CameraRegressorLoss(*weights, loss_type=loss_type)
    with torch.enable_grad():
        leaves = [torch.from_numpy(np.ascontiguousarray(x)).clone().requires_grad_(True) for x in logits]
        loss, d = crit(*leaves, *(torch.from_numpy(np.ascontiguousarray(t)) for t in targets))
        gs = torch.autograd.grad(loss, leaves)
    return np.stack([g.numpy() for g in gs]).astype(np.float32), np.array([float(d[k].detach()) for k in R.LOSS_KEYS], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='the reference checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'camcalib_loss_grad.npz'))
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one summation order, whatever the machine
    module = import_reference_loss(args.reference)
    out = {}
    for name, (B, nbins, scale) in R.FIXTURE_CASES.items():
        for lt in R.LOSS_TYPES:
            logits, targets = R.loss_case(B, nbins, lt, scale)
            out[f'{name}.{lt}.grads'], out[f'{name}.{lt}.values'] = reference_grads(module, logits, targets, lt)
    for nbins in head_ref.NBINS:
        for lt in R.LOSS_TYPES:
            logits, targets = R.saturated_case(nbins, lt)
            out[f'sat{nbins}.{lt}.grads'], out[f'sat{nbins}.{lt}.values'] = reference_grads(module, logits, targets, lt)
    out['meta'] = np.array(json.dumps({'reference_produced': 'd loss / d logits and loss_dict, camcalib/loss.py under torch.autograd, CPU fp32',
                                       'weights': R.WEIGHTS, 'leaf_bindings': dict(refshim.BOUND),
                                       'torch': torch.__version__.split('+')[0]}))
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
