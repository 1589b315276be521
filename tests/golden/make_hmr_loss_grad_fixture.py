#!/usr/bin/env python
"""Generate tests/golden/hmr_loss_grad.npz -- run ONLY where the reference checkout is present.

The gradient of ``loss/total_loss`` of the reference's OWN ``spec/losses.py`` (HMRLoss and HMRCamLoss, loaded from its file as
``make_hmr_loss_fixture.import_reference_losses`` loads it, ``batch_rodrigues`` of the ground truth bound to the fp32 restatement)
with respect to the six prediction tensors, by torch.autograd on CPU fp32, on the four seeded cases of
``tests/hmr_loss_ref.py: CASES`` in both modes.  The prediction handed to the module is ``leaf * 1.0``: HMRCamLoss writes
``pred['smpl_joints2d']`` in place (:191), which autograd refuses on a leaf.  A term masked out entirely leaves ``None``, stored
as zeros.

Stored per case and mode: the five small gradients whole; of d/d smpl_vertices (B x 6890 x 3) per image the count of non-zeros,
the least and largest magnitude among them and the float64 dot product with a seeded probe
(``tests/hmr_loss_grad_ref.py: vertex_summary``).  The inputs are regenerated from the seed, as for hmr_loss.npz.

    python tests/golden/make_hmr_loss_grad_fixture.py --reference DIR [--out tests/golden/hmr_loss_grad.npz]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_hmr_loss_fixture import import_reference_losses  # noqa: E402

from tests import hmr_loss_grad_ref as G  # noqa: E402
from tests import hmr_loss_ref as ref  # noqa: E402

SMALL = ('pred_pose', 'pred_shape', 'pred_cam', 'smpl_joints3d', 'smpl_joints2d')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='the reference checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'hmr_loss_grad.npz'))
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one summation order, whatever the machine
    L = import_reference_losses(args.reference)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {}
    for name in ref.CASES:
        B, V = ref.CASES[name][:2]
        for mode, cls in ((0, L.HMRLoss), (1, L.HMRCamLoss)):
            pred, gt, weights = ref.case_inputs(name, mode)
            with torch.enable_grad():
                leaves = {k: t(pred[k]).clone().requires_grad_(True) for k in ref.PRED_KEYS}
                loss, d = cls(**weights)({k: v * 1.0 for k, v in leaves.items()}, {k: t(v) for k, v in gt.items()})
                gs = torch.autograd.grad(loss.sum(), [leaves[k] for k in ref.PRED_KEYS], allow_unused=True)
            g = {k: (np.zeros(pred[k].shape, np.float32) if gi is None else gi.numpy()) for k, gi in zip(ref.PRED_KEYS, gs)}
            for k in SMALL:
                out[f'{name}.{mode}.{k}'] = g[k].astype(np.float32)
            out[f'{name}.{mode}.vertex_summary'] = G.vertex_summary(g['smpl_vertices'], G.probe(B, V))
            out[f'{name}.{mode}.total'] = np.float32(float(loss.detach().sum()))
    out['meta'] = np.array(json.dumps({'reference_produced': 'd loss/total_loss / d pred, spec/losses.py under torch.autograd, CPU fp32',
                                       'restated_leaf': 'pare.utils.geometry.batch_rodrigues (tests/hmr_loss_ref.py, fp32)',
                                       'probe_seed': G.PROBE_SEED, 'torch': torch.__version__.split('+')[0]}))
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
