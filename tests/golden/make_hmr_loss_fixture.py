#!/usr/bin/env python
"""Generate tests/golden/hmr_loss.npz -- run ONLY where the reference checkout is present.

The reference's OWN ``spec/losses.py`` (HMRLoss and HMRCamLoss), loaded from its file and run on CPU fp32 on the four seeded
cases of ``tests/hmr_loss_ref.py: CASES`` (single image; mixed ``has_smpl`` / ``has_pose_3d``; all masks 0; non-default
weights with ``openpose_train_weight`` != 0, some confidences 0 and non-square ``orig_shape``).  The file imports ``loguru`` and
three ``pare`` modules at import time; they are stubbed HERE.  Of those names the two modules call exactly one,
``pare.utils.geometry.batch_rodrigues``, and it is bound to the restatement of ``tests/hmr_loss_ref.py`` evaluated in fp32:
the fixture therefore pins everything in ``losses.py`` except that one function.

Stored: per case the seed, every small input tensor, a float64 checksum of the two vertex tensors (they are regenerated from
the seed by the tests, never stored), the constructor weights and the seven values of each module's ``loss_dict``.

    python tests/golden/make_hmr_loss_fixture.py [--reference /root/reference] [--out tests/golden/hmr_loss.npz]
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import hmr_loss_ref as ref  # noqa: E402

SMALL_PRED = ('pred_pose', 'pred_shape', 'pred_cam', 'smpl_joints3d')
SMALL_GT = ('pose', 'betas', 'pose_conf', 'pose_3d', 'keypoints', 'keypoints_orig', 'has_smpl', 'has_pose_3d', 'orig_shape', 'scale')


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference_losses(reference_root):
    class _Logger:
        def __getattr__(self, _name):
            return lambda *a, **k: None

    def batch_rodrigues(theta):
        return torch.from_numpy(ref.batch_rodrigues(theta.detach().numpy().astype(np.float32)))

    saved = {k: sys.modules.get(k) for k in ('loguru', 'pare', 'pare.losses', 'pare.losses.keypoints', 'pare.losses.segmentation',
                                             'pare.utils', 'pare.utils.geometry')}
    _stub('loguru', logger=_Logger())
    _stub('pare'); _stub('pare.losses'); _stub('pare.utils')
    _stub('pare.losses.keypoints', JointsMSELoss=None)
    _stub('pare.losses.segmentation', CrossEntropy=None)
    _stub('pare.utils.geometry', batch_rodrigues=batch_rodrigues, rotmat_to_rot6d=None)
    try:
        path = os.path.join(reference_root, 'spec', 'losses.py')
        spec = importlib.util.spec_from_file_location('_reference_spec_losses', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert mod.__file__.startswith(reference_root), mod.__file__
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hmr_loss.npz'))
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)                       # one summation order, whatever the machine
    L = import_reference_losses(args.reference)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {}
    for name in ref.CASES:
        for mode, cls in ((0, L.HMRLoss), (1, L.HMRCamLoss)):
            pred, gt, weights = ref.case_inputs(name, mode)
            fn = cls(**weights)
            loss, d = fn({k: t(v).clone() for k, v in pred.items()}, {k: t(v) for k, v in gt.items()})
            assert tuple(d) == ref.KEYS and float(loss) == float(d['loss/total_loss'])
            out[f'{name}.ref{mode}'] = np.array([float(d[k]) for k in ref.KEYS], np.float32)
            out[f'{name}.joints2d{mode}'] = pred['smpl_joints2d']
        for k in SMALL_PRED:
            out[f'{name}.{k}'] = pred[k]
        for k in SMALL_GT:
            out[f'{name}.{k}'] = gt[k]
        out[f'{name}.vertex_checksum'] = np.array([pred['smpl_vertices'].astype(np.float64).sum(), gt['vertices'].astype(np.float64).sum()])
        out[f'{name}.weights'] = np.array(json.dumps(weights))
        out[f'{name}.seed_B_V'] = np.array([ref.CASE_SEED[name], ref.CASES[name][0], ref.CASES[name][1]], np.int64)
    out['meta'] = np.array(json.dumps({'reference_produced': ['*.ref0 (HMRLoss)', '*.ref1 (HMRCamLoss)'], 'keys': list(ref.KEYS),
                                       'restated_leaf': 'pare.utils.geometry.batch_rodrigues (tests/hmr_loss_ref.py, fp32)',
                                       'torch': torch.__version__.split('+')[0]}))
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
