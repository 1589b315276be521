#!/usr/bin/env python
"""Generate tests/golden/camcalib_eval.npz -- run ONLY where the reference checkout is present.

What CamCalib's test step computes after the network, produced by the reference's OWN modules on seeded logits:

* ``camcalib/loss.py: CameraRegressorLoss`` for the four loss types with the weights (1, 1, 1) and (0.5, 2, 3) on the
  batch, and on every image alone (a batch of one: the mean is the image's own term);
* ``camcalib/cam_utils.py: convert_preds_to_angles`` ('ce' -> float64 bin centres, 'softargmax_l2' -> fp32 angles) and
  ``get_softargmax``;
* ``camcalib/pano_dataset.py: Resize.get_size`` on a table of sizes and ``to_image_list`` on three small tensors.

The two first modules import over ``oracle/refshim.py`` (``loguru`` and ``softargmax1d`` are bound to the shim, as in
``make_fixtures.py``); ``pano_dataset.py`` additionally needs cv2, albumentations, torchvision and the yacs-based
``camcalib/config.py`` at import time only - they are stubbed HERE with empty modules (none of them is touched by
``get_size`` / ``to_image_list``).  ``camcalib/trainer.py`` subclasses Lightning's module and cannot be imported without
it: its three accuracy lines (:111-113, ``|pred - gt|.mean().rad2deg()``) are restated below in this file's own words.
``meta`` in the fixture says which arrays are reference-produced and which are restated.  Only data is stored.

    python tests/golden/make_camcalib_eval_fixture.py [--reference /root/reference] [--out tests/golden/camcalib_eval.npz]
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from spec_amd import synth  # noqa: E402
from oracle import refshim  # noqa: E402

LOSS_TYPES = ('ce', 'kl', 'softargmax_l2', 'softargmax_biased_l2')
WEIGHTS = ((1.0, 1.0, 1.0), (0.5, 2.0, 3.0))
SEED, B, NBINS = 4242, 5, 256
TIE_ROW, BIG_ROW = 1, 3
# (w, h, min_size, max_size): cap hit (landscape, portrait), cap not hit, square, already at size, truncation, no cap
SIZES = [(1920, 1080, 600, 1000), (1080, 1920, 600, 1000), (800, 600, 600, 1000), (600, 800, 600, 1000), (1000, 1000, 600, 1000),
         (640, 480, 600, 1000), (1067, 600, 600, 1000), (600, 1067, 600, 1000), (1066, 600, 600, 1000), (3840, 2160, 600, 1000),
         (4000, 1000, 600, 1000), (1000, 4000, 600, 1000), (1001, 600, 600, 1000), (1333, 750, 600, 1000), (999, 601, 600, 1000),
         (601, 999, 600, 1000), (256, 112, 96, 160), (128, 96, 96, 160), (96, 144, 96, 160), (144, 112, 96, 160), (112, 160, 96, 160),
         (500, 375, 600, 1000), (375, 500, 600, 1000), (1920, 1080, 600, None), (123, 457, 224, 333), (457, 123, 224, 333)]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference(reference_root):
    refshim.install(reference_root)
    for name in [n for n in sys.modules if n == 'camcalib' or n.startswith('camcalib.')]:
        del sys.modules[name]
    sys.path = [reference_root] + [p for p in sys.path if p != reference_root]
    loss = importlib.import_module('camcalib.loss')
    cu = importlib.import_module('camcalib.cam_utils')
    pd = None
    try:
        for n in ('cv2', 'albumentations'):
            if not refshim.have(n):
                _stub(n)
        if not refshim.have('torchvision'):
            tv, tr = _stub('torchvision'), _stub('torchvision.transforms')
            tv.transforms = tr
            tr.functional = _stub('torchvision.transforms.functional')
        _stub('camcalib.config', DATASET_FOLDERS={})
        iu = _stub('pare.utils.image_utils', read_img=None, denormalize_images=None)
        sys.modules['pare.utils'].image_utils = iu
        pd = importlib.import_module('camcalib.pano_dataset')
    except Exception as e:                       # noqa: BLE001 - any import failure means: restate
        print('camcalib.pano_dataset does not import over stubs:', repr(e))
    for m in (loss, cu) + ((pd,) if pd else ()):
        assert m.__file__.startswith(reference_root), m.__file__
    return loss, cu, pd


def inputs():
    """Seeded logits (3, B, 256) with a tie for the maximum in one row and one row of magnitude 1e4, ground-truth angles."""
    logits = synth.normal(SEED, 'camcalib_eval.logits', (3, B, NBINS), std=3.0).astype(np.float32)
    for k in range(3):
        r = logits[k, TIE_ROW]
        r[40 + k] = r[200 - k] = np.float32(r.max() + 1.5)                      # two equal maxima: the FIRST one counts
        logits[k, BIG_ROW] = (synth.uniform(SEED, f'camcalib_eval.big{k}', (NBINS,), -1.0, 1.0) * 1e4).astype(np.float32)
    u = synth.uniform(SEED, 'camcalib_eval.gt', (3, B))
    gt = np.stack([0.3 + 1.7 * u[0], -0.55 + 1.1 * u[1], -0.5 + 1.0 * u[2]]).astype(np.float64)
    return logits, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'camcalib_eval.npz'))
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    L, CU, PD = import_reference(args.reference)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    logits, gt = inputs()
    out = {'logits': logits, 'gt': gt, 'weights': np.asarray(WEIGHTS), 'loss_types': np.array(LOSS_TYPES)}
    meta = {'reference_produced': ['ref_loss_*', 'ref_term_*', 'ref_angle_bins', 'ref_angle_soft', 'ref_soft', 'target_bins', 'target_soft'],
            'restated': ['ref_err_*', 'ref_acc_*'], 'leaf_bindings': dict(refshim.BOUND)}

    # ---- ground-truth encoding with the reference's tables / helpers (the calls of pano_dataset.py:135-142) ----------------
    tb = np.stack([np.digitize(gt[0], CU.vfov_bins), np.digitize(gt[1], CU.pitch_bins), np.digitize(gt[2], CU.roll_bins)]).astype(np.int64)
    ts = np.stack([t(CU.vfov2soft_idx(gt[0])).float().numpy(), t(CU.pitch2soft_idx(gt[1])).float().numpy(),
                   t(CU.roll2soft_idx(gt[2])).float().numpy()])
    out['target_bins'], out['target_soft'] = tb, ts
    gt32 = gt.astype(np.float32)                               # torch.tensor(python float) of the dataset item

    # ---- CameraRegressorLoss ---------------------------------------------------------------------------------------------------
    for lt in LOSS_TYPES:
        tg = tb if lt in ('ce', 'kl') else ts
        for wi, w in enumerate(WEIGHTS):
            fn = L.CameraRegressorLoss(vfov_loss_weight=w[0], pitch_loss_weight=w[1], roll_loss_weight=w[2], loss_type=lt)
            _, d = fn(t(logits[0]), t(logits[1]), t(logits[2]), t(tg[0]), t(tg[1]), t(tg[2]))
            out[f'ref_loss_{lt}_w{wi}'] = np.array([float(d[k]) for k in ('loss', 'vfov_loss', 'pitch_loss', 'roll_loss')], np.float32)
        fn = L.CameraRegressorLoss(loss_type=lt)
        term = np.zeros((3, B), np.float32)
        for b in range(B):                                     # a batch of one: the mean is the image's own term
            _, d = fn(*[t(logits[k, b:b + 1]) for k in range(3)], *[t(tg[k, b:b + 1]) for k in range(3)])
            term[:, b] = [float(d['vfov_loss']), float(d['pitch_loss']), float(d['roll_loss'])]
        out[f'ref_term_{lt}'] = term

    # ---- convert_preds_to_angles ---------------------------------------------------------------------------------------------
    ab = CU.convert_preds_to_angles(t(logits[0]), t(logits[1]), t(logits[2]), loss_type='ce')
    out['ref_angle_bins'] = np.stack([np.asarray(a, dtype=np.float64) for a in ab])
    asf = CU.convert_preds_to_angles(t(logits[0]), t(logits[1]), t(logits[2]), loss_type='softargmax_l2')
    out['ref_angle_soft'] = np.stack([a.numpy().astype(np.float32).reshape(-1) for a in asf])
    out['ref_soft'] = np.stack([CU.get_softargmax(t(logits[k])).numpy().astype(np.float32).reshape(-1) for k in range(3)])
    out['argmax'] = np.argmax(logits, axis=-1).astype(np.int32)                 # np.argmax, as bins2* call it
    centers = (CU.vfov_bins_centers, CU.pitch_bins_centers, CU.roll_bins_centers)
    assert all(np.array_equal(centers[k][out['argmax'][k]], out['ref_angle_bins'][k]) for k in range(3))

    # ---- accuracies: trainer.py:111-113 restated (absolute difference, batch mean, degrees) ------------------------------------
    for name, pred in (('soft', out['ref_angle_soft']), ('bins', out['ref_angle_bins'])):
        err = (t(pred) - t(gt32)).abs()
        out[f'ref_err_{name}'] = err.numpy()
        out[f'ref_acc_{name}'] = np.stack([err[k].mean().rad2deg().numpy() for k in range(3)])

    # ---- Resize.get_size / to_image_list ---------------------------------------------------------------------------------------
    if PD is not None:
        got = [PD.Resize(mn, mx).get_size((w, h)) for w, h, mn, mx in SIZES]
        meta['reference_produced'] += ['size_out', 'pad_out']
        g = torch.Generator().manual_seed(SEED)
        small = [torch.randn(3, 4, 5, generator=g), torch.randn(3, 6, 2, generator=g), torch.randn(3, 5, 5, generator=g)]
        il = PD.to_image_list(small)
        out['pad_in0'], out['pad_in1'], out['pad_in2'] = (s.numpy() for s in small)
        out['pad_out'] = il.tensors.numpy()
    else:
        # in this file's own words: aim the shorter side at min_size; if the longer side would then pass max_size, aim the
        # longer side at max_size instead; keep a frame that already has the aimed size; truncate the other side
        def get_size(w, h, mn, mx):
            short, long_ = min(w, h), max(w, h)
            aim = mn
            if mx is not None and long_ / float(short) * aim > mx:
                aim = int(round(mx * float(short) / long_))
            if short == aim:
                return h, w
            return (int(aim * h / w), aim) if w < h else (aim, int(aim * w / h))
        got = [get_size(*s) for s in SIZES]
        meta['restated'] += ['size_out']
    out['size_in'] = np.array([[w, h, mn, -1 if mx is None else mx] for w, h, mn, mx in SIZES], np.int64)
    out['size_out'] = np.array(got, np.int64)
    out['meta'] = np.array(json.dumps(meta))
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes;', meta)


if __name__ == '__main__':
    main()
