"""CamCalib's test step on the device (spec_amd/camcalib_eval.py, specmi_resize_normalize_ragged, specmi_camcalib_eval), everything
through the C ABI.

Kernel-b bound.  There is no bound to inherit for the fp32 loss terms / soft-argmax / angles / errors, so it is measured against
the reference: with ``f64`` a float64 restatement from the same logits and ``e_ref = max |reference fp32 - f64|`` (the reference's
own fp32 results are in tests/golden/camcalib_eval.npz), the GPU must satisfy ``max |gpu - f64| <= 2 * e_ref + 4 ulp(max |value|)``
- factor 2 because the GPU folds the 256 terms in a shuffle tree instead of torch's order, the ulp floor for values the reference
happens to hit exactly.  The distance is the tensor max-norm of a quantity (the norm of the project's contract),
taken separately over the 1e4-magnitude row and over the ordinary rows so that the large row cannot hide the others.  It is NOT
taken element by element, and that follows from the arithmetic, not from a result: the soft-argmax is ``sp / 255 * 2 - 1`` with
``sp`` around 127, so every implementation - torch's included - carries an ABSOLUTE error of about ulp(1) whatever the final
value is; an element where the reference's rounding errors happen to cancel while the value lies near 0 would ask for an accuracy
no fp32 evaluation of that formula has (measured for the record: element by element the worst ratio is 3.35, on such an element).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from spec_amd import cam_utils
from spec_amd import camcalib_eval as ce

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'camcalib_eval.npz')
SPAN = np.array([2.1 - 0.2617, 0.6 - (-0.6), 0.6 - (-0.6)])
LO = np.array([0.2617, -0.6, -0.6])


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope='module')
def eng():
    return cam_utils._engine(torch.device(DEV))


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def f64_eval(logits, targets, gt, loss_type):
    """float64 restatement of the per-image quantities: (3, B) arrays."""
    x = np.asarray(logits, np.float64)
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    se = e.sum(-1, keepdims=True)
    lsm = x - m - np.log(se)
    soft = (e / se * np.arange(x.shape[-1])).sum(-1) / (x.shape[-1] - 1) * 2 - 1
    if loss_type in ('ce', 'kl'):
        term = -np.take_along_axis(lsm, np.asarray(targets, np.int64)[..., None], -1)[..., 0]
    else:
        tg = np.asarray(targets, np.float64)
        l2 = (tg - soft) ** 2
        term = l2.copy()
        if loss_type == 'softargmax_biased_l2':
            term[0] = np.where(soft[0] > tg[0], l2[0], l2[0] / (l2[0] + 1))
    angle = SPAN[:, None] * ((soft + 1) / 2) + LO[:, None]
    return {'loss_term': term, 'soft': soft, 'angle': angle, 'err': np.abs(angle - np.asarray(gt, np.float32).astype(np.float64))}


def torch32_eval(logits, targets, gt, loss_type):
    """The same quantities with torch's fp32 CPU operators, the arithmetic the reference's loss and decode are written in."""
    import torch.nn.functional as F
    x = torch.as_tensor(np.asarray(logits, np.float32))
    soft = (F.softmax(x, -1) * torch.arange(x.shape[-1], dtype=torch.float32)).sum(-1) / (x.shape[-1] - 1) * 2 - 1
    if loss_type in ('ce', 'kl'):
        tg = torch.as_tensor(np.asarray(targets, np.int64))
        term = -F.log_softmax(x, -1).gather(-1, tg[..., None])[..., 0]
    else:
        tg = torch.as_tensor(np.asarray(targets, np.float32))
        l2 = (tg - soft) ** 2
        term = l2.clone()
        if loss_type == 'softargmax_biased_l2':
            term[0] = torch.where(soft[0] > tg[0], l2[0], l2[0] / (l2[0] + 1))
    span, lo = torch.tensor(SPAN, dtype=torch.float32)[:, None], torch.tensor(LO, dtype=torch.float32)[:, None]
    angle = span * ((soft + 1) / 2) + lo
    err = (angle - torch.as_tensor(np.asarray(gt, np.float32))).abs()
    return {k: v.numpy() for k, v in (('loss_term', term), ('soft', soft), ('angle', angle), ('err', err))}


BIG_ROW = 3          # the row of 1e4-magnitude logits in the fixture


def norm_bound(f64, ref32):
    """2 e_ref + 4 ulp in the tensor max-norm"""
    f64, ref32 = np.asarray(f64, np.float64), np.asarray(ref32, np.float64)
    return 2 * np.abs(ref32 - f64).max() + 4 * float(ulp32(np.abs(f64).max()))


def check_bound(name, gpu, f64, ref32, report):
    """max |gpu - f64| <= 2 max |ref32 - f64| + 4 ulp(max |f64|), over the ordinary rows and over the 1e4 row; the figures are
    printed before the caller asserts."""
    gpu, f64, ref32 = (np.asarray(a, np.float64) for a in (gpu, f64, ref32))
    rows = np.arange(gpu.shape[1])
    worst = 0.0
    for tag, sel in (('rows', rows != BIG_ROW), ('1e4 row', rows == BIG_ROW)):
        e_gpu, e_ref = np.abs(gpu - f64)[:, sel].max(), np.abs(ref32 - f64)[:, sel].max()
        ratio = float(e_gpu / norm_bound(f64[:, sel], ref32[:, sel]))
        print(f'{name} [{tag}]: max |gpu-f64| {e_gpu:.3e}  e_ref {e_ref:.3e}  ratio to bound {ratio:.3f}  (gpu / ref distance {e_gpu / max(e_ref, 1e-300):.2f})')
        worst = max(worst, ratio)
    report.append((name, worst))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# kernel a
# ---------------------------------------------------------------------------------------------------------------------------
def _frames(seed, min_res=96):
    rng = np.random.default_rng(seed)
    u = min_res // 6
    out = []
    for w, h in ce.STANDIN_SHAPES[:8]:
        base = rng.integers(0, 256, ((h * u) // 8 + 1, (w * u) // 8 + 1, 3), dtype=np.uint8)
        fr = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h * u, :w * u]
        out.append((fr.astype(np.int32) + rng.integers(-20, 20, fr.shape)).clip(0, 255).astype(np.uint8))
    return out


def _single(eng, frame, oh, ow):
    from spec_amd import _lib
    from spec_amd.engine import _ptr
    f = torch.from_numpy(np.ascontiguousarray(frame)).to(DEV)
    out = torch.empty(3, oh, ow, device=DEV)
    _lib.check(eng.h, eng.lib.specmi_resize_normalize(eng.h, _ptr(f), frame.shape[0], frame.shape[1], oh, ow, _ptr(out), None, eng._stream()))
    return out


def _ragged(eng, frames, min_res=96, max_res=160, prefill=float('nan')):
    geom, offs, off = [], [], 0
    for fr in frames:
        oh, ow = ce.resize_size(fr.shape[1], fr.shape[0], min_res, max_res)
        geom.append((fr.shape[0], fr.shape[1], oh, ow)); offs.append(off); off += fr.size
    slab = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(DEV)
    out = torch.full((len(frames), 3, max(g[2] for g in geom), max(g[3] for g in geom)), prefill, device=DEV)
    return eng.resize_normalize_ragged(slab, offs, geom, out=out), geom


@pytest.mark.parametrize('n', [8, 1])
def test_kernel_a_exact_regions_and_zero_padding(eng, n):
    frames = _frames(3)[:n] if n > 1 else [_frames(3)[3]]
    out, geom = _ragged(eng, frames)
    assert eng.sync_status() == 0
    resampled = 0
    for f, (fr, (H, W, oh, ow)) in enumerate(zip(frames, geom)):
        assert torch.equal(out[f, :, :oh, :ow], _single(eng, fr, oh, ow)), f
        mask = torch.ones(out.shape[2:], dtype=torch.bool, device=DEV)
        mask[:oh, :ow] = False
        pad = out[f][:, mask]
        assert pad.numel() == 3 * (out.shape[2] * out.shape[3] - oh * ow)
        assert torch.equal(pad.view(torch.int32), torch.zeros_like(pad, dtype=torch.int32)), f    # +0.0 bit for bit (the prefill was NaN)
        resampled += (oh, ow) != (H, W)
    if n > 1:
        assert 0 < resampled < n                                               # both branches ran: resampled and converted-only frames
        assert any(min(g[2], g[3]) < 96 for g in geom)                         # a frame whose longer side hit MAX_RES
    assert eng.sync_status() == 0


def test_kernel_a_independent_of_batch_order(eng):
    frames = _frames(4)
    out, geom = _ragged(eng, frames)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    out_p, geom_p = _ragged(eng, [frames[i] for i in perm])
    assert out_p.shape == out.shape
    for j, i in enumerate(perm):
        assert geom_p[j] == geom[i] and torch.equal(out_p[j], out[i]), (j, i)
    # a different companion set changes the padded size, never the frame's own region
    out_s, geom_s = _ragged(eng, frames[:3])
    for f in range(3):
        oh, ow = geom[f][2:]
        assert torch.equal(out_s[f, :, :oh, :ow], out[f, :, :oh, :ow])
    assert eng.sync_status() == 0


def test_kernel_a_refuses_bad_geometry(eng):
    from spec_amd._lib import SpecmiError
    slab = torch.zeros(100 * 100 * 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(SpecmiError, match='leave the slab'):
        eng.resize_normalize_ragged(slab, [3], [(100, 100, 96, 96)])
    with pytest.raises(SpecmiError):
        eng.resize_normalize_ragged(slab, [0], [(100, 100, 0, 96)])
    assert eng.sync_status() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# kernel b
# ---------------------------------------------------------------------------------------------------------------------------
def test_kernel_b_parity(eng, fx):
    """Arg-max equals the fixture's exactly (first maximum on the tie); the fp32 quantities keep the bound of the module docstring;
    the 1e4-magnitude row is finite where the reference is; batch means equal the float64 mean of the kernel's own per-image values
    within 1 ulp per term and are bit-identical across two calls.

    Measured on MI355X (gfx950), worst ratio max |gpu - f64| / (2 e_ref + 4 ulp) over the four loss types and both row groups:
    loss terms 0.22, soft-argmax 0.42, angle 0.28, error 0.66; the GPU's own distance to float64 is 1.0-1.3 x the reference's for
    the loss terms and the soft-argmax and up to 2.4 x (1.7e-7 rad against 7.1e-8) for the decoded angle."""
    logits, gt = fx['logits'], fx['gt']
    report = []
    for lt in fx['loss_types'].tolist():
        tg = fx['target_bins'] if lt in ('ce', 'kl') else fx['target_soft']
        f64 = f64_eval(logits, tg, gt, lt)
        for wi, w in enumerate(fx['weights'].tolist()):
            ev = eng.camcalib_eval(*[torch.from_numpy(logits[k]).to(DEV) for k in range(3)], tg, gt.astype(np.float32), lt, w)
            ev2 = eng.camcalib_eval(*[torch.from_numpy(logits[k]).to(DEV) for k in range(3)], tg, gt.astype(np.float32), lt, w)
            assert eng.sync_status() == 0
            got = {k: v.cpu().numpy() for k, v in ev.items()}
            for k, v in ev2.items():
                assert np.array_equal(got[k].view(np.int32), v.cpu().numpy().view(np.int32)), (lt, k)     # same bits twice
            np.testing.assert_array_equal(got['argmax'], fx['argmax'])
            assert got['argmax'][0, 1] == 40 and got['argmax'][2, 1] == 42                                 # the FIRST of the two maxima
            ref = {'loss_term': fx[f'ref_term_{lt}'], 'soft': fx['ref_soft'], 'angle': fx['ref_angle_soft'], 'err': fx['ref_err_soft']}
            for k in ('loss_term', 'soft', 'angle', 'err'):
                assert np.isfinite(got[k][np.isfinite(ref[k])]).all(), (lt, k)
                assert np.isfinite(ref[k][:, 3]).all()                                                    # the 1e4 row: torch is finite
                ratio = check_bound(f'{lt} w{wi} {k}', got[k], f64[k], ref[k], report)
                assert ratio <= 1.0, (lt, k, ratio)
            # batch means: the float64 mean of the kernel's OWN per-image values, 1 ulp per term
            B = logits.shape[1]
            hl = np.array([np.float64(np.float32(w[k])) * got['loss_term'][k].astype(np.float64).mean() for k in range(3)])
            want = np.concatenate([[hl.sum()], hl, np.degrees(got['err'].astype(np.float64).mean(1))])
            tol = (B + 3) * ulp32(want)
            tol[0] = tol[1:4].sum() + 3 * ulp32(want[0])
            print(lt, w, 'means', got['means'], 'float64 of own values', want)
            assert (np.abs(got['means'].astype(np.float64) - want) <= tol).all(), (lt, w, got['means'], want)
            # and the reference's batch figures, within the per-image bound carried through the mean
            refm = fx[f'ref_loss_{lt}_w{wi}'].astype(np.float64)
            f64m = np.array([np.float32(w[k]).astype(np.float64) * f64['loss_term'][k].mean() for k in range(3)])
            f64m = np.concatenate([[f64m.sum()], f64m])
            wmax = max(w)
            btm = wmax * 3 * max(norm_bound(f64['loss_term'][:, r], ref['loss_term'][:, r]) for r in ([0, 1, 2, 4], [BIG_ROW]))
            print(lt, w, 'reference batch figures', refm, 'float64', f64m)
            assert (np.abs(got['means'][:4] - f64m) <= btm + (B + 4) * ulp32(f64m)).all(), (lt, w)
            assert (np.abs(refm - f64m) <= btm + (B + 4) * ulp32(f64m)).all(), (lt, w)       # the restatement agrees with the reference
    print('worst ratios:', {k: max(r for n, r in report if n.endswith(' ' + k)) for k in ('loss_term', 'soft', 'angle', 'err')})


def test_kernel_b_values_do_not_depend_on_the_batch(eng, fx):
    logits, gt = fx['logits'], fx['gt'].astype(np.float32)
    tg = fx['target_soft']
    full = eng.camcalib_eval(*[torch.from_numpy(logits[k]).to(DEV) for k in range(3)], tg, gt, 'softargmax_biased_l2')
    for b in range(logits.shape[1]):
        one = eng.camcalib_eval(*[torch.from_numpy(logits[k, b:b + 1]).to(DEV) for k in range(3)], tg[:, b:b + 1], gt[:, b:b + 1],
                                'softargmax_biased_l2')
        for k in ('loss_term', 'argmax', 'soft', 'angle', 'err'):
            assert torch.equal(one[k][:, 0], full[k][:, b]), (k, b)
    with pytest.raises(ValueError):
        eng.camcalib_eval(*[torch.from_numpy(logits[k]).to(DEV) for k in range(3)], tg, gt, 'l2')
    assert eng.sync_status() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the flow
# ---------------------------------------------------------------------------------------------------------------------------
CASES = [('resnet34', 'ce', (1.0, 1.0, 1.0)), ('resnet34', 'kl', (0.5, 2.0, 3.0)), ('resnet34', 'softargmax_l2', (1.0, 1.0, 1.0)),
         ('resnet34', 'softargmax_biased_l2', (0.5, 2.0, 3.0)), ('resnet50', 'ce', (1.0, 1.0, 1.0)),
         ('resnet50', 'softargmax_biased_l2', (1.0, 1.0, 1.0))]
RAN = []


@pytest.mark.parametrize('backbone,loss_type,weights', CASES)
def test_flow_equals_composition_of_existing_parts(tmp_path, eng, backbone, loss_type, weights):
    from oracle.models import CamCalibOracle, load_numpy_state
    from tests.util import cpu_threads, rel_err
    truth = ce.write_standin_tree(str(tmp_path), n_images=10, min_res=96, max_res=160, batch_size=4, backbone=backbone,
                                  loss_type=loss_type, weights=weights)
    hp = ce.load_config(str(tmp_path / ce.STANDIN_CFG))
    model = ce.build_model(hp, None, str(tmp_path), DEV)
    lines = []
    res = ce.run_evaluation(hp, str(tmp_path), model=model, log=lines.append)
    assert model.engine(torch.device(DEV)).sync_status() == 0
    assert len(lines) == 5 and lines[1].startswith('[EPOCH 0] Val loss reached ') and lines[4].startswith('[EPOCH 0] roll acc: ')
    assert [o['n'] for o in res['batches']] == [4, 4, 2] and res['logits'].shape == (3, 10, 256)
    ds = ce.PanoValDataset(hp['DATASET']['VAL_DS'], str(tmp_path))
    oracle = load_numpy_state(CamCalibOracle(backbone=backbone).eval(), truth['camcalib_state'])
    outs = []
    for bi, b0 in enumerate((0, 4, 8)):
        idx = list(range(b0, min(10, b0 + 4)))
        frames = [ds.frame(i) for i in idx]
        sizes = [ce.resize_size(f.shape[1], f.shape[0], 96, 160) for f in frames]
        padded = torch.zeros(len(idx), 3, max(s[0] for s in sizes), max(s[1] for s in sizes), device=DEV)      # to_image_list
        for k, (f, (oh, ow)) in enumerate(zip(frames, sizes)):
            padded[k, :, :oh, :ow] = _single(eng, f, oh, ow)
        assert tuple(padded.shape[2:]) == res['batches'][bi]['padded_hw']
        lg = [t.clone() for t in model(padded)]                                                               # plan pinned by build_model
        for k in range(3):
            assert torch.equal(lg[k].cpu(), torch.from_numpy(res['logits'][k, idx])), (bi, k)
        with cpu_threads():
            ref = oracle(padded.cpu())
        for k in range(3):
            assert rel_err(lg[k].cpu().numpy(), ref[k].numpy()) < 1e-4, (bi, k)
        # losses / accuracies of this batch against float64 from the same logits, the kernel-b bound carried through the mean
        # (e_ref from torch's fp32 CPU operators on these logits, the arithmetic the reference's loss is written in) + one ulp
        # per addition of the mean
        gt = truth['labels'][idx].T
        tg = ce.encode_targets(*gt, loss_type)
        x = np.stack([l.cpu().numpy() for l in lg])
        f64, t32 = f64_eval(x, np.stack(tg), gt, loss_type), torch32_eval(x, np.stack(tg), gt, loss_type)
        n = len(idx)
        w32 = np.asarray(weights, np.float32).astype(np.float64)
        bt = norm_bound(f64['loss_term'], t32['loss_term'])          # every per-image term is within it, hence their mean
        hl = w32 * f64['loss_term'].mean(1)
        tol = w32 * bt + (n + 1) * ulp32(hl)
        got = res['batches'][bi]
        print(backbone, loss_type, 'batch', bi, 'losses', [got[k] for k in ('loss', 'vfov_loss', 'pitch_loss', 'roll_loss')], 'float64', hl.sum(), hl)
        for k, name in enumerate(('vfov_loss', 'pitch_loss', 'roll_loss')):
            assert abs(got[name] - hl[k]) <= tol[k], (name, got[name], hl[k], tol[k])
        assert abs(got['loss'] - hl.sum()) <= tol.sum() + 3 * ulp32(hl.sum())
        if loss_type in ('ce', 'kl'):        # float64 bin centres on the host: exact up to the float64 mean
            centers = (cam_utils.vfov_bins_centers, cam_utils.pitch_bins_centers, cam_utils.roll_bins_centers)
            g32 = gt.astype(np.float32).astype(np.float64)
            acc = [np.degrees(np.abs(centers[k][x[k].argmax(-1)] - g32[k]).mean()) for k in range(3)]
            atol = [1e-12] * 3
        else:
            acc = np.degrees(f64['err'].mean(1))
            atol = np.degrees(norm_bound(f64['err'], t32['err'])) + (n + 2) * ulp32(acc)
        for k, name in enumerate(('vfov_acc', 'pitch_acc', 'roll_acc')):
            assert abs(got[name] - acc[k]) <= atol[k], (name, got[name], acc[k], atol[k])
        outs.append(got)
    agg = ce.epoch_end(outs)
    assert all(res[k] == agg[k] for k in agg)
    assert lines[1] == f"[EPOCH 0] Val loss reached {res['val_loss']}"
    # the padding semantics are real: one batch of ten pads to another size and moves logits
    hp10 = ce.load_config(str(tmp_path / ce.STANDIN_CFG), ['DATASET.BATCH_SIZE', '10'])
    res10 = ce.run_evaluation(hp10, str(tmp_path), model=model, log=lambda s: None)
    assert [o['n'] for o in res10['batches']] == [10]
    moved = [i for i in range(10) if not np.array_equal(res10['logits'][:, i], res['logits'][:, i])]
    assert moved, 'BATCH_SIZE 10 left every logit unchanged: the batch padding is not what the network sees'
    assert np.abs(res10['logits'] - res['logits']).max() > 1e-3
    RAN.append((backbone, loss_type, weights))


def test_sub_batches_leave_every_logit_bit_identical(tmp_path):
    ce.write_standin_tree(str(tmp_path), n_images=10, min_res=96, max_res=160, batch_size=10, loss_type='softargmax_l2')
    hp = ce.load_config(str(tmp_path / ce.STANDIN_CFG))
    model = ce.build_model(hp, None, str(tmp_path), DEV)
    whole = ce.run_evaluation(hp, str(tmp_path), model=model, log=lambda s: None)
    parts = ce.run_evaluation(hp, str(tmp_path), model=model, log=lambda s: None, sub_batch=3)
    assert np.array_equal(whole['logits'].view(np.int32), parts['logits'].view(np.int32))
    for k in ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc'):
        assert whole[k] == parts[k]
    assert model.engine(torch.device(DEV)).sync_status() == 0


def test_script_standin_as_child_process(tmp_path):
    rep = tmp_path / 'rep.json'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'camcalib_eval.py'), '--standin', str(tmp_path / 'tree'),
                        '--report', str(rep)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith('[EPOCH 0]')]
    assert len(lines) == 4 and lines[0].startswith('[EPOCH 0] Val loss reached ') and lines[1].startswith('[EPOCH 0] vfov acc: ')
    assert lines[2].startswith('[EPOCH 0] pitch acc: ') and lines[3].startswith('[EPOCH 0] roll acc: ')
    printed = [float(l.rsplit(' ', 1)[1]) for l in lines]
    hp = ce.load_config(str(tmp_path / 'tree' / ce.STANDIN_CFG))
    res = ce.run_evaluation(hp, str(tmp_path / 'tree'), log=lambda s: None)
    assert printed == [res['val_loss'], res['vfov_acc'], res['pitch_acc'], res['roll_acc']]
    with open(rep) as f:
        assert json.load(f)['val_loss'] == res['val_loss']


def test_zz_every_composition_case_ran():
    assert len(RAN) == len(CASES) == 6 and set(RAN) == set(CASES)
