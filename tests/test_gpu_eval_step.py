"""``specmi_eval_step`` (spec_amd/csrc/eval.hip) through the C ABI against the float64 yardstick tests/eval_step_ref.py, and the
flow that calls it.  Everything per joint and in metres.  Tolerances (derived in tests/eval_step_ref.py; the host test
tests/test_eval_step_host.py shows the yardstick passes each on these very inputs):
  err ................................ 1 fp32 ulp of the float64 value (fp64 arithmetic + one final rounding)
  pa_err ............................. max(2 fp32 ulp, 10 x |Kabsch - Horn| of that joint in float64); below 1e-9 m where the float64
                                       value is below 1e-11 m; NaN exactly where the reference's 0 / 0 is
  V2V on dyadic meshes ............... (ceil(V / 256) + 13) 2^-24 relative
  against eval_mesh / eval_joints .... half an ulp of the mean + the mean of half an ulp of every joint (two roundings of one value)
  NULL outputs, batch position ....... the same bits"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from spec_amd import _lib
from tests import eval_step_ref as R
from tests import metrics_ref as M
from tests.util import t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0x5A5AA5A5
PAD = 64
NAMES = ('err_sel', 'pa_err_sel', 'err_k', 'pa_err_k', 'v2v')


def _abi():
    from spec_amd.cam_utils import _engine
    eng = _engine(torch.device(DEV))
    return eng.lib, eng.h


def _p(a):
    return None if a is None else C.c_void_p(a.data_ptr())


def _dev(a):
    return t(np.array(a)).to(DEV)       # a copy: the shared inputs are read-only


def _err(lib, h):
    return (lib.specmi_last_error(h) or b'').decode()


def _sizes(B, nsel, Jk):
    return {'err_sel': B * nsel, 'pa_err_sel': B * nsel, 'err_k': B * Jk, 'pa_err_k': B * Jk, 'v2v': B}


def _call(pv, gv, w, sel, nsel, pj, gj, Jk, skip=(), expect=_lib.OK):
    """One call through the ABI with every output but ``skip`` given and a sentinel pad behind each -> {name: float32 array}, after
    checking the pads (and, on a refusal, every word)."""
    lib, h = _abi()
    B, V = pv.shape[0], pv.shape[1]
    sizes = _sizes(B, nsel, Jk)
    bufs = {k: torch.full((sizes[k] + PAD,), SENTINEL, dtype=torch.int32, device=DEV) for k in NAMES if k not in skip}
    rc = lib.specmi_eval_step(h, _p(pv), _p(gv), B, V, _p(w), w.shape[0], _p(sel), nsel, _p(pj), _p(gj), Jk,
                              *(_p(bufs.get(k)) for k in NAMES), None)
    assert rc == expect, (rc, _err(lib, h))
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        a = b.cpu().numpy()
        assert np.all(a[sizes[k]:] == SENTINEL), (k, 'wrote past the output')
        if expect != _lib.OK:
            assert np.all(a == SENTINEL), (k, 'a refused call wrote')
            continue
        out[k] = a[:sizes[k]].view(np.float32).reshape((B, -1) if k != 'v2v' else (B,)).copy()
    return out


def _sel(sel):
    return torch.tensor(sel, dtype=torch.int32, device=DEV)


# ---- exact regression ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', R.STEP_V)
def test_exact_regression_sweep(V):
    """V of one vertex, of a second trip for one lane and of several trips with a ragged tail; J on both sides of the chunk of 6 and
    at the cap; selections of 1, 14 and 32 joints (unordered, repeats, joint 0); Jk of 1, 24 and 32; B of 1 and 3.  The regressed
    joints are exact on these inputs, so every per-joint value is held to the rule of ``check_per_joint`` and V2V to its summation
    bound."""
    for J in R.STEP_J:
        for B in R.BATCHES:
            pred, gt, Jr = R.mesh(V, J, B)
            pv, gv, w = _dev(pred), _dev(gt), _dev(Jr)
            vv = R.raw_v2v(pred, gt)
            for sel in M.selections(J):
                ref_sel = R.mesh_per_joint(pred, gt, Jr, sel)
                for Jk in R.STEP_JK:
                    pj, gj = R.dyadic_joints(B, Jk)
                    got = _call(pv, gv, w, _sel(sel), len(sel), _dev(pj), _dev(gj), Jk)
                    why = R.check_per_joint(got['err_sel'], got['pa_err_sel'], *ref_sel)
                    assert why is None, (V, J, B, len(sel), why)
                    why = R.check_per_joint(got['err_k'], got['pa_err_k'], *R.given_per_joint(pj, gj))
                    assert why is None, (V, J, B, Jk, why)
                    assert np.all(np.abs(got['v2v'].astype(np.float64) - vv) <= R.v2v_bound(V) * vv), (V, J, B, got['v2v'], vv)


# ---- Procrustes on the inputs that break solvers -------------------------------------------------------------------------------

_CASES = M.procrustes_cases()
_MESH = R.mesh(257, 7, 3)


def _given(pred, gt):
    """The given-joints path alone, the batch in slices of the small mesh's three images."""
    outs = []
    for b0 in range(0, len(pred), 3):
        p, g = pred[b0:b0 + 3], gt[b0:b0 + 3]
        n = len(p)
        outs.append(_call(_dev(_MESH[0][:n]), _dev(_MESH[1][:n]), _dev(_MESH[2]), None, 1, _dev(p), _dev(g), p.shape[1],
                          skip=('err_sel', 'pa_err_sel', 'v2v')))
    return np.concatenate([o['err_k'] for o in outs]), np.concatenate([o['pa_err_k'] for o in outs])


@pytest.mark.parametrize('family', sorted(_CASES))
def test_procrustes_families(family):
    """``metrics_ref.procrustes_cases`` through the given-joints path, per joint: exact fits (identity, every proper signed
    permutation with a scale and a shift, a mirrored coplanar set, two joints) stay below 1e-9 m at every joint; reflections equal
    the Kabsch value with the det fix; zero variance is NaN at every joint with finite err; the inversion of an octahedron (no
    unique mean distance) keeps the mean of its joints inside the range of the unique squared optimum."""
    pred, gt, expect = _CASES[family]
    err, pk, ph = R.given_per_joint(pred, gt)
    g_err, g_pa = _given(pred, gt)
    if family == 'identity':
        assert np.all(g_err == 0.0)
    if expect == 'range':
        n = pred.shape[1]
        lam = M.horn_eigenvalues(pred[0] - pred[0, :1], gt[0] - gt[0, :1])[-1]
        x1, x2 = pred[0].astype(np.float64) - pred[0].mean(0), gt[0].astype(np.float64) - gt[0].mean(0)
        rms = np.sqrt(((x2 ** 2).sum() - lam ** 2 / (x1 ** 2).sum()) / n)             # the unique squared optimum: var2 - lam^2 / var1
        assert np.all(np.abs(g_err - err) <= M.ulp32(err))
        assert rms / np.sqrt(n) * (1 - 1e-6) <= float(g_pa[0].astype(np.float64).mean()) <= rms * (1 + 1e-6), (g_pa, rms)
        return
    why = R.check_per_joint(g_err, g_pa, err, pk, ph)
    assert why is None, (family, why)
    if expect == 'zero':
        assert np.all(g_pa < R.EXACT_FIT_M), (family, g_pa.max())
    elif expect == 'nan':
        assert np.all(np.isnan(g_pa)) and np.all(np.isfinite(g_err))
    else:
        assert np.all(np.isfinite(g_pa)) and np.all(pk.mean(-1) >= R.EXACT_FIT_M)


# ---- consistency with the existing calls ---------------------------------------------------------------------------------------

def test_means_agree_with_eval_mesh_and_eval_joints():
    """1000 x the mean of the per-joint errors against the per-image millimetres of specmi_eval_mesh / specmi_eval_joints on dyadic
    inputs: both sides round the same float64 quantities, so they differ by the two roundings (``mean_consistency_bound``)."""
    from spec_amd import metrics
    for V, J, B, Jk in ((257, 17, 3, 24), (1200, 7, 3, 32)):
        pred, gt, Jr = R.mesh(V, J, B)
        pj, gj = R.dyadic_joints(B, Jk)
        pv, gv, w = _dev(pred), _dev(gt), _dev(Jr)
        for sel in M.selections(J)[1:]:
            got = _call(pv, gv, w, _sel(sel), len(sel), _dev(pj), _dev(gj), Jk)
            mp = metrics.eval_single(pv, gv, w, joint_sel=sel)[0].cpu().numpy().astype(np.float64)
            mk = metrics.eval_j_24(_dev(pj), _dev(gj))[0].cpu().numpy().astype(np.float64)
            for mean_mm, e in ((mp, got['err_sel']), (mk, got['err_k'])):
                e = e.astype(np.float64)
                diff, bound = np.abs(1000 * e.mean(-1) - mean_mm), R.mean_consistency_bound(mean_mm, e)
                assert np.all(mean_mm > 1) and np.all(diff <= bound), (V, J, len(sel), diff, bound)


# ---- NULL outputs ----------------------------------------------------------------------------------------------------------------

def test_null_outputs_and_null_joints():
    """Every single output NULL, and the joint inputs NULL with their two outputs: what remains has the bits of the full call, and
    the pad behind every buffer keeps its sentinel.  joint_sel NULL selects the first nsel joints."""
    V, J, B, Jk = 257, 17, 3, 24
    pred, gt, Jr = R.mesh(V, J, B)
    sel = M.selections(J)[1]
    pv, gv, w, s = _dev(pred), _dev(gt), _dev(Jr), _sel(sel)
    pj, gj = (_dev(a) for a in R.dyadic_joints(B, Jk))
    full = _call(pv, gv, w, s, len(sel), pj, gj, Jk)
    assert set(full) == set(NAMES) and all(np.isfinite(v).all() for v in full.values())
    for skip in NAMES:
        part = _call(pv, gv, w, s, len(sel), pj, gj, Jk, skip=(skip,))
        assert set(part) == set(NAMES) - {skip}
        for k, v in part.items():
            assert np.array_equal(v.view(np.int32), full[k].view(np.int32)), (skip, k)
    part = _call(pv, gv, w, s, len(sel), None, None, 12345, skip=('err_k', 'pa_err_k'))      # Jk is not read
    for k, v in part.items():
        assert np.array_equal(v.view(np.int32), full[k].view(np.int32)), k
    first = _call(pv, gv, w, _sel(list(range(5))), 5, None, None, 0, skip=('err_k', 'pa_err_k'))
    none = _call(pv, gv, w, None, 5, None, None, 0, skip=('err_k', 'pa_err_k'))
    for k in first:
        assert np.array_equal(first[k].view(np.int32), none[k].view(np.int32)), k


# ---- batch invariance, NaN isolation ---------------------------------------------------------------------------------------------

def test_batch_invariance_and_nan_isolation():
    """Image i alone gives the bits of image i in a batch of 5, and an image without variance (a mesh collapsed to one point, given
    joints all coincident) makes only its own pa_err NaN."""
    V, J, B, Jk = 1200, 17, 5, 24
    pred, gt, Jr = (a.copy() for a in R.mesh(V, J, B))
    pj, gj = (a.copy() for a in R.dyadic_joints(B, Jk))
    sel = list(M.H36M_TO_J14)
    w, s = _dev(Jr), _sel(sel)
    clean = _call(_dev(pred), _dev(gt), w, s, len(sel), _dev(pj), _dev(gj), Jk)
    for i in range(B):
        alone = _call(_dev(pred[i:i + 1]), _dev(gt[i:i + 1]), w, s, len(sel), _dev(pj[i:i + 1]), _dev(gj[i:i + 1]), Jk)
        for k in NAMES:
            assert np.array_equal(alone[k].view(np.int32), clean[k][i:i + 1].view(np.int32)), (i, k)
    bad = 2
    pred[bad] = 0.0                                     # every regressed joint of the prediction at the origin
    pj[bad] = pj[bad, :1]
    got = _call(_dev(pred), _dev(gt), w, s, len(sel), _dev(pj), _dev(gj), Jk)
    keep = np.arange(B) != bad
    for k in ('pa_err_sel', 'pa_err_k'):
        assert np.all(np.isnan(got[k][bad])) and np.array_equal(got[k][keep].view(np.int32), clean[k][keep].view(np.int32)), k
    for k in ('err_sel', 'err_k', 'v2v'):
        assert np.all(np.isfinite(got[k])) and np.array_equal(got[k][keep].view(np.int32), clean[k][keep].view(np.int32)), k
    assert R.check_per_joint(got['err_sel'], got['pa_err_sel'], *R.mesh_per_joint(pred, gt, Jr, sel)) is None
    assert R.check_per_joint(got['err_k'], got['pa_err_k'], *R.given_per_joint(pj, gj)) is None


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_argument_refusals():
    """Every refusal gives SPECMI_ERR_ARG in eval_mesh's words, launches nothing and writes nothing; the edges next to them run."""
    lib, h = _abi()
    x = torch.zeros(1, 64, 3, device=DEV)
    w33, w17 = torch.zeros(33, 64, device=DEV), torch.zeros(17, 64, device=DEV)
    s = torch.zeros(40, dtype=torch.int32, device=DEV)
    j = torch.zeros(1, 40, 3, device=DEV)
    ARG = _lib.ERR_ARG
    _call(x, x, w33, s, 14, j, j, 24, expect=ARG)
    assert '[1,32]' in _err(lib, h)
    _call(x, x, w17, s, 33, j, j, 24, expect=ARG)
    assert '[1,32]' in _err(lib, h)
    _call(x, x, w17, s, 0, j, j, 24, expect=ARG)
    _call(x, x, w17, s, 14, j, j, 33, expect=ARG)
    assert '[1,32]' in _err(lib, h)
    _call(x, x, w17, s, 14, j, j, 0, expect=ARG)
    _call(x, x, w17, None, 18, j, j, 24, expect=ARG)
    assert 'nsel = 18' in _err(lib, h) and 'J = 17' in _err(lib, h)
    _call(x, x, w17, s, 14, j, None, 24, expect=ARG)
    _call(x, x, w17, s, 14, None, j, 24, expect=ARG)
    _call(x, x, w17, s, 14, None, None, 24, expect=ARG)                                   # joint outputs without joint inputs
    _call(x, x, w17, s, 14, None, None, 24, skip=('err_k',), expect=ARG)
    _call(x, x, w17, s, 14, None, None, 24, skip=('pa_err_k',), expect=ARG)
    _call(x[:0], x[:0], w17, s, 14, j, j, 24, expect=ARG)                                 # B = 0
    _call(x[:, :0], x[:, :0], w17[:, :0], s, 14, j, j, 24, expect=ARG)                    # V = 0
    # the handle stays usable, and the edges run: the cap on all three, one vertex
    w32 = torch.ones(32, 1, device=DEV)
    got = _call(x[:, :1], x[:, :1], w32, None, 32, j[:, :32].contiguous(), j[:, :32].contiguous(), 32)
    assert np.all(got['err_sel'] == 0) and np.all(np.isnan(got['pa_err_k'])) and np.all(got['v2v'] == 0)


# ---- the flow --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dataset', ['spec-syn', 'spec-mtp'])
def test_flow_writes_the_validation_step_results(tmp_path, dataset):
    """Six images in batches of four (the last one short).  The pkl's per-joint arrays are bit for bit what
    ``metrics.validation_errors`` gives on tensors recomputed with the same device calls (the flow adds no arithmetic; the
    arithmetic is pinned above); the five lines and the json hold 1000 x their means; with ``step_metrics=False`` the pkl, the
    log and the folder are what they were without the feature."""
    import joblib
    from spec_amd import assets, evaluation, metrics
    d = str(tmp_path)
    evaluation.write_standin_data_tree(d, n_images=6, dataset=dataset)
    cfg = os.path.join(d, 'data/spec/checkpoints/spec_config.yaml')
    hp = evaluation.load_config(cfg)
    assert hp['DATASET']['BATCH_SIZE'] == 4
    log_dir = os.path.join(d, 'logs/eval_standin')
    off = []
    res_off = evaluation.run_evaluation(hp, data_root=d, log=off.append, step_metrics=False)[dataset]
    pkl = os.path.join(log_dir, f'evaluation_results_{dataset}.pkl')
    ev_off = joblib.load(pkl)
    assert sorted(os.listdir(log_dir)) == [f'evaluation_results_{dataset}.pkl'] and 'step' not in res_off
    assert set(ev_off) == {'pose', 'shape', 'cam', 'vertices', 'imgname', 'dataset_name'}
    assert not any(l.startswith(f'{dataset} MPJPE') or 'val_accuracy' in l for l in off)
    on = []
    res = evaluation.run_evaluation(hp, data_root=d, log=on.append)[dataset]
    ev = joblib.load(pkl)
    assert sorted(os.listdir(log_dir)) == [f'evaluation_results_{dataset}.pkl', f'val_accuracy_results_{dataset}.json']
    for k, v in ev_off.items():                          # nothing the old run wrote has changed
        assert np.array_equal(ev[k], v), k
    assert [l for l in on if l in off] == off            # the old lines, in their order
    for k in res_off['mean']:
        assert res['mean'][k] == res_off['mean'][k]
    shapes = {'mpjpe': (6, 14), 'pampjpe': (6, 14), 'mpjpe_24': (6, 24), 'pampjpe_24': (6, 24)}
    for k, shp in shapes.items():
        assert ev[k].shape == shp and ev[k].dtype == np.float32 and np.isfinite(ev[k]).all() and ev[k].min() >= 0, k
    # the same device calls, made here
    body = metrics.BodyModel(assets.smpl_model(), device=DEV)      # (run_evaluation has loaded the tree's body model)
    ds = evaluation.EvalDataset(dataset, d)
    Jh = _dev(np.load(os.path.join(d, 'data/J_regressor_h36m.npy')))
    want = {k: [] for k in list(shapes) + ['v2v']}
    for idx in (np.arange(0, 4), np.arange(4, 6)):
        gt = ds.eval_gt(idx, DEV, body)
        pose, shape, verts = (_dev(ev[k][idx]) for k in ('pose', 'shape', 'vertices'))
        pj24 = body.native(pose, shape, vertices=False)[1]
        e = metrics.validation_errors(verts, gt['vertices'], Jh, pj24, gt['joints_24'])
        assert e['err_sel'].shape == (len(idx), 14) and e['err_k'].shape == (len(idx), 24)
        for k, name in (('mpjpe', 'err_sel'), ('pampjpe', 'pa_err_sel'), ('mpjpe_24', 'err_k'), ('pampjpe_24', 'pa_err_k'), ('v2v', 'v2v')):
            want[k].append(e[name].cpu().numpy())
    want = {k: np.concatenate(v) for k, v in want.items()}
    for k in shapes:
        assert np.array_equal(ev[k].view(np.int32), want[k].view(np.int32)), k
        assert np.array_equal(res['step']['per_sample'][k], ev[k]), k
    assert np.array_equal(res['step']['per_sample']['v2v'].view(np.int32), want['v2v'].view(np.int32))
    acc = res['step']['acc']
    for k in shapes:
        assert acc['val_' + k] == 1000 * want[k].astype(np.float64).mean(-1).mean(), k
    assert acc['val_v2v'] == 1000 * want['v2v'].astype(np.float64).mean()
    new = [l for l in on if l not in off]
    assert new[:5] == [f'{dataset} MPJPE: ' + str(acc['val_mpjpe']), f'{dataset} PA-MPJPE: ' + str(acc['val_pampjpe']),
                       f'{dataset} MPJPE (24j): ' + str(acc['val_mpjpe_24']), f'{dataset} PA-MPJPE (24j): ' + str(acc['val_pampjpe_24']),
                       f'{dataset} V2V: ' + str(acc['val_v2v'])]
    assert json.load(open(os.path.join(log_dir, f'val_accuracy_results_{dataset}.json'))) == [[0, acc, 0]]
    assets.use_synthetic_assets(1003)
