"""The evaluation kernels of spec_amd/csrc/eval.hip against the float64 yardstick tests/metrics_ref.py, at their edges.

Shape sweeps use dyadic inputs whose fp32 sums are exact in any order (tests/test_metrics_ref_host.py checks that on the host), so an
indexing fault is an inequality of bits; the Procrustes solver gets the inputs on which such solvers fail, every one exactly
representable in fp32, so the expected value is known in advance.  Tolerances (derived in tests/metrics_ref.py and at each
assertion; the host test shows the float64 yardstick passes each with its margin):
  regress_joints, rotate_points on dyadic inputs ..... equal to float64, no tolerance
  MPJPE ............................................... 1 fp32 ulp of the float64 value (fp64 arithmetic + one final rounding)
  PA-MPJPE ............................................ max(2 fp32 ulp, 10 x |Kabsch - Horn| of that input in float64); below 1e-6 mm
                                                        where the fit is exact; NaN exactly where the reference's 0 / 0 is
  V2V on dyadic inputs ................................ (ceil(V / 256) + 14) 2^-24 relative
  regress_joints / eval_mesh joints, Gaussian inputs .. (ceil(V / 256) + 9) 2^-24 sum |w||x|
  rotate_points, random rotations ..................... 3 * 2^-24 sum |r||x|"""
import ctypes as C

import numpy as np
import pytest
import torch

from spec_amd import _lib
from tests import metrics_ref as M
from tests.util import t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0x5A5AA5A5


def _abi():
    from spec_amd.cam_utils import _engine
    eng = _engine(torch.device(DEV))
    return eng.lib, eng.h


def _p(a):
    return None if a is None else C.c_void_p(a.data_ptr())


def _dev(a):
    return t(np.ascontiguousarray(a)).to(DEV)


def _sentinels(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)


def _err(lib, h):
    return (lib.specmi_last_error(h) or b'').decode()


# ---- regress_joints ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', M.REGRESS_V)
def test_regress_joints_equals_float64_bit_for_bit(V):
    """Every V with every J (the large V with J on both sides of the chunk of 8) and B in {1, 3}: the sums are exact, so the kernel
    equals float64.  Row J - 1 of the regressor is unlike the others (an out-of-range row that got stored would show), and the
    words after the B * J * 3 outputs keep their sentinel."""
    lib, h = _abi()
    for J in M.regress_js(V):
        for B in M.BATCHES:
            verts, _, Jr = M.dyadic_mesh(V, J, B)
            ref, _ = M.regress(verts, Jr)
            n = B * J * 3
            buf = _sentinels(n + 64)
            v, w = _dev(verts), _dev(Jr)
            assert lib.specmi_regress_joints(h, _p(v), B, V, _p(w), J, _p(buf), None) == _lib.OK, _err(lib, h)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert np.all(got[n:] == SENTINEL), (V, J, B, 'wrote past the output')
            assert np.array_equal(got[:n].view(np.float32).reshape(B, J, 3).astype(np.float64), ref), (V, J, B)


# ---- eval_mesh ---------------------------------------------------------------------------------------------------------------

def _v2v_bound(V):
    # V2V is a sum of positive fp32 terms, so relative errors add: the per-lane chain of ceil(V / 256) adds, 6 shuffle steps, 3 adds of
    # the LDS fold, 2 for dx^2 + dy^2 + dz^2 (three roundings, halved by the square root, rounded up), 1 for the square root and 2 for
    # the final / V * 1000 - (ceil(V / 256) + 14) 2^-24; the differences dx, dy, dz themselves are exact on the dyadic inputs
    return (-(-V // 256) + 14) * M.U24


@pytest.mark.parametrize('V', M.MESH_V)
def test_eval_mesh_edges(V):
    """V below, at and past one block, J on both sides of the chunk of 6 and at the cap, selections of 1, 14 and 32 joints (unordered,
    repeats, joint 0).  The regressed joints are exact, so MPJPE / PA-MPJPE are held as tightly as eval_joints, and V2V to its
    summation bound."""
    from spec_amd import metrics
    for J in M.MESH_J:
        for B in M.BATCHES:
            pred, gt, Jr = M.dyadic_mesh(V, J, B)
            pv, gv, w = _dev(pred), _dev(gt), _dev(Jr)
            for sel in M.selections(J):
                mp, pk, ph, vv = M.mesh_errors(pred, gt, Jr, sel)
                g_mp, g_pa, g_vv = (x.cpu().numpy() for x in metrics.eval_single(pv, gv, w, joint_sel=sel))
                why = M.check_errors(g_mp, g_pa, mp, pk, ph)
                assert why is None, (V, J, B, len(sel), why)
                assert np.all(np.abs(g_vv.astype(np.float64) - vv) <= _v2v_bound(V) * vv), (V, J, B, g_vv, vv)


def test_eval_mesh_null_outputs_and_default_selection():
    """Any output may be NULL: the other two keep their bits.  joint_sel NULL selects the first nsel joints."""
    lib, h = _abi()
    V, J, B = 257, 13, 3
    pred, gt, Jr = M.dyadic_mesh(V, J, B)
    sel = M.selections(J)[1]
    pv, gv, w, s = _dev(pred), _dev(gt), _dev(Jr), torch.tensor(sel, dtype=torch.int32, device=DEV)
    full = _sentinels(3 * B).view(3, B)
    assert lib.specmi_eval_mesh(h, _p(pv), _p(gv), B, V, _p(w), J, _p(s), len(sel), _p(full[0]), _p(full[1]), _p(full[2]), None) == _lib.OK
    assert not bool((full == SENTINEL).any())
    for skip in range(3):
        out = _sentinels(3 * B).view(3, B)
        ptrs = [None if i == skip else _p(out[i]) for i in range(3)]
        assert lib.specmi_eval_mesh(h, _p(pv), _p(gv), B, V, _p(w), J, _p(s), len(sel), *ptrs, None) == _lib.OK, _err(lib, h)
        for i in range(3):
            assert torch.equal(out[i], full[i]) if i != skip else bool((out[i] == SENTINEL).all()), (skip, i)
    first = _sentinels(3 * B).view(3, B)
    s5 = torch.arange(5, dtype=torch.int32, device=DEV)
    assert lib.specmi_eval_mesh(h, _p(pv), _p(gv), B, V, _p(w), J, _p(s5), 5, _p(first[0]), _p(first[1]), _p(first[2]), None) == _lib.OK
    out = _sentinels(3 * B).view(3, B)
    assert lib.specmi_eval_mesh(h, _p(pv), _p(gv), B, V, _p(w), J, None, 5, _p(out[0]), _p(out[1]), _p(out[2]), None) == _lib.OK
    assert torch.equal(out, first)


def test_argument_refusals():
    """J = 33 and nsel = 33 are refused by eval_joints / eval_mesh, and so is a NULL selection that would read joints past J (rows of
    on-chip memory that were never written); regress_joints has no cap (J = 33 runs in the sweep above).  The handle stays usable."""
    lib, h = _abi()
    x = torch.zeros(3 * 40 * 64, device=DEV)
    o = _sentinels(8)
    assert lib.specmi_eval_joints(h, _p(x), _p(x), 1, 33, _p(o), _p(o), None) == _lib.ERR_ARG and '[1,32]' in _err(lib, h)
    assert lib.specmi_eval_joints(h, _p(x), _p(x), 1, 0, _p(o), _p(o), None) == _lib.ERR_ARG
    s = torch.zeros(40, dtype=torch.int32, device=DEV)
    assert lib.specmi_eval_mesh(h, _p(x), _p(x), 1, 64, _p(x), 17, _p(s), 33, _p(o), _p(o), _p(o), None) == _lib.ERR_ARG and '[1,32]' in _err(lib, h)
    assert lib.specmi_eval_mesh(h, _p(x), _p(x), 1, 64, _p(x), 33, _p(s), 14, _p(o), _p(o), _p(o), None) == _lib.ERR_ARG and '[1,32]' in _err(lib, h)
    assert lib.specmi_eval_mesh(h, _p(x), _p(x), 1, 64, _p(x), 17, None, 18, _p(o), _p(o), _p(o), None) == _lib.ERR_ARG
    assert 'nsel = 18' in _err(lib, h) and 'J = 17' in _err(lib, h)
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())
    assert lib.specmi_eval_mesh(h, _p(x), _p(x), 1, 64, _p(x), 17, None, 17, _p(o), _p(o), _p(o), None) == _lib.OK


# ---- rotate_points -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,N', [(1, 1), (3, 85), (5, 24), (257, 1), (2, 6890)])
def test_rotate_points_signed_permutations_bit_for_bit(B, N):
    """A different signed permutation per batch entry, dyadic points: one product per output, exact.  The same points in every batch
    entry, so the only thing that tells the outputs apart is which matrix was applied to which entry."""
    from spec_amd import metrics
    rng = np.random.default_rng(B * 10000 + N)
    P = M.signed_permutations()
    R = P[(np.arange(B) * 7 + 3) % 48]
    x = np.broadcast_to(M.dyadic_points(rng, (1, N, 3)), (B, N, 3)).copy()
    x[:, 0] = [0.25, -0.75, 1.5]                                      # three magnitudes, none zero: the 48 images of this point differ
    ref, _ = M.rotate(R, x)
    got = metrics.rotate_points(_dev(R), _dev(x)).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, ref)
    for b in range(1, B):
        assert not np.array_equal(ref[b], ref[b - 1])


@pytest.mark.parametrize('B,N', [(5, 24), (2, 6890)])
def test_rotate_points_random_rotations(B, N):
    from spec_amd import metrics
    rng = np.random.default_rng(B + N)
    R = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0].astype(np.float32)
    x = (rng.standard_normal((B, N, 3)) * 0.5).astype(np.float32)
    ref, mag = M.rotate(R, x)
    got = metrics.rotate_points(_dev(R), _dev(x)).cpu().numpy().astype(np.float64)
    # three products and two adds (fused or not), each term rounded at most three times: 3 * 2^-24 sum |r||x|
    assert np.all(np.abs(got - ref) <= 3 * M.U24 * mag)


# ---- Gaussian data: the summation bound --------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', [769, 6890])
def test_summation_bound_on_gaussian_meshes(V):
    """regress_joints and the joints inside eval_mesh within n 2^-24 sum |w||x| of float64.  n is the depth of the kernels' summation:
    a lane takes vertices t, t + 256, ... - at most ceil(V / 256) fused multiply-adds in a chain (regress_joints takes two per trip,
    the same chain) - then 6 wave-shuffle steps and 3 adds of the four per-wave partial sums in LDS: n = ceil(V / 256) + 9.
    eval_mesh returns no joints, so each joint j is read through a one-joint selection: MPJPE = 1000 |(jp[j] - jp[0]) - (jg[j] - jg[0])|."""
    from spec_amd import metrics
    rng = np.random.default_rng(V)
    B, n = 2, -(-V // 256) + 9
    gt = (rng.standard_normal((B, V, 3)) * 0.3).astype(np.float32)
    pred = (gt + rng.standard_normal((B, V, 3)) * 0.03 + rng.standard_normal((B, 1, 3)) * 0.2).astype(np.float32)
    for J in (24, 17):
        Jr = (rng.random((J, V)) * (rng.random((J, V)) < 0.3)).astype(np.float32)
        Jr /= Jr.sum(1, keepdims=True)
        ref_p, mag_p = M.regress(pred, Jr)
        ref_g, mag_g = M.regress(gt, Jr)
        got = metrics.regress_joints(_dev(pred), _dev(Jr)).cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - ref_p) <= n * M.U24 * mag_p), (V, J, (np.abs(got - ref_p) / mag_p).max() / M.U24)
        if J != 17:
            continue
        pv, gv, w = _dev(pred), _dev(gt), _dev(Jr)
        for j in range(1, J):
            dp, dg = ref_p[:, j] - ref_p[:, 0], ref_g[:, j] - ref_g[:, 0]
            ref = np.sqrt(((dp - dg) ** 2).sum(-1)) * 1000
            # per coordinate: the four regressed joints to the summation bound, the two fp32 pelvis subtractions to half an ulp each
            e = n * M.U24 * (mag_p[:, j] + mag_p[:, 0] + mag_g[:, j] + mag_g[:, 0])
            e = e + M.U24 * (np.abs(dp) + np.abs(dg) + e)
            tol = 1000 * np.sqrt((e ** 2).sum(-1)) + M.ulp32(ref)        # | |a| - |b| | <= |a - b|, and the final rounding
            got_mp = metrics.eval_single(pv, gv, w, joint_sel=[j])[0].cpu().numpy().astype(np.float64)
            assert np.all(np.abs(got_mp - ref) <= tol), (V, j, got_mp, ref, tol)


# ---- Procrustes on the inputs that break solvers -------------------------------------------------------------------------------

_CASES = M.procrustes_cases()


@pytest.mark.parametrize('family', sorted(_CASES))
def test_procrustes_families(family):
    """See ``metrics_ref.procrustes_cases``.  Exact fits (identity, exact similarity transforms with every proper signed permutation -
    the rotations by pi among them -, a mirrored coplanar set, two joints) stay below 1e-6 mm; an exact mirror image of a non-planar
    body equals the Kabsch value with the reflection fix; zero variance is NaN with a finite MPJPE."""
    from spec_amd import metrics
    pred, gt, expect = _CASES[family]
    mp, pk, ph = M.joint_errors(pred, gt)
    g_mp, g_pa = (x.cpu().numpy() for x in metrics.eval_j_24(_dev(pred), _dev(gt)))
    if family == 'identity':
        assert np.all(g_mp == 0.0)
    if expect == 'range':
        n = pred.shape[1]
        lam = M.horn_eigenvalues(pred[0] - pred[0, :1], gt[0] - gt[0, :1])[-1]
        x1, x2 = pred[0].astype(np.float64) - pred[0].mean(0), gt[0].astype(np.float64) - gt[0].mean(0)
        rms = np.sqrt(((x2 ** 2).sum() - lam ** 2 / (x1 ** 2).sum()) / n) * 1000      # the unique squared optimum: var2 - lam^2 / var1
        assert np.all(np.abs(g_mp - mp) <= M.ulp32(mp))
        assert rms / np.sqrt(n) * (1 - 1e-6) <= float(g_pa[0]) <= rms * (1 + 1e-6), (g_pa, rms)
        return
    why = M.check_errors(g_mp, g_pa, mp, pk, ph)
    assert why is None, (family, why)
    if expect == 'zero':
        assert np.all(g_pa < M.EXACT_FIT_MM), (family, g_pa)
    elif expect == 'nan':
        assert np.all(np.isnan(g_pa)) and np.all(np.isfinite(g_mp))
    else:
        assert np.all(np.isfinite(g_pa)) and np.all(pk >= M.EXACT_FIT_MM)      # so check_errors held it to pa_tolerance


@pytest.mark.parametrize('J', [1, 2, 3, 5, 17, 24, 31, 32])
def test_random_batches_half_mirrored(J):
    """Well-conditioned similarity transforms plus noise, the odd poses mirrored, B on both sides of the 64 poses of a workgroup."""
    from spec_amd import metrics
    for B in (1, 63, 64, 65, 130):
        pred, gt = M.random_batch(B, J, 1)
        if J >= 5 and B >= 2:
            signs = {M.kabsch_det_sign(a - a[:1], b - b[:1]) for a, b in zip(pred, gt)}
            assert signs == {1.0, -1.0}, (B, J, signs)
        mp, pk, ph = M.joint_errors(pred, gt)
        g_mp, g_pa = (x.cpu().numpy() for x in metrics.eval_j_24(_dev(pred), _dev(gt)))
        why = M.check_errors(g_mp, g_pa, mp, pk, ph)
        assert why is None, (B, J, why)


def test_batch_invariance_and_nan_isolation():
    """A pose's result does not depend on where in the batch it sits (first, last lane of a workgroup, first lane of the next, alone),
    and a zero-variance neighbour's NaN stays in its own lane."""
    from spec_amd import metrics
    pred, gt = M.random_batch(130, 14, 2)
    pose_p, pose_g = M.random_batch(1, 14, 3)
    for i in (0, 63, 64):
        pred[i], gt[i] = pose_p[0], pose_g[0]
    alone = [x.clone() for x in metrics.eval_j_24(_dev(pose_p), _dev(pose_g))]
    clean = [x.clone() for x in metrics.eval_j_24(_dev(pred), _dev(gt))]
    for i in (0, 63, 64):
        assert torch.equal(clean[0][i:i + 1], alone[0]) and torch.equal(clean[1][i:i + 1], alone[1]), i
    bad = (1, 62, 65, 129)
    for i in bad:
        pred[i] = pred[i, :1]                           # all joints coincident
    mp, pk, ph = M.joint_errors(pred, gt)
    got = [x.clone() for x in metrics.eval_j_24(_dev(pred), _dev(gt))]
    assert M.check_errors(got[0].cpu().numpy(), got[1].cpu().numpy(), mp, pk, ph) is None
    keep = torch.ones(130, dtype=torch.bool)
    keep[list(bad)] = False
    assert bool(torch.isnan(got[1][~keep.to(DEV)]).all()) and bool(torch.isfinite(got[0]).all())
    assert torch.equal(got[0][keep.to(DEV)], clean[0][keep.to(DEV)]) and torch.equal(got[1][keep.to(DEV)], clean[1][keep.to(DEV)])
