"""NumPy float64 restatement of ``specmi_eval_step`` (spec_amd/csrc/eval.hip; spec/trainer.py:272-344): the yardstick of
tests/test_gpu_eval_step.py, checked on the host by tests/test_eval_step_host.py.  Built on tests/metrics_ref.py.

Everything is PER JOINT and in METRES, the unit of the per-joint arrays in ``evaluation_results_<ds>.pkl``.  The pelvis (joint 0)
is subtracted IN FLOAT32, as the reference and the kernel do; everything after it is evaluated in ``dtype`` (float64: the
yardstick; float32: the reference's own data flow, for the parity test against ``oracle.metrics``).  The Procrustes-aligned error
comes by the two independent routes of metrics_ref - Kabsch / SVD with the det-sign fix, and Horn's quaternion matrix through
``numpy.linalg.eigh``; where the two float64 answers differ, their difference is that joint's noise floor.

The second half holds the rule a kernel result is held to (``check_per_joint``, the per-joint form of
``metrics_ref.check_errors``), the bound on the unaligned V2V, and the inputs the GPU tests and the host test share."""
import functools

import numpy as np

from tests import metrics_ref as M

EXACT_FIT_M = M.EXACT_FIT_MM / 1000          # 1e-9 m: what the kernel's pa_err of an exact fit stays below
EXACT_FIT_REF_M = EXACT_FIT_M / 100          # 1e-11 m: below it the float64 value counts as an exact fit


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def hat_kabsch(p, g):
    """s R (p - mean p) + mean g by the SVD route of ``oracle.metrics.compute_similarity_transform`` -> (N,3).  Zero variance of p
    divides 0 by 0: every entry NaN, like the reference."""
    x1, x2, mu1, mu2 = M._centre(p, g)
    var1 = (x1 ** 2).sum()
    K = x1.T @ x2
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3, dtype=p.dtype)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.trace(R @ K) / var1 * (x1 @ R.T) + mu2


def hat_horn(p, g):
    """The same optimum by Horn's closed form (largest eigenpair of ``metrics_ref.horn_matrix``, scale = eigenvalue / var1)."""
    x1, x2, mu1, mu2 = M._centre(p, g)
    var1 = (x1 ** 2).sum()
    lam, vec = np.linalg.eigh(M.horn_matrix(x1.T @ x2))
    w, x, y, z = vec[:, -1]
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=p.dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        return lam[-1] / var1 * (x1 @ R.T) + mu2


def aligned_per_joint(p, g, dtype=np.float64):
    """(err, pa_kabsch, pa_horn), each (B,N), of pelvis-aligned fp32 joint sets p, g (B,N,3), evaluated in ``dtype``."""
    p, g = np.asarray(p, np.float32).astype(dtype), np.asarray(g, np.float32).astype(dtype)
    dist = lambda a, b: np.sqrt(((a - b) ** 2).sum(-1))
    pk = np.stack([dist(hat_kabsch(a, b), b) for a, b in zip(p, g)])
    ph = np.stack([dist(hat_horn(a, b), b) for a, b in zip(p, g)])
    return dist(p, g), pk, ph


def given_per_joint(pred, gt, dtype=np.float64):
    """The given-joints half (spec/trainer.py:282-283,297-302): joint 0 subtracted from each set in float32."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    return aligned_per_joint(pred - pred[:, :1], gt - gt[:, :1], dtype)


def regressed_aligned(pred_v, gt_v, Jr, sel, dtype=np.float64):
    """The selected regressed joints of both meshes, pelvis subtracted in float32 -> (p, g) float32 (B,nsel,3).  float64: the
    regression in float64 rounded to float32 (what the kernel holds; exact for the dyadic inputs)."""
    pv, gv, w = (np.asarray(a, np.float32) for a in (pred_v, gt_v, Jr))
    if dtype == np.float64:
        jp, jg = M.regress(pv, w)[0].astype(np.float32), M.regress(gv, w)[0].astype(np.float32)
    else:
        jp, jg = np.einsum('jv,bvc->bjc', w, pv), np.einsum('jv,bvc->bjc', w, gv)
    sel = list(sel)
    return jp[:, sel] - jp[:, :1], jg[:, sel] - jg[:, :1]


def mesh_per_joint(pred_v, gt_v, Jr, sel=M.H36M_TO_J14, dtype=np.float64):
    """The regressed half (spec/trainer.py:277-295; the ground truth is the dataset's pose_3d, cam_dataset.py:443-447)."""
    return aligned_per_joint(*regressed_aligned(pred_v, gt_v, Jr, sel, dtype), dtype)


def raw_v2v(pred_v, gt_v, dtype=np.float64):
    """``compute_error_verts`` (spec/trainer.py:312-315): mean_v |gt_v - pred_v| on the meshes as given -> (B,)."""
    d = np.asarray(gt_v, np.float32).astype(dtype) - np.asarray(pred_v, np.float32).astype(dtype)
    return np.sqrt((d ** 2).sum(-1)).mean(-1)


# ---- the rule ----------------------------------------------------------------------------------------------------------------

def pa_tolerance(pk, ph):
    """Bound on |kernel - pa_kabsch| of one joint: 2 fp32 ulp (the final rounding + fp64 arithmetic), or 10 x the disagreement of the
    two float64 routes where the input is ill-conditioned enough for that to be larger."""
    return np.maximum(2 * M.ulp32(pk), 10 * np.abs(np.asarray(pk) - np.asarray(ph)))


def check_per_joint(got_err, got_pa, err, pk, ph):
    """The rule of ``metrics_ref.check_errors`` per joint, in metres; returns a message, or None when it holds.
      * err within 1 fp32 ulp of the float64 value;
      * pa_err NaN exactly where the yardstick is NaN (zero variance: the whole set);
      * where the float64 pa_err is an exact fit (below EXACT_FIT_REF_M = 1e-11 m) the kernel's is below EXACT_FIT_M = 1e-9 m;
      * elsewhere within ``pa_tolerance`` of that joint."""
    got_err, got_pa = np.asarray(got_err, np.float64), np.asarray(got_pa, np.float64)
    if got_err.shape != err.shape or got_pa.shape != pk.shape:
        return 'shapes %r %r vs %r' % (got_err.shape, got_pa.shape, err.shape)
    if not np.all(np.isfinite(got_err)) or np.any(np.abs(got_err - err) > M.ulp32(err)):
        return 'err %r vs float64 %r' % (got_err, err)
    nan = np.isnan(pk)
    if not np.array_equal(np.isnan(got_pa), nan) or not np.array_equal(np.isnan(ph), nan):
        return 'pa_err NaN pattern %r vs float64 %r' % (got_pa, pk)
    fit = ~nan & (pk < EXACT_FIT_REF_M)
    if np.any(got_pa[fit] >= EXACT_FIT_M):
        return 'pa_err of an exact fit %r' % (got_pa[fit],)
    rest = ~nan & ~fit
    tol = pa_tolerance(pk[rest], ph[rest])
    bad = np.abs(got_pa[rest] - pk[rest]) > tol
    if np.any(bad):
        return 'pa_err %r vs float64 %r (tolerance %r)' % (got_pa[rest][bad], pk[rest][bad], tol[bad])
    return None


def v2v_bound(V):
    """Relative bound on the kernel's unaligned V2V on dyadic meshes.  It is a sum of positive fp32 terms, so relative errors add:
    the per-lane chain of ceil(V / 256) adds, 6 wave-shuffle steps, 3 adds of the LDS fold, 2 for dx^2 + dy^2 + dz^2 (three
    roundings, halved by the square root, rounded up), 1 for the square root and 1 for the final / V - (ceil(V / 256) + 13) 2^-24.
    The differences dx, dy, dz are exact on the dyadic inputs.  (``_v2v_bound`` of tests/test_gpu_metrics_edges.py has one
    rounding more, for its x 1000.)"""
    return (-(-V // 256) + 13) * M.U24


def mean_consistency_bound(mean_mm, err):
    """Bound on |1000 mean_i(err[b,i]) - mean_mm[b]|, ``err`` (B,N) the kernel's fp32 per-joint errors in metres and ``mean_mm``
    (B,) the fp32 per-image mean in millimetres of specmi_eval_mesh / specmi_eval_joints.  Both round the same float64 quantities:
    the mean once (half an ulp of it), each joint once (half an ulp of each, averaged and scaled)."""
    return 0.5 * M.ulp32(mean_mm) + 1000 * (0.5 * M.ulp32(err)).mean(-1)


# ---- the inputs --------------------------------------------------------------------------------------------------------------

STEP_V = (1, 257, 1200)                 # one vertex; one lane's second trip; several trips with a ragged tail
STEP_J = (1, 6, 7, 17, 32)              # one joint; both sides of the chunk kJC = 6; the H36M regressor's 17; the cap
STEP_JK = (1, 24, 32)                   # zero variance; the SMPL joints; the cap
BATCHES = M.BATCHES


@functools.lru_cache(maxsize=None)
def mesh(V, J, B):
    """``metrics_ref.dyadic_mesh(V, J, B)``, made once per process and shared (read only)."""
    out = M.dyadic_mesh(V, J, B)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dyadic_joints(B, Jk, seed=5):
    """Given joint sets (pred, gt) float32 (B,Jk,3), multiples of 1/64, joint 0 of both off the origin (the kernel subtracts both)."""
    rng = np.random.default_rng((seed, B, Jk))
    gt = M.dyadic_points(rng, (B, Jk, 3))
    pred = (gt + rng.integers(-32, 33, size=gt.shape) / 64.0).astype(np.float32)
    gt[:, 0], pred[:, 0] = [0.25, -0.5, 1.0], [-0.75, 0.5, 0.125]
    pred.setflags(write=False), gt.setflags(write=False)
    return pred, gt


def sweep():
    """Every (V, J, B, selection, Jk) of the exact-regression test."""
    for V in STEP_V:
        for J in STEP_J:
            for B in BATCHES:
                for sel in M.selections(J):
                    for Jk in STEP_JK:
                        yield V, J, B, sel, Jk


def random_bodies(B, V, seed):
    """Gaussian meshes with a regressor whose rows sum to one, and 24 given joints: well-conditioned inputs for the float32 parity
    with the reference's functions."""
    rng = np.random.default_rng((seed, B, V))
    gt = (rng.standard_normal((B, V, 3)) * 0.3).astype(np.float32)
    pred = (gt + rng.standard_normal((B, V, 3)) * 0.03 + rng.standard_normal((B, 1, 3)) * 0.2).astype(np.float32)
    Jr = (rng.random((17, V)) * (rng.random((17, V)) < 0.3) + 1e-3).astype(np.float32)
    Jr /= Jr.sum(1, keepdims=True)
    gj = (rng.standard_normal((B, 24, 3)) * 0.3).astype(np.float32)
    pj = (gj + rng.standard_normal((B, 24, 3)) * 0.03 + rng.standard_normal((B, 1, 3)) * 0.2).astype(np.float32)
    return pred, gt, Jr, pj, gj
