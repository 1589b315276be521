"""NumPy float64 restatement of the four operations of spec_amd/csrc/eval.hip (spec/utils/compute_error.py:33-86,164-189): the
yardstick of tests/test_gpu_metrics_edges.py, checked on the host by tests/test_metrics_ref_host.py.

``regress`` / ``rotate`` work in float64 from the fp32 inputs and also return Sum |w||x| per output, the quantity every
summation bound multiplies.  ``joint_errors`` subtracts the pelvis IN FLOAT32, as the reference's ``eval_j_24`` and the kernels do,
and computes everything after it in ``dtype`` (float64: the yardstick; float32: the reference's own data flow, for the parity test
against tests/golden/metrics.npz).  PA-MPJPE comes by two independent routes - Kabsch / SVD with the det-sign fix of
``oracle.metrics.compute_similarity_transform``, and Horn's 4x4 quaternion matrix through ``numpy.linalg.eigh``.  Where the two
float64 answers differ the input is ill-conditioned, and their difference is that input's noise floor.

The second half builds the inputs the GPU tests and the host test share: dyadic meshes and regressors whose fp32 sums are exact
in any order, signed permutation matrices, and the Procrustes case families (``procrustes_cases``)."""
import itertools

import numpy as np

U24 = 2.0 ** -24                                   # fp32 unit roundoff
H36M_TO_J14 = (6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10)


# ---- the four operations ----------------------------------------------------------------------------------------------------

def regress(verts, Jr):
    """joints[b,j,c] = sum_v Jr[j,v] verts[b,v,c] in float64 -> (joints, mag), mag = sum_v |Jr[j,v]| |verts[b,v,c]|."""
    v, w = np.asarray(verts, np.float64), np.asarray(Jr, np.float64)
    return np.einsum('jv,bvc->bjc', w, v), np.einsum('jv,bvc->bjc', np.abs(w), np.abs(v))


def rotate(R, x):
    """out[b,n,:] = R[b] x[b,n,:] in float64 -> (out, mag), mag[b,n,c] = sum_k |R[b,c,k]| |x[b,n,k]|."""
    R, x = np.asarray(R, np.float64), np.asarray(x, np.float64)
    return np.einsum('bck,bnk->bnc', R, x), np.einsum('bck,bnk->bnc', np.abs(R), np.abs(x))


def _centre(p, g):
    mu1, mu2 = p.mean(0, keepdims=True), g.mean(0, keepdims=True)
    return p - mu1, g - mu2, mu1, mu2


def kabsch_det_sign(p, g):
    """Sign of det(U V^T) of the cross-covariance's SVD: -1 where the unconstrained optimum is a reflection."""
    x1, x2, _, _ = _centre(np.asarray(p, np.float64), np.asarray(g, np.float64))
    U, _, Vh = np.linalg.svd(x1.T @ x2)
    return float(np.sign(np.linalg.det(U @ Vh)))


def pa_kabsch(p, g):
    """Mean distance (input units) after the least-squares similarity transform of p (N,3) onto g: SVD of K = X1^T X2 with the last
    singular direction flipped when det(U V^T) < 0.  Zero variance of p divides 0 by 0 and returns NaN, like the reference."""
    x1, x2, mu1, mu2 = _centre(p, g)
    var1 = (x1 ** 2).sum()
    K = x1.T @ x2
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3, dtype=p.dtype)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = np.trace(R @ K) / var1
        hat = scale * (x1 @ R.T) + mu2
        return np.sqrt(((hat - g) ** 2).sum(-1)).mean()


def horn_matrix(S):
    """Horn's symmetric 4x4 of the cross-covariance S = sum x1 x2^T: its largest eigenvector is the optimal unit quaternion."""
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = S
    return np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                     [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                     [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
                     [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz]], dtype=S.dtype)


def horn_eigenvalues(p, g):
    """Ascending eigenvalues of Horn's matrix of the centred p, g (float64)."""
    x1, x2, _, _ = _centre(np.asarray(p, np.float64), np.asarray(g, np.float64))
    return np.linalg.eigvalsh(horn_matrix(x1.T @ x2))


def pa_horn(p, g):
    """The same optimum by Horn's closed form: rotation from the largest eigenpair of ``horn_matrix``, scale = eigenvalue / var1."""
    x1, x2, mu1, mu2 = _centre(p, g)
    var1 = (x1 ** 2).sum()
    lam, vec = np.linalg.eigh(horn_matrix(x1.T @ x2))
    w, x, y, z = vec[:, -1]
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=p.dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = lam[-1] / var1
        hat = scale * (x1 @ R.T) + mu2
        return np.sqrt(((hat - g) ** 2).sum(-1)).mean()


def aligned_errors(p, g, dtype=np.float64):
    """(mpjpe, pa_kabsch, pa_horn) in millimetres of pelvis-aligned fp32 joint sets p, g (B,N,3), evaluated in ``dtype``."""
    p, g = np.asarray(p, np.float32).astype(dtype), np.asarray(g, np.float32).astype(dtype)
    mp = np.sqrt(((p - g) ** 2).sum(-1)).mean(-1) * 1000
    pk = np.array([pa_kabsch(a, b) for a, b in zip(p, g)], dtype) * 1000
    ph = np.array([pa_horn(a, b) for a, b in zip(p, g)], dtype) * 1000
    return mp, pk, ph


def joint_errors(pred, gt, dtype=np.float64):
    """eval_j_24: pelvis (joint 0) subtracted in float32, then MPJPE and the two PA-MPJPE routes in ``dtype`` -> three (B,) arrays, mm."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    return aligned_errors(pred - pred[:, :1], gt - gt[:, :1], dtype)


def mesh_errors(pred_v, gt_v, Jr, sel=H36M_TO_J14, dtype=np.float64):
    """eval_single: joints regressed in ``dtype`` and rounded to float32 (what the kernel holds; exact for the dyadic inputs), pelvis
    subtracted in float32, joints ``sel`` selected -> (mpjpe, pa_kabsch, pa_horn, v2v) in mm; V2V in ``dtype`` from the fp32 meshes
    and the fp32 pelvis."""
    pv, gv, w = (np.asarray(a, np.float32) for a in (pred_v, gt_v, Jr))
    if dtype == np.float64:
        jp, jg = regress(pv, w)[0].astype(np.float32), regress(gv, w)[0].astype(np.float32)
    else:
        jp, jg = np.einsum('jv,bvc->bjc', w, pv), np.einsum('jv,bvc->bjc', w, gv)
    sel = list(sel)
    mp, pk, ph = aligned_errors(jp[:, sel] - jp[:, :1], jg[:, sel] - jg[:, :1], dtype)
    d = (gv.astype(dtype) - jg[:, :1].astype(dtype)) - (pv.astype(dtype) - jp[:, :1].astype(dtype))
    return mp, pk, ph, np.sqrt((d ** 2).sum(-1)).mean(-1) * 1000


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


EXACT_FIT_MM = 1e-6      # PA-MPJPE of an exact fit: fp64 epsilon x metre-scale coordinates x 1000 is about 1e-10 mm; an fp32 solver gives 1e-4


def pa_tolerance(pk, ph):
    """Bound on |kernel - pa_kabsch| for a PA-MPJPE: 2 fp32 ulp (final rounding + fp64 arithmetic), or 10 x the disagreement of the
    two float64 routes where the input is ill-conditioned enough for that to be larger."""
    return np.maximum(2 * ulp32(pk), 10 * np.abs(np.asarray(pk) - np.asarray(ph)))


def check_errors(got_mp, got_pa, mp, pk, ph):
    """The contract of one (B,) result against the float64 yardstick; returns a message, or None when it holds.
      * MPJPE within 1 fp32 ulp of the float64 value (fp64 arithmetic + the single final rounding);
      * PA-MPJPE NaN exactly where the yardstick is NaN (zero variance of the prediction);
      * where the float64 PA-MPJPE is an exact fit (below EXACT_FIT_MM / 100: an ulp of nothing is no tolerance) the kernel's is
        below EXACT_FIT_MM;
      * elsewhere within ``pa_tolerance``."""
    got_mp, got_pa = np.asarray(got_mp, np.float64), np.asarray(got_pa, np.float64)
    if not np.all(np.isfinite(got_mp)) or np.any(np.abs(got_mp - mp) > ulp32(mp)):
        return 'MPJPE %r vs float64 %r' % (got_mp, mp)
    nan = np.isnan(pk)
    if not np.array_equal(np.isnan(got_pa), nan) or not np.array_equal(np.isnan(ph), nan):
        return 'PA-MPJPE NaN pattern %r vs float64 %r' % (got_pa, pk)
    fit = ~nan & (pk < EXACT_FIT_MM / 100)
    if np.any(got_pa[fit] >= EXACT_FIT_MM):
        return 'PA-MPJPE of an exact fit %r' % (got_pa[fit],)
    rest = ~nan & ~fit
    bad = np.abs(got_pa[rest] - pk[rest]) > pa_tolerance(pk[rest], ph[rest])
    if np.any(bad):
        return 'PA-MPJPE %r vs float64 %r (tolerance %r)' % (got_pa[rest][bad], pk[rest][bad], pa_tolerance(pk[rest], ph[rest])[bad])
    return None


# ---- inputs whose fp32 sums are exact -----------------------------------------------------------------------------------------

def dyadic_points(rng, shape):
    """Multiples of 1/64 in [-2, 2] (float32)."""
    return (rng.integers(-128, 129, size=shape) / 64.0).astype(np.float32)


def dyadic_regressor(rng, J, V, density=0.5):
    """(J,V) float32, weights multiples of 1/8 in [0, 1], about half of them zero.  Columns 0 and V - 1 are non-zero in every row
    (a dropped first or last vertex moves every joint), and row J - 1 is all ones, unlike any other row (the kernels' out-of-range
    rows alias row J - 1: a stored alias shows)."""
    w = rng.integers(1, 8, size=(J, V)) * (rng.random((J, V)) < density)
    w[:, 0] = rng.integers(1, 8, size=J)
    w[:, V - 1] = rng.integers(1, 8, size=J)
    w[J - 1] = 8
    return (w / 8.0).astype(np.float32)


def assert_exact_sums(verts, Jr):
    """The precondition of the bit-for-bit tests: every partial sum of w * x fits fp32's 24 bits.  Products are multiples of 2^-9, so
    it is enough that 2^9 sum |w||x| < 2^24; checked also in the flesh - fp32 sums in two orders equal the float64 sum."""
    ref, mag = regress(verts, Jr)
    assert np.all(np.asarray(verts, np.float64) * 64 % 1 == 0) and np.all(np.asarray(Jr, np.float64) * 8 % 1 == 0)
    assert mag.max() * 512 < 2 ** 24, mag.max()
    v, w = np.asarray(verts, np.float32), np.asarray(Jr, np.float32)
    fwd = np.zeros(ref.shape, np.float32)
    for i in range(v.shape[1]):                                       # sequential, first to last
        fwd += w[None, :, i, None] * v[:, None, i, :]
    pair = w[None, :, :, None] * v[:, None, :, :]                      # pairwise tree, last to first
    pair = pair[:, :, ::-1]
    while pair.shape[2] > 1:
        if pair.shape[2] % 2:
            pair = np.concatenate([pair, np.zeros_like(pair[:, :, :1])], 2)
        pair = pair[:, :, 0::2] + pair[:, :, 1::2]
    assert fwd.dtype == np.float32 and pair.dtype == np.float32
    assert np.array_equal(fwd.astype(np.float64), ref) and np.array_equal(pair[:, :, 0].astype(np.float64), ref)
    return ref


def signed_permutations(det=None):
    """The 48 signed 3x3 permutation matrices (float32), or the 24 of one determinant."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            P = np.zeros((3, 3), np.float32)
            for r in range(3):
                P[r, perm[r]] = signs[r]
            if det is None or round(float(np.linalg.det(P))) == det:
                out.append(P)
    return np.stack(out)


ROT_PI_Z = np.diag([-1.0, -1.0, 1.0]).astype(np.float32)          # rotation by pi about z: quaternion (0, 0, 0, 1), scalar part 0


# ---- Procrustes case families -------------------------------------------------------------------------------------------------

def _body(rng, J):
    """A non-planar dyadic joint set (J,3), joint 0 off the origin."""
    while True:
        g = dyadic_points(rng, (J, 3))
        if J < 4 or np.linalg.matrix_rank(g - g.mean(0)) == 3:
            return g


def procrustes_cases(seed=20261018):
    """{family: (pred, gt, expect)} with pred, gt float32 (B,J,3), every value exactly representable.  ``expect`` is 'zero' (PA-MPJPE
    below 1e-6 mm), 'value' (equals the Kabsch value within ``pa_tolerance``), 'nan' (zero variance: NaN, MPJPE finite) or 'range'
    (no unique value: between rms / sqrt(N) and rms of the unique squared optimum)."""
    rng = np.random.default_rng(seed)
    cases = {}
    g = np.stack([_body(rng, 24) for _ in range(6)])
    cases['identity'] = (g.copy(), g, 'zero')
    # exact similarity transforms 2^k P g + t, P over all 24 proper signed permutations (ROT_PI_Z and the other rotations by pi
    # among them: zero scalar part of the quaternion), k in {-3, 0, 2}
    P = signed_permutations(det=1)
    assert any(np.array_equal(p, ROT_PI_Z) for p in P)
    gs = np.stack([_body(rng, 17) for _ in range(len(P) * 3)])
    ks = np.repeat(np.array([-3, 0, 2]), len(P))
    Ps = np.tile(P, (3, 1, 1))
    t = dyadic_points(rng, (len(gs), 1, 3)) * 4
    cases['similarity'] = ((np.einsum('bck,bnk->bnc', Ps, gs) * (2.0 ** ks)[:, None, None] + t).astype(np.float32), gs, 'zero')
    g = np.stack([_body(rng, 14) for _ in range(5)])
    cases['mirror'] = (g * np.array([-1, 1, 1], np.float32), g, 'value')
    # coplanar joints (z = 0 after the pelvis, which is joint 0): noisy in the plane; and their exact mirror image, which a rotation
    # by pi about an in-plane axis realises
    g = np.stack([_body(rng, 12) for _ in range(5)])
    g[:, :, 2] = 0.5
    cases['coplanar'] = ((g + dyadic_points(rng, g.shape) / 16 * np.array([1, 1, 0], np.float32)).astype(np.float32), g, 'value')
    cases['coplanar_mirror'] = (g * np.array([-1, 1, 1], np.float32), g, 'zero')
    # collinear joints along a dyadic direction, noisy along the line
    s = dyadic_points(rng, (5, 10, 1))
    d = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, -2, 1], [0.5, 0.25, -1]], np.float32)[:, None, :]
    g = s * d
    cases['collinear'] = (((s + dyadic_points(rng, s.shape) / 16) * d * 2 + 1).astype(np.float32), g, 'value')
    g = np.stack([_body(rng, 2) for _ in range(8)])                     # two points always fit exactly
    cases['two_joints'] = ((g + dyadic_points(rng, g.shape) / 8).astype(np.float32), g, 'zero')
    # repeated largest eigenvalue of Horn's matrix: a collinear prediction against a non-collinear target.  The cross-covariance has
    # rank 1, the eigenvalues are +-|S| twice each, and the free rotation is the one about the prediction's own line - it moves no
    # point, so the error is unique.  (A repeated eigenvalue whose free rotation moves the points, e.g. pred = -gt of an
    # octahedron, has a unique SQUARED error but no unique mean distance: 'inversion' below pins only its range.)
    g = np.stack([_body(rng, 9) for _ in range(5)])
    cases['repeated_eigenvalue'] = ((s[:, :9] * d + 0.25).astype(np.float32), g, 'value')
    octa = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    octa = np.concatenate([np.zeros((1, 3), np.float32), octa])[None]       # pelvis at the centre
    cases['inversion'] = (-octa, octa, 'range')
    # scales and offsets
    g = np.stack([_body(rng, 24) for _ in range(6)])
    p = (g + dyadic_points(rng, g.shape) / 32).astype(np.float32)
    cases['scale_1e-3'] = ((p * np.float32(1e-3)), (g * np.float32(1e-3)), 'value')
    cases['scale_1e3'] = ((p * np.float32(1e3)), (g * np.float32(1e3)), 'value')
    off = np.array([100, -50, 30], np.float32)
    g = (rng.standard_normal((6, 24, 3)) * 0.3).astype(np.float32) + off
    cases['far_pelvis'] = ((g + (rng.standard_normal(g.shape) * 2e-3).astype(np.float32)).astype(np.float32), g, 'value')
    # zero variance of the prediction: one joint; all predicted joints coincident
    g = np.stack([_body(rng, 1) for _ in range(3)])
    cases['one_joint'] = ((g + 0.5).astype(np.float32), g, 'nan')
    g = np.stack([_body(rng, 14) for _ in range(3)])
    cases['coincident'] = (np.broadcast_to(np.array([0.5, -1, 2], np.float32), g.shape).copy(), g, 'nan')
    return cases


def random_batch(B, J, seed):
    """A well-conditioned batch, the odd poses mirrored: pred = s R gt + noise + t with R a random rotation (even b) or a random
    rotation times a reflection (odd b).  Returns float32 (pred, gt)."""
    rng = np.random.default_rng(seed * 1000 + B * 37 + J)
    gt = rng.standard_normal((B, J, 3)) * 0.4
    Q = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]                 # det +1
    Q[1::2] = Q[1::2] @ np.diag([1.0, 1.0, -1.0])                    # det -1 for odd b
    pred = np.einsum('bck,bnk->bnc', Q, gt) * (0.8 + 0.4 * rng.random((B, 1, 1))) \
        + 0.03 * rng.standard_normal((B, J, 3)) + rng.standard_normal((B, 1, 3))
    return pred.astype(np.float32), gt.astype(np.float32)


# ---- the shape sweeps of tests/test_gpu_metrics_edges.py (shared with the host test of their precondition) -------------------

REGRESS_V = (1, 2, 255, 256, 257, 511, 512, 513, 767, 769, 1025, 6890)   # 769 % 512 = 257: the mixed last trip of regress_joints
REGRESS_J = (1, 7, 8, 9, 16, 17, 24, 33)                                 # both sides of the chunk kRC = 8; 33: no cap on J
MESH_V = (1, 2, 255, 256, 257, 1200)
MESH_J = (1, 5, 6, 7, 12, 13, 17, 32)                                    # both sides of the chunk kJC = 6; 32: the cap
BATCHES = (1, 3)


def regress_js(V):
    """The J swept at a V: all of them, except at the one large V, which keeps a J on each side of a multiple of 8, 24 and 33."""
    return REGRESS_J if V < 6890 else (7, 9, 24, 33)


def dyadic_mesh(V, J, B, seed=7):
    """(pred, gt, Jr) float32: gt dyadic, pred = gt + dyadic noise of 1/8 the size (still multiples of 1/64 within [-2, 2])."""
    rng = np.random.default_rng((seed, V, J, B))
    gt = (rng.integers(-96, 97, size=(B, V, 3)) / 64.0).astype(np.float32)
    pred = (gt + rng.integers(-32, 33, size=(B, V, 3)) / 64.0).astype(np.float32)
    return pred, gt, dyadic_regressor(rng, J, V)


def selections(J, seed=11):
    """Joint selections of length 1, 14 and 32 for a J-row regressor: unordered, with repeats, joint 0 among the longer ones.  The
    single joint is the last one (joint 0 alone is the pelvis: all zeros)."""
    rng = np.random.default_rng((seed, J))
    out = [[J - 1]]
    for n in (14, 32):
        s = rng.integers(0, J, size=n)
        s[rng.integers(0, n)] = 0
        s[0] = J - 1
        out.append([int(x) for x in s])
    return out
