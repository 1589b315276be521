"""NumPy float64 restatement of everything between the trunk's feature map and the SMPL mesh - spec_amd/csrc/head.hip plus
head_init_row / rot6d_joint of specmi_internal.h: the yardstick of tests/test_gpu_head_edges.py, pinned to the torch code under
oracle/ by tests/test_head_ref_host.py.  No torch in here.

Every operation follows the reference's definition at the call site head.hip cites: ``linear`` / ``ief`` (pare HMRHead,
spec/models/hmr.py:94-98), ``rot6d_to_rotmat`` (Gram-Schmidt with F.normalize's ``x / max(|x|, eps)``; eps is 1e-12 rounded to
fp32, the value the fp32 tensor meets in torch), ``uncertainty_act`` (torch.nn.functional defaults), ``head_state_row`` (the IEF
state columns), ``decode`` / ``soft_to_angle`` (camcalib/cam_utils.py:110-133: the range ends are python doubles, their span is
rounded to fp32 when it meets the tensor), ``focal`` (scripts/camcalib_demo.py:129), ``cam_RK`` (spec/utils/cam_params.py:37-46,
the quaternion route, K[2,2] = 0), ``bins_argmax`` (np.argmax: first maximum, a NaN counts as the maximum).

``decode_f32_onehot`` is a float32 step-by-step emulation of the decode for rows whose softmax is exactly one-hot, in np.float32
add / multiply / divide only (all correctly rounded, none fused); ``gemv_f32`` is fp32 NumPy in the summation order of
fc_gemv_kernel.  The second half builds the inputs the GPU test and the host test share."""
import numpy as np

U24 = 2.0 ** -24                                   # fp32 unit roundoff
F32_EPS_NORMALIZE = float(np.float32(1e-12))       # F.normalize's eps as an fp32 tensor meets it
VFOV_LO, VFOV_HI, ANGLE_LO, ANGLE_HI = 0.2617, 2.1, -0.6, 0.6      # camcalib/cam_utils.py:94-107
ACTIVATIONS = ('', 'relu', 'softplus', 'sigmoid', 'tanh', 'elu')


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- Linear layers and the regressor loop ------------------------------------------------------------------------------------

def linear(x, w, b, res=None):
    """out[i, n] = w[n] . x[i] + b[n] (+ res[i, n]) in float64 -> (out, mag), mag = sum_k |w||x| + |b| (+ |res|): what every
    summation bound multiplies."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid='ignore'):
        out, mag = x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)
        if res is not None:
            out, mag = out + np.asarray(res, np.float64), mag + np.abs(np.asarray(res, np.float64))
    return out, mag


def ief(xf, cam_feats, state, n_iter=3):
    """HMRHead's iterative error feedback in float64.  ``state``: {'fc1.weight', ..., 'init_pose', 'init_shape', 'init_cam'} with
    the variance decoders in the separate layout ('decpose_var.*', 'decshape_var.*') when present; cam_feats (B, 7) or None
    -> dict(pred_pose_6d, pred_shape, pred_cam [, var_pose, var_shape: the raw variance outputs of the last iteration])."""
    xf = np.asarray(xf, np.float64)
    B = xf.shape[0]
    g = lambda k: np.asarray(state[k], np.float64)
    pose, shape, cam = (np.broadcast_to(g(k).reshape(1, -1), (B, g(k).size)) for k in ('init_pose', 'init_shape', 'init_cam'))
    var = {}
    for _ in range(n_iter):
        xc = np.concatenate([xf, pose, shape, cam] + ([np.asarray(cam_feats, np.float64)] if cam_feats is not None else []), 1)
        h = linear(linear(xc, g('fc1.weight'), g('fc1.bias'))[0], g('fc2.weight'), g('fc2.bias'))[0]
        if 'decpose_var.weight' in state:
            var = {'var_pose': linear(h, g('decpose_var.weight'), g('decpose_var.bias'))[0],
                   'var_shape': linear(h, g('decshape_var.weight'), g('decshape_var.bias'))[0]}
        pose = linear(h, g('decpose.weight'), g('decpose.bias'), pose)[0]
        shape = linear(h, g('decshape.weight'), g('decshape.bias'), shape)[0]
        cam = linear(h, g('deccam.weight'), g('deccam.bias'), cam)[0]
    return dict(pred_pose_6d=pose, pred_shape=shape, pred_cam=cam, **var)


def gemv_f32(x, w, b, res=None):
    """fp32 NumPy in fc_gemv_kernel's order: lane l takes the quads k = 4 l + 256 u, u = 0, 1, ... of the row padded to
    Kp = K rounded up to 32 as one fused-multiply-add chain from +0 (the product is exact in float64, so float32(float64 product +
    acc) is one rounding of the exact value up to a double rounding), then the xor-shuffle tree over the 64 lanes, then bias, then
    residual.  x (B, K), w (N, K), b (N) -> (B, N) float32."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    B, K = x.shape
    N = w.shape[0]
    Kp = -(-K // 32) * 32
    steps = -(-Kp // 256)
    xp, wp = np.zeros((B, steps * 256), np.float64), np.zeros((N, steps * 256), np.float64)
    xp[:, :K], wp[:, :K] = x, w
    acc = np.zeros((B, N, 64), np.float32)
    for u in range(steps):
        for q in range(4):
            k = u * 256 + 4 * np.arange(64) + q
            acc = (xp[:, None, k] * wp[None, :, k] + acc.astype(np.float64)).astype(np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, np.arange(64) ^ o]
    out = acc[:, :, 0] + np.asarray(b, np.float32)[None]
    return out if res is None else out + np.asarray(res, np.float32)


def gemv_c(K):
    """The rounding constant of fc_gemv_kernel: |out - exact| <= gamma(c) mag, c = 4 ceil(Kp / 256) + 8 - the lane-local chain
    rounds once per fused multiply-add (4 per 256-column step), the six shuffle levels once each, bias and residual once each."""
    Kp = -(-K // 32) * 32
    return 4 * -(-Kp // 256) + 8


def gamma(c):
    """(1 + u)^c - 1 <= c u / (1 - c u), u = 2^-24 (Higham's gamma_c)."""
    return c * U24 / (1 - c * U24)


# ---- rot6d, the activations, the state row --------------------------------------------------------------------------------------

def rot6d_to_rotmat(p, dtype=np.float64):
    """(..., 6) viewed (3, 2): a1 = p[0], p[2], p[4], a2 = p[1], p[3], p[5] -> (..., 3, 3) with columns b1 b2 b3.  dtype
    np.float32 evaluates the same steps in correctly rounded fp32 operations, none fused."""
    x = np.asarray(p, np.float32).astype(dtype).reshape(-1, 3, 2)
    eps = dtype(F32_EPS_NORMALIZE)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        nrm = lambda v: np.maximum(np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])), eps)[:, None]
        b1 = a1 / nrm(a1)
        d = (b1[:, 0] * a2[:, 0] + b1[:, 1] * a2[:, 1] + b1[:, 2] * a2[:, 2])[:, None]
        u = a2 - d * b1
        b2 = u / nrm(u)
        b3 = np.stack([b1[:, 1] * b2[:, 2] - b1[:, 2] * b2[:, 1], b1[:, 2] * b2[:, 0] - b1[:, 0] * b2[:, 2],
                       b1[:, 0] * b2[:, 1] - b1[:, 1] * b2[:, 0]], 1)
    return np.stack([b1, b2, b3], -1).reshape(np.shape(p)[:-1] + (3, 3))


def uncertainty_act(x, name):
    """torch.nn.functional.<name> at its defaults, in float64 from the fp32 input: softplus (beta 1, threshold 20), elu (alpha 1)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        if name == '':
            return x
        if name == 'relu':
            return np.where(np.isnan(x), x, np.maximum(x, 0.0))
        if name == 'softplus':
            return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 30.0))))
        if name == 'sigmoid':
            return 1.0 / (1.0 + np.exp(-x))
        if name == 'tanh':
            return np.tanh(x)
        if name == 'elu':
            return np.where(x > 0.0, x, np.expm1(np.minimum(x, 0.0)))
    raise ValueError(name)


def head_state_row(init_pose, init_shape, init_cam, R, K, img_h):
    """The IEF state columns after xf: [pose6d 144 | shape 10 | cam 3 | R[:, :, :2] row-major 6 | vfov = 2 atan(h / (2 K00)) 1]
    -> (B, 164) float64 from fp32 inputs; R (B,3,3), K (B,3,3), img_h (B)."""
    R, K, h = (np.asarray(a, np.float32).astype(np.float64) for a in (R, K, img_h))
    B = R.shape[0]
    head = np.concatenate([np.asarray(a, np.float32).astype(np.float64).reshape(-1) for a in (init_pose, init_shape, init_cam)])
    return np.concatenate([np.broadcast_to(head, (B, 157)), R[:, :, :2].reshape(B, 6), (2 * np.arctan(h / (2 * K[:, 0, 0])))[:, None]], 1)


# ---- CamCalib decode -----------------------------------------------------------------------------------------------------------

def _range(head):
    lo, hi = (VFOV_LO, VFOV_HI) if head == 0 else (ANGLE_LO, ANGLE_HI)
    return np.float32(hi - lo), np.float32(lo)         # python doubles, rounded to fp32 where they meet the tensor


def soft_to_angle(s, head):
    """soft index in [-1, 1] -> radians, float64 arithmetic on the fp32 constants; head 0 = vfov, 1 = pitch, 2 = roll."""
    span, lo = _range(head)
    return float(span) * ((np.asarray(s, np.float64) + 1.0) / 2.0) + float(lo)


def soft_index(logits):
    """softargmax1d(normalize_keypoints=True) of (rows, nbins) logits in float64 -> [-1, 1]; NaN where the softmax is (a NaN, a
    +inf, or nothing but -inf in the row)."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    n = x.shape[-1]
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        e = np.exp(x - x.max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True) * np.arange(n)).sum(-1) / (n - 1) * 2 - 1


def decode(lv, lp, lr):
    """(vfov, pitch, roll) in float64 from three (B, nbins) fp32 logit tensors."""
    return tuple(soft_to_angle(soft_index(l), k) for k, l in enumerate((lv, lp, lr)))


def decode_f32_onehot(k, nbins, head):
    """The angle of a row whose softmax is exactly one-hot at bin k, step by step in np.float32: the expectation is k, then
    k / (nbins - 1) * 2 - 1, then span * ((s + 1) / 2) + lo - divide, multiply, add, each correctly rounded, none fused."""
    f = np.float32
    span, lo = _range(head)
    s = f(k) / f(nbins - 1) * f(2) - f(1)
    return span * ((s + f(1)) / f(2)) + lo


def focal(vfov, h):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.asarray(h, np.float64) / 2.0 / np.tan(np.asarray(vfov, np.float64) / 2.0)


def cam_RK(pitch, roll, f, w, h):
    """R = euler2matrix([pitch, 0, roll]) by the quaternion route and K with K[2,2] = 0 -> (B,3,3), (B,3,3) float64."""
    p, r, f, w, h = (np.asarray(a, np.float64).reshape(-1) for a in (pitch, roll, f, w, h))
    with np.errstate(invalid='ignore'):
        cx, sx, cz, sz = np.cos(p / 2), np.sin(p / 2), np.cos(r / 2), np.sin(r / 2)
        q = np.stack([cx * cz, cz * sx, -sx * sz, cx * sz], 1)             # euler_to_quaternion with y = 0
        q = q / np.sqrt((q * q).sum(1, keepdims=True))
        qw, qx, qy, qz = q.T
        R = np.stack([qw * qw + qx * qx - qy * qy - qz * qz, 2 * qx * qy - 2 * qw * qz, 2 * qw * qy + 2 * qx * qz,
                      2 * qw * qz + 2 * qx * qy, qw * qw - qx * qx + qy * qy - qz * qz, 2 * qy * qz - 2 * qw * qx,
                      2 * qx * qz - 2 * qw * qy, 2 * qw * qx + 2 * qy * qz, qw * qw - qx * qx - qy * qy + qz * qz], 1).reshape(-1, 3, 3)
    K = np.zeros((p.size, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2] = w / 2, h / 2
    return R, K


def bins_argmax(x):
    """np.argmax per row: the first maximum; a NaN counts as the maximum (the first NaN's index)."""
    return np.argmax(np.asarray(x, np.float32), axis=-1).astype(np.int32)


# ---- the tolerance rule ---------------------------------------------------------------------------------------------------------

def budget(f64, ref32, ulps=4):
    """Per element: 2 |fp32 oracle - float64| + ``ulps`` ulp32(float64), with the smallest normal 2^-126 as the floor where the
    result lies in the subnormal range (a flush to zero there is as good as fp32 gets)."""
    f64 = np.asarray(f64, np.float64)
    with np.errstate(invalid='ignore'):
        tol = 2 * np.abs(np.asarray(ref32, np.float64) - f64) + ulps * ulp32(f64)
        return np.where(np.abs(f64) < 2.0 ** -126, np.maximum(tol, 2.0 ** -126), tol)


def norm_budget(f64, ref32, ulps=4):
    """The same rule in the tensor max-norm, as tests/test_gpu_camcalib_eval.py takes it: 2 max |oracle - float64| + ``ulps``
    ulp32(max |float64|)."""
    f64 = np.asarray(f64, np.float64)
    return 2 * np.abs(np.asarray(ref32, np.float64) - f64).max() + ulps * float(ulp32(np.abs(f64).max()))


def same_kind(a, b):
    """NaN where NaN, +inf where +inf, -inf where -inf, finite where finite."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and
                np.array_equal(np.isneginf(a), np.isneginf(b)))


def bits(a):
    """fp32 bit patterns with -0 folded onto +0 (0 - 0 and a fused 0 * 0 - 0 may differ in that sign and in nothing else)."""
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)


# =================================================================================================================================
# shared inputs
# =================================================================================================================================

# ---- Linear layers: (K, N, B, heads, residual in place, ldx - Kp, ldo - N) --------------------------------------------------------
# every K, N and B the kernel treats differently at least once: K below / at / past a quad, a 32-column pad, one 256-column step,
# Kp past 2304 = a second trip of the outer loop; N around a block of four columns; B = 1 (one image per wave), even, odd last pair
GEMV_CASES = [(1, 1, 1, 1, False, 0, 0), (31, 3, 2, 3, False, 0, 0), (32, 4, 3, 1, True, 0, 3), (33, 5, 10, 1, False, 4, 0),
              (252, 157, 11, 1, True, 0, 0), (256, 311, 2, 3, True, 0, 0), (260, 5, 3, 1, False, 0, 0), (1024, 157, 1, 1, True, 0, 0),
              (2212, 157, 3, 1, True, 8, 7), (2304, 4, 2, 1, False, 0, 0), (2305, 3, 11, 3, True, 0, 1), (4640, 5, 10, 1, False, 0, 0),
              (4640, 1, 1, 3, False, 4, 2)]
# matrix cores: (K, N, B); each with option fc_splitk 0 / 1, with and without the in-place residual.  B = 1025 crosses run_fc's row block
# (K = 33: the packed operand's own zero pad, columns 33..63, meets the 7.0 of x)
MFMA_CASES = [(32, 1, 1), (32, 63, 63), (32, 64, 64), (32, 65, 65), (32, 157, 1025), (2240, 157, 1), (2240, 65, 65), (2240, 1, 64),
              (33, 5, 3)]
ROUNDING_CASES = [(2212, 157, 3), (1024, 311, 2)]
PAD_VALUE = 7.0          # what columns [K, ldx) of every x row hold: a weight pad that is not zero shows


def fc_exact_case(K, N, B, heads=1, residual=False, seed=0):
    """Integer operands - w in [-2, 2], x in [-4, 4], bias and residual in [-8, 8]: with K <= 4640 every partial sum stays below
    2^24, so the fp32 result is the same in every summation order and equals float64.  The last row of w and the last image of x
    are patterns unlike the random rest.  -> list of (w (N,K), b (N), x (B,K), res (B,N) or None, expected (B,N) float64)."""
    rng = np.random.default_rng([K, N, B, heads, seed])
    out = []
    for _ in range(heads):
        w = rng.integers(-2, 3, (N, K)).astype(np.float32)
        x = rng.integers(-4, 5, (B, K)).astype(np.float32)
        w[-1] = (np.arange(K) % 5) - 2
        x[-1] = 4 - (np.arange(K) % 9)
        b = rng.integers(-8, 9, N).astype(np.float32)
        res = rng.integers(-8, 9, (B, N)).astype(np.float32) if residual else None
        want, mag = linear(x, w, b, res)
        assert mag.max() < 2 ** 24
        out.append((w, b, x, res, want))
    return out


def fc_gaussian_case(K, N, B, seed=0):
    rng = np.random.default_rng([K, N, B, seed, 1])
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    x, b = rng.standard_normal((B, K)).astype(np.float32), (0.1 * rng.standard_normal(N)).astype(np.float32)
    res = rng.standard_normal((B, N)).astype(np.float32)
    return w, b, x, res


# ---- rot6d: 24 joints ----------------------------------------------------------------------------------------------------------

def _p6(a1, a2):
    # viewed (3, 2): column 0 = a1; + 0.0 turns the -0 of a negated axis into +0 (a -0 would not survive the regressor's 0 + init)
    return np.stack([np.asarray(a1, np.float64), np.asarray(a2, np.float64)], -1).reshape(6) + 0.0


def rot6d_cases():
    """(init_pose (144,) float32, expected (24, 3, 3) float64 with NaN where no closed form is listed, names).  Joints 0..11 have
    dyadic components and a matrix known in advance; 12..23 are well-conditioned random pairs (a rotation's first two columns,
    rescaled, with every entry of the result at least 0.2 in magnitude)."""
    X, Y, Z, O = np.eye(3)[0], np.eye(3)[1], np.eye(3)[2], np.zeros(3)
    col = lambda b1, b2, b3: np.stack([b1, b2, b3], -1)
    tiny = 2.0 ** -45
    b1t = float(np.float32(tiny) / np.float32(F32_EPS_NORMALIZE))           # below the eps: a1 / eps, not a unit vector
    named = [
        ('xy', _p6(X, Y), col(X, Y, Z)), ('yx', _p6(Y, X), col(Y, X, -Z)), ('zx', _p6(Z, X), col(Z, X, Y)),
        ('-x z', _p6(-X, Z), col(-X, Z, Y)), ('y -z', _p6(Y, -Z), col(Y, -Z, -X)), ('-z -y', _p6(-Z, -Y), col(-Z, -Y, -X)),
        ('a1 = 0', _p6(O, 2 * Y), col(O, Y, O)), ('a2 parallel to a1', _p6(X, 0.5 * X), col(X, O, O)),
        ('|a1| = 2^-45', _p6(tiny * X, Y), col(b1t * X, Y, b1t * Z)), ('both zero', _p6(O, O), col(O, O, O)),
        ('3x 4y', _p6(3 * X, 4 * Y), col(X, Y, Z)), ('-2z, y/2', _p6(-2 * Z, 0.5 * Y), col(-Z, Y, X)),
    ]
    rng = np.random.default_rng(24)
    pose, want = [p for _, p, _ in named], [m for _, _, m in named]
    while len(pose) < 24:
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.abs(q).min() < 0.2:
            continue
        s1, s2, t = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(-0.05, 0.05)
        pose.append(_p6(s1 * q[:, 0], s2 * q[:, 1] + t * q[:, 0]))
        want.append(np.full((3, 3), np.nan))
    return np.concatenate(pose).astype(np.float32), np.stack(want), [n for n, _, _ in named]


N_EXACT_JOINTS = 12
INIT_SHAPE = np.array([0.5, -1.25, 3.0, 0.0, 2.0 ** -20, -7.0, 1.5, 0.125, -0.375, 100.0], np.float32)
INIT_CAM = np.array([0.90625, -0.03125, 0.015625], np.float32)

# ---- head_var: the edge values of the six activations ---------------------------------------------------------------------------
# (in fp32 softplus(x) IS x from about 13.9 on - exp(-x) falls below half an ulp of x - so the threshold 20 itself cannot be seen
# in the result: 12 and 13.5, where log1p(exp(x)) still differs from x, are what tells a threshold below them from the right one)
VAR_EDGES = np.array([-np.inf, -104.0, -88.0, -20.0, -1e-8, -0.0, 0.0, 1e-8, 19.999998, 20.0, 20.000002, 88.8, 104.0, np.inf, np.nan,
                      12.0, 13.5], np.float32)


def var_biases():
    """(144,), (10,) float32: the edge values first, padded out with Gaussians; the shape decoder gets the ten of them that decide
    a branch (the two infinities and NaN, the softplus threshold and its neighbours, the kink at 0 and its neighbours)."""
    rng = np.random.default_rng(144)
    pose = np.concatenate([VAR_EDGES, (3 * rng.standard_normal(144 - VAR_EDGES.size)).astype(np.float32)])
    shape = VAR_EDGES[[0, 13, 14, 8, 9, 10, 4, 5, 7, 1]]
    return pose.astype(np.float32), shape.astype(np.float32)


# ---- head_init: the selector model ----------------------------------------------------------------------------------------------

def selector_inputs(B):
    """cam_rotmat with nine distinct small dyadic entries per image (no two images alike), K00 from {300, 5000} and img_h from
    {1, 480} in every combination -> R (B,3,3), K (B,3,3), img_h (B) float32."""
    b = np.arange(B)
    R = ((np.arange(9)[None] * 2 + 1 + 18 * b[:, None]) * np.where(np.arange(9) % 2, -1, 1)[None] / 64.0).reshape(B, 3, 3)
    K = np.zeros((B, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = np.where(b % 2, 5000.0, 300.0)
    K[:, 0, 2], K[:, 1, 2] = 320.0, 240.0
    return R.astype(np.float32), K.astype(np.float32), np.where((b // 2) % 2, 480.0, 1.0).astype(np.float32)


# ---- CamCalib decode rows --------------------------------------------------------------------------------------------------------
NBINS = (2, 63, 64, 65, 256, 257)
IMG_SIZES = ((1.0, 1.0), (480.0, 640.0), (4000.0, 6000.0))        # (img_h, img_w)
ROW_NAMES = ('one-hot first', 'one-hot middle', 'one-hot last', 'all equal', 'spans +-1e4', 'gaussian', 'gaussian', 'gaussian',
             'ties', 'all -inf', 'one +inf', 'one NaN')
ONE_HOT_ROWS, BIG_ROW, ORDINARY_ROWS, NAN_ROWS = (0, 1, 2), 4, (0, 1, 2, 3, 5, 6, 7, 8), (9, 10, 11)


def one_hot_bins(nbins):
    return (0, nbins // 2, nbins - 1)


def tie_bins(nbins):
    """Where the 'ties' row holds its maximum: a first bin, the bin 64 after it where there is one (the same lane of the wave meets
    both), and the last bin."""
    t0 = min(nbins // 3, nbins - 65) if nbins > 64 else nbins // 3
    return sorted({t0, t0 + 64 if t0 + 64 < nbins else t0, nbins - 1})


def decode_rows(nbins):
    """(3, 12, nbins) float32 logits, heads vfov / pitch / roll, rows as ROW_NAMES; (12,) img_h, (12,) img_w.  The one-hot rows sit
    at the same bins in every head (the middle bin of an odd count decodes pitch = roll = 0); the Gaussian rows differ per head;
    'ties' holds its maximum at ``tie_bins`` (the first index wins the argmax)."""
    rng = np.random.default_rng(nbins)
    x = np.empty((3, len(ROW_NAMES), nbins), np.float32)
    for h in range(3):
        for r, k in zip(ONE_HOT_ROWS, one_hot_bins(nbins)):
            x[h, r] = -np.inf
            x[h, r, k] = 0.75 * (h + 1)
        x[h, 3] = -1.5
        x[h, BIG_ROW] = np.linspace(-1e4, 1e4, nbins)
        x[h, 5:8] = (2.0 * rng.standard_normal((3, nbins))).astype(np.float32)
        x[h, 8] = np.round(rng.standard_normal(nbins) * 4) / 4
        x[h, 8, tie_bins(nbins)] = 9.0
        x[h, 9] = -np.inf
        x[h, 10] = x[h, 5]
        x[h, 10, (h + nbins // 2) % nbins] = np.inf
        x[h, 11] = x[h, 6]
        x[h, 11, [(2 * h + 1) % nbins, nbins - 1]] = np.nan
    sizes = np.array([IMG_SIZES[r % 3] for r in range(len(ROW_NAMES))], np.float32)
    return x, sizes[:, 0].copy(), sizes[:, 1].copy()


# ---- cam_params -----------------------------------------------------------------------------------------------------------------
CAM_PARAMS_B = (1, 63, 64, 65)


def cam_params_inputs(B):
    """pitch, roll in +-pi/2 (image 0: both exactly 0 - the identity; image B - 1 unlike the rest), f_pix, img_w, img_h float32."""
    rng = np.random.default_rng(B)
    pitch, roll = (rng.uniform(-np.pi / 2, np.pi / 2, B).astype(np.float32) for _ in range(2))
    f, w, h = (rng.uniform(lo, hi, B).astype(np.float32) for lo, hi in ((200, 5000), (1, 6000), (1, 4000)))
    pitch[0] = roll[0] = 0.0
    pitch[-1], roll[-1], f[-1], w[-1], h[-1] = (0.0 if B == 1 else 1.5), (0.0 if B == 1 else -1.25), 1234.5, 6001.0, 4001.0
    return pitch, roll, f, w, h
