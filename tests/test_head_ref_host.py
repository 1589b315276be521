"""tests/head_ref.py - the float64 yardstick of tests/test_gpu_head_edges.py - pinned on the host to the torch code under oracle/
(oracle.heads.HMRHead, oracle.geometry.rot6d_to_rotmat, oracle.models.decode_angles / focal_from_vfov / cam_params,
torch.nn.functional), on every input family the GPU test uses.  Each test also shows that the fp32 oracle itself stays inside the
tolerance the GPU test applies, with its margin: a tolerance the reference's own arithmetic cannot meet would be no yardstick."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_ref as H

torch.set_grad_enabled(False)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def _ulps(got, f64):
    return np.abs(np.asarray(got, np.float64) - f64) / H.ulp32(f64)


# ---- Linear layers -------------------------------------------------------------------------------------------------------------

def test_integer_layers_are_exact_in_any_order():
    """Every exact case: fp32 torch, fp32 NumPy in the GEMV kernel's order and float64 agree bit for bit."""
    cases = [c[:5] for c in H.GEMV_CASES] + [(K, N, min(B, 65), 1, r) for K, N, B in H.MFMA_CASES for r in (False, True)]
    for K, N, B, heads, res in cases:
        for w, b, x, r, want in H.fc_exact_case(K, N, B, heads, res):
            o32 = F.linear(t(x), t(w), t(b)).numpy() + (0 if r is None else r)
            assert o32.dtype == np.float32 and np.array_equal(o32.astype(np.float64), want), (K, N, B)
            assert np.array_equal(H.gemv_f32(x, w, b, r).astype(np.float64), want), (K, N, B)
            assert not np.array_equal(want[-1], want[0]) or B == 1 or N == 1


def test_gemv_order_meets_its_rounding_bound():
    """Gaussian operands: fp32 in the kernel's order is within gamma(c) mag, c = 4 ceil(Kp / 256) + 8 - and so is torch's fp32 within
    the order-free c = K + 2 the matrix-core path is held to."""
    for K, N, B in H.ROUNDING_CASES:
        w, b, x, res = H.fc_gaussian_case(K, N, B)
        want, mag = H.linear(x, w, b, res)
        got = H.gemv_f32(x, w, b, res).astype(np.float64)
        c = H.gemv_c(K)
        assert c == {2212: 44, 1024: 24}[K]
        reached = (np.abs(got - want) / (H.U24 * mag)).max()
        assert reached <= c / (1 - c * H.U24) and reached < 0.25 * c, (K, reached)        # random roundings: far inside the worst case
        o32 = (F.linear(t(x), t(w), t(b)) + t(res)).numpy().astype(np.float64)
        assert np.all(np.abs(o32 - want) <= H.gamma(K + 2) * mag)


# ---- the regressor loop --------------------------------------------------------------------------------------------------------

def _head(Fc, ucf, var, separate, seed):
    from oracle.heads import HMRHead
    mp = {'pose': np.zeros(144, np.float32), 'shape': np.zeros(10, np.float32), 'cam': np.zeros(3, np.float32)}
    head = HMRHead(Fc, smpl_mean_params=mp, estimate_var=var, use_separate_var_branch=separate, use_cam_feats=ucf).eval()
    g = torch.Generator().manual_seed(seed)
    for p in head.parameters():
        p.copy_(0.05 * torch.randn(p.shape, generator=g))
    pose, _, _ = H.rot6d_cases()
    head.init_pose.copy_(t(pose)[None]); head.init_shape.copy_(t(H.INIT_SHAPE)[None]); head.init_cam.copy_(t(H.INIT_CAM)[None])
    return head


def _separate_state(head):
    sd = {k: v.numpy() for k, v in head.state_dict().items()}
    if head.estimate_var and not head.use_separate_var_branch:
        for name, n in (('decpose', 144), ('decshape', 10)):
            for part in ('weight', 'bias'):
                full = sd[f'{name}.{part}']
                sd[f'{name}.{part}'], sd[f'{name}_var.{part}'] = full[:n], full[n:]
    return sd


@pytest.mark.parametrize('ucf,var,separate', [(True, False, False), (False, False, False), (True, True, False), (True, True, True)])
def test_ief_follows_hmr_head(ucf, var, separate):
    head = _head(64, ucf, var, separate, 5)
    B = 3
    g = torch.Generator().manual_seed(6)
    feat = torch.randn(B, 64, 2, 2, generator=g)
    R, K, ih = (t(a) for a in H.selector_inputs(B))
    vfov = 2 * torch.atan(ih / (2 * K[:, 0, 0]))
    want = head.double()(feat.double(), cam_rotmat=R.double(), cam_vfov=vfov.double()) if ucf else head.double()(feat.double())
    row = H.head_state_row(head.init_pose.numpy(), head.init_shape.numpy(), head.init_cam.numpy(), R.numpy(), K.numpy(), ih.numpy())
    got = H.ief(feat.double().mean((2, 3)).numpy(), row[:, 157:] if ucf else None, _separate_state(head.float()))
    for k in ('pred_pose_6d', 'pred_shape', 'pred_cam'):
        assert np.abs(got[k] - want[k].numpy()).max() < 1e-6, k        # (the camera features pass through fp32 on their way in)
    if var:
        assert np.abs(got['var_pose'] - want['pred_pose_var'][:, 144:].numpy()).max() < 1e-6
        assert np.abs(got['var_shape'] - want['pred_shape_var'][:, 10:].numpy()).max() < 1e-6


def test_state_row_layout_and_vfov_margin():
    """Columns 157..162 are R[:, :, :2] row-major (oracle.geometry.rotmat_to_rot6d), column 163 the vfov; fp32 torch is within 2 ulp
    of the float64 vfov on the four (K00, img_h) combinations - the GPU test allows 4."""
    from oracle.geometry import rotmat_to_rot6d
    R, K, ih = H.selector_inputs(4)
    row = H.head_state_row(np.zeros(144), H.INIT_SHAPE, H.INIT_CAM, R, K, ih)
    assert np.array_equal(row[:, 157:163], rotmat_to_rot6d(t(R)).numpy().astype(np.float64))
    assert np.array_equal(row[0, 144:157], np.concatenate([H.INIT_SHAPE, H.INIT_CAM]).astype(np.float64))
    assert len({(float(K[b, 0, 0]), float(ih[b])) for b in range(4)}) == 4
    v32 = (2 * torch.atan(t(ih) / (2 * t(K)[:, 0, 0]))).numpy()
    assert _ulps(v32, row[:, 163]).max() <= 2
    assert _ulps(np.float32(3) * v32, 3 * row[:, 163]).max() <= 3 and _ulps((v32 + v32) + v32, 3 * row[:, 163]).max() <= 3


def test_zero_weight_head_returns_its_init_vectors():
    """Every head weight and bias zero: the oracle's regressed state IS the init vectors, bit for bit, and its rotations are the
    expected matrices of head_ref.rot6d_cases."""
    head = _head(64, True, False, False, 7)
    for p in head.parameters():
        p.zero_()
    R, K, ih = (t(a) for a in H.selector_inputs(3))
    out = head(torch.randn(3, 64, 2, 2), cam_rotmat=R, cam_vfov=2 * torch.atan(ih / (2 * K[:, 0, 0])))
    pose, want, names = H.rot6d_cases()
    assert np.array_equal(out['pred_pose_6d'].numpy().view(np.uint32), np.broadcast_to(pose, (3, 144)).view(np.uint32))
    assert np.array_equal(out['pred_shape'].numpy(), np.broadcast_to(H.INIT_SHAPE, (3, 10)))
    assert np.array_equal(out['pred_cam'].numpy(), np.broadcast_to(H.INIT_CAM, (3, 3)))
    assert np.array_equal(H.bits(out['pred_pose'].numpy()[0, :H.N_EXACT_JOINTS]), H.bits(want[:H.N_EXACT_JOINTS]))


# ---- rot6d ---------------------------------------------------------------------------------------------------------------------

def test_rot6d_cases_exact_and_margin():
    from oracle.geometry import rot6d_to_rotmat
    pose, want, names = H.rot6d_cases()
    assert len(names) == H.N_EXACT_JOINTS and pose.shape == (144,)
    o32 = rot6d_to_rotmat(t(pose)[None]).numpy().reshape(24, 3, 3)
    f64 = H.rot6d_to_rotmat(pose.reshape(24, 6))
    f32 = H.rot6d_to_rotmat(pose.reshape(24, 6), np.float32)
    n = H.N_EXACT_JOINTS
    # the twelve dyadic joints: the closed form, the float64 yardstick (rounded once: a1 / eps is no fp32 number before that), its
    # fp32 evaluation and the oracle are one set of bits
    for name, a, b, c, d in zip(names, want[:n], f64[:n], f32[:n], o32[:n]):
        assert np.array_equal(H.bits(a), H.bits(b)) and np.array_equal(H.bits(a), H.bits(c)) and np.array_equal(H.bits(a), H.bits(d)), name
    sub = want[names.index('|a1| = 2^-45')]
    assert 0.02 < sub[0, 0] < 0.03 and sub[0, 0] == sub[2, 2]                       # a1 / eps: not a unit vector
    # the random joints: every entry at least 0.2, the oracle within 2 ulp of float64 per element (the GPU test allows 4)
    assert np.abs(f64[n:]).min() >= 0.19 and np.abs(np.linalg.det(f64[n:]) - 1).max() < 1e-12
    assert _ulps(o32[n:], f64[n:]).max() <= 2.0, _ulps(o32[n:], f64[n:]).max()
    assert _ulps(f32[n:], f64[n:]).max() <= 3.0            # every step rounded on its own, nothing fused (measured: 2.3)


# ---- the activations -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', H.ACTIVATIONS)
def test_activations_follow_torch(name):
    """Same kind on the non-finite edges, ReLU and the identity exact, the rest within 2 ulp of float64 (measured: 0.5 on the edge
    values, 1.15 at worst on the Gaussian padding, where torch's vectorised exp is used) - so the GPU budget
    2 |oracle - float64| + 4 ulp is 4 to 8 ulp."""
    pose, shape = H.var_biases()
    x = np.concatenate([pose, shape])
    o32 = (getattr(F, name)(t(x)) if name else t(x)).numpy()
    f64 = H.uncertainty_act(x, name)
    assert H.same_kind(o32, f64), name
    fin = np.isfinite(f64)
    if name in ('', 'relu'):
        assert np.array_equal(o32[fin].astype(np.float64), f64[fin])
    else:
        normal = fin & (np.abs(f64) >= 2.0 ** -126)
        assert _ulps(o32[normal], f64[normal]).max() <= 2.0, _ulps(o32[normal], f64[normal]).max()
        assert np.all(np.abs(o32[fin] - f64[fin]) <= H.budget(f64[fin], o32[fin]))
    want = {'softplus': {20.0: 20.0 + np.log1p(np.exp(-20.0)), 20.000002: float(np.float32(20.000002))}, 'relu': {-np.inf: 0.0},
            'sigmoid': {np.inf: 1.0, -np.inf: 0.0}, 'tanh': {np.inf: 1.0, -np.inf: -1.0}, 'elu': {-np.inf: -1.0, np.inf: np.inf}}
    for v, y in want.get(name, {}).items():
        got = f64[np.flatnonzero(x == np.float32(v))[0]]
        assert got == y or abs(got - y) <= 1e-12 * max(1.0, abs(y)), (name, v)
    assert np.isnan(f64[np.isnan(x)]).all()                                           # a NaN stays a NaN in all six


# ---- CamCalib decode ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nbins', H.NBINS)
def test_decode_follows_the_oracle(nbins):
    from oracle.models import decode_angles, focal_from_vfov
    x, ih, iw = H.decode_rows(nbins)
    o32 = [a.numpy() for a in decode_angles(t(x[0]), t(x[1]), t(x[2]))]
    f64 = H.decode(x[0], x[1], x[2])
    for h in range(3):
        assert o32[h].dtype == np.float32
        # NaN exactly on the all -inf, the +inf and the NaN row
        assert np.array_equal(np.flatnonzero(np.isnan(o32[h])), H.NAN_ROWS) and np.array_equal(np.flatnonzero(np.isnan(f64[h])), H.NAN_ROWS)
        # one-hot rows: the fp32 emulation IS the oracle
        for r, k in zip(H.ONE_HOT_ROWS, H.one_hot_bins(nbins)):
            assert o32[h][r] == H.decode_f32_onehot(k, nbins, h), (nbins, h, k)
        lo, hi = (H.VFOV_LO, H.VFOV_HI) if h == 0 else (H.ANGLE_LO, H.ANGLE_HI)
        assert o32[h][0] == np.float32(lo)
        assert abs(float(o32[h][2]) - hi) <= H.ulp32(hi) and o32[h][2] == H._range(h)[0] + H._range(h)[1]
        if nbins % 2 and h > 0:
            assert o32[h][1] == 0.0                                                   # the middle bin of an odd count: exactly 0
        # the +-1e4 row stays finite and decodes to the top of the range
        assert np.isfinite(o32[h][H.BIG_ROW]) and o32[h][H.BIG_ROW] == o32[h][2]
        fin = list(H.ORDINARY_ROWS) + [H.BIG_ROW]
        assert np.all(np.abs(o32[h][fin] - f64[h][fin]) <= 8 * H.ulp32(np.abs(f64[h][fin]).max()))     # the restatement agrees
    f32 = focal_from_vfov(o32[0], ih)
    assert f32.dtype == np.float32
    fin = ~np.isnan(f64[0])
    assert np.all(np.abs(f32[fin] / ih[fin] - H.focal(f64[0], ih)[fin] / ih[fin]) <= 8 * H.ulp32((H.focal(f64[0], ih) / ih)[fin].max()))
    assert np.isnan(f32[~fin]).all()


@pytest.mark.parametrize('nbins', H.NBINS)
def test_bins_argmax_known_answers(nbins):
    x, _, _ = H.decode_rows(nbins)
    for h in range(3):
        idx = H.bins_argmax(x[h])
        assert list(idx[list(H.ONE_HOT_ROWS)]) == list(H.one_hot_bins(nbins))
        assert idx[3] == 0 and idx[H.BIG_ROW] == nbins - 1 and idx[9] == 0
        ties = H.tie_bins(nbins)
        assert idx[8] == ties[0] and list(np.flatnonzero(x[h, 8] == x[h, 8].max())) == ties and len(ties) >= 2
        assert nbins <= 64 or (ties[1] - ties[0]) % 64 == 0                             # two of them in one lane of the wave
        assert idx[10] == (h + nbins // 2) % nbins and idx[11] == min((2 * h + 1) % nbins, nbins - 1)
        assert np.array_equal(idx, torch.argmax(t(x[h]), dim=-1).numpy()) or nbins == 2


@pytest.mark.parametrize('B', H.CAM_PARAMS_B)
def test_cam_RK_follows_the_oracle(B):
    from oracle.models import cam_params
    pitch, roll, f, w, h = H.cam_params_inputs(B)
    R32, K32 = (a.numpy() for a in cam_params(pitch, roll, f, w, h))
    R64, K64 = H.cam_RK(pitch, roll, f, w, h)
    assert np.array_equal(K32.astype(np.float64), K64) and np.all(K64[:, 2] == 0)
    assert np.array_equal(H.bits(R32[0]), H.bits(np.eye(3))) and np.array_equal(R64[0], np.eye(3))
    assert np.abs(R32 - R64).max() <= 4 * H.U24                # the oracle's own error: a few units of roundoff on entries up to 1
    assert B == 1 or not np.allclose(R64[-1], R64[-2])
