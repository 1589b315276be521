"""Everything between the trunk's feature map and the SMPL mesh - spec_amd/csrc/head.hip, head_init_row and rot6d_joint - against
the float64 yardstick tests/head_ref.py (pinned to the torch oracle by tests/test_head_ref_host.py), at the shapes and values where
such kernels go wrong.

  Linear layers (specmi_fc_forward: commit's packing + launch_fc_gemv / run_fc on caller-supplied weights), integer operands whose
    fp32 sums are exact in any order ............... equal to float64 bit for bit; x pad columns hold 7.0, out is a sentinel buffer
  GEMV, +Inf in the last real quad .................. every output exactly +Inf
  Linear layers, Gaussian operands .................. |gpu - f64| <= gamma(c) (sum |w||x| + |b| + |res|): GEMV c = 4 ceil(Kp / 256) + 8
                                                      from its fixed order (44 at K = 2212, 24 at K = 1024); matrix cores the
                                                      order-free c = K + 2 (the K slicing is not read off the plan here)
  rot6d through a zero-weight model ................. the regressed state IS the init vectors; twelve dyadic joints (axis pairs,
                                                      a1 = 0, a2 parallel to a1, |a1| below the eps, both zero, non-unit) equal
                                                      the closed form and the fp32 oracle bit for bit; twelve random joints within
                                                      4 ulp of float64 per element
  the six uncertainty activations on their edges .... same kind where not finite, ReLU / identity exact, the rest per element
                                                      2 |oracle32 - f64| + 4 ulp32(f64), floor 2^-126 in the subnormal range
  head_init through a selector model ................ pred_shape[:, i] = 3 R[i // 2, i % 2] exactly, the vfov slot within 4 ulp
  camcalib_decode, 2 ... 257 bins .................... one-hot rows equal the fp32 emulation bit for bit, NaN where the oracle's are,
                                                      the rest 2 max |oracle32 - f64| + 4 ulp32(max) per quantity; K exact
  camcalib_bins ...................................... argmax exact (ties, NaN rows), soft index = the decode's
  cam_params, B around its 64-thread block .......... identity at 0, K exact, R under the same rule, null outputs, sentinels

Worst figures measured on an MI355X (profiles/head_edges.json, written by scripts/head_edges.py): rounding constant reached 0.28 /
0.34 on the GEMV (bounds 44 / 24) and 0.60 / 0.85 on the matrix cores; random rot6d joints 1.75 ulp; activations at most 0.20 of
their budget (ReLU and identity exact); vfov slot 0.70 ulp; decode angles at most 0.31, f_pix 0.14, R 0.23 of their budgets;
cam_params R 0.22.  No budget here is derived from the GPU's own output."""
import ctypes as C

import numpy as np
import pytest
import torch

from spec_amd import _lib
from tests import head_ref as H
from tests.util import SEED_HMR, SEED_SMPL, synth_states, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0x5A5AA5A5
F = 2048


def _p(a):
    return None if a is None else C.c_void_p(a.data_ptr())


def _dev(a):
    return t(np.ascontiguousarray(a)).to(DEV)


def _sentinels(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)


def _f32(a):
    return a.detach().cpu().numpy()


@pytest.fixture(scope='module')
def eng():
    from spec_amd.engine import Engine
    return Engine('camcalib', torch.device(DEV)).experimental(True)


# =================================================================================================================================
# Linear layers
# =================================================================================================================================

def _fc(eng, heads, K, N, B, ldx, ldo, path):
    """Run specmi_fc_forward on ``heads`` = [(w, b, x, res or None, ...)]: x rows of ldx floats with PAD_VALUE in [K, ldx), out a
    sentinel buffer of B rows of ldo words + 64 (the residual, when there is one, lies in out).  -> [(B, N) float32] after checking
    that nothing but out[b, :N] was written."""
    xs, outs = [], []
    for w, b, x, res, *_ in heads:
        xd = torch.full((B, ldx), H.PAD_VALUE, device=DEV)
        xd[:, :K] = _dev(x)
        buf = _sentinels(B * ldo + 64)
        if res is not None:
            buf[:B * ldo].view(B, ldo)[:, :N] = _dev(res).view(torch.int32)
        xs.append(xd)
        outs.append(buf)
    has_res = heads[0][3] is not None
    eng.fc_forward([h[0] for h in heads], [h[1] for h in heads], xs, outs, B, residual=outs if has_res else None, path=path,
                   ldx=ldx, ldo=ldo)
    torch.cuda.synchronize()
    got = []
    for buf in outs:
        words = buf.cpu().numpy()
        rows = words[:B * ldo].reshape(B, ldo)
        assert np.all(rows[:, N:] == SENTINEL), (K, N, B, 'wrote columns [N, ldo)')
        assert np.all(words[B * ldo:] == SENTINEL), (K, N, B, 'wrote past the last row')
        got.append(np.ascontiguousarray(rows[:, :N]).view(np.float32))
    return got


def _kp(K):
    return -(-K // 32) * 32


@pytest.mark.parametrize('K,N,B,heads,res,dx,do', H.GEMV_CASES)
def test_gemv_exact(eng, K, N, B, heads, res, dx, do):
    """fc_gemv_kernel on integer operands equals float64 bit for bit.  The pad columns of x hold 7.0: a weight pad that is not zero
    shows.  Columns [N, ldo) and the words after the last row keep their sentinel."""
    cases = H.fc_exact_case(K, N, B, heads, res)
    got = _fc(eng, cases, K, N, B, _kp(K) + dx, N + do, 0)
    for i, (g, c) in enumerate(zip(got, cases)):
        assert np.array_equal(g.astype(np.float64), c[4]), (K, N, B, 'head', i, np.argwhere(g != c[4])[:4])


@pytest.mark.parametrize('K,N,B', H.MFMA_CASES)
def test_matrix_core_exact(eng, K, N, B):
    """run_fc (row blocks of 1024, option fc_splitk 0 / 1, with and without the in-place residual) on the same kind of operands."""
    try:
        for splitk in (0, 1):
            eng.set_option('fc_splitk', splitk)
            for res in (False, True):
                case = H.fc_exact_case(K, N, B, 1, res, seed=splitk)
                got = _fc(eng, case, K, N, B, _kp(K) + 4 * res, N + 3 * res, 1)[0]
                assert np.array_equal(got.astype(np.float64), case[0][4]), (K, N, B, splitk, res, np.argwhere(got != case[0][4])[:4])
    finally:
        eng.set_option('fc_splitk', 1)


@pytest.mark.parametrize('B', [1, 3])
def test_gemv_inf_in_the_last_quad_stays_inf(eng, B):
    """K = 32: lanes 0..7 own one real quad each and re-read the last one (28..31) for the eight steps past the row.  That quad is
    +Inf with weight 1: every output is exactly +Inf - a re-read that contributed 0 * Inf would make it NaN."""
    K, N = 32, 5
    (w, b, x, _, _), = H.fc_exact_case(K, N, B)
    w[:, 28:], x[:, 28:] = 1.0, np.inf
    got = _fc(eng, [(w, b, x, None)], K, N, B, K, N, 0)[0]
    assert np.all(np.isposinf(got)), got


def rounding_report(eng, K, N, B, path):
    """Gaussian operands -> (worst |gpu - f64| / (2^-24 mag), c): GEMV c from the kernel's fixed order - the lane-local chain of
    4 ceil(Kp / 256) fused multiply-adds from +0 rounds once per step, the six shuffle levels once each, bias and residual once
    each (head_ref.gemv_c); matrix cores the order-free c = K + 2 (K products and sums in any order, bias, residual)."""
    w, b, x, res = H.fc_gaussian_case(K, N, B)
    want, mag = H.linear(x, w, b, res)
    got = _fc(eng, [(w, b, x, res)], K, N, B, _kp(K), N, path)[0].astype(np.float64)
    return float((np.abs(got - want) / (H.U24 * mag)).max()), (H.gemv_c(K) if path == 0 else K + 2)


@pytest.mark.parametrize('path', [0, 1])
@pytest.mark.parametrize('K,N,B', H.ROUNDING_CASES)
def test_linear_rounding_bound(eng, K, N, B, path):
    reached, c = rounding_report(eng, K, N, B, path)
    print(f'K={K} N={N} B={B} path={path}: reached c = {reached:.2f}, bound c = {c}')
    assert reached <= c / (1 - c * H.U24), (K, N, B, path, reached, c)


# =================================================================================================================================
# the HMR head through purpose-built models
# =================================================================================================================================

_models = {}


def _hmr(kind):
    """An HMR model (ResNet-50 trunk of the suite's synthetic state, use_cam and use_cam_feats) whose head is 'zero' (every weight
    and bias zero, chosen init vectors), 'var' / 'var_separate' (the same with estimate_var and the edge values as variance biases)
    or 'selector' (fc1 picks the seven camera features, fc2 passes them on, decshape writes them to seven shape slots)."""
    if kind in _models:
        return _models[kind]
    from spec_amd import assets, synth
    from spec_amd.modules import HMR
    assets.use_synthetic_assets(SEED_SMPL)
    var, separate = kind.startswith('var'), kind == 'var_separate'
    sd = {k: v for k, v in synth_states(True)[1].items() if not k.startswith('head.')}
    head = synth.hmr_state(SEED_HMR, True, estimate_var=var, use_separate_var_branch=separate, with_trunk=False)
    head = {k: np.zeros_like(np.asarray(v, np.float32)) for k, v in head.items()}
    pose, _, _ = H.rot6d_cases()
    head['head.init_pose'], head['head.init_shape'], head['head.init_cam'] = pose[None].copy(), H.INIT_SHAPE[None].copy(), H.INIT_CAM[None].copy()
    if var:
        vp, vs = H.var_biases()
        if separate:
            head['head.decpose_var.bias'], head['head.decshape_var.bias'] = vp, vs
        else:
            head['head.decpose.bias'][144:], head['head.decshape.bias'][10:] = vp, vs
    if kind == 'selector':
        head['head.init_shape'][:] = 0.0
        for i in range(7):
            head['head.fc1.weight'][i, F + 157 + i] = head['head.fc2.weight'][i, i] = head['head.decshape.weight'][i, i] = 1.0
    sd.update(head)
    m = HMR(use_cam=True, use_cam_feats=True, estimate_var=var, use_separate_var_branch=separate)
    missing, unexpected = m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith('smpl.') for k in missing), (missing, unexpected)
    m = m.to(DEV).eval()
    m.engine(torch.device(DEV)).experimental(True)
    _models[kind] = m
    return m


def _head_inputs(B):
    rng = np.random.default_rng(B)
    feat = (rng.integers(0, 64, (B, 7, 7, F)) / 16.0).astype(np.float32)
    R, K, ih = H.selector_inputs(B)
    sc, ce, iw = np.full(B, 1.25, np.float32), np.tile(np.float32([300.0, 250.0]), (B, 1)), np.full(B, 640.0, np.float32)
    return [_dev(a) for a in (feat, R, K, sc, ce, iw, ih)]


def _each_config(m, fuses=(0, 3)):
    """Every way the head runs: GEMV and matrix cores (the two plans), composed map and nine-GEMM loop, head_fuse 0 / 3."""
    eng = m.engine(torch.device(DEV))
    try:
        for plan in ('latency', 'throughput'):
            m.set_plan(plan)
            for collapse in (1, 0):
                eng.set_option('head_collapse', collapse)
                for fuse in fuses:
                    eng.set_option('head_fuse', fuse)
                    yield eng, (plan, collapse, fuse)
    finally:
        m.set_plan('auto')
        eng.set_option('head_collapse', 1)
        eng.set_option('head_fuse', 3)


def rot6d_report():
    """-> worst |pred_pose - float64| in ulp over the twelve random joints, every configuration, after asserting the exact parts."""
    from oracle.geometry import rot6d_to_rotmat
    m = _hmr('zero')
    pose, want, names = H.rot6d_cases()
    n = H.N_EXACT_JOINTS
    o32 = rot6d_to_rotmat(t(pose)[None]).numpy().reshape(24, 3, 3)
    f64 = H.rot6d_to_rotmat(pose.reshape(24, 6))
    worst = 0.0
    for eng, cfg in _each_config(m):
        for B in (1, 3):
            feat, R, K, sc, ce, iw, ih = _head_inputs(B)
            # head_final as its own kernel (hmr_head) and, with head_fuse bit 1, inside the SMPL pose kernel (hmr_regress)
            for out in (eng.hmr_head(feat, R, K, ih), eng.hmr_regress(feat, R, K, sc, ce, iw, ih)):
                p6, sh, cam, rot = (_f32(out[k]) for k in ('pred_pose_6d', 'pred_shape', 'pred_cam', 'pred_pose'))
                assert np.array_equal(p6.view(np.uint32), np.broadcast_to(pose, (B, 144)).view(np.uint32)), cfg
                assert np.array_equal(sh.view(np.uint32), np.broadcast_to(H.INIT_SHAPE, (B, 10)).view(np.uint32)), cfg
                assert np.array_equal(cam.view(np.uint32), np.broadcast_to(H.INIT_CAM, (B, 3)).view(np.uint32)), cfg
                for b in range(B):
                    for j, name in enumerate(names):
                        assert np.array_equal(H.bits(rot[b, j]), H.bits(want[j])), (cfg, B, b, name, rot[b, j], want[j])
                        assert np.array_equal(H.bits(rot[b, j]), H.bits(o32[j])), (cfg, B, b, name, 'fp32 oracle')
                worst = max(worst, float((np.abs(rot[:, n:].astype(np.float64) - f64[None, n:]) / H.ulp32(f64[None, n:])).max()))
    return worst


def test_rot6d_edges_through_a_zero_weight_model():
    """head_final_kernel and its copy in the SMPL pose kernel (head_fuse bit 1), B in {1, 3}, both plans, composed map and loop.
    With every head weight zero the regressed state is the init vectors bit for bit (0 * x + bias in the GEMV, 0 + 0 + init in the
    loop's residual epilogue); the dyadic joints are add, multiply, sqrt and divide on exactly representable values, so they equal
    the closed form and the fp32 oracle in every bit; the random joints are held to 4 ulp of float64 per element (every entry at
    least 0.2; the oracle itself is within 2, tests/test_head_ref_host.py)."""
    worst = rot6d_report()
    print(f'rot6d random joints: worst {worst:.2f} ulp of float64')
    assert worst <= 4.0, worst


def activation_report(kind):
    """-> {activation: worst |gpu - f64| / budget over both variance outputs}, after asserting kinds and the exact parts."""
    import torch.nn.functional as TF
    from spec_amd.modules import UNCERTAINTY_ACTIVATIONS
    m = _hmr(kind)
    eng = m.engine(torch.device(DEV))
    x = np.concatenate(H.var_biases())
    pose, _, _ = H.rot6d_cases()
    report = {}
    try:
        for act in H.ACTIVATIONS:
            eng.set_option('uncertainty_activation', UNCERTAINTY_ACTIVATIONS[act])
            f64 = H.uncertainty_act(x, act)
            o32 = (getattr(TF, act)(t(x)) if act else t(x)).numpy()
            tol = H.budget(f64, o32)
            fin = np.isfinite(f64)
            # every path once for softplus (its threshold is the mutation-prone constant), one path for the others
            configs = _each_config(m, fuses=(3,)) if act == 'softplus' else [(eng, ('auto', 1, 3))]
            for _, cfg in configs:
                for B in ((3, 12) if act == 'softplus' else (3,)):
                    feat, R, K, _, _, _, ih = _head_inputs(B)
                    out = eng.hmr_head(feat, R, K, ih)
                    pv, sv = (_f32(a) for a in eng.hmr_uncertainty(B))
                    assert np.array_equal(pv[:, :144].view(np.uint32), _f32(out['pred_pose_6d']).view(np.uint32)), (act, cfg)
                    assert np.array_equal(pv[:, :144].view(np.uint32), np.broadcast_to(pose, (B, 144)).view(np.uint32)), (act, cfg)
                    assert np.array_equal(sv[:, :10].view(np.uint32), np.broadcast_to(H.INIT_SHAPE, (B, 10)).view(np.uint32)), (act, cfg)
                    got = np.concatenate([pv[:, 144:], sv[:, 10:]], 1)
                    for b in range(B):
                        assert H.same_kind(got[b], f64), (act, cfg, b, got[b][~fin], f64[~fin])
                        err = np.abs(got[b, fin].astype(np.float64) - f64[fin])
                        if act in ('', 'relu'):
                            assert np.all(err == 0), (act, cfg, b)
                        ratio = float((err / tol[fin]).max())
                        report[act] = max(report.get(act, 0.0), ratio)
                        assert ratio <= 1.0, (act, cfg, b, x[fin][np.argmax(err / tol[fin])], ratio)
    finally:
        eng.set_option('uncertainty_activation', 0)
    return report


@pytest.mark.parametrize('kind', ['var', 'var_separate'])
def test_uncertainty_activations_on_their_edges(kind):
    """head_var_kernel: the variance decoders of a zero-weight model return their biases - -inf, -104, -88, -20, -1e-8, -0, 0, 1e-8,
    the softplus threshold 20 and its two neighbours, 88.8, 104, +inf, NaN, 12 and 13.5 (the last inputs at which fp32 softplus(x)
    is not x itself), then Gaussians - and every activation is compared per
    element: same kind where not finite, ReLU and the identity exact, the rest within 2 |fp32 torch - f64| + 4 ulp32(f64)
    (2^-126 where the result is subnormal).  Both parameter layouts; softplus on every head path and at B = 12."""
    report = activation_report(kind)
    print(kind, 'worst |gpu - f64| / budget per activation:', {k: round(v, 3) for k, v in report.items()})


def head_init_report():
    """-> worst |vfov slot - float64| in ulp, after asserting the exact slots."""
    m = _hmr('selector')
    B = 4
    feat, R, K, _, _, _, ih = _head_inputs(B)
    row = H.head_state_row(np.zeros(144), np.zeros(10), H.INIT_CAM, _f32(R), _f32(K), _f32(ih))
    want = 3 * row[:, 157:164]
    worst = 0.0
    for eng, cfg in _each_config(m):
        sh = _f32(eng.hmr_head(feat, R, K, ih)['pred_shape']).astype(np.float64)
        assert np.array_equal(sh[:, :6], want[:, :6]), (cfg, sh[:, :6], want[:, :6])
        assert np.all(sh[:, 7:] == 0), cfg
        worst = max(worst, float((np.abs(sh[:, 6] - want[:, 6]) / H.ulp32(want[:, 6])).max()))
    return worst


def test_head_init_through_a_selector_model():
    """head_init_kernel and its copy in the pooling launch (head_fuse bit 0): the selector model returns pred_shape[:, i] =
    3 R[i // 2, i % 2] for i < 6 - nine distinct dyadic entries per image, so a transposed or mis-strided read of R is an inequality
    of bits - and 3 * vfov in slot 6, within 4 ulp of float64 for K00 in {300, 5000} x img_h in {1, 480}."""
    worst = head_init_report()
    print(f'vfov slot: worst {worst:.2f} ulp of float64')
    assert worst <= 4.0, worst


# =================================================================================================================================
# CamCalib decode, bins, cam_params
# =================================================================================================================================

def _norm_ratio(gpu, f64, ref32, rows):
    """|gpu - f64| over ``rows`` in the max-norm, as a fraction of 2 max |oracle32 - f64| + 4 ulp32(max |f64|) over the same rows."""
    g, f, r = (np.asarray(a, np.float64)[list(rows)] for a in (gpu, f64, ref32))
    return float(np.abs(g - f).max() / H.norm_budget(f, r))


def decode_report(eng, nbins):
    from oracle.models import cam_params, decode_angles, focal_from_vfov
    x, ih, iw = H.decode_rows(nbins)
    out = eng.camcalib_decode(_dev(x[0]), _dev(x[1]), _dev(x[2]), _dev(ih), _dev(iw))
    ang = [_f32(out[k]) for k in ('vfov', 'pitch', 'roll')]
    f_pix, R, K = _f32(out['f_pix']), _f32(out['cam_rotmat']), _f32(out['cam_intrinsics'])
    o32 = [a.numpy() for a in decode_angles(t(x[0]), t(x[1]), t(x[2]))]
    f64 = H.decode(x[0], x[1], x[2])
    report = {}
    for h, name in enumerate(('vfov', 'pitch', 'roll')):
        assert np.array_equal(np.flatnonzero(np.isnan(ang[h])), H.NAN_ROWS), (nbins, name, ang[h])
        for r, k in zip(H.ONE_HOT_ROWS, H.one_hot_bins(nbins)):
            want = H.decode_f32_onehot(k, nbins, h)
            assert ang[h][r] == want and ang[h][r] == o32[h][r], (nbins, name, 'bin', k, ang[h][r], want, o32[h][r])
        assert np.isfinite(ang[h][H.BIG_ROW]) and ang[h][H.BIG_ROW] == o32[h][H.BIG_ROW] == ang[h][2], (nbins, name, ang[h][H.BIG_ROW])
        report[name] = max(_norm_ratio(ang[h], f64[h], o32[h], H.ORDINARY_ROWS), _norm_ratio(ang[h], f64[h], o32[h], [H.BIG_ROW]))
    nan = list(H.NAN_ROWS)
    fin = list(H.ORDINARY_ROWS) + [H.BIG_ROW]
    # K: the third row zero, the principal point exact, both focal entries the f_pix output (NaN rows included: same bits)
    assert np.all(K[:, 2, :] == 0) and np.all(K[:, 0, 1] == 0) and np.all(K[:, 1, 0] == 0), nbins
    assert np.array_equal(K[:, 0, 2], iw / 2) and np.array_equal(K[:, 1, 2], ih / 2), nbins
    assert np.array_equal(K[:, 0, 0].view(np.uint32), f_pix.view(np.uint32)) and np.array_equal(K[:, 1, 1].view(np.uint32), f_pix.view(np.uint32))
    assert np.isnan(f_pix[nan]).all() and np.isnan(R[nan]).all() and np.isfinite(f_pix[fin]).all() and np.isfinite(R[fin]).all(), nbins
    if nbins % 2:      # pitch = roll = 0 at the middle bin of an odd count: the identity, bit for bit
        assert ang[1][1] == 0 and ang[2][1] == 0 and np.array_equal(H.bits(R[1]), H.bits(np.eye(3))), (nbins, R[1])
    # f_pix / img_h (so that the 4000-pixel rows cannot hide the 1-pixel ones) and R, from the logits in float64 all the way
    f32 = focal_from_vfov(o32[0], ih)
    R32 = cam_params(o32[1], o32[2], f32, iw, ih)[0].numpy()
    f64f = H.focal(f64[0], ih)
    R64 = H.cam_RK(f64[1], f64[2], f64f, iw, ih)[0]
    for rows, tag in ((H.ORDINARY_ROWS, ''), ([H.BIG_ROW], '_1e4')):
        report['f_pix' + tag] = _norm_ratio(f_pix / ih, f64f / ih, f32 / ih, rows)
        report['R' + tag] = _norm_ratio(R, R64, R32, rows)
    # camcalib_bins on the same rows: np.argmax exactly (ties: the first index; NaN rows: the first NaN), and the decode's soft index
    idx, soft = eng.camcalib_bins(_dev(x), argmax=True, soft=True)
    idx, soft = idx.cpu().numpy(), _f32(soft)
    assert np.array_equal(idx, np.stack([H.bins_argmax(x[h]) for h in range(3)])), (nbins, idx)
    for h in range(3):
        span, lo = H._range(h)
        angle = span * ((soft[h] + np.float32(1)) / np.float32(2)) + lo            # soft_idx_to_angle in fp32, nothing fused
        assert np.array_equal(angle[fin], ang[h][fin]) and np.isnan(soft[h][nan]).all(), (nbins, h, angle, ang[h])
    return report


@pytest.mark.parametrize('nbins', H.NBINS)
def test_camcalib_decode_edges(eng, nbins):
    """camcalib_decode_kernel (its own copy of the softmax) and bins_reduce_kernel at 2 ... 257 bins - below one wave, one short of
    it, exactly it, one past it, four trips and one past four - and image sizes (1, 1), (480, 640), (4000, 6000)."""
    report = decode_report(eng, nbins)
    print(nbins, 'worst |gpu - f64| / (2 max |oracle32 - f64| + 4 ulp):', {k: round(v, 3) for k, v in report.items()})
    for k, v in report.items():
        assert v <= 1.0, (nbins, k, v)


def cam_params_report(eng, B):
    from oracle.models import cam_params
    lib, h = eng.lib, eng.h
    ins = H.cam_params_inputs(B)
    d = [_dev(a) for a in ins]
    R32, K32 = (a.numpy() for a in cam_params(*ins))
    R64, K64 = H.cam_RK(*ins)
    bufs = {}
    for which in ('both', 'R', 'K'):
        Rb, Kb = _sentinels(9 * B + 64), _sentinels(9 * B + 64)
        rc = lib.specmi_cam_params(h, *(_p(a) for a in d), B, _p(Rb) if which != 'K' else None, _p(Kb) if which != 'R' else None, None)
        assert rc == _lib.OK, (lib.specmi_last_error(h) or b'').decode()
        torch.cuda.synchronize()
        bufs[which] = (Rb.cpu().numpy(), Kb.cpu().numpy())
        for buf, used in zip(bufs[which], (which != 'K', which != 'R')):
            assert np.all(buf[9 * B:] == SENTINEL), (B, which, 'wrote past the outputs')
            assert used or np.all(buf == SENTINEL), (B, which, 'wrote a null output')
    R = bufs['both'][0][:9 * B].view(np.float32).reshape(B, 3, 3)
    K = bufs['both'][1][:9 * B].view(np.float32).reshape(B, 3, 3)
    assert np.array_equal(bufs['R'][0], bufs['both'][0]) and np.array_equal(bufs['K'][1], bufs['both'][1]), B
    assert np.array_equal(K.astype(np.float64), K64) and np.array_equal(K, K32), B          # f, w / 2, h / 2 and zeros: exact
    assert np.array_equal(H.bits(R[0]), H.bits(np.eye(3))), (B, R[0])                      # pitch = roll = 0
    return _norm_ratio(R, R64, R32, range(B))


@pytest.mark.parametrize('B', H.CAM_PARAMS_B)
def test_cam_params_edges(eng, B):
    """cam_params_kernel with B below, at and past its 64-thread block: image 0 has pitch = roll = 0 (the identity, exactly), image
    B - 1 is unlike the rest, R and K are each null in turn, K is exact, R follows the 2 x oracle + 4 ulp rule in the max-norm."""
    ratio = cam_params_report(eng, B)
    print(f'B={B}: |R - f64| / (2 max |oracle32 - f64| + 4 ulp) = {ratio:.3f}')
    assert ratio <= 1.0, (B, ratio)
