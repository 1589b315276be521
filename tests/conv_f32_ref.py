"""Test-side reference of one fused fp32 layer (conv_igemm.hip, conv_wsplit.hip, conv_wino.hip, conv_bf16s.hip, stem.hip) with
operands for which fp32 arithmetic is exact, so that the device must equal a float64 reference bit for bit - no tolerance.

The fp32 kernels multiply fp32 by fp32 and accumulate in fp32, in an order that differs from kernel to kernel (tile shape,
K slices, Winograd's transformed domain).  With small-integer activations and weights every product and every partial sum,
in any order, is an integer below 2^24 and therefore exact; with scale in {0.25, 0.5, 1, 2} and shift a multiple of 0.25 the
epilogue's fma and the residual add are exact too.  ``assert_exact_in_fp32`` states that condition and checks it on the CPU
from the operands of a case; every GPU case calls it first.

Winograd F(2x2,3x3) computes Y = A^T [sum_ci (G g G^T) .* (B^T d B)] A.  B and A hold only 0 and +-1, so the device adds and
subtracts; G holds halves, so G g G^T (computed in double by the library, then rounded to fp32) is an integer when the weights
are multiples of 4.  |B^T d B| <= 4 max|x|, |G g G^T| <= 2.25 max|w|, and an output adds at most nine sums over Cin: every
intermediate is an integer of magnitude <= 81 Cin max|x| max|w|."""
import numpy as np
import torch
import torch.nn.functional as F

DEV = 'cuda:0'
CINS = (32, 64, 96, 160, 512)
CINS_WINO = CINS + (16, 48)
COUTS = (1, 3, 17, 32, 33, 48, 64, 96, 100, 160, 192, 256)
X_MAX, W_MAX, SCALES, SHIFT_MAX = 4, 8, (0.25, 0.5, 1.0, 2.0), 8.0
MAC_BUDGET = 3e8          # multiply-adds of one case's float64 CPU reference; H and W shrink until a case fits
GEOMS = ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1))      # (k, stride, pad)


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def round_up(n, m):
    return -(-n // m) * m


def wino_shape(c):
    """conv_wino_supported (conv_wino.hip) on a dense case: 3x3 / stride 1 / pad 1, Cin % 16 == 0, Cout % 64 == 0 or
    (Cout % 32 == 0 and Cout > 64)."""
    return (c['k'] == 3 and c['stride'] == 1 and c['pad'] == 1 and c['cin'] % 16 == 0 and not c.get('ds')
            and (c['cout'] % 64 == 0 or (c['cout'] % 32 == 0 and c['cout'] > 64)))


def case(B, H, W, cin, cout, k, stride, pad, res=False, relu=False, ds=None, seed=0, name=None):
    c = dict(B=B, H=H, W=W, cin=cin, cout=cout, k=k, stride=stride, pad=pad, res=res, relu=relu, ds=ds, seed=seed, name=name)
    c['wino'] = wino_shape(c)       # the weights are multiples of 4
    return c


def case_id(c):
    s = 'B%d_%dx%d_c%d_%d_k%d_s%d_p%d' % (c['B'], c['H'], c['W'], c['cin'], c['cout'], c['k'], c['stride'], c['pad'])
    s += ('_res' if c['res'] else '') + ('_relu' if c['relu'] else '')
    s += '_ds%d_%dx%d_s%d' % c['ds'] if c['ds'] else ''
    return (c['name'] + '-' + s) if c.get('name') else s


def shape_cases(n=40, seed=20250311):
    """n seeded layer shapes: B in 1..5, H and W in 1..23, Cin from CINS (CINS_WINO for 3x3 / stride 1), Cout from COUTS, the
    four kernel geometries in turn, residual and ReLU at random.  H and W shrink until the float64 reference fits MAC_BUDGET."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    cases = []
    for i in range(n):
        k, stride, pad = GEOMS[i % 4]
        B, H, W = int(rng.integers(1, 6)), int(rng.integers(1, 24)), int(rng.integers(1, 24))
        cout = pick(COUTS)
        cin = pick(CINS)
        if (k, stride) == (3, 1) and i % 8 == 2:       # every other 3x3 / stride-1 case is one Winograd takes, 16 / 48 included
            cin, cout = pick(CINS_WINO), pick((64, 96, 160, 192, 256))
        res, relu = bool(rng.integers(2)), bool(rng.integers(2))
        while B * conv_out(H, k, stride, pad) * conv_out(W, k, stride, pad) * cout * cin * k * k > MAC_BUDGET:
            H, W = (max(1, H // 2), W) if H >= W else (H, max(1, W // 2))
        cases.append(case(B, H, W, cin, cout, k, stride, pad, res, relu, seed=seed + 1 + i))
    return cases


# the tails, each named for what it is
NAMED_CASES = [
    case(1, 5, 7, 32, 64, 1, 1, 0, seed=11, name='M35_below_every_tile'),
    case(3, 5, 13, 64, 64, 3, 1, 1, res=True, relu=True, seed=12, name='M195_not_a_multiple_of_64_or_128'),
    case(2, 9, 11, 96, 128, 3, 2, 1, relu=True, seed=13, name='M60_stride2_odd'),
    case(2, 7, 5, 64, 17, 1, 1, 0, res=True, seed=14, name='Cout17_epilogue_tail'),
    case(1, 6, 6, 32, 33, 3, 1, 1, relu=True, seed=15, name='Cout33_epilogue_tail_second_tile'),
    case(2, 4, 3, 64, 3, 3, 2, 1, seed=16, name='Cout3_epilogue_tail'),
    case(2, 7, 9, 64, 96, 3, 1, 1, relu=True, seed=17, name='Cout96_half_masked_wino_column'),
    case(1, 5, 6, 48, 160, 3, 1, 1, res=True, seed=18, name='Cout160_half_masked_wino_column'),
    case(3, 9, 7, 32, 128, 3, 1, 1, seed=19, name='60_wino_tiles_not_a_multiple_of_32'),
    case(1, 13, 11, 16, 64, 3, 1, 1, res=True, relu=True, seed=20, name='42_wino_tiles_one_stage'),
    case(1, 1, 1, 64, 64, 3, 1, 1, seed=21, name='single_output_pixel_3x3'),
    case(1, 1, 1, 32, 1, 1, 1, 0, seed=22, name='single_output_pixel_single_channel'),
    case(1, 2, 2, 512, 256, 3, 2, 1, relu=True, seed=23, name='single_output_pixel_K4608'),
    case(1, 1, 23, 160, 100, 1, 2, 0, res=True, seed=24, name='1xN_row'),
]
# K = 18 chunks of 32: 2, 3, 6, 9 and 18 slices all divide it, and slices of 9 or 3 chunks cut through a filter tap (2 chunks)
SLICED_CASES = [
    case(2, 7, 9, 64, 96, 3, 1, 1, res=True, relu=True, seed=31, name='K18_3x3_s1'),
    case(3, 9, 6, 64, 33, 3, 2, 1, seed=32, name='K18_3x3_s2_tail'),
    case(1, 3, 5, 576, 64, 1, 1, 0, relu=True, seed=33, name='K18_1x1'),
    case(2, 4, 5, 64, 128, 1, 1, 0, res=True, ds=(512, 8, 9, 2), seed=34, name='K18_two_sources'),
]


def all_cases():
    return shape_cases() + NAMED_CASES + SLICED_CASES


def integer_operands(c):
    """The operands of a case as float64 arrays: x (B,H,W,cin) NHWC integers in [-4, 4], w OIHW integers in [-8, 8] (multiples
    of 4 where c['wino']), scale from {0.25, 0.5, 1, 2}, shift multiples of 0.25 in [-8, 8], res (B,OH,OW,cout) integers in
    [-4, 4] or None, x2 (B,H2,W2,cin2) and w2 (cout,cin2,1,1) or None."""
    rng = np.random.default_rng(c['seed'])
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
    OH, OW = conv_out(c['H'], c['k'], c['stride'], c['pad']), conv_out(c['W'], c['k'], c['stride'], c['pad'])
    wshape = (c['cout'], c['cin'], c['k'], c['k'])
    o = dict(x=ints(-X_MAX, X_MAX, (c['B'], c['H'], c['W'], c['cin'])),
             w=ints(-W_MAX // 4, W_MAX // 4, wshape) * 4.0 if c['wino'] else ints(-W_MAX, W_MAX, wshape),
             scale=np.asarray(SCALES)[rng.integers(0, len(SCALES), c['cout'])], shift=ints(-4 * SHIFT_MAX, 4 * SHIFT_MAX, c['cout']) * 0.25,
             res=ints(-X_MAX, X_MAX, (c['B'], OH, OW, c['cout'])) if c['res'] else None, x2=None, w2=None)
    if c.get('ds'):
        cin2, H2, W2, _ = c['ds']
        o['x2'], o['w2'] = ints(-X_MAX, X_MAX, (c['B'], H2, W2, cin2)), ints(-W_MAX, W_MAX, (c['cout'], cin2, 1, 1))
    return o


def nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def conv64(x_nchw, w, stride, pad):
    with torch.inference_mode():
        return F.conv2d(torch.from_numpy(x_nchw), torch.from_numpy(w), stride=stride, padding=pad).numpy()


def _acc(o, stride, pad, stride2, absolute=False):
    """float64 NCHW sum over K = [x | x2 sampled at (oy*stride2, ox*stride2)] of x w (or of |x| |w|)."""
    f = np.abs if absolute else (lambda a: a)
    acc = conv64(f(nchw(o['x'])), f(o['w']), stride, pad)
    if o.get('x2') is not None:
        x2 = nchw(o['x2'])[:, :, ::stride2, ::stride2][:, :, :acc.shape[2], :acc.shape[3]]
        acc = acc + conv64(f(np.ascontiguousarray(x2)), f(o['w2']), 1, 0)
    return acc


def layer_reference(o, stride, pad, relu, stride2=1):
    """float64 NHWC reference of one fused layer from operands shaped as integer_operands returns them:
    act(conv(K, w) * scale + shift [+ res]), K = [x | x2 sampled at (oy*stride2, ox*stride2)]."""
    ref = nhwc(_acc(o, stride, pad, stride2)) * o['scale'] + o['shift']
    if o.get('res') is not None:
        ref = ref + o['res']
    return np.maximum(ref, 0.0) if relu else ref


def wino_weights(w):
    """U = G g G^T of OIHW 3x3 weights in float64, (cout, cin, 4, 4): what pack_wino_weights computes before it rounds to fp32."""
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
    return np.einsum('ia,ocab,jb->ocij', G, np.asarray(w, dtype=np.float64), G)


def _quarters(a):
    return bool(np.all(np.asarray(a) * 4.0 == np.round(np.asarray(a) * 4.0)))


def assert_exact_in_fp32(c, o):
    """The condition under which fp32 arithmetic on these operands is exact in any order; AssertionError if it does not hold.
      * x, w, res (x2, w2) are integers of magnitude <= 255 (one bf16 piece holds them: the split-bf16 path is exact too), scale a
        power of two in [0.25, 2], shift a multiple of 2^-2;
      * direct kernels: max over the outputs of sum |x| |w| (a float64 convolution of the absolute values) < 2^24;
      * Winograd cases: G g G^T is an integer and 81 Cin max|x| max|w| < 2^24;
      * the epilogue: every sum * scale, + shift, + res is a multiple of 2^-2 of magnitude <= S scale + |shift| + |res| < 2^22,
        hence a fp32 number.
    Returns the largest of the bounds relative to its limit."""
    stride2 = c['ds'][3] if c.get('ds') else 1
    for k in ('x', 'w', 'res', 'x2', 'w2'):
        if o.get(k) is not None:
            assert np.all(o[k] == np.round(o[k])) and np.abs(o[k]).max() <= 255, f'{k} is not made of integers up to 255'
    assert np.all(np.isin(o['scale'], SCALES)), 'scale outside {0.25, 0.5, 1, 2}'
    assert _quarters(o['shift']), 'shift is not a multiple of 0.25'
    S = nhwc(_acc(o, c['stride'], c['pad'], stride2, absolute=True))
    worst = S.max() / 2.0 ** 24
    assert S.max() < 2.0 ** 24, f'sum |x||w| reaches {S.max():.0f} >= 2^24'
    if c['wino']:
        U = wino_weights(o['w'])
        assert np.all(U == np.round(U)), 'G g G^T is not an integer: a Winograd case needs weights that are multiples of 4'
        tb = 81.0 * c['cin'] * np.abs(o['x']).max() * np.abs(o['w']).max()
        assert tb < 2.0 ** 24, f'Winograd bound 81 Cin max|x| max|w| = {tb:.0f} >= 2^24'
        worst = max(worst, tb / 2.0 ** 24)
    out = S * o['scale'] + np.abs(o['shift']) + (np.abs(o['res']) if o.get('res') is not None else 0.0)
    assert out.max() < 2.0 ** 22, f'|acc scale + shift + res| reaches {out.max():.2f} >= 2^22'
    acc = nhwc(_acc(o, c['stride'], c['pad'], stride2))
    assert _quarters(acc * o['scale']) and _quarters(acc * o['scale'] + o['shift']), 'a scaled sum is not a multiple of 0.25'
    return max(worst, out.max() / 2.0 ** 22)


def _assert_bit_exact(y, ref, what=''):
    """y (B,OH,OW,N) as the device stored it against the float64 reference: equal as numbers (float32 -> float64 is exact; a NaN
    or an infinity never equals the finite reference), or the first mismatching (b, oy, ox, n) with got and want."""
    y = np.asarray(y)
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    bad = ~(y.astype(np.float64) == ref)
    if bad.any():
        b, oy, ox, n = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} differ, first at (b={b}, oy={oy}, ox={ox}, n={n}): '
                             f'got {float(y[b, oy, ox, n])!r}, want {float(ref[b, oy, ox, n])!r}')


# ---- F(2x2,3x3) restated in float32 NumPy (tests/test_conv_f32_ref_host.py) ------------------------------------------------------
def winograd_f32(x, w):
    """3x3 / stride 1 / pad 1 convolution of x (B,H,W,cin) NHWC with w OIHW as Winograd F(2x2,3x3), every step in float32 with
    explicit G, B, A: U = G g G^T (rounded to float32 from float64, as the library packs it), V = B^T d B, M = sum_ci U V,
    Y = A^T M A.  Returns (B,H,W,cout) float32."""
    f32 = np.float32
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=f32)
    At = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=f32)
    U = wino_weights(w).astype(f32)
    Bn, H, W, cin = x.shape
    TH, TW = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((Bn, 2 * TH + 2, 2 * TW + 2, cin), dtype=f32)
    xp[:, 1:H + 1, 1:W + 1] = x.astype(f32)
    y = np.zeros((Bn, 2 * TH, 2 * TW, w.shape[0]), dtype=f32)
    for ty in range(TH):
        for tx in range(TW):
            d = xp[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]                         # (B,4,4,cin)
            V = np.einsum('ia,bapc,jp->bijc', Bt, d, Bt).astype(f32)
            M = np.einsum('bijc,ncij->bijn', V, U)                                   # float32 products, a float32 sum over ci
            assert M.dtype == f32
            y[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = np.einsum('ia,bapn,jp->bijn', At, M, At).astype(f32)
    return y[:, :H, :W]


# ---- the kernel the library runs for a case, restated (conv_igemm.hip pick_variant, conv_wino.hip wino_pick) ----------------------
DIRECT_NAMES = {1: 'conv_igemm_f32<128x128,2x2>', 2: 'conv_igemm_f32<128x64,2x2>', 3: 'conv_igemm_f32<64x64,2x2>',
                4: 'conv_igemm_f32<128x128,4x2>', 13: 'conv_igemm_f32<128x32,4x1>'}


def direct_kernel(c, force):
    """Name the profiler gives the direct kernel under force_conv_variant = force, or None where the shape does not allow it."""
    npad = round_up(c['cout'], 64)
    if c['cin'] % 32 or (c.get('ds') and c['ds'][0] % 32):
        return None
    if c.get('ds'):
        if force == 4:
            return 'conv_igemm_f32<128x128,4x2,2src>' if npad % 128 == 0 else None
        return 'conv_igemm_f32<64x64,2x2,2src>' if force in (0, 3) else None
    if force in (1, 4):
        return DIRECT_NAMES[force] if npad % 128 == 0 else None
    if force == 0:
        return DIRECT_NAMES[13 if c['cout'] <= 32 else 3]      # (the 128x128 rule needs M >= 131072: no case here)
    return DIRECT_NAMES[force]


def wino_kernel(c, force):
    """Name of the Winograd kernel under force_wino_variant = force (0, 8, 16)."""
    if c['res']:
        return 'conv_wino_f32<32t x64,F(2x2,3x3),res>'
    wide = False
    if force == 16:
        wide = c['cout'] % 128 == 0
    elif force == 0 and c['cout'] % 128 == 0 and c['cin'] >= 512:
        tiles = c['B'] * ((c['H'] + 1) // 2) * ((c['W'] + 1) // 2)
        wide = ((tiles + 31) // 32) * (c['cout'] // 128) >= 128
    return 'conv_wino_f32<32t x128,F(2x2,3x3)>' if wide else 'conv_wino_f32<32t x64,F(2x2,3x3)>'


def k_chunks(c):
    return c['k'] ** 2 * (c['cin'] // 32) + (c['ds'][0] // 32 if c.get('ds') else 0)
