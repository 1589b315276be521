"""CPU checks of tests/conv_f32_ref.py: the float64 reference the fp32 convolution kernels are compared with bit for bit
(tests/test_gpu_conv_f32_exact.py), its operands and the condition under which fp32 arithmetic on them is exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_f32_ref as R

CASES = R.all_cases()


@pytest.fixture(scope='module')
def refs():
    """(operands, reference) of every case, computed once."""
    out = {}
    for c in CASES:
        o = R.integer_operands(c)
        out[R.case_id(c)] = (o, R.layer_reference(o, c['stride'], c['pad'], c['relu'], c['ds'][3] if c['ds'] else 1))
    return out


def test_case_list_is_deterministic_and_spans_the_shapes():
    again = R.all_cases()
    assert [R.case_id(c) for c in again] == [R.case_id(c) for c in CASES] and again == CASES
    assert len(set(R.case_id(c) for c in CASES)) == len(CASES) and len(R.shape_cases()) == 40
    for c in CASES:
        a, b = R.integer_operands(c), R.integer_operands(c)
        assert all(np.array_equal(a[k], b[k]) if a[k] is not None else b[k] is None for k in a)
    sc = R.shape_cases()
    assert {(c['k'], c['stride']) for c in sc} == {(1, 1), (1, 2), (3, 1), (3, 2)}
    assert {c['res'] for c in sc} == {False, True} and {c['relu'] for c in sc} == {False, True}
    assert all(1 <= c['B'] <= 5 and 1 <= c['H'] <= 23 and 1 <= c['W'] <= 23 for c in CASES)
    assert all(c['cin'] in R.CINS_WINO and c['cout'] in R.COUTS for c in sc)
    assert any(c['wino'] for c in sc) and any(c['wino'] and c['cin'] in (16, 48) for c in CASES)


@pytest.mark.parametrize('c', CASES, ids=R.case_id)
def test_every_case_passes_the_exactness_condition(c, refs):
    o, ref = refs[R.case_id(c)]
    assert R.assert_exact_in_fp32(c, o) < 1.0
    # what the condition promises: the reference itself is a fp32 number, element by element
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    if c['wino']:
        assert np.all(o['w'] % 4 == 0)


@pytest.mark.parametrize('c', CASES, ids=R.case_id)
def test_reference_equals_torch_float64(c, refs):
    o, ref = refs[R.case_id(c)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    y = F.conv2d(t(o['x']).permute(0, 3, 1, 2), t(o['w']), stride=c['stride'], padding=c['pad'])
    if c['ds']:
        s2 = c['ds'][3]
        x2 = t(o['x2']).permute(0, 3, 1, 2)[:, :, ::s2, ::s2][:, :, :y.shape[2], :y.shape[3]]
        y = y + F.conv2d(x2, t(o['w2']))
    y = (y * t(o['scale']).view(1, -1, 1, 1) + t(o['shift']).view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    if c['res']:
        y = y + t(o['res'])
    if c['relu']:
        y = F.relu(y)
    assert y.dtype == torch.float64 and np.array_equal(y.numpy(), ref)


def test_hand_worked_1x1():
    """Two pixels, two input channels, two outputs: y[p][n] = relu((x[p] . w[n]) * scale[n] + shift[n] + res[p][n])."""
    o = dict(x=np.array([[[[1.0, 2.0], [3.0, -4.0]]]]), w=np.array([[5.0, 6.0], [-7.0, 8.0]]).reshape(2, 2, 1, 1),
             scale=np.array([0.5, 2.0]), shift=np.array([0.25, -1.0]), res=np.array([[[[1.0, -100.0], [0.0, 0.0]]]]), x2=None, w2=None)
    # pixel 0: (5 + 12, -7 + 16) = (17, 9) -> (8.5 + 0.25 + 1, 18 - 1 - 100) = (9.75, -83);  pixel 1: (15 - 24, -21 - 32) = (-9, -53)
    # -> (-4.5 + 0.25, -106 - 1) = (-4.25, -107)
    assert np.array_equal(R.layer_reference(o, 1, 0, False), np.array([[[[9.75, -83.0], [-4.25, -107.0]]]]))
    assert np.array_equal(R.layer_reference(o, 1, 0, True), np.array([[[[9.75, 0.0], [0.0, 0.0]]]]))
    # the second source: x2 (1,3,3,1) sampled at stride 2 -> its corners; one output row of two pixels reads (0,0) and (0,2)
    o2 = dict(o, res=None, x2=np.arange(9.0).reshape(1, 3, 3, 1), w2=np.array([10.0, -1.0]).reshape(2, 1, 1, 1))
    # pixel 0 reads x2 = 0, pixel 1 reads x2 = 2: sums (17, 9) and (-9 + 20, -53 - 2) = (11, -55) -> (8.75, 17), (5.75, -111)
    assert np.array_equal(R.layer_reference(o2, 1, 0, False, stride2=2), np.array([[[[8.75, 17.0], [5.75, -111.0]]]]))


def test_hand_worked_3x3():
    """One channel, a 3x3 image of 1..9, the filter that is 1 at the centre, 2 to the right and 3 below: stride 1 / pad 1 gives
    y[r][c] = x[r][c] + 2 x[r][c+1] + 3 x[r+1][c] with zeros outside; stride 2 keeps its corners."""
    x = np.arange(1.0, 10.0).reshape(1, 3, 3, 1)
    w = np.zeros((1, 1, 3, 3))
    w[0, 0, 1, 1], w[0, 0, 1, 2], w[0, 0, 2, 1] = 1.0, 2.0, 3.0
    o = dict(x=x, w=w, scale=np.array([1.0]), shift=np.array([0.0]), res=None, x2=None, w2=None)
    want = np.array([[1 + 4 + 12, 2 + 6 + 15, 3 + 0 + 18], [4 + 10 + 21, 5 + 12 + 24, 6 + 0 + 27], [7 + 16, 8 + 18, 9.0]])
    assert np.array_equal(R.layer_reference(o, 1, 1, False)[0, :, :, 0], want)
    assert np.array_equal(R.layer_reference(o, 2, 1, False)[0, :, :, 0], want[::2, ::2])
    o['scale'], o['shift'] = np.array([0.25]), np.array([-6.0])
    assert np.array_equal(R.layer_reference(o, 1, 1, True)[0, :, :, 0], np.maximum(want * 0.25 - 6.0, 0.0))


WINO = [c for c in CASES if c['wino']]


@pytest.mark.parametrize('c', WINO, ids=R.case_id)
def test_winograd_in_float32_reproduces_the_direct_sum(c, refs):
    """F(2x2,3x3) with explicit G, B, A and every step in float32, on the Winograd operands: bit for bit the float64 direct
    convolution.  The exactness claim holds for the algorithm, whatever a kernel does."""
    o, _ = refs[R.case_id(c)]
    y = R.winograd_f32(o['x'], o['w'])
    assert y.dtype == np.float32
    want = R.nhwc(R.conv64(R.nchw(o['x']), o['w'], 1, 1))
    assert np.array_equal(y.astype(np.float64), want)


def test_winograd_in_float32_is_not_exact_without_the_condition():
    """The same restatement with weights that are not multiples of 4 leaves the integers (G g G^T has quarters) - the reason
    the condition asks for them - and with large operands it rounds: the check above can fail, it is not an identity."""
    rng = np.random.default_rng(5)
    x = rng.integers(-2000, 2001, (1, 6, 6, 512)).astype(np.float64)
    w = rng.integers(-2000, 2001, (64, 512, 3, 3)).astype(np.float64) * 4.0
    assert not np.array_equal(R.winograd_f32(x, w).astype(np.float64), R.nhwc(R.conv64(R.nchw(x), w, 1, 1)))
    U = R.wino_weights(np.ones((1, 1, 3, 3)))
    assert not np.all(U == np.round(U))


def test_condition_refuses_what_breaks_it():
    assert len(WINO) >= 8
    # 1. a K long enough for sum |x| |w| to pass 2^24: Cin = 2^17 channels of |x| = 255, |w| = 255 -> 8.5e9
    c = R.case(1, 1, 1, 2 ** 17, 1, 1, 1, 0, seed=1)
    o = R.integer_operands(c)
    o['x'][:], o['w'][:] = 255.0, 255.0
    with pytest.raises(AssertionError, match='2\\^24'):
        R.assert_exact_in_fp32(c, o)
    # ... and with the case's own small operands the same K is fine: 2^17 * 4 * 8 = 2^22
    assert R.assert_exact_in_fp32(c, R.integer_operands(c)) < 1.0
    # 2. a Winograd case with one weight that is not a multiple of 4
    c = next(c for c in R.NAMED_CASES if c['wino'])
    o = R.integer_operands(c)
    R.assert_exact_in_fp32(c, o)
    o['w'][0, 0, 1, 1] = 6.0
    with pytest.raises(AssertionError, match='multiples of 4'):
        R.assert_exact_in_fp32(c, o)
    # 3. the transformed-domain bound: integers that pass the direct bound for most outputs but 81 Cin max|x| max|w| >= 2^24
    o = R.integer_operands(c)
    o['x'][0, 0, 0, 0], o['w'][0, 0, 0, 0] = 250.0, 252.0         # 81 * 64 * 250 * 252 = 3.3e8
    with pytest.raises(AssertionError, match='Winograd bound'):
        R.assert_exact_in_fp32(c, o)
    # 4. a shift that is not a multiple of 0.25, a scale that is not one of the four, an operand that is not an integer
    for k, v, msg in (('shift', 0.125, 'shift'), ('scale', 3.0, 'scale'), ('x', 0.5, 'integers')):
        o = R.integer_operands(c)
        o[k].flat[0] = v
        with pytest.raises(AssertionError, match=msg):
            R.assert_exact_in_fp32(c, o)


def test_mismatch_helper_names_the_first_element():
    ref = np.arange(24.0).reshape(1, 2, 3, 4)
    R._assert_bit_exact(ref.astype(np.float32), ref)
    y = ref.astype(np.float32)
    y[0, 1, 0, 2] += np.float32(2.0 ** -19)                 # one unit in the last place of 14
    y[0, 1, 2, 3] = np.nan
    with pytest.raises(AssertionError, match=r'2 of 24 differ, first at \(b=0, oy=1, ox=0, n=2\): got 14.00000190\d+, want 14.0'):
        R._assert_bit_exact(y, ref, 'x')


def test_kernel_name_restatement():
    c = R.case(1, 8, 8, 64, 128, 3, 1, 1)
    assert R.direct_kernel(c, 0) == 'conv_igemm_f32<64x64,2x2>' and R.direct_kernel(c, 1) == 'conv_igemm_f32<128x128,2x2>'
    assert R.direct_kernel(R.case(1, 8, 8, 64, 32, 3, 1, 1), 0) == 'conv_igemm_f32<128x32,4x1>'
    assert R.direct_kernel(R.case(1, 8, 8, 64, 33, 3, 1, 1), 1) is None and R.direct_kernel(R.case(1, 8, 8, 48, 64, 3, 1, 1), 3) is None
    assert R.wino_kernel(c, 16) == 'conv_wino_f32<32t x128,F(2x2,3x3)>' and R.wino_kernel(c, 0) == 'conv_wino_f32<32t x64,F(2x2,3x3)>'
    assert R.k_chunks(R.SLICED_CASES[0]) == 18 and all(R.k_chunks(s) == 18 for s in R.SLICED_CASES)


def test_engine_reads_the_pixel_stride_of_channel_sliced_views():
    """Engine.conv2d passes x, x2, out and residual as views: unit channel stride, one pixel stride ld >= C; anything else is
    not a layout specmi_conv2d_strided can express (inputs are then copied dense, an ``out`` is refused)."""
    from spec_amd.engine import Engine
    ld = Engine._pixel_rows
    wide = torch.zeros(2, 3, 5, 64)
    assert ld(wide) == 64 and ld(wide[..., 16:48]) == 64 and ld(wide[..., :1]) == 64
    assert ld(wide[:, :, :, ::2]) is None and ld(wide.permute(0, 2, 1, 3)) is None and ld(wide[:, :, 1:4]) is None
    assert ld(wide[:, 1:2, :, :32]) is None                                    # images no longer H * W * ld apart
    assert ld(torch.zeros(1, 1, 1, 7)) == 7 and ld(torch.zeros(3, 1, 1, 64)[..., :32]) == 64 and ld(torch.zeros(1, 4, 1, 64)[..., 8:40]) == 64
    flat = torch.zeros(1000)
    assert ld(flat.as_strided((2, 2, 3, 17), (2 * 3 * 21, 3 * 21, 21, 1), 5)) == 21     # ld % 4 != 0, one float past alignment
    assert ld(flat.as_strided((1, 2, 2, 64), (4 * 32, 2 * 32, 32, 1))) is None            # pixels closer than their channels
