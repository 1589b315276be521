"""The integer cases of tests/test_gpu_fp16_shapes.py are themselves tested here, without a GPU: every case is exact under any
accumulation order (so a device mismatch can only be the kernel's fault), passes the launcher's shape check (so none is silently
refused), and the list as a whole reaches every kernel instance and every tail.  Also the float32-accumulation switch of the
reference trunk."""
import numpy as np
import pytest
import torch

from tests import fp16_ref
from tests.fp16_ref import conv_out

torch.set_grad_enabled(False)
CASES = fp16_ref.shape_cases()


def test_case_list_size_and_ranges():
    assert len(CASES) >= 60
    two = [c for c in CASES if c['ds']]
    assert len(CASES) // 5 <= len(two) <= len(CASES) // 3
    for c in CASES:
        assert 1 <= c['B'] <= 7 and 1 <= c['H'] <= 40 and 1 <= c['W'] <= 40 and c['cout'] in fp16_ref.COUTS
        assert c['k'] in (1, 3, 5, 7) and c['stride'] in (1, 2, 3) and 0 <= c['pad'] <= c['k'] - 1
        assert c['cin'] in (fp16_ref.CINS_2SRC if c['ds'] else fp16_ref.CINS)
    assert fp16_ref.shape_cases() == CASES                                       # seeded: the same list every time
    assert {c['B'] for c in CASES} == set(range(1, 8))
    for key, want in (('k', {1, 3, 5, 7}), ('stride', {1, 2, 3}), ('res', {False, True}), ('relu', {False, True}), ('out32', {False, True})):
        assert {c[key] for c in CASES if not c['ds']} == want, key
    assert {c['cin'] for c in CASES if not c['ds']} == set(fp16_ref.CINS) and {c['cout'] for c in CASES} == set(fp16_ref.COUTS)


def test_two_source_cases_cover_both_sizes_and_strides():
    two = [c for c in CASES if c['ds']]
    assert all(c['cin'] % 32 == 0 and c['ds'][0] % 32 == 0 and c['ds'][3] in (1, 2) and not c['out32'] for c in two)
    assert {c['ds'][3] for c in two} == {1, 2} and {c['res'] for c in two} == {False, True}
    extra = {c['ds'][1] - ((c['H'] - 1) * c['ds'][3] + 1) for c in two}
    assert extra == {0, 1}, extra                                                # the exact size and one larger
    assert any(c['ds'][3] == 2 and c['ds'][1] == 2 * c['H'] for c in two) and any(c['ds'][3] == 2 and c['ds'][1] == 2 * c['H'] - 1 for c in two)
    xb = lambda c: c['H'] * c['W'] * c['cin']
    x2b = lambda c: c['ds'][1] * c['ds'][2] * c['ds'][0]
    assert any(x2b(c) > xb(c) for c in two) and any(x2b(c) < xb(c) for c in two)


@pytest.mark.parametrize('c', CASES, ids=fp16_ref.case_id)
def test_integer_case_is_exact_and_accepted(c):
    o = fp16_ref.integer_operands(c)
    # multiples of 0.5 below 2^23 in magnitude are exact in fp32, and so is every partial sum: the order cannot matter.  (The
    # bound asked for is 2^24 on integers; the scale 0.5 halves the unit, so the bar here is 2^23.)
    assert fp16_ref.exactness_bound(c, o) < 2.0 ** 23
    for a in (o['x'], o['x2'], o['res'], o['w'], o['w2'], o['shift'] * 2, o['scale'] * 2):
        assert a is None or np.array_equal(a, np.round(a))
    ws = o['w'] * o['scale'][:, None, None, None]
    assert np.array_equal(fp16_ref.f16(ws), ws) and np.array_equal(fp16_ref.f16(o['x']), o['x'])
    ref = fp16_ref.layer_reference(o, c['stride'], c['pad'], c['relu'], c['ds'][3] if c['ds'] else 1)
    assert ref.shape == (c['B'], conv_out(c['H'], c['k'], c['stride'], c['pad']), conv_out(c['W'], c['k'], c['stride'], c['pad']), c['cout'])
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    assert np.abs(ref).max() <= fp16_ref.exactness_bound(c, o)
    assert fp16_ref.shape_ok(c), 'the launcher would refuse this case'


def test_case_list_reaches_every_instance_and_tail():
    assert {fp16_ref.instance(c) for c in CASES} == set(fp16_ref.INSTANCE_NAMES)
    M = lambda c: c['B'] * conv_out(c['H'], c['k'], c['stride'], c['pad']) * conv_out(c['W'], c['k'], c['stride'], c['pad'])
    ldx = lambda c: -(-c['cin'] // 8) * 8
    single = [c for c in CASES if not c['ds']]
    assert any(M(c) % 128 for c in CASES) and any(M(c) > 128 and M(c) % 128 for c in CASES)
    assert any((c['k'] ** 2 * ldx(c)) % 32 for c in single)                                        # Kp != K: padding octets
    assert any(c['cout'] % 64 for c in CASES) and any(c['cout'] % 64 and fp16_ref.instance(c)[0] for c in CASES)
    assert any(c['cin'] % 8 and c['k'] > 1 for c in single)
    assert any(c['stride'] == 3 for c in single) and any(c['pad'] > c['k'] // 2 for c in single)
    assert any(c['H'] < c['k'] for c in single) and any(c['W'] < c['k'] for c in single)
    assert any(M(c) % 128 and c['stride'] == 3 for c in single) and any(M(c) % 128 and c['pad'] > c['k'] // 2 for c in single)


def test_shape_ok_restatement_refuses_what_the_launcher_refuses():
    ok = dict(B=1, H=8, W=8, cin=32, cout=64, k=1, stride=1, pad=0, res=False, relu=True, out32=False, ds=(32, 15, 15, 2))
    assert fp16_ref.shape_ok(ok)
    for bad in (dict(cout=6), dict(out32=True), dict(cin=16), dict(ds=(32, 14, 15, 2)), dict(ds=(48, 15, 15, 2)), dict(k=3, pad=1)):
        assert not fp16_ref.shape_ok(dict(ok, **bad)), bad
    assert not fp16_ref.shape_ok(dict(ok, ds=None, H=2, k=3))                      # empty output


def test_directed_tie_sums_are_what_they_claim():
    x, sums, want = fp16_ref.tie_case()
    assert np.array_equal(x.sum(-1).ravel(), sums) and np.array_equal(fp16_ref.f16(x), x)
    assert np.array_equal(fp16_ref.f16(sums), want)
    for s, w in zip(sums, want):                                                 # each sum is the midpoint of two fp16 neighbours
        lo, hi = np.float16(w), np.nextafter(np.float16(w), np.float16(np.inf if s > w else -np.inf))
        assert abs(float(hi) - s) == abs(float(lo) - s) and int(lo.view(np.uint16)) % 2 == 0


@pytest.mark.parametrize('c', fp16_ref.SPLIT_CASES, ids=lambda c: c['side'])
def test_split_case_is_exact_accepted_and_crosses_the_line(c):
    assert fp16_ref.shape_ok(c)
    OH, OW = conv_out(c['H'], c['k'], c['stride'], c['pad']), conv_out(c['W'], c['k'], c['stride'], c['pad'])
    size = {'x': c['B'] * c['H'] * c['W'] * c['cin'] * 2, 'x2': c['B'] * c['ds'][1] * c['ds'][2] * c['ds'][0] * 2 if c['ds'] else 0,
            'out': c['B'] * OH * OW * c['cout'] * (4 if c['out32'] else 2)}
    assert size[c['side']] > 2 ** 31 and all(v < 2 ** 30 for k, v in size.items() if k != c['side'])
    per, probes = fp16_ref.split_images_per_launch(c), fp16_ref.split_probe_images(c)
    assert (per < c['B']) == (c['side'] != 'out')
    assert 0 in probes and c['B'] - 1 in probes and all(0 <= b < c['B'] for b in probes) and len(probes) <= 8
    if c['side'] == 'x':
        assert per == 127 and {126, 127} <= set(probes)
    if c['side'] == 'x2':                                  # per comes from x2: the x image alone would allow the whole batch
        assert per == 127 and {126, 127, 253, 254} <= set(probes) and (2 ** 31 - 1) // (c['H'] * c['W'] * c['cin'] * 2) > c['B']
    if c['side'] == 'out':
        assert {166, 167, 168} <= set(probes)
    o = fp16_ref.split_operands(c, 2, 'cpu')
    K = c['cin'] * c['k'] ** 2 + (c['ds'][0] if c['ds'] else 0)
    assert K * fp16_ref.X_MAX * fp16_ref.W_MAX * max(fp16_ref.SCALES) + fp16_ref.SHIFT_MAX + fp16_ref.X_MAX < 2.0 ** 23
    assert float(o['x'].abs().max()) <= fp16_ref.X_MAX and np.abs(o['w']).max() <= fp16_ref.W_MAX and np.abs(o['shift']).max() <= fp16_ref.SHIFT_MAX
    assert not o['x'][..., c['cin']:].any()
    with torch.inference_mode():
        ref = fp16_ref.split_reference(c, o, [0, 1])
    assert ref.shape == (2, OH, OW, c['cout']) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)


def test_float32_accumulation_switch_of_the_reference_trunk():
    """acc='float32' changes only the accumulation: its distance from the float64 walk is the rounding-flip floor - not zero
    (float32 sums round, and now and then that moves an fp16 store to the neighbouring value), fp16-class at its largest (the
    bar of test_fp16_reference_differs_from_fp64_by_an_fp16_class_amount) and, unlike that one, rare: tiny on average."""
    from spec_amd import synth
    for backbone, depth in (('resnet18', 18), ('resnet50', 50)):
        sd, _ = synth.resnet_family_state(1001, backbone, 'backbone.')
        x = synth.images(5, 1)[:, :, :64, :64].astype(np.float64)
        with torch.inference_mode():
            a = fp16_ref.trunk(sd, x, depth=depth)
            b = fp16_ref.trunk(sd, x, depth=depth, acc='float32')
            c = fp16_ref.trunk_fp64(sd, x, depth=depth)
        assert a.shape == b.shape
        d32 = float(np.abs(a - b).max() / np.abs(a).max())
        d16 = float(np.abs(a - c).max() / np.abs(c).max())
        print('depth', depth, 'float64 walk vs float32 walk', d32, '| fp16 walk vs unrounded', d16)
        assert 0 < d32 < 2e-2, (depth, d32, d16)
        assert float(np.abs(a - b).mean() / np.abs(a).max()) < 1e-4
