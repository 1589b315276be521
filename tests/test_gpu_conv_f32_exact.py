"""The fp32 convolution kernels (conv_igemm.hip with its tile variants and the sliced split-K kernel, conv_wsplit.hip,
conv_wino.hip with both wave layouts and the residual epilogue, the split-bf16 variant, the 7x7 stem) and the average pool
against a float64 reference, BIT FOR BIT, on the MI355X.  The operands (tests/conv_f32_ref.py) are small integers, scales that are
powers of two and shifts that are multiples of 0.25: every product, every partial sum in any order and every epilogue step is
exact in fp32 (assert_exact_in_fp32 checks that on the CPU for every case before it runs), so "the same products in another
order" gives the same bits and anything else - a dropped tap, an edge column that picks up a neighbour's sum, a slab folded
from the wrong slice - does not.  There is no tolerance in this file.

Every case runs on every kernel instance that takes its shape, and the launch profiler must name the intended kernel.  The layer is
also launched as the trunks launch it, through specmi_conv2d_strided: padded channel strides on both sides, the output as a
channel slice of a wider map (HRNet's concat head), output and residual rows that are not 16-byte aligned (the scalar epilogue),
and the second, strided A source of a bottleneck's conv3 - each time into a buffer pre-filled with a sentinel bit pattern that
every float outside the written (pixel, channel < Cout) positions must still hold.

Measured on MI355X: the file (119 tests) takes 3.5 s, the slowest test 0.18 s; 842 MiB of device memory are in use at its peak
(the runtime's own context and the library's workspaces included), 15 MiB of them tensors of these tests."""
import contextlib

import numpy as np
import pytest
import torch

from tests import conv_f32_ref as R
from tests.conv_f32_ref import DEV, _assert_bit_exact, conv_out, round_up
from tests.util import cpu_threads

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CASES = R.all_cases()
DEFAULTS = dict(force_conv_variant=0, winograd=1, force_wino_variant=0, conv2d_sk=0, latency_force_unit=0, conv2d_wsplit=0,
                conv_precision=0)
SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces
SLICES = (-1, 2, 3, 6, 9, 18)


@pytest.fixture(scope='module')
def eng():
    from spec_amd.engine import Engine
    e = Engine('camcalib', torch.device(DEV))
    yield e
    for k, v in DEFAULTS.items():
        e.set_option(k, v)
    e.close()


@contextlib.contextmanager
def options(eng, **kw):
    try:
        for k, v in kw.items():
            eng.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)


_REFS = {}


def operands_and_reference(c):
    """(operands, float64 reference) of a case: checked against the exactness condition and computed once, shared, never changed."""
    key = (R.case_id(c), c['seed'])
    if key not in _REFS:
        o = R.integer_operands(c)
        R.assert_exact_in_fp32(c, o)
        with cpu_threads():
            ref = R.layer_reference(o, c['stride'], c['pad'], c['relu'], c['ds'][3] if c['ds'] else 1)
        _REFS[key] = (o, ref)
    return _REFS[key]


def _padded(a, ld, fill=float('nan')):
    """a (B,H,W,C) float64 -> (device buffer (B,H,W,ld) whose gap channels [C, ld) hold ``fill``, its view of the C channels)."""
    B, H, W, C = a.shape
    buf = torch.full((B, H, W, ld), fill, dtype=torch.float32)
    buf[..., :C] = torch.from_numpy(np.asarray(a)).float()
    buf = buf.to(DEV)
    return buf, buf[..., :C]


def launch(eng, c, o, ldx=None, ldo=None, coff=0, ldx2=None, skew=0, res_skew=None):
    """One launch of the case's layer with the given layout, profiled.  x lives in pixels of ldx floats whose gap channels are
    NaN (x2: ldx2), out in rows of ldo floats at channel offset coff, inside a sentinel-filled buffer that starts ``skew`` floats
    past a 16-byte boundary and has a margin before the first image and after the last; the residual in a buffer of the same
    layout (res_skew: its own skew, default the same as out's) whose other floats are NaN.
    Returns (y (B,OH,OW,cout) float32 ndarray, kernel names); asserts that no float outside the written positions changed."""
    B, cin, cout = c['B'], c['cin'], c['cout']
    OH, OW = conv_out(c['H'], c['k'], c['stride'], c['pad']), conv_out(c['W'], c['k'], c['stride'], c['pad'])
    ldx, ldo = ldx or cin, ldo or cout
    assert ldx >= cin and coff + cout <= ldo
    xbuf, x = _padded(o['x'], ldx)
    kw = {}
    if c['ds']:
        x2buf, x2 = _padded(o['x2'], ldx2 or c['ds'][0])
        kw = dict(x2=x2, w2_oihw=o['w2'].astype(np.float32), stride2=c['ds'][3])
    M = B * OH * OW
    margin = round_up(ldo + 64, 4)
    total = 2 * margin + M * ldo + 8
    strides = (OH * OW * ldo, OW * ldo, ldo, 1)

    def rows(base, off):
        v = base.as_strided((B, OH, OW, cout), strides, margin + off + coff)
        assert v.data_ptr() % 16 == ((off + coff) * 4) % 16
        return v
    obuf = torch.full((total,), SENTINEL, dtype=torch.int32, device=DEV)
    out = rows(obuf.view(torch.float32), skew)
    res = None
    if o['res'] is not None:
        rbuf = torch.full((total,), float('nan'), dtype=torch.float32, device=DEV)
        res = rows(rbuf, skew if res_skew is None else res_skew)
        res.copy_(torch.from_numpy(np.asarray(o['res'])).float())
    eng.profile(True)
    try:
        got = eng.conv2d(x, o['w'].astype(np.float32), o['scale'].astype(np.float32), o['shift'].astype(np.float32), c['stride'], c['pad'],
                         residual=res, relu=c['relu'], out=out, **kw)
        names = [e['kernel'] for e in eng.profile_read()]
    finally:
        eng.profile(False)
    assert got.data_ptr() == out.data_ptr()
    bits = obuf.cpu().numpy()
    written = np.zeros(total, dtype=bool)
    idx = (margin + skew + coff + np.arange(M)[:, None] * ldo + np.arange(cout)[None, :]).reshape(-1)
    written[idx] = True
    stray = np.flatnonzero(~written & (bits != np.int32(SENTINEL)))
    assert stray.size == 0, ('floats outside the (pixel, channel < Cout) positions were written', stray.size, 'first at float',
                             int(stray[0]) - margin - skew, 'of rows of', ldo, 'out starts at channel', coff)
    y = bits[idx].view(np.float32).reshape(B, OH, OW, cout)
    return y, names


def check(eng, c, want_kernel, opts, what, **layout):
    """Run the case under the options, compare with the reference bit for bit and the profiler's kernel with the intended one
    (a string = the exact name, a tuple = substrings that must all occur)."""
    o, ref = operands_and_reference(c)
    with options(eng, **opts):
        y, names = launch(eng, c, o, **layout)
    what = f'{R.case_id(c)} {what}'
    assert len(names) == 1, (what, names)
    if isinstance(want_kernel, str):
        assert names[0] == want_kernel, (what, names, want_kernel)
    else:
        assert all(s in names[0] for s in want_kernel), (what, names, want_kernel)
    _assert_bit_exact(y, ref, f'{what} [{names[0]}]')
    return names[0]


def direct_paths(c, forces=(0, 1, 2, 3, 13)):
    """(intended kernel, options, label) of every direct tile variant the case's shape allows."""
    return [(R.direct_kernel(c, f), dict(winograd=0, force_conv_variant=f), f'force_conv_variant={f}')
            for f in forces if R.direct_kernel(c, f)]


def bf16_paths(c):
    """conv_precision 3 / 6: integers up to 255 are exact in one bf16 piece, so the split path is exact too."""
    if c['cin'] % 16 or c['cout'] % 4 or (c['ds'] and c['ds'][0] % 16):
        return []
    return [(('bf16split', f'{t} terms') + (('2src',) if c['ds'] else ()), dict(conv_precision=t), f'conv_precision={t}') for t in (3, 6)]


def sliced_paths(c):
    """conv2d_sk in SLICES x latency_force_unit 1, 2, 3 on the sliced 64x64 kernel, conv2d_wsplit 2 / 3 on the wave-split one."""
    assert R.k_chunks(c) == 18
    src = ',2src' if c['ds'] else ''
    paths = []
    for S in SLICES:
        for unit in (1, 2, 3):
            # -1: the latency plan's own rule decides how many leaves; one leaf is the unsliced kernel
            want = (f'conv_igemm_f32<64x64,2x2{src}',) if S < 0 else f'conv_igemm_f32<64x64,2x2{src},splitK>'
            paths.append((want, dict(winograd=0, conv2d_sk=S, latency_force_unit=unit), f'conv2d_sk={S} unit={unit}'))
        for ws in (2, 3):
            # 2..4 leaves per group and two chunks per leaf: 2, 3, 6 and 9 slices of 18 chunks run on the wave-split kernel
            want = f'conv_wsplit_f32<32x32,4 leaves{src}>' if S in (2, 3, 6, 9) else ('_f32<',)
            paths.append((want, dict(winograd=0, conv2d_sk=S, conv2d_wsplit=ws), f'conv2d_sk={S} conv2d_wsplit={ws}'))
    return paths


def wino_paths(c):
    return [(R.wino_kernel(c, f), dict(winograd=1, force_wino_variant=f), f'force_wino_variant={f}') for f in (0, 8, 16)] if c['wino'] else []


# ---- a. + b. every kernel instance, same cases, same bits; the tails are the NAMED cases --------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=R.case_id)
def test_every_kernel_instance_bit_exact(eng, c):
    paths = direct_paths(c) + wino_paths(c) + bf16_paths(c)
    if c in R.SLICED_CASES:
        paths += sliced_paths(c)
    if c['ds']:
        paths += direct_paths(c, forces=(4,))
    assert paths, 'no kernel takes this case'
    for want, opts, label in paths:
        check(eng, c, want, opts, label)


def test_every_path_was_proved_by_the_profiler(eng):
    """Each kernel instance of the fp32 convolution path has at least one case in the list whose profiler entry names it."""
    seen = set()
    for c in R.NAMED_CASES + R.SLICED_CASES:
        paths = direct_paths(c) + wino_paths(c) + bf16_paths(c) + (sliced_paths(c) if c in R.SLICED_CASES else [])
        paths += direct_paths(c, forces=(4,)) if c['ds'] else []
        for want, opts, label in paths:
            seen.add(check(eng, c, want, opts, label))
    need = ['conv_igemm_f32<128x128,2x2>', 'conv_igemm_f32<128x64,2x2>', 'conv_igemm_f32<64x64,2x2>', 'conv_igemm_f32<128x32,4x1>',
            'conv_igemm_f32<64x64,2x2,splitK>', 'conv_igemm_f32<64x64,2x2,2src>', 'conv_igemm_f32<128x128,4x2,2src>',
            'conv_igemm_f32<64x64,2x2,2src,splitK>', 'conv_wsplit_f32<32x32,4 leaves>', 'conv_wsplit_f32<32x32,4 leaves,2src>',
            'conv_wino_f32<32t x64,F(2x2,3x3)>', 'conv_wino_f32<32t x128,F(2x2,3x3)>', 'conv_wino_f32<32t x64,F(2x2,3x3),res>',
            'conv1x1_bf16split<128x64,3 terms>', 'conv1x1_bf16split<128x64,6 terms>', 'conv_kxk_bf16split<128xN,3 terms>',
            'conv_kxk_bf16split<128xN,6 terms>', 'conv1x1_bf16split<128xN,3 terms,2src>', 'conv1x1_bf16split<128xN,6 terms,2src>']
    assert not [n for n in need if n not in seen], sorted(seen)


# ---- c. rows and columns no tap reaches must not be read into a result ---------------------------------------------------------------
UNREACHED = [R.case(2, 8, 6, 128, 64, 1, 2, 0, res=True, seed=41, name='unreached_1x1_s2'),
             R.case(3, 6, 10, 64, 48, 3, 2, 0, relu=True, seed=42, name='unreached_3x3_s2'),
             R.case(2, 3, 4, 64, 128, 1, 1, 0, ds=(64, 6, 8, 2), seed=43, name='unreached_x2_s2')]


@pytest.mark.parametrize('c', UNREACHED, ids=R.case_id)
def test_rows_and_columns_no_tap_reaches_are_not_read(eng, c):
    """pad 0 with (H - k) % stride != 0 and (W - k) % stride != 0 (x2: H2 = 2 OH, W2 = 2 OW at stride2 = 2): the last row and the
    last column of the source are NaN, the outputs equal the reference computed without them."""
    o, _ = operands_and_reference(c)
    o = dict(o)
    src = 'x2' if c['ds'] else 'x'
    k, stride = (1, c['ds'][3]) if c['ds'] else (c['k'], c['stride'])
    Hs, Ws = o[src].shape[1:3]
    assert (Hs - k) % stride != 0 and (Ws - k) % stride != 0 and c['pad'] == 0
    cropped = dict(o, **{src: np.ascontiguousarray(o[src][:, :Hs - 1, :Ws - 1])})
    ref = R.layer_reference(cropped, c['stride'], c['pad'], c['relu'], c['ds'][3] if c['ds'] else 1)
    poisoned = o[src].copy()
    poisoned[:, Hs - 1], poisoned[:, :, Ws - 1] = np.nan, np.nan
    o[src] = poisoned
    paths = direct_paths(c, forces=(0, 2, 3, 13, 4) if c['ds'] else (0, 2, 3, 13)) + bf16_paths(c)
    paths += [('splitK', dict(winograd=0, conv2d_sk=2), 'conv2d_sk=2'), ('conv_wsplit', dict(winograd=0, conv2d_sk=2, conv2d_wsplit=2), 'wsplit')]
    for want, opts, label in paths:
        with options(eng, **opts):
            y, names = launch(eng, c, o)
        assert (want in names[0]) if isinstance(want, str) else all(s in names[0] for s in want), (label, names)
        _assert_bit_exact(y, ref, f'{R.case_id(c)} {label} [{names[0]}]')


# ---- d. the layer as the trunks launch it ------------------------------------------------------------------------------------------
# (Cout, channel offset, row width) of HRNet's concat head (hrnet.hip): W32 writes 32 / 64 / 128 / 256 channels into rows of 480,
# W48 48 / 96 / 192 / 384 into rows of 720
CONCAT_SLICES = [(32, 0, 480), (64, 32, 480), (128, 96, 480), (48, 0, 720), (96, 48, 720), (192, 144, 720)]


@pytest.mark.parametrize('cout,coff,ldo', CONCAT_SLICES, ids=lambda v: str(v))
@pytest.mark.parametrize('cin,ldx', [(32, 64), (64, 128), (64, 64)], ids=lambda v: str(v))
def test_channel_strides_direct(eng, cin, ldx, cout, coff, ldo):
    """3x3 / stride 2 direct kernels with ldx > Cin (NaN in the gap channels) and the output as a channel slice of a wider map.
    (Cin, ldx) = (64, 64): the last 16 input channels carry zero weights, as W48's 48 channels padded to 64 do."""
    c = R.case(2, 7, 9, cin, cout, 3, 2, 1, res=cout in (64, 96), relu=cout != 128, seed=500 + cin + ldx + cout, name='concat_slice')
    if ldx == cin:
        o = R.integer_operands(c)
        o['w'][:, 48:] = 0.0
        R.assert_exact_in_fp32(c, o)
        _REFS[(R.case_id(c), c['seed'])] = (o, R.layer_reference(o, 2, 1, c['relu']))
    for want, opts, label in direct_paths(c) + bf16_paths(c):
        check(eng, c, want, opts, label, ldx=ldx, ldo=ldo, coff=coff)


@pytest.mark.parametrize('cin,ldx,cout,coff,ldo,res', [(48, 64, 64, 0, 64, True), (96, 128, 96, 0, 128, False), (32, 64, 128, 0, 128, True),
                                                       (48, 64, 64, 32, 480, False), (64, 64, 128, 96, 480, True),
                                                       (96, 128, 96, 48, 720, True), (160, 192, 192, 144, 720, False)], ids=lambda v: str(v))
def test_channel_strides_winograd(eng, cin, ldx, cout, coff, ldo, res):
    """Winograd on HRNet's stride-1 layers: C = 48 in rows of 64 and 96 in rows of 128 on both sides, and into the concat slices."""
    c = R.case(3, 7, 5, cin, cout, 3, 1, 1, res=res, relu=True, seed=600 + cin + cout + ldo, name='wino_strided')
    assert c['wino']
    for want, opts, label in wino_paths(c):
        check(eng, c, want, opts, label, ldx=ldx, ldo=ldo, coff=coff)
    if cin % 32 == 0:      # the same layout on the direct kernel
        check(eng, c, R.direct_kernel(c, 0), dict(winograd=0), 'direct', ldx=ldx, ldo=ldo, coff=coff)


MISALIGNED = [R.case(2, 5, 7, 64, 64, 3, 1, 1, res=True, relu=True, seed=71, name='misaligned_3x3'),
              R.case(3, 3, 5, 96, 100, 1, 1, 0, res=True, seed=72, name='misaligned_1x1'),
              R.case(1, 9, 4, 32, 32, 3, 2, 1, res=True, relu=True, seed=73, name='misaligned_128x32'),
              R.SLICED_CASES[0], R.SLICED_CASES[3]]


@pytest.mark.parametrize('c', MISALIGNED, ids=R.case_id)
def test_rows_that_are_not_16_byte_aligned_take_the_scalar_epilogue(eng, c):
    """out one float past alignment, the residual alone one float past it, and rows of ldo % 4 != 0: vec_ok = false.  The bits are
    the reference's, i.e. those of the aligned run."""
    paths = direct_paths(c, forces=(0, 1, 2, 3, 13, 4) if c['ds'] else (0, 1, 2, 3, 13))
    if c in R.SLICED_CASES:
        src = ',2src' if c['ds'] else ''
        paths += [(f'conv_igemm_f32<64x64,2x2{src},splitK>', dict(winograd=0, conv2d_sk=6, latency_force_unit=1), 'conv2d_sk=6'),
                  (f'conv_wsplit_f32<32x32,4 leaves{src}>', dict(winograd=0, conv2d_sk=6, conv2d_wsplit=2), 'wsplit')]
    for want, opts, label in paths:
        check(eng, c, want, opts, label + ' aligned')
        check(eng, c, want, opts, label + ' out + 1 float', skew=1)
        check(eng, c, want, opts, label + ' res + 1 float', skew=0, res_skew=1)
        check(eng, c, want, opts, label + ' ldo = Cout + 1', ldo=c['cout'] + 1)
        check(eng, c, want, opts, label + ' ldo = Cout + 6, out + 2 floats', ldo=c['cout'] + 6, skew=2)


def _two_source_cases():
    cases, i = [], 0
    for cin in (64, 256):
        for cin2 in (64, 256, 512):
            for s2 in (1, 2):
                B, OH, OW = 1 + i % 3, 3 + i % 4, 2 + i % 5
                extra = (i // 2) % 2                            # stride2 = 2: H2 = 2 OH - 1 and H2 = 2 OH both occur
                H2, W2 = (OH - 1) * s2 + 1 + (extra if s2 == 2 else 0), (OW - 1) * s2 + 1 + ((1 - extra) if s2 == 2 else 0)
                cout = (64, 128, 100, 256, 33, 192)[i % 6]
                cases.append((R.case(B, OH, OW, cin, cout, 1, 1, 0, res=i % 3 != 0, relu=i % 2 == 0, ds=(cin2, H2, W2, s2), seed=800 + i,
                                     name='two_sources'), cin2 + (32 if i % 4 in (1, 2) else 0)))
                i += 1
    return cases


@pytest.mark.parametrize('c,ldx2', _two_source_cases(), ids=lambda v: R.case_id(v) if isinstance(v, dict) else 'ldx2_%d' % v)
def test_second_a_source(eng, c, ldx2):
    """conv3 with the downsample folded in: K = [x | x2 at (oy * stride2, ox * stride2)], on both tiles dispatch_dual serves, the
    sliced and the wave-split kernel (where the K chunks divide) and the split-bf16 one; ldx2 > Cin2 with NaN in the gap."""
    paths = direct_paths(c, forces=(0, 3, 4)) + bf16_paths(c)
    if R.k_chunks(c) % 2 == 0 and R.k_chunks(c) >= 4:
        paths += [('conv_igemm_f32<64x64,2x2,2src,splitK>', dict(winograd=0, conv2d_sk=2, latency_force_unit=1), 'conv2d_sk=2'),
                  ('conv_wsplit_f32<32x32,4 leaves,2src>', dict(winograd=0, conv2d_sk=2, conv2d_wsplit=3), 'wsplit')]
    for want, opts, label in paths:
        check(eng, c, want, opts, label, ldx2=ldx2, ldo=c['cout'] + (64 if c['cout'] % 4 == 0 else 3), coff=0)


def test_strided_entry_refuses_what_the_kernels_cannot_take(eng):
    """SPECMI_ERR_ARG, nothing launched (no profiler entry, the sentinel buffer untouched), and the handle stays usable."""
    import ctypes as C
    from spec_amd import _lib
    c = R.case(1, 4, 4, 64, 64, 1, 1, 0, seed=90)
    o, ref = operands_and_reference(c)
    w, sc, sh = (np.ascontiguousarray(o[k], dtype=np.float32) for k in ('w', 'scale', 'shift'))
    x = torch.from_numpy(o['x']).float().to(DEV)
    sent = torch.full((4 * 4 * 64 + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    out = sent.view(torch.float32)[:1024].view(1, 4, 4, 64)
    w3, w2 = np.zeros((64, 64, 3, 3), np.float32), np.zeros((64, 64, 1, 1), np.float32)
    x2 = torch.zeros(1, 4, 4, 64, device=DEV)
    wide = torch.zeros(1, 4, 4, 72, device=DEV)
    bad = [('x not 16-byte aligned', dict(x=wide[..., 2:66], w=w)),                   # (8 bytes in, ldx = 72)
           ('ldx % 4 != 0', dict(x=torch.zeros(1, 4, 4, 66, device=DEV)[..., :64], w=w)),
           ('x2 smaller than the outputs need', dict(x=x, w=w, x2=x2[:, :3], w2_oihw=w2)),
           ('x2 at stride 2 does not cover the outputs', dict(x=x, w=w, x2=x2, w2_oihw=w2, stride2=2)),
           ('ldx2 % 4 != 0', dict(x=x, w=w, x2=torch.zeros(1, 4, 4, 66, device=DEV)[..., :64], w2_oihw=w2)),
           # Winograd stores 16 bytes per lane: rows of out that are not 16-byte aligned are refused, not written wrongly
           ('Winograd into misaligned rows', dict(x=x, w=w3, pad=1, out=sent.view(torch.float32)[1:1025].view(1, 4, 4, 64)))]
    eng.profile(True)
    for what, kw in bad:
        kw = dict(kw)
        xx, ww, pad, oo = kw.pop('x'), kw.pop('w'), kw.pop('pad', 0), kw.pop('out', out)
        with pytest.raises(_lib.SpecmiError) as e:
            eng.conv2d(xx, ww, sc, sh, 1, pad, relu=False, out=oo, **kw)
        assert e.value.code == _lib.ERR_ARG, (what, str(e.value))
    # ldx < Cin and ldo < Cout: no tensor view says that, so through the C entry itself
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # ... and a second source on a 3x3 layer
    dp = lambda t: C.c_void_p(t.data_ptr())
    for what, ldx, ldo, k, src2 in (('ldx < Cin', 60, 64, 1, None), ('ldo < Cout', 64, 60, 1, None), ('x2 on a 3x3 layer', 64, 64, 3, x2)):
        rc = eng.lib.specmi_conv2d_strided(eng.h, dp(x), 1, 4, 4, 64, ldx, p(w3 if k == 3 else w), p(sc), p(sh), 64, k, k, 1, k // 2, None, 0,
                                           dp(out), ldo, dp(src2) if src2 is not None else None, 4, 4, 64, 64, 1, eng._stream())
        assert rc == _lib.ERR_ARG, (what, rc)
    assert eng.profile_read() == []
    eng.profile(False)
    assert bool((sent == SENTINEL).all())
    y = eng.conv2d(x, w, sc, sh, 1, 0, relu=False, out=out)
    _assert_bit_exact(y.cpu().numpy(), ref, 'after the refusals')


# ---- e. the other fp32 trunk kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,W', [(1, 1, 1), (1, 7, 9), (3, 13, 8), (2, 33, 47)])
def test_stem_7x7_bit_exact(eng, B, H, W):
    """The MFMA 7x7 / stride 2 / pad 3 stem on integer images and weights: K = 147 products of |x| <= 4, |w| <= 8."""
    rng = np.random.default_rng(7000 + H)
    x = rng.integers(-R.X_MAX, R.X_MAX + 1, (B, 3, H, W)).astype(np.float64)
    w = rng.integers(-R.W_MAX, R.W_MAX + 1, (64, 3, 7, 7)).astype(np.float64)
    scale = np.asarray(R.SCALES)[rng.integers(0, 4, 64)]
    shift = rng.integers(-32, 33, 64) * 0.25
    assert 147 * R.X_MAX * R.W_MAX * 2.0 + 8.0 < 2.0 ** 22
    for relu in (True, False):
        ref = R.nhwc(R.conv64(x, w, 2, 3)) * scale + shift
        ref = np.maximum(ref, 0.0) if relu else ref
        eng.profile(True)
        y = eng.conv2d(torch.from_numpy(x).float().to(DEV), w.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32), 2, 3,
                       relu=relu, nchw_input=True).cpu().numpy()
        names = [e['kernel'] for e in eng.profile_read()]
        eng.profile(False)
        assert names == ['stem_conv7x7_f32'], names
        _assert_bit_exact(y, ref, f'stem relu={relu}')


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', [4, 252, 256, 260, 2048])
def test_avgpool_bit_exact(eng, B, C):
    """Integer maps: the sum is exact in any order, the mean is float32(sum) / float32(HW), one rounding.  The map sizes cross every
    ``parts`` boundary of launch_avgpool (HW / 32 = 1, 2, 15, 16 and its cap), the channel counts the edge of the 64-lane block of
    avgpool_parts_kernel (63, 64, 65 channel quads)."""
    rng = np.random.default_rng(C * 10 + B)
    for HW in (1, 31, 32, 49, 63, 64, 65, 511, 512, 513, 646):
        H, W = (19, 34) if HW == 646 else (1, HW)
        x = rng.integers(-64, 65, (B, H, W, C))
        want = x.reshape(B, HW, C).sum(1).astype(np.float32) / np.float32(HW)
        y = eng.avgpool(torch.from_numpy(x).float().to(DEV)).cpu().numpy()
        assert y.shape == want.shape
        bad = y != want
        assert not bad.any(), (HW, int(bad.sum()), np.argwhere(bad)[0].tolist(), y[bad][:4].tolist(), want[bad][:4].tolist())
