"""The three kernels hrnet.hip adds to the conv kernels - the 3-channel 3x3 / stride-2 stem, the exchange-unit sum with nearest
upsampling (also the strided copy into the concat head) and the align_corners bilinear resize - one launch at a time on the
MI355X, through specmi_hr_stem3x3 / specmi_hr_fuse_sum / specmi_hr_resize_ac: the launchers hrnet_forward itself calls, so what is
pinned here is the trunk's code, at the smallest shapes at which it can go wrong.

  * stem: integer operands for which every fp32 partial sum is exact (tests/hrnet_ref.py, checked on the CPU by
    tests/test_hrnet_ref_host.py) - equal to the float64 reference BIT FOR BIT; one random case within a derived bound;
  * fuse sum: arbitrary fp32 terms over six decades - BIT-EQUAL to a float32 evaluation that adds in the stated order
    ((t0 + t1) + t2) + t3 (fp32 addition is deterministic once the order is fixed);
  * resize: bit for bit where the scale (in - 1) / (out - 1) is an integer or a half-integer (the geometries of trunk inputs 32,
    64 and 96, the OH == 1 / OW == 1 branch included), within a derived bound where it is not.

Every output lives in a buffer pre-filled with a sentinel NaN, as a channel slice (ldo > C, channel offset) of the concat head's
rows where the kernel allows it; every float outside the written slice must still hold the sentinel.

Measured on MI355X: the file (114 tests) takes 2.6 s, the slowest test 0.17 s.  The random stem case reaches 0.10 of its bound, the
four bounded resize cases 0.10 - 0.17 of theirs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import hrnet_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces
# (C, channel offset, row width) of HRNet's concat head: W32 writes 32 / 64 / 128 / 256 channels into rows of 480, W48 48 / 96 / 192 / 384
# into rows of 720
CONCAT = {32: (32, 0, 480), 64: (64, 32, 480), 128: (128, 96, 480), 48: (48, 0, 720), 96: (96, 48, 720)}


@pytest.fixture(scope='module')
def eng():
    from spec_amd.engine import Engine
    e = Engine('hmr', torch.device(DEV))
    yield e
    e.close()


class Slice:
    """A (B,H,W,C) output as channels [coff, coff + C) of rows of ldo floats, inside a sentinel-filled buffer with a margin before the
    first pixel and after the last."""

    def __init__(self, shape, coff=0, ldo=None):
        self.shape = B, H, W, Cc = shape
        self.coff, self.ldo = coff, ldo or Cc
        assert self.coff + Cc <= self.ldo and self.coff % 4 == 0 and self.ldo % 4 == 0
        self.npix = B * H * W
        self.margin = -(-(self.ldo + 64) // 4) * 4
        self.total = 2 * self.margin + self.npix * self.ldo
        self.buf = torch.full((self.total,), SENTINEL, dtype=torch.int32, device=DEV)
        self.view = self.buf.view(torch.float32).as_strided(shape, (H * W * self.ldo, W * self.ldo, self.ldo, 1), self.margin + self.coff)
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def read(self):
        """The written slice as a float32 ndarray; asserts that every float outside it still holds the sentinel."""
        bits = self.buf.cpu().numpy()
        idx = (self.margin + self.coff + np.arange(self.npix)[:, None] * self.ldo + np.arange(self.shape[3])[None, :]).reshape(-1)
        written = np.zeros(self.total, dtype=bool)
        written[idx] = True
        stray = np.flatnonzero(~written & (bits != np.int32(SENTINEL)))
        assert stray.size == 0, ('floats outside the written slice changed', stray.size, 'first at float', int(stray[0]) - self.margin,
                                 'rows of', self.ldo, 'slice starts at channel', self.coff)
        return bits[idx].view(np.float32).reshape(self.shape)


def padded(a, ld):
    """a (B,H,W,C) -> its C channels as a view of a device buffer (B,H,W,ld) whose gap channels [C, ld) hold the sentinel NaN."""
    B, H, W, Cc = a.shape
    buf = torch.full((B, H, W, ld), SENTINEL, dtype=torch.int32).view(torch.float32)
    buf[..., :Cc] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return buf.to(DEV)[..., :Cc]


def assert_same_numbers(y, ref, what):
    """y as the device stored it against the reference: equal as numbers (-0 == +0; a NaN equals nothing), else the first mismatch."""
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    assert not np.isnan(y).any(), (what, 'NaN in the output', int(np.isnan(y).sum()))
    bad = ~(y.astype(np.float64) == np.asarray(ref, dtype=np.float64))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} differ, first at (b, y, x, c) = {i}: got {float(y[i])!r}, want {float(ref[i])!r}')


# ---- stem ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,W', R.STEM_SHAPES)
def test_stem_bit_exact(eng, B, H, W):
    x, w, scale, shift = R.stem_integer_operands(B, H, W, seed=H * 100 + W)
    ref = R.stem3x3(x, w, scale, shift)
    out = Slice(ref.shape)
    eng.hr_stem3x3(torch.from_numpy(x).float(), w, scale, shift, out=out.view)
    assert_same_numbers(out.read(), ref, f'stem B={B} {H}x{W}')


def test_stem_random_within_the_fma_bound(eng):
    """Random fp32 operands against float64.  The device runs 27 fused multiply-adds and one fma(acc, scale, shift) per output: each
    rounds once, relative 2^-24, a quantity bounded by sum |w x| (by sum |w x| |scale| + |shift| for the last, and |shift| stays
    below sum |w x| |scale| here), and the ReLU does not enlarge an error: |err| <= 29 * 2^-24 * sum |w x| * |scale|."""
    B, H, W = 2, 33, 47
    rng = np.random.default_rng(20260)
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    w = rng.standard_normal((64, 3, 3, 3)).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, 64) * rng.choice([-1.0, 1.0], 64)).astype(np.float32)
    shift = (0.25 * rng.standard_normal(64)).astype(np.float32)
    ref = R.stem3x3(x, w, scale, shift)
    S = R.stem3x3_abs(x, w) * np.abs(scale.astype(np.float64))
    assert (np.abs(shift) <= S).all()
    out = Slice(ref.shape)
    eng.hr_stem3x3(torch.from_numpy(x), w, scale, shift, out=out.view)
    y = out.read()
    assert np.isfinite(y).all()
    err = np.abs(y.astype(np.float64) - ref)
    bound = 29 * 2.0 ** -24 * S
    i = np.unravel_index(np.argmax(err - bound), err.shape)
    print('stem random: max err / bound =', float((err / bound).max()))
    assert (err <= bound).all(), (i, err[i], bound[i])


# ---- fuse sum --------------------------------------------------------------------------------------------------------------------
# the shift sets the trunk produces for each output level of a 2-, 3- and 4-branch module, and the single term of the concat copy
SH_SETS = [(0,), (0, 1), (0, 0), (0, 1, 2), (0, 0, 1), (0, 0, 0), (0, 1, 2, 3), (0, 0, 1, 2), (0, 0, 0, 1), (0, 0, 0, 0)]
TERM_LD = {32: (32, 64, 96, 128), 48: (64, 96, 48, 128)}       # every term its own pixel stride; C = 48 in rows of 64 first


def fuse_terms(B, H, W, Cc, sh, seed):
    """randn times a scale per term, the scales spread over 1e-3 .. 1e3"""
    rng = np.random.default_rng(seed)
    decades = rng.permutation(np.linspace(-3.0, 3.0, 4))
    return [(rng.standard_normal((B, H >> s, W >> s, Cc)) * 10.0 ** decades[k]).astype(np.float32) for k, s in enumerate(sh)]


def run_fuse(eng, terms, sh, lds, relu, geom):
    Cc, coff, ldo = geom
    B, h0, w0, _ = terms[0].shape
    out = Slice((B, h0 << sh[0], w0 << sh[0], Cc), coff, ldo)
    eng.hr_fuse_sum([padded(t, ld) for t, ld in zip(terms, lds)], sh, relu=relu, out=out.view)
    return out.read()


@pytest.mark.parametrize('Cc', [32, 48])
@pytest.mark.parametrize('H,W', [(8, 8), (8, 16), (16, 8), (8, 24)])
@pytest.mark.parametrize('sh', SH_SETS, ids=lambda s: 'sh' + ''.join(map(str, s)))
def test_fuse_sum_bit_equal_to_the_ordered_float32_sum(eng, sh, H, W, Cc):
    for B in (1, 3):
        terms = fuse_terms(B, H, W, Cc, sh, seed=B * 1000 + H * 10 + W + Cc + 7 * len(sh) + sum(sh))
        for relu in (False, True):
            ref = R.fuse_sum_f32(terms, sh, relu)
            assert ref.dtype == np.float32 and np.isfinite(ref).all()
            y = run_fuse(eng, terms, sh, TERM_LD[Cc], relu, CONCAT[Cc] if B == 1 else (Cc, 64, 480 if Cc == 32 else 720))
            assert_same_numbers(y, ref, f'fuse sh={sh} B={B} {H}x{W} C={Cc} relu={relu}')
            if relu:
                assert (y >= 0).all()


@pytest.mark.parametrize('B,H,W,Cc,sh', [(3, 2, 6, 48, (0, 1)), (1, 4, 4, 32, (0, 1, 2)), (5, 2, 2, 36, (0, 0, 1))])
def test_fuse_sum_element_count_not_a_multiple_of_256(eng, B, H, W, Cc, sh):
    """B * H * W * C / 4 = 432, 128 and 180 lanes: a last block that is partly idle, and a launch of less than one block."""
    assert (B * H * W * Cc // 4) % 256
    terms = fuse_terms(B, H, W, Cc, sh, seed=B + H + W + Cc)
    lds = (64, 96, 48, 128)
    for relu in (False, True):
        y = run_fuse(eng, terms, sh, lds, relu, (Cc, 48, 720))
        assert_same_numbers(y, R.fuse_sum_f32(terms, sh, relu), f'fuse tail B={B} {H}x{W} C={Cc} relu={relu}')


def test_fuse_sum_as_the_concat_copy(eng):
    """n = 1, relu = 0: W48's lowest-resolution branch (384 channels, dense rows) copied into channels [336, 720) of the head."""
    for B, H, W in ((1, 1, 1), (3, 1, 2), (2, 3, 2)):
        t = fuse_terms(B, H, W, 384, (0,), seed=B * 10 + H + W)[0]
        t[0, 0, 0, :4] = (-0.0, 0.0, -1.5, 1e-30)
        y = run_fuse(eng, [t], (0,), (384,), False, (384, 336, 720))
        assert_same_numbers(y, t, f'concat copy B={B} {H}x{W}')


# ---- resize ----------------------------------------------------------------------------------------------------------------------
def run_resize(eng, x, OH, OW, ld, geom):
    Cc, coff, ldo = geom
    out = Slice((x.shape[0], OH, OW, Cc), coff, ldo)
    eng.hr_resize_ac(padded(x, ld), (OH, OW), out=out.view)
    return out.read()


@pytest.mark.parametrize('hw,ohw', R.RESIZE_EXACT_CASES, ids=lambda v: '%dx%d' % v)
def test_resize_bit_exact_where_the_scale_is_dyadic(eng, hw, ohw):
    (H, W), (OH, OW) = hw, ohw
    for B, Cc, ld in ((3, 32, 32), (1, 64, 96), (2, 48, 64)):
        x = R.resize_integer_input(B, H, W, Cc, seed=H * 100 + W + Cc)
        ref = R.resize_ac(x, OH, OW)
        y = run_resize(eng, x, OH, OW, ld, CONCAT[Cc])
        assert_same_numbers(y, ref, f'resize {H}x{W} -> {OH}x{OW} B={B} C={Cc}')


@pytest.mark.parametrize('hw,ohw', R.RESIZE_BOUNDED_CASES, ids=lambda v: '%dx%d' % v)
def test_resize_within_the_coordinate_bound(eng, hw, ohw):
    """The scale is not an fp32 number: the coordinate fl(fl(s) * o) carries two roundings, at most 2^-23 * (in - 1) together, and
    with it both weights of that axis; a value then moves by at most that times the difference of two neighbours (<= 2 max|x|) per
    axis, and the four products and three sums add some 6 ulp of max|x|: |err| <= 2^-22 * (H + W) * max|x|.  The data are random
    integers, so a wrong neighbour is an error of order max|x|."""
    (H, W), (OH, OW) = hw, ohw
    B, Cc = 2, 128
    x = R.resize_integer_input(B, H, W, Cc, seed=H * 100 + W)
    ref = R.resize_ac(x, OH, OW)
    bound = 2.0 ** -22 * (H + W) * np.abs(x).max()
    y = run_resize(eng, x, OH, OW, 160, CONCAT[Cc])
    assert np.isfinite(y).all()
    err = np.abs(y.astype(np.float64) - ref)
    print(f'resize {H}x{W} -> {OH}x{OW}: max err {err.max():.3e}, bound {bound:.3e}')
    assert err.max() <= bound, (np.unravel_index(err.argmax(), err.shape), err.max(), bound)
    # align_corners: the four corners of the output are the four corners of the input
    for oy, iy in ((0, 0), (OH - 1, H - 1)):
        for ox, ix in ((0, 0), (OW - 1, W - 1)):
            d = np.abs(y[:, oy, ox].astype(np.float64) - x[:, iy, ix]).max()
            assert d <= bound, ('corner', (oy, ox), d, bound)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch(eng):
    """Every class of bad argument returns SPECMI_ERR_ARG with a message, and the sentinel-filled output stays untouched."""
    from spec_amd import _lib
    lib, h = eng.lib, eng.h
    B, H, W, Cc, ld, ldo = 2, 8, 8, 32, 64, 96
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    img = torch.zeros(B, 3, H, W, device=DEV)
    wk, sc, sf = torch.zeros(27 * 64, device=DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    terms = [torch.zeros(B, H >> s, W >> s, ld, device=DEV) for s in (0, 1, 2, 3)]
    xin = torch.zeros(B, H, W, ld, device=DEV)
    out = Slice((B, H, W, 64), 0, ldo)             # large enough for every call below, were it (wrongly) launched
    p = lambda t: C.c_void_p(t.data_ptr())
    po = p(out.view)

    def refused(rc, what):
        torch.cuda.synchronize()
        assert rc == _lib.ERR_ARG, (what, rc)
        msg = lib.specmi_last_error(h)
        assert msg and len(msg) > 8, (what, msg)
        assert out.untouched(), what

    def stem(images=p(img), B=B, H=H, W=W, w=p(wk), scale=p(sc), shift=p(sf), o=po):
        return lib.specmi_hr_stem3x3(h, images, B, H, W, w, scale, shift, o, stream)

    def fuse(ptrs=None, lds=(ld,) * 4, shs=(0, 1, 2, 3), n=4, B=B, H=H, W=W, Cc=Cc, o=po, ldo=ldo, null_arrays=False):
        ptrs = [t.data_ptr() for t in terms] if ptrs is None else ptrs
        a = (C.c_void_p * 4)(*ptrs), (C.c_int * 4)(*lds), (C.c_int * 4)(*shs)
        if null_arrays:
            a = (None, a[1], a[2])
        return lib.specmi_hr_fuse_sum(h, a[0], a[1], a[2], n, B, H, W, Cc, 1, o, ldo, stream)

    def resize(x=p(xin), B=B, H=H, W=W, Cc=Cc, ld=ld, o=po, OH=4, OW=4, ldo=ldo):
        return lib.specmi_hr_resize_ac(h, x, B, H, W, Cc, ld, o, OH, OW, ldo, stream)

    # null pointers
    for kw in (dict(images=None), dict(w=None), dict(scale=None), dict(shift=None), dict(o=None)):
        refused(stem(**kw), ('stem NULL', kw))
    refused(fuse(null_arrays=True), 'fuse NULL terms array')
    refused(fuse(ptrs=[terms[0].data_ptr(), None, terms[2].data_ptr(), terms[3].data_ptr()]), 'fuse NULL term')
    refused(fuse(o=None), 'fuse NULL out')
    refused(resize(x=None), 'resize NULL x')
    refused(resize(o=None), 'resize NULL out')
    # sizes <= 0
    for kw in (dict(B=0), dict(H=0), dict(W=-1)):
        refused(stem(**kw), ('stem size', kw))
        refused(fuse(**kw), ('fuse size', kw))
        refused(resize(**kw), ('resize size', kw))
    for kw in (dict(Cc=0), dict(OH=0), dict(OW=-3)):
        refused(resize(**kw), ('resize size', kw))
    refused(fuse(Cc=0), 'fuse C = 0')
    # C % 4
    refused(fuse(Cc=30), 'fuse C % 4')
    refused(resize(Cc=30), 'resize C % 4')
    # ld % 4, ld < C
    refused(fuse(lds=(ld, ld, 62, ld)), 'fuse ld % 4')
    refused(fuse(lds=(ld, 28, ld, ld)), 'fuse ld < C')
    refused(fuse(ldo=94), 'fuse ldo % 4')
    refused(fuse(ldo=28), 'fuse ldo < C')
    refused(resize(ld=62), 'resize ld % 4')
    refused(resize(ld=28), 'resize ld < C')
    refused(resize(ldo=94), 'resize ldo % 4')
    refused(resize(ldo=28), 'resize ldo < C')
    # H or W not divisible by 2^sh
    refused(fuse(H=12), 'fuse H = 12 with sh = 3')
    refused(fuse(W=4), 'fuse W = 4 with sh = 3')
    refused(fuse(shs=(0, 1, 2, 4)), 'fuse sh = 4 at 8x8')
    refused(fuse(shs=(0, -1, 0, 0)), 'fuse negative sh')
    # n outside 1..4
    refused(fuse(n=0), 'fuse n = 0')
    refused(fuse(n=5), 'fuse n = 5')
    # and the same calls with good arguments run
    assert stem() == _lib.OK and fuse() == _lib.OK and resize() == _lib.OK
    torch.cuda.synchronize()
    assert not out.untouched()
