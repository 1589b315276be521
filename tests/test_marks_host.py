"""Host tests of the marks contract (tests/marks_ref.py, spec_amd/csrc/marks.hip): the NumPy restatement against the installed
Pillow, the composition of strip, mask blend and line against ``render.show_horizon_line`` as it stands and against the
reference's own function (tests/golden/horizon_line.npz), where ``horizon_marks`` falls back, what ``check_draw_marks`` refuses,
the declarations, and the denormalisation.  No device."""
import os
import re

import numpy as np
import pytest

from tests import marks_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pillow_line(H, W, xy, width):
    from PIL import Image, ImageDraw
    im = Image.new('L', (W, H), 0)
    ImageDraw.Draw(im).line(xy, fill=255, width=width)
    return np.array(im)


def ref_line(H, W, xy, width):
    return MR.draw_line(np.zeros((H, W, 1), np.uint8), *xy, width, 255)[..., 0]


def line_cases():
    """5 200 seeded cases: every width 2 .. 64 at least 80 times; frames from 1 x 1 to 1080 x 1920 with 1 x N and N x 1; end
    points out to +-100000 exactly; dy == 0, |dy| <= 1, near-vertical, wholly outside, zero length."""
    rng = np.random.default_rng(20261019)
    lim = MR.LINE_MAX_COORD
    cases = []
    for i in range(5200):
        width = 2 + i % 63
        shape = i % 13
        if i % 260 == 0:
            H, W = 1080, 1920
        elif shape == 0:
            H, W = 1, int(rng.integers(1, 400))
        elif shape == 1:
            H, W = int(rng.integers(1, 400)), 1
        elif shape == 2:
            H, W = 1, 1
        else:
            H, W = int(rng.integers(1, 140)), int(rng.integers(1, 180))
        kind = (i // 13) % 10
        r = lambda a, b: int(rng.integers(a, b + 1))
        if kind == 0:                                               # anywhere in the checked range
            xy = [r(-lim, lim) for _ in range(4)]
        elif kind == 1:                                             # at the limit itself, through or past the frame
            xy = [-lim, r(-lim, lim), lim, r(-lim, lim)] if i % 2 else [r(-lim, lim), lim, r(-lim, lim), -lim]
        elif kind == 2:                                             # the horizon's shape: x from 0 to W, any slope
            xy = [0, r(-3 * H, 4 * H), W, r(-3 * H, 4 * H)]
        elif kind == 3:                                             # dy == 0
            y = r(-70, H + 70)
            xy = [r(-lim, W), y, r(0, lim), y]
        elif kind == 4:                                             # |dy| <= 1 over a long run
            y = r(-40, H + 40)
            xy = [-lim, y, lim, y + r(-1, 1)]
        elif kind == 5:                                             # near-vertical
            x = r(-40, W + 40)
            xy = [x, r(-lim, 0), x + r(-1, 1), r(H, lim)]
        elif kind == 6:                                             # wholly outside
            xy = [r(W + 100, lim), r(-lim, lim), r(W + 100, lim), r(-lim, lim)]
        elif kind == 7:                                             # inside and short
            xy = [r(-20, W + 20), r(-20, H + 20), r(-20, W + 20), r(-20, H + 20)]
        elif kind == 8:                                             # zero length
            x, y = r(-5, W + 5), r(-5, H + 5)
            xy = [x, y, x, y]
        else:                                                       # moderate range
            xy = [r(-3000, 3000) for _ in range(4)]
        cases.append((H, W, xy, width))
    return cases


def test_wide_line_equals_pillow():
    cases = line_cases()
    assert len(cases) >= 5000 and {c[3] for c in cases} == set(range(2, 65))
    assert any(max(abs(v) for v in c[2]) == MR.LINE_MAX_COORD for c in cases)
    bad = [(H, W, xy, width) for H, W, xy, width in cases if not np.array_equal(ref_line(H, W, xy, width), pillow_line(H, W, xy, width))]
    assert not bad, (len(bad), bad[:5])
    drawn = sum(1 for H, W, xy, width in cases[::7] if ref_line(H, W, xy, width).any())
    assert drawn > 200                                                      # the cases do draw


def test_mask_blend_equals_pillow():
    """The general blend - a coloured ink over a coloured background, every mask value - is the installed Pillow's, one rounding
    of the sum; clipped at every edge and at negative positions."""
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(7)
    mask = rng.integers(0, 256, (256, 40), dtype=np.uint8)
    mask[:, 0] = np.arange(256)                                             # every coverage value
    for (H, W), (x, y), ink in (((300, 64), (3, 5), (200, 13, 77)), ((50, 30), (-7, -100), (0, 255, 1)), ((40, 90), (70, 20), (255, 255, 255)),
                                ((20, 20), (-50, 3), (9, 9, 9)), ((300, 64), (0, 0), (0, 0, 0))):
        bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        bg[:, :2] = (0, 0, 0)
        bg[:, 2:4] = (255, 255, 255)
        im = Image.fromarray(bg.copy())
        d = ImageDraw.Draw(im)
        d.draw.draw_bitmap((x, y), Image.fromarray(mask).im, d._getink(ink)[0])
        assert np.array_equal(MR.blend_mask(bg.copy(), mask, x, y, ink), np.array(im)), ((H, W), (x, y))


COLOURS = ((0, 255, 0), (255, 0, 0), (17, 130, 250))


def compose(img, horizons):
    """``plan_horizon_marks`` + ``marks_ref.apply_marks``: what the device route draws, on the host."""
    from spec_amd import render
    plan = render.plan_horizon_marks([img.shape[:2]], [horizons])
    assert plan is not None
    ranges, marks, masks, fracs = plan
    assert tuple(ranges[0]) == (0, marks.shape[0])
    return MR.apply_marks(img.copy(), marks, masks), fracs[0]


def test_composition_equals_show_horizon_line():
    from spec_amd import render
    rng = np.random.default_rng(11)
    n = 0
    for (H, W) in ((96, 128), (64, 40), (33, 300), (30, 7), (200, 150)):     # 40 and 7 wide: narrower than the caption
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for debug in (False, True):
            for GT in (False, True):
                for ts in (16, 30):
                    for width in (3, 5):
                        colour = COLOURS[n % 3]
                        # the line crosses the strip for a horizon near the top (pitch up) or the bottom (pitch down)
                        vfov, pitch, roll = 0.9, (0.38 if n % 4 == 0 else -0.38 if n % 4 == 1 else 0.05), (-0.2, 0.0, 0.31)[n % 3]
                        f_pix = H / 2 / np.tan(vfov / 2)
                        kw = dict(focal_length=f_pix, color=colour, width=width, debug=debug, GT=GT, text_size=ts)
                        want, ctr = render.show_horizon_line(img, vfov, pitch, roll, **kw)
                        got, fr = compose(img, [dict(vfov=vfov, pitch=pitch, roll=roll, **kw)])
                        assert np.array_equal(got, want), (H, W, debug, GT, ts, width)
                        assert fr == [ctr]
                        n += 1
    assert n == 5 * 16


def test_text_over_the_picture_and_numpy_scalars():
    """A strip lower than the caption (text_size 4) lets the text blend over the picture itself: the general blend in the
    composition; float32 scalars take the reference's float32 arithmetic."""
    from spec_amd import render
    img = np.random.default_rng(5).integers(0, 256, (80, 120, 3), dtype=np.uint8)
    for GT in (False, True):
        kw = dict(focal_length=np.float32(77.7), color=(255, 0, 0), width=3, debug=True, GT=GT, text_size=4)
        a = (np.float32(1.1), np.float32(-0.2), np.float32(0.1))
        want, ctr = render.show_horizon_line(img, *a, **kw)
        got, fr = compose(img, [dict(vfov=a[0], pitch=a[1], roll=a[2], **kw)])
        assert np.array_equal(got, want) and fr == [ctr]
        assert ((want[6:12] != img[6:12]) & (want[6:12] != 255)).any() or GT  # blended values, not only ink


def test_two_horizons_in_validation_order():
    """Ground truth (blue, strip at the bottom) then prediction (red, strip at the top), as save_images draws them."""
    from spec_amd import render
    img = np.random.default_rng(3).integers(0, 256, (100, 140, 3), dtype=np.uint8)
    f = lambda v: 100 / 2 / np.tan(v / 2)
    gt = dict(vfov=1.0, pitch=0.1, roll=-0.05, focal_length=f(1.0), color=(0, 0, 255), width=3, debug=True, GT=True, text_size=16)
    pr = dict(vfov=0.8, pitch=0.12, roll=0.3, focal_length=f(0.8), color=(255, 0, 0), width=3, debug=True, GT=False, text_size=16)
    want = img
    for kw in (gt, pr):
        kw = dict(kw)
        want, _ = render.show_horizon_line(want, kw.pop('vfov'), kw.pop('pitch'), kw.pop('roll'), **kw)
    got, fracs = compose(img, [gt, pr])
    assert np.array_equal(got, want) and len(fracs) == 2
    other, _ = compose(img, [pr, gt])
    assert not np.array_equal(other, want)                                  # the order matters: the lines cross


def test_composition_equals_the_reference_fixture():
    import PIL
    from spec_amd import render
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'horizon_line.npz'))
    checked = 0
    for k, cp in enumerate(g['cam_params']):
        host = render.group_panel0(g['frame'], cp)
        got, fr = compose(g['frame'], render._panel0_horizon(cp))
        assert np.array_equal(got, host)
        if np.array_equal(host, g[f'out_{k}']):                             # wherever the present host function equals it
            assert np.array_equal(got, g[f'out_{k}']) and fr == [float(g[f'ctr_{k}'])]
            checked += 1
    assert checked == len(g['cam_params']) or str(g['pillow_version']) != PIL.__version__


def test_horizon_marks_falls_back_exactly_where_listed():
    from spec_amd import render
    hm = lambda **kw: render.horizon_marks(**{**dict(H=64, W=80, vfov=1.0, pitch=0.1, roll=0.1, width=3), **kw})
    ok = hm()
    assert ok is not None and ok[0].shape == (1, 8) and ok[1] is None
    assert hm(debug=True, text_size=64) is not None and hm(debug=True, text_size=0) is not None
    assert hm(roll=np.pi / 2 - 1e-3) is not None                            # steep, but within +-100000
    assert hm(roll=float('nan')) is None and hm(pitch=float('inf')) is None and hm(vfov=0.0) is None      # non-finite end points
    assert hm(roll=np.pi / 2 - 1e-5) is None                                # end points beyond +-100000
    far = 80 * np.tan(1.5) / 2
    assert 32 - far < -5 and hm(roll=1.5) is not None
    edge = np.arctan(2 * (100000.5 - 28.0) / 80)                            # left = ctr - 40 tan(roll) just inside -100001
    assert hm(roll=edge) is not None or hm(roll=edge - 1e-9) is not None
    assert hm(width=1) is None and hm(width=0) is None and hm(width=65) is None and hm(width=64) is not None and hm(width=2) is not None
    assert hm(debug=True, text_size=65) is None and hm(debug=False, text_size=65) is not None
    assert hm(dtype=np.float32) is None and hm(dtype=np.float64) is None and hm(dtype=np.uint8) is not None
    assert render.plan_horizon_marks([(64, 80)], [[dict(vfov=1.0, pitch=0.1, roll=0.1, width=1)]]) is None
    # a float frame keeps the host route in the flows
    assert render._panel0_raw(np.zeros((8, 8, 3), np.float32), None) is None and render._panel0_raw(np.zeros((8, 8, 3), np.uint8), None) is not None
    # the end points are the reference's float64 values, truncated as C does
    m = hm(pitch=0.3, roll=-0.2)[0]
    ctr = 64 * (0.5 - 0.5 * np.tan(0.3) / np.tan(0.5))
    assert m[0].tolist() == [MR.LINE, MR.pack_rgb((0, 255, 0)), 0, int(ctr - 80 * np.tan(-0.2) / 2), 80, int(ctr + 80 * np.tan(-0.2) / 2), 3, 0]


def test_check_draw_marks_refuses_each_listed_argument():
    from spec_amd.engine import check_draw_marks
    geom, offs = [[8, 10, 0, 3]], [[0, 30]]
    marks = [[MR.STRIP, 0, 0, 4, 0, 0, 0, 0], [MR.MASK, 0xffffff, 1, 1, 4, 3, 2, 0], [MR.LINE, 255, 0, 3, 10, 5, 3, 0]]
    ok = lambda **kw: check_draw_marks(**{**dict(geom=geom, offsets=offs, marks=marks, slab_bytes=240, mask_bytes=14), **kw})
    g, o, m = ok()
    assert g.dtype == np.int32 and o.dtype == np.int64 and m.dtype == np.int64 and m.shape == (3, 8)
    ok(geom=[[8, 10, 0, 0]], marks=np.zeros((0, 8), np.int64))               # no marks at all is legal

    def edit(i, col, v):
        mm = np.array(marks, np.int64)
        mm[i, col] = v
        return mm
    refused = [
        dict(geom=np.zeros((0, 4))), dict(geom=np.tile(geom, (65536, 1)), offsets=np.tile(offs, (65536, 1))),
        dict(geom=[[0, 10, 0, 3]]), dict(geom=[[8, 8193, 0, 3]], offsets=[[0, 3 * 8193]], slab_bytes=1 << 30), dict(geom=[[8193, 10, 0, 3]], slab_bytes=1 << 30),
        dict(offsets=[[0, 29]]), dict(slab_bytes=239), dict(offsets=[[-1, 30]]), dict(offsets=[[1, 30]]),
        dict(geom=[[8, 10, 0, 3], [8, 10, 0, 0]], offsets=[[0, 60], [29, 60]], slab_bytes=1000),          # two frames share a byte
        dict(geom=[[8, 10, 1, 3]]), dict(geom=[[8, 10, -1, 2]]), dict(geom=[[8, 10, 0, -1]]),            # a mark range outside the record
        dict(marks=edit(0, 0, 3)), dict(marks=edit(0, 0, -1)), dict(marks=edit(0, 1, 1 << 24)),
        dict(marks=edit(2, 6, 1)), dict(marks=edit(2, 6, 65)),
        dict(marks=edit(2, 2, -100001)), dict(marks=edit(2, 5, 100001)),
        dict(mask_bytes=13), dict(marks=edit(1, 6, -1)), dict(marks=edit(1, 6, 3)),
        dict(marks=edit(1, 4, 0)), dict(marks=edit(1, 5, 8193), mask_bytes=1 << 20),
        dict(marks=edit(1, 2, 16384)), dict(marks=edit(1, 3, -16384)),
        dict(marks=np.zeros((3, 7), np.int64)),
    ]
    for kw in refused:
        with pytest.raises(ValueError):
            ok(**kw)
    ok(marks=edit(2, 2, -100000))
    ok(marks=edit(1, 2, -16383))
    ok(geom=[[8, 10, 0, 3], [8, 10, 0, 0]], offsets=[[0, 60], [30, 60]], slab_bytes=1000)  # side by side: no shared byte


def test_header_declares_the_exports():
    from spec_amd import _lib
    head = open(os.path.join(ROOT, 'include', 'specmi.h')).read()
    internal = open(os.path.join(ROOT, 'spec_amd', 'csrc', 'specmi_internal.h')).read()
    for name, nargs in (('specmi_draw_marks', 11), ('specmi_denormalize_u8', 15)):
        m = re.search(r'\bint ' + name + r'\(([^;]*)\);', head)
        assert m and len(m.group(1).split(',')) == nargs == len(_lib.PROTOTYPES[name][1])
    for k, v in (('SPECMI_MARK_STRIP', _lib.MARK_STRIP), ('SPECMI_MARK_MASK', _lib.MARK_MASK), ('SPECMI_MARK_LINE', _lib.MARK_LINE)):
        assert re.search(r'#define ' + k + r' ' + str(v) + r'\b', head)
    assert (MR.STRIP, MR.MASK, MR.LINE, MR.REC) == (_lib.MARK_STRIP, _lib.MARK_MASK, _lib.MARK_LINE, _lib.MARK_REC)
    assert re.search(r'kMarkStrip = 0, kMarkMask = 1, kMarkLine = 2, kMarkRec = 8;', internal)
    assert f'kMarkMaxCoord = {MR.LINE_MAX_COORD}' in internal and _lib.MARK_MAX_COORD == MR.LINE_MAX_COORD
    assert 'marks.hip' in open(os.path.join(ROOT, 'spec_amd', 'build.py')).read()


def test_denormalize_restatement():
    rng = np.random.default_rng(2)
    mean, std = np.asarray(MR.IMAGENET_MEAN, np.float32).reshape(3, 1, 1), np.asarray(MR.IMAGENET_STD, np.float32).reshape(3, 1, 1)
    u = rng.random((3, 37, 53), dtype=np.float32)                           # denormalised values in [0, 1)
    x = ((u - mean) / std).astype(np.float32)
    want = ((x * std + mean) * 255).astype('uint8').transpose(1, 2, 0)
    assert ((x * std + mean) * 255).min() >= 0 and ((x * std + mean) * 255).max() < 256
    assert np.array_equal(MR.denormalize_u8(x), want)
    edge = np.array([np.nan, -np.inf, np.inf, -5.0, 50.0, 0.0], np.float32).reshape(1, 1, 6).repeat(3, 0)
    assert MR.denormalize_u8(edge)[0, :, 0].tolist() == [0, 0, 255, 0, 255, int(np.float32(0.485) * np.float32(255))]
