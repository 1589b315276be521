"""The tensor checks of the picture wrappers (``Engine.render_views`` ... ``png_decode_into``): what each one refuses about its
slabs and its ``sizes`` / ``status`` vector before the library is reached, on CPU tensors and an engine without a library
(``tests.util.NoLibrary``).  The records themselves have their own host tests (``engine.check_*``).  No GPU."""
import numpy as np
import pytest
import torch

from spec_amd import _lib
from spec_amd.engine import Engine
from tests.util import NoLibrary


def u8(n):
    return torch.zeros(n, dtype=torch.uint8)


ONE = int(np.float32(1).view(np.int32))
# Every call works on 4 x 5 frames in slabs of a few dozen bytes; the encoders and decoders take two, so that (n,) has a stride.
# wrapper -> (a good call, its slab-like arguments, its (n,) vector and dtype or None, its contiguous uint8 arguments of any shape)
CASES = {
    'render_views': (lambda: dict(
        vertices=torch.zeros(1, 3, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32), cam_t=torch.zeros(1, 3), geom=[[4, 5, 0, 1, _lib.RENDER_CULL]],
        offsets=[[0, 15, 0, 15]], cams=[[1, 0, 0, 0, 1, 0, 0, 0, 1, 50., 50., 2., 2.]], in_slab=u8(60), out_slab=u8(60)), ('in_slab', 'out_slab'), None, ()),
    'draw_skeletons': (lambda: dict(kp=torch.zeros(1, 6, 3), slab=u8(60), geom=[[4, 5, 0, 1]], offsets=[[0, 15]], bones=[(0, 1)]), ('slab',), None, ()),
    'draw_marks': (lambda: dict(slab=u8(60), geom=[[4, 5, 0, 1]], offsets=[[0, 15]], marks=[[_lib.MARK_STRIP, 0, 0, 2, 0, 0, 0, 0]], masks=u8(14)),
                   ('slab', 'masks'), None, ()),
    'color_jitter': (lambda: dict(slab=u8(60), offsets=[0], sizes=[(4, 5)], records=np.array([[0, 1, 2, 3, ONE, ONE, ONE, 0]], np.int32), out=u8(60)),
                     ('slab', 'out'), None, ()),
    'denormalize_u8': (lambda: dict(x=torch.zeros(1, 3, 4, 5), index=0, H=4, W=5, slab=u8(60)), ('slab',), None, ()),
    'jpeg_encode_into': (lambda: dict(slab=u8(60), out_slab=u8(1400), geom=[[4, 5]] * 2, offsets=[[0, 15, 0, 700], [0, 15, 700, 700]],
                                      sizes=torch.zeros(2, dtype=torch.int64)),
                         ('slab', 'out_slab'), ('sizes', torch.int64), ()),
    'png_encode_into': (lambda: dict(slab=u8(60), out_slab=u8(140), geom=[[4, 5]] * 2, offsets=[[0, 15, 0, 70], [0, 15, 70, 70]],
                                     sizes=torch.zeros(2, dtype=torch.int64)),
                        ('slab', 'out_slab'), ('sizes', torch.int64), ()),
    'jpeg_decode_into': (lambda: dict(host=np.zeros(40, np.uint8), slab=u8(40), ranges=[[0, 20], [20, 20]], geom=[[4, 5, 444]] * 2, out_slab=u8(120),
                                      outs=[[0, 15], [60, 15]], status=torch.zeros(2, dtype=torch.int32)), ('slab', 'out_slab'), ('status', torch.int32), ()),
    'png_decode_into': (lambda: dict(slab=u8(40), ranges=[[0, 20], [20, 20]], geom=[[4, 5, 2]] * 2, out_slab=u8(120), outs=[[0, 15], [60, 15]],
                                     status=torch.zeros(2, dtype=torch.int32), raw=u8(512)), ('slab', 'out_slab'), ('status', torch.int32), ('raw',)),
}


def _call(name, **kw):
    return getattr(Engine, name)(NoLibrary(), **kw)


def _refused(name, **kw):
    with pytest.raises(ValueError):
        _call(name, **kw)


@pytest.mark.parametrize('name', sorted(CASES))
def test_a_good_call_reaches_the_library(name):
    with pytest.raises(AssertionError, match='the library was called'):
        _call(name, **CASES[name][0]())
    optional = {'render_views': (), 'draw_marks': ('masks',), 'color_jitter': ('out',), 'denormalize_u8': ('slab',)}.get(name, ('sizes', 'status', 'raw'))
    with pytest.raises(AssertionError, match='the library was called'):         # and so does one that leaves the optional tensors out
        _call(name, **{k: v for k, v in CASES[name][0]().items() if k not in optional})


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_slab_is_a_contiguous_1d_uint8_tensor(name):
    good, slabs, _, loose = CASES[name]
    for arg in slabs:
        t = good()[arg]
        for bad in (np.zeros(t.numel(), np.uint8), t.to(torch.int8), t.reshape(2, -1), u8(2 * t.numel())[::2]):
            _refused(name, **{**good(), arg: bad})
    for arg in loose:           # any shape, but still a contiguous uint8 tensor
        t = good()[arg]
        for bad in (np.zeros(t.numel(), np.uint8), t.to(torch.int8), u8(2 * t.numel())[::2]):
            _refused(name, **{**good(), arg: bad})


@pytest.mark.parametrize('name', sorted(k for k, c in CASES.items() if c[2]))
def test_sizes_and_status_are_contiguous_n_vectors_of_their_dtype(name):
    good, _, (arg, dtype), _ = CASES[name]
    other = torch.int32 if dtype == torch.int64 else torch.int64
    for bad in (np.zeros(2, np.int64), torch.zeros(2, dtype=other), torch.zeros(3, dtype=dtype), torch.zeros(2, 1, dtype=dtype), torch.zeros(4, dtype=dtype)[::2]):
        _refused(name, **{**good(), arg: bad})


def test_the_other_tensors_of_the_wrappers():
    """``kp``, ``x``, ``coef`` and the mesh inputs of ``render_views``: dtype, contiguity, rank."""
    good = CASES['draw_skeletons'][0]
    for bad in (np.zeros((1, 6, 3), np.float32), torch.zeros(1, 6, 3, dtype=torch.float64), torch.zeros(6, 3), torch.zeros(1, 6, 6)[:, :, ::2]):
        _refused('draw_skeletons', **{**good(), 'kp': bad})
    good = CASES['denormalize_u8'][0]
    for bad in (np.zeros((1, 3, 4, 5), np.float32), torch.zeros(1, 3, 4, 5, dtype=torch.float64), torch.zeros(3, 4, 5), torch.zeros(1, 4, 4, 5),
                torch.zeros(1, 3, 4, 10)[..., ::2]):
        _refused('denormalize_u8', **{**good(), 'x': bad})
    good = CASES['jpeg_decode_into'][0]
    with pytest.raises(AssertionError, match='the library was called'):
        _call('jpeg_decode_into', **good(), coef=torch.zeros(6, 64, dtype=torch.int16))
    for bad in (np.zeros(384, np.int16), torch.zeros(384, dtype=torch.int32), torch.zeros(768, dtype=torch.int16)[::2]):
        _refused('jpeg_decode_into', **good(), coef=bad)
    _refused('jpeg_decode_into', **{**good(), 'host': np.zeros(41, np.uint8)})
    good = CASES['render_views'][0]
    for arg, bads in (('vertices', (np.zeros((1, 3, 3), np.float32), torch.zeros(1, 3, 3, dtype=torch.float64), torch.zeros(3, 3), torch.zeros(1, 0, 3),
                                    torch.zeros(1, 3, 6)[..., ::2])),
                      ('cam_t', (np.zeros((1, 3), np.float32), torch.zeros(1, 3, dtype=torch.float64), torch.zeros(2, 3), torch.zeros(1, 6)[:, ::2])),
                      ('faces', (np.zeros((1, 3), np.int32), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int32),
                                 torch.zeros(0, 3, dtype=torch.int32), torch.zeros(1, 6, dtype=torch.int32)[:, ::2]))):
        for bad in bads:
            _refused('render_views', **{**good(), arg: bad})
    _refused('render_views', **{**good(), 'in_slab': None})          # the view names a frame
    slab = u8(120)
    _refused('render_views', **{**good(), 'in_slab': slab[:60], 'out_slab': slab[59:119]})          # the slabs overlap
    _refused('color_jitter', **{**CASES['color_jitter'][0](), 'slab': slab[:60], 'out': slab[59:119]})
