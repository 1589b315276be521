"""The two crops at the edges of their one per-pixel path, against the oracle (oracle/preprocess.py: crop_detections, dataset_crop).

The kernel for frames of one size and the ragged kernel of a crop call the same prologue and the same per-pixel function, so
"ragged equals per-frame" (tests/test_gpu_ragged_crops.py) no longer separates two statements of the arithmetic.  Here every
route is compared with the NumPy restatement of the reference, ``np.array_equal``, where the code takes another path: frames
below the 8-byte tap load (W < 2 or fewer than 8 bytes) and the smallest that take it, a partial workgroup (S = 8), a second
workgroup that starts in the middle of a row (S = 46: 2116 = 2048 + 68 pixels), a crop beyond the coordinate tables (S = 2049),
the empty box, and the NHWC8 fp16 store of all of them."""
import numpy as np
import pytest
import torch

from oracle import preprocess as OP
from spec_amd import _lib, cam_utils
from spec_amd.engine import _ptr
from spec_amd.preprocess import (crop_detections, crop_detections_batch, crop_detections_ragged, dataset_crops, dataset_crops_ragged,
                                 pack_frames, pare_crop_boxes)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SIZES = [(1, 1), (1, 7), (2, 1), (3, 2), (37, 53)]      # the first three: narrow loads; (3, 2) = 18 bytes: the smallest wide one
BIG = 4                                                 # the frame that also serves S = 2049
SLABS = (3, BIG)                                        # frames that get two more of their size for the equal-size batch call
CROP_SIZES = (8, 33, 46, 2049)
NORM_ZERO = (np.float32(0) - OP.MEAN) / OP.STD


def _frames_of(S):
    return [BIG] if S > 46 else list(range(len(SIZES)))         # a 2049 x 2049 oracle crop takes a second: one frame only


@pytest.fixture(scope='module')
def world():
    rng = np.random.default_rng(46)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SIZES]
    slab, offsets, sizes = pack_frames(frames, DEV)
    # the equal-size slabs: the frame between two others of its size
    same = {f: [rng.integers(0, 256, frames[f].shape, dtype=np.uint8), frames[f], rng.integers(0, 256, frames[f].shape, dtype=np.uint8)]
            for f in SLABS}
    return {'frames': frames, 'dev': [torch.from_numpy(fr).to(DEV) for fr in frames], 'slab': slab, 'offsets': offsets, 'sizes': sizes,
            'same': same, 'same_dev': {f: torch.from_numpy(np.stack(v)).to(DEV) for f, v in same.items()}}


def _demo_boxes(H, W):
    """[cx, cy, w, h]: centred and 1.3 times the longer side, 2.5 times the frame, centred at (-0.5, -0.5) and mostly outside,
    a fractional centre with w != h"""
    L = float(max(H, W))
    return np.asarray([[W / 2, H / 2, 1.3 * L, 1.3 * L], [W / 2, H / 2, 2.5 * W, 2.5 * H], [-0.5, -0.5, L, L],
                       [0.37 * W + 0.25, 0.61 * H + 0.125, 0.8 * W + 0.3, 0.55 * H + 0.7]], np.float32)


def _dataset_boxes(H, W):
    """(centre x, centre y, scale) of a box inside the frame, half outside, wholly outside, and of the 1 x 1 box [0, 0, 1, 1]"""
    m = min(H, W)
    return np.asarray([[(W + 1) / 2, (H + 1) / 2, max(0.6 * m, 1) / 200 + 0.001], [0.0, (H + 1) / 2, (m + 1) / 200],
                       [-3.0 * W - 50, -3.0 * H - 50, 0.1], [1.0, 1.0, 0.002]], np.float64)


def _f16_equals(got, ref32):
    """(n,S,S,8) NHWC8 halves against the (n,3,S,S) fp32 reference: channels 0-2 rounded once, channels 3-7 the bit pattern 0"""
    g = got.cpu().numpy()
    return np.array_equal(g[..., :3], ref32.transpose(0, 2, 3, 1).astype(np.float16)) and not g[..., 3:].view(np.uint16).any()


def _demo_equals(got, ref, sel=slice(None), raw=True):
    imgs, raws, sc, ce = (r[sel] for r in ref)
    ok = np.array_equal(got['bbox_scale'].cpu().numpy(), sc) and np.array_equal(got['bbox_center'].cpu().numpy(), ce)
    if raw:
        ok = ok and np.array_equal(got['raw'].cpu().numpy(), raws)
    if got['inp_images'].dtype == torch.float16:
        return ok and _f16_equals(got['inp_images'], imgs)
    return ok and np.array_equal(got['inp_images'].cpu().numpy(), imgs)


@pytest.mark.parametrize('scale', [1.0, 1.1])
@pytest.mark.parametrize('S', CROP_SIZES)
def test_demo_crop_equals_the_oracle_on_every_route(world, S, scale):
    use = _frames_of(S)
    boxes = {f: _demo_boxes(*SIZES[f]) for f in use}
    ref = {f: OP.crop_detections(world['frames'][f], boxes[f], scale, S) for f in use}
    for dtype in (torch.float32, torch.float16):
        # one frame per call
        for f in use:
            got = crop_detections(world['dev'][f], boxes[f], scale=scale, crop_size=S, return_raw=True, dtype=dtype)
            assert _demo_equals(got, ref[f]), (SIZES[f], dtype)
            del got
        # a slab of three frames of one size: the frame's crops and, at the small sizes, its neighbours' (listed first and last)
        for f in (f for f in SLABS if f in use):
            three = world['same'][f]
            parts = [(1, boxes[f], ref[f])]
            if S <= 46:
                parts = [(2, boxes[f][:2], OP.crop_detections(three[2], boxes[f][:2], scale, S))] + parts + \
                        [(0, boxes[f][2:], OP.crop_detections(three[0], boxes[f][2:], scale, S))]
            fidx = np.concatenate([np.full(len(b), i, np.int32) for i, b, _ in parts])
            want = [np.concatenate([r[k] for _, _, r in parts]) for k in range(4)]
            got = crop_detections_batch(world['same_dev'][f], fidx, np.concatenate([b for _, b, _ in parts]), scale=scale, crop_size=S,
                                        dtype=dtype)
            assert _demo_equals(got, want, raw=False), (SIZES[f], dtype)
            del got
        # all five frames in one slab, the crops listed out of frame order
        fidx = np.asarray([f for f in use for _ in boxes[f]], np.int32)
        dets = np.concatenate([boxes[f] for f in use])
        want = [np.concatenate([ref[f][k] for f in use]) for k in range(4)]
        order = np.random.default_rng(S).permutation(len(fidx))
        got = crop_detections_ragged(world['slab'], world['offsets'], world['sizes'], fidx[order], dets[order], scale=scale, crop_size=S,
                                     dtype=dtype)
        assert _demo_equals(got, want, order, raw=False), dtype
        del got


@pytest.mark.parametrize('S', CROP_SIZES)
def test_dataset_crop_equals_the_oracle_on_both_routes(world, S):
    use = _frames_of(S)
    cs = {f: _dataset_boxes(*SIZES[f]) for f in use}
    for f in use:       # the boxes are what their names say
        (H, W), b = SIZES[f], pare_crop_boxes(cs[f][:, :2], cs[f][:, 2], S)
        assert (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
        assert b[0, 0] >= 0 and b[0, 1] >= 0 and b[0, 2] <= W and b[0, 3] <= H
        assert b[1, 0] < 0 < b[1, 2] and (b[2, 2] <= 0 and b[2, 3] <= 0) and list(b[3]) == [0, 0, 1, 1]
    ref = {f: np.stack([OP.dataset_crop(world['frames'][f], c[:2], c[2], S) for c in cs[f]]) for f in use}
    for f in use:
        assert np.array_equal(ref[f][2], np.broadcast_to(NORM_ZERO.reshape(3, 1, 1), (3, S, S)))       # wholly outside: all zeros
    fidx = np.asarray([f for f in use for _ in cs[f]], np.int32)
    allc, want = np.concatenate([cs[f] for f in use]), np.concatenate([ref[f] for f in use])
    order = np.random.default_rng(S).permutation(len(fidx))
    for dtype in (torch.float32, torch.float16):
        equals = _f16_equals if dtype == torch.float16 else (lambda got, r: np.array_equal(got.cpu().numpy(), r))
        for f in use:
            assert equals(dataset_crops(world['dev'][f], cs[f][:, :2], cs[f][:, 2], S, dtype=dtype), ref[f]), (SIZES[f], dtype)
        got = dataset_crops_ragged(world['slab'], world['offsets'], world['sizes'], fidx[order], allc[order, :2], allc[order, 2], S,
                                   dtype=dtype)
        assert equals(got, want[order]), dtype
        del got


@pytest.mark.parametrize('S', CROP_SIZES)
def test_an_empty_box_is_normalised_zero(world, S):
    """br <= ul in x only, in y only and in both.  spec_amd.preprocess computes the box from a centre and a scale, so the four
    entry points are called with the box tensor as a C caller would: every pixel is Normalize(0), and no frame is read."""
    eng = cam_utils._engine(torch.device(DEV))
    boxes = torch.tensor([[5, 5, 5, 9], [7, 5, 3, 9], [5, 5, 9, 5], [5, 9, 9, 2], [5, 5, 5, 5], [9, 9, 2, 2]], dtype=torch.int32, device=DEV)
    n, (H, W) = len(boxes), SIZES[BIG]
    fidx = torch.tensor([4, 0, 3, 1, 2, 4], dtype=torch.int32, device=DEV)
    geom = np.ascontiguousarray(world['sizes'], np.int32)
    offsets = np.ascontiguousarray(world['offsets'], np.int64)
    want = np.broadcast_to(NORM_ZERO.reshape(1, 3, 1, 1), (n, 3, S, S))
    for f16 in (False, True):
        for ragged in (False, True):
            out = torch.full((n, S, S, 8), 7.0, dtype=torch.float16, device=DEV) if f16 else torch.full((n, 3, S, S), 7.0, device=DEV)
            if ragged:
                fn = eng.lib.specmi_crop_resize_normalize_f16_ragged if f16 else eng.lib.specmi_crop_resize_normalize_ragged
                rc = fn(eng.h, _ptr(world['slab']), world['slab'].numel(), offsets.ctypes.data_as(_lib.c_int64_p),
                        geom.ctypes.data_as(_lib.c_int32_p), len(SIZES), _ptr(fidx), _ptr(boxes), n, S, _ptr(out), eng._stream())
            else:
                fn = eng.lib.specmi_crop_resize_normalize_f16 if f16 else eng.lib.specmi_crop_resize_normalize
                rc = fn(eng.h, _ptr(world['dev'][BIG]), H, W, _ptr(boxes), n, S, _ptr(out), eng._stream())
            _lib.check(eng.h, rc)
            assert _f16_equals(out, want) if f16 else np.array_equal(out.cpu().numpy(), want), (f16, ragged)
            del out
