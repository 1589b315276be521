"""Pre-processing on the device.

Crop + normalise: the detection loop of ``spec/tester.py:116-128``
(``get_single_image_crop_demo`` per bbox, ``bbox_scale = bbox[2]/200``, ``bbox_center``) as one
HIP launch (``specmi_crop_normalize``) from a uint8 RGB frame that already sits in HBM.

Every producer takes ``dtype=torch.float32`` (the (n,3,H,W) image the reference builds) or ``dtype=torch.float16``: the same
values rounded once to fp16 in the NHWC8 layout (n,H,W,8) the fp16 trunk reads (include/specmi.h, the ``_f16`` exports) - bit
for bit what the fp32 image becomes inside an fp16 forward, without the fp32 image.  Any other dtype raises ``ValueError``."""
from __future__ import annotations

import torch

from . import _lib
from .cam_utils import _engine
from .engine import _dev_f32, _image_out, _ptr, image_tensor, out_dtype


def _frame_arg(name, t):
    """One frame for the producer ``name``: an (H,W,3) uint8 device tensor -> contiguous."""
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise RuntimeError(f'{name} needs a device tensor (no CPU path in spec_amd)')
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f'{name}: frame must be (H,W,3) uint8 RGB')
    return t.contiguous()


def _slab_arg(name, t):
    """A slab of equal-sized frames for the producer ``name``: a contiguous (F,H,W,3) uint8 device tensor."""
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise RuntimeError(f'{name} needs a device tensor (no CPU path in spec_amd)')
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or not t.is_contiguous():
        raise ValueError(f'{name}: frames must be a contiguous (F,H,W,3) uint8 RGB slab')
    return t


def _boxes_arg(dets, dev):
    boxes = _dev_f32(dets, dev)
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError('dets must be (n,4) [cx, cy, w, h]')
    return boxes


@torch.no_grad()
def crop_detections(frame_rgb_u8, dets, scale: float = 1.0, crop_size: int = 224, return_raw: bool = False, out=None,
                    dtype=torch.float32):
    """frame (H,W,3) uint8 device tensor, dets (n,4) [cx, cy, w, h] ->
    dict(inp_images (n,3,S,S) fp32, bbox_scale (n,), bbox_center (n,2)[, raw (n,S,S,3) uint8]).
    ``out``: optional dict of preallocated contiguous tensors (``inp_images``, ``bbox_scale``, ``bbox_center`` - e.g. slices
    of a larger batch buffer) to write into instead of allocating.  ``dtype=torch.float16``: ``inp_images`` is (n,S,S,8) NHWC8
    fp16 (the batch call with one frame)."""
    f16 = out_dtype(dtype)
    frame = _frame_arg('crop_detections', frame_rgb_u8)
    eng = _engine(frame.device)
    dev = eng.device
    boxes = _boxes_arg(dets, dev)
    n, (H, W) = boxes.shape[0], frame.shape[:2]
    img, sc, ce = _crop_outputs(out, n, crop_size, dev, f16)
    raw = torch.empty(n, crop_size, crop_size, 3, device=dev, dtype=torch.uint8) if return_raw else None
    if n > 0 and f16:       # one frame, no index (NULL = every crop from frame 0)
        _lib.check(eng.h, eng.lib.specmi_crop_normalize_batch_f16(eng.h, _ptr(frame), 1, H, W, None, _ptr(boxes), n, float(scale),
                                                                  crop_size, _ptr(img), _ptr(raw), _ptr(sc), _ptr(ce), eng._stream()))
    elif n > 0:
        _lib.check(eng.h, eng.lib.specmi_crop_normalize(eng.h, _ptr(frame), H, W, _ptr(boxes), n, float(scale), crop_size,
                                                        _ptr(img), _ptr(raw), _ptr(sc), _ptr(ce), eng._stream()))
    res = {'inp_images': img, 'bbox_scale': sc, 'bbox_center': ce}
    if return_raw:
        res['raw'] = raw
    return res


def _crop_outputs(out, n, crop_size, dev, f16=False):
    if out is None:
        return (image_tensor(n, crop_size, crop_size, dev, f16),
                torch.empty(n, device=dev, dtype=torch.float32), torch.empty(n, 2, device=dev, dtype=torch.float32))
    img, sc, ce = _image_out(out['inp_images'], n, crop_size, crop_size, f16, dev), out['bbox_scale'], out['bbox_center']
    for t_, shp, dt in ((sc, (n,), torch.float32), (ce, (n, 2), torch.float32)):
        if tuple(t_.shape) != shp or t_.dtype != dt or not t_.is_contiguous() or t_.device != dev:
            raise ValueError(f'out tensor must be a contiguous {dt} device tensor of shape {shp}, got {tuple(t_.shape)} {t_.dtype}')
    return img, sc, ce


@torch.no_grad()
def crop_detections_batch(frames_u8, frame_index, dets, scale: float = 1.0, crop_size: int = 224, out=None, dtype=torch.float32):
    """The detections of MANY equal-sized frames in one launch (``specmi_crop_normalize_batch``): ``frames_u8`` (F,H,W,3) uint8
    device slab, ``frame_index`` (n,) int32 (which frame each detection belongs to), ``dets`` (n,4) [cx, cy, w, h] -> the same
    dict as ``crop_detections`` for all n crops, bit-identical to cutting them frame by frame.  ``dtype=torch.float16``:
    ``inp_images`` is (n,S,S,8) NHWC8 fp16 (``specmi_crop_normalize_batch_f16``)."""
    f16 = out_dtype(dtype)
    frames_u8 = _slab_arg('crop_detections_batch', frames_u8)
    eng = _engine(frames_u8.device)
    dev = eng.device
    boxes = _boxes_arg(dets, dev)
    n = boxes.shape[0]
    fidx = frame_index if isinstance(frame_index, torch.Tensor) else torch.as_tensor(frame_index)
    F, H, W = frames_u8.shape[:3]
    if fidx.device.type == 'cpu' and fidx.numel():
        # still on the host: check the range here (the kernel clamps what reaches it - a wrong crop instead of an
        # out-of-bounds read - but cannot report it)
        lo, hi = int(fidx.min()), int(fidx.max())
        if lo < 0 or hi >= F:
            raise ValueError(f'frame_index values must lie in [0, {F}), got [{lo}, {hi}]')
    fidx = fidx.to(device=dev, dtype=torch.int32).contiguous()
    if fidx.shape != (n,):
        raise ValueError('frame_index must have one entry per detection')
    img, sc, ce = _crop_outputs(out, n, crop_size, dev, f16)
    if n > 0:
        fn = eng.lib.specmi_crop_normalize_batch_f16 if f16 else eng.lib.specmi_crop_normalize_batch
        _lib.check(eng.h, fn(eng.h, _ptr(frames_u8), F, H, W, _ptr(fidx), _ptr(boxes), n, float(scale), crop_size, _ptr(img), None, _ptr(sc),
                             _ptr(ce), eng._stream()))
    return {'inp_images': img, 'bbox_scale': sc, 'bbox_center': ce}


def pack_frames(frames, device=None):
    """Host frames of different sizes -> one slab, the input convention of the ragged calls (``specmi_resize_normalize_ragged``,
    ``specmi_crop_normalize_ragged``, ``specmi_crop_resize_normalize_ragged``): a list of (H,W,3) uint8 arrays ->
    (1-D uint8 slab holding them back to back, (n,) int64 byte offsets, [(H, W)]).  ``device=None``: the slab stays a host
    array; else it is uploaded in ONE copy and returned as a tensor on ``device``."""
    import numpy as np
    frames = list(frames)
    if not frames:
        raise ValueError('at least one frame')
    sizes, offsets, off = [], [], 0
    for fr in frames:
        if not isinstance(fr, np.ndarray) or fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
            raise ValueError('frames must be (H,W,3) uint8 RGB')
        H, W = fr.shape[:2]
        sizes.append((int(H), int(W)))
        offsets.append(off)
        off += H * W * 3
    slab = np.concatenate([np.ascontiguousarray(fr).reshape(-1) for fr in frames])
    if device is not None:
        slab = torch.from_numpy(slab).to(device)
    return slab, np.asarray(offsets, dtype=np.int64), sizes


def _host_rgb(item):
    """A frame on the host route: a path or a file's ``bytes`` -> Pillow's (H,W,3) uint8 RGB, what ``tester._read_rgb`` and
    ``evaluation.read_image_rgb`` return; an array passes."""
    import io
    import numpy as np
    from PIL import Image
    if isinstance(item, np.ndarray):
        return item
    with Image.open(io.BytesIO(item) if isinstance(item, (bytes, bytearray)) else item) as im:
        return np.array(im.convert('RGB'))


def decode_frames(paths, device, jpeg_decode_device=None, png_decode_device=None):
    """The frames of a batch from their files -> the triple ``pack_frames([Pillow's decode of each], device)`` returns, bit for
    bit.  ``paths``: per frame a path, a file's ``bytes`` already read, or a decoded (H,W,3) uint8 array.  ``jpeg_decode_device``
    (None = ``engine.JPEG_DECODE_DEVICE_DEFAULT``): False is exactly that host path; True sends the baseline .jpg / .jpeg files
    ``engine.jpeg_probe`` calls supported up as BYTES in one copy and decodes them in one ``specmi_jpeg_decode`` into their
    places of the slab.  ``png_decode_device`` (None = ``engine.PNG_DECODE_DEVICE_DEFAULT``) does the same for the .png files
    ``engine.png_probe`` calls supported: their zlib streams go up and one ``specmi_png_decode`` writes them into their places of
    the same slab.  Every other frame - a file its probe refuses, a file whose status came back non-zero, an array - is decoded
    by Pillow as before and uploaded into its place of the same slab (a damaged file raises there what it raises today)."""
    import numpy as np
    from .engine import (flow_jpeg_decode_device, flow_png_decode_device, is_jpeg_name, is_png_name, jpeg_probe, png_probe, png_stream,
                         png_takes_device)
    items = list(paths)
    if not items:
        raise ValueError('at least one frame')
    jpeg_on, png_on = flow_jpeg_decode_device(jpeg_decode_device), flow_png_decode_device(png_decode_device)
    if not jpeg_on and not png_on:
        return pack_frames([_host_rgb(p) for p in items], device)
    dev = torch.device(device)
    eng = _engine(dev)
    files, pngs, sizes, host = {}, {}, [None] * len(items), {}

    def classify(p):
        """-> ('png', file, probe, zlib stream) | ('jpeg', file, probe) | ('host', item): reads the file; a PNG's CRC walk and the
        join of its IDAT payloads are done here, so that a batch's files share the host's threads as the host route's decodes do"""
        is_bytes = isinstance(p, (bytes, bytearray))
        named = not is_bytes and not isinstance(p, np.ndarray)
        if is_bytes or (named and ((jpeg_on and is_jpeg_name(p)) or (png_on and is_png_name(p)))):
            if not is_bytes:
                with open(p, 'rb') as f:
                    p = f.read()
            if png_on and p[:4] == b'\x89PNG':
                probe = png_probe(p)
                if png_takes_device(probe):
                    return 'png', bytes(p), probe, png_stream(p, probe[4])
            elif jpeg_on:
                probe = jpeg_probe(p)
                if probe[0] == 'supported':
                    return 'jpeg', bytes(p), probe
        return 'host', p

    if png_on and len(items) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(16, len(items))) as ex:
            kinds = list(ex.map(classify, items))
    else:
        kinds = [classify(p) for p in items]
    for i, k in enumerate(kinds):
        if k[0] == 'png':
            pngs[i], sizes[i] = k[1:], (k[2][1], k[2][2])
            continue
        if k[0] == 'jpeg':
            files[i], sizes[i] = k[1:], (k[2][1], k[2][2])
            continue
        p = k[1]
        host[i] = _host_rgb(p)
        if host[i].dtype != np.uint8 or host[i].ndim != 3 or host[i].shape[2] != 3:
            raise ValueError('frames must be (H,W,3) uint8 RGB')
        sizes[i] = (int(host[i].shape[0]), int(host[i].shape[1]))
    nbytes = np.array([3 * h * w for h, w in sizes], np.int64)
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    slab = torch.empty(int(nbytes.sum()), device=eng.device, dtype=torch.uint8)
    if files:
        order = sorted(files)
        length = np.array([len(files[i][0]) for i in order], np.int64)
        ranges = np.stack([np.concatenate([[0], np.cumsum(length)[:-1]]), length], axis=1)
        blob = np.frombuffer(b''.join(files[i][0] for i in order), np.uint8)
        geom = np.array([files[i][1][1:] for i in order], np.int64)
        status, _ = eng.jpeg_decode_into(blob, torch.from_numpy(blob.copy()).to(eng.device), ranges, geom, slab,
                                         np.stack([offsets[order], 3 * geom[:, 1]], axis=1))
        for i, st in zip(order, status.cpu().tolist()):
            if st:                                            # a scan that does not satisfy T.81: the host route decides
                host[i] = _host_rgb(files[i][0])
                if tuple(host[i].shape) != sizes[i] + (3,):
                    raise ValueError('a damaged file decodes to another size on the host')
    if pngs:
        order = sorted(pngs)
        streams = [pngs[i][2] for i in order]
        short = [i for i, s in zip(order, streams) if len(s) < 8]             # no zlib stream at all: the host route decides
        order, streams = [i for i in order if i not in short], [s for s in streams if len(s) >= 8]
        for i in short:
            host[i] = _host_rgb(pngs[i][0])
        if order:
            length = np.array([len(s) for s in streams], np.int64)
            ranges = np.stack([np.concatenate([[0], np.cumsum(length)[:-1]]), length], axis=1)
            geom = np.array([pngs[i][1][1:4] for i in order], np.int64)
            blob = torch.from_numpy(np.frombuffer(bytearray().join(streams), np.uint8)).to(eng.device)
            status = eng.png_decode_into(blob, ranges, geom, slab, np.stack([offsets[order], 3 * geom[:, 1]], axis=1))
            for i, st in zip(order, status.cpu().tolist()):
                if st:                                            # a stream that does not satisfy RFC 1950 / 1951: the host route decides
                    host[i] = _host_rgb(pngs[i][0])
    for i, fr in host.items():
        if tuple(fr.shape) != tuple(sizes[i]) + (3,):
            raise ValueError('a damaged file decodes to another size on the host')
    for i, fr in host.items():
        slab[int(offsets[i]):int(offsets[i] + nbytes[i])].copy_(torch.from_numpy(np.ascontiguousarray(fr)).reshape(-1))
    return slab, offsets, [(int(h), int(w)) for h, w in sizes]


def _ragged_args(name, slab, offsets, sizes, frame_index, n):
    """The frame side of the ragged crop ``name``, checked in this order: the host tables (one offset and one (H, W) per
    frame), ``frame_index`` against the number of frames while it is still on the host - ``crop_detections_batch``'s check -,
    then the slab (1-D uint8 device tensor).  -> (engine, slab, offsets int64, geom (F,2) int32, frame_index on the device)."""
    import numpy as np
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    geom = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 2)
    F = geom.shape[0]
    if F < 1 or offsets.shape[0] != F:
        raise ValueError(f'{name}: one offset and one (H, W) per frame (at least one frame)')
    fidx = frame_index if isinstance(frame_index, torch.Tensor) else torch.as_tensor(np.asarray(frame_index))
    if fidx.device.type == 'cpu' and fidx.numel():
        lo, hi = int(fidx.min()), int(fidx.max())
        if lo < 0 or hi >= F:
            raise ValueError(f'frame_index values must lie in [0, {F}), got [{lo}, {hi}]')
    if tuple(fidx.shape) != (n,):
        raise ValueError(f'{name}: frame_index must have one entry per crop')
    if not isinstance(slab, torch.Tensor) or slab.device.type != 'cuda':
        raise RuntimeError(f'{name} needs a device tensor (no CPU path in spec_amd)')
    if slab.dtype != torch.uint8 or slab.dim() != 1 or not slab.is_contiguous():
        raise ValueError(f'{name}: slab must be a contiguous 1-D uint8 tensor')
    eng = _engine(slab.device)
    return eng, slab, offsets, geom, fidx.to(device=eng.device, dtype=torch.int32).contiguous()


@torch.no_grad()
def crop_detections_ragged(slab, offsets, sizes, frame_index, dets, scale: float = 1.0, crop_size: int = 224, out=None,
                           dtype=torch.float32):
    """The detections of MANY frames of DIFFERENT sizes in one launch (``specmi_crop_normalize_ragged``): ``slab`` 1-D uint8
    device tensor holding the (H,W,3) frames, ``offsets`` (F,) byte offsets and ``sizes`` [(H, W)] on the host (``pack_frames``
    makes all three), ``frame_index`` (n,) int32, ``dets`` (n,4) [cx, cy, w, h] -> the same dict as ``crop_detections_batch``,
    bit-identical to ``crop_detections`` frame by frame.  ``dtype=torch.float16``: NHWC8 fp16 crops.  A call whose offsets or
    sizes differ from the previous call's synchronises the device (include/specmi.h): not for use under graph capture."""
    f16 = out_dtype(dtype)
    n = len(dets)
    eng, slab, offsets, geom, fidx = _ragged_args('crop_detections_ragged', slab, offsets, sizes, frame_index, n)
    dev = eng.device
    boxes = _boxes_arg(dets, dev)
    img, sc, ce = _crop_outputs(out, n, crop_size, dev, f16)
    if n > 0:
        fn = eng.lib.specmi_crop_normalize_f16_ragged if f16 else eng.lib.specmi_crop_normalize_ragged
        _lib.check(eng.h, fn(eng.h, _ptr(slab), slab.numel(), offsets.ctypes.data_as(_lib.c_int64_p), geom.ctypes.data_as(_lib.c_int32_p),
                             geom.shape[0], _ptr(fidx), _ptr(boxes), n, float(scale), crop_size, _ptr(img), None, _ptr(sc), _ptr(ce),
                             eng._stream()))
    return {'inp_images': img, 'bbox_scale': sc, 'bbox_center': ce}


@torch.no_grad()
def dataset_crops_ragged(slab, offsets, sizes, frame_index, centers, scales, crop_size: int = 224, dtype=torch.float32, out=None):
    """``dataset_crops`` for the samples of a batch whose images differ in size, in one launch
    (``specmi_crop_resize_normalize_ragged``): slab / offsets / sizes / frame_index as in ``crop_detections_ragged``, centers
    (n,2), scales (n,) -> (n,3,S,S) fp32 or (n,S,S,8) NHWC8 fp16, bit-identical to ``dataset_crops`` sample by sample.  The
    boxes still come from ``pare_crop_boxes`` on the host.  ``out``: the batch tensor to write into."""
    f16 = out_dtype(dtype)
    host_boxes = pare_crop_boxes(centers, scales, crop_size)
    n = host_boxes.shape[0]
    eng, slab, offsets, geom, fidx = _ragged_args('dataset_crops_ragged', slab, offsets, sizes, frame_index, n)
    boxes = torch.from_numpy(host_boxes).to(eng.device)
    out = _image_out(out, n, crop_size, crop_size, f16, eng.device)
    if n > 0:
        fn = eng.lib.specmi_crop_resize_normalize_f16_ragged if f16 else eng.lib.specmi_crop_resize_normalize_ragged
        _lib.check(eng.h, fn(eng.h, _ptr(slab), slab.numel(), offsets.ctypes.data_as(_lib.c_int64_p), geom.ctypes.data_as(_lib.c_int32_p),
                             geom.shape[0], _ptr(fidx), _ptr(boxes), n, crop_size, _ptr(out), eng._stream()))
    return out


def pare_crop_boxes(centers, scales, res: int = 224):
    """Integer crop boxes of pare's ``crop(img, center, scale, [res, res])`` (SPIN / PARE image_utils): ``ul = transform([1, 1],
    ..., invert=1) - 1``, ``br = transform([res + 1, res + 1], ..., invert=1) - 1`` with ``transform`` = 3x3 float64 matrix
    (``h = 200 * scale``), ``np.linalg.inv``, ``.astype(int)`` (truncation toward zero) - restated with the same NumPy calls.
    -> (n,4) int32 [ul_x, ul_y, br_x, br_y]."""
    import numpy as np
    out = []
    for c, sc in zip(np.asarray(centers, dtype=np.float64).reshape(-1, 2), np.asarray(scales, dtype=np.float64).reshape(-1)):
        h = 200 * sc
        t = np.zeros((3, 3))
        t[0, 0] = float(res) / h
        t[1, 1] = float(res) / h
        t[0, 2] = res * (-float(c[0]) / h + .5)
        t[1, 2] = res * (-float(c[1]) / h + .5)
        t[2, 2] = 1
        ti = np.linalg.inv(t)

        def tr(pt):
            new_pt = np.dot(ti, np.array([pt[0] - 1, pt[1] - 1, 1.]).T)
            return new_pt[:2].astype(int) + 1
        ul = np.array(tr([1, 1])) - 1
        br = np.array(tr([res + 1, res + 1])) - 1
        out.append([ul[0], ul[1], br[0], br[1]])
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


@torch.no_grad()
def dataset_crops(frame_rgb_u8, centers, scales, crop_size: int = 224, dtype=torch.float32):
    """The evaluation dataset's image path on the device (spec/dataset/cam_dataset.py:253-287,367-377): pare ``crop`` (integer
    box copy + cv2.resize bilinear) + clip + ``/ 255`` + ImageNet Normalize.  frame (H,W,3) uint8 device tensor, centers (n,2),
    scales (n,) (bbox height / 200) -> (n,3,S,S) fp32, or (n,S,S,8) NHWC8 fp16 with ``dtype=torch.float16``."""
    f16 = out_dtype(dtype)
    frame = _frame_arg('dataset_crops', frame_rgb_u8)
    eng = _engine(frame.device)
    boxes = torch.from_numpy(pare_crop_boxes(centers, scales, crop_size)).to(eng.device)
    n, (H, W) = boxes.shape[0], frame.shape[:2]
    out = image_tensor(n, crop_size, crop_size, eng.device, f16)
    fn = eng.lib.specmi_crop_resize_normalize_f16 if f16 else eng.lib.specmi_crop_resize_normalize
    _lib.check(eng.h, fn(eng.h, _ptr(frame), H, W, _ptr(boxes), n, crop_size, _ptr(out), eng._stream()))
    return out


def resize_output_size(w: int, h: int, min_size: int = 600):
    """``torchvision.transforms.Resize(min_size)`` geometry: shorter side -> min_size, longer ->
    ``int(min_size * long / short)``.  Returns (ow, oh)."""
    if w <= h:
        return min_size, int(min_size * h / w)
    return int(min_size * w / h), min_size


@torch.no_grad()
def camcalib_transform(frame_rgb_u8, min_size: int = 600, return_raw: bool = False, dtype=torch.float32):
    """The CamCalib demo's ``ImageFolder`` transform (``camcalib/pano_dataset.py:156-162``): Resize(600) of
    the PIL image (Pillow's antialiased bilinear), ToTensor, ImageNet Normalize - one HIP launch
    (``specmi_resize_normalize``), bit-identical to Pillow + torchvision.  frame (H,W,3) uint8 device tensor ->
    (1,3,oh,ow) fp32 [, (oh,ow,3) uint8]; ``dtype=torch.float16``: (1,oh,ow,8) NHWC8 fp16 (``specmi_resize_normalize_f16``)."""
    f16 = out_dtype(dtype)
    frame = _frame_arg('camcalib_transform', frame_rgb_u8)
    eng = _engine(frame.device)
    H, W = frame.shape[:2]
    ow, oh = resize_output_size(W, H, min_size)
    out = image_tensor(1, oh, ow, eng.device, f16)
    raw = torch.empty(oh, ow, 3, device=eng.device, dtype=torch.uint8) if return_raw else None
    fn = eng.lib.specmi_resize_normalize_f16 if f16 else eng.lib.specmi_resize_normalize
    _lib.check(eng.h, fn(eng.h, _ptr(frame), H, W, oh, ow, _ptr(out), _ptr(raw), eng._stream()))
    return (out, raw) if return_raw else out


@torch.no_grad()
def camcalib_transform_batch(frames_u8, min_size: int = 600, out=None, dtype=torch.float32):
    """``camcalib_transform`` for a slab of F equal-sized frames: (F,H,W,3) uint8 device -> (F,3,oh,ow) fp32, one
    ``specmi_resize_normalize`` launch per frame into ONE batch tensor (CamCalib then runs once on all F frames instead of once
    per frame, ``scripts/camcalib_demo.py:95-102``); each frame's pixels are bit-identical to the single-frame call.
    ``dtype=torch.float16``: (F,oh,ow,8) NHWC8 fp16."""
    f16 = out_dtype(dtype)
    frames_u8 = _slab_arg('camcalib_transform_batch', frames_u8)
    eng = _engine(frames_u8.device)
    F, H, W = frames_u8.shape[:3]
    ow, oh = resize_output_size(W, H, min_size)
    out = _image_out(out, F, oh, ow, f16, eng.device)
    fn = eng.lib.specmi_resize_normalize_f16 if f16 else eng.lib.specmi_resize_normalize
    for f in range(F):
        _lib.check(eng.h, fn(eng.h, _ptr(frames_u8[f]), H, W, oh, ow, _ptr(out[f]), None, eng._stream()))
    return out
