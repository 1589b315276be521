"""``SPECTester`` on MI355X - the class ``scripts/spec_demo.py`` of the reference drives (``spec/tester.py:39-176``),
with the same constructor argument (an argparse namespace: ``cfg``, ``ckpt``, ``no_save``, ...), attributes (``model``,
``model_cfg``, ``device``) and methods (``run_camcalib``, ``run_detector``, ``run_on_image_folder``) and the same files on
disk (``<out>/camcalib/<image name>.pkl``, ``<out>/spec_results/<stem>.pkl``).

Differences by design: ``run_camcalib`` runs CamCalib in this process on the GPU instead of spawning
``python scripts/camcalib_demo.py`` (tester.py:86-88) - the drop-in ``scripts/camcalib_demo.py`` wraps the same function; the
crops of ``run_on_image_folder`` are cut on the device (``specmi_crop_normalize``); the person detector (multi-person-tracker /
YOLOv3, tester.py:73-84) is outside the path: ``run_detector`` reads boxes from ``args.detections`` (joblib: list or
``{image name: (n,4) [cx, cy, w, h]}``).  The three-panel pictures (:165-201) are drawn by this project's own rasteriser on the
device (``spec_amd/render.py``; same geometry and file names, its own declared shading - not pyrender's look) when ``args.no_render``
is present and false; a frame's detections are drawn together, one launch sequence per panel, and that picture is written under
each detection's name.  ``args.render_each`` writes the reference's pictures instead: file ``{stem}_{i:06d}`` shows detection i alone."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

from . import assets, cam_utils, io_formats, render
from .checkpoint import load_pretrained_model, read_checkpoint
from .modules import HMR, CameraRegressorNetwork
from .engine import (flow_image_dtype, flow_jpeg_decode_device, flow_jpeg_device, flow_png_device, flow_ragged_crops, flow_render_batch, image_tensor,
                     is_jpeg_name, is_png_name, jpeg_probe, flow_png_decode_device, png_probe, png_takes_device)
from .preprocess import camcalib_transform, crop_detections, crop_detections_ragged, decode_frames, pack_frames

CAMCALIB_CKPT = 'data/camcalib/checkpoints/camcalib_sa_biased_l2.ckpt'     # scripts/camcalib_demo.py:39
IMG_EXT = ('.png', '.jpg', '.jpeg')


def _log(*a):
    print(*a, file=sys.stderr, flush=True)


def _ns(d):
    return SimpleNamespace(**{k: _ns(v) if isinstance(v, dict) else v for k, v in d.items()})


def update_hparams(cfg_file):
    """``spec/config.py: update_hparams`` for the keys the tester reads (HMR.BACKBONE, HMR.USE_CAM_FEATS, DATASET.IMG_RES,
    TRAINING.PRETRAINED): the yacs YAML merged over the reference's defaults, attribute access like a CfgNode."""
    from .evaluation import load_config
    hp = load_config(cfg_file if cfg_file and os.path.exists(cfg_file) else None)
    hp['TRAINING'].setdefault('PRETRAINED', None)
    return _ns(hp)


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def _read_frame(path, jpeg=True, png=False):
    """A decode-ahead thread's work with a device decode on: the bytes of a .jpg / .jpeg file ``specmi_jpeg_decode`` takes
    (``engine.jpeg_probe``; ``jpeg``) or of a .png file ``specmi_png_decode`` takes (``engine.png_probe``; ``png``); every other
    frame - a progressive or greyscale JPEG, a palette PNG - is decoded here, on the thread, as before."""
    if not ((jpeg and is_jpeg_name(path)) or (png and is_png_name(path))):
        return _read_rgb(path)
    with open(path, 'rb') as f:
        data = f.read()
    if data[:4] == b'\x89PNG':
        return data if png and png_takes_device(png_probe(data)) else _read_rgb(path)
    return data if jpeg and jpeg_probe(data)[0] == 'supported' else _read_rgb(path)


def list_images(image_folder):
    return sorted(os.path.join(image_folder, x) for x in os.listdir(image_folder) if x.endswith(IMG_EXT))


@torch.no_grad()
def run_camcalib_folder(img_folder, out_folder, ckpt=CAMCALIB_CKPT, loss_type='softargmax_l2', model=None, device='cuda', log=_log):
    """The loop of ``scripts/camcalib_demo.py:95-174`` for an image folder: full frame -> Resize(600) transform on the
    device -> CamCalib -> ``convert_preds_to_angles`` -> ``f_pix = h/2/tan(vfov/2)`` -> one ``<name>.pkl`` per image with
    ``{'vfov', 'f_pix', 'pitch', 'roll'}``.  Returns {image path: record}."""
    import joblib
    dev = torch.device(device)
    if model is None:
        model = CameraRegressorNetwork(backbone='resnet50', num_fc_layers=1, num_fc_channels=1024).to(dev)
        model = load_pretrained_model(model, read_checkpoint(ckpt)['state_dict'], remove_lightning=True, strict=True)
        log('Loaded pretrained model')
    model.eval()
    os.makedirs(out_folder, exist_ok=True)
    log('Running CamCalib')
    results = {}
    for img_fname in [f for f in list_images(img_folder) if not os.path.basename(f).startswith('.')]:
        frame = torch.from_numpy(_read_rgb(img_fname)).to(dev)
        orig_h = frame.shape[0]
        preds = model(camcalib_transform(frame, 600, dtype=flow_image_dtype(model)))
        if loss_type in ('kl', 'ce'):
            vfov, pitch, roll = (np.asarray(a).squeeze() for a in cam_utils.convert_preds_to_angles(*preds, loss_type=loss_type, return_type='np'))
        else:
            vfov, pitch, roll = (a.detach().cpu().numpy().squeeze() for a in cam_utils.convert_preds_to_angles(*preds, loss_type=loss_type))
        rec = {'vfov': vfov, 'f_pix': orig_h / 2. / np.tan(vfov / 2.), 'pitch': pitch, 'roll': roll}
        joblib.dump(rec, os.path.join(out_folder, os.path.basename(img_fname) + '.pkl'))
        results[img_fname] = rec
    return results


class SPECTester:
    def __init__(self, args):
        self.args = args
        self.model_cfg = update_hparams(getattr(args, 'cfg', None))
        if not torch.cuda.is_available():
            raise RuntimeError('spec_amd runs on an AMD GPU (torch device "cuda"); there is no CPU path')
        self.device = torch.device('cuda')
        if getattr(args, 'synthetic_assets', False):
            assets.use_synthetic_assets(1003)
        self.model = self._build_model()
        self._load_pretrained_model()
        self.model.eval()
        self._camcalib = getattr(args, 'camcalib_model', None)
        self._fp32_crops = None       # False: NHWC8 fp16 crops for a model at fp16; True: fp32 crops + in-trunk conversion (same bits)
        self._jpeg_decode_device = None     # True: on the ragged route without pictures the frames' files go up as bytes and are decoded on the device (preprocess.decode_frames; same bits); None = engine.JPEG_DECODE_DEVICE_DEFAULT
        self._png_decode_device = None      # the same for the frames' .png files (specmi_png_decode; same bits); None = engine.PNG_DECODE_DEVICE_DEFAULT
        self._ragged_crops = None     # True: a flush's frames in one slab, one upload, one ragged crop launch; False: one of each per frame (same bits)
        self._render_batch = None     # True: a flush's pictures in one render_image_groups call; False: one render_image_group per frame (same bytes)
        self._jpeg_device = None      # True: .jpg / .jpeg pictures are encoded on the device and only the files' bytes come down (same bytes)
        self._png_device = None       # True: .png pictures are encoded on the device and only the files' bytes come down (the same picture, other bytes than Pillow's); None = engine.PNG_DEVICE_DEFAULT (off)
        self._panel0_device = None    # True: the horizon line and caption of panel 0 are drawn on the device, uint8 frames go up raw (same bytes)

    def _build_model(self):
        c = self.model_cfg
        return HMR(backbone=c.HMR.BACKBONE, img_res=c.DATASET.IMG_RES, pretrained=c.TRAINING.PRETRAINED,
                   use_cam_feats=c.HMR.USE_CAM_FEATS, use_cam=True).to(self.device)

    def _load_pretrained_model(self):
        if self.args.ckpt == 'spin':
            _log('CKPT file is not provided, using SPIN weights')
        elif isinstance(self.args.ckpt, dict):                       # an in-memory state dict (tests, synthetic demo)
            load_pretrained_model(self.model, self.args.ckpt, overwrite_shape_mismatch=True, remove_lightning=True)
        else:
            _log(f'Loading pretrained model from {self.args.ckpt}')
            ckpt = read_checkpoint(self.args.ckpt)['state_dict']
            load_pretrained_model(self.model, ckpt, overwrite_shape_mismatch=True, remove_lightning=True)
            _log(f'Loaded pretrained weights from "{self.args.ckpt}"')

    def run_detector(self, image_folder):
        det = getattr(self.args, 'detections', None)
        if det is None:
            raise NotImplementedError('the person detector / tracker (multi-person-tracker, YOLOv3: spec/tester.py:73-84) is '
                                      'outside the hot path; pass --detections <joblib file> with the boxes ([cx, cy, w, h] per person)')
        import joblib
        boxes = joblib.load(det) if isinstance(det, str) else det
        if isinstance(boxes, dict):
            return [np.asarray(boxes.get(os.path.basename(f), boxes.get(f, [])), np.float32).reshape(-1, 4) for f in list_images(image_folder)]
        return [np.asarray(b, np.float32).reshape(-1, 4) for b in boxes]

    def _crop_held(self, held, pending, buf, img_h, img_w, R, K, output_path, res, crop_dtype):
        """The ragged route of ``run_on_image_folder`` for one flush: ``held`` [(RGB array, detections)] and ``pending``
        [(image, first crop, crops)] name the same frames in the same order.  With the device decode on, ``held`` holds the files'
        bytes instead of RGB arrays: ``decode_frames`` takes either and gives the same slab."""
        import joblib
        k = pending[-1][1] + pending[-1][2]
        slab, offsets, sizes = decode_frames([rgb for rgb, _ in held], self.device, any(isinstance(rgb, bytes) for rgb, _ in held),
                                             any(isinstance(rgb, bytes) and rgb[:4] == b'\x89PNG' for rgb, _ in held))
        counts = [n for _, _, n in pending]
        crop_detections_ragged(slab, offsets, sizes, np.repeat(np.arange(len(held), dtype=np.int32), counts),
                               np.concatenate([dets for _, dets in held]), scale=1.0, crop_size=res, dtype=crop_dtype,
                               out={key: v[:k] for key, v in buf.items()})                           # tester.py:116-128
        recs = [joblib.load(io_formats.camcalib_result_path(output_path, f)) for f, _, _ in pending]     # io_formats.read_cam_params
        per_crop = lambda vals: np.repeat(np.asarray(vals, np.float32), counts)
        h, w = per_crop([s[0] for s in sizes]), per_crop([s[1] for s in sizes])
        img_h[:k], img_w[:k] = torch.from_numpy(h).to(self.device), torch.from_numpy(w).to(self.device)
        R[:k], K[:k] = cam_utils.cam_params_from_angles(per_crop([r['pitch'].item() for r in recs]), per_crop([r['roll'].item() for r in recs]),
                                                        per_crop([float(r['f_pix']) for r in recs]), w, h, device=self.device)

    def _frame_camera(self, img_fname, shape, output_path):
        """What the pictures of one frame are drawn with (``spec/tester.py:169-175``): the render rotation
        ``batch_euler2matrix([-pitch, 0, roll])`` = Rx(-pitch) Rz(roll), the frame's f_pix twice, the centre (W // 2, H // 2) and
        the horizon line's (vfov, pitch, roll, f_pix)."""
        import joblib
        rec = joblib.load(io_formats.camcalib_result_path(output_path, img_fname))
        pitch, roll, vfov, f_pix = rec['pitch'].item(), rec['roll'].item(), rec['vfov'].item(), float(rec['f_pix'])
        cp, sp, cr, sr = np.cos(-pitch), np.sin(-pitch), np.cos(roll), np.sin(roll)
        rot = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
        h, w = shape[:2]
        return rot.astype(np.float32), (f_pix, f_pix), (w // 2, h // 2), np.array([vfov, pitch, roll, f_pix])

    def _write_pictures(self, img_fname, pictures, vertices, output_path, output_img_folder):
        """The files of one frame: ``pictures[i]`` (a PIL image, or the ``bytes`` of a file encoded on the device) under detection
        i's name, and with ``args.save_obj`` its mesh."""
        stem, ext = os.path.splitext(os.path.basename(img_fname))
        os.makedirs(output_img_folder, exist_ok=True)
        written = []
        for i in range(vertices.shape[0]):
            written.append(os.path.join(output_img_folder, f'{stem}_{i:06d}{ext}'))
            if isinstance(pictures[i], bytes):
                with open(written[-1], 'wb') as f:
                    f.write(pictures[i])
            else:
                pictures[i].save(written[-1])
            if getattr(self.args, 'save_obj', False):
                mesh_folder = os.path.join(output_path, 'meshes', os.path.basename(img_fname).split('.')[0])
                os.makedirs(mesh_folder, exist_ok=True)
                render.write_obj(os.path.join(mesh_folder, f'{i:06d}.obj'), vertices[i].cpu().numpy() * np.array([1., -1., -1.], np.float32),
                                 assets.faces())
        return written

    def _render_frame(self, img_fname, rgb, vertices, cam_t, output_path, output_img_folder, keypoints=None):
        """``spec/tester.py:165-201`` for one frame: ``vertices`` (n, V, 3) / ``cam_t`` (n, 3) as the step left them on the device.
        The render rotation is ``batch_euler2matrix([-pitch, 0, roll])`` = Rx(-pitch) Rz(roll) (:169-171), the focal length the
        frame's f_pix, the centre (W // 2, H // 2) (:175).  ``keypoints`` (n, 49, 2): the detections' 2D skeletons, drawn on the device
        (``args.draw_keypoints``).  -> the files written."""
        from PIL import Image
        rot, focal, center, cam_params = self._frame_camera(img_fname, rgb.shape, output_path)
        group = render.render_image_group(rgb, cam_t, vertices, rot, focal, center, cam_params=cam_params, device=self.device, keypoints_2d=keypoints,
                                          panel0_device=self._panel0_device)
        if flow_jpeg_device(self._jpeg_device) and is_jpeg_name(img_fname):       # encoded once, written once per detection
            H, W3 = int(group.shape[0]), int(group.shape[1])
            picture = cam_utils._engine(group.device).jpeg_encode(group.view(-1), [[H, W3]], [[0, 3 * W3]], 75)[0]
        elif flow_png_device(self._png_device) and is_png_name(img_fname):
            H, W3 = int(group.shape[0]), int(group.shape[1])
            picture = cam_utils._engine(group.device).png_encode(group.view(-1), [[H, W3]], [[0, 3 * W3]])[0]
        else:
            picture = Image.fromarray(group.cpu().numpy())
        return self._write_pictures(img_fname, [picture] * vertices.shape[0], vertices, output_path, output_img_folder)

    def _render_flush(self, pending, frames, vertices, cam_t, output_path, output_img_folder, each, keypoints=None):
        """``_render_frame`` for every frame of a flush in one ``render_image_groups`` call: ``pending`` [(image, first crop,
        crops)] and ``frames`` (the RGB arrays) in the same order, ``vertices`` / ``cam_t`` the flush's detections on the device.
        Same file names, same bytes; ``each``: file i of a frame shows detection i alone (spec/tester.py:181-201) - with
        ``keypoints`` (the flush's (k, 49, 2) 2D joints) its own skeleton alone.  With ``self._jpeg_device`` the pictures of
        ``.jpg`` / ``.jpeg`` frames come back from that call as the bytes of their files (``encode='jpeg'``, Pillow's default
        quality 75), with ``self._png_device`` those of ``.png`` frames (``encode='png'``); a frame's shared picture is encoded once
        and written once per detection."""
        from PIL import Image
        on_jpeg, on_png = flow_jpeg_device(self._jpeg_device), flow_png_device(self._png_device)
        encode = [('jpeg' if on_jpeg and is_jpeg_name(f) else 'png' if on_png and is_png_name(f) else None) for f, _, _ in pending]
        as_picture = lambda p: p if isinstance(p, bytes) else Image.fromarray(p)
        cams = [self._frame_camera(f, rgb.shape, output_path) for (f, _, _), rgb in zip(pending, frames)]
        counts = [n for _, _, n in pending]
        groups = render.render_image_groups(frames, vertices, cam_t, counts, [c[0] for c in cams], [c[1] for c in cams], [c[2] for c in cams],
                                            cam_params=[c[3] for c in cams], each=each, device=self.device, keypoints_2d=keypoints, encode=encode,
                                            panel0_device=self._panel0_device)
        written, g = [], 0
        for img_fname, k0, n in pending:
            pictures = [as_picture(p) for p in groups[g:g + n]] if each else [as_picture(groups[g])] * n
            g += n if each else 1
            written += self._write_pictures(img_fname, pictures, vertices[k0:k0 + n], output_path, output_img_folder)
        return written

    def run_camcalib(self, image_folder, output_folder):
        return run_camcalib_folder(image_folder, f'{output_folder}/camcalib', ckpt=getattr(self.args, 'camcalib_ckpt', None) or CAMCALIB_CKPT,
                                   model=self._camcalib, device=self.device)

    @torch.no_grad()
    def run_on_image_folder(self, image_folder, detections, output_path, output_img_folder, bbox_scale=1.0):
        """``spec/tester.py:90-163`` with the per-frame loop flattened: frames are decoded ahead on host threads, uploaded
        from pinned memory without blocking, their detections are cropped on the device straight into ONE batch buffer,
        and the model runs once per ``args.frame_batch`` crops (default 256) instead of once per frame.  Within one execution
        plan (``args.plan``: 'throughput' | 'latency' | 'auto', see ``spec_amd.modules._EngineModule.set_plan``) an image's
        outputs do not depend on the batch it travels in (every kernel of the path has a fixed summation order), so with the
        plan pinned the per-frame ``spec_results/<stem>.pkl`` files are bit-identical to ``frame_batch=1``, the reference's
        own structure (one deterministic result per image, ``spec/tester.py:143-163``).  Default (round 5): ONE plan for the
        whole run whatever ``frame_batch`` is - 'throughput' - so the files do not depend on how the frames were batched; the
        choice is logged.  ``--plan auto`` buys the lowest per-frame latency (single / latency plan by detection count) at the
        price of last bits that depend on the batch (contract: 1e-4).
        Decode-ahead is bounded: at most 2 x ``args.decode_threads`` decoded frames wait in host memory (the reference holds
        one frame at a time; an unbounded queue would keep a whole video folder in RAM when decoding outruns the GPU).
        ``self._ragged_crops`` (None = ``engine.RAGGED_CROPS_DEFAULT``): the decoded frames of one flush are held on the host -
        at most ``frame_batch`` of them, on top of the decode window -, packed into one slab, uploaded once and cut by ONE
        ``crop_detections_ragged`` call; ``img_h``, ``img_w`` and the angles behind ``R`` / ``K`` are gathered on the host and go
        up once per flush.  Same crops, same files, bit for bit.
        ``self._render_batch`` (None = ``engine.RENDER_BATCH_DEFAULT``), with ``args.no_render`` false: the pictures of one flush
        are drawn by ONE ``render.render_image_groups`` call - one slab up, one ``specmi_render_views`` call, one slab down per
        chunk - instead of one ``render_image_group`` per frame.  Same file names, same bytes.  ``args.render_each`` (implies the
        batched route): file ``{stem}_{i:06d}`` shows detection i alone, as the reference draws it, instead of the frame's
        detections together.  ``args.draw_keypoints``: the predicted ``smpl_joints2d`` of each frame's detections are drawn onto
        the frame as 2D skeletons before the mesh is laid over it (``render.draw_skeleton``: on the device, this project's own
        drawing contract), on both routes; with ``render_each`` each picture shows its own detection's skeleton alone.  Off by
        default: the pictures are then unchanged.
        ``self._jpeg_device`` (None = ``engine.JPEG_DEVICE_DEFAULT``): the pictures of ``.jpg`` / ``.jpeg`` frames are encoded on
        the device (``specmi_jpeg_encode``, Pillow's default quality 75) and only the files' bytes come down, on both routes; a
        ``.png`` frame keeps the host route.  Same files, byte for byte.
        ``self._panel0_device`` (None = ``engine.PANEL0_DEVICE_DEFAULT``): the horizon line and caption of panel 0 are drawn on
        the device (``specmi_draw_marks``) instead of with Pillow on the host, on both routes.  Same files, byte for byte."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        image_file_names = list_images(image_folder)
        res = self.model_cfg.DATASET.IMG_RES
        cap = max(1, int(getattr(self.args, 'frame_batch', 256) or 1))
        per_frame = cap <= 1                                             # the reference's structure: one forward per frame
        plan = getattr(self.args, 'plan', None)
        if not plan:
            plan = 'throughput'
            _log("execution plan: 'throughput' for the whole run (results bit-identical for any --frame_batch; "
                 "--plan auto = lowest latency per forward, last bits then depend on the batch size)")
        else:
            _log(f"execution plan: '{plan}' (pinned by --plan)")
        self.model.set_plan(plan)
        dev = self.device
        todo = [(i, f) for i, f in enumerate(image_file_names) if len(detections[i]) >= 1]
        if not todo:
            return 0
        cap = max(cap, max(len(detections[i]) for i, _ in todo))       # a frame's detections stay in one batch
        crop_dtype = flow_image_dtype(self.model, self._fp32_crops)
        buf = {'inp_images': image_tensor(cap, res, res, dev, crop_dtype == torch.float16), 'bbox_scale': torch.empty(cap, device=dev),
               'bbox_center': torch.empty(cap, 2, device=dev)}
        img_w, img_h = torch.empty(cap, device=dev), torch.empty(cap, device=dev)
        R, K = torch.empty(cap, 3, 3, device=dev), torch.empty(cap, 3, 3, device=dev)
        ragged = flow_ragged_crops(self._ragged_crops)
        held = []                     # ragged route: (RGB array, detections) of the frames waiting for this flush
        pending, k, n_done = [], 0, 0
        save = not getattr(self.args, 'no_save', False)
        render = not getattr(self.args, 'no_render', True)            # absent = no pictures, as before there were any
        render_each = bool(getattr(self.args, 'render_each', False))
        draw_kp = bool(getattr(self.args, 'draw_keypoints', False))
        render_batch = render_each or flow_render_batch(self._render_batch)     # the per-detection pictures come from the batched call only
        if render and output_img_folder is None:
            raise ValueError('no_render is false: output_img_folder must name the folder the pictures go to')
        shown = {}                    # rendering: the decoded frames of this flush by file name
        if save:
            os.makedirs(os.path.join(output_path, 'spec_results'), exist_ok=True)

        def flush():
            nonlocal k, pending
            if k == 0:
                return
            if ragged:
                self._crop_held(held, pending, buf, img_h, img_w, R, K, output_path, res, crop_dtype)
                held.clear()
            output = self.model(buf['inp_images'][:k], cam_rotmat=R[:k], cam_intrinsics=K[:k], bbox_scale=buf['bbox_scale'][:k],
                                bbox_center=buf['bbox_center'][:k], img_w=img_w[:k], img_h=img_h[:k])
            joints2d = output['smpl_joints2d'][:k].contiguous() if render and draw_kp else None      # (k, 49, 2), full-image pixels
            if render and render_batch:
                self._render_flush(pending, [shown.pop(f) for f, _, _ in pending], output['smpl_vertices'][:k], output['pred_cam_t'][:k],
                                   output_path, output_img_folder, render_each, keypoints=joints2d)
            elif render:
                for img_fname, k0, n in pending:
                    self._render_frame(img_fname, shown.pop(img_fname), output['smpl_vertices'][k0:k0 + n], output['pred_cam_t'][k0:k0 + n],
                                       output_path, output_img_folder, keypoints=None if joints2d is None else joints2d[k0:k0 + n])
            output = {key: v.cpu().numpy() for key, v in output.items()}          # ONE device->host hand-over per batch
            if save:
                import joblib
                for img_fname, k0, n in pending:
                    save_f = os.path.join(output_path, 'spec_results',
                                          os.path.basename(img_fname).replace(img_fname.split('.')[-1], 'pkl'))
                    joblib.dump({key: v[k0:k0 + n].copy() for key, v in output.items()}, save_f)
            k, pending = 0, []

        nthreads = int(getattr(self.args, 'decode_threads', 4) or 1)
        # pictures are drawn on the decoded host frame (shown): with them the host decode stays; without, the threads only read the
        # bytes of the files the device decodes
        jdec, pdec = flow_jpeg_decode_device(self._jpeg_decode_device), flow_png_decode_device(self._png_decode_device)
        read = (lambda path: _read_frame(path, jdec, pdec)) if ragged and not render and (jdec or pdec) else _read_rgb

        def decoded(ex):
            """(todo entry, RGB array) in order, at most 2 x nthreads frames decoded ahead of the consumer"""
            window, it = deque(), iter(todo)
            for entry in it:
                window.append((entry, ex.submit(read, entry[1])))
                if len(window) >= 2 * nthreads:
                    e, fut = window.popleft()
                    yield e, fut.result()
            while window:
                e, fut = window.popleft()
                yield e, fut.result()

        with ThreadPoolExecutor(max_workers=nthreads) as ex:
            for (img_idx, img_fname), rgb in decoded(ex):
                dets = np.asarray(detections[img_idx], np.float32).reshape(-1, 4)
                n = len(dets)
                if k + n > cap:
                    flush()
                if ragged:                                # cropped at the flush (_crop_held)
                    held.append((rgb, dets))
                else:
                    frame = torch.from_numpy(rgb).pin_memory().to(dev, non_blocking=True)
                    orig_height, orig_width = frame.shape[:2]
                    crop_detections(frame, dets, scale=1.0, crop_size=res, dtype=crop_dtype,           # tester.py:116-128
                                    out={key: v[k:k + n] for key, v in buf.items()})
                    img_h[k:k + n] = float(orig_height)
                    img_w[k:k + n] = float(orig_width)
                    cam_rotmat, cam_intrinsics, *_ = io_formats.read_cam_params(output_path, img_fname, (orig_height, orig_width),
                                                                                device=dev)
                    R[k:k + n] = cam_rotmat
                    K[k:k + n] = cam_intrinsics
                pending.append((img_fname, k, n))
                if render:
                    shown[img_fname] = rgb
                k += n
                if per_frame:
                    flush()
                n_done += 1
            flush()
        return n_done
