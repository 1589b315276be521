"""Labelled perspective views out of equirectangular panoramas - the reference's dataset generator for CamCalib
(camcalib/datagen/generateCalibrationDataset.py:58-160 ``makeAndSaveImg`` + camcalib/datagen/image_extraction.py:28-161
``extractImage``) as a source of validation data for the test step (spec_amd/camcalib_eval.py):

* ``sample_cameras`` restates the generator's camera distribution (yaw, aspect ratio, focal length, horizon, roll, portrait
  flip, resolution) over a ``numpy.random.Generator``;
* ``extract_views`` cuts the views out of a device-resident panorama in one launch (``specmi_pano_extract_views``);
* ``PanoViewDataset`` presents the interface ``camcalib_eval.run_evaluation`` reads from ``PanoValDataset`` and hands a
  batch over as a device slab, which ``specmi_resize_normalize_ragged`` consumes where it lies;
* ``write_tree`` stores the same views in the ``pano_scalenet`` layout (``images/NAME.jpg`` at quality 95, ``NAME.json``,
  ``val_images.pkl``) that this project's and the reference's loaders read.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

# camcalib/datagen/generateCalibrationDataset.py:28-34,58-62 ('myDistWider20200403')
ASPECT_RATIOS = (1 / 1, 5 / 4, 4 / 3, 3 / 2, 16 / 9)
AR_PROBABILITIES = (0.09, 0.01, 0.66, 0.20, 0.04)
HORIZON_MU, HORIZON_SIGMA, HORIZON_LOWER, HORIZON_UPPER = 0.523, 0.3, -1.0, 0.95
ROLL_MU, ROLL_SIGMA, ROLL_SIGMA_LOW, ROLL_LOWER, ROLL_UPPER = 0.0, 0.1, 0.001, -np.pi / 6, np.pi / 6
FOCAL_MU, FOCAL_SIGMA, FOCAL_SHAPE, FOCAL_LOWER, FOCAL_UPPER = 14, 17, 0.8, 12, 100
PORTRAIT_PROBABILITY = (0.80, 0.20)
LOW_ROLL_PROBABILITY = 0.33
RES_Y, MIN_RES_X = 600, 256
VIEWS_PER_PANO = 12


def sample_cameras(n: int, rng: np.random.Generator) -> List[dict]:
    """``n`` cameras from ``makeAndSaveImg``'s distribution (:73-117).  The reference draws from numpy's global, unseeded
    generator (and scipy's ``lognorm`` / ``cauchy`` on top of it), so the distribution is the contract, not a sequence:

    * yaw uniform in [-pi, pi); aspect ratio from the table above;
    * focal length 14 + 17 * lognormal(0, 0.8) mm, clipped to [12, 100] and redrawn until strictly inside;
    * horizon normal(0.523, 0.3), redrawn until inside (-1, 0.95); pitch = -atan((horizon - 0.5) / (focal / 24));
    * roll Cauchy around 0 with scale 0.001 (one third of the cameras) or 0.1, redrawn until inside (-pi/6, pi/6);
    * vfov = 2 atan2(sensor, 2 focal) with the 35 mm format's short side 24 - or, for the 20 % portrait cameras, its long
      side 36 and the inverse aspect ratio;
    * resY = 600 (the view's height), resX = int(resY / ratio), and if that is below 256: resX = 256, resY = int(resX * ratio).

    Each entry holds ``pitch, yaw, roll, vfov`` (radians), ``ratio`` (width / height), ``resY, resX`` and ``json``: the
    fields the reference writes next to the image - with its swapped ``"height": resX, "width": resY`` - except ``imgname``."""
    cams = []
    for _ in range(int(n)):
        sensor_size = 24
        yaw = float(rng.uniform(-np.pi, np.pi))
        ar = float(rng.choice(ASPECT_RATIOS, p=AR_PROBABILITIES))
        focal = np.inf
        while not FOCAL_LOWER < focal < FOCAL_UPPER:
            focal = float(np.clip(FOCAL_MU + FOCAL_SIGMA * rng.lognormal(0.0, FOCAL_SHAPE), FOCAL_LOWER, FOCAL_UPPER))
        horizon = float(rng.normal(HORIZON_MU, HORIZON_SIGMA))
        while not HORIZON_LOWER < horizon < HORIZON_UPPER:
            horizon = float(rng.normal(HORIZON_MU, HORIZON_SIGMA))
        scale = ROLL_SIGMA_LOW if rng.random() < LOW_ROLL_PROBABILITY else ROLL_SIGMA
        roll = np.inf
        while not ROLL_LOWER < roll < ROLL_UPPER:
            roll = float(ROLL_MU + scale * rng.standard_cauchy())
        vfov = 2 * float(np.arctan2(sensor_size, 2 * focal))
        fl_px = focal / sensor_size
        pitch = -float(np.arctan((horizon - 0.5) / fl_px))
        is_portrait = bool(rng.choice(2, p=PORTRAIT_PROBABILITY))
        if is_portrait:
            ar = 1 / ar
            sensor_size = 36
            vfov = 2 * float(np.arctan2(sensor_size, 2 * focal))
        res_y = RES_Y
        res_x = int(res_y / ar)
        if res_x < MIN_RES_X:
            res_x = MIN_RES_X
            res_y = int(res_x * ar)
        cams.append({'pitch': pitch, 'yaw': yaw, 'roll': roll, 'vfov': vfov, 'ratio': ar, 'resY': res_y, 'resX': res_x,
                     'is_portrait': is_portrait,
                     'json': {'yaw': yaw, 'pitch': pitch, 'roll': roll, 'vfov': vfov, 'focal_length_35mm_eq': focal, 'f_px': fl_px,
                              'height': res_x, 'width': res_y, 'sensor_size': sensor_size, 'horizon': horizon}})
    return cams


def view_size(height: int, ratio: float):
    """``extractImage``'s ``croppedSize`` (image_extraction.py:81,133): (height, round(height / (1 / ratio))), Python's round."""
    return int(height), int(round(height / (1.0 / ratio)))


def camera_views(cams: Sequence[dict]):
    """-> ((n, 5) float64 [elevation, azimuth, roll, vfov in degrees, ratio], heights) as ``makeAndSaveImg`` calls
    ``extractImage`` (:122-126): [pitch, yaw, roll], resY, vfov * 180 / pi, ratio."""
    views = np.asarray([[c['pitch'], c['yaw'], c['roll'], c['vfov'] * 180 / np.pi, c['ratio']] for c in cams], np.float64).reshape(-1, 5)
    return views, [int(c['resY']) for c in cams]


def as_rgb(pano: np.ndarray) -> np.ndarray:
    """A grey panorama replicated to three channels, channels beyond the third dropped (generateCalibrationDataset.py:179-183)."""
    pano = np.asarray(pano)
    if pano.dtype != np.uint8 or pano.ndim not in (2, 3):
        raise ValueError('a panorama is an (H, W) or (H, W, C) uint8 array')
    pano = np.stack((pano,) * 3, axis=-1) if pano.ndim == 2 else pano[:, :, :3]
    if pano.shape[2] != 3:
        raise ValueError(f'a panorama with {pano.shape[2]} channels')
    return np.ascontiguousarray(pano)


def read_panorama(path: str) -> np.ndarray:
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None                 # panoramas are large (the reference lifts the limit as well)
    with Image.open(path) as im:
        if im.mode not in ('L', 'RGB', 'RGBA'):
            im = im.convert('RGB')
        return as_rgb(np.array(im))


def extract_views(pano: torch.Tensor, views, heights, engine=None) -> List[torch.Tensor]:
    """``extractImage(pano, [elevation, azimuth, roll], height, vfov, ratio)`` for every row of ``views`` (n, 5: elevation,
    azimuth, roll in radians, vfov in degrees, ratio) in one launch.  ``pano``: (PH, PW, 3) uint8 device tensor.  -> n
    (H, W, 3) uint8 device tensors, views of ONE 1-D slab (``.slab``, ``.offsets`` on the returned list) laid out the way
    ``specmi_resize_normalize_ragged`` reads it."""
    from . import cam_utils
    if not isinstance(pano, torch.Tensor) or pano.device.type != 'cuda':
        raise ValueError('pano must be a device tensor: the extractor has no host path')
    eng = engine or cam_utils._engine(pano.device)
    views = np.ascontiguousarray(views, dtype=np.float64).reshape(-1, 5)
    heights = [int(h) for h in np.asarray(heights).reshape(-1)]
    if len(heights) != views.shape[0] or not heights:
        raise ValueError('one height per view (at least one view)')
    hw = [view_size(h, float(r)) for h, r in zip(heights, views[:, 4])]
    slab, offsets = eng.pano_extract_views(pano, views, hw)
    out = ViewList(slab[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offsets.tolist(), hw))
    out.slab, out.offsets, out.sizes = slab, offsets, hw
    return out


class ViewList(list):
    """The views of one extraction and the slab they share."""
    slab: torch.Tensor
    offsets: np.ndarray
    sizes: list


class PanoViewDataset:
    """Validation data generated from panoramas: ``views_per_pano`` cameras per file from ``sample_cameras`` (all drawn at
    construction from ``seed``), presenting what ``run_evaluation`` reads from ``PanoValDataset`` - length, ``imgname``,
    ``labels`` in 'pano_scalenet' units (vfov in radians), ``frame`` - plus ``device_batch``, which hands consecutive views
    over as one device slab.  The views of one panorama are cut in one launch when the first of them is asked for and kept
    until another panorama's are."""
    name = 'pano_scalenet'

    def __init__(self, pano_files: Sequence[str], views_per_pano: int = VIEWS_PER_PANO, seed: int = 0, device='cuda', engine=None):
        self.pano_files = [str(f) for f in pano_files]
        if not self.pano_files or views_per_pano < 1:
            raise ValueError('at least one panorama and one view per panorama')
        self.views_per_pano = int(views_per_pano)
        self.device, self.engine = torch.device(device), engine
        self.cameras = sample_cameras(len(self.pano_files) * self.views_per_pano, np.random.default_rng(seed))
        # the reference names view k of FILE 'FILE.kk.jpg' (generateCalibrationDataset.py:188)
        self.image_filenames = [f'{os.path.basename(f)}.{k:02d}.jpg' for f in self.pano_files for k in range(self.views_per_pano)]
        self._cached = (None, None)
        self.on_extracted = None                   # called with (panorama index, its views) after every extraction (write_tree)

    def __len__(self):
        return len(self.cameras)

    def imgname(self, i: int) -> str:
        return self.image_filenames[i]

    def labels(self, i: int):
        """-> (vfov, pitch, roll) in radians"""
        c = self.cameras[i]
        return float(c['vfov']), float(c['pitch']), float(c['roll'])

    def json_fields(self, i: int, imgname: Optional[str] = None) -> dict:
        return dict(self.cameras[i]['json'], imgname=imgname or self.imgname(i))

    def views_of(self, p: int) -> ViewList:
        """The views of panorama ``p`` on the device."""
        if self._cached[0] != p:
            pano = torch.from_numpy(read_panorama(self.pano_files[p])).to(self.device)
            views, heights = camera_views(self.cameras[p * self.views_per_pano:(p + 1) * self.views_per_pano])
            self._cached = (p, extract_views(pano, views, heights, self.engine))
            if self.on_extracted is not None:
                self.on_extracted(p, self._cached[1])
        return self._cached[1]

    def device_view(self, i: int) -> torch.Tensor:
        return self.views_of(i // self.views_per_pano)[i % self.views_per_pano]

    def device_batch(self, indices):
        """-> (slab, offsets, [(H, W)]) of the views ``indices`` without leaving the device: the panorama's own slab when
        the batch is all of one extraction's views in order, else a device-side concatenation."""
        indices = list(indices)
        vp = self.views_per_pano
        if indices == list(range(indices[0], indices[0] + vp)) and indices[0] % vp == 0:
            vl = self.views_of(indices[0] // vp)
            return vl.slab, [int(o) for o in vl.offsets], list(vl.sizes)
        parts = [self.device_view(i) for i in indices]
        sizes = [tuple(v.shape[:2]) for v in parts]
        offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])[:-1]]).astype(np.int64)
        return torch.cat([v.reshape(-1) for v in parts]), [int(o) for o in offsets], sizes

    def frame(self, i: int) -> np.ndarray:
        return self.device_view(i).cpu().numpy()


def write_tree(ds: PanoViewDataset, out_root: str, image_format: str = 'JPEG', log=print, while_evaluating: bool = False,
               jpeg_device=None, png_device=None) -> str:
    """The dataset as a 'pano_scalenet' tree under ``out_root`` (a data root: the tree is
    ``out_root/data/dataset_folders/pano_scalenet``): ``images/NAME.jpg`` as the reference saves it (quality 95, not optimised,
    not progressive; generateCalibrationDataset.py:131-132), ``images/NAME.json`` with the reference's fields (:149-158) and
    ``val_images.pkl``.  ``image_format`` is what Pillow encodes INTO the ``.jpg`` name (a lossless format takes the JPEG
    round trip out of a comparison; loaders go by content).  ``while_evaluating``: write ``val_images.pkl`` now and a
    panorama's views when the dataset extracts them, so that an evaluation that follows generates every view once.
    ``jpeg_device`` (None = ``engine.JPEG_DEVICE_DEFAULT``) with ``image_format='JPEG'``: all views of a panorama are encoded in
    ONE ``Engine.jpeg_encode`` call at quality 95 from the device slab they share, and only the files' bytes come down - the
    same bytes.  ``png_device`` (None = ``engine.PNG_DEVICE_DEFAULT``, off) with ``image_format='PNG'``: ONE
    ``Engine.png_encode`` call per panorama instead - files that decode to the same views, with bytes of their own.  Views that do
    not lie in a device slab (an extractor on the host) are encoded by Pillow as before."""
    import joblib
    from PIL import Image
    from . import cam_utils
    from .camcalib_eval import DATASET_FOLDERS
    from .engine import flow_jpeg_device, flow_png_device
    on_device = (image_format == 'JPEG' and flow_jpeg_device(jpeg_device)) or (image_format == 'PNG' and flow_png_device(png_device))
    folder = os.path.join(out_root, DATASET_FOLDERS['pano_scalenet'])
    os.makedirs(os.path.join(folder, 'images'), exist_ok=True)
    opts = {'quality': 95, 'optimize': False, 'progressive': False} if image_format == 'JPEG' else {}
    written = set()

    def write_panorama(p: int, views):
        if p in written:
            return
        written.add(p)
        files, slab = None, getattr(views, 'slab', None)
        if on_device and slab is not None and slab.device.type == 'cuda':
            eng = ds.engine or cam_utils._engine(slab.device)
            where = [(int(o), 3 * w) for o, (_, w) in zip(views.offsets, views.sizes)]
            files = eng.jpeg_encode(views.slab, list(views.sizes), where, opts['quality']) if image_format == 'JPEG' else eng.png_encode(views.slab, list(views.sizes), where)
        for k, v in enumerate(views):
            i = p * ds.views_per_pano + k
            path = os.path.join(folder, 'images', ds.imgname(i))
            if files is not None:
                with open(path, 'wb') as f:
                    f.write(files[k])
            else:
                Image.fromarray(v.cpu().numpy()).save(path, format=image_format, **opts)
            with open(path.replace('.jpg', '.json'), 'w') as f:
                json.dump(ds.json_fields(i, path), f)
        if len(written) == len(ds.pano_files):
            log(f'wrote {len(ds)} views of {len(ds.pano_files)} panoramas to {folder}')

    joblib.dump(list(ds.image_filenames), os.path.join(folder, 'val_images.pkl'))
    if while_evaluating:
        ds.on_extracted = write_panorama
    else:
        for p in range(len(ds.pano_files)):
            write_panorama(p, ds.views_of(p))
    return folder


def list_panoramas(directory: str) -> List[str]:
    exts = ('.jpg', '.jpeg', '.png', '.bmp', '.tif', '.tiff')
    files = sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.lower().endswith(exts))
    if not files:
        raise FileNotFoundError(f'no panorama images under {directory}')
    return files
