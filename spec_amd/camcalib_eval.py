"""CamCalib's own test step on MI355X: what ``python scripts/camcalib_train.py --cfg FILE`` does in the reference when
``RUN_TEST`` is set (scripts/camcalib_train.py:91-93 -> ``trainer.test`` -> ``CameraRegressorModule.validation_step`` /
``validation_epoch_end``, camcalib/trainer.py:84-116,176-199, fed by ``val_dataloader`` :236-265):

1. the validation set (camcalib/pano_dataset.py:48-144): frames of different sizes, each resized with
   ``Resize(MIN_RES, MAX_RES)`` (:184-220 - the longer side is capped, unlike the demo's ``Resize(600)``);
2. ``DATASET.BATCH_SIZE`` consecutive frames per batch (the loader does not shuffle), collated with ``to_image_list``
   (:223-306): every frame in the top-left corner of a zero tensor of the batch's largest height and width;
3. ``CameraRegressorNetwork`` -> ``CameraRegressorLoss`` (camcalib/loss.py:24-125) -> ``convert_preds_to_angles`` ->
   ``vfov_acc / pitch_acc / roll_acc`` = mean absolute error in degrees; epoch end = the mean of the per-batch means.

Frames are decoded with Pillow on the host and uploaded as one uint8 slab per batch; resize + normalise + padding
(``specmi_resize_normalize_ragged``), the network, and the loss / decode / error reductions (``specmi_camcalib_eval``)
run on the device.

As in the reference, the network sees the padding: an image's logits depend on which frames share its batch (through
the batch's padded height and width), so ``DATASET.BATCH_SIZE`` is part of the result.  What they do NOT depend on is how
the padded batch is forwarded: the trunk plan is pinned to 'throughput' and a batch too large for one call is forwarded
as whole padded images in sub-batches, bit-identically.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import cam_utils, evaluation
from .checkpoint import load_pretrained_model, read_checkpoint
from .engine import flow_image_dtype, flow_jpeg_decode_device, flow_png_decode_device
from .preprocess import decode_frames

# camcalib/config.py:36-87 (the keys the test step reads)
DEFAULTS = {
    'LOG_DIR': 'logs/camcalib', 'METHOD': 'camcalib', 'RUN_TEST': False,
    'DATASET': {'TRAIN_DS': 'pano', 'VAL_DS': 'pano', 'MIN_RES': 600, 'MAX_RES': 1000, 'BATCH_SIZE': 64},
    'TRAINING': {'PRETRAINED': None},
    'MODEL': {'BACKBONE': 'resnet34', 'NUM_FC_LAYERS': 1, 'NUM_FC_CHANNELS': 1024, 'LOSS_VFOV_WEIGHT': 1.0,
              'LOSS_PITCH_WEIGHT': 1.0, 'LOSS_ROLL_WEIGHT': 1.0, 'LOSS_TYPE': 'ce'},
}
# the reference's DATASET_FOLDERS (camcalib/config.py:30-34) are absolute paths of its authors' cluster; here they
# are looked up under the data root
DATASET_FOLDERS = {'pano': 'data/dataset_folders/pano', 'pano_scalenet': 'data/dataset_folders/pano_scalenet'}
LOSS_TYPES = ('ce', 'kl', 'softargmax_l2', 'softargmax_biased_l2')
STANDIN_CKPT = 'data/camcalib/checkpoints/camcalib_standin.ckpt'
STANDIN_CFG = 'data/camcalib/checkpoints/camcalib_standin.yaml'


def load_config(cfg_path: Optional[str], opts: Optional[List[str]] = None) -> dict:
    """The reference's YAML keys over its defaults, then ``--opts KEY.SUB value ...`` (``evaluation.load_config``'s merge)."""
    return evaluation.load_config(cfg_path, opts, defaults=DEFAULTS)


def resize_size(w: int, h: int, min_size: int = 600, max_size: Optional[int] = 1000):
    """``Resize.get_size`` (camcalib/pano_dataset.py:192-212) for a (w, h) image -> (oh, ow): shorter side -> min_size
    unless that would push the longer side past max_size, in which case the shorter side becomes
    ``round(max_size * short / long)``; a frame whose shorter side already has that size keeps its size; the longer side
    is ``int(size * long / short)`` (truncated)."""
    size = min_size
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def encode_targets(vfov, pitch, roll, loss_type: str):
    """Ground-truth encoding of camcalib/pano_dataset.py:135-142 for arrays of angles in radians -> three arrays:
    ``np.digitize`` against the bin edges (int64) for 'ce' / 'kl', the soft index in [-1, 1] (fp32, ``.float()``) for the
    soft-argmax losses."""
    vfov, pitch, roll = (np.asarray(a, dtype=np.float64) for a in (vfov, pitch, roll))
    if loss_type in ('kl', 'ce'):
        return (np.digitize(vfov, cam_utils.vfov_bins).astype(np.int64), np.digitize(pitch, cam_utils.pitch_bins).astype(np.int64),
                np.digitize(roll, cam_utils.roll_bins).astype(np.int64))
    if loss_type in ('softargmax_l2', 'softargmax_biased_l2'):
        return (cam_utils.vfov2soft_idx(vfov).astype(np.float32), cam_utils.pitch2soft_idx(pitch).astype(np.float32),
                cam_utils.roll2soft_idx(roll).astype(np.float32))
    raise ValueError(f'{loss_type} is not defined..')


def val_dataset_name(hparams: dict) -> str:
    """``val_dataloader`` (camcalib/trainer.py:236-251) tests DATASET.TRAIN_DS - not VAL_DS - for 'pano_agora' and otherwise
    builds ``CameraRegressorDataset(dataset=DATASET.VAL_DS)``; mirrored, with 'pano_agora' refused by name either way."""
    ds = hparams['DATASET']
    if ds.get('TRAIN_DS') == 'pano_agora' or ds.get('VAL_DS') == 'pano_agora':
        raise NotImplementedError("'pano_agora' (PanoAgoraDataset) needs AGORA's own files and is not built; "
                                  "the test step reads 'pano' and 'pano_scalenet'")
    if ds['VAL_DS'] not in DATASET_FOLDERS:
        raise ValueError(f"{ds['VAL_DS']} is not implemented.")
    return ds['VAL_DS']


class PanoValDataset:
    """The ``is_train=False`` half of ``CameraRegressorDataset`` (camcalib/pano_dataset.py:48-144): ``val_images.pkl`` lists
    the file names under ``images/``; labels come from ``images/NAME.json`` ('pano_scalenet': vfov in radians, the image is
    ``NAME.jpg``) or ``annotations/NAME.json`` ('pano': vfov in degrees, the image is ``NAME.png``).  ``split='train'`` lists the
    ``is_train=True`` half's frames instead (``train_images.pkl``, :63), read the same way; the ColorJitter that half applies is
    ``spec_amd.augment.ColorJitter``, applied by the training flow where the batch lies."""

    def __init__(self, name: str, data_root: str = '.', folder: Optional[str] = None, split: str = 'val'):
        import joblib
        if split not in ('val', 'train'):
            raise ValueError(f"split {split!r}: 'val' (val_images.pkl) or 'train' (train_images.pkl)")
        if name == 'pano_agora':
            raise NotImplementedError("'pano_agora' needs AGORA's own files and is not built")
        if name not in DATASET_FOLDERS:
            raise ValueError(f'{name} is not implemented.')
        self.name = name
        self.folder = folder or os.path.join(data_root, DATASET_FOLDERS[name])
        self.split = split
        self.image_filenames = [str(f) for f in joblib.load(os.path.join(self.folder, f'{split}_images.pkl'))]

    def __len__(self):
        return len(self.image_filenames)

    def imgname(self, i: int) -> str:
        return os.path.join(self.folder, 'images', self.image_filenames[i])

    def labels(self, i: int):
        """-> (vfov, pitch, roll) in radians"""
        imgname = self.imgname(i)
        if self.name == 'pano':
            with open(imgname.replace('images', 'annotations').replace('.png', '.json')) as f:
                data = json.load(f)
            return float(np.radians(data['vfov'])), float(data['pitch']), float(data['roll'])
        with open(imgname.replace('.jpg', '.json')) as f:
            data = json.load(f)
        return float(data['vfov']), float(data['pitch']), float(data['roll'])

    def frame(self, i: int) -> np.ndarray:
        return evaluation.read_image_rgb(self.imgname(i))


def pad_batch(frames, min_size: int, max_size: Optional[int], device, engine=None, dtype=torch.float32) -> torch.Tensor:
    """Steps 1-2 for one batch: (H_f, W_f, 3) uint8 host frames -> (n, 3, Hmax, Wmax) fp32 on the device (one upload, two
    launches).  ``frames`` may also be ``(slab, offsets, [(H, W)])`` - frames that already lie in a 1-D uint8 device slab
    (``spec_amd.panorama.PanoViewDataset.device_batch``): nothing is uploaded.  ``dtype=torch.float16``: the batch in the fp16
    trunk's NHWC8 layout (n, Hmax, Wmax, 8), padding +0: 16 B per pixel held by the caller instead of 12 B (the library's workspaces are the same on both routes); what it
    saves is the conversion pass over the batch."""
    from .engine import out_dtype
    out_dtype(dtype)                       # ValueError for anything but fp32 / fp16, before the engine is touched
    eng = engine or cam_utils._engine(torch.device(device))
    if isinstance(frames, tuple):
        slab, offsets, sizes = frames
        return eng.resize_normalize_ragged(slab, offsets, [(H, W) + resize_size(W, H, min_size, max_size) for H, W in sizes], dtype=dtype)
    from .preprocess import pack_frames
    slab, offsets, sizes = pack_frames(frames, eng.device)
    return eng.resize_normalize_ragged(slab, offsets, [(H, W) + resize_size(W, H, min_size, max_size) for H, W in sizes], dtype=dtype)


def forward_limit(H: int, W: int) -> int:
    """Images of a (., 3, H, W) batch one trunk call takes: the stem's activation (64 channels at half resolution, fp32) is
    kept below 2 GiB, the range of the convolution kernels' 32-bit offsets (64 frames at 600 x 1000 give 2.4 GiB)."""
    oh, ow = (H + 2 * 3 - 7) // 2 + 1, (W + 2 * 3 - 7) // 2 + 1
    return max(1, (2 ** 31 - 1) // (oh * ow * 64 * 4))


def forward_padded(model, images: torch.Tensor, sub_batch: Optional[int] = None):
    """The network on one padded batch, whole images in sub-batches of ``sub_batch`` (default: ``forward_limit``) -> three
    (n, nbins) logit tensors; with the plan pinned the sub-batch size does not change a bit."""
    if images.dtype == torch.float16:      # NHWC8 (n, H, W, 8): a slice of whole images is contiguous and 16-byte aligned
        n, H, W, _ = images.shape
    else:
        n, _, H, W = images.shape
    step = min(int(sub_batch), forward_limit(H, W)) if sub_batch else forward_limit(H, W)
    if step >= n:
        return [t.clone() for t in model(images)]
    parts = [model(images[b0:b0 + step]) for b0 in range(0, n, step)]
    return [torch.cat([p[k] for p in parts]) for k in range(3)]


def epoch_end(outputs: List[dict]) -> Dict[str, float]:
    """``validation_epoch_end`` (camcalib/trainer.py:176-193): the fp32 mean of the per-batch values - a short last batch
    weighs as much as a full one."""
    mean = lambda k: float(torch.tensor([float(o[k]) for o in outputs], dtype=torch.float32).mean().item())
    return {'val_loss': mean('loss'), 'vfov_acc': mean('vfov_acc'), 'pitch_acc': mean('pitch_acc'), 'roll_acc': mean('roll_acc')}


def build_model(hparams: dict, ckpt: Optional[str], data_root: str = '.', device='cuda'):
    from .modules import CameraRegressorNetwork
    m = hparams['MODEL']
    model = CameraRegressorNetwork(backbone=m['BACKBONE'], num_fc_layers=int(m['NUM_FC_LAYERS']),
                                   num_fc_channels=int(m['NUM_FC_CHANNELS']))
    ckpt = ckpt or hparams['TRAINING']['PRETRAINED']
    if ckpt is None:
        raise ValueError('no checkpoint: set TRAINING.PRETRAINED in the config or pass --ckpt')
    if not os.path.isabs(ckpt):
        ckpt = os.path.join(data_root, ckpt)
    load_pretrained_model(model, read_checkpoint(ckpt)['state_dict'], remove_lightning=True, strict=True)
    model.set_plan('throughput')          # an image's logits must not depend on the sub-batch
    return model.to(torch.device(device)).eval().commit(torch.device(device), freeze=True)


def validation_horizons(size_hw, gt, pred) -> list:
    """The two horizons of a validation picture in the order ``save_images`` draws them (camcalib/trainer.py:155-161): ground
    truth - blue, width 3, caption strip at the bottom - then prediction - red, width 3, strip at the top -, both with
    ``debug=True``, ``text_size=16`` and ``f_pix = H / 2 / tan(vfov / 2)``; ``gt`` / ``pred`` = (vfov, pitch, roll) as NumPy scalars
    of the run's own dtypes.  -> what ``render.plan_horizon_marks`` / ``show_horizon_lines`` take for one frame."""
    H = int(size_hw[0])
    one = lambda a, colour, GT: dict(vfov=a[0], pitch=a[1], roll=a[2], focal_length=H / 2. / np.tan(a[0] / 2.), debug=True, color=colour, width=3,
                                     GT=GT, text_size=16)
    return [one(gt, (0, 0, 255), True), one(pred, (255, 0, 0), False)]


def save_validation_picture(eng, images: torch.Tensor, size_hw, gt, pred, path: str, jpeg_device=None, index: int = 0) -> str:
    """One picture of ``save_images`` (camcalib/trainer.py:118-169) made where the batch lies: image ``index`` of the padded
    network input ``images`` - (n, 3, H, W) fp32, or the fp16 trunk's (n, H, W, 8), of which the one image is converted with
    ``.float()`` - denormalised to uint8 and cut to its own resized size ``size_hw`` (``Engine.denormalize_u8``: ImageNet's
    constants as pare's un-vendored ``denormalize_images``, parity unpinned; values beyond [0, 255] are clamped where the
    reference's ``astype('uint8')`` is undefined), the two horizons of ``validation_horizons`` drawn by ONE ``draw_marks`` call
    (``render.show_horizon_lines``), and the file written through ``render.save_picture`` - a ``.jpg`` on the device when the
    JPEG route is on.  A horizon the device route cannot reproduce (``horizon_marks`` -> None) is drawn on the host."""
    from . import render
    H, W = int(size_hw[0]), int(size_hw[1])
    if images.dtype == torch.float16:
        x = images[index, :, :, :3].permute(2, 0, 1).float().contiguous()[None]
        index = 0
    else:
        x = images.contiguous()
    frame = eng.denormalize_u8(x, index, H, W)
    horizons = validation_horizons((H, W), gt, pred)
    if render.plan_horizon_marks([(H, W)], [horizons]) is not None:
        render.show_horizon_lines(frame, [(H, W)], [0], [horizons], engine=eng)
        picture = frame.view(H, W, 3)
    else:
        img = frame.cpu().numpy().reshape(H, W, 3)
        for hz in horizons:
            kw = dict(hz)
            img, _ = render.show_horizon_line(img, kw.pop('vfov'), kw.pop('pitch'), kw.pop('roll'), **kw)
        picture = torch.from_numpy(img).to(eng.device)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    return render.save_picture(path, picture, engine=eng, jpeg_device=jpeg_device)


@torch.no_grad()
def run_evaluation(hparams: dict, data_root: str = '.', ckpt: Optional[str] = None, log=print, device='cuda', model=None,
                   sub_batch: Optional[int] = None, dataset=None, _fp32_images: Optional[bool] = None, save_images: Optional[bool] = None,
                   image_dir: Optional[str] = None, jpeg_device=None, jpeg_decode_device=None, png_decode_device=None) -> dict:
    """CamCalib's test epoch over ``DATASET.VAL_DS`` - or over ``dataset``, an object with ``PanoValDataset``'s interface such as
    ``spec_amd.panorama.PanoViewDataset``, whose ``device_batch`` hands frames over without a host round trip: consecutive batches of ``DATASET.BATCH_SIZE`` frames in file order, each
    padded to ITS OWN largest height and width, forwarded, scored.  Returns the four epoch figures the reference logs
    (``val_loss``, ``vfov_acc``, ``pitch_acc``, ``roll_acc``: mean of the per-batch means), the per-batch dicts and, per image,
    the logits, decoded angles and absolute errors (radians).

    As in the reference an image's logits depend on which frames share its batch - through the padding the network sees -
    but not on ``sub_batch`` (how many padded images one trunk call takes).

    The kernel takes the ground-truth angles as fp32; for 'ce' / 'kl' the predictions are the float64 bin centres gathered on
    the host with the kernel's arg-max indices and the accuracies are float64, as in the reference.

    ``_fp32_images=False``: a model at precision 'fp16' is fed NHWC8 fp16 batches (``pad_batch(dtype=torch.float16)``); True: the
    fp32 batch + in-trunk conversion (same bits); None = ``engine.F16_CROPS_DEFAULT``.

    ``jpeg_decode_device`` (None = ``engine.JPEG_DECODE_DEVICE_DEFAULT``): where the frames come from files (``ds.imgname``), the
    files' bytes go up and ``preprocess.decode_frames`` decodes them on the device instead of Pillow on the host (same bits).
    ``png_decode_device`` (None = ``engine.PNG_DECODE_DEVICE_DEFAULT``): the same for .png files, which is what the ``pano`` tree
    holds (camcalib/pano_dataset.py:117).

    ``save_images`` (None = ``TRAINING.SAVE_IMAGES`` of the config, which every config of the reference sets): the validation
    pictures of ``save_images`` (camcalib/trainer.py:94-95,118-169) - for the first image of every fourth batch the network input
    with the ground-truth and the predicted horizon, ``result_{step 0:07d}_{batch:05d}.jpg`` under ``image_dir`` (None =
    ``LOG_DIR/val_output_images``), made on the device (``save_validation_picture``); the files are listed under ``'pictures'``."""
    dev = torch.device(device)
    if save_images is None:
        save_images = bool((hparams.get('TRAINING') or {}).get('SAVE_IMAGES', False))
    if save_images and image_dir is None:
        log_dir = hparams['LOG_DIR'] if os.path.isabs(hparams['LOG_DIR']) else os.path.join(data_root, hparams['LOG_DIR'])
        image_dir = os.path.join(log_dir, 'val_output_images')
    pictures = []
    m = hparams['MODEL']
    loss_type = m['LOSS_TYPE']
    if loss_type not in LOSS_TYPES:
        raise ValueError(f'{loss_type} is not defined..')
    ds = dataset if dataset is not None else PanoValDataset(val_dataset_name(hparams), data_root)
    log(f'Val dataset len: {len(ds)}')
    if model is None:
        model = build_model(hparams, ckpt, data_root, dev)
    else:
        model.set_plan('throughput')
    weights = (float(m['LOSS_VFOV_WEIGHT']), float(m['LOSS_PITCH_WEIGHT']), float(m['LOSS_ROLL_WEIGHT']))
    bs, min_res, max_res = int(hparams['DATASET']['BATCH_SIZE']), int(hparams['DATASET']['MIN_RES']), hparams['DATASET']['MAX_RES']
    eng = model.engine(dev)
    centers = (cam_utils.vfov_bins_centers, cam_utils.pitch_bins_centers, cam_utils.roll_bins_centers)
    outputs, per = [], {k: [] for k in ('logits', 'pred', 'err', 'gt', 'img_sizes')}
    for b0 in range(0, len(ds), bs):
        idx = range(b0, min(len(ds), b0 + bs))
        on_device = hasattr(ds, 'device_batch')
        jdec, pdec = flow_jpeg_decode_device(jpeg_decode_device), flow_png_decode_device(png_decode_device)
        if not on_device and hasattr(ds, 'imgname') and (jdec or pdec):
            # the frames come from files: their bytes go up and are decoded where they land (preprocess.decode_frames; same bits)
            frames, on_device = decode_frames([ds.imgname(i) for i in idx], dev, jdec, pdec), True
        else:
            frames = ds.device_batch(idx) if on_device else [ds.frame(i) for i in idx]
        sizes_hw = frames[2] if on_device else [f.shape[:2] for f in frames]
        gt = np.asarray([ds.labels(i) for i in idx], dtype=np.float64).T              # (3, n): vfov, pitch, roll
        gt32 = gt.astype(np.float32)                                                   # torch.tensor(python float)
        images = pad_batch(frames, min_res, max_res, dev, eng, dtype=flow_image_dtype(model, _fp32_images))
        logits = forward_padded(model, images, sub_batch)
        padded_hw = tuple(images.shape[1:3]) if images.dtype == torch.float16 else tuple(images.shape[2:])
        ev = eng.camcalib_eval(*logits, encode_targets(*gt, loss_type), gt32, loss_type, weights)
        means = ev['means'].cpu().numpy()
        out = {'loss': float(means[0]), 'vfov_loss': float(means[1]), 'pitch_loss': float(means[2]), 'roll_loss': float(means[3]),
               'n': len(idx), 'padded_hw': padded_hw}
        if loss_type in ('ce', 'kl'):
            am = ev['argmax'].cpu().numpy()
            pred = np.stack([centers[k][am[k]] for k in range(3)])                     # float64 bin centres
            # 'pano' reads vfov through np.radians -> a float64 label; every other label is a python float -> fp32
            g = np.stack([gt[0] if ds.name == 'pano' else gt32[0].astype(np.float64), gt32[1].astype(np.float64), gt32[2].astype(np.float64)])
            err = np.abs(pred - g)
            acc = np.degrees(err.mean(axis=1))
        else:
            pred, err = ev['angle'].cpu().numpy(), ev['err'].cpu().numpy()
            acc = means[4:7]
        out.update(vfov_acc=float(acc[0]), pitch_acc=float(acc[1]), roll_acc=float(acc[2]))
        outputs.append(out)
        per['logits'].append(torch.stack(logits, 0).cpu().numpy())
        per['pred'].append(pred); per['err'].append(err); per['gt'].append(gt)
        per['img_sizes'] += [resize_size(w, h, min_res, max_res) for h, w in sizes_hw]
        batch_nb = b0 // bs
        if save_images and batch_nb % 4 == 0:
            # the labels as the reference's batch holds them: fp32 tensors (float64 for 'pano''s vfov); the predictions as decoded
            g0 = (gt[0][0] if ds.name == 'pano' else gt32[0][0], gt32[1][0], gt32[2][0])
            pictures.append(save_validation_picture(eng, images, per['img_sizes'][b0], g0, tuple(pred[k][0] for k in range(3)),
                                                    os.path.join(image_dir, f'result_{0:07d}_{batch_nb:05d}.jpg'), jpeg_device=jpeg_device))
            log(f'wrote {pictures[-1]}')
    if eng.sync_status() != 0:
        raise RuntimeError('a split-K arrival counter was left non-zero')
    res = epoch_end(outputs)
    log(f"[EPOCH 0] Val loss reached {res['val_loss']}")
    log(f"[EPOCH 0] vfov acc: {res['vfov_acc']}")
    log(f"[EPOCH 0] pitch acc: {res['pitch_acc']}")
    log(f"[EPOCH 0] roll acc: {res['roll_acc']}")
    cat = lambda k: np.concatenate(per[k], axis=1)
    res.update(batches=outputs, loss_type=loss_type, imgname=[ds.imgname(i) for i in range(len(ds))], logits=cat('logits'),
               img_sizes=per['img_sizes'], pictures=pictures)
    for k, name in enumerate(('vfov', 'pitch', 'roll')):
        res['pred_' + name], res['err_' + name], res['gt_' + name] = cat('pred')[k], cat('err')[k], cat('gt')[k]
    return res


# ------------------------------------------------------------------------------------------------------------
# stand-in tree in the REAL formats (tests / dry runs; the panorama crops cannot ship)
# ------------------------------------------------------------------------------------------------------------
# (w, h) of the stand-in frames in units of MIN_RES / 6: landscape, portrait, square, one whose aspect ratio triggers the
# MAX_RES cap (for MAX_RES / MIN_RES = 5 / 3), one already at MIN_RES (kept unresampled)
STANDIN_SHAPES = ((9, 7), (7, 10), (8, 8), (16, 7), (8, 6), (13, 8), (6, 9), (11, 9), (7, 7), (9, 12))


def write_standin_tree(root: str, n_images: int = 10, seed: int = 11, dataset: str = 'pano_scalenet', min_res: int = 96,
                       max_res: int = 160, batch_size: int = 4, backbone: str = 'resnet34', loss_type: str = 'ce',
                       weights=(1.0, 1.0, 1.0), ckpt_seed: int = 1001) -> dict:
    """Writes under ``root`` what ``run_evaluation`` reads, synthetic numbers in the real formats: ``val_images.pkl`` (joblib),
    ``images/NAME.jpg`` + ``NAME.json`` ('pano_scalenet') or ``images/NAME.png`` + ``annotations/NAME.json`` with vfov in
    degrees ('pano'), a Lightning-layout checkpoint (``model.``-prefixed ``state_dict``) and the YAML config.  Returns the
    labels and frame sizes it used."""
    import joblib
    import yaml
    from PIL import Image
    from . import synth
    if dataset not in DATASET_FOLDERS:
        raise ValueError(f'{dataset} is not implemented.')
    rng = np.random.default_rng(seed)
    j = lambda *p: os.path.join(root, *p)
    folder = DATASET_FOLDERS[dataset]
    for d in (f'{folder}/images', f'{folder}/annotations', os.path.dirname(STANDIN_CKPT)):
        os.makedirs(j(d), exist_ok=True)
    u = max(1, min_res // 6)
    ext = '.jpg' if dataset == 'pano_scalenet' else '.png'
    names, labels, sizes = [], [], []
    for i in range(n_images):
        w, h = (u * s for s in STANDIN_SHAPES[i % len(STANDIN_SHAPES)])
        # smooth content + noise: JPEG keeps it, the network sees structure
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([127 + 100 * np.sin(xx / (5.0 + i) + c) * np.cos(yy / (7.0 + c)) for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
        name = f'pano_{i:04d}{ext}'
        Image.fromarray(img).save(j(folder, 'images', name), **({'quality': 92} if ext == '.jpg' else {}))
        vfov, pitch, roll = float(rng.uniform(0.4, 1.9)), float(rng.uniform(-0.55, 0.55)), float(rng.uniform(-0.5, 0.5))
        if dataset == 'pano':
            lab = {'vfov': float(np.degrees(vfov)), 'pitch': pitch, 'roll': roll}
            with open(j(folder, 'annotations', name.replace('.png', '.json')), 'w') as f:
                json.dump(lab, f)
            vfov = float(np.radians(lab['vfov']))
        else:
            with open(j(folder, 'images', name.replace('.jpg', '.json')), 'w') as f:
                json.dump({'vfov': vfov, 'pitch': pitch, 'roll': roll}, f)
        names.append(name); labels.append((vfov, pitch, roll)); sizes.append((w, h))
    joblib.dump(names, j(folder, 'val_images.pkl'))
    cs = synth.camcalib_state(ckpt_seed, backbone=backbone)
    torch.save({'epoch': 0, 'global_step': 1, 'pytorch-lightning_version': '1.1.8',
                'state_dict': {'model.' + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cs.items()}}, j(STANDIN_CKPT))
    cfg = {'METHOD': 'camcalib', 'RUN_TEST': True, 'LOG_DIR': 'logs/camcalib_standin',
           'DATASET': {'TRAIN_DS': dataset, 'VAL_DS': dataset, 'MIN_RES': int(min_res), 'MAX_RES': int(max_res), 'BATCH_SIZE': int(batch_size)},
           'TRAINING': {'PRETRAINED': STANDIN_CKPT},
           'MODEL': {'BACKBONE': backbone, 'NUM_FC_LAYERS': 1, 'NUM_FC_CHANNELS': 1024, 'LOSS_TYPE': loss_type,
                     'LOSS_VFOV_WEIGHT': float(weights[0]), 'LOSS_PITCH_WEIGHT': float(weights[1]), 'LOSS_ROLL_WEIGHT': float(weights[2])}}
    with open(j(STANDIN_CFG), 'w') as f:
        yaml.safe_dump(cfg, f)
    return {'names': names, 'labels': np.asarray(labels, np.float64), 'sizes_wh': sizes, 'config': cfg, 'camcalib_state': cs}
