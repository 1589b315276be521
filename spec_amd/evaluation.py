"""Config-5 evaluation flow on MI355X: what ``python scripts/spec_eval.py --cfg data/spec/checkpoints/spec_config.yaml
--opts DATASET.VAL_DS spec-syn`` does in the reference (scripts/spec_eval.py:35-82 -> ``pl.Trainer.test`` ->
``SPECTrainer.validation_step`` spec/trainer.py:230-364 -> ``compute_error`` spec/utils/compute_error.py:89-223),
reading the reference's files in their real container formats:

* ``spec_config.yaml``                      - the yacs dump of ``spec/config.py`` (keys below), plain YAML;
* ``TRAINING.PRETRAINED_LIT`` / ``--ckpt``  - Lightning checkpoint, ``['state_dict']`` with the ``model.`` prefix and
                                               pickled foreign classes (``spec_amd.checkpoint.read_checkpoint``);
* ``data/body_models/smpl/SMPL_NEUTRAL.pkl`` (chumpy / scipy-sparse members), ``data/J_regressor_extra.npy``,
  ``data/smpl_mean_params.npz``, ``data/J_regressor_h36m.npy``  (spec/config.py:34-37);
* ``data/dataset_folders/<ds>/annotations/test.npz`` + the images under ``data/dataset_folders/<ds>``
  (spec/config.py:39-56; keys ``imgname scale center pose shape cam_rotmat cam_int camcalib_pitch camcalib_roll
  camcalib_vfov camcalib_f_pix``, spec/dataset/cam_dataset.py:56-146).

Images are decoded with Pillow on the host (the reference uses cv2.imread), uploaded as uint8 frames and cropped /
normalised on the device the way the reference dataset does it (``specmi_crop_resize_normalize``: PARE's ``crop`` = integer box
copy + cv2.resize bilinear, clip, / 255, Normalize).  Everything after that stays in HBM: forward, metrics.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import assets, io_formats, metrics
from .cam_utils import cam_params_from_angles
from .checkpoint import load_pretrained_model, read_checkpoint
from .engine import flow_image_dtype, flow_ragged_crops
from .preprocess import dataset_crops, dataset_crops_ragged, decode_frames, pack_frames

# spec/config.py:34-56
DATASET_FOLDERS = {'spec-mtp': 'data/dataset_folders/spec-mtp', 'spec-syn': 'data/dataset_folders/spec-syn',
                   '3dpw-test-cam': 'data/dataset_folders/3dpw'}
DATASET_FILES = {'spec-mtp': 'data/dataset_folders/spec-mtp/annotations/test.npz',
                 'spec-syn': 'data/dataset_folders/spec-syn/annotations/test.npz',
                 '3dpw-test-cam': 'data/dataset_extras/3dpw_test_0yaw_inverseyz_w_camcalib.npz'}
README_TABLE = {'spec-mtp': (124.3, 71.8, 147.1), 'spec-syn': (74.9, 54.5, 90.5), '3dpw-test-cam': (106.7, 53.3, 124.7)}

DEFAULTS = {   # the hparams of spec/config.py the evaluation reads
    'LOG_DIR': 'logs/experiments', 'METHOD': 'hmr_cam',
    'DATASET': {'BATCH_SIZE': 64, 'VAL_DS': 'spec-syn_spec-mtp_3dpw-test-cam', 'IMG_RES': 224},
    'TRAINING': {'PRETRAINED_LIT': None, 'USE_AMP': False, 'SAVE_IMAGES': False},
    'TESTING': {'USE_GT_CAM': False, 'SAVE_RESULTS': True, 'SAVE_IMAGES': False, 'SAVE_FREQ': 1},
    'HMR': {'BACKBONE': 'resnet50', 'USE_CAM_FEATS': False},
}


def load_config(cfg_path: Optional[str], opts: Optional[List[str]] = None, defaults: Optional[dict] = None) -> dict:
    """YAML config (yacs dump) merged over the defaults, then ``--opts KEY.SUB value ...`` overrides.  ``defaults``: another
    default tree than this flow's (``spec_amd.camcalib_eval`` merges its own the same way)."""
    import copy
    import yaml
    hp = copy.deepcopy(DEFAULTS if defaults is None else defaults)

    def merge(dst, src):
        for k, v in (src or {}).items():
            if isinstance(v, dict) and isinstance(dst.get(k), dict):
                merge(dst[k], v)
            else:
                dst[k] = v
    if cfg_path:
        with open(cfg_path) as f:
            merge(hp, yaml.safe_load(f))
    opts = list(opts or [])
    if len(opts) % 2:
        raise ValueError('--opts takes KEY value pairs')
    for k, v in zip(opts[0::2], opts[1::2]):
        node = hp
        parts = k.split('.')
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = yaml.safe_load(v) if isinstance(v, str) else v
    return hp


def eval_precision(hparams: dict) -> str:
    """The trunk precision the evaluation runs at: 'fp16' when ``TRAINING.USE_AMP`` is true - the reference then evaluates
    under Lightning ``precision=16`` (scripts/spec_eval.py:63-70) - else 'fp32'."""
    return 'fp16' if bool((hparams.get('TRAINING') or {}).get('USE_AMP', False)) else 'fp32'


def read_image_rgb(path: str) -> np.ndarray:
    """(H,W,3) uint8 RGB (the reference's ``read_img`` = cv2.imread + BGR->RGB)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))       # a writable copy (torch.from_numpy needs one)


class EvalDataset:
    """The evaluation half of ``CamDataset`` (spec/dataset/cam_dataset.py): annotation arrays + image loading; no
    augmentation (is_train=False: flip 0, rot 0, sc 1, pn 1)."""

    def __init__(self, name: str, data_root: str = '.', dataset_file: Optional[str] = None, img_dir: Optional[str] = None):
        self.name = name
        self.img_dir = img_dir or os.path.join(data_root, DATASET_FOLDERS[name])
        self.data = dict(np.load(dataset_file or os.path.join(data_root, DATASET_FILES[name])))
        self.imgname = self.data['imgname']
        self.n = len(self.imgname)
        self._jpeg_decode_device = None     # True: the batch's .jpg files go up as bytes and are decoded on the device (preprocess.decode_frames; same bits); None = engine.JPEG_DECODE_DEVICE_DEFAULT
        self._png_decode_device = None      # the same for the batch's .png files (specmi_png_decode; same bits); None = engine.PNG_DECODE_DEVICE_DEFAULT
        self._ragged_crops = None     # True: one slab, one upload, one ragged crop launch per batch; False: one of each per sample (same bits)

    def __len__(self):
        return self.n

    def loss_gt(self, idx, shapes, device) -> Dict[str, torch.Tensor]:
        """The ground-truth half of ``HMRCamLoss.forward`` for the samples ``idx`` (``shapes``: their (H, W)), without
        ``vertices``.  Fields the annotation file lacks are filled as the reference dataset fills them
        (spec/dataset/cam_dataset.py:93-116,148-157,353-359,386-413,480-486): ``pose_0yaw_inverseyz`` before ``pose``; ``has_smpl``
        = 1 when the file has pose and shape but no such key, 0 (with zero pose and betas) when it has neither; ``pose_conf`` = 1;
        ``pose_3d`` = ``S`` with ``has_pose_3d`` = 1, else zeros with 0; ``part`` / ``openpose`` keypoints, zeros when missing."""
        d, n = self.data, len(idx)
        f = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt)
        pose_key = 'pose_0yaw_inverseyz' if 'pose_0yaw_inverseyz' in d else 'pose'
        if pose_key in d and 'shape' in d:
            has_smpl = np.asarray(d['has_smpl'][idx]) if 'has_smpl' in d else np.ones(n)
            keep = (has_smpl != 0)[:, None]
            pose, betas = np.where(keep, d[pose_key][idx], 0.0), np.where(keep, d['shape'][idx], 0.0)
        else:
            has_smpl, pose, betas = np.zeros(n), np.zeros((n, 72)), np.zeros((n, 10))
        kp = keypoints_orig(d, idx)
        return {'pose': f(pose), 'betas': f(betas), 'pose_conf': torch.ones(n, 24, device=device),
                'pose_3d': f(d['S'][idx]) if 'S' in d else torch.zeros(n, 24, 4, device=device),
                'keypoints_orig': f(kp), 'has_smpl': f(has_smpl != 0, torch.int32),
                'has_pose_3d': torch.full((n,), int('S' in d), device=device, dtype=torch.int32),
                'scale': f(d['scale'][idx]), 'orig_shape': shapes if isinstance(shapes, torch.Tensor) else f(shapes)}

    def eval_gt(self, idx, device, body) -> Dict[str, torch.Tensor]:
        """What the reference dataset adds to an evaluation item for the validation step (spec/dataset/cam_dataset.py:415-478), for
        the samples ``idx``, from ONE call of the body model ``body`` (``metrics.BodyModel``): ``vertices`` (n, V, 3) and
        ``joints_24`` (n, 24, 3), the kinematic-chain joints with the pelvis (joint 0) subtracted (:476-477).  The pose key follows
        ``loss_gt``'s rule: ``pose_0yaw_inverseyz`` before ``pose``.  (``pose_3d`` of :443-447 is the H36M regression of these
        vertices; ``metrics.validation_errors`` regresses it on the device.  ``DATASET.USE_GENDER`` concerns 3dpw / 3dpw-all
        only, which this class does not read.)"""
        d = self.data
        pose_key = 'pose_0yaw_inverseyz' if 'pose_0yaw_inverseyz' in d else 'pose'
        if pose_key not in d or 'shape' not in d:
            raise KeyError(f'{self.name}: the annotations hold no SMPL ground truth (pose and shape), the validation step needs it')
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=torch.float32)
        vertices, joints = body.native(f(d[pose_key][idx]), f(d['shape'][idx]))
        return {'vertices': vertices, 'joints_24': joints - joints[:, :1]}

    def batch(self, idx, device, img_res=224, use_gt_cam=False, dtype=torch.float32) -> Dict[str, torch.Tensor]:
        """``dtype``: what the crops are stored as (``spec_amd.preprocess``: fp32 (n,3,S,S), or NHWC8 fp16 for an fp16 model)."""
        d = self.data
        paths = [os.path.join(self.img_dir, str(self.imgname[i])) for i in idx]
        if flow_ragged_crops(self._ragged_crops):     # the batch's images in one slab, one upload, one launch into the batch tensor
            slab, offsets, shapes = decode_frames(paths, device, self._jpeg_decode_device, self._png_decode_device)     # off: pack_frames of read_image_rgb's decodes
            img = dataset_crops_ragged(slab, offsets, shapes, np.arange(len(paths), dtype=np.int32), d['center'][idx], d['scale'][idx],
                                       img_res, dtype=dtype)                                                    # cam_dataset.py:367-377
        else:
            crops, shapes = [], []
            for i, p in zip(idx, paths):
                frame = torch.from_numpy(read_image_rgb(p)).to(device)
                crops.append(dataset_crops(frame, d['center'][i:i + 1], d['scale'][i:i + 1], img_res, dtype=dtype))   # cam_dataset.py:367-377
                shapes.append(tuple(frame.shape[:2]))
            img = torch.cat(crops)
        shapes = np.asarray(shapes, np.float32)
        f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(device)
        img_h, img_w = f(shapes[:, 0]), f(shapes[:, 1])
        if use_gt_cam:
            R = f(d['cam_rotmat'][idx])
            if 'cam_int' in d:
                K = f(d['cam_int'][idx])
            else:                                     # cam_dataset.py:586-604: built from focal_length, K[2,2] = 0
                fl = np.asarray(d['focal_length'][idx], np.float32).reshape(len(idx), -1)
                K = torch.zeros(len(idx), 3, 3, device=device)
                K[:, 0, 0], K[:, 1, 1] = f(fl[:, 0]), f(fl[:, -1])
                K[:, 0, 2], K[:, 1, 2] = img_w / 2, img_h / 2
        else:                                         # cam_dataset.py:617-653: precomputed CamCalib predictions
            R, K = cam_params_from_angles(d['camcalib_pitch'][idx], d['camcalib_roll'][idx], d['camcalib_f_pix'][idx],
                                          shapes[:, 1], shapes[:, 0], device=device)
        return {'img': img, 'cam_rotmat': R, 'cam_int': K, 'scale': f(d['scale'][idx]),
                'center': f(d['center'][idx]), 'img_h': img_h, 'img_w': img_w,
                'imgname': paths}


def keypoints_orig(data: dict, idx) -> np.ndarray:
    """``keypoints_orig`` of the samples ``idx`` (spec/dataset/cam_dataset.py:148-157,386-413): the 25 ``openpose`` and the 24
    ``part`` keypoints (x, y, confidence) in full-image pixels, zeros where the annotation file lacks them -> (n, 49, 3)."""
    n = len(idx)
    return np.concatenate([data['openpose'][idx] if 'openpose' in data else np.zeros((n, 25, 3)),
                           data['part'][idx] if 'part' in data else np.zeros((n, 24, 3))], axis=1)


def save_batch_picture(ds: 'EvalDataset', idx, pred, save_dir: str, dataloader_nb: int, batch_nb: int, device, panel0_device=None,
                       png_device=None) -> str:
    """``SPECTrainer.validation_summaries`` (spec/trainer.py:366-423) for one batch: ONE picture, of the batch's first image
    (``max_save_img = 1``) - the full image with the ground-truth 2D skeleton ``keypoints_orig`` (drawn on the device), the
    horizon line of the dataset's CamCalib prediction, the predicted mesh over it and the side view.  The render rotation is
    ``batch_euler2matrix([-pitch, 0, roll])`` = Rx(-pitch) Rz(roll), the focal length f_pix twice, the centre (W // 2, H // 2),
    all from the ``camcalib_*`` fields (what the dataset hands out as ``pred_cam_*``, whichever camera the model was given).
    ``panel0_device`` (None = ``engine.PANEL0_DEVICE_DEFAULT``): the line and caption are drawn on the device (the same bytes).
    ``png_device`` (None = ``engine.PNG_DEVICE_DEFAULT``, off): the picture of a ``.png`` image is encoded on the device (the same
    picture, other bytes than Pillow's).  -> the file written: ``save_dir/{epoch 0:04d}_{dataloader:02d}_{batch:05d}_{image 0:02d}_{basename}``."""
    from . import render
    d, i = ds.data, int(idx[0])
    imgname = os.path.join(ds.img_dir, str(ds.imgname[i]))
    image = read_image_rgb(imgname)
    pitch, roll, vfov, f_pix = (float(d[k][i]) for k in ('camcalib_pitch', 'camcalib_roll', 'camcalib_vfov', 'camcalib_f_pix'))
    cp, sp, cr, sr = np.cos(-pitch), np.sin(-pitch), np.cos(roll), np.sin(roll)
    rot = (np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])).astype(np.float32)
    h, w = image.shape[:2]
    os.makedirs(save_dir, exist_ok=True)
    save_filename = os.path.join(save_dir, f'{0:04d}_{dataloader_nb:02d}_{batch_nb:05d}_{0:02d}_{os.path.basename(imgname)}')
    render.render_image_group(image, pred['pred_cam_t'][0], pred['smpl_vertices'][0], rot, (f_pix, f_pix), (w // 2, h // 2),
                              save_filename=save_filename, keypoints_2d=keypoints_orig(d, idx[:1])[0],
                              cam_params=np.array([vfov, pitch, roll, f_pix]), device=device, panel0_device=panel0_device, png_device=png_device)
    return save_filename


def loss_module(hparams: dict):
    """``HMRCamLoss`` as ``SPECTrainer.__init__`` builds it (spec/trainer.py:57-66): the ``HMR.*_WEIGHT`` keys of the config
    where it has them, the constructor's defaults (= the defaults of spec/config.py:155-163) elsewhere."""
    from .losses import HMRCamLoss
    hm = hparams.get('HMR') or {}
    names = {'shape_loss_weight': 'SHAPE_LOSS_WEIGHT', 'keypoint_loss_weight': 'KEYPOINT_LOSS_WEIGHT', 'pose_loss_weight': 'POSE_LOSS_WEIGHT',
             'beta_loss_weight': 'BETA_LOSS_WEIGHT', 'openpose_train_weight': 'OPENPOSE_TRAIN_WEIGHT', 'gt_train_weight': 'GT_TRAIN_WEIGHT',
             'loss_weight': 'LOSS_WEIGHT', 'smpl_part_loss_weight': 'SMPL_PART_LOSS_WEIGHT'}
    return HMRCamLoss(**{k: hm[v] for k, v in names.items() if v in hm})


STEP_KEYS = ('mpjpe', 'pampjpe', 'mpjpe_24', 'pampjpe_24')     # the per-joint arrays of evaluation_results_<ds>.pkl (spec/trainer.py:341-344)


def step_accuracy(per_joint: Dict[str, np.ndarray], v2v) -> dict:
    """``acc`` of ``validation_epoch_end`` (spec/trainer.py:494-512) from the per-joint arrays (n, joints) in metres and the
    per-image ``v2v`` (n,): 1000 x the mean over the images of each image's mean over its joints, taken in float64."""
    img = lambda a: np.asarray(a, np.float64).mean(axis=-1)
    acc = {f'val_{k}': float(1000 * img(per_joint[k]).mean()) for k in STEP_KEYS}
    acc['val_v2v'] = float(1000 * np.asarray(v2v, np.float64).mean())
    return acc


def step_lines(ds_name: str, acc: dict) -> List[str]:
    """The five lines of ``validation_epoch_end`` in their multi-dataset form (spec/trainer.py:500-504), whatever the number of
    datasets: the dataset's name in front keeps them apart from ``compute_error``'s own ``MPJPE:`` lines."""
    return [f'{ds_name} MPJPE: ' + str(acc['val_mpjpe']), f'{ds_name} PA-MPJPE: ' + str(acc['val_pampjpe']),
            f'{ds_name} MPJPE (24j): ' + str(acc['val_mpjpe_24']), f'{ds_name} PA-MPJPE (24j): ' + str(acc['val_pampjpe_24']),
            f'{ds_name} V2V: ' + str(acc['val_v2v'])]


def write_val_accuracy(log_dir: str, ds_name: str, acc: dict) -> str:
    """``val_save_best_results`` (spec/trainer.py:655-662) of a test run: ``val_accuracy_results_<ds>.json`` holding
    ``[[global_step, acc, epoch]]`` with step and epoch 0."""
    import json
    path = os.path.join(log_dir, f'val_accuracy_results_{ds_name}.json')
    os.makedirs(log_dir, exist_ok=True)
    with open(path, 'w') as f:
        json.dump([[0, acc, 0]], f, indent=4)
    return path


@torch.no_grad()
def run_evaluation(hparams: dict, data_root: str = '.', ckpt: Optional[str] = None, log=print, limit: Optional[int] = None,
                   device='cuda', loss: bool = False, step_metrics: bool = True) -> Dict[str, dict]:
    """Test + compute_error for every dataset of ``DATASET.VAL_DS``; returns {dataset: compute_error result}.
    ``step_metrics``: every batch is also scored as ``SPECTrainer.validation_step`` scores it (spec/trainer.py:272-344) - against
    the dataset's own ground truth (``EvalDataset.eval_gt``), per joint, in one launch (``metrics.validation_errors``); the four
    per-joint arrays go into ``evaluation_results_<ds>.pkl``, and per dataset the five lines of ``validation_epoch_end``
    (``step_lines``) are logged, ``val_accuracy_results_<ds>.json`` is written and the result carries ``'step'`` = {'acc', 'per_sample'}.
    Off: the log, the pkl and the folder are what they were without it.  ``loss``: every
    batch also goes through ``HMRCamLoss`` (the objective the checkpoint was trained under, spec/trainer.py:141-168, with the
    ground-truth vertices of the body model); the mean of each key over the run's images (a batch's dict weighted by its size) is
    logged after the error lines and returned under ``'loss'``.  Off by default: the log and the files are then unchanged.
    ``TESTING.SAVE_IMAGES`` with ``TESTING.SAVE_FREQ`` (spec/trainer.py:355-357): every SAVE_FREQ-th batch one picture of the
    batch's first image (``save_batch_picture``) goes to ``LOG_DIR/output_images`` - written only when ``TRAINING.SAVE_IMAGES``
    is set too, the reference's quirk (:402), kept.  Error lines and result files do not change."""
    from .modules import HMR
    dev = torch.device(device)
    if hparams.get('METHOD') != 'hmr_cam':
        raise ValueError(f"METHOD {hparams.get('METHOD')!r} is undefined (spec/trainer.py:47-69 builds HMR for 'hmr_cam' only)")
    testing, training = hparams.get('TESTING') or {}, hparams.get('TRAINING') or {}
    save_images = bool(testing.get('SAVE_IMAGES', False)) and bool(training.get('SAVE_IMAGES', False))
    save_freq = max(1, int(testing.get('SAVE_FREQ', 1)))
    cwd = os.getcwd()
    os.chdir(data_root)                     # the reference's asset paths are relative to the repo root
    try:
        assets.load_assets()
        if save_images:
            assets.faces()                  # the pictures' face table is read from the model file on first use: while its path resolves
        hm = HMR(backbone=hparams['HMR']['BACKBONE'], img_res=hparams['DATASET']['IMG_RES'], pretrained=None,
                 use_cam_feats=bool(hparams['HMR']['USE_CAM_FEATS']), use_cam=True)
        ckpt = ckpt or hparams['TRAINING']['PRETRAINED_LIT']
        if ckpt is None:
            raise ValueError('no checkpoint: set TRAINING.PRETRAINED_LIT in the config or pass --ckpt')
        state = read_checkpoint(ckpt)['state_dict']
        load_pretrained_model(hm, state, overwrite_shape_mismatch=True, remove_lightning=True)
        Jh36m = np.load('data/J_regressor_h36m.npy')
    finally:
        os.chdir(cwd)
    precision = eval_precision(hparams)
    if precision == 'fp16':
        log('Using native 16bit precision (TRAINING.USE_AMP): the ResNet trunk runs in fp16, heads and SMPL in fp32')
    hm.set_precision(precision)           # (no engine yet: recorded, packed by the commit below)
    hm.to(dev).eval().commit(dev, freeze=True)
    body = metrics.BodyModel(assets.smpl_model(), device=dev)
    Jh36m_dev = torch.as_tensor(np.asarray(Jh36m), dtype=torch.float32).to(dev)
    bs = int(hparams['DATASET']['BATCH_SIZE'])
    log_dir = hparams['LOG_DIR'] if os.path.isabs(hparams['LOG_DIR']) else os.path.join(data_root, hparams['LOG_DIR'])
    results = {}
    for dataloader_nb, name in enumerate(str(hparams['DATASET']['VAL_DS']).split('_')):
        ds = EvalDataset(name, data_root)
        n = len(ds) if limit is None else min(limit, len(ds))
        dump = io_formats.EvalDump()
        loss_fn, loss_sum = (loss_module(hparams), None) if loss else (None, None)
        step_v2v = []
        for b0 in range(0, n, bs):
            idx = np.arange(b0, min(n, b0 + bs))
            b = ds.batch(idx, dev, hparams['DATASET']['IMG_RES'], bool(hparams['TESTING']['USE_GT_CAM']), dtype=flow_image_dtype(hm))
            # positional call of spec/trainer.py:139
            pred = hm(b['img'], b['cam_rotmat'], b['cam_int'], b['scale'], b['center'], b['img_w'], b['img_h'])
            if step_metrics:
                gt = ds.eval_gt(idx, dev, body)
                pred_joints_24 = body.native(pred['pred_pose'], pred['pred_shape'], vertices=False)[1]              # spec/trainer.py:249-254
                e = metrics.validation_errors(pred['smpl_vertices'], gt['vertices'], Jh36m_dev, pred_joints_24, gt['joints_24'])
                dump.add(pred, imgnames=b['imgname'], dataset_name=name, mpjpe=e['err_sel'][:, :14], pampjpe=e['pa_err_sel'][:, :14],
                         mpjpe_24=e['err_k'], pampjpe_24=e['pa_err_k'])                                              # :341-344
                step_v2v.append(e['v2v'].cpu().numpy())
            else:
                dump.add(pred, imgnames=b['imgname'], dataset_name=name)
            if save_images and (b0 // bs) % save_freq == 0:
                log(f"wrote {save_batch_picture(ds, idx, pred, os.path.join(log_dir, 'output_images'), dataloader_nb, b0 // bs, dev)}")
            if loss_fn is not None:
                gt = ds.loss_gt(idx, torch.stack([b['img_h'], b['img_w']], 1), dev)
                gt['vertices'] = body.native(gt['pose'], gt['betas'], vertices=True, joints24=False)[0]      # spec/trainer.py:149-155,166
                means = torch.stack(list(loss_fn(pred, gt)[1].values())).double() * len(idx)
                loss_sum = means if loss_sum is None else loss_sum + means
        step = None
        if step_metrics:
            per = {k: np.concatenate(dump.errors[k]) for k in STEP_KEYS}
            per['v2v'] = np.concatenate(step_v2v)
            step = {'acc': step_accuracy(per, per['v2v']), 'per_sample': per}
            for line in step_lines(name, step['acc']):
                log(line)
            log(f"wrote {write_val_accuracy(log_dir, name, step['acc'])}")
        path = dump.write(log_dir, name)
        log(f'wrote {path}')
        if n != len(ds):                            # a truncated run scores the truncated annotations
            sub = os.path.join(log_dir, f'_annotations_{name}_first{n}.npz')
            np.savez(sub, **{k: v[:n] for k, v in ds.data.items() if getattr(v, 'shape', ()) and v.shape[0] == len(ds)})
            res = metrics.compute_error(path, dataset_file=sub, data_root=data_root, body_model=body,
                                        J_regressor_h36m=Jh36m, log=log)
        else:
            res = metrics.compute_error(path, data_root=data_root, body_model=body, J_regressor_h36m=Jh36m, log=log)
        m = res['mean']
        ours = ((m['wmpjpe'], m['pampjpe'], m['wv2v']) if name == '3dpw-test-cam'
                else (m['wmpjpe_24'], m['pampjpe_24'], m['wv2v']))
        ref = README_TABLE.get(name)
        if ref:
            log(f'{name}: W-MPJPE {ours[0]:.1f} (README {ref[0]})  PA-MPJPE {ours[1]:.1f} (README {ref[1]})  '
                f'W-PVE {ours[2]:.1f} (README {ref[2]})')
            # the number BASELINE.json asks for: |delta W-MPJPE| vs the reference's published table (README.md:155-159);
            # meaningful only on the real assets - a stand-in tree holds synthetic weights
            d = [ours[i] - ref[i] for i in range(3)]
            log(f'{name}: delta vs README  W-MPJPE {d[0]:+.2f} mm  PA-MPJPE {d[1]:+.2f} mm  W-PVE {d[2]:+.2f} mm  '
                f'(target |delta W-MPJPE| <= 0.1 mm: {"met" if abs(d[0]) <= 0.1 else "NOT met"})')
            res['readme_delta_mm'] = {'wmpjpe': d[0], 'pampjpe': d[1], 'wpve': d[2]}
        res['precision'] = precision
        if step is not None:
            res['step'] = step
        if loss_fn is not None:
            from .engine import HMR_LOSS_KEYS
            res['loss'] = dict(zip(HMR_LOSS_KEYS, (loss_sum / n).tolist()))
            for k, v in res['loss'].items():
                log(f'{k}: {v:.6g}')
        results[name] = res
    return results


# ------------------------------------------------------------------------------------------------------------
# stand-in ``data/`` tree in the REAL container formats (tests / dry runs; the licensed files cannot ship)
# ------------------------------------------------------------------------------------------------------------
def write_standin_data_tree(root: str, n_images: int = 6, seed: int = 7, dataset: str = 'spec-syn',
                            hmr_seed: int = 1002, smpl_seed: int = 1003, keypoints: bool = False) -> dict:
    """Writes under ``root`` everything run_evaluation reads, with synthetic numbers but the real formats: a Lightning
    ``.ckpt`` (``model.``-prefixed keys, trainer-level ``smpl.*`` / ``J_regressor`` keys that must be ignored, a pickled
    foreign hyper-parameter class), an SMPL ``.pkl`` with chumpy-pickled and scipy-sparse members, the ``.npy`` / ``.npz``
    side files, the yacs-style YAML, annotations and PNG frames.  ``keypoints``: the annotations also hold ``openpose``
    (n, 25, 3) and ``part`` (n, 24, 3) 2D keypoints (x, y in pixels of the frame - some beyond it -, confidences on both sides
    of 0.3 and exact zeros), drawn from a generator of their own: everything else in the tree is unchanged by the switch.
    Returns the ground truth it used."""
    import pickle
    import scipy.sparse as sp
    import yaml
    from PIL import Image
    from . import synth
    rng = np.random.default_rng(seed)
    j = lambda *p: os.path.join(root, *p)
    for d in ('data/body_models/smpl', 'data/spec/checkpoints', f'data/dataset_folders/{dataset}/annotations',
              f'data/dataset_folders/{dataset}/images', 'data/camcalib/checkpoints', 'data/sample_images'):
        os.makedirs(j(d), exist_ok=True)
    model = synth.smpl_model(smpl_seed)
    V = model['v_template'].shape[0]

    # ---- SMPL pickle: chumpy arrays (class chumpy.ch.Ch, state {'x': array}) + scipy sparse J_regressor -------
    import sys
    import types
    ch_mod, ch_sub = types.ModuleType('chumpy'), types.ModuleType('chumpy.ch')

    class Ch:                                      # pickles as chumpy.ch.Ch, like the official SMPL files
        def __init__(self, x):
            self.x = np.asarray(x)

        def __getstate__(self):
            return {'x': self.x}
    Ch.__module__, Ch.__qualname__ = 'chumpy.ch', 'Ch'
    ch_sub.Ch = Ch
    ch_mod.ch = ch_sub
    saved = {k: sys.modules.get(k) for k in ('chumpy', 'chumpy.ch')}
    sys.modules['chumpy'], sys.modules['chumpy.ch'] = ch_mod, ch_sub
    try:
        kintree = np.stack([np.where(model['parents'] < 0, 2 ** 32 - 1, model['parents']).astype(np.uint32),
                            np.arange(24, dtype=np.uint32)])
        smpl_pkl = {
            'v_template': Ch(model['v_template'].astype(np.float64)),
            'shapedirs': Ch(model['shapedirs'].astype(np.float64)),
            'posedirs': Ch(model['posedirs'].T.reshape(V, 3, 207).astype(np.float64)),
            'J_regressor': sp.csc_matrix(model['J_regressor'].astype(np.float64)),
            'weights': Ch(model['lbs_weights'].astype(np.float64)),
            'kintree_table': kintree, 'f': synth.smpl_faces(model['v_template']).astype(np.uint32),
            'bs_type': 'lrotmin', 'bs_style': 'lbs',
        }
        with open(j('data/body_models/smpl/SMPL_NEUTRAL.pkl'), 'wb') as f:
            pickle.dump(smpl_pkl, f, protocol=2)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    np.save(j('data/J_regressor_extra.npy'), model['J_regressor_extra'])
    np.save(j('data/J_regressor_h36m.npy'), synth.h36m_regressor(smpl_seed))
    mean = {'pose': np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), 24), 'shape': np.zeros(10, np.float32),
            'cam': np.array([0.9, 0., 0.], np.float32)}
    np.savez(j('data/smpl_mean_params.npz'), **mean)

    # ---- Lightning checkpoint -------------------------------------------------------------------------------
    hs = synth.hmr_state(hmr_seed, True)
    sd = {'model.' + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in hs.items()}
    sd['model.backbone.bn1.num_batches_tracked'] = torch.tensor(7)
    for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'lbs_weights'):      # smplx buffers of model.smpl.smpl
        sd['model.smpl.smpl.' + k] = torch.from_numpy(np.ascontiguousarray(model[k]))
        sd['smpl.' + k] = sd['model.smpl.smpl.' + k]                                      # trainer-level copies: ignored
        sd['smpl_native.' + k] = sd['model.smpl.smpl.' + k]
    sd['J_regressor'] = torch.from_numpy(synth.h36m_regressor(smpl_seed))
    fake_mod = types.ModuleType('yacs.config')

    class CfgNode(dict):
        pass
    CfgNode.__module__, CfgNode.__qualname__ = 'yacs.config', 'CfgNode'
    fake_mod.CfgNode = CfgNode
    yacs_pkg = types.ModuleType('yacs')
    yacs_pkg.config = fake_mod
    saved = {k: sys.modules.get(k) for k in ('yacs', 'yacs.config')}
    sys.modules['yacs'], sys.modules['yacs.config'] = yacs_pkg, fake_mod
    try:
        torch.save({'epoch': 3, 'global_step': 1234, 'pytorch-lightning_version': '1.1.8', 'state_dict': sd,
                    'hyper_parameters': CfgNode(METHOD='hmr_cam', HMR=CfgNode(USE_CAM_FEATS=True))},
                   j('data/spec/checkpoints/spec_checkpoint.ckpt'))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    # CamCalib Lightning checkpoint (scripts/camcalib_demo.py:39,80-81: strict load after stripping 'model.')
    cs = synth.camcalib_state(1001)
    torch.save({'epoch': 26, 'global_step': 337742,
                'state_dict': {'model.' + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cs.items()}},
               j('data/camcalib/checkpoints/camcalib_sa_biased_l2.ckpt'))
    for i in range(2):                                             # data/sample_images of the demo (README.md:100-104)
        Image.fromarray((rng.random((300, 420, 3)) * 255).astype(np.uint8)).save(j('data/sample_images', f'im{i}.png'))
    with open(j('data/spec/checkpoints/spec_config.yaml'), 'w') as f:
        yaml.safe_dump({'METHOD': 'hmr_cam', 'LOG_DIR': 'logs/eval_standin',
                        'DATASET': {'BATCH_SIZE': 4, 'VAL_DS': dataset, 'IMG_RES': 224},
                        'TRAINING': {'PRETRAINED_LIT': 'data/spec/checkpoints/spec_checkpoint.ckpt'},
                        'HMR': {'BACKBONE': 'resnet50', 'USE_CAM_FEATS': True}}, f)

    # ---- annotations + frames -------------------------------------------------------------------------------
    H, W = 360, 480
    names = []
    for i in range(n_images):
        img = (rng.random((H, W, 3)) * 255).astype(np.uint8)
        names.append(f'images/frame_{i:04d}.png')
        Image.fromarray(img).save(j(f'data/dataset_folders/{dataset}', names[-1]))
    pose = (rng.standard_normal((n_images, 72)) * 0.25).astype(np.float64)
    pose[0] = 0.0                                              # zero pose: Rodrigues at the 1e-8 guard
    shape = (rng.standard_normal((n_images, 10)) * 0.5).astype(np.float64)
    pitch = rng.uniform(-0.4, 0.4, n_images).astype(np.float32)
    roll = rng.uniform(-0.2, 0.2, n_images).astype(np.float32)
    vfov = rng.uniform(0.6, 1.4, n_images).astype(np.float32)
    f_pix = (H / 2. / np.tan(vfov / 2.)).astype(np.float64)
    def rx_rz(p, r):                                           # any rotation serves as stand-in ground truth
        cp, sp_, cr, sr = np.cos(p), np.sin(p), np.cos(r), np.sin(r)
        Rx = np.array([[1, 0, 0], [0, cp, -sp_], [0, sp_, cp]])
        Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
        return Rx @ Rz
    Rgt = np.stack([rx_rz(p + 0.03, r - 0.02) for p, r in zip(pitch, roll)])
    ann = {'imgname': np.array(names), 'scale': rng.uniform(0.9, 1.5, n_images), 'pose': pose, 'shape': shape,
           'center': np.stack([rng.uniform(150, 330, n_images), rng.uniform(120, 240, n_images)], 1),
           'cam_rotmat': Rgt.astype(np.float64), 'camcalib_pitch': pitch, 'camcalib_roll': roll,
           'camcalib_vfov': vfov, 'camcalib_f_pix': f_pix}
    if dataset != 'spec-syn':
        ann['pose_cam'] = (rng.standard_normal((n_images, 72)) * 0.25).astype(np.float64)
        import joblib
        joblib.dump(torch.from_numpy(Rgt), j(f'data/camcalib/{dataset}_cam_rotmat.pkl'))
    if keypoints:
        krng = np.random.default_rng(seed + 1000003)
        for key, nj in (('openpose', 25), ('part', 24)):
            kp = np.concatenate([krng.uniform(-20, W + 20, (n_images, nj, 1)), krng.uniform(-20, H + 20, (n_images, nj, 1)),
                                 krng.uniform(0.0, 1.0, (n_images, nj, 1))], axis=2)
            kp[:, ::5, 2] = 0.0                                      # unannotated joints
            ann[key] = kp
    np.savez(j(DATASET_FILES[dataset]), **ann)
    return {'annotations': ann, 'smpl_model': model, 'hmr_state': hs, 'camcalib_state': cs, 'frame_hw': (H, W)}
