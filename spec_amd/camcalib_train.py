"""Fine-tuning of CamCalib on MI355X - the heads, or the heads and the last ResNet stage: the reference's ``training_step`` (camcalib/trainer.py:60-82 - network ->
``CameraRegressorLoss`` -> ``loss.backward()`` -> ``torch.optim.Adam``, :201-205) on a FROZEN, committed trunk.  What is trained are
the three FC heads (``fc_vfov`` / ``fc_pitch`` / ``fc_roll``) on the trunk's pooled features - what adapting the released
checkpoint to one's own cameras needs, with labelled views such as ``spec_amd.panorama`` cuts out of panoramas.

Per batch: ``DATASET.BATCH_SIZE`` frames in a seeded shuffle, resized and padded as the test step does (``camcalib_eval.pad_batch``),
``Engine.trunk`` under ``no_grad`` -> ``differentiable.CameraRegressorHead`` (sharing the model's Parameters) ->
``losses.CameraRegressorLoss(MODEL.LOSS_*)`` -> ``backward()`` -> ``torch.optim.Adam(lr=OPTIMIZER.LR, weight_decay=OPTIMIZER.WD)``.
The targets come from ``camcalib_eval.encode_targets``.  The optimiser is torch's; forward, loss and both backwards run in the
library (``specmi_camcalib_head_train_forward`` / ``_backward``, ``specmi_camcalib_loss`` / ``_backward``).

``augment=True`` adds the one step by which the reference's training dataset differs from its validation half
(camcalib/pano_dataset.py:62-78): ``ColorJitter(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1)`` on every frame before
the resize, applied to the batch's uint8 slab on the device in Pillow's bytes (``spec_amd.augment``, ``specmi_color_jitter``).
``split='train'`` reads the frames ``train_images.pkl`` lists instead of ``val_images.pkl``'s.

``unfreeze=('layer4',)`` trains the last ResNet stage with the heads, the usual recipe for adapting a released checkpoint: the
frozen part is ``Engine.trunk(images, stages=3)`` under ``no_grad``, then ``differentiable.ResNetStage`` (layer4 on FROZEN BatchNorm
statistics, sharing the model's conv weights; ``specmi_conv2d_train_forward`` / ``specmi_conv2d_backward``) -> the heads -> the loss
-> ``backward()``, and Adam steps the head parameters and the stage's conv weights.  The written checkpoint holds the stepped trunk
weights and the after-evaluation runs on the recommitted model.

``bn='batch'`` (with ``unfreeze=('layer4',)``) is the reference's own semantics - its trainer is a Lightning module, the network is
in ``train()`` during ``training_step``: the stage's blocks are put in ``train()`` for the epochs, every BatchNorm of layer4
normalises with the statistics of the batch (``specmi_batchnorm_train_forward`` / ``specmi_batchnorm_backward``), its running
statistics move and ``num_batches_tracked`` counts, and Adam steps gamma and beta too.  Afterwards the blocks go back to ``eval()``,
the model is committed again - the folded trunk carries the trained running statistics - and the checkpoint holds them.

``unfreeze`` also takes the longer suffixes of the trunk, down to ``'all'`` = the stem and layers 1-4, the reference's own
training mode (its trainer hands Adam every parameter): ``differentiable.ResNetTrunk`` runs what lies below the first trained part
frozen, then the trainable stem (conv7x7/2 -> BatchNorm -> ReLU -> max-pool with its gradient, ``specmi_maxpool3x3s2_backward``)
and stages; ``bn='batch'`` puts every unfrozen module in ``train()`` and hands Adam their gamma / beta.

Out of scope, as for the SPEC side: BasicBlock trunks, SyncBatchNorm across GPUs, an fp16 backward, 'pano_agora'
(the frames are those the tree's ``val_images.pkl`` / ``train_images.pkl`` list, or a ``dataset`` object with
``PanoValDataset``'s interface), second derivatives.
"""
from __future__ import annotations

import copy
import os
from typing import List, Optional

import numpy as np
import torch

from . import camcalib_eval as ce

# camcalib/config.py:63-66,72 over the test step's defaults
DEFAULTS = dict(copy.deepcopy(ce.DEFAULTS), OPTIMIZER={'TYPE': 'adam', 'LR': 0.001, 'WD': 0.0})
TRAIN_KEYS = ('train/loss', 'train/vfov_loss', 'train/pitch_loss', 'train/roll_loss')


def load_config(cfg_path: Optional[str], opts: Optional[List[str]] = None) -> dict:
    """``camcalib_eval.load_config`` with the optimiser keys of camcalib/config.py among the defaults."""
    from . import evaluation
    return evaluation.load_config(cfg_path, opts, defaults=DEFAULTS)


def trunk_features(model, images: torch.Tensor, stages: Optional[int] = None) -> torch.Tensor:
    """The frozen trunk on one padded batch -> (n, fh, fw, C) NHWC features, whole images in sub-batches of
    ``camcalib_eval.forward_limit`` (bit-identical under the pinned plan).  ``stages``: the trunk cut after that stage
    (``Engine.trunk``)."""
    eng = model.engine(images.device)
    n, _, H, W = images.shape
    step = ce.forward_limit(H, W)
    kw = {} if stages is None else {'stages': stages}
    with torch.no_grad():
        if step >= n:
            return eng.trunk(images, **kw)
        return torch.cat([eng.trunk(images[b0:b0 + step], **kw) for b0 in range(0, n, step)])


def write_checkpoint(model, path: str, epoch: int, global_step: int) -> str:
    """The model's state_dict in the Lightning layout ``camcalib_eval.build_model`` reads (``model.``-prefixed keys)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({'epoch': int(epoch), 'global_step': int(global_step), 'pytorch-lightning_version': '1.1.8',
                'state_dict': {'model.' + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}}, path)
    return path


def normalise_unfreeze(unfreeze) -> tuple:
    """``unfreeze`` as ``finetune_heads`` takes it -> () or a suffix of ('stem', 'layer1', 'layer2', 'layer3', 'layer4') in that
    order: 'all' is the whole trunk, the names may come in any order; anything that is not such a suffix - ('layer3',) alone, a part
    left out in the middle - is ``NotImplementedError``: a frozen part ABOVE a trained one is not built."""
    from .differentiable import TRUNK_PARTS
    if isinstance(unfreeze, str):
        unfreeze = TRUNK_PARTS if unfreeze == 'all' else (unfreeze,)
    names = tuple(unfreeze)
    if not names:
        return ()
    if len(set(names)) == len(names) and set(names) <= set(TRUNK_PARTS):
        suffix = TRUNK_PARTS[len(TRUNK_PARTS) - len(names):]
        if set(names) == set(suffix):
            return suffix
    raise NotImplementedError(f"unfreeze = {unfreeze!r}: (), 'all' and the suffixes of {TRUNK_PARTS} are built - the trained part reaches "
                              'from its first stage to layer4')


def finetune_heads(hparams: dict, data_root: str = '.', ckpt: Optional[str] = None, epochs: int = 1, seed: int = 0, out: Optional[str] = None,
                   dataset=None, model=None, log=print, device='cuda', evaluate: bool = True, augment: bool = False, augment_seed: int = 0,
                   split: str = 'val', unfreeze=(), bn: str = 'frozen') -> dict:
    """Fine-tuning (module docstring) for ``epochs`` passes over the labelled frames.  Logs the four ``train/...`` means
    per epoch, runs ``camcalib_eval.run_evaluation`` before and after (``evaluate``), and writes the Lightning-layout checkpoint
    ``out`` (None: ``LOG_DIR/camcalib_finetuned.ckpt``).  -> dict(model, ckpt, epochs = the per-epoch means, before / after = the
    evaluations' four epoch figures).  ``augment``: every batch is packed into a uint8 device slab (or taken as
    ``device_batch`` hands it over), jittered by ``augment.ColorJitter`` with the reference's four settings - the parameters drawn
    frame by frame from a torch CPU generator seeded with ``augment_seed`` - and resized from there; False: exactly the flow
    without it.  ``split``: which list of the tree the training frames come from (the evaluations keep reading 'val').
    ``unfreeze``: ``()`` trains the heads alone; ``('layer4',)`` also the conv weights of the last ResNet stage on frozen BatchNorm;
    the longer suffixes of the trunk - ('layer3', 'layer4') ... ('stem', 'layer1', 'layer2', 'layer3', 'layer4') = 'all', in any
    order - train from that part upwards through ``differentiable.ResNetTrunk`` (``normalise_unfreeze``).  ``bn``: 'frozen' = the stage on its running statistics, gamma / beta untouched; 'batch' = the stage
    in ``train()`` on batch statistics, gamma / beta trained, the running statistics moved (module docstring) - refused with
    ``unfreeze=()``, where no BatchNorm is trained."""
    from .differentiable import CameraRegressorHead, ResNetStage, ResNetTrunk
    unfreeze = normalise_unfreeze(unfreeze)
    if bn not in ('frozen', 'batch'):
        raise ValueError(f"bn = {bn!r}: 'frozen' and 'batch' are built")
    if bn == 'batch' and not unfreeze:
        raise ValueError("bn = 'batch' trains the BatchNorms of an unfrozen stage: pass unfreeze=('layer4',)")
    from .losses import CameraRegressorLoss
    dev = torch.device(device)
    m = hparams['MODEL']
    if m['LOSS_TYPE'] not in ce.LOSS_TYPES:
        raise ValueError(f"{m['LOSS_TYPE']} is not defined..")
    opt_cfg = dict(DEFAULTS['OPTIMIZER'], **(hparams.get('OPTIMIZER') or {}))
    if str(opt_cfg['TYPE']).lower() != 'adam':
        raise NotImplementedError(f"OPTIMIZER.TYPE {opt_cfg['TYPE']!r}: the reference's configure_optimizers builds Adam (camcalib/trainer.py:201-205)")
    ds = dataset if dataset is not None else ce.PanoValDataset(ce.val_dataset_name(hparams), data_root, split=split)
    if model is None:
        model = ce.build_model(hparams, ckpt, data_root, dev)
    else:
        model.set_plan('throughput')
    figures = ('val_loss', 'vfov_acc', 'pitch_acc', 'roll_acc')
    run_eval = lambda: {k: v for k, v in ce.run_evaluation(hparams, data_root, model=model, dataset=dataset, log=log, device=dev,
                                                          save_images=False).items() if k in figures}
    before = run_eval() if evaluate else None
    head = CameraRegressorHead.from_model(model)
    crit = CameraRegressorLoss(float(m['LOSS_VFOV_WEIGHT']), float(m['LOSS_PITCH_WEIGHT']), float(m['LOSS_ROLL_WEIGHT']), m['LOSS_TYPE'])
    # ('layer4',) keeps the stage on the trunk cut after layer3; a longer suffix is a ResNetTrunk whose frozen part, if any, runs below it
    stage = trunk = None
    if unfreeze == ('layer4',):
        stage = ResNetStage.from_model(model, 'layer4', bn)
    elif unfreeze:
        # what lies below layer2 .. layer4 runs in sub-batches, as the head-only flow; a frozen stem below layer1 takes the batch whole
        trunk = ResNetTrunk.from_model(model, unfreeze[0], bn, cut_trunk=lambda images, k: trunk_features(model, images, stages=k))
    part = stage if stage is not None else trunk
    trained = list(head.parameters()) + (part.conv_parameters() if part is not None else []) + (part.bn_parameters() if bn == 'batch' else [])
    optim = torch.optim.Adam(trained, lr=float(opt_cfg['LR']), weight_decay=float(opt_cfg['WD']))
    bs, min_res, max_res = int(hparams['DATASET']['BATCH_SIZE']), int(hparams['DATASET']['MIN_RES']), hparams['DATASET']['MAX_RES']
    rng = np.random.default_rng(seed)
    eng = model.engine(dev)
    jitter = jitter_rng = None
    if augment:
        from .augment import CAMCALIB_TRAIN_JITTER, ColorJitter
        from .preprocess import pack_frames
        jitter, jitter_rng = ColorJitter(**CAMCALIB_TRAIN_JITTER), torch.Generator().manual_seed(int(augment_seed))
    log(f'Train dataset len: {len(ds)}')
    history, step = [], 0
    train_mode = [] if bn != 'batch' else [stage.blocks] if stage is not None else trunk.trained_modules()
    for mod in train_mode:
        mod.train()                           # the unfrozen modules alone: the model itself has no training mode
    for epoch in range(int(epochs)):
        order = rng.permutation(len(ds))
        sums = torch.zeros(4, device=dev)
        nb = 0
        for b0 in range(0, len(ds), bs):
            idx = [int(i) for i in order[b0:b0 + bs]]
            frames = ds.device_batch(idx) if hasattr(ds, 'device_batch') else [ds.frame(i) for i in idx]
            gt = np.asarray([ds.labels(i) for i in idx], dtype=np.float64).T
            if jitter is not None:
                frames = jitter(frames if isinstance(frames, tuple) else pack_frames(frames, dev), jitter_rng, engine=eng)
            images = ce.pad_batch(frames, min_res, max_res, dev, eng)
            feat = None if trunk is not None else trunk_features(model, images, stages=3 if stage is not None else None)
            with torch.enable_grad():
                if stage is not None:
                    feat = stage(feat)
                elif trunk is not None:
                    feat = trunk(images)
                loss, loss_dict = crit(*head(feat, channels_last=True), *ce.encode_targets(*gt, m['LOSS_TYPE']))
                optim.zero_grad(set_to_none=True)
                loss.backward()
            optim.step()
            sums += torch.stack([loss_dict[k].detach() for k in ('loss', 'vfov_loss', 'pitch_loss', 'roll_loss')])
            nb += 1
            step += 1
        means = (sums / max(nb, 1)).cpu().tolist()
        history.append(dict(zip(TRAIN_KEYS, (float(v) for v in means))))
        log(f'[EPOCH {epoch}] ' + ', '.join(f'{k}: {v:.6g}' for k, v in history[-1].items()))
    for mod in train_mode:
        mod.eval()
    model.commit(dev, freeze=True)            # the frozen model skips the per-forward check: commit the stepped weights now
    after = run_eval() if evaluate else None
    if out is None:
        log_dir = hparams['LOG_DIR'] if os.path.isabs(hparams['LOG_DIR']) else os.path.join(data_root, hparams['LOG_DIR'])
        out = os.path.join(log_dir, 'camcalib_finetuned.ckpt')
    path = write_checkpoint(model, out, int(epochs), step)
    log(f'checkpoint written to {path}')
    return {'model': model, 'ckpt': path, 'epochs': history, 'before': before, 'after': after}
