#!/usr/bin/env python
"""Throughput of the non-headline model variants of the path, one JSON line each:
HMR on the HRNet-W32 / W48 trunks (spec/models/hmr.py:44-51) and CamCalib on ResNet-34 (camcalib/config.py:81); ``--fp16``:
the C3 step (CamCalib + SPEC + SMPL) with the fp16 trunk (TRAINING.USE_AMP) against fp32, timed alternately in one process,
with a parity block; ``--f16-input``: the fp16 C3 step from device-resident uint8 frames and boxes, fp32 crops + conversion
against NHWC8 fp16 crops read by the stem ("Input").  Not the BASELINE.json metric (bench.py measures that); numbers quoted in DESIGN.md section 7."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--only', default='', help='comma-separated backbones (default: all)')
    ap.add_argument('--labels', type=int, default=0, help='also print the N most expensive (kernel, layer group) rows')
    ap.add_argument('--fp16', action='store_true', help='only the fp16-trunk C3 step against fp32 (one JSON line)')
    ap.add_argument('--rounds', type=int, default=3, help='--fp16: alternating fp32 / fp16 timing rounds')
    ap.add_argument('--f16-input', action='store_true', help='only the fp16 C3 step from uint8 frames: fp32 crops + conversion vs NHWC8 fp16 crops')
    ap.add_argument('--layers', action='store_true', help='--fp16: also print every fp16 trunk launch against its binding roof')
    args = ap.parse_args()
    from spec_amd import assets, synth
    from spec_amd.cam_utils import cam_params_from_angles
    from spec_amd.modules import HMR, CameraRegressorNetwork
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    assets.use_synthetic_assets(1003)
    B = args.batch
    x = t(synth.images(3, 16)).to(dev).repeat(B // 16 + 1, 1, 1, 1)[:B].contiguous()
    sc, ce, iw, ih = [t(a).to(dev) for a in synth.bbox_inputs(3, B, 224., 224., jitter=False)]
    R, K = cam_params_from_angles(np.full(B, 0.1, np.float32), np.full(B, -0.05, np.float32), np.full(B, 300., np.float32), iw, ih)
    if args.fp16:
        return fp16_step(args, dev, t, x, sc, ce, iw, ih)
    if args.f16_input:
        return f16_input_step(args, dev, t)
    for backbone in ('hrnet_w32-conv', 'hrnet_w32-interp', 'hrnet_w48-conv', 'resnet50'):
        if args.only and backbone not in args.only.split(','):
            continue
        hm = HMR(backbone=backbone, use_cam=True, use_cam_feats=True)
        hm.load_state_dict({k: t(v) for k, v in synth.hmr_state(1002, True, backbone=backbone).items()}, strict=False)
        hm.to(dev).eval().commit(dev, freeze=True)
        eng = hm.engine(dev)
        ms = timed(lambda: hm(x, R, K, sc, ce, iw, ih), args.steps)
        eng.profile(True)
        hm(x, R, K, sc, ce, iw, ih)
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile(False)
        by = {}
        for e in prof:
            by[e['kernel']] = by.get(e['kernel'], 0.0) + e['ms']
        top = sorted(by.items(), key=lambda kv: -kv[1])[:5]
        print(json.dumps({'variant': f'HMR({backbone}) forward', 'batch': B, 'ms_per_step': round(ms, 3),
                          'images_per_s': round(B * 1e3 / ms, 1), 'launches': len(prof) and sum(e['launches'] for e in prof),
                          'top_kernels_ms': {k: round(v, 3) for k, v in top}}), flush=True)
        if args.labels:
            import re
            grp = {}
            for e in prof:     # group layers that differ only in their indices
                key = (e['kernel'], re.sub(r'\d+', '#', e['label']))
                g = grp.setdefault(key, [0.0, 0, 0.0])
                g[0] += e['ms']; g[1] += e['launches']; g[2] += e['flops']
            for (kern, lab), (ms_, n, fl) in sorted(grp.items(), key=lambda kv: -kv[1][0])[:args.labels]:
                print(f'    {ms_:8.3f} ms x{n:<3d} {fl / max(ms_, 1e-9) / 1e9:7.1f} TF/s  {kern:<40s} {lab}', file=sys.stderr)
        del hm, eng
        torch.cuda.empty_cache()
    if args.only:
        return
    cc = CameraRegressorNetwork(backbone='resnet34')
    cc.load_state_dict({k: t(v) for k, v in synth.camcalib_state(1001, backbone='resnet34').items()})
    cc.to(dev).eval().commit(dev, freeze=True)
    ms = timed(lambda: cc(x), args.steps)
    print(json.dumps({'variant': 'CameraRegressorNetwork(resnet34) forward', 'batch': B, 'ms_per_step': round(ms, 3),
                      'images_per_s': round(B * 1e3 / ms, 1)}), flush=True)


def fp16_step(args, dev, t, x, sc, ce, iw, ih):
    """The C3 step (SpecPipeline: CamCalib -> decode -> SPEC -> SMPL -> projection) at fp32 and with the fp16 trunk on both
    networks, synthetic weights and crops, timed alternately (args.rounds rounds of >= 20 steps each after warming up every
    shape), plus a parity block of fp16 against fp32 on the same inputs."""
    from spec_amd import synth
    from spec_amd.modules import HMR, CameraRegressorNetwork
    from spec_amd.pipeline import SpecPipeline
    B = x.shape[0]
    pipes = {}
    for prec in ('fp32', 'fp16'):
        cc = CameraRegressorNetwork()
        cc.load_state_dict({k: t(v) for k, v in synth.camcalib_state(1001).items()})
        hm = HMR(use_cam=True, use_cam_feats=True)
        hm.load_state_dict({k: t(v) for k, v in synth.hmr_state(1002, True).items()}, strict=False)
        for m in (cc, hm):
            m.set_precision(prec)
            m.to(dev).eval().commit(dev, freeze=True)
        pipes[prec] = SpecPipeline(cc, hm)
    steps = max(20, args.steps)
    ms = {'fp32': [], 'fp16': []}
    for _ in range(args.rounds):
        for prec in ('fp32', 'fp16'):
            ms[prec].append(timed(lambda: pipes[prec](x, sc, ce, iw, ih), steps))
    o32 = {k: v.clone() for k, v in pipes['fp32'](x, sc, ce, iw, ih).items()}
    o16 = pipes['fp16'](x, sc, ce, iw, ih)
    torch.cuda.synchronize()
    v32, v16 = o32['smpl_vertices'].double(), o16['smpl_vertices'].double()
    mpjpe = (o16['smpl_joints3d'].double() - o32['smpl_joints3d'].double()).norm(dim=-1).mean(dim=-1) * 1000.0
    ang = {k: float(((o16['cam_' + k].double() - o32['cam_' + k].double()).abs().max()) * 180.0 / np.pi) for k in ('vfov', 'pitch', 'roll')}
    med = {p: float(np.median(v)) for p, v in ms.items()}
    print(json.dumps({'variant': 'C3 step fp16 trunk (TRAINING.USE_AMP) vs fp32', 'batch': B, 'steps_per_round': steps,
                      'rounds_ms_fp32': [round(v, 3) for v in ms['fp32']], 'rounds_ms_fp16': [round(v, 3) for v in ms['fp16']],
                      'ms_per_step_fp32': round(med['fp32'], 3), 'ms_per_step_fp16': round(med['fp16'], 3),
                      'images_per_s_fp32': round(B * 1e3 / med['fp32'], 1), 'images_per_s_fp16': round(B * 1e3 / med['fp16'], 1),
                      'ratio_fp16_over_fp32': round(med['fp16'] / med['fp32'], 4),
                      'parity': {'max_rel_vertex_err': float((v16 - v32).abs().max() / v32.abs().max()),
                                 'mpjpe_mm_mean': float(mpjpe.mean()), 'mpjpe_mm_max': float(mpjpe.max()),
                                 'camcalib_angle_deg_max': ang}}), flush=True)
    if args.layers:
        layer_roofs(pipes['fp16'].hmr.engine(dev), x)


def f16_input_step(args, dev, t):
    """The fp16 C3 step STARTING FROM uint8 frames and boxes in HBM (what every caller of the library has): (a) the crops as
    fp32 NCHW, converted inside each trunk (to_nhwc_f16) - the route before the fp16 entrance existed; (b) the crops as NHWC8 fp16,
    read by both stems where they lie.  Same models, same frames, alternated in one process (args.rounds rounds of >= 20 steps);
    the two routes must give the same bits.  (With NHWC8 input SpecPipeline never groups the two trunks into one launch per layer,
    which it does with fp32 input at B <= 3 and 17-20: run the leg with --batch 2 / 17 to see that difference.)  Also the device
    memory a 64-frame CamCalib validation batch (ragged producer + forward) holds on both routes, each on a fresh model:
    growth of the device's used memory (hipMemGetInfo: the library's hipMalloc workspaces and the caller's tensors), not torch's
    allocator statistics, which do not see the workspaces."""
    from spec_amd import synth
    from spec_amd import camcalib_eval as ce
    from spec_amd.modules import HMR, CameraRegressorNetwork
    from spec_amd.pipeline import SpecPipeline
    from spec_amd.preprocess import crop_detections_batch
    B, F, H, W = args.batch, 32, 720, 1280
    cc = CameraRegressorNetwork()
    cc.load_state_dict({k: t(v) for k, v in synth.camcalib_state(1001).items()})
    hm = HMR(use_cam=True, use_cam_feats=True)
    hm.load_state_dict({k: t(v) for k, v in synth.hmr_state(1002, True).items()}, strict=False)
    for m in (cc, hm):
        m.set_precision('fp16')
        m.to(dev).eval().commit(dev, freeze=True)
    pipe = SpecPipeline(cc, hm)
    g = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    fidx = (torch.arange(B, dtype=torch.int32) % F).to(dev)
    u = torch.rand(B, 4, generator=g)
    boxes = torch.stack([200 + u[:, 0] * (W - 400), 150 + u[:, 1] * (H - 300), 120 + u[:, 2] * 200, 200 + u[:, 3] * 300], 1).to(dev)
    iw, ih = torch.full((B,), float(W), device=dev), torch.full((B,), float(H), device=dev)
    bufs = {dt: {'inp_images': (torch.empty(B, 224, 224, 8, device=dev, dtype=dt) if dt == torch.float16 else torch.empty(B, 3, 224, 224, device=dev)),
                 'bbox_scale': torch.empty(B, device=dev), 'bbox_center': torch.empty(B, 2, device=dev)} for dt in (torch.float32, torch.float16)}

    def step(dt):
        c = crop_detections_batch(frames, fidx, boxes, crop_size=224, out=bufs[dt], dtype=dt)
        return pipe(c['inp_images'], c['bbox_scale'], c['bbox_center'], iw, ih)

    steps = max(20, args.steps)
    routes = {'fp32_crops': torch.float32, 'f16_crops': torch.float16}
    ms = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, dt in routes.items():
            ms[k].append(timed(lambda: step(dt), steps))
    oa = {k: v.clone() for k, v in step(torch.float32).items() if v is not None}
    ob = step(torch.float16)
    torch.cuda.synchronize()
    same = all(torch.equal(oa[k].view(torch.int32), ob[k].view(torch.int32)) for k in oa)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread_a = max(ms['fp32_crops']) - min(ms['fp32_crops'])
    # 64 ragged frames of a CamCalib validation batch (the sizes of profiles/camcalib_eval_aux.json: 600 x 1000 targets)
    rng = np.random.default_rng(0)
    val = [rng.integers(0, 256, (720 + 8 * (i % 5), 1200 + 16 * (i % 7), 3), dtype=np.uint8) for i in range(64)]
    del pipe, hm, cc, frames, bufs, oa, ob
    used = lambda: (lambda free, total: total - free)(*torch.cuda.mem_get_info(dev))
    peak = {}
    for k, dt in routes.items():
        m = CameraRegressorNetwork()                     # a fresh handle per route: its workspaces start empty
        m.load_state_dict({kk: t(v) for kk, v in synth.camcalib_state(1001).items()})
        m.set_precision('fp16'); m.set_plan('throughput')
        m.to(dev).eval().commit(dev, freeze=True)
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        base = used()
        x = ce.pad_batch(val, 600, 1000, dev, m.engine(dev), dtype=dt)
        after_producer = used()
        logits = ce.forward_padded(m, x)
        torch.cuda.synchronize()
        peak[k] = {'image_tensor_MB': round(x.numel() * x.element_size() / 1e6, 1), 'padded_shape': list(x.shape),
                   'device_used_after_producer_MB': round((after_producer - base) / 1e6, 1),
                   'device_used_after_forward_MB': round((used() - base) / 1e6, 1)}
        del x, logits
        m._engine.close(); del m
        torch.cuda.synchronize(); torch.cuda.empty_cache()
    print(json.dumps({'variant': 'fp16 C3 step from uint8 frames: fp32 crops + to_nhwc_f16 (a) vs NHWC8 fp16 crops (b)', 'batch': B,
                      'frames': [F, H, W], 'steps_per_round': steps,
                      'rounds_ms_a_fp32_crops': [round(v, 3) for v in ms['fp32_crops']], 'rounds_ms_b_f16_crops': [round(v, 3) for v in ms['f16_crops']],
                      'ms_per_step_a': round(med['fp32_crops'], 3), 'ms_per_step_b': round(med['f16_crops'], 3),
                      'ratio_b_over_a': round(med['f16_crops'] / med['fp32_crops'], 4), 'round_spread_ms_a': round(spread_a, 3),
                      'b_not_slower_beyond_spread_of_a': bool(med['f16_crops'] <= med['fp32_crops'] + spread_a),
                      'outputs_bit_identical': bool(same), 'camcalib_val_batch_64': peak}), flush=True)


# binding roofs of MI355X (MI355X_MICROARCH.md): dense fp16 MFMA ~2.5 PF, HBM3E 8.0 TB/s peak
PEAK_F16_FLOPS, PEAK_HBM_BYTES = 2.5e15, 8.0e12


def layer_roofs(eng, x):
    """Every launch of one fp16 trunk forward (built-in profiler: algorithmic FLOPs, and bytes at 2 B per fp16 element) against its
    binding roof: roof time = max(FLOPs / fp16 MFMA peak, bytes / HBM peak), share = roof time / measured time."""
    eng.trunk(x)
    torch.cuda.synchronize()
    eng.profile(True)
    eng.trunk(x)
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile(False)
    tot = sum(e['ms'] for e in prof)
    print(f'{"layer":<40s} {"kernel":<28s} {"ms":>8s} {"TF/s":>8s} {"TB/s":>7s} {"bound":>6s} {"share of roof":>13s}')
    for e in prof:
        t_f, t_b = e['flops'] / PEAK_F16_FLOPS * 1e3, e['bytes'] / PEAK_HBM_BYTES * 1e3
        print(f'{e["label"]:<40s} {e["kernel"]:<28s} {e["ms"]:8.3f} {e["flops"] / e["ms"] / 1e9:8.1f} {e["bytes"] / e["ms"] / 1e9:7.2f} '
              f'{"mfma" if t_f >= t_b else "hbm":>6s} {max(t_f, t_b) / e["ms"]:13.3f}')
    fl = sum(e['flops'] for e in prof)
    print(f'trunk B={x.shape[0]}: {tot:.3f} ms, {fl / 1e12:.3f} TFLOP, {fl / tot / 1e9:.1f} TF/s = {fl / tot * 1e3 / PEAK_F16_FLOPS:.3f} of the fp16 MFMA peak',
          flush=True)


if __name__ == '__main__':
    main()
