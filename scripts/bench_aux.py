#!/usr/bin/env python
"""Roofline of the kernels either side of the hot path (SURVEY.md 8f rows 1, 2, 4 and the C5 helpers): device crop /
resize pre-processing, evaluation metrics, the SMPL-only body model, CamCalib bin reductions.

Every kernel is timed by the library's own per-launch HIP events (``specmi_profile_enable`` - events recorded on the
launch stream around each kernel), averaged over ``--iters`` launches after a warm-up, and priced against the HBM roof
(8 TB/s) with the ALGORITHMIC bytes the launch reports (inputs read once + outputs written once, the figures DESIGN.md
section 3 states).  All of them are byte / gather work: none is reshaped into a GEMM.

    python scripts/bench_aux.py [--iters 20] [--out gpurun_out/aux_bench.json]
    python scripts/bench_aux.py --only camcalib_eval      # the two kernels of CamCalib's test step -> profiles/camcalib_eval_aux.json
    python scripts/bench_aux.py --only pano_views         # the panorama view extractor -> profiles/pano_views_aux.json
    python scripts/bench_aux.py --only ragged_crops       # crops from frames of different sizes, per-frame route against the ragged one -> profiles/ragged_crops_aux.json
    python scripts/bench_aux.py --only render             # mesh overlay + side view, 8 meshes on a 1080p frame, both raster launch shapes -> profiles/render_aux.json
    python scripts/bench_aux.py --only render_batch       # the pictures of a 32-frame flush, per-frame loop against the batched call -> profiles/render_batch_aux.json
    python scripts/bench_aux.py --only draw               # the 2D skeletons of a 1080p frame and of a 64-frame flush, next to render_views for the same flush -> profiles/draw_skeletons_aux.json
    python scripts/bench_aux.py --only jpeg_encode        # pictures to JPEG files: device encode + download of the bytes against raw download + Pillow -> profiles/jpeg_encode_aux.json
    python scripts/bench_aux.py --only png_encode         # pictures to PNG files: device encode + download of the bytes against raw download + Pillow -> profiles/png_encode_aux.json
    python scripts/bench_aux.py --only png_decode         # 64 1080p .png frames and 8 three-panel pictures to the frame slab: 16 Pillow threads + upload against streams up + device decode -> profiles/png_decode_aux.json
    python scripts/bench_aux.py --only jpeg_decode        # 64 1080p .jpg frames to the frame slab: 16 Pillow threads + upload against bytes up + device decode -> profiles/jpeg_decode_aux.json
    python scripts/bench_aux.py --only color_jitter       # ColorJitter on 64 1080p frames: the two launches next to a device-to-device copy; Pillow on 16 threads against the device call -> profiles/color_jitter_aux.json
    python scripts/bench_aux.py --only horizon_panel      # panel 0 of eight 1080p frames: Pillow on the host against specmi_draw_marks -> profiles/horizon_panel_aux.json
    python scripts/bench_aux.py --only hmr_loss           # the two launches of the loss forward (HMRCamLoss, per-vertex term on) -> profiles/hmr_loss_aux.json
    python scripts/bench_aux.py --only eval_step          # the validation step's one launch against eval_mesh + eval_joints (means only) -> profiles/eval_step_aux.json
    python scripts/bench_aux.py --head-train --out profiles/head_train_aux.json     # the trainable HMRHead's forward + backward at F = 2048, B = 64 and 256, next to torch autograd over the plain nn.Module on the same device
    python scripts/bench_aux.py --camcalib-train --out profiles/camcalib_train_aux.json     # CamCalib's three FC heads + CameraRegressorLoss, forward + backward with all gradients, at F = 2048, L = 1 and 3, B = 16 and 64: grouped against single launches, next to torch autograd
    python scripts/bench_aux.py --smpl-backward           # the SMPL head's forward, its backward and the loss backward at B = 256, V = 6890, next to torch autograd over the oracle chain on the same device -> profiles/smpl_backward_aux.json
    python scripts/bench_aux.py --only pano_views_host --reference DIR     # the reference's extractImage on this host's CPU, same views (no GPU)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def timed(eng, fn, iters):
    """-> {kernel: (ms per launch, algorithmic bytes per launch, flops per launch)} for the launches ``fn`` makes."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    rows = {}
    for e in eng.profile_read(4096):
        r = rows.setdefault(e['kernel'], [0.0, 0.0, 0.0, 0])
        r[0] += e['ms']; r[1] += e['bytes']; r[2] += e['flops']; r[3] += e['launches']
    eng.profile(False)
    return {k: (v[0] / v[3], v[1] / v[3], v[2] / v[3], v[3] // iters) for k, v in rows.items() if v[3]}


def camcalib_eval_section(eng, a, add, g):
    """The two kernels of CamCalib's test step (spec_amd/camcalib_eval.py).  The ragged resize is also compared, wall clock and
    alternated in this process, with the composition that existed before it: one ``specmi_resize_normalize`` per frame into a
    scratch tensor + one zero-fill of the batch + one slice copy per frame."""
    import time
    from spec_amd import _lib
    from spec_amd.camcalib_eval import resize_size
    from spec_amd.engine import _ptr
    dev = eng.device
    n = 64
    shapes = [(1920, 1080), (1080, 1920), (800, 600), (1000, 1000), (1280, 720), (640, 480), (1600, 1200), (600, 900)]   # (w, h)
    geom, offs, off = [], [], 0
    for i in range(n):
        w, h = shapes[i % len(shapes)]
        oh, ow = resize_size(w, h, 600, 1000)
        geom.append((h, w, oh, ow)); offs.append(off); off += h * w * 3
    slab = torch.randint(0, 256, (off,), generator=g, dtype=torch.uint8).to(dev)
    Hmax, Wmax = max(q[2] for q in geom), max(q[3] for q in geom)
    out = torch.empty(n, 3, Hmax, Wmax, device=dev)
    work = f'{n} uint8 frames of 8 sizes (480p .. 1080p, {off / 1e6:.0f} MB) -> Resize(600, 1000) -> ({n},3,{Hmax},{Wmax}) fp32 zero padded'
    ragged = lambda: eng.resize_normalize_ragged(slab, offs, geom, out=out)
    add('camcalib_eval.pad_batch (specmi_resize_normalize_ragged)', work, timed(eng, ragged, a.iters), ('frames_per_s', n))
    # the same batch stored as NHWC8 fp16 (16 B per pixel in one vector store) - what an fp16 trunk reads without a conversion
    out16 = torch.empty(n, Hmax, Wmax, 8, device=dev, dtype=torch.float16)
    ragged16 = lambda: eng.resize_normalize_ragged(slab, offs, geom, out=out16, dtype=torch.float16)
    add('camcalib_eval.pad_batch (specmi_resize_normalize_ragged_f16)', work.replace(f'({n},3,{Hmax},{Wmax}) fp32', f'({n},{Hmax},{Wmax},8) NHWC8 fp16'),
        timed(eng, ragged16, a.iters), ('frames_per_s', n))
    del out16
    frames = [slab[o:o + h * w * 3] for o, (h, w, _, _) in zip(offs, geom)]
    scratch = [torch.empty(3, oh, ow, device=dev) for _, _, oh, ow in geom]
    out2 = torch.empty_like(out)

    def composed():
        out2.zero_()
        for f, (h, w, oh, ow) in enumerate(geom):
            _lib.check(eng.h, eng.lib.specmi_resize_normalize(eng.h, _ptr(frames[f]), h, w, oh, ow, _ptr(scratch[f]), None, eng._stream()))
            out2[f, :, :oh, :ow].copy_(scratch[f])
    ragged(); composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(out, out2))
    wall = {'ragged': [], 'composed': []}
    for _ in range(max(5, a.iters // 2)):                       # alternated: both see the same clocks and the same neighbours
        for name, fn in (('ragged', ragged), ('composed', composed)):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out_bytes = out.numel() * 4 + off
    cmp_ = {'workload': work, 'bit_identical': same, 'wall_ms_median': {k: round(v, 3) for k, v in med.items()},
            'ratio_composed_over_ragged': round(med['composed'] / med['ragged'], 2),
            'ragged_wall_GBps': round(out_bytes / (med['ragged'] * 1e-3) / 1e9, 1),
            'ragged_frac_of_hbm_peak_wall': round(out_bytes / (med['ragged'] * 1e-3) / HBM_PEAK, 4),
            'note': 'wall clock of one call, host work included: the ragged call builds 64 Pillow coefficient tables on the host '
                    '(identical tables are not uploaded again); the composition rebuilds one table and synchronises the device per frame'}
    print(f"pad_batch: ragged {med['ragged']:.3f} ms  per-frame composition {med['composed']:.3f} ms  ratio {cmp_['ratio_composed_over_ragged']}  "
          f"bit-identical {same}")
    B = a.batch
    lg = [torch.randn(B, 256, generator=g).to(dev) * 3 for _ in range(3)]
    tgt = [torch.randint(0, 256, (B,), generator=g) for _ in range(3)]
    gt = [torch.rand(B, generator=g) for _ in range(3)]
    add('Engine.camcalib_eval (loss + decode + error + batch means)', f'3 x {B} rows x 256 bins, ce',
        timed(eng, lambda: eng.camcalib_eval(*lg, tgt, gt, 'ce'), a.iters), ('rows_per_s', 3 * B))
    return cmp_


PANO_HW, PANO_SEED, PANO_VIEWS = (4096, 8192), 12, 12


def pano_workload():
    """The extractor's workload: a seeded 8192 x 4096 uint8 panorama (smooth content + noise) and 12 cameras of ``sample_cameras``."""
    from spec_amd import panorama
    rng = np.random.default_rng(PANO_SEED)
    H, W = PANO_HW
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    pano = np.stack([127 + 100 * np.sin(xx / (300.0 + 40 * c)) * np.cos(yy / (250.0 + 30 * c)) for c in range(3)], -1)
    pano = np.clip(pano + rng.normal(0, 8, pano.shape).astype(np.float32), 0, 255).astype(np.uint8)
    cams = panorama.sample_cameras(PANO_VIEWS, rng)
    views, heights = panorama.camera_views(cams)
    return pano, views, heights, [panorama.view_size(h, r) for h, r in zip(heights, views[:, 4])]


def scipy_wrap(c, n):
    """The fold the kernel applies (scipy's historical mode="wrap"): only a coordinate OUTSIDE [0, n - 1] moves, by multiples of n - 1."""
    c = np.where(c < 0, c + (n - 1) * (np.trunc(-c / (n - 1)) + 1), c)
    return np.where(c > n - 1, c - (n - 1) * np.trunc(c / (n - 1)), c)


def texels_touched(views, sizes, PH, PW):
    """Distinct panorama texels the four taps of every output pixel read, per view summed (a host float64 evaluation of the
    kernel's coordinates; a tap that lands one texel off at a rounding tie does not change the count materially)."""
    total = 0
    for (el, az, roll, vfov, ratio), (h, w) in zip(views, sizes):
        fy = np.tan(np.radians(vfov) / 2.0); fxx = fy / (1.0 / ratio)
        x, y = np.meshgrid(np.linspace(-fxx, fxx, w), np.linspace(-fy, fy, h), indexing='xy')
        x, y = x * np.cos(roll) + y * np.sin(roll), -x * np.sin(roll) + y * np.cos(roll)
        rho = np.sqrt(x * x + y * y); c = np.arctan(rho)
        lat = np.arcsin(np.clip(np.cos(c) * np.sin(el) + y * np.sin(c) * np.cos(el) / (rho + 1e-10), -1, 1))
        lon = az + np.arctan2(x * np.sin(c), rho * np.cos(el) * np.cos(c) - y * np.sin(el) * np.sin(c))
        lon = np.where(lon > np.pi, lon - 2 * np.pi, lon); lon = np.where(lon < -np.pi, lon + 2 * np.pi, lon)
        col = scipy_wrap(lon / np.pi * PW / 2 + PW / 2, PW); row = scipy_wrap(lat / (np.pi / 2) * PH / 2 + PH / 2, PH)
        r0, c0 = np.floor(row).astype(np.int64), np.floor(col).astype(np.int64)
        r1, c1 = np.minimum(r0 + 1, PH - 1), np.minimum(c0 + 1, PW - 1)
        total += np.unique(np.concatenate([(r * PW + cc).ravel() for r in (r0, r1) for cc in (c0, c1)])).size
    return int(total)


def pano_views_section(eng, a):
    """The extractor on an 8192 x 4096 panorama, 12 views: HIP-event time against the HBM roof with bytes = output bytes + distinct
    texels touched x 3, and - wall clock, same run, same batch - beside the two steps it feeds: the ragged resize and CamCalib's forward."""
    import tempfile
    import time
    from spec_amd import camcalib_eval as ce
    pano_np, views, heights, sizes = pano_workload()
    pano = torch.from_numpy(pano_np).to(eng.device)
    out_bytes = sum(h * w * 3 for h, w in sizes)
    touched = texels_touched(views, sizes, *PANO_HW) * 3
    slab, offsets = eng.pano_extract_views(pano, views, sizes)
    extract = lambda: eng.pano_extract_views(pano, views, sizes, offsets=offsets, out=slab)
    ms = timed(eng, extract, a.iters)['pano_extract'][0]
    geom = [(h, w) + ce.resize_size(w, h, 600, 1000) for h, w in sizes]
    batch = eng.resize_normalize_ragged(slab, offsets, geom)
    with tempfile.TemporaryDirectory() as tmp:
        ce.write_standin_tree(tmp, n_images=1)
        model = ce.build_model(ce.load_config(os.path.join(tmp, ce.STANDIN_CFG)), None, tmp, eng.device)
    meng = model.engine(eng.device)
    steps = {'pano_extract_views': extract, 'resize_normalize_ragged': lambda: meng.resize_normalize_ragged(slab, offsets, geom, out=batch),
             'camcalib_forward_resnet34': lambda: ce.forward_padded(model, batch)}
    wall = {k: [] for k in steps}
    for k, fn in steps.items():
        fn()
    for _ in range(max(5, a.iters // 2)):
        for k, fn in steps.items():
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: round(float(np.median(v)), 3) for k, v in wall.items()}
    row = {'workload': f'{len(sizes)} views of sample_cameras (seed {PANO_SEED}; sizes {sorted(set(sizes))}) out of one {PANO_HW[1]} x {PANO_HW[0]} uint8 panorama',
           'kernel': 'pano_extract', 'ms_per_launch': round(ms, 5), 'output_MB': round(out_bytes / 1e6, 3), 'texels_touched_MB': round(touched / 1e6, 3),
           'achieved_GBps': round((out_bytes + touched) / (ms * 1e-3) / 1e9, 1), 'frac_of_hbm_peak': round((out_bytes + touched) / (ms * 1e-3) / HBM_PEAK, 4),
           'Mpixels_per_s': round(out_bytes / 3 / (ms * 1e-3) / 1e6, 1),
           'wall_ms_median_same_batch': med, 'padded_batch': list(batch.shape),
           'extract_share_of_step': round(med['pano_extract_views'] / sum(med.values()), 4),
           'note': 'wall clock includes host work per call (view table, Pillow coefficient tables); the extractor call synchronises the '
                   'device when its view table changes, which a fresh panorama always does'}
    print(json.dumps(row, indent=1))
    return row


def pano_views_host(a):
    """The reference's own extractImage on THIS host's CPU for the same panorama and views (context for pano_views; no GPU)."""
    import time
    import warnings
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden'))
    from make_panorama_fixture import import_extract_image
    ie = import_extract_image(a.reference)
    pano, views, heights, sizes = pano_workload()
    per = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for (el, az, roll, vfov, ratio), h in zip(views, heights):
            t0 = time.perf_counter()
            im = ie.extractImage(pano, [el, az, roll], h, vfov=vfov, ratio=ratio)
            per.append((time.perf_counter() - t0) * 1e3)
            assert im.shape[:2] == sizes[len(per) - 1]
    row = {'workload': f'{len(sizes)} views, the workload of --only pano_views', 'reference_extractImage_ms_per_view': [round(t, 1) for t in per],
           'reference_extractImage_ms_total': round(sum(per), 1), 'host': f'{os.cpu_count()} logical CPUs, numpy {np.__version__}; one process, as the reference runs it'}
    print(json.dumps(row, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(row, f, indent=1)


def ragged_crops_section(eng, a):
    """Crops from host frames of DIFFERENT sizes, (a) the per-frame route - one upload and one crop launch per frame, plus the
    concatenation for the dataset crop - against (b) the ragged route - one slab, one upload, one launch -, wall clock from host
    frames to crops on the device, alternated in this process in 3 rounds; and the ragged launch alone, HIP-event time against
    the HBM roof.  Decoding the images is outside both routes."""
    import time
    from spec_amd import preprocess as pp
    dev = eng.device
    rng = np.random.default_rng(0)
    shapes = [(1920, 1080), (1080, 1920), (800, 600), (1000, 1000), (1280, 720), (640, 480), (1600, 1200), (600, 900)]   # (w, h)

    def frames_of(n):
        return [rng.integers(0, 256, (shapes[i % len(shapes)][1], shapes[i % len(shapes)][0], 3), dtype=np.uint8) for i in range(n)]

    def compare(route_a, route_b, reps):
        ra, rb = route_a(), route_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(ra, rb))
        del ra, rb
        rounds = {'per_frame': [], 'ragged': []}
        for _ in range(3):                                              # alternated: both see the same clocks and the same neighbours
            wall = {'per_frame': [], 'ragged': []}
            for _ in range(reps):
                for name, fn in (('per_frame', route_a), ('ragged', route_b)):
                    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            for k, v in wall.items():
                rounds[k].append(float(np.median(v)))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        spread = max(rounds['per_frame']) - min(rounds['per_frame'])
        return {'bit_identical': same, 'wall_ms_round_medians': {k: [round(x, 3) for x in v] for k, v in rounds.items()},
                'wall_ms_median': {k: round(v, 3) for k, v in med.items()}, 'per_frame_spread_between_rounds_ms': round(spread, 3),
                'ratio_per_frame_over_ragged': round(med['per_frame'] / med['ragged'], 2),
                'ragged_not_slower_beyond_the_spread': bool(med['ragged'] <= med['per_frame'] + spread)}

    def kernel_row(fn, name):
        ms, by, _, _ = timed(eng, fn, a.iters)[name]
        return {'kernel': name, 'ms_per_launch': round(ms, 5), 'algorithmic_MB': round(by / 1e6, 3), 'achieved_GBps': round(by / (ms * 1e-3) / 1e9, 1),
                'frac_of_hbm_peak': round(by / (ms * 1e-3) / HBM_PEAK, 4)}
    reps = max(3, a.iters // 4)
    out = {}
    # ---- a 64-sample evaluation batch (EvalDataset.batch) -----------------------------------------------------------
    n = 64
    frames = frames_of(n)
    centers = np.stack([[rng.uniform(0.3, 0.7) * f.shape[1], rng.uniform(0.3, 0.7) * f.shape[0]] for f in frames])
    scales = np.asarray([rng.uniform(0.5, 0.9) * f.shape[0] / 200 for f in frames])
    index = np.arange(n, dtype=np.int32)

    def eval_a():
        return torch.cat([pp.dataset_crops(torch.from_numpy(f).to(dev), centers[i:i + 1], scales[i:i + 1], 224) for i, f in enumerate(frames)])

    def eval_b():
        slab, offsets, sizes = pp.pack_frames(frames, dev)
        return pp.dataset_crops_ragged(slab, offsets, sizes, index, centers, scales, 224)
    row = compare(eval_a, eval_b, reps)
    slab, offsets, sizes = pp.pack_frames(frames, dev)
    batch = torch.empty(n, 3, 224, 224, device=dev)
    row.update(workload=f'{n} host frames of 8 sizes (480p .. 1080p, {slab.numel() / 1e6:.0f} MB), one dataset crop each -> ({n},3,224,224) fp32',
               h2d_MB=round(slab.numel() / 1e6, 1), launches={'per_frame': n, 'ragged': 1}, uploads={'per_frame': n, 'ragged': 1},
               ragged_launch=kernel_row(lambda: pp.dataset_crops_ragged(slab, offsets, sizes, index, centers, scales, 224, out=batch),
                                        'crop_resize_normalize_ragged'))
    out['eval_batch'] = row
    print(json.dumps(row, indent=1))
    del slab, batch
    # ---- a 32-frame folder flush, 8 detections per frame (SPECTester.run_on_image_folder) ---------------------------
    F, per = 32, 8
    frames = frames_of(F)
    dets = [np.stack([rng.uniform(0, f.shape[1], per), rng.uniform(0, f.shape[0], per), rng.uniform(100, 500, per), rng.uniform(150, 650, per)],
                     1).astype(np.float32) for f in frames]
    all_dets, fidx = np.concatenate(dets), np.repeat(np.arange(F, dtype=np.int32), per)
    buf = {'inp_images': torch.empty(F * per, 3, 224, 224, device=dev), 'bbox_scale': torch.empty(F * per, device=dev),
           'bbox_center': torch.empty(F * per, 2, device=dev)}

    def flush_a():
        for i, f in enumerate(frames):
            frame = torch.from_numpy(f).pin_memory().to(dev, non_blocking=True)
            pp.crop_detections(frame, dets[i], out={k: v[i * per:(i + 1) * per] for k, v in buf.items()})
        return buf['inp_images'].clone()

    def flush_b():
        slab, offsets, sizes = pp.pack_frames(frames, dev)
        pp.crop_detections_ragged(slab, offsets, sizes, fidx, all_dets, out=buf)
        return buf['inp_images'].clone()
    row = compare(flush_a, flush_b, reps)
    slab, offsets, sizes = pp.pack_frames(frames, dev)
    row.update(workload=f'{F} host frames of 8 sizes (480p .. 1080p, {slab.numel() / 1e6:.0f} MB), {per} detections each -> ({F * per},3,224,224) fp32',
               h2d_MB=round(slab.numel() / 1e6, 1), launches={'per_frame': F, 'ragged': 1}, uploads={'per_frame': F, 'ragged': 1},
               ragged_launch=kernel_row(lambda: pp.crop_detections_ragged(slab, offsets, sizes, fidx, all_dets, out=buf), 'crop_normalize_ragged'),
               note='both routes end with one clone of the crop buffer (the comparison needs a result of its own); the per-frame route '
                    'pins each frame as the folder demo does; the demo\'s per-frame img_h / img_w / R / K assignments are outside both')
    out['folder_flush'] = row
    print(json.dumps(row, indent=1))
    return out


def finish(a, table, extra=None):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(dict({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'batch': a.batch, 'timing': 'per-launch HIP events on the launch stream '
                        '(library profiler)', 'rows': table}, **(extra or {})), f, indent=1)
    w = max(len(r['call']) for r in table)
    for r in table:
        print(f"{r['call']:<{w}}  {r['kernel']:<22} {r['ms_per_launch'] * 1e3:9.1f} us  {r['algorithmic_MB']:9.2f} MB  "
              f"{r['achieved_GBps']:8.1f} GB/s  frac {r['frac_of_hbm_peak']:.3f}   {r['workload']}")


def render_workload(M=8, H=1080, W=1920):
    """8 person-sized closed meshes of SMPL's face count order (icospheres of 5120 faces stretched to 0.5 x 1.7 x 0.3 m) spread
    over a 1080p frame at 3 .. 6 m from a camera of f = 1200 px."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests.render_ref import icosphere
    v, f = icosphere(4)
    v = v * np.array([0.25, 0.85, 0.15], np.float32)
    t = np.array([[-2.4 + 0.7 * m, 0.1 * (m % 3 - 1), 3.0 + 0.43 * m] for m in range(M)], np.float32)
    return np.ascontiguousarray(np.broadcast_to(v, (M,) + v.shape)), f, t, (1200., 1200.), (W / 2, H / 2), (H, W)


def render_section(eng, a):
    """The mesh overlay and the side view (specmi_render_meshes) of 8 meshes on a 1080p frame: per-launch HIP events of the three
    kernels in both launch shapes of the raster kernel, next to the bytes they must touch."""
    from spec_amd import _lib
    v, f, t, focal, center, (H, W) = render_workload()
    dev = eng.device
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8).to(dev)
    args = [torch.from_numpy(x).to(dev) for x in (v, f, t, np.eye(3, dtype=np.float32))]
    rows = {}
    for name, flags in (('overlay', _lib.RENDER_CULL), ('side_view', _lib.RENDER_CULL | _lib.RENDER_SIDE_VIEW | _lib.RENDER_GROUND_PLANE)):
        for shape, bit in (('wave_per_triangle', 0), ('thread_per_triangle', _lib.RENDER_THREAD_PER_TRIANGLE)):
            call = lambda: eng.render_meshes(args[0], args[1], args[2], args[3], focal, center, frame=frame, flags=flags | bit)
            res = timed(eng, call, a.iters)
            covered = int((eng.render_meshes(args[0], args[1], args[2], args[3], focal, center, frame=frame, flags=flags | bit, maps=True)['id_map'] >= 0).sum())
            rows[f'{name}.{shape}'] = {'kernels_ms': {k: round(ms, 5) for k, (ms, _, _, _) in res.items()}, 'total_ms': round(sum(ms for ms, _, _, _ in res.values()), 5),
                                       'algorithmic_MB': {k: round(by / 1e6, 3) for k, (_, by, _, _) in res.items()}, 'mesh_pixels': covered}
    return {'workload': f'{v.shape[0]} meshes of {v.shape[1]} vertices / {f.shape[0]} faces on a {W} x {H} frame, f = {focal[0]:.0f} px', 'calls': rows,
            'must_touch_MB': {'keys_memset_and_resolve': round(H * W * 16 / 1e6, 3), 'frame_in_out': round(H * W * 6 / 1e6, 3),
                              'vertices_faces': round((v.size * 4 * 3 + v.shape[0] * f.size * 4) / 1e6, 3)}}


def render_batch_section(eng, a):
    """The pictures of a 32-frame flush, (a) the per-frame loop - per frame two ``render_meshes`` calls and a concatenation; from
    host frames ``render_image_group`` with its upload and download - against (b) the batched route - one ``render_views`` call per
    chunk of ``plan_views``; from host frames ``render_image_groups`` -, alternated in this process in 3 rounds.  Device-resident
    inputs: HIP events around the whole sequence.  Host frames to host pictures: wall clock, the copies included."""
    import time
    from spec_amd import _lib, render
    from spec_amd.preprocess import pack_frames
    v8, f, t8, _, _, _ = render_workload()
    dev = eng.device
    faces = torch.from_numpy(f).to(dev)
    rng = np.random.default_rng(0)
    rgb = render._rgb('pinkish')
    side = _lib.RENDER_CULL | _lib.RENDER_SIDE_VIEW | _lib.RENDER_GROUND_PLANE
    mixed = [(480, 640), (1080, 1920), (720, 1280), (600, 800), (1080, 1440), (768, 1024), (900, 1600), (1920, 1080)]      # (H, W)
    shapes = {'A_32x1080p_8_meshes': ([(1080, 1920)] * 32, [8] * 32),
              'B_32_mixed_sizes_1_to_8_meshes': ([mixed[i % len(mixed)] for i in range(32)], [int(c) for c in rng.integers(1, 9, 32)])}
    reps = max(3, a.iters // 4)
    out = {}
    for name, (sizes, counts) in shapes.items():
        F = len(sizes)
        first = np.concatenate([[0], np.cumsum(counts)]).tolist()
        host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]
        verts = torch.from_numpy(np.concatenate([v8[:c] for c in counts])).to(dev)
        cam_t = torch.from_numpy(np.concatenate([t8[:c] for c in counts])).to(dev)
        Rs, R_dev = [np.eye(3, dtype=np.float32)] * F, torch.eye(3, device=dev)
        focals, centers = [(1200. * H / 1080, 1200. * H / 1080) for H, _ in sizes], [(W / 2, H / 2) for H, W in sizes]
        frames = [torch.from_numpy(fr).to(dev) for fr in host]
        chunks = render.plan_views(sizes, counts)
        for ch in chunks:
            ch['in_slab'] = pack_frames([host[k] for k in ch['frames']], dev)[0]
            ch['out_slab'] = torch.empty(ch['out_bytes'], device=dev, dtype=torch.uint8)
            ch['cams'] = render.view_cams(ch['view_frame'], Rs, focals, centers)

        def loop_dev(keep=False):
            pics = []
            for k in range(F):
                m = slice(first[k], first[k + 1])
                o = eng.render_meshes(verts[m], faces, cam_t[m], R_dev, focals[k], centers[k], frame=frames[k], rgb=rgb, flags=_lib.RENDER_CULL)
                s = eng.render_meshes(verts[m], faces, cam_t[m], R_dev, focals[k], centers[k], frame=frames[k], rgb=rgb, flags=side)
                pic = torch.cat([frames[k], o, s], dim=1)
                if keep:
                    pics.append(pic.cpu())
            return pics

        def batched_dev(keep=False):
            pics = []
            for ch in chunks:
                eng.render_views(verts, faces, cam_t, ch['geom'], ch['offsets'], ch['cams'], ch['in_slab'], ch['out_slab'], rgb=rgb)
                if keep:
                    slab = ch['out_slab'].cpu()
                    pics += [slab[o:o + 9 * sizes[k][0] * sizes[k][1]].reshape(sizes[k][0], 3 * sizes[k][1], 3) for (k, _), o in zip(ch['pictures'], ch['picture_offsets'])]
            return pics

        def loop_host():
            return [render.render_image_group(host[k], cam_t[first[k]:first[k + 1]], verts[first[k]:first[k + 1]], Rs[k], focals[k], centers[k],
                                              faces=faces, engine=eng).cpu().numpy() for k in range(F)]

        def batched_host():
            return render.render_image_groups(host, verts, cam_t, counts, Rs, focals, centers, faces=faces, engine=eng)

        pa, pb = loop_dev(True), batched_dev(True)
        same = len(pa) == len(pb) == F and all(torch.equal(x, y) for x, y in zip(pa, pb))
        same = same and all(np.array_equal(x, y) for x, y in zip(loop_host(), batched_host()))
        del pa, pb

        def by_events(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def by_wall(fn):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def compare(route_a, route_b, clock):
            rounds = {'per_frame': [], 'batched': []}
            for _ in range(3):                                          # alternated: both see the same clocks and the same neighbours
                ms = {'per_frame': [], 'batched': []}
                for _ in range(reps):
                    for key, fn in (('per_frame', route_a), ('batched', route_b)):
                        ms[key].append(clock(fn))
                for key, v in ms.items():
                    rounds[key].append(float(np.median(v)))
            med = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = max(rounds['per_frame']) - min(rounds['per_frame'])
            return {'ms_round_medians': {k: [round(x, 3) for x in v] for k, v in rounds.items()}, 'ms_median': {k: round(v, 3) for k, v in med.items()},
                    'per_frame_spread_between_rounds_ms': round(spread, 3), 'ratio_per_frame_over_batched': round(med['per_frame'] / med['batched'], 2),
                    'batched_not_slower_beyond_the_spread': bool(med['batched'] <= med['per_frame'] + spread)}
        px = sum(H * W for H, W in sizes)
        row = {'workload': f'{F} frames, {px / 1e6:.1f} Mpx in all, {sum(counts)} meshes of {v8.shape[1]} vertices / {f.shape[0]} faces; '
                           f'{len(chunks)} chunks at the default pixel budget', 'bit_identical': bool(same),
               'calls': {'per_frame': {'render_meshes': 2 * F, 'cat': F, 'uploads': F, 'downloads': F},
                         'batched': {'render_views': len(chunks), 'uploads': len(chunks), 'downloads': len(chunks)}},
               'device_resident_hip_events': compare(loop_dev, batched_dev, by_events),
               'host_frames_to_host_pictures_wall': compare(loop_host, batched_host, by_wall)}
        out[name] = row
        print(json.dumps(row, indent=1))
        del frames, chunks, verts, cam_t
        torch.cuda.empty_cache()
    return out


def draw_section(eng, a):
    """``specmi_draw_skeletons`` (49 joints and the 25 bones of ``constants.SKELETON_SPIN`` per detection, D = 2, keypoints spread
    over the frame as a person's are: a cluster of about a third of the frame's height around a random centre) on (1) one
    1080 x 1920 frame with 8 detections and (2) a 64-frame flush of mixed sizes with 1 to 8 detections each, next to
    ``specmi_render_views`` for the pictures of the same flush, in this process.  HIP events around ``reps`` back-to-back calls
    after a warm-up of the same calls, 3 alternated rounds; the drawing repeats its records, so no call rewrites the table."""
    from spec_amd import render
    from spec_amd.preprocess import pack_frames
    v8, f, t8, _, _, _ = render_workload()
    dev = eng.device
    rng = np.random.default_rng(0)
    faces = torch.from_numpy(f).to(dev)
    rgb = render._rgb('pinkish')
    mixed = [(480, 640), (1080, 1920), (720, 1280), (600, 800), (1080, 1440), (768, 1024), (900, 1600), (1920, 1080)]      # (H, W)
    reps = max(5, a.iters)

    def keypoints(sizes, counts):
        out = []
        for (H, W), c in zip(sizes, counts):
            centre = np.stack([rng.uniform(0.1 * W, 0.9 * W, c), rng.uniform(0.2 * H, 0.8 * H, c)], 1)[:, None, :]
            out.append(centre + rng.normal(0.0, 1.0, (c, 49, 2)) * np.array([0.06 * H, 0.17 * H]))
        return torch.from_numpy(np.concatenate(out).astype(np.float32)).to(dev)

    def events(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(n):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def rounds(fns):
        for fn in fns.values():
            for _ in range(3):
                fn()
        ms = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                ms[k].append(events(fn, reps))
        return {k: {'ms_per_call_rounds': [round(x, 4) for x in v], 'ms_per_call_median': round(float(np.median(v)), 4)} for k, v in ms.items()}

    out = {}
    # (1) one 1080p frame
    sizes, counts = [(1080, 1920)], [8]
    kp = keypoints(sizes, counts)
    slab = pack_frames([rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)], dev)[0]
    geom, offsets = [[1080, 1920, 0, 8]], [[0, 3 * 1920]]
    before = slab.clone()
    eng.draw_skeletons(kp, slab, geom, offsets)
    out['one_1080p_frame_8_detections'] = dict(rounds({'draw_skeletons': lambda: eng.draw_skeletons(kp, slab, geom, offsets)}),
                                               workload='one 1080 x 1920 frame, 8 detections x (49 joints + 25 bones)',
                                               pixels_painted=int((slab != before).reshape(-1, 3).any(dim=1).sum()))
    # (2) a 64-frame flush, and render_views for its pictures
    sizes = [mixed[i % len(mixed)] for i in range(64)]
    counts = [int(c) for c in rng.integers(1, 9, 64)]
    kp = keypoints(sizes, counts)
    host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]
    verts = torch.from_numpy(np.concatenate([v8[:c] for c in counts])).to(dev)
    cam_t = torch.from_numpy(np.concatenate([t8[:c] for c in counts])).to(dev)
    Rs = [np.eye(3, dtype=np.float32)] * 64
    focals, centers = [(1200. * H / 1080, 1200. * H / 1080) for H, _ in sizes], [(W / 2, H / 2) for H, W in sizes]
    chunks = render.plan_views(sizes, counts)
    painted = 0
    for ch in chunks:
        ch['in_slab'] = pack_frames([host[k] for k in ch['frames']], dev)[0]
        ch['out_slab'] = torch.empty(ch['out_bytes'], device=dev, dtype=torch.uint8)
        ch['cams'] = render.view_cams(ch['view_frame'], Rs, focals, centers)
        hw = np.asarray([sizes[k] for k in ch['frames']], np.int64)
        ch['draw_geom'], ch['draw_offsets'] = np.concatenate([hw, ch['frame_dets']], axis=1), np.stack([ch['frame_offsets'], 3 * hw[:, 1]], axis=1)
        before = ch['in_slab'].clone()
        eng.draw_skeletons(kp, ch['in_slab'], ch['draw_geom'], ch['draw_offsets'])
        painted += int((ch['in_slab'] != before).reshape(-1, 3).any(dim=1).sum())
    del host

    def draw_flush():
        for ch in chunks:
            eng.draw_skeletons(kp, ch['in_slab'], ch['draw_geom'], ch['draw_offsets'])

    def views_flush():
        for ch in chunks:
            eng.render_views(verts, faces, cam_t, ch['geom'], ch['offsets'], ch['cams'], ch['in_slab'], ch['out_slab'], rgb=rgb)

    # with several chunks both calls rewrite their record tables between chunks (a device synchronise each): timed as the flows pay it
    row = rounds({'draw_skeletons': draw_flush, 'render_views': views_flush})
    d, r = row['draw_skeletons']['ms_per_call_median'], row['render_views']['ms_per_call_median']
    out['flush_64_mixed_frames'] = dict(row, workload=f'64 frames of 8 sizes, {sum(H * W for H, W in sizes) / 1e6:.1f} Mpx in all, {sum(counts)} detections x '
                                        f'(49 joints + 25 bones); render_views: the same detections as meshes of {v8.shape[1]} vertices / {f.shape[0]} faces; '
                                        f'{len(chunks)} chunks at the default pixel budget, one call of each per chunk',
                                        pixels_painted=painted, draw_over_render_views=round(d / r, 4))
    print(json.dumps(out, indent=1))
    return out


def picture_frame(rng, H, W):
    """A seeded frame: smooth fields with noise."""
    yy, xx = np.mgrid[0:H, 0:W]
    ph = rng.uniform(0, 6.28, (3, 4))
    img = np.stack([127 + 60 * np.sin(xx / 97.0 + p[0]) * np.cos(yy / 71.0 + p[1]) + 40 * np.sin((xx + yy) / 23.0 + p[2]) + 20 * np.cos(yy / 9.0 + p[3])
                    for p in ph], -1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def demo_pictures(eng, rng, v8, f, t8):
    """Eight 1080 x 5760 three-panel pictures as ``render_image_groups`` draws them from seeded 1080p frames, two meshes each, where
    ``render_views`` left them -> (device slab, geom, offsets (n, 2))."""
    from spec_amd import render
    dev = eng.device
    F, (H, W) = 8, (1080, 1920)
    frames = [picture_frame(rng, H, W) for _ in range(F)]
    verts = torch.from_numpy(np.concatenate([v8[:2]] * F)).to(dev)
    cam_t = torch.from_numpy(np.concatenate([t8[2:4]] * F)).to(dev)
    _, slabs = render.render_image_groups(frames, verts, cam_t, [2] * F, [np.eye(3, dtype=np.float32)] * F, [(1200., 1200.)] * F, [(W / 2, H / 2)] * F,
                                          faces=torch.from_numpy(f).to(dev), engine=eng, return_slabs=True)
    assert len(slabs) == 1
    slab, offs, shapes = slabs[0]
    return slab, [tuple(sh) for sh in shapes], [(int(o), 3 * sh[1]) for o, sh in zip(offs, shapes)]


def jpeg_section(eng, a):
    """Pictures on the device to JPEG files on the host, two routes alternated in this process (wall clock with the copies, 3
    rounds): DEVICE = ``Engine.jpeg_encode`` (``specmi_jpeg_encode``, then the sizes and the files' bytes come down), HOST = the raw
    pictures come down and Pillow encodes each.  Workloads: (1) eight 1080 x 5760 three-panel pictures as ``render_image_groups``
    draws them from seeded 1080p frames (smooth fields with noise, two meshes each), quality 75 - the demo's files; (2) twelve
    600 x 800 views of the same kind of content, quality 95 - ``write_tree``'s files.  Per kernel (library profiler, HIP events):
    its time next to the bytes the stage must move, computed here from the shapes and the files' lengths."""
    import io
    import time
    from PIL import Image
    from spec_amd import _lib, render
    dev = eng.device
    v8, f, t8, _, _, _ = render_workload()
    rng = np.random.default_rng(0)

    frame = lambda H, W: picture_frame(rng, H, W)

    def workload(name):
        if name == 'demo_pictures':
            return demo_pictures(eng, rng, v8, f, t8) + (75,)
        pics = [frame(600, 800) for _ in range(12)]
        return torch.from_numpy(np.concatenate([p_.reshape(-1) for p_ in pics])).to(dev), [(600, 800)] * 12, [(k * 600 * 800 * 3, 2400) for k in range(12)], 95

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    out = {}
    for name in ('demo_pictures', 'tree_views'):
        slab, geom, offsets, q = workload(name)
        n, px = len(geom), sum(h * w for h, w in geom)

        def device_route():
            return eng.jpeg_encode(slab, geom, offsets, q)

        def host_route():
            raw = slab.cpu().numpy()
            files = []
            for (h, w), (o, pitch) in zip(geom, offsets):
                b = io.BytesIO()
                Image.fromarray(raw[o:o + h * pitch].reshape(h, w, 3)).save(b, format='JPEG', quality=q, optimize=False, progressive=False)
                files.append(b.getvalue())
            return files

        fd, fh = device_route(), host_route()
        same = fd == fh
        rounds = {'device': [], 'host': []}
        reps = max(2, min(a.iters, 5))
        for _ in range(3):                                              # alternated: both see the same clocks and the same neighbours
            ms = {'device': [], 'host': []}
            for _ in range(reps):
                ms['device'].append(wall(device_route)[0])
                ms['host'].append(wall(host_route)[0])
            for k, v in ms.items():
                rounds[k].append(float(np.median(v)) / n)
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        spread = max(rounds['host']) - min(rounds['host'])
        file_bytes = sum(len(x) for x in fd)
        mcus = sum(-(-h // 16) * -(-w // 16) for h, w in geom)
        scan = file_bytes - n * 625                                      # stuffed scan bytes: an upper bound of the unstuffed ones
        must = {'jpeg_zero': mcus * 1248, 'jpeg_dct': 3 * px + mcus * 768, 'jpeg_count': mcus * 768 + mcus * 4, 'jpeg_scan_bits': (mcus // 256 + n) * 12,
                'jpeg_write': mcus * 768 + mcus * 4 + scan, 'jpeg_ffcount': scan, 'jpeg_scan_ff': (mcus * 1248 // 4096 + n) * 12, 'jpeg_pack': 2 * scan + n * 625}
        kern = {}
        cap = [3 * h * w + 1024 for h, w in geom]
        oo = np.concatenate([[0], np.cumsum(cap)])
        ws_out = torch.empty(int(oo[-1]), device=dev, dtype=torch.uint8)
        full = [(o, p_, int(x), c) for (o, p_), x, c in zip(offsets, oo[:-1], cap)]
        total_ms = 0.0
        for k, (ms_, _, _, nl) in timed(eng, lambda: eng.jpeg_encode_into(slab, ws_out, geom, full, q), a.iters).items():
            kern[k] = {'ms_per_launch': round(ms_, 4), 'must_move_MB': round(must.get(k, 0) / 1e6, 3),
                       'frac_of_hbm_peak': round(must.get(k, 0) / (ms_ * 1e-3) / HBM_PEAK, 4), 'launches_per_call': nl}
            total_ms += ms_ * nl
        row = {'workload': f'{n} pictures of {geom[0][0]} x {geom[0][1]}, quality {q}, {px / 1e6:.1f} Mpx in all', 'byte_identical': bool(same),
               'ms_per_picture_rounds': {k: [round(x, 3) for x in v] for k, v in rounds.items()}, 'ms_per_picture_median': {k: round(v, 3) for k, v in med.items()},
               'host_spread_between_rounds_ms': round(spread, 3), 'ratio_host_over_device': round(med['host'] / med['device'], 2),
               'device_not_slower_beyond_the_spread': bool(med['device'] <= med['host'] + spread),
               'bytes_moved_device_to_host': {'device_route': file_bytes + 8 * n, 'host_route': int(slab.numel())},
               'kernels': kern, 'kernels_ms_per_call': round(total_ms, 4), 'kernels_ms_per_picture': round(total_ms / n, 4),
               'kernels_frac_of_hbm_peak': round(sum(must.values()) / (total_ms * 1e-3) / HBM_PEAK, 4)}
        out[name] = row
        print(json.dumps(row, indent=1))
        del slab, ws_out
        torch.cuda.empty_cache()
    return out


def png_section(eng, a):
    """Pictures on the device to PNG files on the host, two routes alternated in this process (wall clock with the copies, 3
    rounds): DEVICE = ``Engine.png_encode`` (``specmi_png_encode``, then the sizes and the files' bytes come down), HOST = the raw
    pictures come down and Pillow saves each as the flows do (``Image.fromarray(a).save(f, format='PNG')``: zlib on one thread at
    Pillow's default level).  Workload: the eight 1080 x 5760 three-panel pictures of ``--only jpeg_encode``.  The files' sizes
    next to Pillow's at compress_level 1 and 6; per kernel (library profiler, HIP events) its time."""
    import io
    import time
    from PIL import Image
    from spec_amd.engine import png_bound
    dev = eng.device
    v8, f, t8, _, _, _ = render_workload()
    slab, geom, offsets = demo_pictures(eng, np.random.default_rng(0), v8, f, t8)
    n, px = len(geom), sum(h * w for h, w in geom)

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def device_route():
        return eng.png_encode(slab, geom, offsets)

    def host_route(**kw):
        raw = slab.cpu().numpy()
        files = []
        for (h, w), (o, pitch) in zip(geom, offsets):
            b = io.BytesIO()
            Image.fromarray(raw[o:o + h * pitch].reshape(h, w, 3)).save(b, format='PNG', **kw)
            files.append(b.getvalue())
        return files

    fd, fh = device_route(), host_route()
    raw = slab.cpu().numpy()
    lossless = all(np.array_equal(np.array(Image.open(io.BytesIO(x)).convert('RGB')), raw[o:o + h * pitch].reshape(h, w, 3))
                   for x, (h, w), (o, pitch) in zip(fd, geom, offsets))
    level1 = host_route(compress_level=1)
    rounds = {'device': [], 'host': []}
    reps = max(2, min(a.iters, 5))
    for _ in range(3):                                              # alternated: both see the same clocks and the same neighbours
        ms = {'device': [], 'host': []}
        for _ in range(reps):
            ms['device'].append(wall(device_route)[0])
            ms['host'].append(wall(host_route)[0])
        for k, v in ms.items():
            rounds[k].append(float(np.median(v)) / n)
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    spread = max(rounds['host']) - min(rounds['host'])
    cap = [png_bound(h, w) for h, w in geom]
    oo = np.concatenate([[0], np.cumsum(cap)])
    ws_out = torch.empty(int(oo[-1]), device=dev, dtype=torch.uint8)
    full = [(o, p_, int(x), c) for (o, p_), x, c in zip(offsets, oo[:-1], cap)]
    kern, total_ms = {}, 0.0
    for k, (ms_, _, _, nl) in timed(eng, lambda: eng.png_encode_into(slab, ws_out, geom, full), a.iters).items():
        kern[k] = {'ms_per_launch': round(ms_, 4), 'launches_per_call': nl}
        total_ms += ms_ * nl
    size = lambda files: sum(len(x) for x in files)
    row = {'workload': f'{n} pictures of {geom[0][0]} x {geom[0][1]}, {px / 1e6:.1f} Mpx in all', 'decodes_to_the_pictures': bool(lossless),
           'ms_per_picture_rounds': {k: [round(x, 3) for x in v] for k, v in rounds.items()}, 'ms_per_picture_median': {k: round(v, 3) for k, v in med.items()},
           'host_spread_between_rounds_ms': round(spread, 3), 'ratio_host_over_device': round(med['host'] / med['device'], 2),
           'file_bytes': {'device': size(fd), 'pillow_compress_level_6': size(fh), 'pillow_compress_level_1': size(level1), 'raw': 3 * px},
           'fraction_of_raw': {'device': round(size(fd) / (3 * px), 4), 'pillow_compress_level_6': round(size(fh) / (3 * px), 4),
                               'pillow_compress_level_1': round(size(level1) / (3 * px), 4)},
           'bytes_moved_device_to_host': {'device_route': size(fd) + 8 * n, 'host_route': int(slab.numel())},
           'kernels': kern, 'kernels_ms_per_call': round(total_ms, 4), 'kernels_ms_per_picture': round(total_ms / n, 4)}
    print(json.dumps(row, indent=1))
    return {'demo_pictures': row}


def horizon_panel_section(eng, a):
    """Panel 0 of a flush of eight 1080 x 1920 frames with the demo's marks (green line of width 5, caption strip of 30 rows), from
    host frames to a finished slab on the device, two routes alternated in this process (wall clock with the copies, 3 rounds):
    HOST = ``render.group_panel0`` on each frame (Pillow) + ``pack_frames``; DEVICE = ``pack_frames`` of the raw frames +
    ``render.show_horizon_lines`` (one mask upload, one ``specmi_draw_marks`` call).  The launch itself by the library's profiler."""
    import time
    from spec_amd import render
    from spec_amd.preprocess import pack_frames
    F, H, W = 8, 1080, 1920
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(F)]
    cams = [(float(rng.uniform(0.8, 1.4)), float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.2, 0.2)), float(rng.uniform(800, 1500))) for _ in range(F)]
    sizes, horizons = [(H, W)] * F, [render._panel0_horizon(c) for c in cams]
    offs = np.arange(F, dtype=np.int64) * H * W * 3

    def host_route():
        return pack_frames([render.group_panel0(f, c) for f, c in zip(frames, cams)], eng.device)[0]

    def device_route():
        slab = pack_frames(frames, eng.device)[0]
        render.show_horizon_lines(slab, sizes, offs, horizons, engine=eng)
        return slab

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    same = bool(torch.equal(host_route(), device_route()))
    rounds = {'host': [], 'device': []}
    reps = max(2, min(a.iters, 5))
    for _ in range(3):                                                  # alternated: both see the same clocks and the same neighbours
        ms = {'host': [], 'device': []}
        for _ in range(reps):
            ms['host'].append(wall(host_route)[0])
            ms['device'].append(wall(device_route)[0])
        for k, v in ms.items():
            rounds[k].append(float(np.median(v)))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    spread = max(max(v) - min(v) for v in rounds.values())
    slab = pack_frames(frames, eng.device)[0]
    kern = {k: {'ms_per_launch': round(ms_, 5), 'launches_per_call': nl}
            for k, (ms_, _, _, nl) in timed(eng, lambda: render.show_horizon_lines(slab, sizes, offs, horizons, engine=eng), a.iters).items()}
    row = {'workload': f'{F} frames of {H} x {W}, one horizon each: line of width 5, caption strip of 30 rows', 'byte_identical': same,
           'ms_per_flush_rounds': {k: [round(x, 3) for x in v] for k, v in rounds.items()}, 'ms_per_flush_median': {k: round(v, 3) for k, v in med.items()},
           'spread_between_rounds_ms': round(spread, 3), 'ratio_host_over_device': round(med['host'] / med['device'], 2),
           'device_faster_beyond_the_spread': bool(med['device'] + spread < med['host']), 'kernels': kern}
    print(json.dumps(row, indent=1))
    return row


def hmr_loss_section(eng, a, add):
    """``specmi_hmr_loss`` in HMRCamLoss mode with the per-vertex L1 term on: 2 * B * 6890 * 3 floats per call, at the batch of the
    evaluation config (64) and at ``--batch``."""
    rng = np.random.default_rng(0)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(eng.device)
    for B in sorted({64, a.batch}):
        pred = {'pred_pose': f(B, 24, 3, 3), 'pred_shape': f(B, 10), 'pred_cam': f(B, 3).abs() + 0.5, 'smpl_joints3d': f(B, 49, 3),
                'smpl_joints2d': f(B, 49, 2) * 100, 'smpl_vertices': f(B, 6890, 3)}
        gt = {'pose': f(B, 72) * 0.3, 'betas': f(B, 10), 'pose_conf': torch.ones(B, 24, device=eng.device), 'pose_3d': f(B, 24, 4),
              'keypoints_orig': f(B, 49, 3).abs() * 100, 'vertices': f(B, 6890, 3), 'has_smpl': torch.ones(B, dtype=torch.int32, device=eng.device),
              'has_pose_3d': torch.ones(B, dtype=torch.int32, device=eng.device), 'orig_shape': torch.full((B, 2), 480., device=eng.device),
              'scale': torch.ones(B, device=eng.device)}
        out = eng.hmr_loss(1, pred, gt, [1., 5., 1., 1., 0.001, 0., 1., 60.])
        add('Engine.hmr_loss (HMRCamLoss, shape_loss_weight 1)', f'{B} images, 6890 vertices: {2 * B * 6890 * 3 * 4 / 1e6:.1f} MB of vertices',
            timed(eng, lambda: eng.hmr_loss(1, pred, gt, [1., 5., 1., 1., 0.001, 0., 1., 60.], out=out), a.iters), ('images_per_s', B))


def eval_step_section(eng, a):
    """``specmi_eval_step`` (per-joint errors of both joint sets + the unaligned V2V, one launch) against the two launches it sits
    next to, ``specmi_eval_mesh`` + ``specmi_eval_joints`` (per-image means only), at the evaluation config's batch: B = 64,
    V = 6890, J = 17, nsel = 14, Jk = 24.  HIP events around ``iters`` back-to-back calls after a warm-up of the same calls, the
    two alternated in this process, 3 rounds.  The bytes a call must move: both meshes and the regressor once, the joint sets,
    the outputs."""
    from spec_amd import constants, metrics
    dev = eng.device
    rng = np.random.default_rng(0)
    B, V, J, Jk = 64, 6890, 17, 24
    f = lambda *shape, std=0.3: torch.from_numpy((rng.standard_normal(shape) * std).astype(np.float32)).to(dev)
    gv, gj = f(B, V, 3), f(B, Jk, 3)
    pv, pj = gv + f(B, V, 3, std=0.03), gj + f(B, Jk, 3, std=0.03)
    Jr = torch.from_numpy(rng.random((J, V)).astype(np.float32)).to(dev)
    Jr /= Jr.sum(1, keepdim=True)
    sel = list(constants.H36M_TO_J14)

    def pair():
        metrics.eval_single(pv, gv, Jr, joint_sel=sel)
        metrics.eval_j_24(pj, gj)

    def step():
        eng.eval_step(pv, gv, Jr, joint_sel=sel, pred_joints=pj, gt_joints=gj)

    def ms_per_call(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    rounds = {'pair': [], 'eval_step': []}
    for _ in range(3):                                              # alternated: both see the same clocks and the same neighbours
        rounds['pair'].append(ms_per_call(pair))
        rounds['eval_step'].append(ms_per_call(step))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    by = {'eval_step': 4.0 * (B * V * 6 + J * V + B * Jk * 6 + B * (2 * len(sel) + 2 * Jk + 1)),
          'pair': 4.0 * (B * V * 6 + J * V + B * Jk * 6 + B * 5)}
    kern = {k: {'ms_per_launch': round(v[0], 5), 'algorithmic_MB': round(v[1] / 1e6, 3)}
            for fn in (pair, step) for k, v in timed(eng, fn, a.iters).items()}
    row = {'workload': f'B = {B}, V = {V}, J = {J}, nsel = {len(sel)}, Jk = {Jk}; the pair returns 5 per-image means in millimetres, eval_step '
                       f'{2 * len(sel) + 2 * Jk} per-joint errors per image in metres and the unaligned V2V',
           'launches': {'pair': 2, 'eval_step': 1}, 'ms_round_values': {k: [round(x, 5) for x in v] for k, v in rounds.items()},
           'ms_median': {k: round(v, 5) for k, v in med.items()}, 'spread_between_rounds_ms': {k: round(v, 5) for k, v in spread.items()},
           'must_move_MB': {k: round(v / 1e6, 3) for k, v in by.items()},
           'frac_of_hbm_peak': {k: round(by[k] / (med[k] * 1e-3) / HBM_PEAK, 4) for k in med},
           'ratio_pair_over_eval_step': round(med['pair'] / med['eval_step'], 3),
           'eval_step_slower_beyond_the_pairs_spread': bool(med['eval_step'] > med['pair'] + spread['pair']),
           'kernels_by_the_library_profiler': kern}
    print(json.dumps(row, indent=1))
    return row


def natural_frames_1080p(n=64):
    """``n`` synthetic frames of 1080 x 1920 with natural-like content: low-frequency structure plus mild noise"""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:1080, 0:1920]
    noise = [rng.normal(0, 5, (1080, 1920, 3)) for _ in range(4)]
    imgs = []
    for i in range(n):
        base = np.stack([128 + 80 * np.sin(yy / (60.0 + 7 * c + i) + i) * np.cos(xx / (90.0 + 11 * c) + 0.3 * i) + 30 * np.sin((xx + yy) / (17.0 + i % 5))
                         for c in range(3)], axis=2)
        imgs.append(np.clip(base + noise[i % 4], 0, 255).astype(np.uint8))
    return imgs


def binding_statement(full_over_copy, no_hue_over_copy, hue_cost):
    """What bounds the apply launch, from its time against the copy of the same bytes with and without the hue shift (1.25 x = beyond
    what the rounds differ by)"""
    if full_over_copy <= 1.25:
        return 'HBM bandwidth bounds the apply launch: it takes what a copy of the same bytes takes'
    if no_hue_over_copy <= 1.25:
        return f'the hue arithmetic bounds the apply launch: without hue it takes what the copy takes, with it {full_over_copy} x'
    return (f'arithmetic bounds the apply launch, not HBM: with hue taken out of every order it still takes {no_hue_over_copy} x the copy of the same '
            f'bytes (the blends and the byte unpacking), and the hue shift multiplies that by {round(hue_cost, 2)}')


def color_jitter_section(eng, a):
    """``specmi_color_jitter`` on the 64 synthetic 1080p frames of ``--only jpeg_decode`` with the reference's four settings and a
    seeded order per frame (``augment.ColorJitter.records``); the same with contrast removed (one launch) and with the hue shift
    removed (what the hue arithmetic costs).  Per launch: HIP events of the library's profiler after a warm-up, next to a
    device-to-device copy of the same slab timed by events in the same process, alternated over 3 rounds - the copy is the
    yardstick.  Bytes are counted here: 3 N read by the stat launch, 3 N read + 3 N written by the apply launch and by the copy.
    Host comparison, wall clock, 3 alternated rounds: Pillow's chain on 16 threads + ``pack_frames`` (one upload) against
    ``pack_frames`` + the device call; the two slabs are compared."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image, ImageEnhance
    from spec_amd import augment
    from spec_amd.preprocess import pack_frames
    dev = eng.device
    imgs = natural_frames_1080p()
    slab, offsets, sizes = pack_frames(imgs, dev)
    out = torch.empty_like(slab)
    N = sum(H * W for H, W in sizes)
    cj = augment.ColorJitter(**augment.CAMCALIB_TRAIN_JITTER)
    full = cj.records(len(imgs), torch.Generator().manual_seed(0))

    def without(recs, op):
        r = recs.copy()
        for row in r:
            ids = [i for i in row[:4] if i >= 0 and i != op]
            row[:4] = ids + [-1] * (4 - len(ids))
        return r
    workloads = {'full': full, 'no_contrast': without(full, 1), 'no_hue': without(full, 3)}
    counted = {'color_jitter_stat': 3 * N, 'color_jitter_apply': 6 * N, 'copy': 6 * N}

    def copy_ms(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            out.copy_(slab)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    rows = {}
    for name, recs in workloads.items():
        ms = {}
        for _ in range(3):                                              # alternated: the launches and the copy see the same clocks
            for k, (t, _, _, _) in timed(eng, lambda: eng.color_jitter(slab, offsets, sizes, recs, out=out), a.iters).items():
                ms.setdefault(k, []).append(t)
            ms.setdefault('copy', []).append(copy_ms(a.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rows[name] = {'ms_rounds': {k: [round(x, 4) for x in v] for k, v in ms.items()}, 'ms_median': {k: round(v, 4) for k, v in med.items()},
                      'counted_MB': {k: round(counted[k] / 1e6, 1) for k in med}, 'achieved_GBps': {k: round(counted[k] / (med[k] * 1e-3) / 1e9, 1) for k in med},
                      'frac_of_hbm_peak': {k: round(counted[k] / (med[k] * 1e-3) / HBM_PEAK, 3) for k in med},
                      'apply_over_copy': round(med['color_jitter_apply'] / med['copy'], 2)}
    hue_cost = rows['full']['ms_median']['color_jitter_apply'] / rows['no_hue']['ms_median']['color_jitter_apply']
    rows['binding_limit'] = {'apply_full_over_apply_no_hue': round(hue_cost, 2), 'apply_no_hue_over_copy': rows['no_hue']['apply_over_copy'],
                             'apply_full_over_copy': rows['full']['apply_over_copy'],
                             'statement': binding_statement(rows['full']['apply_over_copy'], rows['no_hue']['apply_over_copy'], hue_cost)}

    def pil_chain(arg):
        img, rec = Image.fromarray(arg[0]), arg[1]
        f = rec[4:7].view(np.float32)
        for op in rec[:4]:
            if op == 0:
                img = ImageEnhance.Brightness(img).enhance(float(f[0]))
            elif op == 1:
                img = ImageEnhance.Contrast(img).enhance(float(f[1]))
            elif op == 2:
                img = ImageEnhance.Color(img).enhance(float(f[2]))
            elif op == 3:                                               # torchvision's adjust_hue
                h, s_, v = img.convert('HSV').split()
                h = Image.fromarray((np.asarray(h).astype(np.int32) + int(rec[7])).astype(np.uint8), 'L')
                img = Image.merge('HSV', (h, s_, v)).convert('RGB')
        return np.asarray(img)

    def host_route():
        with ThreadPoolExecutor(max_workers=16) as ex:
            frames = list(ex.map(pil_chain, zip(imgs, full)))
        res = pack_frames(frames, dev)[0]
        torch.cuda.synchronize()
        return res

    def device_route():
        s_, o_, z_ = pack_frames(imgs, dev)
        res = eng.color_jitter(s_, o_, z_, full, out=s_)
        torch.cuda.synchronize()
        return res
    same = bool(torch.equal(host_route(), device_route()))              # warm-up, and the comparison
    wall = {'host': [], 'device': []}
    for _ in range(3):
        for name, fn in (('host', host_route), ('device', device_route)):
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    rows['host_comparison'] = {'host_16_threads_ms': [round(v, 1) for v in wall['host']], 'device_ms': [round(v, 1) for v in wall['device']],
                               'identical_slabs': same, 'ratio_host_over_device': round(float(np.median(wall['host']) / np.median(wall['device'])), 1)}
    rows['workload'] = f'{len(imgs)} frames of 1080 x 1920 ({N * 3 / 1e6:.1f} MB), brightness / contrast / saturation 0.2, hue 0.1, a seeded order per frame'
    print(json.dumps(rows, indent=1))
    return rows


def jpeg_decode_section(eng, a):
    """64 frames of 1080p, natural-like content (low-frequency structure plus mild noise), at quality 75 and 95, from files on disk to
    the frame slab on the device: 16 Pillow threads + pack + one upload against read bytes + one upload + one specmi_jpeg_decode
    (preprocess.decode_frames).  Wall clock, 3 alternated rounds after one warm-up of each; the slabs are compared."""
    import tempfile
    import time
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from spec_amd import preprocess
    dev = eng.device
    rows, imgs = {}, natural_frames_1080p()
    with tempfile.TemporaryDirectory() as tmp:
        for q in (75, 95):
            paths = [os.path.join(tmp, f'q{q}_{i:02d}.jpg') for i in range(64)]
            for path, img in zip(paths, imgs):
                Image.fromarray(img).save(path, quality=q)

            def host_route():
                with ThreadPoolExecutor(max_workers=16) as ex:
                    frames = list(ex.map(preprocess._host_rgb, paths))
                out = preprocess.pack_frames(frames, dev)
                torch.cuda.synchronize()
                return out

            def device_route():
                out = preprocess.decode_frames(paths, dev, True)
                torch.cuda.synchronize()
                return out

            want, got = host_route(), device_route()          # warm-up, and the comparison
            same = bool(torch.equal(want[0], got[0])) and want[2] == got[2]
            ms = {'host': [], 'device': []}
            for _ in range(3):
                for name, fn in (('host', host_route), ('device', device_route)):
                    t0 = time.perf_counter()
                    fn()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            spread = max(ms['host']) - min(ms['host'])
            rows[f'q{q}'] = {'frames': 64, 'size': [1080, 1920], 'file_MB': round(sum(os.path.getsize(p) for p in paths) / 1e6, 2),
                             'host_16_threads_ms': [round(v, 1) for v in ms['host']], 'device_ms': [round(v, 1) for v in ms['device']],
                             'host_spread_ms': round(spread, 1), 'passes': eng.jpeg_decode_passes, 'identical_slabs': same,
                             'device_ahead_beyond_host_spread': bool(min(ms['host']) - max(ms['device']) > spread)}
    rows['default_on_rule'] = 'engine.JPEG_DECODE_DEVICE_DEFAULT becomes True only when device_ahead_beyond_host_spread holds at both qualities'
    rows['rule_met'] = bool(rows['q75']['device_ahead_beyond_host_spread'] and rows['q95']['device_ahead_beyond_host_spread'])
    print(json.dumps(rows, indent=1))
    return rows


def png_decode_section(eng, a):
    """PNG files on disk to the frame slab on the device, two content classes: the 64 synthetic 1080p frames of ``--only jpeg_decode``
    saved at Pillow's default level, and the eight 1080 x 5760 three-panel pictures of ``--only jpeg_encode`` (flat areas with long
    matches).  HOST = 16 Pillow threads + pack + one upload, DEVICE = read bytes + one upload + one specmi_png_decode
    (preprocess.decode_frames).  Wall clock, 3 alternated rounds after one warm-up of each; the slabs are compared.  For information:
    the same with the first 1 and 8 files, and the three stages' times from HIP events (library profiler)."""
    import tempfile
    import time
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from spec_amd import preprocess
    dev = eng.device
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:1080, 0:1920]
    noise = [rng.normal(0, 5, (1080, 1920, 3)) for _ in range(4)]
    frames = []
    for i in range(64):
        base = np.stack([128 + 80 * np.sin(yy / (60.0 + 7 * c + i) + i) * np.cos(xx / (90.0 + 11 * c) + 0.3 * i) + 30 * np.sin((xx + yy) / (17.0 + i % 5))
                         for c in range(3)], axis=2)
        frames.append(np.clip(base + noise[i % 4], 0, 255).astype(np.uint8))
    v8, f, t8, _, _, _ = render_workload()
    slab, geom, offsets = demo_pictures(eng, np.random.default_rng(0), v8, f, t8)
    raw = slab.cpu().numpy()
    panels = [raw[o:o + h * pitch].reshape(h, w, 3) for (h, w), (o, pitch) in zip(geom, offsets)]
    del slab
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        for cls, imgs in (('frames_1080p', frames), ('three_panel', panels)):
            paths = [os.path.join(tmp, f'{cls}_{i:02d}.png') for i in range(len(imgs))]
            for path, img in zip(paths, imgs):
                Image.fromarray(img).save(path)
            for n in sorted({1, 8, len(paths)}):
                sub = paths[:n]

                def host_route():
                    with ThreadPoolExecutor(max_workers=16) as ex:
                        fr = list(ex.map(preprocess._host_rgb, sub))
                    out = preprocess.pack_frames(fr, dev)
                    torch.cuda.synchronize()
                    return out

                def device_route():
                    out = preprocess.decode_frames(sub, dev, False, True)
                    torch.cuda.synchronize()
                    return out

                want, got = host_route(), device_route()          # warm-up, and the comparison
                same = bool(torch.equal(want[0], got[0])) and want[2] == got[2]
                ms = {'host': [], 'device': []}
                for _ in range(3):
                    for name, fn in (('host', host_route), ('device', device_route)):
                        t0 = time.perf_counter()
                        fn()
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                spread = max(ms['host']) - min(ms['host'])
                row = {'files': n, 'size': list(imgs[0].shape[:2]), 'file_MB': round(sum(os.path.getsize(p) for p in sub) / 1e6, 2),
                       'host_16_threads_ms': [round(v, 1) for v in ms['host']], 'device_ms': [round(v, 1) for v in ms['device']],
                       'host_spread_ms': round(spread, 1), 'identical_slabs': same,
                       'device_ahead_beyond_host_spread': bool(min(ms['host']) - max(ms['device']) > spread)}
                if n == len(paths):
                    row['stage_ms'] = {k: round(v[0], 3) for k, v in timed(eng, device_route, 1).items() if k.startswith('pdec_')}
                rows[f'{cls}_{n}'] = row
    full = [rows[f'frames_1080p_{len(frames)}'], rows[f'three_panel_{len(panels)}']]
    rows['default_on_rule'] = ('engine.PNG_DECODE_DEVICE_DEFAULT becomes True only when device_ahead_beyond_host_spread holds for the whole batch of '
                               'both content classes')
    rows['rule_met'] = bool(all(r['device_ahead_beyond_host_spread'] and r['identical_slabs'] for r in full))
    print(json.dumps(rows, indent=1))
    return rows


def smpl_backward_section(a):
    """``specmi_smpl_forward``, ``specmi_smpl_backward`` and ``specmi_hmr_loss_backward`` at B = ``--batch`` (256), V = 6890
    (SMPLCamHead mode), and torch's own autograd (forward + backward) over the oracle chain - oracle/smpl.py, oracle/geometry.py,
    fp32 - moved to the same device.  HIP events around ``iters`` back-to-back calls after a warm-up of the same calls, the four
    alternated in this process, 3 rounds; then the backward's kernels by the library profiler."""
    from oracle.geometry import convert_pare_to_full_img_cam
    from oracle.smpl import SMPLOracle
    from spec_amd import assets, differentiable
    from spec_amd.cam_utils import _engine
    dev = torch.device('cuda', 0)
    B, V = a.batch, 6890
    model = assets.smpl_model()
    eng, leng = differentiable._smpl_engine(dev, model, True, 224, 5000.), _engine(dev)
    rng = np.random.default_rng(0)
    f = lambda *shape, std=1.0: torch.from_numpy((rng.standard_normal(shape) * std).astype(np.float32)).to(dev)
    rot = torch.linalg.qr(f(B, 24, 3, 3))[0].contiguous()
    betas, cam = f(B, 10, std=0.8), torch.cat([0.6 + 0.5 * torch.rand(B, 1, device=dev), f(B, 2, std=0.1)], 1)
    K = torch.zeros(B, 3, 3, device=dev)
    K[:, 0, 0] = K[:, 1, 1] = 1000.
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 960., 540., 1.
    camera = (torch.eye(3, device=dev).repeat(B, 1, 1), K, 0.8 + torch.rand(B, device=dev), torch.tensor([[960., 540.]], device=dev).repeat(B, 1),
              torch.full((B,), 1920., device=dev), torch.full((B,), 1080., device=dev))
    ups = dict(g_vertices=f(B, V, 3, std=0.01), g_joints3d=f(B, 49, 3, std=0.1), g_joints2d=f(B, 49, 2, std=0.001), g_cam_t=f(B, 3, std=0.1))
    pred = {'pred_pose': rot, 'pred_shape': betas, 'pred_cam': cam, 'smpl_joints3d': f(B, 49, 3), 'smpl_joints2d': f(B, 49, 2) * 100,
            'smpl_vertices': f(B, V, 3)}
    gt = {'pose': f(B, 72) * 0.3, 'betas': f(B, 10), 'pose_conf': torch.ones(B, 24, device=dev), 'pose_3d': f(B, 24, 4),
          'keypoints_orig': f(B, 49, 3).abs() * 100, 'vertices': f(B, V, 3), 'has_smpl': torch.ones(B, dtype=torch.int32, device=dev),
          'has_pose_3d': torch.ones(B, dtype=torch.int32, device=dev), 'orig_shape': torch.full((B, 2), 480., device=dev),
          'scale': torch.ones(B, device=dev)}
    wl = [1., 5., 1., 1., 0.001, 0., 1., 60.]
    res = leng.hmr_loss(1, pred, gt, wl)
    gm = torch.tensor([0., 0, 0, 0, 0, 0, 1], device=dev)
    oracle = SMPLOracle(model).to(dev)

    def torch_autograd():
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(True) for t in (rot, betas, cam)]
            verts, j3d = oracle(leaves[1], leaves[0])
            cam_t = convert_pare_to_full_img_cam(pare_cam=leaves[2], bbox_height=camera[2] * 200., bbox_center=camera[3], img_w=camera[4],
                                                 img_h=camera[5], focal_length=K[:, 0, 0], crop_res=224)
            pts = torch.einsum('bij,bkj->bki', camera[0], j3d) + cam_t.unsqueeze(1)
            j2d = torch.einsum('bij,bkj->bki', K, pts / pts[:, :, -1:])[:, :, :-1]
            obj = (verts * ups['g_vertices']).sum() + (j3d * ups['g_joints3d']).sum() + (j2d * ups['g_joints2d']).sum() + (cam_t * ups['g_cam_t']).sum()
            torch.autograd.grad(obj, leaves)

    calls = {'smpl_forward': lambda: eng.smpl(rot, betas, cam, *camera),
             'smpl_backward': lambda: eng.smpl_backward(rot, betas, cam, *camera, **ups),
             'hmr_loss_backward': lambda: leng.hmr_loss_backward(1, pred, gt, wl, res, gm),
             'torch_autograd_forward_and_backward': torch_autograd}

    def ms_per_call(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    rounds = {k: [] for k in calls}
    for _ in range(3):                                              # alternated: all see the same clocks and the same neighbours
        for k, fn in calls.items():
            rounds[k].append(ms_per_call(fn))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    kern = {k: {'ms_per_launch': round(v[0], 5), 'TFLOPs': round(v[2] / (v[0] * 1e-3) / 1e12, 2) if v[2] else None}
            for k, v in timed(eng, calls['smpl_backward'], a.iters).items()}
    row = {'workload': f'B = {B}, V = {V}, SMPLCamHead mode; smpl_backward recomputes the forward (its three kernels are part of its time); '
                       'hmr_loss_backward: HMRCamLoss, shape_loss_weight 1, all six gradients',
           'ms_round_values': {k: [round(x, 5) for x in v] for k, v in rounds.items()}, 'ms_median': {k: round(v, 5) for k, v in med.items()},
           'spread_between_rounds_ms': {k: round(max(v) - min(v), 5) for k, v in rounds.items()},
           'backward_over_forward': round(med['smpl_backward'] / med['smpl_forward'], 3),
           'torch_autograd_over_forward_plus_backward': round(med['torch_autograd_forward_and_backward'] / (med['smpl_forward'] + med['smpl_backward']), 3),
           'smpl_backward_kernels_by_the_library_profiler': kern}
    print(json.dumps(row, indent=1))
    return row


def head_train_section(a):
    """The trainable HMRHead (``specmi_hmr_head_train_forward`` + ``specmi_hmr_head_backward`` with the draw of the dropout masks:
    one training step's forward and backward of the regressor, all eleven gradients) at F = 2048, use_cam_feats, p = 0.5, three
    iterations, B = 64 and B = 256, next to torch's own autograd over the same head as a plain nn.Module (oracle/heads.py in train
    mode, fp32, rocBLAS / hipBLASLt) on the same device and the same parameters.  HIP events around ``iters`` back-to-back calls
    after a warm-up, the two alternated in this process, 3 rounds; then the library's kernels by its profiler."""
    from oracle.heads import HMRHead as PlainHead
    from spec_amd.cam_utils import _engine
    dev = torch.device('cuda', 0)
    eng = _engine(dev)
    F, n_iter, p = 2048, 3, 0.5
    out = {}
    for B in (64, 256):
        torch.manual_seed(B)
        plain = PlainHead(F, smpl_mean_params={'pose': np.tile([1., 0, 0, 1, 0, 0], 24), 'shape': np.zeros(10), 'cam': np.array([0.9, 0, 0])},
                          use_cam_feats=True).to(dev).train()
        params = {k: v.detach() for k, v in plain.named_parameters()}
        xf = torch.rand(B, F, device=dev) * 1.5
        init = torch.cat([plain.init_pose, plain.init_shape, plain.init_cam], 1).expand(B, -1).contiguous()
        rot = torch.linalg.qr(torch.randn(B, 3, 3, device=dev))[0].contiguous()
        vfov = 0.6 + 0.8 * torch.rand(B, device=dev)
        cam_feats = torch.cat([rot[:, :, :2].reshape(B, 6), vfov[:, None]], 1)
        g_state = torch.randn(B, 157, device=dev)

        def library():
            masks = torch.rand(2 * n_iter, B, 1024, device=dev) >= p
            _, tape = eng.hmr_head_train_forward(params, xf, init, cam_feats, masks, p, n_iter)
            eng.hmr_head_backward(params, xf, tape, g_state, cam_feats, masks, p, n_iter)

        def torch_autograd():
            with torch.enable_grad():
                feats = xf[:, :, None, None].detach().requires_grad_(True)
                o = plain(feats, cam_rotmat=rot, cam_vfov=vfov, n_iter=n_iter)
                state = torch.cat([o['pred_pose_6d'], o['pred_shape'], o['pred_cam']], 1)
                torch.autograd.grad((state * g_state).sum(), [feats] + list(plain.parameters()))

        def ms_per_call(fn):
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters
        calls = {'library_forward_and_backward': library, 'torch_autograd_forward_and_backward': torch_autograd}
        rounds = {k: [] for k in calls}
        for _ in range(3):                                          # alternated: both see the same clocks and the same neighbours
            for k, fn in calls.items():
                rounds[k].append(ms_per_call(fn))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        kern = {k: {'launches_per_call': v[3], 'ms_per_launch': round(v[0], 5), 'ms_per_call': round(v[0] * v[3], 5),
                    'TFLOPs': round(v[2] / (v[0] * 1e-3) / 1e12, 2) if v[2] else None} for k, v in timed(eng, library, a.iters).items()}
        out[f'B{B}'] = {'workload': f'B = {B}, F = {F}, use_cam_feats, p = {p}, n_iter = {n_iter}; the library call includes the draw of the masks, '
                                    'torch draws its own inside nn.Dropout; both return g_xf and the ten parameter gradients',
                        'ms_round_values': {k: [round(x, 5) for x in v] for k, v in rounds.items()}, 'ms_median': {k: round(v, 5) for k, v in med.items()},
                        'spread_between_rounds_ms': {k: round(max(v) - min(v), 5) for k, v in rounds.items()},
                        'library_over_torch_autograd': round(med['library_forward_and_backward'] / med['torch_autograd_forward_and_backward'], 3),
                        'library_kernels_by_the_library_profiler': kern}
    print(json.dumps(out, indent=1))
    return out


def camcalib_train_section(a):
    """CamCalib's differentiable tail (``specmi_camcalib_head_train_forward`` -> ``specmi_camcalib_loss`` ->
    ``specmi_camcalib_loss_backward`` -> ``specmi_camcalib_head_backward``, g_xf and all 6 L parameter gradients) at F = 2048,
    nbins = 256, L = 1 and L = 3 x 1024, B = 16 and 64, 'softargmax_biased_l2': the grouped launches (one per step for the three
    heads, the default) against three single launches per step (option "camcalib_head_group" = 0, same bits), next to torch's own
    autograd over the same heads as plain ``nn.Linear``s and the restated loss (fp32, rocBLAS / hipBLASLt) on the same device and
    the same parameters.  HIP events around ``iters`` back-to-back calls after a warm-up, the three alternated in this process,
    3 rounds; then the library's kernels by its profiler."""
    from spec_amd.cam_utils import _engine
    from spec_amd.engine import camcalib_head_param_names
    dev = torch.device('cuda', 0)
    eng = _engine(dev)
    F, nbins, Hc, lt, weights = 2048, 256, 1024, 'softargmax_biased_l2', (1.0, 1.0, 1.0)
    eng.set_option('experimental', 1)           # "camcalib_head_group" is on the experimental list
    g_means = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
    idx = torch.arange(nbins, device=dev, dtype=torch.float32)
    out = {}
    for L in (1, 3):
        for B in (16, 64):
            torch.manual_seed(100 * L + B)
            widths = [F] + [Hc] * (L - 1) + [nbins]
            plain = torch.nn.ModuleDict({h: (torch.nn.Linear(F, nbins) if L == 1 else
                                             torch.nn.Sequential(*(torch.nn.Linear(i, o) for i, o in zip(widths[:-1], widths[1:]))))
                                         for h in ('fc_vfov', 'fc_pitch', 'fc_roll')}).to(dev)
            names = camcalib_head_param_names(L)
            named = dict(plain.named_parameters())
            params = {n: named[n].detach() for n in names}
            xf = torch.rand(B, F, device=dev) * 1.5
            targets = [torch.rand(B, device=dev) * 2 - 1 for _ in range(3)]

            def library():
                logits, tape = eng.camcalib_head_train_forward(params, xf, L)
                eng.camcalib_loss(logits, targets, lt, weights)
                g = eng.camcalib_loss_backward(logits, targets, lt, weights, g_means)
                eng.camcalib_head_backward(params, xf, L, tape, torch.stack(g))

            def single(fn):                                             # the option is set around the timed loop, not inside it
                def run(*args):
                    eng.set_option('camcalib_head_group', 0)
                    try:
                        return fn(*args)
                    finally:
                        eng.set_option('camcalib_head_group', 1)
                return run

            def torch_autograd():
                with torch.enable_grad():
                    x = xf.detach().requires_grad_(True)
                    total = 0.0
                    for k, h in enumerate(('fc_vfov', 'fc_pitch', 'fc_roll')):
                        p = torch.softmax(plain[h](x), -1)
                        s = 2 * (p * idx).sum(-1) / (nbins - 1) - 1
                        l2 = (targets[k] - s) ** 2
                        total = total + weights[k] * (torch.where(s > targets[k], l2, l2 / (l2 + 1)) if k == 0 else l2).mean()
                    torch.autograd.grad(total, [x] + list(plain.parameters()))

            def ms_per_call(fn):
                for _ in range(5):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / a.iters
            calls = {'library_grouped': lambda: ms_per_call(library), 'library_single_launches': single(lambda: ms_per_call(library)),
                     'torch_autograd': lambda: ms_per_call(torch_autograd)}
            rounds = {k: [] for k in calls}
            for _ in range(3):                                          # alternated: all see the same clocks and the same neighbours
                for k, fn in calls.items():
                    rounds[k].append(fn())
            med = {k: float(np.median(v)) for k, v in rounds.items()}

            def kernels(fn):
                return {k: {'launches_per_call': v[3], 'ms_per_launch': round(v[0], 5), 'ms_per_call': round(v[0] * v[3], 5),
                            'TFLOPs': round(v[2] / (v[0] * 1e-3) / 1e12, 2) if v[2] else None} for k, v in timed(eng, fn, a.iters).items()}
            kg, ks = kernels(library), single(kernels)(library)
            out[f'L{L}_B{B}'] = {'workload': f'B = {B}, F = {F}, L = {L}' + (f' x {Hc}' if L > 1 else '') + f', nbins = {nbins}, {lt}; head forward, loss, loss '
                                 'backward, head backward with g_xf and every parameter gradient',
                                 'ms_round_values': {k: [round(x, 5) for x in v] for k, v in rounds.items()},
                                 'ms_median': {k: round(v, 5) for k, v in med.items()},
                                 'spread_between_rounds_ms': {k: round(max(v) - min(v), 5) for k, v in rounds.items()},
                                 'grouped_over_single': round(med['library_grouped'] / med['library_single_launches'], 3),
                                 'library_over_torch_autograd': round(med['library_grouped'] / med['torch_autograd'], 3),
                                 'device_ms_per_call_by_the_library_profiler': {'grouped': round(sum(v['ms_per_call'] for v in kg.values()), 5),
                                                                               'single_launches': round(sum(v['ms_per_call'] for v in ks.values()), 5)},
                                 'launches_per_call': {'grouped': sum(v['launches_per_call'] for v in kg.values()),
                                                       'single_launches': sum(v['launches_per_call'] for v in ks.values())},
                                 'grouped_kernels_by_the_library_profiler': kg, 'single_kernels_by_the_library_profiler': ks}
    print(json.dumps(out, indent=1))
    return out


def conv_backward_section(a):
    """The trainable ResNet layer (``specmi_conv2d_train_forward`` / ``specmi_conv2d_backward``, spec_amd/csrc/conv_bwd.hip) on every
    distinct layer4 layer of ResNet-50 at CamCalib's fine-tuning shape (batch ``DATASET.BATCH_SIZE`` = 64, the stage-3 map of a
    600 x 1000 frame, 38 x 63) and at SPEC's (B = 64, a 14 x 14 stage-3 map, 7 x 7 out): forward, data gradient and weight gradient,
    each next to torch's own ``aten.convolution`` / ``aten.convolution_backward`` (MIOpen) on the same device tensors (NHWC memory,
    OIHW weights), alternated in this process, 3 rounds of ``iters`` back-to-back calls after a warm-up; then the library's kernels by
    its profiler; then the whole fine-tuning step with layer4 unfrozen against the head-only step."""
    from spec_amd import camcalib_eval as ce
    from spec_amd.cam_utils import _engine
    dev = torch.device('cuda', 0)
    eng = _engine(dev)
    bs = int(ce.DEFAULTS['DATASET']['BATCH_SIZE'])
    layers = [('0.conv1', 1024, 512, 1, 1, 0), ('0.conv2', 512, 512, 3, 2, 0), ('0.downsample', 1024, 2048, 1, 2, 0),
              ('n.conv3', 512, 2048, 1, 1, 1), ('1.conv1', 2048, 512, 1, 1, 1), ('1.conv2', 512, 512, 3, 1, 1)]     # last: 1 = on the stage's output map
    shapes = {'camcalib_b%d_38x63' % bs: (bs, 38, 63), 'spec_b64_14x14': (64, 14, 14)}

    def ms_per_call(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    out = {}
    for sname, (B, h, w) in shapes.items():
        for lname, cin, cout, k, stride, on_out in layers:
            H, W = ((h + 1) // 2, (w + 1) // 2) if on_out else (h, w)
            pad = k // 2
            torch.manual_seed(cin + cout + k + stride)
            x = torch.randn(B, H, W, cin, device=dev)
            wt = torch.randn(cout, cin, k, k, device=dev) / float(np.sqrt(cin * k * k))
            scale, shift = 0.5 + torch.rand(cout, device=dev), 0.3 * torch.randn(cout, device=dev)
            relu = lname != '0.downsample'
            y = eng.conv2d_train_forward(x, wt, scale, shift, stride, pad, None, relu)
            g_y = torch.randn_like(y)
            xn, gn = x.permute(0, 3, 1, 2), g_y.permute(0, 3, 1, 2)             # channels_last views of the same memory
            conv = lambda: torch.ops.aten.convolution(xn, wt, None, [stride] * 2, [pad] * 2, [1, 1], False, [0, 0], 1)
            bwd = lambda mask: (lambda: torch.ops.aten.convolution_backward(gn, xn, wt, None, [stride] * 2, [pad] * 2, [1, 1], False, [0, 0], 1, mask))
            lib_bwd = lambda want: (lambda: eng.conv2d_backward(x, wt, scale, stride, pad, y, g_y, relu, None, want))
            calls = {'forward': (lambda: eng.conv2d_train_forward(x, wt, scale, shift, stride, pad, None, relu), conv),
                     'dgrad': (lib_bwd((True, False, False)), bwd([True, False, False])),
                     'wgrad': (lib_bwd((False, True, False)), bwd([False, True, False]))}
            rounds = {p: {'library': [], 'torch': []} for p in calls}
            for _ in range(3):                                          # alternated: both see the same clocks and the same neighbours
                for p, (mine, theirs) in calls.items():
                    rounds[p]['library'].append(ms_per_call(mine))
                    rounds[p]['torch'].append(ms_per_call(theirs))
            kern = timed(eng, lambda: (calls['forward'][0](), eng.conv2d_backward(x, wt, scale, stride, pad, y, g_y, relu, None, (True, True, True))),
                         a.iters)
            row = {'workload': f'B = {B}, {H} x {W} x {cin} -> {cout}, {k}x{k} stride {stride}' + (', relu' if relu else ''),
                   'kernels_by_the_library_profiler': {kk: {'ms_per_launch': round(v[0], 5), 'TFLOPs': round(v[2] / (v[0] * 1e-3) / 1e12, 2) if v[2] else None}
                                                       for kk, v in kern.items()}}
            for p in calls:
                lib, tor = float(np.median(rounds[p]['library'])), float(np.median(rounds[p]['torch']))
                row[p] = {'library_ms': round(lib, 5), 'torch_ms': round(tor, 5), 'library_over_torch': round(lib / tor, 3),
                          'library_rounds_ms': [round(v, 5) for v in rounds[p]['library']], 'torch_rounds_ms': [round(v, 5) for v in rounds[p]['torch']]}
            out[f'{sname}.layer4.{lname}'] = row
            print(sname, lname, {p: (row[p]['library_ms'], row[p]['torch_ms']) for p in calls}, flush=True)
            del x, wt, y, g_y, xn, gn
    # the whole step: stages=3 under no_grad -> ResNetStage -> heads -> loss -> backward -> Adam, against the head-only step
    from spec_amd import synth
    from spec_amd.camcalib_train import trunk_features
    from spec_amd.differentiable import CameraRegressorHead, ResNetStage
    from spec_amd.losses import CameraRegressorLoss
    from spec_amd.modules import CameraRegressorNetwork
    net = CameraRegressorNetwork()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.camcalib_state(1001).items()}, strict=False)
    net = net.to(dev).eval()
    net.set_plan('throughput')
    net.commit(dev, freeze=True)
    images = torch.randn(bs, 3, 600, 1000, device=dev)
    targets = [torch.randint(0, 256, (bs,), device=dev) for _ in range(3)]
    head, stage, crit = CameraRegressorHead.from_model(net), ResNetStage.from_model(net, 'layer4'), CameraRegressorLoss(1.0, 1.0, 1.0, 'ce')
    opts = {'head_only': torch.optim.Adam(head.parameters(), lr=1e-6), 'unfreeze_layer4': torch.optim.Adam(list(head.parameters()) + stage.conv_parameters(), lr=1e-6)}

    def step(which):
        def run():
            feat = trunk_features(net, images, stages=3 if which == 'unfreeze_layer4' else None)
            with torch.enable_grad():
                if which == 'unfreeze_layer4':
                    feat = stage(feat)
                loss, _ = crit(*head(feat, channels_last=True), *targets)
                opts[which].zero_grad(set_to_none=True)
                loss.backward()
            opts[which].step()
        return run
    rounds = {k: [] for k in opts}
    for _ in range(3):
        for k in opts:
            rounds[k].append(ms_per_call(step(k)))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    out['whole_step'] = {'workload': f'ResNet-50 CamCalib, B = {bs} frames of 600 x 1000, ce loss, Adam: frozen trunk -> [layer4 with gradients] -> heads -> loss -> '
                         'backward -> step', 'ms_round_values': {k: [round(x, 3) for x in v] for k, v in rounds.items()},
                         'ms_median': {k: round(v, 3) for k, v in med.items()}, 'unfreeze_over_head_only': round(med['unfreeze_layer4'] / med['head_only'], 3)}
    print(json.dumps(out['whole_step'], indent=1))
    return out


def bn_train_section(a):
    """BatchNorm in training mode (``specmi_batchnorm_train_forward`` / ``specmi_batchnorm_backward``, spec_amd/csrc/bn_train.hip) at
    every distinct BatchNorm shape of layer4 in the fine-tuning step - the output maps of the layers ``conv_backward_section`` times, at
    CamCalib's shape (B = 64, the 38 x 63 stage-3 map) and SPEC's (B = 64, 14 x 14): the forward (statistics, running statistics,
    apply, ReLU; the residual where the BatchNorm is bn3) and forward + backward, each next to torch's ``F.batch_norm`` (+ residual,
    ReLU) with its autograd backward on the same device tensors (channels_last views), alternated in this process, 3 rounds of
    ``iters`` back-to-back calls after a warm-up; the library's kernels by its profiler with the bytes they must move over their
    time; then the whole fine-tuning step with layer4 unfrozen on batch statistics against the same step on frozen BatchNorm, and the
    share of ``conv_bwd_prep_kernel`` - with the identity scale a plain copy of g_z - in it."""
    import torch.nn.functional as F
    from spec_amd import camcalib_eval as ce
    from spec_amd.cam_utils import _engine
    dev = torch.device('cuda', 0)
    eng = _engine(dev)
    bs = int(ce.DEFAULTS['DATASET']['BATCH_SIZE'])
    # (name, map of the stage's input 0 / output 1, channels, residual)
    bns = [('0.bn1', 0, 512, False), ('n.bn2', 1, 512, False), ('n.bn3', 1, 2048, True), ('0.downsample.1', 1, 2048, False)]
    shapes = {'camcalib_b%d_38x63' % bs: (bs, 38, 63), 'spec_b64_14x14': (64, 14, 14)}

    def ms_per_call(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    out = {}
    for sname, (B, h, w) in shapes.items():
        for lname, on_out, Cn, with_res in bns:
            H, W = ((h + 1) // 2, (w + 1) // 2) if on_out else (h, w)
            relu = lname != '0.downsample.1'
            torch.manual_seed(H + W + Cn)
            z = torch.randn(B, H, W, Cn, device=dev)
            gamma, beta = 0.5 + torch.rand(Cn, device=dev), 0.3 * torch.randn(Cn, device=dev)
            rm, rv = torch.zeros(Cn, device=dev), torch.ones(Cn, device=dev)
            res = torch.randn_like(z) if with_res else None
            g_y = torch.randn_like(z)
            want = (True, True, True, with_res)

            def lib_fwd():
                return eng.batchnorm_train_forward(z, gamma, beta, 1e-5, res, relu, rm, rv, 0.1)

            def lib_both():
                y, mean, invstd = lib_fwd()
                return eng.batchnorm_backward(z, gamma, mean, invstd, y if relu else None, g_y, relu, want)
            zt, gt, bt = z.permute(0, 3, 1, 2).requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            rt = res.permute(0, 3, 1, 2).requires_grad_(True) if with_res else None
            gn = g_y.permute(0, 3, 1, 2)

            def torch_fwd():
                with torch.enable_grad():
                    y = F.batch_norm(zt, rm, rv, gt, bt, True, 0.1, 1e-5)
                    y = y + rt if with_res else y
                    return torch.relu(y) if relu else y

            def torch_both():
                torch.autograd.grad(torch_fwd(), [zt, gt, bt] + ([rt] if with_res else []), gn)
            calls = {'forward': (lib_fwd, torch_fwd), 'forward_backward': (lib_both, torch_both)}
            rounds = {p: {'library': [], 'torch': []} for p in calls}
            for _ in range(3):                                          # alternated: both see the same clocks and the same neighbours
                for p, (mine, theirs) in calls.items():
                    rounds[p]['library'].append(ms_per_call(mine))
                    rounds[p]['torch'].append(ms_per_call(theirs))
            kern = timed(eng, lib_both, a.iters)
            row = {'workload': f'(M, C) = ({B * H * W}, {Cn}): B = {B}, {H} x {W}' + (', relu' if relu else '') + (', residual' if with_res else ''),
                   'kernels_by_the_library_profiler': {kk: {'ms_per_launch': round(v[0], 5), 'algorithmic_MB': round(v[1] / 1e6, 3),
                                                            'achieved_GBps': round(v[1] / (v[0] * 1e-3) / 1e9, 1),
                                                            'frac_of_hbm_peak': round(v[1] / (v[0] * 1e-3) / HBM_PEAK, 4)} for kk, v in kern.items()}}
            for p in calls:
                lib, tor = float(np.median(rounds[p]['library'])), float(np.median(rounds[p]['torch']))
                names = [k for k in kern if k.startswith('bn_train')] + ([k for k in kern if k.startswith('bn_bwd')] if p == 'forward_backward' else [])
                by = sum(kern[k][1] for k in names)
                row[p] = {'library_ms': round(lib, 5), 'torch_ms': round(tor, 5), 'library_over_torch': round(lib / tor, 3),
                          'algorithmic_MB': round(by / 1e6, 3), 'library_GBps_over_the_call': round(by / (lib * 1e-3) / 1e9, 1),
                          'library_rounds_ms': [round(v, 5) for v in rounds[p]['library']], 'torch_rounds_ms': [round(v, 5) for v in rounds[p]['torch']]}
            out[f'{sname}.layer4.{lname}'] = row
            print(sname, lname, {p: (row[p]['library_ms'], row[p]['torch_ms']) for p in calls}, flush=True)
            del z, res, g_y, zt, rt, gn
    # the whole step: stages=3 under no_grad -> ResNetStage -> heads -> loss -> backward -> Adam, on batch statistics against frozen BatchNorm
    from spec_amd import synth
    from spec_amd.camcalib_train import trunk_features
    from spec_amd.differentiable import CameraRegressorHead, ResNetStage
    from spec_amd.losses import CameraRegressorLoss
    from spec_amd.modules import CameraRegressorNetwork
    net = CameraRegressorNetwork()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.camcalib_state(1001).items()}, strict=False)
    net = net.to(dev).eval()
    net.set_plan('throughput')
    net.commit(dev, freeze=True)
    images = torch.randn(bs, 3, 600, 1000, device=dev)
    targets = [torch.randint(0, 256, (bs,), device=dev) for _ in range(3)]
    head, crit = CameraRegressorHead.from_model(net), CameraRegressorLoss(1.0, 1.0, 1.0, 'ce')
    stages = {'frozen': ResNetStage.from_model(net, 'layer4', 'frozen'), 'batch': ResNetStage.from_model(net, 'layer4', 'batch')}
    opts = {'frozen': torch.optim.Adam(list(head.parameters()) + stages['frozen'].conv_parameters(), lr=1e-6),
            'batch': torch.optim.Adam(list(head.parameters()) + stages['batch'].conv_parameters() + stages['batch'].bn_parameters(), lr=1e-6)}

    def step(which):
        def run():
            net.backbone.layer4.train(which == 'batch')                 # the blocks alone; the stages share them
            feat = trunk_features(net, images, stages=3)
            with torch.enable_grad():
                loss, _ = crit(*head(stages[which](feat), channels_last=True), *targets)
                opts[which].zero_grad(set_to_none=True)
                loss.backward()
            opts[which].step()
        return run
    rounds = {k: [] for k in opts}
    for _ in range(3):
        for k in opts:
            rounds[k].append(ms_per_call(step(k)))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    kern = timed(eng, step('batch'), a.iters)
    net.backbone.layer4.eval()
    per_step = {k: v[0] * v[3] for k, v in kern.items()}
    out['whole_step'] = {'workload': f'ResNet-50 CamCalib, B = {bs} frames of 600 x 1000, ce loss, Adam: frozen trunk -> layer4 with gradients -> heads -> loss -> '
                         'backward -> step; BatchNorm of layer4 frozen, or on batch statistics with gamma / beta trained',
                         'ms_round_values': {k: [round(x, 3) for x in v] for k, v in rounds.items()}, 'ms_median': {k: round(v, 3) for k, v in med.items()},
                         'batch_over_frozen': round(med['batch'] / med['frozen'], 3),
                         'stage_kernels_ms_per_batch_step_by_the_library_profiler': {k: round(v, 4) for k, v in sorted(per_step.items())},
                         'bn_kernels_share_of_the_batch_step': round(sum(v for k, v in per_step.items() if k.startswith('bn_')) / med['batch'], 4),
                         'conv_bwd_prep_share_of_the_batch_step': round(per_step.get('conv_bwd_prep', 0.0) / med['batch'], 4)}
    print(json.dumps(out['whole_step'], indent=1))
    return out


def trunk_train_section(a):
    """What the trainable trunk adds below layer4 (spec_amd/csrc/pool_bwd.hip, the 7x7 shape and the split weight gradient of
    spec_amd/csrc/conv_bwd.hip) at CamCalib's fine-tuning shape, B = ``DATASET.BATCH_SIZE`` = 64 frames of 600 x 1000: the max-pool
    forward + backward against ``aten.max_pool2d_with_indices`` and its backward on the same channels_last tensors, with the bytes
    the kernels must move over their time; the stem's three products and one 1x1 and one 3x3 of each of layer1 - layer3 (forward and
    weight gradient, with the rule's S) against ``aten.convolution`` / ``aten.convolution_backward``; library and torch alternated in
    this process, 3 rounds of ``iters`` back-to-back calls after a warm-up, medians; the weight gradients of the stem, layer1 and
    layer2 at every candidate S (the experimental option "conv_wgrad_splits" forces it; S = 1 is the unsplit launch), alternated
    over 3 rounds; and the whole training step at SPEC's shape (B = 64, 224 x 224) too - with the heads alone, with layer4 and with
    the whole trunk unfrozen, frozen and batch BatchNorm, each with ``torch.cuda.max_memory_allocated``."""
    from spec_amd import camcalib_eval as ce
    from spec_amd.cam_utils import _engine
    dev = torch.device('cuda', 0)
    eng = _engine(dev)
    bs = int(ce.DEFAULTS['DATASET']['BATCH_SIZE'])

    def ms_per_call(fn, iters):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def compare(calls, iters):
        rounds = {p: {'library': [], 'torch': []} for p in calls}
        for _ in range(3):                                              # alternated: both see the same clocks and the same neighbours
            for p, (mine, theirs) in calls.items():
                rounds[p]['library'].append(ms_per_call(mine, iters))
                rounds[p]['torch'].append(ms_per_call(theirs, iters))
        row = {}
        for p in calls:
            lib, tor = float(np.median(rounds[p]['library'])), float(np.median(rounds[p]['torch']))
            row[p] = {'library_ms': round(lib, 5), 'torch_ms': round(tor, 5), 'library_over_torch': round(lib / tor, 3),
                      'library_rounds_ms': [round(v, 5) for v in rounds[p]['library']], 'torch_rounds_ms': [round(v, 5) for v in rounds[p]['torch']]}
        return row
    out = {}
    # the pool at the stem's output: B x 300 x 500 x 64 -> 150 x 250
    torch.manual_seed(5)
    x = torch.relu(torch.randn(bs, 300, 500, 64, device=dev))
    y, idx = eng.maxpool_train_forward(x)
    g_y = torch.randn_like(y)
    xn, gn = x.permute(0, 3, 1, 2), g_y.permute(0, 3, 1, 2)                 # channels_last views of the same memory
    ty, ti = torch.ops.aten.max_pool2d_with_indices(xn, [3, 3], [2, 2], [1, 1])
    row = compare({'forward': (lambda: eng.maxpool_train_forward(x), lambda: torch.ops.aten.max_pool2d_with_indices(xn, [3, 3], [2, 2], [1, 1])),
                   'backward': (lambda: eng.maxpool_backward(g_y, idx, 300, 500),
                                lambda: torch.ops.aten.max_pool2d_with_indices_backward(gn, xn, [3, 3], [2, 2], [1, 1], [1, 1], False, ti))}, a.iters)
    moved = {'forward': 4.0 * x.numel() + 5.0 * y.numel(), 'backward': 4.0 * x.numel() + 5.0 * y.numel()}
    for p, by in moved.items():
        row[p]['bytes_moved'] = by
        row[p]['TBps'] = round(by / (row[p]['library_ms'] * 1e-3) / 1e12, 3)
        row[p]['fraction_of_hbm_peak'] = round(row[p]['TBps'] * 1e12 / HBM_PEAK, 3)
    row['workload'] = f'B = {bs}, 300 x 500 x 64 -> 150 x 250, post-ReLU input'
    out['maxpool'] = row
    print('maxpool', {p: (row[p]['library_ms'], row[p]['torch_ms']) for p in moved}, flush=True)
    del x, y, idx, g_y, xn, gn, ty, ti
    # the conv products: (name, H, W, Cin, Cout, k, stride, products)
    fw = ('forward', 'wgrad')
    layers = [(f'{sname}.{lname}', H0 // d, W0 // d, cin, cout, k, stride, products)
              for sname, (H0, W0) in {'camcalib_b%d_600x1000' % bs: (600, 1000), 'spec_b64_224x224': (224, 224)}.items()
              for lname, d, cin, cout, k, stride, products in [
                  ('stem.conv1', 1, 3, 64, 7, 2, fw + ('dgrad',)), ('layer1.0.conv1', 4, 64, 64, 1, 1, fw), ('layer1.0.conv2', 4, 64, 64, 3, 1, fw),
                  ('layer2.0.conv1', 4, 256, 128, 1, 1, fw), ('layer2.0.conv2', 4, 128, 128, 3, 2, fw),
                  ('layer3.0.conv1', 8, 512, 256, 1, 1, fw), ('layer3.0.conv2', 8, 256, 256, 3, 2, fw)]]
    for lname, H, W, cin, cout, k, stride, products in layers:
        pad = k // 2
        torch.manual_seed(cin + cout + k + stride)
        x = torch.randn(bs, H, W, cin, device=dev)
        wt = torch.randn(cout, cin, k, k, device=dev) / float(np.sqrt(cin * k * k))
        scale, shift = 0.5 + torch.rand(cout, device=dev), 0.3 * torch.randn(cout, device=dev)
        y = eng.conv2d_train_forward(x, wt, scale, shift, stride, pad, None, True)
        g_y = torch.randn_like(y)
        xn, gn = x.permute(0, 3, 1, 2), g_y.permute(0, 3, 1, 2)
        bwd = lambda mask: (lambda: torch.ops.aten.convolution_backward(gn, xn, wt, None, [stride] * 2, [pad] * 2, [1, 1], False, [0, 0], 1, mask))
        lib_bwd = lambda want: (lambda: eng.conv2d_backward(x, wt, scale, stride, pad, y, g_y, True, None, want))
        calls = {'forward': (lambda: eng.conv2d_train_forward(x, wt, scale, shift, stride, pad, None, True),
                             lambda: torch.ops.aten.convolution(xn, wt, None, [stride] * 2, [pad] * 2, [1, 1], False, [0, 0], 1)),
                 'wgrad': (lib_bwd((False, True, False)), bwd([False, True, False])),
                 'dgrad': (lib_bwd((True, False, False)), bwd([True, False, False]))}
        row = compare({p: calls[p] for p in products}, max(1, a.iters // 4) if 'dgrad' in products else a.iters)
        kern = timed(eng, calls['wgrad'][0], max(1, a.iters // 4))
        row['wgrad_splits'] = eng.conv2d_wgrad_splits(bs, H, W, cin, cout, k, stride, pad)
        if 'layer3' not in lname:
            # the candidates: every S forced in turn (0 = the rule), wgrad product + reduce by HIP events around the call
            cand = sorted({1, 4, 16, 32, 64, 128, 256, 512, 1024, row['wgrad_splits']})
            eng.set_option('experimental', 1)
            sweep = {S: [] for S in cand}
            for _ in range(3):
                for S in cand:
                    eng.set_option('conv_wgrad_splits', S)
                    sweep[S].append(ms_per_call(calls['wgrad'][0], max(2, a.iters // 2)))
            eng.set_option('conv_wgrad_splits', 0)
            prep = kern.get('conv_bwd_prep', (0.0,))[0]
            row['wgrad_ms_by_forced_splits'] = {str(S): {'median_ms': round(float(np.median(v)), 5), 'rounds_ms': [round(x, 5) for x in v]} for S, v in sweep.items()}
            row['wgrad_prep_ms_inside_every_figure'] = round(prep, 5)
            best = min(cand, key=lambda S: float(np.median(sweep[S])))
            row['wgrad_best_S'], row['wgrad_rule_over_best'] = best, round(float(np.median(sweep[row['wgrad_splits']])) / float(np.median(sweep[best])), 3)
            row['wgrad_rule_over_unsplit'] = round(float(np.median(sweep[row['wgrad_splits']])) / float(np.median(sweep[1])), 4)
            print(lname, 'forced S:', {S: round(float(np.median(v)), 3) for S, v in sweep.items()}, flush=True)
        row['wgrad_kernels_by_the_library_profiler'] = {kk: round(v[0], 5) for kk, v in kern.items()}
        row['workload'] = f'B = {bs}, {H} x {W} x {cin} -> {cout}, {k}x{k} stride {stride}, relu'
        out[lname] = row
        print(lname, 'S =', row['wgrad_splits'], {p: (row[p]['library_ms'], row[p]['torch_ms']) for p in products}, flush=True)
        del x, wt, y, g_y, xn, gn
    # the whole step: what lies below runs under no_grad, then the trainable part -> heads -> loss -> backward -> Adam
    from spec_amd import synth
    from spec_amd.camcalib_train import trunk_features
    from spec_amd.differentiable import CameraRegressorHead, ResNetStage, ResNetTrunk
    from spec_amd.losses import CameraRegressorLoss
    from spec_amd.modules import CameraRegressorNetwork
    net = CameraRegressorNetwork()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.camcalib_state(1001).items()}, strict=False)
    net = net.to(dev).eval()
    net.set_plan('throughput')
    net.commit(dev, freeze=True)
    head, crit = CameraRegressorHead.from_model(net), CameraRegressorLoss(1.0, 1.0, 1.0, 'ce')
    for sname, (H, W) in {'camcalib_b%d_600x1000' % bs: (600, 1000), 'spec_b64_224x224': (224, 224)}.items():
        images = torch.randn(bs, 3, H, W, device=dev)
        targets = [torch.randint(0, 256, (bs,), device=dev) for _ in range(3)]
        for what, bn in (('head_only', 'frozen'), ('layer4', 'frozen'), ('layer4', 'batch'), ('all', 'frozen'), ('all', 'batch')):
            part = None if what == 'head_only' else ResNetStage.from_model(net, 'layer4', bn) if what == 'layer4' else ResNetTrunk.from_model(net, 'stem', bn)
            mods = [] if part is None else [part.blocks] if what == 'layer4' else part.trained_modules()
            params = list(head.parameters()) + ([] if part is None else part.conv_parameters() + (part.bn_parameters() if bn == 'batch' else []))
            optim = torch.optim.Adam(params, lr=1e-6)
            for m in mods:
                m.train(bn == 'batch')

            def step():
                feat = None if what == 'all' else trunk_features(net, images, stages=3 if what == 'layer4' else None)
                with torch.enable_grad():
                    feat = part(images) if what == 'all' else part(feat) if part is not None else feat
                    loss, _ = crit(*head(feat, channels_last=True), *targets)
                    optim.zero_grad(set_to_none=True)
                    loss.backward()
                optim.step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ms = ms_per_call(step, 2)
            key = f'whole_step.{sname}.{what}.{bn}'
            out[key] = {'ms_per_step': round(ms, 2), 'max_memory_allocated_GiB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                        'workload': f'ResNet-50, B = {bs} frames of {H} x {W}, ce, Adam; 2 warm-up steps, 2 timed'}
            print(key, out[key]['ms_per_step'], 'ms,', out[key]['max_memory_allocated_GiB'], 'GiB', flush=True)
            for m in mods:
                m.eval()
            del optim, part
        del images
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['eval_step', 'hmr_loss', 'camcalib_eval', 'pano_views', 'pano_views_host', 'ragged_crops', 'render', 'render_batch', 'draw', 'jpeg_encode', 'png_encode', 'jpeg_decode', 'png_decode', 'horizon_panel', 'color_jitter', 'smpl_backward', 'head_train', 'camcalib_train', 'conv_backward', 'bn_train', 'trunk_train'], default=None, help='run one section only')
    ap.add_argument('--smpl-backward', dest='only', action='store_const', const='smpl_backward', help='the same as --only smpl_backward')
    ap.add_argument('--head-train', dest='only', action='store_const', const='head_train', help='the same as --only head_train')
    ap.add_argument('--camcalib-train', dest='only', action='store_const', const='camcalib_train', help='the same as --only camcalib_train')
    ap.add_argument('--conv-backward', dest='only', action='store_const', const='conv_backward',
                    help='the same as --only conv_backward (writes profiles/conv_backward_aux.json unless --out is given)')
    ap.add_argument('--bn-train', dest='only', action='store_const', const='bn_train',
                    help='the same as --only bn_train (writes profiles/bn_train_aux.json unless --out is given)')
    ap.add_argument('--trunk-train', dest='only', action='store_const', const='trunk_train',
                    help='the same as --only trunk_train (writes profiles/trunk_train_aux.json unless --out is given)')
    ap.add_argument('--reference', default=None, help='the reference checkout (--only pano_views_host)')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--out', default='gpurun_out/aux_bench.json')
    a = ap.parse_args()
    if a.only == 'pano_views_host':
        return pano_views_host(a)
    from spec_amd import assets, preprocess, metrics
    from spec_amd.cam_utils import _engine
    assets.use_synthetic_assets(1003)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    eng = _engine(dev)
    g = torch.Generator().manual_seed(0)
    B = a.batch
    table = []

    if a.only == 'smpl_backward':
        from spec_amd import _lib
        row = smpl_backward_section(a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the same calls; 3 alternated rounds; '
                       'kernels: per-launch HIP events (library profiler)', 'smpl_backward': row, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'head_train':
        from spec_amd import _lib
        row = head_train_section(a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the same calls; 3 alternated rounds; '
                       'kernels: per-launch HIP events (library profiler)', 'head_train': row, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'camcalib_train':
        from spec_amd import _lib
        row = camcalib_train_section(a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the same calls; 3 alternated rounds; '
                       'kernels: per-launch HIP events (library profiler)', 'camcalib_train': row, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'conv_backward':
        from spec_amd import _lib
        row = conv_backward_section(a)
        path = a.out if a.out != ap.get_default('out') else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                                         'conv_backward_aux.json')
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the same calls; library and torch '
                       'alternated, 3 rounds, medians; kernels: per-launch HIP events (library profiler)', 'conv_backward': row,
                       'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'bn_train':
        from spec_amd import _lib
        row = bn_train_section(a)
        path = a.out if a.out != ap.get_default('out') else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                                         'bn_train_aux.json')
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the '
                       'same calls; library and torch alternated, 3 rounds, medians; kernels: per-launch HIP events (library profiler), bytes = what '
                       'the kernel must move, computed from the shape', 'bn_train': row, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'trunk_train':
        from spec_amd import _lib
        row = trunk_train_section(a)
        path = a.out if a.out != ap.get_default('out') else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                                         'trunk_train_aux.json')
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the '
                       'same calls; library and torch alternated, 3 rounds, medians; the stem row, which includes the data gradient, runs iters / 4 calls',
                       'wgrad_split_rule': 'the S that specmi_conv2d_wgrad_splits returns is wgrad_splits in every row; the candidates were forced through the '
                       'experimental option conv_wgrad_splits', 'trunk_train': row, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    def add(name, workload, res, per_unit=None):
        for k, (ms, by, fl, n) in res.items():
            row = {'call': name, 'kernel': k, 'workload': workload, 'launches_per_call': n, 'ms_per_launch': round(ms, 5),
                   'algorithmic_MB': round(by / 1e6, 3), 'achieved_GBps': round(by / (ms * 1e-3) / 1e9, 1),
                   'frac_of_hbm_peak': round(by / (ms * 1e-3) / HBM_PEAK, 4)}
            if fl:
                row['TFLOPs'] = round(fl / (ms * 1e-3) / 1e12, 2)
            if per_unit:
                row[per_unit[0]] = round(per_unit[1] / (ms * 1e-3), 1)
            table.append(row)

    if a.only == 'eval_step':
        from spec_amd import _lib
        row = eval_step_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the '
                       'same calls; 3 alternated rounds; kernels: per-launch HIP events (library profiler)', 'eval_step': row,
                       'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'hmr_loss':
        from spec_amd import _lib
        hmr_loss_section(eng, a, add)
        return finish(a, table, {'source_hash': _lib.source_hash()})

    if a.only == 'camcalib_eval':
        from spec_amd import _lib
        cmp_ = camcalib_eval_section(eng, a, add, g)
        return finish(a, table, {'pad_batch_vs_per_frame_composition': cmp_, 'source_hash': _lib.source_hash()})

    if a.only == 'pano_views':
        from spec_amd import _lib
        row = pano_views_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'per-launch HIP events (library profiler); wall clock where named',
                       'pano_views': row, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'render':
        from spec_amd import _lib
        row = render_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'per-launch HIP events (library profiler)', 'render': row,
                       'source_hash': _lib.source_hash()}, f, indent=1)
        print(json.dumps(row))
        return

    if a.only == 'render_batch':
        from spec_amd import _lib
        rows = render_batch_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'device_resident: HIP events around the whole sequence; host_frames_to_host_pictures: wall clock '
                       'with the copies; 3 alternated rounds each', 'render_batch': rows, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'draw':
        from spec_amd import _lib
        rows = draw_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'HIP events around `iters` back-to-back calls after a warm-up of the same calls; 3 alternated rounds',
                       'draw': rows, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'jpeg_encode':
        from spec_amd import _lib
        rows = jpeg_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'routes: wall clock with the copies, 3 alternated rounds, ms per '
                       'picture; kernels: per-launch HIP events (library profiler)', 'jpeg_encode': rows, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'png_encode':
        from spec_amd import _lib
        rows = png_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'routes: wall clock with the copies, 3 alternated rounds, ms per picture; kernels: per-launch HIP '
                       'events (library profiler)', 'png_encode': rows, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'jpeg_decode':
        from spec_amd import _lib
        rows = jpeg_decode_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'timing': 'wall clock from the files on disk to the frame slab on the device, one warm-up then 3 alternated rounds, ms per '
                       '64-frame batch', 'jpeg_decode': rows, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'png_decode':
        from spec_amd import _lib
        rows = png_decode_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'timing': 'wall clock from the files on disk to the frame slab on the device, one warm-up then 3 alternated rounds, ms per '
                       'batch; stage_ms: per-launch HIP events (library profiler)', 'png_decode': rows, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'color_jitter':
        from spec_amd import _lib
        rows = color_jitter_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'launches: per-launch HIP events (library profiler) after a warm-up, the '
                       'device-to-device copy of the same slab by events in the same process, 3 alternated rounds; routes: wall clock from host '
                       'frames to the jittered slab on the device, 3 alternated rounds, ms per 64-frame batch', 'color_jitter': rows,
                       'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'horizon_panel':
        from spec_amd import _lib
        row = horizon_panel_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'iters': a.iters, 'timing': 'routes: wall clock from host frames to the finished slab on the device, 3 alternated rounds, ms per '
                       'flush; kernels: per-launch HIP events (library profiler)', 'horizon_panel': row, 'source_hash': _lib.source_hash()}, f, indent=1)
        return

    if a.only == 'ragged_crops':
        from spec_amd import _lib
        rows = ragged_crops_section(eng, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'hbm_peak_TBps': HBM_PEAK / 1e12, 'iters': a.iters, 'timing': 'wall clock, host frames -> crops on the device, 3 alternated '
                       'rounds; ragged_launch: per-launch HIP events (library profiler)', 'ragged_crops': rows, 'source_hash': _lib.source_hash()},
                      f, indent=1)
        return

    # ---- 8f-1: crops from one 1080p frame ---------------------------------------------------------------------------
    frame = torch.randint(0, 256, (1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    cx = torch.rand(B, generator=g) * 1920; cy = torch.rand(B, generator=g) * 1080
    wh = 150 + torch.rand(B, 2, generator=g) * 500
    dets = torch.stack([cx, cy, wh[:, 0], wh[:, 1]], 1)
    add('preprocess.crop_detections', f'{B} person boxes of one 1920x1080 uint8 frame -> ({B},3,224,224) fp32',
        timed(eng, lambda: preprocess.crop_detections(frame, dets), a.iters), ('crops_per_s', B))
    centers = torch.stack([cx, cy], 1).numpy(); scales = (wh.max(1).values / 200).numpy()
    boxes = torch.from_numpy(preprocess.pare_crop_boxes(centers, scales, 224)).to(dev)
    out = torch.empty(B, 3, 224, 224, device=dev)
    from spec_amd import _lib
    from spec_amd.engine import _ptr

    def ds():
        _lib.check(eng.h, eng.lib.specmi_crop_resize_normalize(eng.h, _ptr(frame), 1080, 1920, _ptr(boxes), B, 224, _ptr(out),
                                                               eng._stream()))
    add('preprocess.dataset_crops (kernel only, boxes precomputed)', f'{B} pare crop boxes of one 1920x1080 frame -> ({B},3,224,224) fp32',
        timed(eng, ds, a.iters), ('crops_per_s', B))
    add('preprocess.camcalib_transform', '1920x1080 uint8 frame -> Resize(600) antialiased -> (1,3,600,1066) fp32',
        timed(eng, lambda: preprocess.camcalib_transform(frame), a.iters), ('frames_per_s', 1))
    big = torch.randint(0, 256, (2160, 3840, 3), generator=g, dtype=torch.uint8).to(dev)
    add('preprocess.camcalib_transform', '3840x2160 uint8 frame -> Resize(600) antialiased -> (1,3,600,1066) fp32',
        timed(eng, lambda: preprocess.camcalib_transform(big), a.iters), ('frames_per_s', 1))

    # ---- 8f-2: evaluation metrics -----------------------------------------------------------------------------------
    V = 6890
    pv = torch.randn(B, V, 3, generator=g).to(dev); gv = (pv.cpu() + 0.01 * torch.randn(B, V, 3, generator=g)).to(dev)
    sm = assets.smpl_model()
    Jh = torch.from_numpy(np.ascontiguousarray(sm['J_regressor_extra'])).float()
    J17 = torch.cat([Jh, Jh[:8]], 0).to(dev)                      # 17 x 6890 stand-in with the H36M regressor's shape
    J24 = torch.from_numpy(np.ascontiguousarray(sm['J_regressor'])).float().to(dev)
    add('metrics.eval_single', f'MPJPE / PA-MPJPE / V2V of {B} meshes (6890 verts, 17x6890 regressor, 14 joints)',
        timed(eng, lambda: metrics.eval_single(pv, gv, J17), a.iters), ('meshes_per_s', B))
    pj = torch.randn(B, 24, 3, generator=g).to(dev); gj = torch.randn(B, 24, 3, generator=g).to(dev)
    add('metrics.eval_j_24', f'MPJPE / PA-MPJPE of {B} x 24 joints', timed(eng, lambda: metrics.eval_j_24(pj, gj), a.iters),
        ('poses_per_s', B))
    add('metrics.regress_joints', f'24x6890 regressor on {B} meshes', timed(eng, lambda: metrics.regress_joints(pv, J24), a.iters),
        ('meshes_per_s', B))
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0].to(dev)
    add('metrics.rotate_points', f'{B} meshes x 6890 points by a per-mesh 3x3', timed(eng, lambda: metrics.rotate_points(R, pv), a.iters),
        ('meshes_per_s', B))

    # ---- C5 helper: the body model alone -----------------------------------------------------------------------------
    bm = metrics.BodyModel(device=dev)
    pose = (0.3 * torch.randn(B, 72, generator=g)).to(dev); betas = torch.randn(B, 10, generator=g).to(dev)
    add('BodyModel.native', f'SMPL (Rodrigues + blend shapes + LBS) for {B} bodies -> vertices + 24 joints',
        timed(bm.engine, lambda: bm.native(pose, betas), a.iters), ('bodies_per_s', B))

    # ---- CamCalib bin reductions ----------------------------------------------------------------------------------
    logits = torch.randn(3 * B, 256, generator=g).to(dev)
    add('cam_utils bins (arg-max + soft-argmax)', f'{3 * B} rows x 256 bins',
        timed(eng, lambda: eng.camcalib_bins(logits, argmax=True, soft=True), a.iters), ('rows_per_s', 3 * B))

    hmr_loss_section(eng, a, add)
    cmp_ = camcalib_eval_section(eng, a, add, g)
    finish(a, table, {'pad_batch_vs_per_frame_composition': cmp_})


if __name__ == '__main__':
    main()
