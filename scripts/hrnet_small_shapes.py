"""Measure what tests/test_gpu_hrnet.py::test_hrnet_small_and_non_square_inputs_per_concat_slice asserts and write it down: the
HRNet trunks at their smallest and at non-square inputs, every slice of the concat head against the float64 oracle, next to the
oracle's own fp32 error in two summation orders.  Needs the GPU.

    python scripts/hrnet_small_shapes.py --out profiles/hrnet_small_shapes.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/hrnet_small_shapes.json')
    args = ap.parse_args()
    from tests import test_gpu_hrnet as T
    cases, worst = [], 0.0
    for backbone in T.BACKBONES:
        for B, H, W in T.SMALL_SHAPES:
            rows = T.small_shape_report(backbone, B, H, W)
            for r in rows:
                r['rel_gpu'], r['rel_cpu'] = r['e_gpu'] / r['max'], r['e_cpu'] / r['max']
                r['gpu_over_cpu'] = r['e_gpu'] / r['e_cpu'] if r['e_cpu'] > 0 else None
                worst = max(worst, r['gpu_over_cpu'] or 0.0)
            cases.append({'backbone': backbone, 'B': B, 'H': H, 'W': W, 'slices': rows})
    doc = {'what': 'max |x - float64 oracle| per concat slice: x = the GPU trunk (e_gpu), the fp32 oracle NCHW on all threads / '
                   'channels_last on one thread (e_cpu = the larger); bound = max(factor * e_cpu, floor * slice maximum)',
           'images': 'synth.images(61, B) cut to H x W, weights synth.hmr_state(1202, True, backbone)',
           'factor': T._slice_factor(), 'floor': T.SLICE_FLOOR, 'worst_gpu_over_cpu': worst, 'cases': cases}
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({'out': args.out, 'cases': len(cases), 'worst_gpu_over_cpu': worst}))


if __name__ == '__main__':
    main()
