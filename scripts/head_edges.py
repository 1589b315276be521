"""Measure what tests/test_gpu_head_edges.py asserts and write it down: the worst figures of the regressor heads and the camera
decode against the float64 yardstick tests/head_ref.py, each next to the budget it is held to.  Needs the GPU.

    python scripts/head_edges.py --out profiles/head_edges.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/head_edges.json')
    args = ap.parse_args()
    import torch
    from spec_amd.engine import Engine
    from tests import head_ref as H
    from tests import test_gpu_head_edges as T
    eng = Engine('camcalib', torch.device(T.DEV)).experimental(True)
    rounding = []
    for K, N, B in H.ROUNDING_CASES:
        for path in (0, 1):
            reached, c = T.rounding_report(eng, K, N, B, path)
            rounding.append({'K': K, 'N': N, 'B': B, 'path': 'gemv' if path == 0 else 'matrix cores', 'c_reached': reached, 'c_bound': c})
    doc = {
        'what': 'worst figures of tests/test_gpu_head_edges.py on an MI355X; a ratio is |gpu - float64| over its budget (<= 1 passes)',
        'linear_rounding': {'unit': '|gpu - f64| / (2^-24 (sum |w||x| + |b| + |res|)), worst output', 'cases': rounding},
        'rot6d_random_joints': {'unit': 'ulp32 of float64 per element, worst', 'worst': T.rot6d_report(), 'budget': 4.0},
        'activations': {'unit': '|gpu - f64| / (2 |fp32 torch - f64| + 4 ulp32(f64)) per element, worst (0 = exact)',
                        'doubled decoders': T.activation_report('var'), 'separate variance layers': T.activation_report('var_separate')},
        'head_init_vfov_slot': {'unit': 'ulp32 of float64, worst', 'worst': T.head_init_report(), 'budget': 4.0},
        'camcalib_decode': {'unit': 'max |gpu - f64| / (2 max |fp32 oracle - f64| + 4 ulp32(max |f64|)) per quantity; _1e4 = the row spanning +-1e4',
                            'nbins': {str(n): T.decode_report(eng, n) for n in H.NBINS}},
        'cam_params_R': {'unit': 'the same ratio', 'B': {str(B): T.cam_params_report(eng, B) for B in H.CAM_PARAMS_B}},
    }
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({'out': args.out, 'worst_rot6d_ulp': doc['rot6d_random_joints']['worst'],
                      'worst_decode_ratio': max(max(r.values()) for r in doc['camcalib_decode']['nbins'].values())}))


if __name__ == '__main__':
    main()
