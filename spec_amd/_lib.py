"""ctypes binding of libspecmi.so (the C ABI in include/specmi.h).

There is NO CPU fallback: if the library is missing or cannot be loaded, importing the ops
raises, and every forward requires device tensors.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SPECMI_LIB') or os.path.join(_HERE, 'lib', 'libspecmi.so')   # SPECMI_LIB: an alternative build (A/B runs)



def source_hash() -> str:
    """sha256 (16 hex digits) over the kernel sources the library is built from (spec_amd/csrc/*, include/specmi.h) - the
    stamp measured artefacts carry (profiles/pmc_traffic_latest.json), so that a number measured on other kernels is
    recognisable as stale.  Sources, not the binary: a rebuild on another box must not change it."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, 'csrc')
    for name in sorted(os.listdir(csrc)):
        if name.endswith(('.hip', '.h', '.inc')):
            with open(os.path.join(csrc, name), 'rb') as f:
                h.update(name.encode() + b'\0' + f.read())
    with open(os.path.join(os.path.dirname(_HERE), 'include', 'specmi.h'), 'rb') as f:
        h.update(b'specmi.h\0' + f.read())
    return h.hexdigest()[:16]


OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_MISSING = 0, 1, 2, 3, 4
PRECISION_FP32, PRECISION_FP16 = 0, 1       # SPECMI_PRECISION_* (include/specmi.h)
MODEL_CAMCALIB, MODEL_HMR, MODEL_SMPL = 0, 1, 2
RENDER_SIDE_VIEW, RENDER_GROUND_PLANE, RENDER_CULL, RENDER_THREAD_PER_TRIANGLE = 1, 2, 4, 8     # SPECMI_RENDER_* (include/specmi.h)
DRAW_MAX_SIDE, DRAW_MAX_COORD, DRAW_MAX_RADIUS, DRAW_MAX_THICKNESS = 8192, 16383, 64, 64      # the limits of specmi_draw_skeletons (include/specmi.h)
MARK_STRIP, MARK_MASK, MARK_LINE, MARK_REC = 0, 1, 2, 8         # SPECMI_MARK_* and the int64 per mark record (include/specmi.h)
# the limits of specmi_draw_marks: frame side, line width, line end point, mask side, mask position (include/specmi.h)
MARK_MAX_SIDE, MARK_MIN_WIDTH, MARK_MAX_WIDTH, MARK_MAX_COORD, MARK_MAX_MASK_SIDE, MARK_MAX_MASK_POS = 8192, 2, 64, 100000, 8192, 16383
# SPECMI_JITTER_* (the operation ids of specmi_color_jitter), the int32 words of its record and its largest frame side (include/specmi.h)
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE, JITTER_REC, JITTER_MAX_SIDE = 0, 1, 2, 3, 8, 8192
JPEG_HEADER_BYTES = 623                       # what specmi_jpeg_header writes; the least capacity of specmi_jpeg_encode (include/specmi.h)
PNG_OVERHEAD_BYTES, PNG_HEADER_BYTES = 63, 33   # the least capacity of specmi_png_encode; what specmi_png_header writes (include/specmi.h)
# SPECMI_JPEG_* (include/specmi.h): what specmi_jpeg_probe answers, by value
JPEG_REASONS = ('supported', 'not_jpeg', 'truncated', 'progressive', 'sof', 'precision', 'components', 'sampling', 'restart', 'scan',
                'colourspace', 'tables', 'size', 'trailing')
# SPECMI_PNG_* (include/specmi.h): what specmi_png_probe answers, by value
PNG_REASONS = ('supported', 'not_png', 'truncated', 'crc', 'depth', 'palette', 'interlaced', 'animated', 'chunk', 'size', 'trailing')
# the inflate stage of specmi_png_decode: lanes of a workgroup = subsequences of a window, bits of the zlib stream per subsequence
# (SPECMI_PNG_LANES, SPECMI_PNG_SUB_BITS); tests size their streams from them
PNG_DECODE_LANES, PNG_DECODE_SUB_BITS = 256, 512
# the status bits of specmi_png_decode (include/specmi.h), by bit number
PNG_STATUS_BITS = ('zlib', 'btype', 'stored', 'lens', 'repeat', 'noeob', 'code', 'symbol', 'far', 'early', 'length', 'leftover', 'adler',
                   'filter')
HMR_LOSS, HMR_CAM_LOSS = 0, 1                 # SPECMI_HMR_LOSS / SPECMI_HMR_CAM_LOSS (include/specmi.h)
# the ground-truth tensors of specmi_hmr_loss in the order of its prototype, per-image shapes (None = (V, 3)); int32 where named has_*
HMR_LOSS_GT = (('pose', (72,)), ('betas', (10,)), ('pose_conf', (24,)), ('pose_3d', (24, 4)), ('keypoints', (49, 3)), ('vertices', None),
               ('has_smpl', ()), ('has_pose_3d', ()), ('orig_shape', (2,)), ('scale', ()))
BN_ROWS_PER_CHUNK = 64                        # SPECMI_BN_ROWS_PER_CHUNK: the rows of a chunk of the BatchNorm reductions (include/specmi.h)
LOSS_TYPES = {'ce': 0, 'kl': 1, 'softargmax_l2': 2, 'softargmax_biased_l2': 3}     # SPECMI_LOSS_* (include/specmi.h)

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_double_p = C.POINTER(C.c_double)


class HmrOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        'smpl_vertices', 'smpl_joints3d', 'smpl_joints2d', 'pred_cam_t', 'pred_pose', 'pred_cam',
        'pred_shape', 'pred_pose_6d')]


HMR_HEAD_PARAMS = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'decpose.weight', 'decpose.bias', 'decshape.weight',
                   'decshape.bias', 'deccam.weight', 'deccam.bias')     # the members of the two structs below, in order


class HmrHeadParams(C.Structure):
    """``specmi_hmr_head_params`` and ``specmi_hmr_head_grads`` (include/specmi.h): ten device pointers under the state_dict names."""
    _fields_ = [(n.replace('.', '_'), C.c_void_p) for n in HMR_HEAD_PARAMS]


CAMCALIB_HEADS = ('fc_vfov', 'fc_pitch', 'fc_roll')     # the head index of the two structs below, in order
CAMCALIB_HEAD_MAX_LAYERS = 3


class CamcalibHeadParams(C.Structure):
    """``specmi_camcalib_head_params`` and ``specmi_camcalib_head_grads`` (include/specmi.h): device pointers [head][layer]."""
    _fields_ = [('weight', (C.c_void_p * 3) * 3), ('bias', (C.c_void_p * 3) * 3)]


class ProfEntry(C.Structure):
    _fields_ = [('kernel', C.c_char * 48), ('label', C.c_char * 48), ('ms', C.c_double),
                ('flops', C.c_double), ('bytes', C.c_double), ('launches', C.c_int)]


class DrawStyle(C.Structure):
    """``specmi_draw_style`` (include/specmi.h); the defaults are the header's."""
    _fields_ = [('radius', C.c_int32), ('thickness', C.c_int32), ('conf_thr', C.c_float), ('joint_rgb', C.c_uint8 * 3),
                ('bone_rgb', (C.c_uint8 * 3) * 2)]

    def __init__(self, radius=4, thickness=2, conf_thr=0.3, joint_rgb=(0, 255, 0), bone_rgb=((0, 0, 255), (255, 0, 0))):
        super().__init__(int(radius), int(thickness), float(conf_thr), (C.c_uint8 * 3)(*joint_rgb),
                         ((C.c_uint8 * 3) * 2)(*[(C.c_uint8 * 3)(*c) for c in bone_rgb]))


class SpecmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'libspecmi error {code}: {msg}')
        self.code = code


# every exported symbol of include/specmi.h with its prototype
PROTOTYPES = {
    'specmi_create': (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    'specmi_destroy': (C.c_int, [C.c_void_p]),
    'specmi_last_error': (C.c_char_p, [C.c_void_p]),
    'specmi_version': (C.c_char_p, []),
    'specmi_set_option_i32': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    'specmi_set_option_f32': (C.c_int, [C.c_void_p, C.c_char_p, C.c_float]),
    'specmi_get_option_i32': (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    'specmi_option_info': (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'specmi_set_tensor_f32': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int64_p, C.c_int]),
    'specmi_set_tensor_i32': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int64_p, C.c_int]),
    'specmi_commit': (C.c_int, [C.c_void_p]),
    'specmi_camcalib_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_camcalib_head_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    'specmi_camcalib_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_camcalib_bins': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_cam_params': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_hmr_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(HmrOutputs), C.c_void_p]),
    'specmi_hmr_regress': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(HmrOutputs), C.c_void_p]),
    'specmi_hmr_uncertainty': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_trunk_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    'specmi_hmr_head_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_smpl_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    'specmi_smpl_native': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    # (h, rotmat, betas, cam, B, 6 camera arguments, 4 upstream gradients, g_rotmat, g_betas, g_cam, stream)
    'specmi_smpl_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_void_p] * 4 +
                             [C.c_void_p] * 3 + [C.c_void_p]),
    'specmi_rot6d_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'specmi_rot6d_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'specmi_hmr_head_tape_floats': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p]),
    # (h, params, xf, ld_xf, cam_feats, init_state, masks, p, B, F, C, n_iter, state, tape, stream)
    'specmi_hmr_head_train_forward': (C.c_int, [C.c_void_p, C.POINTER(HmrHeadParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (h, params, xf, ld_xf, cam_feats, masks, p, B, F, C, n_iter, tape, g_state, g_xf, grads, stream)
    'specmi_hmr_head_backward': (C.c_int, [C.c_void_p, C.POINTER(HmrHeadParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(HmrHeadParams),
                                           C.c_void_p]),
    # (h, 3 logit tensors, B, nbins, loss_type, 3 targets, 3 weights, loss_term, means, stream)
    'specmi_camcalib_loss': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_float] * 3 + [C.c_void_p] * 3),
    # (h, 3 logit tensors, B, nbins, loss_type, 3 targets, 3 weights, g_means, 3 gradients, stream)
    'specmi_camcalib_loss_backward': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_float] * 3 + [C.c_void_p] * 5),
    'specmi_camcalib_head_tape_floats': (C.c_int, [C.c_int] * 5 + [c_int64_p]),
    # (h, params, xf, ld_xf, B, F, L, Hc, nbins, tape, logits, stream)
    'specmi_camcalib_head_train_forward': (C.c_int, [C.c_void_p, C.POINTER(CamcalibHeadParams), C.c_void_p, C.c_int64] + [C.c_int] * 5 +
                                           [C.c_void_p] * 3),
    # (h, params, xf, ld_xf, B, F, L, Hc, nbins, tape, g_logits, g_xf, grads, stream)
    'specmi_camcalib_head_backward': (C.c_int, [C.c_void_p, C.POINTER(CamcalibHeadParams), C.c_void_p, C.c_int64] + [C.c_int] * 5 +
                                      [C.c_void_p] * 3 + [C.POINTER(CamcalibHeadParams), C.c_void_p]),
    # (h, x, B, H, W, Cin, w, scale, shift, Cout, KH, KW, stride, pad, residual, relu, y, stream)
    'specmi_conv2d_train_forward': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int] * 5 +
                                    [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # (h, x, B, H, W, Cin, w, scale, Cout, KH, KW, stride, pad, y, relu, g_y, g_x_add, g_x, g_w, g_res, stream)
    'specmi_conv2d_backward': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int] * 5 +
                               [C.c_void_p, C.c_int] + [C.c_void_p] * 6),
    # (h, z, M, C, gamma, beta, residual, relu, eps, momentum, running_mean, running_var, y, mean, invstd, stream)
    'specmi_batchnorm_train_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_float, C.c_float] +
                                       [C.c_void_p] * 6),
    # (h, z, M, C, gamma, mean, invstd, y, relu, g_y, g_z, g_gamma, g_beta, g_res, stream)
    'specmi_batchnorm_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 6),
    # (B, H, W, Cin, Cout, KH, KW, stride, pad, splits)
    'specmi_conv2d_wgrad_splits': (C.c_int, [C.c_int] * 9 + [C.POINTER(C.c_int)]),
    # (h, x, B, H, W, C, y, idx, stream)
    'specmi_maxpool3x3s2_train_forward': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3),
    # (h, g_y, idx, B, H, W, C, g_x, stream)
    'specmi_maxpool3x3s2_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2),
    # (h, images, B, H, W, n_stages, out, stream)
    'specmi_trunk_forward_stages': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    'specmi_conv2d': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'specmi_conv2d_strided': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'specmi_conv2d_f16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'specmi_set_precision': (C.c_int, [C.c_void_p, C.c_int]),
    'specmi_get_precision': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'specmi_maxpool3x3s2': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p]),
    'specmi_maxpool3x3s2_f16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p]),
    'specmi_to_nhwc_f16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p]),
    'specmi_avgpool': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    # (h, nheads, w_host[3], bias_host[3], N, K, x[3], ldx, residual[3], out[3], ldo, B, path, stream)
    'specmi_fc_forward': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                    C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                    C.c_int, C.c_void_p]),
    'specmi_hr_stem3x3': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    'specmi_hr_fuse_sum': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'specmi_hr_resize_ac': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p]),
    'specmi_trunk_forward_pair': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    'specmi_camcalib_head_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    'specmi_crop_normalize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_crop_normalize_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_crop_resize_normalize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p]),
    'specmi_resize_normalize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    'specmi_resize_normalize_ragged': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, c_int32_p, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p]),
    # NHWC8 fp16 producers / consumers: the prototypes of their fp32 twins (every pointer is a void*)
    'specmi_crop_normalize_batch_f16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_crop_resize_normalize_f16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_void_p]),
    'specmi_resize_normalize_f16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    'specmi_resize_normalize_ragged_f16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, c_int32_p, C.c_int, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_void_p]),
    # ragged crops: (h, slab, slab_bytes, offsets, geom, nframes, frame_index, boxes, n, ...)
    'specmi_crop_normalize_ragged': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, c_int32_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_crop_normalize_f16_ragged': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, c_int32_p, C.c_int, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_crop_resize_normalize_ragged': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, c_int32_p, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'specmi_crop_resize_normalize_f16_ragged': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, c_int32_p, C.c_int, C.c_void_p,
                                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'specmi_trunk_forward_f16in': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'specmi_camcalib_forward_f16in': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_hmr_forward_f16in': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(HmrOutputs), C.c_void_p]),
    'specmi_pano_extract_views': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_double_p, c_int32_p, c_int64_p, C.c_size_t,
                                            C.c_void_p, C.c_int, C.c_void_p]),
    # (h, vertices, M, V, faces, F, cam_t, R, fx, fy, cx, cy, frame, H, W, rgb, flags, out, id_map, depth, screen, stream)
    'specmi_render_meshes': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, c_float_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (h, vertices, Mtot, V, faces, F, cam_t, rgb, in_slab, in_bytes, out_slab, out_bytes, view_geom, view_offsets, view_cams, nviews,
    #  id_map, depth, screen, stream)
    'specmi_render_views': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, c_float_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_size_t, c_int32_p, c_int64_p, c_float_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    # (h, kp, Mtot, J, D, bones, NB, style, slab, slab_bytes, frame_geom, frame_offsets, nframes, stream)
    'specmi_draw_skeletons': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_int32_p, C.c_int, C.POINTER(DrawStyle), C.c_void_p,
                                        C.c_size_t, c_int32_p, c_int64_p, C.c_int, C.c_void_p]),
    # (h, slab, slab_bytes, frame_geom, frame_offsets, nframes, marks, nmarks, masks, mask_bytes, stream)
    'specmi_draw_marks': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int32_p, c_int64_p, C.c_int, c_int64_p, C.c_int, C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    # (h, x, B, Hp, Wp, index, H, W, mean3, std3, slab, slab_bytes, offset, pitch, stream)
    'specmi_denormalize_u8': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p,
                                        C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_void_p]),
    # in slab + bytes, out slab + bytes, frame_geom (n x 2), frame_offsets (n x 4), records (n x 8), nframes, stream
    'specmi_color_jitter': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_int32_p, c_int64_p, c_int32_p, C.c_int,
                                      C.c_void_p]),
    # (h, in_slab, in_bytes, out_slab, out_bytes, pic_geom, pic_offsets, n, quality, sizes, stream)
    'specmi_jpeg_encode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_int32_p, c_int64_p, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p]),
    'specmi_jpeg_header': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    # (h, in_slab, in_bytes, out_slab, out_bytes, pic_geom, pic_offsets, n, sizes, stream)
    'specmi_png_encode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_int32_p, c_int64_p, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    'specmi_png_bound': (C.c_int, [C.c_int, C.c_int, c_int64_p]),
    'specmi_png_header': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    # (file, bytes, reason, H, W, sampling)
    'specmi_jpeg_probe': (C.c_int, [C.c_void_p, C.c_size_t, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    # (h, files_host, in_slab, in_bytes, file_ranges, out_slab, out_bytes, out_offsets, n, status, coef, coef_bytes, passes, stream)
    'specmi_jpeg_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, C.c_void_p, C.c_size_t, c_int64_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_size_t, c_int32_p, C.c_void_p]),
    # (file, bytes, reason, H, W, colour_type, idat_ranges, max_ranges, nranges)
    'specmi_png_probe': (C.c_int, [C.c_void_p, C.c_size_t, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int64_p, C.c_int, c_int32_p]),
    # (h, in_slab, in_bytes, stream_ranges, geom, out_slab, out_bytes, out_offsets, n, status, raw, raw_bytes, stream)
    'specmi_png_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, c_int64_p, c_int32_p, C.c_void_p, C.c_size_t, c_int64_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'specmi_camcalib_eval': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_eval_mesh': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'specmi_eval_joints': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    # (h, pred_vertices, gt_vertices, B, V, J_regressor, J, joint_sel, nsel, pred_joints, gt_joints, Jk, err_sel, pa_err_sel, err_k, pa_err_k, v2v, stream)
    'specmi_eval_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6),
    'specmi_regress_joints': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    # (h, mode, 6 prediction tensors, 6 ground-truth tensors, has_smpl, has_pose_3d, orig_shape, scale, B, V, 8 weights, terms, counts, means, stream)
    'specmi_hmr_loss': (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 16 + [C.c_int, C.c_int] + [C.c_float] * 8 +
                        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (h, mode, the 16 tensors of specmi_hmr_loss, B, V, 8 weights, terms, counts, g_means, 6 gradients, stream)
    'specmi_hmr_loss_backward': (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 16 + [C.c_int, C.c_int] + [C.c_float] * 8 +
                                 [C.c_void_p] * 3 + [C.c_void_p] * 6 + [C.c_void_p]),
    'specmi_rotate_points': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'specmi_trunk_plan': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    'specmi_sync_status': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    'specmi_sync_reset': (C.c_int, [C.c_void_p, C.c_void_p]),
    'specmi_debug_poison_sync': (C.c_int, [C.c_void_p, C.c_uint32]),
    'specmi_profile_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'specmi_profile_read': (C.c_int, [C.c_void_p, C.POINTER(ProfEntry), C.c_int, C.POINTER(C.c_int)]),
}

_lib = None


def load():
    """Load libspecmi.so and attach prototypes; raises if it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64.so; libspecmi.so links the HIP runtime by SONAME.  Whichever copy the
    # process loads first serves both, and tensors / streams must come from the SAME runtime as the kernels that use
    # them - so torch's goes first (loading /opt/rocm's before torch left the process without a visible device).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} not found: build it with `python -m spec_amd.build` '
            '(or __graft_entry__.build()).  spec_amd has no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)       # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(handle, rc):
    if rc != OK:
        msg = load().specmi_last_error(handle)
        raise SpecmiError(rc, msg.decode() if msg else '?')
