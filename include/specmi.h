/*
 * specmi.h - C ABI of the MI355X-native SPEC inference hot path (libspecmi.so).
 *
 * The reference (mkocabas/SPEC) has NO native/FFI seam for this path: its boundary is two
 * Python nn.Module classes whose leaf ops are stock torch ops,
 *
 *   spec/models/hmr.py:28-122      class HMR            (trunk -> HMRHead -> SMPLCamHead)
 *   camcalib/model.py:24-81        class CameraRegressorNetwork (trunk -> avgpool -> 3 FC)
 *   camcalib/cam_utils.py:110-145  soft-argmax decode of the 256-bin logits
 *   spec/utils/cam_params.py:24-50 (pitch, roll, f) -> cam_rotmat, cam_intrinsics
 *
 * so this header DEFINES the boundary a maintainer would bind (ctypes stub in
 * INTEGRATION.md).  Each entry point names the reference interface it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no exceptions cross the ABI.
 *   - return 0 (SPECMI_OK) or an error code; the message is kept per handle
 *     (specmi_last_error).  Passing h == NULL to specmi_last_error returns the last error
 *     of a failed specmi_create.
 *   - parameters are handed over as HOST pointers in the canonical PyTorch layouts under
 *     their state_dict key names; the library folds BatchNorm into a
 *     per-channel scale/shift, re-lays the weights out for the MFMA kernels and uploads
 *     them at specmi_commit.
 *   - every forward I/O buffer is a caller-owned DEVICE pointer (torch.Tensor.data_ptr());
 *     the library owns only the packed weights and its workspace.  All work is enqueued on
 *     the caller's HIP stream (`stream` is a hipStream_t passed as void*; NULL = default
 *     stream); no call synchronises the device except specmi_commit, specmi_destroy and
 *     specmi_profile_read.
 *   - every call runs on the device the handle was created for and restores the caller's current HIP device before
 *     it returns (a second device in the same process is fine; kernel attributes are set per device).
 *   - one handle per model instance; a handle is not thread-safe (the reference is
 *     single-threaded) and is driven from ONE stream at a time (its workspaces, split-K slabs and hand-off counters are per
 *     handle: two streams in the same handle at once would share them); distinct handles are independent.
 *   - all arithmetic is IEEE fp32 by default; index tables are int32.  The reference's evaluation entry point runs under
 *     Lightning precision=16 when its config sets TRAINING.USE_AMP (scripts/spec_eval.py:63-70, spec/config.py:138, default
 *     false): specmi_set_precision(h, SPECMI_PRECISION_FP16) selects the matching reduced-precision ResNet trunk (fp16
 *     activations and weights, fp32 accumulation; "precision" section below).  Heads, decode and SMPL stay fp32 either way.
 */
#ifndef SPECMI_H
#define SPECMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct specmi_handle specmi_handle;

enum {
    SPECMI_OK = 0,
    SPECMI_ERR_ARG = 1,     /* bad argument (null pointer, bad shape, unknown name)      */
    SPECMI_ERR_HIP = 2,     /* a HIP runtime call failed                                  */
    SPECMI_ERR_STATE = 3,   /* call order violated (forward before commit, ...)           */
    SPECMI_ERR_MISSING = 4  /* commit: a required tensor was never set                    */
};

enum {
    SPECMI_MODEL_CAMCALIB = 0, /* camcalib/model.py CameraRegressorNetwork(resnet50, 1 FC) */
    SPECMI_MODEL_HMR = 1,      /* spec/models/hmr.py HMR(resnet50)                         */
    SPECMI_MODEL_SMPL = 2      /* the SMPL body model alone ("smpl.*" tensors only): specmi_smpl_native /
                                  specmi_smpl_forward for ground-truth meshes in the evaluation code
                                  (spec/utils/compute_error.py:118-160, spec/trainer.py:71-86)             */
};

/* Output dict of HMR.forward (spec/models/hmr.py:113,122): device pointers, fp32. */
typedef struct specmi_hmr_outputs {
    float* smpl_vertices; /* (B, V, 3)      */
    float* smpl_joints3d; /* (B, 49, 3)     */
    float* smpl_joints2d; /* (B, 49, 2)     */
    float* pred_cam_t;    /* (B, 3)         */
    float* pred_pose;     /* (B, 24, 3, 3)  */
    float* pred_cam;      /* (B, 3)         */
    float* pred_shape;    /* (B, 10)        */
    float* pred_pose_6d;  /* (B, 144)       */
} specmi_hmr_outputs;

/* One record of the built-in launch profiler (HIP events around every kernel). */
typedef struct specmi_prof_entry {
    char   kernel[48];  /* kernel family, e.g. "conv_igemm_f32<128x128>"                   */
    char   label[48];   /* call site, e.g. "backbone.layer2.0.conv2"                       */
    double ms;          /* accumulated device time                                         */
    double flops;       /* algorithmic FLOPs of the accumulated launches (2*MACs)          */
    double bytes;       /* algorithmic HBM bytes (activations in+out+residual, weights)    */
    int    launches;
} specmi_prof_entry;

/* ---- lifetime ------------------------------------------------------------------------ */

/* Replaces the module constructors HMR.__init__ (spec/models/hmr.py:29-80) and
 * CameraRegressorNetwork.__init__ (camcalib/model.py:25-57). */
int specmi_create(specmi_handle** out, int device_id, int model_kind);
int specmi_destroy(specmi_handle* h);
const char* specmi_last_error(const specmi_handle* h);
const char* specmi_version(void);

/* ---- parameters (replaces load_state_dict / load_pretrained_model,
 *      spec/tester.py:63-71, scripts/camcalib_demo.py:80-81) ---------------------------- */

/* ---- options -------------------------------------------------------------------------------------------------------------
 * specmi_set_option_i32 / _f32 accept the names below and refuse anything else (SPECMI_ERR_ARG).  The option table of the library
 * (specmi_option_info) is the single list; tests/test_abi.py holds this comment and the code to it.
 *
 * STABLE (frozen in round 6: what a reference maintainer binds)
 *   Model shape, before specmi_commit.  CamCalib (camcalib/model.py:25-70): "backbone" (50 default | 18 | 34 | 101 | 152: the
 *   torchvision ResNet family the reference's eval(backbone) resolves, spec/models/hmr.py:53, camcalib/model.py:33; HMR also 32 / 48 =
 *   HRNet-W32 / W48, with "hrnet_use_conv" 1 = the '-conv' variant, hmr.py:44-51), "num_fc_layers" (1..3), "num_fc_channels"
 *   (<= 1024, multiple of 32).  HMR: "use_cam" (SMPLCamHead vs SMPLHead, hmr.py:66-74), "use_cam_feats" (hmr.py:55,94-98),
 *   "img_res" (224; hmr.py:69), "estimate_var" (0; 1 = HMRHead's uncertainty outputs, hmr.py:35-38,57-64: the library then also wants
 *   "head.decpose_var.*" (144 rows) and "head.decshape_var.*" (10 rows) - the separate-branch layout; a binding splits the doubled
 *   decoders of the other layout - and serves specmi_hmr_uncertainty), "uncertainty_activation" (0 none | 1 relu | 2 softplus |
 *   3 sigmoid | 4 tanh | 5 elu: the torch.nn.functional the reference evaluates by name).  Float option: "focal_length" (5000; hmr.py:31).
 *   Execution, any time (read at every forward):
 *   "plan" - the execution plan of the ResNet trunk:
 *     1 = throughput: the kernels the batch-256 benchmark runs (Winograd F(2x2,3x3) + 64x64 / 128x128 implicit GEMM);
 *     2 = latency: for the reference's own operating point - spec/tester.py:109-151 runs the path at batch = #detections of one
 *         frame, scripts/camcalib_demo.py:95-102 at batch 1 - every convolution with K >= 512 is cut into K slices that run as ONE
 *         launch (the last slice of a tile to arrive folds the partial tiles and applies BN / residual / ReLU), layer3 / layer4
 *         3x3 convolutions leave Winograd for the sliced direct kernel;
 *     3 = single: the latency plan with EVERY 3x3 convolution on the sliced direct kernels (no Winograd) - what batch 1-2 wants;
 *     0 = auto (default): single up to 2 images of 224 x 224 per call, latency up to 10 (trunk pair, FC heads) / 16 (single trunk;
 *         one CamCalib frame at 600 x 1066 counts as 12.7 images), throughput beyond.  specmi_trunk_plan reports the choice.
 *     WITHIN a plan an image's result is bit-identical whatever the batch size, the grouping (specmi_trunk_forward_pair) or the
 *     replay (every k sum has one association fixed by the layer's shape; 8 x 256 rank shards == 2048 unsharded).  BETWEEN plans the
 *     last bits differ (other association of the same products, other algorithm on layer3 / layer4 conv2); all meet the 1e-4
 *     contract on every reference fixture (tests/test_gpu_e2e.py, tests/test_gpu_pretrained_like.py).  Callers that need
 *     bit-reproducibility across batch sizes on both sides of a switch pin a plan (spec_amd.tester runs a whole folder under ONE plan
 *     whatever --frame_batch; bench.py pins 'throughput' for rank-sharded runs).
 *   "winograd" (default 1: 3x3 / stride-1 convolutions with Cin % 16 == 0 and Cout % 64 == 0 run as fused Winograd F(2x2,3x3) on the
 *     fp32 matrix cores under the throughput / latency plans; 0: always the direct implicit GEMM);
 *   "fuse_downsample" (default 1: a bottleneck's downsample conv + BN is folded into its conv3 as one 1x1 GEMM over
 *     [conv2 output | block input]; 0: separate launch + residual add, as torchvision writes it);
 *   "head_collapse" (default 1; HMR, read at commit and at forward: the three IEF iterations of HMRHead - an affine map in eval mode,
 *     no activation between fc1 / fc2 / dec* and dropout = identity - run as ONE (features + camera features) -> 157 GEMM whose
 *     matrix is composed in float64 at commit; 0: the nine GEMMs of the reference loop);
 *   "output_ld" (HMR, default 0 = dense outputs; n > 0: every per-image output pointer of specmi_hmr_forward /
 *     specmi_hmr_head_forward / specmi_smpl_forward addresses image 0 and image b lives at pointer + b*n floats, i.e. the outputs are
 *     columns of ONE caller-owned (B, n) record - the packed all-gather record of SURVEY.md 8e - written by the kernels directly);
 *   "angle_ld" (the same for vfov / pitch / roll of specmi_camcalib_decode / specmi_camcalib_head_decode);
 *   "experimental" (default 0; 1 = this handle accepts the names of the next list).
 *
 * EXPERIMENTAL (refused with SPECMI_ERR_STATE unless the environment has SPECMI_EXPERIMENTAL=1 or the handle's "experimental" is 1;
 * setting one to its default is a no-op and always accepted).  Tuning thresholds from single-box sweeps, debug pins, opt-ins that
 * measured slower or neutral on MI355X, and the narrower-arithmetic secondary mode: scaffolding of the experiments recorded in
 * docs/ROUNDS.md and profiles/, same bits as the defaults unless stated, no compatibility promise.
 *   secondary arithmetic: "conv_precision" (0; 3 / 6 = the 1x1 (6: and strided 3x3) convolutions as that many bf16 piece products on
 *     the bf16 matrix cores: NOT the reference's fp32 arithmetic per product, tests/test_gpu_bf16split.py), "conv_precision_3x3" (0);
 *   debug pins: "force_conv_variant" / "force_wino_variant" (0 = auto), "latency_force_unit" (0 = by batch, 1 / 2 / 3 = a leaf / a
 *     group / the whole K per workgroup), "conv2d_sk" (specmi_conv2d only: 0 = throughput kernel, -1 = the latency plan's rule,
 *     n > 1 = n leaves), "conv2d_wsplit" (specmi_conv2d only: 0 | 2 | 3), "smpl_skin_split" (-1 = by batch, 0 / 1 = never / always),
 *     "trunk_subbatch" (0) / "trunk_subbatch_layers" (2), "fc_splitk" (1), "fc_gemv" (1), "head_fuse" (3; bit 0: the regressor's state
 *     init rides in the pooling launch, bit 1: head_final's work is done by the SMPL pose kernel), "camcalib_head_group" (1; 0 = the
 *     CamCalib training heads' independent products as three single launches instead of one grouped launch: same bits),
 *     "conv_wgrad_splits" (0 = specmi_conv2d_wgrad_splits' rule; n >= 1: specmi_conv2d_backward cuts the weight gradient's contraction
 *     into min(n, B OH) splits whatever the shape - other bits than the rule's; how profiles/trunk_train_aux.json measured the rule);
 *   plan thresholds: "single_max_batch" (2), "latency_max_batch" (10), "latency_max_batch_single" (16), "latency_target_wgs" (256),
 *     "latency_min_chunks" (4), "latency_wino_min_tiles" (128), "latency_fill_wgs" (240) / "latency_fill_wgs_large" (400),
 *     "latency_unit_model" (0; 1 = pick the unit by a round model with "latency_unit_slots" 256: measured equal or worse);
 *   wave-split unit of the latency / single plans (spec_amd/csrc/conv_wsplit.hip): "wsplit" (1; 0 = never, 2 / 3 = always with one
 *     group / all groups per workgroup), "wsplit_max_units" (1400, trunk pair), "wsplit_max_units_single" (500), "wsplit_slots" (256). */
int specmi_set_option_i32(specmi_handle* h, const char* name, int value);
int specmi_set_option_f32(specmi_handle* h, const char* name, float value);
/* The effective value of an integer option on this handle: what was set, else the default of the table. */
int specmi_get_option_i32(specmi_handle* h, const char* name, int* value);
/* Entry `index` (0 .. n-1; SPECMI_ERR_ARG past the end) of the option table: name, default and whether it is on the STABLE list.
 * Needs no handle and no GPU. */
int specmi_option_info(int index, const char** name, int* default_value, int* is_stable);

/* Host tensors under state_dict key names, e.g. "backbone.layer1.0.conv1.weight" (OIHW),
 * "backbone.bn1.running_var", "fc_vfov.weight" (out,in), "head.fc1.weight",
 * "head.init_pose"; SMPL body model under "smpl.v_template" (V,3), "smpl.shapedirs"
 * (V,3,10), "smpl.posedirs" (207,3V), "smpl.J_regressor" (24,V), "smpl.lbs_weights" (V,24),
 * "smpl.J_regressor_extra" (9,V); int32: "smpl.parents" (24), "smpl.extra_vertex_ids" (21),
 * "smpl.joint_map" (49).  Data is copied; the caller may free it on return. */
int specmi_set_tensor_f32(specmi_handle* h, const char* name, const float* host_data,
                          const int64_t* shape, int ndim);
int specmi_set_tensor_i32(specmi_handle* h, const char* name, const int32_t* host_data,
                          const int64_t* shape, int ndim);
/* Validate, fold BN, pack and upload to HBM.  May be called again after further set_* calls. */
int specmi_commit(specmi_handle* h);

/* ---- precision (the reference's TRAINING.USE_AMP switch) ----------------------------------------------------------------
 * Model state that specmi_commit reads, not an option.  SPECMI_PRECISION_FP32 (default): every path as documented above.
 * SPECMI_PRECISION_FP16: the ResNet trunk (every convolution and the max-pool) runs on fp16 activations with the BatchNorm
 * scale folded into fp16 weights, fp16 x fp16 products accumulated in fp32 on the fp16 matrix cores, an fp32 epilogue
 * (shift, fp16 residual, ReLU) rounded to nearest even into fp16; the last convolution of layer4 stores fp32, and the
 * avg-pool, heads, decode, SMPL and projection run unchanged in fp32 (numeric contract: DESIGN.md, "fp16 trunk").
 *   - the fp16 weights are packed at specmi_commit; a forward on a handle whose precision changed since its last successful
 *     commit returns SPECMI_ERR_STATE.  Commit returns SPECMI_ERR_ARG, naming the layer, when a folded weight lies outside
 *     the finite fp16 range (never silently inf), and for the HRNet backbones (not built at fp16).
 *   - one kernel family at every batch size and resolution: options "plan", "winograd", "wsplit", the latency_* /
 *     trunk_subbatch tuning and "conv_precision" do not apply to the fp16 trunk; an image's bits do not depend on B.
 *   - specmi_trunk_forward_pair with either handle at fp16 runs as two specmi_trunk_forward calls on the stream (same bits). */
enum { SPECMI_PRECISION_FP32 = 0, SPECMI_PRECISION_FP16 = 1 };
int specmi_set_precision(specmi_handle* h, int precision);
/* the precision last set (what the next commit packs) */
int specmi_get_precision(specmi_handle* h, int* precision);

/* ---- NHWC8 fp16: the image layout of the fp16 trunk's entrance ------------------------------------------------------------
 * (B, H, W, 8) fp16, pixel-major, 16 bytes per pixel, device pointer 16-byte aligned.  Channels 0-2 hold fp16_rne(v), v being
 * the fp32 normalised value the fp32 producer of the same name stores (one rounding to nearest even, nothing else differs);
 * channels 3-7 hold +0 (bits 0x0000).  Bit for bit what specmi_to_nhwc_f16(x, B, 3, H, W) makes of the fp32 NCHW image, and
 * what the Cin = 8 stem of the fp16 trunk reads.
 *   producers: specmi_crop_normalize_batch_f16, specmi_crop_resize_normalize_f16, specmi_resize_normalize_f16,
 *              specmi_resize_normalize_ragged_f16, specmi_crop_normalize_f16_ragged, specmi_crop_resize_normalize_f16_ragged - each takes the arguments of its fp32 twin with `void* out_nhwc8` in place of
 *              the fp32 image; the lane that owns a pixel writes it as one 16-byte vector.  Refused beyond the twin's refusals
 *              (SPECMI_ERR_ARG): an output that is not 16-byte aligned.
 *   consumers: specmi_trunk_forward_f16in, specmi_camcalib_forward_f16in, specmi_hmr_forward_f16in - each takes the arguments
 *              of its twin with `const void* images_nhwc8`: the stem reads the caller's buffer where it lies, no fp32 image
 *              exists and the conversion launch (to_nhwc_f16) is skipped; everything after the stem is the twin's code, so the
 *              outputs equal, bit for bit, the twin's on the fp32 producer's image.  Refused, nothing launched, the handle
 *              serves the next call: SPECMI_ERR_STATE - the handle is not committed at SPECMI_PRECISION_FP16, or has an HRNet
 *              trunk; SPECMI_ERR_ARG - images_nhwc8 is not 16-byte aligned, H or W below 32. */

/* ---- forward: CamCalib ----------------------------------------------------------------- */

/* (The execution plan - option "plan" above - is chosen from the FIRST handle's options and B, H, W for both trunks.)
 * The ResNet trunks of TWO committed models (CamCalib + SPEC: camcalib/model.py:73 `self.backbone(images)` and
 * spec/models/hmr.py:92 `self.backbone(images)`, which the reference runs as two processes / two calls) walked in lockstep
 * with every layer of both as ONE grouped launch: images_a / images_b (B,3,H,W) NCHW -> feat_a / feat_b (B, H/32, W/32, C)
 * NHWC.  Both trunks must be ResNets of the same depth and see the same B, H, W; each keeps its own weights and workspaces.
 * Results are bit-identical to two specmi_trunk_forward calls. */
int specmi_trunk_forward_pair(specmi_handle* ha, specmi_handle* hb, const float* images_a, const float* images_b, int B,
                              int H, int W, float* feat_a, float* feat_b, void* stream);

/* The part of CameraRegressorNetwork.forward after the backbone (camcalib/model.py:74-80: avg-pool, flatten, the three
 * Linear chains) from a trunk feature map (B,fh,fw,C) NHWC -> vfov / pitch / roll logits (B,nbins) each. */
int specmi_camcalib_head_forward(specmi_handle* h, const float* feat_nhwc, int B, int fh, int fw, float* logits_vfov,
                                 float* logits_pitch, float* logits_roll, void* stream);

/* specmi_camcalib_head_forward + specmi_camcalib_decode in one call (round 5).
 * Replaces camcalib/model.py:74-80 + camcalib/cam_utils.py:110-133 + scripts/camcalib_demo.py:129 + spec/utils/cam_params.py:37-46.
 * Outputs as in the two calls (any of vfov .. K may be NULL); "angle_ld" applies to vfov / pitch / roll. */
int specmi_camcalib_head_decode(specmi_handle* h, const float* feat_nhwc, int B, int fh, int fw, float* logits_vfov,
                                float* logits_pitch, float* logits_roll, const float* img_h, const float* img_w, float* vfov,
                                float* pitch, float* roll, float* f_pix, float* cam_rotmat, float* cam_intrinsics, void* stream);

/* CameraRegressorNetwork.forward (camcalib/model.py:72-81): images (B,3,H,W) NCHW fp32 ->
 * three (B,256) logit tensors [vfov, pitch, roll]. */
int specmi_camcalib_forward(specmi_handle* h, const float* images_nchw, int B, int H, int W,
                            float* logits_vfov, float* logits_pitch, float* logits_roll,
                            void* stream);
/* specmi_camcalib_forward from NHWC8 fp16 images (B,H,W,8) ("NHWC8 fp16" above): replaces the fp32 image + its conversion in
 * front of the fp16 trunk.  Refuses a handle not committed at SPECMI_PRECISION_FP16 (SPECMI_ERR_STATE), a misaligned
 * pointer and H / W < 32 (SPECMI_ERR_ARG). */
int specmi_camcalib_forward_f16in(specmi_handle* h, const void* images_nhwc8, int B, int H, int W,
                                  float* logits_vfov, float* logits_pitch, float* logits_roll, void* stream);

/* convert_preds_to_angles soft-argmax branch (camcalib/cam_utils.py:114-133), focal length
 * (scripts/camcalib_demo.py:129) and the CamCalib->SPEC hand-off read_cam_params
 * (spec/utils/cam_params.py:37-48), fused in one launch.  Any output pointer may be NULL.
 * img_h/img_w: (B,) full-image size in pixels.  R (B,3,3) = Rx(pitch) Ry(0) Rz(roll);
 * K (B,3,3) = [[f,0,w/2],[0,f,h/2],[0,0,0]] (K[2,2] stays 0 as in the reference). */
int specmi_camcalib_decode(specmi_handle* h, const float* logits_vfov, const float* logits_pitch,
                           const float* logits_roll, int B, int nbins, const float* img_h,
                           const float* img_w, float* vfov, float* pitch, float* roll,
                           float* f_pix, float* cam_rotmat, float* cam_intrinsics, void* stream);

/* The two per-row reductions of camcalib/cam_utils.py on a (rows, nbins) device logit tensor:
 *   argmax_idx[row] = np.argmax(row) - bins2vfov / bins2pitch / bins2roll / bins2horizon (cam_utils.py:66-91), the 'kl' / 'ce'
 *                     and legacy branches of convert_preds_to_angles (:123-133); first maximum, NaN counts as maximum;
 *                     the caller gathers the bin-centre table (host float64, as the reference returns it);
 *   soft_idx[row]   = get_softargmax (cam_utils.py:110-118): softmax expectation of the index, normalised to [-1, 1].
 * Either output may be NULL (not both). */
int specmi_camcalib_bins(specmi_handle* h, const float* logits, int rows, int nbins, int32_t* argmax_idx,
                         float* soft_idx, void* stream);

/* CamCalib's test step after the network (camcalib/trainer.py:84-116): CameraRegressorLoss (camcalib/loss.py:24-125: the four
 * loss types, three weights applied as :109-116 - 'softargmax_biased_l2' uses the biased criterion for vfov only),
 * convert_preds_to_angles' soft-argmax branch and |pred - gt|, on three (B, nbins) device logit tensors.
 *   target_*  : (B,) int32 bin index (np.digitize, pano_dataset.py:135-138) for SPECMI_LOSS_CE / _KL, (B,) fp32 soft index in
 *               [-1, 1] (pano_dataset.py:139-142) for the soft-argmax losses;  gt_* : (B,) fp32 angles in radians.
 * Per image and head, each a (3, B) array in the order vfov, pitch, roll (all five required):
 *   loss_term (unweighted; ce = kl = -log_softmax(x)[t]: against a one-hot target F.kl_div keeps exactly that term),
 *   argmax_idx (first maximum; the 'ce' / 'kl' decode gathers the host float64 bin-centre tables with it, as
 *   specmi_camcalib_bins' callers do), soft_idx in [-1, 1], angle (radians, soft-argmax branch), abs_err = |angle - gt|.
 * means (7 floats, may be NULL): [loss, vfov_loss, pitch_loss, roll_loss] with the weights applied, then
 *   [vfov_acc, pitch_acc, roll_acc] = mean abs_err in degrees; summed in an order that depends on B alone (bit-reproducible).
 * A per-image value never depends on the other rows of the batch. */
#define SPECMI_LOSS_CE 0
#define SPECMI_LOSS_KL 1
#define SPECMI_LOSS_SOFTARGMAX_L2 2
#define SPECMI_LOSS_SOFTARGMAX_BIASED_L2 3
int specmi_camcalib_eval(specmi_handle* h, const float* logits_vfov, const float* logits_pitch, const float* logits_roll,
                         int B, int nbins, int loss_type, const void* target_vfov, const void* target_pitch,
                         const void* target_roll, const float* gt_vfov, const float* gt_pitch, const float* gt_roll,
                         float weight_vfov, float weight_pitch, float weight_roll, float* loss_term, int32_t* argmax_idx,
                         float* soft_idx, float* angle, float* abs_err, float* means, void* stream);

/* read_cam_params (spec/utils/cam_params.py:24-50) for angles that were decoded earlier, e.g.
 * read back from the CamCalib result pickle: (pitch, roll, f_pix, img_w, img_h) (B,) device ->
 * cam_rotmat (B,3,3), cam_intrinsics (B,3,3) (K[2,2] = 0).  Either output may be NULL. */
int specmi_cam_params(specmi_handle* h, const float* pitch, const float* roll, const float* f_pix,
                      const float* img_w, const float* img_h, int B, float* cam_rotmat,
                      float* cam_intrinsics, void* stream);

/* ---- forward: SPEC --------------------------------------------------------------------- */

/* HMR.forward (spec/models/hmr.py:82-122).  cam_* / bbox_* / img_* may be NULL when the
 * handle was built with use_cam = 0 (and use_cam_feats = 0). */
int specmi_hmr_forward(specmi_handle* h, const float* images_nchw, int B, int H, int W,
                       const float* cam_rotmat, const float* cam_intrinsics,
                       const float* bbox_scale, const float* bbox_center, const float* img_w,
                       const float* img_h, const specmi_hmr_outputs* out, void* stream);
/* specmi_hmr_forward from NHWC8 fp16 images (B,H,W,8) ("NHWC8 fp16" above): replaces the fp32 crops + their conversion in
 * front of the fp16 trunk.  Refuses a handle not committed at SPECMI_PRECISION_FP16 or with an HRNet trunk
 * (SPECMI_ERR_STATE), a misaligned pointer and H / W < 32 (SPECMI_ERR_ARG). */
int specmi_hmr_forward_f16in(specmi_handle* h, const void* images_nhwc8, int B, int H, int W,
                             const float* cam_rotmat, const float* cam_intrinsics,
                             const float* bbox_scale, const float* bbox_center, const float* img_w,
                             const float* img_h, const specmi_hmr_outputs* out, void* stream);

/* The two extra outputs of HMR.forward when the model was built with estimate_var = True (spec/models/hmr.py:35-38,57-64; consumed
 * by spec/losses.py:61-62): pred_pose_var (B, 288) = [pred_pose_6d | var_pose], pred_shape_var (B, 20) = [pred_shape | var_shape],
 * the variances being the extra decoder outputs of the LAST regressor iteration through option "uncertainty_activation".  Call after
 * specmi_hmr_forward / specmi_hmr_regress / specmi_hmr_head_forward of the same batch on the same stream (it reads what that call
 * left in the handle's workspace); dense outputs.  SPECMI_ERR_STATE without option "estimate_var". */
int specmi_hmr_uncertainty(specmi_handle* h, int B, float* pred_pose_var, float* pred_shape_var, void* stream);

/* Everything of HMR.forward after `features = self.backbone(images)` (spec/models/hmr.py:94-122): regressor head +
 * SMPL head from an NHWC layer-4 map (B, fh, fw, C).  Lets a caller run the SPEC trunk beside the CamCalib network
 * (whose output the head needs) on another stream and join afterwards. */
int specmi_hmr_regress(specmi_handle* h, const float* feat_nhwc, int B, int fh, int fw,
                       const float* cam_rotmat, const float* cam_intrinsics, const float* bbox_scale,
                       const float* bbox_center, const float* img_w, const float* img_h,
                       const specmi_hmr_outputs* out, void* stream);

/* ---- stage-level entry points (parity tests, profiling, reuse) ------------------------- */

/* The trunk alone: `self.backbone(images)` (hmr.py:92, camcalib/model.py:73).  Output is the
 * layer4 map in NHWC: (B, H/32, W/32, 2048). */
int specmi_trunk_forward(specmi_handle* h, const float* images_nchw, int B, int H, int W,
                         float* feat_nhwc, void* stream);
/* specmi_trunk_forward from NHWC8 fp16 images (B,H,W,8) ("NHWC8 fp16" above): the stem reads images_nhwc8 itself, the
 * to_nhwc_f16 launch and the fp32 image it read are gone.  A batch whose image passes 2 GiB is still cut into launches of
 * whole images.  Refuses a handle not committed at SPECMI_PRECISION_FP16 or with an HRNet trunk (SPECMI_ERR_STATE), a
 * misaligned pointer and H / W < 32 (SPECMI_ERR_ARG). */
int specmi_trunk_forward_f16in(specmi_handle* h, const void* images_nhwc8, int B, int H, int W,
                               float* feat_nhwc, void* stream);

/* HMRHead.forward on an NHWC feature map (hmr.py:96/98): avg-pool + 3 IEF iterations +
 * rot6d->rotmat.  Outputs any-NULL. */
int specmi_hmr_head_forward(specmi_handle* h, const float* feat_nhwc, int B, int fh, int fw,
                            const float* cam_rotmat, const float* cam_intrinsics,
                            const float* img_h, float* pred_pose, float* pred_shape,
                            float* pred_cam, float* pred_pose_6d, void* stream);

/* SMPLCamHead / SMPLHead forward (hmr.py:101-120): SMPL LBS (pose2rot=False) + 49 joints +
 * camera translation + perspective projection. */
int specmi_smpl_forward(specmi_handle* h, const float* rotmat, const float* betas,
                        const float* cam, int B, const float* cam_rotmat,
                        const float* cam_intrinsics, const float* bbox_scale,
                        const float* bbox_center, const float* img_w, const float* img_h,
                        float* vertices, float* joints3d, float* joints2d, float* cam_t,
                        void* stream);

/* The vector-Jacobian product of specmi_smpl_forward, for both head modes (the handle's "use_cam": SMPLCamHead with the six
 * camera arguments, else SMPLHead weak perspective with normalize_joints2d) - what torch.autograd computes through
 * rot-matrix LBS + 49 joints + convert_pare_to_full_img_cam / convert_weak_perspective_to_perspective + perspective_projection.
 *   inputs: the forward's own - rotmat (B,24,3,3), betas (B,10), cam (B,3) and, with use_cam, cam_rotmat (B,3,3),
 *     cam_intrinsics (B,3,3), bbox_scale (B), bbox_center (B,2), img_w (B), img_h (B) (not read otherwise, may be NULL);
 *   upstream gradients, dense fp32: g_vertices (B,V,3), g_joints3d (B,49,3), g_joints2d (B,49,2), g_cam_t (B,3).  Any of them
 *     may be NULL and counts as zero - the result is the same bits as with an all-zero tensor - but not all four;
 *   outputs, dense fp32: g_rotmat (B,24,3,3), g_betas (B,10), g_cam (B,3).  Any may be NULL (not wanted), not all three; with
 *     only g_cam wanted the two contractions over the vertices are not launched.  The camera arguments get no gradient.
 * Stateless: the call recomputes the forward from its arguments into the handle's scratch and reads nothing an earlier call
 * left there.  Works on SPECMI_MODEL_SMPL and SPECMI_MODEL_HMR handles.  Its workspace (the vertex gradient (B,V,3) and
 * ceil(V / 64) partial slabs of 640 x 32 floats per 32 images) grows on first use of a batch size; after one eager call of a
 * shape nothing is allocated and the call can be captured into a graph.
 * Deterministic: no float atomics; the sums over the vertices are folded in an order fixed by V alone (chunks of 64 vertices,
 * in order), joint_map entries that repeat add in joint order, so every run gives the same bits and an image's gradients do
 * not depend on the batch it is in.
 * Refusals (SPECMI_ERR_ARG, nothing launched): B <= 0; rotmat / betas / cam NULL; all upstream gradients NULL; all outputs
 * NULL; use_cam and one of the six camera arguments NULL. */
int specmi_smpl_backward(specmi_handle* h, const float* rotmat, const float* betas, const float* cam, int B,
                         const float* cam_rotmat, const float* cam_intrinsics, const float* bbox_scale,
                         const float* bbox_center, const float* img_w, const float* img_h,
                         const float* g_vertices, const float* g_joints3d, const float* g_joints2d, const float* g_cam_t,
                         float* g_rotmat, float* g_betas, float* g_cam, void* stream);

/* The head's rot6d -> rotation matrix on its own (pare.utils.geometry.rot6d_to_rotmat; the regressor runs the same function
 * inside its last kernel, same bits): x6d (N,6) -> rotmat (N,3,3).  Any handle.  Refuses NULL pointers and N <= 0. */
int specmi_rot6d_forward(specmi_handle* h, const float* x6d, int N, float* rotmat, void* stream);

/* The backward of the head's rot6d -> rotation matrix (Gram-Schmidt with columns b1, b2, b3; x6d viewed (N,3,2), element
 * [i, c] = row i of column c; F.normalize's eps = 1e-12 kept: below it the divisor is a constant): x6d (N,6), g_rotmat
 * (N,3,3) -> g_x6d (N,6).  One lane per rotation; any handle.  Refuses NULL pointers and N <= 0 (SPECMI_ERR_ARG). */
int specmi_rot6d_backward(specmi_handle* h, const float* x6d, const float* g_rotmat, int N, float* g_x6d, void* stream);

/* pare's HMRHead regressor for training (spec/models/hmr.py:57-64,94-98; STABLE): the iterative loop itself, on parameters
 * that an optimiser rewrites every step, with dropout, a tape, and its vector-Jacobian product.  H = 1024, S = 157 (144 rot6d |
 * 10 betas | 3 cam), C = 7 with use_cam_feats else 0, Kin = F + S + C:
 *     for t in 0 .. n_iter-1:   xc_t = [xf | state_t | cam_feats]
 *                               a1_t = drop1(xc_t fc1^T + b1),  a2_t = drop2(a1_t fc2^T + b2)        (no activation)
 *                               state_{t+1} = state_t + [decpose | decshape | deccam](a2_t)
 * Dropout: a = h * (m ? s : 0) with s = (float)(1 / (1 - p)); `masks` is uint8 (2 n_iter, B, 1024), ordered (t, layer), non-zero
 * = kept, drawn by the caller.  masks NULL is eval mode: no multiply, p is not read.
 * The ten parameters are DEVICE pointers to the tensors of the module's state_dict, in their shapes and row-major layout: fc1
 * (1024, Kin) / (1024), fc2 (1024, 1024) / (1024), decpose (144, 1024) / (144), decshape (10, 1024) / (10), deccam (3, 1024) / (3).
 * They are read in place at every call - nothing is packed, uploaded or committed, and nothing of the handle's committed model
 * is read: both calls work on a handle of any kind, committed or not.
 *
 * specmi_hmr_head_tape_floats: the size of the tape in floats, n_iter B (157 + 2 x 1024) - the states state_0 .. state_{n-1} and
 *   the activations a1_t, a2_t, each stacked in (t, b) row order.  A pure function: no handle, no GPU call.  Refuses (returns
 *   SPECMI_ERR_ARG) the shapes the two calls refuse and floats NULL.
 * specmi_hmr_head_train_forward: xf (B, F), rows ld_xf floats apart; cam_feats (B, 7) dense = [rotmat_to_rot6d(cam_rotmat) |
 *   vfov], NULL with C = 0; init_state (B, 157) dense; -> state (B, 157) dense = state_n, and the tape.  The tape is the
 *   caller's buffer and the only thing the backward needs of the forward: the handle keeps nothing between the two calls.
 * specmi_hmr_head_backward: the forward's params, xf, cam_feats, masks, p and shapes, its tape, and g_state (B, 157) dense, the
 *   gradient of state_n; -> g_xf (B, F) dense and the ten parameter gradients in the parameters' shapes.  g_xf, grads and every
 *   member of grads may be NULL (not wanted), but not all of them.  With only g_xf wanted no weight-gradient product is launched,
 *   with g_xf NULL its product is not; a wanted output has the same bits whatever else is wanted.  init_state and cam_feats get
 *   no gradient.
 * Every product runs on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32), tails in every dimension handled in the
 * kernel.  Deterministic: no float atomics, the order of every sum is fixed by the shapes, two runs give the same bits; row b
 * of state and of g_xf has the same bits whatever batch it is in; the parameter gradients are sums over the n_iter B stacked rows
 * in (t, b) order and depend on B alone.
 * Workspace: B x 1024 floats for the forward, n_iter B (157 + 2 x 1024) + B x 1024 for the backward, in the handle; it grows on
 * the first call of a shape, afterwards nothing is allocated and the calls can be captured into a graph.
 * Refusals (SPECMI_ERR_ARG with a message, nothing launched, no output written): B < 1 or B > 2^20; F < 1 or F > 2^20; C not 0
 * or 7; n_iter outside 1 .. 3; masks given and p outside [0, 1); params, one of its ten pointers, xf, init_state, state, tape
 * resp. g_state NULL; cam_feats NULL with C = 7; a float pointer that is not 4-byte aligned; ld_xf < F; every output NULL. */
typedef struct specmi_hmr_head_params {
    const float *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias, *decpose_weight, *decpose_bias, *decshape_weight, *decshape_bias,
        *deccam_weight, *deccam_bias;
} specmi_hmr_head_params;
typedef struct specmi_hmr_head_grads {
    float *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias, *decpose_weight, *decpose_bias, *decshape_weight, *decshape_bias,
        *deccam_weight, *deccam_bias;
} specmi_hmr_head_grads;
int specmi_hmr_head_tape_floats(int B, int F, int C, int n_iter, int64_t* floats);
int specmi_hmr_head_train_forward(specmi_handle* h, const specmi_hmr_head_params* params, const float* xf, int64_t ld_xf,
                                  const float* cam_feats, const float* init_state, const uint8_t* masks, float p, int B, int F,
                                  int C, int n_iter, float* state, float* tape, void* stream);
int specmi_hmr_head_backward(specmi_handle* h, const specmi_hmr_head_params* params, const float* xf, int64_t ld_xf,
                             const float* cam_feats, const uint8_t* masks, float p, int B, int F, int C, int n_iter,
                             const float* tape, const float* g_state, float* g_xf, const specmi_hmr_head_grads* grads,
                             void* stream);

/* CameraRegressorLoss for training (camcalib/loss.py:24-125; STABLE): the loss part of specmi_camcalib_eval without decode and
 * angle errors - it needs no ground-truth angles - and its gradient with respect to the three logit tensors.
 * specmi_camcalib_loss: three (B, nbins) logit tensors, loss_type, the three target tensors ((B,) int32 bin index for SPECMI_LOSS_CE /
 *   _KL, (B,) fp32 soft index for the soft-argmax losses) and weights as specmi_camcalib_eval takes them -> loss_term (3, B)
 *   (unweighted, heads vfov, pitch, roll) and means (4) = [loss, vfov_loss, pitch_loss, roll_loss].  Both carry the bits
 *   specmi_camcalib_eval writes on the same inputs: the per-row arithmetic is one device function both kernels call.
 * specmi_camcalib_loss_backward: the same inputs and g_means (4, device), the upstream gradients of loss, vfov_loss, pitch_loss and
 *   roll_loss -> g_vfov, g_pitch, g_roll, each (B, nbins) dense.  With p = softmax(x), E = sum_i i p_i, s = 2 E / (nbins - 1) - 1
 *   and c_k = w_k (g_means[0] + g_means[1 + k]) / B:  ce / kl: c_k (p_i - [i == t]);  softargmax_l2: c_k (-2 (t - s))
 *   (2 / (nbins - 1)) p_i (i - E);  softargmax_biased_l2: the vfov head divides -2 (t - s) by ((t - s)^2 + 1)^2 wherever s > t is
 *   false, pitch and roll use the plain form.  i - E is formed relative to the arg-max bin, so that a nearly one-hot row keeps its
 *   leading digits.  One launch, one wave per row; a row never depends on another row; no atomics: two runs give the same bits.
 *   The targets are constants (no gradient); first derivatives only.
 * Refusals (SPECMI_ERR_ARG with a message, nothing launched, no output written): a NULL pointer; B < 1 or B > 2^20; nbins < 2 or
 * nbins > 2^16; an unknown loss_type. */
int specmi_camcalib_loss(specmi_handle* h, const float* logits_vfov, const float* logits_pitch, const float* logits_roll, int B,
                         int nbins, int loss_type, const void* target_vfov, const void* target_pitch, const void* target_roll,
                         float weight_vfov, float weight_pitch, float weight_roll, float* loss_term, float* means, void* stream);
int specmi_camcalib_loss_backward(specmi_handle* h, const float* logits_vfov, const float* logits_pitch, const float* logits_roll,
                                  int B, int nbins, int loss_type, const void* target_vfov, const void* target_pitch,
                                  const void* target_roll, float weight_vfov, float weight_pitch, float weight_roll,
                                  const float* g_means, float* g_vfov, float* g_pitch, float* g_roll, void* stream);

/* CamCalib's three FC heads for training (camcalib/model.py:59-70; STABLE): fc_vfov / fc_pitch / fc_roll on the pooled feature
 * xf (B, F), each one Linear or a chain of L = 2 or 3 Linears with NO activation between them, widths F -> Hc -> .. -> nbins
 * (Hc = num_fc_channels; not read with L = 1, pass 1).  params->weight[k][l] / bias[k][l] (head k = vfov, pitch, roll; layer
 * l < L; the rest is not read) are DEVICE pointers to torch's own row-major (out, in) / (out) tensors, read in place at every
 * call - nothing is packed, uploaded or committed, and nothing of the handle's committed model is read.
 * specmi_camcalib_head_tape_floats: 3 (L - 1) B Hc, the intermediate activations as (3, L - 1, B, Hc); 0 for L = 1.  A pure
 *   function: no handle, no GPU call.  Refuses (returns SPECMI_ERR_ARG) the shapes the two calls refuse and floats NULL.
 * specmi_camcalib_head_train_forward: xf rows ld_xf floats apart -> logits (3, B, nbins) dense and the tape, the caller's buffer
 *   (may be NULL with L = 1) and the only state between the two calls.
 * specmi_camcalib_head_backward: the forward's arguments, its tape and g_logits (3, B, nbins) dense -> g_xf (B, F) dense and the
 *   parameter gradients in the parameters' shapes.  g_xf, grads and every member of grads may be NULL (not wanted), but not all
 *   of them; a wanted output has the same bits whatever else is wanted; with only g_xf wanted no weight-gradient product runs.
 *   Per head G_L = g_logits, G_{l-1} = G_l W_l, dW_l = G_l^T A_{l-1}, db_l = the column sums of G_l (eight interleaved row
 *   slices in row order, then the slices in order); g_xf = the sum over the heads of G_1 W_1, added in the order vfov, pitch, roll.
 * Every product runs on the exact-fp32 matrix instruction with tails in every dimension handled in the kernel; each step whose
 * three heads are independent - a forward layer, a data gradient above layer 1, a weight gradient - is ONE grouped launch, and a
 * head's numbers do not depend on the grouping.  Deterministic: no float atomics; row b of the logits and of g_xf has the same
 * bits in any batch; the parameter gradients depend on B alone; head k's outputs have the same bits whatever the other two
 * heads' parameters hold.
 * Workspace: 3 (L - 1) B Hc floats for the backward, in the handle; it grows on the first call of a shape, afterwards nothing is
 * allocated and the calls can be captured into a graph.
 * Refusals (SPECMI_ERR_ARG with a message, nothing launched, no output written): L outside 1 .. 3; B, F, Hc or nbins < 1 or
 * > 2^20; params, a weight or bias of a layer below L, xf, logits resp. g_logits NULL; tape NULL with L > 1; a float pointer that
 * is not 4-byte aligned; ld_xf < F; every output NULL. */
typedef struct specmi_camcalib_head_params {
    const float* weight[3][3];
    const float* bias[3][3];
} specmi_camcalib_head_params;
typedef struct specmi_camcalib_head_grads {
    float* weight[3][3];
    float* bias[3][3];
} specmi_camcalib_head_grads;
int specmi_camcalib_head_tape_floats(int B, int F, int L, int Hc, int nbins, int64_t* floats);
int specmi_camcalib_head_train_forward(specmi_handle* h, const specmi_camcalib_head_params* params, const float* xf, int64_t ld_xf,
                                       int B, int F, int L, int Hc, int nbins, float* tape, float* logits, void* stream);
int specmi_camcalib_head_backward(specmi_handle* h, const specmi_camcalib_head_params* params, const float* xf, int64_t ld_xf,
                                  int B, int F, int L, int Hc, int nbins, const float* tape, const float* g_logits, float* g_xf,
                                  const specmi_camcalib_head_grads* grads, void* stream);

/* One fused ResNet layer for training, with its gradients (spec_amd/csrc/conv_bwd.hip; STABLE): specmi_conv2d's layer
 *     y = act(conv(x, W) * scale + shift [+ residual])
 * x (B, H, W, Cin), y / residual / g_y / g_res (B, OH, OW, Cout), g_x / g_x_add (B, H, W, Cin): dense NHWC fp32 on the device.
 * w_oihw_dev is torch's own (Cout, Cin, KH, KW) fp32 tensor ON THE DEVICE, read in place at every call, and scale_dev / shift_dev
 * are (Cout) device vectors - the frozen BatchNorm as an affine map: nothing is packed on the host, uploaded or committed, nothing of
 * the handle's committed model is read and the stream is not synchronised.  Both calls work on a handle of any kind, committed or
 * not.  Layer shapes: KH = KW = 1 with pad 0 and KH = KW = 3 with pad 1, stride 1 or 2, and the stem's KH = KW = 7 with pad 3 at
 * stride 2; OH = (H + 2 pad - KH) / stride + 1; any
 * B, H, W, Cin, Cout >= 1, tails in every dimension are handled in the kernel and no access leaves a tensor.
 * specmi_conv2d_train_forward: Y[p, o] = sum_k X[gather(p, k)] W[o, k], k = (ky, kx, ci); padding taps contribute exact zeros;
 *   then v = Y * scale[o] + shift[o] (+ residual), and max(v, 0) with relu != 0.  residual may be NULL.
 * specmi_conv2d_backward: the forward's x, w, scale, its output y (read only with relu != 0: may be NULL otherwise) and g_y ->
 *     g_z = relu ? (y > 0 ? g_y : 0) : g_y        (torch's convention: an output that is exactly zero passes no gradient)
 *     G = g_z * scale[o]
 *     g_res = g_z                                                                        the gradient of the residual
 *     g_x[q, ci] = sum_k G[scatter^-1(q, k)] W[k, ci] (+ g_x_add[q, ci]),  k = (ky, kx, o)
 *     g_w[o, ci, ky, kx] = sum_p G[p, o] X[gather(p, ky, kx), ci],         p = the output pixels in (b, oy, ox) order
 *   g_x, g_w (OIHW, dense) and g_res may be NULL (not wanted), but not all of them.  g_x_add may be NULL, and may be g_x itself
 *   (a block's skip gradient summed in place: an element is read and written by the same lane); it is not read with g_x NULL.
 * Every product runs on the exact-fp32 matrix instruction as an implicit GEMM.  Deterministic: no float atomics, the order of
 * every sum is fixed by the layer's shape; two runs give the same bits; image b's y, g_x and g_res have the same bits in any
 * batch; g_w depends on the shapes alone; a wanted output has the same bits whatever else is wanted; with g_w NULL no
 * weight-gradient product is launched, with g_x NULL no data-gradient product.
 * Workspace: Cout Cin KH KW floats for the forward (the weights transposed on the device at every call to [tap][ci][o], so that a
 * column tile's lanes read contiguous bytes; counted in the call's time) and B OH OW Cout floats (G) for the backward, plus
 * S Cout Cin KH KW floats where the weight gradient is split (below), in the handle; it grows on the first call of a shape,
 * afterwards nothing is allocated and the calls can be captured into a graph.
 * The weight gradient's contraction runs over the B OH output rows.  Where the product has few 32 x 32 tiles and many rows it is
 * cut into S > 1 splits: workgroup (tile, s) sums q = B OH / S contiguous rows, one more where s < r = B OH % S, starting at row
 * s q + min(s, r), into a partial product in the workspace, and a second kernel (profiler name conv_bwd_wgrad_reduce) adds the partials in the order s = 0 .. S - 1.  No atomics.
 * S is a function of the layer's shape alone, never of the device: specmi_conv2d_wgrad_splits returns it (SPECMI_ERR_ARG for a
 * NULL splits, a dimension < 1 or a layer shape that is not built).  S == 1 whenever the product has 256 tiles or more or
 * B OH < 128; S == 1 is one launch writing g_w directly.
 * Refusals (SPECMI_ERR_ARG with a message, nothing launched, no output written): x, w, scale, shift, y (forward) or g_y NULL; every
 * output NULL; y NULL with relu (backward); a layer shape other than the five above; a dimension < 1; a tensor of the layer with
 * 2^31 elements or more; a float pointer that is not 4-byte aligned. */
int specmi_conv2d_wgrad_splits(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* splits);
int specmi_conv2d_train_forward(specmi_handle* h, const float* x, int B, int H, int W, int Cin, const float* w_oihw_dev,
                                const float* scale_dev, const float* shift_dev, int Cout, int KH, int KW, int stride, int pad,
                                const float* residual, int relu, float* y, void* stream);
int specmi_conv2d_backward(specmi_handle* h, const float* x, int B, int H, int W, int Cin, const float* w_oihw_dev,
                           const float* scale_dev, int Cout, int KH, int KW, int stride, int pad, const float* y, int relu,
                           const float* g_y, const float* g_x_add, float* g_x, float* g_w, float* g_res, void* stream);

/* MaxPool2d(3, 2, 1) for training, with its gradient (spec_amd/csrc/pool_bwd.hip; STABLE).  x / g_x (B, H, W, C) and y / g_y
 * (B, OH, OW, C), OH = (H - 1) / 2 + 1, are dense NHWC fp32 on the device; idx (B, OH, OW, C) is one uint8 per output element.
 * Nothing of the handle's committed model is read, no workspace is used, nothing is allocated and the stream is not synchronised:
 * both calls work on a handle of any kind and can be captured into a graph.
 * specmi_maxpool3x3s2_train_forward: the in-range taps of a window are scanned in (ky, kx) ascending order and a tap replaces the
 *   best so far when v > best || isnan(v) (torch's rule): among equal maxima the first tap wins, a padding tap never wins, a NaN
 *   in the window gives NaN.  idx = ky * 3 + kx (0 .. 8) of the tap the scan ends on, y its value: without a NaN in the window
 *   y has the bits of specmi_maxpool3x3s2.
 * specmi_maxpool3x3s2_backward: g_x[b, iy, ix, c] = the sum of g_y over the at most 2 x 2 windows that contain the pixel and whose
 *   idx names it, added in (oy, ox) ascending order in double and rounded once.  Every element of g_x is written exactly once;
 *   pixels that never won get exact zeros.  idx values that name no tap of the window (> 8, or a padding tap) pass no gradient.
 * A lane owns 4 channels as one 16-byte vector where C % 4 == 0, the float tensors are 16-byte aligned and idx 4-byte aligned;
 * otherwise a scalar form gives the same bits.  Deterministic: no atomics, the bits are fixed by the shape, two runs give the
 * same bits and image b's bits do not depend on its batch.
 * Refusals (SPECMI_ERR_ARG with a message, nothing launched, nothing written): a NULL pointer; a dimension < 1; an input of 2^31
 * elements or more; a float pointer that is not 4-byte aligned. */
int specmi_maxpool3x3s2_train_forward(specmi_handle* h, const float* x, int B, int H, int W, int C, float* y, unsigned char* idx,
                                      void* stream);
int specmi_maxpool3x3s2_backward(specmi_handle* h, const float* g_y, const unsigned char* idx, int B, int H, int W, int C,
                                 float* g_x, void* stream);

/* BatchNorm in training mode, with its gradients (spec_amd/csrc/bn_train.hip; STABLE): what nn.BatchNorm2d does in train() after a
 * convolution of a bottleneck, with the block's residual and ReLU,
 *     mean[c] = sum_m z[m, c] / M,  var[c] = sum_m (z[m, c] - mean[c])^2 / M (biased),  invstd = 1 / sqrt(var + eps)
 *     y = (z - mean) invstd gamma + beta (+ residual), and max(., 0) with relu != 0
 * z / y / residual / g_y / g_z / g_res are dense (M, C) fp32 with C contiguous - NHWC with M = B H W - and gamma / beta / mean /
 * invstd / running_mean / running_var / g_gamma / g_beta are (C) vectors; all device pointers, read where torch keeps them.  Nothing
 * of the handle's committed model is read and the stream is not synchronised; both calls work on a handle of any kind, committed
 * or not.  Any M >= 2 and C >= 1 with M C < 2^31: tails in M and C are handled in the kernel and no access leaves a tensor.
 * specmi_batchnorm_train_forward writes y and saves mean and invstd (C) for the backward.  residual may be NULL.  With
 *   running_mean / running_var given (both or neither) they are updated in place by torch's rule with the factor `momentum`
 *   (bn.momentum, or 1 / num_batches_tracked where that is None):
 *     running_mean = (1 - f) running_mean + f mean,   running_var = (1 - f) running_var + f var M / (M - 1)
 *   each evaluated in double from the fp32 values and rounded once, as invstd is: f = 0 leaves their bits, f = 1 replaces them.
 *   The variance is never E[z^2] - E[z]^2: every chunk of rows is centred on its own mean and the chunks are merged by Chan's rule.
 * specmi_batchnorm_backward: the forward's z, gamma, mean, invstd, its output y (read only with relu != 0: may be NULL otherwise)
 *   and g_y ->
 *     g = relu ? (y > 0 ? g_y : 0) : g_y          (the convention of specmi_conv2d_backward: an exact zero passes no gradient)
 *     g_res = g,   g_beta[c] = sum_m g,   g_gamma[c] = sum_m g xhat,   xhat = (z - mean) invstd
 *     g_z = gamma invstd (g - g_beta / M - xhat g_gamma / M)
 *   g_z, g_gamma, g_beta and g_res may be NULL (not wanted), but not all of them; g_res may be g_y itself.
 * Deterministic, the rule of specmi_smpl_backward: no float atomics; the M rows are cut into chunks of SPECMI_BN_ROWS_PER_CHUNK rows
 * (chunk k = rows 64 k ..) and the chunks' partial results are combined in an order fixed by (M, C) alone, never by the device or
 * by what else is wanted: two runs give the same bits and a wanted output has the same bits whatever else is wanted.  Unlike the
 * convolution layer, image b's y and g_z DO depend on the other images of its batch - the statistics are the batch's.
 * Workspace: (2 ceil(M / SPECMI_BN_ROWS_PER_CHUNK) + 2) C floats in the handle; it grows on the first call of a shape, afterwards
 * nothing is allocated and the calls can be captured into a graph.
 * Refusals (SPECMI_ERR_ARG with a message, nothing launched, nothing written): M < 2 (torch refuses one value per channel in
 * training, so does this call); C < 1; M C >= 2^31; z, gamma, beta, y, mean, invstd (forward) or z, gamma, mean, invstd, g_y
 * (backward) NULL; y NULL with relu (backward); every output NULL (backward); eps < 0; momentum outside [0, 1]; exactly one of
 * running_mean / running_var; a float pointer that is not 4-byte aligned. */
#define SPECMI_BN_ROWS_PER_CHUNK 64
int specmi_batchnorm_train_forward(specmi_handle* h, const float* z, int M, int C, const float* gamma, const float* beta,
                                   const float* residual, int relu, float eps, float momentum, float* running_mean,
                                   float* running_var, float* y, float* mean, float* invstd, void* stream);
int specmi_batchnorm_backward(specmi_handle* h, const float* z, int M, int C, const float* gamma, const float* mean,
                              const float* invstd, const float* y, int relu, const float* g_y, float* g_z, float* g_gamma,
                              float* g_beta, float* g_res, void* stream);

/* The frozen part of a fine-tuning step (STABLE): the committed fp32 ResNet trunk's own op list up to the last op of
 * layer{n_stages}, n_stages in 1 .. 4, whose block output goes NHWC to `out` ((B, h, w, C): stride 4, 8, 16, 32 and 256, 512,
 * 1024, 2048 channels for a Bottleneck trunk).  The same kernels, plan and k order as specmi_trunk_forward: with n_stages = 4 `out`
 * has specmi_trunk_forward's bits.  An HRNet trunk and the fp16 trunk are refused with SPECMI_ERR_STATE. */
int specmi_trunk_forward_stages(specmi_handle* h, const float* images_nchw, int B, int H, int W, int n_stages, float* out,
                                void* stream);

/* The body model WITHOUT the 49-joint wrapper - smplx.SMPL.forward as the evaluation code calls it (`smpl_native` /
 * `body_model` / `body_model_orig`, spec/trainer.py:71-86,249-254, spec/utils/compute_error.py:118-160): `pose` is
 * (B,24,3,3) rotation matrices (pose2rot=False) or, with pose_is_axis_angle != 0, (B,72) axis-angle vectors
 * (global_orient | body_pose; smplx batch_rodrigues); outputs vertices (B,V,3) and / or joints24 (B,24,3) =
 * `.joints[:, :24]`, the posed kinematic-chain joints.  Either output may be NULL (not both). */
int specmi_smpl_native(specmi_handle* h, const float* pose, int pose_is_axis_angle, const float* betas, int B,
                       float* vertices, float* joints24, void* stream);

/* A single fused conv+BN(+residual)(+ReLU) layer, y = act(conv(x)*scale + shift [+ res]).
 * x (B,H,W,Cin) NHWC device; w (Cout,Cin,KH,KW) OIHW HOST; scale/shift (Cout) HOST;
 * residual/out (B,OH,OW,Cout) NHWC device.  Cin%32==0 unless (Cin==3,KH==7: stem path,
 * x is then NCHW).  Device pointers 16-byte aligned (the kernels move 16 bytes per lane; a misaligned x is refused by the
 * Winograd path with an error, never read wrongly).  Used by the per-layer parity tests. */
int specmi_conv2d(specmi_handle* h, const float* x, int B, int H, int W, int Cin,
                  const float* w_oihw_host, const float* scale_host, const float* shift_host,
                  int Cout, int KH, int KW, int stride, int pad, const float* residual,
                  int relu, float* out, void* stream);

/* specmi_conv2d with everything the trunks' own launches vary: specmi_conv2d(...) is this call with ldx = Cin, ldo = Cout and
 * no x2, bit for bit.  x is read as (B,H,W) pixels of ldx >= Cin floats of which the first Cin are the channels (the rest are
 * never read); out, and residual if given, as (B,OH,OW) pixels of ldo >= Cout floats of which the first Cout are written
 * (read); nothing else in those rows is touched.  x, out and residual are plain pointers: a channel offset into a wider map
 * (HRNet's concat slices) is the caller's pointer arithmetic.  Optional second A source, the bottleneck's conv3 with its
 * downsample folded in: x2 (B,H2,W2) pixels of ldx2 >= Cin2 floats, read at (oy*stride2, ox*stride2) and concatenated after x
 * along K; w is then (Cout, Cin+Cin2, 1, 1) and the layer 1x1 / stride 1 / pad 0, (OH-1)*stride2 < H2, (OW-1)*stride2 < W2.
 * Refused with SPECMI_ERR_ARG, nothing launched and the handle usable: ldx < Cin, ldo < Cout, an x2 on any other layer, and
 * whatever the kernel that the options select cannot take - the direct kernels need Cin % 32 == 0 (Cin2 too), ldx % 4 == 0
 * (ldx2 too) and 16-byte aligned x (x2); Winograd (3x3 / stride 1 / pad 1, Cin % 16 == 0, Cout % 64 == 0 or Cout % 32 == 0 and
 * Cout > 64) needs an even ldx, x aligned to 8 bytes (16 and ldx % 4 == 0 when Cin % 32 == 0) and 16-byte aligned rows of
 * out / residual (ldo % 4 == 0).  On the direct kernels out and residual need no more than 4-byte alignment and any ldo: rows
 * that are not 16-byte aligned take the scalar epilogue.  The 7x7 stem takes dense tensors only.  Synchronises the stream.
 * Used by the per-layer exactness tests. */
int specmi_conv2d_strided(specmi_handle* h, const float* x, int B, int H, int W, int Cin, int ldx,
                          const float* w_oihw_host, const float* scale_host, const float* shift_host,
                          int Cout, int KH, int KW, int stride, int pad, const float* residual,
                          int relu, float* out, int ldo, const float* x2, int H2, int W2, int Cin2, int ldx2,
                          int stride2, void* stream);

/* One fused layer of the fp16 trunk (conv_f16.hip), as specmi_conv2d is for the fp32 one.  x (B,H,W,Cp) fp16 NHWC device,
 * Cp = Cin rounded up to a multiple of 8 (channels past Cin zero); w (Cout,Cin,KH,KW) OIHW fp32 HOST and scale / shift (Cout)
 * fp32 HOST are folded exactly as specmi_commit folds them: weights fp16_rne(w * scale) from the fp64 product (SPECMI_ERR_ARG
 * if one overflows fp16), shift added in fp32.  residual (B,OH,OW,Cout) fp16 NHWC device or NULL; out (B,OH,OW,Cout) NHWC
 * device, fp16 (out_f32 = 0) or fp32 (out_f32 = 1).  Cout % 4 == 0; device pointers 16-byte aligned.  Optional second A source
 * (the folded downsample): x2 (B,H2,W2,Cin2) fp16 NHWC read at pixel (oy*stride2, ox*stride2) and concatenated after x along
 * K; w is then (Cout, Cin+Cin2, 1, 1), the layer 1x1 / stride 1 and Cin, Cin2 multiples of 32.  Synchronises the stream. */
int specmi_conv2d_f16(specmi_handle* h, const void* x, int B, int H, int W, int Cin,
                      const float* w_oihw_host, const float* scale_host, const float* shift_host,
                      int Cout, int KH, int KW, int stride, int pad, const void* residual, int relu,
                      void* out, int out_f32, const void* x2, int H2, int W2, int Cin2, int stride2, void* stream);

/* MaxPool2d(3,2,1) and global average pool on NHWC device tensors (trunk building blocks). */
int specmi_maxpool3x3s2(specmi_handle* h, const float* x, int B, int H, int W, int C,
                        float* out, void* stream);
int specmi_avgpool(specmi_handle* h, const float* x, int B, int HW, int C, float* out,
                   void* stream);

/* The two small kernels of the fp16 trunk (conv_f16.hip), trunk building blocks as the two above are.  Max-pool: x (B,H,W,C)
 * and out (B,OH,OW,C) fp16 NHWC device, C % 8 == 0, exact (the result is one of the inputs).  Image conversion: x (B,C,H,W) fp32
 * NCHW device, 1 <= C <= 8, out (B,H,W,8) fp16 NHWC device, values rounded to nearest even (|v| >= 65520 becomes inf), channels
 * past C are +0.  Device pointers 16-byte aligned. */
int specmi_maxpool3x3s2_f16(specmi_handle* h, const void* x, int B, int H, int W, int C,
                            void* out, void* stream);
int specmi_to_nhwc_f16(specmi_handle* h, const float* x, int B, int C, int H, int W, void* out,
                       void* stream);

/* One Linear layer of the heads on caller-supplied parameters, through the code the heads run (parity tests): nheads (1..3)
 * layers of one shape, head i with HOST weights w_host[i] (N,K) row-major and bias_host[i] (N), packed and uploaded exactly as
 * specmi_commit packs a Linear layer (K zero padded to Kp = K rounded up to 32) into temporaries that are freed before the
 * call returns.  x[i]: B device rows of ldx floats of which the first Kp are READ (columns K..Kp meet zero weights; they must be
 * readable, their values do not matter as long as they are finite); out[i][b*ldo + n] = w[n] . x[b] + bias[n]
 * (+ residual[i][b*ldo + n]) for n < N; nothing else of out is written.  residual may be NULL (no head has one) and
 * residual[i] may equal out[i].  path 0: the small-batch GEMV kernel, all heads in one launch (an image's sum has a fixed
 * order whatever B is); path 1: the matrix-core GEMM in row blocks of 1024 (option "fc_splitk" applies), one head.  Refused
 * with SPECMI_ERR_ARG and a message, nothing launched: nheads outside 1..3, N, K or B < 1, ldx < Kp, ldx % 4 != 0, ldo < N, an
 * x[i] that is not 16-byte aligned, an out / residual that is not 4-byte aligned, path 1 with more than one head.
 * Synchronises the stream. */
int specmi_fc_forward(specmi_handle* h, int nheads, const float* const* w_host, const float* const* bias_host, int N, int K,
                      const float* const* x, int ldx, const float* const* residual, float* const* out, int ldo, int B, int path,
                      void* stream);

/* The three kernels of the HRNet trunks (hrnet.hip) on their own, through the launchers the trunk itself calls (parity tests).
 * They work on any handle; no HRNet needs to be committed.  All pointers are device pointers, float tensors 16-byte aligned.
 * Bad arguments (NULL, sizes <= 0, C % 4, a pixel stride that is not a multiple of 4 or below C, H or W not divisible by
 * 2^sh[k], n outside 1..4) return SPECMI_ERR_ARG with a message and launch nothing. */

/* The trunk's first layer: 3x3 / stride 2 / pad 1 convolution of the 3-channel NCHW image (B,3,H,W), then
 * ReLU(acc * scale[cout] + shift[cout]), stored NHWC as (B,OH,OW,64) with OH = (H-1)/2+1, OW = (W-1)/2+1.  w holds 27 x 64
 * floats in the kernel's own layout, index ((c*3+ky)*3+kx)*64 + cout; scale and shift hold 64 floats.  Any H, W >= 1. */
int specmi_hr_stem3x3(specmi_handle* h, const float* images_nchw, int B, int H, int W, const float* w, const float* scale,
                      const float* shift, float* out_nhwc, void* stream);

/* The exchange-unit sum: out = [ReLU](((t0 + t1) + t2) + t3) over the first n terms, added in fp32 in exactly that order.
 * Term k is (B, H >> sh[k], W >> sh[k], C) NHWC in pixels of ld[k] floats and is read nearest-upsampled by 2^sh[k]; out is
 * (B,H,W,C) in pixels of ldo floats (ldo > C: a channel slice of a wider map; floats outside the slice are not touched).
 * With n = 1, relu = 0 it is the strided copy into the concat head's slice.  Entries k >= n of the arrays are ignored. */
int specmi_hr_fuse_sum(specmi_handle* h, const float* const terms[4], const int ld[4], const int sh[4], int n, int B, int H, int W,
                       int C, int relu, float* out, int ldo, void* stream);

/* F.interpolate(mode='bilinear', align_corners=True) on NHWC: x (B,H,W,C) in pixels of ld floats -> out (B,OH,OW,C) in pixels
 * of ldo floats.  The source coordinate of output o is o * (in - 1) / (out - 1) along each axis, 0 where out == 1. */
int specmi_hr_resize_ac(specmi_handle* h, const float* x, int B, int H, int W, int C, int ld, float* out, int OH, int OW, int ldo,
                        void* stream);

/* ---- crop + normalise in front of the path ------------------------------------ */

/* The detection loop of spec/tester.py:116-128: for each bbox (cx, cy, w, h) [device, (n,4)]
 * get_single_image_crop_demo(frame, bbox, scale, crop_size) - 3-point affine (rot 0) +
 * cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT) fixed-point bilinear + ToTensor + ImageNet
 * Normalize (spec/constants.py:20-21) - from a uint8 RGB HWC frame in device memory to
 * (n,3,S,S) fp32 NCHW (frames of 4 GiB or more, or with a side of 2^24 pixels, are refused: 32-bit offsets).
 * Optional outputs: raw (n,S,S,3) uint8 crop, bbox_scale = w/200 (n),
 * bbox_center (n,2). */
int specmi_crop_normalize(specmi_handle* h, const uint8_t* frame_rgb_hwc, int H, int W,
                          const float* bboxes, int n, float scale, int crop_size, float* out_nchw,
                          uint8_t* raw_hwc, float* bbox_scale, float* bbox_center, void* stream);

/* The same crops for the detections of MANY frames in one launch - the loop over images of spec/tester.py:109-128 (one
 * frame, its detections, one crop each) flattened: `frames` is a slab of nframes equal-sized uint8 RGB HWC frames in device
 * memory (frame f at frames + f*H*W*3), crop d is cut from frame frame_index[d] (device, (n) int32, values in [0, nframes);
 * the index lives in caller memory the library cannot inspect without a synchronisation: an out-of-range value is CLAMPED into
 * the slab - a wrong crop, never an out-of-bounds read; validate on the host where the index is produced) with bbox d.  Same arithmetic, same outputs per crop as specmi_crop_normalize (bit-identical); what it removes is one
 * launch, one host synchronisation and one small batch per frame. */
int specmi_crop_normalize_batch(specmi_handle* h, const uint8_t* frames_rgb_hwc, int nframes, int H, int W,
                                const int32_t* frame_index, const float* bboxes, int n, float scale, int crop_size,
                                float* out_nchw, uint8_t* raw_hwc, float* bbox_scale, float* bbox_center, void* stream);
/* specmi_crop_normalize_batch with the crops stored as NHWC8 fp16 (n,S,S,8) ("NHWC8 fp16" above) instead of (n,3,S,S) fp32:
 * replaces specmi_crop_normalize[_batch] + specmi_to_nhwc_f16 (the single-frame crop is this call with nframes = 1 and
 * frame_index = NULL, or an all-zero index; a NULL index with nframes > 1 is refused).  raw_hwc, bbox_scale, bbox_center as in the twin.  Refuses what the twin refuses and an out_nhwc8
 * that is not 16-byte aligned (SPECMI_ERR_ARG). */
int specmi_crop_normalize_batch_f16(specmi_handle* h, const uint8_t* frames_rgb_hwc, int nframes, int H, int W,
                                    const int32_t* frame_index, const float* bboxes, int n, float scale, int crop_size,
                                    void* out_nhwc8, uint8_t* raw_hwc, float* bbox_scale, float* bbox_center, void* stream);

/* The evaluation dataset's image path (spec/dataset/cam_dataset.py:253-287 rgb_processing with flip 0 / rot 0 / pn 1, :367-377):
 * pare `crop(img, center, scale, [res, res])` = copy of the integer box [ul, br) (zero outside the frame) scaled to res x res
 * with cv2.resize (bilinear, half-pixel centres, replicated border), clip to [0, 255], float32 / 255, ImageNet Normalize.
 * boxes: (n,4) int32 device [ul_x, ul_y, br_x, br_y] as the reference's `transform(..., invert=1)` yields them (computed on
 * the host: spec_amd.preprocess.pare_crop_boxes); frame uint8 RGB HWC device; out (n,3,S,S) fp32 NCHW. */
int specmi_crop_resize_normalize(specmi_handle* h, const uint8_t* frame_rgb_hwc, int H, int W, const int32_t* boxes, int n,
                                 int crop_size, float* out_nchw, void* stream);
/* specmi_crop_resize_normalize with the crops stored as NHWC8 fp16 (n,S,S,8): replaces it + specmi_to_nhwc_f16.  Refuses
 * what the twin refuses and an out_nhwc8 that is not 16-byte aligned (SPECMI_ERR_ARG). */
int specmi_crop_resize_normalize_f16(specmi_handle* h, const uint8_t* frame_rgb_hwc, int H, int W, const int32_t* boxes, int n,
                                     int crop_size, void* out_nhwc8, void* stream);

/* The crops of specmi_crop_normalize for the detections of MANY frames of DIFFERENT sizes in one launch - what a folder of
 * photographs needs where specmi_crop_normalize_batch (equal-sized frames: video) does not apply; replaces one
 * specmi_crop_normalize launch per frame (spec/tester.py:109-128).  The frames lie in one uint8 RGB HWC device slab of
 * slab_bytes bytes, the slab and offsets convention of specmi_resize_normalize_ragged: frame f starts at byte offsets[f]
 * (HOST, nframes int64; any byte offset, gaps allowed) and is geom[2f] x geom[2f+1] = H x W pixels (HOST, nframes x 2 int32).
 * Crop d is cut from frame frame_index[d] (DEVICE, (n) int32; an out-of-range value is CLAMPED into [0, nframes) as in
 * specmi_crop_normalize_batch - a wrong crop, never an out-of-bounds read; validate on the host where the index is produced)
 * with bbox d (DEVICE, (n,4) float).  Outputs as in specmi_crop_normalize, bit-identical per crop to that call on the crop's frame.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null required pointer (raw_hwc, bbox_scale, bbox_center are optional),
 * n <= 0 or n > 65535, nframes <= 0, H or W below 1 or from 2^24 up, a frame that leaves the slab (negative offset or
 * offset + H*W*3 > slab_bytes), a slab of 4 GiB or more, crop_size < 1, scale <= 0.
 * The per-frame records (offset, H, W) live in one device table owned by the handle and shared by the four ragged crop calls.
 * A call whose records differ from the previous call's rewrites that table and therefore first SYNCHRONISES THE WHOLE DEVICE
 * (crops enqueued earlier, on any stream, may still read it) - the same rule as specmi_resize_normalize_ragged's and
 * specmi_pano_extract_views' tables.  Such a call cannot be made while a stream is being captured (SPECMI_ERR_STATE); a call
 * whose records equal the previous call's does neither. */
int specmi_crop_normalize_ragged(specmi_handle* h, const uint8_t* frames_rgb_hwc, size_t slab_bytes, const int64_t* offsets,
                                 const int32_t* geom, int nframes, const int32_t* frame_index, const float* bboxes, int n,
                                 float scale, int crop_size, float* out_nchw, uint8_t* raw_hwc, float* bbox_scale,
                                 float* bbox_center, void* stream);
/* specmi_crop_normalize_ragged with the crops stored as NHWC8 fp16 (n,S,S,8): replaces it + specmi_to_nhwc_f16.  Refuses what
 * the twin refuses and an out_nhwc8 that is not 16-byte aligned (SPECMI_ERR_ARG). */
int specmi_crop_normalize_f16_ragged(specmi_handle* h, const uint8_t* frames_rgb_hwc, size_t slab_bytes, const int64_t* offsets,
                                     const int32_t* geom, int nframes, const int32_t* frame_index, const float* bboxes, int n,
                                     float scale, int crop_size, void* out_nhwc8, uint8_t* raw_hwc, float* bbox_scale,
                                     float* bbox_center, void* stream);
/* The crops of specmi_crop_resize_normalize for the samples of an evaluation batch whose images differ in size, in one launch:
 * replaces one upload, one specmi_crop_resize_normalize launch of a single crop and one allocation per sample plus the
 * concatenation of the batch (spec/dataset/cam_dataset.py:367-377 under a DataLoader).  Slab, offsets, geom, frame_index, the
 * clamp, the refusals and the table rule as in specmi_crop_normalize_ragged; boxes (DEVICE, (n,4) int32) and out as in
 * specmi_crop_resize_normalize, bit-identical per crop to that call on the crop's frame. */
int specmi_crop_resize_normalize_ragged(specmi_handle* h, const uint8_t* frames_rgb_hwc, size_t slab_bytes, const int64_t* offsets,
                                        const int32_t* geom, int nframes, const int32_t* frame_index, const int32_t* boxes, int n,
                                        int crop_size, float* out_nchw, void* stream);
/* specmi_crop_resize_normalize_ragged with the crops stored as NHWC8 fp16 (n,S,S,8): replaces it + specmi_to_nhwc_f16.  Refuses
 * what the twin refuses and an out_nhwc8 that is not 16-byte aligned (SPECMI_ERR_ARG). */
int specmi_crop_resize_normalize_f16_ragged(specmi_handle* h, const uint8_t* frames_rgb_hwc, size_t slab_bytes, const int64_t* offsets,
                                            const int32_t* geom, int nframes, const int32_t* frame_index, const int32_t* boxes, int n,
                                            int crop_size, void* out_nhwc8, void* stream);

/* The CamCalib frame transform (camcalib/pano_dataset.py:156-162, scripts/camcalib_demo.py:100): torchvision
 * Resize(600) on a PIL image = Pillow's antialiased bilinear resample (Image.resize((OW, OH), BILINEAR): separable
 * triangle filter, 22-bit fixed-point coefficients, uint8 between the passes) + ToTensor + ImageNet Normalize, from a
 * uint8 RGB HWC frame in device memory to (3,OH,OW) fp32; bit-identical to Pillow.  The caller picks (OH, OW)
 * (shorter side 600, longer int(600*long/short)).  Optional raw_hwc: the resized uint8 image (OH,OW,3). */
int specmi_resize_normalize(specmi_handle* h, const uint8_t* frame_rgb_hwc, int H, int W, int OH, int OW,
                            float* out_chw, uint8_t* raw_hwc, void* stream);
/* specmi_resize_normalize with the frame stored as NHWC8 fp16 (OH,OW,8): replaces it + specmi_to_nhwc_f16.  Refuses what the
 * twin refuses and an out_nhwc8 that is not 16-byte aligned (SPECMI_ERR_ARG). */
int specmi_resize_normalize_f16(specmi_handle* h, const uint8_t* frame_rgb_hwc, int H, int W, int OH, int OW,
                                void* out_nhwc8, uint8_t* raw_hwc, void* stream);

/* A CamCalib validation batch (camcalib/pano_dataset.py:184-220 Resize(min_size, max_size) per frame, :223-306 collator /
 * to_image_list): n uint8 RGB HWC frames of DIFFERENT sizes in one device slab -> out (n, 3, Hmax, Wmax) fp32 NCHW.  Frame f
 * (at byte offsets[f], geom[4f .. 4f+3] = H, W, OH, OW; offsets and geom are HOST arrays) is resampled to (OH, OW) with the
 * arithmetic of specmi_resize_normalize, bit for bit, into out[f, :, :OH, :OW]; every other element is exactly 0.0f (zeros in
 * normalised space).  A frame with (OH, OW) == (H, W) is converted without resampling.  The caller picks the target sizes
 * (spec_amd.camcalib_eval.resize_size) and Hmax >= max OH, Wmax >= max OW.  Two launches whatever n is; every output element
 * is written once (no memset).  Refused: n > 65535, a slab of 4 GiB or more, an output plane of 2^31 elements or more. */
int specmi_resize_normalize_ragged(specmi_handle* h, const uint8_t* frames_rgb_hwc, size_t slab_bytes, const int64_t* offsets,
                                   const int32_t* geom, int n, int Hmax, int Wmax, float* out_nchw, void* stream);
/* specmi_resize_normalize_ragged with the batch stored as NHWC8 fp16 (n,Hmax,Wmax,8): replaces it + specmi_to_nhwc_f16.  A
 * pixel outside its frame's (OH, OW) region is 16 bytes of zero (+0 halves: padding stays zero in normalised space); every
 * pixel is written once.  Refuses what the twin refuses and an out_nhwc8 that is not 16-byte aligned (SPECMI_ERR_ARG). */
int specmi_resize_normalize_ragged_f16(specmi_handle* h, const uint8_t* frames_rgb_hwc, size_t slab_bytes, const int64_t* offsets,
                                       const int32_t* geom, int n, int Hmax, int Wmax, void* out_nhwc8, void* stream);

/* Labelled perspective views out of an equirectangular panorama - the per-pixel work of the reference's dataset generator,
 * extractImage's mode="image" branch (camcalib/datagen/image_extraction.py:129-159, called by makeAndSaveImg,
 * camcalib/datagen/generateCalibrationDataset.py:122-126): n views of DIFFERENT sizes cut from ONE uint8 RGB HWC panorama in
 * device memory in one launch.  views (HOST, n x 5 doubles): elevation, azimuth, roll in radians, vfov in degrees, ratio =
 * width / height; out_hw (HOST, n x 2): height and width of view f, the width being round(height / (1 / ratio)) with
 * Python's round (a mismatch is refused); view f is written as uint8 HWC at out_slab + offsets[f] (HOST offsets, the slab
 * and offsets convention of specmi_resize_normalize_ragged, whose input this is).  Bytes of the slab between views are not
 * touched.  Per pixel, in fp64: numpy.linspace grid, roll in the image plane, inverse gnomonic projection with the
 * reference's rho + 1e-10, the two +-2 pi wraps, the reference's pixel maps, then
 * scipy.ndimage.map_coordinates(order=1, prefilter=False, mode="wrap") as scipy computes it (period N - 1) and scipy's
 * uint8 store.  Differs from the reference only where the last ulp of the device's asin / atan2 moves a value across a
 * rounding tie.  Refused (SPECMI_ERR_ARG): a null pointer, n <= 0 or > 65535, a size below 1, a non-finite view parameter,
 * vfov outside (0, 180), ratio <= 0, a view that leaves the slab.
 * The per-view records live in one device table owned by the handle.  A call whose views or sizes differ from the previous
 * call's rewrites that table and therefore first SYNCHRONISES THE WHOLE DEVICE (an extraction enqueued earlier, on any stream,
 * may still read it) - in practice once per panorama; the same rule as specmi_resize_normalize_ragged's tables.  Such a call
 * cannot be made while a stream is being captured (SPECMI_ERR_STATE); a call that repeats the previous views does neither. */
int specmi_pano_extract_views(specmi_handle* h, const uint8_t* pano_rgb_hwc, int PH, int PW, const double* views,
                              const int32_t* out_hw, const int64_t* offsets, size_t slab_bytes, uint8_t* out_slab, int n,
                              void* stream);

/* ---- the demo's pictures ------------------------------------------------------------------------ */

#define SPECMI_RENDER_SIDE_VIEW 1           /* the 270 degree turn about y, black background (renderer_cam.py:82-85,197,207) */
#define SPECMI_RENDER_GROUND_PLANE 2        /* side view only: the checker plane through the lowest vertex (:98-107) */
#define SPECMI_RENDER_CULL 4                /* draw only the faces an outward-wound closed mesh shows */
#define SPECMI_RENDER_THREAD_PER_TRIANGLE 8 /* one thread instead of one wavefront per triangle: the same bits (measurement) */

/* The mesh overlay / side view of the M detections of ONE frame, rasterised on the device: replaces one pyrender / OpenGL
 * OffscreenRenderer.render per detection and panel (spec/utils/renderer_cam.py:44-144 render_overlay_image, called by
 * render_image_group :181-208 from spec/tester.py:191-201) and the device-to-host copy of the vertices that precedes it.
 * Works on a handle of any model kind, committed or not.  DEVICE pointers: vertices (M,V,3) fp32, faces (F,3) int32, cam_t
 * (M,3) fp32 (pred_cam_t), R (3,3) fp32 row-major (the render rotation of tester.py:169-171), frame and out (H,W,3) uint8 RGB,
 * and the optional outputs id_map (H,W) int32 = m*F+f of the visible face, -1 where nothing is drawn, -2 on the ground
 * plane; depth (H,W) fp32 = camera-space z, 0 where nothing is drawn (renderer_cam.py:141 tests rend_depth > 0); screen
 * (M,V,3) 4-byte words = the vertex stage's snapped x and y as int32 in 1/256 pixel (INT32_MIN for a dropped vertex) and z as
 * fp32.  HOST: rgb, 3 floats in [0, 1] (clamped).  frame may be NULL in side view (it is not read); out may be frame.
 * The camera is pyrender's IntrinsicsCamera(fx, fy, cx, cy): x_s = cx + fx X / Z, pixel (i, j) centred at (j + 0.5, i + 0.5).
 * The rasterisation contract - vertex stage, 1/256-pixel snapping, int64 edge functions with the top-left rule, culling,
 * perspective-correct fp32 depth resolved by one 64-bit atomicMin per covered pixel (order-free; ties to the lower id), integer
 * normal sums, this project's own shading min(1, 0.3 + 0.7 max(0, n.l)) and its own analytic ground plane - is stated at the
 * head of spec_amd/csrc/render.hip and restated on the CPU in tests/render_ref.py.  A triangle with a vertex at Z <= 0.05 or
 * at 2^20 pixels or more from the origin is dropped whole: THERE IS NO CLIPPING.  A face index outside [0, V) drops the face.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null required pointer (frame is required without SIDE_VIEW), an unknown
 * flag, GROUND_PLANE without SIDE_VIEW, M, V or F below 1, M*F or 3*M*V of 2^31 or more, H or W outside [1, 32768], a focal
 * length that is not positive and finite, a centre or colour that is not finite.
 * The depth keys (8 bytes per pixel), snapped vertices and normal sums (12 bytes per vertex each) live in one workspace owned
 * by the handle: calls on one handle are ordered on one stream at a time, and a call that needs a larger workspace first
 * SYNCHRONISES THE WHOLE DEVICE and cannot be made while a stream is being captured (SPECMI_ERR_STATE). */
int specmi_render_meshes(specmi_handle* h, const float* vertices, int M, int V, const int32_t* faces, int F, const float* cam_t,
                         const float* R, float fx, float fy, float cx, float cy, const uint8_t* frame_rgb_hwc, int H, int W,
                         const float* rgb, int flags, uint8_t* out_rgb_hwc, int32_t* id_map, float* depth, void* screen,
                         void* stream);

/* MANY VIEWS IN ONE CALL: the pictures of a flush of frames of DIFFERENT sizes - replaces two specmi_render_meshes calls, one
 * upload, one concatenation and one download per frame (the loop of spec/tester.py:165-201).  A VIEW is what one
 * specmi_render_meshes call draws: one camera, one output rectangle, a contiguous range of the call's meshes.  DEVICE pointers:
 * vertices (Mtot,V,3) fp32, cam_t (Mtot,3) fp32, faces (F,3) int32 - one face table and one V for the whole call.  HOST: rgb, 3
 * floats in [0, 1] (clamped).  The frames lie in one uint8 device slab of in_slab_bytes (the slab and offsets convention of
 * specmi_crop_normalize_ragged: what spec_amd.preprocess.pack_frames builds is valid input; in_slab may be NULL when no view
 * names a frame), the outputs go into one uint8 device slab of out_slab_bytes; the two must not overlap.
 * THE VIEW RECORD, three HOST arrays with one row per view:
 *   view_geom    (nviews x 5 int32):  H, W, mesh0, count, flags (SPECMI_RENDER_* above)
 *   view_offsets (nviews x 4 int64):  in_offset (-1 = no frame, legal only with SIDE_VIEW), in_pitch, out_offset, out_pitch -
 *                                     byte offsets into the two slabs and bytes from one row of the view to the next (>= 3 W),
 *                                     so that a view can be written straight into its column of a three-panel picture
 *   view_cams    (nviews x 13 float): R (3,3) row-major, fx, fy, cx, cy
 * View v draws meshes mesh0 .. mesh0 + count - 1; the ranges of different views may overlap (a frame's overlay and side view
 * name the same meshes).  count == 0 is legal: such a view copies its frame rectangle (black in side view) - how panel 0 of a
 * picture is written; GROUND_PLANE with count == 0 is refused.  THREAD_PER_TRIANGLE names the call's one raster launch: it is
 * set on every view or on none.
 * Optional outputs (DEVICE, NULL for none): id_map (int32) and depth (fp32) with the views back to back, view v at the sum of
 * H * W over the views before it; screen with the (view, mesh of the view) pairs back to back in view order, V x 3 words each.
 * CONTRACT: every view equals, bit for bit, what specmi_render_meshes writes when called with that view's arguments on a
 * count >= 1 range - every byte of its output rectangle, every element of its id_map, depth and screen part.  Ids are m F + f
 * with m counted from the view's mesh0; the ground plane lies through the lowest vertex of the view's own meshes and is
 * anchored to the view's first mesh.  Bytes of the output slab outside every view's rectangle are not touched.
 * One launch per stage - vertex, raster, resolve - and two memsets, whatever nviews is (spec_amd/csrc/render.hip).
 * Refused (SPECMI_ERR_ARG), launching nothing: a null required pointer; nviews <= 0 or > 65535; V or F below 1; a mesh range
 * outside [0, Mtot]; count * F or 3 * count * V of a view, or the same products of the counts summed over the views, of 2^31 or
 * more; 2^31 pixels or more in all; H or W outside [1, 32768]; a pitch below 3 W; a view rectangle that leaves its slab; a slab
 * of 4 GiB or more; overlapping slabs; two views whose output rectangles share a byte; an unknown flag; GROUND_PLANE without
 * SIDE_VIEW or with count == 0; in_offset < 0 without SIDE_VIEW; THREAD_PER_TRIANGLE on some views only; a focal length that
 * is not positive and finite; a centre, colour or R entry that is not finite.
 * The view records live in one device table owned by the handle, under the rule of the ragged calls above: a call whose
 * records differ from the previous call's rewrites the table and therefore first SYNCHRONISES THE WHOLE DEVICE, and cannot be
 * made while a stream is being captured (SPECMI_ERR_STATE; the stream is asked first, so the capture stays valid and nothing is
 * enqueued); a call that repeats the previous records does neither and can be captured.  The
 * workspace is specmi_render_meshes' (one per handle, growth synchronises the device): 8 bytes of depth key per pixel of
 * every view with count >= 1, and 24 bytes of snapped vertex and normal sum per vertex of every (view, mesh) pair. */
int specmi_render_views(specmi_handle* h, const float* vertices, int Mtot, int V, const int32_t* faces, int F, const float* cam_t,
                        const float* rgb, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                        const int32_t* view_geom, const int64_t* view_offsets, const float* view_cams, int nviews,
                        int32_t* id_map, float* depth, void* screen, void* stream);

/* How specmi_draw_skeletons paints.  NULL for the style means these defaults. */
typedef struct specmi_draw_style {
    int32_t radius;          /* of a joint's disc in pixels, 0 .. 64; default 4 */
    int32_t thickness;       /* of a bone in pixels, 1 .. 64; default 2 */
    float conf_thr;          /* D == 3: a keypoint is visible when conf > conf_thr (fp32); finite; default 0.3f */
    uint8_t joint_rgb[3];    /* default 0, 255, 0 */
    uint8_t bone_rgb[2][3];  /* bone b takes bone_rgb[b & 1]; defaults 0, 0, 255 (even) and 255, 0, 0 (odd) */
} specmi_draw_style;

/* 2D KEYPOINT SKELETONS painted in place into the uint8 frames of a slab, all frames of a flush in ONE launch: replaces
 * pare.utils.vis_utils.draw_skeleton (cv2.circle / cv2.line on a host image) as render_image_group calls it before the mesh
 * is laid over the frame (spec/utils/renderer_cam.py:159,167-168; spec/trainer.py:219,418), and the device-to-host copy of the
 * keypoints and host-to-device copy of the frame around it.  pare and cv2 are not vendored: coverage, bone table and colours
 * are THIS PROJECT'S OWN CONTRACT, exact and bit-reproducible; cv2's look is not claimed.  Works on a handle of any model kind,
 * committed or not.
 * DEVICE pointers: kp (Mtot, J, D) fp32 with D = 2 (x, y) or 3 (x, y, confidence), in pixels of the detection's frame;
 * slab, uint8, of slab_bytes - the slab and offsets convention of specmi_render_views: what spec_amd.preprocess.pack_frames
 * builds is valid, and so is the panel-0 column of a three-panel picture (pitch 9 W).  HOST: bones (NB x 2 int32 joint
 * indices; may be NULL when NB == 0), style, and the FRAME RECORD, two arrays with one row per frame:
 *   frame_geom    (nframes x 4 int32):  H, W, det0, count - the frame holds detections det0 .. det0 + count - 1 of kp;
 *                                       count == 0 is legal and leaves the frame untouched
 *   frame_offsets (nframes x 2 int64):  byte offset of the frame's first pixel in the slab, bytes from one row to the next
 *                                       (pitch >= 3 W)
 * THE CONTRACT in brief (stated in full at the head of spec_amd/csrc/draw.hip, restated in NumPy in tests/draw_ref.py):
 * a keypoint is visible when x and y are finite, D == 2 or conf > conf_thr, and (int)x, (int)y (truncation) lie in
 * [-16383, 16383]; nothing is clipped, a primitive with an invisible keypoint is not drawn.  Per frame, painter's order: for
 * each detection in turn the J discs in joint order, then the NB bones in table order; later overwrites earlier.  Pixel
 * (px, py) sits at its integer coordinate (no + 0.5).  A disc covers it iff (px - xi)^2 + (py - yi)^2 <= r^2; a bone iff its
 * distance to the closed segment is at most t / 2, decided exactly in 64-bit integers (sides up to 8192 keep every term below
 * 2^63).  Colours are uint8 RGB overwrite: no blending, no antialiasing.  Uncovered pixels, row padding and slab bytes outside
 * every frame rectangle are not touched; no pixel is read; the result does not depend on scheduling.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null required pointer; nframes outside [1, 65535]; J < 1; D not 2 or 3;
 * Mtot < 0; NB < 0, or NB > 0 with bones NULL; a bone index outside [0, J); Mtot * (J + NB) or Mtot * J * D of 2^31 or more;
 * radius outside [0, 64]; thickness outside [1, 64]; a non-finite conf_thr; H or W outside [1, 8192]; a detection range outside
 * [0, Mtot]; a pitch below 3 W; a frame rectangle that leaves the slab; two frames that share a byte.
 * The frame records and the bone table live in one device table owned by the handle, under the rule of the ragged calls above:
 * a call whose records or bones differ from the previous call's rewrites the table and therefore first SYNCHRONISES THE WHOLE
 * DEVICE, and cannot be made while a stream is being captured (SPECMI_ERR_STATE; the stream is asked first, so the capture
 * stays valid and nothing is enqueued); a call that repeats them does neither and can be captured.  The style and the pointers
 * are not part of the table. */
int specmi_draw_skeletons(specmi_handle* h, const float* kp, int Mtot, int J, int D, const int32_t* bones, int NB,
                          const specmi_draw_style* style, uint8_t* slab, size_t slab_bytes, const int32_t* frame_geom,
                          const int64_t* frame_offsets, int nframes, void* stream);

/* HORIZON LINES AND CAPTIONS drawn in place into the uint8 frames of a slab, all frames of a flush in ONE launch: replaces
 * show_horizon_line (camcalib/vis_utils.py:63-110: a black caption strip, ImageDraw.text, ImageDraw.line on a host image) as
 * render_image_group calls it for panel 0 (spec/utils/renderer_cam.py:170-173) and as CamCalib's save_images calls it twice per
 * validation picture (camcalib/trainer.py:118-169), and the copies of the frame to the host and back around it.  The contract
 * is PILLOW'S, byte for byte (stated in full at the head of spec_amd/csrc/marks.hip, restated in NumPy in tests/marks_ref.py
 * and pinned there against the installed Pillow).  Works on a handle of any model kind, committed or not.
 * DEVICE pointers: slab, uint8 RGB, of slab_bytes - the slab and offsets convention of specmi_draw_skeletons: what
 * spec_amd.preprocess.pack_frames builds, or the panel-0 column of a three-panel picture (pitch 9 W); masks, uint8, of
 * mask_bytes: the coverage masks the mask blends name (may be NULL when no mark is a mask blend).  HOST: the FRAME RECORD,
 *   frame_geom    (nframes x 4 int32):  H, W, mark0, count - the frame takes marks mark0 .. mark0 + count - 1 in that order;
 *                                       count == 0 is legal and leaves the frame untouched
 *   frame_offsets (nframes x 2 int64):  byte offset of the frame's first pixel in the slab, bytes from one row to the next
 * and THE MARK RECORD, marks (nmarks x 8 int64): kind, colour as r | g << 8 | b << 16, and six parameters p0 .. p5:
 *   SPECMI_MARK_STRIP: p0 = y0, p1 = y1 - rows [y0, y1) n [0, H) are set to the colour
 *   SPECMI_MARK_MASK:  p0 = x, p1 = y, p2 = mw, p3 = mh, p4 = byte offset in masks - the mw x mh mask with its top-left corner
 *                      at (x, y), clipped to the frame, blended with the colour as Pillow's ImagingFill2 does for a mode L mask:
 *                      per channel, where the mask byte m != 0, t = in * (255 - m) + ink * m + 128, out = ((t >> 8) + t) >> 8;
 *                      a pixel under m == 0 is not written
 *   SPECMI_MARK_LINE:  p0 .. p3 = x0, y0, x1, y1, p4 = width - Pillow's ImagingDrawWideLine, overwriting: the quadrilateral's
 *                      edges come from hypot and Pillow's two rounding macros in double on the host; a row is covered from
 *                      RU(min xx) to RD(max xx) over its edges' xx = (float)(y - ey0) * edx + (float)ex0, a separately rounded
 *                      fp32 multiply and add
 * Unused parameters are ignored.  A pixel's final value is decided by walking its frame's marks in order: no atomics, nothing
 * depends on scheduling.  Pixels that no mark covers, row padding and slab bytes outside every frame rectangle are never
 * written.  Work follows the area the marks can reach (tiles of 64 x 16 pixels listed on the host), not the frames' sizes.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null required pointer (marks with nmarks > 0, masks with a mask blend);
 * nframes outside [1, 65535]; nmarks < 0; H or W outside [1, 8192]; a pitch below 3 W; a frame rectangle that leaves the slab;
 * two frames that share a byte; a mark range outside [0, nmarks]; an unknown kind; a colour outside 24 bits; a width outside
 * [2, 64] (width 1 is Pillow's Bresenham line: not drawn here); a line end point outside [-100000, 100000] - the range pinned
 * against Pillow; mw or mh outside [1, 8192]; a mask position outside [-16383, 16383]; a mask that leaves the mask buffer; marks that reach 2^30
 * tiles or more.
 * The frame records, the marks and the tile list live in one device table owned by the handle, under the rule of the ragged
 * calls above: a call whose records differ from the previous call's rewrites the table and therefore first SYNCHRONISES THE
 * WHOLE DEVICE, and cannot be made while a stream is being captured (SPECMI_ERR_STATE; the stream is asked first, so the
 * capture stays valid and nothing is enqueued); a call that repeats them does neither and can be captured.  The contents of
 * the mask buffer and the pointers are not part of the table. */
#define SPECMI_MARK_STRIP 0
#define SPECMI_MARK_MASK 1
#define SPECMI_MARK_LINE 2
int specmi_draw_marks(specmi_handle* h, uint8_t* slab, size_t slab_bytes, const int32_t* frame_geom, const int64_t* frame_offsets,
                      int nframes, const int64_t* marks, int nmarks, const uint8_t* masks, size_t mask_bytes, void* stream);

/* ONE IMAGE OF A NORMALISED BATCH AS A uint8 FRAME: image `index` of x (B, 3, Hp, Wp) fp32 NCHW on the device, cut to its top-left
 * H x W, written as HWC uint8 at byte `offset` and `pitch` of a slab - the base of CamCalib's validation pictures
 * (camcalib/trainer.py:118-133: pare's denormalize_images, * 255, astype('uint8'), the crop to the image's own resized size).
 * Per channel v = (x * std_c + mean_c) * 255, every operation rounded separately in fp32; NaN gives 0, v is clamped to
 * [0, 255] - the reference's astype('uint8') is undefined outside it: this project's stated deviation - and truncated.
 * mean3 / std3: three HOST floats each, NULL = ImageNet's (0.485, 0.456, 0.406) / (0.229, 0.224, 0.225); pare is not vendored,
 * its denormalize_images is restated with these constants and parity with it is not pinned.
 * Refused (SPECMI_ERR_ARG): a null x or slab; B < 1; Hp or Wp outside [1, 32768]; index outside [0, B); H outside [1, Hp] or W
 * outside [1, Wp]; a pitch below 3 W; a rectangle that leaves the slab; a non-finite mean or std.  Works on a handle of any
 * model kind, committed or not; one launch, nothing synchronised. */
int specmi_denormalize_u8(specmi_handle* h, const float* x, int B, int Hp, int Wp, int index, int H, int W, const float* mean3,
                          const float* std3, uint8_t* slab, size_t slab_bytes, int64_t offset, int64_t pitch, void* stream);

/* TORCHVISION'S ColorJitter on the uint8 RGB frames of a slab, every frame with its own order and factors, in at most TWO kernel
 * launches per call: the one step by which CameraRegressorDataset(is_train=True) differs from the validation half
 * (camcalib/pano_dataset.py:62-78), so that training frames stay where specmi_jpeg_decode / specmi_png_decode /
 * specmi_pano_extract_views left them and specmi_resize_normalize_ragged reads them.  The contract is PILLOW'S, byte for byte
 * (stated in full at the head of spec_amd/csrc/color_jitter.hip, restated in NumPy in tests/color_jitter_ref.py and pinned
 * there against the installed Pillow).  Works on a handle of any model kind, committed or not.
 * DEVICE pointers: in_slab / out_slab, uint8 RGB, of in_slab_bytes / out_slab_bytes.  HOST:
 *   frame_geom    (nframes x 2 int32):  H, W
 *   frame_offsets (nframes x 4 int64):  byte offset of the frame's first pixel and bytes from one row to the next, in in_slab,
 *                                       then the same two in out_slab
 *   records       (nframes x 8 int32):  THE JITTER RECORD - the ids of the operations in application order, -1 = none
 *                                       (SPECMI_JITTER_BRIGHTNESS / _CONTRAST / _SATURATION / _HUE); the bit patterns of the fp32
 *                                       factors of brightness, contrast and saturation (read even where the operation is
 *                                       absent: write 1.0f); the hue shift k = trunc(hue * 255) mod 256
 * Each operation works on the uint8 result of the one before it.  blend(d, v, a) = clamp-and-truncate of float(d) + a *
 * float(v - d), product and sum rounded to fp32 separately.  Brightness: blend(0, v, f).  Saturation: blend(L, v, f) with
 * L = (19595 r + 38470 g + 7471 b + 32768) >> 16.  Contrast: blend(m, v, f), m = int(S / (H W) + 0.5) in float64 with S the
 * 64-bit integer sum of L over the frame as it stands when contrast is reached.  Hue: Pillow's RGB -> HSV, h + k mod 256,
 * HSV -> RGB.  A stat launch sums L for the frames whose order holds contrast (integer atomics: nothing depends on scheduling; a
 * memset node zeroes the sums in front of it), an apply launch writes every pixel once; without contrast anywhere the call
 * is the apply launch alone.  In place - out_slab == in_slab and every frame's two rectangles the same - gives the bytes
 * out of place gives.  Row padding and slab bytes outside every output rectangle are never written.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null pointer; nframes outside [1, 65535]; H or W outside [1, 8192]; a pitch
 * below 3 W; a rectangle that leaves its slab; two frames that share an output byte; slabs that overlap without being in
 * place as above; an id outside [-1, 3] or named twice; a factor that is negative or not finite; k outside [0, 255]; frames that
 * hold 2^31 tiles of 256 x 16 pixels or more.
 * The frame records live in a device table owned by the handle and the sums in a workspace next to it, under the rule of the
 * ragged calls above: a call whose records differ from the previous call's rewrites the table and therefore first
 * SYNCHRONISES THE WHOLE DEVICE, and cannot be made while a stream is being captured (SPECMI_ERR_STATE; the stream is asked
 * first, so the capture stays valid and nothing is enqueued); a call that repeats them does neither and can be captured.  The
 * pointers are not part of the table. */
#define SPECMI_JITTER_BRIGHTNESS 0
#define SPECMI_JITTER_CONTRAST 1
#define SPECMI_JITTER_SATURATION 2
#define SPECMI_JITTER_HUE 3
int specmi_color_jitter(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                        const int32_t* frame_geom, const int64_t* frame_offsets, const int32_t* records, int nframes, void* stream);

/* BASELINE JPEG FILES encoded on the device, all pictures of a flush in one fixed sequence of launches: replaces the download
 * of the raw pictures and the host encoder behind every picture the flows write (cv2.imwrite / PIL's save in
 * spec/utils/renderer_cam.py:213-216, spec/tester.py:188-201, camcalib/datagen/generateCalibrationDataset.py:131-132) - the
 * encoded bytes come down instead, and the host only writes files.  Works on a handle of any model kind, committed or not.
 * DEVICE pointers: in_slab, uint8 RGB, of in_slab_bytes - the slab and offsets convention of specmi_render_views: its output
 * slab (three-panel pictures at pitch 9 W) is valid input, and so is what spec_amd.preprocess.pack_frames builds; out_slab,
 * uint8, of out_slab_bytes, which must not overlap in_slab; sizes (n int64).  HOST: THE PICTURE RECORD, two arrays with one
 * row per picture:
 *   pic_geom    (n x 2 int32):  H, W
 *   pic_offsets (n x 4 int64):  in_offset (byte offset of the picture's first pixel in in_slab), in_pitch (bytes from one row
 *                               to the next, >= 3 W), out_offset (where its file begins in out_slab), out_capacity (bytes it
 *                               may take there)
 * and ONE quality (1 .. 100) for the call.
 * THE CONTRACT (stated in full at the head of spec_amd/csrc/jpeg.hip, restated in NumPy in tests/jpeg_ref.py): picture i's file
 * is, byte for byte, what PIL.Image.fromarray(a).save(f, format='JPEG', quality=q, optimize=False, progressive=False) writes on
 * a libjpeg-turbo build of Pillow - baseline sequential, 4:2:0, the Annex-K Huffman tables, no restart markers; quality 75 is a
 * plain .save(path).  sizes[i] ALWAYS receives the file's true length.  A picture whose length exceeds its capacity has nothing
 * written at or beyond out_offset + out_capacity and is otherwise unspecified; the call still returns SPECMI_OK: the caller reads
 * sizes and encodes that picture again with enough room.  Bytes of out_slab outside [out_offset, out_offset + sizes[i]) of the
 * pictures that fit are not touched.  The result does not depend on scheduling.
 * One memset and seven launches, whatever n and the picture sizes are.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null pointer; n outside [1, 65535]; quality outside [1, 100]; H or W outside
 * [1, 32768]; a pitch below 3 W; a picture rectangle that leaves in_slab; a capacity below the header's 623 bytes; an output
 * range that leaves out_slab; overlapping slabs; two output ranges that share a byte; more than 2^24 blocks of 16 x 16 pixels in
 * all.
 * The picture records and the quality's tables (header, divisors, Huffman codes, built on the host) live in one device table
 * owned by the handle, under the rule of the ragged calls above: a call whose records or quality differ from the previous
 * call's rewrites the table and therefore first SYNCHRONISES THE WHOLE DEVICE, and cannot be made while a stream is being
 * captured (SPECMI_ERR_STATE; the stream is asked first, so the capture stays valid and nothing is enqueued); a call that
 * repeats them does neither and can be captured.  The workspace is one per handle (growth synchronises the device): 7.9 bytes
 * per pixel of the pictures rounded up to whole 16 x 16 blocks - 768 bytes of coefficients, 1248 of unstuffed scan (its worst
 * case) and 4 of bit count per block - plus 12 bytes per chunk of 256 blocks or 4096 scan bytes and 8 per picture. */
int specmi_jpeg_encode(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                       const int32_t* pic_geom, const int64_t* pic_offsets, int n, int quality, int64_t* sizes, void* stream);

/* The 623 header bytes of such a file - SOI, APP0 (JFIF 1.01), two DQT, SOF0, four DHT, SOS - for a quality and a size, into
 * `out` (HOST, of `capacity` >= 623 bytes).  Host only: needs no handle and no device.  SPECMI_ERR_ARG for a null pointer, a
 * quality outside [1, 100], H or W outside [1, 32768] or a capacity below 623. */
int specmi_jpeg_header(int quality, int H, int W, uint8_t* out, size_t capacity);

/* PNG FILES encoded on the device, all pictures of a flush in one fixed sequence of launches: the same service as
 * specmi_jpeg_encode for the pictures of .png frames (spec/tester.py:95 accepts them and :188-201 keeps the frame's extension;
 * camcalib/pano_preprocessing.py:354 writes a tree of them) - the file's bytes come down instead of the raw picture, and zlib
 * does not run on a host thread.  Every convention is specmi_jpeg_encode's: the slabs (DEVICE; in_slab uint8 RGB, the output
 * slab of specmi_render_views and what spec_amd.preprocess.pack_frames builds are valid input; out_slab must not overlap it),
 * THE PICTURE RECORD (HOST) pic_geom (n x 2 int32: H, W) and pic_offsets (n x 4 int64: in_offset, in_pitch, out_offset,
 * out_capacity), sizes (n int64, DEVICE); a handle of any model kind, committed or not.  There is no quality: PNG is lossless.
 * THE CONTRACT (stated in full at the head of spec_amd/csrc/png.hip, restated in NumPy and plain Python in tests/png_ref.py):
 * picture i's file is a valid PNG file - signature, IHDR (8 bit, colour type 2, no interlace), ONE IDAT holding one zlib stream
 * (78 01, deflate, the Adler-32 of the filtered stream), IEND, every CRC-32 correct and computed on the device like the Adler-32 -
 * that decodes to exactly the picture.  Its bytes are NOT zlib's or Pillow's (only the first 33 are); they are fixed by the
 * stated rules and depend on that picture alone, not on its neighbours in the call, on grouping or on scheduling: per row the
 * filter 0 .. 4 with the smallest sum of absolute signed bytes; the filtered stream cut into segments of 32768 bytes, each coded
 * on its own as one dynamic-Huffman block of literals and matches at distances 1 and 3 followed by an empty stored block, or as
 * one stored block where that is not shorter.  No file is longer than specmi_png_bound.
 * sizes[i] ALWAYS receives the file's true length.  A picture whose length exceeds its capacity has nothing written at or beyond
 * out_offset + out_capacity and is otherwise unspecified; the call still returns SPECMI_OK: the caller reads sizes and encodes
 * that picture again with enough room - never needed where the capacity is specmi_png_bound.  Bytes of out_slab outside
 * [out_offset, out_offset + sizes[i]) of the pictures that fit are not touched.
 * One memset and five launches, whatever n and the picture sizes are.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null pointer; n outside [1, 65535]; H or W outside [1, 32768]; a pitch below
 * 3 W; a picture rectangle that leaves in_slab; a capacity below the fixed overhead of 63 bytes (signature, the chunks' frames,
 * zlib's header and checksum); an output range that leaves out_slab; overlapping slabs; two output ranges that share a byte; a
 * picture whose zlib stream with every segment stored does not fit one IDAT chunk (2^31 bytes or more); more than 2^23 segments
 * in all (256 GiB of filtered stream: a launch has a workgroup per segment).  The number of rows is not limited beyond n x H.
 * The picture records live in a device table owned by the handle, under the rule of specmi_jpeg_encode: a call whose records
 * differ from the previous call's rewrites the table and therefore first SYNCHRONISES THE WHOLE DEVICE, and cannot be made while
 * a stream is being captured (SPECMI_ERR_STATE; the stream is asked first, so the capture stays valid and nothing is enqueued);
 * a call that repeats them does neither and can be captured.  The workspace is one per handle (growth synchronises the device):
 * the filtered streams, H (1 + 3 W) bytes per picture rounded up to 256, and 32824 bytes per segment. */
int specmi_png_encode(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                      const int32_t* pic_geom, const int64_t* pic_offsets, int n, int64_t* sizes, void* stream);

/* The length no file of specmi_png_encode for an (H, W) picture exceeds, into *bytes: 63 + L + 5 ceil(L / 32768) with
 * L = H (1 + 3 W) - signature, chunks, the zlib wrapper, and every segment stored.  Host only: needs no handle and no device.
 * SPECMI_ERR_ARG for a null pointer or H or W outside [1, 32768]. */
int specmi_png_bound(int H, int W, int64_t* bytes);

/* The 33 bytes such a file begins with - the signature and IHDR with its CRC - into `out` (HOST, of `capacity` >= 33 bytes).
 * Host only.  SPECMI_ERR_ARG for a null pointer, H or W outside [1, 32768] or a capacity below 33. */
int specmi_png_header(int H, int W, uint8_t* out, size_t capacity);

/* BASELINE JPEG FILES decoded on the device, all files of a call together: the read side of specmi_jpeg_encode.  Replaces the
 * host decode (PIL's Image.open(path).convert('RGB')) and the upload of the raw frames in front of every flow that reads .jpg
 * frames - the files' bytes go up instead, 10 to 20 times fewer.
 * THE CONTRACT (stated in full at the head of spec_amd/csrc/jpeg_dec.hip, restated in NumPy in tests/jpeg_dec_ref.py): for a
 * SUPPORTED file the (H, W, 3) uint8 RGB picture equals np.array(Image.open(f).convert('RGB')) on a libjpeg-turbo build of
 * Pillow, element for element: libjpeg's islow IDCT, fancy 4:2:0 upsampling and 16-bit fixed-point colour conversion.
 *
 * specmi_jpeg_probe: host only, needs no handle and no device.  Parses the markers of `file` (HOST, `bytes` long) and says
 * whether specmi_jpeg_decode takes it: *reason receives SPECMI_JPEG_SUPPORTED or why not, *H and *W the picture's size and
 * *sampling 420 or 444 (all three 0 when not supported).  SUPPORTED is: one SOF0 with 8-bit samples; three
 * components, YCbCr; sampling 2x2,1x1,1x1 or 1x1,1x1,1x1; one interleaved scan (Ss 0, Se 63, Ah/Al 0); 8-bit quantisation
 * tables; Huffman tables from the file's own DHT segments, ids 0 and 1; no DRI with a non-zero interval; H and W in [1, 32768];
 * no Adobe APP14 segment and not the component ids 'R','G','B' without JFIF; EOI as the last two bytes.  The reasons:
 *   NOT_JPEG (no SOI, bytes that are no marker)   TRUNCATED (the header or the EOI is cut off)   PROGRESSIVE (SOF2)
 *   SOF (any other frame type, a second frame)    PRECISION (12-bit samples, 16-bit tables)      COMPONENTS (greyscale, CMYK)
 *   SAMPLING (4:2:2, 4:4:0, ...)   RESTART   SCAN (not one interleaved sequential scan)   COLOURSPACE (Adobe, RGB ids)
 *   TABLES (a table is missing, malformed or has an id above 1)   SIZE   TRAILING (bytes behind the EOI)
 * The probe reads the markers up to the first SOS and the file's last two bytes; it does NOT look inside the scan.  A file with
 * a second scan, or any other marker between the first SOS and the final EOI, therefore counts as supported here; specmi_jpeg_decode
 * launches it, finds the marker (status bit 128) and the caller decodes it on the host like a damaged file.
 * Returns SPECMI_ERR_ARG for a null pointer, else SPECMI_OK.
 *
 * specmi_jpeg_decode.  DEVICE pointers: in_slab, the files' bytes, of in_slab_bytes; out_slab, uint8 RGB, of out_slab_bytes,
 * which must not overlap in_slab - the slab and offsets convention of the ragged calls, what spec_amd.preprocess.pack_frames
 * builds; status (n int32); coef (optional, NULL in the flows: receives the coefficient workspace after the dc stage -
 * (blocks, 64) int16, natural order within a block, MCU order between blocks, file after file - of coef_bytes >= 128 bytes per
 * block; it lets a test name the stage that is wrong).  HOST: files_host, the SAME bytes as in_slab (the probe reads the
 * markers from them; the scan is read on the device only; that the two agree is the caller's contract and is not checked - a
 * difference cannot take a read or a write out of bounds, it only gives a status or pixels that belong to no file); THE FILE RECORD, two arrays with one row per file:
 *   file_ranges (n x 2 int64):  offset of the file's first byte in in_slab and files_host, length
 *   out_offsets (n x 2 int64):  offset of the picture's first pixel in out_slab, pitch (bytes from one row to the next, >= 3 W)
 * and passes (optional): receives how often the sync stage was launched.
 * status[i] is 0 when file i's scan satisfied T.81 F.2.2 completely; else a set of bits - 1 an invalid code, 2 a zigzag index
 * beyond 63, 4 a DC category above 11 or an AC size above 10, 8 |coefficient x quantiser| above 32767, 16 the scan ended early,
 * 32 bits left over, 64 a block count that is not the file's, 128 a marker inside the scan - and the picture's rectangle is then
 * unspecified: the caller decodes that file on the host, so that the device never has to agree with libjpeg on a damaged file.
 * Bytes of out_slab outside the rectangles (H rows of 3 W bytes) are not touched.  A file's pixels do not depend on the other
 * files of the call, on its place in the slabs or on scheduling.
 * Every read of a file is confined to its byte range, every write to its rectangle or its share of the workspace; no kernel
 * waits for another workgroup.  The call SYNCHRONISES THE STREAM once per pass of the sync stage but the last (one word is read
 * back; at most as many passes as the largest file has groups of 256 x 128 scan bytes), and is therefore refused while the
 * stream is being captured (SPECMI_ERR_STATE; the stream is asked first, so the capture stays valid and nothing is enqueued).
 * Refused (SPECMI_ERR_ARG), launching nothing: a null pointer (coef and passes excepted); n outside [1, 65535]; a file range
 * that leaves in_slab; a file the probe refuses; a pitch below 3 W; a rectangle that leaves out_slab; overlapping slabs; two
 * rectangles that share a byte; a coef_bytes too small; more than 2^24 MCUs in all.
 * The file records (with quantisers and Huffman tables) live in one device table owned by the handle, under the rule of the
 * ragged calls above: a call whose records differ from the previous call's rewrites the table and first SYNCHRONISES THE
 * WHOLE DEVICE.  The workspace is one per handle (growth synchronises the device): per MCU of 16 x 16 pixels 768 bytes of
 * coefficients and 384 of planes - 4.5 bytes per pixel of the pictures rounded up to whole MCUs (9 at 4:4:4) - plus 16 bytes
 * per 128 scan bytes and 8 per group. */
#define SPECMI_JPEG_SUPPORTED 0
#define SPECMI_JPEG_NOT_JPEG 1
#define SPECMI_JPEG_TRUNCATED 2
#define SPECMI_JPEG_PROGRESSIVE 3
#define SPECMI_JPEG_SOF 4
#define SPECMI_JPEG_PRECISION 5
#define SPECMI_JPEG_COMPONENTS 6
#define SPECMI_JPEG_SAMPLING 7
#define SPECMI_JPEG_RESTART 8
#define SPECMI_JPEG_SCAN 9
#define SPECMI_JPEG_COLOURSPACE 10
#define SPECMI_JPEG_TABLES 11
#define SPECMI_JPEG_SIZE 12
#define SPECMI_JPEG_TRAILING 13
int specmi_jpeg_probe(const uint8_t* file, size_t bytes, int32_t* reason, int32_t* H, int32_t* W, int32_t* sampling);
int specmi_jpeg_decode(specmi_handle* h, const uint8_t* files_host, const uint8_t* in_slab, size_t in_slab_bytes, const int64_t* file_ranges,
                       uint8_t* out_slab, size_t out_slab_bytes, const int64_t* out_offsets, int n, int32_t* status, int16_t* coef,
                       size_t coef_bytes, int32_t* passes, void* stream);

/* PNG FILES decoded on the device, all files of a call together: the read side of specmi_png_encode.  Replaces the host decode
 * (PIL's Image.open(path).convert('RGB'), of which zlib's inflate is about half) and the upload of the raw frames in front of
 * every flow that reads .png frames (spec/tester.py:95, camcalib/pano_dataset.py:117).
 * THE CONTRACT (stated in full at the head of spec_amd/csrc/png_dec.hip, restated in NumPy in tests/png_dec_ref.py): for a SUPPORTED
 * file the (H, W, 3) uint8 RGB picture equals np.array(Image.open(f).convert('RGB')), element for element.
 *
 * specmi_png_probe: host only, needs no handle and no device.  Walks the chunks of `file` (HOST, `bytes` long) and says whether
 * specmi_png_decode takes it: *reason receives SPECMI_PNG_SUPPORTED or why not, *H, *W and *colour_type the picture (all 0 when
 * not supported), *nranges how many IDAT chunks the file has, and idat_ranges (max_ranges x 2 int64; may be NULL with
 * max_ranges 0) the first max_ranges of their payloads as [offset in the file, length].  A zlib stream is cut across IDAT chunks
 * wherever the writer liked: the caller joins the payloads, so that the device sees the stream contiguous.  SUPPORTED is: the 8
 * signature bytes; IHDR first; at least one IDAT, all IDATs consecutive; IEND last and nothing behind it; every chunk's CRC-32
 * correct; bit depth 8; colour type 0, 2, 4 or 6 (grey is replicated, alpha dropped, tRNS / gAMA / sRGB ignored, as
 * convert('RGB') does); compression 0, filter 0, interlace 0; H and W in [1, 32768]; no acTL; no unknown critical chunk.  The reasons:
 *   NOT_PNG (the signature)   TRUNCATED (a chunk or IEND is cut off)   CRC   DEPTH (16-bit, sub-byte)   PALETTE   INTERLACED
 *   ANIMATED (acTL)   CHUNK (order, a second IHDR, an unknown critical chunk, an unknown colour type or method, no IDAT)   SIZE
 *   TRAILING (bytes behind IEND)
 * Returns SPECMI_ERR_ARG for a null pointer or a negative max_ranges, else SPECMI_OK.
 *
 * specmi_png_decode.  DEVICE pointers: in_slab, of in_slab_bytes, which holds every file's zlib stream CONTIGUOUS (the IDAT
 * payloads joined); out_slab, uint8 RGB, of out_slab_bytes, which must not overlap in_slab - the slab and offsets convention of
 * the ragged calls; status (n int32); raw (optional, NULL in the flows: receives the inflated, still filtered streams, file i's
 * H (1 + W bpp) bytes beginning at the sum of the streams before it, each rounded up to 256; of raw_bytes; it lets a test name
 * the stage that is wrong).  HOST, one row per file:
 *   stream_ranges (n x 2 int64):  offset of the zlib stream in in_slab, length (8 at least)
 *   geom          (n x 3 int32):  H, W, colour type, as the probe gave them
 *   out_offsets   (n x 2 int64):  offset of the picture's first pixel in out_slab, pitch (bytes from one row to the next, >= 3 W)
 * status[i] is 0 when file i's stream satisfied RFC 1950 / 1951 completely, inflated to exactly H (1 + W bpp) bytes with the
 * right Adler-32 and every filter byte in 0 .. 4; else a set of bits - 1 a bad zlib header, 2 block type 3, 4 a stored block whose
 * LEN and NLEN disagree, 8 code lengths that over-subscribe or are incomplete, 16 a repeat code without a previous length or past
 * the end, 32 no end-of-block code, 64 an invalid code, 128 length symbol 286 / 287 or distance symbol 30 / 31, 256 a distance
 * beyond the output so far or the window, 512 the stream ended early, 1024 output longer or shorter than expected, 2048 bytes
 * between the final block and the Adler word, 4096 an Adler-32 mismatch, 8192 a filter byte above 4 - and the picture's
 * rectangle is then unspecified: the caller decodes that file on the host, which raises what it raises today.
 * Bytes of out_slab outside the rectangles (H rows of 3 W bytes) are not touched.  A file's pixels do not depend on the other
 * files of the call, on its place in the slabs or on scheduling.  Every read of a file is confined to its stream's range, every
 * write to its rectangle or its share of the workspace; no kernel waits for another workgroup and every loop has a bound known
 * from the records.  Nothing is read back: the call may be captured once its records and workspace exist.
 * Refused (SPECMI_ERR_ARG), launching nothing: a null pointer (raw excepted); n outside [1, 65535]; a stream range that leaves
 * in_slab; a stream shorter than 8 bytes; H or W outside [1, 32768]; a colour type other than 0, 2, 4, 6; a pitch below 3 W; a
 * rectangle that leaves out_slab; overlapping slabs; two rectangles that share a byte; a raw_bytes too small; more than 2^31
 * inflated bytes in all.
 * The file records live in one device table owned by the handle, under the rule of the ragged calls above: a call whose records
 * differ from the previous call's rewrites the table and first SYNCHRONISES THE WHOLE DEVICE; new records or a larger workspace
 * are refused while the stream is being captured (SPECMI_ERR_STATE; asked first, nothing enqueued).  The workspace is one per
 * handle: per file its inflated stream rounded up to 256 bytes, 512 KiB of match records (SPECMI_PNG_LANES x SPECMI_PNG_SUB_BITS
 * / 2 of 8 bytes), and 8 bytes per 32 KiB of the inflated stream. */
#define SPECMI_PNG_SUPPORTED 0
#define SPECMI_PNG_NOT_PNG 1
#define SPECMI_PNG_TRUNCATED 2
#define SPECMI_PNG_CRC 3
#define SPECMI_PNG_DEPTH 4
#define SPECMI_PNG_PALETTE 5
#define SPECMI_PNG_INTERLACED 6
#define SPECMI_PNG_ANIMATED 7
#define SPECMI_PNG_CHUNK 8
#define SPECMI_PNG_SIZE 9
#define SPECMI_PNG_TRAILING 10
#define SPECMI_PNG_LANES 256      /* lanes of the inflate workgroup: subsequences of a window */
#define SPECMI_PNG_SUB_BITS 512   /* bits of the zlib stream per subsequence */
int specmi_png_probe(const uint8_t* file, size_t bytes, int32_t* reason, int32_t* H, int32_t* W, int32_t* colour_type, int64_t* idat_ranges,
                     int max_ranges, int32_t* nranges);
int specmi_png_decode(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, const int64_t* stream_ranges, const int32_t* geom,
                      uint8_t* out_slab, size_t out_slab_bytes, const int64_t* out_offsets, int n, int32_t* status, uint8_t* raw,
                      size_t raw_bytes, void* stream);

/* ---- evaluation metrics on the path's outputs ---------------------------------- */

/* eval_single (spec/utils/compute_error.py:52-86, spec/trainer.py:272-316): joints =
 * J_regressor (J,V) @ vertices for prediction and ground truth, pelvis (joint 0) alignment,
 * selection of `nsel` joints (`joint_sel` device int32, NULL = the first nsel), then per image
 * MPJPE, PA-MPJPE (similarity Procrustes) and pelvis-aligned V2V, all in millimetres.  All
 * pointers are device pointers; any output may be NULL.  J and nsel in [1,32] (SPECMI_ERR_ARG otherwise; the joints are held
 * on chip); every entry of joint_sel must lie in [0,J) - it is device memory and is not checked - and may repeat; with
 * joint_sel NULL, nsel <= J (SPECMI_ERR_ARG otherwise).  A selection without variance (one joint, coincident joints) has no
 * similarity fit: PA-MPJPE is NaN there, as in the reference (0 / 0), and MPJPE stays finite. */
int specmi_eval_mesh(specmi_handle* h, const float* pred_vertices, const float* gt_vertices, int B,
                     int V, const float* J_regressor, int J, const int32_t* joint_sel, int nsel,
                     float* mpjpe_mm, float* pampjpe_mm, float* v2v_mm, void* stream);

/* eval_j_24 (spec/utils/compute_error.py:33-49): pelvis-aligned MPJPE / PA-MPJPE (mm) of two
 * (B,J,3) joint sets.  J in [1,32] (SPECMI_ERR_ARG otherwise); any output may be NULL.  The pelvis is subtracted in fp32 as the
 * reference does, everything after it runs in fp64; PA-MPJPE of a pose without variance is NaN, as in the reference. */
int specmi_eval_joints(specmi_handle* h, const float* pred_joints, const float* gt_joints, int B,
                       int J, float* mpjpe_mm, float* pampjpe_mm, void* stream);

/* What SPECTrainer.validation_step scores per batch (spec/trainer.py:272-344), in one launch, PER JOINT and in METRES - the unit
 * of the per-joint arrays in evaluation_results_<ds>.pkl (:338-344); callers multiply by 1000 where they print.  Per image:
 *   jp = J_regressor @ pred_vertices, jg = J_regressor @ gt_vertices, fp32, the summation of specmi_eval_mesh;
 *   selected joints p_i = jp[sel[i]] - jp[0], g_i = jg[sel[i]] - jg[0] (fp32 subtraction; joint_sel NULL = the first nsel joints)
 *     -> err_sel, pa_err_sel (B,nsel);
 *   given joints pred_joints, gt_joints (B,Jk,3), joint 0 subtracted from each set in fp32 (:282-283; a no-op on a set whose
 *     joint 0 is already the origin, as the dataset's joints_24 is) -> err_k, pa_err_k (B,Jk);
 *   err[b,i] = |p_i - g_i|; pa_err[b,i] = |s R (p_i - mean p) + mean g - g_i| with (s, R) the least-squares similarity fit of the
 *     whole set (reconstruction_error(..., reduction=None)[1]; Horn's quaternion solution in fp64, as in the two calls above).
 *     Everything after the pelvis subtraction runs in fp64 with one rounding to fp32.  A set without variance has no fit: every
 *     pa_err of it is NaN, as in the reference (0 / 0); its err stays finite;
 *   v2v[b] = mean_v |gt_v - pred_v| on the meshes as given - compute_error_verts (:312-315), NOT the pelvis-aligned V2V of
 *     specmi_eval_mesh.
 * All pointers are device pointers and any output may be NULL.  pred_joints and gt_joints are NULL together; then Jk is not read
 * and err_k / pa_err_k must be NULL.  SPECMI_ERR_ARG (nothing is launched or written): B < 1 or V < 1; J, nsel or (with joints)
 * Jk outside [1,32]; joint_sel NULL with nsel > J; exactly one of the joint sets NULL; a joint output without the joint sets.
 * The entries of joint_sel lie in [0,J) and may repeat (device memory, not checked).  One workgroup per image: an image's outputs
 * do not depend on B or on the other images. */
int specmi_eval_step(specmi_handle* h, const float* pred_vertices, const float* gt_vertices, int B, int V,
                     const float* J_regressor, int J, const int32_t* joint_sel, int nsel,
                     const float* pred_joints, const float* gt_joints, int Jk,
                     float* err_sel, float* pa_err_sel, float* err_k, float* pa_err_k, float* v2v, void* stream);

/* pred_joints = einsum('bik,ji->bjk', vertices, J_regressor) (spec/utils/compute_error.py:184,187): vertices (B,V,3),
 * J_regressor (J,V) device -> joints (B,J,3).  Any J >= 1: unlike the two calls above nothing per joint is held on chip, so
 * there is no cap of 32 (the joints run in chunks of 8, one workgroup per image and chunk). */
int specmi_regress_joints(specmi_handle* h, const float* vertices, int B, int V, const float* J_regressor, int J,
                          float* joints, void* stream);

/* torch.bmm(R, x.transpose(2,1)).transpose(2,1) (spec/utils/compute_error.py:164-165,186): R (B,3,3), points (B,N,3)
 * -> out (B,N,3), out[b,n] = R[b] points[b,n]. */
int specmi_rotate_points(specmi_handle* h, const float* R, const float* points, int B, int N, float* out, void* stream);

/* ---- SPEC's loss modules, forward value ---------------------------------------------------------- */

/* HMRLoss.forward (spec/losses.py:59-141; mode = SPECMI_HMR_LOSS) and HMRCamLoss.forward (:171-271; mode = SPECMI_HMR_CAM_LOSS)
 * as an evaluation quantity: the value only (its gradient: specmi_hmr_loss_backward below).  All pointers are device pointers, fp32 unless stated.
 *   prediction (the dict of HMR.forward): pred_pose (B,24,3,3), pred_shape (B,10), pred_cam (B,3), joints3d (B,49,3) =
 *     smpl_joints3d, joints2d (B,49,2) = smpl_joints2d, vertices (B,V,3) = smpl_vertices;
 *   ground truth (the batch of spec/dataset/cam_dataset.py): pose (B,72) axis-angle, betas (B,10), pose_conf (B,24), pose_3d
 *     (B,24,4) = xyz + confidence, keypoints (B,49,3) = xy + confidence - gt['keypoints'] (crop-normalised) in mode 0,
 *     gt['keypoints_orig'] (pixels) in mode 1 -, gt_vertices (B,V,3) or NULL, has_smpl / has_pose_3d (B) int32 (non-zero =
 *     annotated); mode 1 only: orig_shape (B,2) = (H, W) of the full image, scale (B) = the bbox scale;
 *   the eight weights are the constructor arguments of both classes (:27-36, :145-154); w_smpl_part belongs to the part
 *     segmentation branch, whose criterion the reference never defines (:131, :259), and is not read.
 * The terms, as the reference computes them:
 *   smpl_losses (:412-432): criterion = nn.MSELoss() (mean).  Over the Nv images with has_smpl, loss_regr_pose =
 *     mean(pose_conf over Nv x 24) * MSE(pred_pose, batch_rodrigues(pose)) over Nv x 24 x 3 x 3 - a PRODUCT OF TWO MEANS
 *     (:427 multiplies the confidences by an already reduced scalar), not a confidence-weighted mean; loss_regr_betas = MSE over
 *     Nv x 10; both 0 when Nv = 0.  batch_rodrigues is pare.utils.geometry's, i.e. SPIN's form: angle = |theta + 1e-8| (the
 *     epsilon added to every component), axis = theta / angle, quaternion (cos(angle / 2), sin(angle / 2) * axis) divided by its
 *     norm, quaternion -> matrix.  It is NOT the smplx Rodrigues that specmi_smpl_native applies to an axis-angle pose.
 *   projected_keypoint_loss (:274-296): conf = keypoints[..., 2] times w_openpose for joints 0-24 and w_gt for joints 25-48;
 *     element = conf * (joints2d - keypoints_xy)^2.  Mode 0: mean over B x 49 x 2.  Mode 1: both sides are first mapped to
 *     2 * (xy / (W, H)) - 1 (:188-195; `orig_shape.rot90().T` turns (H, W) into (W, H)), each element is then multiplied by
 *     (W, H) / (scale * 200) on its axis (:222-223), then the mean.  The prediction is only read (the reference overwrites
 *     pred['smpl_joints2d'] in place at :191).
 *   keypoint_3d_loss (:326-348): joints3d[:, 25:] against pose_3d over the Np images with has_pose_3d, each side minus its own
 *     pelvis = (joint 2 + joint 3) / 2; mean over Np x 24 x 3 of conf * squared error; 0 when Np = 0.
 *   shape_loss (:375-387): nn.L1Loss() = mean |vertices - gt_vertices| over Nv x V x 3; 0 when Nv = 0 or gt_vertices is NULL.
 *   loss_cam (:119, :247) = mean over B of exp(-10 * pred_cam[:, 0])^2.
 *   weights (:114-118): shape * w_shape; keypoints and keypoints_3d * w_keypoint; regr_pose * w_pose; regr_betas * w_beta;
 *     total = w_loss * (keypoints + keypoints_3d + regr_pose + regr_betas + shape + cam), added in that order (:135-137).
 * Outputs:
 *   terms (6,B), required: the UNNORMALISED per-image sums, computed for every image whatever its masks say.  Rows: 0 keypoints
 *     (49 x 2 elements, mode 1 already rescaled), 1 keypoints_3d (24 x 3), 2 and 3 the pose term's two factors - 2 the squared
 *     error of the 24 x 9 matrix elements, 3 the sum of the 24 pose confidences -, 4 betas (10), 5 vertices (V x 3; 0 without
 *     gt_vertices).  loss_cam is a function of one float per image and has no row.
 *   counts (2 int32, may be NULL): Nv, Np.
 *   means (7, may be NULL): loss_keypoints, loss_keypoints_3d, loss_regr_pose, loss_regr_betas, loss_shape, loss_cam (weighted,
 *     the reference's loss_dict order), then total_loss.
 * One launch reduces every image in a workgroup of its own (the vertices as 16-byte vectors counted from the image's first float,
 * wavefront shuffles, then LDS, no atomics), one small launch folds the B rows in an order that depends on B alone.  A per-image
 * value never depends on the other rows; the same inputs give the same bits in every run and at every batch position.  Nothing is
 * allocated: the call may be captured into a graph.  Works on a handle of any model kind, committed or not.
 * Refused (SPECMI_ERR_ARG), launching nothing, the message naming the argument: B <= 0, V <= 0 (or V * 3 past 31 bits), a mode
 * outside {0, 1}, a NULL required pointer (gt_vertices may be NULL only when w_shape == 0; counts and means are optional),
 * mode 1 without orig_shape or scale. */
#define SPECMI_HMR_LOSS 0
#define SPECMI_HMR_CAM_LOSS 1
int specmi_hmr_loss(specmi_handle* h, int mode, const float* pred_pose, const float* pred_shape, const float* pred_cam,
                    const float* joints3d, const float* joints2d, const float* vertices, const float* pose, const float* betas,
                    const float* pose_conf, const float* pose_3d, const float* keypoints, const float* gt_vertices,
                    const int32_t* has_smpl, const int32_t* has_pose_3d, const float* orig_shape, const float* scale, int B, int V,
                    float w_shape, float w_keypoint, float w_pose, float w_smpl_part, float w_beta, float w_openpose, float w_gt,
                    float w_loss, float* terms, int32_t* counts, float* means, void* stream);

/* The gradient of specmi_hmr_loss's seven means with respect to the six prediction tensors - what torch.autograd computes through
 * the reference's HMRLoss / HMRCamLoss.  The ground truth is never differentiated.
 *   inputs: mode, every tensor, B, V and the eight weights exactly as given to specmi_hmr_loss, plus what that call produced:
 *     terms (6, B) and counts (2 int32), both required - the pose term is a product of two batch means, so its gradient needs the
 *     batch sum of pose_conf (row 3 of terms over the images with has_smpl) and Nv;
 *   g_means (7): the upstream gradient of means.  The effective coefficient of term k (0 .. 5) is g_means[k] + w_loss *
 *     g_means[6], so any entry of the reference's loss_dict may be backpropagated, not only the total;
 *   outputs, dense fp32, each written in full: g_pred_pose (B,24,3,3), g_pred_shape (B,10), g_pred_cam (B,3) (columns 1 and 2 are
 *     0), g_joints3d (B,49,3) (non-zero only for joints 25 .. 48; joints 27 and 28 - 2 and 3 of those 24 - also carry what the
 *     pelvis takes back from the other 22), g_joints2d (B,49,2) (mode 1: through the normalisation to [-1, 1] and the
 *     (W, H) / (scale * 200) rescale), g_vertices (B,V,3) (the slope of |x|: -k, 0 at exactly 0, +k; written as 16-byte chunks
 *     counted from the image's first float, as the forward reads them).  Any output may be NULL, not all six.
 * An image masked out of a term gets exactly +0 there; Nv = 0 / Np = 0 give zeros, never NaN; a zero confidence gives 0;
 * gt_vertices NULL (w_shape == 0) gives g_vertices = 0.
 * One launch, one workgroup per image, no atomics, nothing allocated (capturable); any handle, committed or not.
 * Refused (SPECMI_ERR_ARG), launching nothing: what specmi_hmr_loss refuses; terms, counts or g_means NULL; every output NULL. */
int specmi_hmr_loss_backward(specmi_handle* h, int mode, const float* pred_pose, const float* pred_shape, const float* pred_cam,
                             const float* joints3d, const float* joints2d, const float* vertices, const float* pose, const float* betas,
                             const float* pose_conf, const float* pose_3d, const float* keypoints, const float* gt_vertices,
                             const int32_t* has_smpl, const int32_t* has_pose_3d, const float* orig_shape, const float* scale, int B, int V,
                             float w_shape, float w_keypoint, float w_pose, float w_smpl_part, float w_beta, float w_openpose, float w_gt,
                             float w_loss, const float* terms, const int32_t* counts, const float* g_means, float* g_pred_pose,
                             float* g_pred_shape, float* g_pred_cam, float* g_joints3d, float* g_joints2d, float* g_vertices,
                             void* stream);

/* Which execution plan a trunk forward of (B, 3, H, W) takes under the handle's current options ("plan" and its thresholds):
 * *mode = 0 throughput, 1 latency, 2 single; pair != 0: as specmi_trunk_forward_pair decides (the FIRST handle's options).  Callers
 * that describe or log what ran ask here instead of re-deriving the rule (bench.py, SpecPipeline). */
int specmi_trunk_plan(specmi_handle* h, int B, int H, int W, int pair, int32_t* mode);

/* ---- in-launch hand-off state (round 5) ---------------------------------------------------
 * The sliced (split-K) layers of the latency / single plans and the FC GEMMs hand partial tiles between the workgroups of ONE
 * launch: every K slice takes a ticket from its tile's arrival counter and the last to arrive folds the slices and re-zeroes the
 * counter (spec_amd/csrc/conv_igemm.hip, conv_wsplit.hip).  These counters are zero between launches.  They have no counterpart
 * in the reference (spec/tester.py:109-151 runs stock torch ops). */

/* Synchronises the device.  *status: 0 = every split-K arrival counter of the handle is zero (the hand-off state is clean);
 * -2 = a counter was not left at zero (a launch died mid-flight, or a protocol error; specmi_sync_reset clears it). */
int specmi_sync_status(specmi_handle* h, int32_t* status);
/* Zeroes the hand-off counters on `stream`.  The library does this itself at specmi_commit and after any forward that returned
 * an error; a caller that destroyed a captured graph mid-replay (or killed a launch some other way) calls it before the next forward. */
int specmi_sync_reset(specmi_handle* h, void* stream);
/* Tests only: overwrites every hand-off counter with `value` (synchronises). */
int specmi_debug_poison_sync(specmi_handle* h, uint32_t value);

/* ---- profiling -------------------------------------------------------------------------- */

/* When on, every kernel launch is bracketed by HIP events on the launch stream. */
int specmi_profile_enable(specmi_handle* h, int on);
/* Synchronises, folds the recorded launches into entries keyed by (kernel,label) and
 * clears the log.  Returns the number of entries in *n (at most max_entries copied). */
int specmi_profile_read(specmi_handle* h, specmi_prof_entry* entries, int max_entries, int* n);

#ifdef __cplusplus
}
#endif
#endif /* SPECMI_H */
