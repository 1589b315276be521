// handle.h - the library handle and the host-side helpers shared by api.hip (ResNet trunks, heads, C ABI) and
// hrnet.hip (HRNet trunks).  Internal to libspecmi.so.
#pragma once
#include <cstdarg>
#include <initializer_list>

#include "specmi_internal.h"

using namespace specmi;

// ------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<float> f;
    std::vector<int32_t> i;
    std::vector<int64_t> shape;
    bool is_int = false;
    size_t numel() const { return is_int ? i.size() : f.size(); }
};

struct ConvW {
    std::string name;  // state-dict prefix of the conv ("layer1.0.conv1"), bn under bn_name
    std::string bn_name;
    int cin = 0, cout = 0, k = 1, stride = 1, pad = 0;
    // channel counts of the activation tensors this layer reads / writes when they are padded to a multiple of 32
    // (HRNet-W48: 48 -> 64); 0 = same as cin / cout.  Padded weights are zero, padded outputs come out as 0.
    int cin_p = 0, cout_p = 0;
    int Kp = 0, Npad = 0;
    float *w = nullptr, *scale = nullptr, *shift = nullptr;  // device
    float* wino = nullptr;  // device: Winograd-domain filters (3x3 stride-1 layers only)
    void* wsplit = nullptr; // device: bf16 pieces of the weights (1x1 stride-1 layers, only when option conv_precision != 0)
    void* w16 = nullptr;    // device: fp16_rne(w * bn scale) [Kp16/8][Npad][8] (precision SPECMI_PRECISION_FP16 only)
    int Kp16 = 0;
};

struct Bneck {
    ConvW c1, c2, c3, ds;
    bool has_ds = false;
    bool basic = false;   // torchvision BasicBlock (ResNet-18/34): c1 = 3x3 (stride), c2 = 3x3, no c3
    // conv3 + bn3 and downsample conv + bn folded into ONE 1x1 GEMM over [conv2 output | block input]:
    // weights pre-multiplied by the BN scales (fp64), shift = shift3 + shift_ds, scale = 1
    float *f_w = nullptr, *f_scale = nullptr, *f_shift = nullptr;
    void* f_wsplit = nullptr;   // bf16 pieces of the same folded matrix (option conv_precision != 0)
    void* f_w16 = nullptr;      // fp16 image of the same folded matrix (precision SPECMI_PRECISION_FP16)
    int f_Npad = 0;
};

struct FcW {  // Linear layers as H=W=1 convolutions
    int nin = 0, nout = 0, Kp = 0, Npad = 0;
    float *w = nullptr, *scale = nullptr, *shift = nullptr;
    float* w_rm = nullptr;   // the same matrix as (nout, Kp) row-major rows, zero padded to Kp: the small-batch GEMV kernel's operand
};

struct HrNet;

// ---- the option list: every integer name specmi_set_option_i32 accepts, its default and whether it is part of the STABLE surface
// (include/specmi.h).  The only place a name and its default are written: enum Opt below and the table specmi_option_info reports
// (options.hip) are the two expansions of it, in this order.
#define SPECMI_OPTIONS(SPECMI_OPT) \
    /* stable: model shape (before commit) */                                                                             \
    SPECMI_OPT(backbone, 50, true)                                                                                        \
    SPECMI_OPT(num_fc_layers, 1, true)                                                                                    \
    SPECMI_OPT(num_fc_channels, 1024, true)                                                                               \
    SPECMI_OPT(use_cam, 0, true)                                                                                          \
    SPECMI_OPT(use_cam_feats, 0, true)                                                                                    \
    SPECMI_OPT(img_res, 224, true)                                                                                        \
    SPECMI_OPT(hrnet_use_conv, 1, true)                                                                                   \
    SPECMI_OPT(estimate_var, 0, true)                                                                                     \
    SPECMI_OPT(uncertainty_activation, 0, true)                                                                           \
    /* stable: execution (any time) */                                                                                    \
    SPECMI_OPT(plan, 0, true)                                                                                             \
    SPECMI_OPT(winograd, 1, true)                                                                                         \
    SPECMI_OPT(fuse_downsample, 1, true)                                                                                  \
    SPECMI_OPT(head_collapse, 1, true)                                                                                    \
    SPECMI_OPT(output_ld, 0, true)                                                                                        \
    SPECMI_OPT(angle_ld, 0, true)                                                                                         \
    SPECMI_OPT(experimental, 0, true)                                                                                     \
    /* experimental: secondary arithmetic, debug pins, tuning thresholds, measured-slower or measured-neutral opt-ins */  \
    SPECMI_OPT(conv_precision, 0, false)                                                                                  \
    SPECMI_OPT(conv_precision_3x3, 0, false)                                                                              \
    SPECMI_OPT(force_conv_variant, 0, false)                                                                              \
    SPECMI_OPT(force_wino_variant, 0, false)                                                                              \
    SPECMI_OPT(fc_splitk, 1, false)                                                                                       \
    SPECMI_OPT(fc_gemv, 1, false)                                                                                         \
    SPECMI_OPT(head_fuse, 3, false)                                                                                       \
    SPECMI_OPT(smpl_skin_split, -1, false)                                                                                \
    SPECMI_OPT(trunk_subbatch, 0, false)                                                                                  \
    SPECMI_OPT(trunk_subbatch_layers, 2, false)                                                                           \
    SPECMI_OPT(single_max_batch, 2, false)                                                                                \
    SPECMI_OPT(latency_max_batch, 10, false)                                                                              \
    SPECMI_OPT(latency_max_batch_single, 16, false)                                                                       \
    SPECMI_OPT(latency_target_wgs, 256, false)                                                                            \
    SPECMI_OPT(latency_min_chunks, 4, false)                                                                              \
    SPECMI_OPT(latency_wino_min_tiles, 128, false)                                                                        \
    SPECMI_OPT(latency_fill_wgs, 240, false)                                                                              \
    SPECMI_OPT(latency_fill_wgs_large, 400, false)                                                                        \
    SPECMI_OPT(latency_unit_model, 0, false)                                                                              \
    SPECMI_OPT(latency_unit_slots, 256, false)                                                                            \
    SPECMI_OPT(latency_force_unit, 0, false)                                                                              \
    SPECMI_OPT(wsplit, 1, false)                                                                                          \
    SPECMI_OPT(wsplit_max_units, 1400, false)                                                                             \
    SPECMI_OPT(wsplit_max_units_single, 500, false)                                                                       \
    SPECMI_OPT(wsplit_slots, 256, false)                                                                                  \
    SPECMI_OPT(conv2d_sk, 0, false)                                                                                       \
    SPECMI_OPT(conv2d_wsplit, 0, false)                                                                                   \
    SPECMI_OPT(camcalib_head_group, 1, false)                                                                             \
    SPECMI_OPT(conv_wgrad_splits, 0, false)

#define SPECMI_OPT(name, def, stable) OPT_##name,
enum Opt { SPECMI_OPTIONS(SPECMI_OPT) OPT_COUNT };
#undef SPECMI_OPT

// A device buffer grown on demand (grow_ragged, api.hip): kept while it is large enough, else replaced by one at least 1.5x its
// size.  The outgrown one joins ws_retired and is freed at specmi_destroy only: work enqueued earlier, or a captured graph, may
// still name it.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// The per-call records of a ragged entry point on the device, with their host image.  The rule, stated once (publish_table,
// api.hip): a call builds its records on the host and compares them with `host`.  Equal bytes are neither copied nor waited
// for, which is what makes a repeated call capturable.  Other bytes, or a table that has to grow (as a DevBuf grows),
// synchronise the WHOLE device first - a call enqueued earlier on any stream may still read the old records - then become
// `host`, which stays alive until the next rewrite, and are copied on the caller's stream.
struct DevTable {
    DevBuf dev;
    std::vector<int> host;              // the records of dev as last uploaded (every record type is a whole number of ints)
};

enum Tab {
    TAB_ragged,     // specmi_resize_normalize_ragged: the per-frame records (RaggedFrame) + their Pillow coefficient tables
    TAB_pano,       // specmi_pano_extract_views: the per-view records (PanoView)
    TAB_crop,       // specmi_crop_normalize_ragged, specmi_crop_resize_normalize_ragged: the per-frame records (CropFrame)
    TAB_views,      // specmi_render_views: the view records, pixel prefix and pair table
    TAB_draw,       // specmi_draw_skeletons: the frame records and the bone table
    TAB_marks,      // specmi_draw_marks: the frame records, the marks and the tile list
    TAB_jpeg,       // specmi_jpeg_encode: the picture records and the quality's tables
    TAB_png,        // specmi_png_encode: the picture records
    TAB_jdec,       // specmi_jpeg_decode: the file records with their tables
    TAB_pdec,       // specmi_png_decode: the file records
    TAB_jitter,     // specmi_color_jitter: the frame records with their jitter records
    TAB_COUNT
};

enum Buf {
    BUF_ragged_tmp, // specmi_resize_normalize_ragged: the uint8 rows between the two passes
    BUF_render,     // mesh rasteriser (specmi_render_meshes, specmi_render_views): depth keys, snapped vertices, normal sums
    BUF_jpeg,       // specmi_jpeg_encode: coefficients, bit counts, the unstuffed scans and the chunk sums (jpeg_ws_layout)
    BUF_png,        // specmi_png_encode: the filtered streams, the segments' blocks and their sums (png_ws_layout)
    BUF_jdec,       // specmi_jpeg_decode: coefficients, planes and the lanes' states (jdec_ws_layout)
    BUF_pdec,       // specmi_png_decode: the inflated streams, the match records and the Adler sums (pdec_ws_layout)
    BUF_smpl_bwd,   // specmi_smpl_backward: smpl_bwd_ws_floats(V, B) floats
    BUF_head_train, // specmi_hmr_head_train_forward / specmi_hmr_head_backward: head_train_fwd_ws_floats / head_train_bwd_ws_floats floats
    BUF_cam_head_train, // specmi_camcalib_head_backward: cam_head_bwd_ws_floats floats
    BUF_jitter,     // specmi_color_jitter: one 64-bit sum of L per frame
    BUF_conv_bwd,   // specmi_conv2d_backward: conv_bwd_ws_floats floats (the gradient operand G)
    BUF_conv_fwd,   // specmi_conv2d_train_forward: conv_fwd_ws_floats floats (the weights transposed for this call)
    BUF_bn_train,   // specmi_batchnorm_train_forward / specmi_batchnorm_backward: bn_ws_floats floats (the chunk partials)
    BUF_COUNT
};

struct specmi_handle {
    specmi_handle();                // options.hip: every option at its default
    int device = 0;
    int kind = 0;
    std::map<std::string, HostTensor> staged;
    int opt[OPT_COUNT];             // one slot per integer option
    float focal_length = 5000.f;    // the one float option (specmi_set_option_f32)
    bool committed = false;
    // SPECMI_PRECISION_*: what specmi_set_precision asked for, and what the last successful commit packed
    int precision = 0, committed_precision = 0;
    std::string err;

    // packed parameters (device)
    ConvW stem;
    std::vector<Bneck> blocks;
    FcW fc_cam[3][3];          // CamCalib: vfov, pitch, roll x up to 3 stacked Linear layers (camcalib/model.py:59-70: no activation between them)
    int fc_layers = 1, feat_ch = 2048;
    FcW fc1, fc2, dec;         // HMR head (dec = decpose|decshape|deccam)
    FcW head_c;                // the 3 IEF iterations composed into ONE affine map [xf | cam feats] -> 157 (commit_head_collapsed)
    bool has_head_c = false;
    // option "estimate_var" (HMRHead's uncertainty outputs, spec/models/hmr.py:35-38,57-64): the variance decoders
    // [decpose_var (144) ; decshape_var (10)] for the nine-GEMM loop; the collapsed map carries them as 154 extra output rows
    FcW head_var;
    bool has_var = false;
    // where the last head forward left the regressed state [pose6d | shape | cam] and the raw variance columns (specmi_hmr_uncertainty)
    const float* last_state = nullptr; long last_ld_state = 0;
    const float* last_var = nullptr; long last_ld_var = 0;
    int last_B = 0;
    int xc_ld = 2240;          // row stride of the IEF state [xf (feat_ch) | pose6d | shape | cam | rot6d(R) | vfov | 0-pad]
    float *init_pose = nullptr, *init_shape = nullptr, *init_cam = nullptr;
    SmplDev smpl;
    HrNet* hrnet = nullptr;    // HRNet trunk (HMR option "backbone" = 32 / 48) instead of the ResNet blocks
    std::vector<void*> param_allocs;

    // workspace (device), grown on demand
    std::vector<void*> ws_allocs;
    std::vector<void*> ws_retired;      // outgrown workspaces, kept until destroy (captured graphs may still name them)
    float* act[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t act_elems = 0;
    float *xc = nullptr, *h1 = nullptr, *h2 = nullptr, *xf = nullptr;
    float* fc_hidden[2] = {nullptr, nullptr};   // (3, B, 1024) each: hidden rows of the three CamCalib Linear chains (latency plan)
    float *rot_ws = nullptr, *betas_ws = nullptr, *cam_ws = nullptr, *verts_ws = nullptr;
    float *pf_ws = nullptr, *A_ws = nullptr, *pj_ws = nullptr;
    int ws_B = 0;
    // specmi_resize_normalize's own table: keyed by the geometry, not by its bytes, and freed when outgrown (resize_normalize, api.hip)
    int* resize_tab = nullptr;          // device copy of the Pillow coefficient tables of the last resize geometry
    size_t resize_tab_ints = 0;
    std::vector<int> resize_host;       // host image of the same (kept alive for the async copy)
    int resize_geom[4] = {0, 0, 0, 0};  // H, W, OH, OW the tables were built for
    // the ragged entry points' record tables and workspaces: what each holds stands at its name in enum Tab / enum Buf
    DevTable tab[TAB_COUNT];
    DevBuf buf[BUF_COUNT];
    SkWs sk;                            // split-K partial tiles + arrival counters (ensure_sk; never allocated under graph capture:
                                        // the warm-up call of a shape sizes it)
    std::vector<void*> sk_retired;      // outgrown split-K buffers, kept until destroy (captured graphs may still name them)

    Profiler prof;
};

int fail(specmi_handle* h, int code, const char* fmt, ...);

#define HIPCHK(h, call)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return fail(h, SPECMI_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

#define LAUNCHCHK(h, rc, what)                                                                   \
    do {                                                                                        \
        int rc__ = (rc);                                                                        \
        if (rc__ != 0)                                                                          \
            return fail(h, SPECMI_ERR_HIP, "launch %s failed: %s", what,                        \
                        hipGetErrorString((hipError_t)rc__));                                   \
    } while (0)


// ---- shared host helpers (api.hip; find / need: commit.hip) -------------------------------------------------------------------------
int round_up(int x, int m);
int conv_out(int x, int k, int s, int p);
int dev_upload(specmi_handle* h, const void* src, size_t bytes, void** out, std::vector<void*>& pool);
int dev_alloc(specmi_handle* h, size_t bytes, void** out, std::vector<void*>& pool);
void free_pool(std::vector<void*>& pool);
const HostTensor* find(specmi_handle* h, const std::string& name);
int need(specmi_handle* h, const std::string& name, std::initializer_list<int64_t> shape, bool is_int, const HostTensor** out);
inline int opt(const specmi_handle* h, Opt o) { return h->opt[o]; }
// ---- commit.hip: packing, BatchNorm folding, the composed regressor, layer tables, SMPL constants ----------
// conv weight + eval-mode BatchNorm under state-dict names prefix + c.name / c.bn_name -> packed device tensors
int commit_conv(specmi_handle* h, const std::string& prefix, ConvW& c);
// OIHW -> [Kp/4][Npad][4], k = (ky*KW + kx)*Cin + ci (zero padded): the MFMA B-fragment layout of the implicit-GEMM kernels
void pack_gemm_weights(const float* w, int cout, int cin, int kh, int kw, int Kp, int Npad, std::vector<float>& out);
int commit_fused_ds(specmi_handle* h, const std::string& prefix, Bneck& b);
int commit_fc(specmi_handle* h, const std::vector<std::string>& names, const std::vector<int>& nouts, int nin, FcW& fc);
// what commit_fc uploads for its stacked (ntot, nin) weights and (ntot) bias, allocated from `pool` (specmi_fc_forward: a temporary one)
int upload_fc(specmi_handle* h, const float* w, const float* b, int ntot, int nin, FcW& fc, std::vector<void*>& pool);
int commit_head_collapsed(specmi_handle* h, int F, int ucf);
void build_resnet(specmi_handle* h, int depth);
int commit_smpl(specmi_handle* h);

// ---- HRNet trunks (hrnet.hip) ------------------------------------------------------------------------------
struct HrNet;
void hrnet_free(HrNet* n);
int hrnet_commit(specmi_handle* h, const std::string& prefix, int width, int use_conv);
// images NCHW -> (B, H/32, W/32, feat_ch) NHWC in feat_out
const float* hrnet_feat_ws(specmi_handle* h);   // the internal (B, fh, fw, feat_ch) buffer used when feat_out == NULL
int hrnet_forward(specmi_handle* h, const float* images, int B, int H, int W, float* feat_out, int* fh, int* fw, hipStream_t s);
// the launchers of HRNet's own kernels, shared by hrnet_forward and the kernel-level entries (specmi_hr_*): they return a
// specmi status and leave the message on the handle.  The callers guarantee C % 4 == 0, ld % 4 == 0 and 16-byte aligned pointers.
int hr_launch_stem3x3(specmi_handle* h, const float* images, int B, int H, int W, const float* w, const float* scale,
                      const float* shift, float* out, const LaunchCtx& ctx);
int hr_launch_fuse_sum(specmi_handle* h, const float* const* terms, const int* ld, const int* sh, int nt, int B, int H, int W, int C,
                       int relu, float* out, int ldo, const LaunchCtx& ctx);
int hr_launch_resize_ac(specmi_handle* h, const float* x, int B, int H, int W, int C, int ld, float* out, int OH, int OW, int ldo,
                        const LaunchCtx& ctx);
