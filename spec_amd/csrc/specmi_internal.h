// Internal declarations shared by the HIP translation units of libspecmi.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/specmi.h"

namespace specmi {

// ----------------------------------------------------------------------------------------
// launch profiler: HIP events on the launch stream around every kernel
// ----------------------------------------------------------------------------------------
struct ProfRecord {
    const char* kernel;
    std::string label;
    double flops, bytes;
    hipEvent_t e0, e1;
};

struct Profiler {
    bool on = false;
    std::vector<ProfRecord> log;
    std::string scope;  // label prefix set by the caller ("backbone.layer1.0.conv1")
};

struct LaunchCtx {
    hipStream_t stream;
    Profiler* prof;
    const char* label;
};

struct ProfScope {  // RAII: records e0 at construction, e1 at destruction
    Profiler* p;
    hipStream_t s;
    ProfRecord r;
    bool active;
    ProfScope(const LaunchCtx& c, const char* kernel, double flops, double bytes)
        : p(c.prof), s(c.stream), active(c.prof && c.prof->on) {
        if (!active) return;
        r.kernel = kernel;
        r.label = c.label ? c.label : "";
        r.flops = flops;
        r.bytes = bytes;
        (void)hipEventCreate(&r.e0);
        (void)hipEventCreate(&r.e1);
        (void)hipEventRecord(r.e0, s);
    }
    ~ProfScope() {
        if (!active) return;
        (void)hipEventRecord(r.e1, s);
        p->log.push_back(r);
    }
};

// hipFuncSetAttribute is a per-DEVICE setting: remember per (kernel instantiation, device) whether the
// dynamic-LDS limit was raised (a second device in the same process must get its own call).
struct DevOnce {
    bool done[64] = {};
};
inline int set_dyn_lds_once(DevOnce& once, const void* fn, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0 && dev < 64 && once.done[dev]) return 0;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0 && dev < 64) once.done[dev] = true;
    return 0;
}

// ----------------------------------------------------------------------------------------
// small helpers that several kernel files use: each is stated here once
// ----------------------------------------------------------------------------------------
// the sum of v over the 64 lanes of a wave, on every lane; the order of the additions is part of every result built on it
template <typename T> __device__ __forceinline__ T wave_sum64(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// a0 b0 + a1 b1 + a2 b2 with the roundings written out (one product, two fused steps): SMPL's pose kernel (both instantiations)
// and its backward must agree to the bit, and left to itself the compiler contracts the same source differently in each
// (-ffp-contract=fast with aggressive FMA fusion picks by context)
__device__ __forceinline__ float dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
#pragma clang fp contract(off)
    return fmaf(a2, b2, fmaf(a1, b1, a0 * b0));
}
// exclusive scan of one value per thread over the 256 threads of a workgroup -> and the total
template <typename T> __device__ __forceinline__ T block_scan(T v, T* lds, T* total) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {
        const T add = tid >= d ? lds[tid - d] : T(0);
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    const T incl = lds[tid];
    *total = lds[255];
    __syncthreads();                     // the caller may use lds again
    return incl - v;
}
// index of the last of n records, sorted by their member `first`, whose `first` is <= key (0 when none is): the picture or file
// that a chunk, row or segment of a whole call belongs to
template <typename T> __host__ __device__ __forceinline__ int last_at_or_before(const T* recs, int n, int key, int T::*first) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (recs[mid].*first <= key) lo = mid; else hi = mid;
    }
    return lo;
}
// libjpeg's FIX(x) at 16 fractional bits, for the colour conversions of the JPEG encoder and decoder
constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }
// ImageNet's mean / std of colour plane c, as torchvision's Normalize and pare's denormalize_images take them (a function:
// device code cannot index a host array with a channel that is not a constant)
__host__ __device__ __forceinline__ void imagenet_mean_std(int c, float& mean, float& stdv) {
    const float m[3] = {0.485f, 0.456f, 0.406f}, s[3] = {0.229f, 0.224f, 0.225f};
    mean = m[c]; stdv = s[c];
}
// Normalize of a ToTensor value x01 = u8 / 255 of colour plane c: a subtraction and a division, each rounded (no reciprocal)
__host__ __device__ __forceinline__ float normalize_unit(float x01, int c) {
    float mean, stdv;
    imagenet_mean_std(c, mean, stdv);
    return (x01 - mean) / stdv;
}

// ----------------------------------------------------------------------------------------
// implicit-GEMM convolution / linear layer on fp32 MFMA  (conv_igemm.hip)
// ----------------------------------------------------------------------------------------
struct ConvArgs {
    const float* x;      // NHWC activations; pixel stride ldx floats
    const float* w;      // packed weights [Kp/4][Npad][4], k = (ky*KW+kx)*Cin + ci
    const float* scale;  // [Npad]
    const float* shift;  // [Npad]
    const float* res;    // optional residual, indexed like out (may alias out)
    float* out;          // [M][ldo]
    int B, H, W, Cin, ldx;
    int OH, OW, Cout, Npad, ldo;
    int KH, KW, stride, pad;
    int relu;
    // optional second A source of a 1x1 layer: out = [x | x2(strided)] * w, K = Cin + Cin2 (rows k >= Cin of w);
    // used to fold a bottleneck's downsample branch into its conv3
    const float* x2 = nullptr;
    int H2 = 0, W2 = 0, ldx2 = 0, Cin2 = 0, stride2 = 1;
    // per-handle tuning overrides (tests / tools): 0 = automatic choice
    int force_variant = 0;   // conv_igemm tile (1: 128x128/4 waves, 2: 128x64/4, 3: 64x64/4, 4: 128x128/8 waves)
    int wino_variant = 0;    // conv_wino frequencies per wave (16 / 8)
};
// 32-channel K chunks of the layer: one per (filter tap, 32 channels of x), then those of the second source
inline int conv_k_chunks(const ConvArgs& a) { return a.KH * a.KW * (a.Cin / 32) + (a.x2 ? a.Cin2 / 32 : 0); }
// no im2col: every output pixel reads one input pixel (any stride)
inline bool conv_is_1x1(const ConvArgs& a) { return a.KH == 1 && a.KW == 1 && a.pad == 0; }
// what the launch profiler records for the layer: algorithmic flops and the bytes of x (+ x2), w, out (+ res) moved once
inline void conv_flops_bytes(const ConvArgs& a, double* flops, double* bytes) {
    const double M = (double)a.B * a.OH * a.OW;
    const double Kd = (double)a.KH * a.KW * a.Cin + (a.x2 ? a.Cin2 : 0);
    *flops = 2.0 * M * a.Cout * Kd;
    *bytes = 4.0 * ((double)a.B * a.H * a.W * a.Cin + (a.x2 ? M * a.Cin2 : 0.0) + M * a.Cout * (a.res ? 2.0 : 1.0) + Kd * a.Cout);
}
// floor(n / d) == umulhi(n, mg) >> sh for every n < 2^31 and 2 <= d < 2^31:
// L = 31 + ceil(log2 d), mg = floor(2^L / d) + 1 (< 2^32), sh = L - 32.  d == 1 is magic_div's own case.
inline void magic_u32(unsigned d, unsigned* mg, unsigned* sh) {
    if (d < 2) { *mg = 0; *sh = 0; return; }
    unsigned s = 0;
    while ((1ull << s) < d) ++s;
    const unsigned L = 31 + s;
    *mg = (unsigned)((1ull << L) / d + 1ull);
    *sh = L - 32;
}
__device__ __forceinline__ int magic_div(int n, int d, unsigned mg, unsigned sh) {
    return d == 1 ? n : (int)(__umulhi((unsigned)n, mg) >> sh);
}
// Cin % 32 == 0, Npad % 64 == 0.  Returns hipError as int.
// b != nullptr: the same layer shape of a SECOND network (own tensors) in the same launch (gridDim.z = 2)
int launch_conv_igemm(const ConvArgs& a, const LaunchCtx& ctx, const ConvArgs* b = nullptr);
// Split-K (conv_igemm.hip header): K slices as gridDim.y of ONE launch; the last slice of a tile to arrive adds the partial
// tiles in slice order and runs the epilogue (deterministic, batch-invariant).
struct SkWs {
    float* ws = nullptr;       // partial tiles: conv_igemm_sk_ws_floats() floats
    size_t floats = 0;
    unsigned* cnt = nullptr;   // one arrival counter per (tile, group), zero between launches
    int ncnt = 0;
};
// The canonical k-sum tree of a sliced layer and the share of it one workgroup computes (conv_igemm.hip header)
struct SkPlan {
    int leaves = 1;   // K = leaves x L chunks; a leaf is one MFMA chain from +0
    int G = 1;        // consecutive leaves that fold into a group (the groups fold into the result)
    int unit = 1;     // leaves per workgroup: 1, G or leaves (= no slabs) - a speed choice, the bits are the same
};
// leaves of the FC GEMMs (every plan; 1 = don't split)
int conv_igemm_splitk_plan(const ConvArgs& a);
// leaves of a convolution in the latency plan: depends on the layer's per-image shape only, never on the batch
int conv_igemm_sk_slices(const ConvArgs& a, int target_wgs, int min_chunks);
// the same + the unit for batch a.B (groups = 2: grouped launch of two networks)
SkPlan conv_igemm_sk_plan(const ConvArgs& a, int groups, int target_wgs, int min_chunks, int fill_wgs);
size_t conv_igemm_sk_ws_floats(const ConvArgs& a, int slabs, int groups);
int conv_igemm_sk_tiles(const ConvArgs& a, int groups);
// conv_igemm_sk_check / the sliced launchers: the tensors pass 32-bit buffer addressing and these launchers do not split the batch -
// the ONE condition on which the caller may take the throughput launcher instead (every other non-zero result is an error)
constexpr int SK_NEEDS_BATCH_SPLIT = -1001;
int launch_conv_igemm_sk(const ConvArgs& a, const SkPlan& pl, const SkWs& sk, const LaunchCtx& ctx, const ConvArgs* b = nullptr);
// the wave-split unit of the same tree (conv_wsplit.hip): a 32x32 tile per workgroup, the leaves of a group on its four waves;
// pl.unit = pl.leaves (no slabs) or pl.G (one group per workgroup, a 4 KB slab per group)
bool conv_wsplit_supported(const ConvArgs& a, const SkPlan& pl);
int conv_wsplit_tiles(const ConvArgs& a, int groups);
size_t conv_wsplit_ws_floats(const ConvArgs& a, int slabs, int groups);
int launch_conv_wsplit(const ConvArgs& a, const SkPlan& pl, const SkWs& sk, const LaunchCtx& ctx, const ConvArgs* b = nullptr);
// pick the tile the launcher would use (for tests / labels)
const char* conv_igemm_variant(const ConvArgs& a);

// ----------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolution as Winograd F(2x2,3x3) on fp32 MFMA  (conv_wino.hip)
// ----------------------------------------------------------------------------------------
// a.w must point at pack_wino_weights() output; Cin % 16 == 0, Cout % 64 == 0, no residual.
bool conv_wino_supported(const ConvArgs& a);
void pack_wino_weights(const float* w_oihw, int cout, int cin, std::vector<float>& out);
int launch_conv_wino(const ConvArgs& a, const LaunchCtx& ctx, const ConvArgs* b = nullptr);   // b: see launch_conv_igemm

// ----------------------------------------------------------------------------------------
// OPTIONAL: 1x1 / stride-1 convolution with fp32-class results on the bf16 matrix cores  (conv_bf16s.hip)
// ----------------------------------------------------------------------------------------
// w_oi (cout, cin) fp32 -> bf16 pieces w0 + w1 + w2 packed [piece][cin/8][Npad][8]
void pack_bf16_split_weights(const float* w_oi, int cout, int cin, int Npad, std::vector<unsigned short>& out);
void pack_bf16_split_weights_oihw(const float* w_oihw, int cout, int cin, int kh, int kw, int Npad, std::vector<unsigned short>& out);
bool conv_bf16s_supported(const ConvArgs& a);
// terms = 6 (fp32-class) or 3 (~1e-5); a.w is ignored, wsplit = the packed pieces on the device
int launch_conv_bf16s(const ConvArgs& a, const void* wsplit, int terms, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// fp16 trunk path: implicit-GEMM convolution on the fp16 matrix cores, image conversion, max-pool  (conv_f16.hip)
// ----------------------------------------------------------------------------------------
struct ConvF16Args {
    const void* x = nullptr;       // fp16 NHWC, pixel stride ldx (multiple of 8, >= Cin; channels past Cin are zero)
    const void* w = nullptr;       // fp16 [Kp/8][Npad][8]: fp16_rne(w * bn_scale), k = (ky*KW + kx)*ldx + ci, zero padded
    const float* shift = nullptr;  // fp32 [Npad]
    const void* res = nullptr;     // optional fp16 residual, indexed like out
    void* out = nullptr;           // fp16 (out_f32 = 0) or fp32 [M][ldo]
    int B = 0, H = 0, W = 0, Cin = 0, ldx = 0;
    int OH = 0, OW = 0, Cout = 0, Npad = 0, ldo = 0;
    int KH = 1, KW = 1, stride = 1, pad = 0, relu = 0, out_f32 = 0;
    int Kp = 0;                    // round_up(KH*KW*ldx, 32), or Cin + Cin2 with x2
    // optional second A source of a 1x1 / stride-1 layer (the folded downsample): K = [x | x2 at (oy*stride2, ox*stride2)]
    const void* x2 = nullptr;
    int H2 = 0, W2 = 0, ldx2 = 0, Cin2 = 0, stride2 = 1;
};
// (cout, K) fp64 products -> fp16 [Kp/8][Npad][8]; returns the index n*K + k of the first product that overflows fp16, or -1
long pack_f16_weights(const std::vector<double>& wk, int cout, int K, int Kp, int Npad, std::vector<unsigned short>& out);
// OIHW weights x per-channel BN scale in fp64, K ordered (ky, kx, ci) over cin_p channels
void fold_f16_oihw(const float* w, const float* scale, int cout, int cin, int cin_p, int kh, int kw, std::vector<double>& wk);
int launch_conv_f16(const ConvF16Args& a, const LaunchCtx& ctx);
// NCHW fp32 (C <= 8) -> NHWC fp16 with 8 channels (zero padded)
int launch_to_nhwc_f16(const float* x, void* out, int B, int C, int H, int W, const LaunchCtx& ctx);
int launch_maxpool_f16(const void* x, void* out, int B, int H, int W, int C, int OH, int OW, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// stem + pooling  (stem.hip)
// ----------------------------------------------------------------------------------------
// x NCHW (B,3,H,W); w = pack_stem_weights() output; out NHWC (B,OH,OW,64), BN+ReLU.
void pack_stem_weights(const float* w_oihw, std::vector<float>& out);
// pair / (x1, out1): the same op of a SECOND network in the same launch (see launch_conv_igemm)
struct StemPair { const float *x, *w, *scale, *shift; float* out; };
int launch_stem(const float* x, const float* w, const float* scale, const float* shift,
                float* out, int B, int H, int W, int OH, int OW, int relu, const LaunchCtx& ctx, const StemPair* pair = nullptr);
int launch_maxpool3x3s2(const float* x, float* out, int B, int H, int W, int C, int OH, int OW,
                        const LaunchCtx& ctx, const float* x1 = nullptr, float* out1 = nullptr);
// IEF state row of image b at xc + b*ld: [xf (F) | pose6d 144 | shape 10 | cam 3 | rot6d(R) 6 | vfov 1 | 0-pad], F = trunk
// features (2048 for ResNet-50: ld = 2240), state_off = F  (head.hip: head_init_kernel; stem.hip: extra workgroups of the avg-pool)
struct HeadInit {
    float* xc; const float *init_pose, *init_shape, *init_cam, *R, *K, *img_h;
    int use_cam_feats, state_off, ld;
};
// columns state_off .. ld of row b, by `nthreads` threads
__device__ __forceinline__ void head_init_row(const HeadInit& a, int b, int tid, int nthreads) {
    float* row = a.xc + (size_t)b * a.ld + a.state_off;
    for (int i = tid; i < a.ld - a.state_off; i += nthreads) {
        float v = 0.f;
        if (i < 144) v = a.init_pose[i];
        else if (i < 154) v = a.init_shape[i - 144];
        else if (i < 157) v = a.init_cam[i - 154];
        else if (a.use_cam_feats && i < 163) {
            const int e = i - 157;                   // rotmat[:, :, :2] row-major: (row, col) = (e/2, e%2)
            v = a.R[(size_t)b * 9 + (e >> 1) * 3 + (e & 1)];
        } else if (a.use_cam_feats && i == 163) {
            v = 2.0f * atanf(a.img_h[b] / (2.0f * a.K[(size_t)b * 9]));
        }
        row[i] = v;
    }
}
// x (B,HW,C) -> out[b*ldo + c] = mean_hw.  init != nullptr: the same launch also writes the IEF state columns of every row
// (B more workgroups; one graph node less on the small-batch path) - returns 1 in *init_done if it did
int launch_avgpool(const float* x, float* out, int B, int HW, int C, int ldo, const LaunchCtx& ctx, const HeadInit* init = nullptr,
                   bool* init_done = nullptr);

// ----------------------------------------------------------------------------------------
// heads  (head.hip)
// ----------------------------------------------------------------------------------------
int launch_head_init(float* xc, const float* init_pose, const float* init_shape,
                     const float* init_cam, const float* cam_rotmat, const float* cam_intrinsics,
                     const float* img_h, int use_cam_feats, int B, int state_off, int ld, const LaunchCtx& ctx);
// rot6d_to_rotmat of one joint (pare: Gram-Schmidt, F.normalize eps 1e-12); p = the joint's 6 numbers viewed (3, 2):
// a1 = p[0], p[2], p[4]; a2 = p[1], p[3], p[5]; Rm row-major with columns b1 b2 b3
__device__ __forceinline__ void rot6d_joint(const float* p, float* Rm) {
    const float a1x = p[0], a1y = p[2], a1z = p[4];
    const float a2x = p[1], a2y = p[3], a2z = p[5];
    const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
    const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const float d = b1x * a2x + b1y * a2y + b1z * a2z;
    const float ux = a2x - d * b1x, uy = a2y - d * b1y, uz = a2z - d * b1z;
    const float n2 = fmaxf(sqrtf(ux * ux + uy * uy + uz * uz), 1e-12f);
    const float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
    const float b3x = b1y * b2z - b1z * b2y;
    const float b3y = b1z * b2x - b1x * b2z;
    const float b3z = b1x * b2y - b1y * b2x;
    Rm[0] = b1x; Rm[1] = b2x; Rm[2] = b3x; Rm[3] = b1y; Rm[4] = b2y; Rm[5] = b3y; Rm[6] = b1z; Rm[7] = b2z; Rm[8] = b3z;
}
// state: 157 regressor outputs per image at stride ld_state; ld_* = per-image strides of pred_pose / pred_shape /
// pred_cam / pred_pose_6d (216 / 10 / 3 / 144 when dense); null outputs are skipped
struct HeadFinal {
    const float* state = nullptr; long ld_state = 0;
    float *pred_pose = nullptr, *pred_shape = nullptr, *pred_cam = nullptr, *pred_pose_6d = nullptr;
    long ld_pose = 216, ld_shape = 10, ld_cam = 3, ld_p6d = 144;
    float *rot_ws = nullptr, *betas_ws = nullptr, *cam_ws = nullptr;
};
int launch_head_final(const float* state, long ld_state, float* pred_pose, float* pred_shape, float* pred_cam,
                      float* pred_pose_6d, const long ld[4], float* rotmat_ws, float* betas_ws, float* cam_ws,
                      int B, const LaunchCtx& ctx);
// pred_pose_var (B, 288) = [pose6d | act(var_pose)], pred_shape_var (B, 20) = [shape | act(var_shape)] (pare HMRHead, estimate_var);
// act: 0 none, 1 relu, 2 softplus, 3 sigmoid, 4 tanh, 5 elu (torch.nn.functional defaults)
int launch_head_var(const float* state, long ld_state, const float* var, long ld_var, int act, float* pose_var, float* shape_var,
                    int B, const LaunchCtx& ctx);
// ld_ang: per-image stride of vfov / pitch / roll (1 when dense)
int launch_camcalib_decode(const float* lv, const float* lp, const float* lr, int B, int nbins,
                           const float* img_h, const float* img_w, float* vfov, float* pitch,
                           float* roll, float* f_pix, float* R, float* K, long ld_ang, const LaunchCtx& ctx);
// per-row argmax (first maximum, NumPy NaN semantics) and / or normalised soft-argmax of (rows, nbins) logits
int launch_bins_reduce(const float* x, int rows, int nbins, int* idx, float* soft, const LaunchCtx& ctx);

// FC layers at small batch: one launch for up to three heads, one wave per output column (head.hip).  w = (N, Kp) row-major,
// zero padded to Kp; x rows ldx floats apart with Kp floats readable; out[b * ldo + n] = w[n] . x[b] + bias[n] (+ res[b * ldo + n])
struct FcGemv { const float* x; const float* w; const float* bias; const float* res; float* out; };
int launch_fc_gemv(const FcGemv* heads, int nheads, int N, int Kp, int ldx, int ldo, int B, const LaunchCtx& ctx);

int launch_cam_params(const float* pitch, const float* roll, const float* f_pix, const float* img_w, const float* img_h,
                      int B, float* R, float* K, const LaunchCtx& ctx);

// CamCalib test step (camcalib/loss.py:24-125 + camcalib/trainer.py:104-116) on three (B, nbins) logit tensors.  Every per-image
// array is (3, B), heads in the order vfov, pitch, roll; means = 7 floats (include/specmi.h: specmi_camcalib_eval)
struct CamEvalArgs {
    const float* logits[3];
    const void* target[3];        // int32 bin index (loss_type 0 / 1) or fp32 soft index (2 / 3)
    const float* gt[3];           // ground-truth angles, radians
    int B, nbins, loss_type;
    float weight[3];
    float* loss_term; int* argmax; float* soft; float* angle; float* err; float* means;
};
int launch_camcalib_eval(const CamEvalArgs& a, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// SMPL  (smpl.hip)
// ----------------------------------------------------------------------------------------
// Operands of the skinning kernel live in MFMA fragment order.  Slot of element (k, n) of a K x 32 operand of
// v_mfma_f32_32x32x2_f32 (n = row of an A operand / column of a B operand) stored as [quad][lane][4]: MFMA step st = k / 2 reads
// register element st % 4 of the 16-byte quad st / 4; lane = (k % 2) * 32 + n.
constexpr int SMPL_KQ = 28;   // K = 224 = 207 pose features + 10 betas + 1 (v_template) + 6 zeros = 112 steps = 28 quads
__host__ __device__ inline size_t frag_slot(int k, int n) {
    const int st = k >> 1;
    return ((size_t)(st >> 2) * 64 + (k & 1) * 32 + n) * 4 + (st & 3);
}

struct SmplDev {
    int V = 0;
    // [group of 32 vertices][coordinate][frag_slot(k, vertex % 32)], k: 0..206 posedirs, 207..216 shapedirs, 217 v_template
    float* dirsT = nullptr;
    float* wT = nullptr;           // [group][frag_slot(joint, vertex % 32)]: lbs_weights, 768 floats per group
    float* J_template = nullptr;   // (24,3)   = J_regressor @ v_template      (fp64 on host)
    float* J_shapedirs = nullptr;  // (24,3,10) = J_regressor @ shapedirs      (fp64 on host)
    float* J_extra = nullptr;      // (9,V)
    int* parents = nullptr;        // (24)
    int* extra_ids = nullptr;      // (21)
    int* joint_map = nullptr;      // (49)
};
struct SmplArgs {
    const float* rotmat;  // (B,24,3,3)
    const float* betas;   // (B,10)
    const float* cam;     // (B,3)
    const float* cam_rotmat;      // (B,3,3) or null (mode 1)
    const float* cam_intrinsics;  // (B,3,3) or null (mode 1)
    const float* bbox_scale;
    const float* bbox_center;
    const float* img_w;
    const float* img_h;
    float* vertices;   // (B,V,3)
    float* joints3d;   // (B,49,3)
    float* joints2d;   // (B,49,2)
    float* cam_t;      // (B,3)
    long ld_verts = 0, ld_j3d = 147, ld_j2d = 98, ld_camt = 3;   // per-image strides (0: V*3)
    // workspace
    float* pose_feat;  // (B,208)
    float* A;          // (B,24,12)
    float* posed_j;    // (B,24,3)
    int B;
    int mode;          // 0: SMPLCamHead (full-image camera), 1: SMPLHead (weak perspective)
    float focal_length;
    float img_res;
    int normalize_joints2d;
    int skin_split = -1;   // -1: by batch, 0 / 1: never / always three waves per vertex group (same bits)
    // non-null: the pose kernel first does head_final's work for its image (rot6d -> rotmat, output gather) and takes rotmat /
    // betas from there instead of a.rotmat / a.betas (one graph node less; same bits)
    const HeadFinal* final_ = nullptr;
};
int launch_smpl(const SmplDev& m, const SmplArgs& a, const LaunchCtx& ctx);
// vertices (optional) + the 24 posed kinematic joints (optional; a.posed_j receives them otherwise)
int launch_smpl_native(const SmplDev& m, const SmplArgs& a, float* joints24, const LaunchCtx& ctx);
// axis-angle (n,3) -> rotation matrices (n,3,3), smplx batch_rodrigues
int launch_rodrigues(const float* aa, float* rot, int n, const LaunchCtx& ctx);

// The vector-Jacobian product of launch_smpl (smpl_bwd.hip).  fwd: the forward's inputs, mode and its scratch (pose_feat, A,
// posed_j, vertices = a (B,V,3) scratch mesh); the forward is recomputed into them, its outputs are not read from the caller.
// Upstream gradients dense ((B,V,3), (B,49,3), (B,49,2), (B,3)), any may be null = zero; outputs (B,24,3,3), (B,10), (B,3), any
// may be null.  ws: smpl_bwd_ws_floats(V, B) floats.
struct SmplBwdArgs {
    SmplArgs fwd;
    const float *g_vertices, *g_joints3d, *g_joints2d, *g_cam_t;
    float *g_rotmat, *g_betas, *g_cam;
    float* ws;
};
size_t smpl_bwd_ws_floats(int V, int B);
int launch_smpl_backward(const SmplDev& m, const SmplBwdArgs& a, const LaunchCtx& ctx);
// rot6d_joint on its own: x6d (n,6) -> rotmat (n,3,3)
int launch_rot6d_forward(const float* x6d, float* rotmat, int n, const LaunchCtx& ctx);
// the backward of rot6d_joint: x6d (n,6), g_rotmat (n,3,3) -> g_x6d (n,6)
int launch_rot6d_backward(const float* x6d, const float* g_rotmat, float* g_x6d, int n, const LaunchCtx& ctx);

// pare's HMRHead regressor for training (head_bwd.hip): the ten parameters where torch keeps them ((N, K) row-major weights),
// xf (B, F) rows ld_xf apart, cam_feats (B, 7) with C = 7 else unused, masks uint8 (2 n_iter, B, 1024) or null (eval: scale is
// not read).  The tape is head_tape_floats(B, n_iter) floats; ws is head_train_fwd_ws_floats(B) resp.
// head_train_bwd_ws_floats(B, n_iter) floats.  g_xf and the members of HeadTrainGrads may be null (not wanted).
struct HeadTrainParams { const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *decpose_w, *decpose_b, *decshape_w, *decshape_b, *deccam_w, *deccam_b; };
struct HeadTrainGrads { float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *decpose_w, *decpose_b, *decshape_w, *decshape_b, *deccam_w, *deccam_b; };
struct HeadTrainArgs {
    HeadTrainParams p;
    const float* xf; long ld_xf;
    const float* cam_feats;
    const uint8_t* masks; float scale;
    int B, F, C, n_iter;
};
size_t head_tape_floats(int B, int n_iter);
size_t head_train_fwd_ws_floats(int B);
size_t head_train_bwd_ws_floats(int B, int n_iter);
int launch_head_train_forward(const HeadTrainArgs& a, const float* init_state, float* state, float* tape, float* ws, const LaunchCtx& ctx);
int launch_head_backward(const HeadTrainArgs& a, const float* tape, const float* g_state, float* g_xf, const HeadTrainGrads& g, float* ws,
                         const LaunchCtx& ctx);

// CamCalib's three FC heads for training (head_bwd.hip): [head vfov / pitch / roll][layer 0 .. L-1] weights (out, in) row-major
// and biases where torch keeps them; xf (B, F) rows ld_xf apart; widths F -> Hc -> .. -> nbins.  tape: cam_head_tape_floats
// floats = the (3, L - 1, B, Hc) hidden rows; logits / g_logits (3, B, nbins) dense; ws: cam_head_bwd_ws_floats floats.  g_xf and
// the members of CamHeadGrads may be null (not wanted).  grouped: the three heads' independent products as one launch each.
struct CamHeadParams { const float* w[3][3]; const float* b[3][3]; };
struct CamHeadGrads { float* w[3][3]; float* b[3][3]; };
struct CamHeadArgs {
    CamHeadParams p;
    const float* xf; long ld_xf;
    int B, F, L, Hc, nbins;
    bool grouped;
};
size_t cam_head_tape_floats(int B, int L, int Hc);
size_t cam_head_bwd_ws_floats(int B, int L, int Hc);
int launch_cam_head_train_forward(const CamHeadArgs& a, float* tape, float* logits, const LaunchCtx& ctx);
int launch_cam_head_backward(const CamHeadArgs& a, const float* tape, const float* g_logits, float* g_xf, const CamHeadGrads& g, float* ws,
                             const LaunchCtx& ctx);

// CameraRegressorLoss for training (camcalib_bwd.hip; include/specmi.h: specmi_camcalib_loss): the loss part of CamEvalArgs.
// loss_term (3, B), means 4 floats; the backward writes three (B, nbins) gradients from g_means (4).
struct CamLossArgs {
    const float* logits[3];
    const void* target[3];        // int32 bin index (loss_type 0 / 1) or fp32 soft index (2 / 3)
    int B, nbins, loss_type;
    float weight[3];
    float* loss_term; float* means;
};
int launch_camcalib_loss(const CamLossArgs& a, const LaunchCtx& ctx);
int launch_camcalib_loss_backward(const CamLossArgs& a, const float* g_means, float* const g_logits[3], const LaunchCtx& ctx);

// One fused ResNet layer for training (conv_bwd.hip; include/specmi.h: specmi_conv2d_train_forward): x (B, H, W, Cin) and
// y / res / g_y / g_res (B, OH, OW, Cout) dense NHWC, w torch's OIHW tensor on the device, scale / shift (Cout) on the device.
// The backward's ws is conv_bwd_ws_floats floats (G = g_z * scale); g_x, g_w and g_res may be null (not wanted), g_x_add may be
// null or g_x itself.
struct ConvTrainArgs {
    const float* x; const float* w; const float* scale; const float* shift;
    int B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad;
};
int conv_wgrad_splits(int B, int OH, int Cin, int Cout, int KH, int KW);   // S of the weight gradient, from the shape alone
size_t conv_bwd_ws_floats(const ConvTrainArgs& t, int S);   // G and, with S > 1 splits of the weight gradient, its S partial products
size_t conv_fwd_ws_floats(const ConvTrainArgs& t);      // the forward's ws: the weights transposed to [tap][ci][o]
int launch_conv_train_forward(const ConvTrainArgs& t, const float* residual, int relu, float* y, float* ws, const LaunchCtx& ctx);
int launch_conv_backward(const ConvTrainArgs& t, const float* y, int relu, const float* g_y, const float* g_x_add, float* g_x, float* g_w,
                         float* g_res, float* ws, int S, const LaunchCtx& ctx);    // S: 1 <= S <= B OH splits of the weight gradient

// BatchNorm in training mode with its backward (bn_train.hip; include/specmi.h: specmi_batchnorm_train_forward): z and
// y / residual / g_y / g_z / g_res dense (M, C) fp32, C contiguous; gamma / beta / mean / invstd / the running statistics (C).  ws is
// bn_ws_floats floats for both calls.  residual and the two running statistics may be null; in the backward g_z, g_gamma, g_beta
// and g_res may be null (not wanted), y is read only with relu, g_res may be g_y itself.
struct BnArgs {
    const float* z; const float* gamma;
    int M, C, relu;
};
size_t bn_ws_floats(int M, int C);
int launch_bn_train_forward(const BnArgs& a, const float* beta, const float* residual, float eps, float f, float* running_mean,
                            float* running_var, float* y, float* mean, float* invstd, float* ws, const LaunchCtx& ctx);
int launch_bn_backward(const BnArgs& a, const float* mean, const float* invstd, const float* y, const float* g_y, float* g_z, float* g_gamma,
                       float* g_beta, float* g_res, float* ws, const LaunchCtx& ctx);

// MaxPool2d(3, 2, 1) for training (pool_bwd.hip; include/specmi.h: specmi_maxpool3x3s2_train_forward): x / g_x (B, H, W, C) and
// y / g_y (B, OH, OW, C) dense NHWC fp32, idx (B, OH, OW, C) uint8 = the winning tap ky * 3 + kx.  Every dimension >= 1 and fewer
// than 2^31 elements (hipErrorInvalidValue otherwise); the vector form is chosen from C and the pointers' alignment.
int launch_maxpool_train_forward(const float* x, int B, int H, int W, int C, float* y, unsigned char* idx, const LaunchCtx& ctx);
int launch_maxpool_backward(const float* g_y, const unsigned char* idx, int B, int H, int W, int C, float* g_x, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// evaluation metrics  (eval.hip)
// ----------------------------------------------------------------------------------------
int launch_eval_mesh(const float* pred, const float* gt, int B, int V, const float* Jr, int J, const int* sel, int nsel,
                     float* mpjpe, float* pampjpe, float* v2v, const LaunchCtx& ctx);
int launch_eval_joints(const float* pred, const float* gt, int B, int J, float* mpjpe, float* pampjpe,
                       const LaunchCtx& ctx);
int launch_eval_step(const float* pred, const float* gt, int B, int V, const float* Jr, int J, const int* sel, int nsel,
                     const float* pj, const float* gj, int Jk, float* err_sel, float* pa_err_sel, float* err_k, float* pa_err_k,
                     float* v2v, const LaunchCtx& ctx);
int launch_regress_joints(const float* verts, int B, int V, const float* Jr, int J, float* out, const LaunchCtx& ctx);
int launch_rotate_points(const float* R, const float* x, int B, int N, float* out, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// SPEC's loss modules, forward value  (loss.hip)
// ----------------------------------------------------------------------------------------
// HMRLoss (mode 0) / HMRCamLoss (mode 1) of spec/losses.py; shapes, rows of `terms` and the order of `means`: include/specmi.h,
// specmi_hmr_loss.  gt_vertices, orig_shape and scale may be null where the header says so; counts and means may be null.
struct HmrLossArgs {
    int mode, B, V;
    const float *pred_pose, *pred_shape, *pred_cam, *joints3d, *joints2d, *vertices;
    const float *pose, *betas, *pose_conf, *pose_3d, *keypoints, *gt_vertices;
    const int *has_smpl, *has_pose_3d;
    const float *orig_shape, *scale;
    float w_shape, w_keypoint, w_pose, w_beta, w_openpose, w_gt, w_loss;
    float* terms; int* counts; float* means;
};
int launch_hmr_loss(const HmrLossArgs& a, const LaunchCtx& ctx);
// The gradient of the seven means (include/specmi.h: specmi_hmr_loss_backward): a = the forward's arguments with the `terms` and
// `counts` it produced (read here; means is not); g_means (7) upstream; any output may be null.
struct HmrLossGrads {
    const float* g_means;
    float *g_pred_pose, *g_pred_shape, *g_pred_cam, *g_joints3d, *g_joints2d, *g_vertices;
};
int launch_hmr_loss_backward(const HmrLossArgs& a, const HmrLossGrads& g, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// crop + normalise  (preprocess.hip)
// ----------------------------------------------------------------------------------------
// Every producer: f16 = false -> `out` is the fp32 NCHW image; f16 = true -> `out` is NHWC8 fp16 (include/specmi.h), 16-byte aligned
// frame_of != nullptr: `frame` is a slab of nframes equal-sized frames and crop d is cut from frame frame_of[d] (device, (n) int32)
int launch_crop_normalize(const unsigned char* frame, int H, int W, const float* bboxes, int n, float scale, int S,
                          void* out, unsigned char* raw, float* bbox_scale, float* bbox_center, const LaunchCtx& ctx,
                          const int* frame_of = nullptr, int nframes = 1, bool f16 = false);

// dataset crop: integer boxes (n,4) [ulx, uly, brx, bry] -> cv2.resize-style bilinear to S x S + ToTensor + Normalize
int launch_crop_resize_normalize(const unsigned char* frame, int H, int W, const int* boxes, int n, int S, void* out,
                                 const LaunchCtx& ctx, bool f16 = false);

// The two crops from frames of DIFFERENT sizes: `frames` is a uint8 slab, `tab` (device) one CropFrame per frame - byte offset
// in the slab, H, W -, crop d is cut from frame frame_of[d] (device, (n) int32, clamped into [0, nframes)).  The caller
// guarantees H, W < 2^24 and a slab below 4 GiB (32-bit offsets); slab_bytes only feeds the profiler's byte count
struct CropFrame { unsigned off; int H, W, pad_; };
int launch_crop_normalize_ragged(const unsigned char* frames, const CropFrame* tab, int nframes, double slab_bytes, const int* frame_of,
                                 const float* bboxes, int n, float scale, int S, void* out, unsigned char* raw, float* bbox_scale,
                                 float* bbox_center, const LaunchCtx& ctx, bool f16 = false);
int launch_crop_resize_normalize_ragged(const unsigned char* frames, const CropFrame* tab, int nframes, double slab_bytes,
                                        const int* frame_of, const int* boxes, int n, int S, void* out, const LaunchCtx& ctx,
                                        bool f16 = false);

// Pillow-exact bilinear resize + ToTensor + Normalize (CamCalib frame transform)
int pillow_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk);
int launch_resize_normalize(const unsigned char* frame, int H, int W, int OH, int OW, const int* hb, const int* hk, int ksh,
                            const int* vb, const int* vk, int ksv, void* out, unsigned char* raw, const LaunchCtx& ctx, bool f16 = false);

// One frame of a ragged batch as the device reads it (kRaggedRec ints at the head of the table buffer): byte offset of the
// frame in the slab, source and target size, int offsets of its coefficient tables (pillow_coeffs layout) in the same buffer,
// byte offset of its H x OW x 3 intermediate in the uint8 workspace; resample = 0: target size == size, convert only
struct RaggedFrame { unsigned src_off; int H, W, OH, OW, hb, hk, ksh, vb, vk, ksv; unsigned tmp_off; int resample, pad_[3]; };
constexpr int kRaggedRec = sizeof(RaggedFrame) / 4;
// max_hpass_px = max over the resampled frames of H * OW (0: no frame is resampled, the horizontal launch is skipped)
int launch_resize_normalize_ragged(const unsigned char* frames, const int* tab, unsigned char* tmp, int n, int max_hpass_px,
                                   int Hmax, int Wmax, double src_bytes, double tmp_bytes, void* out, const LaunchCtx& ctx,
                                   bool f16 = false);

// ----------------------------------------------------------------------------------------
// perspective views out of an equirectangular panorama  (panorama.hip)
// ----------------------------------------------------------------------------------------
// What one view fixes, as the device reads it: sin / cos of elevation and roll, numpy.linspace's start / stop / step per
// axis, the view's byte offset in the output slab and its size
struct PanoView {
    double sin_el, cos_el, azimuth, cos_roll, sin_roll, neg_sin_roll, x_start, x_stop, x_step, y_start, y_stop, y_step;
    long long out_off;
    int H, W;
};
// view = [elevation, azimuth, roll (rad), vfov (deg), ratio]; false: (H, W) is not (H, round(H / (1 / ratio)))
bool make_pano_view(const double* view, int H, int W, long long out_off, PanoView& pv);
int pano_view_tiles(int H, int W);      // workgroups a view of this size takes
int launch_pano_extract(const unsigned char* pano, int PH, int PW, const PanoView* views, int n, int max_tiles, double out_bytes,
                        unsigned char* out, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// mesh overlay / side view rasteriser  (render.hip)
// ----------------------------------------------------------------------------------------
// One specmi_render_meshes call as the three kernels read it.  keys / sws / normals / lowest are the four parts of the
// handle's render workspace (render_ws_layout); screen, id_map, depth are the caller's optional outputs.
struct RenderArgs {
    const float* vertices;      // (M, V, 3)
    const int* faces;           // (F, 3)
    const float* cam_t;         // (M, 3)
    const float* R;             // (3, 3)
    const unsigned char* frame; // H rows of W x 3 bytes, in_pitch bytes apart; unused in side view
    float fx, fy, cx, cy, rgb[3];
    int M, V, F, H, W, side, ground, cull;
    unsigned in_pitch, out_pitch;   // bytes from one row of frame / out to the next (3 W: dense)
    unsigned long long* keys;   // (H, W): float_bits(z) << 32 | id, all ones = nothing drawn; null = nothing drawn anywhere
    int* sws;                   // (M, V, 3): snapped x, y and the bits of z
    int* normals;               // (M, V, 3): fixed-point sums of the incident face normals
    int* lowest;                // the lowest y of the scene as an ordered int (ground plane)
    unsigned char* out;         // H rows of W x 3 bytes, out_pitch bytes apart
    int* id_map;                // (H, W) or null
    float* depth;               // (H, W) or null
    int* screen;                // (M, V, 3) or null: the caller's copy of sws
};
// byte offsets of keys, sws, normals, lowest in the workspace -> its size
size_t render_ws_layout(int M, int V, int H, int W, size_t off[4]);
int launch_render(const RenderArgs& a, bool thread_per_triangle, const LaunchCtx& ctx);

// One view of a specmi_render_views call as the device reads it (28 ints).  pair0 = the view's first (view, mesh) pair, which
// numbers its snapped vertices, normal sums and `screen` part; px0 = its first pixel in id_map / depth; key0 = its first key
// (-1: count == 0, no key plane); offsets and pitches in bytes (slabs stay below 4 GiB)
struct RenderView {
    float R[9], fx, fy, cx, cy;
    int H, W, mesh0, count, side, ground, cull, pair0, px0, key0;
    unsigned in_off, in_pitch, out_off, out_pitch;
    int pad_;
};
constexpr int kRenderViewRec = sizeof(RenderView) / 4;
// One specmi_render_views call as the three kernels read it.  views, px_prefix (nviews + 1) and pair_view (npairs: the view of
// each pair) are the three parts of the handle's view table; keys / sws / normals / lowest the four of its render workspace
// (render_views_ws_layout); id_map, depth, screen the caller's optional outputs
struct RenderViewsArgs {
    const float* vertices;      // (Mtot, V, 3)
    const int* faces;           // (F, 3)
    const float* cam_t;         // (Mtot, 3)
    const RenderView* views;
    const int* px_prefix;
    const int* pair_view;
    const unsigned char* in_slab;
    unsigned char* out_slab;
    float rgb[3];
    int V, F, nviews, npairs, total_px;
    unsigned long long* keys;
    int *sws, *normals, *lowest;
    int* id_map;
    float* depth;
    int* screen;
};
// byte offsets of keys, sws, normals, lowest in the workspace -> its size
size_t render_views_ws_layout(long long keys, long long pairs, int V, int nviews, size_t off[4]);
int launch_render_views(const RenderViewsArgs& b, long long keys, bool any_ground, bool thread_per_triangle, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// 2D keypoint skeletons  (draw.hip)
// ----------------------------------------------------------------------------------------
constexpr int kDrawMaxSide = 8192, kDrawMaxCoord = 16383, kDrawMaxRadius = 64, kDrawMaxThickness = 64;
// One frame of a specmi_draw_skeletons call as the device reads it (10 ints): byte offset of its first pixel in the slab and
// bytes from one row to the next, its size, its detections det0 .. det0 + count - 1, its first tile among the call's tiles
// (a frame with count == 0 has none) and its tiles per row
struct DrawFrame { long long off, pitch; int H, W, det0, count, tile0, tiles_x; };
constexpr int kDrawFrameRec = sizeof(DrawFrame) / 4;
// One specmi_draw_skeletons call as the kernel reads it.  frames (nframes records) and bones (NB x 2) are the two parts of the
// handle's draw table; rgb = joints, even bones, odd bones as r | g << 8 | b << 16
struct DrawArgs {
    const float* kp;            // (Mtot, J, D)
    const DrawFrame* frames;
    const int* bones;
    unsigned char* slab;
    int nframes, J, D, NB, radius, thickness;
    float thr;
    unsigned rgb[3];
};
// the tiles a frame of this size takes -> and its tiles per row
int draw_frame_tiles(int H, int W, int* tiles_x);
int launch_draw_skeletons(const DrawArgs& a, int total_tiles, double kp_bytes, double px, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// horizon lines and captions: strips, mask blends, Pillow's wide line; denormalised frames  (marks.hip)
// ----------------------------------------------------------------------------------------
// THE MARK RECORD of specmi_draw_marks as the caller writes it (include/specmi.h states the same): kMarkRec int64 per mark,
//   [kind, r | g << 8 | b << 16, p0 .. p5] with  strip: p0 = y0, p1 = y1 (rows [y0, y1));
//   mask blend: p0 = x, p1 = y, p2 = mw, p3 = mh, p4 = byte offset of the mask in the mask buffer;
//   wide line: p0 .. p3 = x0, y0, x1, y1, p4 = width.  Unused parameters are ignored.
constexpr int kMarkStrip = 0, kMarkMask = 1, kMarkLine = 2, kMarkRec = 8;
constexpr int kMarkMaxSide = 8192, kMarkMinWidth = 2, kMarkMaxWidth = 64, kMarkMaxCoord = 100000, kMarkMaxMaskSide = 8192, kMarkMaxMaskPos = 16383;
constexpr int kMarkTileW = 64, kMarkTileH = 16;       // one 256-thread workgroup: a wavefront per row, four rows per thread
// One edge of a wide line's quadrilateral as Pillow's add_edge keeps it; dx = (float)(x1 - x0) / (float)(y1 - y0), 0 when horiz
struct MarkEdge { int ymin, ymax, x0, y0; float dx; int xmin, xmax, horiz; };
// One mark as the device reads it (40 ints).  strip: a = y0, b = y1; mask: a = x, b = y, c = mw, d = mh, off; line: e[4]
struct MarkDev { int kind; unsigned rgb; int a, b, c, d; long long off; MarkEdge e[4]; };
constexpr int kMarkDevRec = sizeof(MarkDev) / 4;
// One frame (8 ints): byte offset of its first pixel, bytes from row to row, size, its marks mark0 .. mark0 + count - 1
struct MarkFrame { long long off, pitch; int H, W, mark0, count; };
constexpr int kMarkFrameRec = sizeof(MarkFrame) / 4;
// One call as the kernel reads it.  frames, marks and tiles are the three parts of the handle's marks table; a tile is two ints:
// its frame, and tile row << 16 | tile column
struct MarksArgs {
    const MarkFrame* frames;
    const MarkDev* marks;
    const int* tiles;
    const unsigned char* masks;
    unsigned char* slab;
    int ntiles;
};
// Pillow's ROUND_UP / ROUND_DOWN on an fp32 value: the + 0.5F is an fp32 addition.  |f| stays far below 2^31 here
__host__ __device__ inline int mark_ru(float f) { return (int)(f >= 0.f ? floorf(f + 0.5f) : -floorf(fabsf(f) + 0.5f)); }
__host__ __device__ inline int mark_rd(float f) { return (int)(f >= 0.f ? ceilf(f - 0.5f) : -ceilf(fabsf(f) - 0.5f)); }
// where edge e crosses row y: a separately rounded fp32 multiply and add, as Pillow's x86 build evaluates it - never an FMA.
// The pragma is what keeps the two apart on host and device alike: HIP's __fmul_rn / __fadd_rn are a plain * and + to the
// compiler, which contracts them under the build's default -ffp-contract=fast
__host__ __device__ inline float mark_edge_x(const MarkEdge& e, int y) {
#pragma clang fp contract(off)
    const float p = (float)(y - e.y0) * e.dx;
    return p + (float)e.x0;
}
// the span [xa, xb] (unclipped; xa > xb: none) that the non-horizontal edges of a line give row y: RU(min xx) .. RD(max xx)
// over the edges with ymin <= y <= ymax.  One function for the kernel and for the host's tile list
__host__ __device__ inline void mark_line_span(const MarkEdge* e, int y, int& xa, int& xb) {
    float lo = 3.0e38f, hi = -3.0e38f;
    bool any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (!e[i].horiz && y >= e[i].ymin && y <= e[i].ymax) {
            const float xx = mark_edge_x(e[i], y);
            lo = fminf(lo, xx); hi = fmaxf(hi, xx);
            any = true;
        }
    xa = any ? mark_ru(lo) : 1;
    xb = any ? mark_rd(hi) : 0;
}
int launch_draw_marks(const MarksArgs& a, double px, const LaunchCtx& ctx);
struct DenormArgs {
    const float* x;             // image `index` of (B, 3, Hp, Wp): already offset to it
    unsigned char* out;         // the frame's first pixel
    long long pitch, plane;     // bytes per output row; Hp * Wp
    int h, w, Wp;
    float mean[3], std[3];
};
int launch_denormalize_u8(const DenormArgs& a, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// torchvision's ColorJitter on the frames of a slab, in Pillow's bytes  (color_jitter.hip)
// ----------------------------------------------------------------------------------------
constexpr int kJitterBrightness = 0, kJitterContrast = 1, kJitterSaturation = 2, kJitterHue = 3;
constexpr int kJitterMaxSide = 8192;
constexpr int kJitterTileW = 256, kJitterTileH = 16;  // one 256-thread workgroup: four pixels of a row per thread, four rows in turn
// THE JITTER RECORD of specmi_color_jitter as the caller writes it (include/specmi.h states the same), eight int32 words: the
// ids of the operations in application order (-1: none), the fp32 factors of brightness, contrast and saturation, the hue shift.
// The device reads the same layout with the ids packed to the front
struct JitterRec { int op[4]; float f[3]; int k; };
constexpr int kJitterRec = sizeof(JitterRec) / 4;
// One frame as the device reads it (24 ints): its rectangle in each slab (byte offset, pitch), its size, its first tile among the
// apply launch's and among the stat launch's (a frame without contrast has none there), its tiles per row, how many
// operations it has and how many of them come before contrast (-1: no contrast)
struct JitterFrame { long long in_off, in_pitch, out_off, out_pitch; int H, W, tile0, stile0, tiles_x, nops, npre, pad_; JitterRec rec; };
constexpr int kJitterFrameRec = sizeof(JitterFrame) / 4;
// One call as the kernels read it: frames = the handle's jitter table, sums = one 64-bit sum of L per frame (its workspace)
struct JitterArgs {
    const JitterFrame* frames;
    const unsigned char* in;
    unsigned char* out;
    unsigned long long* sums;
    int nframes;
};
// the tiles a frame of this size takes -> and its tiles per row
int jitter_frame_tiles(int H, int W, int* tiles_x);
// stat_tiles == 0: no frame has contrast, one launch
int launch_color_jitter(const JitterArgs& a, int stat_tiles, int tiles, double stat_px, double px, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// baseline JPEG encoder  (jpeg.hip)
// ----------------------------------------------------------------------------------------
constexpr int kJpegHeaderBytes = 623;
constexpr int kJpegMcuBytes = 1248;       // an MCU codes into at most 6 * (22 + 63 * 26) = 9960 bits = 1245 bytes; 1248 = 16 * 78
constexpr int kJpegMcuChunk = 256;        // MCUs per workgroup of the counting and writing kernels
constexpr int kJpegByteChunk = 4096;      // unstuffed scan bytes per workgroup of the stuffing kernels (16 per thread)
constexpr long long kJpegMaxMcus = 1 << 24;
// One picture of a specmi_jpeg_encode call as the device reads it (16 ints): the four byte fields of its record, its size, its
// MCU grid, and where its MCUs, MCU chunks and byte chunks begin among the call's
struct JpegPic { long long in_off, in_pitch, out_off, cap; int H, W, mx, my, mcu0, mchunk0, bchunk0, pad; };
constexpr int kJpegPicRec = sizeof(JpegPic) / 4;
// What a quality decides, built on the host (jpeg_build_tables): the divisors 8 Q in natural order (table 0 luma, 1 chroma), the
// Annex-K codes and lengths by symbol, and the header with H = W = 0
struct JpegTables {
    unsigned short div[2][64];
    unsigned short dc_code[2][12];
    unsigned char dc_len[2][12];
    unsigned short ac_code[2][256];
    unsigned char ac_len[2][256];
    unsigned char header[624];
};
static_assert(sizeof(JpegTables) % 4 == 0, "the tables follow the picture records in a table of ints");
struct JpegArgs {
    const unsigned char* in;
    unsigned char* out;
    const JpegPic* pics;
    const JpegTables* tabs;
    long long* sizes;                     // (n): every picture's true encoded length
    short* coef;                          // (mcus, 6, 64) quantised coefficients in zigzag order
    unsigned* mcu_bits;                   // (mcus)
    unsigned* mchunk_sum;                 // (mchunks) bits of a chunk's MCUs
    unsigned long long* mchunk_base;      // (mchunks) bits of the picture's chunks before it
    unsigned long long* pic_bits;         // (n)
    unsigned* bitbuf;                     // (mcus * kJpegMcuBytes / 4) the unstuffed scans as big-endian words, zeroed per call
    unsigned* bchunk_ff;                  // (bchunks) 0xFF bytes of a byte chunk
    unsigned long long* bchunk_base;      // (bchunks) 0xFF bytes of the picture's chunks before it
    int n, mcus, mchunks, bchunks;
};
void jpeg_build_tables(int quality, JpegTables* t);
// byte offsets of coef, mcu_bits, mchunk_sum, mchunk_base, pic_bits, bitbuf, bchunk_ff, bchunk_base in the workspace -> its size
size_t jpeg_ws_layout(int n, long long mcus, long long mchunks, long long bchunks, size_t off[8]);
int launch_jpeg_encode(const JpegArgs& a, double in_bytes, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// PNG encoder  (png.hip)
// ----------------------------------------------------------------------------------------
constexpr int kPngSegment = 32768;                 // bytes of the filtered stream one workgroup codes on its own
constexpr int kPngSegStride = kPngSegment + 32;    // room of a segment's blocks in the workspace: a stored block takes 5 + 32768 bytes
constexpr int kPngOverhead = 63;                   // signature 8, IHDR 25, IDAT's length, type and CRC 12, zlib's header 2 and Adler-32 4, IEND 12
constexpr int kPngHeaderBytes = 33;                // signature + IHDR
constexpr long long kPngMaxSegments = 1 << 23;    // a workgroup of 256 per segment: HIP refuses a launch of 2^32 threads or more
constexpr unsigned kPngFilterGrid = 1u << 20;     // workgroups of the filter kernel at most; each takes every 2^20th row
// One picture of a specmi_png_encode call as the device reads it (18 ints): the four byte fields of its record, where its filtered
// stream lies in the workspace and how long it is, its size, and where its rows and segments begin among the call's
struct PngPic { long long in_off, in_pitch, out_off, cap, filt_off, stream; int H, W, row0, seg0, nseg, pad; };
constexpr int kPngPicRec = sizeof(PngPic) / 4;
struct PngArgs {
    const unsigned char* in;
    unsigned char* out;
    const PngPic* pics;
    long long* sizes;                     // (n): every picture's true encoded length
    unsigned char* filt;                  // the filtered streams, each picture's from a multiple of 256
    unsigned* segbuf;                     // (segs * kPngSegStride / 4) every segment's deflate blocks, zeroed per call
    unsigned* seg_bytes;                  // (segs) bytes of a segment's blocks
    unsigned* seg_sum;                    // (segs, 2) Adler-32 partials: the sum of the bytes, the sum of (n - i) byte[i] mod 65521
    unsigned long long* seg_base;         // (segs) bytes of the picture's segments before it
    unsigned* seg_crc;                    // (segs) the segment's blocks' share of IDAT's CRC
    unsigned* pic_adler;                  // (n)
    int n, rows, segs;
};
long long png_bound(int H, int W);
void png_header(int H, int W, unsigned char* out);
// byte offsets of filt, segbuf, seg_bytes, seg_sum, seg_base, seg_crc, pic_adler in the workspace -> its size
size_t png_ws_layout(int n, long long filt_bytes, long long segs, size_t off[7]);
int launch_png_encode(const PngArgs& a, double in_bytes, const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// baseline JPEG decoder  (jpeg_dec.hip)
// ----------------------------------------------------------------------------------------
constexpr int kJdecSubBytes = 128;        // a subsequence: 1024 scan bits = 128 bytes of the file, one lane
constexpr int kJdecGroup = 256;           // subsequences per workgroup of the sync and write kernels
constexpr long long kJdecMaxMcus = 1 << 24;
// One Huffman table as the lanes read it: by the next 8 bits `length << 8 | symbol` (0: the code is longer), and for the
// lengths 9 .. 16 the largest code (-1: none) and what added to a code gives its place in vals
struct JdecHuff {
    unsigned short lut[256];
    int maxcode[18], valoff[18];
    unsigned char vals[256];
};
// One file of a specmi_jpeg_decode call as the device reads it.  Table slots: dc[0..1], ac[0..1]; q per component, natural order
struct JdecFile {
    long long scan_off, scan_len;         // the scan's first byte in the input slab and its length (the EOI excluded)
    long long out_off, pitch;
    long long block0, plane0;             // the file's first block in the coefficient workspace, first byte in the plane workspace
    int H, W, mx, my;
    int s420, bpm, nblocks, nsub;         // 4:2:0 or 4:4:4; blocks per MCU (6 or 3); blocks; subsequences
    int lane0, group0, bchunk0, pchunk0;  // where its lanes (a multiple of kJdecGroup), groups, 256-block and 256-pixel chunks begin
    unsigned char tdc[4], tac[4];         // table slot per component
    unsigned short q[3][64];
    JdecHuff huff[4];
};
static_assert(sizeof(JdecFile) % 8 == 0, "records follow each other in a table of ints");
struct JdecArgs {
    const unsigned char* in;
    unsigned char* out;
    const JdecFile* files;
    int* status;                          // (n) one word per file, zeroed per call, bits joined with atomicOr
    short* coef;                          // (blocks, 64) quantised coefficients in natural order, zeroed per call
    unsigned char* planes;                // per file Y, Cb, Cr in whole MCUs
    unsigned* entry;                      // (lanes) the entry state a lane last decoded from
    unsigned* exits;                      // (lanes) its exit state
    int* count;                           // (lanes) blocks it completed
    int* first;                           // (lanes) blocks of its file completed before it
    unsigned* gexit;                      // (2, groups) every group's last exit as the previous pass left it / as this pass leaves it
    unsigned* changed;                    // one word per call: did the pass change a lane
    int n, groups, bchunks, pchunks;
};
enum { JDEC_SUPPORTED = 0, JDEC_NOT_JPEG, JDEC_TRUNCATED, JDEC_PROGRESSIVE, JDEC_SOF, JDEC_PRECISION, JDEC_COMPONENTS, JDEC_SAMPLING,
       JDEC_RESTART, JDEC_SCAN, JDEC_COLOURSPACE, JDEC_TABLES, JDEC_SIZE, JDEC_TRAILING };
// rule 1 on the host: -> a JDEC_ reason; on JDEC_SUPPORTED f holds H, W, s420, the scan's range within the file (scan_off,
// scan_len), the quantisers, the tables and their selectors
int jpeg_probe(const unsigned char* d, size_t n, JdecFile* f);
// byte offsets of coef, planes, entry, [exits, count, first, gexit, changed] in the workspace -> its size
size_t jdec_ws_layout(long long blocks, long long plane_bytes, long long lanes, long long groups, size_t off[8]);
// the whole sequence; max_groups: the groups of the file that has most; -> passes run
int launch_jpeg_decode(const JdecArgs& a, long long blocks, long long lanes, int max_groups, double in_bytes, double out_bytes, int* passes,
                       const LaunchCtx& ctx);

// ----------------------------------------------------------------------------------------
// PNG decoder  (png_dec.hip)
// ----------------------------------------------------------------------------------------
constexpr int kPdecLanes = 256;           // lanes of the inflate workgroup = subsequences per window
constexpr int kPdecSubBits = 512;         // a subsequence: 512 bits of the zlib stream, one lane
constexpr int kPdecMaxRec = kPdecLanes * kPdecSubBits / 2;     // match records of one window at most: a match takes 2 bits or more
constexpr int kPdecAdlerChunk = 32768;    // inflated bytes per workgroup of the Adler-32 stage
constexpr long long kPdecMaxRaw = 1ll << 31;      // inflated bytes of one call at most (a record's destination is 32 bits)
// One file of a specmi_png_decode call as the device reads it
struct PdecFile {
    long long stream_off, stream_len;     // the zlib stream in the input slab
    long long out_off, pitch;
    long long raw_off, raw_len;           // the inflated stream in the workspace (a multiple of 256) and its length H (1 + W bpp)
    int H, W, bpp, nch;                   // bytes per pixel in the file (1, 3, 2, 4); channels the picture keeps (1 or 3)
    int chunk0, nchunk;                   // its Adler chunks among the call's
};
static_assert(sizeof(PdecFile) % 8 == 0, "records follow each other in a table of ints");
struct PdecArgs {
    const unsigned char* in;
    unsigned char* out;
    const PdecFile* files;
    int* status;                          // (n) one word per file, zeroed per call, bits joined with atomicOr
    unsigned char* raw;                   // the inflated streams
    uint2* rec;                           // (n, kPdecMaxRec) the current window's matches: destination - window's first byte, length | distance << 9
    uint2* sums;                          // (chunks) Adler-32 partials
    int n, chunks;
};
enum { PDEC_SUPPORTED = 0, PDEC_NOT_PNG, PDEC_TRUNCATED, PDEC_CRC, PDEC_DEPTH, PDEC_PALETTE, PDEC_INTERLACED, PDEC_ANIMATED, PDEC_CHUNK,
       PDEC_SIZE, PDEC_TRAILING };
// rule 1 on the host: -> a PDEC_ reason; on PDEC_SUPPORTED H, W, the colour type and the IDAT payload ranges [offset, length] (the
// first max_ranges of them; *nranges: how many the file has)
int png_probe(const unsigned char* d, size_t n, int* H, int* W, int* ctype, long long* ranges, int max_ranges, int* nranges);
// byte offsets of raw, rec, sums in the workspace -> its size
size_t pdec_ws_layout(int n, long long raw_bytes, long long chunks, size_t off[3]);
int launch_png_decode(const PdecArgs& a, double in_bytes, double raw_bytes, double out_bytes, const LaunchCtx& ctx);

}  // namespace specmi
