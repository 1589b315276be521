// head.hip - small per-image kernels around the regressor GEMMs (gfx950).
//
//   * head_init_kernel   : builds the IEF state row of HMRHead (pare, call site
//     spec/models/hmr.py:94-98): xc = [xf(2048) | pose6d(144) | shape(10) | cam(3) |
//     rot6d(cam_rotmat)(6) | vfov(1) | zero pad] with vfov = 2*atan(img_h / (2*K[0,0]))
//     (spec/models/hmr.py:95).  xf is written by the avg-pool kernel; the three dec* GEMMs
//     update the state columns in place (residual epilogue), so torch.cat is never executed.
//   * head_final_kernel  : rot6d_to_rotmat (Gram-Schmidt, F.normalize eps 1e-12) and the
//     output gather pred_pose / pred_shape / pred_cam / pred_pose_6d.
//   * camcalib_decode_kernel : soft-argmax decode of the three 256-bin logit rows
//     (camcalib/cam_utils.py:110-133: softmax expectation -> [-1,1] -> affine to radians),
//     f = h/2/tan(vfov/2) (scripts/camcalib_demo.py:129), R = euler2matrix([pitch,0,roll])
//     via the quaternion route and K with K[2,2] = 0 (spec/utils/cam_params.py:37-46).
//     One wave per (image, head): 64-lane shuffle reductions, no LDS traffic for the softmax.
#include "specmi_internal.h"
#include "camcalib_rows.h"

namespace specmi {

__global__ void __launch_bounds__(256) head_init_kernel(const HeadInit a) { head_init_row(a, blockIdx.x, threadIdx.x, blockDim.x); }

int launch_head_init(float* xc, const float* init_pose, const float* init_shape, const float* init_cam,
                     const float* cam_rotmat, const float* cam_intrinsics, const float* img_h, int use_cam_feats,
                     int B, int state_off, int ld, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "head_init", 0.0, 4.0 * B * (ld - state_off));
    const HeadInit a{xc, init_pose, init_shape, init_cam, cam_rotmat, cam_intrinsics, img_h, use_cam_feats, state_off, ld};
    hipLaunchKernelGGL(head_init_kernel, dim3(B), dim3(256), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

// `state` = the 157 regressor outputs [pose6d | shape | cam] of image b at state[b * ld_state]; every output
// pointer addresses image 0 and is advanced by its own per-image stride (dense, or the row stride of a packed record)
__global__ void __launch_bounds__(256) head_final_kernel(const float* __restrict__ state, long ld_state,
                                                          float* __restrict__ pred_pose, float* __restrict__ pred_shape,
                                                          float* __restrict__ pred_cam, float* __restrict__ pred_pose_6d,
                                                          long ld_pose, long ld_shape, long ld_cam, long ld_p6d,
                                                          float* __restrict__ rot_ws, float* __restrict__ betas_ws,
                                                          float* __restrict__ cam_ws, int B) {
    const int b = blockIdx.x, t = threadIdx.x;
    const float* s = state + (size_t)b * ld_state;
    if (t < 144 && pred_pose_6d) pred_pose_6d[(size_t)b * ld_p6d + t] = s[t];
    if (t >= 144 && t < 154) {
        const float v = s[t];
        if (pred_shape) pred_shape[(size_t)b * ld_shape + t - 144] = v;
        if (betas_ws) betas_ws[(size_t)b * 10 + t - 144] = v;
    }
    if (t >= 154 && t < 157) {
        const float v = s[t];
        if (pred_cam) pred_cam[(size_t)b * ld_cam + t - 154] = v;
        if (cam_ws) cam_ws[(size_t)b * 3 + t - 154] = v;
    }
    if (t >= 192 && t < 216) {
        const int j = t - 192;
        float Rm[9];
        rot6d_joint(s + 6 * j, Rm);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (pred_pose) pred_pose[(size_t)b * ld_pose + j * 9 + k] = Rm[k];
            if (rot_ws) rot_ws[((size_t)b * 24 + j) * 9 + k] = Rm[k];
        }
    }
}

int launch_head_final(const float* state, long ld_state, float* pred_pose, float* pred_shape, float* pred_cam,
                      float* pred_pose_6d, const long ld[4], float* rotmat_ws, float* betas_ws, float* cam_ws, int B,
                      const LaunchCtx& ctx) {
    ProfScope ps(ctx, "head_final_rot6d", 0.0, 4.0 * B * (157 + 157 + 216));
    hipLaunchKernelGGL(head_final_kernel, dim3(B), dim3(256), 0, ctx.stream, state, ld_state, pred_pose, pred_shape,
                       pred_cam, pred_pose_6d, ld[0], ld[1], ld[2], ld[3], rotmat_ws, betas_ws, cam_ws, B);
    return (int)hipGetLastError();
}

// HMRHead with estimate_var (un-vendored pare; constructor flags at spec/models/hmr.py:35-38,57-64, consumer spec/losses.py:61-62):
// 'pred_pose_var' = cat([pred_pose_6d, var_pose]), 'pred_shape_var' = cat([pred_shape, var_shape]), the variances being the
// (optionally activated) extra decoder outputs of the LAST iteration
__device__ __forceinline__ float uncertainty_act(float x, int act) {
    switch (act) {
        case 1: return x < 0.f ? 0.f : x;                              // F.relu: a NaN stays a NaN (fmaxf(NaN, 0) is 0)
        case 2: return x > 20.f ? x : log1pf(expf(x));                 // F.softplus (beta 1, threshold 20)
        case 3: return 1.f / (1.f + expf(-x));                         // F.sigmoid
        case 4: return tanhf(x);                                       // F.tanh
        case 5: return x > 0.f ? x : expm1f(x);                        // F.elu (alpha 1)
        default: return x;
    }
}
__global__ void __launch_bounds__(320) head_var_kernel(const float* __restrict__ state, long ld_state, const float* __restrict__ var, long ld_var,
                                                       int act, float* __restrict__ pose_var, float* __restrict__ shape_var) {
    const int b = blockIdx.x, t = threadIdx.x;
    const float* s = state + (size_t)b * ld_state;
    const float* v = var + (size_t)b * ld_var;
    if (t < 144) pose_var[(size_t)b * 288 + t] = s[t];
    else if (t < 288) pose_var[(size_t)b * 288 + t] = uncertainty_act(v[t - 144], act);
    else if (t < 298) shape_var[(size_t)b * 20 + t - 288] = s[144 + t - 288];
    else if (t < 308) shape_var[(size_t)b * 20 + t - 288] = uncertainty_act(v[144 + t - 298], act);
}
int launch_head_var(const float* state, long ld_state, const float* var, long ld_var, int act, float* pose_var, float* shape_var,
                    int B, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "head_var", 0.0, 4.0 * B * (308 + 308));
    hipLaunchKernelGGL(head_var_kernel, dim3(B), dim3(320), 0, ctx.stream, state, ld_state, var, ld_var, act, pose_var, shape_var);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// R = batch_euler2matrix([pitch, 0, roll]) through the quaternion route and K with K[2,2] = 0
// (spec/utils/cam_params.py:37-46)
__device__ __forceinline__ void build_cam_RK(float pt, float rl, float f, float w, float h, float* R, float* K) {
    if (R) {
        const float hx = pt / 2.0f, hy = 0.0f / 2.0f, hz = rl / 2.0f;
        const float cz = cosf(hz), sz = sinf(hz), cy = cosf(hy), sy = sinf(hy), cx = cosf(hx), sx = sinf(hx);
        float qw = cx * cy * cz - sx * sy * sz;
        float qx = cx * sy * sz + cy * cz * sx;
        float qy = cx * cz * sy - sx * cy * sz;
        float qz = cx * cy * sz + sx * cz * sy;
        const float nq = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
        qw /= nq; qx /= nq; qy /= nq; qz /= nq;
        const float w2 = qw * qw, x2 = qx * qx, y2 = qy * qy, z2 = qz * qz;
        const float wx = qw * qx, wy = qw * qy, wz = qw * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
        R[0] = w2 + x2 - y2 - z2; R[1] = 2 * xy - 2 * wz;     R[2] = 2 * wy + 2 * xz;
        R[3] = 2 * wz + 2 * xy;     R[4] = w2 - x2 + y2 - z2; R[5] = 2 * yz - 2 * wx;
        R[6] = 2 * xz - 2 * wy;     R[7] = 2 * wx + 2 * yz;     R[8] = w2 - x2 - y2 + z2;
    }
    if (K) {
        K[0] = f;   K[1] = 0.f; K[2] = w / 2.0f;
        K[3] = 0.f; K[4] = f;   K[5] = h / 2.0f;
        K[6] = 0.f; K[7] = 0.f; K[8] = 0.f;   // K[2,2] stays 0 as in the reference
    }
}

// ---- FC layers at small batch (latency plan) -------------------------------------------------------------------------
// The three CamCalib heads (camcalib/model.py:77-79: fc_vfov / fc_pitch / fc_roll on the same pooled features) and the HMR
// regressor's composed map (spec/models/hmr.py:96) are M = batch-row GEMMs: on the matrix-core kernel each is a launch of 4-24
// tiles that are 1/64 ... 8/64 full plus a fold of K slices - 11-12 us per GEMM for 0.2 us of arithmetic, and three graph nodes
// where one will do.  Here: ONE launch for up to three heads (blockIdx.y), one WAVE per output column, lanes across K (16-byte
// loads of the row-major weight row: 1 KiB per instruction, coalesced), one or two images per wave, fixed lane-local k
// order and a fixed xor-shuffle tree - an image's result does not depend on the batch it travels in.
struct GemvHead { const float* x; const float* w; const float* bias; const float* res; float* out; };
struct GemvArgs {
    GemvHead hd[3];
    int nheads, N, Kp, ldx, ldo, B;   // w: (N, Kp) row-major, zero padded beyond the true K; x rows ldx apart (>= Kp floats readable)
};

// NB = images per wave (1 or 2; more images = more waves, blockIdx.z).  The kernel is pure latency - a wave's whole k range is
// 9 steps of (1 + NB) 16-byte loads - so GKU steps are requested before the first is used (8 images per wave at two steps in
// flight took 16 us at batch 8 for 1.4 MB of weights).
constexpr int GKU = 9;
template <int NB>
__global__ void __launch_bounds__(256) fc_gemv_kernel(const GemvArgs a) {
    const GemvHead& hd = a.hd[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    const int b0 = blockIdx.z * NB;
    if (n >= a.N) return;
    const int nb = min(NB, a.B - b0);
    const float* wrow = hd.w + (size_t)n * a.Kp;
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    // rows past the batch re-read the last image (results discarded) and k steps past the row re-read its last step with weight
    // 0 (acc + 0 * x = acc): no branch around a load, so all of them are independent and in flight together
    const float* xrow[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) xrow[b] = hd.x + (size_t)(b0 + (b < nb ? b : nb - 1)) * a.ldx;
    for (int k0 = lane * 4; k0 < a.Kp; k0 += 256 * GKU) {
        float4 wv[GKU], xv[GKU][NB];
#pragma unroll
        for (int u = 0; u < GKU; ++u) {
            const int k = min(k0 + u * 256, a.Kp - 4);
            wv[u] = *reinterpret_cast<const float4*>(wrow + k);
#pragma unroll
            for (int b = 0; b < NB; ++b) xv[u][b] = *reinterpret_cast<const float4*>(xrow[b] + k);
        }
#pragma unroll
        for (int u = 0; u < GKU; ++u) {
            // a step past the row re-read the last real quad: BOTH operands are zeroed there, so that it adds exactly +0 even when
            // that x quad holds Inf / NaN (0 * Inf = NaN would reach outputs the matrix-core path leaves finite)
            const bool in = k0 + u * 256 < a.Kp;
            const float wx = in ? wv[u].x : 0.f, wy = in ? wv[u].y : 0.f, wz = in ? wv[u].z : 0.f, ww = in ? wv[u].w : 0.f;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                acc[b] = fmaf(wx, in ? xv[u][b].x : 0.f, acc[b]);
                acc[b] = fmaf(wy, in ? xv[u][b].y : 0.f, acc[b]);
                acc[b] = fmaf(wz, in ? xv[u][b].z : 0.f, acc[b]);
                acc[b] = fmaf(ww, in ? xv[u][b].w : 0.f, acc[b]);
            }
        }
        // all loads of the body first, then the arithmetic (the scheduler otherwise puts each load next to its use: serial round trips)
        __builtin_amdgcn_sched_group_barrier(0x020, GKU * (1 + NB), 0);
        __builtin_amdgcn_sched_group_barrier(0x002, GKU * NB * 8, 0);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = wave_sum64(acc[b]);
    if (lane < nb) {
        float v = 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (lane == b) v = acc[b];
        const size_t o = (size_t)(b0 + lane) * a.ldo + n;
        v += hd.bias[n];
        if (hd.res) v += hd.res[o];
        hd.out[o] = v;
    }
}

int launch_fc_gemv(const FcGemv* heads, int nheads, int N, int Kp, int ldx, int ldo, int B, const LaunchCtx& ctx) {
    if (nheads < 1 || nheads > 3 || N < 1 || B < 1 || Kp % 4 != 0 || ldx % 4 != 0) return (int)hipErrorInvalidValue;
    GemvArgs a;
    a.nheads = nheads; a.N = N; a.Kp = Kp; a.ldx = ldx; a.ldo = ldo; a.B = B;
    for (int i = 0; i < 3; ++i) {
        const FcGemv& f = heads[i < nheads ? i : 0];
        if ((reinterpret_cast<uintptr_t>(f.x) | reinterpret_cast<uintptr_t>(f.w)) & 15) return (int)hipErrorInvalidValue;
        a.hd[i] = GemvHead{f.x, f.w, f.bias, f.res, f.out};
    }
    ProfScope ps(ctx, "fc_gemv_f32", 2.0 * nheads * (double)B * N * Kp, 4.0 * nheads * ((double)N * Kp + (double)B * (Kp + N)));
    // an image's sum is the same in every instantiation (lane-local k order, then the shuffle tree): NB only sets how many share a wave
    const dim3 blk(256);
    if (B == 1) hipLaunchKernelGGL(fc_gemv_kernel<1>, dim3((N + 3) / 4, nheads, 1), blk, 0, ctx.stream, a);
    else hipLaunchKernelGGL(fc_gemv_kernel<2>, dim3((N + 3) / 4, nheads, (B + 1) / 2), blk, 0, ctx.stream, a);
    return (int)hipGetLastError();
}

// soft_idx_to_angle of head 0 / 1 / 2 = vfov / pitch / roll (camcalib/cam_utils.py:94-107,128-133): (max - min) is a python double
// rounded to fp32 when it meets the tensor.  The product and the sum are rounded separately, as torch's two tensor operations are
// (the pragma: under the build's -ffp-contract=fast they became one fused multiply-add, up to 3 ulp away at angles near 0)
__device__ __forceinline__ float soft_idx_to_angle(float s, int head) {
#pragma clang fp contract(off)
    const float span = head == 0 ? (float)(2.1 - 0.2617) : (float)(0.6 - (-0.6));
    const float lo = head == 0 ? (float)0.2617 : (float)-0.6;
    const float p = span * ((s + 1.0f) / 2.0f);
    return p + lo;
}

// soft-argmax decode of image b: waves 0..2 = vfov / pitch / roll (a fourth wave idles), `ang` = 3 floats of LDS
struct DecodeArgs {
    const float *lv, *lp, *lr; int nbins; const float *img_h, *img_w;
    float *vfov, *pitch, *roll, *f_pix, *R, *K; long ld_ang;
};
__device__ __forceinline__ void camcalib_decode_image(const DecodeArgs& a, int b, float* ang) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 3) {
        const float* row = (wave == 0 ? a.lv : wave == 1 ? a.lp : a.lr) + (size_t)b * a.nbins;
        float mx = -INFINITY;
        for (int i = lane; i < a.nbins; i += 64) mx = fmaxf(mx, row[i]);
        mx = wave_max(mx);
        float se = 0.f, sp = 0.f;
        for (int i = lane; i < a.nbins; i += 64) {
            const float e = expf(row[i] - mx);
            se += e;
        }
        se = wave_sum64(se);
        for (int i = lane; i < a.nbins; i += 64) {
            const float pr = expf(row[i] - mx) / se;  // softmax, then expectation of the index
            sp += pr * (float)i;
        }
        sp = wave_sum64(sp);
        if (lane == 0) {
            const float s = sp / (float)(a.nbins - 1) * 2.0f - 1.0f;                  // softargmax1d normalisation
            ang[wave] = soft_idx_to_angle(s, wave);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float vf = ang[0], pt = ang[1], rl = ang[2];
        if (a.vfov) a.vfov[(size_t)b * a.ld_ang] = vf;
        if (a.pitch) a.pitch[(size_t)b * a.ld_ang] = pt;
        if (a.roll) a.roll[(size_t)b * a.ld_ang] = rl;
        const float h = a.img_h ? a.img_h[b] : 0.f, w = a.img_w ? a.img_w[b] : 0.f;
        const float f = h / 2.0f / tanf(vf / 2.0f);
        if (a.f_pix) a.f_pix[b] = f;
        build_cam_RK(pt, rl, f, w, h, a.R ? a.R + (size_t)b * 9 : nullptr, a.K ? a.K + (size_t)b * 9 : nullptr);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(192) camcalib_decode_kernel(const DecodeArgs a) {
    __shared__ float ang[3];
    camcalib_decode_image(a, blockIdx.x, ang);
}

int launch_camcalib_decode(const float* lv, const float* lp, const float* lr, int B, int nbins, const float* img_h,
                           const float* img_w, float* vfov, float* pitch, float* roll, float* f_pix, float* R,
                           float* K, long ld_ang, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "camcalib_decode", 0.0, 4.0 * B * (3.0 * nbins + 24));
    const DecodeArgs a{lv, lp, lr, nbins, img_h, img_w, vfov, pitch, roll, f_pix, R, K, ld_ang};
    hipLaunchKernelGGL(camcalib_decode_kernel, dim3(B), dim3(192), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

// The two per-row reductions of camcalib/cam_utils.py (camcalib_rows.h: wave_argmax_row, wave_softargmax_row), one wave per row
__global__ void __launch_bounds__(256) bins_reduce_kernel(const float* __restrict__ x, int rows, int nbins,
                                                           int* __restrict__ idx, float* __restrict__ soft) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* r = x + (size_t)row * nbins;
    float mx, se;
    const int mi = wave_argmax_row(r, nbins, lane, mx);
    if (idx && lane == 0) idx[row] = mi;
    if (soft) {
        const float sf = wave_softargmax_row(r, nbins, lane, mx, se);
        if (lane == 0) soft[row] = sf;
    }
}

int launch_bins_reduce(const float* x, int rows, int nbins, int* idx, float* soft, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "bins_reduce", 0.0, 4.0 * rows * (nbins + 2.0));
    hipLaunchKernelGGL(bins_reduce_kernel, dim3((rows + 3) / 4), dim3(256), 0, ctx.stream, x, rows, nbins, idx, soft);
    return (int)hipGetLastError();
}

// ---- CamCalib test step -------------------------------------------------------------------------------------------------
// camcalib/trainer.py:84-116 after the network: CameraRegressorLoss (camcalib/loss.py:24-125) + convert_preds_to_angles +
// |pred - gt|.  One wave per (image, head), the reductions of bins_reduce_kernel; per image and head:
//   loss_term : 'ce' / 'kl' (loss_type 0 / 1): -log_softmax(x)[t] = log(sum exp(x - max)) - (x[t] - max), max-subtracted so that
//               logits of 1e4 stay finite (F.kl_div against a one-hot target keeps exactly this term of every row);
//               'softargmax_l2' (2): (t - s)^2; 'softargmax_biased_l2' (3): vfov s > t ? l2 : l2 / (l2 + 1), pitch / roll plain l2
//   argmax, soft (s), angle = soft_idx_to_angle(s), err = |angle - gt| (radians).
// A per-image value depends on its own row only.
__global__ void __launch_bounds__(192) camcalib_eval_kernel(const CamEvalArgs a) {
    const int b = blockIdx.x, head = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* r = a.logits[head] + (size_t)b * a.nbins;
    float mx, se;
    const int mi = wave_argmax_row(r, a.nbins, lane, mx);
    const float s = wave_softargmax_row(r, a.nbins, lane, mx, se);
    if (lane != 0) return;
    const float term = camcalib_row_loss_term(r, a.nbins, a.loss_type, head, a.target[head], b, mx, se, s);
    const float ang = soft_idx_to_angle(s, head);
    const size_t o = (size_t)head * a.B + b;
    a.loss_term[o] = term;
    a.argmax[o] = mi;
    a.soft[o] = s;
    a.angle[o] = ang;
    a.err[o] = fabsf(ang - a.gt[head][b]);
}

// The batch means the reference logs, from the per-image arrays: waves 0..2 = mean loss term of a head times its weight
// (loss.py:109-114), waves 3..5 = mean |error| of a head in degrees (trainer.py:111-113), then loss = vfov + pitch + roll
// (loss.py:116).  A lane adds images lane, lane + 64, ... in ascending order and the wave folds the 64 partial sums in the
// xor-shuffle tree: the order is a function of B alone, so two runs give the same bits.
// means = [loss, vfov_loss, pitch_loss, roll_loss, vfov_acc, pitch_acc, roll_acc]
__global__ void __launch_bounds__(384) camcalib_eval_mean_kernel(const CamEvalArgs a) {
    __shared__ float head_loss[3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, head = wave % 3;
    const float* v = (wave < 3 ? a.loss_term : a.err) + (size_t)head * a.B;
    const float acc = wave_batch_mean(v, a.B, lane);
    if (lane == 0) {
        if (wave < 3) a.means[1 + head] = head_loss[head] = a.weight[head] * acc;
        else a.means[4 + head] = acc * (float)(180.0 / 3.14159265358979323846);     // Tensor.rad2deg
    }
    __syncthreads();
    if (threadIdx.x == 0) a.means[0] = head_loss[0] + head_loss[1] + head_loss[2];
}

int launch_camcalib_eval(const CamEvalArgs& a, const LaunchCtx& ctx) {
    {
        ProfScope ps(ctx, "camcalib_eval", 0.0, 4.0 * a.B * 3 * (a.nbins + 7.0));
        hipLaunchKernelGGL(camcalib_eval_kernel, dim3(a.B), dim3(192), 0, ctx.stream, a);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    if (!a.means) return 0;
    ProfScope ps(ctx, "camcalib_eval_mean", 0.0, 4.0 * (6.0 * a.B + 7));
    hipLaunchKernelGGL(camcalib_eval_mean_kernel, dim3(1), dim3(384), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

// read_cam_params (spec/utils/cam_params.py:24-50) for already-decoded angles: (pitch, roll, f_pix, w, h) -> R, K
__global__ void cam_params_kernel(const float* __restrict__ pitch, const float* __restrict__ roll,
                                  const float* __restrict__ f_pix, const float* __restrict__ img_w,
                                  const float* __restrict__ img_h, int B, float* __restrict__ R, float* __restrict__ K) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    build_cam_RK(pitch[b], roll[b], f_pix[b], img_w[b], img_h[b], R ? R + (size_t)b * 9 : nullptr,
                 K ? K + (size_t)b * 9 : nullptr);
}

int launch_cam_params(const float* pitch, const float* roll, const float* f_pix, const float* img_w, const float* img_h,
                      int B, float* R, float* K, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "cam_params", 0.0, 4.0 * B * 23);
    hipLaunchKernelGGL(cam_params_kernel, dim3((B + 63) / 64), dim3(64), 0, ctx.stream, pitch, roll, f_pix, img_w, img_h, B, R, K);
    return (int)hipGetLastError();
}

}  // namespace specmi
