// loss.hip - SPEC's two loss modules on the device: the forward value (include/specmi.h: specmi_hmr_loss) and, at the end of the
// file, its gradient with respect to the prediction (specmi_hmr_loss_backward: hmr_loss_bwd_kernel, one launch).
//
// Replaces spec/losses.py of the reference: HMRLoss.forward (:59-141, mode 0) and HMRCamLoss.forward (:171-271, mode 1) with the
// helpers they call - projected_keypoint_loss (:274-296), keypoint_3d_loss (:326-348), shape_loss (:375-387), smpl_losses
// (:412-432) - and pare's batch_rodrigues in SPIN's form (angle = |theta + 1e-8|, axis = theta / angle, the unit quaternion
// (cos(angle / 2), sin(angle / 2) axis) normalised once more, quaternion -> matrix; NOT the smplx Rodrigues of smpl.hip).
//
// Two launches, no atomics:
//   hmr_loss_image_kernel  one workgroup of 256 lanes per image -> the image's six unnormalised sums, terms (6, B):
//       row 0  sum over 49 x 2 of conf * (pred - gt)^2 of the projected keypoints (mode 1: normalised and rescaled, below)
//       row 1  sum over 24 x 3 of conf * (pred - gt)^2 of the pelvis-centred 3D joints
//       row 2  sum over 24 x 9 of (pred_pose - rodrigues(pose))^2        } the pose term is the PRODUCT of two batch means
//       row 3  sum over 24 of pose_conf                                  } (:427), so it needs two rows
//       row 4  sum over 10 of (pred_shape - betas)^2
//       row 5  sum over V x 3 of |vertices - gt_vertices|  (0 without gt_vertices)
//     every row is computed for every image, whatever its masks say; loss_cam needs no reduction and has no row.
//     The vertex sum walks the image's V * 3 floats in chunks of four CONSECUTIVE ELEMENTS counted from the image's own first
//     float: chunk k belongs to lane k % 256, a lane adds its chunks in ascending order, and the V * 3 % 4 floats left over go to
//     lanes 0 .. 2.  A chunk is one 16-byte load from a 4-byte aligned address (image b starts b * V * 3 floats into the
//     tensor, which is 16-byte aligned only when V * 3 % 4 == 0); cutting the chunks by element index rather than by address is
//     what makes the sum of an image the same bits at every batch position.  Lanes fold through the xor-shuffle tree, the four
//     waves through LDS in the order 0 + 1 + 2 + 3.
//   hmr_loss_fold_kernel   one workgroup of seven waves, wave r folds row r: lane l adds images l, l + 64, ... in ascending order (masked rows
//       count as +0), then the shuffle tree - an order that depends on B alone.  Wave 6 folds loss_cam, waves 1 and 2 count Np
//       and Nv.  Lane 0 then forms the means, the weights and the total as the reference does.
#include "specmi_internal.h"

namespace specmi {

namespace {

struct __attribute__((packed, aligned(4))) F4 { float x, y, z, w; };   // 16 bytes from a 4-byte aligned address: one global_load_dwordx4

// element e (0 .. 8, row-major) of pare's batch_rodrigues(theta) - SPIN's form, fp32 like the reference
__device__ __forceinline__ float spin_rodrigues_element(float tx, float ty, float tz, int e) {
    const float ex = tx + 1e-8f, ey = ty + 1e-8f, ez = tz + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float nx = tx / angle, ny = ty / angle, nz = tz / angle;
    const float half = angle * 0.5f, c = cosf(half), s = sinf(half);
    float w = c, x = s * nx, y = s * ny, z = s * nz;
    const float qn = sqrtf(w * w + x * x + y * y + z * z);
    w /= qn; x /= qn; y /= qn; z /= qn;
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    switch (e) {
        case 0: return w2 + x2 - y2 - z2;
        case 1: return 2.f * xy - 2.f * wz;
        case 2: return 2.f * wy + 2.f * xz;
        case 3: return 2.f * wz + 2.f * xy;
        case 4: return w2 - x2 + y2 - z2;
        case 5: return 2.f * yz - 2.f * wx;
        case 6: return 2.f * xz - 2.f * wy;
        case 7: return 2.f * wx + 2.f * yz;
        default: return w2 - x2 - y2 + z2;
    }
}

constexpr int kRows = 6;

__global__ void __launch_bounds__(256) hmr_loss_image_kernel(const HmrLossArgs a) {
    __shared__ float part[4 * kRows];
    const int b = blockIdx.x, t = threadIdx.x;
    float acc[kRows] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    if (t < 49) {   // row 0: projected_keypoint_loss (:274-296); HMRCamLoss first normalises both sides (:188-195) and rescales (:222-223)
        const float* kp = a.keypoints + ((size_t)b * 49 + t) * 3;
        const float* pj = a.joints2d + ((size_t)b * 49 + t) * 2;
        const float conf = kp[2] * (t < 25 ? a.w_openpose : a.w_gt);
        float e[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (a.mode == 1) {
                const float size = a.orig_shape[(size_t)b * 2 + (1 - c)];     // (H, W) -> x over W, y over H
                const float pn = 2.f * (pj[c] / size) - 1.f, gn = 2.f * (kp[c] / size) - 1.f, d = pn - gn;
                e[c] = (conf * (d * d)) * (size / (a.scale[b] * 200.f));
            } else {
                const float d = pj[c] - kp[c];
                e[c] = conf * (d * d);
            }
        }
        acc[0] = e[0] + e[1];
    }
    if (t < 24) {   // row 1: keypoint_3d_loss (:326-348), pelvis = mean of joints 2 and 3 on each side; row 3: pose_conf
        const float* g = a.pose_3d + (size_t)b * 24 * 4;
        const float* p = a.joints3d + ((size_t)b * 49 + 25) * 3;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gp = (g[2 * 4 + c] + g[3 * 4 + c]) / 2.f, pp = (p[2 * 3 + c] + p[3 * 3 + c]) / 2.f;
            const float d = (p[t * 3 + c] - pp) - (g[t * 4 + c] - gp);
            s += g[t * 4 + 3] * (d * d);
        }
        acc[1] = s;
        acc[3] = a.pose_conf[(size_t)b * 24 + t];
    }
    if (t < 216) {  // row 2: smpl_losses (:412-432), one matrix element per lane
        const int j = t / 9;
        const float* th = a.pose + (size_t)b * 72 + j * 3;
        const float d = a.pred_pose[(size_t)b * 216 + t] - spin_rodrigues_element(th[0], th[1], th[2], t - j * 9);
        acc[2] = d * d;
    }
    if (t < 10) {   // row 4
        const float d = a.pred_shape[(size_t)b * 10 + t] - a.betas[(size_t)b * 10 + t];
        acc[4] = d * d;
    }
    if (a.gt_vertices) {   // row 5: shape_loss (:375-387)
        const int n = a.V * 3, nchunk = n >> 2;
        const float* pv = a.vertices + (size_t)b * n;
        const float* gv = a.gt_vertices + (size_t)b * n;
        const F4* p4 = reinterpret_cast<const F4*>(pv);
        const F4* g4 = reinterpret_cast<const F4*>(gv);
        float s = 0.f;
#pragma unroll 4
        for (int k = t; k < nchunk; k += 256) {
            const F4 p = p4[k], g = g4[k];
            s += (fabsf(p.x - g.x) + fabsf(p.y - g.y)) + (fabsf(p.z - g.z) + fabsf(p.w - g.w));
        }
        const int tail = (nchunk << 2) + t;
        if (t < 3 && tail < n) s += fabsf(pv[tail] - gv[tail]);
        acc[5] = s;
    }

#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = wave_sum64(acc[r]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) part[(t >> 6) * kRows + r] = acc[r];
    }
    __syncthreads();
    if (t < kRows) a.terms[(size_t)t * a.B + b] = ((part[t] + part[kRows + t]) + part[2 * kRows + t]) + part[3 * kRows + t];
}

// means = [loss_keypoints, loss_keypoints_3d, loss_regr_pose, loss_regr_betas, loss_shape, loss_cam, total_loss] (the reference's
// loss_dict order, weights applied as :114-118, total = loss_weight * sum of the six), counts = [Nv, Np]
__global__ void __launch_bounds__(448) hmr_loss_fold_kernel(const HmrLossArgs a) {
    __shared__ float sum[7];
    __shared__ int cnt[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    {
        // rows 2 .. 5 keep the images with has_smpl, row 1 those with has_pose_3d (the reference tests `== 1` on .bool())
        const int* mask = wave == 1 ? a.has_pose_3d : (wave >= 2 && wave <= 5) ? a.has_smpl : nullptr;
        float acc = 0.f;
        int n = 0;
        for (int i = lane; i < a.B; i += 64) {
            const bool keep = !mask || mask[i] != 0;
            float v;
            if (wave < 6) v = a.terms[(size_t)wave * a.B + i];
            else { const float e = expf(-a.pred_cam[(size_t)i * 3] * 10.f); v = e * e; }     // loss_cam (:119)
            acc += keep ? v : 0.f;
            n += keep ? 1 : 0;
        }
        acc = wave_sum64(acc);
        n = wave_sum64(n);
        if (lane == 0) {
            sum[wave] = acc;
            if (wave == 1) cnt[1] = n;
            if (wave == 2) cnt[0] = n;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int Nv = cnt[0], Np = cnt[1];
    if (a.counts) { a.counts[0] = Nv; a.counts[1] = Np; }
    if (!a.means) return;
    const float fB = (float)a.B, fNv = (float)Nv, fNp = (float)Np;
    const float kp = a.w_keypoint * (sum[0] / (fB * 98.f));
    const float kp3 = a.w_keypoint * (Np > 0 ? sum[1] / (fNp * 72.f) : 0.f);
    const float pose = a.w_pose * (Nv > 0 ? (sum[3] / (fNv * 24.f)) * (sum[2] / (fNv * 216.f)) : 0.f);
    const float betas = a.w_beta * (Nv > 0 ? sum[4] / (fNv * 10.f) : 0.f);
    const float shape = a.w_shape * ((Nv > 0 && a.gt_vertices) ? sum[5] / (float)((double)Nv * a.V * 3.0) : 0.f);
    const float cam = sum[6] / fB;
    a.means[0] = kp; a.means[1] = kp3; a.means[2] = pose; a.means[3] = betas; a.means[4] = shape; a.means[5] = cam;
    a.means[6] = (((((kp + kp3) + pose) + betas) + shape) + cam) * a.w_loss;
}

// The gradient of the seven means with respect to the six prediction tensors, one launch, elementwise outputs (no reduction
// across images other than the three batch scalars every workgroup folds for itself out of `terms`, in hmr_loss_fold_kernel's
// order).  coef[k] = g_means[k] + w_loss * g_means[6]: total_loss = w_loss * sum of the six.  What autograd does to the
// reference: a masked-out image gets +0, an empty mask zeros, |x| at 0 has slope 0, the ground truth is a constant.
__global__ void __launch_bounds__(256) hmr_loss_bwd_kernel(const HmrLossArgs a, const HmrLossGrads g) {
    __shared__ float s_conf;      // sum of pose_conf over the images with has_smpl (row 3 of terms)
    __shared__ float s_pel[3];    // sum over the 24 joints of 2 conf d: what the pelvis (joints 2 and 3) takes back
    const int b = blockIdx.x, t = threadIdx.x;
    const int Nv = a.counts[0], Np = a.counts[1];
    const bool hs = a.has_smpl[b] != 0, hp = a.has_pose_3d[b] != 0;
    float coef[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) coef[k] = g.g_means[k] + a.w_loss * g.g_means[6];
    if (t < 64) {
        float acc = 0.f;
        for (int i = t; i < a.B; i += 64) acc += a.has_smpl[i] != 0 ? a.terms[(size_t)3 * a.B + i] : 0.f;
        acc = wave_sum64(acc);
        if (t == 0) s_conf = acc;
    } else if (t < 128) {
        // keypoint_3d_loss: d_j = (p_j - pelvis_p) - (g_j - pelvis_g), pelvis = (joint 2 + joint 3) / 2
        const int j = t - 64;
        const float* gg = a.pose_3d + (size_t)b * 24 * 4;
        const float* p = a.joints3d + ((size_t)b * 49 + 25) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = 0.f;
            if (j < 24) {
                const float gp = (gg[2 * 4 + c] + gg[3 * 4 + c]) / 2.f, pp = (p[2 * 3 + c] + p[3 * 3 + c]) / 2.f;
                v = 2.f * gg[j * 4 + 3] * ((p[j * 3 + c] - pp) - (gg[j * 4 + c] - gp));
            }
            v = wave_sum64(v);
            if (j == 0) s_pel[c] = v;
        }
    }
    __syncthreads();
    const float fB = (float)a.B, fNv = (float)Nv, fNp = (float)Np;

    if (g.g_joints2d && t < 49) {
        const float* kp = a.keypoints + ((size_t)b * 49 + t) * 3;
        const float* pj = a.joints2d + ((size_t)b * 49 + t) * 2;
        const float conf = kp[2] * (t < 25 ? a.w_openpose : a.w_gt);
        const float k0 = coef[0] * a.w_keypoint / (fB * 98.f);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float v;
            if (a.mode == 1) {   // e = conf d^2 (size / (scale 200)), d = 2 pj / size - 1 - (2 kp / size - 1)
                const float size = a.orig_shape[(size_t)b * 2 + (1 - c)];
                const float d = (2.f * (pj[c] / size) - 1.f) - (2.f * (kp[c] / size) - 1.f);
                v = k0 * (size / (a.scale[b] * 200.f)) * (conf * (2.f * d)) * (2.f / size);
            } else {
                v = k0 * (conf * (2.f * (pj[c] - kp[c])));
            }
            g.g_joints2d[((size_t)b * 49 + t) * 2 + c] = v;
        }
    }
    if (g.g_joints3d && t < 147) {
        const int jt = t / 3, c = t - jt * 3, j = jt - 25;
        float v = 0.f;
        if (j >= 0 && hp && Np > 0) {
            const float* gg = a.pose_3d + (size_t)b * 24 * 4;
            const float* p = a.joints3d + ((size_t)b * 49 + 25) * 3;
            const float gp = (gg[2 * 4 + c] + gg[3 * 4 + c]) / 2.f, pp = (p[2 * 3 + c] + p[3 * 3 + c]) / 2.f;
            float e = 2.f * gg[j * 4 + 3] * ((p[j * 3 + c] - pp) - (gg[j * 4 + c] - gp));
            if (j == 2 || j == 3) e -= 0.5f * s_pel[c];
            v = coef[1] * a.w_keypoint / (fNp * 72.f) * e;
        }
        g.g_joints3d[(size_t)b * 147 + t] = v;
    }
    if (g.g_pred_pose && t < 216) {
        float v = 0.f;
        if (hs && Nv > 0) {
            const int j = t / 9;
            const float* th = a.pose + (size_t)b * 72 + j * 3;
            const float d = a.pred_pose[(size_t)b * 216 + t] - spin_rodrigues_element(th[0], th[1], th[2], t - j * 9);
            v = coef[2] * a.w_pose * (s_conf / (fNv * 24.f)) * (2.f * d) / (fNv * 216.f);
        }
        g.g_pred_pose[(size_t)b * 216 + t] = v;
    }
    if (g.g_pred_shape && t < 10) {
        float v = 0.f;
        if (hs && Nv > 0) v = coef[3] * a.w_beta * (2.f * (a.pred_shape[(size_t)b * 10 + t] - a.betas[(size_t)b * 10 + t])) / (fNv * 10.f);
        g.g_pred_shape[(size_t)b * 10 + t] = v;
    }
    if (g.g_pred_cam && t < 3) {
        float v = 0.f;
        if (t == 0) { const float e = expf(-a.pred_cam[(size_t)b * 3] * 10.f); v = coef[5] * (-20.f * (e * e)) / fB; }
        g.g_pred_cam[(size_t)b * 3 + t] = v;
    }
    if (g.g_vertices) {   // 16-byte chunks counted from the image's first float, as the forward reads them
        const int n = a.V * 3, nchunk = n >> 2;
        float* const ov = g.g_vertices + (size_t)b * n;
        F4* const o4 = reinterpret_cast<F4*>(ov);
        const bool on = hs && Nv > 0 && a.gt_vertices;
        const float k4 = on ? coef[4] * a.w_shape / (float)((double)Nv * a.V * 3.0) : 0.f;
        if (!on) {
            const F4 z = {0.f, 0.f, 0.f, 0.f};
            for (int k = t; k < nchunk; k += 256) o4[k] = z;
            const int tail = (nchunk << 2) + t;
            if (t < 3 && tail < n) ov[tail] = 0.f;
            return;
        }
        const float* pv = a.vertices + (size_t)b * n;
        const float* gv = a.gt_vertices + (size_t)b * n;
        const F4* p4 = reinterpret_cast<const F4*>(pv);
        const F4* g4 = reinterpret_cast<const F4*>(gv);
        auto slope = [k4](float d) { return d > 0.f ? k4 : d < 0.f ? -k4 : 0.f; };
#pragma unroll 4
        for (int k = t; k < nchunk; k += 256) {
            const F4 p = p4[k], q = g4[k];
            const F4 o = {slope(p.x - q.x), slope(p.y - q.y), slope(p.z - q.z), slope(p.w - q.w)};
            o4[k] = o;
        }
        const int tail = (nchunk << 2) + t;
        if (t < 3 && tail < n) ov[tail] = slope(pv[tail] - gv[tail]);
    }
}

}  // namespace

int launch_hmr_loss_backward(const HmrLossArgs& a, const HmrLossGrads& g, const LaunchCtx& ctx) {
    const double per_image = 216 * 2 + 10 * 2 + 3 * 2 + 49 * 5 + 49 * 5 + 72 + 24 * 4 + (g.g_vertices ? (a.gt_vertices ? 9.0 : 3.0) * a.V : 0.0);
    ProfScope ps(ctx, "hmr_loss_bwd", 0.0, 4.0 * a.B * (per_image + a.B));
    hipLaunchKernelGGL(hmr_loss_bwd_kernel, dim3(a.B), dim3(256), 0, ctx.stream, a, g);
    return (int)hipGetLastError();
}

int launch_hmr_loss(const HmrLossArgs& a, const LaunchCtx& ctx) {
    {
        const double per_image = 216 + 10 + 49 * 3 + 49 * 2 + 72 + 10 + 24 + 24 * 4 + 49 * 3 + kRows + (a.gt_vertices ? 6.0 * a.V : 0.0);
        ProfScope ps(ctx, "hmr_loss_image", 0.0, 4.0 * a.B * per_image);
        hipLaunchKernelGGL(hmr_loss_image_kernel, dim3(a.B), dim3(256), 0, ctx.stream, a);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    if (!a.means && !a.counts) return 0;
    ProfScope ps(ctx, "hmr_loss_fold", 0.0, 4.0 * (a.B * (kRows + 3.0) + 9));
    hipLaunchKernelGGL(hmr_loss_fold_kernel, dim3(1), dim3(448), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

}  // namespace specmi
