// camcalib_bwd.hip - CameraRegressorLoss (camcalib/loss.py:24-125) as CamCalib's training step needs it: the loss alone
// (specmi_camcalib_loss) and its gradient with respect to the three logit tensors (specmi_camcalib_loss_backward), gfx950.
//
// The forward is the loss part of specmi_camcalib_eval (head.hip) without decode and angle errors: the same per-row functions
// (camcalib_rows.h), the same two launches, so loss_term and means[0:4] carry the same bits.
//
// The backward is one launch, one wave per (image, head) row, no atomics, no value shared between rows.  With p = softmax(x),
// E = sum_i i p_i, s = 2 E / (n - 1) - 1 and c = w_head (g_means[0] + g_means[1 + head]) / B  (loss = the sum of the three head
// losses, a head loss = weight x batch mean):
//     'ce' / 'kl'             g_i = c (p_i - [i == t])
//     'softargmax_l2'         g_i = c (-2 (t - s)) (2 / (n - 1)) p_i (i - E)
//     'softargmax_biased_l2'  the vfov head divides -2 (t - s) by (l2 + 1)^2 wherever s > t is false, l2 = (t - s)^2
// i - E is formed relative to the arg-max bin m: i - E = (i - m) - E', E' = sum_i p_i (i - m).  On a nearly one-hot row E sits next
// to the integer m and the difference i - E would lose its leading digits; E' is a sum of small terms (the bin m adds an exact 0).
#include "camcalib_rows.h"

namespace specmi {

namespace {

__global__ void __launch_bounds__(192) camcalib_loss_kernel(const CamLossArgs a) {
    const int b = blockIdx.x, head = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* r = a.logits[head] + (size_t)b * a.nbins;
    float mx, se;
    wave_argmax_row(r, a.nbins, lane, mx);
    const float s = wave_softargmax_row(r, a.nbins, lane, mx, se);
    if (lane != 0) return;
    a.loss_term[(size_t)head * a.B + b] = camcalib_row_loss_term(r, a.nbins, a.loss_type, head, a.target[head], b, mx, se, s);
}

// means = [loss, vfov_loss, pitch_loss, roll_loss]: waves 0..2 of camcalib_eval_mean_kernel
__global__ void __launch_bounds__(192) camcalib_loss_mean_kernel(const CamLossArgs a) {
    __shared__ float head_loss[3];
    const int head = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float acc = wave_batch_mean(a.loss_term + (size_t)head * a.B, a.B, lane);
    if (lane == 0) a.means[1 + head] = head_loss[head] = a.weight[head] * acc;
    __syncthreads();
    if (threadIdx.x == 0) a.means[0] = head_loss[0] + head_loss[1] + head_loss[2];
}

__global__ void __launch_bounds__(256) camcalib_loss_bwd_kernel(const CamLossArgs a, const float* __restrict__ g_means,
                                                                 float* __restrict__ g0, float* __restrict__ g1, float* __restrict__ g2) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= 3L * a.B) return;
    const int b = (int)(row / 3), head = (int)(row - 3L * b);
    const int n = a.nbins;
    const float* r = a.logits[head] + (size_t)b * n;
    float* const g = (head == 0 ? g0 : head == 1 ? g1 : g2) + (size_t)b * n;
    float mx, se;
    const int m = wave_argmax_row(r, n, lane, mx);
    const float c = a.weight[head] * (g_means[0] + g_means[1 + head]) / (float)a.B;
    if (a.loss_type <= 1) {
        const int t = camcalib_target_bin(a.target[head], b, n);
        // p_t - 1 = -(the other bins' share): on a row that is nearly one-hot at t the subtraction would cancel
        float so = 0.f;
        se = 0.f;
        for (int i = lane; i < n; i += 64) {
            const float ex = expf(r[i] - mx);
            se += ex;
            so += i == t ? 0.f : ex;
        }
        se = wave_sum64(se);
        so = wave_sum64(so);
        for (int i = lane; i < n; i += 64) g[i] = c * (i == t ? -(so / se) : expf(r[i] - mx) / se);
        return;
    }
    const float s = wave_softargmax_row(r, n, lane, mx, se);      // the forward's s: the same side of t, the same t - s
    const float t = static_cast<const float*>(a.target[head])[b];
    const float d = t - s, l2 = d * d;
    float k = -2.f * d;
    if (a.loss_type == 3 && head == 0 && !(s > t)) k /= (l2 + 1.0f) * (l2 + 1.0f);
    k = c * k * (2.f / (float)(n - 1));
    float e = 0.f;
    for (int i = lane; i < n; i += 64) e += expf(r[i] - mx) / se * (float)(i - m);
    e = wave_sum64(e);
    for (int i = lane; i < n; i += 64) g[i] = k * (expf(r[i] - mx) / se * ((float)(i - m) - e));
}

}  // namespace

int launch_camcalib_loss(const CamLossArgs& a, const LaunchCtx& ctx) {
    {
        ProfScope ps(ctx, "camcalib_loss", 0.0, 4.0 * a.B * 3 * (a.nbins + 2.0));
        hipLaunchKernelGGL(camcalib_loss_kernel, dim3(a.B), dim3(192), 0, ctx.stream, a);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    ProfScope ps(ctx, "camcalib_loss_mean", 0.0, 4.0 * (3.0 * a.B + 4));
    hipLaunchKernelGGL(camcalib_loss_mean_kernel, dim3(1), dim3(192), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

int launch_camcalib_loss_backward(const CamLossArgs& a, const float* g_means, float* const g_logits[3], const LaunchCtx& ctx) {
    const long rows = 3L * a.B;
    ProfScope ps(ctx, "camcalib_loss_bwd", 0.0, 4.0 * rows * (2.0 * a.nbins + 2.0));
    hipLaunchKernelGGL(camcalib_loss_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ctx.stream, a, g_means, g_logits[0],
                       g_logits[1], g_logits[2]);
    return (int)hipGetLastError();
}

}  // namespace specmi
