// camcalib_rows.h - the per-row arithmetic of CamCalib's logit tensors, stated once for head.hip (decode, bins, the test step) and
// camcalib_bwd.hip (the training loss and its gradient): one wave per (rows, nbins) row.
#pragma once
#include "specmi_internal.h"

namespace specmi {

// The two per-row reductions camcalib/cam_utils.py applies to a (rows, nbins) logit tensor, one wave per row:
//   idx[row]  = np.argmax(row)            (bins2vfov / bins2pitch / bins2roll / bins2horizon, cam_utils.py:66-91):
//               FIRST index of the maximum, a NaN counts as the maximum (NumPy semantics) - index work, bit-exact;
//   soft[row] = softargmax1d(row, normalize_keypoints=True) in [-1, 1] (get_softargmax, cam_utils.py:110-118).
// np.argmax of a row by one wave -> index (every lane); mx = the largest non-NaN value (-inf for an all-NaN row)
__device__ __forceinline__ int wave_argmax_row(const float* __restrict__ r, int nbins, int lane, float& mx) {
    mx = -INFINITY;
    int mi = 0x7fffffff, nan_i = 0x7fffffff;
    for (int i = lane; i < nbins; i += 64) {
        const float v = r[i];
        if (v != v) nan_i = min(nan_i, i);
        if (v > mx || (v == mx && i < mi)) { mx = v; mi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float omx = __shfl_xor(mx, o, 64);
        const int omi = __shfl_xor(mi, o, 64);
        nan_i = min(nan_i, __shfl_xor(nan_i, o, 64));
        if (omx > mx || (omx == mx && omi < mi)) { mx = omx; mi = omi; }
    }
    return nan_i != 0x7fffffff ? nan_i : (mi == 0x7fffffff ? 0 : mi);
}
// softargmax1d(normalize_keypoints=True) of a row by one wave, given its maximum -> [-1, 1] (every lane); se = sum exp(x - mx)
__device__ __forceinline__ float wave_softargmax_row(const float* __restrict__ r, int nbins, int lane, float mx, float& se) {
    float sp = 0.f;
    se = 0.f;
    for (int i = lane; i < nbins; i += 64) se += expf(r[i] - mx);
    se = wave_sum64(se);
    for (int i = lane; i < nbins; i += 64) sp += expf(r[i] - mx) / se * (float)i;
    sp = wave_sum64(sp);
    return sp / (float)(nbins - 1) * 2.0f - 1.0f;
}

// The bin index a 'ce' / 'kl' target names, clamped into the row
__device__ __forceinline__ int camcalib_target_bin(const void* target, int b, int nbins) {
    return min(max(static_cast<const int*>(target)[b], 0), nbins - 1);
}

// CameraRegressorLoss's unweighted term of one row (camcalib/loss.py:24-125), from the row's reductions mx, se and s (every lane):
//   'ce' / 'kl' (loss_type 0 / 1): -log_softmax(x)[t] = log(sum exp(x - max)) - (x[t] - max), max-subtracted so that logits of 1e4
//       stay finite (F.kl_div against a one-hot target keeps exactly this term of every row);
//   'softargmax_l2' (2): (t - s)^2; 'softargmax_biased_l2' (3): vfov s > t ? l2 : l2 / (l2 + 1), pitch / roll plain l2
__device__ __forceinline__ float camcalib_row_loss_term(const float* __restrict__ r, int nbins, int loss_type, int head, const void* target,
                                                        int b, float mx, float se, float s) {
    if (loss_type <= 1) return logf(se) - (r[camcalib_target_bin(target, b, nbins)] - mx);
    const float t = static_cast<const float*>(target)[b];
    const float d = t - s, l2 = d * d;
    return (loss_type == 3 && head == 0 && !(s > t)) ? l2 / (l2 + 1.0f) : l2;
}

// The batch mean of one (B) array by one wave (every lane): a lane adds images lane, lane + 64, ... in ascending order and the
// wave folds the 64 partial sums in the xor-shuffle tree - an order that depends on B alone
__device__ __forceinline__ float wave_batch_mean(const float* __restrict__ v, int B, int lane) {
    float acc = 0.f;
    for (int i = lane; i < B; i += 64) acc += v[i];
    return wave_sum64(acc) / (float)B;
}

}  // namespace specmi
