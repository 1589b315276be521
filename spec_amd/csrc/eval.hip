// eval.hip - evaluation metrics on the device, directly on the path's outputs.
//
// Replaces the host NumPy scoring that follows the hot path in the reference:
//   * eval_single  (spec/utils/compute_error.py:52-86; validation step spec/trainer.py:272-316):
//     joints = J_regressor @ vertices, pelvis alignment, joint selection (H36M_TO_J14), MPJPE,
//     PA-MPJPE (similarity Procrustes), pelvis-aligned V2V - all in millimetres.
//   * eval_j_24    (spec/utils/compute_error.py:33-49): pelvis-aligned MPJPE / PA-MPJPE of two
//     joint sets; with joints = J_regressor(24xV) @ vertices this is the README's W-MPJPE.
// The reference copies 21 MB of vertices per batch to the host for this; here the vertices never
// leave HBM and only 3 floats per image come back.
//
// One workgroup per image: joint regression walks the vertices ONCE per chunk of joints (every lane keeps a vertex
// pair in registers and accumulates kJC joints x 6 coordinates; all loads of the loop are independent, so they pipeline;
// one wave-shuffle + LDS reduction per chunk), then one lane solves the Procrustes problem with Horn's quaternion
// method (largest eigenpair of a symmetric 4x4 via cyclic Jacobi in fp64) - the same optimum as the SVD/Kabsch
// solution with its det(R)=+1 fix.
#include "specmi_internal.h"

namespace specmi {

__device__ __forceinline__ float block_sum_256(float v, float* red) {   // blockDim.x == 256
    v = wave_sum64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// Sum N per-lane values over a 256-thread block: wave shuffles, then one LDS exchange.  Result i lands in dst[i]
// (LDS, valid after the call's trailing barrier).  part = LDS scratch of 4 * N floats.
template <int N>
__device__ __forceinline__ void block_sum_many_256(float (&a)[N], float* part, float* dst) {
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = wave_sum64(a[i]);
    __syncthreads();   // part may still be read from the previous call
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[(threadIdx.x >> 6) * N + i] = a[i];
    }
    __syncthreads();
    if (threadIdx.x < N) dst[threadIdx.x] = part[threadIdx.x] + part[N + threadIdx.x] + part[2 * N + threadIdx.x] + part[3 * N + threadIdx.x];
    __syncthreads();
}

// Largest eigenvalue / eigenvector of a symmetric 4x4 (cyclic Jacobi, fp64).
// All matrix indices are compile-time constants after unrolling, so A and V live in registers (no scratch).
__device__ void sym4_max_eig(double A[4][4], double q[4], double* lam) {
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 24; ++sweep) {
        double off = 0, diag = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            diag += A[i][i] * A[i][i];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
        }
        if (off <= 1e-30 * (diag + 1e-300)) break;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                // tan of the rotation angle: t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_rr - a_pp) / (2 a_pr),
                // written without the division that forms theta: one sqrt, one division, one rsqrt per rotation; an
                // already-zero a_pr gives t = 0 (identity rotation) through the guarded denominator
                const double apr2 = 2.0 * A[p][r], diff = A[r][r] - A[p][p];
                const double den = fabs(diff) + sqrt(diff * diff + apr2 * apr2);
                const double t = fabs(A[p][r]) < 1e-300 ? 0.0 : (diff >= 0 ? apr2 : -apr2) / den;
                const double c = rsqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akr = A[k][r];
                    A[k][p] = c * akp - s * akr;
                    A[k][r] = s * akp + c * akr;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], ark = A[r][k];
                    A[p][k] = c * apk - s * ark;
                    A[r][k] = s * apk + c * ark;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkr = V[k][r];
                    V[k][p] = c * vkp - s * vkr;
                    V[k][r] = s * vkp + c * vkr;
                }
            }
        }
    }
    double best = A[0][0];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = V[k][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > best) {
            best = A[i][i];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = V[k][i];
        }
    *lam = best;
}

// MPJPE and PA-MPJPE (mm) of N pelvis-aligned joints p, g: coordinate c of joint i at p[(i * 3 + c) * ST].
template <int ST>
__device__ void joint_errors(const float* p, const float* g, int N, float* mpjpe, float* pampjpe) {
    double e = 0, mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
    for (int i = 0; i < N; ++i) {
        double d = 0;
        for (int c = 0; c < 3; ++c) {
            const double df = (double)p[(i * 3 + c) * ST] - (double)g[(i * 3 + c) * ST];
            d += df * df;
            mu1[c] += p[(i * 3 + c) * ST];
            mu2[c] += g[(i * 3 + c) * ST];
        }
        e += sqrt(d);
    }
    *mpjpe = (float)(e / N * 1000.0);
    for (int c = 0; c < 3; ++c) { mu1[c] /= N; mu2[c] /= N; }
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0;
    for (int i = 0; i < N; ++i) {
        double x1[3], x2[3];
        for (int c = 0; c < 3; ++c) { x1[c] = p[(i * 3 + c) * ST] - mu1[c]; x2[c] = g[(i * 3 + c) * ST] - mu2[c]; var1 += x1[c] * x1[c]; }
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) S[a][b] += x1[a] * x2[b];
    }
    double Nm[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
        {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
        {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
        {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double q[4], lam;
    sym4_max_eig(Nm, q, &lam);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[3][3] = {{w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z}};
    const double scale = lam / var1;
    double pe = 0;
    for (int i = 0; i < N; ++i) {
        double d = 0;
        for (int a = 0; a < 3; ++a) {
            double v = 0;
            for (int b = 0; b < 3; ++b) v += R[a][b] * (p[(i * 3 + b) * ST] - mu1[b]);
            const double df = scale * v + mu2[a] - g[(i * 3 + a) * ST];
            d += df * df;
        }
        pe += sqrt(d);
    }
    *pampjpe = (float)(pe / N * 1000.0);
}

constexpr int kMaxJ = 32;
constexpr int kJC = 6;     // joints regressed per pass over the vertices (kJC * 6 accumulators per lane)

__global__ void __launch_bounds__(256) eval_mesh_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         int V, const float* __restrict__ Jr, int J,
                                                         const int* __restrict__ sel, int nsel, float* __restrict__ mpjpe,
                                                         float* __restrict__ pampjpe, float* __restrict__ v2v) {
    __shared__ float red[4];
    __shared__ float jp[kMaxJ][3], jg[kMaxJ][3];
    __shared__ float sp[kMaxJ * 3], sg[kMaxJ * 3];
    __shared__ float part[4 * kJC * 6], sums[kJC * 6];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* pv = pred + (size_t)b * V * 3;
    const float* gv = gt + (size_t)b * V * 3;
    for (int j0 = 0; j0 < J; j0 += kJC) {
        float a[kJC * 6];
#pragma unroll
        for (int i = 0; i < kJC * 6; ++i) a[i] = 0.f;
        // rows past J alias row J - 1 (unconditional loads - a predicated load would sit in its own exec-masked branch
        // and serialise on the memory latency); their sums are never stored
        const float* wr[kJC];
#pragma unroll
        for (int jj = 0; jj < kJC; ++jj) wr[jj] = Jr + (size_t)min(j0 + jj, J - 1) * V;
#pragma unroll 3
        for (int v = t; v < V; v += 256) {
            const float x[6] = {pv[v * 3 + 0], pv[v * 3 + 1], pv[v * 3 + 2], gv[v * 3 + 0], gv[v * 3 + 1], gv[v * 3 + 2]};
#pragma unroll
            for (int jj = 0; jj < kJC; ++jj) {
                const float w = wr[jj][v];
#pragma unroll
                for (int c = 0; c < 6; ++c) a[jj * 6 + c] = fmaf(w, x[c], a[jj * 6 + c]);
            }
        }
        block_sum_many_256<kJC * 6>(a, part, sums);
        if (t < kJC * 6 && j0 + t / 6 < J) {
            const int jj = t / 6, c = t % 6;
            if (c < 3) jp[j0 + jj][c] = sums[t]; else jg[j0 + jj][c - 3] = sums[t];
        }
    }
    __syncthreads();
    // pelvis-aligned vertex-to-vertex error
    const float ppx = jp[0][0], ppy = jp[0][1], ppz = jp[0][2], gpx = jg[0][0], gpy = jg[0][1], gpz = jg[0][2];
    float acc = 0.f;
#pragma unroll 4
    for (int v = t; v < V; v += 256) {
        const float dx = (gv[v * 3 + 0] - gpx) - (pv[v * 3 + 0] - ppx);
        const float dy = (gv[v * 3 + 1] - gpy) - (pv[v * 3 + 1] - ppy);
        const float dz = (gv[v * 3 + 2] - gpz) - (pv[v * 3 + 2] - ppz);
        acc += sqrtf(dx * dx + dy * dy + dz * dz);
    }
    const float vs = block_sum_256(acc, red);
    if (t < nsel * 3) {
        const int i = t / 3, c = t % 3, j = sel ? sel[i] : i;
        sp[t] = jp[j][c] - jp[0][c];
        sg[t] = jg[j][c] - jg[0][c];
    }
    __syncthreads();
    if (t == 0) {
        if (v2v) v2v[b] = vs / (float)V * 1000.0f;
        float m, pa;
        joint_errors<1>(sp, sg, nsel, &m, &pa);
        if (mpjpe) mpjpe[b] = m;
        if (pampjpe) pampjpe[b] = pa;
    }
}

__global__ void __launch_bounds__(64) eval_joints_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int B,
                                                          int J, float* __restrict__ mpjpe, float* __restrict__ pampjpe) {
    // one lane per pose; the pelvis-aligned joints sit in LDS as [coordinate][lane] (conflict-free, no scratch arrays)
    __shared__ float sp[kMaxJ * 3 * 64], sg[kMaxJ * 3 * 64];
    const int t = threadIdx.x, b0 = blockIdx.x * 64, nb = min(64, B - b0), n3 = J * 3;
    for (int i = t; i < nb * n3; i += 64) {   // coalesced over the block's nb * J * 3 floats
        const int l = i / n3, k = i - l * n3;
        const size_t base = (size_t)(b0 + l) * n3;
        sp[k * 64 + l] = pred[base + k] - pred[base + k % 3];
        sg[k * 64 + l] = gt[base + k] - gt[base + k % 3];
    }
    __syncthreads();
    if (t >= nb) return;
    float m, pa;
    joint_errors<64>(sp + t, sg + t, J, &m, &pa);
    if (mpjpe) mpjpe[b0 + t] = m;
    if (pampjpe) pampjpe[b0 + t] = pa;
}

// ---- the validation step's scores (spec/trainer.py:272-344): per-joint errors in metres, unaligned V2V ------------------------
//
// Similarity fit of N pelvis-aligned joints p onto g (coordinate c of joint i at p[i * 3 + c]), the arithmetic of joint_errors
// above: fit[0..2] = mean of p, fit[3..5] = mean of g, fit[6..14] = scale * R row-major.  Zero variance of p gives 0 / 0 = NaN
// in every entry of scale * R, as in the reference.
__device__ void similarity_fit(const float* p, const float* g, int N, double* fit) {
    double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
    for (int i = 0; i < N; ++i)
        for (int c = 0; c < 3; ++c) { mu1[c] += p[i * 3 + c]; mu2[c] += g[i * 3 + c]; }
    for (int c = 0; c < 3; ++c) { mu1[c] /= N; mu2[c] /= N; }
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0;
    for (int i = 0; i < N; ++i) {
        double x1[3], x2[3];
        for (int c = 0; c < 3; ++c) { x1[c] = p[i * 3 + c] - mu1[c]; x2[c] = g[i * 3 + c] - mu2[c]; var1 += x1[c] * x1[c]; }
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) S[a][b] += x1[a] * x2[b];
    }
    double Nm[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
        {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
        {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
        {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double q[4], lam;
    sym4_max_eig(Nm, q, &lam);
    const double w = q[0], x = q[1], y = q[2], z = q[3], scale = lam / var1;
    const double R[9] = {w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z};
    for (int c = 0; c < 3; ++c) { fit[c] = mu1[c]; fit[3 + c] = mu2[c]; }
    for (int k = 0; k < 9; ++k) fit[6 + k] = scale * R[k];
}

// |p_i - g_i| and |s R (p_i - mu_p) + mu_g - g_i| of one joint, fp64 with one rounding to fp32 each
__device__ __forceinline__ void joint_error(const float* p, const float* g, const double* fit, float* err, float* pa_err) {
    if (err) {
        double d = 0;
        for (int a = 0; a < 3; ++a) {
            const double df = (double)p[a] - (double)g[a];
            d += df * df;
        }
        *err = (float)sqrt(d);
    }
    if (pa_err) {
        double d = 0;
        for (int a = 0; a < 3; ++a) {
            double v = 0;
            for (int b = 0; b < 3; ++b) v += fit[6 + a * 3 + b] * (p[b] - fit[b]);
            const double df = v + fit[3 + a] - g[a];
            d += df * df;
        }
        *pa_err = (float)sqrt(d);
    }
}

// One workgroup per image.  The regression loop is eval_mesh_kernel's (the same summation order, so the same joints); the first
// chunk of joints also accumulates the unaligned V2V from the vertices it already holds, so no pass reads the meshes for V2V
// alone.  Then wave 0 solves the Procrustes problem of the selected regressed joints and wave 1 that of the given joints (lane 0
// each, side by side), and one lane per joint writes that joint's two errors.
__global__ void __launch_bounds__(256) eval_step_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int V,
                                                         const float* __restrict__ Jr, int J, const int* __restrict__ sel, int nsel,
                                                         const float* __restrict__ pj, const float* __restrict__ gj, int Jk,
                                                         float* __restrict__ err_sel, float* __restrict__ pa_err_sel,
                                                         float* __restrict__ err_k, float* __restrict__ pa_err_k,
                                                         float* __restrict__ v2v) {
    __shared__ float red[4];
    __shared__ float jp[kMaxJ][3], jg[kMaxJ][3];
    __shared__ float sp[2][kMaxJ * 3], sg[2][kMaxJ * 3];   // [0] the selected regressed joints, [1] the given joints, pelvis-aligned
    __shared__ float part[4 * kJC * 6], sums[kJC * 6];
    __shared__ double fit[2][15];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* pv = pred + (size_t)b * V * 3;
    const float* gv = gt + (size_t)b * V * 3;
    float acc = 0.f;
    for (int j0 = 0; j0 < J; j0 += kJC) {
        float a[kJC * 6];
#pragma unroll
        for (int i = 0; i < kJC * 6; ++i) a[i] = 0.f;
        const float* wr[kJC];   // rows past J alias row J - 1 (unconditional loads); their sums are never stored
#pragma unroll
        for (int jj = 0; jj < kJC; ++jj) wr[jj] = Jr + (size_t)min(j0 + jj, J - 1) * V;
        const bool first = j0 == 0;
#pragma unroll 3
        for (int v = t; v < V; v += 256) {
            const float x[6] = {pv[v * 3 + 0], pv[v * 3 + 1], pv[v * 3 + 2], gv[v * 3 + 0], gv[v * 3 + 1], gv[v * 3 + 2]};
#pragma unroll
            for (int jj = 0; jj < kJC; ++jj) {
                const float w = wr[jj][v];
#pragma unroll
                for (int c = 0; c < 6; ++c) a[jj * 6 + c] = fmaf(w, x[c], a[jj * 6 + c]);
            }
            if (first) {
                const float dx = x[3] - x[0], dy = x[4] - x[1], dz = x[5] - x[2];
                acc += sqrtf(dx * dx + dy * dy + dz * dz);
            }
        }
        block_sum_many_256<kJC * 6>(a, part, sums);
        if (t < kJC * 6 && j0 + t / 6 < J) {
            const int jj = t / 6, c = t % 6;
            if (c < 3) jp[j0 + jj][c] = sums[t]; else jg[j0 + jj][c - 3] = sums[t];
        }
    }
    const float vs = block_sum_256(acc, red);   // its barriers also publish jp / jg
    if (t == 0 && v2v) v2v[b] = vs / (float)V;
    if (t < nsel * 3) {
        const int i = t / 3, c = t % 3, j = sel ? sel[i] : i;
        sp[0][t] = jp[j][c] - jp[0][c];
        sg[0][t] = jg[j][c] - jg[0][c];
    }
    if (pj && t < Jk * 3) {
        const size_t base = (size_t)b * Jk * 3;
        sp[1][t] = pj[base + t] - pj[base + t % 3];
        sg[1][t] = gj[base + t] - gj[base + t % 3];
    }
    __syncthreads();
    const int w = t >> 6, lane = t & 63;
    const int N = w == 0 ? nsel : (w == 1 && pj) ? Jk : 0;
    float* const err = w == 0 ? err_sel : err_k;
    float* const pa_err = w == 0 ? pa_err_sel : pa_err_k;
    const int q = w & 1;                        // waves 2 and 3 have N = 0 and touch nothing
    if (lane == 0 && N && pa_err) similarity_fit(sp[q], sg[q], N, fit[q]);
    __syncthreads();
    if (lane < N) {
        const size_t o = (size_t)b * N + lane;
        joint_error(sp[q] + lane * 3, sg[q] + lane * 3, fit[q], err ? err + o : nullptr, pa_err ? pa_err + o : nullptr);
    }
}

int launch_eval_step(const float* pred, const float* gt, int B, int V, const float* Jr, int J, const int* sel, int nsel,
                     const float* pj, const float* gj, int Jk, float* err_sel, float* pa_err_sel, float* err_k, float* pa_err_k,
                     float* v2v, const LaunchCtx& ctx) {
    if (J > kMaxJ || nsel > kMaxJ || nsel < 1 || J < 1 || (pj && (Jk > kMaxJ || Jk < 1))) return (int)hipErrorInvalidValue;
    const double nk = pj ? Jk : 0;
    // algorithmic HBM bytes: both meshes once + the regressor once (re-reads per joint chunk come through L2) + the joint sets + the outputs
    ProfScope ps(ctx, "eval_step_metrics", 2.0 * B * (double)V * 6 * J,
                 4.0 * ((double)B * V * 6 + (double)J * V + B * (6.0 * nk + 2.0 * nsel + 2.0 * nk + 1.0)));
    hipLaunchKernelGGL(eval_step_kernel, dim3(B), dim3(256), 0, ctx.stream, pred, gt, V, Jr, J, sel, nsel, pj, gj, Jk, err_sel, pa_err_sel,
                       err_k, pa_err_k, v2v);
    return (int)hipGetLastError();
}

// joints (B,J,3) = J_regressor (J,V) @ vertices (B,V,3)  (torch.einsum('bik,ji->bjk'), compute_error.py:184,187;
// torch.matmul(J_regressor_batch, vertices), :53,58): one workgroup per (image, chunk of kRC joints); the vertices are
// read once per chunk and every load of the loop is independent
constexpr int kRC = 8;
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) regress_joints_kernel(const float* __restrict__ verts, int V,
                                                              const float* __restrict__ Jr, int J, int nchunk,
                                                              float* __restrict__ out) {
    __shared__ float part[4 * kRC * 3], sums[kRC * 3];
    const int b = blockIdx.x / nchunk, j0 = (blockIdx.x % nchunk) * kRC, t = threadIdx.x;
    const float* v = verts + (size_t)b * V * 3;
    float a[kRC * 3];
#pragma unroll
    for (int i = 0; i < kRC * 3; ++i) a[i] = 0.f;
    const float* wr[kRC];      // rows past J alias row J - 1 (unconditional loads); their sums are never stored
#pragma unroll
    for (int jj = 0; jj < kRC; ++jj) wr[jj] = Jr + (size_t)min(j0 + jj, J - 1) * V;
    // two vertices per trip, all 2 * (3 + kRC) loads issued before the first use (the second vertex of a lane's last trip is
    // clamped to a valid index and weighted with zero)
    for (int i = t; i < V; i += 512) {
        const bool two = i + 256 < V;
        const int i2 = two ? i + 256 : i;
        float xa[3], xb[3], wa[kRC], wb[kRC];
#pragma unroll
        for (int c = 0; c < 3; ++c) { xa[c] = v[i * 3 + c]; xb[c] = v[i2 * 3 + c]; }
#pragma unroll
        for (int jj = 0; jj < kRC; ++jj) { wa[jj] = wr[jj][i]; wb[jj] = wr[jj][i2]; }
#pragma unroll
        for (int jj = 0; jj < kRC; ++jj) {
            const float w2 = two ? wb[jj] : 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) a[jj * 3 + c] = fmaf(w2, xb[c], fmaf(wa[jj], xa[c], a[jj * 3 + c]));
        }
    }
    block_sum_many_256<kRC * 3>(a, part, sums);
    if (t < kRC * 3 && j0 + t / 3 < J) out[((size_t)b * J + j0) * 3 + t] = sums[t];
}

int launch_regress_joints(const float* verts, int B, int V, const float* Jr, int J, float* out, const LaunchCtx& ctx) {
    const int nchunk = (J + kRC - 1) / kRC;
    ProfScope ps(ctx, "regress_joints", 2.0 * B * (double)V * 3 * J, 4.0 * ((double)B * V * 3 + (double)J * V + (double)B * J * 3));
    hipLaunchKernelGGL(regress_joints_kernel, dim3(B * nchunk), dim3(256), 0, ctx.stream, verts, V, Jr, J, nchunk, out);
    return (int)hipGetLastError();
}

// out[b,n,:] = R[b] @ x[b,n,:]  (torch.bmm(R, x.transpose(2,1)).transpose(2,1), compute_error.py:164-165,189)
__global__ void __launch_bounds__(256) rotate_points_kernel(const float* __restrict__ R, const float* __restrict__ x,
                                                             int N, long total, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float* r = R + (i / N) * 9;
    const float x0 = x[i * 3 + 0], x1 = x[i * 3 + 1], x2 = x[i * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = r[c * 3 + 0] * x0 + r[c * 3 + 1] * x1 + r[c * 3 + 2] * x2;
}

int launch_rotate_points(const float* R, const float* x, int B, int N, float* out, const LaunchCtx& ctx) {
    const long total = (long)B * N;
    ProfScope ps(ctx, "rotate_points", 18.0 * total, 4.0 * (6.0 * total + 9.0 * B));
    hipLaunchKernelGGL(rotate_points_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx.stream, R, x, N, total, out);
    return (int)hipGetLastError();
}

int launch_eval_mesh(const float* pred, const float* gt, int B, int V, const float* Jr, int J, const int* sel, int nsel,
                     float* mpjpe, float* pampjpe, float* v2v, const LaunchCtx& ctx) {
    if (J > kMaxJ || nsel > kMaxJ || nsel < 1 || J < 1) return (int)hipErrorInvalidValue;
    // algorithmic HBM bytes: both meshes once + the regressor once (re-reads per joint chunk / for V2V come through L2)
    ProfScope ps(ctx, "eval_mesh_metrics", 2.0 * B * (double)V * 6 * J, 4.0 * ((double)B * V * 6 + (double)J * V + 3.0 * B));
    hipLaunchKernelGGL(eval_mesh_kernel, dim3(B), dim3(256), 0, ctx.stream, pred, gt, V, Jr, J, sel, nsel, mpjpe, pampjpe, v2v);
    return (int)hipGetLastError();
}

int launch_eval_joints(const float* pred, const float* gt, int B, int J, float* mpjpe, float* pampjpe, const LaunchCtx& ctx) {
    if (J > kMaxJ || J < 1) return (int)hipErrorInvalidValue;
    ProfScope ps(ctx, "eval_joint_metrics", 0.0, 4.0 * B * J * 6.0);
    hipLaunchKernelGGL(eval_joints_kernel, dim3((B + 63) / 64), dim3(64), 0, ctx.stream, pred, gt, B, J, mpjpe, pampjpe);
    return (int)hipGetLastError();
}

}  // namespace specmi
