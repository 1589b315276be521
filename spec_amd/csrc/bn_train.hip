// bn_train.hip - BatchNorm in training mode with its backward (gfx950): the normalisation of a batch by its own statistics, the
// running-statistics update, the residual and the ReLU of a bottleneck in the forward; g_z, g_gamma, g_beta and g_res in the
// backward.  z / y / residual / g_* are dense fp32 (M, C) with C contiguous - NHWC with M = B H W - gamma / beta / mean / invstd /
// the running statistics are (C) vectors, all read where torch keeps them.
//
// Layout: a workgroup owns a TILE of BN_ROWS = 64 rows x 64 channels, a thread 4 rows x 4 channels of it.  Lanes run along C: 16
// lanes cover the tile's 64 channels, so a wavefront reads 4 adjacent rows of 256 contiguous bytes (1 KiB contiguous at C = 64).
// With C % 4 == 0 and every (M, C) pointer 16-byte aligned a lane loads its 4 channels as one 16-byte vector (lane t: channels
// 4 t .. 4 t + 3); otherwise - the scalar tail - it loads four floats 16 channels apart (lane t: t, t + 16, ..), so the lanes'
// addresses stay adjacent.  A channel's arithmetic never meets another channel's, so both forms give the same bits.  Rows past M
// and channels past C are neither loaded nor stored: no access leaves a tensor.  The tiles are one flat grid, channel tiles fastest.
//
// Forward (z is read once for the statistics and once for the apply):
//   bn_stats_kernel     per tile and channel: the chunk's mean m_k = (sum of its n_k rows) / n_k, then M2_k = sum (z - m_k)^2 from the
//                       SAME registers - a centred second pass without a second read.  Never E[z^2] - E[z]^2.
//   bn_stats_finish     per channel: the chunks' (n_k, m_k, M2_k) pooled in double by Chan's rule in its centred form for many groups,
//                           m = sum n_k m_k / sum n_k,  M2 = sum (M2_k + n_k (m_k - m)^2),
//                       then var = M2 / M (biased), invstd = fp32(1 / sqrt(var + eps)) and the running statistics by torch's rule,
//                           rm = fp32((1 - f) rm + f mean), rv = fp32((1 - f) rv + f var M / (M - 1)),
//                       each evaluated in double from fp32 inputs and rounded once.
//   bn_apply_kernel     y = ((z - mean) invstd) gamma + beta [+ residual], max(., 0) with relu.
// Backward (the reduction and the apply each read z and g_y once), g = relu ? (y > 0 ? g_y : 0) : g_y:
//   bn_bwd_reduce_kernel  per tile and channel: sum g and sum g xhat, xhat = (z - mean) invstd
//   bn_bwd_finish         per channel: the chunks' sums added in double -> g_beta, g_gamma, and g_beta / M, g_gamma / M for the apply
//   bn_bwd_apply_kernel   g_z = gamma invstd (g - g_beta / M - xhat g_gamma / M), g_res = g.  g_res may be g_y itself: an element
//                         is read and written by the same lane, after the reduction has read it.
// With only g_res wanted the two reduction kernels are not launched.
//
// Determinism (the rule of smpl_bwd.hip): no float atomics.  Chunk k is rows 64 k .. 64 k + 63, whatever the device; inside a tile
// a thread adds its rows r, r + 16, r + 32, r + 48 in that order and one thread adds the 16 row lanes' partial sums in lane order;
// the finish kernels give the chunks k, k + 16, k + 32, .. to chunk lane k % 16, which pools them in that order, and pool the 16
// lanes 0 .. 15 in that order.  All of it is fixed by (M, C) alone - never by the CU count or by what else is wanted - so two runs give the
// same bits and a wanted output has the same bits whatever else is wanted.  Unlike the conv layer, image b's output DOES depend on
// the rest of its batch: the statistics are the batch's.
//
// Workspace: (2 ceil(M / 64) + 2) C floats in the handle (the chunk partials; the backward's two per-channel quotients).
// Traffic: the forward reads z twice (statistics, apply), the backward's reduction and apply read z and g_y once each (and y with relu).
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; vector / scalar-tail form): bn_stats_kernel 32 / 30 VGPRs, 4352 B
// of LDS; bn_apply_kernel 32 / 34, no LDS; bn_bwd_reduce_kernel 37 / 36, 4096 B; bn_bwd_apply_kernel 50 / 38, no LDS; bn_bwd_finish 42,
// 4096 B; all at occupancy 8 waves per SIMD; bn_stats_finish 78 (double), 6144 B, occupancy 6.  No AGPRs, scratch 0 and spills 0 in every
// kernel, vector stores only.  Measured errors and times: DESIGN.md section 7, f-23.
#include <initializer_list>

#include "specmi_internal.h"

namespace specmi {

namespace {

constexpr int BN_ROWS = SPECMI_BN_ROWS_PER_CHUNK;      // rows of a chunk: fixes the summation order, so it is part of the arithmetic
constexpr int BN_COLS = 64;                            // channels of a tile
constexpr int RL = 16;                                 // row lanes of a tile: a thread takes rows r, r + 16, .. of the chunk
constexpr int RPT = BN_ROWS / RL;                      // rows per thread
static_assert(BN_ROWS % RL == 0 && BN_COLS == 64, "a tile is 256 threads x (RPT rows x 4 channels)");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the thread's place in its tile
struct Tile {
    int row0, c0, tx, ty, nrows;       // first row and channel of the tile, the thread's channel lane and row lane, rows of the chunk
};

__device__ __forceinline__ Tile tile_of(int M, int C) {
    const int ntc = (C + BN_COLS - 1) / BN_COLS;
    Tile t;
    t.row0 = (int)(blockIdx.x / ntc) * BN_ROWS;
    t.c0 = (int)(blockIdx.x % ntc) * BN_COLS;
    t.tx = threadIdx.x & 15;
    t.ty = threadIdx.x >> 4;
    t.nrows = min(BN_ROWS, M - t.row0);
    return t;
}

// channel j (0 .. 3) of the thread, relative to the tile
template <bool VEC>
__device__ __forceinline__ int chan(const Tile& t, int j) { return VEC ? 4 * t.tx + j : t.tx + 16 * j; }

// the thread's 4 channels of row m (m < M); channels past C read as 0
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p, const Tile& t, int m, int C) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const size_t base = (size_t)m * C + t.c0;
    if (VEC) {
        if (t.c0 + 4 * t.tx < C) v = *reinterpret_cast<const f32x4*>(p + base + 4 * t.tx);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.c0 + chan<false>(t, j) < C) v[j] = p[base + chan<false>(t, j)];
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, const Tile& t, int m, int C, f32x4 v) {
    const size_t base = (size_t)m * C + t.c0;
    if (VEC) {
        if (t.c0 + 4 * t.tx < C) *reinterpret_cast<f32x4*>(p + base + 4 * t.tx) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t.c0 + chan<false>(t, j) < C) p[base + chan<false>(t, j)] = v[j];
    }
}

// a (C) vector at the thread's 4 channels; channels past C read as 0
template <bool VEC>
__device__ __forceinline__ f32x4 chan4(const float* __restrict__ p, const Tile& t, int C) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (t.c0 + chan<VEC>(t, j) < C) v[j] = p[t.c0 + chan<VEC>(t, j)];
    return v;
}

// The 16 row lanes' partial sums of the tile's 64 channels, added in row-lane order by threads 0 .. 63 (thread c: channel c of
// the tile), which get the sum; the other threads get 0.  red is [RL][BN_COLS]; the call is a barrier before and after.
template <bool VEC>
__device__ __forceinline__ float tile_sum(float (*red)[BN_COLS], const Tile& t, f32x4 part) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) red[t.ty][chan<VEC>(t, j)] = part[j];
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < BN_COLS)
#pragma unroll
        for (int r = 0; r < RL; ++r) s += red[r][threadIdx.x];
    return s;
}

// ws[(2 k + 0) C + c] = m_k, ws[(2 k + 1) C + c] = M2_k
template <bool VEC>
__global__ void __launch_bounds__(256) bn_stats_kernel(const float* __restrict__ z, int M, int C, float* __restrict__ ws) {
    __shared__ float red[RL][BN_COLS];
    __shared__ float cmean[BN_COLS];
    const Tile t = tile_of(M, C);
    f32x4 v[RPT], s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = t.ty + RL * i;
        v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (r < t.nrows) { v[i] = load4<VEC>(z, t, t.row0 + r, C); s += v[i]; }
    }
    const float tot = tile_sum<VEC>(red, t, s);
    if (threadIdx.x < BN_COLS) cmean[threadIdx.x] = tot / (float)t.nrows;
    __syncthreads();
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < RPT; ++i)
        if (t.ty + RL * i < t.nrows)
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = v[i][j] - cmean[chan<VEC>(t, j)]; q[j] += d * d; }
    const float m2 = tile_sum<VEC>(red, t, q);
    const int c = t.c0 + (int)threadIdx.x;
    if (threadIdx.x < BN_COLS && c < C) {
        const size_t k = (size_t)(t.row0 / BN_ROWS);
        ws[(2 * k + 0) * C + c] = cmean[threadIdx.x];
        ws[(2 * k + 1) * C + c] = m2;
    }
}

// The finish kernels: a workgroup owns 16 channels (thread & 15) and has 16 chunk lanes (thread >> 4); chunk lane l takes the chunks
// l, l + 16, .. in that order, thread (c, 0) then pools the lanes 0 .. 15 in that order.  Everything here is double.  The moments
// are pooled in the centred form of Chan's rule for many groups at once - first the mean of the groups' means weighted by their
// row counts, then M2 = sum (M2_k + n_k (m_k - mean)^2) - once inside a lane over its chunks and once over the 16 lanes: no division
// sits in a loop, and a constant channel stays exact (every m_k is the constant, every difference 0).
constexpr int FC = 16, FL = 16;

__global__ void __launch_bounds__(256) bn_stats_finish(const float* __restrict__ ws, int M, int C, float eps, float f, float* running_mean,
                                                       float* running_var, float* __restrict__ mean, float* __restrict__ invstd) {
#pragma clang fp contract(off)      // the double expressions below are rounded operation by operation, as a host evaluates them
    __shared__ double sh[3][FL][FC];
    const int cl = threadIdx.x & (FC - 1), l = threadIdx.x / FC, c = (int)blockIdx.x * FC + cl;
    const int nk = (M + BN_ROWS - 1) / BN_ROWS;
    double n = 0.0, sm = 0.0, m2 = 0.0;
    if (c < C) {
        for (int k = l; k < nk; k += FL) {
            const double nb = (double)min(BN_ROWS, M - k * BN_ROWS);
            n += nb;
            sm += nb * (double)ws[(size_t)(2 * k + 0) * C + c];
        }
        if (n > 0.0) sm /= n;                  // the lane's mean
        for (int k = l; k < nk; k += FL) {
            const double nb = (double)min(BN_ROWS, M - k * BN_ROWS), d = (double)ws[(size_t)(2 * k + 0) * C + c] - sm;
            m2 += (double)ws[(size_t)(2 * k + 1) * C + c] + nb * (d * d);
        }
    }
    sh[0][l][cl] = n; sh[1][l][cl] = sm; sh[2][l][cl] = m2;
    __syncthreads();
    if (l > 0 || c >= C) return;
    double mu_d = 0.0, M2 = 0.0;
#pragma unroll
    for (int u = 0; u < FL; ++u) mu_d += sh[0][u][cl] * sh[1][u][cl];
    mu_d /= (double)M;
#pragma unroll
    for (int u = 0; u < FL; ++u) { const double d = sh[1][u][cl] - mu_d; M2 += sh[2][u][cl] + sh[0][u][cl] * (d * d); }
    const double var = M2 / (double)M;
    const float mu = (float)mu_d;
    mean[c] = mu;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double fd = (double)f;
        running_mean[c] = (float)((1.0 - fd) * (double)running_mean[c] + fd * (double)mu);
        running_var[c] = (float)((1.0 - fd) * (double)running_var[c] + fd * (var * (double)M / (double)(M - 1)));
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) bn_apply_kernel(const float* __restrict__ z, int M, int C, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ residual, int relu,
                                                       float* __restrict__ y) {
    const Tile t = tile_of(M, C);
    const f32x4 mu = chan4<VEC>(mean, t, C), is = chan4<VEC>(invstd, t, C), ga = chan4<VEC>(gamma, t, C), be = chan4<VEC>(beta, t, C);
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = t.ty + RL * i;
        if (r >= t.nrows) continue;
        const int m = t.row0 + r;
        f32x4 v = (load4<VEC>(z, t, m, C) - mu) * is * ga + be;
        if (residual) v += load4<VEC>(residual, t, m, C);
        if (relu)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
        store4<VEC>(y, t, m, C, v);
    }
}

// the gradient that reaches the normalisation: an output that is exactly zero passes none (the convention of conv_bwd.hip)
template <bool VEC>
__device__ __forceinline__ f32x4 masked_grad(const float* g_y, const float* y, int relu, const Tile& t, int m, int C) {
    f32x4 g = load4<VEC>(g_y, t, m, C);
    if (relu) {
        const f32x4 yy = load4<VEC>(y, t, m, C);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!(yy[j] > 0.f)) g[j] = 0.f;
    }
    return g;
}

// ws[(2 k + 0) C + c] = sum g, ws[(2 k + 1) C + c] = sum g xhat over chunk k
template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const float* __restrict__ z, int M, int C, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* y, int relu, const float* g_y,
                                                            float* __restrict__ ws) {
    __shared__ float red[RL][BN_COLS];
    const Tile t = tile_of(M, C);
    const f32x4 mu = chan4<VEC>(mean, t, C), is = chan4<VEC>(invstd, t, C);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = t.ty + RL * i;
        if (r >= t.nrows) continue;
        const int m = t.row0 + r;
        const f32x4 g = masked_grad<VEC>(g_y, y, relu, t, m, C);
        const f32x4 xh = (load4<VEC>(z, t, m, C) - mu) * is;
        s1 += g;
        s2 += g * xh;
    }
    const float a = tile_sum<VEC>(red, t, s1);
    const float b = tile_sum<VEC>(red, t, s2);
    const int c = t.c0 + (int)threadIdx.x;
    if (threadIdx.x < BN_COLS && c < C) {
        const size_t k = (size_t)(t.row0 / BN_ROWS);
        ws[(2 * k + 0) * C + c] = a;
        ws[(2 * k + 1) * C + c] = b;
    }
}

// quot[c] = g_beta / M, quot[C + c] = g_gamma / M; g_gamma / g_beta may be null
__global__ void __launch_bounds__(256) bn_bwd_finish(const float* __restrict__ ws, int M, int C, float* __restrict__ g_gamma,
                                                     float* __restrict__ g_beta, float* __restrict__ quot) {
    __shared__ double sh[2][FL][FC];
    const int cl = threadIdx.x & (FC - 1), l = threadIdx.x / FC, c = (int)blockIdx.x * FC + cl;
    const int nk = (M + BN_ROWS - 1) / BN_ROWS;
    double a = 0.0, b = 0.0;
    if (c < C)
        for (int k = l; k < nk; k += FL) { a += (double)ws[(size_t)(2 * k + 0) * C + c]; b += (double)ws[(size_t)(2 * k + 1) * C + c]; }
    sh[0][l][cl] = a; sh[1][l][cl] = b;
    __syncthreads();
    if (l > 0 || c >= C) return;
    a = 0.0; b = 0.0;
#pragma unroll
    for (int u = 0; u < FL; ++u) { a += sh[0][u][cl]; b += sh[1][u][cl]; }
    if (g_beta) g_beta[c] = (float)a;
    if (g_gamma) g_gamma[c] = (float)b;
    quot[c] = (float)(a / (double)M);
    quot[C + c] = (float)(b / (double)M);
}

// g_z and g_res, either may be null (then quot / gamma are not read for g_z)
template <bool VEC>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* __restrict__ z, int M, int C, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd, const float* y,
                                                           int relu, const float* g_y, const float* __restrict__ quot, float* g_z, float* g_res) {
    const Tile t = tile_of(M, C);
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is = mu, k = mu, qa = mu, qb = mu;
    if (g_z) {
        mu = chan4<VEC>(mean, t, C); is = chan4<VEC>(invstd, t, C); k = chan4<VEC>(gamma, t, C) * is;
        qa = chan4<VEC>(quot, t, C); qb = chan4<VEC>(quot + C, t, C);
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = t.ty + RL * i;
        if (r >= t.nrows) continue;
        const int m = t.row0 + r;
        const f32x4 g = masked_grad<VEC>(g_y, y, relu, t, m, C);
        if (g_z) {
            const f32x4 xh = (load4<VEC>(z, t, m, C) - mu) * is;
            store4<VEC>(g_z, t, m, C, k * (g - qa - xh * qb));
        }
        if (g_res) store4<VEC>(g_res, t, m, C, g);
    }
}

bool vec_ok(int C, std::initializer_list<const void*> ps) {
    if (C % 4) return false;
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

long bn_tiles(int M, int C) { return (long)((M + BN_ROWS - 1) / BN_ROWS) * ((C + BN_COLS - 1) / BN_COLS); }

}  // namespace

size_t bn_ws_floats(int M, int C) { return (2 * (size_t)((M + BN_ROWS - 1) / BN_ROWS) + 2) * (size_t)C; }

int launch_bn_train_forward(const BnArgs& a, const float* beta, const float* residual, float eps, float f, float* running_mean,
                            float* running_var, float* y, float* mean, float* invstd, float* ws, const LaunchCtx& ctx) {
    const long tiles = bn_tiles(a.M, a.C);
    if (tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
    const double count = (double)a.M * a.C;
    const bool vec = vec_ok(a.C, {a.z, residual, y});
    const unsigned nfin = (unsigned)((a.C + FC - 1) / FC);
    {
        ProfScope ps(ctx, "bn_train_stats", 4.0 * count, 4.0 * count);
        if (vec) hipLaunchKernelGGL(bn_stats_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, ws);
        else hipLaunchKernelGGL(bn_stats_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, ws);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    {
        ProfScope ps(ctx, "bn_train_finish", 0.0, 4.0 * (double)bn_ws_floats(a.M, a.C));
        hipLaunchKernelGGL(bn_stats_finish, dim3(nfin), dim3(256), 0, ctx.stream, ws, a.M, a.C, eps, f, running_mean, running_var, mean, invstd);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    ProfScope ps(ctx, "bn_train_apply", 4.0 * count, 4.0 * count * (residual ? 3 : 2));
    if (vec) hipLaunchKernelGGL(bn_apply_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, a.gamma, beta, mean, invstd, residual, a.relu, y);
    else hipLaunchKernelGGL(bn_apply_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, a.gamma, beta, mean, invstd, residual, a.relu, y);
    return (int)hipGetLastError();
}

int launch_bn_backward(const BnArgs& a, const float* mean, const float* invstd, const float* y, const float* g_y, float* g_z, float* g_gamma,
                       float* g_beta, float* g_res, float* ws, const LaunchCtx& ctx) {
    const long tiles = bn_tiles(a.M, a.C);
    if (tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
    const double count = (double)a.M * a.C;
    const bool vec = vec_ok(a.C, {a.z, y, g_y, g_z, g_res});
    const int relu = a.relu;
    float* const quot = ws + (bn_ws_floats(a.M, a.C) - 2 * (size_t)a.C);
    if (g_z || g_gamma || g_beta) {
        {
            ProfScope ps(ctx, "bn_bwd_reduce", 5.0 * count, 4.0 * count * (relu ? 3 : 2));
            if (vec) hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, mean, invstd, y, relu, g_y, ws);
            else hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, mean, invstd, y, relu, g_y, ws);
            if (const int rc = (int)hipGetLastError()) return rc;
        }
        ProfScope ps(ctx, "bn_bwd_finish", 0.0, 4.0 * (double)bn_ws_floats(a.M, a.C));
        hipLaunchKernelGGL(bn_bwd_finish, dim3((unsigned)((a.C + FC - 1) / FC)), dim3(256), 0, ctx.stream, ws, a.M, a.C, g_gamma, g_beta, quot);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    if (g_z || g_res) {
        const int n_in = (g_z ? 2 : 1) + (relu ? 1 : 0), n_out = (g_z ? 1 : 0) + (g_res ? 1 : 0);
        ProfScope ps(ctx, "bn_bwd_apply", 6.0 * count, 4.0 * count * (n_in + n_out));
        if (vec) hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, a.gamma, mean, invstd, y, relu, g_y, quot, g_z, g_res);
        else hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a.z, a.M, a.C, a.gamma, mean, invstd, y, relu, g_y, quot, g_z, g_res);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

}  // namespace specmi
