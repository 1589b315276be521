// pool_bwd.hip - MaxPool2d(3, 2, 1) for training (gfx950): the forward that records which tap won, and the gradient.  x / g_x are
// (B, H, W, C) and y / g_y (B, OH, OW, C) dense NHWC fp32, idx one uint8 per output element, OH = (H - 1) / 2 + 1.
//
// Forward: a lane owns one output pixel's 4 channels (one 16-byte vector) - or one channel in the scalar form - and scans the
// in-range taps of its window in (ky, kx) ascending order with torch's rule: a tap replaces the best so far when
// v > best || isnan(v).  The first of equal maxima therefore wins, a padding tap is never looked at, and idx = ky * 3 + kx of the
// tap the scan ends on.  All nine taps are loaded first from coordinates clamped into the image (maxpool3x3s2_kernel's reason: one
// wait for nine loads); a clamped tap is outside the window and is skipped by the scan.  y is the value the scan ends on; without
// a NaN in the window that is the maximum, formed here by maxpool3x3s2_kernel's own fmaxf chain so that the bits are its bits.
//
// Backward, gather form: a lane owns one INPUT pixel's 4 channels.  Row iy lies in the windows oy = iy / 2 and, for odd iy,
// (iy + 1) / 2 (when < OH); columns alike: at most 2 x 2 windows.  They are visited in (oy, ox) ascending order, and g_y is added
// where the window's idx names this pixel (ky = iy + 1 - 2 oy, kx = ix + 1 - 2 ox).  The sum is kept in double and rounded once:
// up to four fp32 addends are then summed exactly (unless their exponents lie more than 29 bits apart), so g_x is the correctly
// rounded sum.  Every element of g_x is written exactly once, pixels that never won get +0.  No atomics; a pixel's sum reads its
// own image only, so the bits are fixed by the shape and image b's bits do not depend on its batch.
//
// The vector forms need C % 4 == 0, 16-byte aligned float tensors and a 4-byte aligned idx; everything else takes the scalar forms,
// which run the same operations per element in the same order and so give the same bits.
#include "specmi_internal.h"

namespace specmi {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned char u8x4 __attribute__((ext_vector_type(4)));

template <typename T> struct PoolVec;
template <> struct PoolVec<float> { typedef unsigned char Idx; static constexpr int n = 1; };
template <> struct PoolVec<f32x4> { typedef u8x4 Idx; static constexpr int n = 4; };

__device__ inline float lane_of(float v, int) { return v; }
__device__ inline float lane_of(const f32x4& v, int j) { return v[j]; }
__device__ inline void set_lane(float& v, int, float s) { v = s; }
__device__ inline void set_lane(f32x4& v, int j, float s) { v[j] = s; }
__device__ inline unsigned lane_of(unsigned char v, int) { return v; }
__device__ inline unsigned lane_of(const u8x4& v, int j) { return v[j]; }
__device__ inline void set_lane(unsigned char& v, int, unsigned s) { v = (unsigned char)s; }
__device__ inline void set_lane(u8x4& v, int j, unsigned s) { v[j] = (unsigned char)s; }

// T = f32x4: CV = C / 4 vectors per pixel; T = float: CV = C.  total = B OH OW CV < 2^31 (the launcher checks it).
template <typename T>
__global__ void __launch_bounds__(256) maxpool_train_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                                 typename PoolVec<T>::Idx* __restrict__ idx, int H, int W, int CV, int OH,
                                                                 int OW, unsigned total) {
    constexpr int NV = PoolVec<T>::n;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned cv = i % (unsigned)CV;
    unsigned pix = i / (unsigned)CV;
    const int ox = (int)(pix % (unsigned)OW); pix /= (unsigned)OW;
    const int oy = (int)(pix % (unsigned)OH);
    const unsigned b = pix / (unsigned)OH;
    const T* img = x + (size_t)b * H * W * CV + cv;
    T v[9];
    bool in[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int ty = oy * 2 - 1 + ky, iy = min(max(ty, 0), H - 1);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int tx = ox * 2 - 1 + kx, ix = min(max(tx, 0), W - 1);
            v[ky * 3 + kx] = img[((size_t)iy * W + ix) * CV];
            in[ky * 3 + kx] = ty == iy && tx == ix;
        }
    }
    // the first in-range tap: where torch's scan starts (its index stands when no tap replaces -inf)
    const unsigned first = (oy == 0 ? 3u : 0u) + (ox == 0 ? 1u : 0u);
    T out;
    typename PoolVec<T>::Idx tap;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        float best = -INFINITY, m = lane_of(v[0], j);
        unsigned at = first;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float s = lane_of(v[k], j);
            if (k) m = fmaxf(m, s);                        // maxpool3x3s2_kernel's chain over the clamped taps: its bits
            if (in[k] && (s > best || s != s)) { best = s; at = (unsigned)k; }
        }
        set_lane(out, j, best != best ? best : m);
        set_lane(tap, j, at);
    }
    y[i] = out;
    idx[i] = tap;
}

// total = B H W CV < 2^31
template <typename T>
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const T* __restrict__ g_y, const typename PoolVec<T>::Idx* __restrict__ idx,
                                                           T* __restrict__ g_x, int H, int W, int CV, int OH, int OW, unsigned total) {
    constexpr int NV = PoolVec<T>::n;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned cv = i % (unsigned)CV;
    unsigned pix = i / (unsigned)CV;
    const int ix = (int)(pix % (unsigned)W); pix /= (unsigned)W;
    const int iy = (int)(pix % (unsigned)H);
    const unsigned b = pix / (unsigned)H;
    const size_t base = (size_t)b * OH * OW * CV + cv;
    // the windows (oy, ox) ascending; the second row / column exists for an odd coordinate whose next window is inside the output
    T g[4];
    typename PoolVec<T>::Idx t[4];
    unsigned want[4];
    bool ok[4];
#pragma unroll
    for (int wy = 0; wy < 2; ++wy) {
        const int oy = iy / 2 + wy;
        const bool yok = wy == 0 || ((iy & 1) && oy < OH);
        const int oyc = yok ? oy : iy / 2;
#pragma unroll
        for (int wx = 0; wx < 2; ++wx) {
            const int ox = ix / 2 + wx;
            const bool xok = wx == 0 || ((ix & 1) && ox < OW);
            const int oxc = xok ? ox : ix / 2;
            const size_t o = base + ((size_t)oyc * OW + oxc) * CV;
            g[wy * 2 + wx] = g_y[o];                       // (loaded from a window of this pixel in any case, then not counted)
            t[wy * 2 + wx] = idx[o];
            ok[wy * 2 + wx] = yok && xok;
            want[wy * 2 + wx] = (unsigned)((iy + 1 - 2 * oyc) * 3 + (ix + 1 - 2 * oxc));
        }
    }
    T out;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k] && lane_of(t[k], j) == want[k]) s += (double)lane_of(g[k], j);
        set_lane(out, j, (float)s);
    }
    g_x[i] = out;
}

bool vec_ok(int C, std::initializer_list<const void*> f32, const void* idx) {
    if (C % 4 || (reinterpret_cast<uintptr_t>(idx) & 3)) return false;
    for (const void* p : f32)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

}  // namespace

int launch_maxpool_train_forward(const float* x, int B, int H, int W, int C, float* y, unsigned char* idx, const LaunchCtx& ctx) {
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const bool vec = vec_ok(C, {x, y}, idx);
    const int CV = vec ? C / 4 : C;
    const long total = (long)B * OH * OW * CV;
    if ((long)B * H * W * C >= (1L << 31) || total > 0x7fffff00L) return (int)hipErrorInvalidValue;
    ProfScope ps(ctx, "maxpool_train_fwd", 0.0, 4.0 * B * H * W * C + 5.0 * B * OH * OW * C);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(maxpool_train_fwd_kernel<f32x4>, grid, dim3(256), 0, ctx.stream, reinterpret_cast<const f32x4*>(x),
                           reinterpret_cast<f32x4*>(y), reinterpret_cast<u8x4*>(idx), H, W, CV, OH, OW, (unsigned)total);
    else
        hipLaunchKernelGGL(maxpool_train_fwd_kernel<float>, grid, dim3(256), 0, ctx.stream, x, y, idx, H, W, CV, OH, OW, (unsigned)total);
    return (int)hipGetLastError();
}

int launch_maxpool_backward(const float* g_y, const unsigned char* idx, int B, int H, int W, int C, float* g_x, const LaunchCtx& ctx) {
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const bool vec = vec_ok(C, {g_y, g_x}, idx);
    const int CV = vec ? C / 4 : C;
    const long total = (long)B * H * W * CV;
    if ((long)B * H * W * C >= (1L << 31) || total > 0x7fffff00L) return (int)hipErrorInvalidValue;
    ProfScope ps(ctx, "maxpool_bwd", 0.0, 4.0 * B * H * W * C + 5.0 * B * OH * OW * C);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(maxpool_bwd_kernel<f32x4>, grid, dim3(256), 0, ctx.stream, reinterpret_cast<const f32x4*>(g_y),
                           reinterpret_cast<const u8x4*>(idx), reinterpret_cast<f32x4*>(g_x), H, W, CV, OH, OW, (unsigned)total);
    else
        hipLaunchKernelGGL(maxpool_bwd_kernel<float>, grid, dim3(256), 0, ctx.stream, g_y, idx, g_x, H, W, CV, OH, OW, (unsigned)total);
    return (int)hipGetLastError();
}

}  // namespace specmi
