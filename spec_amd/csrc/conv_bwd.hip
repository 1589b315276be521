// conv_bwd.hip - one fused ResNet layer for training: y = act(conv(x, W) * scale + shift [+ res]) with its three gradients
// (gfx950).  x / y / res are dense NHWC fp32, W is torch's own OIHW fp32 tensor read where it lies at every call - the optimiser
// rewrites it every step, nothing is packed, uploaded or committed (the rule of head_bwd.hip) - scale / shift are the frozen
// BatchNorm as an affine map.  Layer shapes: 1x1 pad 0 and 3x3 pad 1, stride 1 or 2, and the stem's 7x7 pad 3 stride 2; any
// B, H, W, Cin, Cout >= 1.
//
// Three products, implicit GEMMs with gathered addressing, on ONE kernel template (conv_gemm_kernel<MODE>): head_gemm_tile's
// scheme - a workgroup owns a 32 x 32 tile of the product, its four waves take the k groups of 8 round robin on
// v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fma chain), wave 0 adds the other three accumulators in wave order through
// LDS; elements past an extent or in the padding are loaded from a clamped address and replaced by zero, so no access leaves a
// tensor.  The contraction is cut into SEGMENTS whose addressing is affine, and each segment into groups of 8 (the last one
// padded with zeros); group t of the flat list (segment-major) belongs to wave t % 4:
//     forward (MODE 0)   Y[p, o]    = sum X[gather(p, ky, kx), ci] W[o, ci, ky, kx]    segment = tap (ky, kx), inside it ci; W is
//                        read from a per-call device transpose [tap][ci][o] in the workspace (conv_wt_kernel), so that the 32
//                        lanes of a column tile read 128 contiguous bytes
//     data gradient (1)  g_x[q, ci] = sum G[scatter^-1(q, ky, kx), o] W[o, ci, ky, kx] segment = tap (ky, kx), inside it o; a tap
//                        contributes only where (iy + pad - ky) and (ix + pad - kx) are divisible by the stride and the output
//                        pixel is in range
//     weight gradient (2) g_W[o, (ci, ky, kx)] = sum G[p, o] X[gather(p, ky, kx), ci]  segment = output row (b, oy), inside it ox:
//                        the output pixels in (b, oy, ox) order
// The 7x7 stem's forward cuts its contraction otherwise (conv_gemm_kernel<0, true>): with Cin = 3 a tap segment would fill 3 of a
// group's 8 slots, but in NHWC the (kx, ci) run of one kernel row is contiguous (21 floats), so there a segment is a kernel ROW
// ky, nseg = KH and Kc = KW Cin, with the ix range checked per element; the transpose [tap][ci][o] already has that order.
// A weight gradient with few tiles and many output rows (the stem: 10 tiles over B OH = 19200 rows at 64 frames of 600 x 1000)
// is SPLIT (conv_gemm_kernel<2, true>): S = conv_wgrad_splits(shape) > 1, workgroup (tile, s) takes q = nseg / S contiguous segments
// and one more where s < nseg % S, starting at s q + min(s, nseg % S), and writes its tile of partial s (S M N floats of workspace
// behind G); conv_wgrad_reduce_kernel adds the partials in the order s = 0 .. S - 1.  S == 1 is the one launch described above.
// The gradient operand G = g_z * scale[o], g_z = relu ? (y > 0 ? g_y : 0) : g_y, is written by one elementwise pre-pass
// (conv_bwd_prep_kernel) into the handle's workspace, with g_res = g_z beside it when wanted: the data gradient reads every
// element of G KH KW / stride^2 times and the weight gradient once per column tile, so forming it from three tensors inside the
// operand load would multiply that traffic by three.
//
// Determinism (the rule of smpl_bwd.hip): no float atomics; the segments, the groups and their split among the waves are fixed
// by the layer's shape - for MODE 0 / 1 by the per-image shape alone, a row of the product never meets another row - so two
// runs give the same bits, image b's y, g_x and g_res have the same bits in any batch and g_W depends on the shapes alone.  Each
// product is its own launch and reads only G: a wanted output has the same bits whatever else is wanted.
#include "specmi_internal.h"

namespace specmi {

namespace {

constexpr int KU = 4;      // k groups of 8 a wave loads before it multiplies

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvGemmArgs {
    const float* A;            // MODE 0: x, 1: G, 2: G
    const float* Bm;           // MODE 0: w transposed to [tap][ci][o] (conv_wt_kernel), 1: w, 2: x
    const float* scale;        // epilogue (MODE 0): v = acc * scale[n] + shift[n]; null = v = acc
    const float* shift;
    const float* res;          // [m ldc + n] or null; may be C itself (an element is read and written by one lane)
    float* C; long ldc;
    int relu;
    int B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad;
    int M, N;                  // the product's extents
    int nseg, Kc;              // segments and the contraction length inside one
    int S;                     // MODE 2: the splits of the segment list (gridDim.y); S > 1 writes partials, S == 1 writes C
    float* part;               // MODE 2, S > 1: S partial products of M x N floats, split s at part + s M N
};

// ALT selects the second form of a product, compiled apart so that the first form's code stays as it was: MODE 0 - a segment is a
// kernel ROW ky with (kx, ci) inside it (the 7x7 stem); MODE 2 - the segment list is split over gridDim.y (S > 1)
template <int MODE, bool ALT>
__global__ void __launch_bounds__(256) conv_gemm_kernel(const ConvGemmArgs a) {
    __shared__ float part[3][16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    // the tiles as one list, column tiles fastest: neighbouring workgroups share their rows of A (and no grid extent is outgrown)
    const int ntn = (a.N + 31) / 32;
    const int m0 = (int)(blockIdx.x / ntn) * 32, n0 = (int)(blockIdx.x % ntn) * 32;
    const bool mok = m0 + c < a.M, nok = n0 + c < a.N;
    const int m = mok ? m0 + c : 0, n = nok ? n0 + c : 0;
    const int KK = a.KH * a.KW;
    // the lane's row and column, decoded once
    int rb = 0, ry = 0, rx = 0;            // MODE 0: output pixel (b, oy, ox) of row m; MODE 1: input pixel (b, iy, ix)
    int nci = 0, nky = 0, nkx = 0;         // MODE 2: column n = (ci, ky, kx)
    if (MODE == 0) { rx = m % a.OW; const int t = m / a.OW; ry = t % a.OH; rb = t / a.OH; }
    if (MODE == 1) { rx = m % a.W; const int t = m / a.W; ry = t % a.H; rb = t / a.H; }
    if (MODE == 2) { nkx = n % a.KW; const int t = n / a.KW; nky = t % a.KH; nci = t / a.KH; }
    // split s of S takes q = nseg / S contiguous segments, and one more where s < r = nseg % S: it starts at s q + min(s, r)
    int seg_lo = 0, nseg = a.nseg;
    if (MODE == 2 && ALT) {
        const int s = (int)blockIdx.y, q = a.nseg / a.S, r = a.nseg - q * a.S;
        seg_lo = s * q + min(s, r);
        nseg = q + (s < r ? 1 : 0);
    }
    const int ng = (a.Kc + 7) / 8, T = nseg * ng;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int t0 = w; t0 < T; t0 += 4 * KU) {      // (the trip count is the wave's: every lane is in every MFMA)
        float av[KU][4], bv[KU][4];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int t = t0 + 4 * u;
            const bool tok = t < T;
            const int sl = tok ? t / ng : 0, seg = seg_lo + sl;
            const int c0 = (tok ? t - sl * ng : 0) * 8 + 4 * h;
            const float* pa = nullptr; const float* pb = nullptr;
            long sa = 0, sb = 0;
            int bx0 = 0;                           // MODE 2: ix of element 0 of the segment; the elements step by the stride
            if (MODE == 0 && ALT) {
                const int iy = ry * a.stride - a.pad + seg;
                bx0 = rx * a.stride - a.pad;       // ix of kx = 0; element cj = (kx, ci) lies cj floats past it, in range or not
                if (tok && mok && iy >= 0 && iy < a.H) pa = a.A + ((size_t)(rb * a.H + iy) * a.W) * a.Cin;
                sa = 1;
                if (tok && nok) pb = a.Bm + (size_t)seg * a.Kc * a.Cout + n;      // [ky][kx][ci][o] is the transpose's own order
                sb = a.Cout;
            } else if (MODE == 0) {
                const int ky = seg / a.KW, kx = seg - ky * a.KW;
                const int iy = ry * a.stride - a.pad + ky, ix = rx * a.stride - a.pad + kx;
                if (tok && mok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) pa = a.A + ((size_t)(rb * a.H + iy) * a.W + ix) * a.Cin;
                sa = 1;
                if (tok && nok) pb = a.Bm + (size_t)seg * a.Cin * a.Cout + n;     // the per-call transpose [tap][ci][o]: lanes read along o
                sb = a.Cout;
            } else if (MODE == 1) {
                const int ky = seg / a.KW, kx = seg - ky * a.KW;
                const int ty = ry + a.pad - ky, tx = rx + a.pad - kx;
                const int oy = ty / a.stride, ox = tx / a.stride;
                if (tok && mok && ty >= 0 && tx >= 0 && oy * a.stride == ty && ox * a.stride == tx && oy < a.OH && ox < a.OW)
                    pa = a.A + ((size_t)(rb * a.OH + oy) * a.OW + ox) * a.Cout;
                sa = 1;
                if (tok && nok) pb = a.Bm + (size_t)n * KK + seg;
                sb = (long)a.Cin * KK;
            } else {
                const int b = seg / a.OH, oy = seg - b * a.OH;
                if (tok && mok) pa = a.A + (size_t)seg * a.OW * a.Cout + m;
                sa = a.Cout;
                const int iy = oy * a.stride - a.pad + nky;
                bx0 = nkx - a.pad;
                if (tok && nok && iy >= 0 && iy < a.H) pb = a.Bm + ((size_t)(b * a.H + iy) * a.W) * a.Cin + nci;
                sb = a.Cin;                        // per ix
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cj = c0 + j;
                const bool kok = cj < a.Kc;
                bool aok = kok && pa, bok = kok && pb;
                size_t oa = aok ? (size_t)cj * sa : 0, ob = 0;
                if (MODE == 2) {
                    const int ix = cj * a.stride + bx0;
                    bok = bok && ix >= 0 && ix < a.W;
                    ob = bok ? (size_t)ix * sb : 0;
                } else if (MODE == 0 && ALT) {
                    const int ix = bx0 + cj / a.Cin;
                    aok = aok && ix >= 0 && ix < a.W;
                    oa = aok ? (size_t)((long)bx0 * a.Cin + cj) : 0;           // = ix Cin + ci >= 0
                    ob = bok ? (size_t)cj * sb : 0;
                } else {
                    ob = bok ? (size_t)cj * sb : 0;
                }
                const float x = (aok ? pa : a.A)[oa], y = (bok ? pb : a.Bm)[ob];
                av[u][j] = aok ? x : 0.f;
                bv[u][j] = bok ? y : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][j], bv[u][j], acc, 0, 0, 0);
    }
    if (w > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) part[w - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += part[u][r][lane];
    if (!nok) return;
    const float sc = a.scale ? a.scale[n] : 1.f, sh = a.scale ? a.shift[n] : 0.f;
    float* const C = (MODE == 2 && ALT) ? a.part + (size_t)blockIdx.y * a.M * a.N : a.C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mr = m0 + 4 * h + (r & 3) + 8 * (r >> 2);
        if (mr >= a.M) continue;
        float v = acc[r];
        if (a.scale) v = v * sc + sh;
        if (a.res) v += a.res[(size_t)mr * a.ldc + n];
        if (a.relu) v = v > 0.f ? v : 0.f;
        C[(size_t)mr * a.ldc + n] = v;
    }
}

// G[i] = g_z * scale[o], g_res[i] = g_z with g_z = relu ? (y > 0 ? g_y : 0) : g_y; either output may be null.  g_res may be g_y
// itself: an element is read and written by the same lane.
__global__ void __launch_bounds__(256) conv_bwd_prep_kernel(const float* g_y, const float* y, const float* __restrict__ scale,
                                                            int relu, size_t count, int Cout, float* G, float* g_res) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float gz = g_y[i];
    if (relu && !(y[i] > 0.f)) gz = 0.f;
    if (G) G[i] = gz * scale[i % (size_t)Cout];
    if (g_res) g_res[i] = gz;
}

// wt[tap][ci][o] = w[o][ci][tap]: the forward's B operand with its lanes (o) contiguous, rewritten at every call - the weights are
// the optimiser's - and counted in the layer's time (2.4 M floats for layer4's 3x3)
__global__ void __launch_bounds__(256) conv_wt_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cout, int Cin, int KK) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Cout * Cin * KK) return;
    const int o = (int)(i % Cout);
    const size_t t = i / Cout;
    const int ci = (int)(t % Cin), tap = (int)(t / Cin);
    wt[i] = w[((size_t)o * Cin + ci) * KK + tap];
}

ConvGemmArgs base_args(const ConvTrainArgs& t) {
    ConvGemmArgs g;
    g.A = nullptr; g.Bm = nullptr; g.scale = nullptr; g.shift = nullptr; g.res = nullptr; g.C = nullptr; g.ldc = 0; g.relu = 0;
    g.B = t.B; g.H = t.H; g.W = t.W; g.Cin = t.Cin; g.OH = t.OH; g.OW = t.OW; g.Cout = t.Cout;
    g.KH = t.KH; g.KW = t.KW; g.stride = t.stride; g.pad = t.pad;
    g.M = g.N = g.nseg = g.Kc = 0;
    g.S = 1; g.part = nullptr;
    return g;
}

template <int MODE, bool ALT = false>
int launch_gemm(const char* name, const ConvGemmArgs& g, const LaunchCtx& ctx) {
    const double K = (double)g.nseg * g.Kc;
    ProfScope ps(ctx, name, 2.0 * g.M * g.N * K, 4.0 * ((double)g.M * K + K * g.N + (double)g.M * g.N));
    const long tiles = (long)((g.N + 31) / 32) * ((g.M + 31) / 32);
    if (tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_gemm_kernel<MODE, ALT>), dim3((unsigned)tiles, (unsigned)g.S), dim3(256), 0, ctx.stream, g);
    return (int)hipGetLastError();
}

// g_w[i] = part[0][i] + part[1][i] + ... + part[S - 1][i], added in that order
__global__ void __launch_bounds__(256) conv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ g_w, unsigned count, int S) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    float v = part[i];
    for (int s = 1; s < S; ++s) v += part[(size_t)s * count + i];
    g_w[i] = v;
}

}  // namespace

// The splits of the weight gradient's contraction, a function of the layer's shape alone (never of the device).  The product has
// tiles = ceil(Cout / 32) ceil(Cin KH KW / 32) workgroups and nseg = B OH segments.  One launch (S = 1) where it fills the part
// anyway (tiles >= WGRAD_FULL) or the contraction is short (nseg < WGRAD_MIN_NSEG); otherwise as many splits as leave each one
// WGRAD_MIN_SEGS segments, at most WGRAD_MAX_SPLITS.  The two constants are measured (profiles/trunk_train_aux.json):
// at 64 frames of 600 x 1000 the stem's, layer1's and layer2's weight gradients kept getting faster up to S = 256 - 512, whatever the
// tile count (4 .. 144), and slower again at 1024, where layer2's 3x3 has fewer than 5 rows per split; 512 is the fastest or within
// 5 % of it on all five.
constexpr int WGRAD_FULL = 256, WGRAD_MIN_NSEG = 128, WGRAD_MIN_SEGS = 8, WGRAD_MAX_SPLITS = 512;

int conv_wgrad_splits(int B, int OH, int Cin, int Cout, int KH, int KW) {
    const long tiles = (long)((Cout + 31) / 32) * (((long)Cin * KH * KW + 31) / 32), nseg = (long)B * OH;
    if (tiles >= WGRAD_FULL || nseg < WGRAD_MIN_NSEG) return 1;
    const long s = std::min(nseg / WGRAD_MIN_SEGS, (long)WGRAD_MAX_SPLITS);
    return (int)std::max(s, 1L);
}

static size_t conv_g_floats(const ConvTrainArgs& t) { return (size_t)t.B * t.OH * t.OW * t.Cout; }

// G, and behind it the partial weight gradients of a product in S splits
size_t conv_bwd_ws_floats(const ConvTrainArgs& t, int S) {
    return conv_g_floats(t) + (S > 1 ? (size_t)S * t.Cout * t.Cin * t.KH * t.KW : 0);
}
size_t conv_fwd_ws_floats(const ConvTrainArgs& t) { return (size_t)t.Cout * t.Cin * t.KH * t.KW; }

int launch_conv_train_forward(const ConvTrainArgs& t, const float* residual, int relu, float* y, float* ws, const LaunchCtx& ctx) {
    {
        const size_t count = conv_fwd_ws_floats(t);
        ProfScope ps(ctx, "conv_train_fwd_wt", 0.0, 8.0 * count);
        hipLaunchKernelGGL(conv_wt_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx.stream, t.w, ws, t.Cout, t.Cin, t.KH * t.KW);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    ConvGemmArgs g = base_args(t);
    g.A = t.x; g.Bm = ws; g.scale = t.scale; g.shift = t.shift; g.res = residual; g.relu = relu;
    g.C = y; g.ldc = t.Cout;
    g.M = t.B * t.OH * t.OW; g.N = t.Cout; g.nseg = t.KH * t.KW; g.Kc = t.Cin;
    if (t.KH == 7) {
        g.nseg = t.KH; g.Kc = t.KW * t.Cin;
        return launch_gemm<0, true>("conv_train_fwd_gemm", g, ctx);
    }
    return launch_gemm<0>("conv_train_fwd_gemm", g, ctx);
}

int launch_conv_backward(const ConvTrainArgs& t, const float* y, int relu, const float* g_y, const float* g_x_add, float* g_x, float* g_w,
                         float* g_res, float* ws, int S, const LaunchCtx& ctx) {
    const size_t count = conv_g_floats(t);
    float* const G = (g_x || g_w) ? ws : nullptr;
    {
        ProfScope ps(ctx, "conv_bwd_prep", 2.0 * count, 4.0 * 4 * count);
        hipLaunchKernelGGL(conv_bwd_prep_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx.stream, g_y, y, t.scale, relu, count,
                           t.Cout, G, g_res);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    if (g_x) {
        ConvGemmArgs g = base_args(t);
        g.A = G; g.Bm = t.w; g.res = g_x_add; g.C = g_x; g.ldc = t.Cin;
        g.M = t.B * t.H * t.W; g.N = t.Cin; g.nseg = t.KH * t.KW; g.Kc = t.Cout;
        if (const int rc = launch_gemm<1>("conv_bwd_dgrad_gemm", g, ctx)) return rc;
    }
    if (g_w) {
        ConvGemmArgs g = base_args(t);
        g.A = G; g.Bm = t.x; g.C = g_w; g.ldc = (long)t.Cin * t.KH * t.KW;
        g.M = t.Cout; g.N = t.Cin * t.KH * t.KW; g.nseg = t.B * t.OH; g.Kc = t.OW;
        g.S = S;
        g.part = ws + count;
        if (const int rc = g.S > 1 ? launch_gemm<2, true>("conv_bwd_wgrad_gemm", g, ctx) : launch_gemm<2>("conv_bwd_wgrad_gemm", g, ctx)) return rc;
        if (g.S > 1) {
            const size_t n = (size_t)g.M * g.N;
            ProfScope ps(ctx, "conv_bwd_wgrad_reduce", (double)(g.S - 1) * n, 4.0 * (g.S + 1) * n);
            hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx.stream, g.part, g_w, (unsigned)n, g.S);
            if (const int rc = (int)hipGetLastError()) return rc;
        }
    }
    return 0;
}

}  // namespace specmi
