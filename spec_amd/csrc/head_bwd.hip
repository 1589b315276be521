// head_bwd.hip - pare's HMRHead regressor for training: its forward with dropout and a tape, and its backward (gfx950); at the end
// of the file CamCalib's three FC heads for training on the same product, three heads per launch (head_gemm_group_kernel).
//
// The loop (oracle/heads.py:80-125; H = 1024, S = 157, Kin = F + S + C, C = 7 with use_cam_feats else 0):
//     xc_t = [xf | state_t | c],  a1_t = drop1(fc1(xc_t)),  a2_t = drop2(fc2(a1_t)),  state_{t+1} = state_t + dec(a2_t)
// Dropout, stated once: a = h * (m ? s : 0) with s = float32(1 / (1 - p)); the masks are uint8 (2 n_iter, B, 1024) ordered
// (t, layer), drawn by the caller.  A null mask pointer is eval mode: no multiply, s is not read.
//
// Every product runs on ONE kernel, head_gemm_kernel: C(m, n) = sum_k A(m, k) B(k, n) with both operands addressed by two
// strides, so the three orientations read torch's row-major tensors where they lie - the optimiser rewrites the weights every
// step, nothing is packed, uploaded or committed:
//     forward          Y  = X W^T + b    A = X  (ld, 1)   B = W  (1, ld)    contraction over the input features
//     data gradient    dX = dY W         A = dY (ld, 1)   B = W  (ld, 1)    contraction over the output features
//     weight gradient  dW = dY^T X       A = dY (1, ld)   B = X  (ld, 1)    contraction over the rows (t, b)
// A workgroup owns one 32 x 32 tile of C; its four waves take the k groups of 8 round robin (wave w: groups w, w + 4, ...) on
// v_mfma_f32_32x32x2_f32 - exact fp32, a k-ordered fma chain - and wave 0 adds the other three accumulators in wave order
// through LDS.  Lane l of a wave feeds row / column l % 32 with k = 8 g + 4 (l / 32) + j in step j of group g.  Elements
// past M, N or K are loaded from a clamped address and replaced by zero, so any size and any leading dimension works and no
// load or store leaves the tensors.  Epilogue: v = acc (+ bias[n]) (+ res[m][n]), then v = mask[m][n] ? v * s : 0.
//
// Determinism (the rule of smpl_bwd.hip): no float atomics; the order of every sum is fixed by the shapes - the split of k
// among the four waves never looks at the batch - so two runs give the same bits, row b of state_n and of g_xf has the same
// bits in any batch, and the weight gradients (sums over the n_iter B stacked rows in (t, b) order) depend on B alone.
//
// Forward (launch_head_train_forward): X1 = xf W1[:, :F]^T + b1 (+ c W1[:, F+S:]^T) once, then per iteration
// a1_t = drop1(X1 + state_t W1[:, F:F+S]^T), a2_t = drop2(a1_t W2^T + b2) and the three decoders with the residual.  The tape
// (head_tape_floats) keeps State (n B, 157) | A1 (n B, 1024) | A2 (n B, 1024), rows in (t, b) order: the weight gradients read
// them as stacked operands.
// Backward (launch_head_backward), t = n-1 .. 0 from G_state[n-1] = g_state_n:
//     G_h2[t] = (G_state[t] Wdec) * m2_t s,  G_h1[t] = (G_h2[t] W2) * m1_t s,  G_state[t-1] = G_state[t] + G_h1[t] W1[:, F:F+S]
// (the contraction over the 157 decoder rows runs pose, shape, cam, one launch each onto the same output), then one product per
// wanted gradient: dWdec = G_state^T A2, dW2 = G_h2^T A1, dW1[:, F:F+S] = G_h1^T State and, with Sigma = sum_t G_h1[t] in t order,
// dW1[:, :F] = Sigma^T xf, dW1[:, F+S:] = Sigma^T c, g_xf = Sigma W1[:, :F]; the bias gradients are the column sums of the
// stacked gradients, eight interleaved row slices each in row order, then the slices in order.
#include "specmi_internal.h"

namespace specmi {

namespace {

constexpr int H = 1024, S = 157;
constexpr int KU = 4;      // k groups of 8 a wave loads before it multiplies

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GemmArgs {
    const float* A; long sam, sak;     // A(m, k) = A[m sam + k sak]
    const float* Bm; long sbk, sbn;    // B(k, n) = Bm[k sbk + n sbn]
    const float* bias;                 // [n], or null
    const float* res; long ldr;        // [m ldr + n], or null; may be C itself (an element is read and written by one lane)
    const uint8_t* mask; long ldm;     // [m ldm + n], or null
    float scale;
    float* C; long ldc;
    int M, N, K;
};

// the tile body, stated once for the single launch and the grouped one (blockIdx.z picks the argument block there)
__device__ __forceinline__ void head_gemm_tile(const GemmArgs& a) {
    __shared__ float part[3][16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const bool mok = m0 + c < a.M, nok = n0 + c < a.N;
    const float* const ap = a.A + (size_t)(mok ? m0 + c : 0) * a.sam;
    const float* const bp = a.Bm + (size_t)(nok ? n0 + c : 0) * a.sbn;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // KU of the wave's k groups per trip: their 8 KU loads are in flight together - the launches are latency bound at these
    // shapes (a group past K adds exact zeros)
    for (int kg = w * 8; kg < a.K; kg += 32 * KU) {      // (the trip count is the wave's: every lane is in every MFMA)
        float av[KU][4], bv[KU][4];
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kj = kg + 32 * u + 4 * h + j;
                const bool kok = kj < a.K;
                const size_t k = kok ? kj : 0;
                const float x = ap[k * a.sak], y = bp[k * a.sbk];
                av[u][j] = (kok && mok) ? x : 0.f;
                bv[u][j] = (kok && nok) ? y : 0.f;
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
    const int n = n0 + c;
    if (n >= a.N) return;
    const float bias = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + 4 * h + (r & 3) + 8 * (r >> 2);
        if (m >= a.M) continue;
        float v = acc[r] + bias;
        if (a.res) v += a.res[(size_t)m * a.ldr + n];
        if (a.mask) v = a.mask[(size_t)m * a.ldm + n] ? v * a.scale : 0.f;
        a.C[(size_t)m * a.ldc + n] = v;
    }
}

__global__ void __launch_bounds__(256) head_gemm_kernel(const GemmArgs a) { head_gemm_tile(a); }

// Up to three products of ONE shape (M, N, K) in one launch: the grid's z picks the argument block, everything else is
// head_gemm_kernel's - the same split of k among the four waves, the same wave-order sum - so a product's bits do not depend on
// whether, or with what, it was grouped
struct GemmGroup { GemmArgs g[3]; };
__global__ void __launch_bounds__(256) head_gemm_group_kernel(const GemmGroup a) { head_gemm_tile(a.g[blockIdx.z]); }

// out[n] = sum over the R rows of G[r ld + n]; the n columns are cut into up to three outputs at end[0..2].  A workgroup owns 32
// columns; slice j of 8 adds rows j, j + 8, ... in order and slice 0 adds the eight partial sums in slice order: fixed by R alone
struct ColSumArgs { const float* G; long ld; int R, N; float* out[3]; int end[3]; };
__global__ void __launch_bounds__(256) head_colsum_kernel(const ColSumArgs a) {
    __shared__ float part[8][32];
    const int c = threadIdx.x & 31, j = threadIdx.x >> 5, n = blockIdx.x * 32 + c;
    float s = 0.f;
    if (n < a.N)
        for (int r = j; r < a.R; r += 8) s += a.G[(size_t)r * a.ld + n];
    part[j][c] = s;
    __syncthreads();
    if (j || n >= a.N) return;
#pragma unroll
    for (int u = 1; u < 8; ++u) s += part[u][c];
    const int seg = n < a.end[0] ? 0 : n < a.end[1] ? 1 : 2;
    if (a.out[seg]) a.out[seg][n - (seg ? a.end[seg - 1] : 0)] = s;
}

// Sigma[i] = sum_t G[t count + i], t in order
__global__ void __launch_bounds__(256) head_sum_t_kernel(const float* __restrict__ G, float* __restrict__ out, size_t count, int n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float s = G[i];
    for (int t = 1; t < n; ++t) s += G[(size_t)t * count + i];
    out[i] = s;
}

struct Op { const float* p; long s0, s1; };                    // an operand and its two strides (row / column index of the product, k)
struct Epi { const float* bias; const float* res; long ldr; const uint8_t* mask; };

GemmArgs gemm_args(Op A, Op B, int M, int N, int K, Epi e, float scale, float* C, long ldc) {
    GemmArgs g;
    g.A = A.p; g.sam = A.s0; g.sak = A.s1;
    g.Bm = B.p; g.sbn = B.s0; g.sbk = B.s1;
    g.bias = e.bias; g.res = e.res; g.ldr = e.ldr; g.mask = e.mask; g.ldm = H; g.scale = scale;
    g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    return g;
}

int gemm(const char* name, Op A, Op B, int M, int N, int K, Epi e, float scale, float* C, long ldc, const LaunchCtx& ctx) {
    const GemmArgs g = gemm_args(A, B, M, N, K, e, scale, C, ldc);
    ProfScope ps(ctx, name, 2.0 * M * N * K, 4.0 * ((double)M * K + (double)K * N + (double)M * N));
    hipLaunchKernelGGL(head_gemm_kernel, dim3((N + 31) / 32, (M + 31) / 32), dim3(256), 0, ctx.stream, g);
    return (int)hipGetLastError();
}

// n (1 .. 3) products of one shape: one grouped launch, or - grouped == false, or n == 1 - n single ones; the same bits
int gemm_group(const char* name, const GemmArgs* g, int n, bool grouped, const LaunchCtx& ctx) {
    const int M = g[0].M, N = g[0].N, K = g[0].K;
    const dim3 grid((N + 31) / 32, (M + 31) / 32, 1);
    if (!grouped || n == 1) {
        for (int i = 0; i < n; ++i) {
            ProfScope ps(ctx, name, 2.0 * M * N * K, 4.0 * ((double)M * K + (double)K * N + (double)M * N));
            hipLaunchKernelGGL(head_gemm_kernel, grid, dim3(256), 0, ctx.stream, g[i]);
            if (const int rc = (int)hipGetLastError()) return rc;
        }
        return 0;
    }
    GemmGroup grp;
    for (int i = 0; i < 3; ++i) grp.g[i] = g[i < n ? i : 0];
    ProfScope ps(ctx, name, 2.0 * n * M * N * K, 4.0 * n * ((double)M * K + (double)K * N + (double)M * N));
    hipLaunchKernelGGL(head_gemm_group_kernel, dim3(grid.x, grid.y, n), dim3(256), 0, ctx.stream, grp);
    return (int)hipGetLastError();
}

int colsum(const float* G, long ld, int R, int N, float* o0, int e0, float* o1, int e1, float* o2, const LaunchCtx& ctx) {
    if (!o0 && !o1 && !o2) return 0;
    const ColSumArgs a{G, ld, R, N, {o0, o1, o2}, {e0, e1, N}};
    ProfScope ps(ctx, "head_bias_grad", (double)R * N, 4.0 * ((double)R * N + N));
    hipLaunchKernelGGL(head_colsum_kernel, dim3((N + 31) / 32), dim3(256), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

constexpr Epi NONE{nullptr, nullptr, 0, nullptr};

// the three decoders as one (157, 1024) matrix: rows [0, 144) pose, [144, 154) shape, [154, 157) cam
struct Dec { const float* w; const float* b; int off, n; };
void decoders(const HeadTrainParams& p, Dec d[3]) {
    d[0] = Dec{p.decpose_w, p.decpose_b, 0, 144};
    d[1] = Dec{p.decshape_w, p.decshape_b, 144, 10};
    d[2] = Dec{p.deccam_w, p.deccam_b, 154, 3};
}

#define TRY(x) do { if (int rc__ = (x)) return rc__; } while (0)

}  // namespace

size_t head_tape_floats(int B, int n_iter) { return (size_t)n_iter * B * (S + 2 * H); }
size_t head_train_fwd_ws_floats(int B) { return (size_t)B * H; }
size_t head_train_bwd_ws_floats(int B, int n_iter) { return (size_t)n_iter * B * (S + 2 * H) + (size_t)B * H; }

int launch_head_train_forward(const HeadTrainArgs& a, const float* init_state, float* state, float* tape, float* ws,
                              const LaunchCtx& ctx) {
    const int B = a.B, F = a.F, n = a.n_iter;
    const long Kin = F + S + a.C;
    const HeadTrainParams& p = a.p;
    float* const State = tape;
    float* const A1 = State + (size_t)n * B * S;
    float* const A2 = A1 + (size_t)n * B * H;
    float* const X1 = ws;
    Dec dec[3];
    decoders(p, dec);
    TRY(gemm("head_train_fwd_gemm", Op{a.xf, a.ld_xf, 1}, Op{p.fc1_w, Kin, 1}, B, H, F, Epi{p.fc1_b, nullptr, 0, nullptr}, 0.f, X1, H, ctx));
    if (a.C)
        TRY(gemm("head_train_fwd_gemm", Op{a.cam_feats, a.C, 1}, Op{p.fc1_w + F + S, Kin, 1}, B, H, a.C, Epi{nullptr, X1, H, nullptr}, 0.f, X1, H, ctx));
    TRY((int)hipMemcpyAsync(State, init_state, (size_t)B * S * 4, hipMemcpyDeviceToDevice, ctx.stream));
    for (int t = 0; t < n; ++t) {
        const float* const st = State + (size_t)t * B * S;
        float* const a1 = A1 + (size_t)t * B * H;
        float* const a2 = A2 + (size_t)t * B * H;
        float* const nxt = t == n - 1 ? state : State + (size_t)(t + 1) * B * S;
        const uint8_t* const m1 = a.masks ? a.masks + (size_t)(2 * t) * B * H : nullptr;
        const uint8_t* const m2 = a.masks ? a.masks + (size_t)(2 * t + 1) * B * H : nullptr;
        TRY(gemm("head_train_fwd_gemm", Op{st, S, 1}, Op{p.fc1_w + F, Kin, 1}, B, H, S, Epi{nullptr, X1, H, m1}, a.scale, a1, H, ctx));
        TRY(gemm("head_train_fwd_gemm", Op{a1, H, 1}, Op{p.fc2_w, H, 1}, B, H, H, Epi{p.fc2_b, nullptr, 0, m2}, a.scale, a2, H, ctx));
        for (const Dec& d : dec)
            TRY(gemm("head_train_fwd_gemm", Op{a2, H, 1}, Op{d.w, H, 1}, B, d.n, H, Epi{d.b, st + d.off, S, nullptr}, 0.f, nxt + d.off, S, ctx));
    }
    return 0;
}

int launch_head_backward(const HeadTrainArgs& a, const float* tape, const float* g_state, float* g_xf, const HeadTrainGrads& g,
                         float* ws, const LaunchCtx& ctx) {
    const int B = a.B, F = a.F, n = a.n_iter, R = n * B;
    const long Kin = F + S + a.C;
    const HeadTrainParams& p = a.p;
    const float* const State = tape;
    const float* const A1 = State + (size_t)R * S;
    const float* const A2 = A1 + (size_t)R * H;
    float* const Gs = ws;
    float* const Gh2 = Gs + (size_t)R * S;
    float* const Gh1 = Gh2 + (size_t)R * H;
    float* const Sigma = Gh1 + (size_t)R * H;
    Dec dec[3];
    decoders(p, dec);
    TRY((int)hipMemcpyAsync(Gs + (size_t)(n - 1) * B * S, g_state, (size_t)B * S * 4, hipMemcpyDeviceToDevice, ctx.stream));
    for (int t = n - 1; t >= 0; --t) {
        float* const gs = Gs + (size_t)t * B * S;
        float* const gh2 = Gh2 + (size_t)t * B * H;
        float* const gh1 = Gh1 + (size_t)t * B * H;
        const uint8_t* const m1 = a.masks ? a.masks + (size_t)(2 * t) * B * H : nullptr;
        const uint8_t* const m2 = a.masks ? a.masks + (size_t)(2 * t + 1) * B * H : nullptr;
        for (int i = 0; i < 3; ++i)
            TRY(gemm("head_bwd_dgrad_gemm", Op{gs + dec[i].off, S, 1}, Op{dec[i].w, 1, H}, B, H, dec[i].n,
                     Epi{nullptr, i ? gh2 : nullptr, H, i == 2 ? m2 : nullptr}, a.scale, gh2, H, ctx));
        TRY(gemm("head_bwd_dgrad_gemm", Op{gh2, H, 1}, Op{p.fc2_w, 1, H}, B, H, H, Epi{nullptr, nullptr, 0, m1}, a.scale, gh1, H, ctx));
        if (t > 0)
            TRY(gemm("head_bwd_dgrad_gemm", Op{gh1, H, 1}, Op{p.fc1_w + F, 1, Kin}, B, S, H, Epi{nullptr, gs, S, nullptr}, 0.f,
                     gs - (size_t)B * S, S, ctx));
    }
    const bool w1 = g.fc1_w != nullptr;
    if (g_xf || w1) {
        const size_t count = (size_t)B * H;
        ProfScope ps(ctx, "head_bwd_sum_t", (double)(n - 1) * count, 4.0 * (n + 1) * count);
        hipLaunchKernelGGL(head_sum_t_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx.stream, Gh1, Sigma, count, n);
        TRY((int)hipGetLastError());
    }
    if (g_xf) TRY(gemm("head_bwd_dgrad_gemm", Op{Sigma, H, 1}, Op{p.fc1_w, 1, Kin}, B, F, H, NONE, 0.f, g_xf, F, ctx));
    // weight gradients: A = the stacked gradient (n B, N) read as (N, n B), B = the stacked activation (n B, K)
    float* const dw[3] = {g.decpose_w, g.decshape_w, g.deccam_w};
    for (int i = 0; i < 3; ++i)
        if (dw[i]) TRY(gemm("head_bwd_wgrad_gemm", Op{Gs + dec[i].off, 1, S}, Op{A2, 1, H}, dec[i].n, H, R, NONE, 0.f, dw[i], H, ctx));
    if (g.fc2_w) TRY(gemm("head_bwd_wgrad_gemm", Op{Gh2, 1, H}, Op{A1, 1, H}, H, H, R, NONE, 0.f, g.fc2_w, H, ctx));
    if (w1) {
        TRY(gemm("head_bwd_wgrad_gemm", Op{Sigma, 1, H}, Op{a.xf, 1, a.ld_xf}, H, F, B, NONE, 0.f, g.fc1_w, Kin, ctx));
        TRY(gemm("head_bwd_wgrad_gemm", Op{Gh1, 1, H}, Op{State, 1, S}, H, S, R, NONE, 0.f, g.fc1_w + F, Kin, ctx));
        if (a.C) TRY(gemm("head_bwd_wgrad_gemm", Op{Sigma, 1, H}, Op{a.cam_feats, 1, a.C}, H, a.C, B, NONE, 0.f, g.fc1_w + F + S, Kin, ctx));
    }
    TRY(colsum(Gs, S, R, S, g.decpose_b, 144, g.decshape_b, 154, g.deccam_b, ctx));
    TRY(colsum(Gh2, H, R, H, g.fc2_b, H, nullptr, H, nullptr, ctx));
    TRY(colsum(Gh1, H, R, H, g.fc1_b, H, nullptr, H, nullptr, ctx));
    return 0;
}

// ---- CamCalib's three FC heads for training (camcalib/model.py:59-70) --------------------------------------------------------
// Head k (vfov, pitch, roll) is a chain of L = 1 .. 3 Linears with NO activation between them: A_0 = xf (B, F),
// A_l = A_{l-1} W_l^T + b_l, widths F -> Hc -> .. -> nbins.  The tape keeps A_1 .. A_{L-1} as (3, L - 1, B, Hc); the backward's
// workspace keeps the gradients of the same rows in the same layout.  G_L = g_logits, G_{l-1} = G_l W_l, dW_l = G_l^T A_{l-1},
// db_l = the column sums of G_l; g_xf = the sum over the heads of G_1 W_1, added in the order vfov, pitch, roll onto one output.
// Every step whose three heads are independent - each forward layer, each data gradient above layer 1, each weight gradient - is
// one grouped launch (gemm_group).
size_t cam_head_tape_floats(int B, int L, int Hc) { return (size_t)3 * (L - 1) * B * Hc; }
size_t cam_head_bwd_ws_floats(int B, int L, int Hc) { return cam_head_tape_floats(B, L, Hc); }

namespace {
inline int cam_in(const CamHeadArgs& a, int l) { return l == 0 ? a.F : a.Hc; }
inline int cam_out(const CamHeadArgs& a, int l) { return l == a.L - 1 ? a.nbins : a.Hc; }
// row (head k, layer l) of the tape / of the gradient workspace: the OUTPUT of layer l, l < L - 1
inline size_t cam_slot(const CamHeadArgs& a, int k, int l) { return ((size_t)k * (a.L - 1) + l) * a.B * a.Hc; }
}  // namespace

int launch_cam_head_train_forward(const CamHeadArgs& a, float* tape, float* logits, const LaunchCtx& ctx) {
    const int B = a.B, L = a.L;
    for (int l = 0; l < L; ++l) {
        const int K = cam_in(a, l), N = cam_out(a, l);
        GemmArgs g[3];
        for (int k = 0; k < 3; ++k) {
            const Op X = l == 0 ? Op{a.xf, a.ld_xf, 1} : Op{tape + cam_slot(a, k, l - 1), a.Hc, 1};
            float* const Y = l == L - 1 ? logits + (size_t)k * B * a.nbins : tape + cam_slot(a, k, l);
            g[k] = gemm_args(X, Op{a.p.w[k][l], K, 1}, B, N, K, Epi{a.p.b[k][l], nullptr, 0, nullptr}, 0.f, Y, N);
        }
        TRY(gemm_group("cam_head_fwd_gemm", g, 3, a.grouped, ctx));
    }
    return 0;
}

int launch_cam_head_backward(const CamHeadArgs& a, const float* tape, const float* g_logits, float* g_xf, const CamHeadGrads& gr,
                             float* ws, const LaunchCtx& ctx) {
    const int B = a.B, L = a.L;
    // G(k, l) = the gradient of layer l's output, (B, cam_out(l)) dense
    auto G = [&](int k, int l) -> const float* { return l == L - 1 ? g_logits + (size_t)k * B * a.nbins : ws + cam_slot(a, k, l); };
    bool below[3] = {false, false, false};       // is a gradient below layer l wanted (layers l' < l, or g_xf)
    {
        bool any = g_xf != nullptr;
        for (int l = 0; l < 3; ++l) {
            below[l] = any;
            for (int k = 0; k < 3; ++k) any = any || (l < L && (gr.w[k][l] || gr.b[k][l]));
        }
    }
    for (int l = L - 1; l >= 1 && below[l]; --l) {
        const int N = cam_in(a, l), K = cam_out(a, l);
        GemmArgs g[3];
        for (int k = 0; k < 3; ++k)
            g[k] = gemm_args(Op{G(k, l), K, 1}, Op{a.p.w[k][l], 1, N}, B, N, K, NONE, 0.f, ws + cam_slot(a, k, l - 1), N);
        TRY(gemm_group("cam_head_bwd_dgrad_gemm", g, 3, a.grouped, ctx));
    }
    if (g_xf) {
        const int K = cam_out(a, 0);
        for (int k = 0; k < 3; ++k)
            TRY(gemm("cam_head_bwd_dgrad_gemm", Op{G(k, 0), K, 1}, Op{a.p.w[k][0], 1, a.F}, B, a.F, K,
                     Epi{nullptr, k ? g_xf : nullptr, a.F, nullptr}, 0.f, g_xf, a.F, ctx));
    }
    for (int l = 0; l < L; ++l) {
        const int M = cam_out(a, l), N = cam_in(a, l);
        GemmArgs g[3];
        int n = 0;
        for (int k = 0; k < 3; ++k) {
            if (!gr.w[k][l]) continue;
            const Op X = l == 0 ? Op{a.xf, 1, a.ld_xf} : Op{tape + cam_slot(a, k, l - 1), 1, a.Hc};
            g[n++] = gemm_args(Op{G(k, l), 1, M}, X, M, N, B, NONE, 0.f, gr.w[k][l], N);
        }
        if (n) TRY(gemm_group("cam_head_bwd_wgrad_gemm", g, n, a.grouped, ctx));
        for (int k = 0; k < 3; ++k) TRY(colsum(G(k, l), M, B, M, gr.b[k][l], M, nullptr, M, nullptr, ctx));
    }
    return 0;
}

}  // namespace specmi
