// conv_f16.hip - the fp16 trunk path (handle precision SPECMI_PRECISION_FP16, the reference's TRAINING.USE_AMP switch:
// scripts/spec_eval.py:63-70 runs the model under Lightning precision=16).  Numeric contract: DESIGN.md, "fp16 trunk".
//
//   * conv_f16_kernel     : every ResNet trunk convolution (stem 7x7, 1x1, 3x3 at stride 1 / 2, downsample, the folded
//                           [conv3 | downsample] GEMM) as ONE implicit GEMM over fp16 NHWC activations on
//                           v_mfma_f32_32x32x16_f16 (fp16 x fp16 products, fp32 accumulation).  The BatchNorm scale is folded
//                           into the fp16 weights at commit; the epilogue runs in fp32: acc + shift (+ fp16 residual), ReLU,
//                           then a round-to-nearest-even fp16 store (or an fp32 store: the last layer of layer4).
//   * to_nhwc_f16_kernel  : the normalised fp32 NCHW image -> fp16 NHWC, channels zero padded to 8 (the stem's K octet).
//   * maxpool_f16_kernel  : MaxPool2d(3, 2, 1) on fp16 NHWC (exact: a max of fp16 values is one of them).
//
// A separate file rather than a template over conv_bf16s.hip's tile body: that body splits fp32 A quads into bf16 pieces on
// the way to LDS and walks K in 16-deep stages of 16-channel taps; here A arrives as fp16 octets, a stage is 32 deep and a
// K octet may belong to any tap (the Cin = 8 stem), so a shared body would branch on its caller at every step.
//
// Mapping (CDNA4, wave64): workgroup = 128 rows x BN (128 or 64) columns, 4 waves as 2 x 2, a wave owns 64 x BN/2 (2 x BN/64
// tiles of 32 x 32).  K (ordered (ky, kx, ci), ci over the padded channels) advances in stages of 32 = 4 octets of 8 fp16.
//   * A: every thread loads one 16-byte octet of two rows per stage (buffer loads; taps outside the image, rows past M and
//     octets past K read 0 through an out-of-range offset) and writes it to LDS as [octet][row][8 fp16] - the 32x32x16
//     A-fragment image (lane = row, octet = k half); the octet planes are padded by 64 bytes so that the 4 octets of a row
//     land in different banks.
//   * B: packed at commit as [Kp/8][Npad][8] fp16: a stage is a linear 16-byte-per-lane copy into LDS in fragment order.
//   * double-buffered stages, one barrier per stage; the global loads of stage s+1 are issued before the MFMAs of stage s.
//   * the k-sum order of an output is fixed by the layer's shape (serial over the stages): an image's bits do not depend on
//     the batch, the tile it lands in or the launch it is part of.
//   * epilogue as in conv_bf16s.hip: accumulators transposed through LDS (two passes of 64 rows), row-contiguous stores.
#include <cmath>
#include <cstring>

#include "conv_igemm_tile.h"

namespace specmi {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct HArgs {
    const void* x;          // fp16 NHWC, pixel stride ldx (multiple of 8)
    const void* w;          // fp16 [Kp/8][Npad][8]
    const float* shift;
    const void* res;        // fp16, indexed like out (ldo)
    void* out;              // fp16 or fp32 [M][ldo]
    unsigned x_bytes, w_bytes;
    int ldx, Cout, Npad, ldo, M, nbn, nsteps, relu;
    // implicit GEMM: octet o of K = (tap o / cpo, channels 8 (o % cpo) ..); taps >= ntaps are K padding
    int H, W, KH, KW, stride, pad, cpo, ntaps, OW, OHW;
    // optional second A source (the folded downsample): stages >= nsteps1 read x2 at pixel (b, oy * stride2, ox * stride2)
    const void* x2;
    unsigned x2_bytes;
    int nsteps1, ldx2, H2, W2, stride2;
};

template <int BN, bool DUAL, bool OUT32>
__global__ void __launch_bounds__(256) conv_f16_kernel(const HArgs p) {
    static_assert(BN == 128 || BN == 64, "");
    constexpr int BM = 128;
    constexpr int TN = BN / 64;
    constexpr int APL = BM * 16 + 64;             // bytes per A octet plane (padded)
    constexpr int BPL = BN * 16;
    constexpr int STAGE = 4 * APL + 4 * BPL;
    constexpr int NB = BN / 64;                   // B loads per thread per stage
    extern __shared__ __attribute__((aligned(16))) char smem_h[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hh = lane >> 5;

    const int L = xcd_tile_order(blockIdx.x, gridDim.x);
    const int tile_m = L / p.nbn, tile_n = L - tile_m * p.nbn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t x2rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(DUAL ? p.x2 : p.x), 0, DUAL ? p.x2_bytes : p.x_bytes, 0x00020000);

    // ---- loader coordinates ------------------------------------------------------------------------------------------
    const int a_q = tid & 3, a_r = tid >> 2;      // octet of the stage, row (and row + 64)
    int a_base[2], a_iy[2], a_ix[2];
    unsigned a_voff2[DUAL ? 2 : 1];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + a_r + 64 * i;
        const int mm = m < p.M ? m : 0;
        const int b_ = mm / p.OHW, rem = mm - b_ * p.OHW, oy = rem / p.OW, ox = rem - oy * p.OW;
        const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
        a_iy[i] = m < p.M ? iy0 : -(1 << 20);     // rows past M: every tap out of the image
        a_ix[i] = ix0;
        a_base[i] = ((b_ * p.H + iy0) * p.W + ix0) * p.ldx * 2;   // bytes of tap (0, 0) (may be negative: only valid taps add up)
        if (DUAL) {
            const int pix2 = (b_ * p.H2 + oy * p.stride2) * p.W2 + ox * p.stride2;
            a_voff2[i] = m < p.M ? (unsigned)(pix2 * p.ldx2 * 2) : kOutOfRange;
        }
    }
    const unsigned a_lds = (unsigned)(a_q * APL + a_r * 16);      // + 64 rows: + 1024
    const int b_oct = tid / BN, b_n = tid % BN;                    // (+ 256 / BN octets per further load)

    u32x4 ra[2], rb[NB];
    auto load_stage = [&](int s) {
        const bool second = DUAL && s >= p.nsteps1;       // wave-uniform
        if (second) {
            const unsigned c = (unsigned)(((s - p.nsteps1) * 4 + a_q) * 16);
#pragma unroll
            for (int i = 0; i < 2; ++i)
                ra[i] = __builtin_amdgcn_raw_buffer_load_b128(x2rs, a_voff2[DUAL ? i : 0] == kOutOfRange ? kOutOfRange : a_voff2[DUAL ? i : 0] + c, 0, 0);
        } else {
            const int o = s * 4 + a_q;
            const int tap = o / p.cpo, c8 = o - tap * p.cpo;
            const int ky = tap / p.KW, kx = tap - ky * p.KW;
            const int toff = ((ky * p.W + kx) * p.ldx + c8 * 8) * 2;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool ok = tap < p.ntaps && (unsigned)(a_iy[i] + ky) < (unsigned)p.H && (unsigned)(a_ix[i] + kx) < (unsigned)p.W;
                ra[i] = __builtin_amdgcn_raw_buffer_load_b128(xrs, ok ? (unsigned)(a_base[i] + toff) : kOutOfRange, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j)
            rb[j] = __builtin_amdgcn_raw_buffer_load_b128(wrs, (unsigned)(((s * 4 + b_oct + j * (256 / BN)) * p.Npad + n0 + b_n) * 16), 0, 0);
    };
    auto store_stage = [&](int buf) {
        char* const A = smem_h + buf * STAGE;
        char* const Bs = A + 4 * APL;
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(A + a_lds + i * 1024) = ra[i];
#pragma unroll
        for (int j = 0; j < NB; ++j) *reinterpret_cast<u32x4*>(Bs + (b_oct + j * (256 / BN)) * BPL + b_n * 16) = rb[j];
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const unsigned fa_off = (unsigned)(hh * APL + (wm * 64 + l31) * 16);
    const unsigned fb_off = (unsigned)(hh * BPL + (wn * (BN / 2) + l31) * 16);

    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (int s = 0; s < p.nsteps; ++s) {
        const int buf = s & 1;
        const bool more = s + 1 < p.nsteps;
        if (more) load_stage(s + 1);
        const char* const A = smem_h + buf * STAGE;
        const char* const Bs = A + 4 * APL;
#pragma unroll
        for (int t = 0; t < 2; ++t) {        // two k halves of 16: octets 2t + hh
            f16x8 fa[2], fb[TN];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const f16x8*>(A + 2 * t * APL + fa_off + i * 512);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const f16x8*>(Bs + 2 * t * BPL + fb_off + j * 512);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_stage(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: two passes of 64 rows through LDS -> row-contiguous traffic ------------------------------------------
    constexpr int LDC = BN + 4;
    constexpr int QPR = BN / 4, RPP = 256 / QPR, NPASS = 64 / RPP;
    float* const Cs = reinterpret_cast<float*>(smem_h);
    const int cq = tid % QPR, r0 = tid / QPR;
    const int n = n0 + cq * 4;
    const bool col_ok = n < p.Cout;                  // Cout % 4 == 0 (checked by the launcher): a quad is all in or all out
    f32x4 sh = {0.f, 0.f, 0.f, 0.f};
    if (col_ok) sh = *reinterpret_cast<const f32x4*>(p.shift + n);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) __syncthreads();
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                        Cs[row * LDC + wn * (BN / 2) + j * 32 + l31] = acc[i][j][r];
                    }
        }
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int row = r0 + ps * RPP;
            const int m = m0 + pass * 64 + row;
            if (m < p.M && col_ok) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(Cs + row * LDC + cq * 4);
                const size_t o = (size_t)m * p.ldo + n;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = a[e] + sh[e];
                if (p.res) {
                    const f16x4 rr = *reinterpret_cast<const f16x4*>(static_cast<const _Float16*>(p.res) + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += (float)rr[e];
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if (OUT32) {
                    *reinterpret_cast<f32x4*>(static_cast<float*>(p.out) + o) = v;
                } else {
                    f16x4 hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = (_Float16)v[e];      // round to nearest even
                    *reinterpret_cast<f16x4*>(static_cast<_Float16*>(p.out) + o) = hv;
                }
            }
        }
    }
}

// ---- host: packing ---------------------------------------------------------------------------------------------------
// round-to-nearest-even double -> IEEE binary16 bits (subnormals, overflow to inf)
static unsigned short half_bits(double v) {
    unsigned short sign = std::signbit(v) ? 0x8000 : 0;
    double a = std::fabs(v);
    if (std::isnan(v)) return 0x7e00;
    if (a >= 65520.0) return sign | 0x7c00;                       // rounds to inf
    if (a < std::ldexp(1.0, -14)) {                                // subnormal: multiples of 2^-24
        const double q = std::nearbyint(a * 16777216.0);           // default rounding mode: to nearest even
        return sign | (unsigned short)q;
    }
    int e;
    const double f = std::frexp(a, &e);                            // a = f 2^e, f in [0.5, 1)
    double mant = std::nearbyint(std::ldexp(f, 11));               // 11 significant bits, in [1024, 2048]
    if (mant >= 2048.0) { mant /= 2; ++e; }
    const int E = e - 1 + 15;                                      // biased exponent of 1.xxx 2^(e-1)
    if (E >= 31) return sign | 0x7c00;
    return sign | (unsigned short)((E << 10) | ((int)mant - 1024));
}

// (cout, K) row-major fp64 products -> fp16 [Kp/8][Npad][8]; returns the first (n, k) whose product overflows fp16, or -1
long pack_f16_weights(const std::vector<double>& wk, int cout, int K, int Kp, int Npad, std::vector<unsigned short>& out) {
    out.assign((size_t)Kp * Npad, 0);
    for (int n = 0; n < cout; ++n)
        for (int k = 0; k < K; ++k) {
            const unsigned short h = half_bits(wk[(size_t)n * K + k]);
            if ((h & 0x7c00) == 0x7c00) return (long)n * K + k;
            out[((size_t)(k / 8) * Npad + n) * 8 + (k % 8)] = h;
        }
    return -1;
}

// OIHW fp32 weights x per-output-channel scale (fp64 products) -> K ordered (ky, kx, ci) over ci_p >= cin channels (zeros)
void fold_f16_oihw(const float* w, const float* scale, int cout, int cin, int cin_p, int kh, int kw, std::vector<double>& wk) {
    const int K = cin_p * kh * kw;
    wk.assign((size_t)cout * K, 0.0);
    for (int n = 0; n < cout; ++n)
        for (int ci = 0; ci < cin; ++ci)
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx)
                    wk[(size_t)n * K + (ky * kw + kx) * cin_p + ci] =
                        (double)w[(((size_t)n * cin + ci) * kh + ky) * kw + kx] * (double)scale[n];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static bool conv_f16_shape_ok(const ConvF16Args& a) {
    if (a.B <= 0 || a.Cin <= 0 || a.ldx % 8 || a.ldx < a.Cin || a.Cout % 4 || a.ldo % 4 || a.ldo < a.Cout || a.Npad % 64 ||
        a.Npad < a.Cout || a.KH < 1 || a.KW < 1 || a.stride < 1 || a.pad < 0 || a.Kp % 32 ||
        a.OH != (a.H + 2 * a.pad - a.KH) / a.stride + 1 || a.OW != (a.W + 2 * a.pad - a.KW) / a.stride + 1 || a.OH < 1 || a.OW < 1)
        return false;
    if ((reinterpret_cast<uintptr_t>(a.x) & 15) || (reinterpret_cast<uintptr_t>(a.out) & 15) || (reinterpret_cast<uintptr_t>(a.w) & 15) ||
        (a.res && (reinterpret_cast<uintptr_t>(a.res) & 7)) || (reinterpret_cast<uintptr_t>(a.shift) & 15))
        return false;
    if (a.x2) {
        if (a.KH != 1 || a.KW != 1 || a.stride != 1 || a.pad != 0 || a.Cin % 32 || a.ldx != a.Cin || a.Cin2 % 32 || a.ldx2 % 8 ||
            a.stride2 < 1 || (a.OH - 1) * a.stride2 >= a.H2 || (a.OW - 1) * a.stride2 >= a.W2 || (reinterpret_cast<uintptr_t>(a.x2) & 15) ||
            a.Kp != a.Cin + a.Cin2)
            return false;
    } else if (a.Kp != ((a.KH * a.KW * a.ldx + 31) / 32) * 32) {
        return false;
    }
    return (size_t)a.Kp * a.Npad * 2 < ((size_t)1 << 31);
}

template <int BN, bool DUAL, bool OUT32>
static int f16_launch(HArgs k, const LaunchCtx& ctx, double flops, double bytes) {
    constexpr int stage = 4 * (128 * 16 + 64) + 4 * BN * 16;
    constexpr int cs = 64 * (BN + 4) * 4;
    constexpr int smem = 2 * stage > cs ? 2 * stage : cs;
    static DevOnce once;
    if (int e = set_dyn_lds_once(once, reinterpret_cast<const void*>(&conv_f16_kernel<BN, DUAL, OUT32>), smem)) return e;
    k.nbn = BN == 64 ? (k.Cout + 63) / 64 : k.Npad / 128;
    const int grid = ((k.M + 127) / 128) * k.nbn;
    ProfScope ps(ctx, DUAL ? (BN == 128 ? "conv_f16<128x128,2src>" : "conv_f16<128x64,2src>")
                      : OUT32 ? (BN == 128 ? "conv_f16<128x128,f32 out>" : "conv_f16<128x64,f32 out>")
                              : (BN == 128 ? "conv_f16<128x128>" : "conv_f16<128x64>"),
                 flops, bytes);
    hipLaunchKernelGGL((conv_f16_kernel<BN, DUAL, OUT32>), dim3(grid), dim3(256), smem, ctx.stream, k);
    return (int)hipGetLastError();
}

int launch_conv_f16(const ConvF16Args& a, const LaunchCtx& ctx) {
    if (!conv_f16_shape_ok(a)) return (int)hipErrorInvalidValue;
    const size_t ximg = (size_t)a.H * a.W * a.ldx * 2, x2img = a.x2 ? (size_t)a.H2 * a.W2 * a.ldx2 * 2 : 0;
    const size_t img = ximg > x2img ? ximg : x2img;
    // buffer offsets are 32-bit: the batch is cut into launches of whole images (an image's k order does not depend on it)
    const int per = (int)((((size_t)1 << 31) - 1) / img);
    if (per < 1) return (int)hipErrorInvalidValue;
    const size_t oimg = (size_t)a.OH * a.OW * a.ldo, osz = a.out_f32 ? 4 : 2;
    const bool wide = a.Npad % 128 == 0;
    for (int b0 = 0; b0 < a.B; b0 += per) {
        const int nb = a.B - b0 < per ? a.B - b0 : per;
        HArgs k;
        k.x = static_cast<const char*>(a.x) + b0 * ximg;
        k.w = a.w; k.shift = a.shift;
        k.res = a.res ? static_cast<const char*>(a.res) + b0 * oimg * 2 : nullptr;
        k.out = static_cast<char*>(a.out) + b0 * oimg * osz;
        k.x_bytes = (unsigned)(nb * ximg);
        k.w_bytes = (unsigned)((size_t)a.Kp * a.Npad * 2);
        k.ldx = a.ldx; k.Cout = a.Cout; k.Npad = a.Npad; k.ldo = a.ldo; k.M = nb * a.OH * a.OW; k.nbn = 0;
        k.nsteps = a.Kp / 32; k.relu = a.relu;
        k.H = a.H; k.W = a.W; k.KH = a.KH; k.KW = a.KW; k.stride = a.stride; k.pad = a.pad; k.cpo = a.ldx / 8;
        k.ntaps = a.KH * a.KW; k.OW = a.OW; k.OHW = a.OH * a.OW;
        k.x2 = a.x2 ? static_cast<const char*>(a.x2) + b0 * x2img : nullptr;
        k.x2_bytes = a.x2 ? (unsigned)(nb * x2img) : 0;
        k.nsteps1 = a.x2 ? a.Cin / 32 : k.nsteps; k.ldx2 = a.ldx2; k.H2 = a.H2; k.W2 = a.W2; k.stride2 = a.stride2;
        const int K = a.x2 ? a.Cin + a.Cin2 : a.KH * a.KW * a.Cin;
        const double flops = 2.0 * k.M * (double)a.Cout * K;
        const double bytes = 2.0 * ((double)nb * a.H * a.W * a.Cin + (a.x2 ? (double)nb * a.H2 * a.W2 * a.Cin2 : 0.0) +
                                    (double)k.M * a.Cout * (a.res ? 1.0 : 0.0) + (double)K * a.Cout) +
                             (double)k.M * a.Cout * (double)osz;
        int rc;
        if (a.x2) {
            if (a.out_f32) return (int)hipErrorInvalidValue;
            rc = wide ? f16_launch<128, true, false>(k, ctx, flops, bytes) : f16_launch<64, true, false>(k, ctx, flops, bytes);
        } else if (a.out_f32) {
            rc = wide ? f16_launch<128, false, true>(k, ctx, flops, bytes) : f16_launch<64, false, true>(k, ctx, flops, bytes);
        } else {
            rc = wide ? f16_launch<128, false, false>(k, ctx, flops, bytes) : f16_launch<64, false, false>(k, ctx, flops, bytes);
        }
        if (rc) return rc;
    }
    return 0;
}

// ---- image -> fp16 NHWC (channels padded to 8) ------------------------------------------------------------------------
__global__ void __launch_bounds__(256) to_nhwc_f16_kernel(const float* __restrict__ x, _Float16* __restrict__ out, int C, unsigned HW,
                                                          unsigned total) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned b = i / HW, px = i - b * HW;
    const float* src = x + (size_t)b * C * HW + px;
    f16x8 v;
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < C ? (_Float16)src[(size_t)c * HW] : (_Float16)0.f;
    *reinterpret_cast<f16x8*>(out + (size_t)i * 8) = v;
}

int launch_to_nhwc_f16(const float* x, void* out, int B, int C, int H, int W, const LaunchCtx& ctx) {
    if (C < 1 || C > 8 || (reinterpret_cast<uintptr_t>(out) & 15)) return (int)hipErrorInvalidValue;
    const long total = (long)B * H * W;
    if (total >= (1L << 32) - 256) return (int)hipErrorInvalidValue;
    ProfScope ps(ctx, "to_nhwc_f16", 0.0, (double)total * (4.0 * C + 16.0));
    hipLaunchKernelGGL(to_nhwc_f16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx.stream, x,
                       static_cast<_Float16*>(out), C, (unsigned)(H * W), (unsigned)total);
    return (int)hipGetLastError();
}

// ---- MaxPool2d(3, 2, 1) on fp16 NHWC: one thread per (output pixel, 8 channels) -----------------------------------------
__global__ void __launch_bounds__(256) maxpool_f16_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ out, int H, int W, int C8,
                                                          int OH, int OW, unsigned total) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned c8 = i % (unsigned)C8;
    unsigned pix = i / (unsigned)C8;
    const int ox = (int)(pix % (unsigned)OW); pix /= (unsigned)OW;
    const int oy = (int)(pix % (unsigned)OH);
    const unsigned b = pix / (unsigned)OH;
    const f16x8* img = reinterpret_cast<const f16x8*>(x) + (size_t)b * H * W * C8 + c8;
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = min(max(oy * 2 - 1 + ky, 0), H - 1);     // clamped: a repeated edge pixel does not change the max
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = min(max(ox * 2 - 1 + kx, 0), W - 1);
            const f16x8 v = img[(size_t)(iy * W + ix) * C8];
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)v[e]);
        }
    }
    f16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (_Float16)m[e];           // exact: m is one of the fp16 inputs
    reinterpret_cast<f16x8*>(out)[i] = r;
}

int launch_maxpool_f16(const void* x, void* out, int B, int H, int W, int C, int OH, int OW, const LaunchCtx& ctx) {
    if (C % 8 || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return (int)hipErrorInvalidValue;
    const long total = (long)B * OH * OW * (C / 8);
    if (total >= (1L << 32) - 256) return (int)hipErrorInvalidValue;
    ProfScope ps(ctx, "maxpool_f16", 0.0, 2.0 * ((double)B * H * W * C + (double)B * OH * OW * C));
    hipLaunchKernelGGL(maxpool_f16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx.stream, static_cast<const _Float16*>(x),
                       static_cast<_Float16*>(out), H, W, C / 8, OH, OW, (unsigned)total);
    return (int)hipGetLastError();
}

}  // namespace specmi
