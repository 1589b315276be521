// color_jitter.hip - torchvision's ColorJitter on the uint8 RGB frames of a ragged slab, on the device (DESIGN.md section 7 row
// f-21): the one step in which CameraRegressorDataset(is_train=True) differs from its validation half (camcalib/pano_dataset.py:
// 62-78), applied to the PIL frame before Resize.  On a PIL image ColorJitter is four PILLOW operations in a drawn order; the
// contract is PILLOW'S, byte for byte.  tests/color_jitter_ref.py restates it in NumPy and tests/test_color_jitter_host.py pins
// that restatement against the installed Pillow - blend on the whole 256 x 256 table, both colour conversions on all 2^24 inputs.
//
// THE JITTER CONTRACT.  A frame's record names up to four operations in application order; each works on the uint8 result of
// the one before it.
// L(r, g, b) = (19595 r + 38470 g + 7471 b + 32768) >> 16                                        (Pillow's convert('L'))
// blend(d, v, a) for integers d, v in 0 .. 255 and an fp32 a >= 0: t = float(d) + a * float(v - d), the product and the sum
//   each rounded to fp32 - never an FMA; out = 0 if t <= 0, 255 if t >= 255, else trunc(t).  (Pillow's ImagingBlend only clamps
//   when a lies outside [0, 1]; inside, 0 <= t <= 255 holds anyway - |a x| <= |x| survives the rounding - so one rule serves.)
// Brightness f: blend(0, v, f) per channel.  Saturation f: blend(L(pixel), v, f) per channel (ImageEnhance.Color).
// Contrast f: blend(m, v, f) per channel, m = int(S / N + 0.5) in float64, S = the integer sum of L over the WHOLE frame as it
//   stands when contrast is reached (after the operations before it), N = H W.  S takes 64 bits: 8192 x 8192 x 255 = 1.7e10.
// Hue shift k in 0 .. 255: RGB -> HSV, h' = (h + k) mod 256, HSV -> RGB, both as Pillow's Convert.c evaluates them.
//   RGB -> HSV: v = maxc; maxc == minc: h = s = 0.  Else in fp32 cr = float(maxc - minc), s = cr / float(maxc), rc = float(maxc
//   - r) / cr and gc, bc alike; h = bc - gc in fp32 if r == maxc, else fp32(2.0 + rc - bc) if g == maxc, else fp32(4.0 + gc - rc)
//   with these two sums in double; h = fp32(fmod(double(h) / 6.0 + 1.0, 1.0)); uh = min(int(double(h) * 255.0), 255), us alike.
//   HSV -> RGB: s == 0: grey v.  Else hh = double(h) * 6.0 / 255.0, i = floor(hh), f = fp32(hh - i), fs = fp32(double(s) /
//   255.0); p = round(v (1 - fs)), q = round(v (1 - fs f)), t = round(v (1 - fs (1 - f))) in double, half away from zero;
//   i mod 6 picks (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q).
// Every division here is IEEE's (the build's default: correctly rounded fp32 and fp64 division); fp contraction is off for the
// whole file.
//
// MAPPING.  At most two kernel launches per call, whatever the orders.  The tiles of all frames are numbered back to back and a
// 256-thread workgroup finds its frame by bisecting the tile prefix of the record table (uniform: scalar loads), as the other
// ragged kernels do.  A tile is 256 x 16 pixels: a thread takes four neighbouring pixels (12 bytes) of a row, a wavefront 768
// contiguous bytes, and four rows in turn.  Where the row's first byte is dword aligned in both slabs the twelve bytes move as
// three dwords; elsewhere, and at a row's ragged end, byte by byte - the same values either way.
//   1. stat launch, over the frames whose order holds contrast only: every pixel runs the operations before contrast in
//      registers and takes L; a wave reduction, four LDS words and ONE 64-bit vector atomic add per workgroup to the frame's sum.
//      Integer sums: the result does not depend on scheduling.  The sums are zeroed by a memset node in front of it.
//   2. apply launch: every pixel runs its frame's whole chain, m formed from the sum, and is written once.
// What the hue shift needs per 8-bit value - the sector and f of h', fs of s, two double divisions - a workgroup whose chain
// holds hue tabulates once in LDS (256 entries, one per thread).  A pixel is read and written by the same thread: in place
// (out == in, same rectangles) gives the bytes out of place gives.  Row padding and bytes outside the rectangles are never
// written.
#include "specmi_internal.h"

#pragma clang fp contract(off)

namespace specmi {

// what HSV -> RGB needs of an 8-bit hue or saturation, tabulated per workgroup
struct HueLut { float f[256], fs[256]; int sector[256]; };

__device__ __forceinline__ int jitter_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

__device__ __forceinline__ int jitter_blend(int d, int v, float a) {
    const float p = a * (float)(v - d);
    const float t = (float)d + p;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ void jitter_hue(int k, const HueLut& lut, int& r, int& g, int& b) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    if (maxc == minc) return;                                   // h = s = 0: grey v, the pixel itself
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    // (maxc - x) / cr is exactly 0 for a channel at the maximum and exactly 1 for one at the minimum: only the middle one divides
    const float mid = (float)(maxc - (r + g + b - maxc - minc)) / cr;
    const float rc = r == maxc ? 0.f : (r == minc ? 1.f : mid);
    const float gc = g == maxc ? 0.f : (g == minc ? 1.f : mid);
    const float bc = b == maxc ? 0.f : (b == minc ? 1.f : mid);
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    double hd = (double)h / 6.0 + 1.0;                          // in [5/6, 11/6]: fmod(., 1.0) is an exact subtraction
    hd = hd >= 1.0 ? hd - 1.0 : hd;
    const int uh = min((int)((double)(float)hd * 255.0), 255), us = min((int)((double)s * 255.0), 255);
    if (us == 0) { r = g = b = maxc; return; }
    const int hs = (uh + k) & 255;
    const double v = (double)maxc, fs = (double)lut.fs[us], f = (double)lut.f[hs];
    const int p = min((int)(v * (1.0 - fs) + 0.5), 255);        // all three are >= 0: half away from zero = floor(x + 0.5)
    const int q = min((int)(v * (1.0 - fs * f) + 0.5), 255);
    const int t = min((int)(v * (1.0 - fs * (1.0 - f)) + 0.5), 255);
    switch (lut.sector[hs]) {
        case 0: r = maxc; g = t; b = p; break;
        case 1: r = q; g = maxc; b = p; break;
        case 2: r = p; g = maxc; b = t; break;
        case 3: r = p; g = q; b = maxc; break;
        case 4: r = t; g = p; b = maxc; break;
        default: r = maxc; g = p; b = q; break;
    }
}

// a frame's record as a workgroup keeps it: in scalar registers, read once - the stores of the apply launch may not alias it
struct JitterChain { int op[4]; float a[4]; int k; };

// THE PER-PIXEL CHAIN, stated once: operations [0, n) of a frame's chain on a thread's four pixels r | g << 8 | b << 16; m =
// contrast's grey level (not read unless contrast is among them).  The chain is uniform over the workgroup: one scalar branch per
// operation, the four pixels side by side under it.
__device__ __forceinline__ void jitter_pixels(const JitterChain& c, int n, int m, const HueLut& lut, unsigned (&px)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= n) break;
        const int op = c.op[i];
        const float a = c.a[i];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int r = px[p] & 255, g = (px[p] >> 8) & 255, b = (px[p] >> 16) & 255;
            if (op == kJitterHue) {
                jitter_hue(c.k, lut, r, g, b);
            } else {
                const int d = op == kJitterBrightness ? 0 : (op == kJitterContrast ? m : jitter_luma(r, g, b));
                r = jitter_blend(d, r, a); g = jitter_blend(d, g, a); b = jitter_blend(d, b, a);
            }
            px[p] = (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16;
        }
    }
}

// kStat: the stat launch (operations before contrast, L summed into sums[frame]); else the apply launch
template <bool kStat> __global__ void __launch_bounds__(256) color_jitter_kernel(JitterArgs a) {
    __shared__ HueLut lut;
    __shared__ int s_wave[4];
    // the LAST frame whose first tile is not beyond this one has tiles (a frame outside the launch has none)
    const int blk = blockIdx.x;
    int lo = 0, hi = a.nframes;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((kStat ? a.frames[mid].stile0 : a.frames[mid].tile0) <= blk) lo = mid; else hi = mid;
    }
    const JitterFrame& fr = a.frames[lo];
    JitterChain chain;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int op = fr.rec.op[i];
        chain.op[i] = op;
        chain.a[i] = op == kJitterBrightness ? fr.rec.f[0] : (op == kJitterContrast ? fr.rec.f[1] : fr.rec.f[2]);
    }
    chain.k = fr.rec.k;
    const int H = fr.H, W = fr.W;
    const int tile = blk - (kStat ? fr.stile0 : fr.tile0);
    const int nops = kStat ? fr.npre : fr.nops;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool hue = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) hue = hue || (i < nops && chain.op[i] == kJitterHue);
    if (hue) {                                                  // uniform
        const double hh = (double)tid * 6.0 / 255.0, fl = floor(hh);
        lut.sector[tid] = (int)fl % 6;
        lut.f[tid] = (float)(hh - fl);
        lut.fs[tid] = (float)((double)tid / 255.0);
        __syncthreads();
    }
    int m = 0;
    if (!kStat && fr.npre >= 0) m = (int)((double)a.sums[lo] / ((double)H * (double)W) + 0.5);
    const int x0 = (tile % fr.tiles_x) * kJitterTileW + 4 * lane;
    const int y0 = (tile / fr.tiles_x) * kJitterTileH + wave;
    const int nvalid = min(W - x0, 4);                          // <= 0: the thread is past the row's end
    int lsum = 0;
#pragma unroll 1                                                // the chain is long: one copy of it keeps the kernel in the instruction cache
    for (int it = 0; it < kJitterTileH / 4; ++it) {
        const int y = y0 + 4 * it;
        if (y >= H || nvalid <= 0) continue;
        const unsigned char* src = a.in + fr.in_off + (long long)y * fr.in_pitch + 3 * x0;
        unsigned char* dst = kStat ? nullptr : a.out + fr.out_off + (long long)y * fr.out_pitch + 3 * x0;
        const bool wide = nvalid == 4 && ((uintptr_t)src & 3) == 0 && (kStat || ((uintptr_t)dst & 3) == 0);
        unsigned px[4] = {0, 0, 0, 0};
        if (wide) {
            const unsigned w0 = ((const unsigned*)src)[0], w1 = ((const unsigned*)src)[1], w2 = ((const unsigned*)src)[2];
            px[0] = w0 & 0xffffffu; px[1] = (w0 >> 24) | (w1 & 0xffffu) << 8; px[2] = (w1 >> 16) | (w2 & 0xffu) << 16; px[3] = w2 >> 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nvalid) px[i] = (unsigned)src[3 * i] | (unsigned)src[3 * i + 1] << 8 | (unsigned)src[3 * i + 2] << 16;
        }
        jitter_pixels(chain, nops, m, lut, px);
        if (kStat) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nvalid) lsum += jitter_luma(px[i] & 255, (px[i] >> 8) & 255, (px[i] >> 16) & 255);
        } else if (wide) {
            ((unsigned*)dst)[0] = px[0] | px[1] << 24;
            ((unsigned*)dst)[1] = px[1] >> 8 | px[2] << 16;
            ((unsigned*)dst)[2] = px[2] >> 16 | px[3] << 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nvalid) {
                    dst[3 * i] = (unsigned char)px[i]; dst[3 * i + 1] = (unsigned char)(px[i] >> 8); dst[3 * i + 2] = (unsigned char)(px[i] >> 16);
                }
        }
    }
    if (kStat) {
        // a thread's 16 pixels sum to at most 4080, a workgroup's 4096 to 1044480: 32 bits until the frame's sum
        lsum = wave_sum64(lsum);
        if (lane == 0) s_wave[wave] = lsum;
        __syncthreads();
        if (tid == 0) atomicAdd(a.sums + lo, (unsigned long long)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]));
    }
}

int jitter_frame_tiles(int H, int W, int* tiles_x) {
    *tiles_x = (W + kJitterTileW - 1) / kJitterTileW;
    return *tiles_x * ((H + kJitterTileH - 1) / kJitterTileH);
}

int launch_color_jitter(const JitterArgs& a, int stat_tiles, int tiles, double stat_px, double px, const LaunchCtx& ctx) {
    if (stat_tiles > 0) {
        hipError_t e = hipMemsetAsync(a.sums, 0, (size_t)a.nframes * sizeof(unsigned long long), ctx.stream);
        if (e != hipSuccess) return (int)e;
        ProfScope ps(ctx, "color_jitter_stat", 0.0, stat_px * 3);
        hipLaunchKernelGGL(color_jitter_kernel<true>, dim3((unsigned)stat_tiles), dim3(256), 0, ctx.stream, a);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    ProfScope ps(ctx, "color_jitter_apply", 0.0, px * 6);
    hipLaunchKernelGGL(color_jitter_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

}  // namespace specmi
