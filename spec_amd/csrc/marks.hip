// marks.hip - horizon lines and captions drawn into uint8 frames on the device: what the
// reference's show_horizon_line (camcalib/vis_utils.py:63-110) does on the host with Pillow - a black caption strip, the
// caption text, a wide line - for all frames of a flush in one launch, and the denormalised network input that CamCalib's
// validation pictures are drawn on (camcalib/trainer.py:118-133).  The contract is PILLOW'S, byte for byte; tests/marks_ref.py
// restates it in NumPy and tests/test_marks_host.py pins that restatement against the installed Pillow.
//
// THE MARKS CONTRACT.  A frame's marks are applied in order (painter's order); a pixel that no mark covers is never written.
// Strip [y0, y1) with an RGB value: rows [y0, y1) n [0, H) are set to it - the reference's image[0:text_size] = 0.
// Mask blend: a uint8 coverage mask of mw x mh at a byte offset of the mask buffer, its top-left corner at integer (x, y) of
//   the frame (negative or past the edge: clipped), and an RGB ink.  Pillow's ImagingFill2 with a mode L mask: per channel,
//   where the mask byte m != 0,  t = in * (255 - m) + ink * m + 128;  out = ((t >> 8) + t) >> 8  - ONE rounding of the sum
//   (Pillow's BLEND).  A pixel under m == 0 is not written.  Fonts are not rendered here: the mask comes from Pillow.
// Wide line (x0, y0, x1, y1), integer, |coordinate| <= 100000 (the range pinned against Pillow), width 2 .. 64, overwrites.
//   Pillow's ImagingDrawWideLine.  RU(f) = f >= 0 ? floor(f + 0.5) : -floor(|f| + 0.5);  RD(f) = f >= 0 ? ceil(f - 0.5) :
//   -ceil(|f| - 0.5).  dx = x1 - x0, dy = y1 - y0; dx == dy == 0: the single pixel (x0, y0).  In double: big = hypot(dx, dy),
//   small = (width - 1) / 2.0, rmax = RU(small) / big, rmin = RD(small) / big, dxmin = RD(rmin * dy), dxmax = RD(rmax * dy),
//   dymin = RU(rmin * dx), dymax = RU(rmax * dx).  Vertices (x0 - dxmin, y0 + dymax), (x1 - dxmin, y1 + dymax),
//   (x1 + dxmax, y1 - dymin), (x0 + dxmax, y0 - dymin); the edges join consecutive vertices cyclically, and each
//   non-horizontal one keeps ymin, ymax, its first vertex (ex0, ey0) and edx = (float)(x1 - x0) / (float)(y1 - y0) in fp32.
//   Row y of the frame: over the non-horizontal edges with ymin <= y <= ymax, xx = (float)(y - ey0) * edx + (float)ex0 - a
//   separately rounded fp32 multiply and add, never an FMA; the row covers x from RU(min xx) to RD(max xx) (fp32 + 0.5F),
//   clipped to [0, W - 1].  Every horizontal edge on row y covers [xmin, xmax], clipped.  (Pillow's polygon filler pairs the
//   sorted intersections; for this convex quadrilateral that is the minimum and the maximum.)
//   All of the double arithmetic happens on the host (api.hip, marks_line_edges); the kernel multiplies, adds and compares.
//
// MAPPING.  Work follows the area the marks cover, not the frame: the host lists the 64 x 16 pixel tiles of every frame that
// some mark of that frame can reach (a strip's rows, a mask's clipped rectangle, a line's spans row by row from the very
// function the kernel evaluates, grown by a pixel), and one 256-thread workgroup takes one listed tile: a wavefront per row
// (192 contiguous bytes), four rows per thread.  The workgroup walks its frame's marks in order - the records are uniform:
// scalar loads - and every thread carries its four pixels in registers: a pixel is read only when a blend meets it before
// anything has overwritten it, and written once at the end if a mark covered it.  No atomics, no workspace, nothing that
// depends on scheduling.
#include "specmi_internal.h"

namespace specmi {

__global__ void __launch_bounds__(256) draw_marks_kernel(MarksArgs a) {
    const int f = a.tiles[2 * blockIdx.x], txy = a.tiles[2 * blockIdx.x + 1];
    const MarkFrame fr = a.frames[f];
    const int x = (txy & 0xffff) * kMarkTileW + (threadIdx.x & 63);
    const int yb = (txy >> 16) * kMarkTileH + (threadIdx.x >> 6);
    if (x >= fr.W) return;                                      // no barrier below
    unsigned char* const base = a.slab + fr.off + 3 * x;
    unsigned val[4] = {0, 0, 0, 0};
    bool have[4] = {false, false, false, false};
    for (int m = 0; m < fr.count; ++m) {
        const MarkDev& mk = a.marks[fr.mark0 + m];
        const int kind = mk.kind;
        const unsigned rgb = mk.rgb;
        if (kind == kMarkStrip) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = yb + 4 * r;
                if (y >= mk.a && y < mk.b) { val[r] = rgb; have[r] = true; }
            }
        } else if (kind == kMarkLine) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = yb + 4 * r;
                int xa, xb;
                mark_line_span(mk.e, y, xa, xb);
                bool cov = x >= xa && x <= xb;
#pragma unroll
                for (int i = 0; i < 4; ++i) cov = cov || (mk.e[i].horiz && y == mk.e[i].ymin && x >= mk.e[i].xmin && x <= mk.e[i].xmax);
                if (cov) { val[r] = rgb; have[r] = true; }
            }
        } else {
            const int mx = x - mk.a;
            if (mx < 0 || mx >= mk.c) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = yb + 4 * r, my = y - mk.b;
                if (y >= fr.H || my < 0 || my >= mk.d) continue;
                const unsigned cm = a.masks[mk.off + (long long)my * mk.c + mx];
                if (cm == 0) continue;
                if (!have[r]) {
                    const unsigned char* p = base + (long long)y * fr.pitch;
                    val[r] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
                    have[r] = true;
                }
                unsigned out = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned t = ((val[r] >> (8 * c)) & 255u) * (255u - cm) + ((rgb >> (8 * c)) & 255u) * cm + 128u;
                    out |= ((((t >> 8) + t) >> 8) & 255u) << (8 * c);
                }
                val[r] = out;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = yb + 4 * r;
        if (y >= fr.H || !have[r]) continue;
        unsigned char* o = base + (long long)y * fr.pitch;
        o[0] = (unsigned char)val[r]; o[1] = (unsigned char)(val[r] >> 8); o[2] = (unsigned char)(val[r] >> 16);
    }
}

int launch_draw_marks(const MarksArgs& a, double px, const LaunchCtx& ctx) {
    if (a.ntiles == 0) return 0;                                // no mark reaches a frame
    // at most a read and a write of every listed tile's pixels, and a mask byte each
    ProfScope ps(ctx, "draw_marks", 0.0, px * 7);
    hipLaunchKernelGGL(draw_marks_kernel, dim3((unsigned)a.ntiles), dim3(256), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

// One image of a normalised NCHW fp32 batch -> an HWC uint8 frame: v = (x * std + mean) * 255, every operation rounded
// separately in fp32 (NumPy's order); NaN -> 0, v clamped to [0, 255] - the reference's astype('uint8') is undefined outside
// it: this project's stated deviation - and truncated.  One thread per pixel: three coalesced plane reads, three bytes out.
__global__ void __launch_bounds__(256) denormalize_u8_kernel(DenormArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    const float* p = a.x + (long long)y * a.Wp + x;
    unsigned char* o = a.out + (long long)y * a.pitch + 3 * x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma clang fp contract(off)                                  // x * std + mean must not become an FMA (see mark_edge_x)
        const float t = p[c * a.plane] * a.std[c];
        const float v = (t + a.mean[c]) * 255.f;
        o[c] = (unsigned char)(v > 0.f ? (int)fminf(v, 255.f) : 0);     // a NaN compares false: 0
    }
}

int launch_denormalize_u8(const DenormArgs& a, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "denormalize_u8", 5.0 * a.h * a.w * 3, 15.0 * a.h * a.w);
    hipLaunchKernelGGL(denormalize_u8_kernel, dim3((unsigned)((a.w + 63) / 64), (unsigned)((a.h + 3) / 4)), dim3(256), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

}  // namespace specmi
