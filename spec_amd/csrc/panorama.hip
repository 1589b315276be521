// panorama.hip - perspective views with known (vfov, pitch, roll) cut out of an equirectangular panorama on the device
// (DESIGN.md section 7 row f-6): the per-pixel work of the reference's dataset generator, extractImage's mode="image"
// branch (camcalib/datagen/image_extraction.py:129-159), for n views of DIFFERENT sizes in ONE launch.  The views land
// in a uint8 HWC slab with per-view byte offsets - what specmi_resize_normalize_ragged reads - so a generated validation
// batch never leaves the device.
//
// Per output pixel, in fp64 and in the reference's order of operations:
//   x = linspace(-fovX, fovX, W)[j], y = linspace(-fovY, fovY, H)[i]            (numpy: j * step + start, last sample = stop)
//   (x, y) <- (x cos r + y sin r, -x sin r + y cos r)                            ((i.T * xform).T)
//   rho = sqrt(x^2 + y^2), c = atan(rho)                                         (rectilinear2latlong)
//   elev = asin(cos c sin e + y sin c cos e / (rho + 1e-10))
//   azim = a + atan2(x sin c, rho cos e cos c - y sin e sin c), then the two +-2 pi wraps
//   column = azim / pi * PW / 2 + PW / 2, row = elev / (pi / 2) * PH / 2 + PH / 2
// followed by scipy.ndimage.map_coordinates(order=1, prefilter=False, mode="wrap") as scipy computes it: the historical
// "wrap" folds a coordinate outside [0, N - 1] by multiples of N - 1 (first and last sample overlap), the weights are
// (1 - f, 1 - (1 - f)) of the fractional part, the four taps are accumulated row-major as ((v * wy) * wx), and the uint8
// store is 0 for a non-positive value, else trunc(v + 0.5) clipped to 255.  fp contraction is off: every product and sum
// rounds as the reference's does.  What can differ is the last ulp of the device's asin / atan2 / sin / cos / atan.
//
// The work is a gather: a wavefront covers a compact 16 x 4 output tile (a workgroup 32 x 8), so its taps fall into a few
// neighbouring panorama rows, and the 16 lanes of a tile row write 48 contiguous bytes.  Everything a view fixes - sin /
// cos of elevation and roll, the linspace starts and steps, the slab offset - comes from a per-view record built on the
// host with the host's libm, as the reference evaluates them once per view.
#include <cmath>

#include "specmi_internal.h"

#pragma clang fp contract(off)

namespace specmi {

constexpr int kTileW = 32, kTileH = 8;     // output pixels per workgroup; a wavefront covers 16 x 4 of them

// scipy's map_coordinate() for NI_EXTEND_WRAP: the period is len - 1
__device__ __forceinline__ double wrap_coordinate(double in, int len) {
    if (len <= 1) return (in < 0.0 || in > (double)(len - 1)) ? 0.0 : in;
    const double sz = (double)(len - 1);
    if (in < 0.0) in += sz * ((double)(long long)(-in / sz) + 1.0);
    else if (in > sz) in -= sz * (double)(long long)(in / sz);
    return in;
}

__global__ void __launch_bounds__(256) pano_extract_kernel(const unsigned char* __restrict__ pano, int PH, int PW,
                                                            const PanoView* __restrict__ views, unsigned char* __restrict__ out) {
    const PanoView& v = views[blockIdx.y];
    const int tiles_x = (v.W + kTileW - 1) / kTileW;
    const int tile = blockIdx.x;
    if (tile >= tiles_x * ((v.H + kTileH - 1) / kTileH)) return;       // the grid is sized for the largest view
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int j = (tile % tiles_x) * kTileW + (wave & 1) * 16 + (lane & 15);
    const int i = (tile / tiles_x) * kTileH + (wave >> 1) * 4 + (lane >> 4);
    if (i >= v.H || j >= v.W) return;
    // numpy.linspace: arange(num) * step + start, the last sample set to stop; one sample = start
    const double x0 = (v.W > 1 && j == v.W - 1) ? v.x_stop : (double)j * v.x_step + v.x_start;
    const double y0 = (v.H > 1 && i == v.H - 1) ? v.y_stop : (double)i * v.y_step + v.y_start;
    const double x = x0 * v.cos_roll + y0 * v.sin_roll;
    const double y = x0 * v.neg_sin_roll + y0 * v.cos_roll;
    const double rho = sqrt(x * x + y * y);
    const double c = atan(rho);
    const double sinc = sin(c), cosc = cos(c);
    const double elev = asin(cosc * v.sin_el + y * sinc * v.cos_el / (rho + 1e-10));
    double azim = v.azimuth + atan2(x * sinc, rho * v.cos_el * cosc - y * v.sin_el * sinc);
    const double pi = 3.141592653589793;
    if (azim > pi) azim -= 2.0 * pi;
    if (azim < -pi) azim += 2.0 * pi;
    const double colf = wrap_coordinate(azim / pi * (double)PW / 2.0 + (double)PW / 2.0, PW);
    const double rowf = wrap_coordinate(elev / (pi / 2.0) * (double)PH / 2.0 + (double)PH / 2.0, PH);
    const double fr = floor(rowf), fc = floor(colf);
    // a NaN coordinate (asin of an argument rounded past 1) converts to 0; the clamps keep every tap inside the panorama
    const int r0 = min(max((int)fr, 0), PH - 1), c0 = min(max((int)fc, 0), PW - 1);
    const int r1 = min(r0 + 1, PH - 1), c1 = min(c0 + 1, PW - 1);     // reached only with weight 0 (coordinate == N - 1)
    const double wy0 = 1.0 - (rowf - fr), wy1 = 1.0 - wy0, wx0 = 1.0 - (colf - fc), wx1 = 1.0 - wx0;
    const unsigned char* p00 = pano + ((size_t)r0 * PW + c0) * 3;
    const unsigned char* p01 = pano + ((size_t)r0 * PW + c1) * 3;
    const unsigned char* p10 = pano + ((size_t)r1 * PW + c0) * 3;
    const unsigned char* p11 = pano + ((size_t)r1 * PW + c1) * 3;
    int tap[4][3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { tap[0][ch] = p00[ch]; tap[1][ch] = p01[ch]; tap[2][ch] = p10[ch]; tap[3][ch] = p11[ch]; }
    unsigned char* q = out + v.out_off + ((size_t)i * v.W + j) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double s = 0.0;
        s += (double)tap[0][ch] * wy0 * wx0;
        s += (double)tap[1][ch] * wy0 * wx1;
        s += (double)tap[2][ch] * wy1 * wx0;
        s += (double)tap[3][ch] * wy1 * wx1;
        s = s > 0.0 ? s + 0.5 : 0.0;
        s = s > 255.0 ? 255.0 : s;
        q[ch] = (unsigned char)(int)s;
    }
}

int launch_pano_extract(const unsigned char* pano, int PH, int PW, const PanoView* views, int n, int max_tiles, double out_bytes,
                        unsigned char* out, const LaunchCtx& ctx) {
    // algorithmic bytes: every output byte once + at most the four taps of every pixel, never more than the panorama
    ProfScope ps(ctx, "pano_extract", 0.0, out_bytes + fmin(4.0 * out_bytes, (double)PH * PW * 3));
    hipLaunchKernelGGL(pano_extract_kernel, dim3(max_tiles, n), dim3(256), 0, ctx.stream, pano, PH, PW, views, out);
    return (int)hipGetLastError();
}

// The per-view record from the reference's arguments; false if the size does not follow from (H, ratio).  The width is
// Python's round() (half to even) of H / (1 / ratio), the reference's croppedSize.
bool make_pano_view(const double* view, int H, int W, long long out_off, PanoView& pv) {
    const double elevation = view[0], azimuth = view[1], roll = view[2], vfov = view[3], ratio = view[4];
    const double ratiohw = 1.0 / ratio;
    if (std::nearbyint((double)H / ratiohw) != (double)W) return false;
    const double fovY = std::tan(vfov * (M_PI / 180.0) / 2.0), fovX = fovY / ratiohw;
    pv = PanoView{};
    pv.sin_el = std::sin(elevation); pv.cos_el = std::cos(elevation); pv.azimuth = azimuth;
    pv.cos_roll = std::cos(roll); pv.sin_roll = std::sin(roll); pv.neg_sin_roll = -pv.sin_roll;
    pv.x_start = -fovX; pv.x_stop = fovX; pv.x_step = W > 1 ? (fovX - -fovX) / (double)(W - 1) : 0.0;
    pv.y_start = -fovY; pv.y_stop = fovY; pv.y_step = H > 1 ? (fovY - -fovY) / (double)(H - 1) : 0.0;
    pv.out_off = out_off; pv.H = H; pv.W = W;
    return true;
}

int pano_view_tiles(int H, int W) { return ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH); }

}  // namespace specmi
