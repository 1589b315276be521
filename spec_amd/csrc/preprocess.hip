// preprocess.hip - crop + normalise on the device.
//
// Replaces the per-detection host loop that feeds the hot path (spec/tester.py:116-128):
// get_single_image_crop_demo(img, bbox, scale=1.0, crop_size=224) = VIBE/PARE's 3-point affine
// (rot = 0) + cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT) + ToTensor + Normalize, followed by
// bbox_scale = bbox[2]/200 and bbox_center = bbox[:2].  One launch handles all detections of a
// frame: uint8 RGB HWC frame in HBM -> (n,3,S,S) fp32 NCHW crops, already where the trunk reads
// them (no host crop, no H2D of 602 KB per detection).
//
// The warp reproduces OpenCV's fixed-point bilinear path exactly (integer arithmetic): inverse
// affine in fp64, source coordinates in 1/1024 px rounded to 1/32 px, weights
// (32-fx)(32-fy)*32 ... summing to 2^15, result (sum + 2^14) >> 15; then (u8/255 - mean)/std
// in fp32 like ToTensor + Normalize.  Lanes map to consecutive x of one output row, so the
// NCHW stores are coalesced; the 4 taps x 3 channels come through L2 (a frame is a few MB).
#include <cmath>

#include "specmi_internal.h"

namespace specmi {

// Work mapping of both crops, in their kernels for one frame size and for ragged slabs alike (crop_normalize_pixels and
// crop_resize_pixels state it): a workgroup covers kNB batches of 256 * kPX consecutive output pixels of one crop, each as
// kPX chunks of 256; lane t handles pixel chunk * 256 + t of each chunk.  Neighbouring lanes therefore read neighbouring
// source pixels (a wave's gather touches 2-5 cache lines, not the 10-20 a "4 consecutive pixels per lane" mapping does:
// the L1 tag rate, not HBM, bounds a gather) and write 256 contiguous bytes per colour plane.  All taps of the kPX
// pixels are loaded back to back, unconditionally, from clamped (always valid) addresses and zero-weighted afterwards
// where they leave the frame - predicated loads would each sit in their own exec-masked branch and serialise on the
// memory latency.  The two horizontally adjacent taps of a row (6 contiguous bytes) come from ONE unaligned 8-byte load.
constexpr int kPX = 4;

// The fp16 output form of every producer below (template parameter F16; specmi.h "NHWC8 fp16"): the same fp32 value v per
// channel, rounded once to nearest even, stored as pixel-major (n, H, W, 8) halves - channels 0-2 = fp16(v), 3-7 = +0 - which
// is what to_nhwc_f16_kernel (conv_f16.hip) makes of the fp32 image and what the Cin = 8 stem reads.  The lane that owns a pixel
// writes it as ONE 16-byte vector; lanes own consecutive pixels in every kernel here, so a wave stores 1 KiB contiguous
// (the fp32 form: three 256-byte runs in three colour planes).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void store_nhwc8(void* __restrict__ out, size_t pixel, const float (&v)[3]) {
    const f16x8 p = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f,
                     (_Float16)0.f};
    reinterpret_cast<f16x8*>(out)[pixel] = p;
}

// RGB of the pixels c0 and c1 (0 <= c0 <= c1 <= c0 + 1 <= W - 1) of frame row cy.  WIDE needs W >= 2 and total >= 8 bytes.
template <bool WIDE>
__device__ __forceinline__ void load_tap_pair(const unsigned char* __restrict__ frame, size_t total, int W, int cy, int c0,
                                              int c1, int (&t0)[3], int (&t1)[3]) {
    // 24-bit multiplies (full rate; v_mul_lo_u32 is quarter rate): the launchers guarantee H, W < 2^24 and H*W*3 < 2^32
    if (WIDE) {
        const int bx = min(c0, W - 2);
        const unsigned addr = (__umul24((unsigned)cy, (unsigned)W) + (unsigned)bx) * 3u;
        const unsigned base = min(addr, (unsigned)total - 8u);          // never read past the end of the frame: shift instead
        unsigned long long w;
        __builtin_memcpy(&w, frame + base, 8);
        const unsigned sh = 8u * (addr - base);                          // <= 2 bytes, so 6 valid bytes (two pixels) remain
        const unsigned a = (unsigned)(w >> (sh + 24u * (unsigned)(c0 - bx))) & 0xFFFFFFu;
        const unsigned b = (unsigned)(w >> (sh + 24u * (unsigned)(c1 - bx))) & 0xFFFFFFu;
#pragma unroll
        for (int c = 0; c < 3; ++c) { t0[c] = (a >> (8 * c)) & 255; t1[c] = (b >> (8 * c)) & 255; }
    } else {
        const unsigned row = __umul24((unsigned)cy, (unsigned)W);
        const unsigned char* q0 = frame + (row + (unsigned)c0) * 3u;
        const unsigned char* q1 = frame + (row + (unsigned)c1) * 3u;
#pragma unroll
        for (int c = 0; c < 3; ++c) { t0[c] = q0[c]; t1[c] = q1[c]; }
    }
}

// cv::warpAffine's inverse map of get_single_image_crop_demo's affine (rot = 0: M1 = M3 = +-0, or NaN for a degenerate
// box - in both cases X does not depend on y nor Y on x, so the source coordinate is separable)
struct CropAffine {
    double M0, M1, M2, M3, M4, M5;
    __device__ CropAffine(float cx, float cy, float bw, float bh, float scale, int S) {
        // forward affine (src -> dst), then cv::warpAffine's inversion, all in fp64
        const float sw = (bw * scale) * 0.5f, sh = (bh * scale) * 0.5f;
        const double half = (double)((float)S * 0.5f);
        const double ax = half / (double)sw, ay = half / (double)sh;
        M0 = ax; M1 = 0.0; M2 = half - ax * (double)cx; M3 = 0.0; M4 = ay; M5 = half - ay * (double)cy;
        double D = M0 * M4 - M1 * M3;
        D = D != 0.0 ? 1.0 / D : 0.0;
        const double A11 = M4 * D, A22 = M0 * D;
        M0 = A11; M1 *= -D; M3 *= -D; M4 = A22;
        const double b1 = -M0 * M2 - M1 * M5, b2 = -M3 * M2 - M4 * M5;
        M2 = b1; M5 = b2;
    }
    // (integer source coordinate clamped to [-2, n] - enough to keep the border flags and the clamped taps -, 1/32 fraction)
    __device__ int2 col(int x, int W) const {     // X = (round((M1*y + M2)*1024) + 16 + round(M0*x*1024)) >> 5 at y = 0
        const long long X = (__double2ll_rn((M1 * 0 + M2) * 1024.0) + 16 + __double2ll_rn(M0 * x * 1024.0)) >> 5;
        return make_int2((int)min(max(X >> 5, -2LL), (long long)W), (int)(X & 31));
    }
    __device__ int2 row(int y, int H) const {     // Y = (round((M4*y + M5)*1024) + 16 + round(M3*x*1024)) >> 5 at x = 0
        const long long Y = (__double2ll_rn((M4 * y + M5) * 1024.0) + 16 + __double2ll_rn(M3 * 0 * 1024.0)) >> 5;
        return make_int2((int)min(max(Y >> 5, -2LL), (long long)H), (int)(Y & 31));
    }
};

constexpr int kTabX = 2048;                    // crops up to 2048 x 2048 use the per-workgroup coordinate tables
constexpr int kNB = 2;                        // batches of kPX pixels per lane: a workgroup covers 256 * kPX * kNB pixels
constexpr int kTabY = 256 * kPX * kNB + 2;     // rows a workgroup's pixels can touch (S = 1)

// ToTensor + ImageNet Normalize of a uint8 value of colour plane c: two IEEE divisions and a subtraction
__device__ __forceinline__ float to_tensor_normalize(int v, int c) { return normalize_unit((float)v / 255.0f, c); }

// what the four crop launchers share: the grid (x: workgroups of a crop, y: crops) and the refusal of a frame that the
// 24-bit multiplies and 32-bit byte offsets of load_tap_pair cannot address
static dim3 crop_grid(int S, int n) { return dim3((S * S + 256 * kPX * kNB - 1) / (256 * kPX * kNB), n); }
static bool crop_frame_too_large(int H, int W) { return H >= (1 << 24) || W >= (1 << 24) || (double)H * W * 3 >= 4294967296.0; }
// WIDE's condition: by the host for a launch on one frame size, per crop (wave-uniform) in the ragged kernels
__host__ __device__ __forceinline__ bool crop_wide(int H, int W) { return W >= 2 && (size_t)H * W * 3 >= 8; }

// Each crop is stated once, as a prologue (what a workgroup prepares) and a per-pixel path (crop_*_pixels); its kernel for
// frames of one size and its ragged kernel differ only in where (frame, H, W) come from.
//
// Demo crop.  ToTensor + Normalize of a uint8 value takes two IEEE divisions; the 3 x 256 possible results are tabulated in LDS
// once per workgroup with exactly those divisions.  The separable source coordinates (fp64 -> 1/1024 px fixed point) are
// tabulated too: S columns + the few rows of this workgroup instead of 4 fp64->int64 conversions per pixel.  The
// per-pixel path is integer arithmetic + three LDS reads + two 8-byte loads.
//
// The prologue of crop d = blockIdx.y: the table of normalised values, the box (recorded as bbox_scale / bbox_center by the
// crop's first workgroup), its inverse affine and the coordinate tables; ends with the barrier that publishes the tables
template <bool TABLE>
__device__ __forceinline__ CropAffine crop_normalize_prologue(int H, int W, const float* __restrict__ bboxes, float scale, int S,
                                                              float* __restrict__ bbox_scale, float* __restrict__ bbox_center,
                                                              float (&lut)[3][256], int2* tabx, int2* taby) {
    const int d = blockIdx.y, t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][t] = to_tensor_normalize(t, c);
    const float cx = bboxes[d * 4 + 0], cy = bboxes[d * 4 + 1], bw = bboxes[d * 4 + 2], bh = bboxes[d * 4 + 3];
    if (blockIdx.x == 0 && t == 0) {
        if (bbox_scale) bbox_scale[d] = bw / 200.0f;
        if (bbox_center) { bbox_center[d * 2 + 0] = cx; bbox_center[d * 2 + 1] = cy; }
    }
    const CropAffine A(cx, cy, bw, bh, scale, S);
    if (TABLE) {
        const int npix = S * S, pix0 = blockIdx.x * (256 * kPX * kNB);
        const int yfirst = pix0 / S, ylast = min(pix0 + 256 * kPX * kNB - 1, npix - 1) / S;
        for (int i = t; i < S; i += 256) tabx[i] = A.col(i, W);
        for (int i = t; i <= ylast - yfirst; i += 256) taby[i] = A.row(yfirst + i, H);
    }
    __syncthreads();
    return A;
}

template <bool WIDE, bool TABLE, bool F16>
__device__ __forceinline__ void crop_normalize_pixels(const unsigned char* __restrict__ frame, int H, int W, const CropAffine& A, int S,
                                                      const float (&lut)[3][256], const int2* tabx, const int2* taby,
                                                      void* __restrict__ out_, unsigned char* __restrict__ raw) {
    float* __restrict__ out = static_cast<float*>(out_);
    const int d = blockIdx.y, t = threadIdx.x;
    const int npix = S * S, pix0 = blockIdx.x * (256 * kPX * kNB);
    const int yfirst = pix0 / S;
    const size_t total = (size_t)H * W * 3;
#pragma unroll 1
    for (int kb = 0; kb < kNB; ++kb) {
        const int idx0 = pix0 + kb * (256 * kPX) + t;
        if (idx0 - t >= npix) break;
        // phase 1: taps
        int tap[kPX][4][3], wgt[kPX][4];
#pragma unroll
        for (int k = 0; k < kPX; ++k) {
            const int idx = min(idx0 + k * 256, npix - 1);     // a tail lane recomputes the last pixel and never stores it
            const int y = idx / S, x = idx - y * S;
            const int2 cxf = TABLE ? tabx[x] : A.col(x, W), cyf = TABLE ? taby[y - yfirst] : A.row(y, H);
            const int sx = cxf.x, fx = cxf.y, sy = cyf.x, fy = cyf.y;
            const bool y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H;
            const bool x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W;
            wgt[k][0] = (y0 && x0) ? __mul24(32 - fx, 32 - fy) * 32 : 0;      // a zero weight == a zero (border) pixel
            wgt[k][1] = (y0 && x1) ? __mul24(fx, 32 - fy) * 32 : 0;
            wgt[k][2] = (y1 && x0) ? __mul24(32 - fx, fy) * 32 : 0;
            wgt[k][3] = (y1 && x1) ? __mul24(fx, fy) * 32 : 0;
            const int cy0 = min(max(sy, 0), H - 1), cy1 = min(max(sy + 1, 0), H - 1);
            const int cx0 = min(max(sx, 0), W - 1), cx1 = min(max(sx + 1, 0), W - 1);
            load_tap_pair<WIDE>(frame, total, W, cy0, cx0, cx1, tap[k][0], tap[k][1]);
            load_tap_pair<WIDE>(frame, total, W, cy1, cx0, cx1, tap[k][2], tap[k][3]);
        }
        // phase 2: fixed-point blend, table look-up, stores (256 contiguous bytes per wave and colour plane)
#pragma unroll
        for (int k = 0; k < kPX; ++k) {
            const int idx = idx0 + k * 256;
            if (idx < npix) {
                float r[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int v = (__mul24(tap[k][0][c], wgt[k][0]) + __mul24(tap[k][1][c], wgt[k][1]) + __mul24(tap[k][2][c], wgt[k][2]) +
                             __mul24(tap[k][3][c], wgt[k][3]) + (1 << 14)) >> 15;   // taps < 2^8, weights <= 2^15
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                    if (raw) raw[((size_t)d * npix + idx) * 3 + c] = (unsigned char)v;
                    r[c] = lut[c][v];
                    if (!F16) out[(size_t)(d * 3 + c) * npix + idx] = r[c];
                }
                if (F16) store_nhwc8(out_, (size_t)d * npix + idx, r);
            }
        }
    }
}

template <bool WIDE, bool TABLE, bool F16>
__global__ void __launch_bounds__(256) crop_normalize_kernel(const unsigned char* __restrict__ frame, int H, int W,
                                                              const float* __restrict__ bboxes, float scale, int S,
                                                              void* __restrict__ out, unsigned char* __restrict__ raw,
                                                              float* __restrict__ bbox_scale,
                                                              float* __restrict__ bbox_center,
                                                              const int* __restrict__ frame_of, size_t frame_stride, int nframes) {
    __shared__ float lut[3][256];
    __shared__ int2 tabx[TABLE ? kTabX : 1], taby[TABLE ? kTabY : 1];
    // batched: crop d is cut from frame frame_of[d] of a slab of equal-sized frames.  The index comes from caller memory the host
    // side cannot check without a synchronisation: a stale / negative / too large value is clamped into the slab (a wrong crop,
    // never an out-of-bounds read); spec_amd.preprocess.crop_detections_batch rejects it while the index is still on the host
    if (frame_of) frame += (size_t)min((unsigned)max(frame_of[blockIdx.y], 0), (unsigned)(nframes - 1)) * frame_stride;
    const CropAffine A = crop_normalize_prologue<TABLE>(H, W, bboxes, scale, S, bbox_scale, bbox_center, lut, tabx, taby);
    crop_normalize_pixels<WIDE, TABLE, F16>(frame, H, W, A, S, lut, tabx, taby, out, raw);
}

template <bool WIDE, bool TABLE, bool F16>
static void crop_normalize_go(dim3 grid, hipStream_t st, const unsigned char* frame, int H, int W, const float* bboxes, float scale,
                              int S, void* out, unsigned char* raw, float* bbox_scale, float* bbox_center, const int* frame_of,
                              size_t frame_stride, int nframes) {
    hipLaunchKernelGGL((crop_normalize_kernel<WIDE, TABLE, F16>), grid, dim3(256), 0, st, frame, H, W, bboxes, scale, S, out, raw, bbox_scale,
                       bbox_center, frame_of, frame_stride, nframes);
}

int launch_crop_normalize(const unsigned char* frame, int H, int W, const float* bboxes, int n, float scale, int S,
                          void* out, unsigned char* raw, float* bbox_scale, float* bbox_center, const LaunchCtx& ctx,
                          const int* frame_of, int nframes, bool f16) {
    // algorithmic HBM bytes: every frame once + every output once (the 4 taps x 3 channels of a pixel come through L2)
    ProfScope ps(ctx, f16 ? "crop_normalize_f16" : "crop_normalize", 0.0,
                 (double)H * W * 3 * (frame_of ? nframes : 1) + (double)n * S * S * ((f16 ? 16.0 : 12.0) + (raw ? 3.0 : 0.0)));
    if (crop_frame_too_large(H, W)) return (int)hipErrorInvalidValue;
    const bool wide = crop_wide(H, W), table = S <= kTabX;
    auto go = f16 ? (wide ? (table ? crop_normalize_go<true, true, true> : crop_normalize_go<true, false, true>)
                          : (table ? crop_normalize_go<false, true, true> : crop_normalize_go<false, false, true>))
                  : (wide ? (table ? crop_normalize_go<true, true, false> : crop_normalize_go<true, false, false>)
                          : (table ? crop_normalize_go<false, true, false> : crop_normalize_go<false, false, false>));
    if (frame_of && nframes < 1) return (int)hipErrorInvalidValue;
    go(crop_grid(S, n), ctx.stream, frame, H, W, bboxes, scale, S, out, raw, bbox_scale, bbox_center, frame_of, (size_t)H * W * 3, nframes);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Evaluation-dataset crop (spec/dataset/cam_dataset.py:253-287,367-377: rgb_processing -> pare `crop` -> ToTensor ->
// Normalize).  PARE / SPIN `crop(img, center, scale, res)` copies the integer box [ul, br) (200*scale pixels around the
// centre, zero outside the frame) and scales it to res x res with cv2.resize (INTER_LINEAR on a float64 array: half-pixel
// centres, replicated border, float coefficients, double accumulation); rgb_processing clips to [0, 255], converts to
// float32 / 255 and the dataset normalises with the ImageNet mean / std.  The integer boxes come from the host (the
// reference computes them with a 3x3 float64 inverse; spec_amd/preprocess.py restates that), everything per pixel runs here.
// cv::resize's source index / fraction of destination index i along an axis of n source pixels (clamped to the box)
__device__ __forceinline__ void resize_coord(int i, double scale, int n, int& s0, float& f) {
    f = (float)(((double)i + 0.5) * scale - 0.5);
    s0 = (int)floorf(f);
    f -= (float)s0;
    if (s0 < 0) { f = 0.f; s0 = 0; }
    if (s0 >= n - 1) { f = 0.f; s0 = n - 1; }
}

struct ResizeBox { int ulx, uly, bw, bh; double scale_x, scale_y; };

// crop d = blockIdx.y: the box, cv::resize's scales and the coordinate tables (the coordinates are separable: S columns + this
// workgroup's few rows, once); crop_resize_pixels begins with the barrier that publishes them, so that the frame record a ragged
// kernel reads in between is in flight meanwhile.  An empty box (br <= ul) is all zeros to the reference: the workgroup writes
// its pixels' Normalize(0) here and the caller returns on `false` - a decision per crop, so the whole workgroup takes it
template <bool TABLE, bool F16>
__device__ __forceinline__ bool crop_resize_prologue(const int* __restrict__ boxes, int S, void* __restrict__ out_, ResizeBox& b,
                                                     int* txs, int* tys, float* txf, float* tyf) {
    float* __restrict__ out = static_cast<float*>(out_);
    const int d = blockIdx.y, t = threadIdx.x;
    const int npix = S * S, pix0 = blockIdx.x * (256 * kPX * kNB);     // same mapping as the demo crop
    b.ulx = boxes[d * 4 + 0]; b.uly = boxes[d * 4 + 1];
    b.bw = boxes[d * 4 + 2] - b.ulx; b.bh = boxes[d * 4 + 3] - b.uly;
    if (b.bw <= 0 || b.bh <= 0) {
        for (int i = pix0 + t; i < min(pix0 + 256 * kPX * kNB, npix); i += 256) {
            float r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                r[c] = normalize_unit(0.0f, c);
                if (!F16) out[(size_t)(d * 3 + c) * npix + i] = r[c];
            }
            if (F16) store_nhwc8(out_, (size_t)d * npix + i, r);
        }
        return false;
    }
    // cv::resize INTER_LINEAR: fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx, clamped to the box
    b.scale_x = (double)b.bw / (double)S; b.scale_y = (double)b.bh / (double)S;
    if (TABLE) {
        const int yfirst = pix0 / S, ylast = min(pix0 + 256 * kPX * kNB - 1, npix - 1) / S;
        for (int i = t; i < S; i += 256) resize_coord(i, b.scale_x, b.bw, txs[i], txf[i]);
        for (int i = t; i <= ylast - yfirst; i += 256) resize_coord(yfirst + i, b.scale_y, b.bh, tys[i], tyf[i]);
    }
    return true;
}

template <bool WIDE, bool TABLE, bool F16>
__device__ __forceinline__ void crop_resize_pixels(const unsigned char* __restrict__ frame, int H, int W, const ResizeBox& b, int S,
                                                   const int* txs, const int* tys, const float* txf, const float* tyf,
                                                   void* __restrict__ out_) {
    if (TABLE) __syncthreads();     // the tables of crop_resize_prologue
    float* __restrict__ out = static_cast<float*>(out_);
    const int d = blockIdx.y, t = threadIdx.x;
    const int npix = S * S, pix0 = blockIdx.x * (256 * kPX * kNB);
    const int yfirst = pix0 / S;
    const size_t total = (size_t)H * W * 3;
#pragma unroll 1
    for (int kb = 0; kb < kNB; ++kb) {
        const int idx0 = pix0 + kb * (256 * kPX) + t;
        if (idx0 - t >= npix) break;
        // phase 1: the 4 taps x 3 channels of kPX pixels
        int tap[kPX][4][3];
        bool in[kPX][4];
        float cf[kPX][2];     // fx, fy
#pragma unroll
        for (int k = 0; k < kPX; ++k) {
            const int idx = min(idx0 + k * 256, npix - 1);
            const int dy = idx / S, dx = idx - dy * S;
            int sx, sy;
            float fx, fy;
            if (TABLE) { sx = txs[dx]; fx = txf[dx]; sy = tys[dy - yfirst]; fy = tyf[dy - yfirst]; }
            else { resize_coord(dx, b.scale_x, b.bw, sx, fx); resize_coord(dy, b.scale_y, b.bh, sy, fy); }
            const int sx1 = sx + 1 < b.bw ? sx + 1 : sx, sy1 = sy + 1 < b.bh ? sy + 1 : sy;
            cf[k][0] = fx; cf[k][1] = fy;
            // box pixel -> frame pixel (zero where the box leaves the frame)
            const int iy0 = b.uly + sy, iy1 = b.uly + sy1, ix0 = b.ulx + sx, ix1 = b.ulx + sx1;
            const bool vy0 = (unsigned)iy0 < (unsigned)H, vy1 = (unsigned)iy1 < (unsigned)H;
            const bool vx0 = (unsigned)ix0 < (unsigned)W, vx1 = (unsigned)ix1 < (unsigned)W;
            in[k][0] = vy0 && vx0; in[k][1] = vy0 && vx1; in[k][2] = vy1 && vx0; in[k][3] = vy1 && vx1;
            const int cx0 = min(max(ix0, 0), W - 1), cx1 = min(max(ix1, 0), W - 1);
            load_tap_pair<WIDE>(frame, total, W, min(max(iy0, 0), H - 1), cx0, cx1, tap[k][0], tap[k][1]);
            load_tap_pair<WIDE>(frame, total, W, min(max(iy1, 0), H - 1), cx0, cx1, tap[k][2], tap[k][3]);
        }
        // phase 2: float64 blend exactly as cv::resize orders it, clip, / 255, Normalize, store
#pragma unroll
        for (int k = 0; k < kPX; ++k) {
            const int idx = idx0 + k * 256;
            if (idx < npix) {
                const double a0 = (double)(1.f - cf[k][0]), a1 = (double)cf[k][0], b0 = (double)(1.f - cf[k][1]), b1 = (double)cf[k][1];
                float r[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double p00 = in[k][0] ? (double)tap[k][0][c] : 0.0, p01 = in[k][1] ? (double)tap[k][1][c] : 0.0;
                    const double p10 = in[k][2] ? (double)tap[k][2][c] : 0.0, p11 = in[k][3] ? (double)tap[k][3][c] : 0.0;
                    // separate multiplies and adds (no fma contraction): the reference rounds each product
                    const double r0 = __dadd_rn(__dmul_rn(p00, a0), __dmul_rn(p01, a1));     // horizontal pass
                    const double r1 = __dadd_rn(__dmul_rn(p10, a0), __dmul_rn(p11, a1));
                    double v = __dadd_rn(__dmul_rn(r0, b0), __dmul_rn(r1, b1));             // vertical pass
                    v = fmin(255.0, fmax(0.0, v));                                          // rgb_processing: pn = 1, clip
                    r[c] = normalize_unit((float)v / 255.0f, c);                            // astype('float32') / 255.0, Normalize
                    if (!F16) out[(size_t)(d * 3 + c) * npix + idx] = r[c];
                }
                if (F16) store_nhwc8(out_, (size_t)d * npix + idx, r);
            }
        }
    }
}

template <bool WIDE, bool TABLE, bool F16>
__global__ void __launch_bounds__(256) crop_resize_normalize_kernel(const unsigned char* __restrict__ frame, int H, int W,
                                                                     const int* __restrict__ boxes, int S,
                                                                     void* __restrict__ out) {
    __shared__ int txs[TABLE ? kTabX : 1], tys[TABLE ? kTabY : 1];
    __shared__ float txf[TABLE ? kTabX : 1], tyf[TABLE ? kTabY : 1];
    ResizeBox b;
    if (!crop_resize_prologue<TABLE, F16>(boxes, S, out, b, txs, tys, txf, tyf)) return;
    crop_resize_pixels<WIDE, TABLE, F16>(frame, H, W, b, S, txs, tys, txf, tyf, out);
}

template <bool WIDE, bool TABLE, bool F16>
static void crop_resize_go(dim3 grid, hipStream_t st, const unsigned char* frame, int H, int W, const int* boxes, int S, void* out) {
    hipLaunchKernelGGL((crop_resize_normalize_kernel<WIDE, TABLE, F16>), grid, dim3(256), 0, st, frame, H, W, boxes, S, out);
}

int launch_crop_resize_normalize(const unsigned char* frame, int H, int W, const int* boxes, int n, int S, void* out,
                                 const LaunchCtx& ctx, bool f16) {
    ProfScope ps(ctx, f16 ? "crop_resize_normalize_f16" : "crop_resize_normalize", 0.0,
                 (double)H * W * 3 + (double)n * S * S * (f16 ? 16.0 : 12.0));
    if (crop_frame_too_large(H, W)) return (int)hipErrorInvalidValue;
    const bool wide = crop_wide(H, W), table = S <= kTabX;
    auto go = f16 ? (wide ? (table ? crop_resize_go<true, true, true> : crop_resize_go<true, false, true>)
                          : (table ? crop_resize_go<false, true, true> : crop_resize_go<false, false, true>))
                  : (wide ? (table ? crop_resize_go<true, true, false> : crop_resize_go<true, false, false>)
                          : (table ? crop_resize_go<false, true, false> : crop_resize_go<false, false, false>));
    go(crop_grid(S, n), ctx.stream, frame, H, W, boxes, S, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The two crops from frames of DIFFERENT sizes in one launch (the per-sample loop of EvalDataset.batch, the per-frame loop of
// SPECTester.run_on_image_folder): the frames lie in one uint8 slab, crop d (blockIdx.y) reads frame_of[d] - clamped into
// [0, nframes) like the equal-size batch - and from that its frame's record (CropFrame: byte offset, H, W) out of a device
// table, then calls the crop's prologue and per-pixel path - the functions the kernels above call, so there is one statement of
// the arithmetic, the work mapping, the tables and the stores - on frames + offset with that H and W.  WIDE is decided per crop
// (a slab mixes a 1 x 1 frame with a 1080p one); a workgroup serves one crop, so the branch is wave-uniform and each side
// keeps its taps back to back.  The 8-byte tap load clamps against its own frame's `total`, so it never leaves the frame,
// hence never the slab; frames start at any byte offset (the load is an unaligned memcpy).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ CropFrame ragged_frame(const CropFrame* __restrict__ tab, const int* __restrict__ frame_of, int d, int nframes) {
    return tab[min((unsigned)max(frame_of[d], 0), (unsigned)(nframes - 1))];
}

template <bool TABLE, bool F16>
__global__ void __launch_bounds__(256) crop_normalize_ragged_kernel(const unsigned char* __restrict__ frames,
                                                                     const CropFrame* __restrict__ tab, int nframes,
                                                                     const int* __restrict__ frame_of,
                                                                     const float* __restrict__ bboxes, float scale, int S,
                                                                     void* __restrict__ out, unsigned char* __restrict__ raw,
                                                                     float* __restrict__ bbox_scale, float* __restrict__ bbox_center) {
    __shared__ float lut[3][256];
    __shared__ int2 tabx[TABLE ? kTabX : 1], taby[TABLE ? kTabY : 1];
    const CropFrame fr = ragged_frame(tab, frame_of, blockIdx.y, nframes);
    const CropAffine A = crop_normalize_prologue<TABLE>(fr.H, fr.W, bboxes, scale, S, bbox_scale, bbox_center, lut, tabx, taby);
    if (crop_wide(fr.H, fr.W)) crop_normalize_pixels<true, TABLE, F16>(frames + fr.off, fr.H, fr.W, A, S, lut, tabx, taby, out, raw);
    else crop_normalize_pixels<false, TABLE, F16>(frames + fr.off, fr.H, fr.W, A, S, lut, tabx, taby, out, raw);
}

int launch_crop_normalize_ragged(const unsigned char* frames, const CropFrame* tab, int nframes, double slab_bytes, const int* frame_of,
                                 const float* bboxes, int n, float scale, int S, void* out, unsigned char* raw, float* bbox_scale,
                                 float* bbox_center, const LaunchCtx& ctx, bool f16) {
    // algorithmic HBM bytes: the slab once + every output once
    ProfScope ps(ctx, f16 ? "crop_normalize_ragged_f16" : "crop_normalize_ragged", 0.0,
                 slab_bytes + (double)n * S * S * ((f16 ? 16.0 : 12.0) + (raw ? 3.0 : 0.0)));
    const bool table = S <= kTabX;
    auto k = f16 ? (table ? crop_normalize_ragged_kernel<true, true> : crop_normalize_ragged_kernel<false, true>)
                 : (table ? crop_normalize_ragged_kernel<true, false> : crop_normalize_ragged_kernel<false, false>);
    hipLaunchKernelGGL(k, crop_grid(S, n), dim3(256), 0, ctx.stream, frames, tab, nframes, frame_of, bboxes, scale, S, out, raw, bbox_scale,
                       bbox_center);
    return (int)hipGetLastError();
}

template <bool TABLE, bool F16>
__global__ void __launch_bounds__(256) crop_resize_normalize_ragged_kernel(const unsigned char* __restrict__ frames,
                                                                            const CropFrame* __restrict__ tab, int nframes,
                                                                            const int* __restrict__ frame_of,
                                                                            const int* __restrict__ boxes, int S, void* __restrict__ out) {
    __shared__ int txs[TABLE ? kTabX : 1], tys[TABLE ? kTabY : 1];
    __shared__ float txf[TABLE ? kTabX : 1], tyf[TABLE ? kTabY : 1];
    ResizeBox b;
    if (!crop_resize_prologue<TABLE, F16>(boxes, S, out, b, txs, tys, txf, tyf)) return;     // an empty box reads no frame: before the frame table
    const CropFrame fr = ragged_frame(tab, frame_of, blockIdx.y, nframes);
    if (crop_wide(fr.H, fr.W)) crop_resize_pixels<true, TABLE, F16>(frames + fr.off, fr.H, fr.W, b, S, txs, tys, txf, tyf, out);
    else crop_resize_pixels<false, TABLE, F16>(frames + fr.off, fr.H, fr.W, b, S, txs, tys, txf, tyf, out);
}

int launch_crop_resize_normalize_ragged(const unsigned char* frames, const CropFrame* tab, int nframes, double slab_bytes,
                                        const int* frame_of, const int* boxes, int n, int S, void* out, const LaunchCtx& ctx, bool f16) {
    ProfScope ps(ctx, f16 ? "crop_resize_normalize_ragged_f16" : "crop_resize_normalize_ragged", 0.0,
                 slab_bytes + (double)n * S * S * (f16 ? 16.0 : 12.0));
    const bool table = S <= kTabX;
    auto k = f16 ? (table ? crop_resize_normalize_ragged_kernel<true, true> : crop_resize_normalize_ragged_kernel<false, true>)
                 : (table ? crop_resize_normalize_ragged_kernel<true, false> : crop_resize_normalize_ragged_kernel<false, false>);
    hipLaunchKernelGGL(k, crop_grid(S, n), dim3(256), 0, ctx.stream, frames, tab, nframes, frame_of, boxes, S, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// CamCalib frame transform (camcalib/pano_dataset.py:156-162): torchvision Resize(600) on a PIL image =
// Pillow's separable triangle-filter resample (support grows with the down-scale factor, 22-bit fixed-point
// coefficients, horizontal pass -> uint8 -> vertical pass -> uint8), then ToTensor + Normalize.
// The coefficient tables are built on the host exactly like Pillow's precompute_coeffs /
// normalize_coeffs_8bpc (double precision, C truncation) - pillow_coeffs() - and the kernel evaluates
// both passes per output pixel in integer arithmetic, so the result is bit-identical to Pillow's.
// ------------------------------------------------------------------------------------------------
constexpr int PIL_BITS = 32 - 8 - 2;

// -> ksize; bounds[2*i] = first tap, bounds[2*i+1] = tap count, kk[i*ksize + t] = fixed-point weight
int pillow_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> k(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < ksize; ++x) k[x] = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = 0; x < ksize; ++x)
            kk[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PIL_BITS)) : (int)(0.5 + k[x] * (1 << PIL_BITS));
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

// The pieces of the resample that resize_normalize_kernel and the ragged batch kernels below share (one statement of the filter):
// a pass's accumulator -> the uint8 value Pillow stores (clip8)
__device__ __forceinline__ int pil_clip8(int acc) {
    const int v = acc >> PIL_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// horizontal pass of ONE pixel: `row` = the source row at the first tap, k = the xcnt fixed-point weights -> uint8 RGB
__device__ __forceinline__ void pil_hpass(const unsigned char* __restrict__ row, int xcnt, const int* __restrict__ k, int (&v)[3]) {
    int h[3] = {1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1)};
    for (int x = 0; x < xcnt; ++x) {
        const int w = k[x];
        h[0] += row[3 * x + 0] * w; h[1] += row[3 * x + 1] * w; h[2] += row[3 * x + 2] * w;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = pil_clip8(h[c]);                 // the uint8 image between the two passes
}

template <bool F16>
__global__ void __launch_bounds__(256) resize_normalize_kernel(const unsigned char* __restrict__ frame, int H, int W, int OH,
                                                                int OW, const int* __restrict__ hb, const int* __restrict__ hk,
                                                                int ksh, const int* __restrict__ vb,
                                                                const int* __restrict__ vk, int ksv,
                                                                void* __restrict__ out_, unsigned char* __restrict__ raw) {
    float* __restrict__ out = static_cast<float*>(out_);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= OH * OW) return;
    const int oy = idx / OW, ox = idx - oy * OW;
    const int xmin = hb[2 * ox], xcnt = hb[2 * ox + 1], ymin = vb[2 * oy], ycnt = vb[2 * oy + 1];
    int acc[3] = {1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1)};
    for (int y = 0; y < ycnt; ++y) {
        int v[3];
        pil_hpass(frame + ((size_t)(ymin + y) * W + xmin) * 3, xcnt, hk + (size_t)ox * ksh, v);
        const int wv = vk[(size_t)oy * ksv + y];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += v[c] * wv;
    }
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = pil_clip8(acc[c]);
        if (raw) raw[(size_t)idx * 3 + c] = (unsigned char)v;
        r[c] = to_tensor_normalize(v, c);
        if (!F16) out[((size_t)c * OH + oy) * OW + ox] = r[c];
    }
    if (F16) store_nhwc8(out_, (size_t)idx, r);
}

int launch_resize_normalize(const unsigned char* frame, int H, int W, int OH, int OW, const int* hb, const int* hk, int ksh,
                            const int* vb, const int* vk, int ksv, void* out, unsigned char* raw, const LaunchCtx& ctx, bool f16) {
    ProfScope ps(ctx, f16 ? "resize_normalize_f16" : "resize_normalize", 0.0,
                 (double)H * W * 3 + (double)OH * OW * ((f16 ? 16.0 : 12.0) + (raw ? 3.0 : 0.0)));
    hipLaunchKernelGGL(f16 ? resize_normalize_kernel<true> : resize_normalize_kernel<false>, dim3((OH * OW + 255) / 256), dim3(256), 0,
                       ctx.stream, frame, H, W, OH, OW, hb, hk, ksh, vb, vk, ksv, out, raw);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// CamCalib validation batch (camcalib/pano_dataset.py:184-220 Resize(min_size, max_size) per frame, :223-306 collator /
// to_image_list): n frames of DIFFERENT sizes -> one (n, 3, Hmax, Wmax) tensor, frame f resampled to (OH_f, OW_f) in the
// top-left corner, exact zeros elsewhere.  Two launches whatever n is: the horizontal pass of every frame into a uint8
// workspace (H_f x OW_f x 3: what Pillow holds between its passes), then ONE sweep over the whole output that runs the
// vertical pass + ToTensor + Normalize inside a frame's region and stores 0.0f outside it - every output element is
// written exactly once.  A frame whose target size is its own size is converted, not resampled (torchvision's resize
// returns the image unchanged).  Same device functions, hence the same bits, as resize_normalize_kernel.
// `tab` holds the per-frame records (RaggedFrame, kRaggedRec ints each) followed by the coefficient tables they index.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ragged_hpass_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ tab,
                                                            unsigned char* __restrict__ tmp) {
    const RaggedFrame& fr = reinterpret_cast<const RaggedFrame*>(tab)[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (!fr.resample || idx >= fr.H * fr.OW) return;
    const int y = idx / fr.OW, ox = idx - y * fr.OW;
    const int* hb = tab + fr.hb;
    const int xmin = hb[2 * ox], xcnt = hb[2 * ox + 1];
    int v[3];
    pil_hpass(frames + fr.src_off + ((size_t)y * fr.W + xmin) * 3, xcnt, tab + fr.hk + (size_t)ox * fr.ksh, v);
    unsigned char* q = tmp + fr.tmp_off + (size_t)idx * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = (unsigned char)v[c];
}

template <bool F16>
__global__ void __launch_bounds__(256) ragged_vpass_pad_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ tab,
                                                                const unsigned char* __restrict__ tmp, int Hmax, int Wmax,
                                                                void* __restrict__ out_) {
    const RaggedFrame& fr = reinterpret_cast<const RaggedFrame*>(tab)[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Hmax * Wmax) return;
    const int oy = idx / Wmax, ox = idx - oy * Wmax;
    float r[3] = {0.0f, 0.0f, 0.0f};                                     // to_image_list: zeros in normalised space
    if (oy < fr.OH && ox < fr.OW) {
        int v[3];
        if (fr.resample) {
            const int ymin = tab[fr.vb + 2 * oy], ycnt = tab[fr.vb + 2 * oy + 1];
            const int* vk = tab + fr.vk + (size_t)oy * fr.ksv;
            int acc[3] = {1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1)};
            const unsigned char* col = tmp + fr.tmp_off + ((size_t)ymin * fr.OW + ox) * 3;
            for (int y = 0; y < ycnt; ++y) {
                const int wv = vk[y];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += col[(size_t)y * fr.OW * 3 + c] * wv;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = pil_clip8(acc[c]);
        } else {
            const unsigned char* q = frames + fr.src_off + ((size_t)oy * fr.W + ox) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = q[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = to_tensor_normalize(v[c], c);
    }
    const size_t plane = (size_t)Hmax * Wmax;
    if (F16) {                                                           // padding: 16 bytes of zero (+0 halves)
        store_nhwc8(out_, (size_t)blockIdx.y * plane + idx, r);
    } else {
        float* __restrict__ out = static_cast<float*>(out_);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((size_t)blockIdx.y * 3 + c) * plane + idx] = r[c];
    }
}

int launch_resize_normalize_ragged(const unsigned char* frames, const int* tab, unsigned char* tmp, int n, int max_hpass_px,
                                   int Hmax, int Wmax, double src_bytes, double tmp_bytes, void* out, const LaunchCtx& ctx, bool f16) {
    // algorithmic HBM bytes: every frame once, the uint8 rows between the passes written and read once, every output element once
    if (max_hpass_px > 0) {
        ProfScope ps(ctx, "ragged_hpass", 0.0, src_bytes + tmp_bytes);
        hipLaunchKernelGGL(ragged_hpass_kernel, dim3((max_hpass_px + 255) / 256, n), dim3(256), 0, ctx.stream, frames, tab, tmp);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    ProfScope ps(ctx, f16 ? "ragged_vpass_pad_f16" : "ragged_vpass_pad", 0.0, (f16 ? 16.0 : 12.0) * n * Hmax * Wmax + tmp_bytes);
    hipLaunchKernelGGL(f16 ? ragged_vpass_pad_kernel<true> : ragged_vpass_pad_kernel<false>, dim3((Hmax * Wmax + 255) / 256, n), dim3(256),
                       0, ctx.stream, frames, tab, tmp, Hmax, Wmax, out);
    return (int)hipGetLastError();
}

}  // namespace specmi
