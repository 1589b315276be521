// draw.hip - 2D keypoint skeletons painted into uint8 frames on the device: what the reference
// hands to pare.utils.vis_utils.draw_skeleton / cv2.circle / cv2.line in spec/utils/renderer_cam.py:167-168 before the mesh is
// laid over the frame, for all frames of a call in one launch.  pare and cv2 are not vendored: coverage, bone table and colours
// are THIS PROJECT'S OWN CONTRACT, exact and reproducible bit for bit (tests/draw_ref.py restates it in NumPy); cv2's look -
// its antialiasing, its rounding of thick lines - is not claimed.
//
// THE DRAWING CONTRACT
// Keypoints: kp (Mtot, J, D) fp32, D = 2 (x, y) or 3 (x, y, confidence), in pixels of the detection's frame.  Keypoint k is
//   VISIBLE when x and y are finite, D == 2 or conf > thr (an fp32 compare: a NaN confidence is invisible), and xi = (int)x and
//   yi = (int)y (truncation toward zero, numpy's astype(int)) both lie in [-16383, 16383] - evaluated as |x| < 16384 and
//   |y| < 16384 in fp32, which is the same set and never casts a value an int cannot hold.  Coordinates are NOT clipped;
//   a primitive with an invisible keypoint is not drawn.
// Order: painter's.  For the detections det0, det0 + 1, ... of a frame in turn: the J discs in joint order, then the NB bones
//   in table order.  A later primitive overwrites an earlier one.
// Pixel (px, py) = (column, row) is taken at its integer coordinate, as the int-cast keypoints are: there is no + 0.5.
// Disc of integer radius r (0 .. 64) at (xi, yi): covers the pixel iff (px - xi)^2 + (py - yi)^2 <= r^2.
// Bone (a, b) of integer thickness t (1 .. 64), drawn iff both ends are visible: covers the pixel iff its distance to the
//   closed segment is at most t / 2 (round caps) - exactly, in integers, with d = b - a, L = d.d, p = pixel - a, s = p.d,
//   c = p x d = p.x d.y - p.y d.x:
//     L == 0 or s <= 0:  4 p.p <= t^2                 (nearest point: a)
//     s >= L:            4 (p - d).(p - d) <= t^2     (nearest point: b)
//     otherwise:         c^2 <= floor(t^2 L / 4)      (distance to the line = |c| / sqrt(L); c^2 is an integer, so the floor
//                                                      changes nothing)
//   A disc is the bone (a, a) with t^2 replaced by 4 r^2: one coverage function serves both.
// Integer range: frame sides are at most 8192 (kDrawMaxSide), so 0 <= px, py <= 8191, and |xi|, |yi| <= 16383.  Then every
//   component of p and of p - d (= pixel - b) is at most 8191 + 16383 = 24574 < 2^15 in magnitude and every component of d at
//   most 32766 < 2^15.  So L <= 2 * 32766^2 < 2^31; |s| and |c| are sums of two products below 2^15 * 2^15: |s|, |c| < 2^31 and
//   c^2 < 2^62; 4 p.p <= 8 * 24574^2 < 2^33; t^2 L <= 4096 * 2^31 = 2^43.  Signed 64-bit holds every term.
// Colours: uint8 RGB, overwritten - no blending, no antialiasing.  Discs take joint_rgb, bone b takes bone_rgb[b & 1].
// Untouched: uncovered pixels, row padding and every slab byte outside the frames' rectangles.  The kernel reads no pixel.
//
// MAPPING.  One 256-thread workgroup per 32 x 32 pixel tile of one frame; the tiles of all frames are numbered back to back
// and a workgroup finds its frame by bisecting the tile prefix of the record table (uniform: scalar loads), as the other ragged
// kernels do.  A frame without detections has no tiles.  The frame's count * (J + NB) primitives are visited in painter's order in
// chunks of 256, one per thread: the thread reads its one or two keypoints, converts them once, and tests the primitive's
// bounding box (grown by r, or by ceil(t / 2)) against the tile; the survivors are compacted IN ORDER into LDS with one wave64
// ballot per wavefront and the four wavefronts' counts.  Every thread then walks the chunk's survivors in order for its four
// pixels (rows ty, ty + 8, ty + 16, ty + 24 of column tx) keeping the last hit, and at the end writes three bytes where
// something hit: no atomics, no workspace, no memset, and nothing that depends on scheduling.  A tile whose every chunk is
// culled away touches no memory.
#include "specmi_internal.h"

namespace specmi {

constexpr int kDrawTile = 32;

// keypoint k of D floats -> visible?, with its int-cast position
__device__ __forceinline__ bool draw_keypoint(const float* __restrict__ k, int D, float thr, int& xi, int& yi) {
    const float x = k[0], y = k[1];
    bool vis = fabsf(x) < 16384.f && fabsf(y) < 16384.f;        // false for a NaN or an infinity
    if (D == 3) vis = vis && k[2] > thr;                        // false for a NaN
    xi = vis ? (int)x : 0;
    yi = vis ? (int)y : 0;
    return vis;
}

// the contract's coverage test: p = pixel - a, d = b - a, L = d.d, t2 = t^2 (a disc: d = 0, t2 = 4 r^2)
__device__ __forceinline__ bool draw_covers(int px, int py, int dx, int dy, long long L, long long t2) {
    const long long pp = (long long)px * px + (long long)py * py;
    const long long s = (long long)px * dx + (long long)py * dy;
    if (L == 0 || s <= 0) return 4 * pp <= t2;
    if (s >= L) {
        const long long qx = px - dx, qy = py - dy;
        return 4 * (qx * qx + qy * qy) <= t2;
    }
    const long long c = (long long)px * dy - (long long)py * dx;
    return c * c <= (t2 * L) / 4;
}

__global__ void __launch_bounds__(256) draw_skeletons_kernel(DrawArgs a) {
    __shared__ int s_ax[256], s_ay[256], s_dx[256], s_dy[256], s_kind[256];
    __shared__ int s_count[4];
    // frames[f].tile0 <= blockIdx.x < frames[f + 1].tile0: the LAST frame whose first tile is not beyond this one has tiles
    const int b = blockIdx.x;
    int lo = 0, hi = a.nframes;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.frames[mid].tile0 <= b) lo = mid; else hi = mid;
    }
    const DrawFrame fr = a.frames[lo];
    const int tile = b - fr.tile0;
    const int x0 = (tile % fr.tiles_x) * kDrawTile, y0 = (tile / fr.tiles_x) * kDrawTile;
    const int x1 = min(x0 + kDrawTile - 1, fr.W - 1), y1 = min(y0 + kDrawTile - 1, fr.H - 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px = x0 + (tid & 31), py = y0 + (tid >> 5);
    const int P = a.J + a.NB, nprim = fr.count * P;             // the host keeps Mtot * (J + NB) below 2^31
    const long long disc_t2 = 4LL * a.radius * a.radius, bone_t2 = (long long)a.thickness * a.thickness;
    const int grow_bone = (a.thickness + 1) / 2;
    int hit[4] = {-1, -1, -1, -1};
    for (int q0 = 0; q0 < nprim; q0 += 256) {                   // uniform trip count: the barriers below are safe
        const int q = q0 + tid;
        bool keep = false;
        int ax = 0, ay = 0, bx = 0, by = 0, kind = 0;
        if (q < nprim) {
            const int det = q / P, r = q - det * P;
            const float* k = a.kp + (size_t)(fr.det0 + det) * a.J * a.D;
            if (r < a.J) {
                keep = draw_keypoint(k + (size_t)r * a.D, a.D, a.thr, ax, ay);
                bx = ax; by = ay;
            } else {
                const int bone = r - a.J;
                kind = 1 + (bone & 1);
                const bool va = draw_keypoint(k + (size_t)a.bones[2 * bone] * a.D, a.D, a.thr, ax, ay);
                const bool vb = draw_keypoint(k + (size_t)a.bones[2 * bone + 1] * a.D, a.D, a.thr, bx, by);
                keep = va && vb;
            }
            const int e = kind ? grow_bone : a.radius;
            keep = keep && min(ax, bx) - e <= x1 && max(ax, bx) + e >= x0 && min(ay, by) - e <= y1 && max(ay, by) + e >= y0;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_count[wave] = __popcll(m);
        __syncthreads();
        int first = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int n = s_count[w];
            if (w < wave) first += n;
            total += n;
        }
        if (keep) {
            const int i = first + __popcll(m & ((1ull << lane) - 1ull));
            s_ax[i] = ax; s_ay[i] = ay; s_dx[i] = bx - ax; s_dy[i] = by - ay; s_kind[i] = kind;
        }
        __syncthreads();
        for (int i = 0; i < total; ++i) {                       // every lane reads the same word: an LDS broadcast
            const int dx = s_dx[i], dy = s_dy[i], kind = s_kind[i];
            const int rx = px - s_ax[i], ry = py - s_ay[i];
            const long long L = (long long)dx * dx + (long long)dy * dy, t2 = kind ? bone_t2 : disc_t2;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (draw_covers(rx, ry + 8 * r, dx, dy, L, t2)) hit[r] = kind;
        }
        __syncthreads();                                        // the next chunk overwrites s_count and the survivors
    }
    if (px > x1) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = py + 8 * r;
        if (y > y1 || hit[r] < 0) continue;
        const unsigned c = hit[r] == 0 ? a.rgb[0] : (hit[r] == 1 ? a.rgb[1] : a.rgb[2]);
        unsigned char* o = a.slab + fr.off + (long long)y * fr.pitch + 3 * px;
        o[0] = (unsigned char)c; o[1] = (unsigned char)(c >> 8); o[2] = (unsigned char)(c >> 16);
    }
}

int draw_frame_tiles(int H, int W, int* tiles_x) {
    *tiles_x = (W + kDrawTile - 1) / kDrawTile;
    return *tiles_x * ((H + kDrawTile - 1) / kDrawTile);
}

int launch_draw_skeletons(const DrawArgs& a, int total_tiles, double kp_bytes, double px, const LaunchCtx& ctx) {
    if (total_tiles == 0) return 0;                             // no frame has a detection
    // reads: each tile the keypoints of its frame's primitives (kp_bytes, summed by the caller); writes: at most the frames' pixels
    ProfScope ps(ctx, "draw_skeletons", 0.0, kp_bytes + px * 3);
    hipLaunchKernelGGL(draw_skeletons_kernel, dim3((unsigned)total_tiles), dim3(256), 0, ctx.stream, a);
    return (int)hipGetLastError();
}

}  // namespace specmi
