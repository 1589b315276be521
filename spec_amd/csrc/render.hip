// render.hip - the demo's mesh overlay and side view rasterised on the device: what the reference
// hands to pyrender / OpenGL in spec/utils/renderer_cam.py:44-144 (render_overlay_image), for the M detections of a frame in
// one call.  The geometry is the reference's; the RASTERISATION CONTRACT below is this project's own and is exact (coverage and
// visibility are reproducible bit for bit, tests/render_ref.py restates them); the SHADING is declared as this project's own -
// it does not claim pyrender's metallic-roughness look.
//
// Vertex stage (fp32, no contraction, in this order) - renderer_cam.py:74-117 composed:
//   p = (vx, -vy, -vz)                               the 180 degree turn about x (:78-80)
//   side view: p = (-p.z, p.y, p.x)                  the 270 degree turn about y (:82-85)
//   q = R^T p,  q.k = (R[0][k] p.x + R[1][k] p.y) + R[2][k] p.z
//   X = q.x + t.x,  Y = t.y - q.y,  Z = t.z - q.z     pose = [R | R t'] with t' = (-t.x, t.y, t.z) (:74, :109-112), inverted
//                                                     as R^T p - t' (R is a rotation), then z forward and y down
//   x_s = (fx X) / Z + cx,  y_s = (fy Y) / Z + cy     pyrender's IntrinsicsCamera; pixel (i, j) has its centre at (j + 0.5, i + 0.5)
//   snapped = rint(256 x_s), rint(256 y_s)            1/256 pixel, round half to even, int32
// A vertex with Z <= 0.05 (pyrender's default znear), or |x_s| or |y_s| at or beyond 2^20 pixels, or a NaN anywhere, is DROPPED
// (snapped x = y = INT32_MIN), and a triangle with a dropped vertex is not drawn: THERE IS NO CLIPPING - a triangle that
// straddles the near plane disappears whole.  There is no far plane for meshes.  A face that names a vertex outside [0, V) is
// ignored altogether.
//
// Coverage: int64 edge functions on the snapped coordinates, evaluated at the pixel centre (256 j + 128, 256 i + 128):
//   orient(a, b, c) = (b.x - a.x)(c.y - a.y) - (b.y - a.y)(c.x - a.x),  A = orient(v0, v1, v2),
//   E0 = orient(v1, v2, P), E1 = orient(v2, v0, P), E2 = orient(v0, v1, P)      (E0 + E1 + E2 = A; |.| < 2^60)
// With y down, an outward-wound (counter-clockwise seen from outside) closed mesh shows the faces with A < 0: A == 0 is never
// drawn, A > 0 only with culling off; the signs are then flipped so that inside means E_i >= 0.  A pixel is covered when every
// E_i > 0, or E_i == 0 on an edge whose inward gradient (dE_i/dx, dE_i/dy) has dE_i/dx > 0 (a left edge) or dE_i/dx == 0 and
// dE_i/dy > 0 (a top edge): the top-left rule, so two triangles that share an edge cover each pixel on it exactly once.
//
// Visibility: w_i = (float)E_i / (float)A, 1/z = (w0 / z0 + w1 / z1) + w2 / z2, z = 1 / that - perspective-correct depth in
// fp32 with correctly rounded divisions - and ONE 64-bit atomicMin per covered pixel on float_bits(z) << 32 | (m F + f): the
// nearest surface wins, a tie goes to the lower id, and the result does not depend on the order the triangles arrive in.
// One wavefront per triangle, the 64 lanes striding the bounding box in 8 x 8 pixel blocks (kRenderThreadPerTriangle: one
// thread per triangle walking its bounding box pixel by pixel - the same bits, kept for the comparison in scripts/bench_aux.py).
//
// Normals: the area-weighted face normal (v1 - v0) x (v2 - v0) (twice the area, model space) of EVERY face with valid indices,
// quantised per component to int32 at a scale of 2^28 per metre^2 (rint, each contribution clamped to +-2^30) and atomicAdd-ed
// to the face's three vertices: integer addition is order-free, so the sums are deterministic.  32 incident faces of 0.05 m^2
// each add up to at most 32 x 0.1 x 2^28 = 0.86e9 < 2^31; beyond that budget a sum wraps (a wrong shade, never a wrong address).
//
// Resolve, one thread per pixel: the barycentrics are recomputed from the stored id, made perspective-correct
// (b_i = (w_i / z_i) z), the unit vertex normals interpolated and normalised, and
//   shade = min(1, 0.3 + 0.7 max(0, n . l)),  byte = rint(255 rgb shade)
// with l = world +z: the four directional lights of renderer_cam.py:119-131 all shine along world -z (their poses only
// translate), 0.3 is its ambient term.  n . l is evaluated in model space (-n.z; side view: n.x), which is the same number as
// in the camera frame.  Opaque composite over the frame; an uncovered pixel is the frame's byte; in side view the background is
// black.  The side view's ground plane is NOT rasterised but intersected per pixel: the reference's get_checkerboard_plane lives
// in the un-vendored pare package, so this plane is this project's own - the horizontal plane through the lowest vertex
// (renderer_cam.py:105, in camera-centred world coordinates: min over all meshes of p.y - (R t'_m).y), unlit, a checker of 0.5 m
// tiles in two greys (bytes 140 / 191) anchored to mesh 0's world origin, drawn where 0.05 < depth < 100 (pyrender's znear /
// zfar) and nearer than the mesh.  Per pixel, fp32 in this order: g = ((j + 0.5 - cx) / fx, -((i + 0.5 - cy) / fy), -1),
// d = R g (row k: (R[k][0] g.x + R[k][1] g.y) + R[k][2] g.z), s = y_plane / d.y, hit = o_0 + s d with o_0 = R t'_0,
// tile parity = (floor(hit.x / 0.5) + floor(hit.z / 0.5)) & 1.
//
// MANY VIEWS IN ONE CALL (specmi_render_views).  A view is what one specmi_render_meshes call
// draws - one camera, one output rectangle, a contiguous range of the call's meshes - and every view is drawn by the SAME device
// functions (vertex_one, raster_one, resolve_one) from a RenderArgs put together out of its record, so the contract above holds
// per view, bit for bit.  One launch per stage whatever the number of views: the vertex stage over all (pair, vertex), the raster
// stage over all (pair, triangle), a pair being a (view, mesh of that view) enumerated on the host; the resolve stage over all
// views' pixels.  One memset covers every key plane, one the per-view lowest-vertex words.  A view without meshes has no key plane
// and no pairs: its resolve copies the frame (black in side view).
// Normal sums are computed once per PAIR, not once per mesh: a mesh named by an overlay and a side view is summed twice, into
// two copies, by the raster launch that visits both pairs anyway - integer sums, the same bits, and no pass that would have to
// find the distinct meshes first.
// Pixel -> view: the views' pixels are numbered back to back and a resolve thread finds its view in the prefix table
// (px_prefix): a bisection for the wavefront's first pixel (uniform, about log2(nviews) scalar loads) and a walk forward for
// the lanes behind a boundary.  No thread is idle for views of unequal size - the only waste is the last workgroup's tail, under
// 256 threads per call, where a 2-D grid (view x tiles of the largest view) would idle (max - mean) / max of its workgroups.
#include <climits>

#include "specmi_internal.h"

#pragma clang fp contract(off)

namespace specmi {

constexpr float kZNear = 0.05f, kZFar = 100.f;
constexpr float kScreenLimit = 1048576.f;          // 2^20 pixels
constexpr int kDropped = INT_MIN;
constexpr float kNormalScale = 268435456.f;        // 2^28 per metre^2 of (v1 - v0) x (v2 - v0)
constexpr float kNormalClamp = 1073741824.f;       // 2^30
constexpr float kTile = 0.5f;
constexpr int kGreyEven = 140, kGreyOdd = 191;

// float <-> int such that the ints order as the floats do (atomicMin on the lowest y)
__device__ __forceinline__ int float_ordered(float f) { const int b = __float_as_int(f); return b >= 0 ? b : b ^ 0x7fffffff; }
__device__ __forceinline__ float ordered_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__device__ __forceinline__ long long orient(int ax, int ay, int bx, int by, int cx, int cy) {
    return (long long)(bx - (long long)ax) * (cy - (long long)ay) - (long long)(by - (long long)ay) * (cx - (long long)ax);
}

// o = R t' with t' = (-t.x, t.y, t.z): row k of R
__device__ __forceinline__ float cam_origin(const float* R, const float* t, int k) {
    return (R[3 * k] * -t[0] + R[3 * k + 1] * t[1]) + R[3 * k + 2] * t[2];
}

// vertex i = m V + v of the call `a` -> its height for the lowest-vertex search as an ordered int (INT_MAX without the ground plane)
__device__ __forceinline__ int vertex_one(const RenderArgs& a, int i) {
    const int m = i / a.V;
    const float* v = a.vertices + (size_t)i * 3;
    const float* t = a.cam_t + (size_t)m * 3;
    const float* R = a.R;
    float px = v[0], py = -v[1], pz = -v[2];
    if (a.side) { const float x = px; px = -pz; pz = x; }
    const float qx = (R[0] * px + R[3] * py) + R[6] * pz;
    const float qy = (R[1] * px + R[4] * py) + R[7] * pz;
    const float qz = (R[2] * px + R[5] * py) + R[8] * pz;
    const float X = qx + t[0], Y = t[1] - qy, Z = t[2] - qz;
    const float xs = (a.fx * X) / Z + a.cx, ys = (a.fy * Y) / Z + a.cy;
    const bool keep = Z > kZNear && fabsf(xs) < kScreenLimit && fabsf(ys) < kScreenLimit;     // false for a NaN
    int* s = a.sws + (size_t)i * 3;
    s[0] = keep ? (int)rintf(xs * 256.f) : kDropped;
    s[1] = keep ? (int)rintf(ys * 256.f) : kDropped;
    s[2] = __float_as_int(Z);
    if (a.screen) { int* u = a.screen + (size_t)i * 3; u[0] = s[0]; u[1] = s[1]; u[2] = s[2]; }
    int* n = a.normals + (size_t)i * 3;
    n[0] = 0; n[1] = 0; n[2] = 0;
    return a.ground ? float_ordered(py - cam_origin(R, t, 1)) : INT_MAX;
}

__device__ __forceinline__ int wave_min(int low) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) low = min(low, __shfl_xor(low, o));
    return low;
}

__global__ void __launch_bounds__(256) render_vertex_kernel(RenderArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int low = INT_MAX;
    if (i < a.M * a.V) low = vertex_one(a, i);
    if (a.ground) {
        low = wave_min(low);
        if ((threadIdx.x & 63) == 0 && low != INT_MAX) atomicMin(a.lowest, low);
    }
}

// What raster and resolve both need of a triangle: its snapped vertices, depths, the orientation sign and the positive area
struct ScreenTri { int x[3], y[3]; float z[3]; long long sgn, A; };

__device__ __forceinline__ bool load_tri(const RenderArgs& a, int m, const int idx[3], ScreenTri& t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int* s = a.sws + ((size_t)m * a.V + idx[k]) * 3;
        t.x[k] = s[0]; t.y[k] = s[1]; t.z[k] = __int_as_float(s[2]);
        if (t.x[k] == kDropped) return false;
    }
    const long long A = orient(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
    if (A == 0 || (A > 0 && a.cull)) return false;
    t.sgn = A < 0 ? -1 : 1;
    t.A = A * t.sgn;
    return true;
}

// the three edge functions at the pixel centre, inside >= 0
__device__ __forceinline__ void edge_values(const ScreenTri& t, int px, int py, long long E[3]) {
    const int X = 256 * px + 128, Y = 256 * py + 128;
    E[0] = t.sgn * orient(t.x[1], t.y[1], t.x[2], t.y[2], X, Y);
    E[1] = t.sgn * orient(t.x[2], t.y[2], t.x[0], t.y[0], X, Y);
    E[2] = t.sgn * orient(t.x[0], t.y[0], t.x[1], t.y[1], X, Y);
}

// edge k runs from vertex k+1 to vertex k+2; its value grows by (-sgn dy, sgn dx) per unit of (x, y)
__device__ __forceinline__ bool covers(const ScreenTri& t, const long long E[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (E[k] > 0) continue;
        if (E[k] < 0) return false;
        const int b = (k + 1) % 3, c = (k + 2) % 3;
        const long long gx = -t.sgn * ((long long)t.y[c] - t.y[b]), gy = t.sgn * ((long long)t.x[c] - t.x[b]);
        if (!(gx > 0 || (gx == 0 && gy > 0))) return false;
    }
    return true;
}

__device__ __forceinline__ float depth_at(const ScreenTri& t, const long long E[3], float w[3]) {
    const float fA = (float)t.A;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = (float)E[k] / fA;
    const float s = (w[0] / t.z[0] + w[1] / t.z[1]) + w[2] / t.z[2];
    return 1.f / s;
}

// Triangle f of mesh m of the call `a`, as lane `lane` of the BW x BW lanes that share it sees it.
// BW = 8: one wavefront per triangle, lanes striding the bounding box in 8 x 8 blocks; BW = 1: one thread per triangle
template <int BW>
__device__ __forceinline__ void raster_one(const RenderArgs& a, int m, int f, int lane) {
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = a.faces[(size_t)f * 3 + k];
        if ((unsigned)idx[k] >= (unsigned)a.V) return;
    }
    if (lane == 0) {
        const float* v0 = a.vertices + ((size_t)m * a.V + idx[0]) * 3;
        const float* v1 = a.vertices + ((size_t)m * a.V + idx[1]) * 3;
        const float* v2 = a.vertices + ((size_t)m * a.V + idx[2]) * 3;
        const float ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2];
        const float bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
        const float n[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int q = (int)fminf(fmaxf(rintf(n[c] * kNormalScale), -kNormalClamp), kNormalClamp);     // a NaN becomes -2^30
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(a.normals + ((size_t)m * a.V + idx[k]) * 3 + c, q);
        }
    }
    ScreenTri t;
    if (!load_tri(a, m, idx, t)) return;
    // pixels whose centre 256 j + 128 lies inside the bounding box, clamped to the frame
    const int xmin = min(t.x[0], min(t.x[1], t.x[2])), xmax = max(t.x[0], max(t.x[1], t.x[2]));
    const int ymin = min(t.y[0], min(t.y[1], t.y[2])), ymax = max(t.y[0], max(t.y[1], t.y[2]));
    const int j0 = max((xmin - 128 + 255) >> 8, 0), j1 = min((xmax - 128) >> 8, a.W - 1);
    const int i0 = max((ymin - 128 + 255) >> 8, 0), i1 = min((ymax - 128) >> 8, a.H - 1);
    if (j0 > j1 || i0 > i1) return;
    const int nbx = (j1 - j0) / BW + 1, nby = (i1 - i0) / BW + 1;
    const unsigned id = (unsigned)(m * a.F + f);
    for (int by = 0; by < nby; ++by) {
        const int py = i0 + by * BW + lane / BW;
        if (py > i1) continue;
        for (int bx = 0; bx < nbx; ++bx) {
            const int px = j0 + bx * BW + lane % BW;
            if (px > j1) continue;
            long long E[3];
            edge_values(t, px, py, E);
            if (!covers(t, E)) continue;
            float w[3];
            const float z = depth_at(t, E, w);
            atomicMin(a.keys + (size_t)py * a.W + px, ((unsigned long long)__float_as_uint(z) << 32) | id);
        }
    }
}

template <int BW>
__global__ void __launch_bounds__(256) render_raster_kernel(RenderArgs a) {
    constexpr int L = BW * BW;
    const long long gt = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long tri = gt / L;
    if (tri >= (long long)a.M * a.F) return;
    raster_one<BW>(a, (int)(tri / a.F), (int)(tri % a.F), (int)(gt % L));
}

// pixel p = i W + j of the call `a`
__device__ __forceinline__ void resolve_one(const RenderArgs& a, int p) {
    const int i = p / a.W, j = p % a.W;
    const unsigned long long key = a.keys ? a.keys[p] : ~0ull;      // no key plane: a view without meshes
    const bool hit = key != ~0ull;
    int id = hit ? (int)(unsigned)(key & 0xffffffffull) : -1;
    float z = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
    int grey = -1;
    if (a.ground) {
        const float* R = a.R;
        const float gx = ((float)j + 0.5f - a.cx) / a.fx, gy = -(((float)i + 0.5f - a.cy) / a.fy), gz = -1.f;
        const float dx = (R[0] * gx + R[1] * gy) + R[2] * gz;
        const float dy = (R[3] * gx + R[4] * gy) + R[5] * gz;
        const float dz = (R[6] * gx + R[7] * gy) + R[8] * gz;
        const float s = ordered_float(*a.lowest) / dy;
        if (s > kZNear && s < kZFar && (!hit || s < z)) {      // false for a NaN (dy == 0 and the plane through the camera)
            const float hx = cam_origin(R, a.cam_t, 0) + s * dx, hz = cam_origin(R, a.cam_t, 2) + s * dz;
            grey = (((int)floorf(hx / kTile) + (int)floorf(hz / kTile)) & 1) ? kGreyOdd : kGreyEven;
            id = -2;
            z = s;
        }
    }
    unsigned char c[3];
    if (grey >= 0) {
        c[0] = c[1] = c[2] = (unsigned char)grey;
    } else if (hit) {
        const int m = id / a.F, f = id % a.F;
        int idx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) idx[k] = a.faces[(size_t)f * 3 + k];
        ScreenTri t;
        (void)load_tri(a, m, idx, t);          // the raster kernel drew it: it loads
        long long E[3];
        edge_values(t, j, i, E);
        float w[3];
        const float zz = depth_at(t, E, w);
        float n[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int* q = a.normals + ((size_t)m * a.V + idx[k]) * 3;
            const float x = (float)q[0], y = (float)q[1], u = (float)q[2];
            const float len = sqrtf((x * x + y * y) + u * u);
            const float b = len > 0.f ? ((w[k] / t.z[k]) * zz) / len : 0.f;
            n[0] += b * x; n[1] += b * y; n[2] += b * u;
        }
        const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const float ndl = len > 0.f ? (a.side ? n[0] : -n[2]) / len : 0.f;
        const float shade = fminf(1.f, 0.3f + 0.7f * fmaxf(0.f, ndl));
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (unsigned char)(int)rintf((255.f * a.rgb[k]) * shade);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = a.side ? (unsigned char)0 : a.frame[(size_t)i * a.in_pitch + j * 3 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out[(size_t)i * a.out_pitch + j * 3 + k] = c[k];
    if (a.id_map) a.id_map[p] = id;
    if (a.depth) a.depth[p] = z;
}

__global__ void __launch_bounds__(256) render_resolve_kernel(RenderArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.H * a.W) return;
    resolve_one(a, p);
}

size_t render_ws_layout(int M, int V, int H, int W, size_t off[4]) {
    const auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    off[0] = 0;                                                   // keys: 8 bytes per pixel
    off[1] = off[0] + up((size_t)H * W * 8);                      // snapped vertices: x, y int32, z float bits
    off[2] = off[1] + up((size_t)M * V * 12);                     // normal sums: 3 int32 per vertex
    off[3] = off[2] + up((size_t)M * V * 12);                     // the lowest y, as an ordered int
    return off[3] + 256;
}

int launch_render(const RenderArgs& a, bool thread_per_triangle, const LaunchCtx& ctx) {
    const double px = (double)a.H * a.W, mv = (double)a.M * a.V, mf = (double)a.M * a.F;
    hipError_t e = hipMemsetAsync(a.keys, 0xFF, (size_t)a.H * a.W * 8, ctx.stream);
    if (e != hipSuccess) return (int)e;
    if (a.ground && (e = hipMemsetAsync(a.lowest, 0x7F, 4, ctx.stream)) != hipSuccess) return (int)e;
    {   // reads the vertices, writes the snapped vertices (+ the caller's copy) and zeroes the normal sums
        ProfScope ps(ctx, "render_vertex", 0.0, mv * (12 + 12 + 12 + (a.screen ? 12 : 0)));
        hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)((a.M * a.V + 255) / 256)), dim3(256), 0, ctx.stream, a);
    }
    {   // per triangle: 3 indices, 3 vertices and 3 snapped vertices read, 9 normal adds; the key traffic depends on the scene
        ProfScope ps(ctx, thread_per_triangle ? "render_raster_thread" : "render_raster_wave", 0.0, mf * (12 + 36 + 36 + 36) + px * 8);
        const long long threads = (long long)a.M * a.F * (thread_per_triangle ? 1 : 64);
        const unsigned blocks = (unsigned)((threads + 255) / 256);
        if (thread_per_triangle) hipLaunchKernelGGL(render_raster_kernel<1>, dim3(blocks), dim3(256), 0, ctx.stream, a);
        else hipLaunchKernelGGL(render_raster_kernel<8>, dim3(blocks), dim3(256), 0, ctx.stream, a);
    }
    {   // per pixel: the key, the frame byte triple in, the byte triple out (+ id and depth)
        ProfScope ps(ctx, "render_resolve", 0.0, px * (8 + (a.side ? 0 : 3) + 3 + (a.id_map ? 4 : 0) + (a.depth ? 4 : 0)));
        hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((a.H * a.W + 255) / 256)), dim3(256), 0, ctx.stream, a);
    }
    return (int)hipGetLastError();
}

// ---- many views in one call (specmi_render_views) --------------------------------------------------------------------------
// The RenderArgs of view `view`, put together from its record: the device functions above then see one specmi_render_meshes call
__device__ __forceinline__ RenderArgs view_args(const RenderViewsArgs& b, int view) {
    const RenderView& r = b.views[view];
    const size_t pv = (size_t)r.pair0 * b.V * 3;
    RenderArgs a;
    a.vertices = b.vertices + (size_t)r.mesh0 * b.V * 3;
    a.faces = b.faces;
    a.cam_t = b.cam_t + (size_t)r.mesh0 * 3;
    a.R = r.R;
    a.frame = b.in_slab + r.in_off;
    a.fx = r.fx; a.fy = r.fy; a.cx = r.cx; a.cy = r.cy;
    a.rgb[0] = b.rgb[0]; a.rgb[1] = b.rgb[1]; a.rgb[2] = b.rgb[2];
    a.M = r.count; a.V = b.V; a.F = b.F; a.H = r.H; a.W = r.W; a.side = r.side; a.ground = r.ground; a.cull = r.cull;
    a.in_pitch = r.in_pitch; a.out_pitch = r.out_pitch;
    a.keys = r.key0 >= 0 ? b.keys + r.key0 : nullptr;
    a.sws = b.sws + pv;
    a.normals = b.normals + pv;
    a.lowest = b.lowest + view;
    a.out = b.out_slab + r.out_off;
    a.id_map = b.id_map ? b.id_map + r.px0 : nullptr;
    a.depth = b.depth ? b.depth + r.px0 : nullptr;
    a.screen = b.screen ? b.screen + pv : nullptr;
    return a;
}

__global__ void __launch_bounds__(256) render_views_vertex_kernel(RenderViewsArgs b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int low = INT_MAX, view = -1;
    if (i < b.npairs * b.V) {
        view = b.pair_view[i / b.V];
        low = vertex_one(view_args(b, view), i - b.views[view].pair0 * b.V);
    }
    // the lowest vertex of each view: one atomic per wavefront where the whole wavefront serves one view, one per lane where it
    // straddles two pairs (min is order-free: the same word either way)
    const int first = __shfl(view, 0);
    if (__all(view == first)) {
        low = wave_min(low);
        if ((threadIdx.x & 63) == 0 && low != INT_MAX) atomicMin(b.lowest + first, low);
    } else if (low != INT_MAX) {
        atomicMin(b.lowest + view, low);
    }
}

template <int BW>
__global__ void __launch_bounds__(256) render_views_raster_kernel(RenderViewsArgs b) {
    constexpr int L = BW * BW;
    const long long gt = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long tri = gt / L;
    if (tri >= (long long)b.npairs * b.F) return;
    const int pair = (int)(tri / b.F);
    const int view = b.pair_view[pair];
    raster_one<BW>(view_args(b, view), pair - b.views[view].pair0, (int)(tri % b.F), (int)(gt % L));
}

__global__ void __launch_bounds__(256) render_views_resolve_kernel(RenderViewsArgs b) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= b.total_px) return;
    // px_prefix[v] <= p < px_prefix[v + 1]: bisect for the wavefront's first pixel (uniform), then walk to the lane's own view
    const int p0 = __builtin_amdgcn_readfirstlane(p);
    int lo = 0, hi = b.nviews;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b.px_prefix[mid] <= p0) lo = mid; else hi = mid;
    }
    int view = lo;
    while (p >= b.px_prefix[view + 1]) ++view;
    resolve_one(view_args(b, view), p - b.px_prefix[view]);
}

size_t render_views_ws_layout(long long keys, long long pairs, int V, int nviews, size_t off[4]) {
    const auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    off[0] = 0;                                                   // keys: 8 bytes per pixel of every view that has meshes
    off[1] = off[0] + up((size_t)keys * 8);                       // snapped vertices per (view, mesh) pair
    off[2] = off[1] + up((size_t)pairs * V * 12);                 // normal sums per pair
    off[3] = off[2] + up((size_t)pairs * V * 12);                 // the lowest y of every view
    return off[3] + up((size_t)nviews * 4);
}

int launch_render_views(const RenderViewsArgs& b, long long keys, bool any_ground, bool thread_per_triangle, const LaunchCtx& ctx) {
    const double px = (double)b.total_px, mv = (double)b.npairs * b.V, mf = (double)b.npairs * b.F;
    hipError_t e;
    if (keys && (e = hipMemsetAsync(b.keys, 0xFF, (size_t)keys * 8, ctx.stream)) != hipSuccess) return (int)e;
    if (any_ground && (e = hipMemsetAsync(b.lowest, 0x7F, (size_t)b.nviews * 4, ctx.stream)) != hipSuccess) return (int)e;
    if (b.npairs) {
        {
            ProfScope ps(ctx, "render_views_vertex", 0.0, mv * (12 + 12 + 12 + (b.screen ? 12 : 0)));
            hipLaunchKernelGGL(render_views_vertex_kernel, dim3((unsigned)((b.npairs * b.V + 255) / 256)), dim3(256), 0, ctx.stream, b);
        }
        ProfScope ps(ctx, thread_per_triangle ? "render_views_raster_thread" : "render_views_raster_wave", 0.0, mf * (12 + 36 + 36 + 36) + (double)keys * 8);
        const long long threads = (long long)b.npairs * b.F * (thread_per_triangle ? 1 : 64);
        const unsigned blocks = (unsigned)((threads + 255) / 256);
        if (thread_per_triangle) hipLaunchKernelGGL(render_views_raster_kernel<1>, dim3(blocks), dim3(256), 0, ctx.stream, b);
        else hipLaunchKernelGGL(render_views_raster_kernel<8>, dim3(blocks), dim3(256), 0, ctx.stream, b);
    }
    {
        ProfScope ps(ctx, "render_views_resolve", 0.0, (double)keys * 8 + px * (3 + 3 + (b.id_map ? 4 : 0) + (b.depth ? 4 : 0)));
        hipLaunchKernelGGL(render_views_resolve_kernel, dim3((unsigned)((b.total_px + 255) / 256)), dim3(256), 0, ctx.stream, b);
    }
    return (int)hipGetLastError();
}

}  // namespace specmi
