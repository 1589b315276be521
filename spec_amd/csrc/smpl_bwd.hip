// smpl_bwd.hip - the vector-Jacobian product of smpl.hip (SMPL LBS + 49 joints + camera + projection) and of head.hip's
// rot6d -> rotation matrix (gfx950).
//
// specmi_smpl_backward is stateless: it first runs the three forward kernels of smpl.hip on its arguments (vertices, the 49
// joints, the camera translation, the fragment-ordered features and transforms), then walks them backwards:
//
//   1. smpl_joints_bwd_kernel (one workgroup per image): projection (division by z, K, R) -> joint gradients and the camera
//      translation's gradient -> g_cam; the 49 -> 54 scatter through joint_map (repeated entries add in joint order); the 9
//      regressed joints (J_extra^T) and the 21 picked joints go onto the vertices: gV = g_vertices + both, one dense pass.
//   2. smpl_skin_bwd_feat_kernel / smpl_skin_bwd_A_kernel (a wave = 32 images x a chunk of 2 vertex groups): the two
//      contractions over the vertices on the fp32 matrix cores.  Both recompute their half of the forward as smpl_skin_kernel
//      does (the blended transforms T for the first, v_posed for the second), form g_v_posed = T[:, :3]^T gV resp.
//      g_T = gV (x) [v_posed; 1] lane-locally on the accumulators, and feed those accumulators straight back as the B operand
//      of v_mfma_f32_32x32x2_f32: accumulator register r of a lane holds (image lane % 32, vertex 4 (lane / 32) + (r & 3) +
//      8 (r >> 2)), which is a valid K = 2 slice (k = lane / 32) - the contraction over the 32 vertices of a group is order
//      free, so step r contracts that pair of vertices and no transpose through LDS is needed.  The A operand is the body
//      model in the SAME fragment-ordered tables the forward reads (SmplDev::dirsT / wT), addressed by (vertex, feature)
//      instead of streamed: one 16-byte load serves four MFMAs (four feature rows 2 apart).
//   3. smpl_bwd_reduce_kernel: the chunks' partial slabs are summed in chunk order - the order depends on V alone, there are
//      no float atomics, every run gives the same bits.
//   4. smpl_chain_bwd_kernel (one wave per image, lane = joint): recomputes the kinematic chain as smpl_pose_kernel does and
//      walks the tree leaves to root; children push their parent's gradient through wave shuffles in joint order.
#include "specmi_internal.h"

namespace specmi {

namespace {

constexpr int IT = 32;                     // images per tile = columns of one MFMA (smpl.hip)
constexpr int KQ = SMPL_KQ;
constexpr int FEAT_TILE = KQ * 64 * 4;
constexpr int A_TILE = 12 * 3 * 64 * 4;
constexpr int NG = 2;                      // vertex groups (of 32) per chunk = one partial slab: fixes the summation order, so it is part of the arithmetic.
                                           // Fewer groups = more waves in flight but more slab traffic: 0.51 / 0.33 / 0.26 ms per call at 8 / 4 / 2, B = 256
constexpr int PART_ROWS = 256 + 12 * 32;   // rows of a partial slab: 256 feature rows (218 used) + 12 transform entries x 32 joint rows (24 used)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct JointBwdArgs {
    const float *j3d, *camt;                       // forward values (recomputed by this call)
    const float *cam, *R, *K, *bbox_scale, *bbox_center, *img_w, *img_h;
    const float *g_verts, *g_j3d, *g_j2d, *g_camt; // upstream, any may be null
    const float* J_extra; const int* extra_ids; const int* joint_map;
    float *gV, *gposed, *g_cam;                    // gV / gposed null: the body's gradients are not wanted
    int V, mode, normalize; float focal, img_res;
};

constexpr int JBT = 256;
__global__ void __launch_bounds__(JBT) smpl_joints_bwd_kernel(const JointBwdArgs a) {
    __shared__ float gX[49][3], gP[49][3], g54[54][3], gct[3];
    __shared__ int jm[49];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 49) {
        jm[t] = a.joint_map[t];
        const float X0 = a.j3d[(size_t)b * 147 + t * 3 + 0], X1 = a.j3d[(size_t)b * 147 + t * 3 + 1], X2 = a.j3d[(size_t)b * 147 + t * 3 + 2];
        float gx[3] = {0.f, 0.f, 0.f}, gp[3] = {0.f, 0.f, 0.f};
        if (a.g_j3d) {
#pragma unroll
            for (int i = 0; i < 3; ++i) gx[i] = a.g_j3d[(size_t)b * 147 + t * 3 + i];
        }
        if (a.g_j2d) {
            float Rm[9], Km[9];
            if (a.mode == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) { Rm[k] = a.R[(size_t)b * 9 + k]; Km[k] = a.K[(size_t)b * 9 + k]; }
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) { Rm[k] = (k % 4 == 0) ? 1.f : 0.f; Km[k] = 0.f; }
                Km[0] = a.focal; Km[4] = a.focal; Km[8] = 1.f;
            }
            float P[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) P[i] = Rm[i * 3 + 0] * X0 + Rm[i * 3 + 1] * X1 + Rm[i * 3 + 2] * X2 + a.camt[(size_t)b * 3 + i];
            float gu = a.g_j2d[(size_t)b * 98 + t * 2 + 0], gv = a.g_j2d[(size_t)b * 98 + t * 2 + 1];
            if (a.normalize) { gu = gu / (a.img_res / 2.0f); gv = gv / (a.img_res / 2.0f); }
            // (u, v) = K[:2] (P / z): the third homogeneous coordinate z / z is the constant 1
            const float g0 = Km[0] * gu + Km[3] * gv, g1 = Km[1] * gu + Km[4] * gv;
            const float iz = 1.0f / P[2];
            gp[0] = g0 * iz; gp[1] = g1 * iz; gp[2] = -(g0 * P[0] + g1 * P[1]) * iz * iz;
#pragma unroll
            for (int i = 0; i < 3; ++i) gx[i] += Rm[0 * 3 + i] * gp[0] + Rm[1 * 3 + i] * gp[1] + Rm[2 * 3 + i] * gp[2];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { gX[t][i] = gx[i]; gP[t][i] = gp[i]; }
    }
    __syncthreads();
    if (t < 3) {
        float s = a.g_camt ? a.g_camt[(size_t)b * 3 + t] : 0.f;
        for (int k = 0; k < 49; ++k) s += gP[k][t];
        gct[t] = s;
    } else if (t >= 64 && t < 64 + 162) {
        // the 49 -> 54 scatter: joint_map entries that repeat add in joint order
        const int i = t - 64, jj = i / 3, c = i % 3;
        float s = 0.f;
        for (int k = 0; k < 49; ++k)
            if (jm[k] == jj) s += gX[k][c];
        g54[jj][c] = s;
    }
    __syncthreads();
    if (t == 0 && a.g_cam) {
        const float s = a.cam[b * 3 + 0];
        float gs;
        if (a.mode == 0) {  // convert_pare_to_full_img_cam: every term is c / s
            const float f = a.K[(size_t)b * 9], bh = a.bbox_scale[b] * 200.0f, r = bh / 224.0f;
            const float tz = 2.0f * f / (r * 224.0f * s);
            const float cx = 2.0f * (a.bbox_center[b * 2 + 0] - (a.img_w[b] / 2.0f)) / (s * bh);
            const float cy = 2.0f * (a.bbox_center[b * 2 + 1] - (a.img_h[b] / 2.0f)) / (s * bh);
            gs = -(gct[0] * cx + gct[1] * cy + gct[2] * tz) / s;
        } else {            // convert_weak_perspective_to_perspective: tz = 2 f / (res s + 1e-9)
            const float den = a.img_res * s + 1e-9f;
            gs = -gct[2] * (2.0f * a.focal / den) * a.img_res / den;
        }
        a.g_cam[(size_t)b * 3 + 0] = gs; a.g_cam[(size_t)b * 3 + 1] = gct[0]; a.g_cam[(size_t)b * 3 + 2] = gct[1];
    }
    if (!a.gV) return;
    if (t < 72) a.gposed[(size_t)b * 72 + t] = g54[t / 3][t % 3];
    float* const gv = a.gV + (size_t)b * a.V * 3;
    const float* const up = a.g_verts ? a.g_verts + (size_t)b * a.V * 3 : nullptr;
    for (int v = t; v < a.V; v += JBT) {   // one vertex per lane: its 9 regressor weights are loaded once for the three coordinates
        float s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = up ? up[v * 3 + c] : 0.f;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const float w = a.J_extra[(size_t)e * a.V + v];
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = fmaf(w, g54[45 + e][c], s[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gv[v * 3 + c] = s[c];
    }
    __syncthreads();   // the dense pass is in memory for this workgroup: the picked vertices add onto it, in joint order
    if (t < 3)
        for (int k = 0; k < 21; ++k) gv[(size_t)a.extra_ids[k] * 3 + t] += g54[24 + k][t];
}

// gV of (image lane % 32 of the tile, the 16 vertices of this lane's accumulator slots in group g), zero past B / V
__device__ __forceinline__ void load_gv(const float* __restrict__ gV, int V, int B, int b, int g, int lane, f32x16 gv[3]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int v = g * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
        const bool ok = b < B && v < V;
        const float* p = gV + ((size_t)(ok ? b : 0) * V + (ok ? v : 0)) * 3;
        gv[0][r] = ok ? p[0] : 0.f; gv[1][r] = ok ? p[1] : 0.f; gv[2][r] = ok ? p[2] : 0.f;
    }
}

// partial slab row `row` of (chunk, tile): [row][image of the tile]
__device__ __forceinline__ void store_acc(float* __restrict__ slab, int row0, int lane, const f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) slab[(size_t)(row0 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2)) * IT + (lane & 31)] = acc[r];
}

// g_feat partials: rows 0..255 of the slab = feature k (pose features 0..206, betas 207..216, the template's constant 217)
__global__ void __launch_bounds__(64) smpl_skin_bwd_feat_kernel(const float* __restrict__ dirsT, const float* __restrict__ wT,
                                                                 const float* __restrict__ Afrag, const float* __restrict__ gV,
                                                                 float* __restrict__ part, int V, int B, int G) {
    const int lane = threadIdx.x, chunk = blockIdx.x, tile = blockIdx.y, tiles = gridDim.y;
    const int b = tile * IT + (lane & 31), h = lane >> 5, rho = lane & 31;
    const f32x4* __restrict__ aq = reinterpret_cast<const f32x4*>(Afrag + (size_t)tile * A_TILE) + lane;       // [entry][quad][64]
    f32x16 acc[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[s][q][r] = 0.f;
    // A operand row rho of accumulator (s, q) = feature 8 (16 s + rho / 2) + rho % 2 + 2 q: the four register elements of the
    // quad 16 s + rho / 2, half rho % 2 of the forward's table
    const bool on1 = 16 + (rho >> 1) < KQ;
    const int gend = min(G, (chunk + 1) * NG);
    for (int g = chunk * NG; g < gend; ++g) {
        f32x16 gv[3], gvp[3];
        load_gv(gV, V, B, b, g, lane, gv);
        const f32x4* __restrict__ wq = reinterpret_cast<const f32x4*>(wT + (size_t)g * 768) + lane;
        const f32x4 w0 = wq[0], w1 = wq[64], w2 = wq[128];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) gvp[c][r] = 0.f;
        // g_v_posed[c] = sum_row T[row][c] gV[row], T as the forward accumulates it
#pragma unroll
        for (int row = 0; row < 3; ++row) {
            f32x16 T[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
#pragma unroll
                for (int r = 0; r < 16; ++r) T[d][r] = 0.f;
                const f32x4 b0 = aq[((4 * row + d) * 3 + 0) * 64], b1 = aq[((4 * row + d) * 3 + 1) * 64], b2 = aq[((4 * row + d) * 3 + 2) * 64];
#pragma unroll
                for (int q = 0; q < 4; ++q) T[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[q], b0[q], T[d], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) T[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[q], b1[q], T[d], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) T[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[q], b2[q], T[d], 0, 0, 0);
            }
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) gvp[d][r] = fmaf(T[d][r], gv[row][r], gvp[d][r]);
        }
        const f32x4* __restrict__ dq = reinterpret_cast<const f32x4*>(dirsT + (size_t)g * 3 * FEAT_TILE);       // [coord][quad][64]
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int vl = 4 * h + (r & 3) + 8 * (r >> 2) + 32 * (rho & 1);      // the table's lane of (vertex, k % 2)
                const f32x4 d0 = dq[(size_t)(c * KQ + (rho >> 1)) * 64 + vl];
                f32x4 d1 = {0.f, 0.f, 0.f, 0.f};
                if (on1) d1 = dq[(size_t)(c * KQ + 16 + (rho >> 1)) * 64 + vl];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(d0[q], gvp[c][r], acc[0][q], 0, 0, 0);
                    acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(d1[q], gvp[c][r], acc[1][q], 0, 0, 0);
                }
            }
    }
    float* const slab = part + (size_t)(chunk * tiles + tile) * PART_ROWS * IT;
    // accumulator (s, q), row rho' -> feature 8 (16 s + rho' / 2) + rho' % 2 + 2 q
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = 4 * h + (r & 3) + 8 * (r >> 2);
                const int k = 8 * (16 * s + (rr >> 1)) + (rr & 1) + 2 * q;
                slab[(size_t)k * IT + (lane & 31)] = acc[s][q][r];
            }
}

// g_A partials: rows 256 + 32 e + joint of the slab, e = 4 r + c the entry of the 3 x 4 relative transform
__global__ void __launch_bounds__(64) smpl_skin_bwd_A_kernel(const float* __restrict__ dirsT, const float* __restrict__ wT,
                                                              const float* __restrict__ feat, const float* __restrict__ gV,
                                                              float* __restrict__ part, int V, int B, int G) {
    const int lane = threadIdx.x, chunk = blockIdx.x, tile = blockIdx.y, tiles = gridDim.y;
    const int b = tile * IT + (lane & 31), h = lane >> 5, rho = lane & 31;
    const f32x4* __restrict__ fq = reinterpret_cast<const f32x4*>(feat + (size_t)tile * FEAT_TILE) + lane;     // [quad][64]
    f32x16 acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[e][r] = 0.f;
    const int gend = min(G, (chunk + 1) * NG);
    for (int g = chunk * NG; g < gend; ++g) {
        // v_posed[vertex][image] per coordinate, as smpl_skin_kernel accumulates it
        const f32x4* __restrict__ dq = reinterpret_cast<const f32x4*>(dirsT + (size_t)g * 3 * FEAT_TILE) + lane;
        f32x16 vp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) vp[c][r] = 0.f;
        constexpr int PD = 3;
        f32x4 fb[PD], dd[3][PD];
#pragma unroll
        for (int i = 0; i < PD; ++i) {
            fb[i] = fq[i * 64];
#pragma unroll
            for (int k = 0; k < 3; ++k) dd[k][i] = dq[(k * KQ + i) * 64];
        }
#pragma unroll
        for (int s4 = 0; s4 < KQ; ++s4) {
            const int cur = s4 % PD;
            const f32x4 f = fb[cur];
            f32x4 av[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) av[k] = dd[k][cur];
            if (s4 + PD < KQ) {
                fb[cur] = fq[(s4 + PD) * 64];
#pragma unroll
                for (int k = 0; k < 3; ++k) dd[k][cur] = dq[(k * KQ + s4 + PD) * 64];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int k = 0; k < 3; ++k) vp[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[k][q], f[q], vp[k], 0, 0, 0);
        }
        f32x16 gv[3];
        load_gv(gV, V, B, b, g, lane, gv);
        // A operand row rho = joint: lbs weight of (this step's vertex, joint rho) out of the forward's table
        const float* __restrict__ wg = wT + (size_t)g * 768;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int vl = 4 * h + (r & 3) + 8 * (r >> 2);
            const float w = rho < 24 ? wg[frag_slot(rho, vl)] : 0.f;
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const int row = e >> 2, d = e & 3;
                const float gt = d < 3 ? gv[row][r] * vp[d < 3 ? d : 0][r] : gv[row][r];
                acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, gt, acc[e], 0, 0, 0);
            }
        }
    }
    float* const slab = part + (size_t)(chunk * tiles + tile) * PART_ROWS * IT;
#pragma unroll
    for (int e = 0; e < 12; ++e) store_acc(slab, 256 + 32 * e, lane, acc[e]);
}

// sum pass: chunk order, one thread per (tile, slab row, image) -> g_feat (B, 224), g_A (B, 24, 12)
__global__ void smpl_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ gfeat, float* __restrict__ gA, int nchunk,
                                       int tiles, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= tiles * PART_ROWS * IT) return;
    const int img = i % IT, row = (i / IT) % PART_ROWS, tile = i / (IT * PART_ROWS);
    const int b = tile * IT + img;
    if (b >= B) return;
    const bool isf = row < 224, isa = row >= 256 && ((row - 256) & 31) < 24;
    if (!isf && !isa) return;
    float s = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) s += part[(size_t)(ch * tiles + tile) * PART_ROWS * IT + (size_t)row * IT + img];
    if (isf) gfeat[(size_t)b * 224 + row] = s;
    else gA[((size_t)b * 24 + ((row - 256) & 31)) * 12 + ((row - 256) >> 5)] = s;
}

// b = image (blockIdx.x), j = lane = joint.  The forward half restates smpl_pose_kernel<false>.
__global__ void __launch_bounds__(64) smpl_chain_bwd_kernel(const float* __restrict__ rotmat, const float* __restrict__ betas,
                                                             const float* __restrict__ Jt, const float* __restrict__ Jd,
                                                             const int* __restrict__ parents, const float* __restrict__ gA,
                                                             const float* __restrict__ gfeat, const float* __restrict__ gposed,
                                                             float* __restrict__ g_rotmat, float* __restrict__ g_betas) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, j = threadIdx.x;
    const bool act = j < 24;
    const int jj = act ? j : 0;
    int par = (act && j > 0) ? parents[jj] : -1;
    int depth = 0;
    for (int pp = par; pp >= 0; pp = (pp > 0 ? parents[pp] : -1)) ++depth;
    int maxd = act ? depth : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) maxd = max(maxd, __shfl_xor(maxd, o, 64));

    float R[9], beta[10];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rotmat[((size_t)b * 24 + jj) * 9 + k];
#pragma unroll
    for (int l = 0; l < 10; ++l) beta[l] = betas[(size_t)b * 10 + l];
    float J[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = 0.f;
#pragma unroll
        for (int l = 0; l < 10; ++l) s = fmaf(beta[l], Jd[(jj * 3 + c) * 10 + l], s);
        J[c] = Jt[jj * 3 + c] + s;
    }
    const int src = par >= 0 ? par : 0;
    float rel[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float pj = __shfl(J[c], src, 64);
        rel[c] = (par >= 0) ? J[c] - pj : J[c];
    }
    float G[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[r * 4 + 0] = R[r * 3 + 0]; G[r * 4 + 1] = R[r * 3 + 1]; G[r * 4 + 2] = R[r * 3 + 2]; G[r * 4 + 3] = rel[r];
    }
    for (int d = 1; d <= maxd; ++d) {
        float P[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) P[e] = __shfl(G[e], src, 64);
        if (act && depth == d) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    G[r * 4 + c] = dot3(P[r * 4 + 0], R[0 * 3 + c], P[r * 4 + 1], R[1 * 3 + c], P[r * 4 + 2], R[2 * 3 + c]);
                G[r * 4 + 3] = dot3(P[r * 4 + 0], rel[0], P[r * 4 + 1], rel[1], P[r * 4 + 2], rel[2]) + P[r * 4 + 3];
            }
        }
    }

    // A_j = [G_r | G_t - G_r J], posed_j = G_t
    float gG[12], gJ[3], gR[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float gat = act ? gA[((size_t)b * 24 + jj) * 12 + r * 4 + 3] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gar = act ? gA[((size_t)b * 24 + jj) * 12 + r * 4 + c] : 0.f;
            gG[r * 4 + c] = gar - gat * J[c];
        }
        gG[r * 4 + 3] = gat + (act ? gposed[(size_t)b * 72 + jj * 3 + r] : 0.f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a0 = act ? gA[((size_t)b * 24 + jj) * 12 + 3] : 0.f, a1 = act ? gA[((size_t)b * 24 + jj) * 12 + 7] : 0.f,
                    a2 = act ? gA[((size_t)b * 24 + jj) * 12 + 11] : 0.f;
        gJ[c] = -dot3(G[0 * 4 + c], a0, G[1 * 4 + c], a1, G[2 * 4 + c], a2);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) gR[k] = 0.f;
    // leaves to root: level d's joints are complete once level d + 1 has pushed
    for (int d = maxd; d >= 1; --d) {
        float P[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) P[e] = __shfl(G[e], src, 64);
        const bool mine = act && depth == d;
        float cP[12], crel[3];
#pragma unroll
        for (int e = 0; e < 12; ++e) cP[e] = 0.f;
        crel[0] = crel[1] = crel[2] = 0.f;
        if (mine) {
            // G_j = [P_r R_j | P_r rel_j + P_t]
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gR[a * 3 + c] = dot3(P[0 * 4 + a], gG[0 * 4 + c], P[1 * 4 + a], gG[1 * 4 + c], P[2 * 4 + a], gG[2 * 4 + c]);
                crel[a] = dot3(P[0 * 4 + a], gG[0 * 4 + 3], P[1 * 4 + a], gG[1 * 4 + 3], P[2 * 4 + a], gG[2 * 4 + 3]);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    cP[r * 4 + a] = dot3(gG[r * 4 + 0], R[a * 3 + 0], gG[r * 4 + 1], R[a * 3 + 1], gG[r * 4 + 2], R[a * 3 + 2]) + gG[r * 4 + 3] * rel[a];
                cP[r * 4 + 3] = gG[r * 4 + 3];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) gJ[c] += crel[c];      // rel_j = J_j - J_parent
        }
        for (int k = 1; k < 24; ++k) {                          // children add onto their parent in joint order
            const int pk = __shfl(par, k, 64), dk = __shfl(depth, k, 64);
            if (dk != d) continue;                              // (the same for every lane)
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const float v = __shfl(cP[e], k, 64);
                if (j == pk) gG[e] += v;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = __shfl(crel[c], k, 64);
                if (j == pk) gJ[c] -= v;
            }
        }
    }
    if (j == 0) {   // G_0 = [R_0 | J_0]
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            gR[r * 3 + 0] = gG[r * 4 + 0]; gR[r * 3 + 1] = gG[r * 4 + 1]; gR[r * 3 + 2] = gG[r * 4 + 2];
            gJ[r] += gG[r * 4 + 3];
        }
    }
    if (g_rotmat && act) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float pf = j > 0 ? gfeat[(size_t)b * 224 + (jj - 1) * 9 + k] : 0.f;      // pose feature R_j - I
            g_rotmat[((size_t)b * 24 + j) * 9 + k] = gR[k] + pf;
        }
    }
    if (g_betas) {
#pragma unroll
        for (int l = 0; l < 10; ++l) {
            float s = 0.f;
            if (act) s = dot3(Jd[(jj * 3 + 0) * 10 + l], gJ[0], Jd[(jj * 3 + 1) * 10 + l], gJ[1], Jd[(jj * 3 + 2) * 10 + l], gJ[2]);
            s = wave_sum64(s);
            if (j == 0) g_betas[(size_t)b * 10 + l] = s + gfeat[(size_t)b * 224 + 207 + l];
        }
    }
}

// rot6d_joint alone (the regressor runs it inside head_final / the fused pose kernel): one lane per rotation, the same bits
__global__ void rot6d_fwd_kernel(const float* __restrict__ x6d, float* __restrict__ rot, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s6[6], R[9];
#pragma unroll
    for (int k = 0; k < 6; ++k) s6[k] = x6d[(size_t)i * 6 + k];
    rot6d_joint(s6, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) rot[(size_t)i * 9 + k] = R[k];
}

// the backward of rot6d_joint (head.hip / specmi_internal.h): one lane per rotation
__global__ void rot6d_bwd_kernel(const float* __restrict__ x6d, const float* __restrict__ g, float* __restrict__ gx, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = x6d + (size_t)i * 6;
    const float* gi = g + (size_t)i * 9;
    const float a1[3] = {p[0], p[2], p[4]}, a2[3] = {p[1], p[3], p[5]};
    const float r1 = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), n1 = fmaxf(r1, 1e-12f);
    const float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const float d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const float r2 = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), n2 = fmaxf(r2, 1e-12f);
    const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    float gb1[3] = {gi[0], gi[3], gi[6]}, gb2[3] = {gi[1], gi[4], gi[7]};
    const float gb3[3] = {gi[2], gi[5], gi[8]};
    // b3 = b1 x b2
    gb1[0] += b2[1] * gb3[2] - b2[2] * gb3[1]; gb1[1] += b2[2] * gb3[0] - b2[0] * gb3[2]; gb1[2] += b2[0] * gb3[1] - b2[1] * gb3[0];
    gb2[0] += gb3[1] * b1[2] - gb3[2] * b1[1]; gb2[1] += gb3[2] * b1[0] - gb3[0] * b1[2]; gb2[2] += gb3[0] * b1[1] - gb3[1] * b1[0];
    // b2 = u / max(|u|, eps): below eps the divisor is a constant
    const float s2 = r2 > 1e-12f ? b2[0] * gb2[0] + b2[1] * gb2[1] + b2[2] * gb2[2] : 0.f;
    const float gu[3] = {(gb2[0] - b2[0] * s2) / n2, (gb2[1] - b2[1] * s2) / n2, (gb2[2] - b2[2] * s2) / n2};
    // u = a2 - d b1, d = b1 . a2
    const float gd = -(gu[0] * b1[0] + gu[1] * b1[1] + gu[2] * b1[2]);
    float ga2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gb1[c] += gd * a2[c] - d * gu[c];
        ga2[c] = gu[c] + gd * b1[c];
    }
    const float s1 = r1 > 1e-12f ? b1[0] * gb1[0] + b1[1] * gb1[1] + b1[2] * gb1[2] : 0.f;
    float* o = gx + (size_t)i * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[2 * c] = (gb1[c] - b1[c] * s1) / n1;
        o[2 * c + 1] = ga2[c];
    }
}

struct BwdWs { float *j3d, *camt, *gposed, *gfeat, *gA, *gV, *part; size_t total; };
BwdWs carve(float* base, int V, int B) {
    const int tiles = (B + IT - 1) / IT, G = (V + 31) / 32, nchunk = (G + NG - 1) / NG;
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    BwdWs w;
    size_t o = 0;
    w.j3d = base + o; o += up4((size_t)B * 147);
    w.camt = base + o; o += up4((size_t)B * 3);
    w.gposed = base + o; o += up4((size_t)B * 72);
    w.gfeat = base + o; o += up4((size_t)B * 224);
    w.gA = base + o; o += up4((size_t)B * 288);
    w.gV = base + o; o += up4((size_t)B * V * 3);
    w.part = base + o; o += (size_t)nchunk * tiles * PART_ROWS * IT;
    w.total = o;
    return w;
}

}  // namespace

size_t smpl_bwd_ws_floats(int V, int B) { return carve(nullptr, V, B).total; }

int launch_smpl_backward(const SmplDev& m, const SmplBwdArgs& a, const LaunchCtx& ctx) {
    const int B = a.fwd.B, V = m.V;
    const int tiles = (B + IT - 1) / IT, G = (V + 31) / 32, nchunk = (G + NG - 1) / NG;
    const BwdWs w = carve(a.ws, V, B);
    const bool body = a.g_rotmat || a.g_betas;
    SmplArgs f = a.fwd;
    f.joints3d = w.j3d; f.joints2d = nullptr; f.cam_t = w.camt;
    f.ld_verts = 0; f.ld_j3d = 147; f.ld_j2d = 98; f.ld_camt = 3;
    f.final_ = nullptr;
    if (int rc = launch_smpl(m, f, ctx)) return rc;
    {
        JointBwdArgs j;
        j.j3d = w.j3d; j.camt = w.camt; j.cam = f.cam; j.R = f.cam_rotmat; j.K = f.cam_intrinsics;
        j.bbox_scale = f.bbox_scale; j.bbox_center = f.bbox_center; j.img_w = f.img_w; j.img_h = f.img_h;
        j.g_verts = a.g_vertices; j.g_j3d = a.g_joints3d; j.g_j2d = a.g_joints2d; j.g_camt = a.g_cam_t;
        j.J_extra = m.J_extra; j.extra_ids = m.extra_ids; j.joint_map = m.joint_map;
        j.gV = body ? w.gV : nullptr; j.gposed = body ? w.gposed : nullptr; j.g_cam = a.g_cam;
        j.V = V; j.mode = f.mode; j.normalize = f.normalize_joints2d; j.focal = f.focal_length; j.img_res = f.img_res;
        ProfScope ps(ctx, "smpl_bwd_joints", body ? 2.0 * B * V * 27.0 : 0.0, body ? 4.0 * ((double)B * V * 6 + 9.0 * V) : 4.0 * B * 150);
        hipLaunchKernelGGL(smpl_joints_bwd_kernel, dim3(B), dim3(JBT), 0, ctx.stream, j);
    }
    if (!body) return (int)hipGetLastError();
    {
        // per (vertex, image): T rows (9 x 24 x 2) + g_v_posed (18) + the 3 x 224 contraction
        ProfScope ps(ctx, "smpl_bwd_skin_feat", 2.0 * (double)B * V * (216 + 9 + 3.0 * 224), 4.0 * ((double)B * V * 3 + (double)V * (3.0 * 224 + 24)));
        hipLaunchKernelGGL(smpl_skin_bwd_feat_kernel, dim3(nchunk, tiles), dim3(64), 0, ctx.stream, m.dirsT, m.wT, f.A, w.gV, w.part, V, B, G);
    }
    {
        ProfScope ps(ctx, "smpl_bwd_skin_A", 2.0 * (double)B * V * (3.0 * 224 + 9 + 288), 4.0 * ((double)B * V * 3 + (double)V * (3.0 * 224 + 24)));
        hipLaunchKernelGGL(smpl_skin_bwd_A_kernel, dim3(nchunk, tiles), dim3(64), 0, ctx.stream, m.dirsT, m.wT, f.pose_feat, w.gV, w.part, V, B, G);
    }
    {
        const int n = tiles * PART_ROWS * IT;
        ProfScope ps(ctx, "smpl_bwd_reduce", (double)nchunk * n, 4.0 * ((double)nchunk * n + (double)B * 512));
        hipLaunchKernelGGL(smpl_bwd_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx.stream, w.part, w.gfeat, w.gA, nchunk, tiles, B);
    }
    {
        ProfScope ps(ctx, "smpl_bwd_chain", 0.0, 4.0 * B * (216 + 10 + 288 + 224 + 72 + 216 + 10));
        hipLaunchKernelGGL(smpl_chain_bwd_kernel, dim3(B), dim3(64), 0, ctx.stream, f.rotmat, f.betas, m.J_template, m.J_shapedirs,
                           m.parents, w.gA, w.gfeat, w.gposed, a.g_rotmat, a.g_betas);
    }
    return (int)hipGetLastError();
}

int launch_rot6d_forward(const float* x6d, float* rotmat, int n, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "rot6d_fwd", 0.0, 4.0 * n * 15);
    hipLaunchKernelGGL(rot6d_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx.stream, x6d, rotmat, n);
    return (int)hipGetLastError();
}

int launch_rot6d_backward(const float* x6d, const float* g_rotmat, float* g_x6d, int n, const LaunchCtx& ctx) {
    ProfScope ps(ctx, "rot6d_bwd", 0.0, 4.0 * n * 21);
    hipLaunchKernelGGL(rot6d_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx.stream, x6d, g_rotmat, g_x6d, n);
    return (int)hipGetLastError();
}

}  // namespace specmi
