// conv_igemm_tile.h - what the implicit-GEMM kernels share.  All of them (conv_igemm.hip, conv_wsplit.hip, conv_bf16s.hip,
// conv_f16.hip): the vector types, the out-of-range buffer offset and the XCD-aware tile order.  The two fp32 kernels, which
// must produce the same bits and run the same hand-off: the kernel arguments of a (fused) convolution, the per-network operand
// select, the output row -> input address decode, the ticket step of the split-K hand-off, the epilogue element operation, and
// the host-side argument builder / shape checks.
// Reference call sites served: spec/models/hmr.py:92, camcalib/model.py:73 (the ResNet trunks), spec/models/hmr.py:96,
// camcalib/model.py:77-79 (FC layers).
#pragma once
#include <type_traits>

// The split-K hand-off (sk_last_arriver below) is the form validated on gfx950, not the portable HIP memory-model form.  Refuse
// to build for anything else rather than run a protocol nobody validated there.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libspecmi's in-launch hand-offs are validated on gfx950 (MI355X) only: build with --offload-arch=gfx950"
#endif

#include "specmi_internal.h"

namespace specmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct NetOperands { const float *x, *w, *scale, *shift, *res, *x2; float* out; };   // one network's tensors of a layer

struct KArgs {
    const float* x;
    const float* w;
    const float* scale;
    const float* shift;
    const float* res;
    float* out;
    unsigned x_bytes, w_bytes;  // buffer extents (< 2^31)
    // optional second A source of a 1x1 layer (K = Cin + Cin2): the block input of a fused downsample branch
    const float* x2;
    unsigned x2_bytes;
    int H2, W2, ldx2, stride2, cpc1;   // cpc1 = 32-channel chunks that come from x
    int H, W, ldx;
    int OW, OHW, Cout, Npad, ldo;
    int KH, KW, stride, pad;
    int M, nbn, nchunks, cpc;  // cpc = chunks per filter tap = Cin / 32
    int xcd_cols;              // > 0: XCD x owns tile columns [x * xcd_cols, (x + 1) * xcd_cols) and walks all tile rows (see the tile order)
    unsigned mg_ohw, sh_ohw, mg_ow, sh_ow;  // magic multipliers: n / OHW, n / OW for n < 2^31
    int relu;
    // SPLITK: blockIdx.y = K slice z of nchunks chunks; the raw accumulators of slice z of tile t (t = blockIdx.x + gridDim.x *
    // blockIdx.z) go to sk_ws[(t * S + z) * BM * BN ..] in accumulator order, sk_cnt[t] counts the slices that have arrived
    float* sk_ws;
    unsigned* sk_cnt;
    int sk_leaf, sk_G, sk_unit;   // chunks per leaf; leaves per group; leaves per workgroup (1, sk_G or all: nchunks = sk_unit * sk_leaf)
    int vec_ok;  // out/res rows are 16-byte aligned: float4 epilogue traffic allowed
    // grouped launch (gridDim.z = 2): blockIdx.z = 1 runs the SAME layer shape of a second network on its own tensors - the
    // two ResNet-50 trunks of the path (CamCalib + SPEC) as one launch per layer: half the launches, and the partially
    // filled last round of workgroups of one network is filled by the other
    NetOperands g1;
#ifdef SPECMI_TUNE
    int ablate;  // perf ablation bits (wrong results!): 1 no global loads in loop, 2 no LDS restage, 4 no epilogue stores
    unsigned long long* tprof;  // per-phase cycle counters (s_memtime)
#endif
};

#ifdef SPECMI_TUNE
#define TUNE_ABLATE(bit) (p.ablate & (bit))
#define TUNE_T(var) const long long var = __builtin_amdgcn_s_memtime()
#else
#define TUNE_ABLATE(bit) 0
#define TUNE_T(var)
#endif

constexpr unsigned kOutOfRange = 0x80000000u;  // >= any buffer extent: the load returns zeros

// XCD-aware tile order (bijective for any grid size): workgroup ids go round-robin to the 8 XCDs, so XCD x is given the x-th
// contiguous run of the tile list - tiles that share an A row panel (n fastest) hit the same 4 MiB L2
__device__ __forceinline__ int xcd_tile_order(int bid, int nblk) {
    const int xcd = bid & 7, q8 = nblk >> 3, r8 = nblk & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// the tensors of the network this workgroup serves (grouped launch: blockIdx.z = 1 is the second one); wave-uniform, scalar selects
__device__ __forceinline__ NetOperands net_operands(const KArgs& p) {
    const bool grp = blockIdx.z != 0;
    return {grp ? p.g1.x : p.x, grp ? p.g1.w : p.w, grp ? p.g1.scale : p.scale, grp ? p.g1.shift : p.shift,
            grp ? p.g1.res : p.res, grp ? p.g1.x2 : p.x2, grp ? p.g1.out : p.out};
}

// Output row m -> where its A operand starts.  The tile prologue sits on every workgroup's critical path, so the pixel decode
// avoids the ~40-instruction integer divide: 1x1 / stride-1 rows address the input with m itself, other shapes divide by
// OH*OW and OW with host-computed magic multipliers.
struct RowAddr {
    unsigned voff;    // byte offset of (the row's tap-(0,0) pixel, lane_bytes); out of range when the row is past M (1x1)
    unsigned mask;    // KxK: bit t = filter tap t lies inside the image for this row (0 past M)
    unsigned voff2;   // dual: the row's pixel in the second source (its own size / stride / channel count)
};
struct RowPixel { int b, oy, ox; };
__device__ __forceinline__ RowPixel conv_row_pixel(const KArgs& p, int m) {
    const int b = magic_div(m, p.OHW, p.mg_ohw, p.sh_ohw);
    const int rem = m - b * p.OHW;
    const int oy = magic_div(rem, p.OW, p.mg_ow, p.sh_ow);
    return {b, oy, rem - oy * p.OW};
}
__device__ __forceinline__ RowAddr conv_row_addr(const KArgs& p, bool is1x1, bool dual, int m, int lane_bytes) {
    RowAddr r = {0u, 0u, 0u};
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    if (dual) {
        if (p.stride2 == 1) {
            r.voff2 = ok ? (unsigned)(mm * p.ldx2 * 4 + lane_bytes) : kOutOfRange;
        } else {
            const RowPixel q = conv_row_pixel(p, mm);
            const int pix2 = (q.b * p.H2 + q.oy * p.stride2) * p.W2 + q.ox * p.stride2;
            r.voff2 = ok ? (unsigned)(pix2 * p.ldx2 * 4 + lane_bytes) : kOutOfRange;
        }
    }
    if (is1x1 && p.stride == 1) {
        r.voff = ok ? (unsigned)(mm * p.ldx * 4 + lane_bytes) : kOutOfRange;
    } else {
        const RowPixel q = conv_row_pixel(p, mm);
        const int iy0 = q.oy * p.stride - p.pad, ix0 = q.ox * p.stride - p.pad;
        const int pix0 = (q.b * p.H + iy0) * p.W + ix0;
        const unsigned off = (unsigned)(pix0 * p.ldx * 4 + lane_bytes);   // wraps for padded rows; only used on valid taps
        if (is1x1) {
            r.voff = ok ? off : kOutOfRange;
        } else {
            r.voff = off;
            unsigned colbits = 0, mk = 0;   // tap (ky,kx) is inside the image iff row ky and column kx are
            for (int kx = 0; kx < p.KW; ++kx) colbits |= ((unsigned)(ix0 + kx) < (unsigned)p.W ? 1u : 0u) << kx;
            for (int ky = 0; ky < p.KH; ++ky)
                if ((unsigned)(iy0 + ky) < (unsigned)p.H) mk |= colbits << (ky * p.KW);
            r.mask = ok ? mk : 0u;
        }
    }
    return r;
}

// The ticket step of the split-K hand-off, called by every thread of a workgroup after it has issued its slab stores; true in
// all threads of the LAST of the tile's S workgroups to arrive (which then folds the slabs), false in the others (which return).
// Per-XCD L2s are not kept consistent with each other and a CU's L1 is never refreshed by another CU's stores, so the hand-off
// is the write-through form MI355X_MICROARCH.md documents for gfx950 (inter-workgroup visibility): the slabs are written with
// sc1 stores (they leave the XCD's L2 for memory), every wave drains its stores (vmcnt 0), ONE lane takes the ticket with a
// relaxed agent-scope atomic, and the last arriver reads all slabs with sc1 loads (no L1, fresh from the fabric).  It is NOT
// the portable memory-model form - release on the ticket + acquire in the last arriver = buffer_wbl2 + buffer_inv per
// workgroup, measured 35 us per launch here - and is stress-tested on gfx950 (tests/test_gpu_latency.py::
// test_in_kernel_reduction_is_race_free, tests/test_gpu_round5.py).  flag: one LDS word nobody else uses until the caller's
// next barrier.
__device__ __forceinline__ bool sk_last_arriver(unsigned* cnt, unsigned S, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's slab stores have left for memory
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = ticket == S - 1;
        // every slice has arrived: the counter is free again for the next launch / graph replay
        if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// The epilogue of four consecutive output columns: BatchNorm scale / shift, residual, ReLU
__device__ __forceinline__ f32x4 epilogue_quad(f32x4 acc, f32x4 sc, f32x4 sh, bool has_res, f32x4 res, int relu) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[e], sc[e], sh[e]);
    if (has_res) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += res[e];
    }
    if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    return v;
}
// the same element by element, for a quad that straddles Cout (ncols < 4) or whose rows are not 16-byte aligned; o = the
// offset of the quad's first element in out / res
__device__ __forceinline__ void epilogue_tail(const float* acc, f32x4 sc, f32x4 sh, const float* res, int relu, float* out, size_t o, int ncols) {
    for (int e = 0; e < 4; ++e) {
        if (e < ncols) {
            float t = fmaf(acc[e], sc[e], sh[e]);
            if (res) t += res[o + e];
            if (relu) t = fmaxf(t, 0.f);
            out[o + e] = t;
        }
    }
}

// the shapes / alignments every fp32 implicit-GEMM launcher accepts (b: the twin layer of a grouped launch): 0 or hipErrorInvalidValue
int conv_igemm_check(const ConvArgs& a, const ConvArgs* b);
// fused-conv arguments -> kernel arguments of the sliced 64x64 body (conv_igemm.hip); pl: the layer's canonical tree + unit
void conv_igemm_make_sk_kargs(const ConvArgs& a, const SkPlan& pl, const ConvArgs* b, KArgs& k);
// conv_igemm_check + a consistent plan + tensors within 32-bit buffer addressing (what the sliced launchers check): 0,
// hipErrorInvalidValue or SK_NEEDS_BATCH_SPLIT
int conv_igemm_sk_check(const ConvArgs& a, const SkPlan& pl, const ConvArgs* b);

}  // namespace specmi
