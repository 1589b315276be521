// api.hip - host side of libspecmi.so: the C ABI of include/specmi.h, parameter staging, workspace management and the launch
// sequences of the two networks.  Weight packing / BatchNorm folding / the composed regressor live in commit.hip, the option table
// in options.hip, device code in conv_igemm.hip / conv_wsplit.hip / conv_wino.hip / stem.hip / head.hip / smpl.hip / ...
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "handle.h"

using namespace specmi;

thread_local std::string g_create_err;   // specmi_create's message when no handle exists yet, per calling thread

int fail(specmi_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_err = buf;
    return code;
}

// Every entry point runs on the handle's device and puts the caller's current device back on return (the caller -
// PyTorch - reads hipGetDevice to decide where its next allocation goes; a library must not move it).
struct DeviceGuard {
    int prev = -1;
    hipError_t enter(int dev) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) { prev = -1; return e; }
        if (prev == dev) { prev = -1; return hipSuccess; }
        return hipSetDevice(dev);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};


int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ------------------------------------------------------------------------------------------
// device memory helpers
// ------------------------------------------------------------------------------------------
int dev_upload(specmi_handle* h, const void* src, size_t bytes, void** out, std::vector<void*>& pool) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, bytes ? bytes : 4));
    pool.push_back(p);
    if (bytes) HIPCHK(h, hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *out = p;
    return SPECMI_OK;
}

int dev_alloc(specmi_handle* h, size_t bytes, void** out, std::vector<void*>& pool) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, bytes ? bytes : 4));
    pool.push_back(p);
    *out = p;
    return SPECMI_OK;
}

void free_pool(std::vector<void*>& pool) {
    for (void* p : pool) (void)hipFree(p);
    pool.clear();
}

// ------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------
int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }

// Growing a workspace synchronises the device, frees and allocates - all of which a stream capture forbids.  Say so in words
// instead of a bare HIP error: the remedy is one eager forward of the shape before capturing (GraphedPipeline / GraphedStep do it).
static int sync_for_growth(specmi_handle* h, const char* what) {
    const hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) return SPECMI_OK;
    (void)hipGetLastError();
    if (e == hipErrorStreamCaptureUnsupported || e == hipErrorStreamCaptureImplicit || e == hipErrorStreamCaptureInvalidated ||
        e == hipErrorStreamCaptureIsolation || e == hipErrorStreamCaptureWrongThread || e == hipErrorStreamCaptureUnjoined)
        return fail(h, SPECMI_ERR_STATE, "%s must grow for this batch / resolution, which is not possible while a stream is being "
                    "captured: run one eager forward of this shape first (the capture is invalid now)", what);
    return fail(h, SPECMI_ERR_HIP, "hipDeviceSynchronize failed while growing %s: %s", what, hipGetErrorString(e));
}

// The in-launch hand-offs (split-K tile tickets) rely on arrival counters that every launch leaves at zero.  A launch that dies
// mid-flight does not: zero them whenever that may have happened (after any failed forward), at specmi_commit and on demand
// (specmi_sync_reset).  Enqueued on `s`.
static void reset_sync_state(specmi_handle* h, hipStream_t s) {
    if (h->sk.cnt) (void)hipMemsetAsync(h->sk.cnt, 0, (size_t)h->sk.ncnt * 4, s);
    (void)hipGetLastError();
}

static int ensure_ws(specmi_handle* h, int B, int H, int W) {
    const int oh1 = conv_out(H, 7, 2, 3), ow1 = conv_out(W, 7, 2, 3);
    // largest activation: stem output (B,oh1,ow1,64) == layer1 output (B,oh1/2,ow1/2,256) rounded up
    const int oh2 = conv_out(oh1, 3, 2, 1), ow2 = conv_out(ow1, 3, 2, 1);
    size_t elems = (size_t)B * oh1 * ow1 * 64;
    const size_t l1 = (size_t)B * oh2 * ow2 * 256;
    if (l1 > elems) elems = l1;
    const bool grow_act = elems > h->act_elems;
    const bool grow_b = B > h->ws_B;
    if (!grow_act && !grow_b) return SPECMI_OK;
    if (int rc0 = sync_for_growth(h, "the activation workspace")) return rc0;
    // the outgrown buffers stay alive until specmi_destroy (as the split-K workspace does): a hipGraph captured at a smaller
    // batch / resolution has their addresses baked into its kernel nodes, and replaying it after an eager call at a larger size
    // must not write into freed memory.  Growth is geometric (a dimension that must grow grows to at least 1.5x its old size), so
    // an ascending sweep of batch sizes or resolutions retires a geometric series: at most ~3x the final size in total
    // instead of one full copy per step.
    h->ws_retired.insert(h->ws_retired.end(), h->ws_allocs.begin(), h->ws_allocs.end());
    h->ws_allocs.clear();
    if (grow_act && h->act_elems && elems < h->act_elems + h->act_elems / 2) elems = h->act_elems + h->act_elems / 2;
    if (elems < h->act_elems) elems = h->act_elems;
    int Bw = B > h->ws_B ? B : h->ws_B;
    if (grow_b && h->ws_B && Bw < h->ws_B + h->ws_B / 2) Bw = h->ws_B + h->ws_B / 2;
    // the workspace is gone from here on: if an allocation below fails, the next call must not take the early return
    // above on the strength of the old sizes and launch kernels on freed memory
    h->act_elems = 0; h->ws_B = 0;
    for (int i = 0; i < 4; ++i) h->act[i] = nullptr;
    int rc;
    for (int i = 0; i < 4; ++i)
        if ((rc = dev_alloc(h, elems * 4, (void**)&h->act[i], h->ws_allocs))) return rc;
    h->act_elems = elems;
    const int Bp = round_up(Bw, 8);
    const int V = h->smpl.V > 0 ? h->smpl.V : 1;
    if ((rc = dev_alloc(h, (size_t)Bp * h->xc_ld * 4, (void**)&h->xc, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * 1024 * 4, (void**)&h->h1, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * 1024 * 4, (void**)&h->h2, h->ws_allocs))) return rc;
    for (int i = 0; i < 2; ++i)   // hidden rows of the three CamCalib Linear chains when they run as one launch per layer
        if ((rc = dev_alloc(h, (size_t)3 * Bp * 1024 * 4, (void**)&h->fc_hidden[i], h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * 2048 * 4, (void**)&h->xf, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * 216 * 4, (void**)&h->rot_ws, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * 10 * 4, (void**)&h->betas_ws, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * 3 * 4, (void**)&h->cam_ws, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * V * 3 * 4, (void**)&h->verts_ws, h->ws_allocs))) return rc;
    const int Bp32 = round_up(Bw, 32);   // the skinning kernel's operands come in tiles of 32 images (smpl.hip)
    if ((rc = dev_alloc(h, (size_t)Bp32 * SMPL_KQ * 8 * 4, (void**)&h->pf_ws, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp32 * 288 * 4, (void**)&h->A_ws, h->ws_allocs))) return rc;
    if ((rc = dev_alloc(h, (size_t)Bp * 72 * 4, (void**)&h->pj_ws, h->ws_allocs))) return rc;
    HIPCHK(h, hipMemset(h->pf_ws, 0, (size_t)Bp32 * SMPL_KQ * 8 * 4));   // rows 218..223 of the feature operand stay zero
    HIPCHK(h, hipMemset(h->A_ws, 0, (size_t)Bp32 * 288 * 4));
    h->ws_B = Bw;
    return SPECMI_OK;
}

// split-K workspace (partial tiles + arrival counters), grown on demand and never shrunk.  Growing frees and allocates, which a
// stream capture forbids: the eager warm-up call of a shape (GraphedPipeline runs two) sizes it, captures find it large enough.
static int ensure_sk(specmi_handle* h, size_t floats, int ncnt) {
    if (floats <= h->sk.floats && ncnt <= h->sk.ncnt) return SPECMI_OK;
    if (int rc0 = sync_for_growth(h, "the split-K workspace")) return rc0;
    if (floats < h->sk.floats) floats = h->sk.floats;
    if (ncnt < h->sk.ncnt) ncnt = h->sk.ncnt;
    if (h->sk.floats && floats > h->sk.floats && floats < h->sk.floats + h->sk.floats / 2) floats = h->sk.floats + h->sk.floats / 2;   // geometric: see ensure_ws
    floats = (floats + ((size_t)1 << 20) - 1) >> 20 << 20;
    ncnt = round_up(ncnt < 4096 ? 4096 : ncnt, 4096);
    // the outgrown buffers stay alive until specmi_destroy: a hipGraph captured earlier (GraphedPipeline at another batch
    // size) has their addresses baked into its kernel nodes
    if (h->sk.ws) h->sk_retired.push_back(h->sk.ws);
    if (h->sk.cnt) h->sk_retired.push_back(h->sk.cnt);
    h->sk = SkWs{};
    float* ws = nullptr;
    unsigned* cnt = nullptr;
    HIPCHK(h, hipMalloc((void**)&ws, floats * 4));
    hipError_t e = hipMalloc((void**)&cnt, (size_t)ncnt * 4);
    if (e == hipSuccess) e = hipMemset(cnt, 0, (size_t)ncnt * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(ws);
        if (cnt) (void)hipFree(cnt);
        return fail(h, SPECMI_ERR_HIP, "split-K workspace: %s", hipGetErrorString(e));
    }
    h->sk.ws = ws; h->sk.floats = floats; h->sk.cnt = cnt; h->sk.ncnt = ncnt;
    return SPECMI_OK;
}

// ------------------------------------------------------------------------------------------
// launch sequences
// ------------------------------------------------------------------------------------------
static int run_fc(specmi_handle* h, const FcW& fc, const float* x, int ldx, int B, const float* res, float* out,
                  int ldo, hipStream_t s, const char* label) {
    // Rows are processed in blocks of at most 1024 so that the K slicing (and with it the summation order of every
    // output) is the same for every batch size: an image's result must not depend on how many images share its launch
    // (rank-sharded 8 x 256 == unsharded 2048, bit for bit).
    constexpr int RB = 1024;
    for (int b0 = 0; b0 < B; b0 += RB) {
        const int nb = B - b0 < RB ? B - b0 : RB;
        ConvArgs a;
        a.x = x + (size_t)b0 * ldx; a.w = fc.w; a.scale = fc.scale; a.shift = fc.shift;
        a.res = res ? res + (size_t)b0 * ldo : nullptr; a.out = out + (size_t)b0 * ldo;
        a.B = nb; a.H = 1; a.W = 1; a.Cin = fc.Kp; a.ldx = ldx;
        a.OH = 1; a.OW = 1; a.Cout = fc.nout; a.Npad = fc.Npad; a.ldo = ldo;
        a.KH = 1; a.KW = 1; a.stride = 1; a.pad = 0; a.relu = 0;
        a.force_variant = opt(h, OPT_force_conv_variant);
        LaunchCtx ctx{s, &h->prof, label};
        const int S = opt(h, OPT_fc_splitk) ? conv_igemm_splitk_plan(a) : 1;
        if (S > 1) {
            int rc;
            if ((rc = ensure_sk(h, conv_igemm_sk_ws_floats(a, S, 1), conv_igemm_sk_tiles(a, 1)))) return rc;
            SkPlan pl;
            pl.leaves = S;      // flat fold of S slices, the order these GEMMs have had since round 1
            LAUNCHCHK(h, launch_conv_igemm_sk(a, pl, h->sk, ctx), label);
            continue;
        }
        LAUNCHCHK(h, launch_conv_igemm(a, ctx), label);
    }
    return SPECMI_OK;
}

// images NCHW -> layer4 map NHWC in *feat (a workspace buffer unless feat_out given)
// One launch of the trunk's op list: the stem, the max-pool or a fused conv, with the buffer each
// operand lives in (act[] index, -1 = none, -2 = the caller's feature buffer) and its per-image size.
struct TrunkOp {
    int kind;  // 0 stem, 1 maxpool, 2 conv
    const ConvW* c;
    int in_buf, out_buf, res_buf;
    int H, W;            // input spatial size
    int OH, OW;          // output spatial size
    int relu;
    std::string label;
    size_t in_img, out_img;  // floats per image of input / output (and residual)
    // fused downsample branch (conv3 ops only): the block input as a second A source
    const Bneck* fused = nullptr;
    int in2_buf = -1, H2 = 0, W2 = 0;
    size_t in2_img = 0;
};

// What one op of the list launches: the fused-conv arguments and the kernel family they go to
struct OpLaunch {
    int kind = 2;             // 0 stem, 1 maxpool, 2 conv
    ConvArgs a;
    int family = 0;           // conv: 0 implicit GEMM, 1 Winograd, 2 split-bf16 (optional path)
    int sk = 1;               // latency plan: K slices of the implicit GEMM (1 = the throughput kernel)
    const void* wsplit = nullptr;
    int terms = 0;
    const float *x = nullptr, *w = nullptr, *scale = nullptr, *shift = nullptr;   // stem / maxpool operands
    float* out = nullptr;
};

// the canonical tree of a sliced layer and the unit of this launch (px = pixels of the trunk call, see sk_fill), from the options
static SkPlan sk_plan(const specmi_handle* h, const ConvArgs& a, int groups, long px = 0);

static OpLaunch prepare_op(specmi_handle* h, const TrunkOp& op, const float* images, float* feat_out, int b0, int nb,
                           int Himg, int Wimg, int mode = 0) {
    const bool latency = mode != 0;
    auto buf = [&](int idx) -> float* { return idx == -2 ? feat_out : h->act[idx]; };
    OpLaunch L;
    L.kind = op.kind;
    if (op.kind == 0) {
        L.x = images + (size_t)b0 * 3 * Himg * Wimg; L.w = h->stem.w; L.scale = h->stem.scale; L.shift = h->stem.shift;
        L.out = buf(op.out_buf) + (size_t)b0 * op.out_img;
        return L;
    }
    if (op.kind == 1) {
        L.x = buf(op.in_buf) + (size_t)b0 * op.in_img;
        L.out = buf(op.out_buf) + (size_t)b0 * op.out_img;
        return L;
    }
    const ConvW& c = *op.c;
    ConvArgs& a = L.a;
    a.x = buf(op.in_buf) + (size_t)b0 * op.in_img;
    a.w = c.w; a.scale = c.scale; a.shift = c.shift;
    a.res = op.res_buf == -1 ? nullptr : buf(op.res_buf) + (size_t)b0 * op.out_img;
    a.out = buf(op.out_buf) + (size_t)b0 * op.out_img;
    a.B = nb; a.H = op.H; a.W = op.W; a.Cin = c.cin; a.ldx = c.cin;
    a.OH = op.OH; a.OW = op.OW; a.Cout = c.cout; a.Npad = c.Npad; a.ldo = c.cout;
    a.KH = c.k; a.KW = c.k; a.stride = c.stride; a.pad = c.pad; a.relu = op.relu;
    a.force_variant = opt(h, OPT_force_conv_variant);
    a.wino_variant = opt(h, OPT_force_wino_variant);
    if (op.fused) {
        const Bneck& bk = *op.fused;
        a.w = bk.f_w; a.scale = bk.f_scale; a.shift = bk.f_shift; a.Npad = bk.f_Npad; a.res = nullptr;
        a.x2 = buf(op.in2_buf) + (size_t)b0 * op.in2_img;
        a.H2 = op.H2; a.W2 = op.W2; a.ldx2 = bk.ds.cin; a.Cin2 = bk.ds.cin; a.stride2 = bk.ds.stride;
    }
    if (const void* wsplit = op.fused ? op.fused->f_wsplit : c.wsplit) {
        const int terms = opt(h, OPT_conv_precision);
        // 3x3 layers: the bf16 implicit GEMM spends 9 taps x terms / 16 of an fp32 MFMA cycle per MAC, the fp32 Winograd kernel
        // 16 / 36: with three terms the bf16 path wins on every 3x3 layer, with six only where Winograd does not apply (stride 2)
        const bool wino_ok = c.wino && opt(h, OPT_winograd) && conv_wino_supported(a);
        const bool take = c.k == 1 || terms == 3 || !wino_ok || opt(h, OPT_conv_precision_3x3);
        if ((terms == 3 || terms == 6) && take && conv_bf16s_supported(a)) {
            L.family = 2; L.wsplit = wsplit; L.terms = terms;
            return L;
        }
    }
    bool wino = c.wino && opt(h, OPT_winograd) && conv_wino_supported(a);
    if (latency && !a.force_variant) {
        // Latency plan (batch <= 10 by default).  Every choice below is a function of the layer's per-image shape, never of the batch:
        // an image's bits are the same at batch 1 and 16.  Winograd only where an image alone brings enough 2x2 tiles to
        // fill its 32-tile rows (layer1 / layer2 at 224^2); layer3 / layer4 (49 / 16 tiles per image, U = 16/9 of the
        // weight bytes) run the direct kernel over K slices.
        // (wide layers need proportionally more tiles: layer4 of a 600 x 1066 frame has 170 tiles per image = 48 Winograd workgroups
        // walking Cin = 512 for 75 us, the sliced direct kernel takes 45)
        const int min_tiles = opt(h, OPT_latency_wino_min_tiles);
        if (wino && ((a.OH + 1) / 2) * ((a.OW + 1) / 2) < (min_tiles > a.Cin || min_tiles == 0 || min_tiles >= 100000 ? min_tiles : a.Cin)) wino = false;
        if (mode == 2) wino = false;   // 'single': batch 1-2, the direct kernel wins on layer1 / layer2 too
        if (!wino) L.sk = sk_plan(h, a, 1).leaves;
    }
    if (wino) {
        a.w = c.wino;
        L.family = 1;
    }
    return L;
}

// plan: 0 auto, 1 throughput, 2 latency, 3 single.  Returns the trunk mode of this call: 0 throughput kernels, 1 latency (sliced
// direct kernels on layer3 / layer4, Winograd where an image fills its rows), 2 single (round 5: batch 1-2, the reference's demo
// granularity, scripts/camcalib_demo.py:95-102 - every 3x3 convolution on the sliced direct kernel, which is faster there by
// 21 / 12 us at batch 1 / 2, profiles/r04_b_latency_layers.txt).  auto = single up to "single_max_batch" (2) images' worth of
// pixels, latency up to N = "latency_max_batch" (10) for the trunk PAIR / "latency_max_batch_single" (16) for one trunk - measured
// per batch size (profiles/r04_l_plan_crossover.jsonl: pair 1.67 vs 1.78 ms at 10 images, 2.18 vs 2.15 at 12; one trunk after the
// other 3.08 vs 3.32 ms still at 16; a single CamCalib frame at 600 x 1066 = 12.7 crops' worth of rows: 2.10 vs 2.27 ms for the
// demo's one-frame step)
static int trunk_mode(specmi_handle* h, int B, int H, int W, bool pair = false) {
    const int plan = opt(h, OPT_plan);
    if (plan == 1) return 0;
    if (plan == 2) return 1;
    if (plan == 3) return 2;
    const long px = (long)B * H * W, crop = 224L * 224;
    if (px <= (long)opt(h, OPT_single_max_batch) * crop) return 2;
    const int nmax = pair ? opt(h, OPT_latency_max_batch) : opt(h, OPT_latency_max_batch_single);
    return px <= (long)nmax * crop ? 1 : 0;
}
// the FC layers behind the trunk see batch rows only: the small-batch GEMV kernel (head.hip) up to "latency_max_batch" rows
// the unit rule of the sliced 64x64 kernel (conv_igemm_sk_plan): "latency_unit_model" = 1 -> the round model (fill <= 0 = -slots),
// 0 -> the threshold "latency_fill_wgs"
// px = pixels of the trunk call (B x H x W): beyond ten 224 x 224 crops' worth - a single trunk keeps the latency plan up to 16 - the
// threshold is "latency_fill_wgs_large" (400): measured per batch under the auto structure (profiles/r05_n_unit_rule_sweep.jsonl:
// 1.99 -> 1.80 ms at batch 11, 2.13 -> 1.91 at 12, 2.20 -> 2.10 at 14; at batch <= 10 240 stays ahead: 1.55 vs 2.06 ms at 10)
static int sk_fill(const specmi_handle* h, long px = 0) {
    if (opt(h, OPT_latency_unit_model)) return -opt(h, OPT_latency_unit_slots);
    return px > 10L * 224 * 224 ? opt(h, OPT_latency_fill_wgs_large) : opt(h, OPT_latency_fill_wgs);
}
static SkPlan sk_plan(const specmi_handle* h, const ConvArgs& a, int groups, long px) {
    return conv_igemm_sk_plan(a, groups, opt(h, OPT_latency_target_wgs), opt(h, OPT_latency_min_chunks), sk_fill(h, px));
}

static bool use_latency_heads(specmi_handle* h, int B) {
    const int plan = opt(h, OPT_plan);
    return opt(h, OPT_fc_gemv) && (plan == 2 || plan == 3 || (plan == 0 && B <= opt(h, OPT_latency_max_batch)));
}

// partner != nullptr: the same op of a second network, launched together (one grouped launch); the caller has checked
// that both ops have the same kind / family / shape
static int launch_op(specmi_handle* h, const TrunkOp& op, const OpLaunch& L, const OpLaunch* partner, int nb, int Himg, int Wimg,
                     hipStream_t s) {
    LaunchCtx ctx{s, &h->prof, op.label.c_str()};
    if (L.kind == 0) {
        StemPair sp;
        if (partner) { sp.x = partner->x; sp.w = partner->w; sp.scale = partner->scale; sp.shift = partner->shift; sp.out = partner->out; }
        LAUNCHCHK(h, launch_stem(L.x, L.w, L.scale, L.shift, L.out, nb, Himg, Wimg, op.OH, op.OW, 1, ctx, partner ? &sp : nullptr), "stem");
        return SPECMI_OK;
    }
    if (L.kind == 1) {
        LAUNCHCHK(h, launch_maxpool3x3s2(L.x, L.out, nb, op.H, op.W, 64, op.OH, op.OW, ctx, partner ? partner->x : nullptr,
                                         partner ? partner->out : nullptr), "maxpool");
        return SPECMI_OK;
    }
    if (L.family == 2) {
        LAUNCHCHK(h, launch_conv_bf16s(L.a, L.wsplit, L.terms, ctx), op.label.c_str());
        if (partner) LAUNCHCHK(h, launch_conv_bf16s(partner->a, partner->wsplit, partner->terms, ctx), op.label.c_str());
        return SPECMI_OK;
    }
    if (L.sk > 1) {
        const int groups = partner ? 2 : 1;
        int rc;
        SkPlan pl = sk_plan(h, L.a, groups, (long)nb * Himg * Wimg);
        const int fu = opt(h, OPT_latency_force_unit);   // tests: 1 leaf / 2 group / 3 whole K per workgroup, whatever the batch
        if (fu) pl.unit = fu == 1 ? 1 : (fu == 2 ? pl.G : pl.leaves);
        // The wave-split unit (conv_wsplit.hip, round 5): a 32x32 tile per workgroup, the G leaves of a group on its waves side by
        // side - four times the tiles, slabs of 4 KB per GROUP or none.  Same canonical tree, same bits: a pure speed choice, made
        // from the per-layer tables of profiles/r05_c_wsplit_layers.txt:
        //   * taken when the 64x64 kernel would have to slice K across workgroups (its unit is not the whole K), the layer has one A
        //     source (the strided second source of a folded downsample branch measured slower at every batch) and the launch stays
        //     under "wsplit_max_units" (1400 for the trunk pair, "wsplit_max_units_single" 500 for one trunk) leaf-units = 32x32 tiles x
        //     groups: beyond, several workgroups share a CU and the
        //     8 KB of operands per wave-chunk (6 in the 64x64 kernel) cost more than the slabs (batch 8: layer3 1568 units, slower);
        //   * one group per workgroup (slab per group) or all groups (no slab): whichever needs fewer rounds of workgroups per CU,
        //     a round costing one leaf (L chunks of ~0.45 us) and the slab hand-off ~1 us - the rule that reproduces every row of
        //     the tables (batch 1-4, layer2-4).
        // "wsplit": 0 never, 1 (default) by this rule, 2 / 3 always with one group / all groups per workgroup (tests, tables).
        const int wsplit = opt(h, OPT_wsplit);
        if (wsplit && !fu) {
            SkPlan pw = pl;
            const long t32 = conv_wsplit_tiles(L.a, groups);
            const long ng = pl.leaves / (pl.G > 0 ? pl.G : 1);
            const int nch = conv_k_chunks(L.a);
            const double t_leaf = 0.45 * (double)(nch / pl.leaves);
            const long slots = opt(h, OPT_wsplit_slots);
            const double cost_all = (double)((t32 + slots - 1) / slots) * (double)ng * t_leaf;
            const double cost_group = (double)((t32 * ng + slots - 1) / slots) * t_leaf + 1.0;
            pw.unit = (wsplit == 3 || (wsplit == 1 && cost_all <= cost_group)) ? pl.leaves : pl.G;
            // (whole-step sweep, profiles/r05_d_structure_sweep.jsonl: a single trunk's launches - two trunks on two streams, batch
            // 4-10 - want the cap at 500 units, 1.245 vs 1.285 ms at batch 6, 1.441 vs 1.487 at 8; the pair's grouped launches between 1300 and 1500:
            // 0.884 vs 0.913 ms at batch 3 and 1.312 vs 1.421 at 6 with layer3 / layer4 on the unit (<= 1280 units), 1.546 vs 1.573 at
            // batch 8 without it (1568 / 1664 units))
            const long max_units = groups == 2 ? opt(h, OPT_wsplit_max_units) : opt(h, OPT_wsplit_max_units_single);
            const bool take = wsplit > 1 || (pl.unit != pl.leaves && !L.a.x2 && t32 * ng <= max_units);
            if (take && conv_wsplit_supported(L.a, pw)) {
                if ((rc = ensure_sk(h, conv_wsplit_ws_floats(L.a, pw.leaves / pw.unit, groups), conv_wsplit_tiles(L.a, groups)))) return rc;
                const int wrc = launch_conv_wsplit(L.a, pw, h->sk, ctx, partner ? &partner->a : nullptr);
                if (wrc != SK_NEEDS_BATCH_SPLIT) {
                    LAUNCHCHK(h, wrc, op.label.c_str());
                    return SPECMI_OK;
                }
            }
        }
        if ((rc = ensure_sk(h, conv_igemm_sk_ws_floats(L.a, pl.leaves / pl.unit, groups), conv_igemm_sk_tiles(L.a, groups)))) return rc;
        rc = launch_conv_igemm_sk(L.a, pl, h->sk, ctx, partner ? &partner->a : nullptr);
        if (rc != SK_NEEDS_BATCH_SPLIT) {       // misalignment, a bad plan, an undersized workspace: errors, not a silent change of kernel
            LAUNCHCHK(h, rc, op.label.c_str());
            return SPECMI_OK;
        }
        // the sliced launcher does not split the batch (activations past 32-bit addressing, plan = 'latency' pinned at a large
        // batch or resolution): the throughput launcher below does - other bits (the plans differ anyway), never an error
    }
    int rc = L.family == 1 ? launch_conv_wino(L.a, ctx, partner ? &partner->a : nullptr)
                           : launch_conv_igemm(L.a, ctx, partner ? &partner->a : nullptr);
    if (rc == (int)hipErrorInvalidValue && partner) {
        // a grouped launch is refused when the batch's activations pass the 32-bit addressing limit of one launch (the
        // separate launchers split the batch instead): two launches, same kernels, same bits
        (void)hipGetLastError();
        rc = L.family == 1 ? launch_conv_wino(L.a, ctx) : launch_conv_igemm(L.a, ctx);
        if (!rc) rc = L.family == 1 ? launch_conv_wino(partner->a, ctx) : launch_conv_igemm(partner->a, ctx);
    }
    LAUNCHCHK(h, rc, op.label.c_str());
    return SPECMI_OK;
}

static int exec_op(specmi_handle* h, const TrunkOp& op, const float* images, float* feat_out, int b0, int nb,
                   int Himg, int Wimg, hipStream_t s, int mode = 0) {
    const OpLaunch L = prepare_op(h, op, images, feat_out, b0, nb, Himg, Wimg, mode);
    return launch_op(h, op, L, nullptr, nb, Himg, Wimg, s);
}

struct TrunkPlan {
    std::vector<TrunkOp> ops;
    std::vector<int> stage_of;   // resnet stage (0 = stem/pool, 1..4) of each op
    int final_buf = 1, fh = 0, fw = 0;
};

// the trunk's op list for an (H, W) input: the stem, the max-pool and one fused conv per layer, with the ping-pong
// buffers they read and write
static void plan_trunk(specmi_handle* h, int H, int W, bool to_caller, TrunkPlan& P) {
    float* const feat_out = to_caller ? reinterpret_cast<float*>(1) : nullptr;   // only its null-ness matters here
    std::vector<TrunkOp>& ops = P.ops;
    std::vector<int>& stage_of = P.stage_of;
    const int oh1 = conv_out(H, 7, 2, 3), ow1 = conv_out(W, 7, 2, 3);
    int ch = conv_out(oh1, 3, 2, 1), cw = conv_out(ow1, 3, 2, 1);
    ops.push_back({0, nullptr, -1, 0, -1, H, W, oh1, ow1, 1, "backbone.conv1", (size_t)3 * H * W, (size_t)oh1 * ow1 * 64});
    stage_of.push_back(0);
    ops.push_back({1, nullptr, 0, 1, -1, oh1, ow1, ch, cw, 0, "backbone.maxpool", (size_t)oh1 * ow1 * 64, (size_t)ch * cw * 64});
    stage_of.push_back(0);
    int xi = 1;  // index of the buffer holding the block input
    int final_buf = 1;
    for (size_t bi = 0; bi < h->blocks.size(); ++bi) {
        const Bneck& bk = h->blocks[bi];
        const bool last = (bi + 1 == h->blocks.size());
        int free_idx[3], nf = 0;
        for (int i = 0; i < 4; ++i)
            if (i != xi) free_idx[nf++] = i;
        const int t1 = free_idx[0], t2 = free_idx[1], idb = free_idx[2];
        const int stage = bk.c1.name[5] - '0';   // "layerN.b.conv1"
        const std::string p = "backbone." + bk.c1.name.substr(0, bk.c1.name.rfind('.'));
        const int bstride = bk.basic ? bk.c1.stride : bk.c2.stride;
        const int oh = conv_out(ch, 3, bstride, 1), ow = conv_out(cw, 3, bstride, 1);
        auto add = [&](const ConvW& c, int in, int out, int res, int ih, int iw, int ooh, int oow, int relu, const char* nm) {
            ops.push_back({2, &c, in, out, res, ih, iw, ooh, oow, relu, p + nm, (size_t)ih * iw * c.cin, (size_t)ooh * oow * c.cout});
            stage_of.push_back(stage);
        };
        if (bk.basic) {
            // BasicBlock: relu(bn1(conv3x3_s(x))) -> relu(bn2(conv3x3(.)) + identity | downsample(x))
            add(bk.c1, xi, t1, -1, ch, cw, oh, ow, 1, ".conv1");
            int identity = xi;
            if (bk.has_ds) {
                add(bk.ds, xi, idb, -1, ch, cw, oh, ow, 0, ".downsample");
                identity = idb;
            }
            const int out = (last && feat_out) ? -2 : t2;
            add(bk.c2, t1, out, identity, oh, ow, oh, ow, 1, ".conv2");
            ch = oh; cw = ow;
            xi = out;
            final_buf = out;
            continue;
        }
        add(bk.c1, xi, t1, -1, ch, cw, ch, cw, 1, ".conv1");
        add(bk.c2, t1, t2, -1, ch, cw, oh, ow, 1, ".conv2");
        int identity = xi;
        const bool fuse = bk.has_ds && (bk.f_w || bk.f_w16) && opt(h, OPT_fuse_downsample);
        if (bk.has_ds && !fuse) {
            add(bk.ds, xi, idb, -1, ch, cw, oh, ow, 0, ".downsample");
            identity = idb;
        }
        const int out = (last && feat_out) ? -2 : t1;  // t1 is dead after conv2
        add(bk.c3, t2, out, fuse ? -1 : identity, oh, ow, oh, ow, 1, fuse ? ".conv3+downsample" : ".conv3");
        if (fuse) {
            TrunkOp& o = ops.back();
            o.fused = &bk; o.in2_buf = xi; o.H2 = ch; o.W2 = cw; o.in2_img = (size_t)ch * cw * bk.ds.cin;
        }
        ch = oh; cw = ow;
        xi = t1;
        final_buf = out;
    }
    P.final_buf = final_buf; P.fh = ch; P.fw = cw;
}

// Launch ops [first, n) of a trunk (hb == nullptr) or of a trunk pair, one op at a time.  Every op is prepared (and, for a pair,
// checked against its twin) before the first launch.
static int launch_ops(specmi_handle* ha, specmi_handle* hb, const TrunkPlan& Pa, const TrunkPlan* Pb, const float* img_a, const float* img_b,
                      int B, int H, int W, float* feat_a, float* feat_b, size_t first, int mode, hipStream_t s) {
    const size_t n = Pa.ops.size();
    std::vector<OpLaunch> La(n), Lb(hb ? n : 0);
    for (size_t i = first; i < n; ++i) {
        La[i] = prepare_op(ha, Pa.ops[i], img_a, feat_a, 0, B, H, W, mode);
        if (!hb) continue;
        Lb[i] = prepare_op(hb, Pb->ops[i], img_b, feat_b, 0, B, H, W, mode);
        OpLaunch &A = La[i], &Bp = Lb[i];
        if (A.kind == 2 && Bp.kind == 2 && A.family != 2 && Bp.family != 2 && (Bp.family != A.family || Bp.sk != A.sk)) {
            // the kernel choice reads per-handle options ("winograd", "latency_*"): the pair follows the first handle
            Bp.family = A.family; Bp.sk = A.sk;
            Bp.a.w = A.family == 1 ? Pb->ops[i].c->wino : (Pb->ops[i].fused ? Pb->ops[i].fused->f_w : Pb->ops[i].c->w);
            if (A.family == 1 && !Bp.a.w) return fail(ha, SPECMI_ERR_ARG, "op %zu: the second trunk has no Winograd filters", i);
        }
        const TrunkOp &oa = Pa.ops[i], &ob = Pb->ops[i];
        if (A.kind != Bp.kind || A.family != Bp.family || oa.H != ob.H || oa.W != ob.W || oa.OH != ob.OH || oa.OW != ob.OW ||
            (A.kind == 2 && (oa.c->cin != ob.c->cin || oa.c->cout != ob.c->cout || oa.c->k != ob.c->k || oa.c->stride != ob.c->stride ||
                             (oa.fused != nullptr) != (ob.fused != nullptr) || oa.relu != ob.relu)))
            return fail(ha, SPECMI_ERR_ARG, "op %zu (%s) differs between the two trunks: grouped launches need identical layer shapes",
                        i, oa.label.c_str());
    }
    for (size_t i = first; i < n; ++i)
        if (int rc = launch_op(ha, Pa.ops[i], La[i], hb ? &Lb[i] : nullptr, B, H, W, s)) return rc;
    return SPECMI_OK;
}

// The fp16 trunk (precision SPECMI_PRECISION_FP16, conv_f16.hip): the same op list and ping-pong buffers as the fp32 trunk,
// holding fp16 NHWC activations (half the bytes of the fp32 workspace the same warm-up rule sizes: nothing is allocated under
// graph capture).  The image is converted into act[1] (free until the max-pool writes it), every convolution - the stem
// included - is one conv_f16 launch, and the last one stores fp32 for the heads.  One kernel family at every batch size:
// plan, Winograd, wave-split / sub-batch options do not apply.
// images16 != nullptr (the *_f16in entry points): the caller's NHWC8 fp16 image is the stem's input where it lies and the
// conversion launch is skipped; launch_conv_f16 cuts a batch past 2 GiB into whole images of whichever buffer it is given.
static int run_trunk_f16(specmi_handle* h, const float* images, const void* images16, int B, int H, int W, float* feat_out,
                         const float** feat, int* fh, int* fw, hipStream_t s) {
    TrunkPlan P;
    plan_trunk(h, H, W, feat_out != nullptr, P);
    auto buf = [&](int idx) -> void* { return idx == -2 ? static_cast<void*>(feat_out) : static_cast<void*>(h->act[idx]); };
    const size_t n = P.ops.size();
    for (size_t i = 0; i < n; ++i) {
        const TrunkOp& op = P.ops[i];
        LaunchCtx ctx{s, &h->prof, op.label.c_str()};
        if (op.kind == 1) {
            LAUNCHCHK(h, launch_maxpool_f16(buf(op.in_buf), buf(op.out_buf), B, op.H, op.W, 64, op.OH, op.OW, ctx), "maxpool_f16");
            continue;
        }
        ConvF16Args a;
        const ConvW& c = op.kind == 0 ? h->stem : *op.c;
        if (op.kind == 0 && images16) {
            a.x = images16; a.ldx = 8;
        } else if (op.kind == 0) {
            LaunchCtx cctx{s, &h->prof, "backbone.input_f16"};
            LAUNCHCHK(h, launch_to_nhwc_f16(images, h->act[1], B, 3, H, W, cctx), "to_nhwc_f16");
            a.x = h->act[1]; a.ldx = 8;
        } else {
            a.x = buf(op.in_buf); a.ldx = c.cin;
        }
        a.w = c.w16; a.shift = c.shift; a.Kp = c.Kp16; a.Npad = c.Npad;
        a.res = op.res_buf == -1 ? nullptr : buf(op.res_buf);
        a.out = buf(op.out_buf);
        a.B = B; a.H = op.H; a.W = op.W; a.Cin = c.cin; a.OH = op.OH; a.OW = op.OW; a.Cout = c.cout; a.ldo = c.cout;
        a.KH = c.k; a.KW = c.k; a.stride = c.stride; a.pad = c.pad; a.relu = op.relu;
        a.out_f32 = i + 1 == n;
        if (op.fused) {
            const Bneck& bk = *op.fused;
            a.w = bk.f_w16; a.shift = bk.f_shift; a.Npad = bk.f_Npad; a.Kp = c.cin + bk.ds.cin;
            a.x2 = buf(op.in2_buf); a.H2 = op.H2; a.W2 = op.W2; a.ldx2 = bk.ds.cin; a.Cin2 = bk.ds.cin; a.stride2 = bk.ds.stride;
        }
        if (!a.w) return fail(h, SPECMI_ERR_STATE, "%s: no fp16 weights (commit at SPECMI_PRECISION_FP16 first)", op.label.c_str());
        LAUNCHCHK(h, launch_conv_f16(a, ctx), op.label.c_str());
    }
    *feat = P.final_buf == -2 ? feat_out : h->act[P.final_buf];
    *fh = P.fh; *fw = P.fw;
    return SPECMI_OK;
}

// images NCHW -> layer4 map NHWC in *feat (a workspace buffer unless feat_out given).
// Option "trunk_subbatch" = S > 0: the stem, the max-pool and the first "trunk_subbatch_layers"
// ResNet stages are run S images at a time (activations of a slice are <= 103 MB at S = 32 and stay
// resident in the 256 MiB Infinity Cache between layers); later stages see the whole batch.
// images16 (NHWC8 fp16, include/specmi.h) in place of images: the fp16 ResNet trunk only; refused before anything is allocated or launched.
static int run_trunk(specmi_handle* h, const float* images, int B, int H, int W, float* feat_out, const float** feat,
                     int* fh, int* fw, hipStream_t s, const void* images16 = nullptr, int n_stages = 4) {
    int rc;
    if (images16) {
        if (h->hrnet) return fail(h, SPECMI_ERR_STATE, "fp16 NHWC8 images feed the fp16 ResNet trunk: this handle has an HRNet trunk");
        if (h->committed_precision != SPECMI_PRECISION_FP16)
            return fail(h, SPECMI_ERR_STATE, "fp16 NHWC8 images feed the fp16 trunk: commit at SPECMI_PRECISION_FP16 first");
        if (reinterpret_cast<uintptr_t>(images16) & 15) return fail(h, SPECMI_ERR_ARG, "images_nhwc8 is not 16-byte aligned");
    }
    if (H < 32 || W < 32) return fail(h, SPECMI_ERR_ARG, "image size %dx%d too small", H, W);
    if ((rc = ensure_ws(h, B, H, W))) return rc;
    if (h->hrnet) {
        if ((rc = hrnet_forward(h, images, B, H, W, feat_out, fh, fw, s))) return rc;
        *feat = feat_out ? feat_out : hrnet_feat_ws(h);
        return SPECMI_OK;
    }
    if (h->committed_precision == SPECMI_PRECISION_FP16) return run_trunk_f16(h, images, images16, B, H, W, feat_out, feat, fh, fw, s);
    TrunkPlan P;
    plan_trunk(h, H, W, feat_out != nullptr, P);
    if (n_stages < 4) {
        // specmi_trunk_forward_stages: the same list cut after the last op of layer{n_stages}, which writes the caller's buffer
        size_t n = 0;
        while (n < P.ops.size() && P.stage_of[n] <= n_stages) ++n;
        P.ops.resize(n); P.stage_of.resize(n);
        P.ops.back().out_buf = -2;
        P.final_buf = -2; P.fh = P.ops.back().OH; P.fw = P.ops.back().OW;
    }
    const std::vector<TrunkOp>& ops = P.ops;
    const std::vector<int>& stage_of = P.stage_of;
    const int final_buf = P.final_buf, ch = P.fh, cw = P.fw;
    const int S = opt(h, OPT_trunk_subbatch);
    const int Lsplit = opt(h, OPT_trunk_subbatch_layers);
    const int mode = trunk_mode(h, B, H, W);
    size_t first_full = 0;
    if (S > 0 && S < B) {
        while (first_full < ops.size() && stage_of[first_full] <= Lsplit) ++first_full;
        for (int b0 = 0; b0 < B; b0 += S) {
            const int nb = (B - b0 < S) ? B - b0 : S;
            for (size_t i = 0; i < first_full; ++i)
                if ((rc = exec_op(h, ops[i], images, feat_out, b0, nb, H, W, s, mode))) return rc;
        }
    }
    if ((rc = launch_ops(h, nullptr, P, nullptr, images, nullptr, B, H, W, feat_out, nullptr, first_full, mode, s))) return rc;
    *feat = final_buf == -2 ? feat_out : h->act[final_buf];
    *fh = ch; *fw = cw;
    return SPECMI_OK;
}


// The two ResNet trunks of the path (CamCalib + SPEC: same depth, same input size) walked in lockstep, every layer of both
// as ONE grouped launch (SURVEY.md 7, step 7's alternative to two streams): half the launches, no side-stream join, and the
// last, partially filled round of workgroups of one network is filled by the other.  Each network keeps its own weights and
// activation buffers; an image's result is bit-identical to the separate launches (same kernels, same k order).
static int run_trunk_pair(specmi_handle* ha, specmi_handle* hb, const float* img_a, const float* img_b, int B, int H, int W,
                          float* feat_a, float* feat_b, hipStream_t s) {
    int rc;
    if (H < 32 || W < 32) return fail(ha, SPECMI_ERR_ARG, "image size %dx%d too small", H, W);
    if (ha->committed_precision == SPECMI_PRECISION_FP16 || hb->committed_precision == SPECMI_PRECISION_FP16) {
        // the fp16 trunk has no grouped launches: two single-trunk calls on the stream (the same bits as two calls, by definition)
        const float* f; int fh, fw;
        if ((rc = run_trunk(ha, img_a, B, H, W, feat_a, &f, &fh, &fw, s))) return rc;
        if ((rc = run_trunk(hb, img_b, B, H, W, feat_b, &f, &fh, &fw, s))) { ha->err = hb->err; return rc; }
        return SPECMI_OK;
    }
    if ((rc = ensure_ws(ha, B, H, W))) return rc;
    if ((rc = ensure_ws(hb, B, H, W))) { ha->err = hb->err; return rc; }
    TrunkPlan Pa, Pb;
    plan_trunk(ha, H, W, true, Pa);
    plan_trunk(hb, H, W, true, Pb);
    if (Pa.ops.size() != Pb.ops.size()) return fail(ha, SPECMI_ERR_ARG, "the two trunks have different depths");
    const int mode = trunk_mode(ha, B, H, W, true);   // the first handle's options decide for the pair
    return launch_ops(ha, hb, Pa, &Pb, img_a, img_b, B, H, W, feat_a, feat_b, 0, mode, s);
}

// per-image strides of the HMR outputs: dense, or all equal to option "output_ld" (the outputs are then columns of
// one caller-owned (B, output_ld) record, e.g. the packed all-gather record of SURVEY.md 8e)
struct OutLd {
    long pose = 216, shape = 10, cam = 3, p6d = 144, verts = 0, j3d = 147, j2d = 98, camt = 3;
};
static OutLd out_ld(specmi_handle* h) {
    OutLd o;
    const long ld = opt(h, OPT_output_ld);
    if (ld > 0) o.pose = o.shape = o.cam = o.p6d = o.verts = o.j3d = o.j2d = o.camt = ld;
    return o;
}

// defer != nullptr: head_final is not launched; *defer describes it for the SMPL pose kernel, which does its work (run_smpl)
static int run_head(specmi_handle* h, const float* feat, int B, int fh, int fw, const float* R, const float* K,
                    const float* img_h, float* pred_pose, float* pred_shape, float* pred_cam, float* pred_pose_6d,
                    const OutLd& old, hipStream_t s, HeadFinal* defer = nullptr) {
    int rc;
    const int ucf = opt(h, OPT_use_cam_feats);
    const int F = h->feat_ch, LD = h->xc_ld;
    if (ucf && (!R || !K || !img_h))
        return fail(h, SPECMI_ERR_ARG, "use_cam_feats needs cam_rotmat, cam_intrinsics and img_h");
    // the IEF state columns are written by extra workgroups of the pooling launch (option "head_fuse" bit 0, default on; large
    // maps pool in parts and keep head_init as its own launch)
    const HeadInit hi{h->xc, h->init_pose, h->init_shape, h->init_cam, R, K, img_h, ucf, F, LD};
    bool init_done = false;
    {
        LaunchCtx ctx{s, &h->prof, "head.avgpool"};
        LAUNCHCHK(h, launch_avgpool(feat, h->xc, B, fh * fw, F, LD, ctx, (opt(h, OPT_head_fuse) & 1) ? &hi : nullptr, &init_done), "avgpool");
    }
    if (!init_done) {
        LaunchCtx ctx{s, &h->prof, "head.init"};
        LAUNCHCHK(h, launch_head_init(h->xc, h->init_pose, h->init_shape, h->init_cam, R, K, img_h, ucf, B, F, LD, ctx),
                  "head_init");
    }
    const float* state = h->xc + F;
    long ld_state = LD;
    const bool gemv = use_latency_heads(h, B);
    auto fc = [&](const FcW& w, const float* x, int ldx, const float* res, float* out, int ldo, const char* label) -> int {
        if (gemv && w.w_rm) {     // latency plan: one wave per output column (head.hip: fc_gemv_kernel)
            const FcGemv hd{x, w.w_rm, w.shift, res, out};
            LaunchCtx ctx{s, &h->prof, label};
            LAUNCHCHK(h, launch_fc_gemv(&hd, 1, w.nout, w.Kp, ldx, ldo, B, ctx), label);
            return SPECMI_OK;
        }
        return run_fc(h, w, x, ldx, B, res, out, ldo, s, label);
    };
    if (h->has_head_c && opt(h, OPT_head_collapse)) {
        // the three IEF iterations as one composed affine map (commit_head_collapsed)
        if ((rc = fc(h->head_c, h->xc, LD, nullptr, h->h1, 1024, "head.ief_collapsed"))) return rc;
        state = h->h1;
        ld_state = 1024;
        h->last_var = h->has_var ? h->h1 + 157 : nullptr;      // (the composed map's 154 extra output columns)
        h->last_ld_var = 1024;
    } else {
        for (int it = 0; it < 3; ++it) {
            if ((rc = fc(h->fc1, h->xc, LD, nullptr, h->h1, 1024, "head.fc1"))) return rc;
            if ((rc = fc(h->fc2, h->h1, 1024, nullptr, h->h2, 1024, "head.fc2"))) return rc;
            // the variance decoders read the SAME xc as this iteration's mean decoders; only the last iteration's survive
            if (it == 2 && h->has_var && (rc = fc(h->head_var, h->h2, 1024, nullptr, h->h1, 1024, "head.dec_var"))) return rc;
            float* st = h->xc + F;  // dec* + running estimate, in place
            if ((rc = fc(h->dec, h->h2, 1024, st, st, LD, "head.dec"))) return rc;
        }
        h->last_var = h->has_var ? h->h1 : nullptr;
        h->last_ld_var = 1024;
    }
    h->last_state = state; h->last_ld_state = ld_state; h->last_B = B;
    if (defer) {
        defer->state = state; defer->ld_state = ld_state;
        defer->pred_pose = pred_pose; defer->pred_shape = pred_shape; defer->pred_cam = pred_cam; defer->pred_pose_6d = pred_pose_6d;
        defer->ld_pose = old.pose; defer->ld_shape = old.shape; defer->ld_cam = old.cam; defer->ld_p6d = old.p6d;
        defer->rot_ws = h->rot_ws; defer->betas_ws = h->betas_ws; defer->cam_ws = h->cam_ws;
    } else {
        LaunchCtx ctx{s, &h->prof, "head.final"};
        const long ld[4] = {old.pose, old.shape, old.cam, old.p6d};
        LAUNCHCHK(h, launch_head_final(state, ld_state, pred_pose, pred_shape, pred_cam, pred_pose_6d, ld, h->rot_ws,
                                       h->betas_ws, h->cam_ws, B, ctx),
                  "head_final");
    }
    return SPECMI_OK;
}

static int run_smpl(specmi_handle* h, const float* rotmat, const float* betas, const float* cam, int B, const float* R,
                    const float* K, const float* bbox_scale, const float* bbox_center, const float* img_w,
                    const float* img_h, float* vertices, float* joints3d, float* joints2d, float* cam_t,
                    const OutLd& old, hipStream_t s, const HeadFinal* final_ = nullptr) {
    const int use_cam = opt(h, OPT_use_cam);
    if (use_cam && (!R || !K || !bbox_scale || !bbox_center || !img_w || !img_h))
        return fail(h, SPECMI_ERR_ARG, "use_cam needs cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h");
    SmplArgs a;
    a.rotmat = rotmat; a.betas = betas; a.cam = cam; a.cam_rotmat = R; a.cam_intrinsics = K;
    a.bbox_scale = bbox_scale; a.bbox_center = bbox_center; a.img_w = img_w; a.img_h = img_h;
    a.vertices = vertices ? vertices : h->verts_ws;
    a.ld_verts = vertices ? old.verts : 0;
    a.joints3d = joints3d; a.joints2d = joints2d; a.cam_t = cam_t;
    a.ld_j3d = old.j3d; a.ld_j2d = old.j2d; a.ld_camt = old.camt;
    a.pose_feat = h->pf_ws; a.A = h->A_ws; a.posed_j = h->pj_ws;
    a.B = B;
    a.mode = use_cam ? 0 : 1;
    a.focal_length = h->focal_length;
    a.img_res = (float)opt(h, OPT_img_res);
    a.normalize_joints2d = use_cam ? 0 : 1;  // spec/models/hmr.py:111 vs :119
    a.skin_split = opt(h, OPT_smpl_skin_split);
    a.final_ = final_;
    LaunchCtx ctx{s, &h->prof, "smpl"};
    LAUNCHCHK(h, launch_smpl(h->smpl, a, ctx), "smpl");
    return SPECMI_OK;
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* specmi_version(void) { return "specmi 0.6 (gfx950, fp32 MFMA)"; }

int specmi_create(specmi_handle** out, int device_id, int model_kind) {
    if (!out) return fail(nullptr, SPECMI_ERR_ARG, "out is NULL");
    if (model_kind != SPECMI_MODEL_CAMCALIB && model_kind != SPECMI_MODEL_HMR && model_kind != SPECMI_MODEL_SMPL)
        return fail(nullptr, SPECMI_ERR_ARG, "unknown model kind %d", model_kind);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, SPECMI_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, SPECMI_ERR_ARG, "device %d out of range [0,%d)", device_id, n);
    specmi_handle* h = new specmi_handle();
    h->device = device_id;
    h->kind = model_kind;
    build_resnet(h, 50);
    *out = h;
    return SPECMI_OK;
}

int specmi_destroy(specmi_handle* h) {
    if (!h) return SPECMI_OK;
    DeviceGuard guard;
    (void)guard.enter(h->device);
    (void)hipDeviceSynchronize();
    for (auto& r : h->prof.log) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    free_pool(h->ws_allocs);
    free_pool(h->param_allocs);
    if (h->sk.ws) (void)hipFree(h->sk.ws);
    if (h->sk.cnt) (void)hipFree(h->sk.cnt);
    free_pool(h->sk_retired);
    free_pool(h->ws_retired);
    if (h->resize_tab) (void)hipFree(h->resize_tab);
    for (DevTable& t : h->tab) (void)hipFree(t.dev.p);       // hipFree(nullptr) is a no-op
    for (DevBuf& b : h->buf) (void)hipFree(b.p);
    hrnet_free(h->hrnet);
    delete h;
    return SPECMI_OK;
}

const char* specmi_last_error(const specmi_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

static int stage(specmi_handle* h, const char* name, const void* data, const int64_t* shape, int ndim, bool is_int) {
    if (!h || !name || !data || (ndim > 0 && !shape) || ndim < 0 || ndim > 8) return fail(h, SPECMI_ERR_ARG, "bad argument to set_tensor");
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) return fail(h, SPECMI_ERR_ARG, "negative dimension in '%s'", name);
        n *= (size_t)shape[i];
    }
    HostTensor t;
    t.is_int = is_int;
    t.shape.assign(shape, shape + ndim);
    if (is_int) t.i.assign((const int32_t*)data, (const int32_t*)data + n);
    else t.f.assign((const float*)data, (const float*)data + n);
    h->staged[name] = std::move(t);
    return SPECMI_OK;
}

int specmi_set_tensor_f32(specmi_handle* h, const char* name, const float* d, const int64_t* shape, int ndim) {
    return stage(h, name, d, shape, ndim, false);
}
int specmi_set_tensor_i32(specmi_handle* h, const char* name, const int32_t* d, const int64_t* shape, int ndim) {
    return stage(h, name, d, shape, ndim, true);
}

int specmi_commit(specmi_handle* h) {
    if (!h) return SPECMI_ERR_ARG;
    DeviceGuard guard;
    HIPCHK(h, guard.enter(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    reset_sync_state(h, nullptr);
    HIPCHK(h, hipDeviceSynchronize());
    free_pool(h->param_allocs);
    h->committed = false;
    int rc;
    if (h->kind == SPECMI_MODEL_SMPL) {   // the body model alone (evaluation: ground-truth meshes / joints)
        if ((rc = commit_smpl(h))) return rc;
        free_pool(h->ws_allocs);
        h->act_elems = 0; h->ws_B = 0;
        h->committed = true;
        h->committed_precision = h->precision;
        return SPECMI_OK;
    }
    const std::string bp = "backbone.";
    const int depth = opt(h, OPT_backbone);
    if (depth != 50 && depth != 34 && depth != 18 && depth != 101 && depth != 152 && depth != 32 && depth != 48)
        return fail(h, SPECMI_ERR_ARG, "backbone %d: resnet18 / 34 / 50 / 101 / 152, hrnet_w32 (32) and hrnet_w48 (48) are built", depth);
    if ((depth == 32 || depth == 48) && h->kind != SPECMI_MODEL_HMR)
        return fail(h, SPECMI_ERR_ARG, "the HRNet trunks belong to HMR (camcalib/model.py:33 builds resnet trunks only)");
    if ((depth == 32 || depth == 48) && h->precision != SPECMI_PRECISION_FP32)
        return fail(h, SPECMI_ERR_ARG, "the HRNet backbones are built at SPECMI_PRECISION_FP32 only");
    if (h->hrnet) { hrnet_free(h->hrnet); h->hrnet = nullptr; }
    if (depth == 32 || depth == 48) {
        h->blocks.clear();
        if ((rc = hrnet_commit(h, bp, depth, opt(h, OPT_hrnet_use_conv)))) return rc;
    } else {
        build_resnet(h, depth);
        if ((rc = commit_conv(h, bp, h->stem))) return rc;
        for (Bneck& b : h->blocks) {
            if ((rc = commit_conv(h, bp, b.c1))) return rc;
            if ((rc = commit_conv(h, bp, b.c2))) return rc;
            if (!b.basic && (rc = commit_conv(h, bp, b.c3))) return rc;
            if (b.has_ds && (rc = commit_conv(h, bp, b.ds))) return rc;
            if (!b.basic && b.has_ds && b.c3.cin % 32 == 0 && b.ds.cin % 32 == 0 && (rc = commit_fused_ds(h, bp, b))) return rc;
        }
    }
    if (h->kind == SPECMI_MODEL_CAMCALIB) {
        // camcalib/model.py:39-57: one Linear per angle, or Sequential(Linear x num_fc_layers) WITHOUT activations
        const char* names[3] = {"fc_vfov", "fc_pitch", "fc_roll"};
        const int L = opt(h, OPT_num_fc_layers), hc = opt(h, OPT_num_fc_channels);
        if (L < 1 || L > 3 || hc < 1 || hc > 1024) return fail(h, SPECMI_ERR_ARG, "num_fc_layers in 1..3 and num_fc_channels <= 1024 are built");
        h->fc_layers = L;
        const std::string lastw = L == 1 ? std::string("fc_vfov.weight") : "fc_vfov." + std::to_string(L - 1) + ".weight";
        const HostTensor* w0 = find(h, lastw);
        if (!w0) return fail(h, SPECMI_ERR_MISSING, "missing tensor '%s'", lastw.c_str());
        const int last_in = L == 1 ? h->feat_ch : hc;
        const int nb = (int)(w0->numel() / last_in);
        for (int i = 0; i < 3; ++i)
            for (int l = 0; l < L; ++l) {
                const std::string nm = L == 1 ? std::string(names[i]) : std::string(names[i]) + "." + std::to_string(l);
                const int nin = l == 0 ? h->feat_ch : hc, nout = l == L - 1 ? nb : hc;
                if ((rc = commit_fc(h, {nm}, {nout}, nin, h->fc_cam[i][l]))) return rc;
            }
    } else {
        const int ucf = opt(h, OPT_use_cam_feats);
        const int nin = h->feat_ch + 144 + 13 + (ucf ? 7 : 0);
        h->xc_ld = round_up(h->feat_ch + 164, 32);
        h->has_head_c = false;
        if ((rc = commit_fc(h, {"head.fc1"}, {1024}, nin, h->fc1))) return rc;
        if ((rc = commit_fc(h, {"head.fc2"}, {1024}, 1024, h->fc2))) return rc;
        if ((rc = commit_fc(h, {"head.decpose", "head.decshape", "head.deccam"}, {144, 10, 3}, 1024, h->dec))) return rc;
        h->has_var = opt(h, OPT_estimate_var) != 0;
        if (h->has_var && (rc = commit_fc(h, {"head.decpose_var", "head.decshape_var"}, {144, 10}, 1024, h->head_var))) return rc;
        h->last_state = h->last_var = nullptr; h->last_B = 0;
        const HostTensor *ip, *is, *ic;
        if ((rc = need(h, "head.init_pose", {144}, false, &ip))) return rc;
        if ((rc = need(h, "head.init_shape", {10}, false, &is))) return rc;
        if ((rc = need(h, "head.init_cam", {3}, false, &ic))) return rc;
        if ((rc = dev_upload(h, ip->f.data(), 144 * 4, (void**)&h->init_pose, h->param_allocs))) return rc;
        if ((rc = dev_upload(h, is->f.data(), 10 * 4, (void**)&h->init_shape, h->param_allocs))) return rc;
        if ((rc = dev_upload(h, ic->f.data(), 3 * 4, (void**)&h->init_cam, h->param_allocs))) return rc;
        if (opt(h, OPT_head_collapse) && (rc = commit_head_collapsed(h, h->feat_ch, ucf))) return rc;
        if ((rc = commit_smpl(h))) return rc;
        // the SMPL vertex count sizes the workspace
        free_pool(h->ws_allocs);
        h->act_elems = 0; h->ws_B = 0;
    }
    h->committed = true;
    h->committed_precision = h->precision;
    return SPECMI_OK;
}

#define ENTER(h)                                                                   \
    if (!(h)) return SPECMI_ERR_ARG;                                               \
    DeviceGuard dev_guard__;                                                       \
    HIPCHK(h, dev_guard__.enter((h)->device));

#define NEED_COMMIT(h) \
    if (!(h)->committed) return fail(h, SPECMI_ERR_STATE, "specmi_commit has not succeeded on this handle"); \
    if ((h)->precision != (h)->committed_precision) \
        return fail(h, SPECMI_ERR_STATE, "the precision changed since the last specmi_commit: commit again");

// specmi_trunk_forward and specmi_trunk_forward_f16in: exactly one of images / images16 is given
static int trunk_forward(specmi_handle* h, const float* images, const void* images16, int B, int H, int W, float* feat, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if ((!images && !images16) || !feat || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    const float* f; int fh, fw;
    const int rc = run_trunk(h, images, B, H, W, feat, &f, &fh, &fw, (hipStream_t)stream, images16);
    if (rc) reset_sync_state(h, (hipStream_t)stream);
    return rc;
}

int specmi_trunk_forward(specmi_handle* h, const float* images, int B, int H, int W, float* feat, void* stream) {
    return trunk_forward(h, images, nullptr, B, H, W, feat, stream);
}

int specmi_trunk_forward_stages(specmi_handle* h, const float* images, int B, int H, int W, int n_stages, float* out, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (!images || !out || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (n_stages < 1 || n_stages > 4) return fail(h, SPECMI_ERR_ARG, "trunk_forward_stages: n_stages = %d must be in 1 .. 4", n_stages);
    if (h->hrnet) return fail(h, SPECMI_ERR_STATE, "trunk_forward_stages: the handle has an HRNet trunk, which has no layer1 .. layer4");
    if (h->committed_precision == SPECMI_PRECISION_FP16)
        return fail(h, SPECMI_ERR_STATE, "trunk_forward_stages: the fp16 trunk is not cut into stages (commit at fp32)");
    if (h->blocks.empty()) return fail(h, SPECMI_ERR_STATE, "trunk_forward_stages: the handle has no ResNet trunk");
    const float* f; int fh, fw;
    const int rc = run_trunk(h, images, B, H, W, out, &f, &fh, &fw, (hipStream_t)stream, nullptr, n_stages);
    if (rc) reset_sync_state(h, (hipStream_t)stream);
    return rc;
}

int specmi_trunk_forward_f16in(specmi_handle* h, const void* images_nhwc8, int B, int H, int W, float* feat, void* stream) {
    return trunk_forward(h, nullptr, images_nhwc8, B, H, W, feat, stream);
}

int specmi_trunk_forward_pair(specmi_handle* ha, specmi_handle* hb, const float* images_a, const float* images_b, int B, int H,
                              int W, float* feat_a, float* feat_b, void* stream) {
    ENTER(ha); NEED_COMMIT(ha);
    if (!hb) return fail(ha, SPECMI_ERR_ARG, "second handle is NULL");
    if (!hb->committed) return fail(ha, SPECMI_ERR_STATE, "second handle not committed");
    if (hb->precision != hb->committed_precision)
        return fail(ha, SPECMI_ERR_STATE, "the precision of the second handle changed since its last specmi_commit: commit again");
    if (hb->device != ha->device) return fail(ha, SPECMI_ERR_ARG, "the two handles live on different devices");
    if (!images_a || !images_b || !feat_a || !feat_b || B <= 0) return fail(ha, SPECMI_ERR_ARG, "bad argument");
    if (ha->hrnet || hb->hrnet || ha->blocks.size() != hb->blocks.size() || ha->blocks.empty() ||
        ha->blocks[0].basic != hb->blocks[0].basic)
        return fail(ha, SPECMI_ERR_ARG, "grouped trunk launches need two ResNet trunks of the same depth");
    const int rc = run_trunk_pair(ha, hb, images_a, images_b, B, H, W, feat_a, feat_b, (hipStream_t)stream);
    if (rc) reset_sync_state(ha, (hipStream_t)stream);
    return rc;
}

static int run_camcalib_head(specmi_handle* h, const float* f, int B, int fh, int fw, float* lv, float* lp, float* lr, hipStream_t s);

int specmi_camcalib_head_forward(specmi_handle* h, const float* feat, int B, int fh, int fw, float* lv, float* lp, float* lr,
                                 void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_CAMCALIB) return fail(h, SPECMI_ERR_STATE, "handle is not a CamCalib model");
    if (!feat || !lv || !lp || !lr || B <= 0 || fh <= 0 || fw <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    int rc;
    if ((rc = ensure_ws(h, B, 32, 32))) return rc;
    return run_camcalib_head(h, feat, B, fh, fw, lv, lp, lr, (hipStream_t)stream);
}

static int camcalib_forward(specmi_handle* h, const float* images, const void* images16, int B, int H, int W, float* lv, float* lp,
                            float* lr, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_CAMCALIB) return fail(h, SPECMI_ERR_STATE, "handle is not a CamCalib model");
    if ((!images && !images16) || !lv || !lp || !lr || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    const float* f; int fh, fw, rc;
    if ((rc = run_trunk(h, images, B, H, W, nullptr, &f, &fh, &fw, s, images16)) || (rc = run_camcalib_head(h, f, B, fh, fw, lv, lp, lr, s)))
        reset_sync_state(h, s);
    return rc;
}

int specmi_camcalib_forward(specmi_handle* h, const float* images, int B, int H, int W, float* lv, float* lp, float* lr,
                            void* stream) {
    return camcalib_forward(h, images, nullptr, B, H, W, lv, lp, lr, stream);
}

int specmi_camcalib_forward_f16in(specmi_handle* h, const void* images_nhwc8, int B, int H, int W, float* lv, float* lp, float* lr,
                                  void* stream) {
    return camcalib_forward(h, nullptr, images_nhwc8, B, H, W, lv, lp, lr, stream);
}

static int run_camcalib_head(specmi_handle* h, const float* f, int B, int fh, int fw, float* lv, float* lp, float* lr, hipStream_t s) {
    int rc;
    {
        LaunchCtx ctx{s, &h->prof, "avgpool"};
        LAUNCHCHK(h, launch_avgpool(f, h->xf, B, fh * fw, h->feat_ch, 2048, ctx), "avgpool");
    }
    float* outs[3] = {lv, lp, lr};
    const char* labels[3] = {"fc_vfov", "fc_pitch", "fc_roll"};
    if (use_latency_heads(h, B) && h->fc_cam[0][0].w_rm) {
        // latency plan: the three heads of a layer as ONE launch (head.hip: fc_gemv_kernel); Linear chains layer by layer
        const float* x[3] = {h->xf, h->xf, h->xf};
        int ldx = 2048;
        for (int l = 0; l < h->fc_layers; ++l) {
            const bool lastl = (l + 1 == h->fc_layers);
            FcGemv hd[3];
            // hidden rows of the three heads of layer l: fc_hidden[l & 1] holds them (3 x B x 1024), alternating with the layer that reads them
            const FcW& f0 = h->fc_cam[0][l];
            const int ldy = lastl ? f0.nout : 1024;
            for (int i = 0; i < 3; ++i) {
                const FcW& fc = h->fc_cam[i][l];
                if (fc.nout != f0.nout || fc.Kp != f0.Kp) return fail(h, SPECMI_ERR_STATE, "CamCalib heads differ in shape");
                hd[i] = FcGemv{x[i], fc.w_rm, fc.shift, nullptr, lastl ? outs[i] : h->fc_hidden[l & 1] + (size_t)i * B * 1024};
            }
            LaunchCtx ctx{s, &h->prof, "fc_vfov|pitch|roll"};
            LAUNCHCHK(h, launch_fc_gemv(hd, 3, f0.nout, f0.Kp, ldx, ldy, B, ctx), "fc heads");
            for (int i = 0; i < 3; ++i) x[i] = hd[i].out;
            ldx = ldy;
        }
        return SPECMI_OK;
    }
    for (int i = 0; i < 3; ++i) {
        // Linear chain (no activation in between, camcalib/model.py:59-70); hidden rows live in h1 / h2 (1024 wide)
        const float* x = h->xf;
        int ldx = 2048;
        for (int l = 0; l < h->fc_layers; ++l) {
            const FcW& fc = h->fc_cam[i][l];
            const bool lastl = (l + 1 == h->fc_layers);
            float* y = lastl ? outs[i] : (l == 0 ? h->h1 : h->h2);
            const int ldy = lastl ? fc.nout : 1024;
            if ((rc = run_fc(h, fc, x, ldx, B, nullptr, y, ldy, s, labels[i]))) return rc;
            x = y; ldx = ldy;
        }
    }
    return SPECMI_OK;
}

int specmi_camcalib_head_decode(specmi_handle* h, const float* feat, int B, int fh, int fw, float* lv, float* lp, float* lr,
                                const float* img_h, const float* img_w, float* vfov, float* pitch, float* roll, float* f_pix,
                                float* R, float* K, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_CAMCALIB) return fail(h, SPECMI_ERR_STATE, "handle is not a CamCalib model");
    if (!feat || !lv || !lp || !lr || B <= 0 || fh <= 0 || fw <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = ensure_ws(h, B, 32, 32))) return rc;
    const long ld_ang = opt(h, OPT_angle_ld) > 0 ? opt(h, OPT_angle_ld) : 1;
    if ((rc = run_camcalib_head(h, feat, B, fh, fw, lv, lp, lr, s))) { reset_sync_state(h, s); return rc; }
    LaunchCtx ctx{s, &h->prof, "camcalib.decode"};
    // the bins are the LAST Linear of a head's chain (num_fc_layers > 1: the first one is num_fc_channels wide, camcalib/model.py:59-70)
    const int nbins = h->fc_cam[0][h->fc_layers - 1].nout;
    LAUNCHCHK(h, launch_camcalib_decode(lv, lp, lr, B, nbins, img_h, img_w, vfov, pitch, roll, f_pix, R, K, ld_ang, ctx), "camcalib_decode");
    return SPECMI_OK;
}

int specmi_camcalib_decode(specmi_handle* h, const float* lv, const float* lp, const float* lr, int B, int nbins,
                           const float* img_h, const float* img_w, float* vfov, float* pitch, float* roll, float* f_pix,
                           float* R, float* K, void* stream) {
    ENTER(h);
    if (!lv || !lp || !lr || B <= 0 || nbins < 2) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if ((f_pix || K) && !img_h) return fail(h, SPECMI_ERR_ARG, "f_pix / K need img_h");
    if (K && !img_w) return fail(h, SPECMI_ERR_ARG, "K needs img_w");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.decode"};
    LAUNCHCHK(h, launch_camcalib_decode(lv, lp, lr, B, nbins, img_h, img_w, vfov, pitch, roll, f_pix, R, K,
                                        (long)(opt(h, OPT_angle_ld) > 0 ? opt(h, OPT_angle_ld) : 1), ctx), "decode");
    return SPECMI_OK;
}

int specmi_camcalib_bins(specmi_handle* h, const float* logits, int rows, int nbins, int32_t* argmax_idx,
                         float* soft_idx, void* stream) {
    ENTER(h);
    if (!logits || rows <= 0 || nbins < 2 || (!argmax_idx && !soft_idx)) return fail(h, SPECMI_ERR_ARG, "bad argument");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.bins"};
    LAUNCHCHK(h, launch_bins_reduce(logits, rows, nbins, argmax_idx, soft_idx, ctx), "bins_reduce");
    return SPECMI_OK;
}

int specmi_camcalib_eval(specmi_handle* h, const float* lv, const float* lp, const float* lr, int B, int nbins, int loss_type,
                         const void* target_vfov, const void* target_pitch, const void* target_roll, const float* gt_vfov,
                         const float* gt_pitch, const float* gt_roll, float w_vfov, float w_pitch, float w_roll, float* loss_term,
                         int32_t* argmax_idx, float* soft_idx, float* angle, float* abs_err, float* means, void* stream) {
    ENTER(h);
    if (!lv || !lp || !lr || B <= 0 || nbins < 2) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (loss_type < SPECMI_LOSS_CE || loss_type > SPECMI_LOSS_SOFTARGMAX_BIASED_L2)
        return fail(h, SPECMI_ERR_ARG, "loss_type %d is not defined (camcalib/loss.py:75-85: ce, kl, softargmax_l2, softargmax_biased_l2)", loss_type);
    if (!target_vfov || !target_pitch || !target_roll || !gt_vfov || !gt_pitch || !gt_roll)
        return fail(h, SPECMI_ERR_ARG, "targets and ground-truth angles of all three heads are needed");
    if (!loss_term || !argmax_idx || !soft_idx || !angle || !abs_err) return fail(h, SPECMI_ERR_ARG, "the five per-image outputs are needed");
    if ((double)B * nbins >= 2147483648.0) return fail(h, SPECMI_ERR_ARG, "B * nbins does not fit 31 bits");
    CamEvalArgs a;
    a.logits[0] = lv; a.logits[1] = lp; a.logits[2] = lr;
    a.target[0] = target_vfov; a.target[1] = target_pitch; a.target[2] = target_roll;
    a.gt[0] = gt_vfov; a.gt[1] = gt_pitch; a.gt[2] = gt_roll;
    a.B = B; a.nbins = nbins; a.loss_type = loss_type;
    a.weight[0] = w_vfov; a.weight[1] = w_pitch; a.weight[2] = w_roll;
    a.loss_term = loss_term; a.argmax = argmax_idx; a.soft = soft_idx; a.angle = angle; a.err = abs_err; a.means = means;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.eval"};
    LAUNCHCHK(h, launch_camcalib_eval(a, ctx), "camcalib_eval");
    return SPECMI_OK;
}

int specmi_cam_params(specmi_handle* h, const float* pitch, const float* roll, const float* f_pix, const float* img_w,
                      const float* img_h, int B, float* R, float* K, void* stream) {
    ENTER(h);
    if (!pitch || !roll || !f_pix || !img_w || !img_h || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.cam_params"};
    LAUNCHCHK(h, launch_cam_params(pitch, roll, f_pix, img_w, img_h, B, R, K, ctx), "cam_params");
    return SPECMI_OK;
}

int specmi_hmr_head_forward(specmi_handle* h, const float* feat, int B, int fh, int fw, const float* R, const float* K,
                            const float* img_h, float* pred_pose, float* pred_shape, float* pred_cam,
                            float* pred_pose_6d, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_HMR) return fail(h, SPECMI_ERR_STATE, "handle is not an HMR model");
    if (!feat || B <= 0 || fh <= 0 || fw <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    int rc;
    if ((rc = ensure_ws(h, B, 32, 32))) return rc;
    return run_head(h, feat, B, fh, fw, R, K, img_h, pred_pose, pred_shape, pred_cam, pred_pose_6d, out_ld(h),
                    (hipStream_t)stream);
}

int specmi_smpl_forward(specmi_handle* h, const float* rotmat, const float* betas, const float* cam, int B,
                        const float* R, const float* K, const float* bbox_scale, const float* bbox_center,
                        const float* img_w, const float* img_h, float* vertices, float* joints3d, float* joints2d,
                        float* cam_t, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_HMR && h->kind != SPECMI_MODEL_SMPL) return fail(h, SPECMI_ERR_STATE, "handle has no body model");
    if (!rotmat || !betas || !cam || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    int rc;
    if ((rc = ensure_ws(h, B, 32, 32))) return rc;
    return run_smpl(h, rotmat, betas, cam, B, R, K, bbox_scale, bbox_center, img_w, img_h, vertices, joints3d, joints2d,
                    cam_t, out_ld(h), (hipStream_t)stream);
}

int specmi_smpl_native(specmi_handle* h, const float* pose, int pose_is_axis_angle, const float* betas, int B,
                       float* vertices, float* joints24, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_HMR && h->kind != SPECMI_MODEL_SMPL) return fail(h, SPECMI_ERR_STATE, "handle has no body model");
    if (!pose || !betas || B <= 0 || (!vertices && !joints24)) return fail(h, SPECMI_ERR_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = ensure_ws(h, B, 32, 32))) return rc;
    const float* rot = pose;
    if (pose_is_axis_angle) {
        LaunchCtx ctx{s, &h->prof, "smpl.rodrigues"};
        LAUNCHCHK(h, launch_rodrigues(pose, h->rot_ws, B * 24, ctx), "rodrigues");
        rot = h->rot_ws;
    }
    SmplArgs a;
    a.rotmat = rot; a.betas = betas; a.cam = nullptr; a.cam_rotmat = nullptr; a.cam_intrinsics = nullptr;
    a.bbox_scale = a.bbox_center = a.img_w = a.img_h = nullptr;
    a.vertices = vertices; a.joints3d = a.joints2d = a.cam_t = nullptr;
    a.pose_feat = h->pf_ws; a.A = h->A_ws; a.posed_j = h->pj_ws;
    a.B = B; a.mode = 1; a.focal_length = 0.f; a.img_res = 0.f; a.normalize_joints2d = 0;
    a.skin_split = opt(h, OPT_smpl_skin_split);
    LaunchCtx ctx{s, &h->prof, "smpl.native"};
    LAUNCHCHK(h, launch_smpl_native(h->smpl, a, joints24, ctx), "smpl_native");
    return SPECMI_OK;
}

static int hmr_forward(specmi_handle* h, const float* images, const void* images16, int B, int H, int W, const float* R, const float* K,
                       const float* bbox_scale, const float* bbox_center, const float* img_w, const float* img_h,
                       const specmi_hmr_outputs* out, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_HMR) return fail(h, SPECMI_ERR_STATE, "handle is not an HMR model");
    if ((!images && !images16) || !out || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    const float* f; int fh, fw, rc;
    if ((rc = run_trunk(h, images, B, H, W, nullptr, &f, &fh, &fw, s, images16))) { reset_sync_state(h, s); return rc; }
    const OutLd old = out_ld(h);
    HeadFinal fin;
    const bool fuse = (opt(h, OPT_head_fuse) & 2) != 0;     // head_final's work inside the SMPL pose kernel (same bits, one node less)
    if ((rc = run_head(h, f, B, fh, fw, R, K, img_h, out->pred_pose, out->pred_shape, out->pred_cam, out->pred_pose_6d, old, s,
                       fuse ? &fin : nullptr)) ||
        (rc = run_smpl(h, h->rot_ws, h->betas_ws, h->cam_ws, B, R, K, bbox_scale, bbox_center, img_w, img_h,
                       out->smpl_vertices, out->smpl_joints3d, out->smpl_joints2d, out->pred_cam_t, old, s, fuse ? &fin : nullptr)))
        reset_sync_state(h, s);      // include/specmi.h: the hand-off counters are reset after any forward that returned an error
    return rc;
}

int specmi_hmr_forward(specmi_handle* h, const float* images, int B, int H, int W, const float* R, const float* K,
                       const float* bbox_scale, const float* bbox_center, const float* img_w, const float* img_h,
                       const specmi_hmr_outputs* out, void* stream) {
    return hmr_forward(h, images, nullptr, B, H, W, R, K, bbox_scale, bbox_center, img_w, img_h, out, stream);
}

int specmi_hmr_forward_f16in(specmi_handle* h, const void* images_nhwc8, int B, int H, int W, const float* R, const float* K,
                             const float* bbox_scale, const float* bbox_center, const float* img_w, const float* img_h,
                             const specmi_hmr_outputs* out, void* stream) {
    return hmr_forward(h, nullptr, images_nhwc8, B, H, W, R, K, bbox_scale, bbox_center, img_w, img_h, out, stream);
}

int specmi_hmr_regress(specmi_handle* h, const float* feat, int B, int fh, int fw, const float* R, const float* K,
                       const float* bbox_scale, const float* bbox_center, const float* img_w, const float* img_h,
                       const specmi_hmr_outputs* out, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_HMR) return fail(h, SPECMI_ERR_STATE, "handle is not an HMR model");
    if (!feat || !out || B <= 0 || fh <= 0 || fw <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = ensure_ws(h, B, 32, 32))) return rc;
    const OutLd old = out_ld(h);
    HeadFinal fin;
    const bool fuse = (opt(h, OPT_head_fuse) & 2) != 0;     // head_final's work inside the SMPL pose kernel (same bits, one node less)
    if ((rc = run_head(h, feat, B, fh, fw, R, K, img_h, out->pred_pose, out->pred_shape, out->pred_cam, out->pred_pose_6d, old, s,
                       fuse ? &fin : nullptr)) ||
        (rc = run_smpl(h, h->rot_ws, h->betas_ws, h->cam_ws, B, R, K, bbox_scale, bbox_center, img_w, img_h,
                       out->smpl_vertices, out->smpl_joints3d, out->smpl_joints2d, out->pred_cam_t, old, s, fuse ? &fin : nullptr)))
        reset_sync_state(h, s);
    return rc;
}

int specmi_hmr_uncertainty(specmi_handle* h, int B, float* pred_pose_var, float* pred_shape_var, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_HMR) return fail(h, SPECMI_ERR_STATE, "handle is not an HMR model");
    if (!h->has_var) return fail(h, SPECMI_ERR_STATE, "the model was committed without option \"estimate_var\"");
    if (!pred_pose_var || !pred_shape_var || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (!h->last_state || !h->last_var || h->last_B != B)
        return fail(h, SPECMI_ERR_STATE, "specmi_hmr_uncertainty follows a head forward of the same batch (%d) on the same stream; the last one had %d",
                    B, h->last_B);
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "head.var"};
    LAUNCHCHK(h, launch_head_var(h->last_state, h->last_ld_state, h->last_var, h->last_ld_var, opt(h, OPT_uncertainty_activation), pred_pose_var,
                                 pred_shape_var, B, ctx), "head_var");
    return SPECMI_OK;
}

int specmi_conv2d(specmi_handle* h, const float* x, int B, int H, int W, int Cin, const float* w_host,
                  const float* scale_host, const float* shift_host, int Cout, int KH, int KW, int stride, int pad,
                  const float* residual, int relu, float* out, void* stream) {
    return specmi_conv2d_strided(h, x, B, H, W, Cin, Cin, w_host, scale_host, shift_host, Cout, KH, KW, stride, pad, residual, relu,
                                 out, Cout, nullptr, 0, 0, 0, 0, 1, stream);
}

// The layer as the trunks launch it: channel strides on both sides (HRNet's padded maps and concat slices) and the second A
// source of a bottleneck's conv3 with the downsample folded in.  specmi_conv2d is this with ldx = Cin, ldo = Cout, no x2.
int specmi_conv2d_strided(specmi_handle* h, const float* x, int B, int H, int W, int Cin, int ldx, const float* w_host,
                          const float* scale_host, const float* shift_host, int Cout, int KH, int KW, int stride, int pad,
                          const float* residual, int relu, float* out, int ldo, const float* x2, int H2, int W2, int Cin2, int ldx2,
                          int stride2, void* stream) {
    ENTER(h);
    if (!x || !w_host || !scale_host || !shift_host || !out || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH != KW || KH < 1 ||
        stride < 1 || pad < 0)
        return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (ldx < Cin || ldo < Cout) return fail(h, SPECMI_ERR_ARG, "ldx (%d) < Cin (%d) or ldo (%d) < Cout (%d)", ldx, Cin, ldo, Cout);
    if (conv_out(H, KH, stride, pad) < 1 || conv_out(W, KW, stride, pad) < 1) return fail(h, SPECMI_ERR_ARG, "empty output");
    if (x2) {
        if (KH != 1 || pad != 0 || stride != 1) return fail(h, SPECMI_ERR_ARG, "a second A source needs a 1x1 / stride 1 / pad 0 layer");
        if (Cin2 <= 0 || ldx2 < Cin2 || stride2 < 1 || (H - 1) * (long)stride2 >= H2 || (W - 1) * (long)stride2 >= W2)
            return fail(h, SPECMI_ERR_ARG, "second A source: Cin2 %d, ldx2 %d, stride2 %d, %dx%d does not cover the %dx%d outputs", Cin2, ldx2,
                        stride2, H2, W2, H, W);
    } else Cin2 = 0;
    hipStream_t s = (hipStream_t)stream;
    std::vector<void*> tmp;
    std::vector<float> packed, sc, sh;
    const bool stem = (Cin == 3 && KH == 7 && Cout == 64 && stride == 2 && pad == 3);
    if (stem && (ldx != Cin || ldo != Cout)) return fail(h, SPECMI_ERR_ARG, "the 7x7 stem reads a dense NCHW image and writes dense rows");
    const int Kc = Cin + Cin2;          // input channels of w: with x2 the 1x1 weights of both sources, concatenated along K
    int rc = SPECMI_OK;
    float *dw = nullptr, *dsc = nullptr, *dsh = nullptr;
    const int Npad = round_up(Cout, 64);
    sc.assign(Npad, 0.f); sh.assign(Npad, 0.f);
    std::memcpy(sc.data(), scale_host, (size_t)Cout * 4);
    std::memcpy(sh.data(), shift_host, (size_t)Cout * 4);
    // option "winograd": 1 (default) = F(2x2,3x3) where the shape allows it, 0 = always the direct implicit GEMM
    const bool wino = !stem && opt(h, OPT_winograd) && KH == 3 && stride == 1 && pad == 1 && Cin % 16 == 0 &&
                      (Cout % 64 == 0 || (Cout % 32 == 0 && Cout > 64));
    // (the Winograd kernel stores 16 bytes per lane: its rows of out / residual are 16-byte aligned in every trunk)
    if (wino && (ldo % 4 || (reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(residual) & 15)))
        return fail(h, SPECMI_ERR_ARG, "Winograd: out / residual rows must be 16-byte aligned (ldo %d)", ldo);
    const int terms = opt(h, OPT_conv_precision);
    const bool split = !stem && (terms == 3 || terms == 6) && Cin % 16 == 0 && Cin2 % 16 == 0 && Cout % 4 == 0;
    std::vector<unsigned short> pieces;
    void* dsplit = nullptr;
    if (split) {
        pack_bf16_split_weights_oihw(w_host, Cout, Kc, KH, KW, Npad, pieces);
        if ((rc = dev_upload(h, pieces.data(), pieces.size() * 2, &dsplit, tmp))) { free_pool(tmp); return rc; }
    }
    if (stem) pack_stem_weights(w_host, packed);
    else if (wino) pack_wino_weights(w_host, Cout, Cin, packed);
    else {
        if (Cin % 32 || Cin2 % 32) { free_pool(tmp); return fail(h, SPECMI_ERR_ARG, "Cin (and Cin2) must be multiples of 32 (got %d, %d)", Cin, Cin2); }
        pack_gemm_weights(w_host, Cout, Kc, KH, KW, Kc * KH * KW, Npad, packed);
    }
    if ((rc = dev_upload(h, packed.data(), packed.size() * 4, (void**)&dw, tmp)) ||
        (rc = dev_upload(h, sc.data(), sc.size() * 4, (void**)&dsc, tmp)) ||
        (rc = dev_upload(h, sh.data(), sh.size() * 4, (void**)&dsh, tmp))) {
        free_pool(tmp);
        return rc;
    }
    const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
    LaunchCtx ctx{s, &h->prof, "conv2d"};
    int lrc;
    if (stem) {
        lrc = launch_stem(x, dw, dsc, dsh, out, B, H, W, OH, OW, relu, ctx);
    } else {
        ConvArgs a;
        a.x = x; a.w = dw; a.scale = dsc; a.shift = dsh; a.res = residual; a.out = out;
        a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.OH = OH; a.OW = OW; a.Cout = Cout; a.Npad = Npad;
        a.ldo = ldo; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.relu = relu;
        if (x2) { a.x2 = x2; a.H2 = H2; a.W2 = W2; a.ldx2 = ldx2; a.Cin2 = Cin2; a.stride2 = stride2; }
        a.force_variant = opt(h, OPT_force_conv_variant);
        a.wino_variant = opt(h, OPT_force_wino_variant);
        // option "conv2d_sk" (tests): > 1 = that many leaves, -1 = the latency plan's own rule, 0 = the throughput kernel;
        // "latency_force_unit": 0 = by batch, 1 / 2 / 3 = a leaf / a group / the whole K per workgroup
        int S = wino ? 0 : opt(h, OPT_conv2d_sk);
        if (split && conv_bf16s_supported(a)) lrc = launch_conv_bf16s(a, dsplit, terms, ctx);
        else if (S != 0) {
            SkPlan pl = sk_plan(h, a, 1);
            if (S > 0) {
                pl.leaves = S; pl.G = 1;
                for (int g = 2; g <= 4; ++g)
                    if (S % g == 0) pl.G = g;
                pl.unit = 1;
            }
            const int fu = opt(h, OPT_latency_force_unit);
            if (fu) pl.unit = fu == 1 ? 1 : (fu == 2 ? pl.G : pl.leaves);
            // "conv2d_wsplit" (tests): 2 / 3 = the wave-split unit of the same tree, one group / all groups per workgroup
            const int ws = opt(h, OPT_conv2d_wsplit);
            SkPlan pw = pl;
            pw.unit = ws == 3 ? pl.leaves : pl.G;
            if (ws >= 2 && conv_wsplit_supported(a, pw)) {
                if ((rc = ensure_sk(h, conv_wsplit_ws_floats(a, pw.leaves / pw.unit, 1), conv_wsplit_tiles(a, 1)))) { free_pool(tmp); return rc; }
                lrc = launch_conv_wsplit(a, pw, h->sk, ctx);
            } else {
                if ((rc = ensure_sk(h, conv_igemm_sk_ws_floats(a, pl.leaves / pl.unit, 1), conv_igemm_sk_tiles(a, 1)))) { free_pool(tmp); return rc; }
                lrc = pl.leaves > 1 ? launch_conv_igemm_sk(a, pl, h->sk, ctx) : launch_conv_igemm(a, ctx);
            }
        } else lrc = wino ? launch_conv_wino(a, ctx) : launch_conv_igemm(a, ctx);
    }
    hipError_t se = hipStreamSynchronize(s);
    free_pool(tmp);
    // what conv_igemm_check / conv_wino_supported (and the launchers' alignment and size rules) refuse: nothing was launched
    if (lrc == (int)hipErrorInvalidValue) return fail(h, SPECMI_ERR_ARG, "conv2d: shape, stride or alignment not supported");
    if (lrc) return fail(h, SPECMI_ERR_HIP, "conv2d launch failed: %s", hipGetErrorString((hipError_t)lrc));
    if (se != hipSuccess) return fail(h, SPECMI_ERR_HIP, "conv2d failed: %s", hipGetErrorString(se));
    return SPECMI_OK;
}

int specmi_set_precision(specmi_handle* h, int precision) {
    if (!h) return SPECMI_ERR_ARG;
    if (precision != SPECMI_PRECISION_FP32 && precision != SPECMI_PRECISION_FP16)
        return fail(h, SPECMI_ERR_ARG, "precision %d: SPECMI_PRECISION_FP32 (0) or SPECMI_PRECISION_FP16 (1)", precision);
    h->precision = precision;
    return SPECMI_OK;
}

int specmi_get_precision(specmi_handle* h, int* precision) {
    if (!h || !precision) return h ? fail(h, SPECMI_ERR_ARG, "precision is NULL") : SPECMI_ERR_ARG;
    *precision = h->precision;
    return SPECMI_OK;
}

int specmi_conv2d_f16(specmi_handle* h, const void* x, int B, int H, int W, int Cin, const float* w_host, const float* scale_host,
                      const float* shift_host, int Cout, int KH, int KW, int stride, int pad, const void* residual, int relu,
                      void* out, int out_f32, const void* x2, int H2, int W2, int Cin2, int stride2, void* stream) {
    ENTER(h);
    if (!x || !w_host || !scale_host || !shift_host || !out || B <= 0 || Cin <= 0 || Cout <= 0 || KH != KW || KH < 1 || stride < 1 ||
        pad < 0 || (x2 && (Cin2 <= 0 || stride2 < 1)))
        return fail(h, SPECMI_ERR_ARG, "bad argument");
    const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
    if (OH < 1 || OW < 1) return fail(h, SPECMI_ERR_ARG, "empty output");
    const int Npad = round_up(Cout, 64), cin_p = round_up(Cin, 8);
    const int Ktot = x2 ? Cin + Cin2 : Cin;        // input channels of w
    std::vector<double> wk;
    fold_f16_oihw(w_host, scale_host, Cout, Ktot, x2 ? Ktot : cin_p, KH, KW, wk);
    const int K = x2 ? Ktot : cin_p * KH * KW, Kp = x2 ? K : round_up(K, 32);
    std::vector<unsigned short> w16;
    const long bad = pack_f16_weights(wk, Cout, K, Kp, Npad, w16);
    if (bad >= 0) return fail(h, SPECMI_ERR_ARG, "folded weight %g (output channel %ld) is outside the finite fp16 range", wk[(size_t)bad], bad / K);
    std::vector<float> sh(Npad, 0.f);
    std::memcpy(sh.data(), shift_host, (size_t)Cout * 4);
    std::vector<void*> tmp;
    void *dw = nullptr, *dsh = nullptr;
    int rc;
    if ((rc = dev_upload(h, w16.data(), w16.size() * 2, &dw, tmp)) || (rc = dev_upload(h, sh.data(), sh.size() * 4, &dsh, tmp))) {
        free_pool(tmp);
        return rc;
    }
    ConvF16Args a;
    a.x = x; a.w = dw; a.shift = static_cast<const float*>(dsh); a.res = residual; a.out = out;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.ldx = x2 ? Cin : cin_p; a.OH = OH; a.OW = OW; a.Cout = Cout; a.Npad = Npad; a.ldo = Cout;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.relu = relu; a.out_f32 = out_f32 ? 1 : 0; a.Kp = Kp;
    a.x2 = x2; a.H2 = H2; a.W2 = W2; a.ldx2 = Cin2; a.Cin2 = Cin2; a.stride2 = stride2;
    hipStream_t s = (hipStream_t)stream;
    LaunchCtx ctx{s, &h->prof, "conv2d_f16"};
    const int lrc = launch_conv_f16(a, ctx);
    hipError_t se = hipStreamSynchronize(s);
    free_pool(tmp);
    if (lrc == (int)hipErrorInvalidValue) return fail(h, SPECMI_ERR_ARG, "conv2d_f16: shape or alignment not supported");
    if (lrc) return fail(h, SPECMI_ERR_HIP, "conv2d_f16 launch failed: %s", hipGetErrorString((hipError_t)lrc));
    if (se != hipSuccess) return fail(h, SPECMI_ERR_HIP, "conv2d_f16 failed: %s", hipGetErrorString(se));
    return SPECMI_OK;
}

int specmi_maxpool3x3s2(specmi_handle* h, const float* x, int B, int H, int W, int C, float* out, void* stream) {
    ENTER(h);
    if (!x || !out || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "maxpool"};
    LAUNCHCHK(h, launch_maxpool3x3s2(x, out, B, H, W, C, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), ctx), "maxpool");
    return SPECMI_OK;
}

int specmi_maxpool3x3s2_f16(specmi_handle* h, const void* x, int B, int H, int W, int C, void* out, void* stream) {
    ENTER(h);
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return fail(h, SPECMI_ERR_ARG, "bad argument (C % 8 == 0)");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "maxpool_f16"};
    LAUNCHCHK(h, launch_maxpool_f16(x, out, B, H, W, C, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), ctx), "maxpool_f16");
    return SPECMI_OK;
}

int specmi_to_nhwc_f16(specmi_handle* h, const float* x, int B, int C, int H, int W, void* out, void* stream) {
    ENTER(h);
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 8) return fail(h, SPECMI_ERR_ARG, "bad argument (1 <= C <= 8)");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "to_nhwc_f16"};
    LAUNCHCHK(h, launch_to_nhwc_f16(x, out, B, C, H, W, ctx), "to_nhwc_f16");
    return SPECMI_OK;
}

int specmi_avgpool(specmi_handle* h, const float* x, int B, int HW, int C, float* out, void* stream) {
    ENTER(h);
    if (!x || !out || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "avgpool"};
    LAUNCHCHK(h, launch_avgpool(x, out, B, HW, C, C, ctx), "avgpool");
    return SPECMI_OK;
}

static bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// One Linear layer (or up to three of one shape in one GEMV launch) on caller-supplied parameters, through the code the heads run:
// upload_fc (what commit_fc uploads) into temporaries, then launch_fc_gemv (path 0) or run_fc (path 1)
int specmi_fc_forward(specmi_handle* h, int nheads, const float* const* w_host, const float* const* bias_host, int N, int K,
                      const float* const* x, int ldx, const float* const* residual, float* const* out, int ldo, int B, int path,
                      void* stream) {
    ENTER(h);
    if (!w_host || !bias_host || !x || !out) return fail(h, SPECMI_ERR_ARG, "fc_forward: NULL pointer");
    if (nheads < 1 || nheads > 3) return fail(h, SPECMI_ERR_ARG, "fc_forward: nheads must be 1..3, got %d", nheads);
    if (N <= 0 || K <= 0 || B <= 0) return fail(h, SPECMI_ERR_ARG, "fc_forward: N, K and B must be positive, got %d, %d, %d", N, K, B);
    if (path != 0 && path != 1) return fail(h, SPECMI_ERR_ARG, "fc_forward: path must be 0 (GEMV) or 1 (matrix cores), got %d", path);
    if (path == 1 && nheads != 1) return fail(h, SPECMI_ERR_ARG, "fc_forward: the matrix-core path takes one head, got %d", nheads);
    const int Kp = round_up(K, 32);
    if (ldx < Kp) return fail(h, SPECMI_ERR_ARG, "fc_forward: ldx (%d) < K rounded up to 32 (%d): the kernels read the padded row", ldx, Kp);
    if (ldx % 4) return fail(h, SPECMI_ERR_ARG, "fc_forward: ldx must be a multiple of 4, got %d", ldx);
    if (ldo < N) return fail(h, SPECMI_ERR_ARG, "fc_forward: ldo (%d) < N (%d)", ldo, N);
    for (int i = 0; i < nheads; ++i) {
        if (!w_host[i] || !bias_host[i] || !x[i] || !out[i]) return fail(h, SPECMI_ERR_ARG, "fc_forward: head %d has a NULL pointer", i);
        if (misaligned16(x[i])) return fail(h, SPECMI_ERR_ARG, "fc_forward: x of head %d is not 16-byte aligned", i);
        if ((reinterpret_cast<uintptr_t>(out[i]) & 3) || (residual && (reinterpret_cast<uintptr_t>(residual[i]) & 3)))
            return fail(h, SPECMI_ERR_ARG, "fc_forward: out / residual of head %d is not 4-byte aligned", i);
    }
    hipStream_t s = (hipStream_t)stream;
    std::vector<void*> tmp;
    FcW fc[3];
    int rc = SPECMI_OK;
    for (int i = 0; i < nheads && !rc; ++i) rc = upload_fc(h, w_host[i], bias_host[i], N, K, fc[i], tmp);
    int lrc = 0;
    if (!rc && path == 0) {
        FcGemv hd[3];
        for (int i = 0; i < nheads; ++i) hd[i] = FcGemv{x[i], fc[i].w_rm, fc[i].shift, residual ? residual[i] : nullptr, out[i]};
        LaunchCtx ctx{s, &h->prof, "fc_forward"};
        lrc = launch_fc_gemv(hd, nheads, N, Kp, ldx, ldo, B, ctx);
    } else if (!rc) {
        rc = run_fc(h, fc[0], x[0], ldx, B, residual ? residual[0] : nullptr, out[0], ldo, s, "fc_forward");
    }
    hipError_t se = hipStreamSynchronize(s);
    free_pool(tmp);
    if (rc) return rc;
    if (lrc == (int)hipErrorInvalidValue) return fail(h, SPECMI_ERR_ARG, "fc_forward: shape, stride or alignment not supported");
    if (lrc) return fail(h, SPECMI_ERR_HIP, "fc_forward launch failed: %s", hipGetErrorString((hipError_t)lrc));
    if (se != hipSuccess) return fail(h, SPECMI_ERR_HIP, "fc_forward failed: %s", hipGetErrorString(se));
    return SPECMI_OK;
}

// ---- HRNet's own kernels on their own (hrnet.hip): the launchers hrnet_forward calls, behind argument checks -------------------

int specmi_hr_stem3x3(specmi_handle* h, const float* images_nchw, int B, int H, int W, const float* w, const float* scale,
                      const float* shift, float* out_nhwc, void* stream) {
    ENTER(h);
    if (!images_nchw || !w || !scale || !shift || !out_nhwc) return fail(h, SPECMI_ERR_ARG, "hr_stem3x3: NULL pointer");
    if (B <= 0 || H <= 0 || W <= 0) return fail(h, SPECMI_ERR_ARG, "hr_stem3x3: B, H and W must be positive, got %d, %d, %d", B, H, W);
    if (misaligned16(out_nhwc)) return fail(h, SPECMI_ERR_ARG, "hr_stem3x3: out is not 16-byte aligned");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "hr_stem3x3"};
    return hr_launch_stem3x3(h, images_nchw, B, H, W, w, scale, shift, out_nhwc, ctx);
}

int specmi_hr_fuse_sum(specmi_handle* h, const float* const terms[4], const int ld[4], const int sh[4], int n, int B, int H, int W,
                       int C, int relu, float* out, int ldo, void* stream) {
    ENTER(h);
    if (!terms || !ld || !sh || !out) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: NULL pointer");
    if (n < 1 || n > 4) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: n must be 1..4, got %d", n);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: B, H, W and C must be positive, got %d, %d, %d, %d", B, H, W, C);
    if (C % 4) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: C must be a multiple of 4, got %d", C);
    if (ldo % 4 || ldo < C) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: ldo must be a multiple of 4 and >= C, got %d (C = %d)", ldo, C);
    if (misaligned16(out)) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: out is not 16-byte aligned");
    for (int k = 0; k < n; ++k) {
        if (!terms[k]) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: term %d is NULL", k);
        if (misaligned16(terms[k])) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: term %d is not 16-byte aligned", k);
        if (ld[k] % 4 || ld[k] < C) return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: ld[%d] must be a multiple of 4 and >= C, got %d (C = %d)", k, ld[k], C);
        if (sh[k] < 0 || sh[k] > 30 || (H >> sh[k]) << sh[k] != H || (W >> sh[k]) << sh[k] != W)
            return fail(h, SPECMI_ERR_ARG, "hr_fuse_sum: %dx%d is not divisible by 2^sh[%d] (sh = %d)", H, W, k, sh[k]);
    }
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "hr_fuse_sum"};
    return hr_launch_fuse_sum(h, terms, ld, sh, n, B, H, W, C, relu ? 1 : 0, out, ldo, ctx);
}

int specmi_hr_resize_ac(specmi_handle* h, const float* x, int B, int H, int W, int C, int ld, float* out, int OH, int OW, int ldo,
                        void* stream) {
    ENTER(h);
    if (!x || !out) return fail(h, SPECMI_ERR_ARG, "hr_resize_ac: NULL pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || OH <= 0 || OW <= 0)
        return fail(h, SPECMI_ERR_ARG, "hr_resize_ac: B, H, W, C, OH and OW must be positive, got %d, %d, %d, %d, %d, %d", B, H, W, C, OH, OW);
    if (C % 4) return fail(h, SPECMI_ERR_ARG, "hr_resize_ac: C must be a multiple of 4, got %d", C);
    if (ld % 4 || ld < C) return fail(h, SPECMI_ERR_ARG, "hr_resize_ac: ld must be a multiple of 4 and >= C, got %d (C = %d)", ld, C);
    if (ldo % 4 || ldo < C) return fail(h, SPECMI_ERR_ARG, "hr_resize_ac: ldo must be a multiple of 4 and >= C, got %d (C = %d)", ldo, C);
    if (misaligned16(x) || misaligned16(out)) return fail(h, SPECMI_ERR_ARG, "hr_resize_ac: x or out is not 16-byte aligned");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "hr_resize_ac"};
    return hr_launch_resize_ac(h, x, B, H, W, C, ld, out, OH, OW, ldo, ctx);
}

// every *_f16 producer: the output is NHWC8 fp16 (include/specmi.h), one 16-byte vector per pixel
#define NEED_ALIGNED16(h, p) \
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(h, SPECMI_ERR_ARG, "the NHWC8 fp16 output is not 16-byte aligned");

static int resize_normalize(specmi_handle* h, const uint8_t* frame, int H, int W, int OH, int OW, void* out, bool f16, uint8_t* raw,
                            void* stream) {
    ENTER(h);
    if (!frame || !out || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (f16) NEED_ALIGNED16(h, out);
    hipStream_t s = (hipStream_t)stream;
    // tables: [hb (2 OW) | hk (OW ksh) | vb (2 OH) | vk (OH ksv)], rebuilt only when the geometry changes
    std::vector<int> hb, hk, vb, vk;
    const int ksh = pillow_coeffs(W, OW, hb, hk), ksv = pillow_coeffs(H, OH, vb, vk);
    const size_t o_hk = hb.size(), o_vb = o_hk + hk.size(), o_vk = o_vb + vb.size(), total = o_vk + vk.size();
    if (h->resize_geom[0] != H || h->resize_geom[1] != W || h->resize_geom[2] != OH || h->resize_geom[3] != OW || !h->resize_tab) {
        // a resize enqueued earlier on ANY stream may still read the old tables (the handle is shared by callers on
        // different streams): wait for the whole device before freeing / overwriting them
        HIPCHK(h, hipDeviceSynchronize());
        if (total > h->resize_tab_ints) {
            if (h->resize_tab) (void)hipFree(h->resize_tab);
            h->resize_tab = nullptr;
            HIPCHK(h, hipMalloc((void**)&h->resize_tab, total * 4));
            h->resize_tab_ints = total;
        }
        h->resize_host.resize(total);
        std::memcpy(h->resize_host.data(), hb.data(), hb.size() * 4);
        std::memcpy(h->resize_host.data() + o_hk, hk.data(), hk.size() * 4);
        std::memcpy(h->resize_host.data() + o_vb, vb.data(), vb.size() * 4);
        std::memcpy(h->resize_host.data() + o_vk, vk.data(), vk.size() * 4);
        HIPCHK(h, hipMemcpyAsync(h->resize_tab, h->resize_host.data(), total * 4, hipMemcpyHostToDevice, s));
        h->resize_geom[0] = H; h->resize_geom[1] = W; h->resize_geom[2] = OH; h->resize_geom[3] = OW;
    }
    LaunchCtx ctx{s, &h->prof, "resize_normalize"};
    LAUNCHCHK(h, launch_resize_normalize(frame, H, W, OH, OW, h->resize_tab, h->resize_tab + o_hk, ksh, h->resize_tab + o_vb,
                                         h->resize_tab + o_vk, ksv, out, raw, ctx, f16), "resize_normalize");
    return SPECMI_OK;
}

int specmi_resize_normalize(specmi_handle* h, const uint8_t* frame, int H, int W, int OH, int OW, float* out, uint8_t* raw,
                            void* stream) {
    return resize_normalize(h, frame, H, W, OH, OW, out, false, raw, stream);
}

int specmi_resize_normalize_f16(specmi_handle* h, const uint8_t* frame, int H, int W, int OH, int OW, void* out_nhwc8, uint8_t* raw,
                                void* stream) {
    return resize_normalize(h, frame, H, W, OH, OW, out_nhwc8, true, raw, stream);
}

// a device buffer of a ragged entry point that must hold `need` bytes: kept, or replaced by one at least 1.5x the old size while the
// outgrown one joins ws_retired (the rule of ensure_ws: work enqueued earlier may still name it).  A failed allocation leaves it empty.
static int grow_ragged(specmi_handle* h, DevBuf& b, size_t need, const char* what) {
    if (need <= b.bytes) return SPECMI_OK;
    if (int rc0 = sync_for_growth(h, what)) return rc0;
    if (b.bytes && need < b.bytes + b.bytes / 2) need = b.bytes + b.bytes / 2;
    if (b.p) h->ws_retired.push_back(b.p);
    b = DevBuf{};
    HIPCHK(h, hipMalloc(&b.p, need));
    b.bytes = need;
    return SPECMI_OK;
}

// is a capture under way on the stream?  (a failed query counts as no, and leaves no sticky error behind)
static bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

// The rewrite rule of every DevTable (handle.h), for the records a call has just built - handed over: a rewrite swaps them with the
// host image instead of copying them (the tile list of specmi_draw_marks is large); `ws` with `ws_need`: the workspace the same
// call needs, which grows first.  `what` / `ws_what` name the two in messages.
//   ask_first = the nouns of the refusal ("new frame records or bones"): growing either buffer or rewriting the table synchronises
// the whole device, which would invalidate a capture under way on the stream.  Such a table asks the stream first and refuses with
// SPECMI_ERR_STATE before anything is enqueued or synchronised, so the capture stays valid.
//   ask_first = nullptr: the three older tables (ragged, pano, crop) do not ask: under capture they reach sync_for_growth and
// report that the capture is invalid now.  Making them ask first is a change of behaviour that belongs to another pull request.
// On return the records are in t.dev.p (read it after the call, not before: growing replaces it).
static int publish_table(specmi_handle* h, DevTable& t, std::vector<int>& rec, const char* what, const char* ask_first, hipStream_t s,
                         DevBuf* ws = nullptr, size_t ws_need = 0, const char* ws_what = nullptr) {
    const size_t len = rec.size() * sizeof(int);
    const bool regrown = len > t.dev.bytes;
    const bool rewrite = regrown || rec != t.host;
    if (ask_first && (rewrite || (ws && ws_need > ws->bytes)) && stream_is_capturing(s))
        return fail(h, SPECMI_ERR_STATE, "%s are not possible while the stream is being captured: run one eager call with these records "
                    "first (nothing was enqueued)", ask_first);
    int rc;
    if (ws && (rc = grow_ragged(h, *ws, ws_need, ws_what))) return rc;
    if ((rc = grow_ragged(h, t.dev, len, what))) return rc;
    if (!rewrite) return SPECMI_OK;
    // a call enqueued earlier on ANY stream may still read the old records (specmi_resize_normalize has the same rule); growing
    // the table has just waited for the whole device
    if (!regrown && (rc = sync_for_growth(h, what))) return rc;
    t.host.swap(rec);
    HIPCHK(h, hipMemcpyAsync(t.dev.p, t.host.data(), len, hipMemcpyHostToDevice, s));
    return SPECMI_OK;
}

// ---- byte rectangles: what the ragged entry points check about the places their records name in a slab ------------------------------
// a rectangle = H rows of `row` (3 W) bytes, `pitch` bytes apart, from byte `off` of its slab
struct ByteRect { long long off, pitch, row; int H; long long end() const { return off + (H - 1) * pitch + row; } };

// does the rectangle of H rows of 3 W bytes lie inside a slab of slab_bytes?  In double: no offset or pitch overflows it
static bool rect_in_slab(long long off, long long pitch, int H, int W, size_t slab_bytes) {
    return off >= 0 && (double)off + (double)(H - 1) * (double)pitch + 3.0 * W <= (double)slab_bytes;
}

// a single row has no next row: its pitch is not read, and is stored as 3 W so that equal rectangles give equal records
static long long stored_pitch(long long pitch, int H, int W) { return H > 1 ? pitch : 3LL * W; }

// do two buffers share a byte?
static bool slabs_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (const uint8_t*)b < (const uint8_t*)a + a_bytes && (const uint8_t*)a < (const uint8_t*)b + b_bytes;
}

static bool rects_overlap(ByteRect a, ByteRect b) {
    if (a.off > b.off) std::swap(a, b);
    if (b.off >= a.end()) return false;
    if (a.pitch == b.pitch) {       // the columns of one picture: b starts c bytes into row q of a
        const long long q = (b.off - a.off) / a.pitch, c = (b.off - a.off) % a.pitch;
        return (q < a.H && c < a.row) || (q + 1 < a.H && c + b.row > a.pitch);
    }
    for (int r = 0; r < b.H; ++r) {      // row r of b against the rows of a it reaches
        const long long s0 = b.off + r * b.pitch - a.off, e0 = s0 + b.row - 1;     // first and last byte, counted from a's first
        if (s0 >= a.end() - a.off) break;
        const long long k1 = s0 / a.pitch, k2 = std::min<long long>(e0 / a.pitch, a.H - 1);
        if (k2 - k1 >= 2) return true;                                              // a whole row of a lies inside
        for (long long k = k1; k <= k2; ++k)
            if (std::max(s0, k * a.pitch) <= std::min(e0, k * a.pitch + a.row - 1)) return true;
    }
    return false;
}

// the first two rectangles that share a byte -> true and their indices: sorted by first byte, a rectangle is compared with those
// that start before it ends
static bool first_overlap(const std::vector<ByteRect>& rects, int* a, int* b) {
    const int n = (int)rects.size();
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return rects[x].off < rects[y].off; });
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n && rects[order[j]].off < rects[order[i]].end(); ++j)
            if (rects_overlap(rects[order[i]], rects[order[j]])) { *a = order[i]; *b = order[j]; return true; }
    return false;
}

// the same for gapless ranges (first byte, bytes), which it sorts -> true and the first byte of the later of two that meet
static bool first_shared_byte(std::vector<std::pair<long long, long long>>& ranges, long long* at) {
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 0; i + 1 < ranges.size(); ++i)
        if (ranges[i].first + ranges[i].second > ranges[i + 1].first) { *at = ranges[i + 1].first; return true; }
    return false;
}
// ---- end of byte rectangles -------------------------------------------------------------------------------------------------------

// the two refusals of record i's pitched rectangle in its slab; `noun` = what the call's records are ("frame", "picture", "file")
static int check_rect(specmi_handle* h, const char* noun, int i, long long off, long long pitch, int H, int W, size_t slab_bytes) {
    if (pitch < 3LL * W) return fail(h, SPECMI_ERR_ARG, "%s %d: a pitch of %lld bytes for rows of %d", noun, i, pitch, 3 * W);
    if (!rect_in_slab(off, pitch, H, W, slab_bytes))
        return fail(h, SPECMI_ERR_ARG, "%s %d: its rectangle leaves the slab of %zu bytes", noun, i, slab_bytes);
    return SPECMI_OK;
}

static int resize_normalize_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets,
                                   const int32_t* geom, int n, int Hmax, int Wmax, void* out, bool f16, void* stream) {
    ENTER(h);
    if (!frames || !offsets || !geom || !out || n <= 0 || Hmax <= 0 || Wmax <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (f16) NEED_ALIGNED16(h, out);
    if (n > 65535) return fail(h, SPECMI_ERR_ARG, "at most 65535 frames per call (grid dimension), got %d", n);
    if (slab_bytes >= 4294967296.0 || (double)Hmax * Wmax >= 2147483648.0)
        return fail(h, SPECMI_ERR_ARG, "a frame slab of %zu bytes / a %d x %d output plane is beyond the kernels' 32-bit offsets", slab_bytes, Hmax, Wmax);
    hipStream_t s = (hipStream_t)stream;
    // [n records | per resampled frame: hb (2 OW) | hk (OW ksh) | vb (2 OH) | vk (OH ksv)]
    std::vector<int> tab((size_t)n * kRaggedRec, 0), hb, hk, vb, vk;
    size_t tmp_bytes = 0;
    int max_hpass = 0;
    for (int f = 0; f < n; ++f) {
        const int H = geom[4 * f], W = geom[4 * f + 1], OH = geom[4 * f + 2], OW = geom[4 * f + 3];
        if (H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || OH > Hmax || OW > Wmax)
            return fail(h, SPECMI_ERR_ARG, "frame %d: size %d x %d -> %d x %d does not fit the %d x %d batch", f, H, W, OH, OW, Hmax, Wmax);
        if (!rect_in_slab(offsets[f], 3LL * W, H, W, slab_bytes))
            return fail(h, SPECMI_ERR_ARG, "frame %d: %d x %d x 3 bytes at offset %lld leave the slab of %zu bytes", f, H, W, (long long)offsets[f], slab_bytes);
        RaggedFrame fr{};
        fr.src_off = (unsigned)offsets[f]; fr.H = H; fr.W = W; fr.OH = OH; fr.OW = OW;
        fr.resample = (OH != H || OW != W) ? 1 : 0;
        if (fr.resample) {
            if ((double)H * OW >= 2147483648.0 / 3 || (double)tmp_bytes + (double)H * OW * 3 >= 4294967296.0)
                return fail(h, SPECMI_ERR_ARG, "frame %d: the uint8 rows between the passes are beyond 32-bit offsets", f);
            fr.ksh = pillow_coeffs(W, OW, hb, hk);
            fr.ksv = pillow_coeffs(H, OH, vb, vk);
            if ((double)tab.size() + hb.size() + hk.size() + vb.size() + vk.size() >= 2147483648.0)
                return fail(h, SPECMI_ERR_ARG, "the coefficient tables are beyond 31-bit offsets");
            fr.hb = (int)tab.size(); tab.insert(tab.end(), hb.begin(), hb.end());
            fr.hk = (int)tab.size(); tab.insert(tab.end(), hk.begin(), hk.end());
            fr.vb = (int)tab.size(); tab.insert(tab.end(), vb.begin(), vb.end());
            fr.vk = (int)tab.size(); tab.insert(tab.end(), vk.begin(), vk.end());
            fr.tmp_off = (unsigned)tmp_bytes;
            tmp_bytes += (size_t)H * OW * 3;
            if (H * OW > max_hpass) max_hpass = H * OW;
        }
        std::memcpy(tab.data() + (size_t)f * kRaggedRec, &fr, sizeof(fr));
    }
    DevBuf& tmp = h->buf[BUF_ragged_tmp];
    DevTable& T = h->tab[TAB_ragged];
    if (int rc = publish_table(h, T, tab, "the ragged-resize tables", nullptr, s, &tmp, tmp_bytes, "the ragged-resize row workspace")) return rc;
    LaunchCtx ctx{s, &h->prof, "preprocess.resize_ragged"};
    LAUNCHCHK(h, launch_resize_normalize_ragged(frames, (const int*)T.dev.p, (unsigned char*)tmp.p, n, max_hpass, Hmax, Wmax, (double)slab_bytes,
                                                (double)tmp_bytes, out, ctx, f16),
              "resize_normalize_ragged");
    return SPECMI_OK;
}

int specmi_resize_normalize_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets,
                                   const int32_t* geom, int n, int Hmax, int Wmax, float* out, void* stream) {
    return resize_normalize_ragged(h, frames, slab_bytes, offsets, geom, n, Hmax, Wmax, out, false, stream);
}

int specmi_resize_normalize_ragged_f16(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets,
                                       const int32_t* geom, int n, int Hmax, int Wmax, void* out_nhwc8, void* stream) {
    return resize_normalize_ragged(h, frames, slab_bytes, offsets, geom, n, Hmax, Wmax, out_nhwc8, true, stream);
}

int specmi_pano_extract_views(specmi_handle* h, const uint8_t* pano, int PH, int PW, const double* views, const int32_t* out_hw,
                              const int64_t* offsets, size_t slab_bytes, uint8_t* out_slab, int n, void* stream) {
    ENTER(h);
    if (!pano || !views || !out_hw || !offsets || !out_slab) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (n <= 0) return fail(h, SPECMI_ERR_ARG, "at least one view per call, got %d", n);
    if (n > 65535) return fail(h, SPECMI_ERR_ARG, "at most 65535 views per call (grid dimension), got %d", n);
    if (PH < 1 || PW < 1) return fail(h, SPECMI_ERR_ARG, "a %d x %d panorama", PH, PW);
    hipStream_t s = (hipStream_t)stream;
    static_assert(sizeof(PanoView) % sizeof(int) == 0, "the view records are kept as ints");
    constexpr size_t kRec = sizeof(PanoView) / sizeof(int);
    std::vector<int> tab((size_t)n * kRec, 0);
    int max_tiles = 0;
    double out_bytes = 0.0;
    for (int f = 0; f < n; ++f) {
        const double* v = views + 5 * (size_t)f;
        const int H = out_hw[2 * f], W = out_hw[2 * f + 1];
        for (int k = 0; k < 5; ++k)
            if (!std::isfinite(v[k])) return fail(h, SPECMI_ERR_ARG, "view %d: parameter %d is not finite", f, k);
        if (!(v[3] > 0.0 && v[3] < 180.0) || !(v[4] > 0.0))
            return fail(h, SPECMI_ERR_ARG, "view %d: vfov %g degrees (0 < vfov < 180) / ratio %g (> 0)", f, v[3], v[4]);
        if (H < 1 || W < 1) return fail(h, SPECMI_ERR_ARG, "view %d: size %d x %d", f, H, W);
        if ((double)H * W >= 2147483648.0 / 3) return fail(h, SPECMI_ERR_ARG, "view %d: %d x %d pixels are beyond 31-bit offsets", f, H, W);
        if (!rect_in_slab(offsets[f], 3LL * W, H, W, slab_bytes))
            return fail(h, SPECMI_ERR_ARG, "view %d: %d x %d x 3 bytes at offset %lld leave the slab of %zu bytes", f, H, W, (long long)offsets[f], slab_bytes);
        PanoView r{};
        if (!make_pano_view(v, H, W, (long long)offsets[f], r))
            return fail(h, SPECMI_ERR_ARG, "view %d: a height of %d at ratio %g gives a width of round(h * ratio), not %d", f, H, v[4], W);
        std::memcpy(tab.data() + (size_t)f * kRec, &r, sizeof(r));
        max_tiles = std::max(max_tiles, pano_view_tiles(H, W));
        out_bytes += (double)H * W * 3;
    }
    DevTable& T = h->tab[TAB_pano];
    if (int rc = publish_table(h, T, tab, "the panorama view table", nullptr, s)) return rc;
    LaunchCtx ctx{s, &h->prof, "preprocess.pano_views"};
    LAUNCHCHK(h, launch_pano_extract(pano, PH, PW, (const PanoView*)T.dev.p, n, max_tiles, out_bytes, out_slab, ctx), "pano_extract_views");
    return SPECMI_OK;
}

int specmi_render_meshes(specmi_handle* h, const float* vertices, int M, int V, const int32_t* faces, int F, const float* cam_t,
                         const float* R, float fx, float fy, float cx, float cy, const uint8_t* frame, int H, int W, const float* rgb,
                         int flags, uint8_t* out, int32_t* id_map, float* depth, void* screen, void* stream) {
    ENTER(h);
    const bool side = flags & SPECMI_RENDER_SIDE_VIEW, ground = flags & SPECMI_RENDER_GROUND_PLANE;
    if (!vertices || !faces || !cam_t || !R || !rgb || !out) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (flags & ~(SPECMI_RENDER_SIDE_VIEW | SPECMI_RENDER_GROUND_PLANE | SPECMI_RENDER_CULL | SPECMI_RENDER_THREAD_PER_TRIANGLE))
        return fail(h, SPECMI_ERR_ARG, "unknown render flag in 0x%x", flags);
    if (!side && !frame) return fail(h, SPECMI_ERR_ARG, "an overlay needs the frame it is drawn over (null pointer)");
    if (ground && !side) return fail(h, SPECMI_ERR_ARG, "the ground plane belongs to the side view");
    if (M < 1 || V < 1 || F < 1) return fail(h, SPECMI_ERR_ARG, "%d meshes of %d vertices and %d faces", M, V, F);
    if ((double)M * F >= 2147483648.0 || (double)M * V * 3 >= 2147483648.0)
        return fail(h, SPECMI_ERR_ARG, "%d meshes of %d vertices and %d faces are beyond 31-bit ids", M, V, F);
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return fail(h, SPECMI_ERR_ARG, "a %d x %d frame (1 .. 32768 per side)", H, W);
    if (!(fx > 0.f) || !(fy > 0.f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail(h, SPECMI_ERR_ARG, "focal length (%g, %g) (> 0, finite) / centre (%g, %g) (finite)", (double)fx, (double)fy, (double)cx, (double)cy);
    RenderArgs a{};
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(rgb[k])) return fail(h, SPECMI_ERR_ARG, "base colour component %d is not finite", k);
        a.rgb[k] = std::fmin(std::fmax(rgb[k], 0.f), 1.f);
    }
    size_t off[4];
    const size_t need = render_ws_layout(M, V, H, W, off);
    if (int rc = grow_ragged(h, h->buf[BUF_render], need, "the render workspace")) return rc;
    char* ws = (char*)h->buf[BUF_render].p;
    a.vertices = vertices; a.faces = faces; a.cam_t = cam_t; a.R = R; a.frame = frame;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.M = M; a.V = V; a.F = F; a.H = H; a.W = W; a.side = side; a.ground = ground; a.cull = (flags & SPECMI_RENDER_CULL) ? 1 : 0;
    a.keys = (unsigned long long*)(ws + off[0]); a.sws = (int*)(ws + off[1]); a.normals = (int*)(ws + off[2]); a.lowest = (int*)(ws + off[3]);
    a.in_pitch = a.out_pitch = 3u * (unsigned)W;
    a.out = out; a.id_map = id_map; a.depth = depth; a.screen = (int*)screen;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, side ? "render.side_view" : "render.overlay"};
    LAUNCHCHK(h, launch_render(a, (flags & SPECMI_RENDER_THREAD_PER_TRIANGLE) != 0, ctx), "render_meshes");
    return SPECMI_OK;
}

int specmi_render_views(specmi_handle* h, const float* vertices, int Mtot, int V, const int32_t* faces, int F, const float* cam_t,
                        const float* rgb, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                        const int32_t* view_geom, const int64_t* view_offsets, const float* view_cams, int nviews, int32_t* id_map,
                        float* depth, void* screen, void* stream) {
    ENTER(h);
    if (!vertices || !faces || !cam_t || !rgb || !out_slab || !view_geom || !view_offsets || !view_cams)
        return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (nviews <= 0 || nviews > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 views per call, got %d", nviews);
    if (Mtot < 0 || V < 1 || F < 1) return fail(h, SPECMI_ERR_ARG, "%d meshes of %d vertices and %d faces", Mtot, V, F);
    if (in_slab_bytes >= 4294967296.0 || out_slab_bytes >= 4294967296.0)
        return fail(h, SPECMI_ERR_ARG, "slabs of %zu / %zu bytes are beyond the kernels' 32-bit offsets", in_slab_bytes, out_slab_bytes);
    if (in_slab && slabs_overlap(in_slab, in_slab_bytes, out_slab, out_slab_bytes))
        return fail(h, SPECMI_ERR_ARG, "the frame slab and the output slab overlap");
    RenderViewsArgs b{};
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(rgb[k])) return fail(h, SPECMI_ERR_ARG, "base colour component %d is not finite", k);
        b.rgb[k] = std::fmin(std::fmax(rgb[k], 0.f), 1.f);
    }
    const int known = SPECMI_RENDER_SIDE_VIEW | SPECMI_RENDER_GROUND_PLANE | SPECMI_RENDER_CULL | SPECMI_RENDER_THREAD_PER_TRIANGLE;
    // [nviews records | px_prefix (nviews + 1) | pair_view (npairs)]
    std::vector<int> tab((size_t)nviews * kRenderViewRec + nviews + 1, 0);
    std::vector<ByteRect> rects((size_t)nviews);
    long long px = 0, keys = 0, pairs = 0;
    bool any_ground = false;
    const bool thread_per_triangle = (view_geom[4] & SPECMI_RENDER_THREAD_PER_TRIANGLE) != 0;
    for (int v = 0; v < nviews; ++v) {
        const int H = view_geom[5 * v], W = view_geom[5 * v + 1], mesh0 = view_geom[5 * v + 2], count = view_geom[5 * v + 3], flags = view_geom[5 * v + 4];
        const int64_t in_off = view_offsets[4 * v], in_pitch = view_offsets[4 * v + 1], out_off = view_offsets[4 * v + 2], out_pitch = view_offsets[4 * v + 3];
        const float* cam = view_cams + 13 * (size_t)v;
        const bool side = flags & SPECMI_RENDER_SIDE_VIEW, ground = flags & SPECMI_RENDER_GROUND_PLANE;
        if (flags & ~known) return fail(h, SPECMI_ERR_ARG, "view %d: unknown render flag in 0x%x", v, flags);
        if (ground && !side) return fail(h, SPECMI_ERR_ARG, "view %d: the ground plane belongs to the side view", v);
        if (((flags & SPECMI_RENDER_THREAD_PER_TRIANGLE) != 0) != thread_per_triangle)
            return fail(h, SPECMI_ERR_ARG, "view %d: THREAD_PER_TRIANGLE names the call's one raster launch: set it on every view or on none", v);
        if (H < 1 || W < 1 || H > 32768 || W > 32768) return fail(h, SPECMI_ERR_ARG, "view %d: a %d x %d frame (1 .. 32768 per side)", v, H, W);
        if (count < 0 || mesh0 < 0 || (long long)mesh0 + count > Mtot)
            return fail(h, SPECMI_ERR_ARG, "view %d: meshes %d .. %lld leave the call's %d", v, mesh0, (long long)mesh0 + count, Mtot);
        if ((double)count * F >= 2147483648.0 || (double)count * V * 3 >= 2147483648.0)
            return fail(h, SPECMI_ERR_ARG, "view %d: %d meshes of %d vertices and %d faces are beyond 31-bit ids", v, count, V, F);
        if (ground && count == 0) return fail(h, SPECMI_ERR_ARG, "view %d: a ground plane needs a mesh to lie under", v);
        if (in_off < 0 && !side) return fail(h, SPECMI_ERR_ARG, "view %d: an overlay needs the frame it is drawn over (in_offset %lld)", v, (long long)in_off);
        if (in_off >= 0 && !in_slab) return fail(h, SPECMI_ERR_ARG, "view %d: names a frame, but the frame slab is a null pointer", v);
        if (out_pitch < 3LL * W || (in_off >= 0 && in_pitch < 3LL * W))
            return fail(h, SPECMI_ERR_ARG, "view %d: pitches of %lld / %lld bytes for rows of %d", v, (long long)in_pitch, (long long)out_pitch, 3 * W);
        if (!rect_in_slab(out_off, out_pitch, H, W, out_slab_bytes))
            return fail(h, SPECMI_ERR_ARG, "view %d: its output rectangle leaves the slab of %zu bytes", v, out_slab_bytes);
        if (in_off >= 0 && !rect_in_slab(in_off, in_pitch, H, W, in_slab_bytes))
            return fail(h, SPECMI_ERR_ARG, "view %d: its frame leaves the slab of %zu bytes", v, in_slab_bytes);
        if (!(cam[9] > 0.f) || !(cam[10] > 0.f) || !std::isfinite(cam[9]) || !std::isfinite(cam[10]) || !std::isfinite(cam[11]) || !std::isfinite(cam[12]))
            return fail(h, SPECMI_ERR_ARG, "view %d: focal length (%g, %g) (> 0, finite) / centre (%g, %g) (finite)", v, (double)cam[9], (double)cam[10],
                        (double)cam[11], (double)cam[12]);
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(cam[k])) return fail(h, SPECMI_ERR_ARG, "view %d: R entry %d is not finite", v, k);
        RenderView r{};
        std::memcpy(r.R, cam, 13 * sizeof(float));
        r.H = H; r.W = W; r.mesh0 = mesh0; r.count = count; r.side = side; r.ground = ground; r.cull = (flags & SPECMI_RENDER_CULL) ? 1 : 0;
        r.pair0 = (int)pairs; r.px0 = (int)px; r.key0 = count ? (int)keys : -1;
        r.in_off = in_off >= 0 ? (unsigned)in_off : 0u; r.in_pitch = in_off >= 0 ? (unsigned)stored_pitch(in_pitch, H, W) : 3u * W;
        r.out_off = (unsigned)out_off; r.out_pitch = (unsigned)stored_pitch(out_pitch, H, W);
        std::memcpy(tab.data() + (size_t)v * kRenderViewRec, &r, sizeof(r));
        tab[(size_t)nviews * kRenderViewRec + v] = (int)px;
        rects[v] = ByteRect{out_off, (long long)r.out_pitch, 3LL * W, H};
        px += (long long)H * W;
        if (count) keys += (long long)H * W;
        pairs += count;
        any_ground |= ground;
        if (px >= 2147483648LL) return fail(h, SPECMI_ERR_ARG, "the views hold 2^31 pixels or more");
        if ((double)pairs * F >= 2147483648.0 || (double)pairs * V * 3 >= 2147483648.0)
            return fail(h, SPECMI_ERR_ARG, "the views name %lld meshes of %d vertices and %d faces in all: beyond 31-bit indices", pairs, V, F);
        tab.insert(tab.end(), (size_t)count, v);
    }
    tab[(size_t)nviews * kRenderViewRec + nviews] = (int)px;
    int ra, rb;
    if (first_overlap(rects, &ra, &rb)) return fail(h, SPECMI_ERR_ARG, "the output rectangles of views %d and %d overlap", ra, rb);
    hipStream_t s = (hipStream_t)stream;
    size_t off[4];
    const size_t need = render_views_ws_layout(keys, pairs, V, nviews, off);
    DevTable& T = h->tab[TAB_views];
    if (int rc = publish_table(h, T, tab, "the render view table", "new view records or a larger render workspace", s, &h->buf[BUF_render], need,
                               "the render workspace"))
        return rc;
    char* ws = (char*)h->buf[BUF_render].p;
    const int* dtab = (const int*)T.dev.p;
    b.vertices = vertices; b.faces = faces; b.cam_t = cam_t;
    b.views = (const RenderView*)dtab;
    b.px_prefix = dtab + (size_t)nviews * kRenderViewRec;
    b.pair_view = b.px_prefix + nviews + 1;
    b.in_slab = in_slab; b.out_slab = out_slab;
    b.V = V; b.F = F; b.nviews = nviews; b.npairs = (int)pairs; b.total_px = (int)px;
    b.keys = (unsigned long long*)(ws + off[0]); b.sws = (int*)(ws + off[1]); b.normals = (int*)(ws + off[2]); b.lowest = (int*)(ws + off[3]);
    b.id_map = id_map; b.depth = depth; b.screen = (int*)screen;
    LaunchCtx ctx{s, &h->prof, "render.views"};
    LAUNCHCHK(h, launch_render_views(b, keys, any_ground, thread_per_triangle, ctx), "render_views");
    return SPECMI_OK;
}

int specmi_draw_skeletons(specmi_handle* h, const float* kp, int Mtot, int J, int D, const int32_t* bones, int NB,
                          const specmi_draw_style* style, uint8_t* slab, size_t slab_bytes, const int32_t* frame_geom,
                          const int64_t* frame_offsets, int nframes, void* stream) {
    ENTER(h);
    if (!kp || !slab || !frame_geom || !frame_offsets) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (nframes <= 0 || nframes > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 frames per call, got %d", nframes);
    if (J < 1 || (D != 2 && D != 3) || Mtot < 0) return fail(h, SPECMI_ERR_ARG, "%d detections of %d keypoints of %d floats (J >= 1, D = 2 or 3)", Mtot, J, D);
    if (NB < 0 || (NB > 0 && !bones)) return fail(h, SPECMI_ERR_ARG, "%d bones%s", NB, NB > 0 ? ", but the bone table is a null pointer" : "");
    if ((double)Mtot * ((double)J + NB) >= 2147483648.0 || (double)Mtot * J * D >= 2147483648.0 || (double)J + NB >= 2147483648.0)
        return fail(h, SPECMI_ERR_ARG, "%d detections of %d keypoints and %d bones are beyond 31-bit indices", Mtot, J, NB);
    for (int b = 0; b < 2 * NB; ++b)
        if (bones[b] < 0 || bones[b] >= J) return fail(h, SPECMI_ERR_ARG, "bone %d names joint %d of %d", b / 2, bones[b], J);
    const specmi_draw_style def{4, 2, 0.3f, {0, 255, 0}, {{0, 0, 255}, {255, 0, 0}}};
    const specmi_draw_style& st = style ? *style : def;
    if (st.radius < 0 || st.radius > kDrawMaxRadius || st.thickness < 1 || st.thickness > kDrawMaxThickness)
        return fail(h, SPECMI_ERR_ARG, "radius %d (0 .. %d) / thickness %d (1 .. %d)", st.radius, kDrawMaxRadius, st.thickness, kDrawMaxThickness);
    if (!std::isfinite(st.conf_thr)) return fail(h, SPECMI_ERR_ARG, "the confidence threshold is not finite");
    // [nframes records | bones (NB x 2)]
    std::vector<int> tab((size_t)nframes * kDrawFrameRec, 0);
    std::vector<ByteRect> rects((size_t)nframes);
    long long tiles = 0;
    double kp_bytes = 0.0, px = 0.0;
    for (int f = 0; f < nframes; ++f) {
        const int H = frame_geom[4 * f], W = frame_geom[4 * f + 1], det0 = frame_geom[4 * f + 2], count = frame_geom[4 * f + 3];
        const int64_t off = frame_offsets[2 * f], pitch = frame_offsets[2 * f + 1];
        if (H < 1 || W < 1 || H > kDrawMaxSide || W > kDrawMaxSide)
            return fail(h, SPECMI_ERR_ARG, "frame %d: %d x %d pixels (1 .. %d per side: the exact 64-bit coverage test)", f, H, W, kDrawMaxSide);
        if (count < 0 || det0 < 0 || (long long)det0 + count > Mtot)
            return fail(h, SPECMI_ERR_ARG, "frame %d: detections %d .. %lld leave the call's %d", f, det0, (long long)det0 + count, Mtot);
        if (int rc = check_rect(h, "frame", f, off, pitch, H, W, slab_bytes)) return rc;
        DrawFrame r{};
        r.off = off; r.pitch = stored_pitch(pitch, H, W); r.H = H; r.W = W; r.det0 = det0; r.count = count; r.tile0 = (int)tiles;
        const int n = draw_frame_tiles(H, W, &r.tiles_x);
        if (count) {
            tiles += n;
            kp_bytes += (double)n * count * ((double)J + 2.0 * NB) * D * 4;
            px += (double)H * W;
        }
        if (tiles >= 2147483648LL) return fail(h, SPECMI_ERR_ARG, "the frames hold 2^31 tiles of 32 x 32 pixels or more");
        std::memcpy(tab.data() + (size_t)f * kDrawFrameRec, &r, sizeof(r));
        rects[f] = ByteRect{off, r.pitch, 3LL * W, H};
    }
    int ra, rb;
    if (first_overlap(rects, &ra, &rb)) return fail(h, SPECMI_ERR_ARG, "frames %d and %d share a byte", ra, rb);
    tab.insert(tab.end(), bones, bones + 2 * (size_t)NB);
    hipStream_t s = (hipStream_t)stream;
    DevTable& T = h->tab[TAB_draw];
    if (int rc = publish_table(h, T, tab, "the skeleton frame table", "new frame records or bones", s)) return rc;
    const int* dtab = (const int*)T.dev.p;
    DrawArgs a{};
    a.kp = kp; a.frames = (const DrawFrame*)dtab; a.bones = dtab + (size_t)nframes * kDrawFrameRec; a.slab = slab;
    a.nframes = nframes; a.J = J; a.D = D; a.NB = NB; a.radius = st.radius; a.thickness = st.thickness; a.thr = st.conf_thr;
    const auto pack = [](const uint8_t* c) { return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16; };
    a.rgb[0] = pack(st.joint_rgb); a.rgb[1] = pack(st.bone_rgb[0]); a.rgb[2] = pack(st.bone_rgb[1]);
    LaunchCtx ctx{s, &h->prof, "render.skeletons"};
    LAUNCHCHK(h, launch_draw_skeletons(a, (int)tiles, kp_bytes, px, ctx), "draw_skeletons");
    return SPECMI_OK;
}

// Pillow's ROUND_UP / ROUND_DOWN in double (Draw.c), as ImagingDrawWideLine applies them to the half width and the offsets
static int marks_ru(double f) { return (int)(f >= 0.0 ? std::floor(f + 0.5) : -std::floor(std::fabs(f) + 0.5)); }
static int marks_rd(double f) { return (int)(f >= 0.0 ? std::ceil(f - 0.5) : -std::ceil(std::fabs(f) - 0.5)); }

// The four edges of Pillow's wide line (the contract at the head of marks.hip); the zero-length line is four horizontal edges
// on its one pixel
static void marks_line_edges(int x0, int y0, int x1, int y1, int width, MarkEdge e[4]) {
    const int dx = x1 - x0, dy = y1 - y0;
    int v[4][2] = {{x0, y0}, {x0, y0}, {x0, y0}, {x0, y0}};
    if (dx != 0 || dy != 0) {
        const double big = std::hypot((double)dx, (double)dy), small = (width - 1) / 2.0;
        const double rmax = marks_ru(small) / big, rmin = marks_rd(small) / big;
        const int dxmin = marks_rd(rmin * dy), dxmax = marks_rd(rmax * dy), dymin = marks_ru(rmin * dx), dymax = marks_ru(rmax * dx);
        v[0][0] = x0 - dxmin; v[0][1] = y0 + dymax; v[1][0] = x1 - dxmin; v[1][1] = y1 + dymax;
        v[2][0] = x1 + dxmax; v[2][1] = y1 - dymin; v[3][0] = x0 + dxmax; v[3][1] = y0 - dymin;
    }
    for (int i = 0; i < 4; ++i) {
        const int ax = v[i][0], ay = v[i][1], bx = v[(i + 1) & 3][0], by = v[(i + 1) & 3][1];
        MarkEdge& k = e[i];
        k.xmin = std::min(ax, bx); k.xmax = std::max(ax, bx); k.ymin = std::min(ay, by); k.ymax = std::max(ay, by);
        k.x0 = ax; k.y0 = ay; k.horiz = ay == by;
        k.dx = k.horiz ? 0.f : (float)(bx - ax) / (float)(by - ay);
    }
}

int specmi_draw_marks(specmi_handle* h, uint8_t* slab, size_t slab_bytes, const int32_t* frame_geom, const int64_t* frame_offsets,
                      int nframes, const int64_t* marks, int nmarks, const uint8_t* masks, size_t mask_bytes, void* stream) {
    ENTER(h);
    if (!slab || !frame_geom || !frame_offsets || (nmarks > 0 && !marks)) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (nframes <= 0 || nframes > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 frames per call, got %d", nframes);
    if (nmarks < 0) return fail(h, SPECMI_ERR_ARG, "%d marks", nmarks);
    // the marks first: [nframes frame records | nmarks mark records | tiles]
    const size_t marks_at = (size_t)nframes * kMarkFrameRec, tiles_at = marks_at + (size_t)nmarks * kMarkDevRec;
    std::vector<int> tab(tiles_at, 0);
    for (int m = 0; m < nmarks; ++m) {
        const int64_t* r = marks + (size_t)m * kMarkRec;
        MarkDev d{};
        if (r[0] != kMarkStrip && r[0] != kMarkMask && r[0] != kMarkLine) return fail(h, SPECMI_ERR_ARG, "mark %d: unknown kind %lld", m, (long long)r[0]);
        if (r[1] < 0 || r[1] > 0xffffff) return fail(h, SPECMI_ERR_ARG, "mark %d: colour %lld is not r | g << 8 | b << 16", m, (long long)r[1]);
        d.kind = (int)r[0]; d.rgb = (unsigned)r[1];
        if (d.kind == kMarkStrip) {
            d.a = (int)std::min<int64_t>(std::max<int64_t>(r[2], 0), kMarkMaxSide);       // the kernel writes rows below H only
            d.b = (int)std::min<int64_t>(std::max<int64_t>(r[3], 0), kMarkMaxSide);
        } else if (d.kind == kMarkMask) {
            if (!masks) return fail(h, SPECMI_ERR_ARG, "mark %d is a mask blend, but the mask buffer is a null pointer", m);
            if (r[4] < 1 || r[4] > kMarkMaxMaskSide || r[5] < 1 || r[5] > kMarkMaxMaskSide)
                return fail(h, SPECMI_ERR_ARG, "mark %d: a mask of %lld x %lld (1 .. %d per side)", m, (long long)r[4], (long long)r[5], kMarkMaxMaskSide);
            if (r[2] < -kMarkMaxMaskPos || r[2] > kMarkMaxMaskPos || r[3] < -kMarkMaxMaskPos || r[3] > kMarkMaxMaskPos)
                return fail(h, SPECMI_ERR_ARG, "mark %d: mask position (%lld, %lld) outside [-%d, %d]", m, (long long)r[2], (long long)r[3], kMarkMaxMaskPos, kMarkMaxMaskPos);
            if (r[6] < 0 || (uint64_t)r[6] > mask_bytes || (uint64_t)(r[4] * r[5]) > mask_bytes - (uint64_t)r[6])
                return fail(h, SPECMI_ERR_ARG, "mark %d: its mask leaves the mask buffer of %zu bytes", m, mask_bytes);
            d.a = (int)r[2]; d.b = (int)r[3]; d.c = (int)r[4]; d.d = (int)r[5]; d.off = r[6];
        } else {
            for (int k = 2; k < 6; ++k)
                if (r[k] < -kMarkMaxCoord || r[k] > kMarkMaxCoord)
                    return fail(h, SPECMI_ERR_ARG, "mark %d: line end point %lld outside [-%d, %d]", m, (long long)r[k], kMarkMaxCoord, kMarkMaxCoord);
            if (r[6] < kMarkMinWidth || r[6] > kMarkMaxWidth) return fail(h, SPECMI_ERR_ARG, "mark %d: line width %lld (%d .. %d)", m, (long long)r[6], kMarkMinWidth, kMarkMaxWidth);
            marks_line_edges((int)r[2], (int)r[3], (int)r[4], (int)r[5], (int)r[6], d.e);
        }
        std::memcpy(tab.data() + marks_at + (size_t)m * kMarkDevRec, &d, sizeof(d));
    }
    std::vector<ByteRect> rects((size_t)nframes);
    std::vector<unsigned char> hit;
    long long ntiles = 0;
    for (int f = 0; f < nframes; ++f) {
        const int H = frame_geom[4 * f], W = frame_geom[4 * f + 1], mark0 = frame_geom[4 * f + 2], count = frame_geom[4 * f + 3];
        const int64_t off = frame_offsets[2 * f], pitch = frame_offsets[2 * f + 1];
        if (H < 1 || W < 1 || H > kMarkMaxSide || W > kMarkMaxSide) return fail(h, SPECMI_ERR_ARG, "frame %d: %d x %d pixels (1 .. %d per side)", f, H, W, kMarkMaxSide);
        if (count < 0 || mark0 < 0 || (long long)mark0 + count > nmarks)
            return fail(h, SPECMI_ERR_ARG, "frame %d: marks %d .. %lld leave the call's %d", f, mark0, (long long)mark0 + count, nmarks);
        if (int rc = check_rect(h, "frame", f, off, pitch, H, W, slab_bytes)) return rc;
        MarkFrame r{};
        r.off = off; r.pitch = stored_pitch(pitch, H, W); r.H = H; r.W = W; r.mark0 = mark0; r.count = count;
        std::memcpy(tab.data() + (size_t)f * kMarkFrameRec, &r, sizeof(r));
        rects[f] = ByteRect{off, r.pitch, 3LL * W, H};
        if (!count) continue;
        // the tiles some mark of this frame can reach: a superset is harmless (a tile's threads write only covered pixels)
        const int tx_n = (W + kMarkTileW - 1) / kMarkTileW, ty_n = (H + kMarkTileH - 1) / kMarkTileH;
        hit.assign((size_t)tx_n * ty_n, 0);
        const auto span = [&](int y, int xa, int xb) {          // row y, columns xa .. xb: clipped here
            xa = std::max(xa, 0); xb = std::min(xb, W - 1);
            if (y < 0 || y >= H || xa > xb) return;
            std::memset(hit.data() + (size_t)(y / kMarkTileH) * tx_n + xa / kMarkTileW, 1, (size_t)(xb / kMarkTileW - xa / kMarkTileW + 1));
        };
        for (int m = mark0; m < mark0 + count; ++m) {
            MarkDev d;
            std::memcpy(&d, tab.data() + marks_at + (size_t)m * kMarkDevRec, sizeof(d));
            if (d.kind == kMarkStrip) {
                for (int y = d.a; y < std::min(d.b, H); y = (y / kMarkTileH + 1) * kMarkTileH) span(y, 0, W - 1);
            } else if (d.kind == kMarkMask) {
                for (int y = std::max(d.b, 0); y < std::min(d.b + d.d, H); y = (y / kMarkTileH + 1) * kMarkTileH) span(y, d.a, d.a + d.c - 1);
            } else {
                int ylo = H, yhi = -1;
                for (int i = 0; i < 4; ++i) {
                    if (d.e[i].horiz) span(d.e[i].ymin, d.e[i].xmin, d.e[i].xmax);
                    else { ylo = std::min(ylo, d.e[i].ymin); yhi = std::max(yhi, d.e[i].ymax); }
                }
                for (int y = std::max(ylo, 0); y <= std::min(yhi, H - 1); ++y) {
                    int xa, xb;
                    mark_line_span(d.e, y, xa, xb);
                    if (xa <= xb) span(y, xa - 1, xb + 1);
                }
            }
        }
        for (int t = 0; t < tx_n * ty_n; ++t)
            if (hit[t]) {
                tab.push_back(f);
                tab.push_back((t / tx_n) << 16 | (t % tx_n));
                ++ntiles;
            }
        if (ntiles >= (1LL << 30)) return fail(h, SPECMI_ERR_ARG, "the marks reach 2^30 tiles of %d x %d pixels or more", kMarkTileW, kMarkTileH);
    }
    int ra, rb;
    if (first_overlap(rects, &ra, &rb)) return fail(h, SPECMI_ERR_ARG, "frames %d and %d share a byte", ra, rb);
    hipStream_t s = (hipStream_t)stream;
    DevTable& T = h->tab[TAB_marks];
    if (int rc = publish_table(h, T, tab, "the marks table", "new frame or mark records", s)) return rc;
    const int* dtab = (const int*)T.dev.p;
    MarksArgs a{};
    a.frames = (const MarkFrame*)dtab; a.marks = (const MarkDev*)(dtab + marks_at); a.tiles = dtab + tiles_at;
    a.masks = masks; a.slab = slab; a.ntiles = (int)ntiles;
    LaunchCtx ctx{s, &h->prof, "render.marks"};
    LAUNCHCHK(h, launch_draw_marks(a, (double)ntiles * kMarkTileW * kMarkTileH, ctx), "draw_marks");
    return SPECMI_OK;
}

int specmi_denormalize_u8(specmi_handle* h, const float* x, int B, int Hp, int Wp, int index, int H, int W, const float* mean3,
                          const float* std3, uint8_t* slab, size_t slab_bytes, int64_t offset, int64_t pitch, void* stream) {
    ENTER(h);
    if (!x || !slab) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (B < 1 || Hp < 1 || Wp < 1 || Hp > 32768 || Wp > 32768) return fail(h, SPECMI_ERR_ARG, "a batch of %d images of %d x %d (1 .. 32768 per side)", B, Hp, Wp);
    if (index < 0 || index >= B) return fail(h, SPECMI_ERR_ARG, "image %d of %d", index, B);
    if (H < 1 || H > Hp || W < 1 || W > Wp) return fail(h, SPECMI_ERR_ARG, "a frame of %d x %d out of an image of %d x %d", H, W, Hp, Wp);
    if (pitch < 3LL * W) return fail(h, SPECMI_ERR_ARG, "a pitch of %lld bytes for rows of %d", (long long)pitch, 3 * W);
    if (!rect_in_slab(offset, pitch, H, W, slab_bytes))
        return fail(h, SPECMI_ERR_ARG, "the frame's rectangle leaves the slab of %zu bytes", slab_bytes);
    DenormArgs a{};
    a.plane = (long long)Hp * Wp;
    a.x = x + (size_t)index * 3 * (size_t)a.plane; a.out = slab + offset; a.pitch = pitch; a.h = H; a.w = W; a.Wp = Wp;
    for (int c = 0; c < 3; ++c) {
        imagenet_mean_std(c, a.mean[c], a.std[c]);                       // the defaults, as pare's denormalize_images
        if (mean3) a.mean[c] = mean3[c];
        if (std3) a.std[c] = std3[c];
        if (!std::isfinite(a.mean[c]) || !std::isfinite(a.std[c])) return fail(h, SPECMI_ERR_ARG, "mean and std must be finite");
    }
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "render.denormalize"};
    LAUNCHCHK(h, launch_denormalize_u8(a, ctx), "denormalize_u8");
    return SPECMI_OK;
}

int specmi_color_jitter(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                        const int32_t* frame_geom, const int64_t* frame_offsets, const int32_t* records, int nframes, void* stream) {
    ENTER(h);
    if (!in_slab || !out_slab || !frame_geom || !frame_offsets || !records) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (nframes <= 0 || nframes > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 frames per call, got %d", nframes);
    // in place = the same slab and every frame on its own rectangle; any other shared byte is refused
    const bool in_place = in_slab == out_slab;
    if (!in_place && slabs_overlap(in_slab, in_slab_bytes, out_slab, out_slab_bytes))
        return fail(h, SPECMI_ERR_ARG, "the two slabs overlap without being the same (in place: the same pointer and rectangles)");
    static_assert(sizeof(JitterFrame) == kJitterFrameRec * sizeof(int) && sizeof(JitterRec) == 8 * sizeof(int), "the frame records are kept as ints");
    std::vector<int> tab((size_t)nframes * kJitterFrameRec, 0);
    std::vector<ByteRect> rects((size_t)nframes);
    long long tiles = 0, stiles = 0;
    double px = 0.0, stat_px = 0.0;
    for (int f = 0; f < nframes; ++f) {
        const int H = frame_geom[2 * f], W = frame_geom[2 * f + 1];
        const int64_t* o = frame_offsets + 4 * (size_t)f;
        if (H < 1 || W < 1 || H > kJitterMaxSide || W > kJitterMaxSide)
            return fail(h, SPECMI_ERR_ARG, "frame %d: %d x %d pixels (1 .. %d per side)", f, H, W, kJitterMaxSide);
        if (int rc = check_rect(h, "frame", f, o[0], o[1], H, W, in_slab_bytes)) return rc;
        if (int rc = check_rect(h, "frame (output)", f, o[2], o[3], H, W, out_slab_bytes)) return rc;
        JitterFrame r{};
        r.in_off = o[0]; r.in_pitch = stored_pitch(o[1], H, W); r.out_off = o[2]; r.out_pitch = stored_pitch(o[3], H, W);
        if (in_place && (r.in_off != r.out_off || r.in_pitch != r.out_pitch))
            return fail(h, SPECMI_ERR_ARG, "frame %d: in place, but its output rectangle is not its input rectangle", f);
        r.H = H; r.W = W; r.tile0 = (int)tiles; r.stile0 = (int)stiles; r.npre = -1;
        const int32_t* q = records + 8 * (size_t)f;
        unsigned seen = 0;
        for (int i = 0; i < 4; ++i) {
            if (q[i] < -1 || q[i] > 3) return fail(h, SPECMI_ERR_ARG, "frame %d: operation id %d outside [-1, 3]", f, q[i]);
            if (q[i] < 0) continue;
            if (seen & (1u << q[i])) return fail(h, SPECMI_ERR_ARG, "frame %d: operation %d is named twice", f, q[i]);
            seen |= 1u << q[i];
            if (q[i] == kJitterContrast) r.npre = r.nops;
            r.rec.op[r.nops++] = q[i];
        }
        for (int i = r.nops; i < 4; ++i) r.rec.op[i] = -1;
        std::memcpy(r.rec.f, q + 4, sizeof(r.rec.f));
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(r.rec.f[i]) || r.rec.f[i] < 0.f) return fail(h, SPECMI_ERR_ARG, "frame %d: factor %d is negative or not finite", f, i);
        if (q[7] < 0 || q[7] > 255) return fail(h, SPECMI_ERR_ARG, "frame %d: hue shift %d outside [0, 255]", f, q[7]);
        r.rec.k = q[7];
        const int n = jitter_frame_tiles(H, W, &r.tiles_x);
        tiles += n; px += (double)H * W;
        if (r.npre >= 0) { stiles += n; stat_px += (double)H * W; }
        if (tiles >= 2147483648LL) return fail(h, SPECMI_ERR_ARG, "the frames hold 2^31 tiles of %d x %d pixels or more", kJitterTileW, kJitterTileH);
        std::memcpy(tab.data() + (size_t)f * kJitterFrameRec, &r, sizeof(r));
        rects[f] = ByteRect{r.out_off, r.out_pitch, 3LL * W, H};
    }
    int ra, rb;
    if (first_overlap(rects, &ra, &rb)) return fail(h, SPECMI_ERR_ARG, "frames %d and %d share an output byte", ra, rb);
    hipStream_t s = (hipStream_t)stream;
    DevTable& T = h->tab[TAB_jitter];
    DevBuf& sums = h->buf[BUF_jitter];
    if (int rc = publish_table(h, T, tab, "the jitter frame table", "new frame or jitter records", s, &sums, (size_t)nframes * sizeof(unsigned long long),
                               "the jitter sums"))
        return rc;
    JitterArgs a{};
    a.frames = (const JitterFrame*)T.dev.p; a.in = in_slab; a.out = out_slab; a.sums = (unsigned long long*)sums.p; a.nframes = nframes;
    LaunchCtx ctx{s, &h->prof, "preprocess.color_jitter"};
    LAUNCHCHK(h, launch_color_jitter(a, (int)stiles, (int)tiles, stat_px, px, ctx), "color_jitter");
    return SPECMI_OK;
}

// ---- what specmi_jpeg_encode and specmi_png_encode check alike, each part where both check it ------------------------------------
struct EncodePic { int H, W; long long in_off, in_pitch, out_off, cap; };      // in_pitch as the records store it

static int encode_call_checks(specmi_handle* h, const uint8_t* in_slab, const uint8_t* out_slab, const int32_t* pic_geom,
                              const int64_t* pic_offsets, int n, const int64_t* sizes) {
    if (!in_slab || !out_slab || !pic_geom || !pic_offsets || !sizes) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (n <= 0 || n > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 pictures per call, got %d", n);
    return SPECMI_OK;
}

// picture i: its geometry, its rectangle in the picture slab and its room in the output slab, min_cap bytes (`min_cap_what`) at least
static int encode_pic_checks(specmi_handle* h, int i, const int32_t* pic_geom, const int64_t* pic_offsets, size_t in_slab_bytes,
                             size_t out_slab_bytes, int min_cap, const char* min_cap_what, EncodePic* p) {
    const int H = pic_geom[2 * i], W = pic_geom[2 * i + 1];
    const long long in_off = pic_offsets[4 * i], in_pitch = pic_offsets[4 * i + 1], out_off = pic_offsets[4 * i + 2], cap = pic_offsets[4 * i + 3];
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return fail(h, SPECMI_ERR_ARG, "picture %d: %d x %d pixels (1 .. 32768 per side)", i, H, W);
    if (int rc = check_rect(h, "picture", i, in_off, in_pitch, H, W, in_slab_bytes)) return rc;
    if (cap < min_cap) return fail(h, SPECMI_ERR_ARG, "picture %d: a capacity of %lld bytes is below %s %d", i, cap, min_cap_what, min_cap);
    if (out_off < 0 || (double)out_off + (double)cap > (double)out_slab_bytes)
        return fail(h, SPECMI_ERR_ARG, "picture %d: its output leaves the slab of %zu bytes", i, out_slab_bytes);
    *p = EncodePic{H, W, in_off, stored_pitch(in_pitch, H, W), out_off, cap};
    return SPECMI_OK;
}

// after the pictures: no two outputs (first byte, capacity) share a byte
static int encode_outputs_disjoint(specmi_handle* h, std::vector<std::pair<long long, long long>>& outs) {
    long long at;
    if (first_shared_byte(outs, &at)) return fail(h, SPECMI_ERR_ARG, "two outputs share a byte (at offset %lld)", at);
    return SPECMI_OK;
}

int specmi_jpeg_encode(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                       const int32_t* pic_geom, const int64_t* pic_offsets, int n, int quality, int64_t* sizes, void* stream) {
    ENTER(h);
    int rc;
    if ((rc = encode_call_checks(h, in_slab, out_slab, pic_geom, pic_offsets, n, sizes))) return rc;
    if (quality < 1 || quality > 100) return fail(h, SPECMI_ERR_ARG, "quality %d (1 .. 100)", quality);
    if (slabs_overlap(in_slab, in_slab_bytes, out_slab, out_slab_bytes)) return fail(h, SPECMI_ERR_ARG, "the picture slab and the output slab overlap");
    // [n records | JpegTables]
    std::vector<int> tab((size_t)n * kJpegPicRec + sizeof(JpegTables) / 4, 0);
    std::vector<std::pair<long long, long long>> outs((size_t)n);       // first byte, capacity
    long long mcus = 0, mchunks = 0, bchunks = 0;
    double px = 0.0;
    for (int i = 0; i < n; ++i) {
        EncodePic p;
        if ((rc = encode_pic_checks(h, i, pic_geom, pic_offsets, in_slab_bytes, out_slab_bytes, kJpegHeaderBytes, "the header's", &p))) return rc;
        const int H = p.H, W = p.W;
        JpegPic r{};
        r.in_off = p.in_off; r.in_pitch = p.in_pitch; r.out_off = p.out_off; r.cap = p.cap;
        r.H = H; r.W = W; r.mx = (W + 15) / 16; r.my = (H + 15) / 16;
        r.mcu0 = (int)mcus; r.mchunk0 = (int)mchunks; r.bchunk0 = (int)bchunks;
        const long long m = (long long)r.mx * r.my;
        mcus += m;
        mchunks += (m + kJpegMcuChunk - 1) / kJpegMcuChunk;
        bchunks += (m * kJpegMcuBytes + kJpegByteChunk - 1) / kJpegByteChunk;
        px += (double)H * W;
        if (mcus > kJpegMaxMcus) return fail(h, SPECMI_ERR_ARG, "the pictures hold more than 2^24 blocks of 16 x 16 pixels");
        std::memcpy(tab.data() + (size_t)i * kJpegPicRec, &r, sizeof(r));
        outs[i] = {p.out_off, p.cap};
    }
    if ((rc = encode_outputs_disjoint(h, outs))) return rc;
    JpegTables tables;
    jpeg_build_tables(quality, &tables);
    std::memcpy(tab.data() + (size_t)n * kJpegPicRec, &tables, sizeof(tables));
    hipStream_t s = (hipStream_t)stream;
    size_t off[8];
    const size_t need = jpeg_ws_layout(n, mcus, mchunks, bchunks, off);
    DevTable& T = h->tab[TAB_jpeg];
    if ((rc = publish_table(h, T, tab, "the JPEG picture table", "new picture records, another quality or a larger encoder workspace", s,
                            &h->buf[BUF_jpeg], need, "the JPEG workspace")))
        return rc;
    char* ws = (char*)h->buf[BUF_jpeg].p;
    const int* dtab = (const int*)T.dev.p;
    JpegArgs a{};
    a.in = in_slab; a.out = out_slab; a.sizes = (long long*)sizes;
    a.pics = (const JpegPic*)dtab; a.tabs = (const JpegTables*)(dtab + (size_t)n * kJpegPicRec);
    a.coef = (short*)(ws + off[0]); a.mcu_bits = (unsigned*)(ws + off[1]); a.mchunk_sum = (unsigned*)(ws + off[2]);
    a.mchunk_base = (unsigned long long*)(ws + off[3]); a.pic_bits = (unsigned long long*)(ws + off[4]); a.bitbuf = (unsigned*)(ws + off[5]);
    a.bchunk_ff = (unsigned*)(ws + off[6]); a.bchunk_base = (unsigned long long*)(ws + off[7]);
    a.n = n; a.mcus = (int)mcus; a.mchunks = (int)mchunks; a.bchunks = (int)bchunks;
    LaunchCtx ctx{s, &h->prof, "jpeg.encode"};
    LAUNCHCHK(h, launch_jpeg_encode(a, px * 3, ctx), "jpeg_encode");
    return SPECMI_OK;
}

int specmi_png_encode(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, uint8_t* out_slab, size_t out_slab_bytes,
                      const int32_t* pic_geom, const int64_t* pic_offsets, int n, int64_t* sizes, void* stream) {
    ENTER(h);
    int rc;
    if ((rc = encode_call_checks(h, in_slab, out_slab, pic_geom, pic_offsets, n, sizes))) return rc;
    if (slabs_overlap(in_slab, in_slab_bytes, out_slab, out_slab_bytes)) return fail(h, SPECMI_ERR_ARG, "the picture slab and the output slab overlap");
    std::vector<int> tab((size_t)n * kPngPicRec, 0);
    std::vector<std::pair<long long, long long>> outs((size_t)n);       // first byte, capacity
    long long rows = 0, segs = 0, filt = 0;
    double px = 0.0;
    for (int i = 0; i < n; ++i) {
        EncodePic p;
        if ((rc = encode_pic_checks(h, i, pic_geom, pic_offsets, in_slab_bytes, out_slab_bytes, kPngOverhead, "the fixed overhead of", &p))) return rc;
        const int H = p.H, W = p.W;
        // IDAT's length field: the zlib stream with every segment stored is the bound minus what stands around it
        if (png_bound(H, W) - (kPngOverhead - 6) >= (1LL << 31))
            return fail(h, SPECMI_ERR_ARG, "picture %d: the zlib stream of %d x %d pixels may not fit one IDAT chunk (2^31 bytes)", i, H, W);
        PngPic r{};
        r.in_off = p.in_off; r.in_pitch = p.in_pitch; r.out_off = p.out_off; r.cap = p.cap;
        r.H = H; r.W = W; r.stream = (long long)H * (1 + 3LL * W); r.filt_off = filt;
        r.row0 = (int)rows; r.seg0 = (int)segs; r.nseg = (int)((r.stream + kPngSegment - 1) / kPngSegment);
        rows += H; segs += r.nseg; filt += (r.stream + 255) & ~255LL;
        px += (double)H * W;
        if (segs > kPngMaxSegments) return fail(h, SPECMI_ERR_ARG, "the pictures' filtered streams hold more than 2^23 segments of 32768 bytes");
        std::memcpy(tab.data() + (size_t)i * kPngPicRec, &r, sizeof(r));
        outs[i] = {p.out_off, p.cap};
    }
    if ((rc = encode_outputs_disjoint(h, outs))) return rc;
    hipStream_t s = (hipStream_t)stream;
    size_t off[7];
    const size_t need = png_ws_layout(n, filt, segs, off);
    DevTable& T = h->tab[TAB_png];
    if ((rc = publish_table(h, T, tab, "the PNG picture table", "new picture records or a larger encoder workspace", s, &h->buf[BUF_png], need,
                            "the PNG workspace")))
        return rc;
    char* ws = (char*)h->buf[BUF_png].p;
    PngArgs a{};
    a.in = in_slab; a.out = out_slab; a.sizes = (long long*)sizes; a.pics = (const PngPic*)T.dev.p;
    a.filt = (unsigned char*)(ws + off[0]); a.segbuf = (unsigned*)(ws + off[1]); a.seg_bytes = (unsigned*)(ws + off[2]);
    a.seg_sum = (unsigned*)(ws + off[3]); a.seg_base = (unsigned long long*)(ws + off[4]); a.seg_crc = (unsigned*)(ws + off[5]);
    a.pic_adler = (unsigned*)(ws + off[6]);
    a.n = n; a.rows = (int)rows; a.segs = (int)segs;
    LaunchCtx ctx{s, &h->prof, "png.encode"};
    LAUNCHCHK(h, launch_png_encode(a, px * 3, ctx), "png_encode");
    return SPECMI_OK;
}

int specmi_jpeg_probe(const uint8_t* file, size_t bytes, int32_t* reason, int32_t* H, int32_t* W, int32_t* sampling) {
    if (!file || !reason || !H || !W || !sampling) return SPECMI_ERR_ARG;
    JdecFile f;
    *reason = jpeg_probe(file, bytes, &f);
    *H = f.H; *W = f.W;
    *sampling = *reason != JDEC_SUPPORTED ? 0 : (f.s420 ? 420 : 444);
    return SPECMI_OK;
}

int specmi_jpeg_decode(specmi_handle* h, const uint8_t* files_host, const uint8_t* in_slab, size_t in_slab_bytes, const int64_t* file_ranges,
                       uint8_t* out_slab, size_t out_slab_bytes, const int64_t* out_offsets, int n, int32_t* status, int16_t* coef,
                       size_t coef_bytes, int32_t* passes, void* stream) {
    ENTER(h);
    if (!files_host || !in_slab || !file_ranges || !out_slab || !out_offsets || !status) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (n <= 0 || n > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 files per call, got %d", n);
    if (slabs_overlap(in_slab, in_slab_bytes, out_slab, out_slab_bytes)) return fail(h, SPECMI_ERR_ARG, "the file slab and the output slab overlap");
    std::vector<int> tab((size_t)n * (sizeof(JdecFile) / 4), 0);
    std::vector<ByteRect> rects((size_t)n);
    long long mcus = 0, blocks = 0, plane_bytes = 0, lanes = 0, groups = 0, bchunks = 0, pchunks = 0, max_groups = 1;
    double px = 0.0, in_bytes = 0.0;
    for (int i = 0; i < n; ++i) {
        const int64_t off = file_ranges[2 * i], len = file_ranges[2 * i + 1], out_off = out_offsets[2 * i], pitch = out_offsets[2 * i + 1];
        if (off < 0 || len < 0 || (double)off + (double)len > (double)in_slab_bytes)
            return fail(h, SPECMI_ERR_ARG, "file %d: its bytes leave the slab of %zu bytes", i, in_slab_bytes);
        JdecFile f;
        const int reason = jpeg_probe(files_host + off, (size_t)len, &f);
        if (reason != JDEC_SUPPORTED) return fail(h, SPECMI_ERR_ARG, "file %d is not a supported baseline JPEG file (specmi_jpeg_probe: reason %d)", i, reason);
        if (int rc = check_rect(h, "file", i, out_off, pitch, f.H, f.W, out_slab_bytes)) return rc;
        const long long m = (long long)f.mx * f.my;
        f.scan_off += off; f.out_off = out_off; f.pitch = stored_pitch(pitch, f.H, f.W);
        f.block0 = blocks; f.plane0 = plane_bytes;
        f.nblocks = (int)(m * f.bpm);
        const long long nsub = std::max<long long>(1, (f.scan_len + kJdecSubBytes - 1) / kJdecSubBytes);
        const long long g = (nsub + kJdecGroup - 1) / kJdecGroup;
        mcus += m;
        if (mcus > kJdecMaxMcus || lanes + g * kJdecGroup > (1LL << 30))
            return fail(h, SPECMI_ERR_ARG, "the files hold more than 2^24 MCUs or 2^37 scan bytes");
        f.nsub = (int)nsub; f.lane0 = (int)lanes; f.group0 = (int)groups; f.bchunk0 = (int)bchunks; f.pchunk0 = (int)pchunks;
        blocks += m * f.bpm;
        plane_bytes += m * (f.s420 ? 384 : 192);
        lanes += g * kJdecGroup;
        groups += g;
        max_groups = std::max(max_groups, g);
        bchunks += (m * f.bpm + 255) / 256;
        pchunks += ((long long)f.H * f.W + 255) / 256;
        px += (double)f.H * f.W;
        in_bytes += (double)f.scan_len;
        std::memcpy(tab.data() + (size_t)i * (sizeof(JdecFile) / 4), &f, sizeof(f));
        rects[i] = ByteRect{out_off, f.pitch, 3LL * f.W, f.H};
    }
    int ra, rb;
    if (first_overlap(rects, &ra, &rb)) return fail(h, SPECMI_ERR_ARG, "the output rectangles of files %d and %d share a byte", ra, rb);
    if (coef && coef_bytes < (size_t)blocks * 128)
        return fail(h, SPECMI_ERR_ARG, "the coefficient output holds %zu bytes, these files have %lld", coef_bytes, blocks * 128);
    hipStream_t s = (hipStream_t)stream;
    // the passes are counted on the host, so EVERY call is refused under capture, repeated records or not: asked here, ahead of the
    // table's own rule, which then has nothing left to ask
    if (stream_is_capturing(s))
        return fail(h, SPECMI_ERR_STATE, "specmi_jpeg_decode is not possible while the stream is being captured (nothing was enqueued)");
    size_t woff[8];
    const size_t need = jdec_ws_layout(blocks, plane_bytes, lanes, groups, woff);
    DevTable& T = h->tab[TAB_jdec];
    if (int rc = publish_table(h, T, tab, "the JPEG file table", nullptr, s, &h->buf[BUF_jdec], need, "the JPEG decoder workspace")) return rc;
    char* ws = (char*)h->buf[BUF_jdec].p;
    JdecArgs a{};
    a.in = in_slab; a.out = out_slab; a.files = (const JdecFile*)T.dev.p; a.status = status;
    a.coef = (short*)(ws + woff[0]); a.planes = (unsigned char*)(ws + woff[1]); a.entry = (unsigned*)(ws + woff[2]);
    a.exits = (unsigned*)(ws + woff[3]); a.count = (int*)(ws + woff[4]); a.first = (int*)(ws + woff[5]); a.gexit = (unsigned*)(ws + woff[6]);
    a.changed = (unsigned*)(ws + woff[7]);
    a.n = n; a.groups = (int)groups; a.bchunks = (int)bchunks; a.pchunks = (int)pchunks;
    LaunchCtx ctx{s, &h->prof, "jpeg.decode"};
    int npass = 0;
    LAUNCHCHK(h, launch_jpeg_decode(a, blocks, lanes, (int)max_groups, in_bytes, px * 3, &npass, ctx), "jpeg_decode");
    if (passes) *passes = npass;
    if (coef) HIPCHK(h, hipMemcpyAsync(coef, a.coef, (size_t)blocks * 128, hipMemcpyDeviceToDevice, s));
    return SPECMI_OK;
}

int specmi_png_probe(const uint8_t* file, size_t bytes, int32_t* reason, int32_t* H, int32_t* W, int32_t* colour_type, int64_t* idat_ranges,
                     int max_ranges, int32_t* nranges) {
    if (!file || !reason || !H || !W || !colour_type || !nranges || max_ranges < 0 || (max_ranges > 0 && !idat_ranges)) return SPECMI_ERR_ARG;
    int hh, ww, ct, nr;
    static_assert(sizeof(long long) == sizeof(int64_t), "the ranges are written as long long");
    *reason = png_probe(file, bytes, &hh, &ww, &ct, (long long*)idat_ranges, max_ranges, &nr);
    *H = hh; *W = ww; *colour_type = ct; *nranges = nr;
    return SPECMI_OK;
}

int specmi_png_decode(specmi_handle* h, const uint8_t* in_slab, size_t in_slab_bytes, const int64_t* stream_ranges, const int32_t* geom,
                      uint8_t* out_slab, size_t out_slab_bytes, const int64_t* out_offsets, int n, int32_t* status, uint8_t* raw,
                      size_t raw_bytes, void* stream) {
    ENTER(h);
    if (!in_slab || !stream_ranges || !geom || !out_slab || !out_offsets || !status) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (n <= 0 || n > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 files per call, got %d", n);
    if (slabs_overlap(in_slab, in_slab_bytes, out_slab, out_slab_bytes)) return fail(h, SPECMI_ERR_ARG, "the stream slab and the output slab overlap");
    std::vector<int> tab((size_t)n * (sizeof(PdecFile) / 4), 0);
    std::vector<ByteRect> rects((size_t)n);
    long long raw_total = 0, chunks = 0;
    double px = 0.0, in_bytes = 0.0;
    for (int i = 0; i < n; ++i) {
        const int64_t off = stream_ranges[2 * i], len = stream_ranges[2 * i + 1], out_off = out_offsets[2 * i], pitch = out_offsets[2 * i + 1];
        const int H = geom[3 * i], W = geom[3 * i + 1], ct = geom[3 * i + 2];
        if (off < 0 || len < 0 || (double)off + (double)len > (double)in_slab_bytes)
            return fail(h, SPECMI_ERR_ARG, "file %d: its stream leaves the slab of %zu bytes", i, in_slab_bytes);
        if (len < 8) return fail(h, SPECMI_ERR_ARG, "file %d: a zlib stream of %lld bytes (8 at least: header, a block, Adler-32)", i, (long long)len);
        if (H < 1 || H > 32768 || W < 1 || W > 32768) return fail(h, SPECMI_ERR_ARG, "file %d: %d x %d pixels (1 .. 32768 per side)", i, H, W);
        if (ct != 0 && ct != 2 && ct != 4 && ct != 6) return fail(h, SPECMI_ERR_ARG, "file %d: colour type %d (0, 2, 4 or 6)", i, ct);
        if (int rc = check_rect(h, "file", i, out_off, pitch, H, W, out_slab_bytes)) return rc;
        PdecFile f{};
        f.stream_off = off; f.stream_len = len; f.out_off = out_off; f.pitch = stored_pitch(pitch, H, W);
        f.H = H; f.W = W; f.bpp = ct == 0 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4; f.nch = (ct & 2) ? 3 : 1;
        f.raw_off = raw_total; f.raw_len = (long long)H * (1 + (long long)W * f.bpp);
        f.chunk0 = (int)chunks; f.nchunk = (int)((f.raw_len + kPdecAdlerChunk - 1) / kPdecAdlerChunk);
        raw_total += (f.raw_len + 255) & ~255LL;
        chunks += f.nchunk;
        if (raw_total > kPdecMaxRaw) return fail(h, SPECMI_ERR_ARG, "the files' inflated streams hold more than 2^31 bytes");
        px += (double)H * W;
        in_bytes += (double)len;
        std::memcpy(tab.data() + (size_t)i * (sizeof(PdecFile) / 4), &f, sizeof(f));
        rects[i] = ByteRect{out_off, f.pitch, 3LL * W, H};
    }
    int ra, rb;
    if (first_overlap(rects, &ra, &rb)) return fail(h, SPECMI_ERR_ARG, "the output rectangles of files %d and %d share a byte", ra, rb);
    if (raw && raw_bytes < (size_t)raw_total)
        return fail(h, SPECMI_ERR_ARG, "the raw output holds %zu bytes, these files' inflated streams take %lld", raw_bytes, raw_total);
    hipStream_t s = (hipStream_t)stream;
    size_t woff[3];
    const size_t need = pdec_ws_layout(n, raw_total, chunks, woff);
    DevTable& T = h->tab[TAB_pdec];
    if (int rc = publish_table(h, T, tab, "the PNG file table", "new file records or a larger decoder workspace", s, &h->buf[BUF_pdec], need,
                               "the PNG decoder workspace"))
        return rc;
    char* ws = (char*)h->buf[BUF_pdec].p;
    PdecArgs a{};
    a.in = in_slab; a.out = out_slab; a.files = (const PdecFile*)T.dev.p; a.status = status;
    a.raw = (unsigned char*)(ws + woff[0]); a.rec = (uint2*)(ws + woff[1]); a.sums = (uint2*)(ws + woff[2]);
    a.n = n; a.chunks = (int)chunks;
    LaunchCtx ctx{s, &h->prof, "png.decode"};
    LAUNCHCHK(h, launch_png_decode(a, in_bytes, (double)raw_total, px * 3, ctx), "png_decode");
    if (raw) HIPCHK(h, hipMemcpyAsync(raw, a.raw, (size_t)raw_total, hipMemcpyDeviceToDevice, s));
    return SPECMI_OK;
}

int specmi_crop_normalize(specmi_handle* h, const uint8_t* frame, int H, int W, const float* bboxes, int n, float scale,
                          int crop_size, float* out, uint8_t* raw, float* bbox_scale, float* bbox_center, void* stream) {
    ENTER(h);
    if (!frame || !bboxes || !out || H <= 0 || W <= 0 || n <= 0 || crop_size <= 0 || !(scale > 0.f))
        return fail(h, SPECMI_ERR_ARG, "bad argument");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "preprocess.crop"};
    LAUNCHCHK(h, launch_crop_normalize(frame, H, W, bboxes, n, scale, crop_size, out, raw, bbox_scale, bbox_center, ctx),
              "crop_normalize");
    return SPECMI_OK;
}

static int crop_normalize_batch(specmi_handle* h, const uint8_t* frames, int nframes, int H, int W, const int32_t* frame_index,
                                const float* bboxes, int n, float scale, int crop_size, void* out, bool f16, uint8_t* raw,
                                float* bbox_scale, float* bbox_center, void* stream) {
    ENTER(h);
    // the fp16 form is also the single-frame crop: frame_index == NULL with nframes == 1 means "every crop from frame 0"
    const bool single = f16 && !frame_index && nframes == 1;
    if (!frames || (!frame_index && !single) || !bboxes || !out || nframes <= 0 || H <= 0 || W <= 0 || n <= 0 || crop_size <= 0 || !(scale > 0.f))
        return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (f16) NEED_ALIGNED16(h, out);
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "preprocess.crop_batch"};
    LAUNCHCHK(h, launch_crop_normalize(frames, H, W, bboxes, n, scale, crop_size, out, raw, bbox_scale, bbox_center, ctx,
                                       frame_index, nframes, f16),
              "crop_normalize_batch");
    return SPECMI_OK;
}

int specmi_crop_normalize_batch(specmi_handle* h, const uint8_t* frames, int nframes, int H, int W, const int32_t* frame_index,
                                const float* bboxes, int n, float scale, int crop_size, float* out, uint8_t* raw,
                                float* bbox_scale, float* bbox_center, void* stream) {
    return crop_normalize_batch(h, frames, nframes, H, W, frame_index, bboxes, n, scale, crop_size, out, false, raw, bbox_scale,
                                bbox_center, stream);
}

int specmi_crop_normalize_batch_f16(specmi_handle* h, const uint8_t* frames, int nframes, int H, int W, const int32_t* frame_index,
                                    const float* bboxes, int n, float scale, int crop_size, void* out_nhwc8, uint8_t* raw,
                                    float* bbox_scale, float* bbox_center, void* stream) {
    return crop_normalize_batch(h, frames, nframes, H, W, frame_index, bboxes, n, scale, crop_size, out_nhwc8, true, raw, bbox_scale,
                                bbox_center, stream);
}

static int crop_resize_normalize(specmi_handle* h, const uint8_t* frame, int H, int W, const int32_t* boxes, int n, int crop_size,
                                 void* out, bool f16, void* stream) {
    ENTER(h);
    if (!frame || !boxes || !out || H <= 0 || W <= 0 || n <= 0 || crop_size <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (f16) NEED_ALIGNED16(h, out);
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "preprocess.dataset_crop"};
    LAUNCHCHK(h, launch_crop_resize_normalize(frame, H, W, boxes, n, crop_size, out, ctx, f16), "crop_resize_normalize");
    return SPECMI_OK;
}

int specmi_crop_resize_normalize(specmi_handle* h, const uint8_t* frame, int H, int W, const int32_t* boxes, int n,
                                 int crop_size, float* out, void* stream) {
    return crop_resize_normalize(h, frame, H, W, boxes, n, crop_size, out, false, stream);
}

int specmi_crop_resize_normalize_f16(specmi_handle* h, const uint8_t* frame, int H, int W, const int32_t* boxes, int n,
                                     int crop_size, void* out_nhwc8, void* stream) {
    return crop_resize_normalize(h, frame, H, W, boxes, n, crop_size, out_nhwc8, true, stream);
}

// the checks and the record table the two ragged crops share; everything is checked before the table is touched
static int crop_ragged_table(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets, const int32_t* geom,
                             int nframes, const int32_t* frame_index, const void* boxes, int n, int crop_size, const void* out, bool f16,
                             hipStream_t s) {
    if (!frames || !offsets || !geom || !frame_index || !boxes || !out) return fail(h, SPECMI_ERR_ARG, "bad argument (null pointer)");
    if (n <= 0 || n > 65535) return fail(h, SPECMI_ERR_ARG, "1 to 65535 crops per call (grid dimension), got %d", n);
    if (nframes <= 0) return fail(h, SPECMI_ERR_ARG, "at least one frame per call, got %d", nframes);
    if (crop_size < 1) return fail(h, SPECMI_ERR_ARG, "a crop size of %d", crop_size);
    if (f16) NEED_ALIGNED16(h, out);
    if (slab_bytes >= 4294967296.0) return fail(h, SPECMI_ERR_ARG, "a frame slab of %zu bytes is beyond the kernels' 32-bit offsets", slab_bytes);
    static_assert(sizeof(CropFrame) % sizeof(int) == 0, "the frame records are kept as ints");
    constexpr size_t kRec = sizeof(CropFrame) / sizeof(int);
    std::vector<int> tab((size_t)nframes * kRec, 0);
    for (int f = 0; f < nframes; ++f) {
        const int H = geom[2 * f], W = geom[2 * f + 1];
        if (H < 1 || W < 1 || H >= (1 << 24) || W >= (1 << 24)) return fail(h, SPECMI_ERR_ARG, "frame %d: size %d x %d (1 <= side < 2^24)", f, H, W);
        if (!rect_in_slab(offsets[f], 3LL * W, H, W, slab_bytes))
            return fail(h, SPECMI_ERR_ARG, "frame %d: %d x %d x 3 bytes at offset %lld leave the slab of %zu bytes", f, H, W, (long long)offsets[f], slab_bytes);
        const CropFrame r{(unsigned)offsets[f], H, W, 0};
        std::memcpy(tab.data() + (size_t)f * kRec, &r, sizeof(r));
    }
    return publish_table(h, h->tab[TAB_crop], tab, "the ragged-crop frame table", nullptr, s);
}

static int crop_normalize_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets, const int32_t* geom,
                                 int nframes, const int32_t* frame_index, const float* bboxes, int n, float scale, int crop_size,
                                 void* out, bool f16, uint8_t* raw, float* bbox_scale, float* bbox_center, void* stream) {
    ENTER(h);
    if (!(scale > 0.f)) return fail(h, SPECMI_ERR_ARG, "a scale of %g", (double)scale);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = crop_ragged_table(h, frames, slab_bytes, offsets, geom, nframes, frame_index, bboxes, n, crop_size, out, f16, s)) return rc;
    LaunchCtx ctx{s, &h->prof, "preprocess.crop_ragged"};
    LAUNCHCHK(h, launch_crop_normalize_ragged(frames, (const CropFrame*)h->tab[TAB_crop].dev.p, nframes, (double)slab_bytes, frame_index, bboxes, n, scale, crop_size, out,
                                              raw, bbox_scale, bbox_center, ctx, f16),
              "crop_normalize_ragged");
    return SPECMI_OK;
}

int specmi_crop_normalize_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets, const int32_t* geom,
                                 int nframes, const int32_t* frame_index, const float* bboxes, int n, float scale, int crop_size,
                                 float* out, uint8_t* raw, float* bbox_scale, float* bbox_center, void* stream) {
    return crop_normalize_ragged(h, frames, slab_bytes, offsets, geom, nframes, frame_index, bboxes, n, scale, crop_size, out, false, raw,
                                 bbox_scale, bbox_center, stream);
}

int specmi_crop_normalize_f16_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets, const int32_t* geom,
                                     int nframes, const int32_t* frame_index, const float* bboxes, int n, float scale, int crop_size,
                                     void* out_nhwc8, uint8_t* raw, float* bbox_scale, float* bbox_center, void* stream) {
    return crop_normalize_ragged(h, frames, slab_bytes, offsets, geom, nframes, frame_index, bboxes, n, scale, crop_size, out_nhwc8, true, raw,
                                 bbox_scale, bbox_center, stream);
}

static int crop_resize_normalize_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets,
                                        const int32_t* geom, int nframes, const int32_t* frame_index, const int32_t* boxes, int n,
                                        int crop_size, void* out, bool f16, void* stream) {
    ENTER(h);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = crop_ragged_table(h, frames, slab_bytes, offsets, geom, nframes, frame_index, boxes, n, crop_size, out, f16, s)) return rc;
    LaunchCtx ctx{s, &h->prof, "preprocess.dataset_crop_ragged"};
    LAUNCHCHK(h, launch_crop_resize_normalize_ragged(frames, (const CropFrame*)h->tab[TAB_crop].dev.p, nframes, (double)slab_bytes, frame_index, boxes, n, crop_size, out, ctx, f16),
              "crop_resize_normalize_ragged");
    return SPECMI_OK;
}

int specmi_crop_resize_normalize_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets,
                                        const int32_t* geom, int nframes, const int32_t* frame_index, const int32_t* boxes, int n,
                                        int crop_size, float* out, void* stream) {
    return crop_resize_normalize_ragged(h, frames, slab_bytes, offsets, geom, nframes, frame_index, boxes, n, crop_size, out, false, stream);
}

int specmi_crop_resize_normalize_f16_ragged(specmi_handle* h, const uint8_t* frames, size_t slab_bytes, const int64_t* offsets,
                                            const int32_t* geom, int nframes, const int32_t* frame_index, const int32_t* boxes, int n,
                                            int crop_size, void* out_nhwc8, void* stream) {
    return crop_resize_normalize_ragged(h, frames, slab_bytes, offsets, geom, nframes, frame_index, boxes, n, crop_size, out_nhwc8, true, stream);
}

int specmi_eval_mesh(specmi_handle* h, const float* pred, const float* gt, int B, int V, const float* Jr, int J,
                     const int32_t* sel, int nsel, float* mpjpe, float* pampjpe, float* v2v, void* stream) {
    ENTER(h);
    if (!pred || !gt || !Jr || B <= 0 || V <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (J < 1 || J > 32 || nsel < 1 || nsel > 32) return fail(h, SPECMI_ERR_ARG, "J and nsel must be in [1,32]");
    if (!sel && nsel > J) return fail(h, SPECMI_ERR_ARG, "eval_mesh: joint_sel is NULL (the first nsel joints) but nsel = %d exceeds J = %d", nsel, J);
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "eval.mesh"};
    LAUNCHCHK(h, launch_eval_mesh(pred, gt, B, V, Jr, J, sel, nsel, mpjpe, pampjpe, v2v, ctx), "eval_mesh");
    return SPECMI_OK;
}

int specmi_eval_joints(specmi_handle* h, const float* pred, const float* gt, int B, int J, float* mpjpe, float* pampjpe,
                       void* stream) {
    ENTER(h);
    if (!pred || !gt || B <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (J < 1 || J > 32) return fail(h, SPECMI_ERR_ARG, "J must be in [1,32]");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "eval.joints"};
    LAUNCHCHK(h, launch_eval_joints(pred, gt, B, J, mpjpe, pampjpe, ctx), "eval_joints");
    return SPECMI_OK;
}

int specmi_eval_step(specmi_handle* h, const float* pred, const float* gt, int B, int V, const float* Jr, int J, const int32_t* sel,
                     int nsel, const float* pj, const float* gj, int Jk, float* err_sel, float* pa_err_sel, float* err_k,
                     float* pa_err_k, float* v2v, void* stream) {
    ENTER(h);
    if (!pred || !gt || !Jr || B <= 0 || V <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    if (J < 1 || J > 32 || nsel < 1 || nsel > 32) return fail(h, SPECMI_ERR_ARG, "J and nsel must be in [1,32]");
    if (!sel && nsel > J) return fail(h, SPECMI_ERR_ARG, "eval_step: joint_sel is NULL (the first nsel joints) but nsel = %d exceeds J = %d", nsel, J);
    if (!pj != !gj) return fail(h, SPECMI_ERR_ARG, "eval_step: pred_joints and gt_joints are given together or not at all");
    if (!pj && (err_k || pa_err_k)) return fail(h, SPECMI_ERR_ARG, "eval_step: err_k / pa_err_k asked for without pred_joints and gt_joints");
    if (pj && (Jk < 1 || Jk > 32)) return fail(h, SPECMI_ERR_ARG, "Jk must be in [1,32]");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "eval.step"};
    LAUNCHCHK(h, launch_eval_step(pred, gt, B, V, Jr, J, sel, nsel, pj, gj, Jk, err_sel, pa_err_sel, err_k, pa_err_k, v2v, ctx), "eval_step");
    return SPECMI_OK;
}

int specmi_regress_joints(specmi_handle* h, const float* vertices, int B, int V, const float* Jr, int J, float* joints,
                          void* stream) {
    ENTER(h);
    if (!vertices || !Jr || !joints || B <= 0 || V <= 0 || J <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "eval.regress_joints"};
    LAUNCHCHK(h, launch_regress_joints(vertices, B, V, Jr, J, joints, ctx), "regress_joints");
    return SPECMI_OK;
}

int specmi_hmr_loss(specmi_handle* h, int mode, const float* pred_pose, const float* pred_shape, const float* pred_cam,
                    const float* joints3d, const float* joints2d, const float* vertices, const float* pose, const float* betas,
                    const float* pose_conf, const float* pose_3d, const float* keypoints, const float* gt_vertices,
                    const int32_t* has_smpl, const int32_t* has_pose_3d, const float* orig_shape, const float* scale, int B, int V,
                    float w_shape, float w_keypoint, float w_pose, float w_smpl_part, float w_beta, float w_openpose, float w_gt,
                    float w_loss, float* terms, int32_t* counts, float* means, void* stream) {
    ENTER(h);
    (void)w_smpl_part;   // the part-segmentation branch: its criterion is never defined in the reference (spec/losses.py:131,259)
    if (B <= 0) return fail(h, SPECMI_ERR_ARG, "hmr_loss: B = %d must be positive", B);
    if (V <= 0 || V > 0x7fffffff / 3) return fail(h, SPECMI_ERR_ARG, "hmr_loss: V = %d must be positive with V * 3 below 2^31", V);
    if (mode != SPECMI_HMR_LOSS && mode != SPECMI_HMR_CAM_LOSS)
        return fail(h, SPECMI_ERR_ARG, "hmr_loss: mode = %d is not defined (0 = HMRLoss, 1 = HMRCamLoss)", mode);
    const struct { const void* p; const char* name; } required[] = {
        {pred_pose, "pred_pose"}, {pred_shape, "pred_shape"}, {pred_cam, "pred_cam"}, {joints3d, "joints3d"}, {joints2d, "joints2d"},
        {vertices, "vertices"}, {pose, "pose"}, {betas, "betas"}, {pose_conf, "pose_conf"}, {pose_3d, "pose_3d"},
        {keypoints, "keypoints"}, {has_smpl, "has_smpl"}, {has_pose_3d, "has_pose_3d"}, {terms, "terms"}};
    for (const auto& r : required)
        if (!r.p) return fail(h, SPECMI_ERR_ARG, "hmr_loss: %s is NULL", r.name);
    if (!gt_vertices && w_shape != 0.f)
        return fail(h, SPECMI_ERR_ARG, "hmr_loss: gt_vertices is NULL but shape_loss_weight = %g (NULL is accepted only with weight 0)", (double)w_shape);
    if (mode == SPECMI_HMR_CAM_LOSS && !orig_shape) return fail(h, SPECMI_ERR_ARG, "hmr_loss: orig_shape is NULL (HMRCamLoss needs it)");
    if (mode == SPECMI_HMR_CAM_LOSS && !scale) return fail(h, SPECMI_ERR_ARG, "hmr_loss: scale is NULL (HMRCamLoss needs it)");
    HmrLossArgs a;
    a.mode = mode; a.B = B; a.V = V;
    a.pred_pose = pred_pose; a.pred_shape = pred_shape; a.pred_cam = pred_cam; a.joints3d = joints3d; a.joints2d = joints2d;
    a.vertices = vertices; a.pose = pose; a.betas = betas; a.pose_conf = pose_conf; a.pose_3d = pose_3d; a.keypoints = keypoints;
    a.gt_vertices = gt_vertices; a.has_smpl = has_smpl; a.has_pose_3d = has_pose_3d; a.orig_shape = orig_shape; a.scale = scale;
    a.w_shape = w_shape; a.w_keypoint = w_keypoint; a.w_pose = w_pose; a.w_beta = w_beta; a.w_openpose = w_openpose; a.w_gt = w_gt;
    a.w_loss = w_loss;
    a.terms = terms; a.counts = counts; a.means = means;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "loss.hmr"};
    LAUNCHCHK(h, launch_hmr_loss(a, ctx), "hmr_loss");
    return SPECMI_OK;
}

int specmi_hmr_loss_backward(specmi_handle* h, int mode, const float* pred_pose, const float* pred_shape, const float* pred_cam,
                             const float* joints3d, const float* joints2d, const float* vertices, const float* pose, const float* betas,
                             const float* pose_conf, const float* pose_3d, const float* keypoints, const float* gt_vertices,
                             const int32_t* has_smpl, const int32_t* has_pose_3d, const float* orig_shape, const float* scale, int B, int V,
                             float w_shape, float w_keypoint, float w_pose, float w_smpl_part, float w_beta, float w_openpose, float w_gt,
                             float w_loss, const float* terms, const int32_t* counts, const float* g_means, float* g_pred_pose,
                             float* g_pred_shape, float* g_pred_cam, float* g_joints3d, float* g_joints2d, float* g_vertices,
                             void* stream) {
    ENTER(h);
    (void)w_smpl_part;
    if (B <= 0) return fail(h, SPECMI_ERR_ARG, "hmr_loss_backward: B = %d must be positive", B);
    if (V <= 0 || V > 0x7fffffff / 3) return fail(h, SPECMI_ERR_ARG, "hmr_loss_backward: V = %d must be positive with V * 3 below 2^31", V);
    if (mode != SPECMI_HMR_LOSS && mode != SPECMI_HMR_CAM_LOSS)
        return fail(h, SPECMI_ERR_ARG, "hmr_loss_backward: mode = %d is not defined (0 = HMRLoss, 1 = HMRCamLoss)", mode);
    const struct { const void* p; const char* name; } required[] = {
        {pred_pose, "pred_pose"}, {pred_shape, "pred_shape"}, {pred_cam, "pred_cam"}, {joints3d, "joints3d"}, {joints2d, "joints2d"},
        {vertices, "vertices"}, {pose, "pose"}, {betas, "betas"}, {pose_conf, "pose_conf"}, {pose_3d, "pose_3d"},
        {keypoints, "keypoints"}, {has_smpl, "has_smpl"}, {has_pose_3d, "has_pose_3d"}, {terms, "terms"}, {counts, "counts"},
        {g_means, "g_means"}};
    for (const auto& r : required)
        if (!r.p) return fail(h, SPECMI_ERR_ARG, "hmr_loss_backward: %s is NULL", r.name);
    if (!gt_vertices && w_shape != 0.f)
        return fail(h, SPECMI_ERR_ARG, "hmr_loss_backward: gt_vertices is NULL but shape_loss_weight = %g (NULL is accepted only with weight 0)", (double)w_shape);
    if (mode == SPECMI_HMR_CAM_LOSS && (!orig_shape || !scale))
        return fail(h, SPECMI_ERR_ARG, "hmr_loss_backward: orig_shape or scale is NULL (HMRCamLoss needs both)");
    if (!g_pred_pose && !g_pred_shape && !g_pred_cam && !g_joints3d && !g_joints2d && !g_vertices)
        return fail(h, SPECMI_ERR_ARG, "hmr_loss_backward: every output is NULL");
    HmrLossArgs a;
    a.mode = mode; a.B = B; a.V = V;
    a.pred_pose = pred_pose; a.pred_shape = pred_shape; a.pred_cam = pred_cam; a.joints3d = joints3d; a.joints2d = joints2d;
    a.vertices = vertices; a.pose = pose; a.betas = betas; a.pose_conf = pose_conf; a.pose_3d = pose_3d; a.keypoints = keypoints;
    a.gt_vertices = gt_vertices; a.has_smpl = has_smpl; a.has_pose_3d = has_pose_3d; a.orig_shape = orig_shape; a.scale = scale;
    a.w_shape = w_shape; a.w_keypoint = w_keypoint; a.w_pose = w_pose; a.w_beta = w_beta; a.w_openpose = w_openpose; a.w_gt = w_gt;
    a.w_loss = w_loss;
    a.terms = const_cast<float*>(terms); a.counts = const_cast<int*>(counts); a.means = nullptr;      // (read only by the backward)
    HmrLossGrads g{g_means, g_pred_pose, g_pred_shape, g_pred_cam, g_joints3d, g_joints2d, g_vertices};
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "loss.hmr_backward"};
    LAUNCHCHK(h, launch_hmr_loss_backward(a, g, ctx), "hmr_loss_backward");
    return SPECMI_OK;
}

int specmi_smpl_backward(specmi_handle* h, const float* rotmat, const float* betas, const float* cam, int B, const float* R,
                         const float* K, const float* bbox_scale, const float* bbox_center, const float* img_w, const float* img_h,
                         const float* g_vertices, const float* g_joints3d, const float* g_joints2d, const float* g_cam_t,
                         float* g_rotmat, float* g_betas, float* g_cam, void* stream) {
    ENTER(h); NEED_COMMIT(h);
    if (h->kind != SPECMI_MODEL_HMR && h->kind != SPECMI_MODEL_SMPL) return fail(h, SPECMI_ERR_STATE, "handle has no body model");
    if (B <= 0) return fail(h, SPECMI_ERR_ARG, "smpl_backward: B = %d must be positive", B);
    if (!rotmat || !betas || !cam) return fail(h, SPECMI_ERR_ARG, "smpl_backward: rotmat, betas and cam are required");
    if (!g_vertices && !g_joints3d && !g_joints2d && !g_cam_t)
        return fail(h, SPECMI_ERR_ARG, "smpl_backward: every upstream gradient is NULL");
    if (!g_rotmat && !g_betas && !g_cam) return fail(h, SPECMI_ERR_ARG, "smpl_backward: every output is NULL");
    const int use_cam = opt(h, OPT_use_cam);
    if (use_cam && (!R || !K || !bbox_scale || !bbox_center || !img_w || !img_h))
        return fail(h, SPECMI_ERR_ARG, "use_cam needs cam_rotmat, cam_intrinsics, bbox_scale, bbox_center, img_w, img_h");
    int rc;
    if ((rc = ensure_ws(h, B, 32, 32))) return rc;
    if ((rc = grow_ragged(h, h->buf[BUF_smpl_bwd], smpl_bwd_ws_floats(h->smpl.V, B) * 4, "the SMPL backward workspace"))) return rc;
    SmplBwdArgs a;
    SmplArgs& f = a.fwd;
    f.rotmat = rotmat; f.betas = betas; f.cam = cam; f.cam_rotmat = R; f.cam_intrinsics = K;
    f.bbox_scale = bbox_scale; f.bbox_center = bbox_center; f.img_w = img_w; f.img_h = img_h;
    f.vertices = h->verts_ws; f.joints3d = f.joints2d = f.cam_t = nullptr;
    f.pose_feat = h->pf_ws; f.A = h->A_ws; f.posed_j = h->pj_ws;
    f.B = B;
    f.mode = use_cam ? 0 : 1;
    f.focal_length = h->focal_length;
    f.img_res = (float)opt(h, OPT_img_res);
    f.normalize_joints2d = use_cam ? 0 : 1;
    f.skin_split = opt(h, OPT_smpl_skin_split);
    a.g_vertices = g_vertices; a.g_joints3d = g_joints3d; a.g_joints2d = g_joints2d; a.g_cam_t = g_cam_t;
    a.g_rotmat = g_rotmat; a.g_betas = g_betas; a.g_cam = g_cam;
    a.ws = (float*)h->buf[BUF_smpl_bwd].p;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "smpl.backward"};
    LAUNCHCHK(h, launch_smpl_backward(h->smpl, a, ctx), "smpl_backward");
    return SPECMI_OK;
}

int specmi_rot6d_forward(specmi_handle* h, const float* x6d, int N, float* rotmat, void* stream) {
    ENTER(h);
    if (!x6d || !rotmat || N <= 0) return fail(h, SPECMI_ERR_ARG, "rot6d_forward: x6d, rotmat and N > 0 are required");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "smpl.rot6d_forward"};
    LAUNCHCHK(h, launch_rot6d_forward(x6d, rotmat, N, ctx), "rot6d_forward");
    return SPECMI_OK;
}

int specmi_rot6d_backward(specmi_handle* h, const float* x6d, const float* g_rotmat, int N, float* g_x6d, void* stream) {
    ENTER(h);
    if (!x6d || !g_rotmat || !g_x6d || N <= 0) return fail(h, SPECMI_ERR_ARG, "rot6d_backward: x6d, g_rotmat, g_x6d and N > 0 are required");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "smpl.rot6d_backward"};
    LAUNCHCHK(h, launch_rot6d_backward(x6d, g_rotmat, g_x6d, N, ctx), "rot6d_backward");
    return SPECMI_OK;
}

// the refusals the two HMRHead training calls and the tape size share; nullptr = accepted, else the message
static const char* head_train_shape_refusal(int B, int F, int C, int n_iter) {
    if (B < 1 || B > (1 << 20)) return "B must be in [1, 2^20]";
    if (F < 1 || F > (1 << 20)) return "F must be in [1, 2^20]";
    if (C != 0 && C != 7) return "C must be 0 or 7 (use_cam_feats)";
    if (n_iter < 1 || n_iter > 3) return "n_iter must be in 1 .. 3";
    return nullptr;
}

int specmi_hmr_head_tape_floats(int B, int F, int C, int n_iter, int64_t* floats) {
    if (!floats || head_train_shape_refusal(B, F, C, n_iter)) return SPECMI_ERR_ARG;
    *floats = (int64_t)head_tape_floats(B, n_iter);
    return SPECMI_OK;
}

// the argument checks of both calls, and the kernels' argument block; `second` = init_state resp. g_state
static int head_train_args(specmi_handle* h, const char* who, const specmi_hmr_head_params* params, const float* xf, int64_t ld_xf,
                           const float* cam_feats, const uint8_t* masks, float p, int B, int F, int C, int n_iter, const void* tape,
                           const void* second, const char* second_name, HeadTrainArgs& a) {
    if (const char* why = head_train_shape_refusal(B, F, C, n_iter))
        return fail(h, SPECMI_ERR_ARG, "%s: %s (B = %d, F = %d, C = %d, n_iter = %d)", who, why, B, F, C, n_iter);
    if (masks && !(p >= 0.f && p < 1.f)) return fail(h, SPECMI_ERR_ARG, "%s: p = %g must be in [0, 1) when masks are given", who, (double)p);
    if (!params) return fail(h, SPECMI_ERR_ARG, "%s: params is NULL", who);
    const struct { const void* p; const char* name; } required[] = {
        {params->fc1_weight, "fc1.weight"}, {params->fc1_bias, "fc1.bias"}, {params->fc2_weight, "fc2.weight"}, {params->fc2_bias, "fc2.bias"},
        {params->decpose_weight, "decpose.weight"}, {params->decpose_bias, "decpose.bias"}, {params->decshape_weight, "decshape.weight"},
        {params->decshape_bias, "decshape.bias"}, {params->deccam_weight, "deccam.weight"}, {params->deccam_bias, "deccam.bias"},
        {xf, "xf"}, {tape, "tape"}, {second, second_name}, {C ? cam_feats : xf, "cam_feats"}};      // (cam_feats is read with C = 7 only)
    for (const auto& r : required) {
        if (!r.p) return fail(h, SPECMI_ERR_ARG, "%s: %s is NULL", who, r.name);
        if (reinterpret_cast<uintptr_t>(r.p) & 3) return fail(h, SPECMI_ERR_ARG, "%s: %s is not 4-byte aligned", who, r.name);
    }
    if (ld_xf < F) return fail(h, SPECMI_ERR_ARG, "%s: ld_xf = %lld is below the row length F = %d", who, (long long)ld_xf, F);
    a.p = HeadTrainParams{params->fc1_weight, params->fc1_bias, params->fc2_weight, params->fc2_bias, params->decpose_weight,
                          params->decpose_bias, params->decshape_weight, params->decshape_bias, params->deccam_weight, params->deccam_bias};
    a.xf = xf; a.ld_xf = (long)ld_xf; a.cam_feats = C ? cam_feats : nullptr; a.masks = masks;
    a.scale = masks ? (float)(1.0 / (1.0 - (double)p)) : 1.f;
    a.B = B; a.F = F; a.C = C; a.n_iter = n_iter;
    return SPECMI_OK;
}

int specmi_hmr_head_train_forward(specmi_handle* h, const specmi_hmr_head_params* params, const float* xf, int64_t ld_xf,
                                  const float* cam_feats, const float* init_state, const uint8_t* masks, float p, int B, int F, int C,
                                  int n_iter, float* state, float* tape, void* stream) {
    ENTER(h);
    HeadTrainArgs a;
    if (int rc = head_train_args(h, "hmr_head_train_forward", params, xf, ld_xf, cam_feats, masks, p, B, F, C, n_iter, tape, init_state,
                                 "init_state", a))
        return rc;
    if (!state) return fail(h, SPECMI_ERR_ARG, "hmr_head_train_forward: every output is NULL (state is required)");
    if (reinterpret_cast<uintptr_t>(state) & 3) return fail(h, SPECMI_ERR_ARG, "hmr_head_train_forward: state is not 4-byte aligned");
    if (int rc = grow_ragged(h, h->buf[BUF_head_train], head_train_fwd_ws_floats(B) * 4, "the HMRHead training workspace")) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "head.train_forward"};
    LAUNCHCHK(h, launch_head_train_forward(a, init_state, state, tape, (float*)h->buf[BUF_head_train].p, ctx), "hmr_head_train_forward");
    return SPECMI_OK;
}

int specmi_hmr_head_backward(specmi_handle* h, const specmi_hmr_head_params* params, const float* xf, int64_t ld_xf,
                             const float* cam_feats, const uint8_t* masks, float p, int B, int F, int C, int n_iter, const float* tape,
                             const float* g_state, float* g_xf, const specmi_hmr_head_grads* grads, void* stream) {
    ENTER(h);
    HeadTrainArgs a;
    if (int rc = head_train_args(h, "hmr_head_backward", params, xf, ld_xf, cam_feats, masks, p, B, F, C, n_iter, tape, g_state, "g_state", a))
        return rc;
    HeadTrainGrads g{};
    if (grads)
        g = HeadTrainGrads{grads->fc1_weight, grads->fc1_bias, grads->fc2_weight, grads->fc2_bias, grads->decpose_weight,
                           grads->decpose_bias, grads->decshape_weight, grads->decshape_bias, grads->deccam_weight, grads->deccam_bias};
    float* const outs[] = {g_xf, g.fc1_w, g.fc1_b, g.fc2_w, g.fc2_b, g.decpose_w, g.decpose_b, g.decshape_w, g.decshape_b, g.deccam_w, g.deccam_b};
    bool any = false;
    for (float* o : outs) {
        any = any || o;
        if (reinterpret_cast<uintptr_t>(o) & 3) return fail(h, SPECMI_ERR_ARG, "hmr_head_backward: an output is not 4-byte aligned");
    }
    if (!any) return fail(h, SPECMI_ERR_ARG, "hmr_head_backward: every output is NULL");
    if (int rc = grow_ragged(h, h->buf[BUF_head_train], head_train_bwd_ws_floats(B, n_iter) * 4, "the HMRHead training workspace")) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "head.backward"};
    LAUNCHCHK(h, launch_head_backward(a, tape, g_state, g_xf, g, (float*)h->buf[BUF_head_train].p, ctx), "hmr_head_backward");
    return SPECMI_OK;
}

// the refusals the two CamCalib head training calls and the tape size share; nullptr = accepted, else the message
static const char* cam_head_shape_refusal(int B, int F, int L, int Hc, int nbins) {
    if (L < 1 || L > 3) return "L must be in 1 .. 3";
    if (B < 1 || B > (1 << 20)) return "B must be in [1, 2^20]";
    if (F < 1 || F > (1 << 20)) return "F must be in [1, 2^20]";
    if (Hc < 1 || Hc > (1 << 20)) return "Hc must be in [1, 2^20]";
    if (nbins < 1 || nbins > (1 << 20)) return "nbins must be in [1, 2^20]";
    return nullptr;
}

int specmi_camcalib_head_tape_floats(int B, int F, int L, int Hc, int nbins, int64_t* floats) {
    if (!floats || cam_head_shape_refusal(B, F, L, Hc, nbins)) return SPECMI_ERR_ARG;
    *floats = (int64_t)cam_head_tape_floats(B, L, Hc);
    return SPECMI_OK;
}

// the argument checks of both calls, and the kernels' argument block; `second` = logits resp. g_logits
static int cam_head_args(specmi_handle* h, const char* who, const specmi_camcalib_head_params* params, const float* xf, int64_t ld_xf,
                         int B, int F, int L, int Hc, int nbins, const void* tape, const void* second, const char* second_name,
                         CamHeadArgs& a) {
    if (const char* why = cam_head_shape_refusal(B, F, L, Hc, nbins))
        return fail(h, SPECMI_ERR_ARG, "%s: %s (B = %d, F = %d, L = %d, Hc = %d, nbins = %d)", who, why, B, F, L, Hc, nbins);
    if (!params) return fail(h, SPECMI_ERR_ARG, "%s: params is NULL", who);
    static const char* const heads[3] = {"fc_vfov", "fc_pitch", "fc_roll"};
    for (int k = 0; k < 3; ++k)
        for (int l = 0; l < L; ++l) {
            const void* const two[2] = {params->weight[k][l], params->bias[k][l]};
            for (int i = 0; i < 2; ++i) {
                if (!two[i]) return fail(h, SPECMI_ERR_ARG, "%s: %s layer %d %s is NULL", who, heads[k], l, i ? "bias" : "weight");
                if (reinterpret_cast<uintptr_t>(two[i]) & 3)
                    return fail(h, SPECMI_ERR_ARG, "%s: %s layer %d %s is not 4-byte aligned", who, heads[k], l, i ? "bias" : "weight");
            }
        }
    const struct { const void* p; const char* name; } required[] = {{xf, "xf"}, {L > 1 ? tape : xf, "tape"}, {second, second_name}};
    for (const auto& r : required) {
        if (!r.p) return fail(h, SPECMI_ERR_ARG, "%s: %s is NULL", who, r.name);
        if (reinterpret_cast<uintptr_t>(r.p) & 3) return fail(h, SPECMI_ERR_ARG, "%s: %s is not 4-byte aligned", who, r.name);
    }
    if (ld_xf < F) return fail(h, SPECMI_ERR_ARG, "%s: ld_xf = %lld is below the row length F = %d", who, (long long)ld_xf, F);
    std::memset(&a, 0, sizeof(a));
    for (int k = 0; k < 3; ++k)
        for (int l = 0; l < L; ++l) { a.p.w[k][l] = params->weight[k][l]; a.p.b[k][l] = params->bias[k][l]; }
    a.xf = xf; a.ld_xf = (long)ld_xf; a.B = B; a.F = F; a.L = L; a.Hc = Hc; a.nbins = nbins;
    a.grouped = opt(h, OPT_camcalib_head_group) != 0;
    return SPECMI_OK;
}

int specmi_camcalib_head_train_forward(specmi_handle* h, const specmi_camcalib_head_params* params, const float* xf, int64_t ld_xf,
                                       int B, int F, int L, int Hc, int nbins, float* tape, float* logits, void* stream) {
    ENTER(h);
    CamHeadArgs a;
    if (int rc = cam_head_args(h, "camcalib_head_train_forward", params, xf, ld_xf, B, F, L, Hc, nbins, tape, logits, "logits", a)) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.head_train_forward"};
    LAUNCHCHK(h, launch_cam_head_train_forward(a, tape, logits, ctx), "camcalib_head_train_forward");
    return SPECMI_OK;
}

int specmi_camcalib_head_backward(specmi_handle* h, const specmi_camcalib_head_params* params, const float* xf, int64_t ld_xf, int B,
                                  int F, int L, int Hc, int nbins, const float* tape, const float* g_logits, float* g_xf,
                                  const specmi_camcalib_head_grads* grads, void* stream) {
    ENTER(h);
    CamHeadArgs a;
    if (int rc = cam_head_args(h, "camcalib_head_backward", params, xf, ld_xf, B, F, L, Hc, nbins, tape, g_logits, "g_logits", a)) return rc;
    CamHeadGrads g;
    std::memset(&g, 0, sizeof(g));
    bool any = g_xf != nullptr;
    if (reinterpret_cast<uintptr_t>(g_xf) & 3) return fail(h, SPECMI_ERR_ARG, "camcalib_head_backward: an output is not 4-byte aligned");
    if (grads)
        for (int k = 0; k < 3; ++k)
            for (int l = 0; l < L; ++l) {
                g.w[k][l] = grads->weight[k][l]; g.b[k][l] = grads->bias[k][l];
                any = any || g.w[k][l] || g.b[k][l];
                if ((reinterpret_cast<uintptr_t>(g.w[k][l]) | reinterpret_cast<uintptr_t>(g.b[k][l])) & 3)
                    return fail(h, SPECMI_ERR_ARG, "camcalib_head_backward: an output is not 4-byte aligned");
            }
    if (!any) return fail(h, SPECMI_ERR_ARG, "camcalib_head_backward: every output is NULL");
    if (L > 1)
        if (int rc = grow_ragged(h, h->buf[BUF_cam_head_train], cam_head_bwd_ws_floats(B, L, Hc) * 4, "the CamCalib head training workspace")) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.head_backward"};
    LAUNCHCHK(h, launch_cam_head_backward(a, tape, g_logits, g_xf, g, (float*)h->buf[BUF_cam_head_train].p, ctx), "camcalib_head_backward");
    return SPECMI_OK;
}

// the five layer shapes of the trainable conv layer
static bool conv_train_shape_ok(int KH, int KW, int stride, int pad) {
    const bool k1 = KH == 1 && KW == 1 && pad == 0, k3 = KH == 3 && KW == 3 && pad == 1, k7 = KH == 7 && KW == 7 && pad == 3;
    return ((k1 || k3) && (stride == 1 || stride == 2)) || (k7 && stride == 2);
}

int specmi_conv2d_wgrad_splits(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* splits) {
    if (!splits || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || !conv_train_shape_ok(KH, KW, stride, pad)) return SPECMI_ERR_ARG;
    *splits = conv_wgrad_splits(B, conv_out(H, KH, stride, pad), Cin, Cout, KH, KW);
    return SPECMI_OK;
}

// the argument checks specmi_conv2d_train_forward and specmi_conv2d_backward share, and the kernels' argument block
static int conv_train_args(specmi_handle* h, const char* who, const float* x, int B, int H, int W, int Cin, const float* w, const float* scale,
                           int Cout, int KH, int KW, int stride, int pad, ConvTrainArgs& t) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1)
        return fail(h, SPECMI_ERR_ARG, "%s: every dimension must be >= 1 (B = %d, H = %d, W = %d, Cin = %d, Cout = %d)", who, B, H, W, Cin, Cout);
    if (!conv_train_shape_ok(KH, KW, stride, pad))
        return fail(h, SPECMI_ERR_ARG, "%s: the layers built are 1x1 pad 0 and 3x3 pad 1 at stride 1 or 2 and 7x7 pad 3 at stride 2 (KH = %d, KW = %d, "
                    "stride = %d, pad = %d)", who, KH, KW, stride, pad);
    const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
    const double lim = 2147483648.0;
    if ((double)B * H * W * Cin >= lim || (double)B * OH * OW * Cout >= lim || (double)Cout * Cin * KH * KW >= lim || (double)B * H * W >= lim)
        return fail(h, SPECMI_ERR_ARG, "%s: a tensor of this layer has 2^31 elements or more", who);
    if (!x || !w || !scale) return fail(h, SPECMI_ERR_ARG, "%s: x, w or scale is NULL", who);
    t = ConvTrainArgs{x, w, scale, nullptr, B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad};
    return SPECMI_OK;
}

static bool misaligned4(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 3) return true;
    return false;
}

int specmi_conv2d_train_forward(specmi_handle* h, const float* x, int B, int H, int W, int Cin, const float* w_oihw_dev, const float* scale_dev,
                                const float* shift_dev, int Cout, int KH, int KW, int stride, int pad, const float* residual, int relu,
                                float* y, void* stream) {
    ENTER(h);
    ConvTrainArgs t;
    if (int rc = conv_train_args(h, "conv2d_train_forward", x, B, H, W, Cin, w_oihw_dev, scale_dev, Cout, KH, KW, stride, pad, t)) return rc;
    if (!shift_dev || !y) return fail(h, SPECMI_ERR_ARG, "conv2d_train_forward: shift or y is NULL");
    if (misaligned4({x, w_oihw_dev, scale_dev, shift_dev, residual, y}))
        return fail(h, SPECMI_ERR_ARG, "conv2d_train_forward: a float pointer is not 4-byte aligned");
    t.shift = shift_dev;
    if (int rc = grow_ragged(h, h->buf[BUF_conv_fwd], conv_fwd_ws_floats(t) * 4, "the convolution training workspace")) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "conv.train_forward"};
    LAUNCHCHK(h, launch_conv_train_forward(t, residual, relu != 0, y, (float*)h->buf[BUF_conv_fwd].p, ctx), "conv2d_train_forward");
    return SPECMI_OK;
}

int specmi_conv2d_backward(specmi_handle* h, const float* x, int B, int H, int W, int Cin, const float* w_oihw_dev, const float* scale_dev,
                           int Cout, int KH, int KW, int stride, int pad, const float* y, int relu, const float* g_y, const float* g_x_add,
                           float* g_x, float* g_w, float* g_res, void* stream) {
    ENTER(h);
    ConvTrainArgs t;
    if (int rc = conv_train_args(h, "conv2d_backward", x, B, H, W, Cin, w_oihw_dev, scale_dev, Cout, KH, KW, stride, pad, t)) return rc;
    if (!g_y) return fail(h, SPECMI_ERR_ARG, "conv2d_backward: g_y is NULL");
    if (relu && !y) return fail(h, SPECMI_ERR_ARG, "conv2d_backward: relu needs y (the mask is y > 0)");
    if (!g_x && !g_w && !g_res) return fail(h, SPECMI_ERR_ARG, "conv2d_backward: every output is NULL");
    if (misaligned4({x, w_oihw_dev, scale_dev, y, g_y, g_x_add, g_x, g_w, g_res}))
        return fail(h, SPECMI_ERR_ARG, "conv2d_backward: a float pointer is not 4-byte aligned");
    // the splits of the weight gradient: the rule of the shape, or what the experimental option forces (measurements)
    const int forced = opt(h, OPT_conv_wgrad_splits);
    const long rows = (long)B * t.OH;
    const int S = forced > 0 ? (int)std::min<long>({(long)forced, rows, 4096L}) : conv_wgrad_splits(B, t.OH, Cin, Cout, KH, KW);
    if (g_x || g_w)
        if (int rc = grow_ragged(h, h->buf[BUF_conv_bwd], conv_bwd_ws_floats(t, g_w ? S : 1) * 4, "the convolution backward workspace")) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "conv.backward"};
    LAUNCHCHK(h, launch_conv_backward(t, y, relu != 0, g_y, g_x ? g_x_add : nullptr, g_x, g_w, g_res, (float*)h->buf[BUF_conv_bwd].p, S, ctx),
              "conv2d_backward");
    return SPECMI_OK;
}

// the argument checks specmi_batchnorm_train_forward and specmi_batchnorm_backward share, and the kernels' argument block
static int bn_args(specmi_handle* h, const char* who, const float* z, int M, int C, const float* gamma, int relu, BnArgs& a) {
    if (M < 2) return fail(h, SPECMI_ERR_ARG, "%s: M = %d: batch statistics need more than one value per channel", who, M);
    if (C < 1) return fail(h, SPECMI_ERR_ARG, "%s: C = %d must be >= 1", who, C);
    if ((double)M * C >= 2147483648.0) return fail(h, SPECMI_ERR_ARG, "%s: the tensor has 2^31 elements or more (M = %d, C = %d)", who, M, C);
    if (!z || !gamma) return fail(h, SPECMI_ERR_ARG, "%s: z or gamma is NULL", who);
    a = BnArgs{z, gamma, M, C, relu != 0};
    return SPECMI_OK;
}

int specmi_batchnorm_train_forward(specmi_handle* h, const float* z, int M, int C, const float* gamma, const float* beta, const float* residual,
                                   int relu, float eps, float momentum, float* running_mean, float* running_var, float* y, float* mean,
                                   float* invstd, void* stream) {
    ENTER(h);
    BnArgs a;
    if (int rc = bn_args(h, "batchnorm_train_forward", z, M, C, gamma, relu, a)) return rc;
    if (!beta || !y || !mean || !invstd) return fail(h, SPECMI_ERR_ARG, "batchnorm_train_forward: beta, y, mean or invstd is NULL");
    if (!(eps >= 0.f)) return fail(h, SPECMI_ERR_ARG, "batchnorm_train_forward: eps = %g must be >= 0", (double)eps);
    if (!(momentum >= 0.f && momentum <= 1.f))
        return fail(h, SPECMI_ERR_ARG, "batchnorm_train_forward: the momentum factor %g must be in [0, 1]", (double)momentum);
    if (!running_mean != !running_var)
        return fail(h, SPECMI_ERR_ARG, "batchnorm_train_forward: running_mean and running_var are given together or not at all");
    if (misaligned4({z, gamma, beta, residual, running_mean, running_var, y, mean, invstd}))
        return fail(h, SPECMI_ERR_ARG, "batchnorm_train_forward: a float pointer is not 4-byte aligned");
    if (int rc = grow_ragged(h, h->buf[BUF_bn_train], bn_ws_floats(M, C) * 4, "the BatchNorm training workspace")) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "bn.train_forward"};
    LAUNCHCHK(h, launch_bn_train_forward(a, beta, residual, eps, momentum, running_mean, running_var, y, mean, invstd,
                                         (float*)h->buf[BUF_bn_train].p, ctx), "batchnorm_train_forward");
    return SPECMI_OK;
}

int specmi_batchnorm_backward(specmi_handle* h, const float* z, int M, int C, const float* gamma, const float* mean, const float* invstd,
                              const float* y, int relu, const float* g_y, float* g_z, float* g_gamma, float* g_beta, float* g_res,
                              void* stream) {
    ENTER(h);
    BnArgs a;
    if (int rc = bn_args(h, "batchnorm_backward", z, M, C, gamma, relu, a)) return rc;
    if (!mean || !invstd || !g_y) return fail(h, SPECMI_ERR_ARG, "batchnorm_backward: mean, invstd or g_y is NULL");
    if (relu && !y) return fail(h, SPECMI_ERR_ARG, "batchnorm_backward: relu needs y (the mask is y > 0)");
    if (!g_z && !g_gamma && !g_beta && !g_res) return fail(h, SPECMI_ERR_ARG, "batchnorm_backward: every output is NULL");
    if (misaligned4({z, gamma, mean, invstd, y, g_y, g_z, g_gamma, g_beta, g_res}))
        return fail(h, SPECMI_ERR_ARG, "batchnorm_backward: a float pointer is not 4-byte aligned");
    if (int rc = grow_ragged(h, h->buf[BUF_bn_train], bn_ws_floats(M, C) * 4, "the BatchNorm training workspace")) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "bn.backward"};
    LAUNCHCHK(h, launch_bn_backward(a, mean, invstd, y, g_y, g_z, g_gamma, g_beta, g_res, (float*)h->buf[BUF_bn_train].p, ctx),
              "batchnorm_backward");
    return SPECMI_OK;
}

// the argument checks specmi_maxpool3x3s2_train_forward and specmi_maxpool3x3s2_backward share
static int pool_train_args(specmi_handle* h, const char* who, int B, int H, int W, int C, std::initializer_list<const void*> f32,
                           const void* idx) {
    if (B < 1 || H < 1 || W < 1 || C < 1)
        return fail(h, SPECMI_ERR_ARG, "%s: every dimension must be >= 1 (B = %d, H = %d, W = %d, C = %d)", who, B, H, W, C);
    if ((double)B * H * W * C >= 2147483648.0) return fail(h, SPECMI_ERR_ARG, "%s: the input has 2^31 elements or more", who);
    for (const void* p : f32)
        if (!p) return fail(h, SPECMI_ERR_ARG, "%s: a tensor is NULL", who);
    if (!idx) return fail(h, SPECMI_ERR_ARG, "%s: idx is NULL", who);
    if (misaligned4(f32)) return fail(h, SPECMI_ERR_ARG, "%s: a float pointer is not 4-byte aligned", who);
    return SPECMI_OK;
}

int specmi_maxpool3x3s2_train_forward(specmi_handle* h, const float* x, int B, int H, int W, int C, float* y, unsigned char* idx,
                                      void* stream) {
    ENTER(h);
    if (int rc = pool_train_args(h, "maxpool3x3s2_train_forward", B, H, W, C, {x, y}, idx)) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "maxpool.train_forward"};
    LAUNCHCHK(h, launch_maxpool_train_forward(x, B, H, W, C, y, idx, ctx), "maxpool3x3s2_train_forward");
    return SPECMI_OK;
}

int specmi_maxpool3x3s2_backward(specmi_handle* h, const float* g_y, const unsigned char* idx, int B, int H, int W, int C, float* g_x,
                                 void* stream) {
    ENTER(h);
    if (int rc = pool_train_args(h, "maxpool3x3s2_backward", B, H, W, C, {g_y, g_x}, idx)) return rc;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "maxpool.backward"};
    LAUNCHCHK(h, launch_maxpool_backward(g_y, idx, B, H, W, C, g_x, ctx), "maxpool3x3s2_backward");
    return SPECMI_OK;
}

// the argument checks of specmi_camcalib_loss and its backward, and the kernels' argument block
static int cam_loss_args(specmi_handle* h, const char* who, const float* lv, const float* lp, const float* lr, int B, int nbins, int loss_type,
                         const void* tv, const void* tp, const void* tr, float wv, float wp, float wr, CamLossArgs& a) {
    if (B < 1 || B > (1 << 20)) return fail(h, SPECMI_ERR_ARG, "%s: B = %d must be in [1, 2^20]", who, B);
    if (nbins < 2 || nbins > (1 << 16)) return fail(h, SPECMI_ERR_ARG, "%s: nbins = %d must be in [2, 2^16]", who, nbins);
    if (loss_type < SPECMI_LOSS_CE || loss_type > SPECMI_LOSS_SOFTARGMAX_BIASED_L2)
        return fail(h, SPECMI_ERR_ARG, "%s: loss_type %d is not defined (camcalib/loss.py:75-85: ce, kl, softargmax_l2, softargmax_biased_l2)", who, loss_type);
    if (!lv || !lp || !lr) return fail(h, SPECMI_ERR_ARG, "%s: a logit tensor is NULL", who);
    if (!tv || !tp || !tr) return fail(h, SPECMI_ERR_ARG, "%s: a target tensor is NULL", who);
    a.logits[0] = lv; a.logits[1] = lp; a.logits[2] = lr;
    a.target[0] = tv; a.target[1] = tp; a.target[2] = tr;
    a.B = B; a.nbins = nbins; a.loss_type = loss_type;
    a.weight[0] = wv; a.weight[1] = wp; a.weight[2] = wr;
    a.loss_term = nullptr; a.means = nullptr;
    return SPECMI_OK;
}

int specmi_camcalib_loss(specmi_handle* h, const float* lv, const float* lp, const float* lr, int B, int nbins, int loss_type,
                         const void* target_vfov, const void* target_pitch, const void* target_roll, float w_vfov, float w_pitch,
                         float w_roll, float* loss_term, float* means, void* stream) {
    ENTER(h);
    CamLossArgs a;
    if (int rc = cam_loss_args(h, "camcalib_loss", lv, lp, lr, B, nbins, loss_type, target_vfov, target_pitch, target_roll, w_vfov, w_pitch, w_roll, a))
        return rc;
    if (!loss_term || !means) return fail(h, SPECMI_ERR_ARG, "camcalib_loss: loss_term or means is NULL");
    a.loss_term = loss_term; a.means = means;
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.loss"};
    LAUNCHCHK(h, launch_camcalib_loss(a, ctx), "camcalib_loss");
    return SPECMI_OK;
}

int specmi_camcalib_loss_backward(specmi_handle* h, const float* lv, const float* lp, const float* lr, int B, int nbins, int loss_type,
                                  const void* target_vfov, const void* target_pitch, const void* target_roll, float w_vfov, float w_pitch,
                                  float w_roll, const float* g_means, float* g_vfov, float* g_pitch, float* g_roll, void* stream) {
    ENTER(h);
    CamLossArgs a;
    if (int rc = cam_loss_args(h, "camcalib_loss_backward", lv, lp, lr, B, nbins, loss_type, target_vfov, target_pitch, target_roll, w_vfov,
                               w_pitch, w_roll, a))
        return rc;
    if (!g_means) return fail(h, SPECMI_ERR_ARG, "camcalib_loss_backward: g_means is NULL");
    if (!g_vfov || !g_pitch || !g_roll) return fail(h, SPECMI_ERR_ARG, "camcalib_loss_backward: a gradient output is NULL");
    float* const g[3] = {g_vfov, g_pitch, g_roll};
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "camcalib.loss_backward"};
    LAUNCHCHK(h, launch_camcalib_loss_backward(a, g_means, g, ctx), "camcalib_loss_backward");
    return SPECMI_OK;
}

int specmi_rotate_points(specmi_handle* h, const float* R, const float* points, int B, int N, float* out, void* stream) {
    ENTER(h);
    if (!R || !points || !out || B <= 0 || N <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    LaunchCtx ctx{(hipStream_t)stream, &h->prof, "eval.rotate_points"};
    LAUNCHCHK(h, launch_rotate_points(R, points, B, N, out, ctx), "rotate_points");
    return SPECMI_OK;
}

int specmi_trunk_plan(specmi_handle* h, int B, int H, int W, int pair, int32_t* mode) {
    if (!h) return SPECMI_ERR_ARG;
    if (!mode || B <= 0 || H <= 0 || W <= 0) return fail(h, SPECMI_ERR_ARG, "bad argument");
    *mode = h->hrnet ? 0 : trunk_mode(h, B, H, W, pair != 0);
    return SPECMI_OK;
}

int specmi_sync_status(specmi_handle* h, int32_t* status) {
    ENTER(h);
    if (!status) return fail(h, SPECMI_ERR_ARG, "null argument");
    HIPCHK(h, hipDeviceSynchronize());
    *status = 0;
    if (h->sk.cnt) {   // the last arriver of every sliced tile re-zeroes its counter: anything else is a protocol error
        std::vector<unsigned> v((size_t)h->sk.ncnt);
        HIPCHK(h, hipMemcpy(v.data(), h->sk.cnt, v.size() * 4, hipMemcpyDeviceToHost));
        for (unsigned c : v)
            if (c) *status = -2;
    }
    return SPECMI_OK;
}

int specmi_sync_reset(specmi_handle* h, void* stream) {
    ENTER(h);
    reset_sync_state(h, (hipStream_t)stream);
    return SPECMI_OK;
}

int specmi_debug_poison_sync(specmi_handle* h, uint32_t value) {
    ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());
    if (h->sk.cnt) {
        std::vector<unsigned> v((size_t)h->sk.ncnt, value);
        HIPCHK(h, hipMemcpy(h->sk.cnt, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    }
    return SPECMI_OK;
}

int specmi_profile_enable(specmi_handle* h, int on) {
    if (!h) return SPECMI_ERR_ARG;
    h->prof.on = on != 0;
    return SPECMI_OK;
}

int specmi_profile_read(specmi_handle* h, specmi_prof_entry* entries, int max_entries, int* n) {
    ENTER(h);
    if (!n) return fail(h, SPECMI_ERR_ARG, "n is NULL");
    std::vector<specmi_prof_entry> acc;
    for (auto& r : h->prof.log) {
        (void)hipEventSynchronize(r.e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
        specmi_prof_entry* e = nullptr;
        for (auto& a : acc)
            if (!std::strncmp(a.kernel, r.kernel, sizeof(a.kernel) - 1) && !std::strncmp(a.label, r.label.c_str(), sizeof(a.label) - 1)) {
                e = &a;
                break;
            }
        if (!e) {
            specmi_prof_entry ne;
            std::memset(&ne, 0, sizeof(ne));
            std::strncpy(ne.kernel, r.kernel, sizeof(ne.kernel) - 1);
            std::strncpy(ne.label, r.label.c_str(), sizeof(ne.label) - 1);
            acc.push_back(ne);
            e = &acc.back();
        }
        e->ms += ms; e->flops += r.flops; e->bytes += r.bytes; e->launches += 1;
    }
    h->prof.log.clear();
    *n = (int)acc.size();
    for (int i = 0; i < (int)acc.size() && i < max_entries && entries; ++i) entries[i] = acc[i];
    return SPECMI_OK;
}

}  // extern "C"
