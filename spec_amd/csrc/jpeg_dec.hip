// jpeg_dec.hip - baseline JPEG files decoded on the device into uint8 RGB rectangles of a slab: the
// read side of jpeg.hip.  What the flows get from PIL's Image.open(path).convert('RGB') for every frame they read
// (spec_amd/tester.py, spec_amd/evaluation.py, spec_amd/camcalib_eval.py), for all supported files of a call together, so that the
// files' bytes go up instead of the raw frames.
//
// THE CONTRACT.  For a supported file the (H, W, 3) picture equals np.array(Image.open(f).convert('RGB')) on a libjpeg-turbo
// build of Pillow, element for element (tests/jpeg_dec_ref.py restates it in NumPy).  The rules are libjpeg's:
// 1. Supported files.  One SOF0 with 8-bit samples; three components, YCbCr; sampling 2x2,1x1,1x1 (4:2:0) or 1x1,1x1,1x1
//    (4:4:4); one interleaved scan (Ss 0, Se 63, Ah/Al 0); 8-bit quantisation tables; any Huffman tables from the file's own DHT
//    segments (table ids 0 and 1); no DRI with a non-zero interval; H and W in 1 .. 32768; no Adobe APP14 segment and not the
//    component ids 'R', 'G', 'B' without JFIF; the file ends with EOI.  Everything else is refused by jpeg_probe on the host.
//    The probe reads the markers up to the first SOS and the file's last two bytes; it does not look inside the scan.  What only
//    the scan shows - a second scan, a DHT or DRI between scans, any marker before the final EOI - is found by the write kernel
//    and sets the status (rule 2), so such a file is launched and then takes the host route like a damaged one.
// 2. Entropy decode (T.81 F.2.2).  Bits MSB first; the byte behind a 0xFF data byte is stuffing and is skipped.  Blocks in the
//    MCU's order (Y00 Y01 Y10 Y11 Cb Cr, or Y Cb Cr).  DC: category code plus value bits, predicted per component.  AC: (run, size)
//    codes, 0xF0 = 16 zeros, 0x00 = end of block.  The scan must end with every MCU decoded, fewer than 8 fill bits, and EOI next.
//    A file's status word is non-zero after: an invalid code (also a 0xFF inside the scan that is not followed by 0x00, or an
//    (r, 0) symbol other than these two); a zigzag index beyond 63; a DC category above 11 or an AC size above 10;
//    |coefficient x quantiser| above 32767; the scan ending early, or bits left over.  Its pixels are then unspecified.
// 3. Dequantise and IDCT.  libjpeg's jidctint ("islow"): CONST_BITS 13, PASS1_BITS 2; columns first with DESCALE(x, 11), then
//    rows with DESCALE(x, 18); DESCALE(x, n) = (x + (1 << (n - 1))) >> n, arithmetic shift; the constants 2446, 3196, 4433, 6270,
//    7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172; sample = clamp(x + 128, 0, 255).
// 4. Real plane size.  At 4:2:0 the real part of a chroma plane is ceil(H / 2) x ceil(W / 2); samples beyond it are never read.
// 5. Chroma upsampling at 4:2:0 (h2v2_fancy_upsample).  For output row 2 r + v the neighbour row is r - 1 (v = 0) or r + 1
//    (v = 1), clamped to the real plane.  s[c] = 3 p[r][c] + p[nb][c].  Even column 2 c: (3 s[c] + s[c - 1] + 8) >> 4, odd column
//    2 c + 1: (3 s[c] + s[c + 1] + 7) >> 4; the first column (4 s[0] + 8) >> 4, the last odd column (4 s[last] + 7) >> 4.
// 5b. Narrow planes.  With ceil(W / 2) <= 2 every chroma sample is replicated 2 x 2 instead.
// 6. Colour (jdcolor.c).  F(x) = int(x 65536 + 0.5), cb and cr minus 128:  R = Y + ((F(1.402) cr + 32768) >> 16),
//    G = Y + ((-F(0.34414) cb + 32768 - F(0.71414) cr) >> 16),  B = Y + ((F(1.772) cb + 32768) >> 16), each clamped to 0 .. 255.
//
// STAGES.  A file's scan is cut into SUBSEQUENCES of 1024 bits = 128 bytes of the file; one lane decodes every symbol that
// STARTS in its subsequence.  A lane's state between symbols is (bits of the left neighbour's last symbol that reach into the
// subsequence, block of the MCU, zigzag position); positions count DATA bits, so a boundary between a 0xFF and its stuffed zero
// needs no special case.  Workgroups own 256 consecutive subsequences of one file and find it by bisecting the group prefix of
// the record table, as the other ragged kernels do.
//   sync    one lane per subsequence, writes no coefficient: decodes from its left neighbour's exit state (an invalid exit is a
//           cold start, never copied on) and records its own exit state and the blocks it completed.  A workgroup settles its 256
//           lanes in LDS - rounds separated by barriers until none changes, at most 257 -, and takes its first lane's entry from
//           what the PREVIOUS launch left.  The host repeats the launch until the one "changed" word it reads back is zero, at
//           most as often as the largest file has groups: after launch k the first k groups of every file are exact, by induction.
//           No workgroup waits for another, nothing is polled, every loop has a bound known at launch.
//   scan    one workgroup per file: exclusive scan of the lanes' block counts -> each lane's first block; a total that is not the
//           file's block count sets the status
//   write   the same decode from the settled entry states into the zeroed int16 coefficients: non-zeros only, natural order
//           within a block, MCU order between blocks, DC as the difference; the anomalies of rule 2 set the status
//   dc      one workgroup per file and component: inclusive scan of the DC differences in scan order
//   idct    one thread per block: rule 3 into 8-bit planes
//   colour  one thread per pixel: rules 4 to 6 into the file's rectangle at its pitch
// Every read of a file stays inside its scan's byte range, every write inside its rectangle or its share of the workspace.
// WORKSPACE, one per handle, grown under the rule of the ragged calls: per MCU of 16 x 16 pixels (4:2:0) 768 bytes of coefficients
// and 384 of planes, i.e. 4.5 bytes per pixel of the pictures rounded up to whole MCUs (9 at 4:4:4), plus 16 bytes per subsequence
// and 8 per group.
#include "specmi_internal.h"

namespace specmi {

namespace {

constexpr unsigned char kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__constant__ unsigned char kNaturalDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// status bits
enum { ST_CODE = 1, ST_ZIGZAG = 2, ST_SIZE = 4, ST_RANGE = 8, ST_EARLY = 16, ST_LEFTOVER = 32, ST_BLOCKS = 64, ST_MARKER = 128 };

// ---- host half: rule 1 ------------------------------------------------------------------------------------------------------------
// Annex C: canonical codes from BITS and HUFFVAL -> the look-ahead table and the lists for longer codes; false: not a code
bool build_huff(const unsigned char* bits, const unsigned char* vals, int nvals, JdecHuff* t) {
    std::memset(t, 0, sizeof(*t));
    std::memcpy(t->vals, vals, (size_t)nvals);
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->maxcode[l] = -1;
        t->valoff[l] = k - (int)code;
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            if (code >= (1u << l) || k >= nvals) return false;
            if (l <= 8)
                for (unsigned j = 0; j < (1u << (8 - l)); ++j) t->lut[(code << (8 - l)) + j] = (unsigned short)(l << 8 | vals[k]);
            t->maxcode[l] = (int)code;
        }
        code <<= 1;
    }
    t->maxcode[0] = t->maxcode[17] = -1;
    return true;
}

}  // namespace

int jpeg_probe(const unsigned char* d, size_t n, JdecFile* f) {
    std::memset(f, 0, sizeof(*f));
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return JDEC_NOT_JPEG;
    size_t at = 2;
    unsigned short qt[4][64];
    JdecHuff huff[4];
    bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
    bool jfif = false, adobe = false, progressive = false, other_sof = false, wide_q = false;
    const unsigned char* sof = nullptr;
    size_t sof_len = 0;
    int restart = 0;
    const unsigned char* sos = nullptr;
    size_t sos_len = 0;
    for (;;) {
        if (at + 4 > n) return JDEC_TRUNCATED;
        if (d[at] != 0xFF) return JDEC_NOT_JPEG;
        const int m = d[at + 1];
        if (m == 0xFF) { ++at; continue; }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { at += 2; continue; }
        if (m == 0xD9) return JDEC_TRUNCATED;
        const size_t len = (size_t)d[at + 2] << 8 | d[at + 3];
        if (len < 2 || at + 2 + len > n) return JDEC_TRUNCATED;
        const unsigned char* body = d + at + 4;
        const size_t bn = len - 2;
        at += 2 + len;
        if (m == 0xE0 && bn >= 5 && !std::memcmp(body, "JFIF\0", 5)) {
            jfif = true;
        } else if (m == 0xEE && bn >= 5 && !std::memcmp(body, "Adobe", 5)) {
            adobe = true;
        } else if (m == 0xDB) {
            for (size_t k = 0; k < bn;) {
                const int pq = body[k] >> 4, tq = body[k] & 15;
                if (pq) { wide_q = true; k += 129; continue; }
                if (tq > 3 || k + 65 > bn) return JDEC_TABLES;
                for (int i = 0; i < 64; ++i) qt[tq][kNatural[i]] = body[k + 1 + i];
                have_q[tq] = true;
                k += 65;
            }
        } else if (m == 0xC4) {
            for (size_t k = 0; k < bn;) {
                if (k + 17 > bn) return JDEC_TABLES;
                const int tc = body[k] >> 4, th = body[k] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += body[k + 1 + i];
                if (tc > 1 || th > 1 || cnt > 256 || k + 17 + (size_t)cnt > bn) return JDEC_TABLES;
                if (!build_huff(body + k + 1, body + k + 17, cnt, &huff[2 * tc + th])) return JDEC_TABLES;
                have_h[2 * tc + th] = true;
                k += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            restart = bn >= 2 ? (body[0] << 8 | body[1]) : 1;
        } else if (m == 0xC2) {
            progressive = true;
            if (!sof) { sof = body; sof_len = bn; }
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (m != 0xC0 || sof) other_sof = true;
            sof = body; sof_len = bn;
        } else if (m == 0xDA) {
            sos = body; sos_len = bn;
            break;
        }
    }
    if (!sof || sof_len < 6) return JDEC_TRUNCATED;
    if (progressive) return JDEC_PROGRESSIVE;
    if (other_sof) return JDEC_SOF;
    if (sof[0] != 8 || wide_q) return JDEC_PRECISION;
    const int H = sof[1] << 8 | sof[2], W = sof[3] << 8 | sof[4], nc = sof[5];
    if (nc != 3 || sof_len < 6 + 9) return JDEC_COMPONENTS;
    const unsigned char* c = sof + 6;       // id, sampling, quantiser per component
    const bool s420 = c[1] == 0x22;
    if ((c[1] != 0x22 && c[1] != 0x11) || c[4] != 0x11 || c[7] != 0x11) return JDEC_SAMPLING;
    if (restart) return JDEC_RESTART;
    if (H < 1 || H > 32768 || W < 1 || W > 32768) return JDEC_SIZE;
    if (adobe || (!jfif && c[0] == 'R' && c[3] == 'G' && c[6] == 'B')) return JDEC_COLOURSPACE;
    if (sos_len != 10 || sos[0] != 3 || sos[1] != c[0] || sos[3] != c[3] || sos[5] != c[6] || sos[7] != 0 || sos[8] != 63 || sos[9] != 0)
        return JDEC_SCAN;
    for (int i = 0; i < 3; ++i) {
        const int td = sos[2 + 2 * i] >> 4, ta = sos[2 + 2 * i] & 15, tq = c[3 * i + 2];
        if (tq > 3 || !have_q[tq] || td > 1 || ta > 1 || !have_h[td] || !have_h[2 + ta]) return JDEC_TABLES;
        std::memcpy(f->q[i], qt[tq], sizeof(qt[tq]));
        f->tdc[i] = (unsigned char)td;
        f->tac[i] = (unsigned char)(2 + ta);
    }
    for (int i = 0; i < 4; ++i)
        if (have_h[i]) f->huff[i] = huff[i];
    if (n - at < 2 || d[n - 2] != 0xFF || d[n - 1] != 0xD9) {       // the EOI is not the end: is there one further in (bytes behind it)?
        for (size_t k = n; k >= at + 2; --k)
            if (d[k - 2] == 0xFF && d[k - 1] == 0xD9) return JDEC_TRAILING;
        return JDEC_TRUNCATED;
    }
    f->H = H; f->W = W; f->s420 = s420 ? 1 : 0; f->bpm = s420 ? 6 : 3;
    f->mx = s420 ? (W + 15) / 16 : (W + 7) / 8;
    f->my = s420 ? (H + 15) / 16 : (H + 7) / 8;
    f->scan_off = (long long)at; f->scan_len = (long long)(n - 2 - at);
    return JDEC_SUPPORTED;
}

// ---- device half ------------------------------------------------------------------------------------------------------------------
namespace {

constexpr unsigned kInvalid = 0u, kNever = 0xFFFFFFFFu, kStart = 1u << 31;      // a state: valid << 31 | zigzag << 16 | block << 8 | overflow

// the file's tables in LDS
struct JdecLds {
    JdecHuff huff[4];
    unsigned char tsel[8];
};

__device__ __forceinline__ void load_tables(JdecLds& s, const JdecFile* f) {
    const int* src = reinterpret_cast<const int*>(f->huff);
    int* dst = reinterpret_cast<int*>(s.huff);
    for (int i = threadIdx.x; i < (int)(sizeof(s.huff) / 4); i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x < 4) { s.tsel[threadIdx.x] = f->tdc[threadIdx.x]; s.tsel[4 + threadIdx.x] = f->tac[threadIdx.x]; }
    __syncthreads();
}

// Subsequence `lane` of file f from the entry state: every symbol that starts in it (rule 2).  -> the exit state (kInvalid after
// an anomaly or at the scan's end) and the blocks completed.  WRITE: the coefficients of the blocks from `blk` on are stored and
// the anomalies returned as status bits.  At most 1024 symbols start in a subsequence (each takes a bit or more).
template <bool WRITE>
__device__ __forceinline__ unsigned decode_lane(const JdecFile* f, const unsigned char* p, const JdecLds& s, int lane, unsigned entry, int blk,
                                                short* coef, int* count, int* status) {
    const long long end = f->scan_len;
    const long long range_end = (long long)(lane + 1) * kJdecSubBytes;
    long long next = (long long)lane * kJdecSubBytes;
    if (lane > 0 && p[next - 1] == 0xFF) ++next;          // the subsequence begins with the stuffed zero of the byte before it
    unsigned long long acc = 0;
    int nbits = 0, consumed = 0, budget = 0;
    int b = (int)(entry >> 8) & 0xFF, z = (int)(entry >> 16) & 0xFF, done = 0, st = 0;
    const int bpm = f->bpm, nblocks = f->nblocks, s420 = f->s420;
    const bool last = lane == f->nsub - 1;
    bool valid = true;
    int skip = (int)(entry & 0xFF);
#pragma unroll 1
    for (int it = 0; it < 8 * kJdecSubBytes + 2; ++it) {
        while (nbits <= 56 && next < end) {
            const unsigned v = p[next];
            if (next < range_end) budget += 8;
            next += v == 0xFF ? 2 : 1;
            acc = acc << 8 | v;
            nbits += 8;
        }
        if (skip) {                                       // the left neighbour's last symbol reaches this far
            if (skip > nbits) { valid = false; break; }
            nbits -= skip; consumed += skip; skip = 0;
            continue;
        }
        if (consumed >= budget) break;
        if (WRITE && blk >= nblocks) {                    // every block is there: fewer than 8 fill bits may remain
            if (!(last && next >= end && nbits < 8)) st |= ST_LEFTOVER;
            valid = false;
            break;
        }
        const unsigned code = nbits >= 16 ? (unsigned)(acc >> (nbits - 16)) & 0xFFFFu : (unsigned)(acc << (16 - nbits)) & 0xFFFFu;
        const int comp = s420 ? (b < 4 ? 0 : b - 3) : b;
        const JdecHuff& t = s.huff[s.tsel[(z ? 4 : 0) + comp]];
        const unsigned e = t.lut[code >> 8];
        int len = (int)(e >> 8), sym = (int)(e & 255);
        if (!len) {
#pragma unroll 1
            for (int l = 9; l <= 16; ++l) {
                const int cl = (int)(code >> (16 - l));
                if (cl <= t.maxcode[l]) {
                    sym = t.vals[(t.valoff[l] + cl) & 255];
                    len = l;
                    break;
                }
            }
        }
        if (!len) { st |= (next >= end && nbits < 16) ? ST_EARLY : ST_CODE; valid = false; break; }
        const int r = z ? sym >> 4 : 0, sz = z ? sym & 15 : sym;
        if (sz > (z ? 10 : 11)) { st |= ST_SIZE; valid = false; break; }
        if (len + sz > nbits) { st |= ST_EARLY; valid = false; break; }
        nbits -= len;
        int v = 0;
        if (sz) {
            v = (int)((acc >> (nbits - sz)) & ((1u << sz) - 1u));
            if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
            nbits -= sz;
        }
        consumed += len + sz;
        if (z == 0) {
            if (WRITE && v) coef[(long long)blk * 64] = (short)v;
            z = 1;
        } else if (sz == 0) {
            if (r == 15) {
                z += 16;
                if (z > 64) { st |= ST_ZIGZAG; valid = false; break; }
            } else if (r == 0) {
                z = 64;
            } else {
                st |= ST_CODE; valid = false; break;
            }
        } else {
            z += r;
            if (z > 63) { st |= ST_ZIGZAG; valid = false; break; }
            if (WRITE) coef[(long long)blk * 64 + kNaturalDev[z]] = (short)v;
            ++z;
        }
        if (z == 64) {
            z = 0;
            b = b + 1 == bpm ? 0 : b + 1;
            ++done;
            ++blk;
        }
    }
    *count = done;
    if (WRITE) *status = st;
    if (!valid || consumed < budget) return kInvalid;
    return kStart | (unsigned)z << 16 | (unsigned)b << 8 | (unsigned)(consumed - budget);
}

__global__ void __launch_bounds__(kJdecGroup) jdec_sync_kernel(JdecArgs a, int pass) {
    __shared__ JdecLds s;
    __shared__ unsigned sexit[kJdecGroup];
    const JdecFile* f = a.files + last_at_or_before(a.files, a.n, blockIdx.x, &JdecFile::group0);
    load_tables(s, f);
    const int tid = threadIdx.x, g = (int)blockIdx.x - f->group0, lane = g * kJdecGroup + tid;
    const bool live = lane < f->nsub;
    const int gl = f->lane0 + lane;
    unsigned entry = live ? a.entry[gl] : kNever, ex = live ? a.exits[gl] : kInvalid;
    int cnt = live ? a.count[gl] : 0;
    const unsigned gin = g > 0 ? a.gexit[(size_t)(pass & 1) * a.groups + blockIdx.x - 1] : kStart;
    const unsigned char* p = a.in + f->scan_off;
    bool any = false;
#pragma unroll 1
    for (int round = 0; round <= kJdecGroup; ++round) {
        sexit[tid] = ex;
        __syncthreads();
        unsigned e = tid == 0 ? gin : sexit[tid - 1];
        if (e == kInvalid) e = kStart;                  // an invalid exit is a cold start for the right neighbour
        int moved = 0;
        if (live && e != entry) {
            entry = e;
            ex = decode_lane<false>(f, p, s, lane, e, 0, nullptr, &cnt, nullptr);
            moved = 1;
        }
        if (!__syncthreads_or(moved)) break;
        any = true;
    }
    if (live) { a.entry[gl] = entry; a.exits[gl] = ex; a.count[gl] = cnt; }
    if (tid == kJdecGroup - 1) a.gexit[(size_t)((pass + 1) & 1) * a.groups + blockIdx.x] = ex;
    if (tid == 0 && any) atomicOr(a.changed, 1u);
}

// one workgroup per file: exclusive scan of the lanes' block counts
__global__ void __launch_bounds__(256) jdec_scan_kernel(JdecArgs a) {
    __shared__ long long lds[256];
    const JdecFile* f = a.files + blockIdx.x;
    const int tid = threadIdx.x;
    long long running = 0;
    for (int c = 0; c < f->nsub; c += 256) {            // uniform trip count
        const int i = c + tid;
        const long long v = i < f->nsub ? a.count[f->lane0 + i] : 0;
        lds[tid] = v;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < 256; d <<= 1) {
            const long long add = tid >= d ? lds[tid - d] : 0;
            __syncthreads();
            lds[tid] += add;
            __syncthreads();
        }
        const long long excl = running + lds[tid] - v;
        if (i < f->nsub) a.first[f->lane0 + i] = (int)(excl < f->nblocks ? excl : f->nblocks);
        running += lds[255];
        __syncthreads();
    }
    if (tid == 0 && running != f->nblocks) atomicOr(a.status + blockIdx.x, (int)ST_BLOCKS);
}

__global__ void __launch_bounds__(kJdecGroup) jdec_write_kernel(JdecArgs a) {
    __shared__ JdecLds s;
    const JdecFile* f = a.files + last_at_or_before(a.files, a.n, blockIdx.x, &JdecFile::group0);
    load_tables(s, f);
    const int lane = ((int)blockIdx.x - f->group0) * kJdecGroup + (int)threadIdx.x;
    if (lane >= f->nsub) return;
    const int gl = f->lane0 + lane;
    unsigned e = lane == 0 ? kStart : a.exits[gl - 1];
    if (e == kInvalid) e = kStart;
    const unsigned char* p = a.in + f->scan_off;
    int cnt, st = 0, marker = 0;
    decode_lane<true>(f, p, s, lane, e, a.first[gl], a.coef + f->block0 * 64, &cnt, &st);
    const long long k1 = min((long long)(lane + 1) * kJdecSubBytes, f->scan_len);
    for (long long k = (long long)lane * kJdecSubBytes; k < k1; ++k)        // a 0xFF inside the scan is followed by its stuffed zero
        if (p[k] == 0xFF && (k + 1 >= f->scan_len || p[k + 1] != 0)) marker = ST_MARKER;
    if (st | marker) atomicOr(a.status + (f - a.files), st | marker);
}

// where block e of component c's scan order lies among the file's blocks
__device__ __forceinline__ long long comp_block(int s420, int c, long long e) {
    if (!s420) return e * 3 + c;
    return c == 0 ? (e >> 2) * 6 + (e & 3) : e * 6 + 3 + c;
}

// one workgroup per file and component: inclusive scan of the DC differences
__global__ void __launch_bounds__(256) jdec_dc_kernel(JdecArgs a) {
    __shared__ int lds[256];
    const JdecFile* f = a.files + blockIdx.x / 3;
    const int c = blockIdx.x % 3, tid = threadIdx.x;
    const long long mcus = (long long)f->mx * f->my, E = f->s420 && c == 0 ? 4 * mcus : mcus;
    short* coef = a.coef + f->block0 * 64;
    int running = 0, bad = 0;
    for (long long e0 = 0; e0 < E; e0 += 256) {         // uniform trip count
        const long long e = e0 + tid;
        const long long at = comp_block(f->s420, c, e < E ? e : 0) * 64;
        const int v = e < E ? coef[at] : 0;
        lds[tid] = v;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < 256; d <<= 1) {
            const int add = tid >= d ? lds[tid - d] : 0;
            __syncthreads();
            lds[tid] += add;
            __syncthreads();
        }
        const int dc = running + lds[tid];
        if (e < E) {
            if (dc < -32768 || dc > 32767) bad = 1;
            coef[at] = (short)dc;
        }
        running += lds[255];
        __syncthreads();
    }
    if (bad) atomicOr(a.status + blockIdx.x / 3, (int)ST_RANGE);
}

__device__ __forceinline__ int descale(long long x, int n) { return (int)((x + (1ll << (n - 1))) >> n); }

// one pass of jidctint over eight values.  The sums are 64-bit, as libjpeg's JLONG is where it matters: dequantised values up to
// 32767 in magnitude pass rule 2, and several of them in one column take the odd part beyond 2^31.  The values between the passes
// fit 32 bits (at most 8 x 32767 x 3.1 x 4 after the first pass, less after the second).
template <int N> __device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    using L = long long;
    L z1 = ((L)d2 + d6) * 4433;
    L t2 = z1 + (L)d6 * -15137, t3 = z1 + (L)d2 * 6270;
    L t0 = ((L)d0 + d4) * 8192, t1 = ((L)d0 - d4) * 8192;
    const L t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d7; t1 = d5; t2 = d3; t3 = d1;
    z1 = t0 + t3;
    L z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const L z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    d0 = descale(t10 + t3, N); d7 = descale(t10 - t3, N);
    d1 = descale(t11 + t2, N); d6 = descale(t11 - t2, N);
    d2 = descale(t12 + t1, N); d5 = descale(t12 - t1, N);
    d3 = descale(t13 + t0, N); d4 = descale(t13 - t0, N);
}

// where the planes of a file lie: Y of (ph, pw), then Cb and Cr of (ch, cw), all in whole MCUs
__device__ __forceinline__ void plane_geom(const JdecFile* f, int* pw, int* cw, long long* ysize, long long* csize) {
    *cw = 8 * f->mx;
    *pw = f->s420 ? 16 * f->mx : 8 * f->mx;
    *csize = 64ll * f->mx * f->my;
    *ysize = f->s420 ? 4 * *csize : *csize;
}

__global__ void __launch_bounds__(256) jdec_idct_kernel(JdecArgs a) {
    const JdecFile* f = a.files + last_at_or_before(a.files, a.n, blockIdx.x, &JdecFile::bchunk0);
    const int B = ((int)blockIdx.x - f->bchunk0) * 256 + (int)threadIdx.x;
    if (B >= f->nblocks) return;
    const int m = B / f->bpm, b = B - m * f->bpm;
    const int comp = f->s420 ? (b < 4 ? 0 : b - 3) : b;
    const int mcy = m / f->mx, mcx = m - mcy * f->mx;
    const uint4* src = reinterpret_cast<const uint4*>(a.coef + (f->block0 + B) * 64);
    const unsigned short* q = f->q[comp];
    int v[64];
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 w = src[i];
        const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(short)(j & 1 ? ws[j >> 1] >> 16 : ws[j >> 1] & 0xffffu);
            const int d = c * (int)q[8 * i + j];
            bad |= (d > 32767 || d < -32767) ? 1 : 0;
            v[8 * i + j] = d;
        }
    }
    if (bad) atomicOr(a.status + (f - a.files), (int)ST_RANGE);
#pragma unroll
    for (int c = 0; c < 8; ++c) idct8<11>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
    for (int r = 0; r < 8; ++r) idct8<18>(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7]);
    int pw, cw;
    long long ysize, csize;
    plane_geom(f, &pw, &cw, &ysize, &csize);
    unsigned char* plane = a.planes + f->plane0;
    int width, bx, by;
    if (comp == 0) {
        width = pw;
        bx = f->s420 ? 2 * mcx + (b & 1) : mcx;
        by = f->s420 ? 2 * mcy + (b >> 1) : mcy;
    } else {
        plane += ysize + (comp == 2 ? csize : 0);
        width = cw; bx = mcx; by = mcy;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        unsigned w[2] = {0, 0};
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c >> 2] |= (unsigned)min(max(v[8 * r + c] + 128, 0), 255) << (8 * (c & 3));
        *reinterpret_cast<uint2*>(plane + (long long)(8 * by + r) * width + 8 * bx) = make_uint2(w[0], w[1]);
    }
}

// rules 4, 5 and 5b: the chroma sample of pixel (y, x) from the plane p of row length cw
__device__ __forceinline__ int fancy(const unsigned char* p, int cw, int Hc, int Wc, int y, int x) {
    const int r = y >> 1, c = x >> 1;
    const unsigned char* row = p + (long long)r * cw;
    if (Wc <= 2) return row[c];
    const int nbr = (y & 1) ? min(r + 1, Hc - 1) : max(r - 1, 0);
    const unsigned char* nb = p + (long long)nbr * cw;
    const int s = 3 * row[c] + nb[c];
    if (x & 1) {
        if (c == Wc - 1) return (4 * s + 7) >> 4;
        return (3 * s + 3 * row[c + 1] + nb[c + 1] + 7) >> 4;
    }
    if (c == 0) return (4 * s + 8) >> 4;
    return (3 * s + 3 * row[c - 1] + nb[c - 1] + 8) >> 4;
}

__global__ void __launch_bounds__(256) jdec_colour_kernel(JdecArgs a) {
    const JdecFile* f = a.files + last_at_or_before(a.files, a.n, blockIdx.x, &JdecFile::pchunk0);
    const long long i = (long long)((int)blockIdx.x - f->pchunk0) * 256 + threadIdx.x;
    const int H = f->H, W = f->W;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    int pw, cw;
    long long ysize, csize;
    plane_geom(f, &pw, &cw, &ysize, &csize);
    const unsigned char* plane = a.planes + f->plane0;
    const int Y = plane[(long long)y * pw + x];
    int cb, cr;
    if (f->s420) {
        const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
        cb = fancy(plane + ysize, cw, Hc, Wc, y, x);
        cr = fancy(plane + ysize + csize, cw, Hc, Wc, y, x);
    } else {
        cb = plane[ysize + (long long)y * cw + x];
        cr = plane[ysize + csize + (long long)y * cw + x];
    }
    cb -= 128; cr -= 128;
    const int R = Y + ((fix16(1.402) * cr + 32768) >> 16);
    const int G = Y + ((-fix16(0.34414) * cb + 32768 - fix16(0.71414) * cr) >> 16);
    const int Bl = Y + ((fix16(1.772) * cb + 32768) >> 16);
    unsigned char* o = a.out + f->out_off + (long long)y * f->pitch + 3ll * x;
    o[0] = (unsigned char)min(max(R, 0), 255);
    o[1] = (unsigned char)min(max(G, 0), 255);
    o[2] = (unsigned char)min(max(Bl, 0), 255);
}

}  // namespace

size_t jdec_ws_layout(long long blocks, long long plane_bytes, long long lanes, long long groups, size_t off[8]) {
    const size_t sizes[8] = {(size_t)blocks * 128, (size_t)plane_bytes, (size_t)lanes * 4, (size_t)lanes * 4, (size_t)lanes * 4,
                             (size_t)lanes * 4, (size_t)groups * 8, 4};
    size_t at = 0;
    for (int i = 0; i < 8; ++i) {
        off[i] = at;
        at += (sizes[i] + 255) & ~(size_t)255;
    }
    return at;
}

int launch_jpeg_decode(const JdecArgs& a, long long blocks, long long lanes, int max_groups, double in_bytes, double out_bytes, int* passes,
                       const LaunchCtx& ctx) {
    const double coef = (double)blocks * 128;
    {
        ProfScope ps(ctx, "jdec_zero", 0.0, coef);
        if (hipError_t e = hipMemsetAsync(a.status, 0, (size_t)a.n * 4, ctx.stream)) return (int)e;
        if (hipError_t e = hipMemsetAsync(a.coef, 0, (size_t)blocks * 128, ctx.stream)) return (int)e;
        if (hipError_t e = hipMemsetAsync(a.entry, 0xFF, (size_t)lanes * 4, ctx.stream)) return (int)e;
        // exits, count, first, gexit and changed follow each other (jdec_ws_layout)
        if (hipError_t e = hipMemsetAsync(a.exits, 0, (size_t)((char*)a.changed + 4 - (char*)a.exits), ctx.stream)) return (int)e;
    }
    int p = 0;
    while (p < max_groups) {
        ProfScope ps(ctx, "jdec_sync", 0.0, in_bytes);
        if (p > 0)
            if (hipError_t e = hipMemsetAsync(a.changed, 0, 4, ctx.stream)) return (int)e;
        hipLaunchKernelGGL(jdec_sync_kernel, dim3((unsigned)a.groups), dim3(kJdecGroup), 0, ctx.stream, a, p);
        ++p;
        if (p >= max_groups) break;
        unsigned changed = 0;
        if (hipError_t e = hipMemcpyAsync(&changed, a.changed, 4, hipMemcpyDeviceToHost, ctx.stream)) return (int)e;
        if (hipError_t e = hipStreamSynchronize(ctx.stream)) return (int)e;
        if (!changed) break;
    }
    *passes = p;
    {
        ProfScope ps(ctx, "jdec_scan", 0.0, (double)lanes * 8);
        hipLaunchKernelGGL(jdec_scan_kernel, dim3((unsigned)a.n), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jdec_write", 0.0, in_bytes);
        hipLaunchKernelGGL(jdec_write_kernel, dim3((unsigned)a.groups), dim3(kJdecGroup), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jdec_dc", 0.0, 0.0);
        hipLaunchKernelGGL(jdec_dc_kernel, dim3((unsigned)a.n * 3), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jdec_idct", 0.0, coef);
        hipLaunchKernelGGL(jdec_idct_kernel, dim3((unsigned)a.bchunks), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jdec_colour", 0.0, out_bytes);
        hipLaunchKernelGGL(jdec_colour_kernel, dim3((unsigned)a.pchunks), dim3(256), 0, ctx.stream, a);
    }
    return (int)hipGetLastError();
}

}  // namespace specmi
