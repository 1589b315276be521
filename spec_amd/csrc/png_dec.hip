// png_dec.hip - PNG files decoded on the device into uint8 RGB rectangles of a slab: the read side
// of png.hip.  What the flows get from PIL's Image.open(path).convert('RGB') for every .png frame they read (spec_amd/tester.py,
// spec_amd/evaluation.py, spec_amd/camcalib_eval.py), for all supported files of a call together.
//
// THE CONTRACT.  For a supported file the (H, W, 3) picture equals np.array(Image.open(f).convert('RGB')), element for element
// (tests/png_dec_ref.py restates every stage in NumPy).  PNG is lossless: there is no arithmetic, only routes.
// 1. Supported files (png_probe, host only).  The 8 signature bytes; IHDR first; at least one IDAT, all IDATs consecutive; IEND
//    last and nothing behind it; every chunk's CRC-32 correct; bit depth 8; colour type 0, 2, 4 or 6 (grey is replicated, alpha
//    dropped, tRNS / gAMA / sRGB ignored, as convert('RGB') does); compression 0, filter 0, interlace 0; H and W in 1 .. 32768; no
//    acTL; no unknown critical chunk.  The probe also returns the IDAT payload ranges: the caller joins them, so that the device
//    sees the zlib stream contiguous.
// 2. The stream (RFC 1950 / 1951).  zlib header: CM 8, CINFO <= 7, FCHECK valid, no FDICT.  Stored, fixed and dynamic blocks.  The
//    inflated length is exactly H (1 + W bpp) and the final block is reached exactly there; the Adler-32 behind the last block
//    matches; every filter byte is in 0 .. 4.  A file's STATUS WORD is non-zero after:
//      1     ST_ZLIB      a bad zlib header
//      2     ST_BTYPE     block type 3
//      4     ST_STORED    a stored block whose LEN and NLEN disagree
//      8     ST_LENS      code lengths that over-subscribe, or are incomplete (other than a single distance code of one bit or no
//                         distance code at all), or more than 286 literal/length or 30 distance codes
//      16    ST_REPEAT    a repeat code with no previous length, or one running past HLIT + HDIST
//      32    ST_NOEOB     no end-of-block code
//      64    ST_CODE      an invalid code
//      128   ST_SYMBOL    length symbol 286 or 287, or distance symbol 30 or 31
//      256   ST_FAR       a distance beyond the bytes produced so far, or beyond 1 << (CINFO + 8)
//      512   ST_EARLY     the stream ending early
//      1024  ST_LENGTH    output longer or shorter than H (1 + W bpp)
//      2048  ST_LEFTOVER  bytes left between the final block and the Adler word
//      4096  ST_ADLER     an Adler-32 mismatch
//      8192  ST_FILTER    a filter byte above 4
//    Its pixels are then unspecified and the caller decodes it with Pillow.
// 3. Unfilter (PNG 1.2 section 6): None, Sub, Up, Average (floor), Paeth (ties: left, above, upper left), per byte against the
//    byte bpp before it; the first row reads zeros above.  Every channel is filtered by itself, so the alpha channel, which the
//    picture drops, is never reconstructed.
//
// STAGES.
//   inflate   one workgroup of kPdecLanes = 256 per file walks the file's blocks in order.  A block header is parsed by one lane
//             (the <= 320 code lengths are serial) and the canonical tables - a look-ahead table of 10 (distances: 8) bits and
//             first-code / count lists for longer codes - are filled by all.  A dynamic or fixed block is decoded in WINDOWS of
//             256 SUBSEQUENCES of kPdecSubBits = 512 bits, staged in LDS: a lane decodes every symbol that STARTS in its
//             subsequence - a literal, the end-of-block code, or a whole (length, extra, distance, extra) group -, so its state
//             between symbols is a bit position.  Lanes settle as jpeg_dec.hip's sync stage does: lane t's entry is lane t - 1's
//             exit, rounds separated by barriers until none changes, at most 257; lane 0's entry is exact, so k rounds make k lanes
//             exact.  A lane that meets the end-of-block code or an anomaly stops there; the first such lane ends the window and
//             the lanes behind it are dropped.  An exclusive scan of the lanes' byte and match counts places them; the write pass
//             stores literals and appends (destination, length, distance) records; one wavefront then resolves the records in
//             stream order, 64 at a time: the longest prefix of records whose sources lie wholly before the first one's
//             destination is copied concurrently, a lane each (one record alone: 64 bytes per step).  A match with distance <
//             length is the distance's bytes repeated, so no copy ever reads what it writes.  Stored blocks are a cooperative copy.
//   adler     a workgroup per 32 KiB chunk of the inflated streams -> two sums; a workgroup per file joins them and compares.
//   unfilter  one wavefront per file, strips of 64 rows in order: lane k works on row r0 + k one pixel behind lane k - 1, takes
//             the pixel above through a lane shuffle and keeps the previous one as upper left; lane 0 reads row r0 - 1 from the
//             finished output.  Colour type -> RGB at the rectangle's pitch.
// Every read of a file stays inside its stream's byte range, every write inside its rectangle or its share of the workspace, and
// every loop has a bound known from the records: blocks <= stream bits / 3 + 1 (a block takes 3 bits or more), windows <= stream
// bits / (256 x 512) + 1 per block, symbols per lane <= 512, records per window <= 256 x 512 / 2 (a match takes 2 bits or more).
// WORKSPACE, one per handle, grown under the rule of the ragged calls: per file its inflated stream H (1 + W bpp) rounded up to 256
// bytes, 512 KiB of match records, and 8 bytes per 32 KiB of the inflated stream.
#include "specmi_internal.h"

namespace specmi {

namespace {

enum { ST_ZLIB = 1, ST_BTYPE = 2, ST_STORED = 4, ST_LENS = 8, ST_REPEAT = 16, ST_NOEOB = 32, ST_CODE = 64, ST_SYMBOL = 128, ST_FAR = 256,
       ST_EARLY = 512, ST_LENGTH = 1024, ST_LEFTOVER = 2048, ST_ADLER = 4096, ST_FILTER = 8192 };

// ---- host half: rule 1 ------------------------------------------------------------------------------------------------------------
// the table CRC-32 of PNG (polynomial 0xEDB88320), eight bytes per step: table k carries a byte over k further bytes
struct CrcTables {
    unsigned t[8][256];
    CrcTables() {
        for (unsigned i = 0; i < 256; ++i) {
            unsigned c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (int k = 1; k < 8; ++k)
            for (unsigned i = 0; i < 256; ++i) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255];
    }
};

unsigned crc32_of(const unsigned char* p, size_t n) {
    static const CrcTables tab;
    const unsigned(*t)[256] = tab.t;
    unsigned c = 0xFFFFFFFFu;
    for (; n >= 8; n -= 8, p += 8) {
        const unsigned a = c ^ ((unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24);
        c = t[7][a & 255] ^ t[6][(a >> 8) & 255] ^ t[5][(a >> 16) & 255] ^ t[4][a >> 24] ^ t[3][p[4]] ^ t[2][p[5]] ^ t[1][p[6]] ^ t[0][p[7]];
    }
    for (size_t i = 0; i < n; ++i) c = t[0][(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

unsigned be32(const unsigned char* p) { return (unsigned)p[0] << 24 | (unsigned)p[1] << 16 | (unsigned)p[2] << 8 | p[3]; }

}  // namespace

int png_probe(const unsigned char* d, size_t n, int* H, int* W, int* ctype, long long* ranges, int max_ranges, int* nranges) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    *H = *W = *ctype = 0;
    *nranges = 0;
    if (n < 8) return std::memcmp(d, sig, n) ? PDEC_NOT_PNG : PDEC_TRUNCATED;
    if (std::memcmp(d, sig, 8)) return PDEC_NOT_PNG;
    size_t at = 8;
    bool first = true, ended = false, idat_open = false, idat_closed = false;
    int reason = PDEC_SUPPORTED, count = 0, h = 0, w = 0, ct = 0;
    while (!ended) {
        if (at + 12 > n) return PDEC_TRUNCATED;
        const unsigned len = be32(d + at);
        if (len > 0x7FFFFFFFu || (size_t)len > n - at - 12) return PDEC_TRUNCATED;
        const unsigned char* type = d + at + 4;
        const unsigned char* body = d + at + 8;
        if (crc32_of(type, 4 + (size_t)len) != be32(body + len)) return PDEC_CRC;
        const bool is_idat = !std::memcmp(type, "IDAT", 4);
        if (first) {
            if (std::memcmp(type, "IHDR", 4) || len != 13) return PDEC_CHUNK;
            first = false;
            w = (int)std::min<unsigned>(be32(body), 0x7FFFFFFFu);
            h = (int)std::min<unsigned>(be32(body + 4), 0x7FFFFFFFu);
            const int depth = body[8];
            ct = body[9];
            // a reason is kept and the walk goes on: a truncated, damaged or trailing-byte file is named as that first
            if (ct == 3) reason = PDEC_PALETTE;
            else if (ct != 0 && ct != 2 && ct != 4 && ct != 6) reason = PDEC_CHUNK;
            else if (depth != 8) reason = PDEC_DEPTH;
            else if (body[10] != 0 || body[11] != 0) reason = PDEC_CHUNK;
            else if (body[12] != 0) reason = PDEC_INTERLACED;
            else if (h < 1 || h > 32768 || w < 1 || w > 32768) reason = PDEC_SIZE;
        } else if (!std::memcmp(type, "IHDR", 4)) {
            if (reason == PDEC_SUPPORTED) reason = PDEC_CHUNK;
        } else if (is_idat) {
            if (idat_closed && reason == PDEC_SUPPORTED) reason = PDEC_CHUNK;
            idat_open = true;
            if (count < max_ranges && ranges) { ranges[2 * count] = (long long)(at + 8); ranges[2 * count + 1] = (long long)len; }
            ++count;
        } else if (!std::memcmp(type, "IEND", 4)) {
            if (len != 0 && reason == PDEC_SUPPORTED) reason = PDEC_CHUNK;
            ended = true;
        } else if (!std::memcmp(type, "acTL", 4)) {
            if (reason == PDEC_SUPPORTED) reason = PDEC_ANIMATED;
        } else if (!(type[0] & 0x20) && std::memcmp(type, "PLTE", 4)) {
            if (reason == PDEC_SUPPORTED) reason = PDEC_CHUNK;         // an unknown critical chunk
        }
        if (!is_idat && idat_open) idat_closed = true;
        at += 12 + (size_t)len;
    }
    if (reason != PDEC_SUPPORTED) return reason;
    if (at != n) return PDEC_TRAILING;
    if (count == 0) return PDEC_CHUNK;
    *H = h; *W = w; *ctype = ct;
    *nranges = count;
    return PDEC_SUPPORTED;
}

// ---- device half ------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int kWinBytes = kPdecLanes * kPdecSubBits / 8;      // 16 KiB of the stream per window
constexpr int kWinWords = (kWinBytes + 32) / 4;               // and what the last lane's last symbol and its look-ahead reach
constexpr int kLitBits = 10, kDistBits = 8;
constexpr int kFlagEob = 1 << 30;                             // in a lane's flags, beside the ST_ bits

__constant__ unsigned short kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ unsigned char kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ unsigned short kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ unsigned char kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ unsigned char kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// a canonical code: per length the first code, how many, and where its symbols begin in `sorted` (symbols by length, then value)
struct Canon {
    unsigned short first[16], count[16], offs[16];
};

struct PdecLds {
    unsigned win[kWinWords + 1];
    unsigned short llut[1 << kLitBits];       // length << 9 | symbol by the next 10 bits, MSB first; 0: longer, or no code
    unsigned short dlut[1 << kDistBits];
    unsigned short lsorted[288], dsorted[32], lcode[288], dcode[32];
    unsigned char lens[320];
    Canon lit, dist;
    unsigned short len_base[29], dist_base[30];
    unsigned char len_extra[29], dist_extra[30];
    int sexit[kPdecLanes];
    unsigned long long scan[kPdecLanes];
    // what one lane decides for all: block type, final flag, status, where the symbols (or the stored bytes) begin, stored length
    int btype, bfinal, status, stored_len, first_flagged;
    long long bits_at;
};

// bits [at, at + n) of the stream, LSB first, n <= 16; bits from `end` on read as zero (a caller compares at + n with end itself)
__device__ __forceinline__ unsigned stream_bits(const unsigned char* p, long long at, int n, long long end) {
    unsigned v = 0;
    for (int k = 0; k < 3; ++k) {
        const long long byte = (at >> 3) + k;
        if (byte * 8 < end) v |= (unsigned)p[byte] << (8 * k);
    }
    return (v >> (at & 7)) & ((1u << n) - 1u);
}

// thread 0: the canonical code of lens[0 .. n): -> 0 complete, > 0 incomplete, < 0 over-subscribed; *maxlen the longest length
__device__ int canon_build(const unsigned char* lens, int n, Canon& c, unsigned short* sorted, unsigned short* code, int* maxlen) {
    for (int l = 0; l < 16; ++l) c.count[l] = 0;
    for (int i = 0; i < n; ++i) ++c.count[lens[i]];
    c.count[0] = 0;
    int left = 1, first = 0, off = 0, mx = 0;
    unsigned short next[16];
    for (int l = 1; l < 16; ++l) {
        left = 2 * left - (int)c.count[l];
        if (left < 0) return -1;
        first = (first + (int)c.count[l - 1]) << 1;
        c.first[l] = (unsigned short)first;
        c.offs[l] = (unsigned short)off;
        next[l] = (unsigned short)off;
        off += c.count[l];
        if (c.count[l]) mx = l;
    }
    c.first[0] = c.offs[0] = 0;
    for (int i = 0; i < n; ++i)
        if (lens[i]) {
            const int l = lens[i], at = next[l]++;
            sorted[at] = (unsigned short)i;
            code[i] = (unsigned short)(c.first[l] + (at - c.offs[l]));
        }
    *maxlen = mx;
    return left;
}

// the symbol whose code the 15 bits c (MSB first) begin with: -> length << 9 | symbol, 0: no code
__device__ __forceinline__ unsigned canon_lookup(const Canon& c, const unsigned short* sorted, unsigned c15, int from) {
#pragma unroll 1
    for (int l = from; l <= 15; ++l) {
        const unsigned d = (c15 >> (15 - l)) - c.first[l];
        if (d < c.count[l]) return (unsigned)l << 9 | sorted[c.offs[l] + d];
    }
    return 0;
}

// thread 0: the header of the block at bit `at` -> what PdecLds holds for all
__device__ void parse_header(PdecLds& s, const unsigned char* p, long long at, long long end) {
    s.status = 0;
    if (at + 3 > end) { s.status = ST_EARLY; return; }
    const unsigned h = stream_bits(p, at, 3, end);
    s.bfinal = (int)(h & 1);
    s.btype = (int)(h >> 1);
    at += 3;
    if (s.btype == 3) { s.status = ST_BTYPE; return; }
    if (s.btype == 0) {
        at = (at + 7) & ~7ll;
        if (at + 32 > end) { s.status = ST_EARLY; return; }
        const unsigned len = stream_bits(p, at, 16, end), nlen = stream_bits(p, at + 16, 16, end);
        if ((len ^ nlen) != 0xFFFFu) { s.status = ST_STORED; return; }
        at += 32;
        if (at + 8ll * len > end) { s.status = ST_EARLY; return; }
        s.stored_len = (int)len;
        s.bits_at = at;
        return;
    }
    int nlit = 288, ndist = 30;
    if (s.btype == 1) {
        for (int i = 0; i < 288; ++i) s.lens[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) s.lens[288 + i] = 5;
        ndist = 32;
    } else {
        if (at + 14 > end) { s.status = ST_EARLY; return; }
        nlit = 257 + (int)stream_bits(p, at, 5, end);
        ndist = 1 + (int)stream_bits(p, at + 5, 5, end);
        const int ncl = 4 + (int)stream_bits(p, at + 10, 4, end);
        at += 14;
        if (nlit > 286 || ndist > 30) { s.status = ST_LENS; return; }
        if (at + 3 * ncl > end) { s.status = ST_EARLY; return; }
        unsigned char cl[19];
        for (int i = 0; i < 19; ++i) cl[i] = 0;
        for (int i = 0; i < ncl; ++i, at += 3) cl[kClOrder[i]] = (unsigned char)stream_bits(p, at, 3, end);
        Canon cc;
        unsigned short csorted[19], ccode[19];
        int mx;
        if (canon_build(cl, 19, cc, csorted, ccode, &mx) != 0) { s.status = ST_LENS; return; }
        int i = 0;
        while (i < nlit + ndist) {                            // every turn adds a length or more: at most 316 turns
            const unsigned w = stream_bits(p, at, 7, end);
            const unsigned e = canon_lookup(cc, csorted, (__brev(w) >> 25) << 8, 1);
            const int l = (int)(e >> 9), sym = (int)(e & 511);
            if (!l || l > 7) { s.status = at + 7 > end ? ST_EARLY : ST_CODE; return; }
            at += l;
            if (at > end) { s.status = ST_EARLY; return; }
            if (sym < 16) { s.lens[i++] = (unsigned char)sym; continue; }
            const int eb = sym == 16 ? 2 : sym == 17 ? 3 : 7, base = sym == 18 ? 11 : 3;
            if (at + eb > end) { s.status = ST_EARLY; return; }
            const int rep = base + (int)stream_bits(p, at, eb, end);
            at += eb;
            if (sym == 16 && i == 0) { s.status = ST_REPEAT; return; }
            if (i + rep > nlit + ndist) { s.status = ST_REPEAT; return; }
            const unsigned char v = sym == 16 ? s.lens[i - 1] : 0;
            for (int k = 0; k < rep; ++k) s.lens[i++] = v;
        }
        if (s.lens[256] == 0) { s.status = ST_NOEOB; return; }
        // the distance lengths follow the literal/length lengths: move them to their own place, zero the rest
        unsigned char dl[32];
        for (int k = 0; k < 32; ++k) dl[k] = k < ndist ? s.lens[nlit + k] : 0;
        for (int k = nlit; k < 288; ++k) s.lens[k] = 0;
        for (int k = 0; k < 32; ++k) s.lens[288 + k] = dl[k];
        nlit = 288; ndist = 32;
    }
    int mx;
    if (canon_build(s.lens, nlit, s.lit, s.lsorted, s.lcode, &mx) != 0) { s.status = ST_LENS; return; }
    const int left = canon_build(s.lens + 288, ndist, s.dist, s.dsorted, s.dcode, &mx);
    if (left < 0 || (left > 0 && mx > 1)) { s.status = ST_LENS; return; }       // mx 0: no distance code; mx 1: a single one
    s.bits_at = at;
}

// all lanes: the look-ahead tables from the lengths and codes parse_header left
__device__ void fill_luts(PdecLds& s) {
    const int tid = threadIdx.x;
    for (int i = tid; i < (1 << kLitBits); i += kPdecLanes) s.llut[i] = 0;
    if (tid < (1 << kDistBits)) s.dlut[tid] = 0;
    __syncthreads();
    for (int i = tid; i < 288 + 32; i += kPdecLanes) {
        const bool d = i >= 288;
        const int sym = d ? i - 288 : i, l = s.lens[i], bits = d ? kDistBits : kLitBits;
        if (l == 0 || l > bits) continue;
        const unsigned code = d ? s.dcode[sym] : s.lcode[sym];
        unsigned short* lut = d ? s.dlut : s.llut;
        const unsigned e = (unsigned)l << 9 | (unsigned)sym;
        for (unsigned j = 0; j < (1u << (bits - l)); ++j) lut[(code << (bits - l)) + j] = (unsigned short)e;
    }
    __syncthreads();
}

// 32 bits of the window from bit p on, LSB first
__device__ __forceinline__ unsigned peek(const PdecLds& s, int p) {
    const unsigned long long v = (unsigned long long)s.win[(p >> 5) + 1] << 32 | s.win[p >> 5];
    return (unsigned)(v >> (p & 31));
}

// One lane: every symbol that starts in [entry, lane_end) of the window (bit positions from the window's base).  -> the exit (the
// bit behind its last symbol; lane_end after the end-of-block code or an anomaly: a cold start for the right neighbour), the bytes
// and matches it produces, and its flags (kFlagEob with *eob_at, or ST_ bits).  WRITE: literals go to raw[o ...] and the matches
// to rec[...]; the caller has checked that the window's bytes fit.  At most kPdecSubBits symbols start in a subsequence.
template <bool WRITE>
__device__ __forceinline__ int decode_lane(const PdecLds& s, int entry, int lane_end, int end, unsigned* nbytes, unsigned* nmatch, int* flags,
                                           int* eob_at, unsigned char* raw, long long o, long long win_o, uint2* rec, long long max_dist) {
    int p = entry, fl = 0;
    unsigned nb = 0, nm = 0;
#pragma unroll 1
    for (int it = 0; it < kPdecSubBits && p < lane_end; ++it) {
        if (p >= end) { fl = ST_EARLY; break; }
        const unsigned w = peek(s, p);
        const unsigned c = __brev(w) >> 17;
        unsigned e = s.llut[c >> (15 - kLitBits)];
        if (!e) e = canon_lookup(s.lit, s.lsorted, c, kLitBits + 1);
        if (!e) { fl = ST_CODE; break; }
        const int l = (int)(e >> 9), sym = (int)(e & 511);
        int p2 = p + l;
        if (p2 > end) { fl = ST_EARLY; break; }
        if (sym < 256) {
            if (WRITE) raw[o] = (unsigned char)sym;
            ++o; ++nb; p = p2;
            continue;
        }
        if (sym == 256) { fl = kFlagEob; *eob_at = p2; break; }
        if (sym >= 286) { fl = ST_SYMBOL; break; }
        const int eb = s.len_extra[sym - 257];
        const int length = s.len_base[sym - 257] + (int)((w >> l) & ((1u << eb) - 1u));
        p2 += eb;
        const unsigned w2 = peek(s, p2);
        const unsigned c2 = __brev(w2) >> 17;
        unsigned e2 = s.dlut[c2 >> (15 - kDistBits)];
        if (!e2) e2 = canon_lookup(s.dist, s.dsorted, c2, kDistBits + 1);
        if (!e2) { fl = p2 + 15 > end ? ST_EARLY : ST_CODE; break; }
        const int dl = (int)(e2 >> 9), dsym = (int)(e2 & 511);
        if (dsym >= 30) { fl = ST_SYMBOL; break; }
        const int deb = s.dist_extra[dsym];
        const int dist = s.dist_base[dsym] + (int)((w2 >> dl) & ((1u << deb) - 1u));
        p2 += dl + deb;
        if (p2 > end) { fl = ST_EARLY; break; }
        if (WRITE) {
            if (dist > o || dist > max_dist) { fl = ST_FAR; break; }
            rec[nm] = make_uint2((unsigned)(o - win_o), (unsigned)length | (unsigned)dist << 9);
        }
        o += length; nb += (unsigned)length; ++nm; p = p2;
    }
    *nbytes = nb; *nmatch = nm; *flags = fl;
    return fl ? lane_end : (p > lane_end ? p : lane_end);
}

__global__ void __launch_bounds__(kPdecLanes) pdec_inflate_kernel(PdecArgs a) {
    __shared__ PdecLds s;
    const PdecFile* f = a.files + blockIdx.x;
    const int tid = threadIdx.x;
    const unsigned char* p = a.in + f->stream_off;
    const long long len = f->stream_len, end = (len - 4) * 8, raw_len = f->raw_len;
    unsigned char* raw = a.raw + f->raw_off;
    uint2* rec = a.rec + (long long)blockIdx.x * kPdecMaxRec;
    if (tid < 29) { s.len_base[tid] = kLenBase[tid]; s.len_extra[tid] = kLenExtra[tid]; }
    if (tid < 30) { s.dist_base[tid] = kDistBase[tid]; s.dist_extra[tid] = kDistExtra[tid]; }
    for (int i = tid; i <= kWinWords; i += kPdecLanes) s.win[i] = 0;
    const unsigned cmf = p[0], flg = p[1];
    int st = 0;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (cmf * 256 + flg) % 31 != 0 || (flg & 32)) st = ST_ZLIB;
    const long long max_dist = 1ll << ((cmf >> 4) + 8);
    long long bp = 16, op = 0;
    bool final_seen = false;
    const long long max_blocks = end / 3 + 1;
#pragma unroll 1
    for (long long blk = 0; blk < max_blocks && !st; ++blk) {
        __syncthreads();
        if (tid == 0) parse_header(s, p, bp, end);
        __syncthreads();
        st = s.status;
        if (st) break;
        const int btype = s.btype, bfinal = s.bfinal;
        bp = s.bits_at;
        if (btype == 0) {
            const int n = s.stored_len;
            if (op + n > raw_len) { st = ST_LENGTH; break; }
            const unsigned char* src = p + (bp >> 3);
            for (int i = tid; i < n; i += kPdecLanes) raw[op + i] = src[i];
            op += n;
            bp += 8ll * n;
        } else {
            fill_luts(s);
            const long long max_windows = (end - bp) / (kPdecLanes * kPdecSubBits) + 1;
            bool open = true;
#pragma unroll 1
            for (long long win = 0; win < max_windows && open && !st; ++win) {
                // stage the window: whole words from a byte that is a multiple of 4; bytes from the Adler word on read as zero
                const long long base = (bp >> 3) & ~3ll;
                __syncthreads();
                for (int i = tid; i < kWinWords; i += kPdecLanes) {
                    unsigned v = 0;
                    for (int k = 0; k < 4; ++k) {
                        const long long byte = base + 4ll * i + k;
                        if (byte < len - 4) v |= (unsigned)p[byte] << (8 * k);
                    }
                    s.win[i] = v;
                }
                if (tid == 0) s.first_flagged = kPdecLanes;
                const int rel0 = (int)(bp - base * 8);
                const int wend = (int)min(end - base * 8, (long long)(kWinWords * 32));
                const int lane_end = rel0 + (tid + 1) * kPdecSubBits;
                int entry = -1, ex = lane_end, fl = 0, eob_at = 0;
                unsigned nb = 0, nm = 0;
                __syncthreads();
#pragma unroll 1
                for (int round = 0; round <= kPdecLanes; ++round) {
                    s.sexit[tid] = ex;
                    __syncthreads();
                    const int e = tid == 0 ? rel0 : s.sexit[tid - 1];
                    int moved = 0;
                    if (e != entry) {
                        entry = e;
                        ex = decode_lane<false>(s, e, lane_end, wend, &nb, &nm, &fl, &eob_at, nullptr, 0, 0, nullptr, 0);
                        moved = 1;
                    }
                    if (!__syncthreads_or(moved)) break;
                }
                if (fl) atomicMin(&s.first_flagged, tid);
                __syncthreads();
                const int ff = s.first_flagged;
                const bool mine = tid <= ff;
                const unsigned long long v = mine ? (unsigned long long)nb << 32 | nm : 0ull;
                s.scan[tid] = v;
                __syncthreads();
#pragma unroll
                for (int d = 1; d < kPdecLanes; d <<= 1) {
                    const unsigned long long add = tid >= d ? s.scan[tid - d] : 0ull;
                    __syncthreads();
                    s.scan[tid] += add;
                    __syncthreads();
                }
                const unsigned long long excl = s.scan[tid] - v, total = s.scan[kPdecLanes - 1];
                const long long win_bytes = (long long)(total >> 32);
                const int win_matches = (int)(total & 0xFFFFFFFFu);
                if (ff < kPdecLanes) s.sexit[0] = 0;                   // the flagged lane tells all what it met
                __syncthreads();
                if (tid == ff) { s.sexit[0] = fl; s.sexit[1] = eob_at; }
                __syncthreads();
                const int ffl = ff < kPdecLanes ? s.sexit[0] : 0, feob = ff < kPdecLanes ? s.sexit[1] : 0;
                const int last_exit = s.sexit[kPdecLanes - 1];
                __syncthreads();
                if (ffl & ~kFlagEob) { st = ffl & ~kFlagEob; break; }
                if (op + win_bytes > raw_len || win_matches > kPdecMaxRec) { st = ST_LENGTH; break; }
                if (tid == 0) s.status = 0;
                __syncthreads();
                if (mine) {
                    int wfl, weob;
                    unsigned wnb, wnm;
                    decode_lane<true>(s, entry, lane_end, wend, &wnb, &wnm, &wfl, &weob, raw, op + (long long)(excl >> 32), op,
                                      rec + (excl & 0xFFFFFFFFu), max_dist);
                    if (wfl & ~kFlagEob) atomicOr(&s.status, wfl & ~kFlagEob);
                }
                __syncthreads();
                st = s.status;
                if (st) break;
                if (tid < 64) {
                    // one wavefront resolves the matches in stream order, 64 records at a time
#pragma unroll 1
                    for (int rb = 0; rb < win_matches;) {
                        const int j = rb + tid;
                        const bool have = j < win_matches;
                        const uint2 r = have ? rec[j] : make_uint2(0, 1 | 1 << 9);
                        const long long dst = op + r.x;
                        const int length = (int)(r.y & 511), dist = (int)(r.y >> 9);
                        const long long dst0 = __shfl(dst, 0);
                        const bool indep = have && dst - dist + min(length, dist) <= dst0;
                        const unsigned long long mask = __ballot(indep);
                        const int m = ~mask ? __builtin_ctzll(~mask) : 64;          // lane 0's record is always independent
                        if (m <= 1) {
                            const int L = __shfl(length, 0), D = __shfl(dist, 0);
                            for (int k = tid; k < L; k += 64) raw[dst0 + k] = raw[dst0 - D + k % D];
                        } else if (tid < m) {
                            int q = 0;
                            for (int k = 0; k < length; ++k) {
                                raw[dst + k] = raw[dst - dist + q];
                                if (++q == dist) q = 0;
                            }
                        }
                        __threadfence_block();
                        rb += m < 1 ? 1 : m;
                    }
                }
                op += win_bytes;
                if (ffl & kFlagEob) { bp = base * 8 + feob; open = false; }
                else bp = base * 8 + last_exit;
            }
            if (st) break;
            if (open) { st = ST_EARLY; break; }                       // the windows ran out without an end-of-block code
        }
        if (bfinal) { final_seen = true; break; }
    }
    if (!st) {
        if (!final_seen) st = ST_EARLY;
        else if (op != raw_len) st = ST_LENGTH;
        else if (((bp + 7) & ~7ll) != end) st = ST_LEFTOVER;
    }
    if (tid == 0 && st) atomicOr(a.status + blockIdx.x, st);
}

// a workgroup per chunk of kPdecAdlerChunk inflated bytes: the sum of the bytes and the sum of (n - i) byte[i], both mod 65521
__global__ void __launch_bounds__(256) pdec_adler_kernel(PdecArgs a) {
    __shared__ unsigned long long l1[256], l2[256];
    const PdecFile* f = a.files + last_at_or_before(a.files, a.n, blockIdx.x, &PdecFile::chunk0);
    const long long at = (long long)((int)blockIdx.x - f->chunk0) * kPdecAdlerChunk;
    const int n = (int)min((long long)kPdecAdlerChunk, f->raw_len - at), tid = threadIdx.x;
    const unsigned char* raw = a.raw + f->raw_off + at;
    unsigned s1 = 0, s2 = 0;                                  // a thread's 128 bytes: at most 128 x 255 x 32768 < 2^32
    for (int i = tid; i < n; i += 256) {
        const unsigned v = raw[i];
        s1 += v;
        s2 += v * (unsigned)(n - i);
    }
    l1[tid] = s1; l2[tid] = s2;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) { l1[tid] += l1[tid + d]; l2[tid] += l2[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) a.sums[blockIdx.x] = make_uint2((unsigned)(l1[0] % 65521ull), (unsigned)(l2[0] % 65521ull));
}

// a workgroup per file: with s1 = P in front of a chunk of n bytes, s2 grows by n P + sum (n - i) byte[i]
__global__ void __launch_bounds__(256) pdec_adler_join_kernel(PdecArgs a) {
    __shared__ unsigned long long l1[256], l2[256];
    const PdecFile* f = a.files + blockIdx.x;
    const int tid = threadIdx.x;
    // s1 = 1 + all bytes; s2 = sum over chunks of (sum2 + n (1 + bytes before it)): a thread's chunks first need the bytes before them
    unsigned long long mine1 = 0;
    for (int c = tid; c < f->nchunk; c += 256) mine1 += a.sums[f->chunk0 + c].x;
    l1[tid] = mine1 % 65521ull;
    __syncthreads();
    unsigned long long s2 = 0;
    if (tid == 0) {
        unsigned long long before = 1;                        // serial over the chunks: 200 of them in a 1080p frame
        for (int c = 0; c < f->nchunk; ++c) {
            const uint2 v = a.sums[f->chunk0 + c];
            const unsigned long long n = (unsigned long long)min((long long)kPdecAdlerChunk, f->raw_len - (long long)c * kPdecAdlerChunk);
            s2 = (s2 + v.y + n % 65521ull * before) % 65521ull;
            before = (before + v.x) % 65521ull;
        }
        l2[0] = s2;
    }
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) l1[tid] += l1[tid + d];
        __syncthreads();
    }
    if (tid == 0 && a.status[blockIdx.x] == 0) {              // a stream that did not inflate whole has no sum to compare
        const unsigned adler = (unsigned)l2[0] << 16 | (unsigned)((1ull + l1[0]) % 65521ull);
        const unsigned char* t = a.in + f->stream_off + f->stream_len - 4;
        const unsigned want = (unsigned)t[0] << 24 | (unsigned)t[1] << 16 | (unsigned)t[2] << 8 | t[3];
        if (adler != want) atomicOr(a.status + blockIdx.x, (int)ST_ADLER);
    }
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// one wavefront per file, strips of 64 rows in order (rule 3)
__global__ void __launch_bounds__(64) pdec_unfilter_kernel(PdecArgs a) {
    const PdecFile* f = a.files + blockIdx.x;
    if (a.status[blockIdx.x] & ~(int)ST_ADLER) return;               // the inflated stream is not whole: its pixels are unspecified
    const int lane = threadIdx.x, H = f->H, W = f->W, bpp = f->bpp, nch = f->nch;
    const long long line = 1 + (long long)W * bpp;
    const unsigned char* raw = a.raw + f->raw_off;
    unsigned char* out = a.out + f->out_off;
    int bad = 0;
#pragma unroll 1
    for (int r0 = 0; r0 < H; r0 += 64) {
        const int row = r0 + lane;
        const bool live = row < H;
        const unsigned char* src = raw + (long long)(live ? row : 0) * line;
        const int ft = live ? src[0] : 0;
        if (ft > 4) bad = 1;
        unsigned char* dst = out + (long long)(live ? row : 0) * f->pitch;
        const unsigned char* above = out + (long long)(r0 > 0 ? r0 - 1 : 0) * f->pitch;
        int cur[3] = {0, 0, 0}, up[3] = {0, 0, 0};            // this row's last pixel; the pixel above it
#pragma unroll 1
        for (int step = 0; step < W + 63; ++step) {
            const int x = step - lane;
            const bool on = live && x >= 0 && x < W;
            int upleft[3], left[3], nup[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // lane k - 1 finished pixel x of the row above in the step before
                int v = __shfl_up(cur[c], 1);
                if (lane == 0) v = (r0 > 0 && x >= 0 && x < W) ? above[3ll * x + c] : 0;
                nup[c] = v;
                upleft[c] = x > 0 ? up[c] : 0;
                left[c] = x > 0 ? cur[c] : 0;
            }
            if (on) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c < nch) {
                        const int v = src[1 + (long long)x * bpp + c];
                        int pred = 0;
                        if (ft == 1) pred = left[c];
                        else if (ft == 2) pred = nup[c];
                        else if (ft == 3) pred = (left[c] + nup[c]) >> 1;
                        else if (ft == 4) pred = paeth(left[c], nup[c], upleft[c]);
                        cur[c] = (v + pred) & 255;
                    } else {
                        cur[c] = cur[0];
                    }
                    dst[3ll * x + c] = (unsigned char)cur[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) up[c] = nup[c];
        }
        __threadfence_block();                                // the next strip's first lane reads this strip's last row
    }
    if (bad) atomicOr(a.status + blockIdx.x, (int)ST_FILTER);
}

}  // namespace

size_t pdec_ws_layout(int n, long long raw_bytes, long long chunks, size_t off[3]) {
    const size_t sizes[3] = {(size_t)raw_bytes, (size_t)n * kPdecMaxRec * 8, (size_t)chunks * 8};
    size_t at = 0;
    for (int i = 0; i < 3; ++i) {
        off[i] = at;
        at += (sizes[i] + 255) & ~(size_t)255;
    }
    return at;
}

int launch_png_decode(const PdecArgs& a, double in_bytes, double raw_bytes, double out_bytes, const LaunchCtx& ctx) {
    if (hipError_t e = hipMemsetAsync(a.status, 0, (size_t)a.n * 4, ctx.stream)) return (int)e;
    {
        ProfScope ps(ctx, "pdec_inflate", 0.0, in_bytes + raw_bytes);
        hipLaunchKernelGGL(pdec_inflate_kernel, dim3((unsigned)a.n), dim3(kPdecLanes), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "pdec_adler", 0.0, raw_bytes);
        hipLaunchKernelGGL(pdec_adler_kernel, dim3((unsigned)a.chunks), dim3(256), 0, ctx.stream, a);
        hipLaunchKernelGGL(pdec_adler_join_kernel, dim3((unsigned)a.n), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "pdec_unfilter", 0.0, raw_bytes + out_bytes);
        hipLaunchKernelGGL(pdec_unfilter_kernel, dim3((unsigned)a.n), dim3(64), 0, ctx.stream, a);
    }
    return (int)hipGetLastError();
}

}  // namespace specmi
