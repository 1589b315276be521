// png.hip - PNG files encoded on the device from uint8 RGB rectangles of a slab: what the reference
// hands to cv2.imwrite / PIL's save for the picture of a .png frame (spec/tester.py:95 accepts them, :188-201 keeps the frame's
// extension; camcalib/pano_preprocessing.py:354 writes a tree of them), for all pictures of a flush in one fixed sequence of
// launches, so that the encoded bytes come down instead of the raw pictures.
//
// THE CONTRACT.  PNG is lossless, so the file is not "Pillow's bytes" but a valid file that decodes to exactly the picture, with
// bytes fixed by the rules below and by nothing else - not by a picture's neighbours in the call, by grouping or by scheduling.
// tests/png_ref.py restates the rules in NumPy and plain Python; the device's file equals its file byte for byte.
// 1. Layout.  The 8 signature bytes; IHDR (W, H, 8 bit, colour type 2, compression 0, filter 0, no interlace); exactly ONE IDAT
//    holding one zlib stream: 78 01, the deflate blocks of rules 3 to 7, the Adler-32 of the filtered stream; IEND.  Every chunk
//    carries its CRC-32.  The first 33 bytes are Pillow's.
// 2. Filter.  Row y becomes 1 + 3 W bytes: the filter type, then the bytes filtered against the raw neighbours at distance 3
//    (left), the row above and both (PNG 1.2 section 6; the Paeth predictor picks a, then b, then c on equal distances; bytes left
//    of the row and above the picture count 0).  A row takes the type 0 .. 4 whose filtered bytes, read as signed, have the
//    smallest sum of absolute values (a byte v costs v below 128, else 256 - v); equal sums go to the lowest type.
// 3. Segments.  The filtered stream of H (1 + 3 W) bytes is cut into segments of 32768 bytes (the last one shorter).  Every segment
//    is coded on its own into whole bytes; nothing but its length reaches the next.
// 4. Tokens.  At byte i of a segment, M1 is how many bytes from i on equal the byte before them (inside the segment, at most 258),
//    M3 the same for the byte 3 before them.  With M = max(M1, M3) >= 3 the token is a match of length M, at distance 1 if
//    M1 >= M3, else 3; otherwise the literal byte.  The parse is greedy from byte 0: the next token starts where this one ends.
// 5. Codes.  The literal / length alphabet (286 symbols, RFC 1951 3.2.5) is counted over the tokens, plus one end-of-block.  The
//    symbols with a non-zero count are sorted by (count, symbol) into a queue of leaves; Huffman's algorithm joins the two
//    smallest fronts of the leaf queue and the queue of joined nodes (in order of creation), a leaf first where counts are equal.
//    A leaf's depth is its code length.  While a length exceeds 15, every non-zero count c becomes (c + 1) >> 1 and the tree is
//    built again.  Codes are canonical (RFC 1951 3.2.2).  A distance that occurs is one bit long: distance 1 is the code 0,
//    distance 3 the code 1 - or 0 where distance 1 does not occur.
// 6. The coded form: one dynamic block, BFINAL 0, HLIT 29, HDIST 2, HCLEN 15; of the code-length alphabet the symbols 0 .. 15
//    are 4 bits long (symbol k is the code k) and 16, 17, 18 unused, so every one of the 286 + 3 lengths is sent as itself - a
//    header of 1230 bits; the tokens; the end-of-block.
// 7. Then an empty stored block (3 header bits, zero bits up to the byte, 00 00 FF FF) realigns the stream; it carries BFINAL on
//    the picture's last segment.  A segment whose coded form with that block is not shorter than 5 + n bytes is ONE stored block
//    instead: BFINAL (a whole byte), n and its complement as 16-bit little-endian, the n bytes.
// 8. Bound.  No file is longer than 63 + L + 5 ceil(L / 32768) bytes, L = H (1 + 3 W): every segment stored (specmi_png_bound).
//
// STAGES - one memset and five launches, whatever the number of pictures and their sizes.  Rows and segments of the pictures are
// numbered back to back; a workgroup finds its picture by bisecting the record table, as the other ragged kernels do.
//   filter   one workgroup per row (at most 2^20 workgroups, each then takes every 2^20th row): the five sums, the choice, the
//            filtered row into the workspace
//   segment  one workgroup per segment, which holds it in LDS: matches, the greedy parse, counts, code lengths, the byte count,
//            then the blocks into the segment's room in the workspace - Huffman codes as bits joined with atomicOr into zeroed
//            words (an integer OR of disjoint bits does not depend on the order), a stored block with plain stores - and the
//            segment's two Adler-32 sums.  The segment lies in LDS interleaved by owner (at_lds), so that a wavefront's lanes
//            read neighbouring bytes.  The parse is made parallel in three steps: every thread owns 128 bytes and finds, from
//            their end backwards, where the parse leaves them for EACH byte it could enter at; one thread then hops from range to
//            range (at most 256 hops) and notes where the real parse enters each; every thread walks its own range from there.
//   scan     one workgroup per picture: exclusive scan of its segments' bytes -> each segment's place, sizes[], the Adler-32
//   pack     one workgroup per segment: its blocks to their place in the file, and their share of IDAT's CRC-32 - the CRC of
//            the bytes with register 0 times x^(8 bytes behind them) in GF(2)[x] mod the CRC polynomial, which is linear, so
//            that shares are joined with XOR
//   finish   one workgroup per picture: the shares joined, signature, IHDR with its CRC, IDAT's length and type, 78 01, the
//            Adler-32, IDAT's CRC, IEND.
// Nothing is written at or beyond a picture's capacity.  No kernel spins or waits for another workgroup; every loop's trip count
// is bounded by a constant or by a size the host checked.
// WORKSPACE, one per handle, grown under the rule of the ragged calls: the filtered streams (each rounded up to 256 bytes), 32800
// bytes per segment for its blocks and 24 for its sums, 4 per picture.
#include "specmi_internal.h"

namespace specmi {

namespace {

constexpr unsigned kCrcPoly = 0xedb88320u;
constexpr int kPngHeaderBits = 3 + 14 + 19 * 3 + (286 + 3) * 4;       // rule 6
constexpr int kPngOwn = kPngSegment / 256;                            // bytes of a segment one thread owns

// ---- CRC-32 as polynomials over GF(2), bit 31 = x^0 (the reflected form of the CRC register) -------------------------------------
__host__ __device__ inline unsigned gf_mul(unsigned a, unsigned b) {        // a b mod the CRC polynomial
    unsigned p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
__host__ __device__ inline unsigned gf_xpow8(unsigned long long bytes) {    // x^(8 bytes)
    unsigned p = 0x80000000u, sq = 0x00800000u;                             // x^0, x^8
    for (int i = 0; i < 61 && (bytes >> i); ++i) {
        if ((bytes >> i) & 1ull) p = gf_mul(sq, p);
        sq = gf_mul(sq, sq);
    }
    return p;
}
__host__ __device__ inline unsigned crc_byte(unsigned c, unsigned char b) {  // one byte through the register, bit by bit
    c ^= b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}
__host__ __device__ inline unsigned crc_std(const unsigned char* d, int n) {
    unsigned c = 0xffffffffu;
    for (int i = 0; i < n; ++i) c = crc_byte(c, d[i]);
    return c ^ 0xffffffffu;
}
__host__ __device__ inline void put_be32(unsigned char* p, unsigned v) {
    p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}
// rule 1: signature and IHDR
__host__ __device__ inline void header33(int H, int W, unsigned char* o) {
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int i = 0; i < 8; ++i) o[i] = sig[i];
    put_be32(o + 8, 13);
    o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
    put_be32(o + 16, (unsigned)W); put_be32(o + 20, (unsigned)H);
    o[24] = 8; o[25] = 2; o[26] = 0; o[27] = 0; o[28] = 0;
    put_be32(o + 29, crc_std(o + 12, 17));
}

// ---- device half ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// rule 2 for byte x of a row: the five filtered bytes
__device__ __forceinline__ void filtered(const unsigned char* cur, const unsigned char* up, int x, int (&v)[5]) {
    const int r = cur[x], a = x >= 3 ? cur[x - 3] : 0, b = up ? up[x] : 0, c = (up && x >= 3) ? up[x - 3] : 0;
    v[0] = r; v[1] = (r - a) & 255; v[2] = (r - b) & 255; v[3] = (r - ((a + b) >> 1)) & 255; v[4] = (r - paeth(a, b, c)) & 255;
}

// one row of the call, by the whole workgroup; `sums` is its five counters in LDS
__device__ __forceinline__ void filter_row(const PngArgs& a, int row, int* sums) {
    const PngPic p = a.pics[last_at_or_before(a.pics, a.n, row, &PngPic::row0)];
    const int y = row - p.row0, n = 3 * p.W;
    const unsigned char* cur = a.in + p.in_off + (long long)y * p.in_pitch;
    const unsigned char* up = y ? cur - p.in_pitch : nullptr;
    if (threadIdx.x < 5) sums[threadIdx.x] = 0;
    __syncthreads();
    int s[5] = {0, 0, 0, 0, 0}, v[5];
    for (int x = threadIdx.x; x < n; x += 256) {
        filtered(cur, up, x, v);
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += v[k] < 128 ? v[k] : 256 - v[k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) atomicAdd(&sums[k], s[k]);             // integer sums: the order does not matter
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k)
        if (sums[k] < sums[t]) t = k;
    unsigned char* out = a.filt + p.filt_off + (long long)y * (n + 1);
    if (threadIdx.x == 0) out[0] = (unsigned char)t;
    for (int x = threadIdx.x; x < n; x += 256) {
        filtered(cur, up, x, v);
        out[1 + x] = (unsigned char)(t == 0 ? v[0] : t == 1 ? v[1] : t == 2 ? v[2] : t == 3 ? v[3] : v[4]);
    }
    __syncthreads();            // before the next row zeroes the counters
}

// A call may hold 65535 x 32768 rows, more than one launch has workgroups for: the grid is capped at kPngFilterGrid and a workgroup
// takes every gridDim.x-th row.  The trip count is the same for all threads of a workgroup, so the barriers are safe.
__global__ void __launch_bounds__(256) png_filter_kernel(PngArgs a) {
    __shared__ int sums[5];
    for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) filter_row(a, (int)row, sums);
}

// `len` bits of v into a zeroed little-endian bit stream at bit `at` (len <= 32)
__device__ __forceinline__ void or_bits(unsigned* buf, unsigned at, unsigned v, int len) {
    const unsigned long long w = (unsigned long long)v << (at & 31);
    atomicOr(buf + (at >> 5), (unsigned)w);
    if ((int)(at & 31) + len > 32) atomicOr(buf + (at >> 5) + 1, (unsigned)(w >> 32));
}

// bits appended LSB first to such a stream; a word may be shared with a neighbour, so every word is joined with atomicOr
struct BitWriter {
    unsigned* word;
    unsigned long long acc;
    int fill;                   // bits of acc that belong to *word, 0 .. 31
    __device__ __forceinline__ BitWriter(unsigned* buf, unsigned bit) : word(buf + (bit >> 5)), acc(0), fill((int)(bit & 31)) {}
    __device__ __forceinline__ void put(unsigned v, int len) {          // len <= 32: acc holds at most 31 + 32 bits
        acc |= (unsigned long long)v << fill;
        fill += len;
        if (fill >= 32) {
            atomicOr(word++, (unsigned)acc);
            acc >>= 32;
            fill -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (fill) atomicOr(word, (unsigned)acc);
    }
};

// RFC 1951 3.2.5: a match length 3 .. 258 -> its symbol, the number of extra bits and their value
__device__ __forceinline__ int length_symbol(int len, int* extra, int* value) {
    const int l = len - 3;
    if (l < 8 || len == 258) {
        *extra = 0; *value = 0;
        return len == 258 ? 285 : 257 + l;
    }
    const int e = 29 - __clz(l);
    *extra = e; *value = l & ((1 << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}
__device__ __forceinline__ int symbol_extra(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }

// what the segment kernel keeps in LDS (105 KiB: one workgroup per CU's 160 KiB).  A thread owns 128 consecutive bytes of the
// segment and walks them one by one; were they consecutive in LDS too, the lanes of a wavefront would read at strides of 128 bytes
// (256 in `tok`), fall into one or two banks and serialise every access.  So byte i of the segment lies at at_lds(i): byte o of
// thread t's range at 256 o + t, and the lanes of a wavefront that are at the same step of their ranges read neighbouring bytes.
// The rules name no layout: this changes no byte of the output.  KNOWN COST, not tuned: one thread builds the tree while the
// others wait.
__device__ __forceinline__ int at_lds(int i) { return ((i & (kPngOwn - 1)) << 8) | (i >> 7); }
static_assert(kPngOwn == 128 && kPngSegment == 256 * kPngOwn, "at_lds: 256 ranges of 128 bytes");
struct alignas(16) PngSeg {
    unsigned char byte[kPngSegment];
    unsigned short tok[kPngSegment];    // first where the parse leaves the owner's range from here; then the token: length | distance 3 << 15
    unsigned hist[288];                 // counts: 286 literal / length symbols, then distance 1 and distance 3
    unsigned work[286];                 // the counts as halved
    unsigned weight[571];               // leaves in order, then the joined nodes
    unsigned short parent[571];
    unsigned short leaf_sym[286];
    unsigned short code[286];           // bits reversed: as they go into the stream
    unsigned char depth[571];
    unsigned char len[286];
    unsigned short entry[256];          // where the parse enters each thread's range, 0xffff: nowhere
    unsigned scan[256];
    unsigned count[16], next[16];
    unsigned leaves, too_long, bits, sum_a, sum_b;
};

// rule 4 over the owner's bytes [lo, hi), backwards.  EXIT: tok[i] = where the parse that enters at i leaves [lo, hi); else the token
template <bool EXIT> __device__ __forceinline__ void match_pass(PngSeg& s, int lo, int hi, int n) {
    int c1 = 0, c3 = 0;             // M1 and M3 at hi
    if (hi < n) {                   // hi >= 128 here
        while (c1 < 258 && hi + c1 < n && s.byte[at_lds(hi + c1)] == s.byte[at_lds(hi + c1 - 1)]) ++c1;
        while (c3 < 258 && hi + c3 < n && s.byte[at_lds(hi + c3)] == s.byte[at_lds(hi + c3 - 3)]) ++c3;
    }
    for (int i = hi - 1; i >= lo; --i) {
        const int b = s.byte[at_lds(i)];
        c1 = (i >= 1 && b == s.byte[at_lds(i - 1)]) ? min(258, c1 + 1) : 0;
        c3 = (i >= 3 && b == s.byte[at_lds(i - 3)]) ? min(258, c3 + 1) : 0;
        const int best = max(c1, c3), len = best >= 3 ? best : 1;
        if (EXIT) s.tok[at_lds(i)] = (unsigned short)(i + len >= hi ? i + len : s.tok[at_lds(i + len)]);
        else s.tok[at_lds(i)] = (unsigned short)(len | ((best >= 3 && c3 > c1) ? 0x8000 : 0));
    }
}

__global__ void __launch_bounds__(256) png_segment_kernel(PngArgs a) {
    __shared__ PngSeg s;
    const int tid = threadIdx.x;
    const int pi = last_at_or_before(a.pics, a.n, blockIdx.x, &PngPic::seg0);
    const PngPic p = a.pics[pi];
    const int k = (int)blockIdx.x - p.seg0;
    const int n = (int)min((long long)kPngSegment, p.stream - (long long)k * kPngSegment);
    const bool last = k == p.nseg - 1;
    const int lo = tid * kPngOwn, hi = min(lo + kPngOwn, n);
    {   // a thread's own range into LDS, read as words: a stream begins at a multiple of 256 and its room is rounded up to one
        const unsigned* src = reinterpret_cast<const unsigned*>(a.filt + p.filt_off + (long long)k * kPngSegment) + tid * (kPngOwn / 4);
        for (int w = 0; w < kPngOwn / 4 && lo + 4 * w < n; ++w) {
            const unsigned v = src[w];
#pragma unroll
            for (int b = 0; b < 4; ++b) s.byte[at_lds(lo + 4 * w + b)] = (unsigned char)(v >> (8 * b));
        }
    }
    for (int i = tid; i < 288; i += 256) s.hist[i] = i == 256 ? 1u : 0u;
    s.entry[tid] = 0xffff;
    if (tid == 0) { s.bits = 0; s.sum_a = 0; s.sum_b = 0; }
    __syncthreads();
    {   // the Adler-32 partials; a thread's sums fit 32 bits (128 bytes of at most 255 (32768 - i))
        unsigned sa = 0, sb = 0;
        for (int i = lo; i < hi; ++i) { sa += s.byte[at_lds(i)]; sb += (unsigned)(n - i) * s.byte[at_lds(i)]; }
        atomicAdd(&s.sum_a, sa);
        atomicAdd(&s.sum_b, sb % 65521u);
    }
    match_pass<true>(s, lo, hi, n);
    __syncthreads();
    if (tid == 0) {
        int at = 0;
        for (int hop = 0; hop < 256 && at < n; ++hop) {
            s.entry[at / kPngOwn] = (unsigned short)at;
            at = s.tok[at_lds(at)];
        }
    }
    __syncthreads();
    match_pass<false>(s, lo, hi, n);
    const int enter = s.entry[tid];
    if (enter != 0xffff) {
        for (int i = enter, t = 0; i < hi && t < kPngOwn; ++t) {
            const int tk = s.tok[at_lds(i)], len = tk & 0x1ff;
            if (len == 1) {
                atomicAdd(&s.hist[s.byte[at_lds(i)]], 1u);
            } else {
                int e, v;
                atomicAdd(&s.hist[length_symbol(len, &e, &v)], 1u);
                atomicAdd(&s.hist[286 + (tk >> 15)], 1u);
            }
            i += len;
        }
    }
    __syncthreads();
    // rule 5
    for (int i = tid; i < 286; i += 256) s.work[i] = s.hist[i];
    for (int round = 0; round < 17; ++round) {          // 2^15 bytes at most: after 16 halvings every count is 1, a tree of depth 9
        if (tid == 0) s.leaves = 0;
        __syncthreads();
        for (int i = tid; i < 286; i += 256) {
            const unsigned f = s.work[i];
            s.len[i] = 0;
            if (!f) continue;
            int rank = 0;
            for (int j = 0; j < 286; ++j) {
                const unsigned g = s.work[j];
                rank += (g && (g < f || (g == f && j < i))) ? 1 : 0;
            }
            s.weight[rank] = f;
            s.leaf_sym[rank] = (unsigned short)i;
            atomicAdd(&s.leaves, 1u);
        }
        __syncthreads();
        if (tid == 0) {
            const int m = (int)s.leaves;                // >= 2: a segment's first byte is a literal, and the end-of-block
            int i = 0, j = m;
            for (int node = m; node < 2 * m - 1; ++node) {
                unsigned w = 0;
                for (int half = 0; half < 2; ++half) {
                    int pick;
                    if (i < m && (j >= node || s.weight[i] <= s.weight[j])) pick = i++; else pick = j++;
                    w += s.weight[pick];
                    s.parent[pick] = (unsigned short)node;
                }
                s.weight[node] = w;
            }
            s.depth[2 * m - 2] = 0;
            int deepest = 0;
            for (int x = 2 * m - 3; x >= 0; --x) {
                const int d = s.depth[s.parent[x]] + 1;
                s.depth[x] = (unsigned char)min(d, 255);
                if (x < m) {
                    deepest = max(deepest, d);
                    s.len[s.leaf_sym[x]] = (unsigned char)min(d, 255);
                }
            }
            s.too_long = deepest > 15;
        }
        __syncthreads();
        if (!s.too_long) break;                         // the same for every thread
        for (int i = tid; i < 286; i += 256) s.work[i] = (s.work[i] + 1) >> 1;
        __syncthreads();
    }
    // canonical codes, and the bits of the coded form
    if (tid < 16) s.count[tid] = 0;
    __syncthreads();
    for (int i = tid; i < 286; i += 256)
        if (s.len[i]) atomicAdd(&s.count[s.len[i]], 1u);
    __syncthreads();
    if (tid == 0) {
        unsigned code = 0;
        s.count[0] = 0;
        for (int b = 1; b < 16; ++b) {
            code = (code + s.count[b - 1]) << 1;
            s.next[b] = code;
        }
    }
    __syncthreads();
    for (int i = tid; i < 286; i += 256) {
        const int l = s.len[i];
        if (!l) { s.code[i] = 0; continue; }
        unsigned c = s.next[l];
        for (int j = 0; j < i; ++j) c += s.len[j] == l ? 1u : 0u;
        s.code[i] = (unsigned short)(__brev(c) >> (32 - l));
        atomicAdd(&s.bits, s.hist[i] * (unsigned)(l + symbol_extra(i)));
    }
    __syncthreads();
    const unsigned body = s.bits - s.len[256] + s.hist[286] + s.hist[287];             // the tokens' bits, without the end-of-block
    const unsigned coded = ((kPngHeaderBits + body + s.len[256] + 3 + 7) >> 3) + 4;   // rule 7
    const bool stored = coded >= (unsigned)n + 5u;
    unsigned* out = a.segbuf + (size_t)blockIdx.x * (kPngSegStride / 4);
    if (tid == 0) {
        a.seg_bytes[blockIdx.x] = stored ? (unsigned)n + 5u : coded;
        a.seg_sum[2 * blockIdx.x] = s.sum_a;
        a.seg_sum[2 * blockIdx.x + 1] = s.sum_b % 65521u;
    }
    if (stored) {
        unsigned char* o = reinterpret_cast<unsigned char*>(out);
        if (tid == 0) {
            o[0] = last ? 1 : 0;
            o[1] = (unsigned char)(n & 255); o[2] = (unsigned char)(n >> 8);
            o[3] = (unsigned char)(~n & 255); o[4] = (unsigned char)((~n >> 8) & 255);
        }
        for (int i = tid; i < n; i += 256) o[5 + i] = s.byte[at_lds(i)];
        return;
    }
    // rule 6: the header.  BFINAL 0, BTYPE 2, HLIT 29, HDIST 2, HCLEN 15: 17 bits; the 19 code-length lengths in the order 16 17 18 0 8 ...
    if (tid == 0) {
        or_bits(out, 0, 0u | 2u << 1 | 29u << 3 | 2u << 8 | 15u << 13, 17);
        for (int j = 3; j < 19; ++j) or_bits(out, 17 + 3 * j, 4u, 3);       // 16, 17, 18 stay 0; the sixteen others are 4 bits long
    }
    const bool d1 = s.hist[286] != 0, d3 = s.hist[287] != 0;
    for (int i = tid; i < 289; i += 256) {
        const unsigned l = i < 286 ? s.len[i] : (i == 286 ? (d1 ? 1u : 0u) : (i == 288 ? (d3 ? 1u : 0u) : 0u));
        or_bits(out, 74 + 4 * i, __brev(l) >> 28, 4);
    }
    // the tokens: what each thread's cost, a scan, then the bits
    const unsigned code3 = d1 ? 1u : 0u;
    unsigned mine = 0;
    if (enter != 0xffff) {
        for (int i = enter, t = 0; i < hi && t < kPngOwn; ++t) {
            const int tk = s.tok[at_lds(i)], len = tk & 0x1ff;
            if (len == 1) {
                mine += s.len[s.byte[at_lds(i)]];
            } else {
                int e, v;
                mine += s.len[length_symbol(len, &e, &v)] + e + 1;
            }
            i += len;
        }
    }
    unsigned total;
    const unsigned first = block_scan(mine, s.scan, &total);
    if (enter != 0xffff) {
        BitWriter bw(out, kPngHeaderBits + first);
        for (int i = enter, t = 0; i < hi && t < kPngOwn; ++t) {
            const int tk = s.tok[at_lds(i)], len = tk & 0x1ff;
            if (len == 1) {
                const int b = s.byte[at_lds(i)];
                bw.put(s.code[b], s.len[b]);
            } else {
                int e, v;
                const int sym = length_symbol(len, &e, &v), l = s.len[sym];
                bw.put((unsigned)s.code[sym] | (unsigned)v << l | ((tk >> 15) ? code3 : 0u) << (l + e), l + e + 1);
            }
            i += len;
        }
        bw.flush();
    }
    if (tid == 0) {
        const unsigned at = kPngHeaderBits + body;          // == kPngHeaderBits + total
        or_bits(out, at, s.code[256], s.len[256]);
        or_bits(out, at + s.len[256], last ? 1u : 0u, 3);
        or_bits(out, 8 * (coded - 2), 0xffffu, 16);
    }
}

// one workgroup per picture: where each segment's blocks go, the file's length, the Adler-32 of the filtered stream
__global__ void __launch_bounds__(256) png_scan_kernel(PngArgs a) {
    __shared__ unsigned long long scan[256];
    const int pi = blockIdx.x;
    const PngPic p = a.pics[pi];
    unsigned long long bytes = 0, sum_a = 0, s2 = 0;
    for (int c = 0; c < p.nseg; c += 256) {                     // uniform trip count: the barriers of block_scan are safe
        const int k = c + (int)threadIdx.x;
        const bool live = k < p.nseg;
        unsigned long long total;
        const unsigned long long before = block_scan(live ? (unsigned long long)a.seg_bytes[p.seg0 + k] : 0ull, scan, &total);
        if (live) a.seg_base[p.seg0 + k] = bytes + before;
        bytes += total;
        const unsigned long long sa = live ? a.seg_sum[2 * (p.seg0 + k)] : 0ull;
        const unsigned long long a_before = block_scan(sa, scan, &total);
        // Adler-32: with s1 = P in front of a segment of n bytes, s2 grows by n P + sum (n - i) byte[i]
        unsigned long long term = 0;
        if (live) {
            const unsigned long long n = min((long long)kPngSegment, p.stream - (long long)k * kPngSegment);
            term = n * ((1ull + sum_a + a_before) % 65521ull) + a.seg_sum[2 * (p.seg0 + k) + 1];
        }
        sum_a += total;
        block_scan(term, scan, &total);
        s2 += total;
    }
    if (threadIdx.x == 0) {
        a.pic_adler[pi] = (unsigned)(s2 % 65521ull) << 16 | (unsigned)((1ull + sum_a) % 65521ull);
        a.sizes[pi] = (long long)(kPngOverhead + bytes);
    }
}

// one workgroup per segment: its blocks into the file, and their share of IDAT's CRC
__global__ void __launch_bounds__(256) png_pack_kernel(PngArgs a) {
    __shared__ unsigned table[256];
    __shared__ unsigned share;
    const int tid = threadIdx.x;
    const int pi = last_at_or_before(a.pics, a.n, blockIdx.x, &PngPic::seg0);
    const PngPic p = a.pics[pi];
    {
        unsigned c = (unsigned)tid;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        table[tid] = c;
    }
    if (tid == 0) share = 0;
    __syncthreads();
    const unsigned char* src = reinterpret_cast<const unsigned char*>(a.segbuf + (size_t)blockIdx.x * (kPngSegStride / 4));
    const int nb = (int)a.seg_bytes[blockIdx.x];
    const long long at = kPngHeaderBytes + 10 + (long long)a.seg_base[blockIdx.x];      // behind IDAT's length and type and 78 01
    unsigned char* out = a.out + p.out_off;
    for (int i = tid; i < nb; i += 256)
        if (at + i < p.cap) out[at + i] = src[i];
    // the CRC with register 0 of the bytes [nb - 132 (tid + 1), nb - 132 tid): zeros in front of them do not change it
    constexpr int kPer = 132;                           // 256 x 132 >= 32768 + 5
    unsigned c = 0;
    const int end = nb - kPer * tid;
    for (int i = max(end - kPer, 0); i < end; ++i) c = table[(c ^ src[i]) & 255] ^ (c >> 8);
    if (c) atomicXor(&share, gf_mul(c, gf_xpow8((unsigned long long)kPer * tid)));
    __syncthreads();
    if (tid == 0) {
        const long long behind = a.sizes[pi] - 16 - (at + nb);          // to the end of IDAT's data: the Adler-32 is part of it
        a.seg_crc[blockIdx.x] = gf_mul(share, gf_xpow8((unsigned long long)behind));
    }
}

// one workgroup per picture: everything around the blocks
__global__ void __launch_bounds__(256) png_finish_kernel(PngArgs a) {
    __shared__ unsigned share;
    __shared__ unsigned char head[kPngHeaderBytes + 10], tail[20];
    const int pi = blockIdx.x;
    const PngPic p = a.pics[pi];
    if (threadIdx.x == 0) share = 0;
    __syncthreads();
    unsigned c = 0;
    for (int k = threadIdx.x; k < p.nseg; k += 256) c ^= a.seg_crc[p.seg0 + k];
    if (c) atomicXor(&share, c);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long size = a.sizes[pi], zlen = size - (kPngOverhead - 6);       // IDAT's data: 78 01, the blocks, the Adler-32
    unsigned char* out = a.out + p.out_off;
    header33(p.H, p.W, head);
    put_be32(head + 33, (unsigned)zlen);
    head[37] = 'I'; head[38] = 'D'; head[39] = 'A'; head[40] = 'T'; head[41] = 0x78; head[42] = 0x01;
    for (int i = 0; i < kPngHeaderBytes + 10; ++i) out[i] = head[i];       // the capacity holds it (checked by the host)
    // IDAT's CRC: the register after "IDAT" 78 01, carried over the zlen - 2 bytes behind them, joined with the blocks' and the Adler's shares
    const unsigned adler = a.pic_adler[pi];
    unsigned reg = crc_std(head + 37, 6) ^ 0xffffffffu;
    reg = gf_mul(reg, gf_xpow8((unsigned long long)(zlen - 2))) ^ share;
    put_be32(tail, adler);
    unsigned ac = 0;
    for (int i = 0; i < 4; ++i) ac = crc_byte(ac, tail[i]);
    put_be32(tail + 4, reg ^ ac ^ 0xffffffffu);
    const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) tail[8 + i] = iend[i];
    for (int i = 0; i < 20; ++i)
        if (size - 20 + i < p.cap) out[size - 20 + i] = tail[i];
}

}  // namespace

long long png_bound(int H, int W) {
    const long long L = (long long)H * (1 + 3LL * W);
    return kPngOverhead + L + 5 * ((L + kPngSegment - 1) / kPngSegment);
}

void png_header(int H, int W, unsigned char* out) { header33(H, W, out); }

size_t png_ws_layout(int n, long long filt_bytes, long long segs, size_t off[7]) {
    const size_t sizes[7] = {(size_t)filt_bytes, (size_t)segs * kPngSegStride, (size_t)segs * 4, (size_t)segs * 8, (size_t)segs * 8,
                             (size_t)segs * 4, (size_t)n * 4};
    size_t at = 0;
    for (int i = 0; i < 7; ++i) {
        off[i] = at;
        at += (sizes[i] + 255) & ~(size_t)255;
    }
    return at;
}

int launch_png_encode(const PngArgs& a, double in_bytes, const LaunchCtx& ctx) {
    const double blocks = (double)a.segs * kPngSegStride;
    {
        ProfScope ps(ctx, "png_zero", 0.0, blocks);
        if (hipError_t e = hipMemsetAsync(a.segbuf, 0, (size_t)a.segs * kPngSegStride, ctx.stream)) return (int)e;
    }
    {
        ProfScope ps(ctx, "png_filter", 0.0, 2.0 * in_bytes);
        hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)a.rows < kPngFilterGrid ? (unsigned)a.rows : kPngFilterGrid), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "png_segment", 0.0, in_bytes + blocks);
        hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)a.segs), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "png_scan", 0.0, (double)a.segs * 20);
        hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)a.n), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "png_pack", 0.0, 2.0 * blocks);
        hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)a.segs), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "png_finish", 0.0, (double)a.segs * 4);
        hipLaunchKernelGGL(png_finish_kernel, dim3((unsigned)a.n), dim3(256), 0, ctx.stream, a);
    }
    return (int)hipGetLastError();
}

}  // namespace specmi

extern "C" int specmi_png_bound(int H, int W, int64_t* bytes) {
    if (!bytes || H < 1 || H > 32768 || W < 1 || W > 32768) return SPECMI_ERR_ARG;
    *bytes = specmi::png_bound(H, W);
    return SPECMI_OK;
}

extern "C" int specmi_png_header(int H, int W, uint8_t* out, size_t capacity) {
    if (!out || H < 1 || H > 32768 || W < 1 || W > 32768 || capacity < (size_t)specmi::kPngHeaderBytes) return SPECMI_ERR_ARG;
    specmi::png_header(H, W, out);
    return SPECMI_OK;
}
