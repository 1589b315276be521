// jpeg.hip - baseline JPEG files encoded on the device from uint8 RGB rectangles of a slab: what the
// reference hands to cv2.imwrite / PIL's save for every picture it writes (spec/utils/renderer_cam.py:213-216,
// spec/tester.py:188-201, camcalib/datagen/generateCalibrationDataset.py:131-132), for all pictures of a flush in one fixed
// sequence of launches, so that the encoded bytes come down instead of the raw pictures.
//
// THE CONTRACT.  For an (H, W, 3) picture and a quality q in 1 .. 100 the output is, byte for byte, what
//   PIL.Image.fromarray(a).save(f, format='JPEG', quality=q, optimize=False, progressive=False)
// writes on a libjpeg-turbo build of Pillow: baseline sequential, 4:2:0, the Annex-K Huffman tables of ITU-T T.81, no restart
// markers (tests/jpeg_ref.py restates it in NumPy).  The rules are libjpeg's:
// 1. Colour.  16-bit fixed point, F(x) = int(x 65536 + 0.5):  Y = (F(.299) R + F(.587) G + F(.114) B + 32768) >> 16,
//    Cb = (-F(.16874) R - F(.33126) G + F(.5) B + (128 << 16) + 32767) >> 16,
//    Cr = (F(.5) R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16.
// 2. Edges.  Every plane is extended to the right by repeating its last column up to W rounded up to 16.  Y is extended
//    downwards by repeating its last row.  The chroma SOURCE is extended by one repeated row only when H is odd; then it is
//    downsampled, and the DOWNSAMPLED rows are repeated to the bottom (not the same thing as downsampling repeated rows).
// 3. Chroma.  h2v2: (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... along the output columns, starting at 1 in every row.
// 4. DCT.  libjpeg's jfdctint ("islow") on samples minus 128: CONST_BITS 13, PASS1_BITS 2, rows then columns, outputs scaled
//    by 8; DESCALE(x, n) = (x + (1 << (n - 1))) >> n with an arithmetic shift.
// 5. Quantisation by qv = 8 Q[k]:  sign(c) ((|c| + (qv >> 1)) / qv).
// 6. Dummy blocks (Y only at 4:2:0): a Y block of an MCU whose column is >= ceil(W / 8) or whose row is >= ceil(H / 8) is not
//    transformed.  Its AC is 0, its DC the quantised DC of the block before it in MCU order (the left neighbour; for the second
//    block row the last block of the first), and it takes part in DC prediction like any block.  The DC that jfdctint gives is
//    the plain sum of the block's 64 samples minus 128 (<< 2 in pass 1, DESCALE by 2 in pass 2), so a dummy block's thread sums
//    the REAL block its chain ends in and quantises that: no thread waits for another.
// 7. Scan.  MCUs in raster order, blocks Y00 Y01 Y10 Y11 Cb Cr.  Per block the DC difference against the previous block of the
//    same component as a category code plus the value bits (v, or v + 2^s - 1 when negative); then the AC coefficients in zigzag
//    order as (run, size) codes, 0xF0 for each 16 zeros ahead of a non-zero coefficient, 0x00 when the block ends in zeros.  Bits
//    are packed MSB first, a 0x00 follows every 0xFF data byte, the last byte is filled with 1 bits (and stuffed like any other),
//    then FF D9.
// 8. Header, 623 bytes: SOI; APP0 JFIF 1.01, units 0, density 1 x 1, no thumbnail; two DQT (tables 0 and 1, zigzag order); SOF0
//    (8 bits, H, W, components 1 / 2 / 3 sampling 0x22 / 0x11 / 0x11, tables 0 / 1 / 1); four DHT (DC0, AC0, DC1, AC1); SOS.
// 9. Tables.  jpeg_set_quality(q, force_baseline) on the Annex-K base tables: scale = 5000 / q below 50, else 200 - 2 q;
//    entry = (base scale + 50) / 100 clamped to 1 .. 255.
//
// STAGES - one memset and seven launches, whatever the number of pictures and their sizes.  The pictures' MCUs (16 x 16 pixels)
// are numbered back to back; a picture's MCUs are cut into chunks of 256 and its unstuffed scan into chunks of 4096 bytes (as many
// as its worst case needs: the grid cannot wait for the device to know the length), and a workgroup finds its picture by
// bisecting the chunk prefix of the record table, as the other ragged kernels do.
//   dct     one thread per block: colour conversion, downsample, DCT, quantisation -> int16 coefficients in zigzag order
//   count   one thread per MCU: the bits its six blocks code into (the DC predictor is the previous block's coefficient, in
//           memory already), and the sum per chunk
//   scan    one workgroup per picture: exclusive scan of its chunk sums (64-bit) -> each chunk's first bit, the picture's bits
//   write   one thread per MCU: its bits at its offset, into zeroed big-endian 32-bit words joined with atomicOr - an integer OR
//           of disjoint bits, so the result does not depend on the order
//   ffcount one thread per 16 scan bytes: the 0xFF bytes per byte chunk (the fill bits are applied on the fly)
//   scan    the same kernel on those counts -> each byte chunk's stuffed zeros before it, and sizes[] = 623 + bytes + 0xFF's + 2
//   pack    the scan bytes behind the header, a zero behind every 0xFF; the first chunk of a picture writes header and EOI.
//           Nothing is written at or beyond a picture's capacity.
// WORKSPACE, one per handle, grown under the rule of the ragged calls: per MCU 768 bytes of coefficients, 1248 bytes of scan (its
// worst case: 6 blocks of 22 + 63 x 26 bits) and 4 of bit count, i.e. 7.9 bytes per pixel of the pictures rounded up to whole MCUs,
// plus 12 bytes per chunk and 8 per picture.
#include "specmi_internal.h"

namespace specmi {

namespace {

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- host half: what a quality decides ----------------------------------------------------------------------------------------
const unsigned char kQLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                                  69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                                  81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                    99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const unsigned char kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const unsigned char kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// Annex C: canonical codes from BITS and HUFFVAL, stored by symbol
void huff_by_symbol(const unsigned char* bits, const unsigned char* vals, unsigned short* code, unsigned char* len) {
    unsigned c = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++c) {
            code[vals[k]] = (unsigned short)c;
            len[vals[k]] = (unsigned char)l;
        }
        c <<= 1;
    }
}

unsigned char* put_segment(unsigned char* p, int marker, const unsigned char* body, int n) {
    *p++ = 0xFF; *p++ = (unsigned char)marker;
    *p++ = (unsigned char)((n + 2) >> 8); *p++ = (unsigned char)((n + 2) & 255);
    std::memcpy(p, body, (size_t)n);
    return p + n;
}

}  // namespace

void jpeg_build_tables(int quality, JpegTables* t) {
    std::memset(t, 0, sizeof(*t));
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    unsigned char q[2][64];
    for (int i = 0; i < 64; ++i) {
        const int base[2] = {kQLuma[i], kQChroma[i]};
        for (int k = 0; k < 2; ++k) {
            int v = (base[k] * scale + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            q[k][i] = (unsigned char)v;
            t->div[k][i] = (unsigned short)(8 * v);
        }
    }
    unsigned char dc_vals[12];
    for (int i = 0; i < 12; ++i) dc_vals[i] = (unsigned char)i;
    for (int k = 0; k < 2; ++k) {
        huff_by_symbol(kDcBits[k], dc_vals, t->dc_code[k], t->dc_len[k]);
        huff_by_symbol(kAcBits[k], kAcVals[k], t->ac_code[k], t->ac_len[k]);
    }
    unsigned char* p = t->header;
    *p++ = 0xFF; *p++ = 0xD8;
    const unsigned char app0[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    p = put_segment(p, 0xE0, app0, 14);
    for (int k = 0; k < 2; ++k) {
        unsigned char body[65];
        body[0] = (unsigned char)k;
        for (int i = 0; i < 64; ++i) body[1 + i] = q[k][kZigzag[i]];
        p = put_segment(p, 0xDB, body, 65);
    }
    const unsigned char sof[15] = {8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};     // H and W (bytes 1 .. 4) per picture
    p = put_segment(p, 0xC0, sof, 15);
    for (int k = 0; k < 2; ++k) {
        unsigned char body[1 + 16 + 162];
        body[0] = (unsigned char)k;
        std::memcpy(body + 1, kDcBits[k], 16);
        std::memcpy(body + 17, dc_vals, 12);
        p = put_segment(p, 0xC4, body, 29);
        body[0] = (unsigned char)(0x10 | k);
        std::memcpy(body + 1, kAcBits[k], 16);
        std::memcpy(body + 17, kAcVals[k], 162);
        p = put_segment(p, 0xC4, body, 179);
    }
    const unsigned char sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    p = put_segment(p, 0xDA, sos, 10);
    static_assert(2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14 == kJpegHeaderBytes, "the header's length");
}

constexpr int kJpegSofSize = 2 + 18 + 2 * 69 + 5;      // where H (2 bytes, big-endian) and then W stand in the header

// ---- device half ------------------------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ int luma(const unsigned char* px) {
    return (fix16(.299) * px[0] + fix16(.587) * px[1] + fix16(.114) * px[2] + 32768) >> 16;
}
template <bool CR> __device__ __forceinline__ int chroma(const unsigned char* px) {
    return CR ? (fix16(.5) * px[0] - fix16(.41869) * px[1] - fix16(.08131) * px[2] + (128 << 16) + 32767) >> 16
              : (-fix16(.16874) * px[0] - fix16(.33126) * px[1] + fix16(.5) * px[2] + (128 << 16) + 32767) >> 16;
}

// the 64 samples minus 128 of a chroma block of MCU (mcx, mcy): rules 2 and 3
template <bool CR> __device__ __forceinline__ void load_chroma(const unsigned char* base, const JpegPic& p, int mcx, int mcy, int (&v)[64]) {
    const int Hc = (p.H + 1) >> 1;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int cy = min(mcy * 8 + r, Hc - 1);
        const unsigned char* r0 = base + (long long)(2 * cy) * p.in_pitch;
        const unsigned char* r1 = base + (long long)min(2 * cy + 1, p.H - 1) * p.in_pitch;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int cx = mcx * 8 + c;
            const int x0 = 3 * min(2 * cx, p.W - 1), x1 = 3 * min(2 * cx + 1, p.W - 1);
            const int s = chroma<CR>(r0 + x0) + chroma<CR>(r0 + x1) + chroma<CR>(r1 + x0) + chroma<CR>(r1 + x1);
            v[8 * r + c] = ((s + 1 + (c & 1)) >> 2) - 128;
        }
    }
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint over eight values
template <bool FIRST> __device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d0 = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d4 = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d2 = descale(z1 + t13 * 6270, N);
    d6 = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d7 = descale(t4 + z1 + z3, N);
    d5 = descale(t5 + z2 + z4, N);
    d3 = descale(t6 + z2 + z3, N);
    d1 = descale(t7 + z1 + z4, N);
}

__device__ __forceinline__ int quantise(int c, int qv) {
    const int q = (int)(((unsigned)abs(c) + ((unsigned)qv >> 1)) / (unsigned)qv);
    return c < 0 ? -q : q;
}

__global__ void __launch_bounds__(256) jpeg_dct_kernel(JpegArgs a) {
    const int chunk = blockIdx.x / 6, b = blockIdx.x % 6;      // the whole workgroup works on one kind of block
    const int pi = last_at_or_before(a.pics, a.n, chunk, &JpegPic::mchunk0);
    const JpegPic p = a.pics[pi];
    const int m = (chunk - p.mchunk0) * kJpegMcuChunk + (int)threadIdx.x;
    if (m >= p.mx * p.my) return;
    const int mcy = m / p.mx, mcx = m - mcy * p.mx;
    const unsigned char* base = a.in + p.in_off;
    int v[64];
    bool dummy = false;
    if (b < 4) {
        const int wb = (p.W + 7) >> 3, hb = (p.H + 7) >> 3;
        int bx = 2 * mcx + (b & 1), by = 2 * mcy + (b >> 1);
        if (by >= hb) {             // rule 6: the chain ends in the last real block of the MCU's first block row
            dummy = true;
            by -= 1;
            bx = 2 * mcx + 1 < wb ? 2 * mcx + 1 : 2 * mcx;
        } else if (bx >= wb) {
            dummy = true;
            bx -= 1;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned char* row = base + (long long)min(by * 8 + r, p.H - 1) * p.in_pitch;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[8 * r + c] = luma(row + 3 * min(bx * 8 + c, p.W - 1)) - 128;
        }
    } else if (b == 4) {
        load_chroma<false>(base, p, mcx, mcy, v);
    } else {
        load_chroma<true>(base, p, mcx, mcy, v);
    }
    const unsigned short* div = a.tabs->div[b >= 4];
    unsigned w[32];
    if (dummy) {
        int s = 0;
#pragma unroll
        for (int i = 0; i < 64; ++i) s += v[i];
#pragma unroll
        for (int i = 0; i < 32; ++i) w[i] = 0;
        w[0] = (unsigned)quantise(s, div[0]) & 0xffffu;
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r)
            fdct8<true>(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7]);
#pragma unroll
        for (int c = 0; c < 8; ++c) fdct8<false>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
        for (int i = 0; i < 64; ++i) v[i] = quantise(v[i], div[i]);
#pragma unroll
        for (int i = 0; i < 32; ++i)
            w[i] = ((unsigned)v[kZigzag[2 * i]] & 0xffffu) | ((unsigned)v[kZigzag[2 * i + 1]] << 16);
    }
    uint4* out = reinterpret_cast<uint4*>(a.coef + ((size_t)(p.mcu0 + m) * 6 + b) * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// the code tables in LDS
struct JpegCodes {
    unsigned short dc_code[2][12];
    unsigned char dc_len[2][12];
    unsigned short ac_code[2][256];
    unsigned char ac_len[2][256];
};

__device__ __forceinline__ void load_codes(JpegCodes& s, const JpegTables* t) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) {
        (&s.ac_code[0][0])[i] = (&t->ac_code[0][0])[i];
        (&s.ac_len[0][0])[i] = (&t->ac_len[0][0])[i];
    }
    if (threadIdx.x < 24) {
        (&s.dc_code[0][0])[threadIdx.x] = (&t->dc_code[0][0])[threadIdx.x];
        (&s.dc_len[0][0])[threadIdx.x] = (&t->dc_len[0][0])[threadIdx.x];
    }
    __syncthreads();
}

// bits appended MSB first to a stream of big-endian 32-bit words that starts out zero; a word may be shared with a neighbour,
// so every word is joined with atomicOr
struct BitWriter {
    unsigned* word;
    unsigned long long acc;
    int fill;                   // bits of acc that belong to *word, 0 .. 31
    __device__ __forceinline__ BitWriter(unsigned* buf, unsigned long long bit) : word(buf + (bit >> 5)), acc(0), fill((int)(bit & 31)) {}
    __device__ __forceinline__ void put(unsigned v, int len) {          // len <= 32: acc holds at most 31 + 32 bits
        acc = (acc << len) | v;
        fill += len;
        if (fill >= 32) {
            fill -= 32;
            atomicOr(word++, (unsigned)(acc >> fill));
            acc &= (1ull << fill) - 1ull;
        }
    }
    __device__ __forceinline__ void flush() {
        if (fill) atomicOr(word, (unsigned)(acc << (32 - fill)));
    }
};

__device__ __forceinline__ int category(int v) { return 32 - __clz(abs(v)); }      // 0 for 0
__device__ __forceinline__ unsigned value_bits(int v, int s) { return (unsigned)(v < 0 ? v + (1 << s) - 1 : v); }

// rule 7 for one block: its 64 coefficients as eight uint4 at `blk`, the predictor `pred`, table t -> the bits it takes; WRITE: emitted
template <bool WRITE> __device__ __forceinline__ int code_block(const uint4* blk, int pred, int t, const JpegCodes& s, BitWriter* bw, int* dc_out) {
    int bits = 0, run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 q = blk[g];
        const unsigned ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(short)(j & 1 ? ws[j >> 1] >> 16 : ws[j >> 1] & 0xffffu);
            if (g == 0 && j == 0) {
                const int diff = c - pred, n = category(diff);
                *dc_out = c;
                bits += s.dc_len[t][n] + n;
                if (WRITE) bw->put((unsigned)s.dc_code[t][n] << n | value_bits(diff, n), s.dc_len[t][n] + n);
            } else if (c == 0) {
                ++run;
            } else {
                while (run > 15) {
                    bits += s.ac_len[t][0xF0];
                    if (WRITE) bw->put(s.ac_code[t][0xF0], s.ac_len[t][0xF0]);
                    run -= 16;
                }
                const int n = category(c), sym = run << 4 | n;
                bits += s.ac_len[t][sym] + n;
                if (WRITE) bw->put((unsigned)s.ac_code[t][sym] << n | value_bits(c, n), s.ac_len[t][sym] + n);
                run = 0;
            }
        }
    }
    if (run) {
        bits += s.ac_len[t][0];
        if (WRITE) bw->put(s.ac_code[t][0], s.ac_len[t][0]);
    }
    return bits;
}

// the six blocks of MCU m (>= 0) of its picture, global MCU g
template <bool WRITE> __device__ __forceinline__ int code_mcu(const short* coef, int g, int m, const JpegCodes& s, BitWriter* bw) {
    const uint4* blk = reinterpret_cast<const uint4*>(coef + (size_t)g * 384);
    int pred[3] = {0, 0, 0};
    if (m > 0) {
        const short* prev = coef + (size_t)(g - 1) * 384;
        pred[0] = prev[3 * 64]; pred[1] = prev[4 * 64]; pred[2] = prev[5 * 64];
    }
    int bits = 0;
#pragma unroll 1
    for (int b = 0; b < 6; ++b) {
        const int comp = b < 4 ? 0 : b - 3;
        int dc;
        bits += code_block<WRITE>(blk + 8 * b, comp == 0 ? pred[0] : (comp == 1 ? pred[1] : pred[2]), b >= 4, s, bw, &dc);
        if (comp == 0) pred[0] = dc; else if (comp == 1) pred[1] = dc; else pred[2] = dc;
    }
    return bits;
}

__global__ void __launch_bounds__(256) jpeg_count_kernel(JpegArgs a) {
    __shared__ JpegCodes s;
    __shared__ unsigned scan[256];
    load_codes(s, a.tabs);
    const int pi = last_at_or_before(a.pics, a.n, blockIdx.x, &JpegPic::mchunk0);
    const JpegPic p = a.pics[pi];
    const int m = ((int)blockIdx.x - p.mchunk0) * kJpegMcuChunk + (int)threadIdx.x;
    unsigned bits = 0;
    if (m < p.mx * p.my) {
        bits = (unsigned)code_mcu<false>(a.coef, p.mcu0 + m, m, s, nullptr);
        a.mcu_bits[p.mcu0 + m] = bits;
    }
    unsigned total;
    block_scan(bits, scan, &total);
    if (threadIdx.x == 0) a.mchunk_sum[blockIdx.x] = total;
}

// one workgroup per picture: exclusive 64-bit scan of the sums of its chunks.  BYTES false: the MCU chunks' bits -> mchunk_base and
// pic_bits; true: the byte chunks' 0xFF counts -> bchunk_base and sizes
template <bool BYTES> __global__ void __launch_bounds__(256) jpeg_scan_kernel(JpegArgs a) {
    __shared__ unsigned long long scan[256];
    const int pi = blockIdx.x;
    const int c0 = BYTES ? a.pics[pi].bchunk0 : a.pics[pi].mchunk0;
    const int c1 = pi + 1 < a.n ? (BYTES ? a.pics[pi + 1].bchunk0 : a.pics[pi + 1].mchunk0) : (BYTES ? a.bchunks : a.mchunks);
    const unsigned* sum = BYTES ? a.bchunk_ff : a.mchunk_sum;
    unsigned long long* base = BYTES ? a.bchunk_base : a.mchunk_base;
    unsigned long long running = 0;
    for (int c = c0; c < c1; c += 256) {                        // uniform trip count: the barriers of block_scan are safe
        const int i = c + (int)threadIdx.x;
        const unsigned long long v = i < c1 ? sum[i] : 0ull;
        unsigned long long total;
        const unsigned long long excl = block_scan(v, scan, &total);
        if (i < c1) base[i] = running + excl;
        running += total;
    }
    if (threadIdx.x == 0) {
        if (BYTES) a.sizes[pi] = (long long)(kJpegHeaderBytes + ((a.pic_bits[pi] + 7) >> 3) + running + 2);
        else a.pic_bits[pi] = running;
    }
}

__global__ void __launch_bounds__(256) jpeg_write_kernel(JpegArgs a) {
    __shared__ JpegCodes s;
    __shared__ unsigned scan[256];
    load_codes(s, a.tabs);
    const int pi = last_at_or_before(a.pics, a.n, blockIdx.x, &JpegPic::mchunk0);
    const JpegPic p = a.pics[pi];
    const int m = ((int)blockIdx.x - p.mchunk0) * kJpegMcuChunk + (int)threadIdx.x;
    const bool live = m < p.mx * p.my;
    unsigned total;
    const unsigned first = block_scan(live ? a.mcu_bits[p.mcu0 + m] : 0u, scan, &total);
    if (!live) return;
    BitWriter bw(a.bitbuf + (size_t)p.mcu0 * (kJpegMcuBytes / 4), a.mchunk_base[blockIdx.x] + first);
    code_mcu<true>(a.coef, p.mcu0 + m, m, s, &bw);
    bw.flush();
}

// the 16 scan bytes from byte i0 (a multiple of 16) of a picture's unstuffed scan of nbytes bytes / bits bits, the fill bits
// applied; -> how many of them exist
__device__ __forceinline__ int scan_bytes16(const unsigned* buf, long long i0, long long nbytes, unsigned long long bits, unsigned char (&o)[16]) {
    if (i0 >= nbytes) return 0;
    const uint4 q = *reinterpret_cast<const uint4*>(buf + (i0 >> 2));
    const unsigned ws[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) o[k] = (unsigned char)(ws[k >> 2] >> (24 - 8 * (k & 3)));
    const int n = (int)min(16ll, nbytes - i0);
    if ((bits & 7) && i0 + n == nbytes) {
        const unsigned char fillbits = (unsigned char)(0xFFu >> (bits & 7));
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k == n - 1) o[k] |= fillbits;
    }
    return n;
}

template <bool PACK> __global__ void __launch_bounds__(256) jpeg_stuff_kernel(JpegArgs a) {
    __shared__ unsigned scan[256];
    const int pi = last_at_or_before(a.pics, a.n, blockIdx.x, &JpegPic::bchunk0);
    const JpegPic p = a.pics[pi];
    const int j = (int)blockIdx.x - p.bchunk0;
    const unsigned long long bits = a.pic_bits[pi];
    const long long nbytes = (long long)((bits + 7) >> 3);
    const long long i0 = (long long)j * kJpegByteChunk + 16 * (long long)threadIdx.x;
    unsigned char o[16];
    const int n = scan_bytes16(a.bitbuf + (size_t)p.mcu0 * (kJpegMcuBytes / 4), i0, nbytes, bits, o);
    unsigned ff = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) ff += (k < n && o[k] == 0xFF) ? 1u : 0u;
    unsigned total;
    const unsigned first = block_scan(ff, scan, &total);
    if (!PACK) {
        if (threadIdx.x == 0) a.bchunk_ff[blockIdx.x] = total;
        return;
    }
    unsigned char* out = a.out + p.out_off;
    if (j == 0) {               // header and EOI; the capacity holds the header (checked by the host)
        for (int i = threadIdx.x; i < kJpegHeaderBytes; i += 256) {
            unsigned char c = a.tabs->header[i];
            if (i == kJpegSofSize) c = (unsigned char)(p.H >> 8);
            if (i == kJpegSofSize + 1) c = (unsigned char)(p.H & 255);
            if (i == kJpegSofSize + 2) c = (unsigned char)(p.W >> 8);
            if (i == kJpegSofSize + 3) c = (unsigned char)(p.W & 255);
            out[i] = c;
        }
        if (threadIdx.x == 0) {
            const long long size = a.sizes[pi];
            if (size - 2 < p.cap) out[size - 2] = 0xFF;
            if (size - 1 < p.cap) out[size - 1] = 0xD9;
        }
    }
    long long dst = kJpegHeaderBytes + i0 + (long long)(a.bchunk_base[blockIdx.x] + first);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k >= n) break;
        if (dst < p.cap) out[dst] = o[k];
        ++dst;
        if (o[k] == 0xFF) {
            if (dst < p.cap) out[dst] = 0;
            ++dst;
        }
    }
}

}  // namespace

size_t jpeg_ws_layout(int n, long long mcus, long long mchunks, long long bchunks, size_t off[8]) {
    const size_t sizes[8] = {(size_t)mcus * 768, (size_t)mcus * 4, (size_t)mchunks * 4, (size_t)mchunks * 8, (size_t)n * 8,
                             (size_t)mcus * kJpegMcuBytes, (size_t)bchunks * 4, (size_t)bchunks * 8};
    size_t at = 0;
    for (int i = 0; i < 8; ++i) {
        off[i] = at;
        at += (sizes[i] + 255) & ~(size_t)255;
    }
    return at;
}

int launch_jpeg_encode(const JpegArgs& a, double in_bytes, const LaunchCtx& ctx) {
    const double coef = (double)a.mcus * 768, scan = (double)a.mcus * kJpegMcuBytes;
    {
        ProfScope ps(ctx, "jpeg_zero", 0.0, scan);
        if (hipError_t e = hipMemsetAsync(a.bitbuf, 0, (size_t)a.mcus * kJpegMcuBytes, ctx.stream)) return (int)e;
    }
    {
        ProfScope ps(ctx, "jpeg_dct", 0.0, in_bytes + coef);
        hipLaunchKernelGGL(jpeg_dct_kernel, dim3((unsigned)a.mchunks * 6), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jpeg_count", 0.0, coef);
        hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)a.mchunks), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jpeg_scan_bits", 0.0, (double)a.mchunks * 12);
        hipLaunchKernelGGL(jpeg_scan_kernel<false>, dim3((unsigned)a.n), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jpeg_write", 0.0, coef);
        hipLaunchKernelGGL(jpeg_write_kernel, dim3((unsigned)a.mchunks), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jpeg_ffcount", 0.0, 0.0);
        hipLaunchKernelGGL(jpeg_stuff_kernel<false>, dim3((unsigned)a.bchunks), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jpeg_scan_ff", 0.0, (double)a.bchunks * 12);
        hipLaunchKernelGGL(jpeg_scan_kernel<true>, dim3((unsigned)a.n), dim3(256), 0, ctx.stream, a);
    }
    {
        ProfScope ps(ctx, "jpeg_pack", 0.0, 0.0);
        hipLaunchKernelGGL(jpeg_stuff_kernel<true>, dim3((unsigned)a.bchunks), dim3(256), 0, ctx.stream, a);
    }
    return (int)hipGetLastError();
}

}  // namespace specmi

extern "C" int specmi_jpeg_header(int quality, int H, int W, uint8_t* out, size_t capacity) {
    if (!out || quality < 1 || quality > 100 || H < 1 || H > 32768 || W < 1 || W > 32768 || capacity < (size_t)specmi::kJpegHeaderBytes)
        return SPECMI_ERR_ARG;
    specmi::JpegTables t;
    specmi::jpeg_build_tables(quality, &t);
    std::memcpy(out, t.header, specmi::kJpegHeaderBytes);
    out[specmi::kJpegSofSize] = (uint8_t)(H >> 8); out[specmi::kJpegSofSize + 1] = (uint8_t)(H & 255);
    out[specmi::kJpegSofSize + 2] = (uint8_t)(W >> 8); out[specmi::kJpegSofSize + 3] = (uint8_t)(W & 255);
    return SPECMI_OK;
}
