"""NumPy restatement of the baseline JPEG contract of ``specmi_jpeg_encode`` (spec_amd/csrc/jpeg.hip states the rules): the byte
string ``PIL.Image.fromarray(a).save(f, format='JPEG', quality=q, optimize=False, progressive=False)`` writes on a libjpeg-turbo
build of Pillow - baseline sequential, 4:2:0, the Annex-K Huffman tables of ITU-T T.81, no restart markers.  Everything is built
here: header, quantisation tables, code tables, scan.  Nothing is read from a Pillow file."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HEADER_BYTES = 623


def quant_tables(quality):
    """Rule 9: jpeg_set_quality(q, force_baseline) on the Annex-K base tables -> (luma, chroma), natural order."""
    if not 1 <= quality <= 100:
        raise ValueError('quality 1 .. 100')
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.int64) for base in (Q_LUMA, Q_CHROMA))


def code_table(bits, vals):
    """Annex C: canonical codes from a BITS list and a HUFFVAL list -> {symbol: (code, length)}."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(quality, H, W):
    """Rule 8: the 623 bytes in front of the scan."""
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in q[ZIGZAG]))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, (bits, vals) in ((0x00, (DC_BITS[0], DC_VALS[0])), (0x10, (AC_BITS[0], AC_VALS[0])),
                              (0x01, (DC_BITS[1], DC_VALS[1])), (0x11, (AC_BITS[1], AC_VALS[1]))):
        out += seg(0xC4, bytes([cls]) + bytes(bits) + bytes(vals))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint over the LAST axis of d (..., 8) int64."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(blocks, q):
    """Rules 4 and 5: blocks (..., 8, 8) of samples -> quantised coefficients (..., 64) in natural order."""
    d = _fdct_pass(blocks.astype(np.int64) - 128, True)                       # rows
    d = np.swapaxes(_fdct_pass(np.swapaxes(d, -1, -2), False), -1, -2)        # columns
    c = d.reshape(d.shape[:-2] + (64,))
    qv = 8 * q
    return np.sign(c) * ((np.abs(c) + (qv >> 1)) // qv)


def planes(a):
    """Rules 1 to 3: (H, W, 3) uint8 -> Y (16 my, 16 mx) and Cb, Cr (8 my, 8 mx), edges extended."""
    H, W = a.shape[:2]
    my, mx = -(-H // 16), -(-W // 16)
    F = lambda x: int(x * 65536 + 0.5)
    r, g, b = (a[..., i].astype(np.int64) for i in range(3))
    y = (F(.299) * r + F(.587) * g + F(.114) * b + 32768) >> 16
    cb = (-F(.16874) * r - F(.33126) * g + F(.5) * b + (128 << 16) + 32767) >> 16
    cr = (F(.5) * r - F(.41869) * g - F(.08131) * b + (128 << 16) + 32767) >> 16
    right = lambda p: np.concatenate([p, np.repeat(p[:, -1:], 16 * mx - W, axis=1)], axis=1)
    down = lambda p, rows: np.concatenate([p, np.repeat(p[-1:], rows - p.shape[0], axis=0)], axis=0)
    out = [down(right(y), 16 * my)]
    for c in (cb, cr):
        c = down(right(c), H + (H & 1))
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1]) & 1)
        out.append(down((s + bias[None, :]) >> 2, 8 * my))
    return out


def coefficients(a, quality):
    """-> (my, mx, 6, 64) quantised coefficients in ZIGZAG order, blocks Y00 Y01 Y10 Y11 Cb Cr, dummy blocks as rule 6 has them."""
    H, W = a.shape[:2]
    my, mx = -(-H // 16), -(-W // 16)
    hb, wb = -(-H // 8), -(-W // 8)
    ql, qc = quant_tables(quality)
    y, cb, cr = planes(a)
    blk = lambda p: p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2)
    yq = fdct_quant(blk(y), ql)                                             # (2 my, 2 mx, 64)
    out = np.zeros((my, mx, 6, 64), np.int64)
    for k in range(4):
        out[:, :, k] = yq[k >> 1::2, k & 1::2]
    out[:, :, 4], out[:, :, 5] = fdct_quant(blk(cb), qc), fdct_quant(blk(cr), qc)
    for k in range(1, 4):                                                      # dummy blocks, in MCU order so that they chain
        dummy = ((2 * np.arange(my) + (k >> 1) >= hb)[:, None] | (2 * np.arange(mx) + (k & 1) >= wb)[None, :])
        out[:, :, k][dummy] = 0
        out[:, :, k, 0] = np.where(dummy, out[:, :, k - 1, 0], out[:, :, k, 0])
    return out[..., ZIGZAG]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1


def scan(coef):
    """Rule 7: the entropy-coded segment of (my, mx, 6, 64) zigzag coefficients, fill bits included."""
    dc = [code_table(DC_BITS[i], DC_VALS[i]) for i in (0, 1)]
    ac = [code_table(AC_BITS[i], AC_VALS[i]) for i in (0, 1)]
    w = _Bits()
    pred = [0, 0, 0]
    flat = coef.reshape(-1, 6, 64)
    for m in range(flat.shape[0]):
        for k in range(6):
            comp, t = max(0, k - 3), int(k >= 4)
            c = flat[m, k]
            diff = int(c[0]) - pred[comp]
            pred[comp] = int(c[0])
            s = abs(diff).bit_length()
            w.put(*dc[t][s])
            if s:
                w.put(diff if diff >= 0 else diff + (1 << s) - 1, s)
            last = 0
            for i in np.nonzero(c[1:])[0] + 1:
                run = int(i) - last - 1
                last = int(i)
                while run > 15:
                    w.put(*ac[t][0xF0])
                    run -= 16
                v = int(c[i])
                s = abs(v).bit_length()
                w.put(*ac[t][(run << 4) | s])
                w.put(v if v >= 0 else v + (1 << s) - 1, s)
            if last != 63:
                w.put(*ac[t][0x00])
    if w.n:
        w.put((1 << (8 - w.n)) - 1, 8 - w.n)
    return bytes(w.out)


def encode(a, quality=75):
    """(H, W, 3) uint8 RGB -> the JPEG file as bytes."""
    a = np.asarray(a)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('an (H, W, 3) uint8 picture')
    return header(quality, a.shape[0], a.shape[1]) + scan(coefficients(a, quality)) + b'\xff\xd9'


SIZES = ((1, 1), (7, 5), (8, 8), (16, 16), (17, 16), (24, 24), (33, 47), (40, 56), (9, 200), (65, 130))
QUALITIES = (1, 10, 50, 75, 95, 100)
CONTENTS = ('noise', 'zeros', 'ones', 'checker', 'sparse', 'smooth')


def picture(content, H, W, seed=0):
    """The seeded test pictures: noise, all 0, all 255, a 1-pixel checkerboard, 1 % outliers on grey, a smooth gradient."""
    rng = np.random.default_rng([seed, H, W, CONTENTS.index(content)])
    if content == 'noise':
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if content == 'zeros':
        return np.zeros((H, W, 3), np.uint8)
    if content == 'ones':
        return np.full((H, W, 3), 255, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    if content == 'checker':
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    if content == 'sparse':
        a = np.full((H, W, 3), 128, np.uint8)
        hit = rng.random((H, W)) < 0.01
        a[hit] = rng.integers(0, 256, (int(hit.sum()), 3), dtype=np.uint8)
        return a
    g = np.stack([yy * 255.0 / max(H - 1, 1), xx * 255.0 / max(W - 1, 1), (yy + xx) * 255.0 / max(H + W - 2, 1)], axis=2)
    return g.astype(np.uint8)
