"""The PNG contract of spec_amd/csrc/png.hip restated in NumPy and plain Python: encode((H, W, 3) uint8) -> the file's bytes, the same
bytes the device writes.  PNG is lossless, so the contract is not "Pillow's bytes" but "a valid file that decodes to the picture,
with bytes fixed by the rules below"; the rule numbers are those at the head of png.hip.  `report` says which paths a picture took,
so that the tests can prove their tables reach every edge."""
import struct
import zlib

import numpy as np

SEGMENT = 32768                     # rule 3
MAX_MATCH = 258
OVERHEAD_BYTES = 63                 # signature 8, IHDR 25, IDAT's length / type / CRC 12, zlib's header 2 and Adler-32 4, IEND 12
SIGNATURE = b'\x89PNG\r\n\x1a\n'
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS = 3 + 14 + 19 * 3 + (286 + 3) * 4


def bound(H, W):
    """Rule 8: the length no file of an (H, W) picture exceeds - every segment stored."""
    L = H * (1 + 3 * W)
    return OVERHEAD_BYTES + L + 5 * -(-L // SEGMENT)


def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body))


def header(H, W):
    """Rule 1: signature and IHDR, 33 bytes."""
    return SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0))


def filter_rows(a):
    """Rule 2: (H, W, 3) uint8 -> the filtered stream (H, 1 + 3 W) uint8 and the (H, 5) sums the choice was made on."""
    H, W = a.shape[:2]
    x = a.reshape(H, 3 * W).astype(np.int64)
    left = np.concatenate([np.zeros((H, 3), np.int64), x[:, :-3]], axis=1)
    up = np.concatenate([np.zeros((1, 3 * W), np.int64), x[:-1]], axis=0)
    upleft = np.concatenate([np.zeros((H, 3), np.int64), up[:, :-3]], axis=1)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    cand = np.stack([x, x - left, x - up, x - ((left + up) >> 1), x - paeth]) & 255           # (5, H, 3W)
    sums = np.where(cand < 128, cand, 256 - cand).sum(axis=2).T                               # (H, 5)
    types = sums.argmin(axis=1)                                                               # the first of equal sums: the lowest type
    rows = cand[types, np.arange(H)]
    return np.concatenate([types[:, None], rows], axis=1).astype(np.uint8), sums


def _match(seg, d):
    """Rule 4: per position the bytes that repeat the byte d before them, from there on, inside the segment, capped at 258."""
    n = seg.size
    e = np.zeros(n, bool)
    e[d:] = seg[d:] == seg[:-d]
    stop = np.where(e, n, np.arange(n))
    nxt = np.minimum.accumulate(stop[::-1])[::-1]
    return np.minimum(nxt - np.arange(n), MAX_MATCH)


def tokens(seg):
    """Rule 4: the greedy parse -> a list of (length, distance); a literal is (1, 0)."""
    m1, m3 = _match(seg, 1), _match(seg, 3)
    out, i = [], 0
    while i < seg.size:
        best = max(int(m1[i]), int(m3[i]))
        if best >= 3:
            out.append((best, 1 if m1[i] >= m3[i] else 3))
        else:
            out.append((1, 0))
        i += out[-1][0]
    return out


def length_symbol(length):
    k = max(j for j in range(29) if LEN_BASE[j] <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def huffman_lengths(freq):
    """Rule 5: code lengths of the symbols with a non-zero count -> (lengths, how often the counts had to be halved).  Leaves in
    order of (count, symbol); the two smallest of the leaf queue's and the node queue's fronts are joined, a leaf first where
    counts are equal; while a length exceeds 15 every non-zero count c becomes (c + 1) >> 1 and the tree is built again."""
    freq = [int(f) for f in freq]
    halved = 0
    while True:
        leaves = sorted((f, s) for s, f in enumerate(freq) if f)
        m = len(leaves)
        assert m >= 2
        weight = [f for f, _ in leaves] + [0] * (m - 1)
        parent = [0] * (2 * m - 1)
        i, j = 0, m
        for k in range(m, 2 * m - 1):
            pick = []
            for _ in range(2):
                if i < m and (j >= k or weight[i] <= weight[j]):
                    pick.append(i)
                    i += 1
                else:
                    pick.append(j)
                    j += 1
            weight[k] = weight[pick[0]] + weight[pick[1]]
            parent[pick[0]] = parent[pick[1]] = k
        depth = [0] * (2 * m - 1)
        for x in range(2 * m - 3, -1, -1):
            depth[x] = depth[parent[x]] + 1
        if max(depth[:m]) <= 15:
            lengths = [0] * len(freq)
            for r, (_, s) in enumerate(leaves):
                lengths[s] = depth[r]
            return lengths, halved
        freq = [(f + 1) >> 1 for f in freq]
        halved += 1


def canonical(lengths):
    """RFC 1951 3.2.2 -> per symbol the code with its bits reversed (deflate packs Huffman codes from their most significant bit)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(int(format(nxt[l], '0%db' % l)[::-1], 2))
            nxt[l] += 1
        else:
            out.append(0)
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.fill = bytearray(), 0, 0

    def put(self, value, n):
        self.acc |= value << self.fill
        self.fill += n
        while self.fill >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.fill -= 8

    def align(self):
        if self.fill:
            self.put(0, 8 - self.fill)


def code_segment(seg, final, rep=None):
    """Rules 4 to 7: one segment of the filtered stream (1 .. 32768 bytes) -> its deflate blocks, whole bytes."""
    n = seg.size
    toks = tokens(seg)
    freq, dist = [0] * 286, [0, 0]
    freq[256] = 1
    i = 0
    for length, d in toks:
        if d:
            freq[length_symbol(length)[0]] += 1
            dist[d == 3] += 1
        else:
            freq[seg[i]] += 1
        i += length
    lengths, halved = huffman_lengths(freq)
    codes = canonical(lengths)
    # rule 6: the block's header.  286 literal / length codes, 3 distance codes, 19 code-length codes of which 0 .. 15 are 4 bits
    # long (symbol k is the code k) and 16, 17, 18 unused; every length is sent as itself.  A used distance is one bit long.
    dlen = [1 if dist[0] else 0, 0, 1 if dist[1] else 0]
    dcode = {1: 0, 3: 1 if dist[0] else 0}
    w = _Bits()
    w.put(0, 1); w.put(2, 2); w.put(29, 5); w.put(2, 5); w.put(15, 4)
    for s in CL_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for l in lengths + dlen:
        w.put(int(format(l, '04b')[::-1], 2), 4)
    assert 8 * len(w.out) + w.fill == HEADER_BITS
    i = 0
    for length, d in toks:
        if d:
            s, eb, ev = length_symbol(length)
            w.put(codes[s], lengths[s]); w.put(ev, eb); w.put(dcode[d], 1)
        else:
            w.put(codes[seg[i]], lengths[seg[i]])
        i += length
    w.put(codes[256], lengths[256])
    # rule 7: an empty stored block realigns the stream; it carries BFINAL on the picture's last segment
    w.put(1 if final else 0, 1); w.put(0, 2); w.align(); w.put(0, 16); w.put(0xFFFF, 16)
    stored = len(w.out) >= n + 5
    if rep is not None:
        rep['segments'].append(dict(tokens=toks, stored=stored, halved=halved, distances=tuple(dist), bytes=n))
    if stored:
        return bytes([1 if final else 0]) + struct.pack('<HH', n, n ^ 0xFFFF) + seg.tobytes()
    return bytes(w.out)


def encode(a, report=None):
    """(H, W, 3) uint8 RGB -> the PNG file as bytes.  `report`: a dict that receives the filter types, their sums and per segment
    its tokens, whether it was stored, how often its counts were halved and how many matches each distance took."""
    a = np.asarray(a)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('an (H, W, 3) uint8 picture')
    H, W = a.shape[:2]
    rows, sums = filter_rows(a)
    stream = rows.reshape(-1)
    if report is not None:
        report.update(filters=rows[:, 0].copy(), sums=sums, segments=[])
    nseg = -(-stream.size // SEGMENT)
    body = b'\x78\x01' + b''.join(code_segment(stream[k * SEGMENT:(k + 1) * SEGMENT], k == nseg - 1, report) for k in range(nseg))
    body += struct.pack('>I', zlib.adler32(stream.tobytes()))
    out = header(H, W) + chunk(b'IDAT', body) + chunk(b'IEND', b'')
    assert len(out) <= bound(H, W)
    return out


# ---- the test pictures that reach the edges of the rules -------------------------------------------------------------------------
def row_picture(stream):
    """A (1, W, 3) picture whose Sub-filtered row is `stream` (3 W small signed values): each channel's running sum.  With values
    near 0 the row takes filter 1, so the filtered stream is 1 followed by `stream` - the tests assert it on the report."""
    d = np.asarray(stream, np.int64).reshape(-1, 3)
    return (np.cumsum(d, axis=0) & 255).astype(np.uint8)[None]


def matches_row():
    """Every match length 3 .. 258 at both distances, and runs of 1, 2, 259, 260 and 261 repeats of a byte."""
    out, k = [], 0
    sep = lambda: [(7, 8, 9)[k % 3], (10, 11, 12)[k % 3]]        # never equal to their neighbours, 1 or 3 back
    for length in list(range(3, 259)) + [1, 2, 259, 260, 261]:
        out += sep() + [1 + k % 2] * (length + 1)                # a literal and `length` repeats of it
        k += 1
    for length in range(3, 259):
        out += sep() + ([3, 4, 5] * 88)[:3 + length]             # three literals and `length` bytes that repeat the byte 3 back
        k += 1
    for length, run in ((253, [1]), (242, [3, 4, 5])):          # the two that the segment ends above cut
        out += sep() + (run * 256)[:len(run) + length]
        k += 1
    out += [6] * (-len(out) % 3)
    return row_picture(out)


def deep_row(symbols=19):
    """Literal counts that follow Fibonacci's numbers (the end-of-block and the filter type are the two 1s in front) - Huffman's
    tree of them is a chain deeper than 15 - in an order in which no byte equals the byte 1 or 3 before it, so that nothing is a
    match."""
    fib = [2, 3]
    while len(fib) < symbols:
        fib.append(fib[-1] + fib[-2])
    values = sorted(range(-11, 12), key=lambda v: (abs(v), v))[1:1 + symbols][::-1]      # the most frequent are the smallest; 0 and 1 stay free
    left = dict(zip(values, fib))
    out = []
    while any(left.values()):
        banned = {out[-1] if out else None, out[-3] if len(out) > 2 else None}
        pick = max((v for v in values if left[v] and v not in banned), key=lambda v: (left[v], -abs(v), v), default=None)
        if pick is None:
            break
        out.append(pick)
        left[pick] -= 1
    out = out[:len(out) // 3 * 3]
    return row_picture(out)


EDGES = {
    'matches': matches_row,
    'deep': deep_row,
    'filters': lambda: np.random.default_rng(7).integers(0, 256, (33, 47, 3), dtype=np.uint8),          # every filter type
    'tie': lambda: np.zeros((5, 7, 3), np.uint8),                                                       # every sum 0: type 0
    'constant': lambda: np.full((64, 1365, 3), 77, np.uint8),                                           # eight whole segments of eight rows
    'cut': lambda: np.full((9, 1364, 3), 77, np.uint8),                                                 # a run cut by a segment end
    'all255': lambda: np.full((64, 1365, 3), 255, np.uint8),
    'noise': lambda: np.random.default_rng(8).integers(0, 256, (12, 1365, 3), dtype=np.uint8),          # stored segments, no match
}
