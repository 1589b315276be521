"""specmi_png_decode restated in NumPy / Python (spec_amd/csrc/png_dec.hip states the contract): the probe, the inflate stage with
its windows of LANES subsequences of SUB_BITS bits and their settle rounds, the Adler-32 and the unfilter wavefront's arithmetic.

Every index the scheme forms is asserted against the stream range, the staged window and the output range before it is used -
NumPy and Python wrap negative indices silently -, so that a bound missing from the scheme shows here, on the CPU, before anything
runs on a device.  ``inflate`` also counts which paths a stream reached (``counters``): a test of a path names the counter."""
import struct
import zlib

import numpy as np

from spec_amd import _lib

LANES, SUB_BITS = _lib.PNG_DECODE_LANES, _lib.PNG_DECODE_SUB_BITS
WIN_BYTES = LANES * SUB_BITS // 8
WIN_WORDS = (WIN_BYTES + 32) // 4
MAX_REC = LANES * SUB_BITS // 2
ST = {name: 1 << k for k, name in enumerate(_lib.PNG_STATUS_BITS)}
SIGNATURE = b'\x89PNG\r\n\x1a\n'
BPP = {0: 1, 2: 3, 4: 2, 6: 4}

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
REV15 = [int(f'{i:015b}'[::-1], 2) for i in range(1 << 15)]


# ---- the probe ---------------------------------------------------------------------------------------------------------------------
def probe(d):
    """-> {'reason', 'H', 'W', 'ctype', 'ranges'}: the rules of png_probe, in its order."""
    d = bytes(d)
    out = {'reason': 'supported', 'H': 0, 'W': 0, 'ctype': 0, 'ranges': []}

    def no(reason):
        out['reason'] = reason
        return out
    if len(d) < 8:
        return no('truncated' if SIGNATURE.startswith(d) else 'not_png')
    if d[:8] != SIGNATURE:
        return no('not_png')
    at, first, ended, idat_open, idat_closed, reason, ranges = 8, True, False, False, False, 'supported', []
    H = W = ct = 0
    while not ended:
        if at + 12 > len(d):
            return no('truncated')
        n = struct.unpack('>I', d[at:at + 4])[0]
        if n > 0x7FFFFFFF or n > len(d) - at - 12:
            return no('truncated')
        kind, body = d[at + 4:at + 8], d[at + 8:at + 8 + n]
        if zlib.crc32(kind + body) != struct.unpack('>I', d[at + 8 + n:at + 12 + n])[0]:
            return no('crc')
        keep = reason == 'supported'
        if first:
            if kind != b'IHDR' or n != 13:
                return no('chunk')
            first = False
            W, H, depth, ct, comp, flt, lace = struct.unpack('>IIBBBBB', body)
            if ct == 3:
                reason = 'palette'
            elif ct not in BPP:
                reason = 'chunk'
            elif depth != 8:
                reason = 'depth'
            elif comp or flt:
                reason = 'chunk'
            elif lace:
                reason = 'interlaced'
            elif not (1 <= H <= 32768 and 1 <= W <= 32768):
                reason = 'size'
        elif kind == b'IHDR':
            reason = 'chunk' if keep else reason
        elif kind == b'IDAT':
            if idat_closed and keep:
                reason = 'chunk'
            idat_open = True
            ranges.append((at + 8, n))
        elif kind == b'IEND':
            if n and keep:
                reason = 'chunk'
            ended = True
        elif kind == b'acTL':
            reason = 'animated' if keep else reason
        elif not kind[0] & 0x20 and kind != b'PLTE':
            reason = 'chunk' if keep else reason
        if kind != b'IDAT' and idat_open:
            idat_closed = True
        at += 12 + n
    if reason != 'supported':
        return no(reason)
    if at != len(d):
        return no('trailing')
    if not ranges:
        return no('chunk')
    out.update(H=H, W=W, ctype=ct, ranges=ranges)
    return out


def stream_of(d, ranges):
    return b''.join(bytes(d[o:o + n]) for o, n in ranges)


# ---- inflate -----------------------------------------------------------------------------------------------------------------------
class _Bits:
    """The stream as parse_header reads it: bits from ``end`` on read as zero, no byte at or behind len - 4 is touched."""

    def __init__(self, stream):
        self.s, self.end = stream, (len(stream) - 4) * 8

    def get(self, at, n):
        assert 0 <= n <= 16 and at >= 0
        v = 0
        for k in range(3):
            byte = (at >> 3) + k
            if byte * 8 < self.end:
                assert 0 <= byte < len(self.s) - 4, 'a header read outside the deflate range'
                v |= self.s[byte] << (8 * k)
        return (v >> (at & 7)) & ((1 << n) - 1)


def canon_build(lens):
    """-> (left, longest length, table): left 0 complete, > 0 incomplete, < 0 over-subscribed; table[15 bits, MSB first] =
    length << 9 | symbol or 0."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left, first, firsts, mx = 1, 0, [0] * 16, 0
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            return -1, 0, None
        first = (first + count[l - 1]) << 1
        firsts[l] = first
        if count[l]:
            mx = l
    table = np.zeros(1 << 15, np.int32)
    nxt = list(firsts)
    for sym, l in enumerate(lens):
        if l:
            code = nxt[l]
            nxt[l] += 1
            assert code < (1 << l)
            table[code << (15 - l):(code + 1) << (15 - l)] = l << 9 | sym
    return left, mx, table.tolist()


def parse_header(bits, at):
    """-> dict(status) or dict(btype, bfinal, at, stored_len | lit, dist)."""
    end = bits.end
    if at + 3 > end:
        return {'status': ST['early']}
    h = bits.get(at, 3)
    bfinal, btype = h & 1, h >> 1
    at += 3
    if btype == 3:
        return {'status': ST['btype']}
    if btype == 0:
        at = (at + 7) & ~7
        if at + 32 > end:
            return {'status': ST['early']}
        n, nn = bits.get(at, 16), bits.get(at + 16, 16)
        if n ^ nn != 0xFFFF:
            return {'status': ST['stored']}
        at += 32
        if at + 8 * n > end:
            return {'status': ST['early']}
        return {'status': 0, 'btype': 0, 'bfinal': bfinal, 'at': at, 'stored_len': n}
    if btype == 1:
        lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        dist = [5] * 32
    else:
        if at + 14 > end:
            return {'status': ST['early']}
        nlit, ndist, ncl = 257 + bits.get(at, 5), 1 + bits.get(at + 5, 5), 4 + bits.get(at + 10, 4)
        at += 14
        if nlit > 286 or ndist > 30:
            return {'status': ST['lens']}
        if at + 3 * ncl > end:
            return {'status': ST['early']}
        cl = [0] * 19
        for i in range(ncl):
            cl[CL_ORDER[i]] = bits.get(at, 3)
            at += 3
        left, _, ctab = canon_build(cl)
        if left != 0:
            return {'status': ST['lens']}
        lens = []
        while len(lens) < nlit + ndist:
            w = bits.get(at, 7)
            e = ctab[REV15[w] & 0x7F00]
            l, sym = e >> 9, e & 511
            if not l or l > 7:
                return {'status': ST['early'] if at + 7 > end else ST['code']}
            at += l
            if at > end:
                return {'status': ST['early']}
            if sym < 16:
                lens.append(sym)
                continue
            eb, base = {16: (2, 3), 17: (3, 3), 18: (7, 11)}[sym]
            if at + eb > end:
                return {'status': ST['early']}
            rep = base + bits.get(at, eb)
            at += eb
            if sym == 16 and not lens:
                return {'status': ST['repeat']}
            if len(lens) + rep > nlit + ndist:
                return {'status': ST['repeat']}
            lens += [lens[-1] if sym == 16 else 0] * rep
        if lens[256] == 0:
            return {'status': ST['noeob']}
        lit, dist = lens[:nlit] + [0] * (288 - nlit), lens[nlit:] + [0] * (32 - ndist)
    left, _, ltab = canon_build(lit)
    if left != 0:
        return {'status': ST['lens']}
    left, mx, dtab = canon_build(dist)
    if left < 0 or (left > 0 and mx > 1):
        return {'status': ST['lens']}
    return {'status': 0, 'btype': btype, 'bfinal': bfinal, 'at': at, 'lit': ltab, 'dist': dtab}


EOB = 1 << 30


def decode_lane(win, ltab, dtab, entry, lane_end, end, write=None):
    """One lane (decode_lane of png_dec.hip): -> (exit, bytes, matches, flags, eob_at).  ``write``: (raw, o, win_o, records,
    max_dist, raw_len) - literals are stored, matches appended as (destination, length, distance)."""
    p, fl, nb, nm, eob_at = entry, 0, 0, 0, 0
    if write:
        raw, o, win_o, recs, max_dist, raw_len = write

    def peek(q):
        assert 0 <= q and (q >> 5) + 1 <= WIN_WORDS, 'a look-ahead outside the staged window'
        k = q >> 3
        return (int.from_bytes(win[k:k + 5], 'little') >> (q & 7)) & 0xFFFFFFFF
    for _ in range(SUB_BITS):
        if p >= lane_end:
            break
        if p >= end:
            fl = ST['early']
            break
        w = peek(p)
        e = ltab[REV15[w & 0x7FFF]]
        if not e:
            fl = ST['code']
            break
        l, sym = e >> 9, e & 511
        p2 = p + l
        if p2 > end:
            fl = ST['early']
            break
        if sym < 256:
            if write:
                assert 0 <= o < raw_len, 'a literal outside the inflated stream'
                raw[o] = sym
                o += 1
            nb += 1
            p = p2
            continue
        if sym == 256:
            fl, eob_at = EOB, p2
            break
        if sym >= 286:
            fl = ST['symbol']
            break
        eb = LEN_EXTRA[sym - 257]
        length = LEN_BASE[sym - 257] + ((w >> l) & ((1 << eb) - 1))
        p2 += eb
        w2 = peek(p2)
        e2 = dtab[REV15[w2 & 0x7FFF]]
        if not e2:
            fl = ST['early'] if p2 + 15 > end else ST['code']
            break
        dl, dsym = e2 >> 9, e2 & 511
        if dsym >= 30:
            fl = ST['symbol']
            break
        deb = DIST_EXTRA[dsym]
        dist = DIST_BASE[dsym] + ((w2 >> dl) & ((1 << deb) - 1))
        p2 += dl + deb
        if p2 > end:
            fl = ST['early']
            break
        if write:
            if dist > o or dist > max_dist:
                fl = ST['far']
                break
            assert 0 <= o - win_o < 1 << 32
            recs.append((o, length, dist))
            o += length
        nb += length
        nm += 1
        p = p2
    return (lane_end if fl else max(p, lane_end)), nb, nm, fl, eob_at


def new_counters():
    return {'stored': 0, 'fixed': 0, 'dynamic': 0, 'windows_max': 0, 'eob_last_lane': 0, 'header_mid_subsequence': 0, 'lane_decodes_max': 0,
            'rounds_max': 0, 'len258_dist1': 0, 'dist32768': 0, 'dist_max': 0, 'batches_of_one': 0, 'batches_of_many': 0, 'matches': 0}


def inflate(stream, raw_len, counters=None, line=None):
    """The inflate kernel for one file: -> (raw bytearray of raw_len, status).  ``line``: the filtered row's length, for the
    counter of matches that cross a row's end."""
    c = counters if counters is not None else new_counters()
    stream = bytes(stream)
    n = len(stream)
    assert n >= 8
    raw = bytearray(raw_len)
    cmf, flg = stream[0], stream[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or (cmf * 256 + flg) % 31 or flg & 32:
        return raw, ST['zlib']
    max_dist = 1 << ((cmf >> 4) + 8)
    bits = _Bits(stream)
    end, bp, op, final_seen = bits.end, 16, 0, False
    for _ in range(end // 3 + 1):
        h = parse_header(bits, bp)
        if h['status']:
            return raw, h['status']
        bp = h['at']
        if h['btype'] == 0:
            k = h['stored_len']
            c['stored'] += 1
            if op + k > raw_len:
                return raw, ST['length']
            assert bp % 8 == 0 and 0 <= bp >> 3 and (bp >> 3) + k <= n - 4, 'a stored copy outside the deflate range'
            raw[op:op + k] = stream[bp >> 3:(bp >> 3) + k]
            op += k
            bp += 8 * k
        else:
            c['fixed' if h['btype'] == 1 else 'dynamic'] += 1
            ltab, dtab = h['lit'], h['dist']
            is_open, windows = True, 0
            for _w in range((end - bp) // (LANES * SUB_BITS) + 1):
                if not is_open:
                    break
                windows += 1
                base = (bp >> 3) & ~3
                assert 0 <= base <= n - 4
                stop = min(base + 4 * WIN_WORDS, n - 4)                 # bytes from the Adler word on read as zero
                win = stream[base:stop] + bytes(4 * WIN_WORDS + 8 - (stop - base))
                rel0 = bp - base * 8
                wend = min(end - base * 8, WIN_WORDS * 32)
                lane_end = [rel0 + (t + 1) * SUB_BITS for t in range(LANES)]
                entry, ex, res, decodes = [-1] * LANES, list(lane_end), [None] * LANES, [0] * LANES
                rounds = 0
                for rnd in range(LANES + 1):
                    sexit = list(ex)
                    moved = False
                    for t in range(LANES):
                        e = rel0 if t == 0 else sexit[t - 1]
                        if e != entry[t]:
                            entry[t] = e
                            res[t] = decode_lane(win, ltab, dtab, e, lane_end[t], wend)
                            ex[t] = res[t][0]
                            decodes[t] += 1
                            moved = True
                    if not moved:
                        break
                    rounds = rnd + 1
                else:
                    raise AssertionError('the lanes did not settle in LANES + 1 rounds')
                c['lane_decodes_max'] = max(c['lane_decodes_max'], max(decodes))
                c['rounds_max'] = max(c['rounds_max'], rounds)
                ff = next((t for t in range(LANES) if res[t][3]), LANES)
                mine = range(min(ff, LANES - 1) + 1)
                win_bytes, win_matches = sum(res[t][1] for t in mine), sum(res[t][2] for t in mine)
                ffl, feob = (res[ff][3], res[ff][4]) if ff < LANES else (0, 0)
                if ffl & ~EOB:
                    return raw, ffl & ~EOB
                if op + win_bytes > raw_len or win_matches > MAX_REC:
                    return raw, ST['length']
                recs, o, st = [], op, 0
                for t in mine:
                    mine_recs = []
                    r = decode_lane(win, ltab, dtab, entry[t], lane_end[t], wend, (raw, o, op, mine_recs, max_dist, raw_len))
                    st |= r[3] & ~EOB
                    if not r[3] & ~EOB:
                        assert r[1:3] == res[t][1:3]
                    recs += mine_recs
                    o += res[t][1]
                if st:
                    return raw, st
                assert len(recs) == win_matches
                rb = 0
                while rb < win_matches:                                 # the resolving wavefront: 64 records at a time
                    dst0 = recs[rb][0]
                    m = 0
                    for dst, length, dist in recs[rb:rb + 64]:
                        if dst - dist + min(length, dist) <= dst0:
                            m += 1
                        else:
                            break
                    assert m >= 1
                    c['batches_of_one' if m == 1 else 'batches_of_many'] += 1
                    for dst, length, dist in recs[rb:rb + m]:
                        assert dst - dist >= 0 and dst + length <= op + win_bytes <= raw_len, 'a match outside the inflated stream'
                        assert dst - dist + min(length, dist) <= dst0 or m == 1
                        for k in range(length):
                            raw[dst + k] = raw[dst - dist + k % dist]
                        c['matches'] += 1
                        c['len258_dist1'] += length == 258 and dist == 1
                        c['dist32768'] += dist == 32768
                        c['dist_max'] = max(c['dist_max'], dist)
                        if line and dst // line != (dst + length - 1) // line:
                            c['crosses_row'] = c.get('crosses_row', 0) + 1
                    rb += m
                op += win_bytes
                if ffl & EOB:
                    bp = base * 8 + feob
                    is_open = False
                    c['eob_last_lane'] += ff == LANES - 1
                    c['header_mid_subsequence'] += feob < lane_end[ff] and (feob - rel0) % SUB_BITS != 0
                else:
                    bp = base * 8 + ex[LANES - 1]
            c['windows_max'] = max(c['windows_max'], windows)
            if is_open:
                return raw, ST['early']
        if h['bfinal']:
            final_seen = True
            break
    if not final_seen:
        return raw, ST['early']
    if op != raw_len:
        return raw, ST['length']
    if (bp + 7) & ~7 != end:
        return raw, ST['leftover']
    return raw, 0


# ---- Adler-32 ----------------------------------------------------------------------------------------------------------------------
def adler_status(stream, raw, chunk=32768):
    """The two Adler kernels: per chunk the sum of the bytes and of (n - i) byte[i], joined in order, compared with the last word."""
    a = np.frombuffer(bytes(raw), np.uint8).astype(np.uint64)
    before, s2 = 1, 0
    for at in range(0, len(a), chunk):
        part = a[at:at + chunk]
        k = len(part)
        s2 = (s2 + int((part * (k - np.arange(k, dtype=np.uint64))).sum()) % 65521 + k % 65521 * before) % 65521
        before = (before + int(part.sum())) % 65521
    assert len(stream) >= 4
    return 0 if (s2 << 16 | before) == struct.unpack('>I', bytes(stream[-4:]))[0] else ST['adler']


# ---- unfilter ----------------------------------------------------------------------------------------------------------------------
def unfilter(raw, H, W, ctype):
    """Rule 3 -> ((H, W, 3) uint8, status).  Rows in order, every kept channel by itself; strips of 64 rows hand their last row on
    through the finished output, which holds the kept channels only."""
    bpp, nch = BPP[ctype], 3 if ctype & 2 else 1
    line = 1 + W * bpp
    assert len(raw) == H * line
    a = np.frombuffer(bytes(raw), np.uint8).reshape(H, line)
    if (a[:, 0] > 4).any():
        return None, ST['filter']
    px = a[:, 1:].reshape(H, W, bpp)[:, :, :nch].astype(np.int32)
    out = np.zeros((H, W, nch), np.int32)
    for y in range(H):
        ft = int(a[y, 0])
        up = out[y - 1] if y > 0 else np.zeros((W, nch), np.int32)
        if ft == 0:
            out[y] = px[y]
        elif ft == 2:
            out[y] = (px[y] + up) & 255
        elif ft == 1:
            out[y] = np.cumsum(px[y], axis=0) & 255
        else:
            left, upleft = np.zeros(nch, np.int32), np.zeros(nch, np.int32)
            for x in range(W):
                if ft == 3:
                    pred = (left + up[x]) >> 1
                else:
                    pa, pb, pc = abs(up[x] - upleft), abs(left - upleft), abs(left + up[x] - 2 * upleft)
                    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up[x], upleft))
                left = (px[y, x] + pred) & 255
                upleft = up[x]
                out[y, x] = left
    out = out.astype(np.uint8)
    return (out if nch == 3 else np.repeat(out, 3, axis=2)), 0


def decode(data, counters=None):
    """A whole file: -> (pixels or None, status, raw)."""
    info = probe(data)
    assert info['reason'] == 'supported', info['reason']
    return decode_stream(stream_of(data, info['ranges']), info['H'], info['W'], info['ctype'], counters)


def decode_stream(stream, H, W, ctype, counters=None):
    line = 1 + W * BPP[ctype]
    raw, st = inflate(stream, H * line, counters, line)
    if st:
        return None, st, raw
    st = adler_status(stream, raw)
    if counters is not None and H > 64:
        counters['strip_boundary'] = counters.get('strip_boundary', 0) + 1
    px, st2 = unfilter(raw, H, W, ctype)
    return (None if st | st2 else px), st | st2, raw


def pillow_pixels(data):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert('RGB'))


# ---- files -------------------------------------------------------------------------------------------------------------------------
def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body))


def ihdr(H, W, ctype, depth=8, lace=0):
    return chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, ctype, 0, 0, lace))


def assemble(H, W, ctype, stream, cuts=None, before=(), after=()):
    """A file around a zlib stream; ``cuts``: the lengths of the IDAT payloads (the rest goes into the last), ``before`` / ``after``:
    chunks around the IDATs."""
    parts, at = [], 0
    for n in (cuts or []):
        parts.append(stream[at:at + n])
        at += n
    parts.append(stream[at:])
    return SIGNATURE + ihdr(H, W, ctype) + b''.join(before) + b''.join(chunk(b'IDAT', p) for p in parts) + b''.join(after) + chunk(b'IEND', b'')


def filter_rows(px, filters):
    """(H, W, bpp) uint8 pixels, a filter type per row -> the filtered stream (PNG 1.2 section 6)."""
    H, W, bpp = px.shape
    rows = px.reshape(H, W * bpp).astype(np.int32)
    out = bytearray()
    for y in range(H):
        cur = rows[y]
        up = rows[y - 1] if y > 0 else np.zeros_like(cur)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]])
        ft = filters[y]
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) >> 1
        else:
            pa, pb, pc = abs(up - upleft), abs(left - upleft), abs(left + up - 2 * upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[flush_at:]) + co.flush()


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.put(int(f'{c:0{n}b}'[::-1], 2), n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def fixed_block(bw, tokens, final):
    """Tokens - an int literal or (length, distance) - as one fixed-Huffman block."""
    def lit(s):
        if s < 144:
            bw.code(0x30 + s, 8)
        elif s < 256:
            bw.code(0x190 + s - 144, 9)
        elif s < 280:
            bw.code(s - 256, 7)
        else:
            bw.code(0xC0 + s - 280, 8)
    bw.put(final | 1 << 1, 3)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            li = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length != 258))
            lit(257 + li)
            bw.put(length - LEN_BASE[li], LEN_EXTRA[li])
            di = max(i for i in range(30) if DIST_BASE[i] <= dist)
            bw.code(di, 5)
            bw.put(dist - DIST_BASE[di], DIST_EXTRA[di])
        else:
            lit(t)
    lit(256)


def stored_block(bw, data, final):
    bw.put(final, 3)
    bw.align()
    bw.put(len(data), 16)
    bw.put(len(data) ^ 0xFFFF, 16)
    bw.out += data


def zlib_wrap(bw, raw):
    bw.align()
    return b'\x78\x01' + bytes(bw.out) + struct.pack('>I', zlib.adler32(raw))


# ---- the test files, shared by the host and the device tests ----------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (7, 1), (65, 3), (120, 121)]
MODES = {0: 'L', 2: 'RGB', 4: 'LA', 6: 'RGBA'}


def picture(H, W, ctype, content, seed=0):
    """(H, W, bpp) uint8: 'noise', 'smooth' or 'flat' content."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W + ctype)
    bpp = BPP[ctype]
    if content == 'noise':
        return rng.integers(0, 256, (H, W, bpp), dtype=np.uint8)
    if content == 'flat':
        a = np.full((H, W, bpp), 200, np.uint8)
        a[H // 3:, W // 2:] = 17
        return a
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([128 + 100 * np.sin(yy / 9.0 + c) * np.cos(xx / 7.0 - c) for c in range(bpp)], axis=2)
    return np.clip(a + rng.normal(0, 2, a.shape), 0, 255).astype(np.uint8)


def pillow_save(a, ctype, **kw):
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a, MODES[ctype]).save(b, 'PNG', **kw)
    return b.getvalue()


def pillow_set():
    """[(name, file)]: Pillow-saved files at compress_level 0, 1, 6, 9 and optimize=True, of noise, smooth and flat content, in all
    four colour types and the five sizes."""
    out = []
    for H, W in SIZES:
        for ct in MODES:
            for content in ('noise', 'smooth', 'flat'):
                a = picture(H, W, ct, content)
                for name, kw in (('l0', {'compress_level': 0}), ('l1', {'compress_level': 1}), ('l6', {'compress_level': 6}),
                                 ('l9', {'compress_level': 9}), ('opt', {'optimize': True})):
                    out.append((f'pillow-{H}x{W}-ct{ct}-{content}-{name}', pillow_save(a, ct, **kw)))
    return out


def hand_file(a, ctype, filters=None, **kw):
    """A hand-assembled file of picture ``a``: per-row filter types (default: row y takes y % 5), ``deflate``'s keywords."""
    H = a.shape[0]
    return_stream = kw.pop('stream_only', False)
    extra = {k: kw.pop(k) for k in ('cuts', 'before', 'after') if k in kw}
    s = deflate(filter_rows(a, filters if filters is not None else [y % 5 for y in range(H)]), **kw)
    return s if return_stream else assemble(H, a.shape[1], ctype, s, **extra)


def hand_set():
    """[(name, file)]: hand-assembled files (the local chunk writer and per-row filters above)."""
    out = []
    for H, W in SIZES:
        for ct in MODES:
            a = picture(H, W, ct, 'smooth', 1)
            for ft in range(5):
                out.append((f'filter{ft}-{H}x{W}-ct{ct}', hand_file(a, ct, [ft] * H)))
            out.append((f'mixed-{H}x{W}-ct{ct}', hand_file(a, ct)))
    for H, W in SIZES:
        a, n = picture(H, W, 2, 'smooth', 2), picture(H, W, 2, 'noise', 2)
        for name, kw in (('fixed', {'strategy': zlib.Z_FIXED}), ('huffman', {'strategy': zlib.Z_HUFFMAN_ONLY}), ('rle', {'strategy': zlib.Z_RLE}),
                         ('wbits9', {'wbits': 9}), ('wbits15', {'wbits': 15}), ('flush', {'flush_at': (H * (1 + 3 * W)) // 2}),
                         ('cuts', {'cuts': [1, 0, 1, 1, 0]})):
            out.append((f'{name}-{H}x{W}', hand_file(a, 2, **kw)))
            out.append((f'{name}-noise-{H}x{W}', hand_file(n, 2, **kw)))
    g, rgb = picture(23, 17, 0, 'smooth', 3), picture(23, 17, 2, 'smooth', 3)
    anc = [chunk(b'gAMA', struct.pack('>I', 45455)), chunk(b'pHYs', struct.pack('>IIB', 2835, 2835, 1)), chunk(b'tEXt', b'Comment\0hand made')]
    out.append(('ancillary-grey', hand_file(g, 0, before=anc + [chunk(b'tRNS', struct.pack('>H', int(g[3, 3, 0])))], after=[chunk(b'tEXt', b'k\0v')])))
    out.append(('ancillary-rgb', hand_file(rgb, 2, before=anc + [chunk(b'tRNS', struct.pack('>HHH', *[int(v) for v in rgb[3, 3]]))])))
    out.append(('flat-rle-120x121', hand_file(picture(120, 121, 2, 'flat'), 2, [0] * 120, strategy=zlib.Z_RLE)))
    return out


def crafted_set():
    """[(name, file)]: streams written token by token, for the paths zlib's encoder does not reach."""
    out = []
    # 16383 literals of 8 bits fill the first window up to its last 8 bits: the end-of-block code starts in the last subsequence
    assert LANES * SUB_BITS == 131072, 'the sizes below are worked out for 256 lanes of 512 bits'
    a = picture(127, 128, 0, 'noise', 4) % 144
    raw = filter_rows(a, [0] * 127)
    bw = BitWriter()
    fixed_block(bw, list(raw), 1)
    out.append(('eob-last-lane', assemble(127, 128, 0, zlib_wrap(bw, raw))))
    # a match at distance 32768: 128 stored rows of 256 bytes, then row 0 again
    a = picture(129, 255, 0, 'noise', 5)
    a[128] = a[0]
    raw = filter_rows(a, [0] * 129)
    bw = BitWriter()
    stored_block(bw, raw[:32768], 0)
    fixed_block(bw, [(256, 32768)], 1)
    out.append(('distance-32768', assemble(129, 255, 0, zlib_wrap(bw, raw))))
    # a match of 258 at distance 1 that crosses rows, between two stored blocks and an empty fixed block
    a = np.zeros((9, 40, 3), np.uint8)
    raw = filter_rows(a, [0] * 9)
    bw = BitWriter()
    fixed_block(bw, [0, (258, 1), (258, 1), (258, 1)], 0)
    fixed_block(bw, [], 0)
    stored_block(bw, b'', 0)
    fixed_block(bw, [(258, 1), 0, 0, (54, 3)], 1)
    assert 1 + 258 * 4 + 2 + 54 == len(raw)
    out.append(('runs-258', assemble(9, 40, 2, zlib_wrap(bw, raw))))
    return out


def big_file():
    """The one 300 x 300 picture: noise of 24 levels over a coarse smooth picture, unfiltered (zlib codes it in dynamic blocks of several windows, and
    a lane that starts at a wrong bit stays wrong for long), its stream cut into IDATs of 1 byte, 0 bytes and 64 KiB."""
    a = picture(300, 300, 2, 'smooth', 6) // 64 + 8 * np.random.default_rng(9).integers(0, 24, (300, 300, 3))
    return 'noisy-300x300', hand_file(a.astype(np.uint8), 2, [0] * 300, cuts=[1, 0, 65536, 1, 0, 65536])


def encoder_set():
    """[(name, file)]: tests/png_ref.encode's files of its edge pictures - the two halves of the codec meet."""
    from tests import png_ref
    rng = np.random.default_rng(12)
    pics = [('one', np.array([[[1, 2, 3]]], np.uint8)), ('noise-23x17', rng.integers(0, 256, (23, 17, 3), dtype=np.uint8)),
            ('flat-65x3', np.full((65, 3, 3), 9, np.uint8)), ('matches-row', png_ref.row_picture(png_ref.matches_row())),
            ('deep-row', png_ref.row_picture(png_ref.deep_row())), ('smooth-120x121', picture(120, 121, 2, 'smooth', 7))]
    return [(f'encoder-{name}', png_ref.encode(a), a) for name, a in pics]


def damaged_set():
    """[(name, file)]: supported files whose streams break a stream rule."""
    a = picture(40, 41, 2, 'smooth', 8)
    s = hand_file(a, 2, stream_only=True)
    assert (s[2] >> 1) & 3 == 2, 'a dynamic block first'

    def flip(k, bit=0):
        b = bytearray(s)
        b[k] ^= 1 << bit
        return bytes(b)
    streams = [('code-lengths', flip(4, 3)), ('symbols', flip(len(s) // 2, 2)), ('adler', flip(len(s) - 1)), ('truncated', s[:-12]),
               ('extra-byte', s + b'\0'), ('extra-byte-inside', s[:-4] + b'\0' + s[-4:]), ('header', b'\x79' + s[1:])]
    return [(f'damaged-{name}', assemble(40, 41, 2, t)) for name, t in streams]
