"""A model of the parallel inflate of one DEFLATE stream, restated from RFC 1951 in plain Python -
not from the kernels: an inflater that reports where its blocks lie, the probe for dynamic block headers, the candidates of
the chunks, the live chain, the decode into literals and window markers, and the resolution of the windows.  The GPU path
(csrc/gzip_stream.hip) is held to it: the same text, and exactly the same numbers of chunks, candidates and live chunks.

``raw`` is always the DEFLATE data alone (what lies between a gzip member's header and its eight trailer bytes); bit
positions count from its first byte, least significant bit first.  Slow (a byte of text costs microseconds): keep the
streams to tens of kilobytes."""
import numpy as np

WINDOW = 32768
MARKER = 0x8000
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class ModelError(ValueError):
    pass


def canonical(lengths):
    """code lengths -> {(length, code): symbol} (RFC 1951 3.2.2), and the code space left in units of 2^-15"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt, left = 0, [0] * 16, 1 << 15
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
        left -= count[bits] << (15 - bits)
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table, left


class Stream(object):
    """The bits of ``raw`` and what was decoded from them so far (a block per start bit: the chunk sizes share them)."""

    def __init__(self, raw):
        self.raw = bytes(raw)
        self.n_bits = 8 * len(self.raw)
        self.bits = np.unpackbits(np.frombuffer(self.raw + b'\0' * 64, dtype=np.uint8), bitorder='little').tolist()
        self.blocks = {}

    def take(self, pos, n):
        v = 0
        for k in range(n):
            v |= self.bits[pos + k] << k
        return v

    def symbol(self, table, pos):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | self.bits[pos + l - 1]
            sym = table.get((l, code))
            if sym is not None:
                return sym, pos + l
        raise ModelError('no code at bit %d' % pos)

    def code_lengths(self, pos):
        """a dynamic block's header from the bit behind BTYPE -> (literal lengths, distance lengths, bit behind it)"""
        hlit, hdist, hclen = self.take(pos, 5) + 257, self.take(pos + 5, 5) + 1, self.take(pos + 10, 4) + 4
        pos += 14
        if hlit > 286 or hdist > 30:
            raise ModelError('HLIT or HDIST')
        cl = [0] * 19
        for k in range(hclen):
            cl[CL_ORDER[k]] = self.take(pos, 3)
            pos += 3
        table, left = canonical(cl)
        self.cl_left = left
        if left < 0:
            raise ModelError('code length code oversubscribed')
        lens = []
        while len(lens) < hlit + hdist:
            if pos > self.n_bits:
                raise ModelError('input ends in a header')
            sym, pos = self.symbol(table, pos)
            if sym < 16:
                lens.append(sym)
                continue
            if sym == 16:
                if not lens:
                    raise ModelError('repeat of nothing')
                rep, val, pos = 3 + self.take(pos, 2), lens[-1], pos + 2
            elif sym == 17:
                rep, val, pos = 3 + self.take(pos, 3), 0, pos + 3
            else:
                rep, val, pos = 11 + self.take(pos, 7), 0, pos + 7
            if len(lens) + rep > hlit + hdist:
                raise ModelError('repeat overruns')
            lens.extend([val] * rep)
        return lens[:hlit], lens[hlit:], pos

    def block(self, start):
        """the block at bit ``start`` -> (end bit, BFINAL, BTYPE, tokens); a token is a literal byte or (length, distance)"""
        got = self.blocks.get(start)
        if got is not None:
            return got
        if start + 3 > self.n_bits:
            raise ModelError('input ends')
        final, btype, pos = self.bits[start], self.take(start + 1, 2), start + 3
        tokens = []
        if btype == 0:
            pos = (pos + 7) & ~7
            n, nn = self.take(pos, 16), self.take(pos + 16, 16)
            if n != (~nn & 0xffff) or pos + 32 + 8 * n > self.n_bits:
                raise ModelError('stored block')
            at = pos // 8 + 4
            tokens = list(self.raw[at:at + n])
            pos = 8 * (at + n)
        elif btype == 3:
            raise ModelError('block type 3')
        else:
            if btype == 1:
                lit, dist = FIXED_LIT, FIXED_DIST
            else:
                lit, dist, pos = self.code_lengths(pos)
                if not lit[256]:
                    raise ModelError('no end of block code')
            (lit_t, lit_left), (dist_t, dist_left) = canonical(lit), canonical(dist)
            if lit_left < 0 or dist_left < 0:
                raise ModelError('oversubscribed')
            while True:
                if pos >= self.n_bits:
                    raise ModelError('input ends in a block')
                sym, pos = self.symbol(lit_t, pos)
                if sym < 256:
                    tokens.append(sym)
                elif sym == 256:
                    break
                else:
                    if sym > 285:
                        raise ModelError('length symbol')
                    k = sym - 257
                    length, pos = LEN_BASE[k] + self.take(pos, LEN_EXTRA[k]), pos + LEN_EXTRA[k]
                    d, pos = self.symbol(dist_t, pos)
                    if d > 29:
                        raise ModelError('distance symbol')
                    tokens.append((length, DIST_BASE[d] + self.take(pos, DIST_EXTRA[d])))
                    pos += DIST_EXTRA[d]
        if pos > self.n_bits:
            raise ModelError('input ends in a block')
        got = self.blocks[start] = (pos, final, btype, tokens)
        return got


def token_bytes(tokens):
    return sum(1 if isinstance(t, int) else t[0] for t in tokens)


def inflate(raw):
    """-> (text, [(start bit, end bit, BTYPE, BFINAL, bytes)]) of the whole stream, the ordinary way"""
    s = raw if isinstance(raw, Stream) else Stream(raw)
    out, blocks, pos = bytearray(), [], 0
    while True:
        end, final, btype, tokens = s.block(pos)
        before = len(out)
        for t in tokens:
            if isinstance(t, int):
                out.append(t)
            else:
                length, dist = t
                if dist > len(out):
                    raise ModelError('distance beyond the text')
                for _ in range(length):
                    out.append(out[-dist])
        blocks.append((pos, end, btype, final, len(out) - before))
        pos = end
        if final:
            return bytes(out), blocks


# ---- the probe -------------------------------------------------------------------------------------------------------------------
def header_ok(s, pos):
    """zlib's checks of a dynamic block header at bit ``pos``: BTYPE = 2, HLIT <= 29, HDIST <= 29, a complete code length
    code, legal repeats, a length for symbol 256, a complete literal / length code, a distance code that is complete or a
    single code of one bit; all of it in front of the data's end"""
    if pos + 17 > s.n_bits or s.take(pos + 1, 2) != 2:
        return False
    if s.take(pos + 3, 5) > 29 or s.take(pos + 8, 5) > 29:
        return False
    try:
        lit, dist, end = s.code_lengths(pos + 3)
    except (ModelError, IndexError):
        return False
    if s.cl_left != 0 or end > s.n_bits or not lit[256]:
        return False
    if canonical(lit)[1] != 0:
        return False
    used = [l for l in dist if l]
    return canonical(dist)[1] == 0 or used == [1]


def survivors(s):
    """the bit positions that pass the checks a vector can make: BTYPE, HLIT, HDIST and the complete code length code"""
    b = np.array(s.bits[:s.n_bits + 64], dtype=np.int64)
    n = s.n_bits
    def field(off, width):
        return sum(b[off + k:off + k + n] << k for k in range(width))
    ok = (field(1, 2) == 2) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    pos = np.nonzero(ok)[0]
    pos = pos[pos + 17 + 3 * 19 < len(b) - 3]
    ncl = sum(b[pos + 13 + k] << k for k in range(4)) + 4
    kraft = np.zeros(len(pos), dtype=np.int64)
    for i in range(19):
        at = pos + 17 + 3 * i
        v = b[at] | (b[at + 1] << 1) | (b[at + 2] << 2)
        kraft += np.where((i < ncl) & (v > 0), 128 >> v, 0)
    return pos[kraft == 128].tolist()


def candidates(raw, chunk):
    """per chunk of ``chunk`` bytes: the chunk's candidate, counted in bits from the chunk's first (None: it has none).
    Chunk 0's is the stream's first bit; every other chunk's the first position in it that passes header_ok."""
    s = raw if isinstance(raw, Stream) else Stream(raw)
    n_chunks = max(1, -(-len(s.raw) // chunk))
    out = [None] * n_chunks
    out[0] = 0
    if not hasattr(s, 'survivors'):
        s.survivors, s.header_ok = survivors(s), {}
    for pos in s.survivors:
        j = pos // (8 * chunk)
        if j == 0 or j >= n_chunks or out[j] is not None:
            continue
        ok = s.header_ok.get(pos)
        if ok is None:
            ok = s.header_ok[pos] = header_ok(s, pos)
        if ok:
            out[j] = pos - 8 * chunk * j
    return out


# ---- count and link ----------------------------------------------------------------------------------------------------------------
def walk(s, start, cands, chunk):
    """block after block from ``start`` until BFINAL or a block end that is the candidate of the chunk it lies in
    -> (landing bit, bytes, BFINAL, [block starts])"""
    pos, n, starts = start, 0, []
    while True:
        starts.append(pos)
        end, final, _btype, tokens = s.block(pos)
        n += token_bytes(tokens)
        pos = end
        j = pos // (8 * chunk)
        if final or (j < len(cands) and cands[j] is not None and 8 * chunk * j + cands[j] == pos):
            return pos, n, final, starts


def live_chain(s, cands, chunk):
    """-> [(chunk, start bit, landing bit, bytes, place in the text, block starts)] of the chunks on the chain from chunk 0"""
    out, j, off = [], 0, 0
    while True:
        start = 8 * chunk * j + cands[j]
        land, n, final, starts = walk(s, start, cands, chunk)
        out.append((j, start, land, n, off, starts))
        off += n
        if final:
            return out
        j = land // (8 * chunk)


# ---- decode, windows, translation --------------------------------------------------------------------------------------------------
def decode_markers(s, starts):
    """the blocks at ``starts`` -> one symbol per byte: a literal, or MARKER | k = byte k of the 32 KiB in front of the chunk"""
    sym = []
    for pos in starts:
        for t in s.block(pos)[3]:
            if isinstance(t, int):
                sym.append(t)
                continue
            length, dist = t
            for _ in range(length):
                at = len(sym) - dist
                sym.append(sym[at] if at >= 0 else MARKER | (WINDOW + at))
    return sym


def resolve(chain_symbols):
    """[(place, symbols)] of the live chunks -> the text: first the last 32 KiB of every chunk, in order, then the rest"""
    total = sum(len(sym) for _, sym in chain_symbols)
    text, done = bytearray(total), bytearray(total)

    def byte(off, v):
        if not v & MARKER:
            return v
        at = off - WINDOW + (v & 0x7fff)
        if at < 0 or not done[at]:
            raise ModelError('a marker points at a byte that is not resolved')
        return text[at]
    for off, sym in chain_symbols:
        for k in range(max(0, len(sym) - WINDOW), len(sym)):
            text[off + k], done[off + k] = byte(off, sym[k]), 1
    for off, sym in chain_symbols:
        for k in range(max(0, len(sym) - WINDOW)):
            text[off + k], done[off + k] = byte(off, sym[k]), 1
    return bytes(text)


def parallel_inflate(raw, chunk):
    """The whole procedure -> dict(text, chunks, candidates, live, cands, chain)"""
    s = raw if isinstance(raw, Stream) else Stream(raw)
    cands = candidates(s, chunk)
    chain = live_chain(s, cands, chunk)
    text = resolve([(off, decode_markers(s, starts)) for _j, _start, _land, _n, off, starts in chain])
    return dict(text=text, chunks=len(cands), candidates=sum(c is not None for c in cands[1:]), live=len(chain), cands=cands,
                chain=chain)


def gzip_member(raw, text, flags=0, extra=b'', name=b'', comment=b''):
    """``raw`` wrapped as a gzip member (RFC 1952) with the optional header fields ``flags`` asks for"""
    import struct
    import zlib
    head = b'\x1f\x8b\x08' + bytes([flags]) + b'\0\0\0\0\0\x03'
    if flags & 4:
        head += struct.pack('<H', len(extra)) + extra
    if flags & 8:
        head += name + b'\0'
    if flags & 16:
        head += comment + b'\0'
    if flags & 2:
        head += struct.pack('<H', zlib.crc32(head) & 0xffff)
    return head + bytes(raw) + struct.pack('<II', zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff)
