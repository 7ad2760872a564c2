"""Test scaffolding: a pure-Python writer of BGZF files in every layout a reader may meet - any payload size per block, any
zlib level (0: stored), extra subfields behind BC, empty blocks anywhere, with or without the EOF block - on
zlib.compressobj(wbits=-15); a walk of such bytes by the rules of besst_amd/csrc/bgzf_scan.h; and the ways the readers'
tests damage a file.  tests/bgzf_util.py holds the validator of the files the package WRITES."""
import struct
import zlib

from tests.bgzf_util import EOF

MAX_BLOCK = 65536                                            # BSIZE is sixteen bits


def block(raw, level=6, extra=b'', deflate=None):
    """One BGZF block of ``raw`` (at most 65536 bytes).  ``extra``: further subfields, laid behind BC; ``deflate``: the raw
    DEFLATE data, where another compressor made it."""
    raw = bytes(raw)
    assert len(raw) <= 65536
    if deflate is None:
        comp = zlib.compressobj(level, zlib.DEFLATED, -15)
        deflate = comp.compress(raw) + comp.flush()
    size = 12 + 6 + len(extra) + len(deflate) + 8
    assert size <= MAX_BLOCK, 'the block does not fit BSIZE: use a smaller payload'
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff' + struct.pack('<H', 6 + len(extra)) + b'BC\x02\0' + struct.pack('<H', size - 1)
            + extra + deflate + struct.pack('<II', zlib.crc32(raw) & 0xffffffff, len(raw)))


def subfield(tag=b'XY', data=b'more'):
    return bytes(tag) + struct.pack('<H', len(data)) + bytes(data)


def blocks_of(raw, payload=65280, level=6, extra=b''):
    raw = bytes(raw)
    return [block(raw[at:at + payload], level, extra) for at in range(0, len(raw), payload)]


def bgzf(raw, payload=65280, level=6, extra=b'', eof=True, empty_at=()):
    """``raw`` as a BGZF file.  ``empty_at``: indices (among the data blocks; -1: behind the last) in front of which an
    empty block - the EOF block's bytes - is laid."""
    parts = blocks_of(raw, payload, level, extra)
    out = []
    for k, b in enumerate(parts):
        if k in empty_at:
            out.append(EOF)
        out.append(b)
    if -1 in empty_at:
        out.append(EOF)
    return b''.join(out) + (EOF if eof else b'')


def walk(data, more_follows=False):
    """The blocks of ``data`` by bgzf_scan.h's rules -> ([(offset, size, payload offset, payload size, ISIZE, CRC)], end):
    ``end`` is the first byte that is no whole block.  With ``more_follows`` a block cut by the end of the bytes is no
    error; the third value says whether the walk ended at an error."""
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        left = len(data) - at
        if left < 18:
            return out, at, not more_follows
        h = data[at:at + 18]
        xlen = struct.unpack_from('<H', h, 10)[0]
        if h[:3] != b'\x1f\x8b\x08' or not h[3] & 4 or xlen < 6 or h[12:14] != b'BC' or h[14:16] != b'\x02\0':
            return out, at, True
        bsize = struct.unpack_from('<H', h, 16)[0] + 1
        if bsize < 18:
            return out, at, True
        if left < bsize:
            return out, at, not more_follows
        if bsize - 18 < xlen - 6 + 8:
            return out, at, True
        crc, isize = struct.unpack_from('<II', data, at + bsize - 8)
        if isize > 65536:
            return out, at, True
        out.append((at, bsize, at + 12 + xlen, bsize - 12 - xlen - 8, isize, crc))
        at += bsize
    return out, at, False


def offsets(data):
    return [b[0] for b in walk(data)[0]]


# ---- damage ----------------------------------------------------------------------------------------------------------------
def flip(data, at):
    data = bytearray(data)
    data[at] ^= 0x55
    return bytes(data)


def damaged(data, k, how):
    """``data`` with its block ``k`` damaged -> (bytes, compressed offset the reader must name).  'payload': a byte in the
    middle of the DEFLATE data flipped; 'crc': a byte of the CRC-32; 'isize+' / 'isize-': ISIZE one off; 'cut': the file
    ends in the middle of the block."""
    at, size, p_at, p_len, isize, _crc = walk(data)[0][k]
    if how == 'payload':
        return flip(data, p_at + p_len // 2), at
    if how == 'crc':
        return flip(data, at + size - 7), at
    if how in ('isize+', 'isize-'):
        new = isize + (1 if how == 'isize+' else -1)
        return data[:at + size - 4] + struct.pack('<I', new) + data[at + size:], at
    if how == 'cut':
        return data[:at + size // 2], at
    raise ValueError(how)


def host_inflate(data):
    """What zlib makes of the file, member by member -> (inflated bytes, None) or (None, offset of the member at fault)."""
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(data[at:]))
        except zlib.error:
            return None, at
        if not d.eof:
            return None, at
        at = len(data) - len(d.unused_data)
    return b''.join(out), None
