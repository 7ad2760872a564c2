"""Test scaffolding: a pure-Python walker and validator of BGZF files, and the size yardstick of the compressor's tests
(zlib level 1, raw DEFLATE, on the same blocks).  The validator is the format's rules as a reader meets them: the fixed
header, BSIZE, a DEFLATE stream that inflates ALONE (nothing in front of it to refer to) and ends exactly at the trailer,
CRC-32, ISIZE, full blocks but for the last, one EOF block at the very end."""
import struct
import zlib

HEADER = bytes(bytearray([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0]))
EOF = HEADER + bytes(bytearray([0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
BLOCK_PAYLOAD = 65280
BLOCK_OVERHEAD = 26                      # header 18, CRC-32 and ISIZE 8


class BgzfError(AssertionError):
    pass


def _fail(at, what):
    raise BgzfError('BGZF block at byte %d: %s' % (at, what))


def walk(data):
    """-> [(offset, block bytes)] from the BSIZE fields alone"""
    data = bytes(data)
    blocks, at = [], 0
    while at < len(data):
        if len(data) - at < 18:
            _fail(at, 'the file ends inside a header')
        if data[at:at + 16] != HEADER:
            _fail(at, 'header bytes %r' % data[at:at + 16])
        bsize = struct.unpack_from('<H', data, at + 16)[0] + 1
        if bsize < 28 or at + bsize > len(data):
            _fail(at, 'BSIZE %d does not fit (%d bytes left)' % (bsize, len(data) - at))
        blocks.append((at, data[at:at + bsize]))
        at += bsize
    return blocks


def inflate_block(at, block):
    """the payload of one block, every field checked"""
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(block[18:-8])
    except zlib.error as exc:
        _fail(at, 'the DEFLATE data does not inflate on its own: %s' % exc)
    if not d.eof:
        _fail(at, 'the DEFLATE data does not end in front of the trailer (BSIZE too small, or no final block)')
    if d.unused_data:
        _fail(at, '%d bytes between the DEFLATE data and the trailer (BSIZE too large)' % len(d.unused_data))
    crc, isize = struct.unpack('<II', block[-8:])
    if isize != len(raw):
        _fail(at, 'ISIZE %d, %d bytes inflated' % (isize, len(raw)))
    if crc != (zlib.crc32(raw) & 0xffffffff):
        _fail(at, 'CRC-32 %08x, the bytes have %08x' % (crc, zlib.crc32(raw) & 0xffffffff))
    return raw


def validate(data, payload=BLOCK_PAYLOAD, eof=True):
    """The file's bytes, every block checked -> (inflated bytes, [size of every data block]).  ``payload``: what every data
    block but the last must carry (None: any); ``eof``: the file must end with the one EOF block (False: it must hold none)."""
    data = bytes(data)
    blocks = walk(data)
    n_eof = sum(1 for _at, b in blocks if b == EOF)
    if eof:
        if not blocks or blocks[-1][1] != EOF or data[-28:] != EOF:
            raise BgzfError('the file does not end with the EOF block')
        if n_eof != 1:
            raise BgzfError('%d EOF blocks' % n_eof)
        blocks = blocks[:-1]
    elif n_eof:
        raise BgzfError('%d EOF blocks in a file that should have none' % n_eof)
    parts, sizes = [], []
    for k, (at, block) in enumerate(blocks):
        raw = inflate_block(at, block)
        if not raw:
            _fail(at, 'an empty data block')
        if payload is not None and (len(raw) > payload or (len(raw) != payload and k + 1 < len(blocks))):
            _fail(at, 'carries %d bytes, not %d' % (len(raw), payload))
        parts.append(raw)
        sizes.append(len(block))
    return b''.join(parts), sizes


def zlib_block(raw, level=1):
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = comp.compress(raw) + comp.flush()
    return HEADER + struct.pack('<H', len(body) + 25) + body + struct.pack('<II', zlib.crc32(raw) & 0xffffffff, len(raw))


def zlib_file(raw, payload=BLOCK_PAYLOAD, level=1, eof=True):
    """``raw`` as a BGZF file from zlib: the yardstick's file"""
    raw = bytes(raw)
    return b''.join(zlib_block(raw[at:at + payload], level) for at in range(0, len(raw), payload)) + (EOF if eof else b'')


def yardstick(raw, payload=BLOCK_PAYLOAD, level=1):
    """bytes of zlib at ``level`` (raw DEFLATE per block, + 26 per block) for the same blocks, without the EOF block"""
    return len(zlib_file(raw, payload, level, eof=False))


def scaffold_text(n, seed=1):
    """n bytes the shape PrintOutput writes: '>scaffold_<k>_uid_<id>' lines, random ACGT, 'n' and runs of 'N' of 1 to 2000"""
    import numpy as np
    rng = np.random.default_rng(seed)
    parts, have, k = [], 0, 0
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    while have < n:
        new = []
        if k == 0 or rng.integers(0, 6) == 0:
            k += 1
            new.append((b'' if have == 0 else b'\n') + b'>scaffold_%d_uid_1700000000\n' % k)
        new.append(letters[rng.integers(0, 4, int(rng.integers(200, 20000)))].tobytes())
        new.append(b'n' if rng.integers(0, 4) == 0 else b'N' * int(rng.integers(1, 2001)))
        parts += new
        have += sum(len(p) for p in new)
    return b''.join(parts)[:n]
