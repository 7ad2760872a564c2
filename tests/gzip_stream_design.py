"""The designed gzip members of the parallel-inflate tests (tests/test_gzip_stream_model.py on the CPU,
tests/test_gpu_gzip_stream.py on the device), each built once per process, and what the model (tests/gzip_stream_model.py)
makes of them at every chunk size.  Every stream carries a border of the scheme; the CPU test asserts that the border is
really there (a census, as tests/record_design.py does for the record loop)."""
import functools
import struct
import zlib

import numpy as np

from tests import gzip_stream_model as M
from tests import libdeflate_util as LD

CHUNKS = (256, 512, 1024, 65536)
MAX_COMPRESSED = 40 << 10


def acgt(n, seed):
    return np.frombuffer(b'ACGT', dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def fasta_text(n, seed=1, line=70):
    """about n bytes of contigs in lines of ``line`` bases (as tests/test_gpu_bgzf_fasta_input.py builds its text)"""
    rng = np.random.default_rng(seed)
    parts, have, k = [], 0, 0
    while have < n:
        k += 1
        seq = acgt(int(rng.integers(1, 4000)), seed * 1000 + k)
        new = b'>contig_%d len=%d\n' % (k, len(seq)) + b'\n'.join(seq[a:a + line] for a in range(0, len(seq), line)) + b'\n'
        parts.append(new)
        have += len(new)
    return b''.join(parts)


def deflate(text, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, every=0, last=True):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if not every:
        return c.compress(text) + c.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH)
    out = []
    for at in range(0, len(text), every):
        out.append(c.compress(text[at:at + every]))
        out.append(c.flush(flush) if at + every < len(text) else b'')
    return b''.join(out) + c.flush(zlib.Z_FINISH)


def repeat_text():
    """a contig that comes back 32 000 to 32 500 bytes later, again and again, and once exactly 32 768 bytes later"""
    parts = []
    unit = b'>unit\n' + acgt(2400, 77) + b'\n'
    for k, gap in enumerate((32000, 32768, 32500)):
        parts.append(unit)
        filler = b'>gap_%d\n' % k + acgt(gap, 100 + k)
        parts.append(filler[:gap - len(unit)])                   # the next copy begins `gap` bytes behind this one
    parts.append(unit)
    return b''.join(parts)


def stitched():
    """dynamic / Z_FIXED / a hand-made stored block whose payload is 2 KB of another DEFLATE stream / level 0 / dynamic"""
    text = fasta_text(60000, seed=4)
    a, b, d, e = text[:14000], text[14000:20000], text[20000:27000], text[27000:45000]
    inner = deflate(fasta_text(30000, seed=9), 6, 1)[:2048]
    parts = [deflate(a, 6, 1, last=False), deflate(b, 6, 8, zlib.Z_FIXED, last=False),
             b'\0' + struct.pack('<HH', len(inner), len(inner) ^ 0xffff) + inner,
             deflate(d, 0, 8, last=False), deflate(e, 6, 1)]
    return b''.join(parts), a + b + inner + d + e


def fixed_match_block(length_symbol, distance_symbol, distance_extra, extra_bits, final=True):
    """a hand-made fixed-code block of ONE match and the end-of-block code (RFC 1951 3.2.6; lengths 280.. without extra bits)"""
    bits = [1 if final else 0, 1, 0]                             # BFINAL, BTYPE = 01
    assert 280 <= length_symbol <= 285 and length_symbol in (285,)
    bits += [int(b) for b in format(0xc0 + length_symbol - 280, '08b')]          # Huffman codes go most significant bit first
    bits += [int(b) for b in format(distance_symbol, '05b')]
    bits += [(distance_extra >> k) & 1 for k in range(extra_bits)]               # extra bits least significant first
    bits += [0] * 7                                                              # symbol 256
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(b << k for k, b in enumerate(bits[at:at + 8])) for at in range(0, len(bits), 8))


def distance_32768():
    """small dynamic blocks / a stored block of 34 000 bytes / one dynamic block of a short text / a fixed block that copies 258
    bytes from exactly 32 768 bytes back: the copy begins a few hundred bytes into a live chunk and reads in front of it"""
    a, body, s = fasta_text(3000, seed=21), acgt(34000, 22), fasta_text(500, seed=23)[:500]
    parts = [deflate(a, 6, 1, last=False), b'\0' + struct.pack('<HH', len(body), len(body) ^ 0xffff) + body,
             deflate(s, 6, 8, last=False), fixed_match_block(285, 29, 32768 - 24577, 13)]
    text = a + body + s
    return b''.join(parts), text + text[len(text) - 32768:len(text) - 32768 + 258]


@functools.lru_cache(maxsize=None)
def streams():
    """name -> (raw DEFLATE data, text)"""
    out = {}
    text = fasta_text(80000, seed=3)
    for level in (1, 6, 9):
        out['mem1_level%d' % level] = (deflate(text, level, 1), text)
    out['mem8'] = (deflate(text, 6, 8), text)
    out['stitched'] = stitched()
    rep = repeat_text()
    out['repeat_zlib'] = (deflate(rep, 9, 8), rep)
    out['repeat_zlib_mem1'] = (deflate(rep, 9, 1), rep)
    if LD.available():
        for level in (1, 6, 12):
            out['repeat_libdeflate%d' % level] = (LD.deflate(rep, level), rep)
    out['distance_32768'] = distance_32768()
    short = text[:50000]
    out['sync_flush'] = (deflate(short, 6, 8, flush=zlib.Z_SYNC_FLUSH, every=300), short)
    out['partial_flush'] = (deflate(short, 6, 8, flush=zlib.Z_PARTIAL_FLUSH, every=300), short)
    out['empty'] = (deflate(b''), b'')
    for name, (raw, t) in out.items():
        assert len(raw) <= MAX_COMPRESSED, (name, len(raw))
        assert zlib.decompress(raw, -15) == t, name
    return out


@functools.lru_cache(maxsize=None)
def stream_model(name):
    return M.Stream(streams()[name][0])


@functools.lru_cache(maxsize=None)
def modelled(name, chunk):
    """the model's parallel_inflate of a stream at a chunk size"""
    return M.parallel_inflate(stream_model(name), chunk)


def members():
    """name -> (gzip member, text): every stream under the plain ten-byte header"""
    return {name: (M.gzip_member(raw, text), text) for name, (raw, text) in streams().items()}


HEADER_FLAGS = {'fname': 8, 'fcomment': 16, 'fextra': 4, 'fhcrc': 2, 'all': 30}


def header_variants():
    """name -> (gzip member, text, header bytes): FNAME, FCOMMENT, FEXTRA (a subfield that is not BGZF's BC), FHCRC"""
    raw, text = streams()['mem1_level6']
    out = {}
    for name, flags in HEADER_FLAGS.items():
        member = M.gzip_member(raw, text, flags, extra=b'XY\x03\x00abc', name=b'contigs.fa', comment=b'a comment')
        out[name] = (member, text, len(member) - len(raw) - 8)
    return out
