"""The designed gzip files of SEVERAL members: the inputs of tests/test_gzip_members_model.py on the
CPU and of tests/test_gpu_gzip_members.py on the device, each built once per process from the streams of
tests/gzip_stream_design.py, and what the model (tests/gzip_members_model.py) makes of them at every chunk size.  Every file
is a series of members that zlib reads, except the damaged ones and ``reach_bad``; every one is under 200 KB."""
import functools
import gzip
import struct
import zlib

from tests import bgzf_writer as BW
from tests import gzip_members_model as MM
from tests import gzip_stream_design as D
from tests import gzip_stream_model as M

CHUNKS = (256, 1024, 65536)
MAX_FILE = 200000
BORDER = 65536                           # a chunk border of every size in CHUNKS, counted from member 0's data


def member(raw, text, **kw):
    return M.gzip_member(raw, text, **kw)


def packed(text, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    return member(D.deflate(text, level, mem_level, strategy), text, **kw)


def stored(payload, final=False):
    """a hand-made stored block (it begins at a byte boundary)"""
    return bytes([1 if final else 0]) + struct.pack('<HH', len(payload), len(payload) ^ 0xffff) + bytes(payload)


def fixed_block(symbols, final=True):
    """a hand-made fixed-code block: literals 0..255, 256 (the end), or ('match', length symbol, extra bits value, extra bits,
    distance symbol) with a distance that needs no extra bits"""
    bits = [1 if final else 0, 1, 0]

    def code(sym):
        if sym < 144:
            return format(0x30 + sym, '08b')
        if sym < 256:
            return format(0x190 + sym - 144, '09b')
        if sym < 280:
            return format(sym - 256, '07b')
        return format(0xc0 + sym - 280, '08b')
    for s in symbols:
        if isinstance(s, tuple):
            _tag, length_symbol, extra, n_extra, distance_symbol = s
            bits += [int(b) for b in code(length_symbol)]
            bits += [(extra >> k) & 1 for k in range(n_extra)]
            bits += [int(b) for b in format(distance_symbol, '05b')]
        else:
            bits += [int(b) for b in code(s)]
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(b << k for k, b in enumerate(bits[at:at + 8])) for at in range(0, len(bits), 8))


def magic_in_fixed_codes():
    """a fixed-code block whose CODED bits spell 1f 8b 08 00 at a byte boundary: five literals of nine bits behind the three
    header bits end at bit 48; literal 241 (111110001), literal 114 (10100010), length symbol 272 (0010000) with extra
    bits 00, distance symbol 0 (00000) and the end-of-block code follow -> (raw, text, offset of the magic in raw)"""
    raw = fixed_block([200, 201, 202, 203, 204, 241, 114, ('match', 272, 0, 2, 0), 256])
    text = bytes([200, 201, 202, 203, 204, 241, 114]) + bytes([114]) * 31
    assert raw[6:10] == b'\x1f\x8b\x08\x00' and zlib.decompress(raw, -15) == text
    return raw, text, 6


@functools.lru_cache(maxsize=None)
def files():
    """name -> (file, text, is a FASTA file)"""
    S = D.streams()
    text = S['mem8'][1]
    cut = len(text) // 3
    a, b = text[:cut], text[cut:]
    mem_a, mem_b = packed(a, 1), packed(b, 9)
    empty = member(S['empty'][0], b'')
    assert len(empty) == 20
    out = {}
    # 1. two members, level 1 and level 9
    out['two_members'] = (mem_a + mem_b, text, True)
    # 2., 3. a plain member followed by a BGZF chain with its empty EOF member: 23 members, and 326 of about 140 bytes
    out['plain_then_bgzf_4096'] = (packed(a) + BW.bgzf(text, 4096), a + text, True)
    out['plain_then_bgzf_256'] = (packed(a) + BW.bgzf(text, 256), a + text, True)
    # 4. empty members
    out['empty_front'] = (empty + mem_a + mem_b, text, True)
    out['empty_middle'] = (mem_a + empty + empty + mem_b, text, True)
    out['empty_end'] = (mem_a + mem_b + empty, text, True)
    out['empty_only'] = (empty * 3, b'', False)
    # 5. members whose first block is stored, fixed and dynamic (memLevel 1: many blocks each)
    q = len(text) // 4
    parts = [text[:q], text[q:2 * q], text[2 * q:3 * q], text[3 * q:]]
    out['first_blocks'] = (packed(parts[0], 6, 1) + packed(parts[1], 0) + packed(parts[2], 6, 8, zlib.Z_FIXED) +
                           packed(parts[3], 6, 1), text, True)
    # 6. headers
    out['fname_false_start'] = (mem_a + packed(b, 9, flags=8, name=b'x\x1f\x8b\x08x'), text, True)
    out['fname_flagged_false_start'] = (mem_a + packed(b, 9, flags=8, name=b'x\x1f\x8b\x08\x08y'), text, True)
    out['fextra_holds_member'] = (mem_a + packed(b, 9, flags=4, extra=BW.subfield(b'XY', empty)), text, True)
    inner = mem_a[:len(mem_a)] + mem_b[:2000]                # a whole member and 2000 bytes of another, as a payload
    rest = text[:20000]
    raw = stored(inner) + D.deflate(rest, 6, 1)
    out['stored_holds_member'] = (packed(a, 6, 1) + member(raw, inner + rest), a + inner + rest, False)
    magic_raw, magic_text, _at = magic_in_fixed_codes()
    out['magic_in_codes'] = (packed(a, 6, 1) + member(magic_raw, magic_text) + packed(b, 6, 1), a + magic_text + b, False)
    first = packed(a, 6, 1)
    for name, delta in (('border_on', 0), ('border_before', -1), ('border_behind', 1), ('border_straddled', -5)):
        # member 2 begins BORDER + delta bytes behind member 0's data: member 1's FCOMMENT is as long as that needs
        middle = packed(b[:3000], 6, 8, flags=16, comment=b'')
        pad = 10 + BORDER + delta - len(first) - len(middle)
        assert 0 < pad < 65000
        middle = packed(b[:3000], 6, 8, flags=16, comment=b'c' * pad)
        assert len(first) + len(middle) == 10 + BORDER + delta
        out[name] = (first + middle + packed(b[3000:], 6, 1), text, True)
    # 7. reach: a match that reaches exactly its member's first byte, and one that reaches one byte further
    lead = member(*S['mem1_level1'])
    lead_text = S['mem1_level1'][1]
    out['reach_ok'] = (lead + member(stored(b'A') + D.fixed_match_block(285, 0, 0, 0), b'A' * 259), lead_text + b'A' * 259, False)
    for name, (data, t, _fasta) in out.items():
        assert len(data) < MAX_FILE, (name, len(data))
        assert gzip.decompress(data) == t, name
    return out


def reach_bad():
    """-> (file, offset of the member zlib refuses): fixed_match_block(285, 0, 0, 0) alone as a second member reaches one
    byte into the first member's text.  Its trailer is that of the 258 copies of that byte, so that a decoder which checks
    the distance against the whole text finds nothing wrong with the file."""
    raw, text = D.streams()['mem1_level1']
    lead = member(raw, text)
    return lead + member(D.fixed_match_block(285, 0, 0, 0), text[-1:] * 258), len(lead)


DAMAGE = ('crc_of_member_2', 'isize_of_member_1', 'text_between_members', 'zeros_behind_the_last', 'cut_in_member_2',
          'cm_7_in_member_2')


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> (file, the device's status or a tuple of acceptable ones, the member the host's error names)"""
    text = D.streams()['mem8'][1]
    cut = len(text) // 3
    m1, m2 = packed(text[:cut], 1, 1), packed(text[cut:], 9, 1)
    crc1, isize1 = struct.unpack('<II', m1[-8:])
    crc2, isize2 = struct.unpack('<II', m2[-8:])
    return {
        'crc_of_member_2': (m1 + m2[:-8] + struct.pack('<II', crc2 ^ 0x8000, isize2), 'crc', len(m1)),
        'isize_of_member_1': (m1[:-8] + struct.pack('<II', crc1, isize1 + 1) + m2, 'isize', 0),
        'text_between_members': (m1 + b'0123456789' + m2, 'trailing_bytes', len(m1)),
        'zeros_behind_the_last': (m1 + m2 + b'\0\0\0\0', 'trailing_bytes', len(m1) + len(m2)),
        'cut_in_member_2': (m1 + m2[:len(m2) // 2], None, len(m1)),
        'cm_7_in_member_2': (m1 + m2[:2] + b'\x07' + m2[3:], 'trailing_bytes', len(m1)),
    }


@functools.lru_cache(maxsize=None)
def file_model(name):
    return MM.FileModel(files()[name][0])


@functools.lru_cache(maxsize=None)
def modelled(name, chunk):
    """the model's parallel inflate of a file at a chunk size"""
    return file_model(name).inflate(chunk)
