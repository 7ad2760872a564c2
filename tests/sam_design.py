"""Designed SAM files for the device parser's borders (tests/test_gpu_sam.py), with the proof that every case they claim
is in them: the cases are asserted from byte offsets, as tests/sort_design.py does for the sort's size classes.

border_file(tile=1024): about 1 200 records whose QNAME lengths (1..254) are steered so that, counted from the first
record line (where the parsed text begins), the file holds
  - a line start on a tile's first byte, i.e. a '\\n' on a tile's last byte,
  - '\\r' and '\\n' split by a tile border,
  - each of tabs 1..11 on a tile's last byte and on a tile's first byte,
  - a 16-byte lane slice that holds a line start and at least four of its tabs (a whole record cannot lie inside one
    slice: eleven fields are at least 21 bytes - lines that short are errors and are in the error tests),
  - lines that span more than 3 tiles (SEQ of 5 000 bases) and one line of 70 000 bases, which saturates qlen
    (``long_lines``),
and, for a reader that cuts chunks of ``chunk`` bytes at their last line end (chunk_plan), carried tails of every length
class: 0 bytes, fewer than 16, more than a tile (a record of 1 500 bases across the chunk's end).
"""
import numpy as np

REFS = ['ctg1', 'ctg10', 'ctg100', 'c', 'a_rather_long_reference_name_to_cross_a_tile_border', 'ctgB']
LENGTHS = [90000, 5000, 12345, 300, 70000, 2000000]
CIGARS = ['100M', '5S90M5S', '3H10S80M10S2H', '50M2I48M', '50M3D50M', '30M1000N70M', '50=2X48=', '*', '20S30M50S', '100S150N',
          '10S', '4H']
OPTIONAL = '\tNM:i:1\tMD:Z:100\tXX:Z:some text'


def header_bytes():
    return ('@HD\tVN:1.4\tSO:unknown\n' + ''.join('@SQ\tSN:%s\tLN:%d\n' % r for r in zip(REFS, LENGTHS))
            + '@PG\tID:design\tPN:sam_design\n').encode()


def _fields(rng, seq_len):
    """fields 2..11 of a record (no QNAME), as text"""
    tid = int(rng.randint(-1, len(REFS)))
    rname = '*' if tid < 0 else REFS[tid]
    pick = int(rng.randint(0, 4))
    rnext = '=' if pick < 2 and tid >= 0 else ('*' if pick == 2 else REFS[int(rng.randint(0, len(REFS)))])
    cigar = CIGARS[int(rng.randint(0, len(CIGARS)))] if seq_len <= 1500 else '%dM' % seq_len
    seq = '*' if seq_len == 0 else ('ACGT' * (seq_len // 4 + 1))[:seq_len]
    qual = '*' if seq_len == 0 else 'I' * seq_len
    return [str(int(rng.randint(0, 65536))), rname, str(int(rng.randint(0, 100000))), str(int(rng.randint(0, 256))), cigar,
            rnext, str(int(rng.randint(0, 100000))), str(int(rng.randint(-5000, 5000))), seq, qual]


def border_file(tile=1024, chunk=4096, n_records=1200, long_lines=True, seed=7):
    """-> (file bytes, header bytes); the cases are steered greedily: a record takes the QNAME length that puts the next
    wanted byte on the wanted offset when a length in 1..254 does, else a filler length"""
    rng = np.random.RandomState(seed)
    want = [('nl', tile - 1), ('crlf', None)] + [('tab', k, r) for k in range(1, 12) for r in (tile - 1, 0)]
    want += [('tail0',), ('tail_small',), ('tail_big',)] * 2
    body, s = [], 0                                              # s: offset of the next line among the record lines
    c_at = 0                                                     # where the chunk that holds s begins
    for i in range(n_records):
        seq_len = 100
        if i % 11 == 3:
            seq_len = 0
        if long_lines and i in (200, 700):
            seq_len = 5000
        if long_lines and i == 450:
            seq_len = 70000
        room = c_at + chunk - s                                  # bytes of the chunk left at this line's start
        if want and want[0] == ('tail_big',) and 1040 <= room <= 1400:
            seq_len = 1500
        crlf = i % 5 == 0 or (want and want[0][0] == 'crlf')
        optional = OPTIONAL if i % 3 == 0 or (want and want[0][0] == 'tab' and want[0][1] == 11) else ''
        f = _fields(rng, seq_len)
        eol = '\r\n' if crlf else '\n'
        rest = '\t' + '\t'.join(f) + optional + eol              # the line behind its QNAME
        length = None
        if want:
            w = want[0]
            if w[0] == 'nl':
                length = (w[1] + 1 - s - len(rest)) % tile
            elif w[0] == 'crlf':
                length = (tile - (s + len(rest) - 1)) % tile     # the '\n' on a tile's first byte, the '\r' in front of it
            elif w[0] == 'tab':
                behind = sum(len(x) + 1 for x in f[:w[1] - 1])   # bytes between tab 1 and tab k
                length = (w[2] - s - behind) % tile
            elif w[0] == 'tail0':
                length = room - len(rest)
            elif w[0] == 'tail_small':
                length = room - 5 - len(rest)
            elif w[0] == 'tail_big' and seq_len == 1500:
                length = 1 + i % 200
            if length is not None and 1 <= length <= 254:
                want.pop(0)
            else:
                length = None
        if length is None:
            length = 1 + (i * 37) % 254
        line = 'q' * length + rest
        body.append(line)
        end = s + len(line)
        while end > c_at + chunk and s > c_at:                   # the chunk is cut at this line's start
            c_at = s
        if end == c_at + chunk:
            c_at = end
        s = end
    assert not want, want
    head = header_bytes()
    return head + ''.join(body).encode(), head


def chunk_plan(n_bytes, line_ends, chunk):
    """The chunks of a reader that fills ``chunk`` bytes and cuts at the last line end (``line_ends``: the offset behind
    every line, the last line's too) -> list of (offset, bytes parsed, bytes carried to the next chunk)"""
    ends = np.asarray(line_ends, dtype=np.int64)
    out, at = [], 0
    while at < n_bytes:
        hi = min(n_bytes, at + chunk)
        k = int(np.searchsorted(ends, hi, side='right')) - 1
        cut = int(ends[k]) if k >= 0 and ends[k] > at else at
        if hi == n_bytes:
            cut = n_bytes
        if cut == at:
            raise ValueError('the line at %d is longer than a chunk' % at)
        out.append((at, cut - at, hi - cut))
        at = cut
    return out


def cases_present(data, head, tile=1024, chunk=4096, long_lines=True):
    """Assert, from the bytes, every case of the module docstring; -> the chunk plan"""
    text = data[len(head):]
    buf = np.frombuffer(text, dtype=np.uint8)
    nl = np.flatnonzero(buf == 10)
    starts = np.r_[0, nl[:-1] + 1] if text.endswith(b'\n') else np.r_[0, nl + 1]
    assert (nl % tile == tile - 1).any() and (starts % tile == 0).any()
    split = [p for p in nl.tolist() if p % tile == 0 and p > 0 and buf[p - 1] == 13]
    assert split, 'no \\r\\n split by a tile border'
    tab_at = {(k, r): False for k in range(1, 12) for r in (tile - 1, 0)}
    slice_case, spans = False, []
    for a, b in zip(starts.tolist(), np.r_[starts[1:], len(buf)].tolist()):
        tabs = a + np.flatnonzero(buf[a:b] == 9)
        for k, p in enumerate(tabs[:11].tolist(), 1):
            if (k, int(p % tile)) in tab_at:
                tab_at[(k, int(p % tile))] = True
        if np.count_nonzero(tabs < (a // 16 + 1) * 16) >= 4:
            slice_case = True
        spans.append((b - 1) // tile - a // tile + 1)
    assert all(tab_at.values()), [k for k, v in tab_at.items() if not v]
    assert slice_case
    if long_lines:
        assert sum(1 for t in spans if t > 3) >= 3 and max(spans) > 68
        return None
    assert max(spans) <= 5                                       # (nothing longer than the 1 500-base records)
    ends = np.r_[starts[1:], len(buf)]
    plan = chunk_plan(len(buf), ends, chunk)
    tails = [t for _, _, t in plan]
    assert 0 in tails[:-1] and any(0 < t < 16 for t in tails) and any(t > tile for t in tails), sorted(set(tails))[:20]
    return plan


GOOD_LINE = 'read\t99\tctg1\t101\t60\t100M\t=\t401\t400\tACGT\tIIII'


def _with(index, value):
    f = GOOD_LINE.split('\t')
    f[index] = value
    return '\t'.join(f)


# (name, a line that cannot be read, the reason's number in include/besst_amd.h BESST_SAM_*): every error class once
ERROR_LINES = [
    ('few_fields', '\t'.join(GOOD_LINE.split('\t')[:10]), 1),
    ('empty_line', '', 2),
    ('header_behind_a_record', '@CO\tlate', 3),
    ('flag_not_a_number', _with(1, '0x63'), 4),
    ('flag_out_of_range', _with(1, '65536'), 4),
    ('flag_empty', _with(1, ''), 4),
    ('pos_out_of_range', _with(3, '2147483648'), 5),
    ('pos_negative', _with(3, '-1'), 5),
    ('mapq_out_of_range', _with(4, '256'), 6),
    ('pnext_not_a_number', _with(7, '4o1'), 7),
    ('tlen_out_of_range', _with(8, '2147483648'), 8),
    ('tlen_two_signs', _with(8, '--4'), 8),
    ('rname_unknown', _with(2, 'ctg1000'), 9),
    ('rnext_unknown', _with(6, 'ctg1x'), 10),
    ('cigar_no_count', _with(5, '10MS'), 11),
    ('cigar_bad_letter', _with(5, '10M5Q'), 11),
    ('cigar_count_too_large', _with(5, '268435456M'), 11),
    ('cigar_no_operation', _with(5, '100'), 11),
    ('cigar_empty', _with(5, ''), 11),
]

# numbers at their limits: (name, line, readable)
LIMIT_LINES = [
    ('flag_65535', _with(1, '65535'), True), ('mapq_255', _with(4, '255'), True),
    ('pos_2_31_less_1', _with(3, '2147483647'), True), ('pos_0', _with(3, '0'), True), ('pnext_2_31', _with(7, '2147483648'), False),
    ('tlen_least', _with(8, '-2147483647'), True), ('tlen_int32_min', _with(8, '-2147483648'), True),
    ('tlen_below_int32', _with(8, '-2147483649'), False), ('tlen_most', _with(8, '2147483647'), True),
    ('cigar_2_28_less_1', _with(5, '268435455M'), True), ('cigar_2_28_in_the_middle', _with(5, '5M268435456D5M'), False),
    ('leading_zeros', _with(1, '000000000000000000000099'), True),
    ('qlen_saturates', _with(5, '70000M').replace('ACGT', '*'), True), ('qlen_65535', _with(5, '65535M5S') .replace('ACGT', '*'), True),
    ('qlen_65536', _with(5, '65536M').replace('ACGT', '*'), True), ('clips_only', _with(5, '3S2S'), True),
    ('seq_star', _with(9, '*'), True), ('twelve_fields', GOOD_LINE + '\tNM:i:0\tXX:Z:a\tb', True),
    ('empty_qual', _with(10, ''), True),
]


def reference_names(n=70000):
    """A table of n names for the lookup tests: ctg1 / ctg10 / ctg100 among 'ctg<i>' names, pairs that differ in the last
    byte only, a 1-byte and a 200-byte name -> (names, absent names that share a present one's prefix or more)"""
    names = ['ctg%d' % i for i in range(n - 6)]
    names += ['scaffold_0000A', 'scaffold_0000B', 'c', 'N' * 200, 'N' * 199 + 'M', 'ctg']
    absent = ['ctg%d' % n, 'ctg1_', 'ct', 'N' * 199, 'N' * 201, 'scaffold_0000C', 'scaffold_0000', 'C']
    return names, absent
