"""A pure-Python SAM decoder for the tests: bytes.split plus the rules of DESIGN 13 written out again.  It shares no code
with besst_amd.bamio or csrc/sam_core.h.

    decode(data) -> dict: references, lengths, the columns tid mtid pos mpos tlen flag mapq qlen rlen alen (numpy), the
                    number of saturated records, the byte offset of every record line, header_bytes
    SamModelError  : .offset (first byte of the line at fault), .line (1-based), .code (the reason's number)
"""
import re

import numpy as np

FEW_FIELDS, EMPTY_LINE, HEADER_LINE, BAD_FLAG, BAD_POS, BAD_MAPQ, BAD_PNEXT, BAD_TLEN, BAD_RNAME, BAD_RNEXT, BAD_CIGAR = range(1, 12)
CODE_NAMES = {FEW_FIELDS: 'fewer than eleven fields', EMPTY_LINE: 'empty line', HEADER_LINE: 'header line behind a record',
              BAD_FLAG: 'FLAG', BAD_POS: 'POS', BAD_MAPQ: 'MAPQ', BAD_PNEXT: 'PNEXT', BAD_TLEN: 'TLEN', BAD_RNAME: 'RNAME',
              BAD_RNEXT: 'RNEXT', BAD_CIGAR: 'CIGAR'}
_DIGITS = re.compile(rb'[0-9]+\Z')
_SIGNED = re.compile(rb'-?[0-9]+\Z')
_CIGAR_OP = re.compile(rb'([0-9]+)([MIDNSHP=X])')


class SamModelError(ValueError):
    def __init__(self, code, offset, line):
        ValueError.__init__(self, '%s at byte %d, line %d' % (CODE_NAMES[code], offset, line))
        self.code, self.offset, self.line = code, offset, line


def lines_of(data):
    """(offset, line without its terminator) of every line: '\\n' ends a line, a '\\r' directly in front of it belongs to the
    terminator, a last line without '\\n' is a line"""
    out, at = [], 0
    parts = data.split(b'\n')
    if parts and parts[-1] == b'':
        parts.pop()                                              # the file ends with '\n': no line behind it
    for part in parts:
        out.append((at, part[:-1] if part.endswith(b'\r') else part))
        at += len(part) + 1
    return out


def unsigned(text, limit):
    if not _DIGITS.match(text):
        return None
    v = int(text)
    return v if v <= limit else None


def cigar_lengths(text):
    """CIGAR text -> (list of (op, len)) or None when malformed; '*' -> []"""
    if text == b'*':
        return []
    ops, at = [], 0
    while at < len(text):
        m = _CIGAR_OP.match(text, at)
        if not m or int(m.group(1)) >= 1 << 28:
            return None
        ops.append((m.group(2).decode(), int(m.group(1))))
        at = m.end()
    return ops if ops else None


def query_lengths(ops, l_seq):
    """pysam 0.8.4: (qlen before saturation, alen)"""
    q_total = sum(n for op, n in ops if op in 'MIS=X')
    alen = sum(n for op, n in ops if op in 'MDN=X')
    lead = 0
    for op, n in ops:
        if op == 'S':
            lead += n
        elif op != 'H':
            break
    trail = 0
    for op, n in reversed(ops[1:]):                              # the first operation is never looked at
        if op == 'S':
            trail += n
        elif op != 'H':
            break
    return max(0, (l_seq if l_seq else q_total) - lead - trail), alen


def parse_header(lines):
    names, lengths, seen = [], [], set()
    for _, line in lines:
        fields = line.split(b'\t')
        if fields[0] != b'@SQ':
            continue
        tags = {f[:2]: f[3:] for f in fields[1:] if f[2:3] == b':'}
        if b'SN' not in tags or b'LN' not in tags:
            raise ValueError('@SQ without SN or LN')
        name = tags[b'SN'].decode()
        if name in seen:
            raise ValueError('repeated SN')
        seen.add(name)
        names.append(name)
        lengths.append(int(tags[b'LN']))
    return names, lengths


def decode_record(line, row_of):
    """one record line -> (values, saturated) or an error code"""
    if line == b'':
        return EMPTY_LINE
    if line.startswith(b'@'):
        return HEADER_LINE
    f = line.split(b'\t')
    if len(f) < 11:
        return FEW_FIELDS
    flag = unsigned(f[1], 65535)
    if flag is None:
        return BAD_FLAG
    if f[2] == b'*':
        tid = -1
    elif f[2] in row_of:
        tid = row_of[f[2]]
    else:
        return BAD_RNAME
    pos = unsigned(f[3], 2 ** 31 - 1)
    if pos is None:
        return BAD_POS
    mapq = unsigned(f[4], 255)
    if mapq is None:
        return BAD_MAPQ
    ops = cigar_lengths(f[5])
    if ops is None:
        return BAD_CIGAR
    if f[6] == b'=':
        mtid = tid
    elif f[6] == b'*':
        mtid = -1
    elif f[6] in row_of:
        mtid = row_of[f[6]]
    else:
        return BAD_RNEXT
    mpos = unsigned(f[7], 2 ** 31 - 1)
    if mpos is None:
        return BAD_PNEXT
    if not _SIGNED.match(f[8]) or not -2 ** 31 <= int(f[8]) <= 2 ** 31 - 1:
        return BAD_TLEN
    l_seq = 0 if f[9] == b'*' else len(f[9])
    qlen, alen = query_lengths(ops, l_seq)
    return dict(tid=tid, mtid=mtid, pos=pos - 1, mpos=mpos - 1, tlen=int(f[8]), flag=flag, mapq=mapq, qlen=min(qlen, 65535),
                rlen=l_seq, alen=alen), qlen > 65535


DTYPES = dict(tid=np.int32, mtid=np.int32, pos=np.int32, mpos=np.int32, tlen=np.int32, flag=np.uint16, mapq=np.uint8,
              qlen=np.uint16, rlen=np.int32, alen=np.int32)


def decode(data):
    lines = lines_of(data)
    n_head = 0
    while n_head < len(lines) and lines[n_head][1].startswith(b'@'):
        n_head += 1
    references, lengths = parse_header(lines[:n_head])
    row_of = {name.encode(): i for i, name in enumerate(references)}
    cols = {k: [] for k in DTYPES}
    saturated, offsets = 0, []
    for no, (at, line) in enumerate(lines[n_head:], n_head + 1):
        got = decode_record(line, row_of)
        if isinstance(got, int):
            raise SamModelError(got, at, no)
        values, sat = got
        for k in DTYPES:
            cols[k].append(values[k])
        saturated += bool(sat)
        offsets.append(at)
    out = {k: np.array(v, dtype=np.int64).astype(DTYPES[k]) for k, v in cols.items()}
    out.update(references=references, lengths=lengths, saturated=saturated, offsets=offsets,
               header_bytes=lines[n_head][0] if n_head < len(lines) else len(data))
    return out
