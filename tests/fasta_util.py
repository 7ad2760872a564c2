"""Test-side restatement of the contig FASTA reader (reference runBESST:45-74, ``ReadInContigseqs``) on the BYTES of the
file, written from its rules and sharing nothing with besst_amd:

  * ``\\n`` and ``\\r`` each end a line (the reference reads in text mode: ``\\r\\n`` is then two terminators with an empty
    line between them, which adds nothing);
  * a line whose first byte is ``>`` is a header, its name the first whitespace-delimited token behind the ``>``; a header
    without one is an error at the line's offset (the reference: IndexError);
  * every other line, stripped of leading and trailing whitespace (Python's ASCII set, interior whitespace stays), is
    appended to the current contig; text in front of the first header goes to the first contig; no header at all is one
    contig named '';
  * a byte >= 0x80 is an error at its offset; of several errors the smallest offset is reported;
  * as a dict: a name that occurs twice keeps the place of its first occurrence and the sequence of its last.

tests/golden/fasta_reader.json.gz (captured from the real function) pins it.
"""
import base64
import gzip
import json
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fasta_reader.json.gz')

WHITESPACE = frozenset((9, 10, 11, 12, 13, 28, 29, 30, 31, 32))
TERMINATORS = frozenset((10, 13))


class FastaError(ValueError):
    def __init__(self, offset, what):
        ValueError.__init__(self, '%s at byte %d' % (what, offset))
        self.offset = offset


def lines_of(data):
    """-> [(offset, line without its terminator)]"""
    out, start = [], 0
    for i, c in enumerate(data):
        if c in TERMINATORS:
            out.append((start, data[start:i]))
            start = i + 1
    if start < len(data):
        out.append((start, data[start:]))
    return out


def strip(line):
    lo, hi = 0, len(line)
    while lo < hi and line[lo] in WHITESPACE:
        lo += 1
    while hi > lo and line[hi - 1] in WHITESPACE:
        hi -= 1
    return line[lo:hi]


def first_token(line):
    lo = 0
    while lo < len(line) and line[lo] in WHITESPACE:
        lo += 1
    hi = lo
    while hi < len(line) and line[hi] not in WHITESPACE:
        hi += 1
    return line[lo:hi]


def parse_rows(data):
    """-> [(name, sequence)] as str, one per header line in file order (names may repeat); FastaError with the smallest
    offending offset."""
    data = bytes(data)
    errors = [(i, 'a byte outside ASCII') for i, c in enumerate(data) if c >= 128][:1]
    names, seqs, parts = [], [], []
    for offset, line in lines_of(data):
        if line[:1] == b'>':
            token = first_token(line[1:])
            if not token:
                errors.append((offset, 'a header without a name'))
            if names:                                            # the text in front of the first header stays with it
                seqs.append(b''.join(parts))
                parts = []
            names.append(token)
        else:
            parts.append(strip(line))
    if errors:
        raise FastaError(*min(errors))
    seqs.append(b''.join(parts))
    if not names:
        names.append(b'')
    return [(n.decode('ascii'), s.decode('ascii')) for n, s in zip(names, seqs)]


def as_dict(rows):
    out = {}
    for name, seq in rows:
        out[name] = seq
    return out


def read_contigs(data, filter_length=None):
    """-> (dict in the reference's order, Information text): what ReadInContigseqs returns and prints, with the filter it
    intended (the reference deletes while it iterates the keys and raises RuntimeError on Python 3)."""
    contigs = as_dict(parse_rows(data))
    info = 'Initial number of contigs: {}. \n'.format(len(contigs))
    if filter_length:
        short = [name for name, seq in contigs.items() if len(seq) < filter_length]
        for name in short:
            del contigs[name]
        info += 'Number of contigs discarded from further analysis (with -filter_contigs set to {0}): {1}\n'.format(
            filter_length, len(short))
    return contigs, info


def pool_of(rows):
    """-> (pool bytes, offsets, lengths) of the rows end to end"""
    offsets, lengths, at = [], [], 0
    for _name, seq in rows:
        offsets.append(at)
        lengths.append(len(seq))
        at += len(seq)
    return ''.join(seq for _name, seq in rows).encode('ascii'), offsets, lengths


def load_golden():
    with gzip.open(GOLDEN, 'rt') as fh:
        doc = json.load(fh)
    for case in doc['cases']:
        case['data'] = base64.b64decode(case['input'])
    return doc


_ALPHABET = (b'>' * 6 + b'\n' * 10 + b'\r' * 5 + b' ' * 6 + b'\t' * 4 + b'\x1c' * 3 + b'ACGTNacgtn' * 5 + b'\x0b\x0c\x1d\x1e\x1f'
             + b'RYKMx_|.1')


def random_text(seed, max_len=8192):
    """A seeded text for the differential tests: mostly what a FASTA holds, with every structural byte frequent; one in
    eight texts carries a byte outside ASCII."""
    rng = random.Random(seed)
    n = rng.choice((rng.randrange(0, 64), rng.randrange(0, 2048), rng.randrange(0, max_len + 1)))
    mode = rng.randrange(3)
    out = bytearray()
    while len(out) < n:
        if mode == 0:                                            # byte soup
            out.append(rng.choice(_ALPHABET))
        else:                                                    # lines: long runs with structure between them
            run = rng.choice((0, 1, 3, 17, 60, 61, 300, 1100 if mode == 2 else 80))
            kind = rng.randrange(8)
            if kind == 0:
                out += b'>' + bytes(rng.choice(b'abcXYZ_09') for _ in range(rng.randrange(0, 12)))
                out += rng.choice((b'', b' comment', b'\t', b' \x1c x'))
            elif kind == 1:
                out += bytes(rng.choice(b' \t\x1c\x0b') for _ in range(rng.randrange(0, run + 1)))
            else:
                out += bytes(rng.choice(b'ACGTNacgtn') for _ in range(rng.randrange(0, run + 1)))
            out += rng.choice((b'\n', b'\n', b'\n', b'\r\n', b'\r', b'', b' \n', b'\t', b' ', b'>'))
    del out[n:]
    if out and rng.randrange(8) == 0:
        out[rng.randrange(len(out))] = rng.choice((128, 200, 255))
    return bytes(out)
