"""Designed compressed SAM files for the streamed reader's borders (tests/test_gpu_sam_stream.py), written with
tests/bgzf_writer.py from tests/sam_design.py's lines, and the census that proves - from the bytes and the pinned rule of a
round (tests/sam_stream_model.py) - that every case they claim is in them, at chunk_bytes = 4096 and tile 1024:

  - a carry of 0 (a round that ends on '\\n'),
  - a line held by two and by three rounds.  Under the pinned rule a buffer of chunk_bytes or more without a line end is an
    error, so a line is carried once at most - but for the line behind the round that ends the header: the records behind
    the header start the next buffer, that round takes no block when they are a chunk or more, and its last, cut line is
    carried once more,
  - '\\r' last in one round with '\\n' first in the next,
  - a round whose last block overshoots chunk_bytes,
  - an empty block first and last in a round,
  - a header across three rounds, a header that ends exactly at a round's end, a header-only file,
  - no final newline,
  - a line of exactly chunk_bytes (read), a line longer than chunk_bytes + 65536 (refused),
over block payloads of 97, 700 and 65280 bytes and a hand-cut layout of 1024-byte blocks.
"""
import numpy as np

from tests import bgzf_writer, sam_design, sam_stream_model
from tests.bgzf_util import EOF

CHUNK, TILE = 4096, 1024
PAYLOADS = (97, 700, 65280)


def record(i, total, eol='\n'):
    """a good record line of exactly ``total`` bytes, terminator included (the QNAME is as long as that takes)"""
    rest = '\t' + '\t'.join(sam_design.GOOD_LINE.split('\t')[1:]) + eol
    k = total - len(rest)
    assert k >= 1
    return (('r%d' % i).ljust(k, 'q')[:k] + rest).encode()


def comment(total):
    """a header line of exactly ``total`` bytes"""
    return b'@CO\t' + b'c' * (total - 5) + b'\n'


def _case(name, text, pieces=None, payload=None, **kw):
    """pieces: the inflated bytes of every block, in file order (b'': an empty block); else ``payload`` bytes per block"""
    if pieces is None:
        pieces = [text[at:at + payload] for at in range(0, len(text), payload)] + [b'']
    assert b''.join(pieces) == text
    data = b''.join(EOF if not piece else bgzf_writer.block(piece, level=1) for piece in pieces)
    return dict(name=name, text=text, isizes=[len(piece) for piece in pieces], data=data, **kw)


def hand_cut():
    """1024-byte blocks: a header of exactly three rounds that ends at the third one's end, a line of exactly chunk_bytes
    alone in a round, an empty block first in the next round, whose last byte is a '\\r' with its '\\n' in the next"""
    head = sam_design.header_bytes()
    pad = 64 - len(head) % 64
    head += comment(pad if pad >= 6 else pad + 64)
    assert len(head) % 64 == 0 and len(head) <= CHUNK
    head += comment(64) * ((3 * CHUNK - len(head)) // 64)
    assert len(head) == 3 * CHUNK
    body = [record(0, CHUNK)]
    body += [record(1 + i, 200) for i in range(20)] + [record(21, 97, '\r\n')]
    assert sum(len(b) for b in body[1:]) == CHUNK + 1
    body += [record(30 + i, 150 + i) for i in range(40)]
    text = head + b''.join(body)
    pieces = [text[at:at + 1024] for at in range(0, len(text), 1024)]
    pieces.insert(16, b'')                                       # in front of the fifth round's first block
    pieces.append(b'')
    return _case('hand_cut', text, pieces)


def designed_files():
    """-> the cases: dicts of name, text, isizes, data (the BGZF file) and, where the file must be refused, ``too_long``"""
    data, head = sam_design.border_file(tile=TILE, chunk=CHUNK, long_lines=False)
    cases = [_case('borders_%d' % p, data, payload=p) for p in PAYLOADS]
    cases.append(hand_cut())
    long_head = head + b''.join(comment(100 + i % 7) for i in range(90))
    cases.append(_case('long_header_700', long_head + data[len(head):], payload=700))
    cases.append(_case('no_final_newline_700', data[:-1], payload=700))
    assert data.endswith(b'\n')
    cases.append(_case('header_only_97', long_head, payload=97, header_only=True))
    cases.append(_case('header_only_no_newline_700', long_head[:-1], payload=700, header_only=True))
    lines = [record(i, 180 + i) for i in range(30)]
    too_long = head + b''.join(lines[:20]) + record(99, CHUNK + 65536 + 1) + b''.join(lines[20:])
    cases.append(_case('line_too_long_65280', too_long, payload=65280, too_long=len(head) + sum(len(b) for b in lines[:20])))
    return cases


def census(cases, chunk=CHUNK):
    """Assert every case of the module docstring from the bytes and the model's rounds -> {case name: Plan or LineTooLong}"""
    seen = dict.fromkeys(('carry_0', 'line_in_two_rounds', 'line_in_three_rounds', 'cr_lf_split', 'overshoot', 'empty_first',
                          'empty_last', 'header_three_rounds', 'header_ends_with_a_round', 'header_only', 'no_final_newline',
                          'line_of_a_chunk', 'line_too_long'), False)
    plans = {}
    for case in cases:
        text, name = case['text'], case['name']
        try:
            plan = sam_stream_model.rounds(case['isizes'], text, chunk)
        except sam_stream_model.LineTooLong as exc:
            assert exc.offset == case.get('too_long'), (name, exc.offset)
            nl = text.find(b'\n', exc.offset)
            assert nl + 1 - exc.offset > chunk + 65536
            seen['line_too_long'] = True
            plans[name] = exc
            continue
        assert 'too_long' not in case, name
        plans[name] = plan
        assert sum(n for _, n in plan.pushes) + plan.header_bytes == len(text), name
        ends = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1
        starts = np.r_[0, ends[:-1]] if len(ends) and ends[-1] == len(text) else np.r_[0, ends]
        stops = np.r_[starts[1:], len(text)]
        lo = np.array([r['text_at'] for r in plan.rounds])
        hi = np.array([r['text_at'] + r['held'] for r in plan.rounds])
        # the rounds whose buffer holds a byte of the line: first round with hi > start .. last round with lo < stop
        held_by = np.searchsorted(lo, stops, side='left') - np.searchsorted(hi, starts, side='right')
        seen['line_in_two_rounds'] |= bool((held_by == 2).any())
        seen['line_in_three_rounds'] |= bool((held_by == 3).any())
        seen['line_of_a_chunk'] |= bool(((stops - starts == chunk) & (starts >= plan.header_bytes)).any())
        header_rounds = [r for r in plan.rounds if r['kind'] == 'header']
        seen['header_three_rounds'] |= len(header_rounds) >= 3
        if header_rounds and header_rounds[-1]['carry_out'] == 0 and not header_rounds[-1]['eof']:
            seen['header_ends_with_a_round'] = True
        if case.get('header_only'):
            assert not plan.pushes and plan.header_bytes == len(text), name
            seen['header_only'] = True
        if not text.endswith(b'\n') and plan.pushes:
            seen['no_final_newline'] = True
        for r in plan.rounds:
            end = r['text_at'] + r['held']
            if r['kind'] == 'records' and r['carry_out'] == 0 and not r['eof'] and r['last_byte'] == b'\n':
                seen['carry_0'] = True
            if r['last_byte'] == b'\r' and text[end:end + 1] == b'\n' and r['carry_out'] > 0:
                seen['cr_lf_split'] = True
            if r['overshoot'] > 0 and r['n_blocks'] > 1:
                seen['overshoot'] = True
            if r['n_blocks'] > 1 and r['isizes'][0] == 0:
                seen['empty_first'] = True
            if r['n_blocks'] > 1 and r['isizes'][-1] == 0:
                seen['empty_last'] = True
    assert all(seen.values()), [k for k, v in seen.items() if not v]
    return plans


def cutter_cases():
    """The line cutter's borders -> [(name, bytes, [(n, want_header_end, count_upto)])]: newlines at byte 0, 15, 16 and
    n - 1, no newline, '@' at every position of a 16-byte slice behind a '\\n' that is the slice before's last byte, n that
    is no multiple of 16 (the bytes behind n are there and must be masked), count_upto at 0, inside a slice and at n."""
    def queries(n):
        return [(n, want, upto) for want in (0, 1) for upto in sorted({0, n // 3, n // 2 + 1 if n else 0, n})]
    cases = []
    t = b'\n' + b'x' * 14 + b'\n\n' + b'y' * 20 + b'\n'
    assert [i for i in range(len(t)) if t[i] == 10] == [0, 15, 16, len(t) - 1] and len(t) % 16
    cases.append(('newlines_0_15_16_last', t, queries(len(t)) + queries(16) + queries(17)))
    cases.append(('no_newline', b'x' * 100, queries(100) + queries(96)))
    cases.append(('no_newline_header', b'@' * 100, queries(100)))
    cases.append(('empty', b'\n', queries(0)))
    for k in range(16):
        s = bytearray(b'A' * 16)
        s[k] = 64
        t = b'@HD' + b'h' * 12 + b'\n' + bytes(s) + b'\n@tail'
        assert t[15] == 10
        cases.append(('at_%d' % k, t, queries(len(t)) + queries(32)))
    t = b'@abc\n@def\nXYZ\n@x\n'
    cases.append(('every_n', t, [(n, 1, n // 2) for n in range(len(t) + 1)]))
    cases.append(('header_whole', b'@a\n@b\n' * 9, queries(54) + queries(53)))
    return cases
