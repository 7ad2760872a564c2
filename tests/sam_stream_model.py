"""A pure-Python model of the streamed BGZF SAM reader (bamio.ResidentSam._read_bgzf) and of its line cutter
(besst_dev_sam_lines): plain byte searches, no code shared with the package.

    cutter(text, want_header_end, count_upto) -> the four words the device leaves in ``out``
    rounds(isizes, text, chunk_bytes)         -> Plan: what every round holds, where it is cut, what it carries and pushes

The pinned rule of a round: the buffer holds the carry (the bytes behind the last cut) at offset 0; whole blocks are
appended in file order, by their ISIZE, while fewer than ``chunk_bytes`` bytes are held.  While the header lasts the cut is
the header's end (or the last line end, where the buffer is header lines throughout) and those bytes go to the host; the
first record line starts the next buffer at offset 0 (it stays where it is when the file has no header).  Behind the header
the cut is the last line end - at the end of the file, the end of the text - and the text in front of it is one push.  A
buffer of ``chunk_bytes`` or more without a line end is a line longer than a chunk.
"""


class LineTooLong(ValueError):
    def __init__(self, offset):
        ValueError.__init__(self, 'the line at byte %d is longer than a chunk' % offset)
        self.offset = offset


def cutter(text, want_header_end=False, count_upto=0):
    text = bytes(text)
    n = len(text)
    first = -1
    if want_header_end and n:
        at = 0
        while at < n:
            if text[at:at + 1] != b'@':
                first = at
                break
            nl = text.find(b'\n', at)
            if nl < 0:
                break                                            # a header line that is not whole: none
            at = nl + 1
        else:
            first = n                                            # header lines throughout, the last one whole
    return [text.rfind(b'\n') + 1, first, text.count(b'\n', 0, count_upto), 0]


class Plan(object):
    """rounds: one dict per round - first_block, n_blocks, carry_in, held, overshoot (bytes the last block goes past
    chunk_bytes), kind ('header' / 'records'), take (the cut), carry_out, text_at (text offset of the buffer's first byte),
    isizes (of its blocks); pushes: (text offset, bytes) in order; header_bytes."""

    def __init__(self):
        self.rounds, self.pushes, self.header_bytes = [], [], 0


def rounds(isizes, text, chunk_bytes):
    text = bytes(text)
    assert sum(isizes) == len(text)
    plan = Plan()
    block, inflated, carry, text_at, in_header = 0, 0, b'', 0, True
    while True:
        buf, first = carry, block
        while len(buf) < chunk_bytes and block < len(isizes):
            buf += text[inflated:inflated + isizes[block]]
            inflated += isizes[block]
            block += 1
        eof = block == len(isizes)
        held = len(buf)
        if held == 0:
            break
        r = dict(first_block=first, n_blocks=block - first, carry_in=len(carry), held=held, overshoot=max(0, held - chunk_bytes)
                 if block > first else 0, text_at=text_at, isizes=list(isizes[first:block]), last_byte=buf[-1:], first_byte=buf[:1])
        last_end, header_end = cutter(buf, in_header)[:2]
        if in_header and header_end != 0:
            r['kind'] = 'header'
            if header_end < 0:
                take = held if eof else last_end
            else:
                take, in_header = header_end, header_end == held
            if take == 0 and held >= chunk_bytes:
                raise LineTooLong(text_at)
            plan.header_bytes += take
        else:
            in_header = False
            r['kind'] = 'records'
            take = held if eof else last_end
            if take == 0 and held >= chunk_bytes:
                raise LineTooLong(text_at)
            if take:
                plan.pushes.append((text_at, take))
        r.update(take=take, carry_out=held - take, eof=eof)
        plan.rounds.append(r)
        carry, text_at = buf[take:], text_at + take
    return plan
