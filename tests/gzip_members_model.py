"""A model of the parallel inflate of a gzip file of SEVERAL members, restated in plain Python on
top of the one-member model (tests/gzip_stream_model.py) - not from the kernels: the member candidates, the header parse,
the chain with its passages from member to member, the segments, and the distance rule that is relative to the member.
The GPU path (csrc/gzip_stream.hip, besst_dev_gzip_members_*) is held to it: the same text and exactly the same numbers
of chunks, candidates, live segments, members and member candidates.

The one-member model reads "raw" DEFLATE data and counts bits from its first byte.  Here ``raw`` is the FILE from member
0's first data byte to the eight bytes in front of its end - headers, trailers and all -, so that the chunks are the
device's; a position in the file is ``8 * data_off`` more."""
import struct
import zlib

from tests import gzip_stream_model as M

HEADER_FIELD_LIMIT = 65536               # bytes of an FNAME or FCOMMENT, its zero included
STATUS_OF = {'stored block': 'stored_length', 'block type 3': 'block_type'}


def member_candidates(data):
    """every offset behind the first whose four bytes read 1f 8b 08 and a FLG without reserved bits"""
    out, at = [], data.find(b'\x1f\x8b\x08', 1)
    while at >= 0:
        if at + 4 <= len(data) and not data[at + 3] & 0xe0:
            out.append(at)
        at = data.find(b'\x1f\x8b\x08', at + 1)
    return out


def member_data_offset(data, at):
    """the header at ``at`` -> where its DEFLATE data begins; None: not a header, a field that does not end inside the file
    or the limit, or no room for a block and a trailer (RFC 1952; the twin of GenerateOutput.gzip_header_bytes)"""
    n = len(data)
    if n - at < 18 or data[at:at + 3] != b'\x1f\x8b\x08' or data[at + 3] & 0xe0:
        return None
    flg, p = data[at + 3], at + 10
    if flg & 4:
        if n - p < 2:
            return None
        p += 2 + struct.unpack_from('<H', data, p)[0]
    for bit in (8, 16):
        if flg & bit:
            end = data.find(b'\0', p, p + HEADER_FIELD_LIMIT) if p < n else -1
            if end < 0:
                return None
            p = end + 1
    if flg & 2:
        p += 2
    return p if p <= n and n - p >= 8 else None


class FileModel(object):
    def __init__(self, data):
        self.data = bytes(data)
        self.data_off = member_data_offset(self.data, 0)
        assert self.data_off is not None
        self.s = M.Stream(self.data[self.data_off:len(self.data) - 8])
        self.bit0 = 8 * self.data_off
        self.marks = member_candidates(self.data)
        self.starts = {at: member_data_offset(self.data, at) for at in self.marks}

    def walk(self, start, cands, chunk):
        """M.walk from a bit of the stream -> (landing, bytes, BFINAL, block starts), or the status of a walk that fails"""
        try:
            return M.walk(self.s, start, cands, chunk)
        except M.ModelError as exc:
            return STATUS_OF.get(str(exc), 'bad_data')
        except IndexError:
            return 'input_overrun'

    def chain(self, chunk):
        """-> (status, segments, members, index of the member the status is about): a segment is dict(kind 'chunk' or 'member', start, land, bytes, off, member_off,
        starts), positions in bits of the stream; a member dict(at, data, trailer, off, bytes) in bytes of the file"""
        cands = M.candidates(self.s, chunk)
        segs, members = [], []
        kind, start, off, mem_off, mem_at, mem_data = 'chunk', 0, 0, 0, 0, self.data_off
        while True:
            got = self.walk(start, cands, chunk)
            if isinstance(got, str):
                segs.append(dict(kind=kind, start=start, land=None, bytes=0, off=off, member_off=mem_off, starts=[]))
                return got, segs, members, len(members)
            land, n, final, starts = got
            segs.append(dict(kind=kind, start=start, land=land, bytes=n, off=off, member_off=mem_off, starts=starts))
            off += n
            if not final:
                kind, start = 'chunk', land
                j = land // (8 * chunk)
                assert cands[j] is not None and 8 * chunk * j + cands[j] == land
                continue
            trailer = self.data_off + (land + 7) // 8
            members.append(dict(at=mem_at, data=mem_data, trailer=trailer, off=mem_off, bytes=off - mem_off))
            if struct.unpack_from('<I', self.data, trailer + 4)[0] != (off - mem_off) & 0xffffffff:
                return 'isize', segs, members, len(members) - 1
            if trailer + 8 == len(self.data):
                return 'ok', segs, members, None
            mem_at, mem_off = trailer + 8, off
            mem_data = self.starts.get(mem_at)
            if mem_data is None:
                return 'trailing_bytes', segs, members, len(members)
            kind, start = 'member', 8 * (mem_data - self.data_off)

    def decode(self, seg, whole_text_rule=False):
        """a segment's blocks -> one symbol per byte (M.decode_markers), with the distance rule: a match reaches its member's
        first byte and no further (``whole_text_rule``: the text's first byte - what a one-member decoder checks)"""
        reach0 = seg['off'] - (0 if whole_text_rule else seg['member_off'])
        sym = []
        for pos in seg['starts']:
            for t in self.s.block(pos)[3]:
                if isinstance(t, int):
                    sym.append(t)
                    continue
                length, dist = t
                if dist > reach0 + len(sym):
                    raise M.ModelError('distance')
                for _ in range(length):
                    at = len(sym) - dist
                    sym.append(sym[at] if at >= 0 else M.MARKER | (M.WINDOW + at))
        return sym

    def inflate(self, chunk, whole_text_rule=False, member_cap=None):
        """The whole procedure -> dict(status, text, chunks, candidates, live, members, member_candidates, bad_member,
        bad_member_offset, segments, member_table, cands)"""
        cands = M.candidates(self.s, chunk)
        out = dict(chunks=len(cands), candidates=sum(c is not None for c in cands[1:]), member_candidates=len(self.marks),
                   cands=cands, text=None, bad_member=None, bad_member_offset=None, live=0, members=0, segments=[],
                   member_table=[])
        if member_cap is not None and len(self.marks) > member_cap:
            out['status'] = 'too_many_members'
            return out
        status, segs, members, bad = self.chain(chunk)
        out.update(status=status, live=len(segs), members=len(members), segments=segs, member_table=members)
        if status == 'ok':
            try:
                text = M.resolve([(g['off'], self.decode(g, whole_text_rule)) for g in segs])
            except M.ModelError:
                out['status'] = 'bad_distance'
                return out
            out['text'] = text
            for k, m in enumerate(members):
                if struct.unpack_from('<I', self.data, m['trailer'])[0] != zlib.crc32(text[m['off']:m['off'] + m['bytes']]):
                    out['status'], bad = 'crc', k
                    break
        if bad is not None:
            at = members[bad]['at'] if bad < len(members) else members[-1]['trailer'] + 8
            out.update(bad_member=bad, bad_member_offset=at)
        return out

    def census(self, chunk):
        """what the file holds at this chunk size: member starts per chunk, the kinds of the member candidates the chain
        dropped ('header', 'stored', 'codes'), where the live members begin relative to the chunk borders"""
        res = self.inflate(chunk)
        live_at = {m['at'] for m in res['member_table']}
        per_chunk = {}
        for m in res['member_table'][1:]:
            j = (m['at'] - self.data_off) // chunk
            per_chunk[j] = per_chunk.get(j, 0) + 1
        headers = [(m['at'], m['data']) for m in res['member_table']]
        payloads = []
        for g in res['segments']:
            for pos in g['starts']:
                end, _final, btype, _tokens = self.s.block(pos)
                if btype == 0:
                    payloads.append((self.data_off + ((pos + 3 + 7) // 8) + 4, self.data_off + end // 8))
        dropped = {}
        for at in self.marks:
            if at in live_at:
                continue
            kind = 'codes'
            if any(lo < at < hi for lo, hi in headers):
                kind = 'header'
            elif any(lo <= at < hi for lo, hi in payloads):
                kind = 'stored'
            dropped.setdefault(kind, []).append(at)
        borders = {(m['at'] - self.data_off) % chunk for m in res['member_table'][1:]}
        straddled = [m for m in res['member_table'][1:] if (m['at'] - self.data_off) // chunk != (m['data'] - 1 - self.data_off) // chunk]
        return dict(result=res, starts_per_chunk=per_chunk, dropped=dropped, border_offsets=borders, straddled=straddled)
