"""BAM or SAM file -> resident records through the library's own readers (no pysam, no htslib).

This is the front-end the reference gets from ``pysam.Samfile(param.bamfile, 'rb')`` (runBESST:162): header
references/lengths plus, per record, exactly the attributes the hot path reads.  A BAM is inflated and decoded on the
device (or on host threads); the decoded columns are the same SoA layout the device kernels consume.

SAM text - what ``bwa mem``, ``bowtie2`` and ``minimap2`` print - is read by :class:`ResidentSam`: the header on the
host, the record lines parsed on the device (csrc/sam.hip) into the same columns, with the values the BAM of the same
records gives.  The file may be plain, BGZF or gzip; :func:`open_bam` tells the format by content, never by name.  The
record loop is exact on any record order, so an aligner's read-ordered SAM goes straight in.
"""
import os
import zlib

import numpy as np

from . import _lib
from .records import RecordBatch


def reader_threads():
    """Workers of the reader's pool: twice the CPUs the process may use (_lib.effective_cpus: affinity and cgroup quota -
    a worker blocked in a page fault leaves its share unused), at most 128."""
    return min(128, 2 * _lib.effective_cpus())


def _open(lib, path, threads):
    handle = lib.besst_bam_open(os.fsencode(path), int(threads))
    if not handle:
        raise IOError('cannot read BAM %s: %s' % (path, _lib.last_error()))
    names, lengths = _header(lib, handle)
    return handle, names, lengths


def _header(lib, handle):
    """(reference names, lengths) of an open reader; the names in one call (a C5 header has 2 M of them)."""
    n_ref = lib.besst_bam_n_references(handle)
    need = lib.besst_bam_reference_names(handle, None, 0)
    buf = np.zeros(max(int(need), 1), dtype=np.uint8)
    lib.besst_bam_reference_names(handle, _lib.ptr(buf), int(need))
    names = buf[:need].tobytes().decode().split('\0')[:n_ref] if n_ref else []
    lengths = np.zeros(max(n_ref, 1), dtype=np.int32)
    _lib.check(lib.besst_bam_reference_lengths(handle, _lib.ptr(lengths)), 'bam_reference_lengths')
    return names, lengths[:n_ref].tolist()


class ResidentBam(object):
    """A BAM file whose records went straight to HBM - besst_ctx_push_bam_device: the compressed file is uploaded and
    inflated + decoded on the GPU (any BGZF block layout); else besst_ctx_push_bam: decode on host threads, pinned
    staging, copies under the next chunk's decode; ``mode`` as in GraphContext.push_bam - the `bam_file` argument for libmetrics.get_metrics and CreateGraph.PE when nothing
    on the host needs the record columns; ``part=(r, W)``: rank r's slice of the stream (htslib's layout; with ``first_skip`` - -1: guess, >= 0: inflated bytes in front of the slice's first record - the SLICE form for any block layout, ``boundary`` = (offset used, bytes of the last record in the next slice): distributed.ingest_slice runs the check between ranks; multi-GPU ingest: ``len()`` and the
    head arrays then describe that slice only - such an object is for distributed.ingest_slice, not for
    libmetrics.get_metrics, whose < 1000-record check and read-length step are about the whole file).  It carries what the host side of those two does read: the header
    (``references``, ``lengths``), the record count (``len()``) and ``rlen`` / ``alen`` / ``qlen`` of the first 1000
    records (the read-length step, libmetrics.py:246-273); ``ctx`` is the GraphContext that holds the records and
    ``ingest`` the timings of the upload."""

    def __init__(self, path, device_index=0, threads=None, chunk_records=4 << 20, mode=None, chunk_blocks=0, part=None,
                 first_skip=None):
        from . import device
        lib = _lib.load()
        threads = threads or reader_threads()
        handle, self.references, self.lengths = _open(lib, path, threads)
        self.path = path
        self.ctx = None
        try:
            self.ctx = device.GraphContext(device_index)     # (inside the try: a context that cannot be made must not leak the reader)
            zeros = np.zeros(len(self.references), dtype=np.int32)
            self.ctx.set_contigs(scaf_id=zeros, scaf_len=zeros, ctg_pos=zeros, ctg_len=zeros, direction=zeros, cls=zeros)
            self.ingest, self.rlen, self.alen, self.qlen = self.ctx.push_bam(handle, chunk_records, mode=mode, chunk_blocks=chunk_blocks, part=part,
                                                                              first_skip=first_skip)
            self.boundary = getattr(self.ctx, 'slice_boundary', None)
            clamped = lib.besst_bam_clamped_records(handle)
        except Exception:
            if self.ctx is not None:
                self.ctx.close()
            raise
        finally:
            lib.besst_bam_close(handle)
        self._n = int(self.ingest.records)
        if clamped > 0:
            import warnings
            warnings.warn('%s: %d record(s) align more than 65535 query bases; their qlen is stored as 65535' % (path, clamped))

    def __len__(self):
        return self._n

    def layout_state(self):
        """GraphContext.layout_state(): after a device ingest the bit planes and the candidate side stream of the records are
        there already (all three watermarks at ``len()``), and the first build launches no maker."""
        return self.ctx.layout_state()

    def report(self, isize_bins=32768):
        """The BAM report of the file (GraphContext.library_report, besst_amd.report) with the header's names and lengths.
        Over a ``part`` it describes that slice."""
        rep = self.ctx.library_report(isize_bins)
        rep.references, rep.lengths = list(self.references), [int(x) for x in self.lengths]
        return rep

    def close(self):
        self.ctx.close()


class ShardedBam(object):
    """The `bam_file` argument of libmetrics.get_metrics / CreateGraph.PE under a process group (one process per GPU):
    this rank's slice of the file, inflated and decoded on its GPU (distributed.ingest_slice: any BGZF block layout, the
    ranks settle where each slice's first record begins), plus what the host side reads of the whole file - header,
    global record count, rlen / alen / qlen of the stream's first 1000 records (sharded.ShardedHead).  ``ingest``: the
    slice's timings."""

    def __init__(self, path, group=None, device_index=None, threads=None, chunk_blocks=0):
        import torch
        import torch.distributed as dist
        from . import distributed, pipeline, sharded
        self.path, self.group = path, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        dev = torch.cuda.current_device() if device_index is None else int(device_index)
        self.slice, cols = distributed.ingest_slice(path, self.rank, self.world, device_index=dev, threads=threads,
                                                    chunk_blocks=chunk_blocks, group=group)
        self.ingest = self.slice.ingest
        self.references, self.lengths = self.slice.references, self.slice.lengths
        device = torch.device('cuda', dev)
        rec = pipeline.DeviceRecords.from_columns(cols)
        self.engine = sharded.HipRankEngine(device, rec, len(self.references), keep=self.slice)
        self.head = sharded.ShardedHead(self.references, self.lengths, len(self.slice),
                                        (self.slice.rlen, self.slice.alen, self.slice.qlen), group, self.world)
        self.rlen, self.alen, self.qlen = self.head.rlen, self.head.alen, self.head.qlen

    def __len__(self):
        return len(self.head)

    def report(self, isize_bins=32768):
        """The BAM report of the WHOLE file on every rank (collective): each rank runs besst_dev_library_report over its
        slice, the words are summed over the group - the digest's xor word is gathered and xor-ed instead."""
        import torch
        import torch.distributed as dist
        from . import distributed, report, sharded
        words, err = None, None
        try:
            words = report.dev_report_tensor(self.engine.rec, len(self.references), isize_bins)
            xor_word = int(words[report.DIGEST_XOR].item())
            words[report.DIGEST_XOR] = 0
        except Exception as e:
            err = '%s: %s' % (type(e).__name__, e)
        sharded._agree(self.group, self.world, err)          # (nobody enters the all-reduce without the others)
        distributed._all_reduce(words, self.group)
        xors = [None] * self.world
        dist.all_gather_object(xors, xor_word, group=self.group)
        host = words.cpu().numpy().view(np.uint64).copy()
        for x in xors:
            host[report.DIGEST_XOR] ^= np.uint64(x & 0xffffffffffffffff)
        return report.LibraryReport(host, len(self.references), isize_bins, self.references, self.lengths)

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None


class SamError(ValueError):
    """A SAM file cannot be read.  ``offset``: the first byte of the line at fault (of the inflated text where the file is
    compressed), ``line``: its 1-based number or None, ``reason``: one of SAM_REASONS' words.  ``reason`` 'compressed
    data': the file's gzip / BGZF data is damaged; ``offset`` is then the block's or member's in the COMPRESSED file."""

    def __init__(self, message, offset, line=None, reason=None):
        ValueError.__init__(self, message)
        self.offset, self.line, self.reason = offset, line, reason


# include/besst_amd.h: BESST_SAM_*
SAM_REASONS = {1: 'fewer than eleven fields', 2: 'empty line', 3: 'header line behind a record', 4: 'FLAG is not a number in 0..65535',
               5: 'POS is not a number in 0..2^31-1', 6: 'MAPQ is not a number in 0..255', 7: 'PNEXT is not a number in 0..2^31-1',
               8: 'TLEN is not a number within int32', 9: 'RNAME is not among the references',
               10: 'RNEXT is not among the references', 11: 'CIGAR is malformed'}
GZIP_MAGIC = b'\x1f\x8b'
SAM_CHUNK_BYTES = 64 << 20               # ResidentSam streams a plain file through two pinned buffers of this size
SAM_DEFAULT_TILE = 16384                 # csrc/sam.hip: the tile of tile_bytes = 0
SAM_TEXT_PAD = 64                        # readable bytes behind a chunk's end in HBM
SAM_MAX_TEXT = (1 << 32) - 17            # one parsed chunk (besst_ctx_push_sam_text)
HEAD_RECORDS = 1000


def parse_sam_header(lines):
    """The header's lines (bytes, terminators included or not) -> (names, lengths): one reference per @SQ line in file
    order, SN: and LN: found among its tab-separated tags in any order; other lines are skipped.  SamError (offset of the
    line within the header, 1-based line): an @SQ without SN or LN, an LN that is no number in 0..2^31-1 (a BAM header may say 0, so 0 is taken), a repeated SN."""
    names, lengths, seen, at = [], [], set(), 0
    for no, raw in enumerate(lines, 1):
        line = raw.rstrip(b'\n')
        if line.endswith(b'\r'):
            line = line[:-1]
        fields = line.split(b'\t')
        if fields[0] == b'@SQ':
            sn = [f[3:] for f in fields[1:] if f.startswith(b'SN:')]
            ln = [f[3:] for f in fields[1:] if f.startswith(b'LN:')]
            if not sn or not ln or not sn[0]:
                raise SamError('@SQ line %d has no SN or no LN' % no, at, no, 'header')
            if not ln[0].isdigit() or int(ln[0]) >= (1 << 31):
                raise SamError('@SQ line %d: LN is not a length' % no, at, no, 'header')
            name = sn[0].decode('utf-8', 'surrogateescape')
            if name in seen:
                raise SamError('@SQ line %d repeats SN:%s' % (no, name), at, no, 'header')
            seen.add(name)
            names.append(name)
            lengths.append(int(ln[0]))
        at += len(raw)
    return names, lengths


def _read_plain_header(fh):
    """The leading run of '@' lines of an open binary file -> (lines, their bytes); the file stands behind them."""
    lines, size = [], 0
    while True:
        here = fh.tell()
        if fh.read(1) != b'@':
            fh.seek(here)
            return lines, size
        line = b'@' + fh.readline()
        lines.append(line)
        size += len(line)


def _sam_error(path, info, line, compressed):
    off, code = int(info[2]), int(info[3])
    reason = SAM_REASONS.get(code, 'reason %d' % code)
    where = ' of the inflated text (the file is compressed)' if compressed else ''
    return SamError('%s: %s at byte %d%s%s' % (path, reason, off, where, '' if line is None else ', line %d' % line),
                    off, line, reason)


class ResidentSam(object):
    """A SAM text file whose records went to HBM, parsed on the device (csrc/sam.hip): the interface of ResidentBam -
    ``references``, ``lengths``, ``ctx``, ``ingest``, ``rlen`` / ``alen`` / ``qlen`` of the first 1000 records, ``len()``,
    ``layout_state()``, ``report()``, ``close()`` - so that libmetrics.get_metrics and CreateGraph.PE take it unchanged.

    A plain file: the header is read on the host, the record lines stream through two pinned buffers of ``chunk_bytes``
    (a multiple of ``tile_bytes``), each chunk cut at its last line end and the tail carried to the front of the next one -
    only the columns stay resident, the file may be larger than HBM.  A file that begins with the gzip magic is brought to
    HBM whole by GenerateOutput's uploaders (BGZF inflated on the device; gzip by zlib on the host, or on the device with
    ``gzip_on_gpu``) and parsed there; its inflated text has to fit beside the columns, and below 4 GiB.

    The mate / run planes and the candidate side stream are not written while decoding: ``layout_state()`` shows the
    watermarks at 0 and the first build runs the makers, as after a host push.  SamError: a line that cannot be read (the
    smallest offset wins); the context is then gone with its records."""

    def __init__(self, path, device_index=0, chunk_bytes=None, tile_bytes=None, gzip_on_gpu=False):
        import time
        from . import device
        tile = int(tile_bytes or 0)
        if tile and (tile % 1024 or not 1024 <= tile <= 65536):
            raise ValueError('tile_bytes must be a multiple of 1024 in 1024..65536')
        chunk = int(SAM_CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        if chunk < (tile or SAM_DEFAULT_TILE) or chunk % (tile or SAM_DEFAULT_TILE) or chunk > SAM_MAX_TEXT:
            raise ValueError('chunk_bytes must be a multiple of tile_bytes, at least one tile and below 4 GiB')
        self.path, self.ctx = path, None
        self._lib = _lib.load()
        self._tile, self._saturated = tile, 0
        self.inflate, self.inflate_stats = None, None            # a compressed file: 'device', 'device_gzip' or 'host'
        self.ingest = _lib.IngestStats()
        self.ingest.on_device = 1
        self._head = (np.zeros(HEAD_RECORDS, dtype=np.int32), np.zeros(HEAD_RECORDS, dtype=np.int32),
                      np.zeros(HEAD_RECORDS, dtype=np.uint16))
        t0 = time.perf_counter()
        with open(path, 'rb') as fh:
            compressed = fh.read(2) == GZIP_MAGIC
        try:
            if compressed:
                self._read_compressed(device, int(device_index), bool(gzip_on_gpu))
            else:
                self._read_plain(device, int(device_index), chunk)
        except Exception:
            if self.ctx is not None:
                self.ctx.close()                                 # (clear_records and all: nothing half-pushed is used)
                self.ctx = None
            raise
        self.ingest.seconds = time.perf_counter() - t0
        self._n = int(self.ingest.records)
        k = min(HEAD_RECORDS, self._n)
        self.rlen, self.alen, self.qlen = (a[:k] for a in self._head)
        if self._saturated > 0:
            import warnings
            warnings.warn('%s: %d record(s) align more than 65535 query bases; their qlen is stored as 65535'
                          % (path, self._saturated))

    # ---- the header becomes the context --------------------------------------------------------------------------------
    def _open_context(self, device, device_index, header_lines):
        self.references, self.lengths = parse_sam_header(header_lines)
        self.ctx = device.GraphContext(device_index)
        zeros = np.zeros(len(self.references), dtype=np.int32)
        self.ctx.set_contigs(scaf_id=zeros, scaf_len=zeros, ctg_pos=zeros, ctg_len=zeros, direction=zeros, cls=zeros)
        blobs = [n.encode('utf-8', 'surrogateescape') for n in self.references]
        off = np.zeros(len(blobs) + 1, dtype=np.int64)
        np.cumsum(np.fromiter((len(b) for b in blobs), dtype=np.int64, count=len(blobs)), out=off[1:])
        pool = np.frombuffer(b''.join(blobs) or b'\0', dtype=np.uint8)
        _lib.check(self._lib.besst_ctx_set_sam_references(self.ctx._ctx, _lib.ptr(pool), _lib.ptr(off), len(blobs)),
                   'set_sam_references')

    def _push(self, stream, text_ptr, n_bytes, file_offset):
        """One chunk in HBM -> the context; -> info (records, saturated, error offset, reason)."""
        import ctypes as C
        info = np.zeros(4, dtype=np.int64)
        rlen, alen, qlen = self._head
        _lib.check(self._lib.besst_ctx_push_sam_text(self.ctx._ctx, C.c_void_p(stream), C.c_void_p(text_ptr), int(n_bytes),
                                                     int(file_offset), self._tile, HEAD_RECORDS, _lib.ptr(rlen), _lib.ptr(alen),
                                                     _lib.ptr(qlen), _lib.ptr(info)), 'push_sam_text')
        if info[2] < 0:
            self.ingest.records += int(info[0])
            self.ingest.chunks += 1
            self._saturated += int(info[1])
        return info

    # ---- a plain file: chunks through two pinned buffers -----------------------------------------------------------------
    def _read_plain(self, device, device_index, chunk):
        import torch
        with open(self.path, 'rb') as fh:
            header, at = _read_plain_header(fh)
            self._open_context(device, device_index, header)
            dev = torch.device('cuda', device_index)
            step = self._tile or SAM_DEFAULT_TILE
            left = os.fstat(fh.fileno()).st_size - at             # (a file smaller than a chunk needs no more than its size)
            chunk = min(chunk, max(step, -(-left // step) * step))
            _lib.check(self._lib.besst_ctx_sam_expect_text(self.ctx._ctx, int(left)), 'sam_expect_text')
            with torch.cuda.device(dev):
                h_buf = [torch.empty(chunk, dtype=torch.uint8).pin_memory() for _ in range(2)]
                # (not zeroed: the parser masks every byte behind a chunk's end, the pad only has to be readable - and a
                # fill on the current stream would have to be ordered in front of the first copies on the side stream)
                d_buf = [torch.empty(chunk + SAM_TEXT_PAD, dtype=torch.uint8, device=dev) for _ in range(2)]
                views = [memoryview(b.numpy()) for b in h_buf]
                copy = torch.cuda.Stream(dev)
                copy.wait_stream(torch.cuda.current_stream(dev))
                lines_before = len(header)
                pending = None                                   # (slot, bytes, file offset, copied event) of the chunk in flight
                carry, slot, eof = 0, 0, False

                def parse(job):
                    nonlocal lines_before
                    j_slot, j_bytes, j_off, j_done = job
                    torch.cuda.current_stream(dev).wait_event(j_done)
                    info = self._push(torch.cuda.current_stream(dev).cuda_stream, d_buf[j_slot].data_ptr(), j_bytes, j_off)
                    if info[2] >= 0:
                        rel = int(info[2]) - j_off
                        line = lines_before + 1 + int(np.count_nonzero(h_buf[j_slot].numpy()[:rel] == 10))
                        raise _sam_error(self.path, info, line, False)
                    lines_before += int(info[0])

                try:
                    while not eof:
                        view = views[slot]
                        room = chunk - carry
                        got = _read_full(fh, view[carry:chunk]) if room else 0
                        have = carry + got
                        eof = got < room
                        if have == 0:
                            break
                        cut = have if eof else _last_line_end(view, have)
                        if cut == 0:
                            if pending is not None:
                                parse(pending)                   # (an earlier line's error comes first)
                            raise SamError('%s: the line at byte %d is longer than chunk_bytes = %d; raise chunk_bytes'
                                           % (self.path, at, chunk), at, None, 'line longer than a chunk')
                        with torch.cuda.stream(copy):
                            d_buf[slot][:cut].copy_(h_buf[slot][:cut], non_blocking=True)
                            done = torch.cuda.Event()
                            done.record(copy)
                        self.ingest.bytes_h2d += cut
                        job = (slot, cut, at, done)
                        if pending is not None:
                            parse(pending)                       # chunk c - 1 is parsed while chunk c crosses
                        pending = job
                        other = views[1 - slot]                  # (its chunk was parsed just now: the buffer is free)
                        carry = have - cut
                        other[:carry] = view[cut:have]
                        at += cut
                        slot = 1 - slot
                    if pending is not None:
                        parse(pending)
                finally:
                    copy.synchronize()                           # no copy is in flight when the buffers are let go, error or not
        self.ingest.inflated_bytes = at

    # ---- a compressed file: the text is inflated into HBM whole and parsed in place ---------------------------------------
    def _read_compressed(self, device, device_index, gzip_on_gpu):
        from . import GenerateOutput as GO
        torch, dev = GO._torch_device(device_index)
        stats = dict(chunks=0, candidates=0, live=0, text_bytes=0, status=None)
        with torch.cuda.device(dev):
            try:
                text, n, self.inflate = GO._upload_gzip_file(torch, dev, self.path, None,
                                                             GO.GZIP_CHUNK_BYTES if gzip_on_gpu else None, stats)
            except GO.FastaError as exc:
                # (the uploaders word their errors for the contig file; the offset is the damaged block's or member's in
                # the COMPRESSED file - the text was never inflated that far)
                raise SamError('%s: %s (byte %d of the compressed file, not of the inflated text)'
                               % (self.path, str(exc).replace('compressed FASTA file', 'compressed SAM file'), exc.offset),
                               exc.offset, None, 'compressed data')
            except torch.cuda.OutOfMemoryError:
                raise MemoryError('%s: the inflated SAM text does not fit in HBM beside the record columns; inflate the file '
                                  'first - a plain SAM file is streamed in chunks' % self.path)
            self.inflate_stats = stats
            self.ingest.bytes_h2d = os.path.getsize(self.path)
            self.ingest.inflated_bytes = n
            # the header is fetched back from the front of the text
            header, h_bytes, window, done = [], 0, 1 << 20, False
            while not done and h_bytes < n:
                front = text[h_bytes:min(n, h_bytes + window)].cpu().numpy().tobytes()
                at_end, at = h_bytes + len(front) == n, 0
                while at < len(front):
                    if front[at:at + 1] != b'@':
                        done = True
                        break
                    nl = front.find(b'\n', at)
                    if nl < 0 and not at_end:
                        break                                    # the line goes on behind the window
                    line = front[at:] if nl < 0 else front[at:nl + 1]
                    header.append(line)
                    at += len(line)
                h_bytes += at
                if at == 0 and not done:
                    window *= 4                                  # a header line longer than the window
            self._open_context(device, device_index, header)
            body = n - h_bytes
            if body > SAM_MAX_TEXT:
                raise MemoryError('%s: %d bytes of inflated record text; a compressed SAM is parsed as one chunk of less than '
                                  '4 GiB - inflate the file first, a plain SAM file is streamed in chunks' % (self.path, body))
            if body == 0:
                return
            if h_bytes % 16:                                     # the parser wants its text 16-byte aligned: the records move
                step = 32 << 20                                  # down over the header, front to back through a bounce buffer
                tmp = torch.empty(min(step, body), dtype=torch.uint8, device=dev)
                for lo in range(0, body, step):
                    k = min(step, body - lo)
                    tmp[:k].copy_(text[h_bytes + lo:h_bytes + lo + k])
                    text[lo:lo + k].copy_(tmp[:k])
                text[body:body + min(16, h_bytes)].zero_()
                base = text.data_ptr()
            else:
                base = text.data_ptr() + h_bytes
            info = self._push(torch.cuda.current_stream(dev).cuda_stream, base, body, h_bytes)
            if info[2] >= 0:
                rel = int(info[2]) - h_bytes
                moved = h_bytes if h_bytes % 16 else 0
                lo = h_bytes - moved
                line = len(header) + 1 + int((text[lo:lo + rel] == 10).sum().item())
                raise _sam_error(self.path, info, line, True)
            del text

    def __len__(self):
        return self._n

    def layout_state(self):
        """GraphContext.layout_state(): after a SAM ingest the three watermarks stand at 0 - the planes and the candidate
        side stream are made by the first build."""
        return self.ctx.layout_state()

    def report(self, isize_bins=32768):
        """The report of the file (GraphContext.library_report, besst_amd.report) with the header's names and lengths."""
        rep = self.ctx.library_report(isize_bins)
        rep.references, rep.lengths = list(self.references), [int(x) for x in self.lengths]
        return rep

    def close(self):
        if self.ctx is not None:
            self.ctx.close()


def _read_full(fh, view):
    """readinto until the view is full or the file ends -> bytes read"""
    got = 0
    while got < len(view):
        k = fh.readinto(view[got:])
        if not k:
            break
        got += k
    return got


def _last_line_end(view, have):
    """The offset behind the last '\\n' of view[:have] (0: none), looked for from the end in windows."""
    hi = have
    while hi > 0:
        lo = max(0, hi - (1 << 16))
        at = bytes(view[lo:hi]).rfind(b'\n')
        if at >= 0:
            return lo + at + 1
        hi = lo
    return 0


def sniff_format(path):
    """'bam' or 'sam', by content: a file that begins with the gzip magic and whose first member's first bytes (zlib on
    the host, the first 64 KiB of the file) inflate to ``BAM\\1`` is a BAM - and so is one whose first member cannot be
    inflated, so that every error of the BAM reader stays what it is; gzip around any other text, and a file without the
    gzip magic, is SAM."""
    with open(path, 'rb') as fh:
        front = fh.read(65536)
    if front[:2] != GZIP_MAGIC:
        return 'sam'
    first, data = b'', front
    try:
        while len(first) < 4 and data:                           # (an empty member in front - a BGZF EOF block - is passed over)
            d = zlib.decompressobj(31)
            first += d.decompress(data, 1 << 20)                 # (as far as the 64 KiB go: damage there is the BAM reader's to name)
            if not d.eof:
                break
            data = d.unused_data
    except zlib.error:
        return 'bam'
    if len(first) < 4 and not d.eof:
        return 'bam'                                             # the member ends early: the BAM reader says so
    return 'bam' if first[:4] == b'BAM\1' else 'sam'


def reader_class(path):
    """The class open_bam uses for ``path`` outside a process group (no device is touched)."""
    return ResidentBam if sniff_format(path) == 'bam' else ResidentSam


SHARDED_SAM_MESSAGE = ('%s is SAM text: under a process group the sharded input is BAM (every rank reads its slice of the BGZF '
                       'blocks); convert the file to BAM or run on one GPU')


def open_bam(path, threads=None, **kw):
    """What a caller of the two entry points opens in place of ``pysam.Samfile(path, 'rb')`` (runBESST:162): a ResidentBam,
    a ResidentSam where the file is SAM text (plain, BGZF or gzip: sniff_format), or - under a process group for which
    sharding has been switched on (sharded.enable() / BESST_SHARDED=1: torchrun, one process per GPU) - this rank's
    ShardedBam.  A SAM file under a process group is refused on every rank alike, before any collective."""
    from . import sharded
    cls = reader_class(path)
    if sharded.active_group() is not None:
        if cls is ResidentSam:
            raise ValueError(SHARDED_SAM_MESSAGE % path)
        return ShardedBam(path, group=sharded.PROCESS_GROUP, threads=threads,
                          **{k: v for k, v in kw.items() if k in ('device_index', 'chunk_blocks')})
    if cls is ResidentSam:
        return ResidentSam(path, **{k: v for k, v in kw.items() if k in ('device_index', 'chunk_bytes', 'tile_bytes', 'gzip_on_gpu')})
    return ResidentBam(path, threads=threads, **{k: v for k, v in kw.items() if k != 'gzip_on_gpu'})


def inflate_bgzf_device(data, device_index=0, out_cap=None):
    """Test hook: the BGZF blocks of ``data`` (bytes) inflated by the GPU kernel, concatenated."""
    import ctypes as C
    lib = _lib.load()
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(out_cap if out_cap is not None else max(1, 66 * len(data)), dtype=np.uint8)
    n = C.c_size_t(0)
    _lib.check(lib.besst_bgzf_inflate_device(int(device_index), _lib.ptr(src), len(data), _lib.ptr(out), out.size, C.byref(n)),
               'bgzf_inflate_device')
    return out[:n.value].tobytes()


def write_bam(path, batch, threads=None, level=1, realistic=False):
    """Test / bench scaffolding (besst_bam_write_records): the batch as a BAM file in htslib's block layout.  realistic:
    pseudo-random bases and slowly changing qualities instead of constant bytes (the file compresses ~3 x, not ~13 x)."""
    if realistic:
        level = int(level) | 16
    import ctypes as C
    lib = _lib.load()
    names = (C.c_char_p * len(batch.references))(*[n.encode() for n in batch.references])
    lengths = np.ascontiguousarray(batch.lengths, dtype=np.int32)
    rlen = batch.rlen if batch.rlen is not None else batch.qlen
    cols = [_lib.as_col(batch.tid, np.int32), _lib.as_col(batch.mtid, np.int32), _lib.as_col(batch.pos, np.int32),
            _lib.as_col(batch.mpos, np.int32), _lib.as_col(batch.tlen, np.int32), _lib.as_col(batch.flag, np.uint16),
            _lib.as_col(batch.mapq, np.uint8), _lib.as_col(batch.qlen, np.uint16), _lib.as_col(rlen, np.int32)]
    _lib.check(lib.besst_bam_write_records(os.fsencode(path), len(batch.references), names, _lib.ptr(lengths), len(batch),
                                           *[_lib.ptr(c) for c in cols], int(threads or reader_threads()),
                                           int(level)), 'bam_write_records')


def read_bam(path, threads=None, chunk_records=8_000_000):
    lib = _lib.load()
    threads = threads or reader_threads()
    handle = lib.besst_bam_open(os.fsencode(path), int(threads))
    if not handle:
        raise IOError('cannot read BAM %s: %s' % (path, _lib.last_error()))
    try:
        names, lengths = _header(lib, handle)
        spec = (('tid', np.int32), ('mtid', np.int32), ('pos', np.int32), ('mpos', np.int32), ('tlen', np.int32),
                ('flag', np.uint16), ('mapq', np.uint8), ('qlen', np.uint16), ('rlen', np.int32), ('alen', np.int32))
        parts = {k: [] for k, _ in spec}
        while True:
            bufs = [np.empty(chunk_records, dtype=dt) for _, dt in spec]
            got = lib.besst_bam_read_records(handle, chunk_records, *[_lib.ptr(b) for b in bufs])
            if got < 0:
                raise IOError('error while reading %s: %s' % (path, _lib.last_error()))
            if got == 0:
                break
            for (k, _), b in zip(spec, bufs):
                parts[k].append(b[:got])
        cols = {k: (np.concatenate(v) if v else np.empty(0, dtype=dt)) for (k, dt), v in zip(spec, parts.values())}
        clamped = lib.besst_bam_clamped_records(handle)
        if clamped > 0:
            import warnings
            warnings.warn('%s: %d record(s) align more than 65535 query bases; their qlen (the coverage numerator of '
                          'CreateGraph.py:138-139) is stored as 65535' % (path, clamped))
    finally:
        lib.besst_bam_close(handle)
    return RecordBatch(names, lengths, **cols)
